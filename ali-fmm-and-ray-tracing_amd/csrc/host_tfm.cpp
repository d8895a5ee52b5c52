// host_tfm.cpp — the TFM family over resident fields: alifmm_tfm / _f64 / _coh (delay and sum),
// alifmm_tfm_model (its transpose) and alifmm_tfm_lsq (the least-squares solve on both).  One front
// half: the checks (tfm_check), the parameter blocks (tfm_params, tfm_model_params) and the
// modelling kernel's launch plan (tfm_model_plan).  alifmm_tfm_lsq_pulse is the same solve with the
// trace FIR (host_fir.cpp, trace_fir.hip) around the two products, and alifmm_tfm_sparse the
// ℓ1-regularised solve (FISTA, tfm_sparse.hip) on the same two products (TfmOperator).
#include <chrono>

#include "host_internal.h"

// the sizes and the window every member of the family takes; fx: the fields' row pitch (tfm_check)
struct TfmCall {
  int ntx, nrx, nt, ncomp;
  double t0, fs;
  int iz0, ix0, niz, nix, step;
  int fx;
  size_t npair() const { return (size_t)ntx * nrx; }
  size_t ndata() const { return npair() * (size_t)nt * ncomp; }
  size_t nwin() const { return (size_t)niz * nix; }  // pixels of the window
};

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The argument checks of the family (`what` names the caller in messages; in: the data or the map,
// out: the image or the modelled data); on success tab = the transmitters' fields, then the
// receivers', C.fx = their row pitch
static int tfm_check(alifmm_ctx* ctx, const char* what, int subgrid, const int32_t* tx_slot, const int32_t* rx_slot,
                     const void* in, const void* out, TfmCall& C, std::vector<const double*>& tab) {
  const int ntx = C.ntx, nrx = C.nrx, iz0 = C.iz0, ix0 = C.ix0, niz = C.niz, nix = C.nix, step = C.step;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "%s: no model", what);
  if (!tx_slot || !rx_slot || !in || !out) return fail(ctx, ALIFMM_E_ARG, "%s: null pointer", what);
  if (ntx < 1 || nrx < 1 || C.nt < 2) return fail(ctx, ALIFMM_E_ARG, "%s: ntx %d, nrx %d, nt %d", what, ntx, nrx, C.nt);
  if (C.ncomp != 1 && C.ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "%s: ncomp %d is not 1 or 2", what, C.ncomp);
  if (!(std::isfinite(C.fs) && C.fs > 0) || !std::isfinite(C.t0))
    return fail(ctx, ALIFMM_E_ARG, "%s: fs %g, t0 %g", what, C.fs, C.t0);
  if (step < 1 || niz < 1 || nix < 1) return fail(ctx, ALIFMM_E_ARG, "%s: step %d, window %d x %d", what, step, niz, nix);
  // the slots: resident fields of `subgrid`, one shape
  int fz = 0, fx = 0;
  tab.assign((size_t)ntx + nrx, nullptr);
  for (int k = 0; k < ntx + nrx; k++) {
    const int s = k < ntx ? tx_slot[k] : rx_slot[k - ntx];
    if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
      return fail(ctx, ALIFMM_E_ARG, "%s: no field in slot %d", what, s);
    const Field& f = ctx->fields[s];
    if (f.sg != subgrid) return fail(ctx, ALIFMM_E_ARG, "%s: slot %d holds a subgrid-%d field, not %d", what, s, f.sg, subgrid);
    if (k == 0) fz = f.nz, fx = f.nx;
    if (f.nz != fz || f.nx != fx)
      return fail(ctx, ALIFMM_E_ARG, "%s: slot %d is %d x %d, slot %d is %d x %d", what, s, f.nz, f.nx, tx_slot[0], fz, fx);
    tab[k] = f.d;
  }
  if (iz0 < 0 || ix0 < 0 || (int64_t)iz0 + (int64_t)step * (niz - 1) > fz - 1 ||
      (int64_t)ix0 + (int64_t)step * (nix - 1) > fx - 1)
    return fail(ctx, ALIFMM_E_ARG, "%s: window (%d, %d) + %d x (%d, %d) outside the %d x %d field", what, iz0, ix0, step,
                niz, nix, fz, fx);
  C.fx = fx;
  return ALIFMM_OK;
}

// The TFM kernel's block from the call and the device pointers: the slot table (transmitters, then
// receivers), the data as float32 or float64 (the other null), the weights (or null), the image
static af::TfmParams tfm_params(const TfmCall& C, const double* const* tab, const float* fmc, const double* fmc64,
                                const float* w, double* image) {
  af::TfmParams P;
  P.tx = tab;
  P.rx = tab + C.ntx;
  P.fmc = fmc;
  P.fmc64 = fmc64;
  P.pair_w = w;
  P.image = image;
  P.t0 = C.t0;
  P.fs = C.fs;
  P.ntx = C.ntx;
  P.nrx = C.nrx;
  P.nt = C.nt;
  P.ncomp = C.ncomp;
  P.fnx = C.fx;
  P.iz0 = C.iz0;
  P.ix0 = C.ix0;
  P.niz = C.niz;
  P.nix = C.nix;
  P.step = C.step;
  return P;
}

// The modelling kernel's launch plan: receivers per workgroup, samples per pass, pixel slabs
struct TfmModelPlan {
  int rg, tile, slabs;
};
// ... for a call that models npix pixels, from the options in force (ALIFMM_E_ARG: more trace groups
// than one launch takes); what it chose is what "tfm_model_tile_used" / "_slabs_used" report
static int tfm_model_plan(alifmm_ctx* ctx, const char* what, const TfmCall& C, size_t npix, TfmModelPlan* plan) {
  const int rg = ctx->tfm_model_rx;
  const int64_t ngroups = (int64_t)C.ntx * ((C.nrx + rg - 1) / rg);
  if (ngroups > 0x7fffffffLL)
    return fail(ctx, ALIFMM_E_ARG, "%s: %d x %d pairs are more than one launch takes", what, C.ntx, C.nrx);
  const int tile = af::tfm_model_tile(ctx->tfm_model_tile, C.nt, C.ncomp, rg);
  int64_t slabs = ctx->tfm_model_slabs;
  if (slabs == 0) {  // two workgroups per CU where the pairs alone do not give them, a slab no shorter than a workgroup
    slabs = (2 * (int64_t)std::max(ctx->n_cu, 1) + ngroups - 1) / ngroups;
    slabs = std::min<int64_t>(slabs, ((int64_t)npix + 1023) / 1024);
  }
  slabs = std::max<int64_t>(1, std::min<int64_t>({slabs, 64, (int64_t)npix}));
  ctx->tfm_model_tile_used = tile;
  ctx->tfm_model_slabs_used = (int)slabs;
  *plan = {rg, tile, (int)slabs};
  return ALIFMM_OK;
}

// The modelling kernel's block: the slot table, the npix pixels' field offsets and reflectivities,
// the weights (or null), the modelled data
static af::TfmModelParams tfm_model_params(const alifmm_ctx* ctx, const TfmCall& C, const TfmModelPlan& plan,
                                           const double* const* tab, const int64_t* pix, size_t npix, const double* refl,
                                           const float* w, double* out) {
  af::TfmModelParams P;
  P.tx = tab;
  P.rx = tab + C.ntx;
  P.pix = pix;
  P.refl = refl;
  P.pair_w = w;
  P.out = out;
  P.t0 = C.t0;
  P.fs = C.fs;
  P.npix = (int64_t)npix;
  P.ntx = C.ntx;
  P.nrx = C.nrx;
  P.nt = C.nt;
  P.ncomp = C.ncomp;
  P.rg = plan.rg;
  P.tile = plan.tile;
  P.slabs = plan.slabs;
  P.combine = ctx->tfm_model_combine;
  return P;
}

// What alifmm_tfm, alifmm_tfm_f64 and alifmm_tfm_coh share after the checks: the data, the weights
// and the slot table `tab` go into the context's grow-only buffers (their copies' host time into
// *t_upload), the image's buffer holds the window, and P is filled in full
static int tfm_stage(alifmm_ctx* ctx, bool f64, const std::vector<const double*>& tab, const TfmCall& C, const void* fmc,
                     const float* pair_w, af::TfmParams* P, double* t_upload) {
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::TfmBufs& B = ctx->tfm;
  HIPCHK(f64 ? B.fmc64.grow(C.ndata()) : B.fmc.grow(C.ndata()));
  if (pair_w) HIPCHK(B.w.grow(C.npair()));
  HIPCHK(B.tab.grow(tab.size()));
  HIPCHK(B.img.grow(C.nwin() * C.ncomp));
  const auto c0 = std::chrono::steady_clock::now();
  if (f64) HIPCHK(hipMemcpy(B.fmc64, fmc, C.ndata() * sizeof(double), hipMemcpyHostToDevice));
  else HIPCHK(hipMemcpy(B.fmc, fmc, C.ndata() * sizeof(float), hipMemcpyHostToDevice));
  if (pair_w) HIPCHK(hipMemcpy(B.w, pair_w, C.npair() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.tab, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
  *t_upload = ms_since(c0);
  *P = tfm_params(C, B.tab, f64 ? nullptr : B.fmc.p, f64 ? B.fmc64.p : nullptr, pair_w ? B.w.p : nullptr, B.img);
  return ALIFMM_OK;
}

// alifmm_tfm (fmc float32) and alifmm_tfm_f64 (f64: fmc float64): the same call but for the data's type
static int tfm_impl(alifmm_ctx* ctx, const char* what, bool f64, int subgrid, const int32_t* tx_slot,
                    const int32_t* rx_slot, const void* fmc, const float* pair_w, TfmCall C, double* image) {
  if (!ctx) return ALIFMM_E_ARG;
  std::vector<const double*> tab;
  if (int rc = tfm_check(ctx, what, subgrid, tx_slot, rx_slot, fmc, image, C, tab)) return rc;
  af::TfmParams P;
  if (int rc = tfm_stage(ctx, f64, tab, C, fmc, pair_w, &P, &ctx->t_tfm_upload)) return rc;
  const int chunk = ctx->tfm_chunk;
  const auto launch = [&](hipStream_t st) { return f64 ? af_launch_tfm_f64(&P, chunk, st) : af_launch_tfm(&P, chunk, st); };
  HIPCHK(timed_section(ctx, launch, &ctx->t_tfm_kernel));
  HIPCHK(hipMemcpy(image, P.image, C.nwin() * C.ncomp * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

extern "C" int alifmm_tfm(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                          const float* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                          int niz, int nix, int step, double* image) {
  return tfm_impl(ctx, "tfm", false, subgrid, tx_slot, rx_slot, fmc, pair_w,
                  {ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0}, image);
}

extern "C" int alifmm_tfm_f64(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                              const int32_t* rx_slot, const double* fmc, int nt, int ncomp, double t0, double fs,
                              const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double* image) {
  return tfm_impl(ctx, "tfm_f64", true, subgrid, tx_slot, rx_slot, fmc, pair_w,
                  {ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0}, image);
}

extern "C" int alifmm_tfm_coh(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                              const int32_t* rx_slot, const float* fmc, int nt, int ncomp, double t0, double fs,
                              const float* pair_w, int iz0, int ix0, int niz, int nix, int step, int kind, double* image,
                              double* factor, double* sums) {
  if (!ctx) return ALIFMM_E_ARG;
  TfmCall C{ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0};
  std::vector<const double*> tab;
  if (int rc = tfm_check(ctx, "tfm_coh", subgrid, tx_slot, rx_slot, fmc, image, C, tab)) return rc;
  if (!factor) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: null pointer");
  if (kind < 1 || kind > 3) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: kind %d is not 1 (CF), 2 (SCF) or 3 (PCF)", kind);
  if (kind == 3 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "tfm_coh: kind 3 (PCF) needs ncomp 2, not %d", ncomp);
  af::TfmCohParams Q;
  if (int rc = tfm_stage(ctx, false, tab, C, fmc, pair_w, &Q.T, &ctx->t_tfm_coh_upload)) return rc;
  const size_t npix = C.nwin();
  alifmm_ctx::TfmBufs& B = ctx->tfm;
  HIPCHK(B.coh_f.grow(npix));
  if (sums) HIPCHK(B.coh_s.grow(3 * npix));
  Q.factor = B.coh_f;
  Q.sums = sums ? B.coh_s.p : nullptr;
  const int chunk = ctx->tfm_chunk;
  const auto launch = [&](hipStream_t st) { return af_launch_tfm_coh(&Q, kind, chunk, st); };
  HIPCHK(timed_section(ctx, launch, &ctx->t_tfm_coh_kernel));
  HIPCHK(hipMemcpy(image, Q.T.image, npix * ncomp * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(factor, Q.factor, npix * sizeof(double), hipMemcpyDeviceToHost));
  if (sums) HIPCHK(hipMemcpy(sums, Q.sums, 3 * npix * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

// alifmm_tfm_model's map: every value finite; the pixels that are not all zero, in raster order, as
// field offsets and values (a zero pixel never reaches the device).  The component count is a
// template argument: the loop over 4096² pixels is a third slower with a count read at run time.
template <int NC>
static int tfm_model_compact(alifmm_ctx* ctx, const TfmCall& C, const double* refl, std::vector<int64_t>& pix,
                             std::vector<double>& val) {
  const int niz = C.niz, nix = C.nix;
  for (int i = 0; i < niz; i++)
    for (int j = 0; j < nix; j++) {
      const double* x = refl + ((int64_t)i * nix + j) * NC;
      bool any = false;
      for (int c = 0; c < NC; c++) {
        if (!std::isfinite(x[c])) return fail(ctx, ALIFMM_E_ARG, "tfm_model: refl[%d][%d][%d] is %g", i, j, c, x[c]);
        any |= x[c] != 0.0;
      }
      if (!any) continue;
      pix.push_back(af::tfm_model_pixel_offset(C.iz0, C.ix0, C.step, C.fx, i, j));
      for (int c = 0; c < NC; c++) val.push_back(x[c]);
    }
  return ALIFMM_OK;
}

extern "C" int alifmm_tfm_model(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                                const int32_t* rx_slot, const double* refl, int ncomp, int nt, double t0, double fs,
                                const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double* fmc_out) {
  if (!ctx) return ALIFMM_E_ARG;
  TfmCall C{ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0};
  std::vector<const double*> tab;
  if (int rc = tfm_check(ctx, "tfm_model", subgrid, tx_slot, rx_slot, refl, fmc_out, C, tab)) return rc;
  const auto c0 = std::chrono::steady_clock::now();
  std::vector<int64_t> pix;
  std::vector<double> val;
  if (int rc = ncomp == 2 ? tfm_model_compact<2>(ctx, C, refl, pix, val) : tfm_model_compact<1>(ctx, C, refl, pix, val))
    return rc;
  const size_t npix = pix.size(), nout = C.ndata();
  TfmModelPlan plan;
  if (int rc = tfm_model_plan(ctx, "tfm_model", C, npix, &plan)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::TfmModelBufs& B = ctx->tfm_model;
  HIPCHK(B.pix.grow(npix));
  HIPCHK(B.refl.grow(val.size()));
  if (pair_w) HIPCHK(B.w.grow(C.npair()));
  HIPCHK(B.tab.grow(tab.size()));
  HIPCHK(B.out.grow(nout));
  if (npix) {
    HIPCHK(hipMemcpy(B.pix, pix.data(), npix * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(B.refl, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (pair_w) HIPCHK(hipMemcpy(B.w, pair_w, C.npair() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.tab, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
  ctx->t_tfm_model_upload = ms_since(c0);
  const af::TfmModelParams P = tfm_model_params(ctx, C, plan, B.tab, B.pix, npix, B.refl, pair_w ? B.w.p : nullptr, B.out);
  const auto launch = [&](hipStream_t st) {
    // one slab stores every sample of its traces; several add into zeros; no pixel: all zeros
    hipError_t e = (plan.slabs > 1 || npix == 0) ? hipMemsetAsync(B.out, 0, nout * sizeof(double), st) : hipSuccess;
    if (e == hipSuccess && npix) e = af_launch_tfm_model(&P, st);
    return e;
  };
  HIPCHK(timed_section(ctx, launch, &ctx->t_tfm_model_kernel));
  HIPCHK(hipMemcpy(fmc_out, B.out, nout * sizeof(double), hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

// What the solves over B = P A share on the device (F null: no pulse, B = A): the small buffers of
// a call and their upload, and the two products.  With a pulse a data-sized vector `mid` lies
// between the FIR and A (A writes it and P reads it, Pᵀ writes it and Aᵀ reads it).
struct TfmOperator {
  alifmm_ctx* ctx;
  const TfmCall& C;
  const TfmModelPlan& plan;
  const FirTaps* F;
  const double* const* tab = nullptr;
  int64_t* pix = nullptr;
  const float* w = nullptr;
  double* mid = nullptr;

  // the pixel list, the weights, the slot table and the taps into B's buffers (the copies before
  // the caller's own time stamp ends)
  hipError_t stage(alifmm_ctx::TfmLsqBufs& B, const std::vector<const double*>& t, const float* pair_w) {
    hipError_t e = B.pix.grow(C.nwin());
    if (e == hipSuccess && pair_w) e = B.w.grow(C.npair());
    if (e == hipSuccess) e = B.tab.grow(t.size());
    if (e == hipSuccess && F) e = ctx->fir.taps.grow((size_t)F->ntap * F->tap_comp);
    if (e == hipSuccess && F)
      e = hipMemcpy(ctx->fir.taps, F->taps, (size_t)F->ntap * F->tap_comp * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && pair_w) e = hipMemcpy(B.w, pair_w, C.npair() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(B.tab, t.data(), t.size() * sizeof(double*), hipMemcpyHostToDevice);
    tab = B.tab;
    pix = B.pix;
    w = pair_w ? B.w.p : nullptr;
    return e;
  }
  hipError_t pixels() const {
    return af_launch_tfm_lsq_pix(C.iz0, C.ix0, C.step, C.fx, C.niz, C.nix, pix, ctx->stream);
  }
  // out = P in (transpose 0) or Pᵀ in (1) over the ntx nrx traces
  hipError_t fir(const double* in, double* out, int transpose) const {
    const af::TraceFirParams Q{in, out, ctx->fir.taps, (int64_t)C.npair(), C.nt, F->ntap, F->origin, transpose};
    return af_launch_trace_fir(&Q, C.ncomp, F->tap_comp, ctx->stream);
  }
  // out = B refl
  hipError_t forward(const double* refl, double* out) const {
    double* const aq = F ? mid : out;  // what A writes
    const af::TfmModelParams M = tfm_model_params(ctx, C, plan, tab, pix, C.nwin(), refl, w, aq);
    // several slabs add into what A writes with atomics: zeroed every time
    hipError_t e = plan.slabs > 1 ? hipMemsetAsync(aq, 0, C.ndata() * sizeof(double), ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = af_launch_tfm_model(&M, ctx->stream);
    if (e == hipSuccess && F) e = fir(aq, out, 0);
    return e;
  }
  // t = Bᵀ r
  hipError_t adjoint(const double* r, double* t) const {
    hipError_t e = F ? fir(r, mid, 1) : hipSuccess;
    const af::TfmParams T = tfm_params(C, tab, nullptr, F ? mid : r, w, t);
    return e == hipSuccess ? af_launch_tfm_f64(&T, ctx->tfm_chunk, ctx->stream) : e;
  }
};

// The device half of alifmm_tfm_lsq (F null) and of alifmm_tfm_lsq_pulse (F: the pulse), after the
// checks: hipSuccess or the first error (the caller frees the call's buffers on one).  With a pulse
// the operator is P A: a third data-sized vector w lies between the FIR and the two products
// (A writes it, Aᵀ reads it), q = P w and w = Pᵀ r.
static hipError_t tfm_lsq_run(alifmm_ctx* ctx, const std::vector<const double*>& tab, const TfmCall& C,
                              const TfmModelPlan& plan, const FirTaps* F, const double* fmc, const float* pair_w,
                              double damp, double smooth, int max_iter, double tol, double* image, double* resid,
                              CglsResult* R) {
#define LSQ(call)                    \
  do {                               \
    hipError_t e_ = (call);          \
    if (e_ != hipSuccess) return e_; \
  } while (0)
  const size_t npix = C.nwin(), nd = C.ndata(), ni = npix * C.ncomp;
  LSQ(hipSetDevice(ctx->device));
  alifmm_ctx::TfmLsqBufs& B = ctx->tfm_lsq;
  LSQ(B.data.grow((F ? 3 : 2) * nd));
  LSQ(B.img.grow(4 * ni));
  LSQ(B.small.grow((size_t)af::kSolveMaxParts + af::kSolScalars));
  af::SolveVecs V;
  V.x = B.img;
  V.p = B.img + ni;
  V.s = B.img + 2 * ni;
  V.t = B.img + 3 * ni;
  V.xs = nullptr;
  V.r = B.data;
  V.q = B.data + nd;
  V.parts = B.small;
  V.scal = B.small + af::kSolveMaxParts;
  V.damp2 = damp * damp;
  V.smooth2 = smooth * smooth;
  TfmOperator Op{ctx, C, plan, F};
  Op.mid = F ? B.data + 2 * nd : nullptr;
  const auto c0 = std::chrono::steady_clock::now();
  LSQ(hipMemcpy(V.r, fmc, nd * sizeof(double), hipMemcpyHostToDevice));
  LSQ(Op.stage(B, tab, pair_w));
  ctx->t_tfm_lsq_upload = ms_since(c0);
  af::TfmLsqDims G;
  G.niz = C.niz;
  G.nix = C.nix;
  G.nc = C.ncomp;
  G.nimg = (int64_t)ni;
  G.ndata = (int64_t)nd;
  hipStream_t st = ctx->stream;
  const auto form_t = [&] { return Op.adjoint(V.r, V.t); };  // t = Aᵀ r, with a pulse Aᵀ Pᵀ r
  LSQ(hipEventRecord(ctx->ev[0], st));
  LSQ(Op.pixels());
  LSQ(cgls_run(
      V, ni, nd, st, ctx->ev[0], ctx->ev[1], max_iter, tol, form_t,
      [&] { return af_launch_tfm_lsq_grad(&G, &V, 1, st); },  // x = 0: s = Aᵀ d, p = s, gamma_0 = |s|²
      [&] {
        hipError_t e = Op.forward(V.p, V.q);  // q = A p, with a pulse P A p
        if (e == hipSuccess) e = af_launch_tfm_lsq_step(&G, &V, st);
        if (e == hipSuccess) e = form_t();
        if (e == hipSuccess) e = af_launch_tfm_lsq_grad(&G, &V, 0, st);
        return e;
      },
      R, &ctx->t_tfm_lsq_kernel));
  ctx->tfm_lsq_iters = R->iters;
  LSQ(hipMemcpy(image, V.x, ni * sizeof(double), hipMemcpyDeviceToHost));
  if (resid) LSQ(hipMemcpy(resid, V.r, nd * sizeof(double), hipMemcpyDeviceToHost));
  return hipSuccess;
#undef LSQ
}

// alifmm_tfm_lsq (F null) and alifmm_tfm_lsq_pulse: the checks, the plan, the solve
static int tfm_lsq_impl(alifmm_ctx* ctx, const char* what, int subgrid, const int32_t* tx_slot, const int32_t* rx_slot,
                        const double* fmc, const float* pair_w, TfmCall C, const FirTaps* F, double damp, double smooth,
                        int max_iter, double tol, double* image, double* resid, double* info8) {
  if (!ctx) return ALIFMM_E_ARG;
  std::vector<const double*> tab;
  if (int rc = tfm_check(ctx, what, subgrid, tx_slot, rx_slot, fmc, image, C, tab)) return rc;
  if (!info8) return fail(ctx, ALIFMM_E_ARG, "%s: info8 is NULL", what);
  if (int rc = cgls_check(ctx, what, damp, smooth, max_iter, tol)) return rc;
  if (F)
    if (int rc = fir_check_taps(ctx, what, C.ncomp, *F)) return rc;
  const size_t nd = C.ndata();
  for (size_t k = 0; k < nd; k++)
    if (!std::isfinite(fmc[k])) return fail(ctx, ALIFMM_E_ARG, "%s: fmc[%zu] is not finite", what, k);
  // the modelling kernel's plan (alifmm_tfm_model), every pixel of the window counting
  TfmModelPlan plan;
  if (int rc = tfm_model_plan(ctx, what, C, C.nwin(), &plan)) return rc;
  CglsResult R;
  const hipError_t e = tfm_lsq_run(ctx, tab, C, plan, F, fmc, pair_w, damp, smooth, max_iter, tol, image, resid, &R);
  if (e != hipSuccess) {  // (out of memory, for one): the call's buffers go
    (void)hipStreamSynchronize(ctx->stream);
    ctx->tfm_lsq = {};
    return fail(ctx, ALIFMM_E_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  R.pack(info8, 0.0);
  return ALIFMM_OK;
}

extern "C" int alifmm_tfm_lsq(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                              const int32_t* rx_slot, const double* fmc, int nt, int ncomp, double t0, double fs,
                              const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double damp,
                              double smooth, int max_iter, double tol, double* image, double* resid, double* info8) {
  return tfm_lsq_impl(ctx, "tfm_lsq", subgrid, tx_slot, rx_slot, fmc, pair_w,
                      {ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0}, nullptr, damp, smooth, max_iter, tol,
                      image, resid, info8);
}

extern "C" int alifmm_tfm_lsq_pulse(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                                    const int32_t* rx_slot, const double* fmc, int nt, int ncomp, double t0, double fs,
                                    const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double damp,
                                    double smooth, int max_iter, double tol, int ntap, int tap_comp, const double* taps,
                                    int origin, double* image, double* resid, double* info8) {
  const FirTaps F{ntap, tap_comp, taps, origin};
  return tfm_lsq_impl(ctx, "tfm_lsq_pulse", subgrid, tx_slot, rx_slot, fmc, pair_w,
                      {ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0}, &F, damp, smooth, max_iter, tol, image,
                      resid, info8);
}

// ---- alifmm_tfm_sparse ----

// what a sparse solve reports beside the image (info12)
struct SparseResult {
  int iters = 0, reason = 1, backtracks = 0, restarts = 0;
  double g0 = 0, gk = 0, rhs = 0, res = 0, lam_max = 0, lam = 0, L = 0, nnz = 0;
  void pack(double* info12) const {
    const double info[12] = {(double)iters, g0, gk, rhs, res, (double)reason, lam_max, lam, L, (double)backtracks,
                             (double)restarts, nnz};
    std::copy(info, info + 12, info12);
  }
};

// The device half of alifmm_tfm_sparse after the checks (F null: no pulse): FISTA with backtracking
// and gradient restart, the iteration of include/alifmm.h line for line.  hipSuccess or the first
// error (the caller frees the call's buffers on one).  x and x⁺, B x and B x⁺ swap by pointer when a
// trial is accepted; B y is never formed.
static hipError_t tfm_sparse_run(alifmm_ctx* ctx, const std::vector<const double*>& tab, const TfmCall& C,
                                 const TfmModelPlan& plan, const FirTaps* F, const double* fmc, const float* pair_w,
                                 double damp, double smooth, int max_iter, double tol, double lam, double lipschitz,
                                 int power_iters, int restart, double* image, double* resid, SparseResult* R) {
#define SP(call)                     \
  do {                               \
    hipError_t e_ = (call);          \
    if (e_ != hipSuccess) return e_; \
  } while (0)
  const size_t npix = C.nwin(), nd = C.ndata(), ni = npix * C.ncomp;
  SP(hipSetDevice(ctx->device));
  alifmm_ctx::TfmLsqBufs& B = ctx->tfm_sparse;
  SP(B.data.grow((F ? 5 : 4) * nd));
  SP(B.img.grow(5 * ni));
  SP(B.small.grow((size_t)af::kSpPartArrays * af::kSolveMaxParts + af::kSpScalars + af::kSolScalars));
  af::SparseVecs V;
  V.x = B.img;
  V.y = B.img + ni;  // (y follows x: both zeroed at once)
  V.xn = B.img + 2 * ni;
  V.g = B.img + 3 * ni;
  V.t = B.img + 4 * ni;
  V.d = B.data;
  V.bx = B.data + nd;
  V.bxn = B.data + 2 * nd;
  V.r = B.data + 3 * nd;
  V.parts = B.small;
  V.scal = B.small + (size_t)af::kSpPartArrays * af::kSolveMaxParts;
  V.damp2 = damp * damp;
  V.smooth2 = smooth * smooth;
  af::SolveVecs N = {};  // what af_launch_solve_norm takes: the partials and a scalar block of its own
  N.parts = V.parts;
  N.scal = V.scal + af::kSpScalars;
  TfmOperator Op{ctx, C, plan, F};
  Op.mid = F ? B.data + 4 * nd : nullptr;
  const auto c0 = std::chrono::steady_clock::now();
  SP(hipMemcpy(V.d, fmc, nd * sizeof(double), hipMemcpyHostToDevice));
  SP(Op.stage(B, tab, pair_w));
  ctx->t_tfm_sparse_upload = ms_since(c0);
  af::TfmLsqDims G;
  G.niz = C.niz;
  G.nix = C.nix;
  G.nc = C.ncomp;
  G.nimg = (int64_t)ni;
  G.ndata = (int64_t)nd;
  hipStream_t st = ctx->stream;
  // n scalars of the device's from `which` on (at most 32 bytes, one copy) after the work queued so far
  const auto scalars = [&](int which, int n, double* v) {
    hipError_t e = hipMemcpyAsync(v, V.scal + which, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  };
  SP(hipEventRecord(ctx->ev[0], st));
  SP(Op.pixels());
  SP(hipMemsetAsync(V.x, 0, 2 * ni * sizeof(double), st));  // x = y = 0
  SP(hipMemsetAsync(V.bx, 0, nd * sizeof(double), st));     // B x = 0
  SP(hipMemsetAsync(V.scal, 0, (af::kSpScalars + af::kSolScalars) * sizeof(double), st));
  SP(af_launch_solve_norm(V.d, (long)nd, &N, st));  // |d|²
  SP(Op.adjoint(V.d, V.t));                         // t = Bᵀ d
  SP(af_launch_tfm_sparse_start(&G, &V, N.scal + af::kSolNorm, st));
  double s4[4];
  SP(scalars(af::kSpG0, 3, s4));  // |g0|², lam_max, |d|²
  R->g0 = sqrt(s4[0]);
  R->lam_max = s4[1];
  R->rhs = sqrt(s4[2]);
  R->lam = lam < 0 ? -lam * R->lam_max : lam;
  double L = lipschitz;
  bool go = R->g0 != 0.0;
  if (go && !(lipschitz > 0)) {  // the power estimate: v = g0 / |g0|; w = Bᵀ B v + R(v), est = |w|, v = w / |w|
    for (int k = 0; k < power_iters; k++) {
      SP(af_launch_tfm_sparse_power_scale(&G, &V, st));
      SP(Op.forward(V.xn, V.bxn));
      SP(Op.adjoint(V.bxn, V.t));
      SP(af_launch_tfm_sparse_power(&G, &V, st));
    }
    SP(scalars(af::kSpEst, 1, &L));
    go = std::isfinite(L) && L > 0;
  }
  ctx->tfm_sparse_l0 = go ? L : 0.0;
  R->reason = go ? 1 : 2;
  double theta = 1.0;
  int doublings = 0;
  for (int k = 1; go && k <= max_iter; k++) {
    // (g and fy belong to y: the start left them for y = 0, the end of an iteration for the next)
    for (;;) {
      const double step = 1.0 / L, tau = R->lam * step;
      SP(af_launch_tfm_sparse_prox(&G, &V, step, tau, st));
      SP(Op.forward(V.xn, V.bxn));
      SP(af_launch_tfm_sparse_trial(&G, &V, L, st));
      SP(scalars(af::kSpOut, 4, s4));  // the one read of a trial: f⁺, Q + slack, |x⁺ - y|², the restart dot
      if (s4[0] <= s4[1]) break;
      if (++doublings > af::kSpMaxDoublings) {
        go = false;
        break;
      }
      L = 2 * L;
      R->backtracks++;
    }
    if (!go) {
      R->reason = 2;
      break;
    }
    R->gk = L * sqrt(s4[2]);
    R->iters = k;
    std::swap(V.x, V.xn);  // x⁺ is the iterate, the old iterate the next trial's room
    std::swap(V.bx, V.bxn);
    if (restart && s4[3] > 0) theta = 1.0, R->restarts++;
    const double theta1 = (1.0 + sqrt(1.0 + 4.0 * theta * theta)) / 2.0, beta = (theta - 1.0) / theta1;
    theta = theta1;
    if (R->gk <= tol * R->g0) {
      R->reason = 0;
      break;
    }
    if (k == max_iter) break;  // (the momentum step of a last iteration would serve nothing)
    // (after the swap x is x⁺ and xn the iterate before it)
    af::SparseVecs W = V;
    W.xn = V.x, W.x = V.xn, W.bxn = V.bx, W.bx = V.bxn;
    SP(af_launch_tfm_sparse_momentum(&G, &W, beta, st));
    SP(Op.adjoint(V.r, V.t));
    SP(af_launch_tfm_sparse_grad(&G, &V, st));
  }
  R->L = L;
  SP(af_launch_tfm_sparse_final(&G, &V, st));  // r = d - B x of the returned x, computed, and its non-zero pixels
  SP(scalars(af::kSpRes, 2, s4));
  R->res = sqrt(s4[0]);
  R->nnz = s4[1];
  SP(hipEventRecord(ctx->ev[1], st));
  SP(hipStreamSynchronize(st));
  float t = 0;
  SP(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
  ctx->t_tfm_sparse_kernel = t;
  ctx->tfm_sparse_iters = R->iters;
  ctx->tfm_sparse_backtracks = R->backtracks;
  SP(hipMemcpy(image, V.x, ni * sizeof(double), hipMemcpyDeviceToHost));
  if (resid) SP(hipMemcpy(resid, V.r, nd * sizeof(double), hipMemcpyDeviceToHost));
  return hipSuccess;
#undef SP
}

extern "C" int alifmm_tfm_sparse(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                                 const int32_t* rx_slot, const double* fmc, int nt, int ncomp, double t0, double fs,
                                 const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double damp,
                                 double smooth, int max_iter, double tol, int ntap, int tap_comp, const double* taps,
                                 int origin, double lam, double lipschitz, int power_iters, int restart, double* image,
                                 double* resid, double* info12) {
  if (!ctx) return ALIFMM_E_ARG;
  const char* what = "tfm_sparse";
  TfmCall C{ntx, nrx, nt, ncomp, t0, fs, iz0, ix0, niz, nix, step, 0};
  std::vector<const double*> tab;
  if (int rc = tfm_check(ctx, what, subgrid, tx_slot, rx_slot, fmc, image, C, tab)) return rc;
  if (!info12) return fail(ctx, ALIFMM_E_ARG, "%s: info12 is NULL", what);
  if (int rc = cgls_check(ctx, what, damp, smooth, max_iter, tol)) return rc;
  const bool pulse = ntap != 0 || taps != nullptr;  // ntap 0 and taps NULL: no pulse
  const FirTaps F{ntap, tap_comp, taps, origin};
  if (pulse)
    if (int rc = fir_check_taps(ctx, what, C.ncomp, F)) return rc;
  if (!std::isfinite(lam)) return fail(ctx, ALIFMM_E_ARG, "%s: lam %g", what, lam);
  if (!(lipschitz >= 0) || !std::isfinite(lipschitz)) return fail(ctx, ALIFMM_E_ARG, "%s: lipschitz %g", what, lipschitz);
  if (!(lipschitz > 0) && power_iters < 1)
    return fail(ctx, ALIFMM_E_ARG, "%s: power_iters %d without a lipschitz constant", what, power_iters);
  if (restart != 0 && restart != 1) return fail(ctx, ALIFMM_E_ARG, "%s: restart %d is not 0 or 1", what, restart);
  const size_t nd = C.ndata();
  for (size_t k = 0; k < nd; k++)
    if (!std::isfinite(fmc[k])) return fail(ctx, ALIFMM_E_ARG, "%s: fmc[%zu] is not finite", what, k);
  TfmModelPlan plan;
  if (int rc = tfm_model_plan(ctx, what, C, C.nwin(), &plan)) return rc;
  SparseResult R;
  const hipError_t e = tfm_sparse_run(ctx, tab, C, plan, pulse ? &F : nullptr, fmc, pair_w, damp, smooth, max_iter, tol,
                                      lam, lipschitz, power_iters, restart, image, resid, &R);
  if (e != hipSuccess) {  // (out of memory, for one): the call's buffers go
    (void)hipStreamSynchronize(ctx->stream);
    ctx->tfm_sparse = {};
    return fail(ctx, ALIFMM_E_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  R.pack(info12);
  return ALIFMM_OK;
}
