// host_ops.cpp — the module-level operators on the device: time_between_points, the local
// operators of a batch of patches (local_ops), the band kernel's fouds18 fallback (fouds18_band) and
// the correctly rounded trigonometric functions themselves (cr_math).
#include <cstring>
#include <limits>

#include "host_internal.h"

extern "C" int alifmm_time_between_points(alifmm_ctx* ctx, int n, const double* x1, const double* x2, const double* y1,
                               const double* y2, int subgrid, double* out) {
  if (!ctx || !ctx->have_model || n < 0 || subgrid < 1) return fail(ctx, ALIFMM_E_ARG, "time_between_points: bad args");
  if (n == 0) return ALIFMM_OK;
  HIPCHK(hipSetDevice(ctx->device));
  double* d = nullptr;
  HIPCHK(dalloc(&d, (size_t)5 * n));
  hipError_t e = hipSuccess;
  const double* src[4] = {x1, x2, y1, y2};
  for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpy(d + (size_t)k * n, src[k], 8 * (size_t)n, hipMemcpyHostToDevice);
  af::DevModel M = dev_model(ctx);
  if (e == hipSuccess) e = af_launch_tbp(&M, n, d, d + n, d + 2 * n, d + 3 * n, ctx->dnx, subgrid, d + 4 * n, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + 4 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(d);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "time_between_points: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

extern "C" int alifmm_cr_math(alifmm_ctx* ctx, int fn, int lds_tables, int64_t n, const double* x, double* out,
                              double* out2) {
  if (!ctx) return ALIFMM_E_ARG;
  if (fn < 0 || fn > 4) return fail(ctx, ALIFMM_E_ARG, "cr_math: fn %d (0 atan, 1 sin, 2 cos, 3 tan, 4 sincos)", fn);
  if (lds_tables != 0 && lds_tables != 1) return fail(ctx, ALIFMM_E_ARG, "cr_math: lds_tables %d (0 or 1)", lds_tables);
  if (n < 0) return fail(ctx, ALIFMM_E_ARG, "cr_math: n %lld", (long long)n);
  if (n == 0) return ALIFMM_OK;
  if (!x || !out || (fn == 4 && !out2)) return fail(ctx, ALIFMM_E_ARG, "cr_math: null %s", !x ? "x" : !out ? "out" : "out2");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t m = (size_t)n, nout = fn == 4 ? 2 : 1;
  double* d = nullptr;  // [x | out | out2]
  HIPCHK(dalloc(&d, (1 + nout) * m));
  hipError_t e = hipMemcpy(d, x, 8 * m, hipMemcpyHostToDevice);
  double* d2 = fn == 4 ? d + 2 * m : nullptr;
  if (e == hipSuccess)
    e = lds_tables ? af_launch_cr_eval_lds(fn, n, d, d + m, d2, ctx->stream) : af_launch_cr_eval(fn, n, d, d + m, d2, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + m, 8 * m, hipMemcpyDeviceToHost);
  if (e == hipSuccess && fn == 4) e = hipMemcpy(out2, d2, 8 * m, hipMemcpyDeviceToHost);
  dfree(d);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "cr_math: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

// The test entries (ops 3..6) read each patch as the field kernels read their grids, so their
// arguments are checked as no module-level call needs: the cell inside the patch, update()'s and
// fouds18_A()'s column bound inside it (rows past it read -1 / 0), and a finite ttn at every valid
// node (NaN is the HBM grids' code for a far node: a NaN there would turn the node invalid).
static int test_form_args(alifmm_ctx* ctx, const char* who, int n, int pz, int px, const double* ttn,
                          const int32_t* nsts, const int32_t* iz, const int32_t* ix, const int32_t* nnx_arg) {
  const size_t pn = (size_t)pz * px;
  for (int k = 0; k < n; k++) {
    if (iz[k] < 0 || iz[k] >= pz || ix[k] < 0 || ix[k] >= px || nnx_arg[k] > px)
      return fail(ctx, ALIFMM_E_ARG, "%s: case %d: cell (%d, %d) or nnx %d outside the %d x %d patch", who, k, iz[k],
                  ix[k], nnx_arg[k], pz, px);
    for (size_t i = k * pn; i < (k + 1) * pn; i++)
      if (nsts[i] >= 0 && !std::isfinite(ttn[i]))
        return fail(ctx, ALIFMM_E_ARG, "%s: case %d: ttn is not finite at a valid node (%d, %d)", who, k,
                    (int)((i - k * pn) / px), (int)((i - k * pn) % px));
  }
  return ALIFMM_OK;
}

extern "C" int alifmm_local_ops(alifmm_ctx* ctx, int op, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                                const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz, const int32_t* nnz_arg,
                                const int32_t* nnx_arg, const double* cell_veln, const int64_t* cell_velpn, const double* cell_vm,
                                const int64_t* cell_stif, const double* tab, int ncol, double* out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (op != 0 && op != 1 && (op < 3 || op > 5))
    return fail(ctx, ALIFMM_E_ARG, "local_ops: op %d (0, 1; test entries 3, 4, 5)", op);
  if (n < 0 || pz < 1 || px < 1 || ncol < 1) return fail(ctx, ALIFMM_E_ARG, "local_ops: bad args");
  if (n == 0) return ALIFMM_OK;
  const size_t pn = (size_t)pz * px;
  std::vector<double> coded;  // ops 3, 4: the patches as the HBM grids hold them
  if (op >= 3) {
    if (int rc = test_form_args(ctx, "local_ops", n, pz, px, ttn, nsts, iz, ix, nnx_arg)) return rc;
    if (op != 5) {
      coded.resize(pn * n);
      for (size_t i = 0; i < coded.size(); i++) coded[i] = nsts[i] >= 0 ? ttn[i] : std::numeric_limits<double>::quiet_NaN();
      ttn = coded.data();
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int> vp(n);
  for (int k = 0; k < n; k++) vp[k] = (int)cell_velpn[k];
  std::vector<double> st;
  if (cell_stif) {
    st.resize((size_t)5 * n);
    for (size_t k = 0; k < st.size(); k++) st[k] = (double)cell_stif[k];
  }
  // one device block: [ttn | cveln | cvm | dnx | dnz | tab | stif | out] doubles, [nsts | iz | ix | nnz | nnx | velpn] ints
  size_t nd = pn * n + 4 * (size_t)n + 361 * (size_t)ncol + st.size() + n;
  size_t ni = pn * n + 5 * (size_t)n;
  double* dd = nullptr;
  int* di = nullptr;
  HIPCHK(dalloc(&dd, nd));
  if (hipMalloc((void**)&di, ni * 4) != hipSuccess) {
    dfree(dd);
    return fail(ctx, ALIFMM_E_HIP, "local_ops: out of memory");
  }
  double* p = dd;
  af::LocalOpsParams P;
  memset(&P, 0, sizeof P);
  P.op = op;
  P.n = n;
  P.pz = pz;
  P.px = px;
  hipError_t e = hipSuccess;
  auto putd = [&](const double* h, size_t cnt) {
    double* q = p;
    if (e == hipSuccess && cnt) e = hipMemcpy(q, h, cnt * 8, hipMemcpyHostToDevice);
    p += cnt;
    return (const double*)q;
  };
  P.ttn = putd(ttn, pn * n);
  P.cveln = putd(cell_veln, n);
  P.cvm = putd(cell_vm, n);
  P.dnx = putd(dnx, n);
  P.dnz = putd(dnz ? dnz : dnx, n);
  P.tab = putd(tab, 361 * (size_t)ncol);
  P.cstif = cell_stif ? putd(st.data(), st.size()) : nullptr;
  P.out = p;
  int* q = di;
  auto puti = [&](const int32_t* h, size_t cnt) {
    int* r = q;
    if (e == hipSuccess && cnt) e = hipMemcpy(r, h, cnt * 4, hipMemcpyHostToDevice);
    q += cnt;
    return (const int*)r;
  };
  P.nsts = puti(nsts, pn * n);
  P.iz = puti(iz, n);
  P.ix = puti(ix, n);
  P.nnz_arg = puti(nnz_arg, n);
  P.nnx_arg = puti(nnx_arg, n);
  P.cvelpn = puti(vp.data(), n);
  P.ncol = ncol;
  if (e == hipSuccess) e = af_launch_local_ops(&P, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, P.out, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(dd);
  dfree(di);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "local_ops: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

// op 2: one lane per case (alifmm_fouds18_band); op 6: four lanes per case (alifmm_fouds18_band_lanes)
static int fouds18_band_op(alifmm_ctx* ctx, int op, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                           const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                           const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz, const int32_t* mx,
                           int quant, double* out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model || n < 0 || pz < 1 || px < 1 || (quant != 0 && quant != 1))
    return fail(ctx, ALIFMM_E_ARG, "fouds18_band: bad args or no model");
  if (!ctx->dm.mid || !ctx->dm.mslo)
    return fail(ctx, ALIFMM_E_ARG, "fouds18_band: the model has no per-material table (too many materials)");
  for (int k = 0; k < n; k++)
    if (mz[k] < 0 || mz[k] >= ctx->nz0 || mx[k] < 0 || mx[k] >= ctx->nx0)
      return fail(ctx, ALIFMM_E_ARG, "fouds18_band: model cell %d (%d, %d) outside the grid", k, mz[k], mx[k]);
  if (n == 0) return ALIFMM_OK;
  if (op == 6)
    if (int rc = test_form_args(ctx, "fouds18_band", n, pz, px, ttn, nsts, iz, ix, nnx_arg)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t pn = (size_t)pz * px;
  // [ttn | dnx | dnz | out] doubles, [nsts | iz | ix | nnz | nnx | mz | mx] ints
  double* dd = nullptr;
  int* di = nullptr;
  HIPCHK(dalloc(&dd, pn * n + 3 * (size_t)n));
  if (hipMalloc((void**)&di, (pn * n + 6 * (size_t)n) * 4) != hipSuccess) {
    dfree(dd);
    return fail(ctx, ALIFMM_E_HIP, "fouds18_band: out of memory");
  }
  af::LocalOpsParams P;
  memset(&P, 0, sizeof P);
  P.op = op;
  P.n = n;
  P.pz = pz;
  P.px = px;
  P.RM = dev_model(ctx);
  P.quant = quant;
  hipError_t e = hipSuccess;
  double* p = dd;
  auto putd = [&](const double* h, size_t cnt) {
    double* q = p;
    if (e == hipSuccess && cnt) e = hipMemcpy(q, h, cnt * 8, hipMemcpyHostToDevice);
    p += cnt;
    return (const double*)q;
  };
  int* q = di;
  auto puti = [&](const int32_t* h, size_t cnt) {
    int* r = q;
    if (e == hipSuccess && cnt) e = hipMemcpy(r, h, cnt * 4, hipMemcpyHostToDevice);
    q += cnt;
    return (const int*)r;
  };
  P.ttn = putd(ttn, pn * n);
  P.dnx = putd(dnx, n);
  P.dnz = putd(dnz ? dnz : dnx, n);
  P.out = p;
  P.nsts = puti(nsts, pn * n);
  P.iz = puti(iz, n);
  P.ix = puti(ix, n);
  P.nnz_arg = puti(nnz_arg, n);
  P.nnx_arg = puti(nnx_arg, n);
  P.mz = puti(mz, n);
  P.mx = puti(mx, n);
  if (e == hipSuccess) e = af_launch_local_ops(&P, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, P.out, 8 * (size_t)n, hipMemcpyDeviceToHost);
  dfree(dd);
  dfree(di);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "fouds18_band: %s", hipGetErrorString(e));
  return ALIFMM_OK;
}

extern "C" int alifmm_fouds18_band(alifmm_ctx* ctx, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                        const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                        const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz, const int32_t* mx, int quant,
                        double* out) {
  return fouds18_band_op(ctx, 2, n, pz, px, ttn, nsts, iz, ix, dnx, dnz, nnz_arg, nnx_arg, mz, mx, quant, out);
}

extern "C" int alifmm_fouds18_band_lanes(alifmm_ctx* ctx, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                                         const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                                         const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz,
                                         const int32_t* mx, int quant, double* out) {
  return fouds18_band_op(ctx, 6, n, pz, px, ttn, nsts, iz, ix, dnx, dnz, nnz_arg, nnx_arg, mz, mx, quant, out);
}
