// host_travel.cpp — travel-time fields: the per-chunk work arena and the source-init hand-overs,
// the band launch of one chunk of sources (travel_chunk), alifmm_travel / _into / _seeded.
// Sources are processed in launches of at most `batch` (and at most half the CUs: >= 2 band
// workgroups per source), all workgroups of a launch co-resident.
#include <cstring>
#include <unordered_map>

#include "host_internal.h"

// scells: cells of the row-major status S (fmm_exact_kernel's region and the mode-1 hand-over:
// subgrid > 1 only; 0 at subgrid 1, where the band kernel keeps its status in the bricked Sb)
static int ensure_arena(alifmm_ctx* ctx, int nsrc, long cells, long scells, long capL, long capC, long capS, int K,
                        long capR, long ecells, long tbc, long sbc) {
  Arena& a = ctx->arena;
  if (a.nsrc >= nsrc && a.cells >= cells && a.scells >= scells && a.capL >= capL && a.capC >= capC &&
      a.capS >= capS && a.K >= K && a.capR >= capR && a.ecells >= ecells && a.tbc >= tbc && a.sbc >= sbc)
    return ALIFMM_OK;
  // the source-init hand-overs, their signatures and jobs are no part of what a launch's geometry
  // sizes: they stay as they are (ensure_handover sizes them, for source-init launches only), so
  // that a launch of another size, member count or capacity — a seeded call's between two travel
  // calls — leaves what init_reuse vouches for and what alifmm_init_profile reads
  DevBuf<af::HandoverOut> keep_ho = std::move(a.ho);
  DevBuf<af::InitSig> keep_sig = std::move(a.sig);
  DevBuf<af::InitJob> keep_jobs = std::move(a.jobs);
  a = {};
  a.ho = std::move(keep_ho);
  a.sig = std::move(keep_sig);
  a.jobs = std::move(keep_jobs);
  a.nsrc = nsrc;
  a.cells = cells;
  a.scells = scells;
  a.capL = capL;
  a.capC = capC;
  a.capS = capS;
  a.K = K;
  a.capR = capR;
  a.ecells = ecells;
  a.tbc = tbc;
  a.sbc = sbc;
  HIPCHK(a.Tb.grow((size_t)nsrc * tbc));
  HIPCHK(a.Sb.grow((size_t)nsrc * sbc));
  if (scells > 0) HIPCHK(a.S.grow((size_t)nsrc * scells));
  HIPCHK(a.lists.grow((size_t)nsrc * (4 * capL + 6 * capC)));
  HIPCHK(a.dlists.grow((size_t)nsrc * (capL + 2 * capC)));
  if (K > 1) {
    HIPCHK(a.rimc.grow((size_t)nsrc * K * 2 * capR));
    HIPCHK(a.rimt.grow((size_t)nsrc * K * 2 * capR));
  }
  HIPCHK(a.kx.grow(nsrc));
  if (capS > 0) {
    HIPCHK(a.Ts.grow((size_t)nsrc * 2 * capS));
    HIPCHK(a.Ss.grow((size_t)nsrc * 2 * capS));
  }
  HIPCHK(a.srcs.grow(nsrc));
  HIPCHK(a.dscx.grow(nsrc));
  HIPCHK(a.dscz.grow(nsrc));
  return ALIFMM_OK;
}

// hand-over slots, signatures and jobs for a source-init launch of n sources (travel_chunk's own
// launch: subgrid 1, no hand-over made elsewhere); grown only, and only here
static int ensure_handover(alifmm_ctx* ctx, int n) {
  Arena& a = ctx->arena;
  if (a.jobs.n >= (size_t)n) return ALIFMM_OK;  // (jobs: the last to grow)
  if (ctx->ho_last == a.ho) {  // init profile of a chunk whose hand-overs go away
    ctx->ho_last = nullptr;
    ctx->n_ho_last = 0;
  }
  a.ho.release();
  a.sig.release();
  a.jobs.release();
  HIPCHK(a.ho.grow(n));
  HIPCHK(a.sig.grow(n));
  HIPCHK(hipMemsetAsync(a.sig, 0, sizeof(af::InitSig) * n, ctx->stream));  // no slot valid
  HIPCHK(a.jobs.grow(n));
  return ALIFMM_OK;
}

extern "C" int af_ensure_field(alifmm_ctx* ctx, int slot, int sg, int fz, int fx, long extra_cells) {
  if ((int)ctx->fields.size() <= slot) ctx->fields.resize(slot + 1);
  Field& f = ctx->fields[slot];
  const size_t bytes = (size_t)fz * fx * sizeof(double), need = bytes + (size_t)extra_cells * sizeof(double);
  HIPCHK(f.d.grow(need / sizeof(double)));
  f.bytes = bytes;
  f.sg = sg;
  f.nz = fz;
  f.nx = fx;
  return ALIFMM_OK;
}

// members per source of the band kernel: the largest K <= kMaxK whose grid (nsrc padded to 8, times
// K workgroups, one per CU) is co-resident, with >= 2 stripes per member
// (option "members" forces a value, still capped by residency and by the stripe count: a member
// without a stripe would only take its 1 / K share of the work lists, travel_chunk capL / K, from
// the members that own cells)
static int choose_members(const alifmm_ctx* ctx, int n, int fx) {
  const int by_cu = std::max(1, ctx->n_cu / (8 * ((n + 7) / 8)));
  if (ctx->members > 0) {
    int K = std::max(1, std::min(ctx->members, by_cu));
    // the stripe width follows K (travel_chunk) unless "stripe_log" fixes it: lower K until it fits
    for (;;) {
      const int wlog = ctx->stripe_log ? ctx->stripe_log : (K >= 16 ? 4 : K >= 8 ? 5 : 6);
      const long nstr = ((long)fx + (1L << wlog) - 1) >> wlog;
      if (K <= nstr) return K;
      K = (int)nstr;
    }
  }
  // >= 2 stripes per member at the stripe width the member count selects
  auto stripes = [&](int k) { return (long)(fx + (1 << (k >= 8 ? 4 : 6)) - 1) >> (k >= 8 ? 4 : 6); };
  int K = std::min(af::kMaxK, by_cu);
  while (K > 1 && 2L * K > stripes(K)) K--;
  return K;
}

// subgrid-1 source init (fmm_init_kernel) of n sources into ho (jobs: device scratch of n InitJobs)
// sig: the slots' signatures; reused / reused_stride: where the kernel reports each skipped walk
static int launch_source_init(alifmm_ctx* ctx, int n, const double* scx, const double* scz, af::InitJob* djobs,
                              af::HandoverOut* ho, af::InitSig* sig, int* reused, int reused_stride) {
  std::vector<af::InitJob> jobs(n);
  for (int i = 0; i < n; i++) {
    jobs[i].isx = (long)std::nearbyint((scx[i] - ctx->gox) / ctx->dnx);
    jobs[i].isz = (long)std::nearbyint((scz[i] - ctx->goz) / ctx->dnz);
    jobs[i].dnx = ctx->dnx;
    jobs[i].dnz = ctx->dnz;
    jobs[i].exact_r = ctx->exact_r;
    jobs[i].tab_epoch = ctx->tab_epoch;
    jobs[i].tstop = ctx->exact_r * ctx->dnx / ctx->vmax;
    if (jobs[i].isx < 0 || jobs[i].isx >= ctx->nx0 || jobs[i].isz < 0 || jobs[i].isz >= ctx->nz0)
      return fail(ctx, ALIFMM_E_ARG, "source %d (%g, %g) outside the grid", i, scx[i], scz[i]);
  }
  af::DevModel M = dev_model(ctx);
  HIPCHK(hipMemcpyAsync(djobs, jobs.data(), sizeof(af::InitJob) * n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(af_launch_init(&M, djobs, n, ho, sig, ctx->init_reuse, reused, reused_stride, ctx->stream));
  return ALIFMM_OK;
}

// travel_chunk: a plain band launch whose members were not all resident (another process held CUs);
// alifmm_travel re-runs the chunk once with a cooperative launch
static const int kRetryCoop = -100;

// one chunk of sources; returns ALIFMM_E_CAPACITY when a work list overflowed
static int travel_chunk(alifmm_ctx* ctx, int sg, int n, const double* scx, const double* scz, int first_slot, int fz,
                        int fx, float* ms_init, float* ms_band, const af::HandoverOut* pre_ho = nullptr,
                        StreamOut* so = nullptr, int* init_reused = nullptr) {
  const long cells = (long)fz * fx;
  long capL = std::min(cells, std::max(65536L, cells / 8) * ctx->cap_scale);
  long capC = capL;
  long capS = 0;
  if (sg > 1) {
    long s1 = 9L * 2 * (2L * sg + (sg - 1) / 2) + 1;             // stage-1 grid side (x9)
    long s2 = 3L * 2 * (2L * sg + (sg - 1) / 2 + 3L * sg) + 1;  // stage-2 grid side (x3)
    capS = std::max(s1 * s1, s2 * s2);
    capL = std::max(capL, std::min(capS, 262144L));
    capC = capL;
  }
  // band kernel: members per source and the stripe geometry (KGeom)
  const int K = choose_members(ctx, n, fx);
  // stripe width: 16 columns at 16 members, 32 at 8, 64 below (C4 sweeps, profiles/r6z*)
  const int wlog = ctx->stripe_log ? ctx->stripe_log : (K >= 16 ? 4 : K >= 8 ? 5 : 6), W = 1 << wlog;
  const long nstripes = (fx + W - 1) / W;
  const long capR = K > 1 ? 2L * fz * ((nstripes + K - 1) / K) + 64 : 0;
  const long ecells = K > 1 ? nstripes * 4L * fz : 0;  // per edge buffer (4 columns per stripe)
  // the band kernel's working field (af_band_tb_cells: its layout) and its edge buffers
  const long tb_cells = af_band_tb_cells(fz, fx), tbc = tb_cells + 2 * ecells, sbc = af_band_sb_cells(fz, fx);
  // the band kernel indexes the working field and both edge buffers with 32-bit cell indices
  if (tbc >= (1L << 31) - 1)
    return fail(ctx, ALIFMM_E_ARG, "travel: %d x %d grid with %ld edge cells exceeds the band kernel's 32-bit indexing",
                fz, fx, 2 * ecells);
  // the arena is sized for this chunk (reused while later chunks fit in it)
  int rc = ensure_arena(ctx, n, cells, sg > 1 ? cells : 0, capL, capC, capS, K, capR, ecells, tbc, sbc);
  if (rc) return rc;
  Arena& a = ctx->arena;
  // subgrid 1: the fields are first written by the band kernel, so their initialisation runs on
  // the fill stream beside the source-init kernel (which uses one CU per source); subgrid > 1:
  // the exact-stage kernel writes them, so in order on the main stream
  hipStream_t fs = (sg == 1 && ctx->fill) ? ctx->fill : ctx->stream;
  if (fs != ctx->stream) {  // the fill stream must not overwrite fields a previous call still reads
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    HIPCHK(hipStreamWaitEvent(fs, ctx->ev[3], 0));
  }
  std::vector<af::BandSrc> hs(n);
  for (int i = 0; i < n; i++) {
    int slot = first_slot + i;
    if ((rc = af_ensure_field(ctx, slot, sg, fz, fx))) return rc;
    af::BandSrc& b = hs[i];
    memset(&b, 0, sizeof b);
    b.T = ctx->fields[slot].d;
    b.S = sg > 1 ? a.S + (size_t)i * a.scells : nullptr;
    int* base = a.lists + (size_t)i * (4 * a.capL + 6 * a.capC);
    b.Lin = base;
    b.FS = base + a.capL;
    b.A = base + 2 * a.capL;
    b.L = base + 3 * a.capL;
    b.C = base + 4 * a.capL;
    b.Cp = b.C + a.capC;
    b.D = b.C + 2 * a.capC;
    b.Rx = b.C + 3 * a.capC;
    b.Bl = b.C + 4 * a.capC;
    b.Bp = b.C + 5 * a.capC;
    double* dbase = a.dlists + (size_t)i * (a.capL + 2 * a.capC);
    b.Lt = dbase;
    b.V = dbase + a.capL;
    b.Dv = b.V + a.capC;
    b.kx = a.kx + i;
    b.Tb = a.Tb + (size_t)i * a.tbc;
    HIPCHK(hipMemsetAsync(b.Tb, 0xFF, (size_t)tbc * 8, fs));  // far: NaN (working field + edge buffers)
    b.Sb = a.Sb + (size_t)i * a.sbc;
    HIPCHK(hipMemsetAsync(b.Sb, 0xFF, (size_t)sbc * 4, fs));  // kFar = -1
    if (K > 1) {
      b.rimc = a.rimc + (size_t)i * K * 2 * capR;
      b.rimt = a.rimt + (size_t)i * K * 2 * capR;
      b.E = b.Tb + tb_cells;  // edge buffers after the working field (fmm_band_k.hip indexes both from Tb)
    }
    if (capS > 0) {
      b.Ts[0] = a.Ts + (size_t)i * 2 * a.capS;
      b.Ts[1] = b.Ts[0] + a.capS;
      b.Ss[0] = a.Ss + (size_t)i * 2 * a.capS;
      b.Ss[1] = b.Ss[0] + a.capS;
    }
    // subgrid > 1: fmm_exact_kernel writes the exact region into the result field, which must
    // start far (NaN, fields.h); subgrid 1: the band kernel's copy-out writes every cell
    if (sg > 1) HIPCHK(hipMemsetAsync(b.T, 0xFF, (size_t)cells * 8, fs));
    if (sg > 1) HIPCHK(hipMemsetAsync(b.S, 0xFF, (size_t)cells * 4, fs));  // the exact kernel's status: kFar
  }
  if (fs != ctx->stream) HIPCHK(hipEventRecord(ctx->ev_fill, fs));
  HIPCHK(hipMemcpyAsync(a.srcs, hs.data(), sizeof(af::BandSrc) * n, hipMemcpyHostToDevice, ctx->stream));
  af::DevModel M = dev_model(ctx);
  af::BandParams P;
  memset(&P, 0, sizeof P);
  P.M = M;
  P.nsrc = n;
  P.sg = sg;
  P.nz = fz;
  P.nx = fx;
  P.dnx = ctx->dnx;
  P.dnz = ctx->dnz;
  P.cdelta = band_cdelta(ctx, sg);
  P.vmax = ctx->vmax;
  P.r0 = ctx->r0;
  P.cdelta_far = sg <= ctx->far_sg ? band_cdelta_far(ctx, sg) : 0.0;
  P.r_far = ctx->r_far;
  P.capL = (int)capL;
  P.capC = (int)capC;
  P.capS = (int)capS;
  P.src = a.srcs;
  P.gox = ctx->gox;
  P.goz = ctx->goz;
  P.prof = ctx->prof;
  P.coop = ctx->coop;
  P.K = K;
  P.wlog = wlog;
  P.xcd_local = ctx->xcd_local;
  P.capR = (int)capR;
  P.ecells = ecells;
  P.tb_pitch = af_band_tb_pitch(fx);
  P.tb_cells = tb_cells;
  P.sb_pitch = af_band_sb_pitch(fx);
  P.max_steps = 200L * (fz + fx) + 100000;
  if (so) {  // stream the fields to the host while the band runs (subgrid 1)
    so->active = false;
    if (sg == 1 && ctx->stream_out && (rc = stream_setup(ctx, so, n, K, wlog, fz, fx))) return rc;
    if (so->active) {
      P.hs = static_cast<double*>(ctx->hstage);
      P.hq = ctx->hq;
      P.hcons = ctx->hcons;
      P.qcap = so->g.qcap;
      P.rslots = so->g.rslots;
      P.tr_log = so->g.trlog;
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  if (sg == 1) {
    if (pre_ho) {  // initialised by the travel call for all its chunks (alifmm_travel)
      P.ho = const_cast<af::HandoverOut*>(pre_ho);
    } else {
      if ((rc = ensure_handover(ctx, n))) return rc;
      // (a.srcs is uploaded above, on this stream: the kernel's word lands in the copy read back below)
      if ((rc = launch_source_init(ctx, n, scx, scz, a.jobs, a.ho, a.sig, &a.srcs[0].init_reused,
                                   (int)(sizeof(af::BandSrc) / sizeof(int)))))
        return rc;
      P.ho = a.ho;
      ctx->ho_last = a.ho;
      ctx->n_ho_last = n;
    }
    P.mode = 0;
  } else {
    for (int i = 0; i < n; i++) {
      long ix = (long)std::nearbyint((scx[i] - ctx->gox) / ctx->dnx), iz = (long)std::nearbyint((scz[i] - ctx->goz) / ctx->dnz);
      if (ix < 0 || ix >= ctx->nx0 || iz < 0 || iz >= ctx->nz0)
        return fail(ctx, ALIFMM_E_ARG, "source %d (%g, %g) outside the grid", i, scx[i], scz[i]);
    }
    HIPCHK(hipMemcpyAsync(a.dscx, scx, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(a.dscz, scz, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    P.mode = 1;
    P.scx = a.dscx;
    P.scz = a.dscz;
    // exact heap walk: both stage grids plus the fine-grid main loop out to exact_r fine nodes
    // beyond the stage-2 window (field units before the final / subgrid: coarse dnx per fine node)
    const long size2 = 2L * sg + (sg - 1) / 2 + 3L * sg;
    P.tstop = (double)(size2 + ctx->exact_r) * ctx->dnx / ctx->vmax;
    P.exact_r = ctx->exact_r;
    P.capL = (int)capL;
    P.capS = (int)capS;
    P.src = a.srcs;
    if (ctx->exact_lds && af_exact_lds_fits(sg, ctx->exact_r)) {
      HIPCHK(af_launch_exact_lds(&P, ctx->stream));
      // a heap past the LDS walk's capacity (error 9): those sources again, from scratch, with
      // the HBM walk (fmm_exact.hip)
      std::vector<af::BandSrc> chk(n);
      HIPCHK(hipMemcpyAsync(chk.data(), a.srcs, sizeof(af::BandSrc) * n, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      bool redo = false;
      for (int i = 0; i < n; i++) redo |= chk[i].err == 9;
      for (int i = 0; i < n; i++) ctx->exact_redo += chk[i].err == 9;
      if (redo) {
        for (int i = 0; i < n; i++) {
          HIPCHK(hipMemsetAsync(hs[i].T, 0xFF, (size_t)cells * 8, ctx->stream));
          HIPCHK(hipMemsetAsync(hs[i].S, 0xFF, (size_t)cells * 4, ctx->stream));
        }
        HIPCHK(hipMemcpyAsync(a.srcs, hs.data(), sizeof(af::BandSrc) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(af_launch_exact(&P, ctx->stream));
      }
    } else {
      HIPCHK(af_launch_exact(&P, ctx->stream));
    }
  }
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  if (fs != ctx->stream) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_fill, 0));
  HIPCHK(hipEventRecord(ctx->ev[4], ctx->stream));  // ev[1] .. ev[4]: the fill not hidden by the source init
  HIPCHK(hipMemsetAsync(a.kx, 0, sizeof(af::KX) * n, ctx->stream));
  HIPCHK(af_launch_band_k(&P, ctx->stream));
  // the copy team takes the tiles as they arrive; joined on every return path below
  struct StreamJoin {
    alifmm_ctx* c;
    StreamOut* s;
    ~StreamJoin() {
      if (!s) return;
      // an early return: the kernel may still store into the pinned ring; it must have ended
      // before the drain stops and the next call resets or frees those buffers
      (void)hipStreamSynchronize(c->stream);
      (void)hipGetLastError();
      stream_finish(c, s);
    }
  } sjoin{ctx, nullptr};
  if (so && so->active) {
    stream_start(ctx, so);
    sjoin.s = so;
  }
  ctx->last_k = K;
  HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
  if (sg > 1)
    for (int i = 0; i < n; i++) HIPCHK(af_launch_scale(hs[i].T, cells, (double)sg, ctx->stream));
  HIPCHK(hipMemcpyAsync(hs.data(), a.srcs, sizeof(af::BandSrc) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (sjoin.s) {
    stream_finish(ctx, so);
    sjoin.s = nullptr;
  }
  float t1 = 0, t2 = 0;
  (void)hipEventElapsedTime(&t1, ctx->ev[0], ctx->ev[1]);
  (void)hipEventElapsedTime(&t2, ctx->ev[1], ctx->ev[2]);
  *ms_init += t1;
  *ms_band += t2;
  float t3 = 0;
  (void)hipEventElapsedTime(&t3, ctx->ev[1], ctx->ev[4]);
  ctx->t_fill_wait += t3;
  if (init_reused)  // walks this chunk's own init launch skipped
    for (int i = 0; i < n; i++) *init_reused += hs[i].init_reused;
  int cap_err = 0;
  for (int i = 0; i < n; i++) {
    Field& f = ctx->fields[first_slot + i];
    for (int k = 0; k < 4; k++) f.steps[k] = hs[i].steps[k];
    f.sweeps = hs[i].nupd;
    for (int k = 0; k < 6; k++) f.prof[k] = hs[i].ph[k];
    for (int k = 0; k < 3; k++) f.prof[6 + k] = hs[i].lsum[k];
    f.prof[9] = hs[i].lmax;
    f.span[0] = hs[i].t_begin;
    f.span[1] = hs[i].t_end;
    for (int k = 0; k < 4; k++) f.prof[10 + k] = hs[i].sub[k];
    if (hs[i].err == 2) cap_err = 1;
    else if (hs[i].err == 3) return fail(ctx, ALIFMM_E_KERNEL, "source %d: init heap overflow", i);
    else if (hs[i].err == 4) return fail(ctx, ALIFMM_E_KERNEL, "source %d: stage grid capacity", i);
    else if (hs[i].err == 7 && !P.coop) return fail(ctx, kRetryCoop, "source %d: band members not co-resident", i);
    else if (hs[i].err) return fail(ctx, ALIFMM_E_KERNEL, "source %d: kernel error %d", i, hs[i].err);
  }
  if (cap_err) return fail(ctx, ALIFMM_E_CAPACITY, "work-list capacity %ld exceeded", capL);
  return ALIFMM_OK;
}

// dsts: per source, the caller's (pageable) field, or null (the fields stay resident only)
static int travel_impl(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                       double* const* dsts) {
  if (!ctx || !ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "travel: no model");
  if ((long)subgrid * (ctx->nz0 - 1) + 1 >= 32768 || (long)subgrid * (ctx->nx0 - 1) + 1 >= 32768)
    return fail(ctx, ALIFMM_E_ARG, "travel: field sides must stay below 32768 nodes (packed list keys)");
  if (subgrid < 1 || subgrid % 2 == 0) return fail(ctx, ALIFMM_E_ARG, "travel: subgrid must be odd, got %d", subgrid);
  if (nsrc < 0 || first_slot < 0 || (nsrc > 0 && (!scx || !scz))) return fail(ctx, ALIFMM_E_ARG, "travel: bad args");
  HIPCHK(hipSetDevice(ctx->device));
  int fz, fx;
  alifmm_field_shape(ctx, subgrid, &fz, &fx);
  const long cells = (long)fz * fx;
  float ms_init = 0, ms_band = 0;
  // Sources per launch: at most half the CUs, so that every source gets >= 2 band members (256
  // C5 receivers on 256 CUs: one launch with one member each 927 ms, two launches of 128 with two
  // members each 810 ms, profiles/r3w_batch.json), balanced over the launches (multiples of 8)
  int chunk = std::max(1, std::min(ctx->batch, std::max(8, ctx->n_cu / 2 / 8 * 8)));
  if (nsrc > chunk) {
    const int nl = (nsrc + chunk - 1) / chunk;
    chunk = std::min(chunk, ((nsrc + nl - 1) / nl + 7) / 8 * 8);
  }
  // subgrid 1 over several launches: one source-init launch for every source of the call (the
  // init uses one CU per source; chunk by chunk it would run alone before each band launch)
  const bool pre_init = subgrid == 1 && nsrc > chunk;
  auto& all = ctx->all;
  if (pre_init && all.reused.n < (size_t)nsrc) {  // (reused: the last to grow)
    if (ctx->ho_last == all.ho) {
      ctx->ho_last = nullptr;
      ctx->n_ho_last = 0;
    }
    all = {};
    HIPCHK(all.ho.grow(nsrc));
    HIPCHK(all.jobs.grow(nsrc));
    HIPCHK(all.sig.grow(nsrc));
    HIPCHK(all.reused.grow(nsrc));
    HIPCHK(hipMemsetAsync(all.sig, 0, sizeof(af::InitSig) * nsrc, ctx->stream));  // no slot valid
  }
  ctx->t_stream_tail = 0;
  ctx->stream_fallback = 0;
  ctx->exact_redo = 0;
  ctx->init_reused = 0;
  ctx->t_fill_wait = 0;
  HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  // the call's timing events, destroyed on every return path
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() {
      if (e) (void)hipEventDestroy(e);
    }
  } t_begin, t_end;
  HIPCHK(hipEventCreate(&t_begin.e));
  HIPCHK(hipEventCreate(&t_end.e));
  HIPCHK(hipEventRecord(t_begin.e, ctx->stream));
  const af::HandoverOut* pre = nullptr;
  if (pre_init) {
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    int rc = launch_source_init(ctx, nsrc, scx, scz, all.jobs, all.ho, all.sig, all.reused, 1);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<int> skipped(nsrc);  // read back before the wait this path already makes
    HIPCHK(hipMemcpyAsync(skipped.data(), all.reused, sizeof(int) * nsrc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int v : skipped) ctx->init_reused += v;
    float t = 0;
    (void)hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]);
    ms_init += t;
    pre = all.ho;
    ctx->ho_last = all.ho;
    ctx->n_ho_last = nsrc;
  }
  for (int s0 = 0; s0 < nsrc; s0 += chunk) {
    int n = std::min(chunk, nsrc - s0);
    int rc;
    StreamOut so;
    so.dst = dsts ? dsts + s0 : nullptr;
    so.n = n;
    StreamOut* sop = dsts ? &so : nullptr;
    // walks skipped by the chunk's first launch (a retry finds the hand-overs that launch wrote)
    int skipped = 0, skipped_retry = 0;
    const long cap0 = ctx->cap_scale;
    for (;;) {
      rc = travel_chunk(ctx, subgrid, n, scx + s0, scz + s0, first_slot + s0, fz, fx, &ms_init, &ms_band,
                        pre ? pre + s0 : nullptr, sop, ctx->cap_scale == cap0 ? &skipped : &skipped_retry);
      if (rc == kRetryCoop) {  // once, gang-scheduled
        const int c0 = ctx->coop;
        ctx->coop = 1;
        rc = travel_chunk(ctx, subgrid, n, scx + s0, scz + s0, first_slot + s0, fz, fx, &ms_init, &ms_band,
                          pre ? pre + s0 : nullptr, sop, &skipped_retry);
        ctx->coop = c0;
        if (rc == kRetryCoop) rc = ALIFMM_E_KERNEL;
      }
      if (rc != ALIFMM_E_CAPACITY || ctx->cap_scale * 4 > 64) break;
      ctx->cap_scale *= 4;  // retry the chunk with larger work lists
    }
    if (rc) return rc;
    ctx->init_reused += skipped;
    if (dsts) {  // fields not streamed (or a tile that never arrived): through the pinned staging ring
      for (int i = 0; i < n; i++) {
        if (so.active && !so.missing[i].load()) continue;
        if (so.active) ctx->stream_fallback++;
        rc = alifmm_copy_fields(ctx, first_slot + s0 + i, 1, dsts[s0 + i], 0, nullptr);
        if (rc) return rc;
      }
    }
  }
  HIPCHK(hipEventRecord(t_end.e, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, t_begin.e, t_end.e);
  ctx->t_init = ms_init;
  ctx->t_band = ms_band;
  ctx->t_total = tot;
  return ALIFMM_OK;
}

extern "C" int alifmm_travel(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                             double* out) {
  if (!out) return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, nullptr);
  int fz = 0, fx = 0;
  if (ctx && ctx->have_model) alifmm_field_shape(ctx, subgrid, &fz, &fx);
  std::vector<double*> d(std::max(nsrc, 0));
  for (int i = 0; i < nsrc; i++) d[i] = out + (size_t)i * fz * fx;
  return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, d.data());
}

extern "C" int alifmm_travel_into(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz, int first_slot,
                                  double* const* dst) {
  if (nsrc > 0 && !dst) return fail(ctx, ALIFMM_E_ARG, "travel_into: no destinations");
  for (int i = 0; i < nsrc; i++)
    if (!dst[i]) return fail(ctx, ALIFMM_E_ARG, "travel_into: destination %d is null", i);
  return travel_impl(ctx, subgrid, nsrc, scx, scz, first_slot, dst);
}

extern "C" hipError_t af_launch_seed(const af::DevModel* M, int nz, int nx, double dnx, double dnz, int nfield, int nseed,
                                     int nclose, const int* seed_cell, const int* close_cell, const int* win,
                                     const double* seed_t, const double* const* from, af::HandoverOut* out,
                                     hipStream_t stream);

// Fields from seed nodes with given times (include/alifmm.h): the host builds the geometry the
// fields share (close cells, their 5 x 5 windows into the seed list) and checks everything it can
// before any launch; fmm_seed_kernel writes one hand-over per field into the context's own buffer;
// travel_chunk runs the band from there as from a source init made elsewhere (pre_ho).
extern "C" int alifmm_travel_seeded(alifmm_ctx* ctx, int nfield, int nseed, const int32_t* seed_iz, const int32_t* seed_ix,
                         const double* seed_t, const int32_t* from_slot, int first_slot, double* out) {
  if (!ctx || !ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: no model");
  if (nfield < 1 || nseed < 1) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: nfield %d, nseed %d", nfield, nseed);
  if (!seed_iz || !seed_ix || first_slot < 0) return fail(ctx, ALIFMM_E_ARG, "travel_seeded: bad args");
  if ((seed_t != nullptr) == (from_slot != nullptr))
    return fail(ctx, ALIFMM_E_ARG, "travel_seeded: exactly one of seed_t and from_slot must be given");
  const int nz = ctx->nz0, nx = ctx->nx0;
  if (nz >= 32768 || nx >= 32768)
    return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field sides must stay below 32768 nodes (packed list keys)");
  std::vector<int> cell(nseed);
  std::unordered_map<int, int> index;  // cell -> place in the seed list
  index.reserve((size_t)nseed * 2);
  for (int k = 0; k < nseed; k++) {
    if (seed_iz[k] < 0 || seed_iz[k] >= nz || seed_ix[k] < 0 || seed_ix[k] >= nx)
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: seed %d (%d, %d) outside the %d x %d grid", k, seed_iz[k],
                  seed_ix[k], nz, nx);
    cell[k] = seed_iz[k] * nx + seed_ix[k];
    if (!index.emplace(cell[k], k).second)
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: seed %d (%d, %d) is listed twice", k, seed_iz[k], seed_ix[k]);
  }
  if (from_slot) {
    for (int i = 0; i < nfield; i++) {
      const int s = from_slot[i];
      if (s < 0 || s >= (int)ctx->fields.size() || !ctx->fields[s].d)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: no field in from_slot %d", s);
      const Field& f = ctx->fields[s];
      if (f.sg != 1 || f.nz != nz || f.nx != nx)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: from_slot %d holds a %d x %d field of subgrid %d, not a subgrid-1 field of the model",
                    s, f.nz, f.nx, f.sg);
      if (s >= first_slot && s < first_slot + nfield)
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: from_slot %d lies inside the destination slots %d .. %d", s,
                    first_slot, first_slot + nfield - 1);
    }
  } else {
    for (size_t k = 0; k < (size_t)nfield * nseed; k++)
      if (!(seed_t[k] >= 0.0) || seed_t[k] == INFINITY || std::signbit(seed_t[k]))
        return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field %d, seed %d: time %g is not finite or is negative",
                    (int)(k / nseed), (int)(k % nseed), seed_t[k]);
  }
  // step -1's cells: every in-grid 4-neighbour of a seed that is no seed, ascending
  std::vector<int> close;
  close.reserve((size_t)nseed * 2);
  auto is_seed = [&](int z, int x) { return index.find(z * nx + x) != index.end(); };
  for (int k = 0; k < nseed; k++) {
    const int z = seed_iz[k], x = seed_ix[k];
    if (x > 0 && !is_seed(z, x - 1)) close.push_back(cell[k] - 1);
    if (x < nx - 1 && !is_seed(z, x + 1)) close.push_back(cell[k] + 1);
    if (z > 0 && !is_seed(z - 1, x)) close.push_back(cell[k] - nx);
    if (z < nz - 1 && !is_seed(z + 1, x)) close.push_back(cell[k] + nx);
  }
  std::sort(close.begin(), close.end());
  close.erase(std::unique(close.begin(), close.end()), close.end());
  const int nclose = (int)close.size();
  ctx->seed_nodes = nseed;
  ctx->seed_close = nclose;
  if ((long)nseed + nclose > af::kHandoverMax)
    return fail(ctx, ALIFMM_E_CAPACITY, "travel_seeded: %d seeds and %d close cells exceed the hand-over's %d entries",
                nseed, nclose, af::kHandoverMax);
  std::vector<int> win((size_t)nclose * 25);
  for (int j = 0; j < nclose; j++) {
    const int z = close[j] / nx, x = close[j] % nx;
    for (int o = 0; o < 25; o++) {
      const int zz = z + o / 5 - 2, xx = x + o % 5 - 2;
      int k = -1;
      if (zz >= 0 && zz < nz && xx >= 0 && xx < nx) {
        auto it = index.find(zz * nx + xx);
        if (it != index.end()) k = it->second;
      }
      win[(size_t)j * 25 + o] = k;
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  auto& sb = ctx->seed;
  HIPCHK(sb.ho.grow((size_t)nfield));
  HIPCHK(sb.cell.grow((size_t)nseed));
  HIPCHK(sb.close.grow((size_t)nclose));
  HIPCHK(sb.win.grow(win.size()));
  ctx->t_stream_tail = 0;
  ctx->stream_fallback = 0;
  ctx->exact_redo = 0;
  ctx->init_reused = 0;
  ctx->t_fill_wait = 0;
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() {
      if (e) (void)hipEventDestroy(e);
    }
  } t_begin, t_end;
  HIPCHK(hipEventCreate(&t_begin.e));
  HIPCHK(hipEventCreate(&t_end.e));
  HIPCHK(hipEventRecord(t_begin.e, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  HIPCHK(hipMemcpyAsync(sb.cell, cell.data(), sizeof(int) * nseed, hipMemcpyHostToDevice, ctx->stream));
  if (nclose > 0) {
    HIPCHK(hipMemcpyAsync(sb.close, close.data(), sizeof(int) * nclose, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(sb.win, win.data(), sizeof(int) * win.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  std::vector<const double*> from;
  if (from_slot) {
    from.resize(nfield);
    for (int i = 0; i < nfield; i++) from[i] = ctx->fields[from_slot[i]].d;
    HIPCHK(sb.from.grow((size_t)nfield));
    HIPCHK(hipMemcpyAsync(sb.from, from.data(), sizeof(double*) * nfield, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIPCHK(sb.t.grow((size_t)nfield * nseed));
    HIPCHK(hipMemcpyAsync(sb.t, seed_t, sizeof(double) * nfield * nseed, hipMemcpyHostToDevice, ctx->stream));
  }
  // n and err of every hand-over: zeroed before, read back after the seed pass
  HIPCHK(hipMemset2DAsync(sb.ho, sizeof(af::HandoverOut), 0, 2 * sizeof(int), nfield, ctx->stream));
  af::DevModel M = dev_model(ctx);
  HIPCHK(af_launch_seed(&M, nz, nx, ctx->dnx, ctx->dnz, nfield, nseed, nclose, sb.cell, sb.close, sb.win,
                        from_slot ? nullptr : sb.t, from_slot ? sb.from : nullptr, sb.ho, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  std::vector<int> head(2 * (size_t)nfield);
  HIPCHK(hipMemcpy2DAsync(head.data(), 2 * sizeof(int), sb.ho, sizeof(af::HandoverOut), 2 * sizeof(int), nfield,
                          hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms_init = 0, ms_band = 0;
  (void)hipEventElapsedTime(&ms_init, ctx->ev[0], ctx->ev[1]);
  ctx->t_seed = ms_init;
  for (int i = 0; i < nfield; i++) {
    if (head[2 * i + 1])  // before the band launch: a negative Tmin would never accept anything
      return fail(ctx, ALIFMM_E_ARG, "travel_seeded: field %d: a seed time read from slot %d is not finite or is negative",
                  i, from_slot ? from_slot[i] : -1);
    if (head[2 * i] != nseed + nclose)
      return fail(ctx, ALIFMM_E_KERNEL, "travel_seeded: field %d: hand-over of %d entries, %d expected", i, head[2 * i],
                  nseed + nclose);
  }
  // chunks, the capacity retry and the cooperative retry as alifmm_travel (travel_impl)
  int chunk = std::max(1, std::min(ctx->batch, std::max(8, ctx->n_cu / 2 / 8 * 8)));
  if (nfield > chunk) {
    const int nl = (nfield + chunk - 1) / chunk;
    chunk = std::min(chunk, ((nfield + nl - 1) / nl + 7) / 8 * 8);
  }
  for (int s0 = 0; s0 < nfield; s0 += chunk) {
    const int n = std::min(chunk, nfield - s0);
    int rc;
    for (;;) {
      rc = travel_chunk(ctx, 1, n, nullptr, nullptr, first_slot + s0, nz, nx, &ms_init, &ms_band, sb.ho + s0);
      if (rc == kRetryCoop) {  // once, gang-scheduled
        const int c0 = ctx->coop;
        ctx->coop = 1;
        rc = travel_chunk(ctx, 1, n, nullptr, nullptr, first_slot + s0, nz, nx, &ms_init, &ms_band, sb.ho + s0);
        ctx->coop = c0;
        if (rc == kRetryCoop) rc = ALIFMM_E_KERNEL;
      }
      if (rc != ALIFMM_E_CAPACITY || ctx->cap_scale * 4 > 64) break;
      ctx->cap_scale *= 4;  // retry the chunk with larger work lists
    }
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(t_end.e, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float tot = 0;
  (void)hipEventElapsedTime(&tot, t_begin.e, t_end.e);
  ctx->t_init = ms_init;
  ctx->t_band = ms_band;
  ctx->t_total = tot;
  if (out) return alifmm_copy_fields(ctx, first_slot, nfield, out, 0, nullptr);
  return ALIFMM_OK;
}
