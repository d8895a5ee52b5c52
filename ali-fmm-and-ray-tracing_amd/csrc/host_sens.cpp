// host_sens.cpp — travel-time sensitivities along rays (alifmm_ray_sens), the resident operator
// built from them (alifmm_sens_op_build / _release / _apply) and its CGLS solve (alifmm_sens_op_solve).
#include <chrono>
#include <cstring>

#include "host_internal.h"

// The front half of a sensitivity request, shared by alifmm_ray_sens and alifmm_sens_op_build (`what`
// names the caller in messages): the rays' first points, the chunks of whole rays whose points are
// on the device together, the per-ray arrays uploaded, the count pass run, and the row offsets and
// status of every ray on the host.  run_chunk then runs the fill pass chunk by chunk.
struct SensRequest {
  struct Chunk {
    int r0, r1;       // [first ray, end ray)
    const double* d;  // device pointer (kept points) or null (host points, uploaded into the context's buffer)
  };
  const char* what = "";
  const double* ray_xy = nullptr;
  std::vector<long long> off, rows;
  std::vector<int32_t> status;
  std::vector<Chunk> chunks;
  af::SensParams P;
  int resident = -1;  // the host chunk whose points the context's buffer holds
  long long total = 0;
};

static int sens_check_args(alifmm_ctx* ctx, const char* what, int subgrid, int nrays, const int32_t* ray_len) {
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "%s: no model", what);
  if (subgrid < 1) return fail(ctx, ALIFMM_E_ARG, "%s: subgrid %d", what, subgrid);
  if (nrays < 0) return fail(ctx, ALIFMM_E_ARG, "%s: nrays %d", what, nrays);
  if (!ray_len) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len is NULL", what);
  return ALIFMM_OK;
}

// the chunk's points on the device, then one pass (count or fill) over its rays
static int sens_run_chunk(alifmm_ctx* ctx, SensRequest& R, int ci, bool fill) {
  alifmm_ctx::SensBufs& B = ctx->sens;
  af::SensParams& P = R.P;
  const SensRequest::Chunk& c = R.chunks[ci];
  const long long n = R.off[c.r1] - R.off[c.r0];
  if (c.d) {
    P.xy = c.d;
  } else {
    if (R.resident != ci) {
      HIPCHK(B.xy.grow((size_t)2 * std::max<long long>(n, 1)));
      const auto t0 = std::chrono::steady_clock::now();
      if (n) HIPCHK(hipMemcpy(B.xy, R.ray_xy + 2 * R.off[c.r0], (size_t)n * 16, hipMemcpyHostToDevice));
      ctx->t_sens_upload += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      R.resident = ci;
    }
    P.xy = B.xy;
  }
  P.pt0 = R.off[c.r0];
  P.ray0 = c.r0;
  P.nrays = c.r1 - c.r0;
  double ms = 0;
  const auto launch = [&](hipStream_t st) { return fill ? af_launch_sens_fill(&P, st) : af_launch_sens_count(&P, st); };
  HIPCHK(timed_section(ctx, launch, &ms));
  ctx->t_sens_kernel += ms;
  return ALIFMM_OK;
}

static int sens_count_pass(alifmm_ctx* ctx, SensRequest& R, int subgrid, int nrays, const int32_t* ray_len,
                           const int32_t* flags, const double* ray_xy, const double* ray_w) {
  const char* what = R.what;
  R.ray_xy = ray_xy;
  // the rays' first points; a length below 0 counts as no points
  std::vector<long long>& off = R.off;
  off.assign((size_t)nrays + 1, 0);
  for (int k = 0; k < nrays; k++) off[k + 1] = off[k] + std::max(ray_len[k], 0);
  const long long npts = off[nrays];
  std::vector<SensRequest::Chunk>& chunks = R.chunks;
  if (!ray_xy) {
    if (!ctx->kept_rays.empty())
      return fail(ctx, ALIFMM_E_ARG, "%s: the kept rays are staged on the host (several subgrids in one "
                                     "find_rays call); pass their points as ray_xy", what);
    if (npts != ctx->kept_pts)
      return fail(ctx, ALIFMM_E_ARG, "%s: ray_len adds up to %lld points, %lld are kept", what, npts,
                  (long long)ctx->kept_pts);
    int r = 0;
    for (auto& k : ctx->kept_dev) {
      const long long end = off[r] + k.npts;
      int r1 = r;
      while (r1 < nrays && off[r1 + 1] <= end) r1++;
      if (off[r1] != end) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len does not match the kept rays", what);
      if (r1 > r) chunks.push_back({r, r1, k.d});
      r = r1;
    }
    if (r != nrays && off[r] != npts) return fail(ctx, ALIFMM_E_ARG, "%s: ray_len does not match the kept rays", what);
  } else {
    const long long kChunkPts = 1LL << 24;  // 256 MB of points per upload (a longer ray is a chunk of its own)
    for (int r = 0; r < nrays;) {
      int r1 = r + 1;
      while (r1 < nrays && off[r1 + 1] - off[r] <= kChunkPts) r1++;
      chunks.push_back({r, r1, nullptr});
      r = r1;
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SensBufs& B = ctx->sens;
  const size_t nr = (size_t)nrays;
  ctx->t_sens_upload = ctx->t_sens_kernel = 0;
  ctx->sens_entries = 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(now() - t).count();
  };
  HIPCHK(B.off.grow(nr));
  HIPCHK(B.len.grow(nr));
  HIPCHK(B.cnt.grow(nr));
  HIPCHK(B.status.grow(nr));
  if (flags) HIPCHK(B.flags.grow(nr));
  if (ray_w) HIPCHK(B.w.grow(nr));
  {
    const auto t0 = now();
    if (nrays) {
      HIPCHK(hipMemcpy(B.off, off.data(), nr * 8, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(B.len, ray_len, nr * 4, hipMemcpyHostToDevice));
      if (flags) HIPCHK(hipMemcpy(B.flags, flags, nr * 4, hipMemcpyHostToDevice));
      if (ray_w) HIPCHK(hipMemcpy(B.w, ray_w, nr * 8, hipMemcpyHostToDevice));
    }
    ctx->t_sens_upload += ms_since(t0);
  }
  af::SensParams& P = R.P;
  memset(&P, 0, sizeof P);
  P.M = dev_model(ctx);
  P.sg = subgrid;
  P.dnx = ctx->dnx;
  P.off = B.off;
  P.len = B.len;
  P.flags = flags ? B.flags : nullptr;
  P.w = ray_w ? B.w : nullptr;
  P.cnt = B.cnt;
  P.status = B.status;
  int rc = ALIFMM_OK;
  for (int ci = 0; ci < (int)chunks.size(); ci++)
    if ((rc = sens_run_chunk(ctx, R, ci, false))) return rc;
  // row offsets (rays outside every chunk have no points: no entries, status 0)
  R.rows.assign(nr + 1, 0);
  R.status.assign(nr, 0);
  {
    std::vector<long long> cnt(nr, 0);
    for (const SensRequest::Chunk& c : chunks) {
      HIPCHK(hipMemcpy(cnt.data() + c.r0, B.cnt + c.r0, (size_t)(c.r1 - c.r0) * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(R.status.data() + c.r0, B.status + c.r0, (size_t)(c.r1 - c.r0) * 4, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < nr; k++) R.rows[k + 1] = R.rows[k] + cnt[k];
  }
  R.total = R.rows[nr];
  ctx->sens_entries = R.total;
  return ALIFMM_OK;
}

extern "C" int alifmm_ray_sens(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                               const double* ray_xy, const double* ray_w, double* maps, int64_t* row_ptr, int64_t cap,
                               int32_t* col, double* len, double* time, double* dth, int32_t* ray_status) {
  if (!ctx) return ALIFMM_E_ARG;
  if (int rc = sens_check_args(ctx, "ray_sens", subgrid, nrays, ray_len)) return rc;
  const bool want_rows = col || len || time || dth;
  if (!maps && !row_ptr && !want_rows && !ray_status)
    return fail(ctx, ALIFMM_E_ARG, "ray_sens: nothing requested (maps, row_ptr and ray_status are NULL)");
  if (want_rows && !row_ptr) return fail(ctx, ALIFMM_E_ARG, "ray_sens: row arrays without row_ptr");
  SensRequest R;
  R.what = "ray_sens";
  int rc = sens_count_pass(ctx, R, subgrid, nrays, ray_len, flags, ray_xy, ray_w);
  if (rc) return rc;
  alifmm_ctx::SensBufs& B = ctx->sens;
  af::SensParams& P = R.P;
  const std::vector<long long>& rows = R.rows;
  const size_t nr = (size_t)nrays, ncell = (size_t)ctx->nz0 * ctx->nx0;
  const long long total = R.total;
  if (row_ptr)
    for (size_t k = 0; k <= nr; k++) row_ptr[k] = rows[k];
  if (ray_status && nrays) memcpy(ray_status, R.status.data(), nr * 4);
  if (want_rows && cap < total)
    return fail(ctx, ALIFMM_E_ARG, "ray_sens: cap %lld < %lld entries (row_ptr holds the sizes)", (long long)cap, total);
  if (!maps && !want_rows) return ALIFMM_OK;
  // the fill pass: maps in the context's buffer, rows in buffers of this call
  int32_t* d_col = nullptr;
  double* d_e[3] = {nullptr, nullptr, nullptr};
  auto cleanup = [&] {
    dfree(d_col);
    for (double* p : d_e) dfree(p);
  };
  double* const h_e[3] = {len, time, dth};
  hipError_t e = hipSuccess;
  if (maps) {
    e = B.maps.grow(3 * ncell);
    if (e == hipSuccess) e = hipMemsetAsync(B.maps, 0, 3 * ncell * 8, ctx->stream);
  }
  if (want_rows && total > 0) {
    if (e == hipSuccess) e = B.row.grow(nr);
    if (e == hipSuccess) e = hipMemcpy(B.row, rows.data(), nr * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && col) e = dalloc(&d_col, (size_t)total);
    for (int q = 0; q < 3; q++)
      if (e == hipSuccess && h_e[q]) e = dalloc(&d_e[q], (size_t)total);
  }
  if (e != hipSuccess) {
    cleanup();
    return fail(ctx, ALIFMM_E_HIP, "ray_sens: %s", hipGetErrorString(e));
  }
  P.maps = maps ? B.maps : nullptr;
  if (want_rows && total > 0) {
    P.row = B.row;
    P.col = d_col;
    P.elen = d_e[0];
    P.etime = d_e[1];
    P.edth = d_e[2];
  }
  if (total > 0 && (maps || P.row))
    for (int ci = 0; ci < (int)R.chunks.size() && !rc; ci++) rc = sens_run_chunk(ctx, R, ci, true);
  if (!rc && maps) {
    std::vector<D2HSeg> segs{{(const char*)B.maps.p, (char*)maps, 3 * ncell * 8}};
    rc = d2h_pageable(ctx, segs);
  }
  if (!rc && P.row) {
    std::vector<D2HSeg> segs;
    if (col) segs.push_back({(const char*)d_col, (char*)col, (size_t)total * 4});
    for (int q = 0; q < 3; q++)
      if (h_e[q]) segs.push_back({(const char*)d_e[q], (char*)h_e[q], (size_t)total * 8});
    rc = d2h_pageable(ctx, segs);
  }
  cleanup();
  return rc;
}

extern "C" int alifmm_sens_op_release(alifmm_ctx* ctx) {
  if (!ctx) return ALIFMM_E_ARG;
  (void)hipSetDevice(ctx->device);
  ctx->op = {};
  return ALIFMM_OK;
}

extern "C" int alifmm_sens_op_build(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                         const double* ray_xy, int quantity, const double* col_scale, int64_t* entries,
                         int32_t* ray_status) {
  if (!ctx) return ALIFMM_E_ARG;
  if (int rc = sens_check_args(ctx, "sens_op_build", subgrid, nrays, ray_len)) return rc;
  if (quantity < 0 || quantity > 2) return fail(ctx, ALIFMM_E_ARG, "sens_op_build: quantity %d (0 len, 1 time, 2 dth)", quantity);
  const size_t nr = (size_t)nrays, ncell = (size_t)ctx->nz0 * ctx->nx0;
  if (col_scale)
    for (size_t c = 0; c < ncell; c++)
      if (!std::isfinite(col_scale[c])) return fail(ctx, ALIFMM_E_ARG, "sens_op_build: col_scale[%zu] is not finite", c);
  const auto t0 = std::chrono::steady_clock::now();
  SensRequest R;
  R.what = "sens_op_build";
  int rc = sens_count_pass(ctx, R, subgrid, nrays, ray_len, flags, ray_xy, nullptr);
  if (rc) return rc;
  ctx->op = {};  // the request is good: the new operator replaces the resident one
  const long long total = R.total;
  if (entries) *entries = total;
  if (ray_status && nrays) memcpy(ray_status, R.status.data(), nr * 4);
  if (total >= (1LL << 31))
    return fail(ctx, ALIFMM_E_CAPACITY, "sens_op_build: %lld entries, an operator holds fewer than 2^31", total);
  alifmm_ctx::SensOpBufs& O = ctx->op;
  const size_t ne = (size_t)total;
  unsigned* scratch = nullptr;  // key | key2 | idx | idx2
  void* temp = nullptr;
  int* cursor = nullptr;
  const size_t temp_bytes = total ? af_solve_sort_temp(total, (long)ncell) : 0;
  auto drop = [&] {
    dfree(scratch);
    dfree(temp);
    dfree(cursor);
  };
  auto bail = [&](hipError_t e) {
    drop();
    ctx->op = {};
    return fail(ctx, ALIFMM_E_HIP, "sens_op_build: %s", hipGetErrorString(e));
  };
  hipError_t e = O.row_ptr.grow(nr + 1);
  if (e == hipSuccess) e = O.col.grow(ne);
  if (e == hipSuccess) e = O.val.grow(ne);
  if (e == hipSuccess) e = O.col_ptr.grow(ncell + 1);
  if (e == hipSuccess) e = O.row.grow(ne);
  if (e == hipSuccess) e = O.cval.grow(ne);
  if (e == hipSuccess && col_scale) e = O.cs.grow(ncell);
  if (e == hipSuccess) e = dalloc(&scratch, 4 * ne);
  if (e == hipSuccess) e = dalloc((char**)&temp, temp_bytes);
  if (e == hipSuccess) e = dalloc(&cursor, 3);
  if (e == hipSuccess) e = hipMemcpy(O.row_ptr, R.rows.data(), (nr + 1) * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && col_scale) e = hipMemcpy(O.cs, col_scale, ncell * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) return bail(e);
  // the fill pass writes the CSR in place: the columns and the one quantity
  af::SensParams& P = R.P;
  P.row = O.row_ptr;
  P.col = O.col;
  (quantity == 0 ? P.elen : quantity == 1 ? P.etime : P.edth) = O.val;
  if (total > 0)
    for (int ci = 0; ci < (int)R.chunks.size() && !rc; ci++) rc = sens_run_chunk(ctx, R, ci, true);
  if (rc) {
    drop();
    ctx->op = {};
    return rc;
  }
  af::SensOp& A = O.A;
  A.nrays = nrays;
  A.nz = ctx->nz0;
  A.nx = ctx->nx0;
  A.ncell = (long)ncell;
  A.entries = total;
  A.row_ptr = O.row_ptr;
  A.col = O.col;
  A.val = O.val;
  A.col_ptr = O.col_ptr;
  A.row = O.row;
  A.cval = O.cval;
  A.cs = O.cs;
  // the transposed copy, then the non-empty columns by length class: counted, then listed
  e = af_launch_solve_transpose(&A, O.col_ptr, O.row, O.cval, scratch, scratch + ne, scratch + 2 * ne, scratch + 3 * ne,
                                temp, temp_bytes, ctx->stream);
  int n3[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, sizeof n3, ctx->stream);
  if (e == hipSuccess) e = af_launch_solve_classify(O.col_ptr, (long)ncell, nullptr, cursor, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(n3, cursor, sizeof n3, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = O.cols.grow((size_t)n3[0] + n3[1] + n3[2]);
  const int first3[3] = {0, n3[0], n3[0] + n3[1]};
  if (e == hipSuccess) e = hipMemcpyAsync(cursor, first3, sizeof first3, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = af_launch_solve_classify(O.col_ptr, (long)ncell, O.cols, cursor, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return bail(e);
  for (int q = 0; q < 3; q++) {
    A.cols[q] = O.cols + first3[q];
    A.ncols[q] = n3[q];
  }
  drop();
  O.have = true;
  ctx->t_solve_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ALIFMM_OK;
}

extern "C" int alifmm_sens_op_apply(alifmm_ctx* ctx, int transpose, const double* in, double* out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: no model");
  if (!ctx->op.have) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: no resident operator (alifmm_sens_op_build)");
  if (!in || !out) return fail(ctx, ALIFMM_E_ARG, "sens_op_apply: %s is NULL", in ? "out" : "in");
  const af::SensOp& A = ctx->op.A;
  const size_t nc = (size_t)A.ncell, nr = (size_t)A.nrays;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SolveBufs& S = ctx->solve;
  HIPCHK(S.cell.grow(5 * nc));
  HIPCHK(S.ray.grow(2 * nr));
  double* din = transpose ? S.ray : S.cell;
  double* dout = transpose ? S.cell : S.ray;
  const size_t nin = transpose ? nr : nc, nout = transpose ? nc : nr;
  if (nin) HIPCHK(hipMemcpy(din, in, nin * 8, hipMemcpyHostToDevice));
  const auto launch = [&](hipStream_t st) {
    return transpose ? af_launch_solve_colprod(&A, din, dout, st) : af_launch_solve_rowprod(&A, din, S.cell + nc, dout, st);
  };
  HIPCHK(timed_section(ctx, launch, &ctx->t_solve_kernel));
  if (nout) HIPCHK(hipMemcpy(out, dout, nout * 8, hipMemcpyDeviceToHost));
  return ALIFMM_OK;
}

extern "C" int alifmm_sens_op_solve(alifmm_ctx* ctx, const double* rhs, double damp, double smooth, int max_iter, double tol,
                         double* x, double* info8) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!ctx->have_model) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: no model");
  if (!ctx->op.have) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: no resident operator (alifmm_sens_op_build)");
  if (!rhs || !x) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: %s is NULL", rhs ? "x" : "rhs");
  if (int rc = cgls_check(ctx, "sens_op_solve", damp, smooth, max_iter, tol)) return rc;
  const af::SensOp& A = ctx->op.A;
  const size_t nc = (size_t)A.ncell, nr = (size_t)A.nrays;
  for (size_t k = 0; k < nr; k++)
    if (!std::isfinite(rhs[k])) return fail(ctx, ALIFMM_E_ARG, "sens_op_solve: rhs[%zu] is not finite", k);
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::SolveBufs& S = ctx->solve;
  HIPCHK(S.cell.grow(5 * nc));
  HIPCHK(S.ray.grow(2 * nr));
  HIPCHK(S.small.grow((size_t)af::kSolveMaxParts + af::kSolScalars));
  af::SolveVecs V;
  V.x = S.cell;
  V.p = S.cell + nc;
  V.s = S.cell + 2 * nc;
  V.t = S.cell + 3 * nc;
  V.xs = S.cell + 4 * nc;
  V.r = S.ray;
  V.q = S.ray + nr;
  V.parts = S.small;
  V.scal = S.small + af::kSolveMaxParts;
  V.damp2 = damp * damp;
  V.smooth2 = smooth * smooth;
  hipStream_t st = ctx->stream;
  if (nr) HIPCHK(hipMemcpy(V.r, rhs, nr * 8, hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  CglsResult R;
  const hipError_t e = cgls_run(
      V, nc, nr, st, ctx->ev[0], ctx->ev[1], max_iter, tol, [&] { return af_launch_solve_colprod(&A, V.r, V.t, st); },
      [&] { return af_launch_solve_start(&A, &V, st); },  // x = 0: s = Aᵀ rhs, p = s, gamma_0 = |s|²
      [&] { return af_launch_solve_iter(&A, &V, st); }, &R, &ctx->t_solve_kernel);
  if (e != hipSuccess) return fail(ctx, ALIFMM_E_HIP, "sens_op_solve: %s", hipGetErrorString(e));
  ctx->solve_iters = R.iters;
  if (nc) HIPCHK(hipMemcpy(x, V.x, nc * 8, hipMemcpyDeviceToHost));
  if (info8) R.pack(info8, (double)A.entries);
  return ALIFMM_OK;
}
