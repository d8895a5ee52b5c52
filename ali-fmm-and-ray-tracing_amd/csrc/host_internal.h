// host_internal.h — what the host units (host_*.cpp) share beside the context: each function is
// defined in the unit named next to it; what one unit alone needs stays static in that unit.
#pragma once
#include <atomic>
#include <cmath>
#include <memory>

#include "context.h"
#include "tile_stream.h"

// ---- host_ctx.cpp ----
extern std::atomic<int> g_live_ctx;  // contexts alive in this process (they share its CPU share)
void free_model(alifmm_ctx* c);      // the resident model and the operator built on it

// ---- host_model.cpp ----
af::DevModel dev_model(const alifmm_ctx* c);

// ---- host_fields.cpp ----
// alifmm_travel_into / alifmm_travel with a host destination: the caller's field of each source of
// a chunk, and the state of streaming them out of the band kernel (subgrid 1)
struct StreamOut {
  double* const* dst = nullptr;  // per source of the chunk
  int n = 0;
  bool active = false;  // the band launch streams (stream_setup)
  af::ts::Geometry g;
  std::atomic<int> kernel_done{0};
  std::unique_ptr<std::atomic<int>[]> missing;  // per source: a tile never arrived (copied after)
};
int stream_setup(alifmm_ctx* ctx, StreamOut* so, int n, int K, int wlog, int fz, int fx);
void stream_start(alifmm_ctx* ctx, StreamOut* so);
void stream_finish(alifmm_ctx* ctx, StreamOut* so);
void free_stream_bufs(alifmm_ctx* ctx);
void destroy_team(alifmm_ctx* ctx);
// Device -> pageable host copy of a list of segments through the pinned staging ring
struct D2HSeg {
  const char* src;
  char* dst;
  size_t bytes;
};
int d2h_pageable(alifmm_ctx* ctx, const std::vector<D2HSeg>& segs);

// ---- host_rays.cpp ----
void release_kept_rays(alifmm_ctx* c);  // points kept by alifmm_find_rays(..., ALIFMM_KEEP_RAYS)

// ---- host_fir.cpp ----
// the taps of a trace FIR as an entry point takes them: taps[ntap][tap_comp] on the host
struct FirTaps {
  int ntap, tap_comp;
  const double* taps;
  int origin;
};
// the tap conditions of alifmm_trace_fir and alifmm_tfm_lsq_pulse (`what` names the caller) against
// data of ncomp components
int fir_check_taps(alifmm_ctx* ctx, const char* what, int ncomp, const FirTaps& F);

// ---- host_fft.cpp ----
// alifmm_trace_spectral up to its download (`what` names the caller in messages): its checks of
// these arguments, the upload into ctx->fft.in, the kernel; the filtered traces [ntrace][nt][2] of
// the input's dtype are left in ctx->fft.out.  *t_upload, *t_kernel: the two parts (ms)
int fft_front(alifmm_ctx* ctx, const char* what, int64_t ntrace, int nt, int ncomp, int dtype, const void* in, int nfft,
              int resp_comp, const double* resp, int analytic, double* t_upload, double* t_kernel);

// ---- timed sections ----
// `launch(stream)` between the context's first two events, waited for; its device time into *ms
template <class F>
static hipError_t timed_section(alifmm_ctx* ctx, F launch, double* ms) {
  hipError_t e = hipEventRecord(ctx->ev[0], ctx->stream);
  if (e == hipSuccess) e = launch(ctx->stream);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  float t = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]);
  if (e == hipSuccess) *ms = t;
  return e;
}

// ---- the CGLS solves (alifmm_sens_op_solve, alifmm_tfm_lsq) ----
// the solver arguments both share (`what` names the caller in messages)
static inline int cgls_check(alifmm_ctx* ctx, const char* what, double damp, double smooth, int max_iter, double tol) {
  if (!(damp >= 0) || !std::isfinite(damp)) return fail(ctx, ALIFMM_E_ARG, "%s: damp %g", what, damp);
  if (!(smooth >= 0) || !std::isfinite(smooth)) return fail(ctx, ALIFMM_E_ARG, "%s: smooth %g", what, smooth);
  if (max_iter < 1) return fail(ctx, ALIFMM_E_ARG, "%s: max_iter %d", what, max_iter);
  if (!(tol >= 0) || !std::isfinite(tol)) return fail(ctx, ALIFMM_E_ARG, "%s: tol %g", what, tol);
  return ALIFMM_OK;
}

struct CglsResult {
  int iters = 0, reason = 1;  // reason: 0 converged, 1 max_iter, 2 breakdown
  double rhs2 = 0, gamma0 = 0, gamma = 0, res2 = 0;  // |d|², gamma_0, gamma, |r|²
  // info8 as both entry points report it (slot 6: the operator's entries, 0 for imaging)
  void pack(double* info8, double slot6) const {
    const double info[8] = {(double)iters, sqrt(gamma0), sqrt(gamma), sqrt(rhs2), sqrt(res2), (double)reason, slot6, 0.0};
    std::copy(info, info + 8, info8);
  }
};

// CGLS on the device.  On entry V.r holds the right-hand side (nd values) and the caller has
// recorded ev0; ev1 is recorded here after the last launch (*ms: ev0 .. ev1).  x = p = 0 (nx values
// each); the norm of the right-hand side; form_t: t = Aᵀ r; start: s, p and gamma_0 = |s|² from t
// (0: breakdown); then iter (which ends in a t = Aᵀ r of its own) until its report is -1
// (breakdown) or gamma <= tol² gamma_0; the final norm.  One 8-byte read per norm, one for the
// start and one per iteration.
template <class FormT, class Start, class Iter>
static hipError_t cgls_run(const af::SolveVecs& V, size_t nx, size_t nd, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1,
                           int max_iter, double tol, FormT form_t, Start start, Iter iter, CglsResult* out, double* ms) {
#define CG(call)                     \
  do {                               \
    hipError_t e_ = (call);          \
    if (e_ != hipSuccess) return e_; \
  } while (0)
  // one scalar of the device's (8 bytes) after the work queued so far
  auto scalar = [&](int which, double* v) {
    hipError_t e = hipMemcpyAsync(v, V.scal + which, 8, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  };
  double rhs2 = 0, gamma0 = 0, gamma = 0, res2 = 0;
  CG(hipMemsetAsync(V.x, 0, 2 * nx * sizeof(double), st));  // x = p = 0 (p follows x)
  CG(hipMemsetAsync(V.scal, 0, af::kSolScalars * sizeof(double), st));
  CG(af_launch_solve_norm(V.r, (long)nd, &V, st));
  CG(scalar(af::kSolNorm, &rhs2));
  CG(form_t());
  CG(start());
  CG(scalar(af::kSolReport, &gamma0));
  gamma = gamma0;
  int iters = 0, reason = 1;
  if (gamma0 == 0.0) reason = 2;
  else
    for (int it = 1; it <= max_iter; it++) {
      CG(iter());
      double rep = 0;
      CG(scalar(af::kSolReport, &rep));  // the one read of an iteration: the new gamma, -1: |q|² was 0
      if (rep < 0) {
        reason = 2;
        break;
      }
      gamma = rep;
      iters = it;
      if (gamma <= tol * tol * gamma0) {
        reason = 0;
        break;
      }
    }
  CG(af_launch_solve_norm(V.r, (long)nd, &V, st));
  CG(scalar(af::kSolNorm, &res2));
  CG(hipEventRecord(ev1, st));
  CG(hipStreamSynchronize(st));
  float t = 0;
  CG(hipEventElapsedTime(&t, ev0, ev1));
  *ms = t;
  out->iters = iters, out->reason = reason;
  out->rhs2 = rhs2, out->gamma0 = gamma0, out->gamma = gamma, out->res2 = res2;
  return hipSuccess;
#undef CG
}
