// host_pick.cpp — alifmm_trace_pick: time-of-flight picks from traces the caller holds
// (trace_pick.hip): the argument checks, the upload of the traces and the gates (filter 1: through
// alifmm_trace_spectral's front end, host_fft.cpp fft_front, whose output stays on the device and is
// what the picker reads), one pick kernel, and the download of six numbers per trace.
#include <chrono>

#include "host_internal.h"

extern "C" int alifmm_trace_pick(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, int dtype, const void* in, int filter,
                                 int nfft, int resp_comp, const double* resp, int analytic, const int32_t* gate_lo,
                                 const int32_t* gate_hi, int mode, double frac, int guard, double* pos, double* amp,
                                 int32_t* idx, double* amp2, int32_t* idx2, int32_t* flags) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!in || !gate_lo || !gate_hi || !pos || !amp || !idx || !amp2 || !idx2 || !flags)
    return fail(ctx, ALIFMM_E_ARG, "trace_pick: null pointer");
  if (ntrace < 1) return fail(ctx, ALIFMM_E_ARG, "trace_pick: ntrace %lld", (long long)ntrace);
  if (nt < 1) return fail(ctx, ALIFMM_E_ARG, "trace_pick: nt %d", nt);
  if (ncomp != 1 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "trace_pick: ncomp %d is not 1 or 2", ncomp);
  if (dtype != 0 && dtype != 1) return fail(ctx, ALIFMM_E_ARG, "trace_pick: dtype %d is not 0 or 1", dtype);
  if (filter != 0 && filter != 1) return fail(ctx, ALIFMM_E_ARG, "trace_pick: filter %d is not 0 or 1", filter);
  if (mode != 0 && mode != 1) return fail(ctx, ALIFMM_E_ARG, "trace_pick: mode %d is not 0 or 1", mode);
  if (mode == 1 && !(frac > 0.0 && frac <= 1.0)) return fail(ctx, ALIFMM_E_ARG, "trace_pick: frac %g outside (0, 1]", frac);
  if (guard < 0) return fail(ctx, ALIFMM_E_ARG, "trace_pick: guard %d", guard);
  if (ntrace > INT64_MAX / 16 / nt)
    return fail(ctx, ALIFMM_E_ARG, "trace_pick: %lld traces of %d samples", (long long)ntrace, nt);
  for (int64_t t = 0; t < ntrace; t++)
    if (gate_lo[t] < 0 || gate_hi[t] > nt)
      return fail(ctx, ALIFMM_E_ARG, "trace_pick: gate %lld [%d, %d) leaves the trace of %d samples", (long long)t,
                  gate_lo[t], gate_hi[t], nt);
  if (!filter && (nfft != 0 || resp_comp != 0 || resp != nullptr || analytic != 0))
    return fail(ctx, ALIFMM_E_ARG, "trace_pick: filter 0 with nfft %d, resp_comp %d, resp %s, analytic %d", nfft, resp_comp,
                resp ? "given" : "NULL", analytic);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  double t_upload = 0, t_filter = 0;
  const void* traces = nullptr;  // what the picker reads, on the device
  int pick_comp = ncomp;
  if (filter) {
    const int rc = fft_front(ctx, "trace_pick", ntrace, nt, ncomp, dtype, in, nfft, resp_comp, resp, analytic, &t_upload,
                             &t_filter);
    if (rc != ALIFMM_OK) return rc;
    traces = ctx->fft.out.p;
    pick_comp = 2;
  } else {
    const size_t bin = (size_t)ntrace * nt * ncomp * (dtype ? sizeof(float) : sizeof(double));
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->fft.in.grow((bin + 7) / 8));
    const auto c0 = now();
    HIPCHK(hipMemcpy(ctx->fft.in, in, bin, hipMemcpyHostToDevice));
    t_upload = ms(c0, now());
    traces = ctx->fft.in.p;
  }
  alifmm_ctx::PickBufs& B = ctx->pick;
  const size_t n = (size_t)ntrace;
  HIPCHK(B.gates.grow(2 * n));
  HIPCHK(B.outd.grow(3 * n));
  HIPCHK(B.outi.grow(3 * n));
  const auto c1 = now();
  HIPCHK(hipMemcpy(B.gates.p, gate_lo, n * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.gates.p + n, gate_hi, n * sizeof(int), hipMemcpyHostToDevice));
  ctx->t_pick_upload = t_upload + ms(c1, now());
  ctx->t_pick_filter = t_filter;
  const af::TracePickParams P{traces,   B.gates.p,    B.gates.p + n,    ntrace,   nt,           mode,
                              guard,    frac,         B.outd.p,         B.outd.p + n, B.outd.p + 2 * n,
                              B.outi.p, B.outi.p + n, B.outi.p + 2 * n};
  HIPCHK(timed_section(ctx, [&](hipStream_t st) { return af_launch_trace_pick(&P, pick_comp, dtype, st); }, &ctx->t_pick_kernel));
  std::vector<double> hd(3 * n);
  std::vector<int32_t> hi(3 * n);
  const auto c2 = now();
  HIPCHK(hipMemcpy(hd.data(), B.outd.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), B.outi.p, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost));
  ctx->t_pick_download = ms(c2, now());
  std::copy(hd.begin(), hd.begin() + n, pos);
  std::copy(hd.begin() + n, hd.begin() + 2 * n, amp);
  std::copy(hd.begin() + 2 * n, hd.end(), amp2);
  std::copy(hi.begin(), hi.begin() + n, idx);
  std::copy(hi.begin() + n, hi.begin() + 2 * n, idx2);
  std::copy(hi.begin() + 2 * n, hi.end(), flags);
  return ALIFMM_OK;
}
