// host_fft.cpp — alifmm_trace_spectral: the per-trace spectral filter y = IDFT(G · DFT(x)) on traces
// the caller holds (trace_fft.hip).  fft_front is its front end, which alifmm_trace_pick
// (host_pick.cpp) shares: the argument checks, the response permuted to the transform's element
// order, upload, one kernel, the output left in the context's device buffer.  The entry point adds
// the download.
#include <chrono>

#include "host_internal.h"

int fft_front(alifmm_ctx* ctx, const char* what, int64_t ntrace, int nt, int ncomp, int dtype, const void* in, int nfft,
              int resp_comp, const double* resp, int analytic, double* t_upload, double* t_kernel) {
  static_assert(ALIFMM_FFT_MAX == af::kFftMax, "the header's cap is the kernel's");
  if (ntrace < 1) return fail(ctx, ALIFMM_E_ARG, "%s: ntrace %lld", what, (long long)ntrace);
  if (nt < 1 || nt > ALIFMM_FFT_MAX) return fail(ctx, ALIFMM_E_ARG, "%s: nt %d outside 1 .. %d", what, nt, ALIFMM_FFT_MAX);
  if (ncomp != 1 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "%s: ncomp %d is not 1 or 2", what, ncomp);
  if (dtype != 0 && dtype != 1) return fail(ctx, ALIFMM_E_ARG, "%s: dtype %d is not 0 or 1", what, dtype);
  const int n = nfft == 0 ? 1 << af::fft_log2(nt) : nfft;
  if (n < nt || n > ALIFMM_FFT_MAX || (n & (n - 1)))
    return fail(ctx, ALIFMM_E_ARG, "%s: nfft %d is not 0 or a power of two in [%d, %d]", what, nfft, nt, ALIFMM_FFT_MAX);
  if (resp_comp < 0 || resp_comp > 2) return fail(ctx, ALIFMM_E_ARG, "%s: resp_comp %d is not 0, 1 or 2", what, resp_comp);
  if ((resp_comp > 0) != (resp != nullptr))
    return fail(ctx, ALIFMM_E_ARG, "%s: resp_comp %d with resp %s", what, resp_comp, resp ? "given" : "NULL");
  if (analytic != 0 && analytic != 1) return fail(ctx, ALIFMM_E_ARG, "%s: analytic %d is not 0 or 1", what, analytic);
  if (ntrace > INT64_MAX / 16 / nt) return fail(ctx, ALIFMM_E_ARG, "%s: %lld traces of %d samples", what, (long long)ntrace, nt);
  const int logn = af::fft_log2(n);
  // the response in element order: element idx of the transformed trace is bin bitrev(idx)
  std::vector<double> hrev((size_t)n * resp_comp);
  for (int k = 0; k < n; k++)
    for (int c = 0; c < resp_comp; c++) {
      const double h = resp[(size_t)k * resp_comp + c];
      if (!std::isfinite(h)) return fail(ctx, ALIFMM_E_ARG, "%s: resp[%d] is not finite", what, k);
      hrev[(size_t)af::fft_bitrev((unsigned)k, logn) * resp_comp + c] = h;
    }
  const size_t esz = dtype ? sizeof(float) : sizeof(double);
  const size_t bin = (size_t)ntrace * nt * ncomp * esz, bout = (size_t)ntrace * nt * 2 * esz;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::FftBufs& B = ctx->fft;
  HIPCHK(B.in.grow((bin + 7) / 8));
  HIPCHK(B.out.grow((bout + 7) / 8));
  HIPCHK(B.resp.grow(hrev.size()));
  const auto c0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemcpy(B.in, in, bin, hipMemcpyHostToDevice));
  if (resp_comp) HIPCHK(hipMemcpy(B.resp, hrev.data(), hrev.size() * sizeof(double), hipMemcpyHostToDevice));
  *t_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  const af::TraceFftParams P{B.in.p, B.out.p, resp_comp ? B.resp.p : nullptr, ntrace,
                             af::FftShape{nt, n, logn, resp_comp, analytic, 1.0 / n}};
  HIPCHK(timed_section(ctx, [&](hipStream_t st) { return af_launch_trace_fft(&P, ncomp, dtype, st); }, t_kernel));
  return ALIFMM_OK;
}

extern "C" int alifmm_trace_spectral(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, int dtype, const void* in,
                                     int nfft, int resp_comp, const double* resp, int analytic, void* out) {
  if (!ctx) return ALIFMM_E_ARG;
  if (!in || !out) return fail(ctx, ALIFMM_E_ARG, "trace_spectral: null pointer");
  if (in == out) return fail(ctx, ALIFMM_E_ARG, "trace_spectral: out may not be in");
  const int rc = fft_front(ctx, "trace_spectral", ntrace, nt, ncomp, dtype, in, nfft, resp_comp, resp, analytic,
                           &ctx->t_fft_upload, &ctx->t_fft_kernel);
  if (rc != ALIFMM_OK) return rc;
  const size_t bout = (size_t)ntrace * nt * 2 * (dtype ? sizeof(float) : sizeof(double));
  const auto c1 = std::chrono::steady_clock::now();
  HIPCHK(hipMemcpy(out, ctx->fft.out, bout, hipMemcpyDeviceToHost));
  ctx->t_fft_download = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c1).count();
  return ALIFMM_OK;
}
