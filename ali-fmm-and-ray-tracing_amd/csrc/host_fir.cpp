// host_fir.cpp — alifmm_trace_fir: the per-trace FIR and its transpose on traces the caller holds
// (trace_fir.hip), and the tap checks it shares with alifmm_tfm_lsq_pulse (host_tfm.cpp).
#include <chrono>

#include "host_internal.h"

int fir_check_taps(alifmm_ctx* ctx, const char* what, int ncomp, const FirTaps& F) {
  if (!F.taps) return fail(ctx, ALIFMM_E_ARG, "%s: taps is NULL", what);
  if (F.tap_comp != 1 && F.tap_comp != 2) return fail(ctx, ALIFMM_E_ARG, "%s: tap_comp %d is not 1 or 2", what, F.tap_comp);
  if (F.tap_comp == 2 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "%s: complex taps need ncomp 2, not %d", what, ncomp);
  if (F.ntap < 1 || F.ntap > ALIFMM_FIR_MAX_TAPS)
    return fail(ctx, ALIFMM_E_ARG, "%s: ntap %d outside 1 .. %d", what, F.ntap, ALIFMM_FIR_MAX_TAPS);
  if (F.origin < 0 || F.origin >= F.ntap) return fail(ctx, ALIFMM_E_ARG, "%s: origin %d outside [0, %d)", what, F.origin, F.ntap);
  for (int k = 0; k < F.ntap * F.tap_comp; k++)
    if (!std::isfinite(F.taps[k])) return fail(ctx, ALIFMM_E_ARG, "%s: taps[%d] is not finite", what, k / F.tap_comp);
  return ALIFMM_OK;
}

extern "C" int alifmm_trace_fir(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, const double* in, int ntap,
                                int tap_comp, const double* taps, int origin, int transpose, double* out) {
  static_assert(ALIFMM_FIR_MAX_TAPS == af::kFirMaxTaps, "the header's cap is the kernel's");
  if (!ctx) return ALIFMM_E_ARG;
  if (!in || !out) return fail(ctx, ALIFMM_E_ARG, "trace_fir: null pointer");
  if (ntrace < 1 || nt < 1) return fail(ctx, ALIFMM_E_ARG, "trace_fir: ntrace %lld, nt %d", (long long)ntrace, nt);
  if (ncomp != 1 && ncomp != 2) return fail(ctx, ALIFMM_E_ARG, "trace_fir: ncomp %d is not 1 or 2", ncomp);
  if (ntrace > INT64_MAX / 16 / nt) return fail(ctx, ALIFMM_E_ARG, "trace_fir: %lld traces of %d samples", (long long)ntrace, nt);
  const FirTaps F{ntap, tap_comp, taps, origin};
  if (int rc = fir_check_taps(ctx, "trace_fir", ncomp, F)) return rc;
  if (transpose != 0 && transpose != 1) return fail(ctx, ALIFMM_E_ARG, "trace_fir: transpose %d is not 0 or 1", transpose);
  const size_t n = (size_t)ntrace * nt * ncomp, nh = (size_t)ntap * tap_comp;
  HIPCHK(hipSetDevice(ctx->device));
  alifmm_ctx::FirBufs& B = ctx->fir;
  HIPCHK(B.in.grow(n));
  HIPCHK(B.out.grow(n));
  HIPCHK(B.taps.grow(nh));
  const auto c0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemcpy(B.in, in, n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(B.taps, taps, nh * sizeof(double), hipMemcpyHostToDevice));
  ctx->t_fir_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  const af::TraceFirParams P{B.in, B.out, B.taps, ntrace, nt, ntap, origin, transpose};
  HIPCHK(timed_section(ctx, [&](hipStream_t st) { return af_launch_trace_fir(&P, ncomp, tap_comp, st); }, &ctx->t_fir_kernel));
  HIPCHK(hipMemcpy(out, B.out, n * sizeof(double), hipMemcpyDeviceToHost));  // (out may be in: the device's vectors are two)
  return ALIFMM_OK;
}
