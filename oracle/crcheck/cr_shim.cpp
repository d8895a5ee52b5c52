// C entry points of cr_math.h (the device's correctly rounded atan / sin / cos / tan) for the
// oracle's CR build (oracle/Makefile: lib/liboracle_cr.so): the same C restatement with the
// trigonometric calls the device makes instead of glibc's.
#include "../../ali-fmm-and-ray-tracing_amd/csrc/cr_math.h"

extern "C" {
double oref_cr_atan(double x) { return crm::atan(x); }
double oref_cr_sin(double x) { return crm::sin(x); }
double oref_cr_cos(double x) { return crm::cos(x); }
double oref_cr_tan(double x) { return crm::tan(x); }

// n arguments at once, numbered as alifmm_cr_math numbers them: fn 0 atan, 1 sin, 2 cos, 3 tan ->
// out; 4 sincos -> sin out, cos out2.  0, or -1 for an unknown fn / a missing out2 (nothing written).
int oref_cr_batch(int fn, long long n, const double* x, double* out, double* out2) {
  if (fn < 0 || fn > 4 || (fn == 4 && !out2)) return -1;
  for (long long i = 0; i < n; i++) {
    switch (fn) {
      case 0: out[i] = crm::atan(x[i]); break;
      case 1: out[i] = crm::sin(x[i]); break;
      case 2: out[i] = crm::cos(x[i]); break;
      case 3: out[i] = crm::tan(x[i]); break;
      default: crm::sincos(x[i], out + i, out2 + i);
    }
  }
  return 0;
}
}
