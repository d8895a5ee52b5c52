// cr_eval.hip — cr_math.h's atan / sin / cos / tan / sincos on caller-supplied arguments with the
// tables in LDS, as the solver kernels read them (fmm_band_k.hip, fmm_init.hip, fmm_exact*.hip,
// rays.hip, ray_sens.hip): the lds_tables = 1 side of alifmm_cr_math (utils.hip: the global tables).
#define CR_LDS_TABLES  // cr_math.h tables in LDS (crm::lds_init at kernel start)
#include "kernels.h"
#include "cr_eval.h"

namespace af {

__global__ void __launch_bounds__(kCrEvalThreads) cr_eval_lds_kernel(int fn, long long n, const double* x, double* out,
                                                                     double* out2) {
  crm::lds_init();
  __syncthreads();
  const long long k = (long long)blockIdx.x * kCrEvalThreads + threadIdx.x;
  if (k >= n) return;
  cr_eval_one(fn, x[k], out + k, out2 ? out2 + k : nullptr);
}

}  // namespace af

extern "C" hipError_t af_launch_cr_eval_lds(int fn, long long n, const double* x, double* out, double* out2,
                                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const unsigned blocks = af::cr_eval_blocks(n);
  if (!blocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(af::cr_eval_lds_kernel, dim3(blocks), dim3(af::kCrEvalThreads), 0, stream, fn, n, x, out, out2);
  return hipGetLastError();
}
