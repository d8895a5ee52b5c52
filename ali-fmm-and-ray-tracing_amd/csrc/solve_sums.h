// solve_sums.h — the device side of solve_ops.h's sums: a workgroup's sum and stage 1 of a two-stage
// sum, shared by the CGLS kernels of sens_solve.hip and tfm_solve.hip.  HIP device code; the orders
// are solve_ops.h's.
#pragma once
#include "device_common.h"
#include "solve_ops.h"

namespace af {

// the workgroup's sum of a (solve_ops.h: wave tree, then the waves' sums); valid in thread 0
AF_DEV double solve_block_sum(double a, double* w) {
  a = solve_wave_tree(a, [](double v, int o) { return __shfl_xor(v, o); });
  if ((threadIdx.x & (kSolveLanes - 1)) == 0) w[threadIdx.x / kSolveLanes] = a;
  __syncthreads();
  return solve_block_tree(w);
}

// stage 1 of a two-stage sum over n elements (solve_ops.h solve_parts): parts[blockIdx.x]
template <class Term>
AF_DEV void solve_part(long n, double* parts, double* w, Term term) {
  const double a = solve_block_sum(
      solve_lane_sum(n, (int)(blockIdx.x * kSolveBlock + threadIdx.x), (int)(gridDim.x * kSolveBlock), term), w);
  if (threadIdx.x == 0) parts[blockIdx.x] = a;
}

}  // namespace af
