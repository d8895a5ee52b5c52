// skip_pairs.hip — back-wall echo paths between element pairs (include/alifmm.h alifmm_skip_pick,
// alifmm_skip_rays): the pick of the specular node, w* = argmin over the reflector nodes of
// T_a(w) + T_b(w), and the join of the two back-traced legs w* -> a and w* -> b into one ray
// a ... w* ... b.  The per-element code (finite test, key order, joined-point indices) is
// skip_pick.h, shared with the host simulation tests/skip_sim.cpp.
//
//   skip_gather_kernel  W[f][q] = T_f(w_q) for every distinct field of the request: a reflector is a
//                       strided walk through a field (a column: one node per row), read once per
//                       field here instead of once per pair
//   skip_pair_kernel    one wavefront per pair: lane l takes nodes l, l + 64, ... in ascending order
//                       into its running minimum, then the 64 minima are combined over the lane
//                       distances 32 .. 1.  The key order is total (value, then node number), so
//                       the result is the same for every tree
//   skip_join_kernel    one workgroup per pair: the points of legs 2 p and 2 p + 1 of the ray
//                       kernel's buffers into the packed (x, z) buffer of kept rays
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "skip_pick.h"

namespace af {

constexpr int kSkipWaves = 4;  // pairs per workgroup of skip_pair_kernel

__global__ __launch_bounds__(256) void skip_gather_kernel(const double* const* fld, const int* w_iz, const int* w_ix,
                                                          int fnx, int nw, double* W) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nw) return;
  const int f = blockIdx.y;
  W[(int64_t)f * nw + q] = fld[f][skip_node_offset(w_iz[q], w_ix[q], fnx)];
}

__global__ __launch_bounds__(64 * kSkipWaves) void skip_pair_kernel(const double* W, const int* row_a, const int* row_b,
                                                                     int npairs, int nw, double* pick_time, int* hit) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * kSkipWaves + (threadIdx.x >> 6);
  if (pair >= npairs) return;  // whole wavefronts leave: the shuffles below see all 64 lanes
  const double* wa = W + (int64_t)row_a[pair] * nw;
  const double* wb = W + (int64_t)row_b[pair] * nw;
  SkipKey best = skip_key_none();
  for (int q = lane; q < nw; q += 64) best = skip_key_take(best, wa[q], wb[q], q);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    SkipKey o;
    o.v = __shfl_xor(best.v, d, 64);
    o.q = __shfl_xor(best.q, d, 64);
    best = skip_key_min(best, o);
  }
  if (lane == 0) {
    pick_time[pair] = best.v;
    hit[pair] = best.q;
  }
}

__global__ __launch_bounds__(256) void skip_join_kernel(const double* rx, const double* ry, const int* leg_len,
                                                        const long long* off, int max_pts, double* packed) {
  const int64_t pair = blockIdx.x;
  const int len_a = leg_len[2 * pair], len_b = leg_len[2 * pair + 1];
  const int n = skip_join_len(len_a, len_b);
  const int64_t o = off[pair];
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int64_t s = skip_join_src(pair, i, len_a, max_pts), d = skip_join_dst(o, i);
    packed[d] = rx[s];
    packed[d + 1] = ry[s];
  }
}

}  // namespace af

extern "C" hipError_t af_launch_skip_pick(const double* const* fld, int nfld, const int* w_iz, const int* w_ix, int fnx,
                                          int nw, double* W, const int* row_a, const int* row_b, int npairs,
                                          double* pick_time, int* hit, hipStream_t stream) {
  if (nfld <= 0 || nw <= 0 || npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(af::skip_gather_kernel, dim3((nw + 255) / 256, nfld), dim3(256), 0, stream, fld, w_iz, w_ix, fnx, nw,
                     W);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(af::skip_pair_kernel, dim3((npairs + af::kSkipWaves - 1) / af::kSkipWaves),
                     dim3(64 * af::kSkipWaves), 0, stream, W, row_a, row_b, npairs, nw, pick_time, hit);
  return hipGetLastError();
}

extern "C" hipError_t af_launch_skip_join(const double* rx, const double* ry, const int* leg_len, const long long* off,
                                          int npairs, int max_pts, double* packed, hipStream_t stream) {
  if (npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(af::skip_join_kernel, dim3(npairs), dim3(256), 0, stream, rx, ry, leg_len, off, max_pts, packed);
  return hipGetLastError();
}
