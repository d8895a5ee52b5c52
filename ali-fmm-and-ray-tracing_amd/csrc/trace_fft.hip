// trace_fft.hip — the spectral trace filter y = IDFT(G · DFT(x)) on the device (include/alifmm.h
// alifmm_trace_spectral).  The arithmetic, the register passes, their index maps and the padded LDS
// layout are trace_fft_term.h's, shared with tests/trace_fft_sim.cpp.
//
// One workgroup of kFftBlock threads per batch of fft_pack(N) traces (one trace from N = 2048 on,
// 2048 / N shorter ones, at most one per thread); the batches are walked with the grid's stride and
// every trace offset is 64-bit.  A batch runs the 2 npass - 1 steps of fft_step with a barrier
// between two steps: a thread takes work items (trace of the batch, group of 2^L elements) with the
// block's stride, runs the step's L <= 3 layers in registers and puts the group back.  The first
// step reads the caller's samples and the last one writes the scaled output, both coalesced (the
// lanes' groups are consecutive, element j of a group lies j hl further on); the step in the middle
// is the last forward pass, the pointwise step and the first inverse pass on one register group.
// In between the traces live in dynamic LDS as complex float64 at fft_slot (one element of padding
// per 8): 72 KiB at N = 4096, 144 KiB at 8192.  Twiddles come from the 16 KiB sine table through
// the cache; the response, permuted to element order by the host, is read once per element.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fft_twiddles.h"
#include "kernels.h"

namespace af {

constexpr int kFftMaxBlocks = 1024;  // workgroups of a launch ("trace_fft_grid"): 4 per CU, each walking its share
static_assert((size_t)(kFftMax + kFftMax / 8) * sizeof(FftC) <= 160 * 1024, "a trace at the cap fits a CU's LDS");
static_assert(sizeof(FftC) == 16, "one ds_read_b128 per element");

template <typename T, int NC>
__global__ __launch_bounds__(kFftBlock) void trace_fft_kernel(TraceFftParams P) {
  extern __shared__ __align__(16) unsigned char fft_lds_raw[];
  FftC* lds = reinterpret_cast<FftC*>(fft_lds_raw);
  const FftShape S = P.S;
  const int pack = fft_pack(S.n), nsteps = fft_nsteps(S.logn);
  const int64_t nbatch = (P.ntrace + pack - 1) / pack;
  const T* in = static_cast<const T*>(P.in);
  T* out = static_cast<T*>(P.out);
  for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
    for (int step = 0; step < nsteps; step++) {
      int l0, L, flags;
      fft_step(S.logn, step, &l0, &L, &flags);
      __syncthreads();  // the step before, or the batch before, is through with the LDS image
      const int items = pack << (S.logn - L);
      for (int w = threadIdx.x; w < items; w += kFftBlock)
        fft_item<T, NC>(S, l0, L, flags, b * pack, P.ntrace, w, in, out, lds, P.hrev, kFftQuarterSin);
    }
  }
}

template <typename T, int NC>
static hipError_t launch(const TraceFftParams& P, hipStream_t stream) {
  const size_t lds = (size_t)fft_lds_total(P.S.n) * sizeof(FftC);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)trace_fft_kernel<T, NC>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int pack = fft_pack(P.S.n);
  const int64_t nbatch = (P.ntrace + pack - 1) / pack;
  const dim3 grid((unsigned)std::min<int64_t>(nbatch, kFftMaxBlocks));
  hipLaunchKernelGGL((trace_fft_kernel<T, NC>), grid, dim3(kFftBlock), lds, stream, P);
  return hipGetLastError();
}

}  // namespace af

using namespace af;

extern "C" int af_trace_fft_grid() { return kFftMaxBlocks; }

extern "C" hipError_t af_launch_trace_fft(const TraceFftParams* P, int ncomp, int dtype, hipStream_t stream) {
  const FftShape& S = P->S;
  if (P->ntrace < 1 || S.nt < 1 || S.n < S.nt || S.n > kFftMax || (S.n & (S.n - 1)) || S.logn != fft_log2(S.n) ||
      S.inv_n != 1.0 / S.n || !(ncomp == 1 || ncomp == 2) || !(dtype == 0 || dtype == 1) || S.resp_comp < 0 ||
      S.resp_comp > 2 || (S.resp_comp > 0) != (P->hrev != nullptr) || !(S.analytic == 0 || S.analytic == 1) || !P->in ||
      !P->out || P->in == P->out)
    return hipErrorInvalidValue;
  if (dtype == 0) return ncomp == 1 ? launch<double, 1>(*P, stream) : launch<double, 2>(*P, stream);
  return ncomp == 1 ? launch<float, 1>(*P, stream) : launch<float, 2>(*P, stream);
}
