// utils.hip — batched evaluation of single device functions (module-level API of the drop-in
// Anis_TTF_rays.py and device-level parity tests):
//   update() / fouds18_A() on independent caller-supplied neighbourhoods (:904-1410, :240-901)
//   time_between_points() on the resident model (:2835-2989)
//   cr_math.h's atan / sin / cos / tan / sincos on caller-supplied arguments (global tables)
//
// local_ops_kernel's ops 3..6 are test entry points for the forms of the two local operators that
// the field kernels run (tests/test_gpu_local_ops.py holds every form to the oracle's bits):
//   3  update() on a register neighbourhood: NbFieldT::load of the NaN-coded patch, update_nb
//   4  the same selection spread over a wavefront: update_select_lanes, update_nb_select where it
//      returns false, update_nb_finish (as fmm_exact_lds.hip's relax_value and fmm_init.hip's relax role)
//   5  fouds18_A() on four lanes: fouds18_part<false> of parts 0..3, f18_min, fouds18_combine
//   6  the same with fouds18_part<true> on the resident model's material record and slownesses
//      (the band kernel's fallback rounds)
// The lane-local slot loaders of fmm_init.hip (lane_slot_lds) and fmm_exact_lds.hip
// (stencil_from_lds) are private to their kernels and are not reached from here.
#include "kernels.h"
#include "local_ops.h"
#include "fields.h"
#include "band_common.h"
#include "cr_eval.h"

namespace af {

struct PatchField {  // caller patch; rows past pz read as nsts=-1 / ttn=0 (padded semantics)
  const double* T;
  const int* S;
  int nz, nx;
  AF_DEV int st(long z, long x) const { return z >= nz ? -1 : S[z * nx + x]; }
  AF_DEV double tt(long z, long x) const { return z >= nz ? 0.0 : T[z * nx + x]; }
};

// value of NbField slot k
AF_DEV double nb_slot(const NbFieldT& nb, int k) {
  return k == 0 ? nb.t0 : k == 1 ? nb.t1 : k == 2 ? nb.t2 : k == 3 ? nb.t3 : k == 4 ? nb.t4 : k == 5 ? nb.t5
       : k == 6 ? nb.t6 : k == 7 ? nb.t7 : k == 8 ? nb.t8 : k == 9 ? nb.t9 : k == 10 ? nb.t10 : nb.t11;
}

// the material of case k: the caller's (ops 0, 1, 3..5) or resident-model cell (mz, mx)'s (ops 2, 6)
AF_DEV CellMat local_ops_mat(const LocalOpsParams& P, long k, DevModel& M, MatView& v) {
  if (P.op == 2 || P.op == 6) {
    v.s1z = v.s1x = v.s2 = 1;
    v.side1z = v.side1x = v.side2 = v.lo1z = v.lo1x = v.lo2z = v.lo2x = 0;
    v.quant = P.quant;
    M = P.RM;
    return band_mat<true>(P.RM, P.RM.mtab, P.RM.stab, v, P.mz[k], P.mx[k]);
  }
  M.mslo = nullptr;
  M.nz0 = 1;
  M.nx0 = 1;
  M.veln = P.cveln + k;
  M.velpn = P.cvelpn + k;
  M.vm = P.cvm + k;
  M.sidx = nullptr;
  M.stab = nullptr;
  M.gtab = P.tab;
  M.ptab = P.tab;
  M.ncol = P.ncol;
  CellMat cm;
  cm.veln = P.cveln[k];
  cm.vm = P.cvm[k];
  cm.velpn = P.cvelpn[k];
  cm.stif = P.cstif ? P.cstif + 5 * k : nullptr;
  return cm;
}

// blocks of one wavefront; a case takes one lane (ops 0..3), a wavefront (op 4) or four lanes (ops 5, 6)
__global__ void __launch_bounds__(64) local_ops_kernel(LocalOpsParams P) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x;
  const long k = P.op == 4 ? tid >> 6 : P.op >= 5 ? tid >> 2 : tid;
  if (k >= P.n) return;  // (the same for every lane of a case)
  const long pn = (long)P.pz * P.px;
  PatchField F{P.ttn + k * pn, P.nsts + k * pn, P.pz, P.px};
  DevModel M;
  MatView v;
  const CellMat cm = local_ops_mat(P, k, M, v);
  const int iz = P.iz[k], ix = P.ix[k];
  if (P.op == 2) {  // the band kernel's fallback: fouds18<true> on the material record + mslo
    P.out[k] = fouds18<true>(F, M, cm, iz, ix, P.dnx[k], P.dnz[k], P.nnx_arg[k], P.nnz_arg[k],
                             mat_slo(M, v, P.mz[k], P.mx[k]));
  } else if (P.op == 0) {
    P.out[k] = update(F, M, cm, iz, ix, P.dnx[k], P.nnz_arg[k], P.nnx_arg[k]);
  } else if (P.op == 1) {
    P.out[k] = fouds18(F, M, cm, iz, ix, P.dnx[k], P.dnz[k], P.nnx_arg[k], P.nnz_arg[k]);
  } else if (P.op == 3 || P.op == 4) {
    // ttn is NaN-coded as the HBM grids are (the host codes it): the production loader's clamped
    // reads and its validity, then update()'s bounds on top (update_nb_select's inb)
    const int nnz = P.nnz_arg[k], nnx = P.nnx_arg[k];
    NbFieldT nb;
    nb.load(F.T, P.pz, P.px, iz, ix);
    if (P.op == 3) {
      P.out[k] = update_nb(nb, M, cm, iz, ix, P.dnx[k], nnz, nnx);
    } else {  // every lane of the wavefront holds the case's neighbourhood; lane k < 12 gives slot k
      const double tk = lane < 12 ? nb_slot(nb, lane) : 0.0;
      const bool vk = lane < 12 && ((nb.vm >> lane) & 1u);
      UpdSel s2;
      const bool par = update_select_lanes(tk, vk, iz, ix, nnz, nnx, lane, s2);
      if (lane == 0) {
        if (!par) s2 = update_nb_select(nb, iz, ix, nnz, nnx);
        P.out[k] = update_nb_finish(M, cm, iz, ix, P.dnx[k], s2);
      }
    }
  } else {  // ops 5, 6: four lanes per case, one candidate of each stencil family per lane
    const int part = lane & 3;
    const double dnx = P.dnx[k], dnz = P.dnz[k];
    const long nnx = P.nnx_arg[k], nnz = P.nnz_arg[k];
    F18Part fp = P.op == 5 ? fouds18_part<false>(F, M, cm, iz, ix, dnx, dnz, nnx, nnz, nullptr, part)
                           : fouds18_part<true>(F, M, cm, iz, ix, dnx, dnz, nnx, nnz,
                                                mat_slo(M, v, P.mz[k], P.mx[k]), part);
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      F18Part ot;
#pragma unroll
      for (int q = 0; q < 4; q++) ot.m[q] = __shfl_xor(fp.m[q], o);
      fp = f18_min(fp, ot);
    }
    if (part == 0) P.out[k] = fouds18_combine(fp, F.tt(iz, ix));
  }
}

__global__ void tbp_kernel(DevModel M, int n, const double* x1, const double* x2, const double* y1, const double* y2,
                           double dnx, int sg, double* out) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  out[k] = tbp(M, x1[k], x2[k], y1[k], y2[k], dnx, sg);
}

// fouds18_A()'s four stencil-family slownesses of every distinct material, for both MatView
// quantisations (sg = 1: as is; sg > 1: finer_grid_n's int32 orientation / float32 vel_map), with
// the CellMat band_mat() builds -> DevModel::mslo [nmat][2][4]
__global__ void mat_slowness_kernel(DevModel M, double* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= 2 * M.nmat) return;
  const MatRec m = M.mtab[k >> 1];
  const bool quant = k & 1;
  CellMat c;
  c.velpn = m.velpn;
  c.veln = quant ? (double)(int)m.veln : m.veln;
  c.vm = quant ? (double)(float)m.vm : m.vm;
  c.stif = m.sidx >= 0 ? M.stab + 5 * m.sidx : nullptr;
  for (int q = 0; q < 4; q++) out[4 * k + q] = fouds18_slowness(M, c, q);
}

}  // namespace af

extern "C" hipError_t af_launch_local_ops(const af::LocalOpsParams* P, hipStream_t stream) {
  if (P->n <= 0) return hipSuccess;
  const long lanes = P->op == 4 ? 64 : P->op >= 5 ? 4 : 1;  // per case
  const long blocks = (P->n * lanes + 63) / 64;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(af::local_ops_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, *P);
  return hipGetLastError();
}

extern "C" hipError_t af_launch_tbp(const af::DevModel* M, int n, const double* x1, const double* x2, const double* y1,
                                    const double* y2, double dnx, int sg, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(af::tbp_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, *M, n, x1, x2, y1, y2, dnx, sg, out);
  return hipGetLastError();
}

extern "C" hipError_t af_launch_mat_slowness(const af::DevModel* M, double* out, hipStream_t stream) {
  if (M->nmat <= 0) return hipSuccess;
  hipLaunchKernelGGL(af::mat_slowness_kernel, dim3((2 * M->nmat + 63) / 64), dim3(64), 0, stream, *M, out);
  return hipGetLastError();
}

namespace af {
// cr_math.h's functions as the operators call them (AF_ATAN ...), one argument per thread, with the
// tables as this unit reads them: the global constants (cr_eval.hip: the same from LDS)
__global__ void __launch_bounds__(kCrEvalThreads) cr_eval_kernel(int fn, long long n, const double* x, double* out,
                                                                 double* out2) {
  const long long k = (long long)blockIdx.x * kCrEvalThreads + threadIdx.x;
  if (k >= n) return;
  cr_eval_one(fn, x[k], out + k, out2 ? out2 + k : nullptr);
}
}  // namespace af

extern "C" hipError_t af_launch_cr_eval(int fn, long long n, const double* x, double* out, double* out2,
                                        hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const unsigned blocks = af::cr_eval_blocks(n);
  if (!blocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(af::cr_eval_kernel, dim3(blocks), dim3(af::kCrEvalThreads), 0, stream, fn, n, x, out, out2);
  return hipGetLastError();
}

namespace af {
// final scaling of travel_finer_grid (:2832 ttn / subgrid_size)
__global__ void scale_kernel(double* T, long n, double inv) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) T[i] = T[i] / inv;
}
}  // namespace af

extern "C" hipError_t af_launch_scale(double* T, long n, double sg, hipStream_t stream) {
  hipLaunchKernelGGL(af::scale_kernel, dim3(2048), dim3(256), 0, stream, T, n, sg);
  return hipGetLastError();
}
