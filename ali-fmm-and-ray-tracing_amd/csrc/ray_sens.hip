// ray_sens.hip — travel-time sensitivities along traced rays (include/alifmm.h alifmm_ray_sens).
//
// time_between_points() (Anis_TTF_rays.py:2835-2989) sums len * slowness over the pieces of a
// segment and throws the pieces away; these kernels keep them: per piece the coarse cell, the
// length, the time and the time's derivative in the cell's orientation (Fermat: the path is fixed
// to first order), as CSR rows and / or summed into three maps on the coarse grid.
// One wavefront per ray, kSensWaves per workgroup; the lanes take 64 consecutive segments at a
// time.  Count pass (sens_count_kernel): geometry only; validates every segment (sens_walk.h
// sens_count: finite coordinates, cells inside the grid, the piece bound) and leaves the ray's
// entry count and status; the host turns the counts into row offsets.  Fill pass
// (sens_fill_kernel): a wave prefix sum of the lanes' piece counts gives each lane its rows; the
// lane walks its segment, evaluates the slowness and its centred difference once per run of equal
// material id (as tbp() reuses slown), writes the rows and adds the pieces of a run in one cell
// together before its three float64 atomic adds.  Material records, stiffness rows, group table
// and the CR trig tables are staged in LDS as in find_ray_kernel (LDSMAT; false for models past the
// LDS tables).  The walk and the entry arithmetic are sens_walk.h's, shared with tests/sens_sim.cpp.
#define CR_LDS_TABLES  // cr_math.h tables in LDS (crm::lds_init at kernel start)
#include <type_traits>

#include "kernels.h"
#include "sens_walk.h"

namespace af {

constexpr int kSensWaves = 4;
constexpr int kSensMatLds = 256, kSensStabLds = 64, kSensGtabLds = 722;  // rays.hip's LDS tables

__global__ __launch_bounds__(64 * kSensWaves) void sens_count_kernel(SensParams P) {
  const int wl = threadIdx.x & 63;
  const long rl = (long)blockIdx.x * kSensWaves + (threadIdx.x >> 6);
  if (rl >= P.nrays) return;  // (uniform per wavefront)
  const long ray = P.ray0 + rl;
  const int n = gld(P.len + ray);
  const int fl = P.flags ? gld(P.flags + ray) : 0;
  long long total = 0;
  int bad = 0;
  if (n >= 2 && !(fl & 6)) {
    const double* p = P.xy + 2 * (gld(P.off + ray) - P.pt0);
    for (long s0 = 0; s0 < n - 1; s0 += 64) {
      const long s = s0 + wl;
      if (s < n - 1) {
        const int c = sens_count(gld(p + 2 * s), gld(p + 2 * s + 2), gld(p + 2 * s + 1), gld(p + 2 * s + 3), P.sg,
                                 P.M.nz0, P.M.nx0);
        if (c < 0) bad = 1;
        else total += c;
      }
      if (__any(bad)) break;
    }
    for (int o = 32; o > 0; o >>= 1) {
      total += __shfl_xor(total, o);
      bad |= __shfl_xor(bad, o);
    }
  }
  if (wl == 0) {
    P.cnt[ray] = bad ? 0 : total;
    P.status[ray] = bad;
  }
}

struct SensSlow {
  double s, ds;
};
// one copy of the three group-velocity evaluations in the kernel (as rays.hip ray_slowness)
__attribute__((noinline)) AF_DEV SensSlow sens_slowness_dev(double veln, double vm, int velpn, const double* stif,
                                                            double angle, const double* gtab, int ncol) {
  const bool christoffel = !(velpn != 0 || stif == nullptr);  // group_vel_cell's selector
  SensSlow r;
  sens_slowness(
      veln, angle, christoffel,
      [&](double eff) { return christoffel ? christoffel_group(stif, eff, vm) : table_vel(gtab, ncol, eff, velpn, vm); },
      r.s, r.ds);
  return r;
}

template <bool LDSMAT>
__global__ __launch_bounds__(64 * kSensWaves) void sens_fill_kernel(SensParams P) {
  __shared__ MatRec smat[LDSMAT ? kSensMatLds : 1];
  __shared__ double sstab[LDSMAT ? 5 * kSensStabLds : 1];
  __shared__ double sgtab[LDSMAT ? kSensGtabLds : 1];
  crm::lds_init();
  if (LDSMAT) {
    for (int k = threadIdx.x; k < P.M.nmat; k += blockDim.x) smat[k] = P.M.mtab[k];
    for (int k = threadIdx.x; k < 5 * P.M.nstab; k += blockDim.x) sstab[k] = P.M.stab[k];
    for (int k = threadIdx.x; k < 361 * P.M.ncol; k += blockDim.x) sgtab[k] = P.M.gtab[k];
  }
  __syncthreads();
  const std::conditional_t<LDSMAT, MatLds, MatGlobal> ms = [&] {
    if constexpr (LDSMAT) return MatLds{P.M, smat, sstab, sgtab};
    else return MatGlobal{P.M};
  }();
  const int wl = threadIdx.x & 63;
  const long rl = (long)blockIdx.x * kSensWaves + (threadIdx.x >> 6);
  if (rl >= P.nrays) return;  // (uniform per wavefront; no barrier follows)
  const long ray = P.ray0 + rl;
  if (gld(P.cnt + ray) == 0) return;  // skipped, invalid or without pieces
  const int n = gld(P.len + ray);
  const double* p = P.xy + 2 * (gld(P.off + ray) - P.pt0);
  const double wgt = P.w ? gld(P.w + ray) : 1.0;
  const bool maps = P.maps && wgt != 0.0;
  const bool rows = P.row != nullptr;
  const int nz0 = P.M.nz0, nx0 = P.M.nx0;
  const long ncell = (long)nz0 * nx0;
  long long base = rows ? gld(P.row + ray) : 0;
  for (long s0 = 0; s0 < n - 1; s0 += 64) {
    const long s = s0 + wl;
    const bool ok = s < n - 1;
    double x1 = 0, x2 = 0, y1 = 0, y2 = 0;
    int c = 0;
    if (ok) {
      x1 = gld(p + 2 * s), y1 = gld(p + 2 * s + 1), x2 = gld(p + 2 * s + 2), y2 = gld(p + 2 * s + 3);
      c = sens_count(x1, x2, y1, y2, P.sg, nz0, nx0);
      if (c < 0) c = 0;  // (the count pass accepted every segment of the ray)
    }
    // the lane's first row: the ray's rows so far + the pieces of the lanes before it
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (wl >= o) inc += t;
    }
    long long e = base + (inc - c);
    base += __shfl(inc, 63);
    if (c == 0) continue;
    SensWalk W;
    W.start(x1, x2, y1, y2, P.sg);
    int last_id = -1, acc_col = -1;
    SensSlow sl{0.0, 0.0};
    double a_len = 0.0, a_time = 0.0, a_dth = 0.0;
    auto flush = [&]() {
      if (acc_col < 0) return;
      unsafeAtomicAdd(P.maps + acc_col, a_len);
      unsafeAtomicAdd(P.maps + ncell + acc_col, a_time);
      unsafeAtomicAdd(P.maps + 2 * ncell + acc_col, a_dth);
    };
    for (int j = 0; j < c && W.more(); j++, e++) {
      int y_pos, x_pos;
      double len;
      if (!W.next(nz0, nx0, P.dnx, y_pos, x_pos, len)) break;
      const int id = ms.id(y_pos, x_pos);
      if (id < 0 || id != last_id) {
        const CellMat cm = ms.cm(id, y_pos, x_pos);
        sl = sens_slowness_dev(cm.veln, cm.vm, cm.velpn, cm.stif, W.angle, ms.gtab(), P.M.ncol);
        last_id = id;
      }
      const int col = y_pos * nx0 + x_pos;
      const double time = len * sl.s, dth = len * sl.ds;
      if (rows) {
        if (P.col) gst(P.col + e, col);
        if (P.elen) gst(P.elen + e, len);
        if (P.etime) gst(P.etime + e, time);
        if (P.edth) gst(P.edth + e, dth);
      }
      if (maps) {
        if (col != acc_col) {
          flush();
          acc_col = col;
          a_len = wgt * len;
          a_time = wgt * time;
          a_dth = wgt * dth;
        } else {
          a_len += wgt * len;
          a_time += wgt * time;
          a_dth += wgt * dth;
        }
      }
    }
    if (maps) flush();
  }
}

}  // namespace af

static dim3 sens_grid(int nrays) { return dim3((nrays + af::kSensWaves - 1) / af::kSensWaves); }

extern "C" hipError_t af_launch_sens_count(const af::SensParams* P, hipStream_t stream) {
  if (P->nrays <= 0) return hipSuccess;
  hipLaunchKernelGGL(af::sens_count_kernel, sens_grid(P->nrays), dim3(64 * af::kSensWaves), 0, stream, *P);
  return hipGetLastError();
}

extern "C" hipError_t af_launch_sens_fill(const af::SensParams* P, hipStream_t stream) {
  if (P->nrays <= 0) return hipSuccess;
  // the LDS tables when they fit, as af_launch_rays
  const bool lds = P->M.mid && P->M.mtab && P->M.nmat <= af::kSensMatLds && P->M.nstab <= af::kSensStabLds &&
                   361 * P->M.ncol <= af::kSensGtabLds;
  const dim3 grid = sens_grid(P->nrays), block(64 * af::kSensWaves);
  if (lds) hipLaunchKernelGGL((af::sens_fill_kernel<true>), grid, block, 0, stream, *P);
  else hipLaunchKernelGGL((af::sens_fill_kernel<false>), grid, block, 0, stream, *P);
  return hipGetLastError();
}
