// fmm_seed.hip — hand-over to the band kernel (fmm_band_k.hip mode 0) from a set of seed nodes with
// given times (alifmm_travel_seeded): the seeds known (cls 1) with their times exactly as given,
// every in-grid non-seed 4-neighbour of a seed close (cls 3) with the value of one band step's
// evaluation against the seeds-only state: update(), on -1 the fouds18_A() fallback, with the
// material path of the band kernel's evaluate phase (band_mat<true>, fouds18<true> on mat_slo where
// the model has its material table, the model arrays otherwise: the same values).
//
// The node list is shared by every field of a call, so the host builds the geometry once: the
// close cells in ascending cell index, and per close cell the 5 x 5 window (the operators' reach)
// of indices into the seed list, -1 where the position is no seed or outside the grid.  A lane
// stages its window's times in LDS and both operators answer from it: no scratch grid, no scatter,
// no atomics; one lane per hand-over entry.
#include "kernels.h"
#include "local_ops.h"
#include "fields.h"
#include "band_common.h"

namespace af {

constexpr int kSeedThreads = 128;

struct SeedParams {
  DevModel M;
  int nz, nx;
  double dnx, dnz;
  int nfield, nseed, nclose;
  const int* seed_cell;        // [nseed] iz * nx + ix, list order
  const int* close_cell;       // [nclose] ascending
  const int* win;              // [nclose][25] seed index at (dz + 2) * 5 + (dx + 2), or -1
  const double* seed_t;        // [nfield][nseed] times, or null
  const double* const* from;   // [nfield] resident fields (row-major nz x nx) the times are read from, or null
  HandoverOut* out;            // [nfield]; err zeroed by the host before the launch
};

// the 5 x 5 window of one close cell: times (0 where no seed: the reference's ttn of a never-relaxed
// node) and the seeds as a bit mask; "known" and "valid" coincide in the seeds-only state
struct SeedWin {
  const double* t;
  unsigned known;
  int iz, ix;
  AF_DEV int st(long z, long x) const {
    const long dz = z - iz + 2, dx = x - ix + 2;
    if (dz < 0 || dz > 4 || dx < 0 || dx > 4) return -1;
    return (known >> (dz * 5 + dx)) & 1u ? (int)kKnown : -1;
  }
  AF_DEV double tt(long z, long x) const {
    const long dz = z - iz + 2, dx = x - ix + 2;
    if (dz < 0 || dz > 4 || dx < 0 || dx > 4) return 0.0;
    return t[dz * 5 + dx];
  }
};

AF_DEV bool seed_time_ok(double t) { return t == t && t < INFINITY && !signbit(t); }

template <bool MATTAB>
__global__ __launch_bounds__(kSeedThreads) void fmm_seed_kernel(SeedParams P) {
  __shared__ double wins[kSeedThreads * 25];
  const int f = blockIdx.y;
  const int e = blockIdx.x * kSeedThreads + threadIdx.x;
  HandoverOut* O = P.out + f;
  const double* fld = P.from ? P.from[f] : nullptr;
  const double* tl = P.seed_t ? P.seed_t + (long)f * P.nseed : nullptr;
  auto seed_time = [&](int k) { return fld ? gld(fld + gld(P.seed_cell + k)) : gld(tl + k); };
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) O->n = P.nseed + P.nclose;
    if (threadIdx.x < 16) O->prof[threadIdx.x] = 0;
  }
  if (e >= P.nseed + P.nclose) return;
  if (e < P.nseed) {
    const double t = seed_time(e);
    if (!seed_time_ok(t)) O->err = 1;  // (every lane that writes, writes 1)
    O->cell[e] = gld(P.seed_cell + e);
    O->ttn[e] = t;
    O->cls[e] = 1;
    return;
  }
  const int j = e - P.nseed;
  const int c = gld(P.close_cell + j);
  const int z = c / P.nx, x = c - z * P.nx;
  double* const w = wins + threadIdx.x * 25;
  unsigned known = 0;
  for (int o = 0; o < 25; o++) {
    const int k = gld(P.win + (long)j * 25 + o);
    double t = 0.0;
    if (k >= 0) {
      t = seed_time(k);
      known |= 1u << o;
    }
    w[o] = t;
  }
  // update() on the register neighbourhood the band kernel evaluates (fmm_band_k.hip load_tb)
  const int dz[12] = {0, 0, 0, 0, -2, -1, 1, 2, -1, -1, 1, 1};
  const int dx[12] = {-2, -1, 1, 2, 0, 0, 0, 0, -1, 1, -1, 1};
  NbFieldT nb;
  nb.iz = z;
  nb.ix = x;
  double t[12];
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const int o = (dz[k] + 2) * 5 + dx[k] + 2;
    t[k] = w[o];
    if ((known >> o) & 1u) m |= 1u << k;
  }
  nb.vm = m;
  nb.t0 = t[0]; nb.t1 = t[1]; nb.t2 = t[2]; nb.t3 = t[3]; nb.t4 = t[4]; nb.t5 = t[5];
  nb.t6 = t[6]; nb.t7 = t[7]; nb.t8 = t[8]; nb.t9 = t[9]; nb.t10 = t[10]; nb.t11 = t[11];
  MatView mv;  // the main grid is the model grid (subgrid 1): the identity view, no quantisation
  mv.s1z = mv.s1x = mv.s2 = 1;
  mv.side1z = mv.side1x = mv.side2 = mv.lo1z = mv.lo1x = mv.lo2z = mv.lo2x = 0;
  mv.quant = 0;
  const CellMat cm = MATTAB ? band_mat<true, true>(P.M, P.M.mtab, P.M.stab, mv, z, x) : cell_mat(P.M, mv, z, x);
  double v = update(nb, P.M, cm, z, x, P.dnx, P.nz, P.nx);
  if (v == -1.0) {
    const SeedWin F{w, known, z, x};
    v = fouds18<MATTAB>(F, P.M, cm, z, x, P.dnx, P.dnz, P.nx, P.nz, MATTAB ? mat_slo(P.M, mv, z, x) : nullptr);
  }
  O->cell[e] = c;
  O->ttn[e] = v;
  O->cls[e] = 3;
}

}  // namespace af

extern "C" hipError_t af_launch_seed(const af::DevModel* M, int nz, int nx, double dnx, double dnz, int nfield, int nseed,
                                     int nclose, const int* seed_cell, const int* close_cell, const int* win,
                                     const double* seed_t, const double* const* from, af::HandoverOut* out,
                                     hipStream_t stream) {
  af::SeedParams P;
  P.M = *M;
  P.nz = nz;
  P.nx = nx;
  P.dnx = dnx;
  P.dnz = dnz;
  P.nfield = nfield;
  P.nseed = nseed;
  P.nclose = nclose;
  P.seed_cell = seed_cell;
  P.close_cell = close_cell;
  P.win = win;
  P.seed_t = seed_t;
  P.from = from;
  P.out = out;
  const dim3 g((nseed + nclose + af::kSeedThreads - 1) / af::kSeedThreads, nfield), b(af::kSeedThreads);
  if (M->mid && M->mslo && M->mtab) hipLaunchKernelGGL(af::fmm_seed_kernel<true>, g, b, 0, stream, P);
  else hipLaunchKernelGGL(af::fmm_seed_kernel<false>, g, b, 0, stream, P);
  return hipGetLastError();
}
