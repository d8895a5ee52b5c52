// trace_fir_term.h — the per-output sum of the trace FIR P and of its transpose Pᵀ (include/alifmm.h
// alifmm_trace_fir, alifmm_tfm_lsq_pulse), and the index mappings of the tiled walk that makes it.
// Shared verbatim by the kernel (trace_fir.hip) and by a stand-alone host program
// (tests/trace_fir_sim.cpp, built with ASan and UBSan) that walks the same tiles.  Includes nothing
// from HIP; build with -ffp-contract=off (the contract fixes the operation order).
//
// Layout.  Data [ntrace][nt][NC] float64, NC 1 (real) or 2 (re, im interleaved).  Taps h[ntap][TC]
// float64: TC 1 real taps, applied to each component; TC 2 complex taps (NC 2 only).  origin is the
// tap index of the pulse's time zero, 0 <= origin < ntap.
//
// Definition (everything float64, no contraction, operations in the order written):
//   forward    y[t] = sum over j = 0 .. ntap - 1, ascending, of h[j] * x[t - j + origin]
//   transpose  z[t] = sum over j ascending of conj(h[j]) * y[t + j - origin]
// The accumulator starts at +0.0 per component.  A sample index outside 0 .. nt - 1 adds nothing;
// taps being finite and the accumulator never -0, adding h * 0 from a zero-padded segment gives the
// same bits, which is what the tiled walk does.
//   real tap     acc_c += h * x_c                                   (one multiply, one add)
//   complex tap  pr = (hr * xr) - (hi * xi); pi = (hr * xi) + (hi * xr); acc_r += pr; acc_i += pi
//                (transpose: hi negated first; negation is exact)
// Consequences: the outputs are bit-reproducible; a trace's result does not depend on the other
// traces, on the tile an output falls in or on the launch; <P x, y> = <x, Pᵀ y> to rounding under
// the real inner product (each product h[j] x[s] y[t] appears on both sides, rounded differently).
//
// The tiled walk.  A tile is `tile` consecutive outputs t0 .. t0 + tile - 1 of one trace; it reads
// the segment of seg = tile + ntap - 1 samples around them.  Both directions run ONE loop,
//   out'[u] = sum over j ascending of g[j] * s[u + j],   u = 0 .. tile - 1,
// over a staged segment s and staged taps g: the transpose stages the samples ascending from
// t0 - origin, g = conj(h), and out'[u] is z[t0 + u]; the forward sum stages them descending from
// t0 + tile - 1 + origin and out'[u] is y[t0 + tile - 1 - u] (the index mapping mirrored), g = h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_FIR_HD __host__ __device__ inline
#else
#define AF_FIR_HD inline
#endif

namespace af {

constexpr int kFirMaxTaps = 1024;  // ALIFMM_FIR_MAX_TAPS
constexpr int kFirOutPerThread = 4;  // consecutive outputs of a thread: the width of its sliding window

// samples of a tile's segment
AF_FIR_HD int trace_fir_seg(int tile, int ntap) { return tile + ntap - 1; }

// the sample index (may lie outside 0 .. nt - 1: a zero) staged at position i of the segment of
// the tile at t0
AF_FIR_HD int64_t trace_fir_src(int transpose, int64_t t0, int tile, int origin, int i) {
  return transpose ? t0 - origin + i : t0 + (tile - 1) + origin - i;
}

// the output sample that out'[u] of the tile at t0 is
AF_FIR_HD int64_t trace_fir_dst(int transpose, int64_t t0, int tile, int u) { return transpose ? t0 + u : t0 + (tile - 1) - u; }

// Where position i of a segment lies in its staging buffer of 4 * quarter samples, quarter =
// trace_fir_quarter(seg): a thread's window walks positions 4 * thread + k, so position i goes to
// row i mod 4, column i / 4, and the threads of a wave read consecutive columns of one row.
AF_FIR_HD int trace_fir_quarter(int seg) { return (seg + kFirOutPerThread - 1) / kFirOutPerThread; }
AF_FIR_HD int trace_fir_slot(int i, int quarter) { return (i % kFirOutPerThread) * quarter + i / kFirOutPerThread; }

// one tap of one output: acc[NC] += g * x, g = (gr, gi) a staged tap (gi unused when TC is 1)
template <int NC, int TC>
AF_FIR_HD void trace_fir_tap(double* acc, double gr, double gi, const double* x) {
  if (TC == 1) {
    for (int c = 0; c < NC; c++) acc[c] = acc[c] + gr * x[c];
  } else {
    const double pr = (gr * x[0]) - (gi * x[1]);
    const double pi = (gr * x[1]) + (gi * x[0]);
    acc[0] = acc[0] + pr;
    acc[1] = acc[1] + pi;
  }
}

// the staged tap g[j] from h[j]: the transpose conjugates
template <int TC>
AF_FIR_HD void trace_fir_stage_tap(const double* h, int j, int transpose, double* g) {
  g[0] = h[(int64_t)j * TC];
  if (TC == 2) g[1] = transpose ? -h[(int64_t)j * TC + 1] : h[(int64_t)j * TC + 1];
}

// position i (0 .. seg - 1) of the segment of the tile at t0 of the trace x[nt][NC], into the staging
// buffer s: the sample, or zeros outside the trace
template <int NC>
AF_FIR_HD void trace_fir_stage(const double* x, int nt, int transpose, int64_t t0, int tile, int origin, int i,
                               int quarter, double* s) {
  const int64_t src = trace_fir_src(transpose, t0, tile, origin, i);
  const bool in = src >= 0 && src < nt;
  double* d = s + (int64_t)trace_fir_slot(i, quarter) * NC;
  for (int c = 0; c < NC; c++) d[c] = in ? x[src * NC + c] : 0.0;
}

// out'[u] = acc of the tile at t0 into the trace y[nt][NC], where it lies inside the trace
template <int NC>
AF_FIR_HD void trace_fir_store(double* y, int nt, int transpose, int64_t t0, int tile, int u, const double* acc) {
  const int64_t dst = trace_fir_dst(transpose, t0, tile, u);
  if (dst < 0 || dst >= nt) return;
  for (int c = 0; c < NC; c++) y[dst * NC + c] = acc[c];
}

// one sample (NC doubles at p, 8 NC-byte aligned) in one read
template <int NC>
AF_FIR_HD void trace_fir_read(const double* p, double* v) {
  const double* q = (const double*)__builtin_assume_aligned(p, 8 * NC);
  for (int c = 0; c < NC; c++) v[c] = q[c];
}

// out'[4 thread + r], r = 0 .. 3, of a tile from its staging buffer s (trace_fir_slot, 16-byte
// aligned) and its staged taps g[ntap][TC]: one accumulator per output, taps ascending.  Position
// 4 thread + k of the segment is in win[k mod 4] while an output needs it, so a tap reads one new
// sample: position 4 thread + j + 3, row (j + 3) mod 4, column thread + (j + 3) / 4.
template <int NC, int TC>
AF_FIR_HD void trace_fir_thread(const double* s, int quarter, const double* g, int ntap, int thread,
                                double (*acc)[NC]) {
  static_assert(kFirOutPerThread == 4, "the window's rotation is written for four outputs");
  double win[4][NC];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < NC; c++) acc[r][c] = 0.0;
  for (int k = 0; k < 3; k++) trace_fir_read<NC>(s + (int64_t)(k * quarter + thread) * NC, win[k]);
  for (int j = 0; j < ntap; j += 4) {
#pragma unroll
    for (int sh = 0; sh < 4; sh++) {
      if (j + sh < ntap) {
        trace_fir_read<NC>(s + (int64_t)(((sh + 3) & 3) * quarter + thread + (j >> 2) + ((sh + 3) >> 2)) * NC,
                           win[(sh + 3) & 3]);
        double gt[2] = {0.0, 0.0};
        trace_fir_read<TC>(g + (int64_t)(j + sh) * TC, gt);
        for (int r = 0; r < 4; r++) trace_fir_tap<NC, TC>(acc[r], gt[0], gt[1], win[(r + sh) & 3]);
      }
    }
  }
}

}  // namespace af
