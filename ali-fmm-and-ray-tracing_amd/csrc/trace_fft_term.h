// trace_fft_term.h — the arithmetic and the index maps of the spectral trace filter
// y = IDFT(G · DFT(x)) (include/alifmm.h alifmm_trace_spectral): the loads and their conversion, the
// radix-2 butterflies, the pointwise step, the scaled store, the layout of a trace in LDS and the
// schedule of register passes.  Shared verbatim by the kernel (trace_fft.hip) and by a stand-alone
// host program (tests/trace_fft_sim.cpp, built with ASan and UBSan) that replays the same passes.
// Includes nothing from HIP; build with -ffp-contract=off (the contract fixes the operation order).
//
// The contract (N = nfft = 2^logn, everything float64, no contraction, operations as written):
//   load      v[n] = (x[n], +0.0) or (re, im) for n < nt, (+0.0, +0.0) for nt <= n < N; a float32
//             sample converts exactly
//   twiddle   W_N^m = (c_m, -s_m), 0 <= m < N / 2, c_m = cos(2 pi m / N) and s_m = sin(2 pi m / N)
//             of the exact argument rounded once, read from the table of N = 8192 at m (8192 / N)
//   product   (a · w) = ((ar * wr) - (ai * wi), (ar * wi) + (ai * wr)): four rounded products, then
//             the subtraction and the addition
//   forward   decimation in frequency, in place: for l = 0 .. logn - 1, half = N >> (l + 1), every
//             block of 2 half elements and i < half: a = v[p], b = v[p + half], v[p] = a + b,
//             d = a - b, v[p + half] = d · W_N^(i << l).  X_k lies at v[bitrev(k)].
//   pointwise at v[bitrev(k)]: v = v · H_k for a complex response (the product above, w = H_k),
//             v = (vr * H_k, vi * H_k) for a real one; then, if analytic: v = (vr * 2, vi * 2) for
//             0 < k < N / 2, v = (+0.0, +0.0) for k > N / 2, v unchanged for k = 0 and k = N / 2
//   inverse   decimation in time from bit-reversed to natural order: for l = logn - 1 .. 0, the same
//             pairs: a = v[p], b = v[p + half] · conj(W_N^(i << l)), v[p] = a + b, v[p + half] = a - b
//   store     y[n] = (vr * (1 / N), vi * (1 / N)) for n < nt, rounded once to float32 for dtype 1
// Every butterfly multiplies by its twiddle, W^0 = (1, -0) included: no layer and no element is
// special, here, in the numpy restatement (tests/trace_fft_ref.py) and in the host program.
//
// Register passes.  A pass covers L <= 3 consecutive layers l0 .. l0 + L - 1.  These layers close
// over groups of 2^L elements q + j hl, j < 2^L, hl = N >> (l0 + L), q = (block << (logn - l0)) + i,
// i < hl: a work item loads one group, runs its L layers in registers and stores it.  The first
// pass takes the remainder (fft_first_len), the others 3 layers; the forward sweep runs the passes
// in order, the inverse sweep the same passes in reverse, so the last forward pass, the pointwise
// step and the first inverse pass share one group in registers (hl = 1 there: a group's elements
// are consecutive and element idx is bin bitrev(idx), whose class for the analytic mask shows in
// idx itself: k = 0 is idx 0, k = N / 2 is idx 1, k > N / 2 an odd idx, 0 < k < N / 2 an even one).
// The first forward pass reads the caller's trace and the last inverse pass writes the output, so
// a transform of up to 8 points never touches LDS.  An element sees exactly the contract's
// operations in the contract's order: the passes only decide where it waits in between.
//
// LDS.  A trace is N complex float64 (16 bytes) at slot fft_slot(idx) = idx + (idx >> 3): one
// element of padding per 8, so the power-of-two strides of the passes (8 hl elements between the
// lanes' groups when hl < 64) spread over the 64 banks of ds_read_b128 instead of meeting in a few.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_FFT_HD __host__ __device__ inline
#else
#define AF_FFT_HD inline
#endif

namespace af {

constexpr int kFftMax = 8192;   // ALIFMM_FFT_MAX
constexpr int kFftMaxLog = 13;
constexpr int kFftBlock = 512;  // threads of a workgroup (measured: 256 is 19% slower at N = 4096, 31% at 8192)
// what a pass does around its layers
enum { kFftFromGlobal = 1, kFftDif = 2, kFftPoint = 4, kFftDit = 8, kFftToGlobal = 16 };

struct alignas(16) FftC {
  double re, im;
};

// one call's shape: N = 1 << logn, the response's components (0: none) and the mask
struct FftShape {
  int nt, n, logn, resp_comp, analytic;
  double inv_n;  // 1 / N, exact
};

AF_FFT_HD int fft_log2(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}

// idx with its low logn bits reversed
AF_FFT_HD unsigned fft_bitrev(unsigned idx, int logn) {
  unsigned r = 0;
  for (int b = 0; b < logn; b++) r |= ((idx >> b) & 1u) << (logn - 1 - b);
  return r;
}

// the passes of a sweep, the layers of the first one, and what step 0 .. 2 npass - 2 of the whole
// transform (forward sweep, pointwise, inverse sweep) is: its first layer, its layers, its flags
AF_FFT_HD int fft_npass(int logn) { return logn <= 3 ? 1 : (logn + 2) / 3; }
AF_FFT_HD int fft_first_len(int logn) { return logn - 3 * (fft_npass(logn) - 1); }
AF_FFT_HD int fft_nsteps(int logn) { return 2 * fft_npass(logn) - 1; }
AF_FFT_HD void fft_step(int logn, int step, int* l0, int* L, int* flags) {
  const int np = fft_npass(logn), first = fft_first_len(logn);
  const int s = step < np ? step : 2 * np - 2 - step;
  *l0 = s == 0 ? 0 : first + 3 * (s - 1);
  *L = s == 0 ? first : 3;
  int f = 0;
  if (step <= np - 1) f |= kFftDif;
  if (step == np - 1) f |= kFftPoint;
  if (step >= np - 1) f |= kFftDit;
  if (step == 0) f |= kFftFromGlobal;
  if (step == 2 * np - 2) f |= kFftToGlobal;
  *flags = f;
}

// traces a workgroup transforms at a time: short transforms share it
AF_FFT_HD int fft_pack(int n) { return n >= 2048 ? 1 : (2048 / n > kFftBlock ? kFftBlock : 2048 / n); }
// a trace in LDS
AF_FFT_HD int fft_slot(int idx) { return idx + (idx >> 3); }
AF_FFT_HD int fft_lds_elems(int n) { return n + (n >> 3); }
// FftC elements of a workgroup's LDS (none when the transform is one pass)
AF_FFT_HD int fft_lds_total(int n) { return fft_npass(fft_log2(n)) > 1 ? fft_pack(n) * fft_lds_elems(n) : 0; }

// (c, s) = (cos, sin)(2 pi j / 8192), 0 <= j < 4096, from tab[m] = sin(2 pi m / 8192), m = 0 .. 2048:
// sin(pi - t) = sin t, cos t = sin(pi / 2 - t), cos t = -sin(t - pi / 2), exact in the argument
AF_FFT_HD void fft_twiddle(const double* tab, int j, double* c, double* s) {
  const int up = j > 2048;
  const int d = up ? j - 2048 : 2048 - j;
  const double cm = tab[d];
  *s = tab[2048 - d];
  *c = up ? -cm : cm;
}

AF_FFT_HD void fft_mul(double ar, double ai, double wr, double wi, double* pr, double* pi) {
  const double rr = ar * wr, ii = ai * wi, ri = ar * wi, ir = ai * wr;
  *pr = rr - ii;
  *pi = ri + ir;
}

template <typename T, int NC>
AF_FFT_HD void fft_load(const T* x, int nt, int n, double* re, double* im) {
  *re = n < nt ? (double)x[(int64_t)n * NC] : 0.0;
  *im = (NC == 2 && n < nt) ? (double)x[(int64_t)n * NC + 1] : 0.0;
}

template <typename T>
AF_FFT_HD void fft_store(T* y, int nt, double inv_n, int n, double re, double im) {
  if (n >= nt) return;
  y[(int64_t)n * 2] = (T)(re * inv_n);
  y[(int64_t)n * 2 + 1] = (T)(im * inv_n);
}

// the pointwise step on element idx (bin bitrev(idx)); hrev is the response in element order,
// hrev[idx][resp_comp] = H[bitrev(idx)]
AF_FFT_HD void fft_pointwise(const FftShape& S, const double* hrev, int idx, double* re, double* im) {
  if (S.resp_comp == 1) {
    const double h = hrev[idx];
    *re = *re * h;
    *im = *im * h;
  } else if (S.resp_comp == 2) {
    fft_mul(*re, *im, hrev[2 * (int64_t)idx], hrev[2 * (int64_t)idx + 1], re, im);
  }
  if (S.analytic) {
    if (idx & 1) {
      if (idx != 1) *re = 0.0, *im = 0.0;
    } else if (idx != 0) {
      *re = *re * 2.0;
      *im = *im * 2.0;
    }
  }
}

// layers l0 .. l0 + L - 1 of the forward transform on a group in registers (i: the group's offset
// in its block of layer l0 + L - 1, i < hl)
template <int L>
AF_FFT_HD void fft_dif(double* re, double* im, int logn, int l0, int i, int hl, const double* tab) {
#pragma unroll
  for (int t = 0; t < L; t++) {
    const int span = 1 << (L - 1 - t), l = l0 + t;
#pragma unroll
    for (int j = 0; j < (1 << L); j++) {
      if (j & span) continue;
      double c, s;
      fft_twiddle(tab, ((i + (j & (span - 1)) * hl) << l) << (kFftMaxLog - logn), &c, &s);
      const double ar = re[j], ai = im[j], br = re[j + span], bi = im[j + span];
      re[j] = ar + br;
      im[j] = ai + bi;
      fft_mul(ar - br, ai - bi, c, -s, &re[j + span], &im[j + span]);
    }
  }
}

// the same layers of the inverse transform, l0 + L - 1 down to l0
template <int L>
AF_FFT_HD void fft_dit(double* re, double* im, int logn, int l0, int i, int hl, const double* tab) {
#pragma unroll
  for (int t = L - 1; t >= 0; t--) {
    const int span = 1 << (L - 1 - t), l = l0 + t;
#pragma unroll
    for (int j = 0; j < (1 << L); j++) {
      if (j & span) continue;
      double c, s, br, bi;
      fft_twiddle(tab, ((i + (j & (span - 1)) * hl) << l) << (kFftMaxLog - logn), &c, &s);
      fft_mul(re[j + span], im[j + span], c, s, &br, &bi);
      const double ar = re[j], ai = im[j];
      re[j] = ar + br;
      im[j] = ai + bi;
      re[j + span] = ar - br;
      im[j + span] = ai - bi;
    }
  }
}

// One work item: group g (0 <= g < N >> L) of the pass over layers l0 .. l0 + L - 1 of one trace.
// x, y: the trace's input [nt][NC] and output [nt][2]; v: its LDS image (unused by a pass that is
// both first and last); hrev: the response in element order (null: none); tab: the sine table.
template <typename T, int NC, int L>
AF_FFT_HD void fft_group(const FftShape& S, int l0, int flags, int g, const T* x, T* y, FftC* v, const double* hrev,
                         const double* tab) {
  double re[1 << L], im[1 << L];
  const int lh = S.logn - l0 - L, hl = 1 << lh;
  const int i = g & (hl - 1), q = ((g >> lh) << (S.logn - l0)) + i;
#pragma unroll
  for (int j = 0; j < (1 << L); j++) {
    if (flags & kFftFromGlobal) {
      fft_load<T, NC>(x, S.nt, q + j * hl, &re[j], &im[j]);
    } else {
      const FftC e = v[fft_slot(q + j * hl)];
      re[j] = e.re, im[j] = e.im;
    }
  }
  if (flags & kFftDif) fft_dif<L>(re, im, S.logn, l0, i, hl, tab);
  if (flags & kFftPoint) {
#pragma unroll
    for (int j = 0; j < (1 << L); j++) fft_pointwise(S, hrev, q + j, &re[j], &im[j]);  // (hl is 1 here)
  }
  if (flags & kFftDit) fft_dit<L>(re, im, S.logn, l0, i, hl, tab);
#pragma unroll
  for (int j = 0; j < (1 << L); j++) {
    if (flags & kFftToGlobal) {
      fft_store<T>(y, S.nt, S.inv_n, q + j * hl, re[j], im[j]);
    } else {
      FftC e;
      e.re = re[j], e.im = im[j];
      v[fft_slot(q + j * hl)] = e;
    }
  }
}

// Work item w (0 <= w < fft_pack(N) << (logn - L)) of a step on the batch of traces from `first`:
// its trace is first + (w >> (logn - L)), its group the low bits.  in / out: the call's arrays; lds:
// the workgroup's image of fft_lds_total(N) elements.
template <typename T, int NC>
AF_FFT_HD void fft_item(const FftShape& S, int l0, int L, int flags, int64_t first, int64_t ntrace, int w, const T* in,
                        T* out, FftC* lds, const double* hrev, const double* tab) {
  const int tl = w >> (S.logn - L), g = w & ((S.n >> L) - 1);
  const int64_t trace = first + tl;
  if (trace >= ntrace) return;
  const T* x = in + trace * (int64_t)S.nt * NC;
  T* y = out + trace * (int64_t)S.nt * 2;
  const int ends = kFftFromGlobal | kFftToGlobal;
  FftC* v = (flags & ends) == ends ? nullptr : lds + (int64_t)tl * fft_lds_elems(S.n);
  switch (L) {
    case 0: fft_group<T, NC, 0>(S, l0, flags, g, x, y, v, hrev, tab); break;
    case 1: fft_group<T, NC, 1>(S, l0, flags, g, x, y, v, hrev, tab); break;
    case 2: fft_group<T, NC, 2>(S, l0, flags, g, x, y, v, hrev, tab); break;
    default: fft_group<T, NC, 3>(S, l0, flags, g, x, y, v, hrev, tab); break;
  }
}

}  // namespace af
