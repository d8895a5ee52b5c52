// trace_pick_term.h — the per-trace rules of the time-of-flight picker (include/alifmm.h
// alifmm_trace_pick): a sample's energy and its finite test, the total order the peak and the
// runner-up are the maximum of, the combines a reduction tree uses, a lane's two walks over the gate
// and the refinement to a fractional sample.  Shared verbatim by the kernel (trace_pick.hip) and by
// a stand-alone host program (tests/trace_pick_sim.cpp, built with ASan and UBSan) that walks the
// same lanes and combines them with the same butterfly, so the order, the "none" keys of idle lanes
// and every sample offset are checked on a CPU before the kernel runs.  Includes nothing from HIP;
// build with -ffp-contract=off and without fast-math (the float64 sqrt and division are correctly
// rounded).
//
// The contract, for one trace of nt samples and a gate [lo, hi), 0 <= lo < hi <= nt (everything
// float64, no contraction, operations as written):
//   energy     e[n] = (re * re) + (im * im), x * x for real data; a float32 sample converts exactly
//   candidate  a sample of the gate whose e is neither NaN nor +-inf (a test on the bits); any
//              other sample in the gate sets flag 16
//   peak       idx: the maximum over the gate's candidates of "larger e first, of equal e the lower
//              n"; amp = sqrt(e[idx]).  No candidate, or e[idx] == 0: flag 2, idx = idx2 = -1,
//              pos = NaN, amp = amp2 = 0
//   runner-up  idx2: the maximum of the same order over the gate's candidates with
//              |n - idx| > guard; amp2 = sqrt(e[idx2]); none: idx2 = -1, amp2 = 0
//   mode 0     m = idx.  With 0 < m < nt - 1 and e[m - 1], e[m + 1] both neither NaN nor +-inf
//              (they may lie outside the gate): a- = sqrt(e[m - 1]), a0 = amp, a+ = sqrt(e[m + 1]);
//              if a- <= a0, a+ <= a0 and den = (a- - (2 * a0)) + a+ < 0:
//              delta = (0.5 * (a- - a+)) / den.  In every other case delta = 0 and flag 4.  Flag 8
//              if m == lo or m == hi - 1
//   mode 1     thr = (frac * frac) * e[idx]; m: the lowest candidate n of the gate with e[n] >= thr
//              (idx is one).  With m > 0, e[m - 1] neither NaN nor +-inf and e[m - 1] < thr:
//              at = sqrt(thr), am = sqrt(e[m]), a- = sqrt(e[m - 1]), den = am - a-; if den > 0:
//              delta = -((am - at) / den).  In every other case delta = 0 and flag 4.  Flag 8 if
//              m == lo
//   position   pos = (double)m + delta
//   no gate    lo >= hi: flag 1 alone, the outputs as under flag 2
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_PICK_HD __host__ __device__ inline
#else
#define AF_PICK_HD inline
#endif

namespace af {

constexpr int kPickLanes = 64;  // the lanes that share a trace
enum { kPickNoGate = 1, kPickEmpty = 2, kPickUnrefined = 4, kPickAtEdge = 8, kPickNonFinite = 16 };

// a candidate: its energy and its sample; n = -1 with e = +0.0 is "none"
struct PickKey {
  double e;
  int n;
};

// what a trace's pick is
struct PickOut {
  double pos, amp, amp2;
  int idx, idx2, flags;
};

AF_PICK_HD PickKey pick_key_none() { return PickKey{0.0, -1}; }

// neither NaN nor +-inf: the exponent field is not all ones (skip_pick.h skip_finite)
AF_PICK_HD bool pick_finite(double e) {
  const uint64_t b = __builtin_bit_cast(uint64_t, e);
  return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// a comes before b: a candidate before none, the larger energy first, of equal energies the lower
// sample.  Keys hold finite energies (never -0.0: they are sums of squares) or are pick_key_none().
AF_PICK_HD bool pick_key_before(PickKey a, PickKey b) {
  if (a.n < 0) return false;
  if (b.n < 0) return true;
  return a.e > b.e || (a.e == b.e && a.n < b.n);
}

// the maximum of two keys and the lower of two sample indices (-1: none): total orders, so both
// are associative and commutative and a reduction tree of any shape gives the same bits
AF_PICK_HD PickKey pick_key_max(PickKey a, PickKey b) { return pick_key_before(b, a) ? b : a; }
AF_PICK_HD int pick_idx_min(int a, int b) { return a < 0 ? b : (b < 0 ? a : (b < a ? b : a)); }

template <typename T, int NC>
AF_PICK_HD double pick_energy(const T* x, int64_t n) {
  const double re = (double)x[n * NC];
  if (NC == 1) return re * re;
  const double im = (double)x[n * NC + 1];
  const double rr = re * re, ii = im * im;
  return rr + ii;
}

// the threshold of mode 1 from the peak's energy
AF_PICK_HD double pick_threshold(double frac, double e_peak) { return (frac * frac) * e_peak; }

// First walk of lane `lane`: samples lo + lane, lo + lane + 64, ... of the gate into the lane's best
// key; *bad becomes 1 when one of them is no candidate.
template <typename T, int NC>
AF_PICK_HD PickKey pick_lane_peak(const T* x, int lo, int hi, int lane, int* bad) {
  PickKey best = pick_key_none();
  for (int64_t n = (int64_t)lo + lane; n < hi; n += kPickLanes) {
    const double e = pick_energy<T, NC>(x, n);
    if (!pick_finite(e)) {
      *bad = 1;
      continue;
    }
    best = pick_key_max(best, PickKey{e, (int)n});
  }
  return best;
}

// Second walk of the same samples, the peak `idx` (>= 0) being known: the lane's best key among the
// candidates further than `guard` from it, and (mode 1) its lowest candidate with e >= thr.
template <typename T, int NC>
AF_PICK_HD PickKey pick_lane_second(const T* x, int lo, int hi, int lane, int idx, int guard, int mode, double thr,
                                    int* onset) {
  PickKey second = pick_key_none();
  for (int64_t n = (int64_t)lo + lane; n < hi; n += kPickLanes) {
    const double e = pick_energy<T, NC>(x, n);
    if (!pick_finite(e)) continue;
    const int64_t d = n < idx ? idx - n : n - idx;
    if (d > guard) second = pick_key_max(second, PickKey{e, (int)n});
    if (mode == 1 && e >= thr) *onset = pick_idx_min(*onset, (int)n);
  }
  return second;
}

AF_PICK_HD PickOut pick_out_none(int flags) {
  return PickOut{__builtin_bit_cast(double, (uint64_t)0x7ff8000000000000ull), 0.0, 0.0, -1, -1, flags};
}

// does the peak the first walk found stand (else flag 2 and no second walk)
AF_PICK_HD bool pick_has_peak(PickKey best) { return best.n >= 0 && best.e != 0.0; }

// The trace's outputs from the combined keys: best and bad of the first walk, second and onset of
// the second (what one lane does after the reductions).
template <typename T, int NC>
AF_PICK_HD PickOut pick_refine(const T* x, int nt, int lo, int hi, int mode, double frac, PickKey best, int bad,
                               PickKey second, int onset) {
  const int nonfinite = bad ? kPickNonFinite : 0;
  if (!pick_has_peak(best)) return pick_out_none(kPickEmpty | nonfinite);
  PickOut o;
  o.idx = best.n;
  o.amp = __builtin_sqrt(best.e);
  o.idx2 = second.n;
  o.amp2 = second.n < 0 ? 0.0 : __builtin_sqrt(second.e);
  o.flags = nonfinite;
  double delta = 0.0;
  bool refined = false;
  int m;
  if (mode == 0) {
    m = best.n;
    if (m > 0 && m < nt - 1) {
      const double em = pick_energy<T, NC>(x, (int64_t)m - 1), ep = pick_energy<T, NC>(x, (int64_t)m + 1);
      if (pick_finite(em) && pick_finite(ep)) {
        const double am = __builtin_sqrt(em), a0 = o.amp, ap = __builtin_sqrt(ep);
        if (am <= a0 && ap <= a0) {
          const double den = (am - (2.0 * a0)) + ap;
          if (den < 0.0) {
            delta = (0.5 * (am - ap)) / den;
            refined = true;
          }
        }
      }
    }
    if (m == lo || m == hi - 1) o.flags |= kPickAtEdge;
  } else {
    m = onset;  // >= 0: the peak itself passes the threshold
    const double thr = pick_threshold(frac, best.e);
    if (m > 0) {
      const double em = pick_energy<T, NC>(x, (int64_t)m - 1);
      if (pick_finite(em) && em < thr) {
        const double at = __builtin_sqrt(thr), a1 = __builtin_sqrt(pick_energy<T, NC>(x, (int64_t)m));
        const double am = __builtin_sqrt(em), den = a1 - am;
        if (den > 0.0) {
          delta = -((a1 - at) / den);
          refined = true;
        }
      }
    }
    if (m == lo) o.flags |= kPickAtEdge;
  }
  if (!refined) o.flags |= kPickUnrefined;
  o.pos = (double)m + delta;
  return o;
}

}  // namespace af
