// skip_pick.h — the per-element code of the back-wall echo paths of include/alifmm.h
// (alifmm_skip_pick, alifmm_skip_rays): the finite test of a candidate sum, the total order the pick
// is the minimum of, and the index arithmetic of a joined two-leg ray.  Shared verbatim by the
// kernels (skip_pairs.hip) and by a stand-alone host program (tests/skip_sim.cpp, built with ASan and
// UBSan), so the order and the offsets are checked on a CPU before the kernels run.  Includes
// nothing from HIP; build with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_SKIP_HD __host__ __device__
#else
#define AF_SKIP_HD
#endif

namespace af {

// a candidate of the pick: the sum s_q = T_a(w_q) + T_b(w_q) and its node number q; q = -1 with
// v = +inf is "no candidate"
struct SkipKey {
  double v;
  int q;
};

AF_SKIP_HD inline SkipKey skip_key_none() { return SkipKey{__builtin_huge_val(), -1}; }

// neither NaN nor +-inf: the exponent field is not all ones (a test on the bits, so no rewriting of
// s - s or s == s by the compiler can change it)
AF_SKIP_HD inline bool skip_finite(double s) {
  const uint64_t b = __builtin_bit_cast(uint64_t, s);
  return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// a comes before b in the pick's total order: a candidate before none, the smaller sum first, of
// equal sums (-0.0 == 0.0) the smaller node number.  Keys hold finite sums or are skip_key_none().
AF_SKIP_HD inline bool skip_key_before(SkipKey a, SkipKey b) {
  if (a.q < 0) return false;
  if (b.q < 0) return true;
  return a.v < b.v || (a.v == b.v && a.q < b.q);
}

// the minimum of two keys: what a reduction tree combines, in any shape
AF_SKIP_HD inline SkipKey skip_key_min(SkipKey a, SkipKey b) { return skip_key_before(b, a) ? b : a; }

// node q with field values ta, tb taken into the running minimum: one float64 add, the finite test
AF_SKIP_HD inline SkipKey skip_key_take(SkipKey best, double ta, double tb, int q) {
  const double s = ta + tb;
  if (!skip_finite(s)) return best;
  return skip_key_min(best, SkipKey{s, q});
}

// field offset of reflector node (iz, ix)
AF_SKIP_HD inline int64_t skip_node_offset(int iz, int ix, int fnx) { return (int64_t)iz * fnx + ix; }

// The joined ray of a pair: leg A (hit -> a, len_a points) reversed, then leg B (hit -> b, len_b
// points) from its second point on.  Both legs start at the hit node, which so appears once.
AF_SKIP_HD inline int skip_join_len(int len_a, int len_b) { return len_a + len_b - 1; }

// point i of the joined ray (0 <= i < skip_join_len): its slot in the ray kernel's point buffers
// ([leg][max_pts] per coordinate), legs 2 p (A) and 2 p + 1 (B) of pair p of the launch
AF_SKIP_HD inline int64_t skip_join_src(int64_t pair, int i, int len_a, int max_pts) {
  const int64_t leg = 2 * pair + (i < len_a ? 0 : 1);
  const int idx = i < len_a ? len_a - 1 - i : i - len_a + 1;
  return leg * (int64_t)max_pts + idx;
}

// x of point i of a ray whose first point is point `off` of the packed buffer (z follows at + 1)
AF_SKIP_HD inline int64_t skip_join_dst(int64_t off, int i) { return 2 * (off + (int64_t)i); }

}  // namespace af
