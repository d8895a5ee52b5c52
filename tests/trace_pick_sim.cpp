// Stand-alone host run of the time-of-flight picker's own code (csrc/trace_pick_term.h), built with
// ASan and UBSan by tests/test_trace_pick_ref.py.  It replays trace_pick.hip's schedule on 64
// simulated lanes: per trace every lane's first walk, the butterfly over the lane distances 32 .. 1
// on the keys and on the non-finite mark, every lane's second walk with the combined peak, the same
// butterfly on the runner-up keys and the onset indices, and lane 0's refinement.  Each trace is
// copied into a buffer of exactly its nt samples, so a read outside the trace is ASan's to report;
// after every butterfly all 64 lanes must hold the same value (the combines are commutative), which
// is checked.  So the order, the "none" keys of idle lanes and every sample offset are checked on a
// CPU before the kernel runs on a GPU.  Test infrastructure only.
//   trace_pick_sim INPUT OUTPUT   INPUT: the file of tests/trace_pick_ref.py write_sim_input();
//   OUTPUT: pos, amp, amp2 float64 [ntrace] each, then idx, idx2, flags int32 [ntrace] each.
//   Exit status 0, 2 on a malformed input, 3 when the lanes disagree after a butterfly.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "trace_pick_term.h"

using namespace af;

static bool same(PickKey a, PickKey b) { return a.n == b.n && memcmp(&a.e, &b.e, sizeof(double)) == 0; }

// what the kernel's __shfl_xor loops do: lane l combines with lane l ^ d, d = 32 .. 1
template <class V, class F>
static bool butterfly(V* v, F combine, bool (*eq)(V, V)) {
  for (int d = 32; d >= 1; d >>= 1) {
    V o[kPickLanes];
    for (int l = 0; l < kPickLanes; l++) o[l] = v[l ^ d];
    for (int l = 0; l < kPickLanes; l++) v[l] = combine(v[l], o[l]);
  }
  for (int l = 1; l < kPickLanes; l++)
    if (!eq(v[0], v[l])) return false;
  return true;
}

static bool same_int(int a, int b) { return a == b; }

template <typename T, int NC>
static int one(const T* x, int nt, int lo, int hi, int mode, double frac, int guard, PickOut* out) {
  *out = pick_out_none(kPickNoGate);
  if (!(lo < hi && lo >= 0 && hi <= nt)) return 0;
  PickKey key[kPickLanes];
  int bad[kPickLanes], onset[kPickLanes];
  for (int l = 0; l < kPickLanes; l++) {
    bad[l] = 0;
    key[l] = pick_lane_peak<T, NC>(x, lo, hi, l, &bad[l]);
  }
  if (!butterfly<PickKey>(key, pick_key_max, same)) return 3;
  if (!butterfly<int>(bad, [](int a, int b) { return a | b; }, same_int)) return 3;
  const PickKey best = key[0];
  PickKey second = pick_key_none();
  int first = -1;
  if (pick_has_peak(best)) {
    const double thr = pick_threshold(frac, best.e);
    for (int l = 0; l < kPickLanes; l++) {
      onset[l] = -1;
      key[l] = pick_lane_second<T, NC>(x, lo, hi, l, best.n, guard, mode, thr, &onset[l]);
    }
    if (!butterfly<PickKey>(key, pick_key_max, same)) return 3;
    if (!butterfly<int>(onset, pick_idx_min, same_int)) return 3;
    second = key[0];
    first = onset[0];
  }
  *out = pick_refine<T, NC>(x, nt, lo, hi, mode, frac, best, bad[0], second, first);
  return 0;
}

template <typename T>
static int whole(FILE* f, const char* path, int64_t ntrace, int nt, int nc, int mode, double frac, int guard,
                 const std::vector<int32_t>& lo, const std::vector<int32_t>& hi) {
  const size_t n = (size_t)ntrace;
  std::vector<double> d(3 * n);
  std::vector<int32_t> i(3 * n);
  for (size_t t = 0; t < n; t++) {
    std::vector<T> x((size_t)nt * nc);  // the trace alone: its neighbours are out of bounds
    if (fread(x.data(), sizeof(T), x.size(), f) != x.size()) return 2;
    PickOut o;
    const int r = nc == 1 ? one<T, 1>(x.data(), nt, lo[t], hi[t], mode, frac, guard, &o)
                          : one<T, 2>(x.data(), nt, lo[t], hi[t], mode, frac, guard, &o);
    if (r) return r;
    d[t] = o.pos, d[n + t] = o.amp, d[2 * n + t] = o.amp2;
    i[t] = o.idx, i[n + t] = o.idx2, i[2 * n + t] = o.flags;
  }
  FILE* g = fopen(path, "wb");
  if (!g || fwrite(d.data(), sizeof(double), d.size(), g) != d.size() || fwrite(i.data(), sizeof(int32_t), i.size(), g) != i.size())
    return 2;
  fclose(g);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t h[8];
  if (fread(h, sizeof(int64_t), 8, f) != 8) return 2;
  const int64_t ntrace = h[0];
  const int nt = (int)h[1], nc = (int)h[2], dtype = (int)h[3], mode = (int)h[4], guard = (int)h[5];
  double frac;
  memcpy(&frac, &h[6], sizeof frac);
  if (ntrace < 1 || ntrace > (1 << 24) || nt < 1 || (nc != 1 && nc != 2) || (dtype != 0 && dtype != 1) ||
      (mode != 0 && mode != 1) || guard < 0 || (mode == 1 && !(frac > 0.0 && frac <= 1.0)))
    return 2;
  std::vector<int32_t> lo((size_t)ntrace), hi((size_t)ntrace);
  if (fread(lo.data(), sizeof(int32_t), lo.size(), f) != lo.size()) return 2;
  if (fread(hi.data(), sizeof(int32_t), hi.size(), f) != hi.size()) return 2;
  const int r = dtype ? whole<float>(f, argv[2], ntrace, nt, nc, mode, frac, guard, lo, hi)
                      : whole<double>(f, argv[2], ntrace, nt, nc, mode, frac, guard, lo, hi);
  fclose(f);
  return r;
}
