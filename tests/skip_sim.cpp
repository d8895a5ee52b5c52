// Stand-alone host run of the echo-path kernels' per-element code (csrc/skip_pick.h: the finite test,
// the key order, the joined-point index arithmetic with 64-bit offsets), built with ASan and UBSan by
// tests/test_skip_ref.py, so that code is checked on a CPU before the kernels (skip_pairs.hip, which
// call the very same functions) run on a GPU.  The pair reduction is laid out as the kernel's: 64
// lanes take the nodes round robin, then combine over the lane distances 32 .. 1; the join writes
// into a buffer of exactly the joined rays' size.  Test infrastructure only.
//   skip_sim INPUT OUTPUT   INPUT: the file of tests/skip_ref.py write_sim_input(); OUTPUT:
//   pick_time float64 [npairs], hit int32 [npairs], joined lengths int32 [njoin], packed points.
//   Exit status 0, or 2 on a malformed input.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "skip_pick.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> h;
  if (!rd(f, h, 8)) return 2;
  const int64_t npairs = h[0], nw = h[1], nf = h[2], nj = h[3], max_pts = h[4];
  if (npairs < 0 || nw < 1 || nf < 1 || nj < 0 || max_pts < 2 || nw > INT32_MAX || max_pts > INT32_MAX) return 2;
  std::vector<double> W, rx, ry;
  std::vector<int32_t> ra, rb, leg_len;
  if (!rd(f, W, (size_t)(nf * nw)) || !rd(f, ra, npairs) || !rd(f, rb, npairs) || !rd(f, leg_len, 2 * nj) ||
      !rd(f, rx, (size_t)(2 * nj * max_pts)) || !rd(f, ry, (size_t)(2 * nj * max_pts)))
    return 2;
  fclose(f);
  std::vector<double> pick(npairs);
  std::vector<int32_t> hit(npairs);
  for (int64_t k = 0; k < npairs; k++) {
    if (ra[k] < 0 || ra[k] >= nf || rb[k] < 0 || rb[k] >= nf) return 2;
    const double* wa = W.data() + (int64_t)ra[k] * nw;
    const double* wb = W.data() + (int64_t)rb[k] * nw;
    af::SkipKey lane[64];
    for (int l = 0; l < 64; l++) {
      lane[l] = af::skip_key_none();
      for (int q = l; q < nw; q += 64) lane[l] = af::skip_key_take(lane[l], wa[q], wb[q], q);
    }
    for (int d = 32; d >= 1; d >>= 1) {
      af::SkipKey next[64];
      for (int l = 0; l < 64; l++) next[l] = af::skip_key_min(lane[l], lane[l ^ d]);
      for (int l = 0; l < 64; l++) lane[l] = next[l];
    }
    for (int l = 1; l < 64; l++)  // every lane ends with the same key
      if (lane[l].q != lane[0].q) return 3;
    pick[k] = lane[0].v;
    hit[k] = lane[0].q;
  }
  std::vector<int32_t> jl(nj);
  std::vector<int64_t> off(nj + 1, 0);
  for (int64_t p = 0; p < nj; p++) {
    const int la = leg_len[2 * p], lb = leg_len[2 * p + 1];
    if (la < 2 || lb < 2 || la > max_pts || lb > max_pts) return 2;
    jl[p] = af::skip_join_len(la, lb);
    off[p + 1] = off[p] + jl[p];
  }
  std::vector<double> packed((size_t)(2 * off[nj]));
  for (int64_t p = 0; p < nj; p++)
    for (int i = 0; i < jl[p]; i++) {
      const int64_t s = af::skip_join_src(p, i, leg_len[2 * p], (int)max_pts), d = af::skip_join_dst(off[p], i);
      packed.at((size_t)d) = rx.at((size_t)s);
      packed.at((size_t)d + 1) = ry.at((size_t)s);
    }
  FILE* g = fopen(argv[2], "wb");
  if (!g || !wr(g, pick) || !wr(g, hit) || !wr(g, jl) || !wr(g, packed)) return 2;
  fclose(g);
  return 0;
}
