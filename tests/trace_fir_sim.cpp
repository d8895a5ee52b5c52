// Stand-alone host run of the trace FIR's own code (csrc/trace_fir_term.h), built with ASan and
// UBSan by tests/test_trace_fir_ref.py.  It walks the (trace, tile) space as trace_fir.hip's
// workgroups do, with the tile length read from the input: the taps staged once, then per tile the
// segment staged into a buffer of exactly the kernel's size (trace_fir_stage), every thread's four
// outputs through its sliding window (trace_fir_thread) and the stores (trace_fir_store), so the
// mirrored index mapping, the staging layout and the window's rotation are checked on a CPU, out of
// bounds accesses included, before the kernel runs on a GPU.  Test infrastructure only.
//   trace_fir_sim INPUT OUTPUT   INPUT: the file of tests/trace_fir_ref.py write_sim_input(); OUTPUT:
//   float64 [ntrace][nt][ncomp].  Exit status 0, or 2 on a malformed input.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "trace_fir_term.h"

using namespace af;

template <int NC, int TC>
static void run(const double* in, double* out, const double* taps, int64_t ntrace, int nt, int ntap, int origin,
                int transpose, int tile) {
  const int seg = trace_fir_seg(tile, ntap), quarter = trace_fir_quarter(seg), threads = tile / kFirOutPerThread;
  std::vector<double> s((size_t)4 * quarter * NC), g((size_t)ntap * TC);
  for (int j = 0; j < ntap; j++) trace_fir_stage_tap<TC>(taps, j, transpose, g.data() + (size_t)j * TC);
  const int64_t ntiles = ((int64_t)nt + tile - 1) / tile;
  for (int64_t w = 0; w < ntrace * ntiles; w++) {
    const int64_t trace = w / ntiles, t0 = (w % ntiles) * tile;
    const double* x = in + trace * (int64_t)nt * NC;
    double* y = out + trace * (int64_t)nt * NC;
    for (double& v : s) v = -7.0;  // (a position the staging misses would show in the sums)
    for (int i = 0; i < seg; i++) trace_fir_stage<NC>(x, nt, transpose, t0, tile, origin, i, quarter, s.data());
    for (int tid = 0; tid < threads; tid++) {
      double acc[kFirOutPerThread][NC];
      trace_fir_thread<NC, TC>(s.data(), quarter, g.data(), ntap, tid, acc);
      for (int r = 0; r < kFirOutPerThread; r++)
        trace_fir_store<NC>(y, nt, transpose, t0, tile, kFirOutPerThread * tid + r, acc[r]);
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t h[8];
  if (fread(h, sizeof(int64_t), 8, f) != 8) return 2;
  const int64_t ntrace = h[0];
  const int nt = (int)h[1], nc = (int)h[2], ntap = (int)h[3], tc = (int)h[4], origin = (int)h[5], transpose = (int)h[6],
            tile = (int)h[7];
  if (ntrace < 1 || nt < 1 || (nc != 1 && nc != 2) || (tc != 1 && tc != 2) || tc > nc || ntap < 1 || ntap > kFirMaxTaps ||
      origin < 0 || origin >= ntap || (transpose != 0 && transpose != 1) || tile < kFirOutPerThread ||
      tile % kFirOutPerThread)
    return 2;
  std::vector<double> in((size_t)ntrace * nt * nc), taps((size_t)ntap * tc), out(in.size(), -9.0);
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  if (fread(taps.data(), sizeof(double), taps.size(), f) != taps.size()) return 2;
  fclose(f);
  if (nc == 1) run<1, 1>(in.data(), out.data(), taps.data(), ntrace, nt, ntap, origin, transpose, tile);
  else if (tc == 1) run<2, 1>(in.data(), out.data(), taps.data(), ntrace, nt, ntap, origin, transpose, tile);
  else run<2, 2>(in.data(), out.data(), taps.data(), ntrace, nt, ntap, origin, transpose, tile);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  fclose(f);
  return 0;
}
