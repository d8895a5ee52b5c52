// Stand-alone host run of the spectral trace filter's own code (csrc/trace_fft_term.h), built with
// ASan and UBSan by tests/test_trace_fft_ref.py.  It replays trace_fft.hip's schedule: batches of
// fft_pack(N) traces, per batch the steps of fft_step in order, per step every work item through
// fft_item, over an LDS image of exactly the kernel's size (poisoned with NaN before each batch, so
// a slot a pass misses shows in the output), the response permuted to element order as the host
// unit does it.  So the group index maps, the LDS padding, the twiddle index and the fused middle
// step are checked on a CPU, out-of-bounds accesses included, before the kernel runs on a GPU.
// Test infrastructure only.
//   trace_fft_sim INPUT OUTPUT   INPUT: the file of tests/trace_fft_ref.py write_sim_input(); OUTPUT:
//   [ntrace][nt][2] in the data's dtype.  Exit status 0, or 2 on a malformed input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fft_twiddles.h"
#include "trace_fft_term.h"

using namespace af;

template <typename T, int NC>
static void run(const FftShape& S, int64_t ntrace, const T* in, T* out, const double* hrev) {
  const int pack = fft_pack(S.n), nsteps = fft_nsteps(S.logn);
  std::vector<FftC> lds((size_t)fft_lds_total(S.n));
  for (int64_t first = 0; first < ntrace; first += pack) {
    for (FftC& e : lds) e.re = e.im = NAN;
    for (int step = 0; step < nsteps; step++) {
      int l0, L, flags;
      fft_step(S.logn, step, &l0, &L, &flags);
      const int items = pack << (S.logn - L);
      for (int w = 0; w < items; w++) fft_item<T, NC>(S, l0, L, flags, first, ntrace, w, in, out, lds.data(), hrev, kFftQuarterSin);
    }
  }
}

template <typename T>
static int whole(FILE* f, const char* path, const FftShape& S, int64_t ntrace, int nc) {
  std::vector<T> in((size_t)ntrace * S.nt * nc), out((size_t)ntrace * S.nt * 2, (T)-9);
  std::vector<double> h((size_t)S.n * S.resp_comp), hrev(h.size());
  if (fread(in.data(), sizeof(T), in.size(), f) != in.size()) return 2;
  if (fread(h.data(), sizeof(double), h.size(), f) != h.size()) return 2;
  for (int idx = 0; idx < S.n; idx++)
    for (int c = 0; c < S.resp_comp; c++) hrev[(size_t)idx * S.resp_comp + c] = h[(size_t)fft_bitrev(idx, S.logn) * S.resp_comp + c];
  const double* hp = S.resp_comp ? hrev.data() : nullptr;
  if (nc == 1) run<T, 1>(S, ntrace, in.data(), out.data(), hp);
  else run<T, 2>(S, ntrace, in.data(), out.data(), hp);
  FILE* g = fopen(path, "wb");
  if (!g || fwrite(out.data(), sizeof(T), out.size(), g) != out.size()) return 2;
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
  const int nt = (int)h[1], nc = (int)h[2], dtype = (int)h[3], rc = (int)h[5], analytic = (int)h[6];
  int n = (int)h[4];
  if (ntrace < 1 || nt < 1 || nt > kFftMax || (nc != 1 && nc != 2) || (dtype != 0 && dtype != 1) || rc < 0 || rc > 2 ||
      (analytic != 0 && analytic != 1))
    return 2;
  if (n == 0) n = 1 << fft_log2(nt);
  if (n < nt || n > kFftMax || (n & (n - 1))) return 2;
  const FftShape S{nt, n, fft_log2(n), rc, analytic, 1.0 / n};
  const int r = dtype ? whole<float>(f, argv[2], S, ntrace, nc) : whole<double>(f, argv[2], S, ntrace, nc);
  fclose(f);
  return r;
}
