// Stand-alone driver of oref_cr_batch (cr_shim.cpp) for sanitizer runs of cr_math.h on the host:
//   cr_batch_main FN IN OUT    IN: n float64 arguments; OUT: n results (FN 4: n sines, then n cosines)
// Built with -fsanitize=address,undefined by tests/test_crmath.py; needs no preloaded runtime.
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int oref_cr_batch(int fn, long long n, const double* x, double* out, double* out2);

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int fn = atoi(argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long long n = ftell(f) / 8;
  fseek(f, 0, SEEK_SET);
  // exactly n elements each: a write past an end is the sanitizer's to report
  std::vector<double> x(n), out(n), out2(fn == 4 ? n : 0);
  if ((long long)fread(x.data(), 8, n, f) != n) return 3;
  fclose(f);
  if (oref_cr_batch(fn, n, x.data(), out.data(), fn == 4 ? out2.data() : nullptr) != 0) return 4;
  FILE* g = fopen(argv[3], "wb");
  if (!g) return 5;
  fwrite(out.data(), 8, n, g);
  if (!out2.empty()) fwrite(out2.data(), 8, out2.size(), g);
  return fclose(g) == 0 ? 0 : 5;
}
