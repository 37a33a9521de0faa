// The reference window of a path-following MPC step (cddp-cpp_amd/csrc/ref_window.hpp) on the host: the function the window kernel runs per
// element, over rows_per_step 1.0, 2.0, 0.5 and 0.3, paths of one row and of nine, nx = 1, 3 and 14, cursors that run past the end of the
// path.  The path is held in a heap array of EXACTLY rows * nx doubles, so the sanitized build faults on any index outside it.
// Checked here: rows_per_step 1.0 copies path rows bit for bit; past the end every row is the last row; every value is finite.
// Stand-alone: built by tests/test_ref_window_host.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_ref_window OUT -- every case's path and windows go to OUT as hex floats, for the numpy restatement to be held against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/ref_window.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double rnd() {   // uniform in [-1, 1): a 64-bit LCG, its top 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

void dump(FILE *f, const char *name, const double *v, size_t n) {
  std::fprintf(f, "%s %zu", name, n);
  for (size_t i = 0; i < n; ++i) std::fprintf(f, " %a", v[i]);
  std::fprintf(f, "\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s OUT\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "w");
  if (!f) { std::perror(argv[1]); return 2; }
  const double rates[] = {1.0, 2.0, 0.5, 0.3};
  const int dims[] = {1, 3, 14};
  const long long lens[] = {1, 9};
  const long long cursors[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 40, 1000000, 4611686018427387904ll};
  const int N = 6;
  int bad = 0, cases = 0;
  for (double rps : rates)
    for (int nx : dims)
      for (long long L : lens) {
        double *path = new double[(size_t)L * nx];
        for (size_t i = 0; i < (size_t)L * nx; ++i) path[i] = 3.0 * rnd();
        for (long long k : cursors) {
          std::vector<double> w((size_t)(N + 1) * nx);
          for (int t = 0; t <= N; ++t)
            for (int e = 0; e < nx; ++e) w[(size_t)t * nx + e] = cddp_ref::window_elem(path, L, nx, k, rps, t, e);
          for (int t = 0; t <= N; ++t)
            for (int e = 0; e < nx; ++e) {
              const double v = w[(size_t)t * nx + e];
              if (!std::isfinite(v)) { std::printf("not finite: rps %g nx %d L %lld k %lld t %d e %d\n", rps, nx, L, k, t, e); ++bad; }
              const double last = path[(size_t)(L - 1) * nx + e];
              const double pos = (double)(k + t) * rps;
              if (pos >= (double)(L - 1) && std::memcmp(&v, &last, sizeof v) != 0) { std::printf("past the end is not the last row: rps %g nx %d L %lld k %lld t %d\n", rps, nx, L, k, t); ++bad; }
              if (rps == 1.0 && k + t < L && std::memcmp(&v, &path[(size_t)(k + t) * nx + e], sizeof v) != 0) { std::printf("rows_per_step 1 is not a copy: nx %d L %lld k %lld t %d\n", nx, L, k, t); ++bad; }
            }
          std::fprintf(f, "case %d %lld %d %lld %a\n", nx, L, N, k, rps);
          dump(f, "path", path, (size_t)L * nx);
          dump(f, "window", w.data(), w.size());
          ++cases;
        }
        delete[] path;
      }
  std::fclose(f);
  if (bad) { std::printf("ref window: %d FAILED\n", bad); return 1; }
  std::printf("ref window: ok (%d cases)\n", cases);
  return 0;
}
