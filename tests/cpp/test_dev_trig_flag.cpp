// dev_trig.hpp::sincos_fast_flag (host build of the same source): the bits of sincos_fast, and the range flag set exactly for
// |a| >= 1e9, NaN and inf.
// usage: test_dev_trig_flag [n]   -> prints "mismatches flag_errors n" and exits 0 when both are 0.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <cmath>
#include "../../cddp-cpp_amd/csrc/dev_trig.hpp"

static uint64_t rng_state = 0x13198A2E03707344ull;
static double urand() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0); }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
  long mismatches = 0, flag_errors = 0;
  auto check = [&](double x, bool want_flag) {
    bool flag = false;
    const cddp_dev::SinCosPair a = cddp_dev::sincos_fast_flag(x, flag);
    if (flag != want_flag) ++flag_errors;
    if (!want_flag) {   // in range: the bits of the shared routine (out of range the value is discarded by contract)
      const cddp_dev::SinCosPair b = cddp_dev::sincos_fast(x);
      if (bits(a.s) != bits(b.s) || bits(a.c) != bits(b.c)) ++mismatches;
    }
    bool sticky = true;   // a set flag stays set
    cddp_dev::sincos_fast_flag(x, sticky);
    if (!sticky) ++flag_errors;
  };
  const double ranges[] = {0.8, 7.0, 1000.0, 1.0e6, 1.0e9};
  const long per = n / 5;
  for (double R : ranges)
    for (long i = 0; i < per; ++i) {
      const double x = (2.0 * urand() - 1.0) * R;
      check(x, !(std::fabs(x) < 1.0e9));
    }
  for (int k = -4000; k <= 4000; ++k) check(k * 1.5707963267948966, false);   // every quadrant, both signs
  check(0.0, false); check(-0.0, false);
  const double below = std::nextafter(1.0e9, 0.0);
  check(below, false); check(-below, false);
  check(1.0e9, true); check(-1.0e9, true);
  check(std::nextafter(1.0e9, INFINITY), true);
  check(2.0e9, true); check(-3.0e300, true);
  check(INFINITY, true); check(-INFINITY, true); check(NAN, true);
  std::printf("%ld %ld %ld\n", mismatches, flag_errors, n);
  return (mismatches == 0 && flag_errors == 0) ? 0 : 1;
}
