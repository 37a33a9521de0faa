// Host build of the probe cases (dev_probe_cases.hpp): the same bodies, the same product headers, compiled by g++ with the product's
// -ffp-contract=off into a shared library at test time (tests/dev_probe.py).  Same entry points as the device library, so a case
// set runs through both and the results are compared bit for bit.
#define CDDP_PROBE_HOST 1
#include <cstddef>
#include "dev_probe_cases.hpp"

#define PROBE_HOST(name, C)                                                                       \
  extern "C" int probe_##name(const double *in, double *out, int B) {                             \
    for (int i = 0; i < B; ++i) C::run(probe::Io{in, out, (size_t)B, (size_t)i});                 \
    return 0;                                                                                     \
  }                                                                                               \
  extern "C" void probe_##name##_dims(int *nin, int *nout) { *nin = C::NIN; *nout = C::NOUT; }

PROBE_LANE_CASES(PROBE_HOST)
