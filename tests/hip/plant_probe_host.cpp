// Host build of the plant probe cases (plant_probe_cases.hpp): the same bodies over the same product header, compiled by g++ with
// -ffp-contract=off -DCDDP_TRIG_SHARED=1 into a shared library at test time (tests/plant_probe.py) -- the plants' host build in the
// kernels' own sin / cos.  Same entry points as the device library, plus hess() of the eight plants whose tensors exist on the host only.
#define CDDP_PROBE_HOST 1
#include <cstddef>
#include "plant_probe_cases.hpp"

#define PROBE_HOST(name, ...)                                                                               \
  extern "C" int probe_##name(const double *in, double *out, int B) {                                       \
    for (int i = 0; i < B; ++i) __VA_ARGS__::run(probe::Io{in, out, (size_t)B, (size_t)i});                 \
    return 0;                                                                                               \
  }                                                                                                         \
  extern "C" void probe_##name##_dims(int *nin, int *nout) { *nin = __VA_ARGS__::NIN; *nout = __VA_ARGS__::NOUT; }

#define Y_F(tag, M) PROBE_HOST(f_##tag, probe::CaseF<M>)
#define Y_STEP(tag, M) PROBE_HOST(step_##tag, probe::CaseStep<M>)
#define Y_JAC(tag, M) PROBE_HOST(jac_##tag, probe::CaseJac<M>)
#define Y_HESS(tag, M) PROBE_HOST(hess_##tag, probe::CaseHess<M>)
#define Y_HESS3(tag, M, Dyn) PROBE_HOST(hess_##tag, probe::CaseHess<M>)
#define Y_TENSOR(tag, M, Dyn) PROBE_HOST(tensor_##tag, probe::CaseTensor<M, Dyn>)
#define Y_JACBLK(tag, M, Dyn, BS) PROBE_HOST(jacblk_##tag, probe::CaseJacBlocked<M, Dyn, BS>)
PLANT_MODELS(Y_F)
PLANT_MODELS(Y_STEP)
PLANT_MODELS(Y_JAC)
PLANT_HESS_BOTH(Y_HESS)
PLANT_BLOCKED(Y_HESS3)   // host only
PLANT_BLOCKED(Y_TENSOR)
PLANT_JAC_BLOCKED(Y_JACBLK)
