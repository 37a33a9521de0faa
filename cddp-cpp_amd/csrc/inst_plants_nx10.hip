// Explicit instantiation of the solver kernels for the two built-in plants of nx = 10 (see launch.hpp): the rate-controlled quadrotor
// and the nonlinear relative-motion spacecraft, each unconstrained and with a control box.  A unit of its own, so that neither this
// one nor inst_plants_small.hip governs the parallel build.
#include "launch.hpp"
namespace cddp_dev {
void register_plants_nx10(std::vector<KernelSet> &v) {
  v.push_back(Launcher<QuadrotorRateModel, ConList<>>::set("quadrotor_rate/none"));
  v.push_back(Launcher<QuadrotorRateModel, ConList<CtrlBox<4>>>::set("quadrotor_rate/ctrlbox"));
  v.push_back(Launcher<SpacecraftNonlinearModel, ConList<>>::set("spacecraft_nonlinear/none"));
  v.push_back(Launcher<SpacecraftNonlinearModel, ConList<CtrlBox<3>>>::set("spacecraft_nonlinear/ctrlbox"));
}
}  // namespace cddp_dev
