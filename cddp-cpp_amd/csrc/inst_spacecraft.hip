// Explicit instantiation of the solver kernels for the spacecraft plants of nx <= 8 (see launch.hpp): the three rigid-body attitude
// forms, the two-body point mass and the 2-D lander, each unconstrained and with a control box.  Nothing else: every list costs
// compile time.
#include "launch.hpp"
namespace cddp_dev {
void register_spacecraft(std::vector<KernelSet> &v) {
  v.push_back(Launcher<EulerAttitudeModel, ConList<>>::set("euler_attitude/none"));
  v.push_back(Launcher<EulerAttitudeModel, ConList<CtrlBox<3>>>::set("euler_attitude/ctrlbox"));
  v.push_back(Launcher<QuaternionAttitudeModel, ConList<>>::set("quaternion_attitude/none"));
  v.push_back(Launcher<QuaternionAttitudeModel, ConList<CtrlBox<3>>>::set("quaternion_attitude/ctrlbox"));
  v.push_back(Launcher<MrpAttitudeModel, ConList<>>::set("mrp_attitude/none"));
  v.push_back(Launcher<MrpAttitudeModel, ConList<CtrlBox<3>>>::set("mrp_attitude/ctrlbox"));
  v.push_back(Launcher<SpacecraftTwobodyModel, ConList<>>::set("twobody/none"));
  v.push_back(Launcher<SpacecraftTwobodyModel, ConList<CtrlBox<3>>>::set("twobody/ctrlbox"));
  v.push_back(Launcher<SpacecraftLanding2DModel, ConList<>>::set("landing2d/none"));
  v.push_back(Launcher<SpacecraftLanding2DModel, ConList<CtrlBox<2>>>::set("landing2d/ctrlbox"));
}
}  // namespace cddp_dev
