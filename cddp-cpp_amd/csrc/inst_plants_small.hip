// Explicit instantiation of the solver kernels for the remaining built-in plants of nx <= 8 (see launch.hpp): Dubins car, Dreyfus
// rocket, acrobot, 3-DOF surface vessel, forklift and the HCW plant with a fuel state, each unconstrained and with a control box.
#include "launch.hpp"
namespace cddp_dev {
void register_plants_small(std::vector<KernelSet> &v) {
  v.push_back(Launcher<DubinsCarModel, ConList<>>::set("dubins_car/none"));
  v.push_back(Launcher<DubinsCarModel, ConList<CtrlBox<1>>>::set("dubins_car/ctrlbox"));
  v.push_back(Launcher<DreyfusRocketModel, ConList<>>::set("dreyfus_rocket/none"));
  v.push_back(Launcher<DreyfusRocketModel, ConList<CtrlBox<1>>>::set("dreyfus_rocket/ctrlbox"));
  v.push_back(Launcher<AcrobotModel, ConList<>>::set("acrobot/none"));
  v.push_back(Launcher<AcrobotModel, ConList<CtrlBox<1>>>::set("acrobot/ctrlbox"));
  v.push_back(Launcher<Usv3DofModel, ConList<>>::set("usv_3dof/none"));
  v.push_back(Launcher<Usv3DofModel, ConList<CtrlBox<3>>>::set("usv_3dof/ctrlbox"));
  v.push_back(Launcher<ForkliftModel, ConList<>>::set("forklift/none"));
  v.push_back(Launcher<ForkliftModel, ConList<CtrlBox<2>>>::set("forklift/ctrlbox"));
  v.push_back(Launcher<SpacecraftLinearFuelModel, ConList<>>::set("linear_fuel/none"));
  v.push_back(Launcher<SpacecraftLinearFuelModel, ConList<CtrlBox<3>>>::set("linear_fuel/ctrlbox"));
}
}  // namespace cddp_dev
