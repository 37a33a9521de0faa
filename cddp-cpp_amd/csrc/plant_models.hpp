// Every model struct of dev_models.hpp as one list: what the kernels that are dispatched on the model id rather than compiled into a
// KernelSet are instantiated over (inst_plant.hip: the device-resident plant; inst_score.hip: the scoring rollout).
#pragma once
#include "dev_models.hpp"

namespace cddp_dev {

typedef LTIModel<1, 1> Lti11;
typedef LTIModel<2, 1> Lti21;

// every model struct: Y(Model).  The two LTI shapes are the ones inst_lti.hip builds solver kernels for.
#define PLANT_MODEL_LIST(Y) \
  Y(PendulumModel) Y(CartPoleModel) Y(UnicycleModel) Y(QuadrotorModel) Y(ManipulatorModel) Y(Quad12Model) Y(Manip7Model) Y(BicycleModel) \
  Y(CarModel) Y(HCWModel) Y(EulerAttitudeModel) Y(QuaternionAttitudeModel) Y(MrpAttitudeModel) Y(SpacecraftTwobodyModel) \
  Y(SpacecraftLanding2DModel) Y(DubinsCarModel) Y(DreyfusRocketModel) Y(AcrobotModel) Y(Usv3DofModel) Y(ForkliftModel) \
  Y(QuadrotorRateModel) Y(SpacecraftLinearFuelModel) Y(SpacecraftNonlinearModel) Y(Lti11) Y(Lti21)

}  // namespace cddp_dev
