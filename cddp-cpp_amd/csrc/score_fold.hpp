// The path rows of a scoring rollout folded into its violation: what k_score (inst_score.hip) and k_mppi_score (inst_mppi.hip) share, so
// that a candidate drawn in the lane is valued exactly as one read from memory.  P->cons[] is walked at run time and every kind struct is
// reached through a compile-time loop over the dimensions the model admits (inst_score.hip's head has the reasoning).
#pragma once
#include "score_kernels.hpp"
#include "plant_models.hpp"
#include "dev_terminal.hpp"

namespace cddp_dev {

template <class C, int NX, int NU>
DEV void fold_rows(const ConDev &c, const double *pool, const double *x, const double *u, double &viol) {
  double g[C::DUAL];
  C::template eval<NX, NU>(c, pool, x, u, g);
#pragma unroll
  for (int i = 0; i < C::DUAL; ++i) viol = dmax(viol, g[i]);
}

// Kind<D> for the D that equals c.dim, D = D0 .. DMAX
template <template <int> class Kind, int NX, int NU, int D, int DMAX>
DEV void fold_dim(const ConDev &c, const double *pool, const double *x, const double *u, double &viol) {
  if (c.dim == D) fold_rows<Kind<D>, NX, NU>(c, pool, x, u, viol);
  else if constexpr (D < DMAX) fold_dim<Kind, NX, NU, D + 1, DMAX>(c, pool, x, u, viol);
}

template <int NX, int NU>
DEV void fold_path_rows(const ProblemDev *P, const double *x, const double *u, double &viol) {
  const double *pool = P->pool;
#pragma unroll 1
  for (int ci = 0; ci < P->n_cons; ++ci) {
    const ConDev &c = P->cons[ci];
    switch (c.kind) {
      case CDDP_HIP_CON_CONTROL_BOX: fold_rows<CtrlBox<NU>, NX, NU>(c, pool, x, u, viol); break;
      case CDDP_HIP_CON_STATE_BOX: fold_rows<StateBox<NX>, NX, NU>(c, pool, x, u, viol); break;
      case CDDP_HIP_CON_BALL: fold_dim<Ball, NX, NU, 1, NX>(c, pool, x, u, viol); break;
      case CDDP_HIP_CON_LINEAR: fold_dim<Linear, NX, NU, 1, 4>(c, pool, x, u, viol); break;
      case CDDP_HIP_CON_SOC:
        if constexpr (NX >= 3) fold_rows<SecondOrderCone, NX, NU>(c, pool, x, u, viol);
        break;
      case CDDP_HIP_CON_THRUST: fold_rows<ThrustMagnitude<NU, true>, NX, NU>(c, pool, x, u, viol); break;
      case CDDP_HIP_CON_MAX_THRUST: fold_rows<ThrustMagnitude<NU, false>, NX, NU>(c, pool, x, u, viol); break;
      default: break;   // (capi.hip::flatten has refused every other kind)
    }
  }
}

template <class M> bool is_model(int model, int nx, int nu) { return model == M::ID && nx == M::NX && nu == M::NU; }

}  // namespace cddp_dev
