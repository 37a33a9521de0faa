// Which of a trajectory's scored candidates seeds the solve: the ONE statement of the selection rule of cddp_hip_seed_best
// (include/cddp_hip.h "scoring candidate control sequences").  Plain functions, host and device, no other header needed: the selection
// kernel of inst_score.hip runs it one lane per trajectory, tests/cpp/test_score_select.cpp compiles this file with g++ and checks it on
// hand-built records.
//
//   finite      cost and viol are both finite
//   admissible  finite and viol <= viol_tol
//   winner      the admissible candidate of lowest cost; when none is admissible the finite candidate of lowest viol, then of lowest
//               cost; ties go to the lowest index; -1 when no candidate is finite
#pragma once

#if defined(__HIPCC__)
#define CDDP_SCORE_HD __host__ __device__ __forceinline__
#else
#define CDDP_SCORE_HD inline
#endif

namespace cddp_score {

// false for NaN and +-Inf (x - x is 0 exactly for every finite x, NaN otherwise)
CDDP_SCORE_HD bool finite(double v) { return v - v == 0.0; }

// cost[c], viol[c] for c < ncand; viol == nullptr: every violation is 0
CDDP_SCORE_HD int select(int ncand, const double *cost, const double *viol, double viol_tol) {
  int best = -1;
  bool best_adm = false;
  double best_cost = 0.0, best_viol = 0.0;
  for (int c = 0; c < ncand; ++c) {
    const double jc = cost[c], vc = viol ? viol[c] : 0.0;
    if (!finite(jc) || !finite(vc)) continue;
    const bool adm = vc <= viol_tol;
    bool better;
    if (best < 0) better = true;
    else if (adm != best_adm) better = adm;
    else if (adm) better = jc < best_cost;
    else better = vc < best_viol || (vc == best_viol && jc < best_cost);
    if (better) { best = c; best_adm = adm; best_cost = jc; best_viol = vc; }
  }
  return best;
}

// the candidate the handle is seeded from: the winner, or candidate 0 when none is finite
CDDP_SCORE_HD int seed_index(int winner) { return winner < 0 ? 0 : winner; }

}  // namespace cddp_score
