// The selection rule of cddp_hip_seed_best (cddp-cpp_amd/csrc/score_select.hpp) on hand-built records, as a program of its own: the header
// is plain C++ that a host compiler reads, so the rule is checked here without a device -- and under the address and undefined-behaviour
// sanitizers (tests/test_score_select_cpp.py builds this file with -fsanitize=address,undefined).  The records are those of
// tests/test_score_rollouts.py::hand_built_records, where the selection KERNEL is held to the same winners.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../cddp-cpp_amd/csrc/score_select.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static int pick(std::vector<double> cost, std::vector<double> viol, double tol) {
  // exact-size heap arrays: a read past candidate S - 1 is an error the address sanitizer reports
  return cddp_score::select((int)cost.size(), cost.data(), viol.empty() ? nullptr : viol.data(), tol);
}

// the rule written out the long way: two passes, no running state
static int pick_ref(const std::vector<double> &cost, const std::vector<double> &viol, double tol) {
  const int S = (int)cost.size();
  auto v = [&](int c) { return viol.empty() ? 0.0 : viol[c]; };
  int best = -1;
  for (int c = 0; c < S; ++c) {
    if (!std::isfinite(cost[c]) || !std::isfinite(v(c)) || !(v(c) <= tol)) continue;
    if (best < 0 || cost[c] < cost[best]) best = c;
  }
  if (best >= 0) return best;
  for (int c = 0; c < S; ++c) {
    if (!std::isfinite(cost[c]) || !std::isfinite(v(c))) continue;
    if (best < 0 || v(c) < v(best) || (v(c) == v(best) && cost[c] < cost[best])) best = c;
  }
  return best;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  EXPECT(pick({3.0, 3.0, 3.0}, {0.0, 0.0, 0.0}, 0.0) == 0);                 // all tied: the lowest index
  EXPECT(pick({5.0, 2.0, 2.0}, {0.0, 0.0, 0.0}, 0.0) == 1);                 // a tie of the lowest cost: the lower index
  EXPECT(pick({nan, 4.0, 6.0}, {0.0, 0.0, 0.0}, 0.0) == 1);                 // a NaN cost loses
  EXPECT(pick({1.0, 2.0, 3.0}, {0.5, 0.2, 0.2}, 0.0) == 1);                 // none admissible: lowest viol, then lowest cost
  EXPECT(pick({nan, inf, 1.0}, {0.0, 0.0, nan}, 0.0) == -1);                // none finite
  EXPECT(pick({1.0, 2.0, 3.0}, {0.05, 0.0, 0.0}, 0.0) == 1);                // viol_tol changes the winner ...
  EXPECT(pick({1.0, 2.0, 3.0}, {0.05, 0.0, 0.0}, 0.1) == 0);                // ... from 1 to 0
  EXPECT(pick({-inf, 2.0, 3.0}, {0.0, 0.3, 0.0}, 0.0) == 2);                // -inf is not finite
  EXPECT(pick({1.0, 2.0, 3.0}, {inf, 0.4, 0.4}, 0.0) == 1);                 // an infinite violation loses; tie of viol: the lower cost
  EXPECT(pick({1.0, 2.0}, {}, 0.0) == 0);                                   // viol == nullptr: all 0
  EXPECT(pick({7.0}, {9.0}, 0.0) == 0 && pick({nan}, {0.0}, 0.0) == -1);    // S = 1
  EXPECT(pick({2.0, 1.0}, {0.0, 0.0}, nan) == 1);                           // a NaN tolerance admits nothing: lowest viol, then cost
  EXPECT(cddp_score::seed_index(-1) == 0 && cddp_score::seed_index(4) == 4);
  EXPECT(!cddp_score::finite(nan) && !cddp_score::finite(inf) && !cddp_score::finite(-inf) && cddp_score::finite(0.0) && cddp_score::finite(-1e308));
  // a sweep of small records over a value set with ties and non-finite entries against the two-pass statement
  const double vals[] = {0.0, 1.0, 1.0, 2.0, nan, inf, -1.0};
  const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
  long checked = 0;
  for (int S = 1; S <= 3; ++S) {
    int total = 1;
    for (int k = 0; k < 2 * S; ++k) total *= nv;
    for (int code = 0; code < total; ++code) {
      std::vector<double> cost(S), viol(S);
      int r = code;
      for (int c = 0; c < S; ++c) { cost[c] = vals[r % nv]; r /= nv; viol[c] = vals[r % nv]; r /= nv; }
      for (double tol : {0.0, 1.0}) { EXPECT(pick(cost, viol, tol) == pick_ref(cost, viol, tol)); ++checked; }
      if (fails > 5) return 1;
    }
  }
  if (fails == 0) std::printf("score select: ok (%ld swept records)\n", checked);
  return fails == 0 ? 0 : 1;
}
