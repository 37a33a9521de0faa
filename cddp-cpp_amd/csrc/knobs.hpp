// The CDDP_HIP_* environment switches of the resident solver (capi.hip, launch.hpp).  Constructing a Knobs reads them: cddp_hip_create
// makes ONE per handle, so its kernel route, ladder rules and group plan are fixed properties of the handle.  Host only.
// (The stack-fed handle, stacks.hip, and the plug-in route, plugin_solve.hip, keep their own switches.)
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

namespace cddp_dev {

inline char env_first(const char *name) { const char *e = std::getenv(name); return e ? e[0] : 0; }   // first character of the value, 0 if unset
inline bool env_is(const char *name, const char *v) { const char *e = std::getenv(name); return e && !std::strcmp(e, v); }
inline int env_num(const char *name, int dflt, int lo, int hi) { const char *e = std::getenv(name); const int n = e ? std::atoi(e) : dflt; return (n >= lo && n <= hi) ? n : dflt; }
inline long env_long(const char *name, long dflt) { const char *e = std::getenv(name); return e ? std::atol(e) : dflt; }
inline std::string env_str(const char *name) { const char *e = std::getenv(name); return e ? e : ""; }

struct Knobs {
  enum Sweep { kSweepCoop, kSweepLane, kSweepElem, kSweepMfma };
  // kernel route (launch.hpp::Launcher::route).  SWEEP=lane | elem | mfma: one-lane / element-ownership / matrix-core sweeps (else cooperative)
  int sweep = env_is("CDDP_HIP_SWEEP", "lane") ? kSweepLane : env_is("CDDP_HIP_SWEEP", "elem") ? kSweepElem : env_is("CDDP_HIP_SWEEP", "mfma") ? kSweepMfma : kSweepCoop;
  bool t4 = env_first("CDDP_HIP_T4") != '0';                     // T4=0: wave-tiled instead of sub-tile-minor stacks for the G = 16 sweeps
  int sweep_roles = env_num("CDDP_HIP_SWEEP_ROLES", 1, 0, 2);    // helper wavefronts of the role-split IPDDP sweep, 0 | 1 | 2
  bool coop_h2 = env_first("CDDP_HIP_COOP_H") == '2';            // COOP_H=2: the nx > 8 one-wave sweep with two lanes per column
  bool coop_w1 = env_first("CDDP_HIP_COOP_W") == '1';            // COOP_W=1: the nx > 8 sweep on one wavefront instead of two
  int k4_na = env_num("CDDP_HIP_K4_NA", 1, 1, 3);                // step sizes per rollout workgroup of the small path-constrained layouts
  bool k4_consumers2 = env_first("CDDP_HIP_K4_CONSUMERS") == '2';   // two consumer waves in the IPDDP rollout where instantiated
  // Time-sliced wave priority of the two-role IPDDP rollout (capi.hip::roll_slice_for; kernels_lean.hpp::k_forward_ipddp_pc_sl, cart-pole and
  // unicycle layouts).  K4_SLICE_US unset: on the launches whose running waves exceed the SIMDs of the stream's share of the chip, early- and
  // late-placed workgroups take wave priority 3 in alternating windows of 2.56 us (capi.hip, kK4SliceUs; chosen from the sweep of
  // profiles/r17_simd_sharing.md section 3: 1.28 / 2.56 / 5.12 / 10.24 / 20.48 us -> 35.68 / 35.59 / 36.21 / 36.74 / 36.80 ms per C2 solve, off 37.11);
  // 0: off; n: a window of about n us (rounded to a power of two of 10-ns ticks) on every launch (the tests)
  int k4_slice_us = env_num("CDDP_HIP_K4_SLICE_US", -1, 0, 10000);
  bool k4_late_prio = env_first("CDDP_HIP_K4_LATE_PRIO") == '1';    // comparison row: a fixed priority 3 for the late-placed workgroups instead of the window
  bool ms_lane_rollout = env_is("CDDP_HIP_MS_ROLLOUT", "lane");  // the one-wave MSIPDDP rollout
  bool lg_lane_rollout = env_is("CDDP_HIP_LG_ROLLOUT", "lane");  // the one-wave LogDDP rollout
  // solve loop (capi.hip::SolveRun)
  bool graph = env_first("CDDP_HIP_GRAPH") == '1';               // capture the iterations between two polls into hipGraphs, replay them
  char ls_stages = env_first("CDDP_HIP_LS_STAGES");              // '1' | '2': pin the one-stage / two-stage line-search ladder
  int ls_first = env_num("CDDP_HIP_LS_FIRST", 0, INT_MIN, INT_MAX);   // step sizes of stage 1 (used for 1 <= k < ladder length)
  long ls_two_max_waves = env_long("CDDP_HIP_LS_TWO_MAX_WAVES", 768);   // largest first stage (wavefronts) a two-stage ladder keeps
  int ls_small_frac = env_num("CDDP_HIP_LS_SMALL_FRAC", 3, 1, INT_MAX);   // one stage when more than 1 / n of a small ladder is needed
  int ls_margin = env_num("CDDP_HIP_LS_MARGIN", -1, 0, 8);       // step sizes added to the histogram's first-stage count (unset, -1: 0 where both stages run in one rollout launch, else 1)
  bool ls_inkernel = env_first("CDDP_HIP_LS_INKERNEL") != '0';   // LS_INKERNEL=0: a two-stage ladder is always two rollout launches (capi.hip::SolveRun::inkernel_stages)
  int ls_poll_us = env_num("CDDP_HIP_TEST_LS_POLL_US", -1, 0, INT_MAX);   // test hook: the stage-2 poll's give-up bound in microseconds (0: give up at once; unset: kLsPollUs)
  int run_ahead = env_num("CDDP_HIP_RUNAHEAD", 1, 0, 16);        // iterations enqueued behind a poll before the host waits for it
  int poll_every = env_num("CDDP_HIP_POLL_EVERY", 4, 1, INT_MAX);   // iterations between two "anything still running?" polls
  bool event_fence = env_first("CDDP_HIP_EVENT_FENCE") == '1';   // class-timing events with the default (system-scope fence) flags
  bool debug_ladder = std::getenv("CDDP_HIP_DEBUG_LADDER") != nullptr;   // print each ladder decision to stderr
  // group plan and device buffers (capi.hip::pick_groups, cu_spec_for_group, in_create)
  int groups = env_num("CDDP_HIP_GROUPS", 0, INT_MIN, INT_MAX);  // n > 0: n tile groups, all in flight at once
  bool chunking = env_num("CDDP_HIP_CHUNK", 1, INT_MIN, INT_MAX) > 0;   // CHUNK <= 0: never cut a large batch into chunks
  int chunk = env_num("CDDP_HIP_CHUNK", 0, 1, INT_MAX);          // trajectories per chunk (0: the automatic size)
  int partition = env_num("CDDP_HIP_PARTITION", 0, 1, 16);       // CU slices per chunk, a divisor of 256 (0: the default)
  bool cumask_set = std::getenv("CDDP_HIP_CUMASK") != nullptr;   // CUMASK set at all, even empty: no default partition
  std::string cumask = env_str("CDDP_HIP_CUMASK");               // "<spec>[|<spec> ...]": explicit CU plan per group (capi.hip::parse_cu_spec)
  bool pingpong = env_first("CDDP_HIP_PINGPONG") == '1';         // two groups whose rollouts alternate
  bool xcd_map = env_first("CDDP_HIP_XCD_MAP") != '0';           // XCD_MAP=0: no XCD-aware block -> tile map of the G = 16 sweeps
  int fail_costate = env_num("CDDP_HIP_TEST_FAIL_COSTATE", 0, INT_MIN, INT_MAX);   // test hook: DevBuf::fail_costate_mask
  // K4b schedule (capi.hip::shadow_eligible): COSTATE=sync: the costate kernel on the iteration's chain everywhere; COSTATE=shadow: deferred
  // into the next sweep launch on every eligible layout; unset: deferred where the sweep launch leaves a second workgroup place free on its CUs (shadow_eligible)
  enum Costate { kCostateAuto, kCostateSync, kCostateShadow };
  int costate = env_is("CDDP_HIP_COSTATE", "sync") ? kCostateSync : env_is("CDDP_HIP_COSTATE", "shadow") ? kCostateShadow : kCostateAuto;
  int fail_shadow = env_num("CDDP_HIP_TEST_FAIL_SHADOW", 0, 1, INT_MAX);   // test hook: the deferred costate of that outer iteration reports "not finite" (DevBuf::cs_fail_stamp)
};

}  // namespace cddp_dev
