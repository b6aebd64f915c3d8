// sdc_mpc_schedule.hpp -- the decision schedule of sdc_rollout_cem_stats (sdc_capi.hip): for every step of the call, whether the
// planner plans or idles, over how many steps, whether it starts afresh or from the carried result moved up by a step, and which draw
// it uses.  No HIP, no handle: integers in, integers out, so that a host compiler alone can build and test it
// (tests/test_mpc_schedule.py).  The contract: include/sustaindc_hip.h.
//
// THE RULE is the Python agent's (dc_rl_amd/agents.py _mpc_horizon, CEMMPCAgent._start), word for word.  With `left` the steps the
// episode has left before the step (sdc_steps_to_episode_end):
//   K = min(horizon, auto_reset ? left - 1 : left)      the planner does not look across an episode's end, and with auto-reset the
//                                                        episode's last step would reset the envs and kill the mark
//   planned  iff  left >= 2 && K >= 1;  otherwise the decision is IDLE: idle_action is played, no draw is consumed, and the carried
//                                                        distribution is dropped
//   a planned decision starts FRESH (uniform probs, best_seq = idle_action) when warm_start == 0, when nothing is carried -- the
//   call's first planned decision without `resume`, the decision behind an idle one -- and when K exceeds the steps the carried result
//   has; otherwise from the carried result SHIFTED: steps 0 .. K - 2 take steps 1 .. K - 1, step K - 1 is uniform / idle_action
//   the j-th planned decision of the call uses draw + j (mod 2^32)
// A planned decision's result of K steps is what the next one carries.
#pragma once

struct SdcMpcDecision {
  int steps;            // K of a planned decision, 0 of an idle one
  int planned;          // 1: plan over `steps` steps; 0: idle
  int fresh;            // a planned decision: 1 fresh, 0 shifted
  unsigned draw_index;  // a planned decision: j, the number of planned decisions of the call before it
};

struct SdcMpcSchedule {
  int horizon, warm_start, auto_reset;
  int carried;       // steps of the result the next decision may start from (0: none)
  unsigned planned;  // planned decisions so far

  // resume_steps: the steps of the caller's unshifted result of an earlier decision (0: none, the first planned decision starts fresh)
  SdcMpcSchedule(const int horizon_, const int warm_start_, const int auto_reset_, const int resume_steps)
      : horizon(horizon_), warm_start(warm_start_), auto_reset(auto_reset_), carried(resume_steps), planned(0) {}

  // the decision before a step with `left` steps to the episode's end; the schedule moves on by that step
  SdcMpcDecision next(const int left) {
    const int reach = auto_reset ? left - 1 : left;
    const int K = horizon < reach ? horizon : reach;
    SdcMpcDecision d = {0, 0, 0, 0};
    if (!(left >= 2 && K >= 1)) {
      carried = 0;
      return d;
    }
    d.steps = K;
    d.planned = 1;
    d.fresh = (!warm_start || carried == 0 || K > carried) ? 1 : 0;
    d.draw_index = planned++;
    carried = K;
    return d;
  }
};

// the planned decisions among the n_steps steps of a call that starts with `left` steps to the episode's end (n_steps <= left)
inline unsigned sdc_mpc_planned(const int horizon, const int auto_reset, const int left, const int n_steps) {
  SdcMpcSchedule S(horizon, 1, auto_reset, 0);
  for (int t = 0; t < n_steps; t++) (void)S.next(left - t);
  return S.planned;
}
