// The schedule of one step launch as a pure host function (plain C++17, no HIP): launch_step
// follows it, hs_batch_schedule and hs_debug_queue_order report it, tools/schedule_plan_check.cpp checks it.
#pragma once
#include <algorithm>
#include <cstdint>

namespace hs {

enum StepMode { MODE_ENV_STEP = 0, MODE_RESET = 1, MODE_PHYSICS = 2 };
// hs_env_config.schedule (SCHED_FIXED_ORDER: AUTO with the chunk queue's claims in the fixed
// permutation instead of cost order -- A/B runs and tests)
enum Schedule { SCHED_AUTO = 0, SCHED_DIRECT = 1, SCHED_SINGLE = 2, SCHED_FIXED_ORDER = 3 };
constexpr int QTAG_STEPS = 511;   // most env steps per tape launch (the hand-off tags, hs_kernels.h qtag)

struct SchedulePlan {
  bool valid;   // false: the launch is refused (hipErrorInvalidValue)
  int nsteps;   // env steps per launch, at least 1
  int queue, single, qorder, qmul, dbg_lose_pair1;   // StepParams' members of these names
  int units;    // what a wave steps, and the chunk queue's unit: envs (single) or env pairs
  int grid;     // the resident tier's grid; a queue instance caps it at the waves it holds (queue_waves)
  int wide_grid;
  bool wide;    // a wide-tier launch follows the resident tier's (never a tape launch)
};

// resident: the waves of the resident step kernel the device holds at once (<= 0: unknown); queue_bufs: the
// batch has its hand-off rows and sync words (EnvBuffers::mid, qsync); lose_env1: the lost-hand-off test hook,
// env + 1 or 0
inline SchedulePlan schedule_plan(int schedule, int mode, int nsub, int nsteps, bool rollout, int nenv, int resident,
                                  bool queue_bufs, int lose_env1) {
  SchedulePlan s{};
  s.nsteps = std::max(nsteps, 1);
  // chunk-queue schedule when the env pairs outnumber the waves the GPU holds at once (the fp64
  // engine: 1 wave per SIMD), for multi-substep calls (HS_SCHED_DIRECT: never)
  const int npairs = (nenv + 1) / 2;
  const bool may_queue = schedule == SCHED_AUTO || schedule == SCHED_FIXED_ORDER;
  s.queue = may_queue && queue_bufs && mode != MODE_RESET && nsub >= 2 && resident > 0 && npairs > resident;
  // tape launch (several env steps of an action tape; a fused rollout is one even for one step): always the
  // chunk queue, with whole env steps as items, whatever the batch size -- a pair's next env step starts as soon
  // as its own previous one is committed, so the steps of different pairs overlap
  const bool tape = s.nsteps > 1 || rollout;
  if (tape) {
    if (mode != MODE_ENV_STEP || !queue_bufs || resident <= 0 || s.nsteps > QTAG_STEPS) return s;
    s.queue = 1;
  }
  // a tape launch of a small batch (every env fits a resident wave of its own) queues single envs, not pairs:
  // twice the waves, each env's steps back to back
  const bool qsingle = tape && may_queue && nenv <= resident;
  // single-env schedule: one wave per env (the upper half-wave a ghost of the lower) when every env gets a
  // resident wave of its own -- small batches would otherwise leave SIMDs idle with one wave per env pair
  s.single = qsingle || (!s.queue && (schedule == SCHED_SINGLE ||
                                      (schedule == SCHED_AUTO && resident > 0 && nenv <= resident)));
  s.units = s.single ? nenv : npairs;
  s.qorder = schedule == SCHED_AUTO;
  // fallback claim order (first queued launch, SCHED_FIXED_ORDER): a fixed multiplicative permutation of the
  // units (the same for both chunk kinds, so a pair's last substep is still claimed npairs items after its first
  // chunk), so that items whose cost is correlated with the env index are spread over the launch
  s.qmul = 1;
  if (s.queue) {
    auto gcd = [](uint32_t a, uint32_t b) { while (b) { uint32_t t = a % b; a = b; b = t; } return a; };
    uint32_t q = (uint32_t)(0.6180339887 * s.units) | 1u;
    while (gcd(q, (uint32_t)s.units) != 1u) q += 2;
    s.qmul = (int)(q % (uint32_t)s.units == 0 ? 1 : q);
  }
  // the lost-hand-off test hook names an env (+ 1); the kernel compares it with its queue unit
  s.dbg_lose_pair1 = (lose_env1 > 0 && !qsingle) ? (lose_env1 - 1) / 2 + 1 : lose_env1;
  s.grid = s.queue && !tape ? resident : s.queue ? std::min(resident, s.units) : s.units;
  // the wide tier's grid: enough waves for a few deferred envs at once, few enough that the common no-overflow
  // launch (every wave reads the count and exits) costs a few microseconds
  s.wide_grid = std::min(npairs, 32);
  s.wide = !tape;
  s.valid = true;
  return s;
}

}  // namespace hs
