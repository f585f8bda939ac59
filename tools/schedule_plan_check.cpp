// Stand-alone check of the step launch's schedule plan (csrc/hs_schedule.h), built with
// -fsanitize=address,undefined (make asan-schedule-plan) and run by tests/test_schedule_plan.py.  The
// expectations are written out from the documented rule, not computed by the function under test.
//   schedule_plan_check       -> one line per check, "ok ..." or "FAIL ...", exit status 0 / 1
#include <cstdio>
#include <numeric>

#include "hs_schedule.h"

namespace {

using hs::schedule_plan;
using hs::SchedulePlan;
constexpr int AUTO = hs::SCHED_AUTO, DIRECT = hs::SCHED_DIRECT, SINGLE = hs::SCHED_SINGLE, FIXED = hs::SCHED_FIXED_ORDER;
constexpr int STEP = hs::MODE_ENV_STEP, RESET = hs::MODE_RESET, PHYSICS = hs::MODE_PHYSICS;

int fails = 0;
long checks = 0;
void expect(bool ok, const char* what, int R, int nenv) {
  checks++;
  if (!ok && fails++ < 20) std::printf("FAIL %s R=%d nenv=%d\n", what, R, nenv);
}

// an env step (one launch step, no rollout) with the queue buffers and no hook
SchedulePlan step(int schedule, int nsub, int nenv, int R) { return schedule_plan(schedule, STEP, nsub, 1, false, nenv, R, true, 0); }

// env steps around the boundaries of one resident count
void check_env_steps(int R) {
  for (int nsub : {2, 3, 5}) {
    // every env has a wave of its own: single, not queued
    SchedulePlan p = step(AUTO, nsub, R, R);
    expect(p.valid && !p.queue && p.single && p.units == R && p.grid == R && p.wide, "nenv = R: single", R, R);
    // the pairs fit the resident waves (npairs <= R): paired, not queued
    for (int n : {R + 1, 2 * R}) {
      p = step(AUTO, nsub, n, R);
      expect(p.valid && !p.queue && !p.single && p.units == (n + 1) / 2 && p.grid == (n + 1) / 2 && p.wide,
             "R < nenv <= 2R: paired", R, n);
    }
    // more pairs than resident waves: the chunk queue, a grid of R, pair units
    for (int n : {2 * R + 1, 2 * R + 2}) {
      for (int sched : {AUTO, FIXED}) {
        p = step(sched, nsub, n, R);
        expect(p.valid && p.queue && !p.single && p.units == (n + 1) / 2 && p.grid == R && p.wide,
               "nenv > 2R, nsub >= 2: queued, grid R", R, n);
        expect(p.qorder == (sched == AUTO ? 1 : 0), "qorder only for SCHED_AUTO", R, n);
      }
    }
  }
  // the same sizes are never queued with one substep, SCHED_DIRECT, SCHED_SINGLE, MODE_RESET, without the queue
  // buffers or without a resident count
  for (int n : {R, R + 1, 2 * R, 2 * R + 1, 2 * R + 2}) {
    const int npairs = (n + 1) / 2;
    SchedulePlan p = step(AUTO, 1, n, R);
    expect(p.valid && !p.queue && p.single == (n <= R) && p.grid == (n <= R ? n : npairs), "nsub = 1: not queued", R, n);
    p = step(DIRECT, 3, n, R);
    expect(p.valid && !p.queue && !p.single && p.grid == npairs && p.qorder == 0, "SCHED_DIRECT: paired", R, n);
    p = step(SINGLE, 3, n, R);
    expect(p.valid && !p.queue && p.single && p.grid == n && p.qorder == 0, "SCHED_SINGLE: single", R, n);
    p = schedule_plan(AUTO, RESET, 3, 1, false, n, R, true, 0);
    expect(p.valid && !p.queue && p.single == (n <= R), "MODE_RESET: not queued", R, n);
    p = schedule_plan(AUTO, STEP, 3, 1, false, n, R, false, 0);
    expect(p.valid && !p.queue && p.single == (n <= R), "no queue buffers: not queued", R, n);
    p = schedule_plan(AUTO, STEP, 3, 1, false, n, 0, true, 0);
    expect(p.valid && !p.queue && !p.single && p.grid == npairs, "R = 0: paired, not queued", R, n);
    expect(step(AUTO, 3, n, R).wide_grid == (npairs < 32 ? npairs : 32), "wide grid min(npairs, 32)", R, n);
  }
  // a physics call queues like an env step
  SchedulePlan p = schedule_plan(AUTO, PHYSICS, 4, 1, false, 2 * R + 2, R, true, 0);
  expect(p.valid && p.queue && p.grid == R, "MODE_PHYSICS, nenv > 2R: queued", R, 2 * R + 2);
}

// tape launches (nsteps = 2, or a rollout of one step): always queued
void check_tapes(int R) {
  for (int n : {1, R, R + 1, 2 * R, 2 * R + 1, 2 * R + 2}) {
    for (int rollout = 0; rollout < 2; rollout++) {
      const int nsteps = rollout ? 1 : 2, npairs = (n + 1) / 2;
      for (int sched : {AUTO, FIXED, DIRECT, SINGLE}) {
        for (int nsub : {1, 3}) {
          const SchedulePlan p = schedule_plan(sched, STEP, nsub, nsteps, rollout != 0, n, R, true, 0);
          // single envs when every env fits a resident wave (the schedules that may queue), else pairs
          const bool single = n <= R && (sched == AUTO || sched == FIXED);
          const int units = single ? n : npairs;
          expect(p.valid && p.queue && p.single == (single ? 1 : 0) && p.units == units, "tape: queued, its unit", R, n);
          expect(p.grid == (R < units ? R : units), "tape: grid min(R, units)", R, n);
          expect(!p.wide, "tape: no wide launch", R, n);
          expect(p.qorder == (sched == AUTO ? 1 : 0), "tape: qorder only for SCHED_AUTO", R, n);
          expect(p.nsteps == nsteps, "tape: nsteps", R, n);
        }
      }
      expect(!schedule_plan(AUTO, STEP, 3, nsteps, rollout != 0, n, R, false, 0).valid, "tape without queue buffers", R, n);
      expect(!schedule_plan(AUTO, STEP, 3, nsteps, rollout != 0, n, 0, true, 0).valid, "tape with R = 0", R, n);
      expect(!schedule_plan(AUTO, RESET, 3, nsteps, rollout != 0, n, R, true, 0).valid, "tape in MODE_RESET", R, n);
      expect(!schedule_plan(AUTO, PHYSICS, 3, nsteps, rollout != 0, n, R, true, 0).valid, "tape in MODE_PHYSICS", R, n);
    }
    expect(schedule_plan(AUTO, STEP, 3, hs::QTAG_STEPS, false, n, R, true, 0).valid, "tape of QTAG_STEPS steps", R, n);
    expect(!schedule_plan(AUTO, STEP, 3, hs::QTAG_STEPS + 1, false, n, R, true, 0).valid, "tape of QTAG_STEPS + 1 steps", R, n);
    expect(!schedule_plan(AUTO, STEP, 3, hs::QTAG_STEPS + 1, true, n, R, true, 0).valid, "rollout of QTAG_STEPS + 1 steps", R, n);
  }
  // a step count below 1 is one step
  const SchedulePlan p = schedule_plan(AUTO, STEP, 3, 0, false, R, R, true, 0);
  expect(p.valid && p.nsteps == 1 && !p.queue && p.single, "nsteps < 1 is an env step", R, R);
}

// the fallback permutation: coprime to the unit count, at least 1; one unit gives 1
void check_qmul() {
  // nenv = 2 units envs queue `units` pairs with R = 1 ... except units = 1, which a tape launch of one env queues
  for (int units = 1; units <= 4100; units++) {
    const SchedulePlan p = units == 1 ? schedule_plan(AUTO, STEP, 3, 2, false, 1, 1, true, 0)
                                      : schedule_plan(AUTO, STEP, 3, 1, false, 2 * units, 1, true, 0);
    expect(p.valid && p.queue && p.units == units, "qmul case is queued", 1, units);
    expect(p.qmul >= 1 && std::gcd(p.qmul, units) == 1, "gcd(qmul, units) = 1", 1, units);
    if (units == 1) expect(p.qmul == 1, "one unit: qmul 1", 1, units);
    // the same count as the single units of a small tape launch
    const SchedulePlan t = schedule_plan(AUTO, STEP, 3, 2, false, units, 4100, true, 0);
    expect(t.valid && t.single && t.units == units && t.qmul == p.qmul, "qmul depends on the unit count alone", 4100, units);
  }
  expect(step(AUTO, 3, 64, 1024).qmul == 1 && step(DIRECT, 3, 4098, 1024).qmul == 1, "not queued: qmul 1", 1024, 64);
}

// the lost-hand-off hook: env e + 1 becomes pair e / 2 + 1 for pair units and stays e + 1 for single units
void check_hook(int R) {
  for (int e : {0, 1, 2, 5, 2 * R, 2 * R + 1}) {
    const SchedulePlan q = schedule_plan(AUTO, STEP, 3, 1, false, 2 * R + 2, R, true, e + 1);
    expect(q.queue && q.dbg_lose_pair1 == e / 2 + 1, "hook, pair units (queued env step)", R, e);
    const SchedulePlan t = schedule_plan(AUTO, STEP, 3, 2, false, 2 * R + 2, R, true, e + 1);
    expect(t.queue && !t.single && t.dbg_lose_pair1 == e / 2 + 1, "hook, pair units (tape)", R, e);
  }
  for (int e : {0, 1, R - 1}) {
    if (e < 0 || e >= R) continue;
    const SchedulePlan t = schedule_plan(AUTO, STEP, 3, 2, false, R, R, true, e + 1);
    expect(t.queue && t.single && t.dbg_lose_pair1 == e + 1, "hook, single units (small tape)", R, e);
  }
  expect(step(AUTO, 3, 2 * R + 2, R).dbg_lose_pair1 == 0, "hook off stays 0", R, 0);
}

}  // namespace

int main() {
  for (int R : {1, 7, 1024, 2048}) {
    const long before = checks;
    const int f0 = fails;
    check_env_steps(R);
    check_tapes(R);
    check_hook(R);
    std::printf("%s R=%d checks=%ld\n", fails == f0 ? "ok" : "FAIL", R, checks - before);
  }
  const long before = checks;
  const int f0 = fails;
  check_qmul();
  std::printf("%s qmul units=1..4100 checks=%ld\n", fails == f0 ? "ok" : "FAIL", checks - before);
  return fails ? 1 : 0;
}
