"""The step launch's schedule plan (csrc/hs_schedule.h: schedule_plan) on the host.

tools/schedule_plan_check.cpp is a stand-alone program built with -fsanitize=address,undefined (make
asan-schedule-plan).  For resident wave counts R in {1, 7, 1024, 2048} it asserts, from the documented rule and
not from the function itself: R envs run one per wave, R + 1 and 2R envs in pairs, 2R + 1 and 2R + 2 envs on the
chunk queue with a grid of R (two substeps or more; never with one substep, HS_SCHED_DIRECT, HS_SCHED_SINGLE, a
reset, without the queue buffers or with R = 0); a tape launch (two steps, or a rollout of one) is always queued,
by single envs when they fit the resident waves, with a grid of min(R, units) and no wide launch after it, and
is refused without the queue buffers, with R = 0, outside env-step mode or past QTAG_STEPS steps; the wide grid
is min(npairs, 32); the claims are cost-ordered only under HS_SCHED_AUTO; the fallback permutation's multiplier
is coprime to every unit count in 1 .. 4100; the lost-hand-off hook names the pair of its env, or the env itself
for single units.  No GPU needed.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_plan_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mujocoposelearning_amd", "csrc"),
                           "asan-schedule-plan"])
    exe = os.path.join(ROOT, "build", "asan", "schedule_plan_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5 and all(l.startswith("ok ") for l in lines), r.stdout
    assert [l.split()[1] for l in lines] == ["R=1", "R=7", "R=1024", "R=2048", "qmul"], r.stdout
