// The two built-in termination conditions (reward_program.py `fallen` / `lost_balance`, custom_env.py:167-200)
// as ONE function of the env's qpos row, for the step kernel's fused TERM instances (hs_env_step.h
// env_outcome), for hs_set_termination_builtin's probe-table check of a predicate program against it, and
// for the host (hs_termination_builtin_eval_host, tools/term_builtin_check.cpp).  The interpreter
// (hs_reward_prog.h) stays the yardstick: a batch's program and its built-in are the same predicate, and the
// fused instances end an episode at the step the per-step path ends it.  Compiles as plain C++ too.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "hs_reward_prog.h"

namespace hs {

// include/hsim.h HS_TERM_* (static_assert in hs_api.cpp)
enum TermKind : int32_t { TERM_NONE = 0, TERM_FALLEN = 1, TERM_LOST_BALANCE = 2 };

// Does the condition hold on the state whose qpos row is `qpos` (qpos[2] the height, qpos[3..6] the root
// quaternion w, x, y, z)?  Each expression in the association of reward_program.py (`fallen`,
// `lost_balance`, quaternion_to_euler) and never contracted, so the value compared is the interpreter's, op
// for op.  A comparison with a NaN is false: the unclamped pitch (|2 (w y - z x)| > 1 -> asin = NaN) does
// not terminate.  Roll and pitch are computed for TERM_LOST_BALANCE only (the kind is wave-uniform).
template <typename T>
RP_HD inline bool term_builtin_holds(int kind, T min_height, T max_roll_pitch, const T* qpos) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool holds = qpos[2] < min_height;
  if (kind == TERM_LOST_BALANCE) {
    const T w = qpos[3], x = qpos[4], y = qpos[5], z = qpos[6];
    const T roll = atan2(T(2) * (w * x + y * z), T(1) - T(2) * (x * x + y * y));
    const T pitch = asin(T(2) * (w * y - z * x));
    holds = holds || fabs(roll) > max_roll_pitch || fabs(pitch) > max_roll_pitch;
  }
  return holds;
}

// The probe rows hs_set_termination_builtin evaluates both on: heights either side of min_height (upright),
// quaternions tilted either side of max_roll_pitch in roll and in pitch (well above min_height, both signs),
// four tilted far (1.5 and 3 rad: whatever max_roll_pitch is, and it means nothing to TERM_FALLEN, a program
// that looks at the orientation at all shows here), and one quaternion with |2 (w y - z x)| > 1 and no roll, whose NaN pitch must not terminate.
// out: [TERM_NPROBE][5] = qpos[2..6].
constexpr int TERM_NPROBE = 4 + 8 + 4 + 1;
inline void term_probe_rows(double min_height, double max_roll_pitch, double (*out)[5]) {
  int n = 0;
  auto put = [&](double h, double w, double x, double y, double z) {
    out[n][0] = h; out[n][1] = w; out[n][2] = x; out[n][3] = y; out[n][4] = z;
    n++;
  };
  for (double d : {-0.05, -1e-6, 1e-6, 0.05}) put(min_height + d, 1.0, 0.0, 0.0, 0.0);
  const double up = min_height + 0.5;
  for (double sign : {1.0, -1.0})
    for (double d : {-0.02, 0.02}) {
      const double a = 0.5 * sign * (max_roll_pitch + d);
      put(up, std::cos(a), std::sin(a), 0.0, 0.0);   // roll
      put(up, std::cos(a), 0.0, std::sin(a), 0.0);   // pitch
    }
  put(up, std::cos(0.75), std::sin(0.75), 0.0, 0.0);     // roll 1.5
  put(up, std::cos(0.75), 0.0, -std::sin(0.75), 0.0);    // pitch -1.5
  put(up, std::cos(1.5), -std::sin(1.5), 0.0, 0.0);      // roll -3
  put(up, std::cos(0.75), 0.0, std::sin(0.75), 0.0);     // pitch 1.5
  put(up, 0.9, 0.0, 0.6, 0.0);   // 2 w y = 1.08: pitch NaN; roll = atan2(0, 0.28) = 0
}

// The check: `code` (a VALIDATED predicate that reads qpos only) against the built-in on the probe rows.
// Returns the index of the first row whose truth values differ, or -1 when all agree.
inline int term_probe_mismatch(const RpDims& d, const int32_t* code, int n_instr, const double* consts,
                               const double* params, int kind, double min_height, double max_roll_pitch) {
  double rows[TERM_NPROBE][5];
  term_probe_rows(min_height, max_roll_pitch, rows);
  const int nq = d.nq;
  if (nq < 7) return 0;
  std::vector<double> q((size_t)nq, 0.0);
  for (int i = 0; i < TERM_NPROBE; i++) {
    for (int k = 0; k < 5; k++) q[2 + k] = rows[i][k];
    const double* field[RP_NFIELDS] = {};
    field[RP_F_QPOS] = q.data();
    double v = 0;
    rp_eval_host(d, code, n_instr, consts, params, 1, field, &v);
    if (rp_truth(v) != term_builtin_holds<double>(kind, min_height, max_roll_pitch, q.data())) return i;
  }
  return -1;
}

}  // namespace hs
