// Reward programs (include/hsim.h hs_reward_program_*): a user's reward function, traced once in Python
// (reward_program.py) into a flat, branch-free instruction list, evaluated for every env of a batch by
// reward_program_kernel (hs_reward_prog.hip) or on the host in double (rp_eval_host below).
// This header is the one definition of the opcode table, the limits, one op's arithmetic (host and
// device, the same expression) and the validator; it compiles as plain C++ too (tools/reward_prog_check.cpp).
//
// Encoding: n_instr x (op, dst, a, b, c) int32, n_consts float64 constants, n_params float64 parameter
// slots supplied at every call.  Values live in numbered slots (the tracer allocates them by liveness);
// dst is the slot an instruction writes, a / b / c the slots it reads, except:
//   RP_CONST  a = constant index      RP_PARAM  a = parameter index
//   RP_LOAD   a = field (RP_F_*), b = the flat index within the env's row of that field
//   RP_RESULT a = the slot holding the reward; exactly one, the last instruction
//   RP_OUT    a = the slot holding a named component of the reward, b = the component's index; writes no
//             slot, may stand anywhere before RP_RESULT; a program created with n_outputs components holds
//             exactly one RP_OUT per index in [0, n_outputs)
// Comparisons and the logical ops give 1 or 0; RP_WHERE and the logical ops read "not zero" as true.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RP_HD __host__ __device__
#else
#define RP_HD
#endif

namespace hs {

// the limits (include/hsim.h HS_RP_MAX_*); a program is bounded by its LIVE values, not its length
constexpr int RP_MAX_INSTR = 4096, RP_MAX_SLOTS = 64, RP_MAX_CONSTS = 256, RP_MAX_PARAMS = 32, RP_MAX_OUTPUTS = 16;

enum RpOp : int32_t {
  RP_CONST = 0, RP_PARAM, RP_LOAD,
  RP_ADD, RP_SUB, RP_MUL, RP_DIV, RP_ATAN2, RP_LT, RP_LE, RP_GT, RP_GE, RP_EQ, RP_NE, RP_AND, RP_OR,   // binary
  RP_NEG, RP_ABS, RP_SQRT, RP_EXP, RP_LOG, RP_SIN, RP_COS, RP_TANH, RP_ASIN, RP_ACOS, RP_NOT,          // unary
  RP_WHERE,                                                                                             // ternary
  RP_RESULT,
  RP_OUT,                                                                                               // a component
  RP_NOPS
};

// the env_data fields a program may read, and the row each is indexed within
enum RpField : int32_t {
  RP_F_QPOS = 0,   // [nq]
  RP_F_QVEL,       // [nv]
  RP_F_CTRL,       // [nu]
  RP_F_TIME,       // [1]
  RP_F_QFRC,       // qfrc_actuator [nv]
  RP_F_CINERT,     // [nbody][10]
  RP_F_CVEL,       // [nbody][6]
  RP_F_COM,        // subtree_com[0] [3] (the root's row: what the aux row holds)
  RP_F_CFRC,       // cfrc_ext [nbody][6]
  RP_F_LINVEL,     // subtree_linvel [nbody][3]
  RP_NFIELDS,      // the fields a caller supplies as arrays: the members of hs_reward_fields
  // the reference motion's sample at the env's own (episode, time) -- see "reference motion" below: no array of
  // the caller's, computed from the bound rows; read with RP_LOAD like any field.  A block of its own at 16: the
  // ids from RP_NFIELDS to 15 stay unknown fields, left for state fields to come
  RP_F_REF_QPOS = 16,   // [nq]
  RP_F_REF_QVEL,        // [nv]
  RP_NFIELDS_ALL
};
inline bool rp_field_known(int f) { return (f >= 0 && f < RP_NFIELDS) || f == RP_F_REF_QPOS || f == RP_F_REF_QVEL; }
constexpr unsigned RP_REF_FIELDS = (1u << RP_F_REF_QPOS) | (1u << RP_F_REF_QVEL);

struct RpDims { int nq, nv, nu, nbody; };

inline int rp_field_len(const RpDims& d, int f) {
  switch (f) {
    case RP_F_QPOS: return d.nq;
    case RP_F_QVEL: return d.nv;
    case RP_F_CTRL: return d.nu;
    case RP_F_TIME: return 1;
    case RP_F_QFRC: return d.nv;
    case RP_F_CINERT: return 10 * d.nbody;
    case RP_F_CVEL: return 6 * d.nbody;
    case RP_F_COM: return 3;
    case RP_F_CFRC: return 6 * d.nbody;
    case RP_F_LINVEL: return 3 * d.nbody;
    case RP_F_REF_QPOS: return d.nq;
    case RP_F_REF_QVEL: return d.nv;
  }
  return 0;
}

// slots an op reads (0 for RP_CONST / RP_PARAM / RP_LOAD, whose operands are indices; RP_RESULT and RP_OUT read one)
RP_HD inline int rp_arity(int op) {
  if (op >= RP_ADD && op <= RP_OR) return 2;
  if ((op >= RP_NEG && op <= RP_NOT) || op == RP_RESULT || op == RP_OUT) return 1;
  if (op == RP_WHERE) return 3;
  return 0;
}

// tanh of the host interpreter goes through long double where that is wider: the C library's double tanh
// is 1.23 ulp off near |x| = 1e-3 (its documented bound is 2 ulp), and the host interpreter is the device
// code's reference, held to 1 ulp of the exact value for every libm op (tests/test_program_ops.py).  The
// device's tanh is its own libm's (tests/test_gpu_program_ops.py measures it).
template <typename T>
RP_HD inline T rp_tanh(T a) {
#if !defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == sizeof(double) && sizeof(long double) > sizeof(double))
    return (T)tanhl((long double)a);
#endif
  return tanh(a);
}

// One op's arithmetic: each a single operation (or one libm call) of T, never contracted, so a program
// rounds exactly as the same expression written out in reward_formula.  + - * are correctly rounded in
// both dtypes, / and sqrt in double; the DEVICE's float / and sqrt are not: the kernel is built with the
// fp32 engine's flags (Makefile KFLAGS, <= 2.5 ulp; measured 1.45 and 0.80 ulp), which is what makes a
// restated built-in equal reward_formula bitwise.  The device's libm is within 1.1 ulp in double and 2.3
// ulp in float (profiles/reward_programs.md, "Op conformance"; tests/test_gpu_program_ops.py).
// A comparison with a NaN is false (RP_NE: true); RP_WHERE selects, both arms are always evaluated.
// (always inlined: the kernel's two instances, with and without reference fields, would otherwise share one
// out-of-line copy, a call per instruction)
template <typename T>
RP_HD inline __attribute__((always_inline)) T rp_op(int op, T a, T b, T c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  switch (op) {
    case RP_ADD: return a + b;
    case RP_SUB: return a - b;
    case RP_MUL: return a * b;
    case RP_DIV: return a / b;
    case RP_ATAN2: return atan2(a, b);
    case RP_LT: return a < b ? T(1) : T(0);
    case RP_LE: return a <= b ? T(1) : T(0);
    case RP_GT: return a > b ? T(1) : T(0);
    case RP_GE: return a >= b ? T(1) : T(0);
    case RP_EQ: return a == b ? T(1) : T(0);
    case RP_NE: return a != b ? T(1) : T(0);
    case RP_AND: return (a != T(0) && b != T(0)) ? T(1) : T(0);
    case RP_OR: return (a != T(0) || b != T(0)) ? T(1) : T(0);
    case RP_NEG: return -a;
    case RP_ABS: return fabs(a);
    case RP_SQRT: return sqrt(a);
    case RP_EXP: return exp(a);
    case RP_LOG: return log(a);
    case RP_SIN: return sin(a);
    case RP_COS: return cos(a);
    case RP_TANH: return rp_tanh(a);
    case RP_ASIN: return asin(a);
    case RP_ACOS: return acos(a);
    case RP_NOT: return a != T(0) ? T(0) : T(1);
    case RP_WHERE: return a != T(0) ? b : c;
  }
  return T(0);
}

// What validation learns about a program.
struct RpInfo {
  int n_slots = 0;        // highest slot written + 1
  unsigned fields = 0;    // bit f set: the program reads field f
  int n_outputs = 0;      // named components (RP_OUT); 0: the program has the reward alone
};

// Validate an encoding against the limits and a model's dimensions.  Returns "" and fills `info`, or
// the reason a program is refused: nothing that fails here is ever uploaded or launched.
// n_outputs: the components the program is created with -- every index in [0, n_outputs) written by exactly one
// RP_OUT (so with 0 any RP_OUT is refused).
inline std::string rp_validate(const RpDims& d, const int32_t* code, int n_instr, const double* consts,
                               int n_consts, int n_params, int n_outputs, RpInfo* info) {
  auto at = [](int i) { return " (instruction " + std::to_string(i) + ")"; };
  if (n_instr < 1 || n_instr > RP_MAX_INSTR)
    return "reward program: " + std::to_string(n_instr) + " instructions, the limit is " + std::to_string(RP_MAX_INSTR);
  if (n_consts < 0 || n_consts > RP_MAX_CONSTS)
    return "reward program: " + std::to_string(n_consts) + " constants, the limit is " + std::to_string(RP_MAX_CONSTS);
  if (n_params < 0 || n_params > RP_MAX_PARAMS)
    return "reward program: " + std::to_string(n_params) + " parameters, the limit is " + std::to_string(RP_MAX_PARAMS);
  if (n_outputs < 0 || n_outputs > RP_MAX_OUTPUTS)
    return "reward program: " + std::to_string(n_outputs) + " outputs, the limit is " + std::to_string(RP_MAX_OUTPUTS);
  if (!code || (n_consts > 0 && !consts)) return "reward program: null code or constants";
  bool written[RP_MAX_SLOTS] = {};
  bool out_written[RP_MAX_OUTPUTS] = {};
  RpInfo r;
  r.n_outputs = n_outputs;
  for (int i = 0; i < n_instr; i++) {
    const int32_t* in = code + 5 * (size_t)i;
    const int op = in[0], dst = in[1];
    if (op < 0 || op >= RP_NOPS) return "reward program: unknown opcode " + std::to_string(op) + at(i);
    if (op == RP_RESULT && i != n_instr - 1) return "reward program: a result before the last instruction" + at(i);
    if (op != RP_RESULT && i == n_instr - 1) return "reward program: missing result (the last instruction must be the result)";
    const int ar = rp_arity(op);
    for (int k = 0; k < ar; k++) {
      const int s = in[2 + k];
      if (s < 0 || s >= RP_MAX_SLOTS)
        return "reward program: slot " + std::to_string(s) + " out of range [0, " + std::to_string(RP_MAX_SLOTS) + ")" + at(i);
      if (!written[s]) return "reward program: slot " + std::to_string(s) + " is read before it is written" + at(i);
    }
    if (op == RP_CONST && (in[2] < 0 || in[2] >= n_consts))
      return "reward program: constant index " + std::to_string(in[2]) + " out of range" + at(i);
    if (op == RP_PARAM && (in[2] < 0 || in[2] >= n_params))
      return "reward program: parameter index " + std::to_string(in[2]) + " out of range" + at(i);
    if (op == RP_LOAD) {
      if (!rp_field_known(in[2])) return "reward program: unknown field " + std::to_string(in[2]) + at(i);
      if (in[3] < 0 || in[3] >= rp_field_len(d, in[2]))
        return "reward program: field index " + std::to_string(in[3]) + " outside the model's dimensions (field " +
               std::to_string(in[2]) + " has " + std::to_string(rp_field_len(d, in[2])) + " values)" + at(i);
      r.fields |= 1u << in[2];
    }
    if (op == RP_OUT) {
      const int c = in[3];
      if (c < 0 || c >= n_outputs)
        return "reward program: output index " + std::to_string(c) + " outside [0, " + std::to_string(n_outputs) +
               "): the program has " + std::to_string(n_outputs) + " outputs" + at(i);
      if (out_written[c]) return "reward program: output " + std::to_string(c) + " is written twice" + at(i);
      out_written[c] = true;
    }
    if (op == RP_RESULT || op == RP_OUT) continue;
    if (dst < 0 || dst >= RP_MAX_SLOTS)
      return "reward program: slot " + std::to_string(dst) + " out of range [0, " + std::to_string(RP_MAX_SLOTS) + ")" + at(i);
    written[dst] = true;
    if (dst + 1 > r.n_slots) r.n_slots = dst + 1;
  }
  for (int c = 0; c < n_outputs; c++)
    if (!out_written[c]) return "reward program: output " + std::to_string(c) + " is never written (no out instruction)";
  if (info) *info = r;
  return "";
}

// a program with the reward alone (n_outputs = 0)
inline std::string rp_validate(const RpDims& d, const int32_t* code, int n_instr, const double* consts,
                               int n_consts, int n_params, RpInfo* info) {
  return rp_validate(d, code, n_instr, consts, n_consts, n_params, 0, info);
}

// -- reference motion (include/hsim.h hs_set_reference_motion) ------------------------------------
// K rows qpos [K][nq] / qvel [K][nv], key_dt seconds apart.  ref_qpos / ref_qvel of an env are the rows'
// linear interpolation at the env's phase x = j0 + time / key_dt: a pure function of (seed, env, episode, time)
// and the bound table, so nothing is carried between steps.  The one definition, shared by the kernel and the
// host interpreter and restated in numpy (reference_motion.sample).
constexpr int RP_REF_HOLD = 0, RP_REF_LOOP = 1;              // past the last row: stay on it / start over
constexpr int RP_REF_START_ZERO = 0, RP_REF_START_DRAWN = 2; // j0 = 0 / the row the episode's initial state drew
constexpr int RP_REF_MAX_ROWS = 4096;
constexpr int RP_REF_INIT_SLOT = 128;                        // hs_env_step.h INIT_SLOT

// the step kernels' counter hash (hs_env_step.h splitmix / bank_row), restated so that this unit does not
// include theirs: the bank row the reset of (seed, env, episode) drew, min(K - 1, floor(u K))
RP_HD inline uint64_t rp_splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
RP_HD inline int rp_bank_row(uint64_t seed, int env, uint32_t ep, int K) {
  const uint64_t h =
      rp_splitmix(seed ^ rp_splitmix(((uint64_t)env << 32) ^ ((uint64_t)ep << 8) ^ (uint64_t)RP_REF_INIT_SLOT));
  const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);   // [0, 1)
  const int j = (int)(u * (double)K);
  return j < K - 1 ? j : K - 1;
}

// The start row: 0, or with RP_REF_START_DRAWN the initial-state draw's own row (episode 0 was never reset: 0).
RP_HD inline int rp_ref_start(int flags, uint64_t seed, int env, int32_t episode, int K) {
  if (!(flags & RP_REF_START_DRAWN) || episode == 0) return 0;
  return rp_bank_row(seed, env, (uint32_t)episode, K);
}

// The phase of one env: the two rows *i, *i1 in [0, K - 1] for EVERY input (NaN, +-inf, 1e300) and the weight
// of the second in [0, 1).  Always in double, also for a float batch: the float build's divide is not correctly
// rounded (Makefile KFLAGS) and the row index must not depend on that.  K == 1: the row itself, key_dt ignored.
RP_HD inline double rp_ref_phase(int K, int flags, int j0, double time, double key_dt, int* i, int* i1) {
  if (K <= 1) {
    *i = *i1 = 0;
    return 0.0;
  }
  double x = (double)j0 + time / key_dt;
  if (!(x >= 0.0)) x = 0.0;                         // NaN or negative
  if (flags & RP_REF_LOOP) {
    if (!(x < 4503599627370496.0)) x = 4503599627370496.0;   // 2^52: beyond it a double has no fraction to index by
    const double f = floor(x);
    const int r = (int)((int64_t)f % (int64_t)K);
    *i = r;
    *i1 = r + 1 < K ? r + 1 : 0;
    return x - f;
  }
  if (!(x < (double)(K - 1))) x = (double)(K - 1);
  const double f = floor(x);
  const int r = (int)f;
  *i = r;
  *i1 = r + 1 < K ? r + 1 : K - 1;
  return x - f;
}

// The value: a + w (b - a), each operation rounded in T, never contracted; w == 0 gives a.  Quaternion components
// are interpolated like any other coordinate and NOT renormalised: a program divides by the norm where it matters.
template <typename T>
RP_HD inline T rp_ref_value(T a, T b, T w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T d = b - a;
  const T s = w * d;
  return a + s;
}

// What the host interpreter samples a reference from: the rows as doubles (of a float batch: float values),
// per-state episode numbers and seeds, the env index of state e (env ? env[e] : env_base + e); `fp32`: the
// sample is computed in float, as a float batch's kernel does, and widened.  The time is the state's own time field.
struct RpRefHost {
  int K = 0;
  const double* qpos = nullptr;   // [K][nq]
  const double* qvel = nullptr;   // [K][nv], or NULL: zeros
  double key_dt = 0;
  int flags = 0;
  bool fp32 = false;
  const int32_t* episode = nullptr;
  const uint64_t* seed = nullptr;
  const int32_t* env = nullptr;
  int env_base = 0;
};

inline double rp_ref_load_host(const RpDims& d, const RpRefHost& ref, int field, int index, int i, int i1, double w) {
  const bool pos = field == RP_F_REF_QPOS;
  const double* rows = pos ? ref.qpos : ref.qvel;
  if (!rows) return 0.0;
  const size_t ld = (size_t)(pos ? d.nq : d.nv);
  const double a = rows[(size_t)i * ld + index], b = rows[(size_t)i1 * ld + index];
  if (ref.fp32) return (double)rp_ref_value<float>((float)a, (float)b, (float)w);
  return rp_ref_value<double>(a, b, w);
}

// The host interpreter: a VALIDATED program on n states in double.  field[f]: [n][rp_field_len(d, f)]
// contiguous doubles, or NULL for a field the program does not read (checked by the caller).  comp_out: the
// component sink, component-major [n_outputs][n] (component c of state e at c * n + e), or NULL: RP_OUT is then
// a no-op.  ref: the reference motion, for a program that reads ref_qpos / ref_qvel (the caller has checked that
// it is there, with the time field, episode and seed).
inline void rp_eval_host(const RpDims& d, const int32_t* code, int n_instr, const double* consts, const double* params,
                         int n, const double* const* field, double* out, double* comp_out = nullptr,
                         const RpRefHost* ref = nullptr) {
  int len[RP_NFIELDS];
  for (int f = 0; f < RP_NFIELDS; f++) len[f] = rp_field_len(d, f);
  for (int e = 0; e < n; e++) {
    double v[RP_MAX_SLOTS];
    double res = 0;
    int ri = 0, ri1 = 0;
    double rw = 0;
    if (ref) {
      int j0 = 0;   // (episode and seed are needed, and read, for a drawn start only)
      if (ref->flags & RP_REF_START_DRAWN)
        j0 = rp_ref_start(ref->flags, ref->seed[e], ref->env ? ref->env[e] : ref->env_base + e, ref->episode[e], ref->K);
      rw = rp_ref_phase(ref->K, ref->flags, j0, field[RP_F_TIME][e], ref->key_dt, &ri, &ri1);
      if (ref->fp32) rw = (double)(float)rw;
    }
    for (int i = 0; i < n_instr; i++) {
      const int32_t* in = code + 5 * (size_t)i;
      const int op = in[0];
      double r;
      if (op == RP_CONST) r = consts[in[2]];
      else if (op == RP_PARAM) r = params[in[2]];
      else if (op == RP_LOAD && in[2] >= RP_NFIELDS) r = ref ? rp_ref_load_host(d, *ref, in[2], in[3], ri, ri1, rw) : 0.0;
      else if (op == RP_LOAD) r = field[in[2]][(size_t)e * len[in[2]] + in[3]];
      else if (op == RP_RESULT) { res = v[in[2]]; break; }
      else if (op == RP_OUT) {
        if (comp_out) comp_out[(size_t)in[3] * n + e] = v[in[2]];
        continue;
      } else {
        const int ar = rp_arity(op);
        r = rp_op<double>(op, v[in[2]], ar > 1 ? v[in[3]] : 0.0, ar > 2 ? v[in[4]] : 0.0);
      }
      v[in[1]] = r;
    }
    out[e] = res;
  }
}

// -- termination conditions (include/hsim.h hs_set_termination) ----------------------------------
// A predicate is a program whose value is read as a truth value: it holds iff the value is non-zero and
// not NaN (a comparison with a NaN is already 0; a bare NaN value does not terminate either).
template <typename T>
RP_HD inline bool rp_truth(T v) { return v != T(0) && v == v; }

// The grace counter of one env (custom_env.py:169-180 without its reward scaling): the number of consecutive
// env steps of the CURRENT episode at which the predicate has held.  It is stored with the episode number it
// belongs to and reads as 0 when that differs from the env's current one, so every kind of reset clears it
// without the reset kernels knowing.  Returns the new count (saturating); *early = the episode ends now.
RP_HD inline int32_t rp_grace_update(int32_t stored_count, int32_t stored_episode, int32_t episode, bool holds,
                                     int32_t grace_steps, bool* early) {
  const int32_t prev = stored_episode == episode ? stored_count : 0;
  const int32_t count = holds ? (prev < INT32_MAX ? prev + 1 : prev) : 0;
  *early = count >= grace_steps;
  return count;
}

// The host path: a VALIDATED predicate and the grace update on n states in double.  count / episode_tag
// [n] are read and updated in place, episode [n] is each env's current episode number; early [n] out.
inline void rp_termination_eval_host(const RpDims& d, const int32_t* code, int n_instr, const double* consts,
                                     const double* params, int grace_steps, int n, const double* const* field,
                                     const int32_t* episode, int32_t* count, int32_t* episode_tag, uint8_t* early,
                                     const RpRefHost* ref = nullptr) {
  for (int e = 0; e < n; e++) {
    const double* one[RP_NFIELDS];
    for (int f = 0; f < RP_NFIELDS; f++) one[f] = field[f] ? field[f] + (size_t)e * rp_field_len(d, f) : nullptr;
    double v = 0;
    RpRefHost r1;   // state e's slice of the reference's per-state arrays
    if (ref) {
      r1 = *ref;
      if (ref->episode) r1.episode = ref->episode + e;
      if (ref->seed) r1.seed = ref->seed + e;
      if (ref->env) r1.env = ref->env + e;
      r1.env_base = ref->env_base + e;
    }
    rp_eval_host(d, code, n_instr, consts, params, 1, one, &v, nullptr, ref ? &r1 : nullptr);
    bool ends = false;
    count[e] = rp_grace_update(count[e], episode_tag[e], episode[e], rp_truth(v), grace_steps, &ends);
    episode_tag[e] = episode[e];
    early[e] = ends ? 1 : 0;
  }
}

#if defined(__HIPCC__)
// One encoded program as the kernel sees it: code / consts on the device, the parameters by value.
// n_instr = 0: none.
struct RpCode {
  const int32_t* code;
  const double* consts;
  int n_instr;
  double params[RP_MAX_PARAMS];
};

// reward_program_kernel's arguments.  field[f] is the base of field f and ld[f] its env stride in
// values (a NULL field reads as 0: cfrc_ext / subtree_linvel without HS_FULL_STATE).  outcome = 0:
// out[env] = the reward program's value.  outcome = 1 (hs_step_program, hs_step with a termination set,
// hs_apply_termination; after a step without auto-reset): the env step's outcome rows, see the kernel --
// `prog` the reward program or none (the step kernel's reward stays), `pred` the termination predicate or none.
// The reference motion as the kernel sees it (the batch's, hs_set_reference_motion).  K = 0: the launch's programs
// read no reference field -- the host sets K only from their field masks, and launch_reward_program then runs the
// kernel instance that has no phase prologue and no reference load: the code a launch ran before the feature.
template <typename T>
struct RpRef {
  const T* q;                 // [K][nq]
  const T* v;                 // [K][nv]
  int K, flags, nq, nv;
  double key_dt;
  uint64_t seed;
  const T* time;              // [n]
  const int32_t* episode;     // [n]
};

template <typename T>
struct RpArgs {
  RpCode prog, pred;
  int n_slots, n, outcome;          // n_slots: the larger of the two programs'
  const T* field[RP_NFIELDS];
  long long ld[RP_NFIELDS];
  T* out;
  // the component rows, component-major [n_outputs][n] (one RP_OUT is one coalesced store of the wave), or NULL:
  // RP_OUT is then a no-op.  Outcome mode: the step's values (0 for a truncated env), with comp_total the
  // episode's running sums, comp_episode [n] the episode number the sums belong to (they read as 0 when it
  // differs from episode[env]: the grace counter's idiom) and term_comp_total the sums of the envs done this step
  T* comp;
  T* comp_total;
  int32_t* comp_episode;
  T* term_comp_total;
  int n_outputs;
  // outcome mode: the batch's rows
  T* reward;
  T* total_reward;
  uint8_t* terminated;
  const uint8_t* truncated;
  const T* obs;
  T* terminal_obs;
  int obs_dim;
  const int32_t* step_count;
  int32_t* term_step_count;
  T* term_total_reward;
  uint8_t* done;
  // the env's episode number (with a predicate or component rows); with a predicate: the grace counter and its
  // episode tag, the early byte
  const int32_t* episode;
  int32_t* grace_count;
  int32_t* grace_episode;
  uint8_t* early;
  int grace_steps;
  // the reference motion, for programs that read ref_qpos / ref_qvel (last: every other member keeps its offset)
  RpRef<T> ref;
};

template <typename T>
hipError_t launch_reward_program(const RpArgs<T>& a, hipStream_t stream);
#endif

}  // namespace hs
