// hsim C ABI: rewards and episode ends evaluated on the device outside the step kernel -- the built-in rewards
// on given state (hs_reward_eval, hs_reward), reward programs with their named components, and termination
// conditions (hs_reward_prog.h, hs_term_builtin.h).
#include "hs_api_batch.h"
#include "hs_term_builtin.h"

static_assert(HS_RP_MAX_INSTR == hs::RP_MAX_INSTR && HS_RP_MAX_SLOTS == hs::RP_MAX_SLOTS &&
                  HS_RP_MAX_CONSTS == hs::RP_MAX_CONSTS && HS_RP_MAX_PARAMS == hs::RP_MAX_PARAMS &&
                  HS_RP_MAX_OUTPUTS == hs::RP_MAX_OUTPUTS,
              "include/hsim.h reward program limits");
static_assert(sizeof(hs_reward_fields) == hs::RP_NFIELDS * sizeof(void*), "hs_reward_fields: one pointer per field");
static_assert(HS_REF_HOLD == hs::RP_REF_HOLD && HS_REF_LOOP == hs::RP_REF_LOOP &&
                  HS_REF_START_ZERO == hs::RP_REF_START_ZERO && HS_REF_START_DRAWN == hs::RP_REF_START_DRAWN &&
                  HS_MAX_REFERENCE_ROWS == hs::RP_REF_MAX_ROWS,
              "include/hsim.h reference motion flags");
static_assert(HS_TERM_FALLEN == hs::TERM_FALLEN && HS_TERM_LOST_BALANCE == hs::TERM_LOST_BALANCE, "built-in kinds");

namespace {
using hs::by_precision;
using hs::DeviceGuard;
using hs::fail;
using hs::hip_ok;
using hs::hip_rc;
using hs::order_streams;

// what hs_reward_eval and hs_reward fill alike: the reward, the row count, the model's dimensions and the
// kneeling parameters
template <typename T>
hs::RewardEvalArgs<T> reward_eval_args(const hs::HostModel& h, int reward_id, int n, const double* kneel) {
  hs::RewardEvalArgs<T> a{};
  a.reward_id = reward_id;
  a.n = n;
  a.nq = h.nq;
  a.nv = h.nv;
  a.nu = h.nu;
  a.nbody = h.nbody;
  for (int k = 0; k < 9; k++) a.kneel[k] = kneel[k];
  return a;
}

// -- reward programs (hs_reward_prog.h) --------------------------------------------------------
const char* const kRpFieldNames[hs::RP_NFIELDS_ALL] = {
    "qpos", "qvel", "ctrl", "time", "qfrc_actuator", "cinert", "cvel", "subtree_com[0]", "cfrc_ext", "subtree_linvel",
    "", "", "", "", "", "",   // (ids 10 .. 15: no field)
    "ref_qpos", "ref_qvel"};
static_assert(hs::RP_F_REF_QPOS == 16 && hs::RP_NFIELDS_ALL == 18, "kRpFieldNames follows RpField");

// the reference field a program reads, by name ("" when it reads none)
std::string rp_ref_field_read(const hs_reward_program* p) {
  for (int k = hs::RP_F_REF_QPOS; k < hs::RP_NFIELDS_ALL; k++)
    if (p->info.fields & (1u << k)) return kRpFieldNames[k];
  return "";
}

// every field the program (`noun`: "program" / "predicate") reads must be given; `who`: the entry point's name.
// A reference field has no member of hs_reward_fields: with_ref tells whether the entry point was given a reference
int rp_check_fields(const char* who, const char* noun, const hs_reward_program* p, const hs_reward_fields* f,
                    bool with_ref = false) {
  const void* const* fp = reinterpret_cast<const void* const*>(f);
  if (!with_ref && (p->info.fields & hs::RP_REF_FIELDS))
    return fail(std::string(who) + ": the " + noun + " reads " + rp_ref_field_read(p) +
                ", a sample of a reference motion, which hs_reward_fields does not carry: evaluate it on a batch with "
                "one bound (hs_set_reference_motion; hs_reward_program_batch, hs_step_program) or on the host with "
                "hs_reward_program_eval_host_reference");
  for (int k = 0; k < hs::RP_NFIELDS; k++)
    if ((p->info.fields & (1u << k)) && !fp[k])
      return fail(std::string(who) + ": the " + noun + " reads " + kRpFieldNames[k] + ", which is NULL");
  return 0;
}

// the program's code and constants on `device` (uploaded on first use there; hs_reward_program_create
// uploads to the device current at the time, so a later launch -- possibly under graph capture -- allocates nothing)
const hs_reward_program::Dev* rp_resident(const hs_reward_program* prog, int device) {
  auto* p = const_cast<hs_reward_program*>(prog);
  std::lock_guard<std::mutex> lk(p->mu);
  for (auto& d : p->dev)
    if (d.device == device) return &d;
  DeviceGuard g(device);
  hs_reward_program::Dev d{device, nullptr, nullptr};
  const size_t cb = p->code.size() * sizeof(int32_t), kb = std::max<size_t>(p->consts.size(), 1) * sizeof(double);
  if (!hip_ok(hipMalloc((void**)&d.code, cb), "hipMalloc(reward program)") ||
      !hip_ok(hipMalloc((void**)&d.consts, kb), "hipMalloc(reward program)") ||
      !hip_ok(hipMemcpy(d.code, p->code.data(), cb, hipMemcpyHostToDevice), "reward program upload") ||
      (!p->consts.empty() &&
       !hip_ok(hipMemcpy(d.consts, p->consts.data(), p->consts.size() * sizeof(double), hipMemcpyHostToDevice),
               "reward program upload"))) {
    if (d.code) (void)hipFree(d.code);
    if (d.consts) (void)hipFree(d.consts);
    return nullptr;
  }
  p->dev.push_back(d);
  return &p->dev.back();
}

hs::RpCode rp_code(const hs_reward_program* p, const hs_reward_program::Dev* d, const double* params) {
  hs::RpCode c{};
  c.code = d->code;
  c.consts = d->consts;
  c.n_instr = (int)(p->code.size() / 5);
  for (int k = 0; k < p->n_params; k++) c.params[k] = params[k];
  return c;
}

template <typename T>
hs::RpArgs<T> rp_args(const hs_reward_program* p, const hs_reward_program::Dev* d, const double* params, int n) {
  hs::RpArgs<T> a{};
  a.prog = rp_code(p, d, params);
  a.n_slots = p->info.n_slots;
  a.n = n;
  return a;
}

// the batch's own buffers as a program's fields: cinert / cvel / qfrc_actuator are the obs row's
// (custom_env.py:242-256), subtree_com[0] the aux row's; cfrc_ext / subtree_linvel read as zeros
// unless HS_FULL_STATE, as the built-in rewards see them (mj_step leaves them uncomputed)
template <typename T>
void rp_batch_fields(const hs_batch* b, hs::RpArgs<T>& a) {
  const hs::HostModel& h = b->model->host;
  const int o2 = (h.nq - 2) + h.nv, o3 = o2 + 10 * h.nbody, o4 = o2 + 16 * h.nbody;
  auto set = [&](int f, const void* p, long long ld) { a.field[f] = (const T*)p; a.ld[f] = ld; };
  set(hs::RP_F_QPOS, b->buf.qpos, h.nq);
  set(hs::RP_F_QVEL, b->buf.qvel, h.nv);
  set(hs::RP_F_CTRL, b->buf.ctrl, h.nu);
  set(hs::RP_F_TIME, b->buf.time, 1);
  set(hs::RP_F_QFRC, (const T*)b->buf.obs + o4, b->obs_dim);
  set(hs::RP_F_CINERT, (const T*)b->buf.obs + o2, b->obs_dim);
  set(hs::RP_F_CVEL, (const T*)b->buf.obs + o3, b->obs_dim);
  set(hs::RP_F_COM, (const T*)b->buf.aux + hs::MAXDOF, hs::AUXDIM);
  set(hs::RP_F_CFRC, b->full_state ? b->buf.cfrc_ext : nullptr, 6 * h.nbody);
  set(hs::RP_F_LINVEL, b->full_state ? b->buf.subtree_linvel : nullptr, 3 * h.nbody);
}

// the batch's reference motion for a launch whose programs read `fields`: set only when one of them reads a
// reference field (rp_check_batch has checked that it is bound), so that any other launch is what it was
template <typename T>
void rp_batch_ref(const hs_batch* b, unsigned fields, hs::RpArgs<T>& a) {
  if (!(fields & hs::RP_REF_FIELDS)) return;
  a.ref.q = (const T*)b->ref_q;
  a.ref.v = (const T*)b->ref_v;
  a.ref.K = b->ref_n;
  a.ref.flags = b->ref_flags;
  a.ref.nq = b->model->host.nq;
  a.ref.nv = b->model->host.nv;
  a.ref.key_dt = b->ref_key_dt;
  a.ref.seed = b->seed;
  a.ref.time = (const T*)b->buf.time;
  a.ref.episode = (const int32_t*)b->buf.episode;
}

// what a program needs of a batch before anything is launched; `stepped`: the check runs ahead of the
// step that will write the outputs (hs_step_program), so a stale data.ctrl does not matter
int rp_check_batch(const char* who, const hs_batch* b, const hs_reward_program* p, const double* params, bool stepped) {
  const std::string w(who);
  if (!b || !p) return fail(w + ": null argument");
  if (p->n_params > 0 && !params) return fail(w + ": the program has parameters, params must not be NULL");
  const hs::HostModel& h = b->model->host;
  if (p->dims.nq != h.nq || p->dims.nv != h.nv || p->dims.nu != h.nu || p->dims.nbody != h.nbody)
    return fail(w + ": the program was compiled for a model of other dimensions");
  const unsigned f = p->info.fields;
  if ((f & (1u << hs::RP_F_CTRL)) && (!(b->cfg.outputs & HS_OUT_CTRL) || (!stepped && b->ctrl_stale)))
    return fail(w + ": the program reads ctrl, which needs the data.ctrl copy (HS_OUT_CTRL) written by the last step");
  if ((f & (1u << hs::RP_F_COM)) && !(b->cfg.outputs & HS_OUT_AUX))
    return fail(w + ": the program reads subtree_com, which needs the aux row (HS_OUT_AUX) written by the last step");
  if (b->full_state && (f & ((1u << hs::RP_F_CFRC) | (1u << hs::RP_F_LINVEL))) &&
      (!b->buf.cfrc_ext || !b->buf.subtree_linvel))
    return fail(w + ": the batch has no cfrc_ext / subtree_linvel buffers");
  if (f & hs::RP_REF_FIELDS) {
    if (b->ref_n <= 0)
      return fail(w + ": the program reads " + rp_ref_field_read(p) +
                  ", but the batch has no reference motion bound (hs_set_reference_motion)");
    if ((b->ref_flags & HS_REF_START_DRAWN) && b->init_n != b->ref_n)
      return fail(w + ": the reference motion starts at the drawn row (HS_REF_START_DRAWN), which needs a bank of "
                  "initial states of the same " + std::to_string(b->ref_n) + " rows bound (hs_set_initial_states); " +
                  (b->init_n > 0 ? "the bank bound has " + std::to_string(b->init_n) : std::string("none is bound")));
  }
  return 0;
}

// The outcome launch on the batch's post-step, pre-reset state (hs_reward_prog.hip): the reward program `p`
// if there is one, the batch's termination predicate if one is set, the terminal rows and the done bytes.
// One launch; the caller has checked the batch and ordered the streams.
int outcome_launch(hs_batch* b, const hs_reward_program* p, const double* params, void* stream) {
  const hs_reward_program* t = b->term_prog;
  const hs_reward_program::Dev* dp = p ? rp_resident(p, b->device) : nullptr;
  const hs_reward_program::Dev* dt = t ? rp_resident(t, b->device) : nullptr;
  if ((p && !dp) || (t && !dt)) return -1;
  return by_precision(b->precision, [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RpArgs<T> a{};
    if (p) a.prog = rp_code(p, dp, params);
    if (t) a.pred = rp_code(t, dt, b->term_params);
    a.n_slots = std::max(p ? p->info.n_slots : 1, t ? t->info.n_slots : 1);
    a.n = b->n;
    rp_batch_fields<T>(b, a);
    rp_batch_ref<T>(b, (p ? p->info.fields : 0u) | (t ? t->info.fields : 0u), a);
    a.outcome = 1;
    a.reward = (T*)b->buf.reward;
    a.total_reward = (T*)b->buf.total_reward;
    a.terminated = b->buf.terminated;
    a.truncated = b->buf.truncated;
    a.obs = (const T*)b->buf.obs;
    a.terminal_obs = (T*)b->buf.terminal_obs;
    a.obs_dim = b->obs_dim;
    a.step_count = b->buf.step_count;
    a.term_step_count = b->buf.terminal_step_count;
    a.term_total_reward = (T*)b->buf.terminal_total_reward;
    a.done = b->prog_done;
    a.episode = (const int32_t*)b->buf.episode;
    if (p && b->comp_n > 0) {   // (the counts agree: step_outcome_reset checks before the step)
      a.comp = (T*)b->comp;
      a.comp_total = (T*)b->comp_total;
      a.comp_episode = b->comp_episode;
      a.term_comp_total = (T*)b->term_comp_total;
      a.n_outputs = b->comp_n;
    }
    if (t) {
      a.grace_count = b->grace_count;
      a.grace_episode = b->grace_episode;
      a.early = b->early;
      a.grace_steps = b->grace_steps;
    }
    return hip_rc(hs::launch_reward_program<T>(a, (hipStream_t)stream), "reward_program_kernel");
  });
}

// A reference row's free-joint quaternion divided by its norm; false for a zero one.  Never contracted: the
// expression numpy evaluates (initial_state.normalize_quaternions), bit for bit, so that the host can state the
// rows the device holds (HsBatch.reference_motion) and a sample of them exactly.
bool ref_normalize_quat(double* r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ww = r[3] * r[3], xx = r[4] * r[4], yy = r[5] * r[5], zz = r[6] * r[6];
  const double norm = std::sqrt(((ww + xx) + yy) + zz);
  if (!(norm >= 1e-15)) return false;
  for (int c = 3; c < 7; c++) r[c] = r[c] / norm;
  return true;
}

// The flags of a reference motion, checked (`who`: the entry point's name).
int ref_check_flags(const std::string& who, int flags) {
  if (flags & ~(HS_REF_LOOP | HS_REF_START_DRAWN))
    return fail(who + ": flags " + std::to_string(flags) + " hold a bit that is neither HS_REF_LOOP (1) nor "
                "HS_REF_START_DRAWN (2)");
  return 0;
}

// a host caller's reference for a program that reads one, checked and turned into the interpreter's RpRefHost
int ref_host(const char* who_c, const hs_reward_program* p, const hs_reward_fields* f, const hs_reference_host* ref,
             hs::RpRefHost* r) {
  const std::string who(who_c);
  if (ref->n_rows < 1 || ref->n_rows > HS_MAX_REFERENCE_ROWS)
    return fail(who + ": the program reads " + rp_ref_field_read(p) + ", the reference needs n_rows in [1, " +
                std::to_string(HS_MAX_REFERENCE_ROWS) + "], got " + std::to_string(ref->n_rows));
  if (!ref->qpos) return fail(who + ": the reference's qpos must not be NULL");
  if (ref->n_rows > 1 && !(ref->key_dt > 0.0 && std::isfinite(ref->key_dt)))
    return fail(who + ": key_dt must be finite and > 0 with more than one row");
  if (ref_check_flags(who, ref->flags)) return -1;
  const int prec = ref->precision & 0xFF;
  if (prec != HS_FP32 && prec != HS_FP64) return fail(who + ": the reference's precision must be HS_FP32 or HS_FP64");
  if (!f->time) return fail(who + ": a reference is sampled at the state's time, which is NULL");
  if ((ref->flags & HS_REF_START_DRAWN) && (!ref->episode || !ref->seed))
    return fail(who + ": HS_REF_START_DRAWN needs the per-state episode and seed arrays");
  r->K = ref->n_rows;
  r->qpos = ref->qpos;
  r->qvel = ref->qvel;
  r->key_dt = ref->key_dt;
  r->flags = ref->flags;
  r->fp32 = prec == HS_FP32;
  r->episode = ref->episode;
  r->seed = ref->seed;
  r->env = ref->env;
  return 0;
}

// a predicate is read as one truth value: a program with named outputs is a reward, refused as a condition
int term_refuse_outputs(const char* who, const hs_reward_program* pred) {
  if (pred && pred->info.n_outputs > 0)
    return fail(std::string(who) + ": the program has " + std::to_string(pred->info.n_outputs) +
                " outputs; a termination predicate has none (it is read as one truth value)");
  return 0;
}
}  // namespace

// hs_step / hs_step_program on a batch with a termination set, and hs_step_program on any batch: the step
// without auto-reset, the outcome launch, the masked reset
int hs::step_outcome_reset(hs_batch* b, const float* actions, const hs_reward_program* p, const double* params,
                           void* stream) {
  // the predicate's needs once more, in case the config changed after hs_set_termination: before any launch
  if (b->term_prog && rp_check_batch("hs_step", b, b->term_prog, b->term_params, true)) return -1;
  // component rows bound: the program must write exactly that many, or a row would stay stale (or be overrun)
  if (p && b->comp_n > 0 && p->info.n_outputs != b->comp_n)
    return fail("hs_step_program: the program has " + std::to_string(p->info.n_outputs) + " outputs, the batch has " +
                std::to_string(b->comp_n) + " component rows bound (hs_set_reward_components)");
  DeviceGuard g(b->device);
  if (p && !rp_resident(p, b->device)) return -1;
  // 1. the env step without auto-reset -- and, for a reward program, without a reward: the program and the
  //    predicate see the post-step state
  const hs_env_config saved = b->cfg;
  if (p) b->cfg.reward_id = HS_REWARD_NONE;
  b->cfg.autoreset = 0;
  int rc = step_launch(b, actions, stream);
  b->cfg = saved;
  if (rc) return rc;
  // 2. the program and / or the predicate, and the step's outcome rows
  rc = outcome_launch(b, p, params, stream);
  if (rc) return rc;
  // 3. SB3's auto-reset of the finished envs: the masked reset, with the noise an in-kernel auto-reset draws
  if (!saved.autoreset) return 0;
  return launch(b, hs::MODE_RESET, nullptr, b->prog_done, b->ar_qpos_noise, b->ar_qvel_noise, 1, stream);
}

extern "C" {

int hs_reward_eval(const hs_model* m, int precision, int reward_id, const double* kneel_params, int n,
                   const void* qpos, const void* qvel, const void* ctrl, const void* time, const void* subtree_com0,
                   const void* subtree_linvel0, const void* cfrc_ext, const void* qfrc_actuator, void* out,
                   void* stream) {
  if (!m) return fail("hs_reward_eval: null model");
  if (n < 0) return fail("hs_reward_eval: negative n");
  if (reward_id != HS_REWARD_STAND && reward_id != HS_REWARD_KNEELING && reward_id != HS_REWARD_WALK)
    return fail("hs_reward_eval: unknown reward id " + std::to_string(reward_id));
  const int prec = precision & 0xFF;
  if (prec != HS_FP32 && prec != HS_FP64) return fail("hs_reward_eval: precision must be HS_FP32 or HS_FP64");
  const hs::HostModel& h = m->host;
  if (h.nv < 6 || h.nv > 32 || h.nu > 32 || h.nbody < 2 || h.nq < 7)
    return fail("hs_reward_eval: the model needs a free root joint, nv <= 32, nu <= 32 and >= 2 bodies");
  if (n == 0) return 0;
  if (!qpos || !qvel || !ctrl || !time || !subtree_com0 || !subtree_linvel0 || !cfrc_ext || !qfrc_actuator || !out)
    return fail("hs_reward_eval: null buffer");
  static const double kdef[9] = {1.282, 0.85, 3.14159265358979323846 / 6, 0.1, 0.3, 0.3, 0.2, 0.1, 0.1};
  return by_precision(prec, [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RewardEvalArgs<T> a = reward_eval_args<T>(h, reward_id, n, kneel_params ? kneel_params : kdef);
    a.qpos = (const T*)qpos;
    a.qvel = (const T*)qvel;
    a.ctrl = (const T*)ctrl;
    a.time = (const T*)time;
    a.subtree_com0 = (const T*)subtree_com0;
    a.subtree_linvel0 = (const T*)subtree_linvel0;
    a.cfrc_ext = (const T*)cfrc_ext;
    a.qfrc_actuator = (const T*)qfrc_actuator;
    a.out = (T*)out;
    return hip_rc(hs::launch_reward_eval<T>(a, (hipStream_t)stream), "reward_eval_kernel");
  });
}

int hs_reward(hs_batch* b, int reward_id, const double* kneel_params, void* out, void* stream) {
  if (!b || !out) return fail("hs_reward: null argument");
  if (reward_id != HS_REWARD_STAND && reward_id != HS_REWARD_KNEELING && reward_id != HS_REWARD_WALK)
    return fail("hs_reward: unknown reward id " + std::to_string(reward_id));
  if (!(b->cfg.outputs & HS_OUT_AUX) || !(b->cfg.outputs & HS_OUT_CTRL) || b->ctrl_stale)
    return fail("hs_reward: needs the aux row (subtree com) and the data.ctrl copy (HS_OUT_AUX | HS_OUT_CTRL) "
                "written by the last step");
  if (!b->buf.cfrc_ext || !b->buf.subtree_linvel)
    return fail("hs_reward: the batch has no cfrc_ext / subtree_linvel buffers (external buffers without them)");
  const hs::HostModel& h = b->model->host;
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  const int o4 = (h.nq - 2) + h.nv + 16 * h.nbody;   // qfrc_actuator's offset in the obs row (custom_env.py:250)
  return by_precision(b->precision, [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RewardEvalArgs<T> a =
        reward_eval_args<T>(h, reward_id, b->n, kneel_params ? kneel_params : b->cfg.kneel_params);
    a.qpos = (const T*)b->buf.qpos;
    a.qvel = (const T*)b->buf.qvel;
    a.ctrl = (const T*)b->buf.ctrl;
    a.time = (const T*)b->buf.time;
    a.subtree_com0 = (const T*)b->buf.aux + hs::MAXDOF;   // aux row: qacc[MAXDOF], com[3], ...
    a.ld_com = hs::AUXDIM;
    a.subtree_linvel0 = (const T*)b->buf.subtree_linvel;   // zeros unless HS_FULL_STATE (mj_step leaves it)
    a.ld_linv = 3 * h.nbody;
    a.cfrc_ext = (const T*)b->buf.cfrc_ext;
    a.qfrc_actuator = (const T*)b->buf.obs + o4;
    a.ld_qfrc = b->obs_dim;
    a.out = (T*)out;
    return hip_rc(hs::launch_reward_eval<T>(a, (hipStream_t)stream), "reward_eval_kernel");
  });
}

int hs_reward_program_create_components(const hs_model* m, const int32_t* code, int n_instr, const double* consts,
                                        int n_consts, int n_params, int n_outputs, hs_reward_program** prog) {
  if (!m || !prog) return fail("hs_reward_program_create: null argument");
  *prog = nullptr;
  const hs::HostModel& h = m->host;
  const hs::RpDims dims{h.nq, h.nv, h.nu, h.nbody};
  hs::RpInfo info;
  const std::string why = hs::rp_validate(dims, code, n_instr, consts, n_consts, n_params, n_outputs, &info);
  if (!why.empty()) return fail("hs_reward_program_create: " + why);
  auto* p = new hs_reward_program();
  p->dims = dims;
  p->code.assign(code, code + 5 * (size_t)n_instr);
  if (n_consts > 0) p->consts.assign(consts, consts + n_consts);
  p->n_params = n_params;
  p->info = info;
  int ndev = 0, cur = 0;   // with a GPU: resident on the current device now, so no launch has to allocate
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDevice(&cur) == hipSuccess && !rp_resident(p, cur)) {
    delete p;
    return -1;
  }
  *prog = p;
  return 0;
}

int hs_reward_program_create(const hs_model* m, const int32_t* code, int n_instr, const double* consts, int n_consts,
                             int n_params, hs_reward_program** prog) {
  return hs_reward_program_create_components(m, code, n_instr, consts, n_consts, n_params, 0, prog);
}

int hs_reward_program_outputs(const hs_reward_program* p, int* n_outputs) {
  if (!p || !n_outputs) return fail("hs_reward_program_outputs: null argument");
  *n_outputs = p->info.n_outputs;
  return 0;
}

void hs_reward_program_destroy(hs_reward_program* p) {
  if (!p) return;
  for (auto& d : p->dev) {
    DeviceGuard g(d.device);
    (void)hipFree(d.code);
    (void)hipFree(d.consts);
  }
  delete p;
}

int hs_reward_program_info(const hs_reward_program* p, int* n_instr, int* n_slots, unsigned* fields) {
  if (!p) return fail("hs_reward_program_info: null program");
  if (n_instr) *n_instr = (int)(p->code.size() / 5);
  if (n_slots) *n_slots = p->info.n_slots;
  if (fields) *fields = p->info.fields;
  return 0;
}

int hs_reward_program_eval_host_components(const hs_reward_program* p, const double* params, int n,
                                           const hs_reward_fields* f, double* out, double* comp_out) {
  return hs_reward_program_eval_host_reference(p, params, n, f, nullptr, out, comp_out);
}

int hs_reward_program_eval_host_reference(const hs_reward_program* p, const double* params, int n,
                                          const hs_reward_fields* f, const hs_reference_host* ref, double* out,
                                          double* comp_out) {
  const char* who = ref ? "hs_reward_program_eval_host_reference" : "hs_reward_program_eval_host";
  if (!p || !f) return fail(std::string(who) + ": null argument");
  if (n < 0) return fail(std::string(who) + ": negative n");
  if (comp_out && p->info.n_outputs == 0)
    return fail("hs_reward_program_eval_host_components: the program has no outputs, comp_out must be NULL");
  hs::RpRefHost r;
  const bool reads_ref = (p->info.fields & hs::RP_REF_FIELDS) != 0;
  if (ref && reads_ref && ref_host(who, p, f, ref, &r)) return -1;
  if (n == 0) return 0;
  if (!out || (p->n_params > 0 && !params)) return fail(std::string(who) + ": null out or params");
  if (rp_check_fields(who, "program", p, f, ref != nullptr)) return -1;
  hs::rp_eval_host(p->dims, p->code.data(), (int)(p->code.size() / 5), p->consts.data(), params, n,
                   reinterpret_cast<const double* const*>(f), out, comp_out, ref && reads_ref ? &r : nullptr);
  return 0;
}

int hs_reward_program_eval_host(const hs_reward_program* p, const double* params, int n, const hs_reward_fields* f,
                                double* out) {
  return hs_reward_program_eval_host_components(p, params, n, f, out, nullptr);
}

int hs_reward_program_eval(const hs_reward_program* p, int precision, const double* params, int n,
                           const hs_reward_fields* f, void* out, void* stream) {
  if (!p || !f) return fail("hs_reward_program_eval: null argument");
  if (n < 0) return fail("hs_reward_program_eval: negative n");
  const int prec = precision & 0xFF;
  if (prec != HS_FP32 && prec != HS_FP64) return fail("hs_reward_program_eval: precision must be HS_FP32 or HS_FP64");
  if (n == 0) return 0;
  if (!out || (p->n_params > 0 && !params)) return fail("hs_reward_program_eval: null out or params");
  if (rp_check_fields("hs_reward_program_eval", "program", p, f)) return -1;
  int cur = 0;
  if (!hip_ok(hipGetDevice(&cur), "hipGetDevice")) return -1;
  const auto* d = rp_resident(p, cur);
  if (!d) return -1;
  return by_precision(prec, [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RpArgs<T> a = rp_args<T>(p, d, params, n);
    for (int k = 0; k < hs::RP_NFIELDS; k++) {
      a.field[k] = (const T*)reinterpret_cast<const void* const*>(f)[k];
      a.ld[k] = hs::rp_field_len(p->dims, k);
    }
    a.out = (T*)out;
    return hip_rc(hs::launch_reward_program<T>(a, (hipStream_t)stream), "reward_program_kernel");
  });
}

int hs_set_reward_components(hs_batch* b, int n_outputs, void* comp, void* comp_total, int32_t* comp_episode,
                             void* terminal_comp_total) {
  if (!b) return fail("hs_set_reward_components: null batch");
  if (n_outputs < 0 || n_outputs > HS_RP_MAX_OUTPUTS)
    return fail("hs_set_reward_components: n_outputs " + std::to_string(n_outputs) + " outside [0, " +
                std::to_string(HS_RP_MAX_OUTPUTS) + "]");
  const bool any = comp || comp_total || comp_episode || terminal_comp_total;
  const bool all = comp && comp_total && comp_episode && terminal_comp_total;
  if (n_outputs > 0 && any && !all)
    return fail("hs_set_reward_components: pass all four buffers, or none (NULL) to clear the binding");
  if (n_outputs == 0 || !all) {   // clear
    b->comp_n = 0;
    b->comp = b->comp_total = b->term_comp_total = nullptr;
    b->comp_episode = nullptr;
    return 0;
  }
  // no sum belongs to any episode yet: the tag -1 is no episode number (as hs_set_termination's)
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "hs_set_reward_components") ||
      !hip_ok(hipMemset(comp_episode, 0xFF, (size_t)b->n * sizeof(int32_t)), "hs_set_reward_components") ||
      !hip_ok(hipDeviceSynchronize(), "hs_set_reward_components"))
    return -1;
  b->comp_n = n_outputs;
  b->comp = comp;
  b->comp_total = comp_total;
  b->comp_episode = comp_episode;
  b->term_comp_total = terminal_comp_total;
  return 0;
}

int hs_reward_program_batch_components(hs_batch* b, const hs_reward_program* p, const double* params, void* out,
                                       void* comp_out, void* stream) {
  if (!out) return fail("hs_reward_program_batch: null argument");
  if (rp_check_batch("hs_reward_program_batch", b, p, params, false)) return -1;
  if (comp_out && p->info.n_outputs == 0)
    return fail("hs_reward_program_batch_components: the program has no outputs, comp_out must be NULL");
  DeviceGuard g(b->device);
  const auto* d = rp_resident(p, b->device);
  if (!d) return -1;
  if (order_streams(b, (hipStream_t)stream)) return -1;
  return by_precision(b->precision, [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RpArgs<T> a = rp_args<T>(p, d, params, b->n);
    rp_batch_fields<T>(b, a);
    rp_batch_ref<T>(b, p->info.fields, a);
    a.out = (T*)out;
    a.comp = (T*)comp_out;
    a.n_outputs = p->info.n_outputs;
    return hip_rc(hs::launch_reward_program<T>(a, (hipStream_t)stream), "reward_program_kernel");
  });
}

int hs_reward_program_batch(hs_batch* b, const hs_reward_program* p, const double* params, void* out, void* stream) {
  return hs_reward_program_batch_components(b, p, params, out, nullptr, stream);
}

int hs_step_program(hs_batch* b, const float* actions, const hs_reward_program* p, const double* params, void* stream) {
  if (!actions) return fail("hs_step_program: actions must not be NULL");
  if (rp_check_batch("hs_step_program", b, p, params, true)) return -1;
  return hs::step_outcome_reset(b, actions, p, params, stream);
}

int hs_set_termination(hs_batch* b, const hs_reward_program* pred, const double* params, int grace_steps) {
  if (term_refuse_outputs("hs_set_termination", pred)) return -1;
  if (!b) return fail("hs_set_termination: null batch");
  b->term_kind = 0;   // (hs_set_termination_builtin marks the condition fused-capable after this call)
  if (!pred) {   // clear: the buffers stay, the next hs_set_termination starts their counters afresh
    b->term_prog = nullptr;
    return 0;
  }
  if (grace_steps < 1) return fail("hs_set_termination: grace_steps must be >= 1");
  if (rp_check_batch("hs_set_termination", b, pred, params, true)) return -1;
  DeviceGuard g(b->device);
  if (!rp_resident(pred, b->device)) return -1;
  const size_t N = (size_t)b->n;
  if (!b->grace_count &&
      (!hip_ok(hipMalloc((void**)&b->grace_count, N * sizeof(int32_t)), "hipMalloc(grace_count)") ||
       !hip_ok(hipMalloc((void**)&b->grace_episode, N * sizeof(int32_t)), "hipMalloc(grace_episode)") ||
       !hip_ok(hipMalloc((void**)&b->early, N), "hipMalloc(early_terminated)")))
    return -1;
  // no count belongs to any episode yet: the tag -1 is no episode number (they start at 0 and count up)
  if (!hip_ok(hipDeviceSynchronize(), "hs_set_termination") ||
      !hip_ok(hipMemset(b->grace_count, 0, N * sizeof(int32_t)), "hs_set_termination") ||
      !hip_ok(hipMemset(b->grace_episode, 0xFF, N * sizeof(int32_t)), "hs_set_termination") ||
      !hip_ok(hipMemset(b->early, 0, N), "hs_set_termination") ||
      !hip_ok(hipDeviceSynchronize(), "hs_set_termination"))
    return -1;
  for (int k = 0; k < HS_RP_MAX_PARAMS; k++) b->term_params[k] = k < pred->n_params ? params[k] : 0.0;
  b->grace_steps = grace_steps;
  b->term_prog = pred;
  return 0;
}

int hs_set_termination_builtin(hs_batch* b, const hs_reward_program* pred, const double* params, int grace_steps,
                               int kind, double min_height, double max_roll_pitch) {
  const std::string who = "hs_set_termination_builtin";
  if (term_refuse_outputs("hs_set_termination_builtin", pred)) return -1;
  if (!b || !pred) return fail(who + ": null batch or predicate");
  if (kind != HS_TERM_FALLEN && kind != HS_TERM_LOST_BALANCE)
    return fail(who + ": kind " + std::to_string(kind) + " is neither HS_TERM_FALLEN (1) nor HS_TERM_LOST_BALANCE (2)");
  if (!(min_height == min_height) || !(max_roll_pitch == max_roll_pitch))
    return fail(who + ": min_height / max_roll_pitch must not be NaN");
  if (pred->n_params > 0 && !params) return fail(who + ": the program has parameters, params must not be NULL");
  // program and built-in must be the same predicate: the program reads qpos only, and agrees with the built-in
  // on the probe rows (hs_term_builtin.h) -- refused before anything is set or launched
  if (pred->info.fields & ~(1u << hs::RP_F_QPOS)) {
    std::string names;
    for (int k = 0; k < hs::RP_NFIELDS_ALL; k++)
      if (k != hs::RP_F_QPOS && (pred->info.fields & (1u << k))) names += std::string(names.empty() ? "" : ", ") + kRpFieldNames[k];
    return fail(who + ": the predicate reads " + names + "; a built-in condition is a function of qpos alone");
  }
  const int bad = hs::term_probe_mismatch(pred->dims, pred->code.data(), (int)(pred->code.size() / 5), pred->consts.data(),
                                          params, kind, min_height, max_roll_pitch);
  if (bad >= 0)
    return fail(who + ": the predicate and the built-in (kind " + std::to_string(kind) + ", min_height " +
                std::to_string(min_height) + ", max_roll_pitch " + std::to_string(max_roll_pitch) +
                ") differ on probe row " + std::to_string(bad) + ": not the same condition");
  if (int rc = hs_set_termination(b, pred, params, grace_steps)) return rc;
  DeviceGuard g(b->device);
  const size_t N = (size_t)b->n;
  if (!b->mid_count && !hs::uc_alloc(b->device, N * sizeof(int32_t), (void**)&b->mid_count, "grace hand-off counts"))
    return -1;
  // (a recycled uncached block holds another batch's words: a lost hand-off would read them)
  if (!hip_ok(hipMemset(b->mid_count, 0, N * sizeof(int32_t)), "hs_set_termination_builtin") ||
      !hip_ok(hipDeviceSynchronize(), "hs_set_termination_builtin"))
    return -1;
  b->term_kind = kind;
  b->term_min_height = min_height;
  b->term_max_roll_pitch = max_roll_pitch;
  return 0;
}

int hs_termination_builtin_eval_host(int kind, double min_height, double max_roll_pitch, int n, const double* qpos,
                                     int ld, uint8_t* out) {
  if (kind != HS_TERM_FALLEN && kind != HS_TERM_LOST_BALANCE)
    return fail("hs_termination_builtin_eval_host: kind must be HS_TERM_FALLEN (1) or HS_TERM_LOST_BALANCE (2)");
  if (n < 0) return fail("hs_termination_builtin_eval_host: negative n");
  if (n == 0) return 0;
  if (!qpos || !out || ld < 7) return fail("hs_termination_builtin_eval_host: null qpos / out, or ld < 7");
  for (int i = 0; i < n; i++)
    out[i] = hs::term_builtin_holds<double>(kind, min_height, max_roll_pitch, qpos + (size_t)i * ld) ? 1 : 0;
  return 0;
}

int hs_termination_state(const hs_batch* b, int* grace_steps, const uint8_t** early_terminated,
                         const int32_t** grace_count, const int32_t** grace_episode) {
  if (!b) return fail("hs_termination_state: null batch");
  if (grace_steps) *grace_steps = b->term_prog ? b->grace_steps : 0;
  if (early_terminated) *early_terminated = b->early;
  if (grace_count) *grace_count = b->grace_count;
  if (grace_episode) *grace_episode = b->grace_episode;
  return b->term_prog ? 1 : 0;
}

int hs_apply_termination(hs_batch* b, void* stream) {
  if (!b) return fail("hs_apply_termination: null batch");
  if (!b->term_prog) return fail("hs_apply_termination: the batch has no termination condition (hs_set_termination)");
  if (rp_check_batch("hs_apply_termination", b, b->term_prog, b->term_params, false)) return -1;
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  return outcome_launch(b, nullptr, nullptr, stream);
}

int hs_termination_eval_host(const hs_reward_program* pred, const double* params, int grace_steps, int n,
                             const hs_reward_fields* f, const int32_t* episode, int32_t* count, int32_t* episode_tag,
                             uint8_t* early) {
  return hs_termination_eval_host_reference(pred, params, grace_steps, n, f, nullptr, episode, count, episode_tag, early);
}

int hs_termination_eval_host_reference(const hs_reward_program* pred, const double* params, int grace_steps, int n,
                                       const hs_reward_fields* f, const hs_reference_host* ref, const int32_t* episode,
                                       int32_t* count, int32_t* episode_tag, uint8_t* early) {
  if (term_refuse_outputs("hs_termination_eval_host", pred)) return -1;
  if (!pred || !f) return fail("hs_termination_eval_host: null argument");
  hs::RpRefHost r;
  const bool reads_ref = (pred->info.fields & hs::RP_REF_FIELDS) != 0;
  if (ref && reads_ref && ref_host("hs_termination_eval_host_reference", pred, f, ref, &r)) return -1;
  if (n < 0) return fail("hs_termination_eval_host: negative n");
  if (grace_steps < 1) return fail("hs_termination_eval_host: grace_steps must be >= 1");
  if (n == 0) return 0;
  if (!episode || !count || !episode_tag || !early || (pred->n_params > 0 && !params))
    return fail("hs_termination_eval_host: null episode, count, episode_tag, early or params");
  if (rp_check_fields("hs_termination_eval_host", "predicate", pred, f, ref != nullptr)) return -1;
  hs::rp_termination_eval_host(pred->dims, pred->code.data(), (int)(pred->code.size() / 5), pred->consts.data(), params,
                               grace_steps, n, reinterpret_cast<const double* const*>(f), episode, count, episode_tag,
                               early, ref && reads_ref ? &r : nullptr);
  return 0;
}

int hs_set_reference_motion(hs_batch* b, int n_rows, const double* qpos, const double* qvel, double key_dt, int flags) {
  const std::string who = "hs_set_reference_motion";
  if (!b) return fail(who + ": null batch");
  if (n_rows < 0 || n_rows > HS_MAX_REFERENCE_ROWS)
    return fail(who + ": n_rows " + std::to_string(n_rows) + " must lie in [0, HS_MAX_REFERENCE_ROWS = " +
                std::to_string(HS_MAX_REFERENCE_ROWS) + "]");
  if (n_rows == 0) {   // unbind: the blocks stay for the next bind
    b->ref_n = 0;
    return 0;
  }
  if (!qpos) return fail(who + ": qpos must not be NULL with n_rows > 0");
  if (n_rows > 1 && !(key_dt > 0.0 && std::isfinite(key_dt)))
    return fail(who + ": key_dt must be finite and > 0 with more than one row (the seconds between consecutive rows)");
  if (ref_check_flags(who, flags)) return -1;
  const auto& h = b->model->host;
  const size_t K = (size_t)n_rows, nq = (size_t)h.nq, nv = (size_t)h.nv;
  std::vector<double> q(qpos, qpos + K * nq), v(K * nv, 0.0);
  if (qvel) v.assign(qvel, qvel + K * nv);
  for (size_t i = 0; i < q.size(); i++)
    if (!std::isfinite(q[i]))
      return fail(who + ": qpos[" + std::to_string(i / nq) + "][" + std::to_string(i % nq) + "] is not finite");
  for (size_t i = 0; i < v.size(); i++)
    if (!std::isfinite(v[i]))
      return fail(who + ": qvel[" + std::to_string(i / nv) + "][" + std::to_string(i % nv) + "] is not finite");
  // the free joint's quaternion, normalised as hs_set_initial_states normalises a bank's
  if (h.njnt > 0 && h.jnt_type[0] == hs::JNT_FREE && nq >= 7)
    for (size_t j = 0; j < K; j++)
      if (!ref_normalize_quat(q.data() + j * nq))
        return fail(who + ": row " + std::to_string(j) + " has a zero free-joint quaternion");
  DeviceGuard g(b->device);
  // after the batch's pending launches, whatever stream they are on (they may read the rows written below)
  if (!hip_ok(hipDeviceSynchronize(), "hs_set_reference_motion")) return -1;
  const size_t es = hs::elem_size(b);
  if (n_rows > b->ref_cap) {
    void *q_blk = nullptr, *v_blk = nullptr;
    const int cap = std::min(HS_MAX_REFERENCE_ROWS, std::max(n_rows, 2 * b->ref_cap));
    if (!hip_ok(hipMalloc(&q_blk, (size_t)cap * nq * es), "hipMalloc(reference motion)") ||
        !hip_ok(hipMalloc(&v_blk, (size_t)cap * nv * es), "hipMalloc(reference motion)")) {
      if (q_blk) (void)hipFree(q_blk);
      return -1;
    }
    if (b->ref_q) b->ref_retired.push_back(b->ref_q);
    if (b->ref_v) b->ref_retired.push_back(b->ref_v);
    b->ref_n = 0;
    b->ref_q = q_blk;
    b->ref_v = v_blk;
    b->ref_cap = cap;
  }
  const bool ok = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    const std::vector<T> tq(q.begin(), q.end()), tv(v.begin(), v.end());
    return hip_ok(hipMemcpy(b->ref_q, tq.data(), tq.size() * sizeof(T), hipMemcpyHostToDevice), "reference qpos") &&
           hip_ok(hipMemcpy(b->ref_v, tv.data(), tv.size() * sizeof(T), hipMemcpyHostToDevice), "reference qvel");
  });
  if (!ok) {
    b->ref_n = 0;
    return -1;
  }
  b->ref_n = n_rows;
  b->ref_key_dt = n_rows > 1 ? key_dt : 1.0;
  b->ref_flags = flags;
  return 0;
}

int hs_get_reference_motion(const hs_batch* b, int* n_rows, double* key_dt, int* flags) {
  if (!b) return fail("hs_get_reference_motion: null batch");
  if (n_rows) *n_rows = b->ref_n;
  if (key_dt) *key_dt = b->ref_n > 0 ? b->ref_key_dt : 0.0;
  if (flags) *flags = b->ref_n > 0 ? b->ref_flags : 0;
  return 0;
}

}  // extern "C"
