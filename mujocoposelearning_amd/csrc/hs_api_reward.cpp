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
const char* const kRpFieldNames[hs::RP_NFIELDS] = {"qpos", "qvel", "ctrl", "time", "qfrc_actuator", "cinert", "cvel",
                                                   "subtree_com[0]", "cfrc_ext", "subtree_linvel"};

// every field the program (`noun`: "program" / "predicate") reads must be given; `who`: the entry point's name
int rp_check_fields(const char* who, const char* noun, const hs_reward_program* p, const hs_reward_fields* f) {
  const void* const* fp = reinterpret_cast<const void* const*>(f);
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
  if (!p || !f) return fail("hs_reward_program_eval_host: null argument");
  if (n < 0) return fail("hs_reward_program_eval_host: negative n");
  if (comp_out && p->info.n_outputs == 0)
    return fail("hs_reward_program_eval_host_components: the program has no outputs, comp_out must be NULL");
  if (n == 0) return 0;
  if (!out || (p->n_params > 0 && !params)) return fail("hs_reward_program_eval_host: null out or params");
  if (rp_check_fields("hs_reward_program_eval_host", "program", p, f)) return -1;
  hs::rp_eval_host(p->dims, p->code.data(), (int)(p->code.size() / 5), p->consts.data(), params, n,
                   reinterpret_cast<const double* const*>(f), out, comp_out);
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
    for (int k = 0; k < hs::RP_NFIELDS; k++)
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
  if (term_refuse_outputs("hs_termination_eval_host", pred)) return -1;
  if (!pred || !f) return fail("hs_termination_eval_host: null argument");
  if (n < 0) return fail("hs_termination_eval_host: negative n");
  if (grace_steps < 1) return fail("hs_termination_eval_host: grace_steps must be >= 1");
  if (n == 0) return 0;
  if (!episode || !count || !episode_tag || !early || (pred->n_params > 0 && !params))
    return fail("hs_termination_eval_host: null episode, count, episode_tag, early or params");
  if (rp_check_fields("hs_termination_eval_host", "predicate", pred, f)) return -1;
  hs::rp_termination_eval_host(pred->dims, pred->code.data(), (int)(pred->code.size() / 5), pred->consts.data(), params,
                               grace_steps, n, reinterpret_cast<const double* const*>(f), episode, count, episode_tag,
                               early);
  return 0;
}

}  // extern "C"
