// hsim C ABI: the fused launches of a batch -- several env steps in one kernel launch (hs_step_tape), with
// the policy in the loop (hs_rollout*) and over whole episodes (hs_evaluate*).
#include <cmath>

#include "hs_act.h"
#include "hs_api_batch.h"

static_assert(HS_ACT_RELU == hs::ACT_RELU && HS_ACT_TANH == hs::ACT_TANH, "activation ids");

namespace {
using hs::DeviceGuard;
using hs::fail;
using hs::hip_ok;
using hs::order_streams;

// -- tape launches (hs_step_tape, hs_rollout) --------------------------------------------------
// Each env finishes at most one episode per tape launch (its terminal obs / info rows are then written
// once, see hs_env_step.h step_pair): launches of at most the shortest episode's length.  An episode
// starts at time = one timestep (the reset's mj_step) and ends at time >= duration (custom_env.py:213)
// or at max_steps.
int min_episode_len(const hs_batch* b) {
  const auto& h = b->model->host;
  const double dt = h.timestep * b->cfg.frame_skip;
  const double spans = std::floor((b->cfg.duration - h.timestep) / dt - 1e-9);
  return (int)std::max(1.0, std::min((double)b->cfg.max_steps, spans));
}

// the most env steps of one fused launch: each env finishes at most one episode in it (min_episode_len), unless
// a fused-capable condition is set -- its instances write nothing once per episode (hs_env_step.h env_outcome)
int fused_step_cap(const hs_batch* b) {
  return b->term_prog && b->term_kind != 0 ? hs::QTAG_STEPS : std::min(min_episode_len(b), hs::QTAG_STEPS);
}

const char kNoFusedWithTermination[] =
    ": the batch has a termination condition set (hs_set_termination), and a fused launch is bounded by the "
    "shortest possible episode, which a state-dependent end makes unknowable -- step with hs_step / "
    "hs_step_program, or clear the condition";
// the condition keeps the fused launches out unless it is fused-capable (hs_set_termination_builtin)
bool term_blocks_fused(const hs_batch* b) { return b->term_prog && b->term_kind == 0; }

struct Region { void* p; size_t bytes; };

// the env state a tape launch changes (restored when it aborts on a resident-tier overflow)
std::vector<Region> state_regions(const hs_batch* b) {
  const auto& h = b->model->host;
  const size_t N = (size_t)b->n, es = hs::elem_size(b);
  std::vector<Region> regs = {{b->buf.qpos, N * h.nq * es}, {b->buf.qvel, N * h.nv * es},
                              {b->buf.qacc_warmstart, N * h.nv * es}, {b->buf.ctrl, N * h.nu * es},
                              {b->buf.time, N * es}, {b->buf.total_reward, N * es}, {b->buf.step_count, N * 4},
                              {b->buf.episode, N * 4}, {b->buf.warning, N * HS_NWARN * 4},
                              {b->redo_total, sizeof(unsigned long long)}};
  // a fused-capable termination condition: the launch's last step commits the grace counters, their episode
  // tags and the early bytes, and the per-step replay of an aborted launch starts from the counters it found
  if (b->term_prog && b->term_kind != 0) {
    regs.push_back({b->grace_count, N * sizeof(int32_t)});
    regs.push_back({b->grace_episode, N * sizeof(int32_t)});
    regs.push_back({b->early, N});
  }
  return regs;
}

// Back up `regs`, run `go` (the tape launch), and read the abort word: 0 = done, 1 = aborted (the
// regions are restored and the redo list cleared), -1 = error.  Synchronizes the stream.
template <typename F>
int guarded_tape(hs_batch* b, const std::vector<Region>& regs, hipStream_t st, F&& go) {
  size_t total = 0;
  for (auto& r : regs) total += (r.bytes + 255) & ~(size_t)255;
  if (total > b->tape_backup_bytes) {
    if (b->tape_backup) (void)hipFree(b->tape_backup);
    b->tape_backup = nullptr;
    b->tape_backup_bytes = 0;
    if (!hip_ok(hipMalloc(&b->tape_backup, total), "hipMalloc(tape backup)")) return -1;
    b->tape_backup_bytes = total;
  }
  size_t off = 0;
  for (auto& r : regs) {
    if (!hip_ok(hipMemcpyAsync((char*)b->tape_backup + off, r.p, r.bytes, hipMemcpyDeviceToDevice, st), "tape backup"))
      return -1;
    off += (r.bytes + 255) & ~(size_t)255;
  }
  if (!hip_ok(hipMemsetAsync(b->qsync + hs::QS_ABORT, 0, sizeof(int), st), "tape abort word")) return -1;
  // HIP events right around the kernel launch on its stream (hs_last_tape_ms: the bench's roofline of
  // the fused rollout kernel); one pair per tape launch, which is one per several env steps
  for (auto& e : b->tape_ev)
    if (!e && !hip_ok(hipEventCreate(&e), "hipEventCreate")) return -1;
  if (!hip_ok(hipEventRecord(b->tape_ev[0], st), "tape event")) return -1;
  int rc = go();
  if (rc) return rc < 0 ? rc : -1;
  if (!hip_ok(hipEventRecord(b->tape_ev[1], st), "tape event")) return -1;
  int aborted = 0;
  if (!hip_ok(hipMemcpyAsync(&aborted, b->qsync + hs::QS_ABORT, sizeof(int), hipMemcpyDeviceToHost, st),
              "tape abort word") ||
      !hip_ok(hipStreamSynchronize(st), "tape launch"))
    return -1;
  if (!hip_ok(hipEventElapsedTime(&b->last_tape_ms, b->tape_ev[0], b->tape_ev[1]), "tape event time")) return -1;
  if (!aborted) return 0;
  off = 0;
  for (auto& r : regs) {
    if (!hip_ok(hipMemcpyAsync(r.p, (char*)b->tape_backup + off, r.bytes, hipMemcpyDeviceToDevice, st), "tape restore"))
      return -1;
    off += (r.bytes + 255) & ~(size_t)255;
  }
  if (!hip_ok(hipMemsetAsync(b->redo, 0, 2 * sizeof(int), st), "tape redo list")) return -1;
  b->tape_aborts++;
  return 1;
}

// step t's slice of the four per-step output arrays
hs_tape_out tape_slice(const hs_batch* b, const hs_tape_out& out, size_t t) {
  const size_t N = (size_t)b->n, es = hs::elem_size(b);
  return {(char*)out.obs + t * N * b->obs_dim * es, (char*)out.reward + t * N * es, out.terminated + t * N,
          out.truncated + t * N};
}

// one step's four arrays between the batch's own output buffers and the slice `s`, towards the batch or from it
int tape_copy(hs_batch* b, const hs_tape_out& s, bool to_batch, hipStream_t st) {
  const size_t N = (size_t)b->n, es = hs::elem_size(b);
  const struct { void* own; void* slice; size_t bytes; const char* what; } rows[] = {
      {b->buf.obs, s.obs, N * b->obs_dim * es, "tape obs"}, {b->buf.reward, s.reward, N * es, "tape reward"},
      {b->buf.terminated, s.terminated, N, "tape terminated"}, {b->buf.truncated, s.truncated, N, "tape truncated"}};
  for (auto& r : rows)
    if (!hip_ok(hipMemcpyAsync(to_batch ? r.own : r.slice, to_batch ? r.slice : r.own, r.bytes,
                               hipMemcpyDeviceToDevice, st), r.what))
      return -1;
  return 0;
}

// what hs_rollout_act and hs_evaluate ask of the batch, the policy and the step range (`who`: the entry
// point's name in the error text); `hidden` out: the pi net's width
int fused_policy_check(const hs_batch* b, const hs_policy* pol, int act, int t_begin, int n_steps, int t_total,
                       const std::string& who, int* hidden_out) {
  const auto& h = b->model->host;
  if (term_blocks_fused(b)) return fail(who + kNoFusedWithTermination);
  if (b->precision != HS_FP64 || h.solver == 1)
    return fail(who + ": the fused rollout runs on the fp64 Newton engine");
  if (!b->cfg.autoreset || b->ar_qpos_noise || b->cfg.reward_id == HS_REWARD_NONE)
    return fail(who + ": needs auto-reset with the on-device reset noise and a device reward");
  if (b->cfg.schedule != HS_SCHED_AUTO && b->cfg.schedule != HS_SCHED_FIXED_ORDER)
    return fail(who + ": needs the chunk-queue schedule (HS_SCHED_AUTO or HS_SCHED_FIXED_ORDER)");
  const int hidden = pol->hidden ? pol->hidden : 256;   // 0: a caller from before the field
  if (pol->obs_dim != b->obs_dim || pol->act_dim != h.nu || pol->act_dim > 32 || pol->obs_dim % 4 ||
      pol->obs_dim > 512 || (hidden != 64 && hidden != 128 && hidden != 256) || pol->ld1 < hidden || pol->ld1 % 4)
    return fail(who + ": policy shape (obs_dim " + std::to_string(pol->obs_dim) + ", act_dim " +
                std::to_string(pol->act_dim) + ", ld1 " + std::to_string(pol->ld1) + ", hidden " +
                std::to_string(pol->hidden) +
                ") does not fit the fused forward (obs_dim = the batch's, a multiple of 4 and <= 512; act_dim = nu "
                "<= 32; two hidden layers of 64, 128 or 256 (hidden = 0: 256); ld1 >= hidden, a multiple of 4)");
  if (act != HS_ACT_RELU && act != HS_ACT_TANH)
    return fail(who + ": activation " + std::to_string(act) + " is neither HS_ACT_RELU (0) nor HS_ACT_TANH (1)");
  if (n_steps < 1 || t_begin < 0 || t_begin + n_steps > t_total || n_steps > fused_step_cap(b))
    return fail(who + ": steps [t_begin, t_begin + n_steps) must lie in [0, t_total) and n_steps in [1, " +
                std::to_string(fused_step_cap(b)) + "] (hs_rollout_max_steps)");
  *hidden_out = hidden;
  return 0;
}

hs::RolloutArgs policy_args(const hs_policy* pol, int hidden, int act) {
  hs::RolloutArgs ro{};
  ro.w1 = pol->w1; ro.b1 = pol->b1; ro.w2 = pol->w2; ro.b2 = pol->b2; ro.w3 = pol->w3; ro.b3 = pol->b3;
  ro.log_std = pol->log_std;
  ro.ld1 = pol->ld1; ro.D = pol->obs_dim; ro.A = pol->act_dim; ro.H = hidden; ro.hact = act;
  return ro;
}

// hs_rollout_norm / hs_evaluate_norm: the moments the policy normalises its obs with
int norm_args_check(const hs_batch* b, const hs_obs_norm_args* on, const std::string& who, hs::NormArgs* out) {
  if (!on) return fail(who + ": null hs_obs_norm_args");
  if (!on->mean || !on->inv_std) return fail(who + ": null mean / inv_std");
  if (on->obs_dim != b->obs_dim)
    return fail(who + ": hs_obs_norm_args.obs_dim " + std::to_string(on->obs_dim) + " is not the batch's obs_dim " +
                std::to_string(b->obs_dim));
  if (!(on->clip > 0.f)) return fail(who + ": need clip > 0");
  out->mean = on->mean; out->inv_std = on->inv_std; out->clip = on->clip;
  return 0;
}

// the step range and what every fused launch with a policy is given besides its own buffers
struct FusedCall {
  const hs_policy* pol;
  int act, t_begin, n_steps, t_total;
  void* stream;
  const hs_obs_norm_args* on;   // hs_*_norm only (norm)
  bool norm;
};

// The frame hs_rollout* and hs_evaluate* share (`who`: "hs_rollout" / "hs_evaluate", `bufs`: the caller's
// buffer struct): the policy and norm checks, the caller's own (`check`), the device guard, stream ordering and
// the resident-wave check, then the guarded launch over the state regions.  `fill` completes the RolloutArgs
// (`ev`: the caller's EvalArgs, which it fills too; null for a rollout) and adds the caller's regions.
template <typename Check, typename Fill>
int fused_policy_launch(hs_batch* b, const FusedCall& c, const void* bufs, const std::string& who, hs::EvalArgs* ev,
                        Check&& check, Fill&& fill) {
  if (!b || !c.pol || !bufs) return fail("null argument");
  const std::string who_norm = c.norm ? who + "_norm" : who;
  int hidden = 0;
  if (int rc = fused_policy_check(b, c.pol, c.act, c.t_begin, c.n_steps, c.t_total, who_norm, &hidden)) return rc;
  hs::LaunchExtra x;
  x.nsteps = c.n_steps;
  if (c.norm)
    if (int rc = norm_args_check(b, c.on, who_norm, &x.fused.nm)) return rc;
  if (int rc = check()) return rc;
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)c.stream)) return -1;
  const int resident = hs::resident_waves<double>(false);
  if (resident <= 0 || !b->mid || !b->qsync) return fail(who + ": no resident-wave count / queue buffers");
  hs::RolloutArgs& ro = x.fused.ro = policy_args(c.pol, hidden, c.act);
  ro.t_begin = c.t_begin; ro.t_total = c.t_total;
  std::vector<Region> regs = state_regions(b);
  if (int rc = fill(ro, regs)) return rc;
  if (ev) x.fused.ev = *ev;
  int rc = guarded_tape(b, regs, (hipStream_t)c.stream, [&] {
    return hs::launch(b, hs::MODE_ENV_STEP, ro.act_clip, nullptr, nullptr, nullptr, b->cfg.frame_skip, c.stream, x);
  });
  if (rc == 0) hs::env_step_committed(b);
  return rc;
}

int rollout_impl(hs_batch* b, const FusedCall& c, const hs_rollout_bufs* rb) {
  auto check = [&]() -> int {
    const hs_policy* pol = c.pol;
    for (const void* q : {(const void*)pol->w1, (const void*)pol->b1, (const void*)pol->w2, (const void*)pol->b2,
                          (const void*)pol->w3, (const void*)pol->b3, (const void*)pol->log_std, (const void*)rb->obs,
                          (const void*)rb->obs_last, (const void*)rb->actions, (const void*)rb->log_probs,
                          (const void*)rb->episode_starts, (const void*)rb->rewards, (const void*)rb->dones,
                          (const void*)rb->episode_returns, (const void*)rb->boot, (const void*)rb->terminal_obs,
                          (const void*)rb->ep_acc, (const void*)rb->episode_start, (const void*)rb->actions_clipped,
                          (const void*)rb->counter_base})
      if (!q) return fail("hs_rollout: every policy weight and rollout buffer must be given");
    return 0;
  };
  auto fill = [&](hs::RolloutArgs& ro, std::vector<Region>& regs) -> int {
    ro.obs = rb->obs; ro.obs_last = rb->obs_last; ro.act = rb->actions; ro.logp = rb->log_probs;
    ro.start = rb->episode_starts; ro.rew = rb->rewards; ro.done = rb->dones; ro.epret = rb->episode_returns;
    ro.boot = rb->boot; ro.tobs = rb->terminal_obs; ro.ep_acc = rb->ep_acc; ro.episode_start = rb->episode_start;
    ro.act_clip = rb->actions_clipped; ro.ctr_base = rb->counter_base;
    ro.k0 = (uint32_t)rb->seed; ro.k1 = (uint32_t)(rb->seed >> 32); ro.deterministic = rb->deterministic;
    const size_t N = (size_t)b->n;
    regs.push_back({rb->ep_acc, N * sizeof(double)});
    regs.push_back({rb->episode_start, N * sizeof(float)});
    regs.push_back({rb->actions_clipped, N * (size_t)c.pol->act_dim * sizeof(float)});
    return 0;
  };
  return fused_policy_launch(b, c, rb, "hs_rollout", nullptr, check, fill);
}

int evaluate_impl(hs_batch* b, const FusedCall& c, const hs_eval_bufs* eb) {
  auto check = [&]() -> int {
    const hs_policy* pol = c.pol;
    for (const void* q : {(const void*)pol->w1, (const void*)pol->b1, (const void*)pol->w2, (const void*)pol->b2,
                          (const void*)pol->w3, (const void*)pol->b3, (const void*)pol->log_std,
                          (const void*)eb->actions_clipped, (const void*)eb->episode0, (const void*)eb->ep_return,
                          (const void*)eb->ep_length, (const void*)eb->ep_end_step, (const void*)eb->counter_base})
      if (!q) return fail("hs_evaluate: every policy weight, actions_clipped, episode0, the three result arrays and "
                          "counter_base must be given");
    if (eb->max_episodes < 1) return fail("hs_evaluate: max_episodes must be >= 1");
    if (eb->n_trace < 0 || eb->n_trace > b->n)
      return fail("hs_evaluate: n_trace " + std::to_string(eb->n_trace) + " must lie in [0, n_envs = " +
                  std::to_string(b->n) + "]");
    if (eb->n_trace > 0 && (!eb->trace_qpos || !eb->trace_qvel || !eb->trace_actions || !eb->trace_rewards ||
                            !eb->trace_dones))
      return fail("hs_evaluate: n_trace > 0 needs all five trace arrays");
    return 0;
  };
  hs::EvalArgs ev{};
  auto fill = [&](hs::RolloutArgs& ro, std::vector<Region>& regs) -> int {
    // the staging rows: one [obs_dim] f32 row per env, rewritten every env step by waves on any XCD, so
    // uncached memory like the hand-off rows (hs_env_step.h step_pair); allocated at the first evaluation
    const size_t N = (size_t)b->n;
    if (!b->eval_obs && !hs::uc_alloc(b->device, N * (size_t)b->obs_dim * sizeof(float), &b->eval_obs, "eval obs rows"))
      return -1;
    ro.obs = (float*)b->eval_obs;
    ro.act_clip = eb->actions_clipped; ro.ctr_base = eb->counter_base;
    ro.k0 = (uint32_t)eb->seed; ro.k1 = (uint32_t)(eb->seed >> 32); ro.deterministic = eb->deterministic;
    ev.episode0 = eb->episode0; ev.max_episodes = eb->max_episodes; ev.n_trace = eb->n_trace;
    ev.ep_return = eb->ep_return; ev.ep_length = eb->ep_length; ev.ep_end_step = eb->ep_end_step;
    ev.tr_qpos = eb->trace_qpos; ev.tr_qvel = eb->trace_qvel; ev.tr_act = eb->trace_actions;
    ev.tr_rew = eb->trace_rewards; ev.tr_done = eb->trace_dones;
    regs.push_back({eb->actions_clipped, N * (size_t)c.pol->act_dim * sizeof(float)});
    return 0;
  };
  return fused_policy_launch(b, c, eb, "hs_evaluate", &ev, check, fill);
}
}  // namespace

extern "C" {

int hs_step_tape(hs_batch* b, const float* actions, int n_steps, const hs_tape_out* out, void* stream) {
  if (!b) return fail("null batch");
  if (!actions) return fail("hs_step_tape: actions must not be NULL");
  if (n_steps < 1) return fail("hs_step_tape: n_steps must be >= 1");
  if (out && (!out->obs || !out->reward || !out->terminated || !out->truncated))
    return fail("hs_step_tape: pass all four per-step output arrays, or out = NULL");
  if (term_blocks_fused(b)) return fail(std::string("hs_step_tape") + kNoFusedWithTermination);
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  const auto& h = b->model->host;
  const size_t N = (size_t)b->n, nu = (size_t)h.nu;
  hipStream_t st = (hipStream_t)stream;
  // n_steps hs_step calls, each step's outputs copied into its slice (the reference path, and the
  // replay of an aborted tape launch)
  auto per_step = [&]() -> int {
    for (int t = 0; t < n_steps; t++) {
      int rc = hs_step(b, actions + (size_t)t * N * nu, stream);
      if (rc) return rc;
      if (out && tape_copy(b, tape_slice(b, *out, (size_t)t), false, st)) return -1;
    }
    return 0;
  };
  const int resident =
      hs::by_precision(b->precision, [&](auto zero) { return hs::resident_waves<decltype(zero)>(h.solver == 1); });
  const bool tape_sched = b->cfg.schedule == HS_SCHED_AUTO || b->cfg.schedule == HS_SCHED_FIXED_ORDER;
  // without auto-reset a finished env keeps rewriting its terminal info every step (one launch
  // must write each batch address once, see hs_env_step.h step_pair): step by step
  if (n_steps == 1 || !tape_sched || !b->cfg.autoreset || resident <= 0 || !b->mid || !b->qsync) return per_step();
  // a fused-capable termination condition: its instances ask what the fused rollout asks
  if (b->term_prog) {
    if (b->precision != HS_FP64 || h.solver == 1)
      return fail("hs_step_tape: with a termination condition the tape launch runs on the fp64 Newton engine");
    if (b->ar_qpos_noise || b->cfg.reward_id == HS_REWARD_NONE)
      return fail("hs_step_tape: with a termination condition the tape launch needs auto-reset with the on-device "
                  "reset noise and a device reward");
  }
  // one launch covers at most the shortest episode and at most QTAG_STEPS steps (its hand-off tags)
  const int min_len = fused_step_cap(b);
  if (n_steps > min_len) {
    for (int t0 = 0; t0 < n_steps; t0 += min_len) {
      const int k = std::min(min_len, n_steps - t0);
      hs_tape_out sub{};
      if (out) sub = tape_slice(b, *out, (size_t)t0);
      int rc = hs_step_tape(b, actions + (size_t)t0 * N * nu, k, out ? &sub : nullptr, stream);
      if (rc) return rc;
    }
    return 0;
  }
  // an env that overflows the resident tier stops the tape launch (QS_ABORT), and the tape is then
  // replayed step by step from the saved state (the wide tier re-runs the overflowing steps) -- the
  // same results, bitwise, as n_steps hs_step calls either way
  hs::LaunchExtra x;
  x.nsteps = n_steps; x.tape = out;
  int rc = guarded_tape(b, state_regions(b), st, [&] {
    return hs::launch(b, hs::MODE_ENV_STEP, actions, nullptr, b->ar_qpos_noise, b->ar_qvel_noise, b->cfg.frame_skip,
                      stream, x);
  });
  if (rc < 0) return rc;
  if (rc == 1) return per_step();
  hs::env_step_committed(b);
  // the batch's own output buffers hold the last step, as after n_steps hs_step calls
  if (out) return tape_copy(b, tape_slice(b, *out, (size_t)n_steps - 1), true, st);
  return 0;
}

int hs_rollout_max_steps(const hs_batch* b) {
  if (!b) return fail("null batch");
  return fused_step_cap(b);
}

int hs_rollout_act(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb, int t_begin, int n_steps,
                   int t_total, void* stream) {
  return rollout_impl(b, {pol, act, t_begin, n_steps, t_total, stream, nullptr, false}, rb);
}

int hs_rollout(hs_batch* b, const hs_policy* pol, const hs_rollout_bufs* rb, int t_begin, int n_steps, int t_total,
               void* stream) {
  return hs_rollout_act(b, pol, HS_ACT_RELU, rb, t_begin, n_steps, t_total, stream);
}

int hs_rollout_norm(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb,
                    const hs_obs_norm_args* norm, int t_begin, int n_steps, int t_total, void* stream) {
  return rollout_impl(b, {pol, act, t_begin, n_steps, t_total, stream, norm, true}, rb);
}

int hs_evaluate(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, int t_begin, int n_steps,
                int t_total, void* stream) {
  return evaluate_impl(b, {pol, act, t_begin, n_steps, t_total, stream, nullptr, false}, eb);
}

int hs_evaluate_norm(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, const hs_obs_norm_args* norm,
                     int t_begin, int n_steps, int t_total, void* stream) {
  return evaluate_impl(b, {pol, act, t_begin, n_steps, t_total, stream, norm, true}, eb);
}

int hs_last_tape_ms(const hs_batch* b, double* ms) {
  if (!b || !ms) return fail("null argument");
  *ms = (double)b->last_tape_ms;
  return 0;
}

int hs_tape_aborts(const hs_batch* b, uint64_t* n) {
  if (!b || !n) return fail("null argument");
  *n = b->tape_aborts;
  return 0;
}

}  // extern "C"
