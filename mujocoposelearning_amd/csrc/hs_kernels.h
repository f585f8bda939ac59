// hsim device buffers and launch interface (product).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_model.h"
#include "hs_schedule.h"

namespace hs {

constexpr int AUXDIM = MAXDOF + 8;   // per env: qacc[nv], com[3], ncon, nefc, newton iters, solver flag
constexpr int DBGDIM = 32768;        // stage dump (env 0 only) for parity debugging
// hand-off row of a queued env step (qpos, qvel, qacc_warmstart, time, warning counters, and the
// env bookkeeping a tape launch carries from one env step to the next: step count, episode, return)
constexpr int MID_NWARN = 5;   // == NWARN (static_assert below)
constexpr int MID_Q = 0, MID_V = MAXQ, MID_WS = MAXQ + MAXDOF, MID_TIME = MAXQ + 2 * MAXDOF, MID_W = MID_TIME + 1;
constexpr int MID_SC = MID_W + MID_NWARN, MID_EP = MID_SC + 1, MID_TOT = MID_SC + 2;
// a fused rollout (hs_rollout) also hands over the next step's clipped action and the episode return
constexpr int MID_ACT = MID_TOT + 1, MID_EPACC = MID_ACT + 32;
constexpr int MIDDIM = MID_EPACC + 1;
// chunk-queue sync words (uncached device memory): claim counter, exit counter, launch epoch,
// per-pair flags.  A pair's flag holds the tag of the launch whose first chunk last handed its state
// over (tag = epoch + 1, the epoch advanced by the last wave out of every queued launch), so a flag
// left over from an earlier launch -- e.g. by a producer that arrived after its consumer timed out
// -- never matches: no reset store, no returning atomic.  QS_ABORT: a tape launch (p.nsteps > 1)
// stops when an env overflows the resident tier (the host replays the tape step by step).
constexpr int QS_HEAD = 0, QS_EXIT = 1, QS_EPOCH = 2, QS_ABORT = 3, QS_FLAG = 4;
// flag value of a queued hand-off: the launch tag (epoch + 1, 20 bits) and the hand-off's position
// in the launch (the env step of a tape launch and its stage), so a consumer waits for exactly its
// predecessor: stage 0 = first chunk of step t handed over, 1 = step t committed
// (QTAG_STEPS, hs_schedule.h: most env steps per tape launch)
__host__ __device__ constexpr int qtag(uint32_t epoch, int t, int stage) {
  return (int)((((epoch & 0xFFFFFu) + 1u) << 10) | (uint32_t)(2 * t + stage + 1));
}
// Cost-ordered claims: every queued launch measures each pair's duration (first chunk + last
// substep, 100 MHz realtime clock) and counts the pair into one of QNB buckets of QBIN ticks,
// heaviest first; the next queued launch claims the pairs bucket by bucket (a counting sort done
// by the previous launch), so the launch ends on the cheapest last substeps.  Bucket 0 is not a
// duration bucket: it takes the pairs with an env that will auto-reset in the next env step (its
// clock or step count already says so, hs_env_step.h resets_next), whose last item then runs the
// reset's mj_step as well -- about two substeps that no measured duration foretells.  After the flags:
// qcost[npairs] (first-chunk durations), cnt[2][QNB] (bucket counts, by epoch parity: the launch
// reads cnt[e & 1], counts into cnt[(e + 1) & 1], and its last wave out zeroes cnt[e & 1]),
// ord[2][QNB][npairs] (the pairs of each bucket).  A launch whose read counts do not sum to npairs
// (the batch's first queued launch) claims in the fixed multiplicative permutation (p.qmul).
constexpr int QNB = 32, QBIN = 2500;   // 32 buckets of 25 us
constexpr size_t qs_cost(int npairs) { return QS_FLAG + (size_t)npairs; }
constexpr size_t qs_cnt(int npairs, int par) { return QS_FLAG + 2 * (size_t)npairs + (size_t)par * QNB; }
constexpr size_t qs_ord(int npairs, int par) {
  return QS_FLAG + 2 * (size_t)npairs + 2 * QNB + (size_t)par * QNB * npairs;
}
// sized for n_envs units: the queue's unit is an env pair, or one env in the single-env mode of
// small-batch tape launches (launch_step)
constexpr size_t qsync_words(int n_envs) { return qs_ord(n_envs, 2); }

enum RewardId { REWARD_NONE = -1, REWARD_STAND = 0, REWARD_KNEELING = 1, REWARD_WALK = 2 };
// per-env warning counters: MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc resets, contacts past the
// wide tier, and a lost chunk-queue hand-off (a scheduling failure, not physics: the env is reset the
// same way and the trainer raises on it)
enum Warn { WARN_BADQPOS = 0, WARN_BADQVEL = 1, WARN_BADQACC = 2, WARN_OVERFLOW = 3, WARN_HANDOFF = 4, NWARN = 5 };
static_assert(NWARN == MID_NWARN, "hand-off row warning slots");

template <typename T>
struct EnvBuffers {
  T* qpos;               // [N][nq]
  T* qvel;               // [N][nv]
  T* qacc_ws;            // [N][nv]  (mjData.qacc_warmstart)
  T* ctrl;               // [N][nu]
  T* time;               // [N]
  int* step_count;       // [N]
  uint32_t* episode;     // [N]      reset counter (device RNG stream)
  T* total_reward;       // [N]
  int* warning;          // [N][NWARN]
  T* obs;                // [N][obs_dim]
  T* terminal_obs;       // [N][obs_dim]  written for envs that auto-reset this step
  T* reward;             // [N]
  uint8_t* terminated;   // [N]
  uint8_t* truncated;    // [N]
  T* aux;                // [N][AUXDIM]
  T* cfrc_ext;           // [N][nbody][6]  (full_state)
  T* subtree_linvel;     // [N][nbody][3]  (full_state)
  int* term_step_count;  // [N] or null: step_count of envs that auto-reset this step (SB3 final info)
  T* term_total_reward;  // [N] or null: their episode return
  int* redo;             // [2 + N] wide-tier work list: count, done counter, env ids (hs_batch owned)
  T* mid;                // [N][MIDDIM] state between the chunks of a queued env step (hs_batch owned)
  int* qsync;            // [qsync_words(N)] chunk queue: claim / exit counters, pair flags (hs_batch owned)
  unsigned long long* redo_total;   // cumulative number of wide-tier re-runs (diagnostics)
  T* dbg;                // [DBGDIM] or nullptr
};

struct StepParams {
  int mode;              // StepMode
  int nsub;              // substeps per call (frame_skip for env steps, n for physics)
  int max_steps;         // custom_env.py:201 truncation (750)
  int reward_id;         // RewardId
  int autoreset;         // SB3 VecEnv auto-reset semantics
  int obs_dim;
  int max_newton;        // Newton iteration cap
  int full_state;        // compute cfrc_ext / subtree_linvel; obs gains cfrc_ext[1:]
  double duration;       // custom_env.py:213 (10.0 in training)
  double init_height;    // custom_env.py:59 (1.282)
  double noise_scale;    // custom_env.py:109-110 (0.01)
  uint64_t seed;
  double kneel[9];       // target_height, min_height, max_roll_pitch, com_radius, energy_w, posture_w,
                         // com_w, foot_w, alive_w (reward_functions.py:71-81)
  int solver;            // SOLVER_NEWTON (MuJoCo default) or SOLVER_PGS: selects the kernel instance
  int outputs;           // OUT_* bits: optional per-env outputs written at commit
  int schedule;          // HS_SCHED_AUTO (0) / HS_SCHED_DIRECT (1) (hs_env_config.schedule)
  int queue;             // set by launch_step: 1 = chunk-queue schedule (persistent grid), 0 = one wave per pair
  int qmul;              // chunk-queue fallback claim order: item i -> pair (i * qmul) mod npairs (coprime)
  int qorder;            // chunk queue: 1 = cost-ordered claims (QNB buckets), 0 = the qmul permutation only
  int dbg_lose_pair1;    // test hook (hs_debug_lose_handoff): env + 1 from the host; launch_step turns it into the
                         // queue unit (pair or env) + 1 whose hand-off is treated as lost; 0 = off
  int single;            // set by launch_step: 1 = one env per wave (upper half-wave a ghost), 0 = env pairs
                         // (also the chunk queue's unit for small-batch tape launches)
  int nsteps;            // env steps per launch: 1, or a tape launch of nsteps (MODE_ENV_STEP, chunk queue)
};
// per-step outputs of a tape launch ([nsteps][N][...] each; null: the batch's own buffers, last step wins)
template <typename T>
struct TapeOut {
  T* obs;
  T* reward;
  uint8_t* terminated;
  uint8_t* truncated;
};
// optional outputs (hs_env_config.outputs): the aux row (qacc, subtree com, ncon, nefc, solver
// iterations -- data views and stats) and the data.ctrl copy (data views / host rewards)
enum Outputs { OUT_AUX = 1, OUT_CTRL = 2 };
enum Solver { SOLVER_NEWTON = 0, SOLVER_PGS = 1 };

// Fused PPO rollout (hs_rollout, fp64 engine): a tape launch whose actions come from the policy.
// After each env step the env's wave runs the SB3 MlpPolicy's pi net (2 hidden layers of H = 64, 128
// or 256, ReLU or Tanh) on the new obs, draws the action (the Philox stream of ppo_act_kernel) and does the
// rollout buffer bookkeeping of ppo_post_kernel, so a K-step rollout is one launch.  Rollout buffers
// are indexed by the global step g = t_begin + t.
struct RolloutArgs {
  const float* w1;      // [D][ld1] pi layer 1 ([in][out], columns 0..H-1), ld1 >= H
  const float* b1;      // [H]
  const float* w2;      // [H][H]
  const float* b2;      // [H]
  const float* w3;      // [H][A]
  const float* b3;      // [A]
  const float* log_std; // [A]
  int ld1, D, A;
  int H;                // hidden width: 64, 128 or 256 (policy_mean dispatches on it)
  int hact;             // hidden activation: ACT_RELU or ACT_TANH (hs_act.h; policy_mean dispatches on it)
  int t_begin, t_total; // global step of this launch's first step; rollout length (n_steps)
  float* obs;           // [t_total][N][D]: rows g + 1 written (row 0 is the caller's)
  float* obs_last;      // [N][D]: the obs after step t_total - 1 (the next rollout's first obs)
  float* act;           // [t_total][N][A] unclipped samples (row t_begin is the caller's)
  float* logp;          // [t_total][N]
  float* start;         // [t_total][N] episode_start before step g
  float* rew;           // [t_total][N]
  uint8_t* done;        // [t_total][N]
  double* epret;        // [t_total][N] episode return so far (ppo_post's ep_return_out)
  uint8_t* boot;        // [t_total][N] TimeLimit.truncated and not terminated
  float* tobs;          // [t_total][N][D] terminal obs of the boot envs
  double* ep_acc;       // [N] running episode return, in / out
  float* episode_start; // [N] out: done of the launch's last step
  float* act_clip;      // [N][A] in: step t_begin's clipped action; out: the next launch's
  const uint64_t* ctr_base;   // noise counter base (device); step g draws counter g + *ctr_base
  uint32_t k0, k1;            // Philox key (the 64-bit seed)
  int deterministic;
};
// Fused policy evaluation (hs_evaluate): the rollout's loop -- env step, pi net on the step's obs, the
// action handed to the pair's next step -- without the RolloutBuffer.  Of RolloutArgs it uses the policy,
// t_begin / t_total, act_clip, ctr_base / k0 / k1 / deterministic, and ro.obs as ONE [N][D] staging row per
// env (uncached memory, agent-scope accesses: rewritten every step, read back by the wave that wrote it);
// every other RolloutArgs pointer is null.  Per finished episode it writes three result slots, and for
// the envs [0, n_trace) one trace row per env step.  Memory does not grow with the number of steps
// (the trace aside).  Pointers in the batch's precision are typed by the kernel (fp64 engine only).
struct EvalArgs {
  const uint32_t* episode0;   // [N] the batch's episode counters when the evaluation began
  int max_episodes;           // E: slots e = episode - episode0[env] < E are written
  int n_trace;                // envs [0, n_trace) are traced (0: none)
  double* ep_return;          // [E][N] the env's own sum of rewards (info["total_reward"])
  int* ep_length;             // [E][N] its step count
  int* ep_end_step;           // [E][N] the global step g the episode ended in
  void* tr_qpos;              // [t_total][n_trace][nq] state the step's reward was computed from
  void* tr_qvel;              // [t_total][n_trace][nv]
  float* tr_act;              // [t_total][n_trace][A] the clipped action step g ran with
  void* tr_rew;               // [t_total][n_trace]
  uint8_t* tr_done;           // [t_total][n_trace]
};

// Observation normalisation of the fused policy's obs load (hs_rollout_norm / hs_evaluate_norm, the NORM
// kernel instances only): the policy reads clamp((obs - mean) inv_std, +-clip) (hs_norm.h) of each raw obs
// value; the rollout buffer rows and the evaluation's staging row stay raw.
struct NormArgs {
  const float* mean;      // [D]
  const float* inv_std;   // [D] 1 / sqrt(var + eps), fp32
  float clip;
};

// The fused policy's parts of a launch, as the rollout and evaluation entry points fill them (fp64 engine)
struct FusedArgs {
  RolloutArgs ro;   // absent: ro.obs null
  EvalArgs ev;      // absent: ev.episode0 null
  NormArgs nm;      // absent: nm.mean null
};

// A built-in termination condition evaluated inside a tape launch (hs_set_termination_builtin, the TERM kernel
// instances only; hs_term_builtin.h): after every env step the predicate on the post-step qpos, the grace
// counter, terminated |= early.  The count travels from an env's step to its next beside the hand-off row, in
// mid_count (uncached memory, handled like b.mid); the launch's last step commits it with the state.
// In a TERM instance an env may end several episodes in one launch, so the per-env terminal rows
// (b.terminal_obs, term_step_count, term_total_reward) are written by the launch's last step only: they are
// defined for the envs that were done on that step.
struct TermArgs {
  int kind;                 // TERM_FALLEN / TERM_LOST_BALANCE (0: none, every other instance)
  int grace_steps;          // >= 1
  double min_height, max_roll_pitch;
  int32_t* grace_count;     // [N] the batch's grace counters, read by the first step and written by the last
  int32_t* grace_episode;   // [N] the episode number each count belongs to
  uint8_t* early;           // [N] early_terminated of the launch's last step
  int32_t* mid_count;       // [N] the count between an env's steps (uncached, hs_batch owned)
};

// The bank of initial states a reset draws its start from (hs_set_initial_states; hs_env_step.h reset_draw):
// K rows of qpos / qvel in the batch precision, owned by the batch.  K = 0: the reference's reset.
template <typename T>
struct InitArgs {
  const T* q;   // [K][nq]
  const T* v;   // [K][nv]
  int K;
};

// One step launch.  The optional parts (tape, fused.*, tm, in) are held by value; a value-initialised one is
// absent: the member the kernels key on is null / 0 (fused.ro.obs, fused.ev.episode0, fused.nm.mean, tm.kind, in.K).
// p.nsteps > 1: a tape launch -- actions [nsteps][N][nu], outputs per step in `tape`, env steps of one env
// pair run back to back on the chunk queue with the state handed over through b.mid; no wide-tier launch
// follows (an overflow sets qsync[QS_ABORT], the host replays the tape).
template <typename T>
struct StepLaunch {
  const DevModel<T>* model;
  int nv;
  EnvBuffers<T> b;
  const float* actions;        // [N][nu] float32 (may be null in MODE_RESET)
  const uint8_t* reset_mask;   // [N] (null = all)
  const T *noise_qpos, *noise_qvel;   // [N][nq] / [N][nv] host-supplied reset noise (null = device RNG)
  StepParams p;
  int nenv;
  TapeOut<T> tape;
  FusedArgs fused;
  TermArgs tm;
  InitArgs<T> in;
};
template <typename T>
hipError_t launch_step(const StepLaunch<T>& s, hipStream_t stream);

// A chunk-queue kernel instance: the solver and the fused features compiled into it
enum QueueInstance : unsigned { QI_PGS = 1, QI_ROLL = 2, QI_EVAL = 4, QI_NORM = 8, QI_TERM = 16 };
// The queue instances in code objects of their own: the two with obs normalisation (QI_NORM without QI_TERM)
// and the five with a built-in termination condition (QI_TERM).  s: launch_step's request with the schedule
// plan in s.p (KArgs is private to each pass over hs_kernels.hip: every object builds its own); max_grid: the
// plan's grid; hipErrorInvalidValue: no such instance.
hipError_t launch_queue_norm(const StepLaunch<double>& s, unsigned instance, unsigned max_grid, hipStream_t stream);
hipError_t launch_queue_term(const StepLaunch<double>& s, unsigned instance, unsigned max_grid, hipStream_t stream);

// waves of the resident step-kernel instance the current device holds at once (0 if unknown)
template <typename T>
int resident_waves(bool pgs);

// mj_kinematics/mj_comPos of one state (device qpos[nq]) -> out[KINDIM] (see kin_kernel)
constexpr int KINDIM = MAXBODY * 12 + MAXGEOM * 6 + 3;
template <typename T>
hipError_t launch_kinematics(const DevModel<T>* dmodel, int nv, const T* qpos, T* out, hipStream_t stream);
// the same for n states in one launch -> out[n][KINDIM]: rows of qpos[n][nq], or (envs != null, a device
// list of n env ids) rows envs[i] of the batch's state rows state_qpos (kin_batch_kernel)
template <typename T>
hipError_t launch_kinematics_batch(const DevModel<T>* dmodel, int nv, int n, const T* qpos, const T* state_qpos,
                                   const int* envs, T* out, hipStream_t stream);

// the step kernel's reward code (reward_formula) on caller-supplied per-env fields (hs_reward_eval)
template <typename T>
struct RewardEvalArgs {
  int reward_id, n, nq, nv, nu, nbody;
  double kneel[9];            // StepParams::kneel
  const T* qpos;              // [n][nq]
  const T* qvel;              // [n][nv]
  const T* ctrl;              // [n][nu]
  const T* time;              // [n]
  const T* subtree_com0;      // [n][3]
  const T* subtree_linvel0;   // [n][3]
  const T* cfrc_ext;          // [n][nbody][6]
  const T* qfrc_actuator;     // [n][nv]
  T* out;                     // [n]
  // row strides (elements) of subtree_com0 / subtree_linvel0 / qfrc_actuator; 0 = packed (3, 3, nv) --
  // hs_reward reads the batch's own buffers in place (aux row, subtree_linvel rows, obs rows)
  int ld_com, ld_linv, ld_qfrc;
};
template <typename T>
hipError_t launch_reward_eval(const RewardEvalArgs<T>& a, hipStream_t stream);

// one step's host-bound outputs packed into one float64 buffer (hs_pack_outputs)
template <typename T>
struct PackArgs {
  int n, obs_dim, ncols, nwarn, nwarn_stride;
  const T* obs;
  const T* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const T* total_reward;
  const int* step_count;
  const int* term_step_count;
  const T* term_total_reward;
  const int* warning;
  double* out;
};
template <typename T>
hipError_t launch_pack(const PackArgs<T>& a, hipStream_t stream);

// PPO rollout bookkeeping around the policy GEMMs and the env step (ppo_rollout.hip)
hipError_t launch_ppo_act(const float* mean, int mean_ld, const float* value, int value_ld, const float* log_std,
                          const float* episode_start, uint64_t seed, uint64_t counter, const uint64_t* counter_base,
                          int deterministic, float* act,
                          float* act_clip, float* logp, float* val, float* start_out, int N, int A,
                          hipStream_t stream);
hipError_t launch_ppo_post(const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                           const float* terminal_value, const float* terminal_obs, float* boot_obs_out,
                           uint8_t* boot_out, int obs_dim, float gamma, const float* obs, float* obs_out,
                           size_t obs_floats, float* reward_out, uint8_t* done_out, double* ep_acc,
                           double* ep_return_out, float* episode_start, int N, hipStream_t stream);
// fused 2-hidden-layer (H = 64, 128 or 256; act = ACT_RELU or ACT_TANH, hs_act.h) MLP forward of one packed
// policy net (ppo_mlp.hip mlp2_fwd_kernel)
hipError_t launch_mlp2_fwd(const float* X, int ldx, int D, int N, int H, int act, const float* W1, int ld1,
                           const float* b1, const float* W2, int ld2, const float* b2, const float* W3, int ld3,
                           const float* b3, int A, float* out, int ldo, hipStream_t stream);
// column sums of a row-major [rows][cols] float32 matrix (ppo_reduce.hip); workspace of
// colsum_workspace(rows, cols) floats (0: none needed)
size_t colsum_workspace(size_t rows, size_t cols);
hipError_t launch_colsum(const float* x, size_t rows, size_t cols, const float* row_weight, float* workspace,
                         float* out, hipStream_t stream);
// diagonal-Gaussian log-prob of given actions and its backward (ppo_rollout.hip)
hipError_t launch_gauss_logp(const float* mean, int mean_ld, const float* act, const float* log_std, float* logp, int N,
                             int A, hipStream_t stream);
hipError_t launch_gauss_logp_grad(const float* mean, int mean_ld, const float* act, const float* log_std,
                                  const float* g_logp, float* g_mean, float* gls_rows, int N, int A,
                                  hipStream_t stream);
// SB3 PPO minibatch loss (clipped surrogate + value MSE) forward / backward (ppo_update.hip); workspace
// of ppo_loss_workspace(B) floats, written by the forward and read by the backward
size_t ppo_loss_workspace(int B);
hipError_t launch_ppo_loss_fwd(const float* logp, const float* v, const int64_t* idx, const float* adv,
                               const float* ret, const float* old_logp, int B, float clip, int normalize, float* pg,
                               float* vf, float* ws, hipStream_t stream);
hipError_t launch_ppo_loss_bwd(const float* logp, const float* v, int B, float clip, const float* ws,
                               const float* g_pg, const float* g_vf, float* g_logp, float* g_v, hipStream_t stream);
// The same with SB3's train controls on the device (hs_ppo_loss_ex, include/hsim.h): the float32
// hyperparameter block hp[HP_*], the control words ctl[CTL_*] and the stats block stats[ST_*]
// (== HS_PPO_HP_* / HS_PPO_CTL_* / HS_PPO_STAT_* of the header, static_assert in hs_api_ops.cpp)
constexpr int HP_LR = 0, HP_CLIP = 1, HP_CLIP_VF = 2, HP_KL_STOP = 3;
constexpr int CTL_STOP = 0, CTL_EPOCH = 1;
constexpr int ST_PG = 0, ST_VF = 1, ST_CLIPFRAC = 2, ST_ENT = 3, ST_LOSS = 4, ST_LOSS_LAST = 5, ST_COUNT = 6,
              ST_KL_LAST = 7, ST_EXPL_VAR = 8, ST_STD = 9, ST_KL = 10;
struct PpoLossEx {
  const float* hp;        // [4] device hyperparameters
  const float* log_std;   // [A] (entropy of the state-independent Gaussian)
  int A;
  float vf_coef, ent_coef;
  float* stats;           // [ST_KL + 2 n_epochs]
  int n_epochs;
  int* ctl;               // [2]
  float* kl_out;          // NULL, or where the minibatch's approx_kl goes when the decision is deferred
};
size_t ppo_loss_workspace_ex(int B);
hipError_t launch_ppo_loss_fwd_ex(const float* logp, const float* v, const int64_t* idx, const float* adv,
                                  const float* ret, const float* old_logp, const float* old_v, int B, int normalize,
                                  const PpoLossEx& x, float* pg, float* vf, float* ws, hipStream_t stream);
hipError_t launch_ppo_loss_bwd_ex(const float* logp, const float* v, int B, const float* hp, const float* ws,
                                  const float* g_pg, const float* g_vf, float* g_logp, float* g_v,
                                  hipStream_t stream);
hipError_t launch_ppo_kl_stop(const float* kl, const float* hp, float* stats, int n_epochs, int* ctl,
                              hipStream_t stream);
// clip_grad_norm_ + Adam over up to 1024 tensors (ppo_update.hip); part: adam_partials(total numel) floats.
// hp / skip non-NULL: lr = hp[HP_LR] (device), and nothing is written when *skip != 0
int adam_partials(long long total);
hipError_t launch_adam_clip(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                            float* const* step, const long long* numel, float* part, float max_norm, double lr,
                            double b1, double b2, double eps, hipStream_t stream, const float* hp = nullptr,
                            const int* skip = nullptr);
// activation-backward (act = ACT_RELU or ACT_TANH) + bias-gradient first pass, and a paired single-pass column
// sum (ppo_reduce.hip)
size_t colsum_partial_rows(size_t rows, size_t cols);
// (G W) times act'(X) (X > 0 for ReLU, 1 - X^2 for Tanh) and its per-workgroup column sums (ppo_mlp.hip
// dgrad_mask_*_kernel): the input gradient of a Linear layer fed by an activation, fused with that
// activation's backward; N = 256
hipError_t launch_dgrad_mask(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B,
                             int N, int act, float* GX, float* partial, float* workspace, hipStream_t stream);
size_t dgrad_mask_partial_rows(int B, int K);
size_t dgrad_mask_workspace(int K);
hipError_t launch_relu_colsum(const float* g, const float* y, size_t rows, size_t cols, int act, float* gm,
                              float* partial, hipStream_t stream);
hipError_t launch_colsum_pair(const float* x0, size_t rows0, size_t cols0, float* out0, const float* x1, size_t rows1,
                              size_t cols1, float* out1, hipStream_t stream);
// VecNormalize (ppo_norm.hip; include/hsim.h hs_obs_norm, hs_rms_merge, hs_return_moments, hs_reward_scale)
size_t obs_norm_workspace(size_t R, int D);
hipError_t launch_obs_norm(const float* x, size_t ldx, size_t R, int D, const float* mean, const float* inv_std,
                           float clip, float* out, size_t ldo, double* moments, void* workspace, hipStream_t stream);
hipError_t launch_rms_merge(double* state, int D, const double* sets, int nsets, size_t set_stride, double eps,
                            float* mean32, float* inv_std32, hipStream_t stream);
hipError_t launch_return_moments(const float* rew, const uint8_t* done, int T, int N, double gamma, double* carry,
                                 double* ret_ws, double* out, hipStream_t stream);
hipError_t launch_reward_scale(float* rew, int T, int N, double* state, const double* sets, int nsets,
                               size_t set_stride, double eps, double clip, double* scale_ws, hipStream_t stream);
// GAE reverse scan over [T][N] float32 rollout arrays (gae.hip)
hipError_t launch_gae(const float* rew, const float* val, const float* start, const float* last_val,
                      const float* last_done, float* adv, float* ret, int T, int N, float gamma, float lam,
                      hipStream_t stream);

}  // namespace hs
