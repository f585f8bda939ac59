/* hsim -- MI355X-native batched humanoid simulation: the drop-in C ABI.
 *
 * This is the boundary the reference's Python env would bind instead of the `mujoco`
 * pybind11 module + SB3's SubprocVecEnv.  Each entry point names the reference interface it
 * replaces (paths relative to the reference repo):
 *
 *   hs_model_load        <- mujoco.MjModel.from_xml_path(model_path)      custom_env.py:53
 *   hs_model_field       <- MjModel attribute reads (nq, nv, nu, body_mass, ...) custom_env.py:87,59-61
 *                           (+ "contact_bound": the 4 static worst-case counts of hs_batch_info)
 *   hs_batch_create      <- mujoco.MjData(model) per env                  custom_env.py:54
 *                           x SubprocVecEnv([make_env(...)] * n_envs)     train_sb3.py:203
 *   hs_set_seed          <- VecEnv.seed / np.random.seed(seed) of reset (custom_env.py:99-100)
 *   hs_set_config        <- env_config keys duration/frame_skip/reward_config custom_env.py:21-32,
 *                           train_sb3.py:183-200
 *   hs_reset             <- HumanoidEnv.reset: mj_resetData + noise + one mj_step  custom_env.py:97-150
 *   hs_step              <- HumanoidEnv.step: frame_skip x mj_step, _get_state, reward, done
 *                           custom_env.py:152-230 (+ SB3 auto-reset on done)
 *   hs_step_tape         <- K x HumanoidEnv.step over a given action tape (open loop), one launch
 *   hs_rollout(_act)     <- SB3 PPO.collect_rollouts' per-step loop (policy + env step + buffers), one launch;
 *                           pi nets of two layers of 64 (config.py's net_arch), 128 or 256, ReLU (config.py's
 *                           activation_fn) or Tanh (SB3's MlpPolicy default, policies.py)
 *   hs_evaluate          <- render_policy.py:24-41's predict(deterministic=True) / env.step loop and SB3's
 *                           evaluate_policy (common/evaluation.py): whole episodes, per-episode results
 *   hs_mlp2_forward(_h, _act) <- ActorCriticPolicy.forward's mlp_extractor + action_net / value_net GEMMs
 *                           of the same nets (policies.py, SB3 2.3.2), one launch per net
 *   hs_physics_step      <- raw `data.ctrl[:] = a; mujoco.mj_step(model, data)` custom_env.py:159-160
 *   hs_pack_outputs      <- the worker -> main-process pipe transfer of SubprocVecEnv.step_wait (obs,
 *                           rewards, dones, info values; train_sb3.py:203): one packed device buffer
 *   hs_reward_eval       <- REWARD_FUNCTIONS[type](data, params) reward_functions.py:66-269 (the device
 *                           formulas of hs_step on supplied fields)
 *   hs_reward            <- the same on the batch's current states (custom_env.py:263-271 _compute_reward)
 *   hs_reward_program_*  <- a user's entry in REWARD_FUNCTIONS (reward_functions.py:264-269), compiled to a
 *                           reward program: create / destroy / info, eval_host (CPU, double), eval (device
 *                           fields), batch (the batch's states)
 *   hs_step_program      <- HumanoidEnv.step with such a reward (custom_env.py:152-230): step, program, masked reset
 *   hs_set_termination   <- the fall conditions custom_env.py:167-200 holds commented out (height < 0.8 for a
 *                           grace period; height < 0.8 or |roll|, |pitch| > 45 deg): a predicate on the post-step
 *                           state that ends the episode; hs_apply_termination (its outcome launch alone),
 *                           hs_termination_state (its buffers), hs_termination_eval_host (CPU, double)
 *   hs_debug_lose_handoff   (test hook: mj_step's warning + mj_resetData path, custom_env.py:160)
 *   hs_debug_queue_order    (test view of the chunk queue's next claim order; no counterpart)
 *   hs_debug_queue_counters (test view of the chunk queue's claim / exit counters; no counterpart)
 *   hs_last_tape_ms, hs_tape_aborts, hs_stream_orders, hs_batch_counters   (diagnostics)
 *   hs_state_io          <- reads/writes of data.qpos/qvel/qacc_warmstart/time/ctrl (custom_env.py:105-117)
 *   hs_kinematics        <- the pose fields mujoco.Renderer.update_scene reads from one mjData
 *   hs_kinematics_batch  <- the same for n poses (env states or recorded qpos rows) in one launch, on the device
 *   hs_render_frames     <- mujoco.Renderer.update_scene + render (custom_env.py:273-289) for n frames in one
 *                           launch: the video path of custom_env.py:291-321, train_sb3.py:13-61, render_policy.py
 *   hs_get_buffers       <- data.* arrays as device buffers (obs, reward, terminated, ...)
 *   hs_last_error        <- mujoco's error callback / MjModel load error string
 *   hs_gae               <- SB3 RolloutBuffer.compute_returns_and_advantage (stable_baselines3 2.3.2
 *                           common/buffers.py), run by PPO.learn once per rollout (train_sb3.py:229)
 *   hs_ppo_act           <- SB3 PPO.collect_rollouts per step (on_policy_algorithm.py, 2.3.2): the
 *                           DiagGaussian sample + log_prob of ActorCriticPolicy.forward, np.clip of
 *                           the actions, RolloutBuffer.add of actions/values/log_probs/episode_starts
 *   hs_ppo_post          <- the same loop after env.step: TimeLimit.truncated bootstrap of the reward,
 *                           dones, episode returns, new episode_starts, next obs into the buffer
 *   hs_gauss_logp(_grad) <- DiagGaussianDistribution.log_prob of the buffered actions in the PPO
 *                           update (SB3 ActorCriticPolicy.evaluate_actions) and its backward
 *   hs_ppo_loss(_grad)   <- SB3 PPO.train's minibatch loss: advantage normalisation, clipped
 *                           surrogate, value MSE (stable_baselines3 2.3.2 ppo/ppo.py) and its backward
 *   hs_adam_clip         <- torch.nn.utils.clip_grad_norm_(max_grad_norm) + torch.optim.Adam.step of
 *                           SB3 PPO.train (ppo.py: max_grad_norm 0.5, Adam eps 1e-5)
 *   hs_ppo_loss_ex(_grad_ex), hs_ppo_kl_stop, hs_adam_clip_ex <- the same update with SB3 PPO.train's
 *                           target_kl early stop, clip_range_vf, per-iteration schedules and logged
 *                           statistics (approx_kl, clip_fraction, entropy_loss, loss) decided and
 *                           accumulated on the device, so a captured epoch needs no host check
 *   hs_dgrad_mask, hs_dgrad_act <- the input gradient of each layer fed by an activation (ReLU; ReLU or
 *                           Tanh), fused with that activation's backward (same loss.backward())
 *   hs_relu_grad_colsum, hs_act_grad_colsum, hs_colsum_pair <- the activation backward (threshold_backward /
 *                           tanh_backward) + bias / weight-gradient sums of the same loss.backward()
 *                           (fewer passes and launches)
 *   hs_colsum            <- the bias-gradient and split-K weight-gradient reductions of the PPO
 *                           update's loss.backward() (SB3 PPO.train, ppo.py; train_sb3.py:229)
 *
 * Conventions: status int (0 ok, <0 error, message via hs_last_error(), thread-local); the
 * model is immutable and shareable; a batch owns (or is bound to) device buffers; every call
 * takes an optional HIP stream (NULL = default stream) and is asynchronous unless noted; a
 * batch is not re-entrant.  No torch types cross this boundary.
 * Launches of ONE batch are ordered by the library: like one mjData, a batch is a single state (two
 * unordered launches would race on every buffer, and on the chunk-queue schedule share the batch's
 * claim counters, so pairs could be stepped twice or skipped).  A call on another stream than the
 * batch's previous call first makes its stream wait for everything already issued on the old one
 * (an event; counted by hs_stream_orders).  Streams in graph capture are not joined this way: the
 * capturing framework orders a capture against its origin stream.  The library keeps the handle of a
 * batch's last stream to record that event, so a stream a batch was launched on must stay alive until
 * the batch's next call (or hs_batch_destroy).
 * Uncached memory (the chunk queue's hand-off rows and sync words, ~1.2 KB per fp64 env) is recycled
 * within the process as uncached memory only, in power-of-two size classes >= 64 KB: the process keeps
 * at most the peak of concurrently live uncached memory of each class, each block up to twice its
 * request, until it exits.
 */
#ifndef HSIM_H
#define HSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_model hs_model;
typedef struct hs_batch hs_batch;

enum { HS_FP32 = 0, HS_FP64 = 1 };
/* OR-ed into hs_batch_create's `precision` argument: the full-state option.  cfrc_ext (contact
 * wrenches, mj_rnePostConstraint) and subtree_linvel (mj_subtreeVel) are computed every substep
 * and the observation gains cfrc_ext[1:] -- the reference's commented-out obs component
 * (custom_env.py:247,255) -- so obs_dim = 352 + 6 (nbody - 1) = 448 for humanoid.xml; rewards then
 * read the real foot forces / com velocity.  Off (default) = the reference's zeros. */
enum { HS_FULL_STATE = 0x100 };
enum { HS_REWARD_NONE = -1, HS_REWARD_STAND = 0, HS_REWARD_KNEELING = 1, HS_REWARD_WALK = 2 };
/* Per-env warning counters (hs_buffers.warning): MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc
 * resets (mj_step's mju_warning + mj_resetData, custom_env.py:160), contacts dropped past the wide
 * tier, and HS_WARN_HANDOFF: a lost chunk-queue hand-off (a scheduling failure -- e.g. more concurrent
 * queued batches than the GPU holds -- after which the env was reset like a bad state). */
enum { HS_WARN_BADQPOS = 0, HS_WARN_BADQVEL = 1, HS_WARN_BADQACC = 2, HS_WARN_OVERFLOW = 3, HS_WARN_HANDOFF = 4,
       HS_NWARN = 5 };
#define HS_AUXDIM 40   /* per env aux row: qacc[32], com[3], ncon, nefc, newton iterations, pad */
/* Optional per-env outputs (hs_env_config.outputs).  HS_OUT_AUX: the aux row (qacc, subtree com,
 * contact / row counts, solver iterations) that data views and statistics read.  HS_OUT_CTRL: the
 * data.ctrl copy (the action; data views and host reward callables read it,
 * reward_functions.py:194).  A trainer on the device reward needs neither. */
enum { HS_OUT_AUX = 1, HS_OUT_CTRL = 2 };

/* Env semantics (custom_env.py defaults in brackets; train_sb3.py overrides in parentheses). */
typedef struct {
  int frame_skip;          /* [5] (3)   custom_env.py:28, train_sb3.py:199 */
  int max_steps;           /* [750]     custom_env.py:201 forced truncation */
  int reward_id;           /* HS_REWARD_*; reward_config['type'] custom_env.py:263-271 */
  int autoreset;           /* 1 = SB3 VecEnv auto-reset (terminal obs kept in terminal_obs) */
  int max_newton;          /* Newton iteration cap [100 = opt.iterations] */
  int outputs;             /* HS_OUT_* bits: optional per-env outputs [all] */
  double duration;         /* [15] (10.0) custom_env.py:23, train_sb3.py:187 */
  double init_height;      /* 1.282   custom_env.py:59 */
  double noise_scale;      /* 0.01    custom_env.py:109-110 */
  double kneel_params[9];  /* reward_functions.py:71-81: target_height, min_height, max_roll_pitch,
                              com_radius, energy_weight, posture_weight, com_weight, foot_weight,
                              alive_weight */
  int schedule;            /* HS_SCHED_*: how the step kernel maps env pairs to waves [AUTO] */
} hs_env_config;

/* hs_env_config.schedule.  AUTO: one wave per env (the upper half-wave mirrors the lower one and
 * commits nothing) when every env gets a resident wave of its own (small batches, e.g. configs[4]'s
 * 1024 envs per GPU); else one wave per env pair when every pair fits on the GPU at once; else (the
 * fp64 engine at 4096 envs) a persistent grid that runs each env step as two chunk items (substeps
 * [0, frame_skip - 1), then the last substep + obs / reward / auto-reset) from a queue.
 * The queue claims the pairs heaviest first by the durations its previous launch measured.
 * DIRECT: always one wave per pair.  SINGLE: always one wave per env.  FIXED_ORDER: AUTO with the
 * queue's claims in a fixed permutation (A/B runs, tests).  Results are bitwise identical
 * whichever schedule runs. */
enum { HS_SCHED_AUTO = 0, HS_SCHED_DIRECT = 1, HS_SCHED_SINGLE = 2, HS_SCHED_FIXED_ORDER = 3 };

/* Device buffers of a batch (row-major, env-major).  Element type of the T* entries is float
 * (HS_FP32) or double (HS_FP64). */
typedef struct {
  void* qpos;              /* [N][nq]  */
  void* qvel;              /* [N][nv]  */
  void* qacc_warmstart;    /* [N][nv]  */
  void* ctrl;              /* [N][nu]  */
  void* time;              /* [N]      */
  int32_t* step_count;     /* [N]      */
  uint32_t* episode;       /* [N]      */
  void* total_reward;      /* [N]      */
  int32_t* warning;        /* [N][HS_NWARN] */
  void* obs;               /* [N][obs_dim]  custom_env.py:242-256 layout */
  void* terminal_obs;      /* [N][obs_dim]  obs before auto-reset (SB3 info["terminal_observation"]) */
  void* reward;            /* [N]      */
  uint8_t* terminated;     /* [N]      */
  uint8_t* truncated;      /* [N]      */
  void* aux;               /* [N][HS_AUXDIM] */
  void* cfrc_ext;          /* [N][nbody][6]  (torque, force) at the root subtree com; HS_FULL_STATE only */
  void* subtree_linvel;    /* [N][nbody][3]  HS_FULL_STATE only */
  int32_t* terminal_step_count;  /* [N] or NULL: info["step_count"] of envs that auto-reset this step */
  void* terminal_total_reward;   /* [N] or NULL: their info["total_reward"] (custom_env.py:216-224) */
} hs_buffers;

typedef struct {
  int n_envs, precision, nq, nv, nu, nbody, obs_dim, elem_size;
  /* per-env contact / constraint-row capacity of the resident kernel tier (every launch) and of the
   * wide tier that re-runs the envs overflowing it; only wide-tier overflow drops contacts
   * (HS_WARN_OVERFLOW).  MuJoCo has no per-env cap (custom_env.py:160). */
  int resident_con, resident_efc, wide_con, wide_efc;
  /* waves of the resident step kernel the device holds at once (2 envs per wave); with more env
   * pairs than this, HS_SCHED_AUTO runs multi-substep calls on the chunk-queue schedule */
  int resident_waves;
  /* static worst case of one env from the model's collision pair list (most contacts per pair
   * type x rows per contact, + one row per limited joint / tendon): every pair touching at once
   * (geometric, unreachable) and every geom on the floor at once (a flat-lying body).  Models
   * whose floor bound exceeds the wide tier are rejected by hs_batch_create. */
  int bound_con_all, bound_efc_all, bound_con_floor, bound_efc_floor;
} hs_batch_info;

hs_model* hs_model_load(const char* xml_path, char* err, int errsz);
void hs_model_free(hs_model* m);
int hs_model_field(const hs_model* m, const char* name, double* out, int n);
/* The model's lane table: the constants the step kernel reads at a per-lane index, packed by the model
 * compiler for one precision (HS_FP32 / HS_FP64); the fp64 kernels keep a copy in LDS.  Introspection
 * for tests, no device needed.
 * hs_model_lane_table: the table's size in bytes (copied to `out` if nbytes holds it), -1 on error.
 * hs_lane_layout: the number of entries; for 0 <= i < that, entry i's name (the compiled model's field
 *   it packs), byte offset in the table, element count and element kind (0: the precision's real, 1: uint32,
 *   2: int8).  Any output pointer may be NULL.
 * hs_model_lane_source: the compiled model's field `name` itself, flattened, as doubles: the number of
 *   values (written if n holds them), -1 if the table has no such entry. */
int hs_model_lane_table(const hs_model* m, int precision, void* out, int nbytes);
int hs_lane_layout(int precision, int i, char* name, int namesz, int* offset, int* count, int* kind);
int hs_model_lane_source(const hs_model* m, int precision, const char* name, double* out, int n);

/* external == NULL: the library allocates (hipMalloc) and owns the buffers.
 * external != NULL: every pointer must be a device buffer of the documented size on `device`;
 * the caller keeps ownership (used by the Python layer to hand in torch-allocated tensors). */
hs_batch* hs_batch_create(const hs_model* m, int n_envs, int device, uint64_t seed, int precision /* | flags */,
                          const hs_buffers* external);
void hs_batch_destroy(hs_batch* b);
int hs_batch_get_info(const hs_batch* b, hs_batch_info* out);
/* The schedule the batch, as configured, runs an env step of `nsub` substeps on (n_steps = 1), or a tape launch
 * of n_steps > 1 such steps: *queue = 1 for the chunk queue, *single = 1 when a wave steps one env, not a pair
 * (with the queue: its unit).  The launches follow the same plan.  -1 when the batch cannot run that tape launch. */
int hs_batch_schedule(const hs_batch* b, int nsub, int n_steps, int* queue, int* single);
int hs_get_buffers(const hs_batch* b, hs_buffers* out);
int hs_set_config(hs_batch* b, const hs_env_config* cfg);
/* Base seed of the on-device reset RNG (VecEnv.seed; SB3 seeds workers with seed + rank). */
int hs_set_seed(hs_batch* b, uint64_t seed);
int hs_get_config(const hs_batch* b, hs_env_config* cfg);

/* mask: [N] uint8 device (NULL = all envs).  qpos_noise/qvel_noise: [N][nq]/[N][nv] device
 * arrays of the batch precision with the reset noise (NULL = on-device counter RNG). */
int hs_reset(hs_batch* b, const uint8_t* mask, const void* qpos_noise, const void* qvel_noise, void* stream);
/* actions: [N][nu] float32 device. Runs frame_skip substeps, writes obs/reward/terminated/truncated. */
int hs_step(hs_batch* b, const float* actions, void* stream);
/* Per-step outputs of hs_step_tape, device arrays (batch precision for obs / reward):
 * obs [K][N][obs_dim], reward [K][N], terminated / truncated [K][N] uint8. */
typedef struct hs_tape_out {
  void* obs;
  void* reward;
  uint8_t* terminated;
  uint8_t* truncated;
} hs_tape_out;
/* K = n_steps consecutive hs_step calls over an action tape: actions [K][N][nu] float32 device.
 * Same results, bitwise, as K hs_step calls (states, per-step obs / reward / done flags, auto-resets
 * and their final-step info; the terminal obs / info rows hold each env's last finished episode).
 * One launch on the chunk-queue schedule with whole env steps as items: an env pair's step t + 1
 * starts as soon as its own step t is committed, so steps of different pairs overlap and the launch
 * does not end every step on its slowest pair.  out = NULL: only the batch's buffers (last step);
 * otherwise every step's outputs, and the batch buffers as after the last step.  If an env overflows
 * the resident contact tier the launch stops and the tape is replayed step by step (counted by
 * hs_tape_aborts).  Synchronizes the stream.  K >= 1: the host splits the tape into launches of at
 * most min(the shortest episode, 511) steps (hs_rollout_max_steps).  With HS_SCHED_DIRECT / SINGLE, or
 * K = 1, it runs the K hs_step calls.  Open-loop stepping (a given action tape: benchmarks,
 * trajectory evaluation); a policy in the loop steps with hs_step. */
int hs_step_tape(hs_batch* b, const float* actions, int n_steps, const hs_tape_out* out, void* stream);
/* tape launches of this batch that were replayed step by step (resident-tier overflow) */
int hs_tape_aborts(const hs_batch* b, uint64_t* n);
/* duration in ms of the last tape / rollout kernel launch of this batch (hs_step_tape, hs_rollout), from
 * HIP events recorded around it on its stream; -1 before the first one (diagnostics: the bench's roofline) */
int hs_last_tape_ms(const hs_batch* b, double* ms);
/* cross-stream waits the library inserted to keep this batch's launches ordered (diagnostics) */
int hs_stream_orders(const hs_batch* b, uint64_t* n);

/* Hidden-layer activation of a policy net: SB3's policy_kwargs["activation_fn"] -- nn.ReLU (the reference's
 * config.py) or nn.Tanh (the default of ActorCriticPolicy, policies.py, SB3 2.3.2).  The Tanh is one
 * function in every kernel: sign(x) (1 - 2 / (exp(2 |x|) + 1)), odd, exact at 0, +-1 beyond |x| = 16,
 * within ~2^-23 of the exact tanh. */
#define HS_ACT_RELU 0
#define HS_ACT_TANH 1

/* Fused PPO rollout (the fp64 Newton engine).  The SB3 MlpPolicy's pi net -- two hidden layers of
 * the same width `hidden` (64, 128 or 256), ReLU or Tanh (the `act` of hs_rollout_act; the struct does
 * not carry it), then the action head, fp32 -- with [in][out]
 * row-major weights and the DiagGaussian log_std:
 *   w1 [obs_dim][ld1], columns 0..hidden-1 the pi net's (b1 [hidden]);
 *   w2 [hidden][hidden] (b2 [hidden]);
 *   w3 [hidden][act_dim] (b3 [act_dim]);
 *   ld1 >= hidden, ld1 % 4 == 0.
 * hidden = 0 means 256 (callers from before the field).  The struct must be zero-initialised
 * (hs_policy p = {0};) before its fields are filled in, so that a caller that does not know `hidden`
 * passes 0 and not an indeterminate value.  `hidden` sits in what was tail padding: the size stays 72. */
typedef struct hs_policy {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *log_std;
  int ld1, obs_dim, act_dim;
  int hidden;
} hs_policy;
/* The RolloutBuffer of SB3 PPO.collect_rollouts (on_policy_algorithm.py, 2.3.2) for t_total steps of
 * N envs, device arrays: obs [t_total][N][obs_dim] (row 0 = the rollout's first obs), obs_last
 * [N][obs_dim] (the obs after the last step), actions [t_total][N][act_dim] (unclipped samples),
 * log_probs / episode_starts / rewards [t_total][N] f32, dones / boot [t_total][N] u8 (boot:
 * TimeLimit.truncated and not terminated), episode_returns [t_total][N] f64, terminal_obs
 * [t_total][N][obs_dim] (rows of the boot envs), ep_acc [N] f64 (running return, in / out),
 * episode_start [N] f32 (out), actions_clipped [N][act_dim] (in: step t_begin's clipped action;
 * out: step t_begin + n_steps'), counter_base (device u64) and seed: the noise of hs_ppo_act. */
typedef struct hs_rollout_bufs {
  float* obs;
  float* obs_last;
  float* actions;
  float* log_probs;
  float* episode_starts;
  float* rewards;
  uint8_t* dones;
  double* episode_returns;
  uint8_t* boot;
  float* terminal_obs;
  double* ep_acc;
  float* episode_start;
  float* actions_clipped;
  const uint64_t* counter_base;
  uint64_t seed;
  int deterministic;
} hs_rollout_bufs;
/* Steps [t_begin, t_begin + n_steps) of a PPO rollout in ONE launch: hs_step with the given clipped
 * action for step t_begin, then for every later step the policy forward on the returned obs, the
 * Gaussian sample (hs_ppo_act's Philox stream, counter step + *counter_base), the clip, and
 * hs_ppo_post's bookkeeping (rewards, dones, episode returns, bootstrap flags / terminal obs, the
 * next obs row, episode_start) -- on each env's wave, each env pair's step t + 1 starting when its
 * own step t is done.  Replaces the per-step loop of SB3 collect_rollouts (train_sb3.py:229 ->
 * on_policy_algorithm.py) for envs stepped by this engine; values are evaluated after the rollout.
 * n_steps <= hs_rollout_max_steps(b) (the shortest episode, at most 511 steps; 511 with a fused-capable termination
 * condition, hs_set_termination_builtin).  Returns 0, or 1 when an env overflowed
 * the resident contact tier: the env state, ep_acc, episode_start and actions_clipped are restored
 * to the call's start, and the caller collects these steps step by step (hs_step).  Synchronizes. */
int hs_rollout(hs_batch* b, const hs_policy* pol, const hs_rollout_bufs* rb, int t_begin, int n_steps, int t_total,
               void* stream);
/* hs_rollout for a pi net whose hidden activation is `act` (HS_ACT_RELU or HS_ACT_TANH; anything else is an
 * error): the same per-step loop of SB3 collect_rollouts (on_policy_algorithm.py) for an MlpPolicy built with
 * activation_fn = nn.ReLU or nn.Tanh (policies.py).  hs_rollout is this with HS_ACT_RELU; hs_policy and
 * hs_rollout_bufs are the same structs. */
int hs_rollout_act(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb, int t_begin, int n_steps,
                   int t_total, void* stream);
int hs_rollout_max_steps(const hs_batch* b);

/* Closed-loop policy evaluation over whole episodes (the fp64 Newton engine): what render_policy.py:24-41
 * does one env.step at a time (obs -> model.predict(obs, deterministic=True) -> env.step, "make deterministic
 * (critical)"), train_sb3.py:52-60's VideoRecorderCallback and generate_trajectories.py do the same way, and
 * SB3's evaluate_policy sums up (common/evaluation.py, 2.3.2: per env the episode's rewards and its length).
 * The struct must be zero-initialised before its fields are filled in.  Device arrays:
 *   actions_clipped [N][act_dim] f32, in: step t_begin's clipped action; out: step t_begin + n_steps';
 *   episode0 [N] u32: the batch's episode counters (hs_buffers.episode) when the evaluation began;
 *   ep_return [max_episodes][N] f64, ep_length / ep_end_step [max_episodes][N] i32: when env i ends its
 *     episode number e (counted from episode0[i]) at global step g, slot [e][i] gets the env's own sum of
 *     rewards (info["total_reward"], custom_env.py:216-224), its step count, and g; e >= max_episodes: nothing;
 *   trace (n_trace > 0; envs 0 .. n_trace - 1, row [g][env] of each): trace_qpos [t_total][n_trace][nq] and
 *     trace_qvel [..][nv] in the batch precision -- the state the step's reward was computed from (on a done
 *     step the terminal state, not the reset one) --, trace_actions [..][act_dim] f32 (the clipped action
 *     step g ran with), trace_rewards [..] (batch precision), trace_dones [..] u8;
 *   counter_base (device u64), seed, deterministic: hs_ppo_act's noise, step g draws counter g + *counter_base
 *     (deterministic != 0: the action is the mean). */
typedef struct hs_eval_bufs {
  float* actions_clipped;
  const uint32_t* episode0;
  int max_episodes;
  int n_trace;
  double* ep_return;
  int32_t* ep_length;
  int32_t* ep_end_step;
  void* trace_qpos;
  void* trace_qvel;
  float* trace_actions;
  void* trace_rewards;
  uint8_t* trace_dones;
  const uint64_t* counter_base;
  uint64_t seed;
  int deterministic;
} hs_eval_bufs;
/* Steps [t_begin, t_begin + n_steps) of an evaluation of t_total steps in ONE launch: hs_step with the
 * given clipped action for step t_begin, then for every later step the policy forward (hs_policy, `act` as
 * hs_rollout_act) on the step's obs, the mean or its Gaussian sample, the clip -- on each env's wave, as
 * hs_rollout_act, but with no rollout buffer: device memory does not grow with the number of steps (the
 * trace aside; the step's obs is staged in one library-owned [N][obs_dim] f32 row per env).  Same
 * preconditions and n_steps <= hs_rollout_max_steps(b) as hs_rollout_act.  Returns 0, or 1 when an env
 * overflowed the resident contact tier: the env state and actions_clipped are restored to the call's start
 * (result slots and trace rows of steps >= t_begin may hold anything), and the caller runs these steps one
 * hs_step at a time.  < 0: error (hs_last_error).  Synchronizes; hs_last_tape_ms covers the launch. */
int hs_evaluate(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, int t_begin, int n_steps,
                int t_total, void* stream);
/* VecNormalize's observation moments for the fused policy (SB3 2.3.2 common/vec_env/vec_normalize.py):
 * device arrays mean [obs_dim] and inv_std [obs_dim] (float32; 1 / sqrt(var + epsilon), as hs_rms_merge
 * writes them) and clip_obs.  The struct must be zero-initialised before its fields are filled in. */
typedef struct hs_obs_norm_args {
  const float* mean;
  const float* inv_std;
  float clip;
  int obs_dim;      /* must equal the batch's obs_dim */
} hs_obs_norm_args;
/* hs_rollout_act on a VecNormalize-wrapped env <- VecNormalize.step_wait's normalize_obs in front of
 * PPO.collect_rollouts' policy forward: the policy inside the kernel reads clamp((obs - mean) inv_std, +-clip)
 * of every obs value (the same fp32 expression as hs_obs_norm, bitwise), computed as the obs row is
 * loaded.  The rollout buffer rows (obs, obs_last, terminal_obs) are written RAW, as by hs_rollout_act: the
 * caller normalises them afterwards in one hs_obs_norm pass with the same moments, which stay fixed for the
 * whole rollout.  Every other argument, the return values and the overflow undo are hs_rollout_act's. */
int hs_rollout_norm(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb,
                    const hs_obs_norm_args* norm, int t_begin, int n_steps, int t_total, void* stream);
/* hs_evaluate for a policy trained on normalised obs <- evaluate_policy(model, VecNormalize(env,
 * training=False)): the policy reads the normalised obs as above, the moments are not updated, the
 * staging rows stay raw and the episode returns are the env's raw ones. */
int hs_evaluate_norm(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, const hs_obs_norm_args* norm,
                     int t_begin, int n_steps, int t_total, void* stream);
/* Auto-reset noise source of hs_step: [N][nq] / [N][nv] device arrays of the batch precision with
 * the raw U(-noise_scale, noise_scale) draws of the NEXT reset of each env (the kernel applies the
 * x0.1 height factor and zeroes the quaternion part, custom_env.py:109-114); NULL, NULL = the
 * on-device counter RNG (default).  The caller refreshes an env's row after it auto-resets -- the
 * SubprocVecEnv-exact mode where worker i continues its own np.random stream seeded with
 * seed + i (custom_env.py:99-110, SB3 VecEnv.seed).  The arrays stay owned by the caller. */
int hs_set_autoreset_noise(hs_batch* b, const void* qpos_noise, const void* qvel_noise);
/* Where an episode begins.  Bind (n_states > 0) or unbind (n_states == 0) the bank of initial states resets draw
 * from.  qpos [K][nq], qvel [K][nv] or NULL (zeros): HOST doubles.  The library converts them to the batch
 * precision, copies them to the device and owns the copy.  With a bank bound, every reset -- hs_reset and the
 * auto-reset inside hs_step, hs_step_tape, hs_rollout* and hs_evaluate* alike -- starts its episode from row
 *   j = min(K - 1, floor(u K)),
 * u the [0, 1) value of the reset noise's counter hash at (seed, env, new episode number, slot 128), a slot no
 * noise draw uses; the index comes from that hash whichever noise source is bound.  Then qpos = row + noise and
 * qvel = row + noise with the noise of an unbound reset (the hs_reset arguments or the hs_set_autoreset_noise rows
 * if given, else the counter RNG; U(+-noise_scale), the free joint's height noise x0.1, no quaternion noise);
 * init_height and the upright quaternion are not imposed, the row supplies them.  ctrl = 0, time = 0 and the one
 * mj_step of the reset are as ever.  The draw is uniform over the rows: repeat a row to weight it.  With no bank
 * bound a reset is the reference's own (custom_env.py:97-130), and a bank of the one row (qpos0 with z =
 * init_height and the upright quaternion; zero qvel) gives bitwise that reset.
 * Refused (-1, the reason in hs_last_error): n_states < 0 or above HS_MAX_INITIAL_STATES, NULL qpos with
 * n_states > 0, a value that is not finite, a zero free-joint quaternion.  The free joint's quaternion of every row
 * is normalised (q / sqrt(w w + x x + y y + z z)) before it is stored.
 * The call waits for the batch's pending launches on every stream, so the next launch sees the new bank and no
 * earlier one does.  A launch recorded into a HIP graph keeps the bank (pointers and row count) it was recorded
 * with: re-record it after a rebind.  The memory it points to stays the batch's until the batch is destroyed.
 * A floor-lying row can overflow the resident contact tier during the reset's mj_step: a per-step launch re-runs
 * the env in the wide tier, a fused launch aborts and is replayed step by step (hs_tape_aborts). */
#define HS_MAX_INITIAL_STATES 4096
int hs_set_initial_states(hs_batch* b, int n_states, const double* qpos, const double* qvel);
/* *n_states = the rows bound (0: none). */
int hs_get_initial_states(const hs_batch* b, int* n_states);
/* One step's host-bound outputs in ONE launch, for a single device-to-host copy (the SubprocVecEnv
 * step_wait / Gym step() return values, custom_env.py:216-230, train_sb3.py:203): writes the float64
 * device buffer out = [obs N x obs_dim][ncols x N columns of reward, terminated, truncated,
 * total_reward, step_count, terminal_step_count, terminal_total_reward (first ncols of them)]
 * [warnings ? HS_NWARN x N warning counters (kind-major) : nothing].  Asynchronous on `stream`. */
int hs_pack_outputs(hs_batch* b, double* out, int ncols, int warnings, void* stream);
/* ctrl: [N][nu] float32 device (NULL = keep current ctrl).  nsub raw mj_step's, obs refreshed.
 * Resets and raw physics calls always write data.ctrl; env steps (hs_step) only with HS_OUT_CTRL.
 * After an hs_step with HS_OUT_CTRL off the ctrl buffer no longer holds data.ctrl, and until it is
 * rewritten (a full hs_reset, an hs_physics_step with ctrl, an hs_state_io set of ctrl) both
 * hs_physics_step(ctrl = NULL) and an hs_state_io get of ctrl fail instead of using it. */
int hs_physics_step(hs_batch* b, const float* ctrl, int nsub, void* stream);
/* Test hook of the chunk-queue schedule (never used on the product path): from the next launch on,
 * the hand-off of env `env`'s pair (env / 2) is treated as lost by its consumer item, exactly as
 * if its bounded wait had timed out -- both envs of the pair are reset as mj_checkPos resets a bad
 * state (qpos0, qvel 0, time 0), HS_WARN_HANDOFF += 1, and the step continues from there.
 * env = -1 turns it off.  Only launches on the queued schedule consult it. */
int hs_debug_lose_handoff(hs_batch* b, int env);
/* Debug view of the chunk queue (tests only): the order in which the batch's next queued launch
 * will claim its units (env pairs; single envs for a batch small enough that every env has a
 * resident wave of its own) -- the bucket lists the previous queued launch filed, concatenated,
 * bucket 0 (the pairs with an env about to auto-reset) first.  Writes min(count, n) unit indices
 * to `out` and returns the count; 0 when that launch would claim in the fixed permutation (no
 * queued launch yet, or a schedule other than HS_SCHED_AUTO); -1 on error.  Synchronous. */
int hs_debug_queue_order(hs_batch* b, int* out, int n);
/* Debug view of the chunk queue's sync words (tests only): out[0..3] = claim counter, exit counter,
 * launch epoch, tape-abort word.  Between launches both counters are 0 (the last wave out of every
 * queued launch resets them) and the epoch counts the queued launches so far.  Returns 0, or -1 on
 * error (a batch without queue buffers included).  Synchronous. */
int hs_debug_queue_counters(hs_batch* b, int* out);

/* Synchronous host<->device state copy in fp64.  dir 0: device -> host, 1: host -> device.
 * Any pointer may be NULL.  Arrays are [N][nq], [N][nv], [N][nv], [N], [N][nu]. */
int hs_state_io(hs_batch* b, int dir, double* qpos, double* qvel, double* qacc_warmstart, double* time,
                double* ctrl);
/* mj_kinematics + mj_comPos of env `env` (visualisation; the pose data mujoco.Renderer.update_scene
 * reads from mjData at custom_env.py:284-288).  qpos: nq fp64 values to pose instead of the env's
 * current state (NULL = current).  Outputs, each nullable: xpos [nbody][3], xmat [nbody][9],
 * geom_xpos [ngeom][3], geom_zaxis [ngeom][3] (capsule axis), com [3] (subtree_com of the root).
 * Synchronous; not on the step path. */
int hs_kinematics(hs_batch* b, int env, const double* qpos, double* xpos, double* xmat, double* geom_xpos,
                  double* geom_zaxis, double* com);
/* One kinematics record: [xpos MAXBODY*3][xmat MAXBODY*9][geom_xpos MAXGEOM*3][geom z-axis MAXGEOM*3][com 3]
 * values of the batch's precision, with the engine's capacities MAXBODY = 20, MAXGEOM = 24 (rows past the
 * model's nbody / ngeom are not written). */
#define HS_KINDIM 387
/* hs_kinematics for n poses in one launch, device to device: record i (HS_KINDIM values of the batch's
 * precision) goes to kin_dev[i].  The poses are either rows of qpos_dev [n][nq] (device, the batch's
 * precision) or, with envs (n env ids in HOST memory, read before the call returns), the current states of
 * those envs; exactly one of the two is non-NULL.  The env ids are checked against [0, N) before anything is
 * launched.  Asynchronous on `stream`, ordered like every launch of the batch; the env states are only
 * read.  The device copy of the id list is the batch's own (grown on demand, no per-call allocation). */
int hs_kinematics_batch(hs_batch* b, int n, const int32_t* envs, const void* qpos_dev, void* kin_dev, void* stream);

/* The camera of hs_render_frames.  HS_CAM_BODY: position xpos[body] + xmat[body] pos, rotation
 * xmat[body] rot (an MJCF camera of mode "fixed").  HS_CAM_COM: position com + pos, rotation rot (mode
 * "trackcom" with its offset and rotation at qpos0, and the free camera, pos = -distance x forward).
 * rot is row-major with the camera's x, y, z axes as columns (it looks along -z); fovy in degrees. */
enum { HS_CAM_BODY = 0, HS_CAM_COM = 1 };
typedef struct {
  int mode;        /* HS_CAM_* */
  int body;        /* HS_CAM_BODY: the body the camera is attached to, in [0, nbody) */
  double pos[3];
  double rot[9];
  double fovy;     /* in (0, 180) */
} hs_camera;
/* Ray-cast n frames <- mujoco.Renderer.update_scene(data, camera) + render() (custom_env.py:284-288): frame i
 * draws kinematics record kin_dev[i] (hs_kinematics_batch) from `cam` into rgb_dev[i] of
 * uint8 rgb_dev[n][H][W][3] (device).  The scene is the model's plane, spheres and capsules in the "body"
 * material, the 0.5 m checker floor, the gradient sky, a headlight and the "top" light above the COM;
 * fp64 per pixel, the arithmetic of the package's host renderer.  H and W in [1, 4096].  Asynchronous on
 * `stream`, ordered like every launch of the batch.  A bad argument (NULL pointer, n < 1, H / W / fovy out
 * of range, unknown mode, body outside [0, nbody)) returns -1 with a message and launches nothing. */
int hs_render_frames(hs_batch* b, int n, const void* kin_dev, const hs_camera* cam, int H, int W, uint8_t* rgb_dev,
                     void* stream);
/* Stage dump of env 0 after its last substep (parity debugging); n >= 16384 doubles. */
int hs_set_debug(hs_batch* b, int enable);
int hs_get_debug(hs_batch* b, double* out, int n);
int hs_synchronize(hs_batch* b);
/* Diagnostics (synchronous): *wide_reruns = cumulative count of env steps whose contacts or
 * constraint rows overflowed the resident kernel tier (32 contacts / 128 rows) and were re-run by
 * the wide tier (64 / 256); contacts are only dropped (HS_WARN_OVERFLOW) past the wide tier. */
int hs_batch_counters(const hs_batch* b, uint64_t* wide_reruns);

/* The device reward plug-ins on supplied fields <- REWARD_FUNCTIONS[type](env_data, params)
 * (reward_functions.py:66-269, utils.py:3-21; called at custom_env.py:263-271).  Runs the SAME device
 * code the step kernel inlines after each env step (reward_formula + numpy-order sums), on n states
 * given as device arrays of the `precision` type (HS_FP32 / HS_FP64): qpos [n][nq], qvel [n][nv],
 * ctrl [n][nu], time [n], subtree_com0 / subtree_linvel0 [n][3] (subtree_com[0], subtree_linvel[0]),
 * cfrc_ext [n][nbody][6], qfrc_actuator [n][nv]; writes out [n].  reward_id: HS_REWARD_STAND ("default",
 * "stand"), HS_REWARD_KNEELING, HS_REWARD_WALK; kneel_params: 9 host doubles in hs_env_config's order
 * (NULL = the reference defaults, reward_functions.py:71-81).  The step kernel itself passes zeros for
 * cfrc_ext / subtree_linvel unless HS_FULL_STATE (mj_step leaves them uncomputed).  Asynchronous. */
int hs_reward_eval(const hs_model* m, int precision, int reward_id, const double* kneel_params, int n,
                   const void* qpos, const void* qvel, const void* ctrl, const void* time, const void* subtree_com0,
                   const void* subtree_linvel0, const void* cfrc_ext, const void* qfrc_actuator, void* out,
                   void* stream);

/* The reward of every env's current state under any built-in reward <- REWARD_FUNCTIONS[type](data, params)
 * on each env's data (custom_env.py:263-271): hs_reward_eval on the batch's own buffers (qpos, qvel,
 * data.ctrl, time, the aux row's subtree com, subtree_linvel / cfrc_ext -- zeros unless HS_FULL_STATE,
 * as mj_step leaves them -- and the obs row's qfrc_actuator), so it needs HS_OUT_AUX | HS_OUT_CTRL written
 * by the last step.  out: [N] of the batch precision (device).  kneel_params NULL = the batch's.  After an
 * hs_step with reward_id r it equals the step's reward buffer bitwise, except for truncated envs (which
 * the step rewards 0, custom_env.py:201-211) and envs that auto-reset (whose buffers hold the reset
 * state).  Asynchronous. */
int hs_reward(hs_batch* b, int reward_id, const double* kneel_params, void* out, void* stream);

/* Reward programs <- one more entry in REWARD_FUNCTIONS (reward_functions.py:264-269; the reference's "addition
 * and selection of custom reward function"), evaluated on the device.  A program is a user's reward function
 * traced once (reward_program.py) into a flat, branch-free list of n_instr instructions (op, dst, a, b, c),
 * int32 each, over numbered value slots, with n_consts float64 constants and n_params float64 parameter slots
 * that every call supplies (reward_config["params"] over the function's defaults, custom_env.py:263-271).  The
 * opcode table, the operand meaning and one op's arithmetic are csrc/hs_reward_prog.h; every op is one
 * operation or libm call of the batch precision, never contracted (+ - * correctly rounded, / and sqrt in
 * double too; the device's float / and sqrt are the fp32 engine's, <= 2.5 ulp), comparisons with a NaN
 * are false, and a select evaluates both arms.  The limits (a program is bounded by its LIVE values, the
 * slots, not by its length): */
#define HS_RP_MAX_INSTR 4096
#define HS_RP_MAX_SLOTS 64
#define HS_RP_MAX_CONSTS 256
#define HS_RP_MAX_PARAMS 32
typedef struct hs_reward_program hs_reward_program;
/* The env_data fields a program may read (reward_functions.py's `env_data.*`), one array per field, each
 * [n][row] contiguous in the call's precision: qpos [nq], qvel [nv], ctrl [nu], time [1], qfrc_actuator [nv],
 * cinert [nbody][10], cvel [nbody][6], subtree_com0 [3] (subtree_com[0], the root's row), cfrc_ext [nbody][6],
 * subtree_linvel [nbody][3].  A field the program does not read may be NULL. */
typedef struct {
  const void* qpos;
  const void* qvel;
  const void* ctrl;
  const void* time;
  const void* qfrc_actuator;
  const void* cinert;
  const void* cvel;
  const void* subtree_com0;
  const void* cfrc_ext;
  const void* subtree_linvel;
} hs_reward_fields;
/* hs_reward_program_create VALIDATES the encoding against the limits and the model's dimensions before anything
 * is uploaded: an unknown opcode, a slot / constant / parameter index out of range, a field index outside
 * the model's nq / nv / nu / nbody, a slot read before it is written, a missing result (the last instruction
 * must be the one result) or an over-limit count returns -1 with the reason (hs_last_error) and *prog = NULL;
 * such a program is never launched.  With a GPU present the code is copied to the current device here
 * (synchronously), so later calls on that device allocate nothing; without one the program still serves
 * hs_reward_program_eval_host.  hs_reward_program_info: instruction count, slots used and the bit set of the
 * fields read (bit k = the k-th member of hs_reward_fields); any pointer may be NULL. */
int hs_reward_program_create(const hs_model* m, const int32_t* code, int n_instr, const double* consts, int n_consts,
                             int n_params, hs_reward_program** prog);
void hs_reward_program_destroy(hs_reward_program* prog);
int hs_reward_program_info(const hs_reward_program* prog, int* n_instr, int* n_slots, unsigned* fields);
/* The program interpreted on the CPU in double on n states (host arrays of double): needs no GPU.  params:
 * n_params host doubles.  Synchronous. */
int hs_reward_program_eval_host(const hs_reward_program* prog, const double* params, int n,
                                const hs_reward_fields* fields, double* out);
/* The program on caller-supplied device fields of `precision` (HS_FP32 / HS_FP64), the counterpart of
 * hs_reward_eval: writes out [n] (device) on the current device.  Asynchronous on `stream`. */
int hs_reward_program_eval(const hs_reward_program* prog, int precision, const double* params, int n,
                           const hs_reward_fields* fields, void* out, void* stream);
/* The program on the batch's own buffers, the counterpart of hs_reward: cinert / cvel / qfrc_actuator are the
 * obs row's, subtree_com0 the aux row's, cfrc_ext / subtree_linvel zeros unless HS_FULL_STATE.  Refused (before
 * any launch) when the program reads ctrl or subtree_com and the batch's outputs do not carry them
 * (HS_OUT_CTRL / HS_OUT_AUX) or data.ctrl is stale, and when a full-state batch has no cfrc_ext /
 * subtree_linvel buffers.  out: [N] of the batch precision (device).  Asynchronous. */
int hs_reward_program_batch(hs_batch* b, const hs_reward_program* prog, const double* params, void* out, void* stream);
/* One env step with a program reward <- HumanoidEnv.step with REWARD_FUNCTIONS[type] a user's function
 * (custom_env.py:152-230 + SB3 auto-reset), as launches only -- no host synchronisation, no copy:
 *   1. hs_step with no reward and no auto-reset, whatever the batch's config says;
 *   2. the program on the post-step, pre-reset state: reward (0 for a truncated env, custom_env.py:203-206),
 *      total_reward += reward, and for finished envs terminal_obs, terminal_step_count, terminal_total_reward;
 *   3. if the batch's config has autoreset on: hs_reset masked by the finished envs, with the reset noise an
 *      auto-reset inside hs_step draws (the bound arrays of hs_set_autoreset_noise or the device RNG).
 * The same refusals as hs_reward_program_batch, made before step 1 (the step itself rewrites data.ctrl).  For a
 * program that restates a built-in reward every buffer equals hs_step's with that reward id, bitwise. */
int hs_step_program(hs_batch* b, const float* actions, const hs_reward_program* prog, const double* params,
                    void* stream);

/* Named reward components <- info['reward_components'] (custom_env.py:134-140, :217): a reward function may
 * return a dict of name -> term (with the key "total", the reward) instead of one value.  Its program then holds
 * one `out` instruction per entry, (RP_OUT, 0, a = slot, b = component index, 0), anywhere before the result, and
 * is created with n_outputs = the number of entries, at most: */
#define HS_RP_MAX_OUTPUTS 16
/* hs_reward_program_create_components validates as hs_reward_program_create does (which means n_outputs = 0), and
 * refuses n_outputs outside [0, 16], an `out` whose index is outside [0, n_outputs) (so any `out` of a program
 * created with 0), a component written twice, one never written, and a source slot read before it is written.
 * hs_reward_program_outputs: the count a program was created with.
 *
 * Component rows are COMPONENT-MAJOR, [n_outputs][n] -- component c of env e at c * n + e -- in the call's
 * precision: every lane of a wave executes the same `out`, so one `out` is one store of 64 consecutive values
 * (env-major rows would be strided by n_outputs).  With comp_out NULL (or no rows bound, below) an `out` does
 * nothing, so the same program runs anywhere.  comp_out non-NULL with a program without outputs is refused.
 * hs_reward_program_eval_host_components: comp_out [n_outputs][n] host doubles.
 * hs_reward_program_batch_components: comp_out [n_outputs][N] of the batch precision (device); out as before.
 *
 * hs_set_reward_components binds the rows hs_step_program (and its outcome launch) fills, like the termination
 * state a call of its own (hs_buffers is unchanged).  All four are device memory, caller-owned, and must outlive
 * the binding: comp, comp_total, terminal_comp_total [n_outputs][N] of the batch precision, comp_episode [N]
 * int32.  n_outputs = 0 or NULL pointers clear the binding.  Binding sets every comp_episode tag to -1 (no
 * episode; synchronous).  With rows bound, launch 2 of hs_step_program also writes, for every env:
 *   comp[c]                the step's value of component c, or 0 when the env is truncated, exactly as the reward is;
 *   comp_total[c]          the episode's running sum, prev + value rounded in the batch precision, where prev reads
 *                          as 0 when comp_episode differs from the env's episode number (the grace counter's idiom:
 *                          every reset clears the sums without the reset kernels knowing); then comp_episode = episode;
 *   terminal_comp_total[c] the sums of the envs that are done this step, beside terminal_total_reward.
 * A program whose n_outputs differs from the bound count is refused (-1, both numbers in hs_last_error) BEFORE
 * the step is launched.  With no rows bound hs_step_program is what it was.  A termination predicate has no
 * outputs: hs_set_termination*, hs_termination_eval_host refuse a program created with n_outputs > 0.  The
 * fused launches evaluate no program, so they fill no component rows. */
int hs_reward_program_create_components(const hs_model* m, const int32_t* code, int n_instr, const double* consts,
                                        int n_consts, int n_params, int n_outputs, hs_reward_program** prog);
int hs_reward_program_outputs(const hs_reward_program* prog, int* n_outputs);
int hs_reward_program_eval_host_components(const hs_reward_program* prog, const double* params, int n,
                                           const hs_reward_fields* fields, double* out, double* comp_out);
int hs_reward_program_batch_components(hs_batch* b, const hs_reward_program* prog, const double* params, void* out,
                                       void* comp_out, void* stream);
int hs_set_reward_components(hs_batch* b, int n_outputs, void* comp, void* comp_total, int32_t* comp_episode,
                             void* terminal_comp_total);

/* Termination conditions <- the fall conditions custom_env.py:167-200 holds commented out (`height < 0.8` held
 * for a grace period, custom_env.py:169-180 without its reward scaling; `height < 0.8` or |roll|, |pitch| > 45
 * degrees, custom_env.py:183-200) and Gymnasium Humanoid's terminate_when_unhealthy: an episode that ends on a
 * condition of the state.  A condition is a PREDICATE, a program of the reward-program language above whose value
 * is read as a truth value (it holds iff the value is non-zero and not NaN; comparisons with a NaN are false),
 * plus an integer grace period: the episode ends at the first env step at which the predicate has held for
 * grace_steps >= 1 consecutive env steps of that episode.  The per-env counter lives in the batch and belongs
 * to the episode: it is stored with the env's `episode` number and reads as 0 when that number differs from the
 * current one, so every reset (auto, masked, hs_reset) clears it; hs_state_io leaves it alone.
 *
 * hs_set_termination: predicate NULL clears the condition.  Otherwise the predicate is checked against the
 * batch as hs_reward_program_batch checks a program (model dimensions; ctrl / subtree_com need HS_OUT_CTRL /
 * HS_OUT_AUX) and refused before anything is launched; params (n_params doubles) are copied, the predicate is
 * NOT (it must outlive its use); the counter, its episode tag and the early_terminated bytes are allocated
 * once per batch and cleared at every call.  Synchronous.  Off (the default) nothing changes: a batch without
 * a condition runs exactly the launches it ran before.
 *
 * With a condition set, hs_step (with a device reward) and hs_step_program are, as launches only:
 *   1. the step without auto-reset (hs_step_program: and without reward), whatever the config says;
 *   2. ONE outcome launch on the post-step, pre-reset state: the reward program if there is one (else the step
 *      kernel's reward / total_reward stay), the predicate, the grace counter, early = count >= grace_steps,
 *      terminated |= early (whether or not the env is truncated; TimeLimit.truncated stays truncated &&
 *      !terminated), the early_terminated byte, and every finished env's terminal_obs / terminal_step_count /
 *      terminal_total_reward;
 *   3. if the config has autoreset on: hs_reset masked by terminated || truncated, with the auto-reset's noise.
 * hs_step with HS_REWARD_NONE is the step alone, as configured: the reward is the caller's, and so is the
 * outcome that must follow it -- write reward / total_reward, then call hs_apply_termination, which is launch 2
 * on the batch's current state with no reset (call it once per env step: it advances the grace counter).
 * One stream group.
 *
 * THE LIMIT: the fused launches -- hs_step_tape, hs_rollout*, hs_evaluate* -- refuse a batch whose condition was
 * set with hs_set_termination (-1, the reason in hs_last_error): a user-registered predicate needs the
 * interpreter, which the step kernel has no room for.  The host bounds an ordinary fused launch so that each env
 * finishes at most one episode in it, from the shortest possible episode; a state-dependent end makes that bound
 * unknowable.
 *
 * hs_set_termination_builtin lifts the limit for the two built-in conditions (HS_TERM_FALLEN: qpos[2] <
 * min_height; HS_TERM_LOST_BALANCE: that, or |roll| or |pitch| > max_roll_pitch with quaternion_to_euler's
 * unclamped pitch).  It does everything hs_set_termination(b, predicate, params, grace_steps) does -- the
 * predicate stays set, and hs_step keeps running the three launches above with the interpreter, unchanged: that
 * path is the yardstick and the fallback of an aborted fused launch -- and also records the built-in, which makes
 * the condition FUSED-CAPABLE.  Before recording it checks that program and built-in are the same predicate: the
 * program may read qpos only, and it is evaluated on the host on a fixed table of probe rows (heights either
 * side of min_height, quaternions tilted either side of max_roll_pitch in roll and in pitch, one quaternion with
 * |2 (w y - z x)| > 1 whose NaN pitch must not terminate); any truth value that differs from the built-in's
 * refuses the call (-1), before any launch.  hs_set_termination (new or cleared) drops the mark.
 * With a fused-capable condition hs_step_tape, hs_rollout_act / _norm and hs_evaluate / _norm launch instead
 * of refusing (their other preconditions stay: the fp64 Newton engine, auto-reset with the on-device reset noise,
 * a device reward, the chunk-queue schedule): kernel instances of their own evaluate the built-in after every env
 * step, bitwise the per-step path's results.  An env may then end several episodes in one launch, so the launch
 * cap is 511 steps alone (hs_rollout_max_steps returns it), and THE TERMINAL ROWS' CONTRACT is: terminal_obs,
 * terminal_step_count and terminal_total_reward are written by the launch's last step only, i.e. after a fused
 * launch they are defined for the envs that were done on its last step (what every reader uses: a per-step
 * output, a rollout's terminal obs rows and an evaluation's result slots have an address of their own per step
 * or per episode).  The early_terminated byte and the grace counter / episode tag are committed by the last
 * step with the state; an aborted launch (return 1) restores them with it.
 * hs_termination_builtin_eval_host: the built-in predicate alone on n host rows (qpos + i * ld, ld >= 7 doubles;
 * out [n] bytes), needing no batch and no GPU.
 *
 * hs_termination_state: returns 1 if a condition is set, else 0; *grace_steps (0 when none) and the device
 * pointers of the [N] early_terminated bytes, grace counters and their episode tags (NULL before the first
 * hs_set_termination); any out pointer may be NULL.
 * hs_termination_eval_host: predicate + grace update over n host states in double, the counterpart of
 * hs_reward_program_eval_host (needs no GPU): episode [n] the envs' current episode numbers, count /
 * episode_tag [n] read and updated in place, early [n] written. */
int hs_set_termination(hs_batch* b, const hs_reward_program* predicate, const double* params, int grace_steps);
#define HS_TERM_FALLEN 1
#define HS_TERM_LOST_BALANCE 2
int hs_set_termination_builtin(hs_batch* b, const hs_reward_program* predicate, const double* params, int grace_steps,
                               int kind, double min_height, double max_roll_pitch);
int hs_termination_builtin_eval_host(int kind, double min_height, double max_roll_pitch, int n, const double* qpos,
                                     int ld, uint8_t* out);
int hs_apply_termination(hs_batch* b, void* stream);
int hs_termination_state(const hs_batch* b, int* grace_steps, const uint8_t** early_terminated,
                         const int32_t** grace_count, const int32_t** grace_episode);
int hs_termination_eval_host(const hs_reward_program* predicate, const double* params, int grace_steps, int n,
                             const hs_reward_fields* fields, const int32_t* episode, int32_t* count,
                             int32_t* episode_tag, uint8_t* early);

/* Reference-motion targets <- the recording an episode started from (hs_set_initial_states binds it as a start
 * distribution), visible to rewards and termination conditions: "be where the recording is NOW", "hold the
 * keyframe you started from", "end the episode once you have drifted off the recording".  A batch may hold one
 * REFERENCE MOTION: n_rows = K >= 1 rows qpos [K][nq] / qvel [K][nv] (HOST doubles; qvel NULL: zeros), key_dt > 0
 * seconds between consecutive rows (required with K > 1, ignored with K == 1; the `time` attributes of recorded
 * <key> elements are not trusted), an end mode and a start mode:
 *   HS_REF_HOLD | HS_REF_LOOP              past the last row: stay on it | start over at row 0
 *   HS_REF_START_ZERO | HS_REF_START_DRAWN  the episode's first row j0: 0 | the row its initial state drew,
 *                                           min(K - 1, floor(u K)) of hs_set_initial_states (0 for episode 0)
 * Programs read it as two more fields, ref_qpos [nq] and ref_qvel [nv] (field ids 16 and 17, a block of their own after
 * subtree_linvel -- the ids 10 .. 15 stay unknown fields, left for state fields to come; hs_reward_program_info's
 * mask reports them as bits 16 and 17), with the ordinary load instruction.  They are NOT
 * members of hs_reward_fields, whose layout is unchanged: a sample is no array of the caller's but a pure
 * function of (seed, env, episode[env], time[env]) and the rows, so nothing is carried between steps:
 *   x  = (double)j0 + (double)time / key_dt        in double also for an fp32 batch; NaN or negative: 0
 *   hold:  x = min(x, K - 1); i = floor(x); i1 = min(i + 1, K - 1)
 *   loop:  x = min(x, 2^52);  i = floor(x) mod K; i1 = (i + 1) mod K
 *   w  = (T)(x - floor(x));   ref[k] = a + w (b - a),  a = row_i[k], b = row_i1[k]
 * each operation rounded in the batch precision T, never contracted; i and i1 lie in [0, K - 1] for every input.
 * The free joint's quaternion of every row is normalised when bound (as hs_set_initial_states does), but the
 * interpolated components are NOT renormalised: a program divides by the norm where it matters.
 *
 * hs_set_reference_motion: n_rows = 0 clears the binding.  The library converts the rows to the batch precision
 * and owns the copy, by the rules of hs_set_initial_states: the call waits for the batch's pending launches,
 * writes in place when the rows fit the blocks, otherwise allocates anew and keeps the old blocks until the batch
 * is destroyed; a launch recorded into a HIP graph keeps the reference it was recorded with: re-record it after a
 * rebind.  Refused (-1): n_rows outside [0, HS_MAX_REFERENCE_ROWS], NULL qpos, key_dt not finite or <= 0 with
 * K > 1, unknown flag bits, a value that is not finite, a zero free-joint quaternion.
 * A program that reads a reference field is refused BEFORE ANY LAUNCH by hs_reward_program_batch*, hs_step_program,
 * hs_step / hs_apply_termination (the predicate) and hs_set_termination when the batch has no reference bound, and
 * when the reference has HS_REF_START_DRAWN but no bank of initial states of the same n_rows is bound.  The
 * entry points that take hs_reward_fields alone (hs_reward_program_eval, hs_reward_program_eval_host*,
 * hs_termination_eval_host) refuse such a program and name the batch entry points.  A batch with a reference
 * bound whose programs do not read it runs exactly the launches it ran before, fused ones included.
 * hs_get_reference_motion: the rows bound (0: none), key_dt and the flags; any pointer may be NULL.
 *
 * hs_reward_program_eval_host_reference / hs_termination_eval_host_reference: the host interpreter with a
 * reference (ref NULL: hs_reward_program_eval_host_components / hs_termination_eval_host).  The rows are used as
 * given (not normalised); precision HS_FP32 computes the sample in float, as an fp32 batch does, and widens it.
 * fields->time is required.  episode / seed [n]: each state's episode number and its batch's (group's) seed,
 * required with HS_REF_START_DRAWN only; env [n]: each state's env index within that batch, NULL: 0 .. n-1. */
#define HS_REF_HOLD 0
#define HS_REF_LOOP 1
#define HS_REF_START_ZERO 0
#define HS_REF_START_DRAWN 2
#define HS_MAX_REFERENCE_ROWS 4096
typedef struct {
  int n_rows;
  const double* qpos;
  const double* qvel;
  double key_dt;
  int flags;
  int precision;
  const int32_t* episode;
  const uint64_t* seed;
  const int32_t* env;
} hs_reference_host;
int hs_set_reference_motion(hs_batch* b, int n_rows, const double* qpos, const double* qvel, double key_dt, int flags);
int hs_get_reference_motion(const hs_batch* b, int* n_rows, double* key_dt, int* flags);
int hs_reward_program_eval_host_reference(const hs_reward_program* prog, const double* params, int n,
                                          const hs_reward_fields* fields, const hs_reference_host* ref, double* out,
                                          double* comp_out);
int hs_termination_eval_host_reference(const hs_reward_program* predicate, const double* params, int grace_steps, int n,
                                       const hs_reward_fields* fields, const hs_reference_host* ref,
                                       const int32_t* episode, int32_t* count, int32_t* episode_tag, uint8_t* early);

/* GAE(gamma, lambda) reverse scan over a device rollout buffer, SB3 semantics: [T][N] float32
 * rewards, values, episode_starts; [N] last_values, last_dones; writes [T][N] advantages and
 * returns (= advantages + values).  All pointers are device memory on the current device;
 * asynchronous on `stream`.  advantages / returns must not overlap the inputs or each other (checked:
 * an error, not wrong advantages): for T >= 256 the scan runs as three launches that keep their
 * per-chunk maps and carries in those output rows. */
int hs_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
           const float* last_dones, float* advantages, float* returns, int T, int N, float gamma, float gae_lambda,
           void* stream);
/* VecNormalize.normalize_obs over rows <- np.clip((obs - obs_rms.mean) / np.sqrt(obs_rms.var + epsilon),
 * -clip_obs, clip_obs) (vec_normalize.py), and optionally in the same pass the batch moments that
 * obs_rms.update(obs) takes of the RAW rows.  X [rows][ldx] float32 (first obs_dim columns), mean / inv_std
 * [obs_dim] float32; out [rows][ldo] may be X itself (in place).  out = clamp((x - mean) * inv_std, +-clip),
 * float32, subtraction and product each rounded to nearest (no FMA): bitwise what the fused policy of
 * hs_rollout_norm reads.  moments != NULL: moments[0] = rows, moments[1 + c] = the mean and
 * moments[1 + obs_dim + c] = the sum of squared deviations (M2 = var * rows) of column c, float64, taken about
 * the first row as a shift and reduced in a fixed two-stage order (no atomics: two runs are bitwise equal);
 * `workspace` then holds hs_obs_norm_workspace(rows, obs_dim) bytes.  obs_dim <= 512.  16-byte accesses when
 * obs_dim, ldx, ldo are multiples of 4 and every pointer is 16-byte aligned.  Asynchronous on `stream`. */
uint64_t hs_obs_norm_workspace(uint64_t rows, int obs_dim);
int hs_obs_norm(const float* X, uint64_t ldx, uint64_t rows, int obs_dim, const float* mean, const float* inv_std,
                float clip, float* out, uint64_t ldo, double* moments, void* workspace, void* stream);
/* RunningMeanStd.update_from_moments (common/running_mean_std.py) on the device, float64: state = (count,
 * mean [dim], var [dim]) absorbs n_sets batch moment sets (count, mean [dim], M2 [dim]) -- hs_obs_norm's
 * layout -- at sets + k * set_stride, in ascending k, each by Chan's merge in SB3's operation order; a set
 * with count 0 is skipped.  Then, when given, mean_f32 [dim] = mean and inv_std_f32 [dim] =
 * 1 / sqrt(var + epsilon) rounded to float32: the arrays hs_obs_norm and hs_rollout_norm read.  n_sets = 0
 * only refreshes those arrays.  One small launch, asynchronous on `stream`: no host synchronisation. */
int hs_rms_merge(double* state, int dim, const double* sets, int n_sets, uint64_t set_stride, double epsilon,
                 float* mean_f32, float* inv_std_f32, void* stream);
/* VecNormalize's reward path over a finished rollout, phase A <- self.returns = self.returns * gamma + rewards
 * of step_wait, step by step: rewards [T][N] float32 (raw), dones [T][N] uint8; returns_carry [N] float64
 * holds self.returns between rollouts (in / out; zeroed where done, after the step's moments).  Writes
 * moments [T][3] float64 = (N, mean, M2) of the step's returns over the N envs -- what ret_rms.update(
 * self.returns) takes -- in a fixed reduction order.  `workspace`: T * N doubles.  Asynchronous. */
int hs_return_moments(const float* rewards, const uint8_t* dones, int T, int N, double gamma, double* returns_carry,
                      double* workspace, double* moments, void* stream);
/* Phase B <- ret_rms.update + normalize_reward of step_wait: for t = 0 .. T - 1 the step's batch -- the
 * union, in ascending k, of the n_sets sets at moments + k * set_stride + 3 t (one set per rank: the
 * all-gathered hs_return_moments blocks; n_sets = 1 for one process) -- is merged into state = (count, mean,
 * var) of ret_rms (float64), and rewards[t][:] = clip(rewards[t][:] / sqrt(var + epsilon), +-clip) with the
 * variance after that merge (quotient in float64, rounded to float32).  In place; `workspace`: T doubles.
 * Asynchronous on `stream`. */
int hs_reward_scale(float* rewards, int T, int N, double* state, const double* moments, int n_sets,
                    uint64_t set_stride, double epsilon, double clip, double* workspace, void* stream);
/* One PPO rollout step's policy sampling and buffer writes over N envs (A <= 32 actions):
 * mean [N][mean_ld] (first A columns), value [N] at stride value_ld, log_std [A], episode_start
 * [N] (all float32 device memory).  actions = mean + exp(log_std) * z with z ~ N(0, 1) from the
 * counter-based Philox4x32-10 stream (seed, counter + *counter_base when counter_base (a device
 * uint64) is not NULL -- graph replays then draw fresh noise; z = 0 when deterministic != 0); writes
 * actions [N][A] (unclipped, the buffer copy), actions_clipped [N][A] (clip to [-1, 1], what the
 * env steps with), log_prob [N], values [N] and episode_starts_out [N].  Asynchronous on `stream`. */
/* Fused forward of one 2-hidden-layer MLP (H = 256, ReLU; hs_mlp2_forward_act: ReLU or Tanh): out[N][A] = relu(relu(X W1' + b1) W2' + b2)
 * W3' + b3, weights as nn.Linear stores them, [out][in] row-major (W1 [256][ld1 >= D], W2 [256][ld2],
 * W3 [A][ld3], ld2 / ld3 >= 256); D <= 512, A <= 32.  16-byte weight loads when every weight row
 * is 16-byte aligned, element loads otherwise.  Replaces the three GEMMs of SB3's MlpPolicy forward (ActorCriticPolicy.forward ->
 * mlp_extractor -> action_net / value_net, policies.py, SB3 2.3.2) in the rollout: the pi net's mean
 * per env step and the vf net's values over the rollout buffer.  fp32 in, fp32 MFMA accumulation.
 * Asynchronous on `stream`. */
int hs_mlp2_forward(const float* X, int ldx, int D, int N, const float* W1, int ld1, const float* b1, const float* W2,
                    int ld2, const float* b2, const float* W3, int ld3, const float* b3, int A, float* out, int ldo,
                    void* stream);
/* The same forward for hidden layers of H = 64, 128 or 256 (W1 [H][ld1 >= D], W2 [H][ld2], W3 [A][ld3],
 * ld2 / ld3 >= H): H / 32 waves per workgroup.  hs_mlp2_forward is this with H = 256. */
int hs_mlp2_forward_h(const float* X, int ldx, int D, int N, int H, const float* W1, int ld1, const float* b1,
                      const float* W2, int ld2, const float* b2, const float* W3, int ld3, const float* b3, int A,
                      float* out, int ldo, void* stream);
/* The same forward with the hidden activation `act` (HS_ACT_RELU or HS_ACT_TANH): out = act(act(X W1' + b1)
 * W2' + b2) W3' + b3, the mlp_extractor + head of an MlpPolicy built with activation_fn = nn.ReLU or nn.Tanh
 * (ActorCriticPolicy.forward, policies.py, SB3 2.3.2).  hs_mlp2_forward_h is this with HS_ACT_RELU. */
int hs_mlp2_forward_act(const float* X, int ldx, int D, int N, int H, int act, const float* W1, int ld1,
                        const float* b1, const float* W2, int ld2, const float* b2, const float* W3, int ld3,
                        const float* b3, int A, float* out, int ldo, void* stream);
int hs_ppo_act(const float* mean, int mean_ld, const float* value, int value_ld, const float* log_std,
               const float* episode_start, uint64_t seed, uint64_t counter, const uint64_t* counter_base,
               int deterministic, float* actions,
               float* actions_clipped, float* log_prob, float* values, float* episode_starts_out, int N, int A,
               void* stream);
/* The rest of the PPO rollout step after the env step, over N envs: reward [N] float32,
 * terminated / truncated [N] uint8.  boot = truncated && !terminated (TimeLimit.truncated).
 * Immediate bootstrap: terminal_value [N] = V(terminal obs) given -> reward_out = reward +
 * gamma * terminal_value where boot (else reward).  Deferred bootstrap: terminal_value NULL ->
 * reward_out = reward, boot_out [N] uint8 = boot, and for boot envs the terminal_obs row (obs_dim
 * float32) is copied to boot_obs_out (row n); the caller adds gamma V(row) at the end of the
 * rollout.  Both: done_out = terminated || truncated (uint8), ep_acc += reward (float64, zeroed
 * where done, after ep_return_out = the accumulated value is written), episode_start = done
 * (float32), and obs_floats float32 copied from obs to obs_out (the next rollout-buffer slot;
 * NULL obs skips it).  Asynchronous on `stream`. */
int hs_ppo_post(const float* reward, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value,
                const float* terminal_obs, float* boot_obs_out, uint8_t* boot_out, int obs_dim, float gamma,
                const float* obs, float* obs_out, uint64_t obs_floats, float* reward_out, uint8_t* done_out,
                double* ep_acc, double* ep_return_out, float* episode_start, int N, void* stream);
/* logp[n] = sum_j (-z^2/2 - log_std[j]) - A log(sqrt(2 pi)), z = (actions[n][j] - mean[n][j]) /
 * exp(log_std[j]); mean [N][mean_ld], actions [N][A] contiguous, A <= 32.  The backward, given
 * g_logp [N]: g_mean[n][j] = g z / sigma and gls_rows[n][j] = g (z^2 - 1), whose column sums
 * (hs_colsum) are dL/dlog_std.  Asynchronous on `stream`. */
int hs_gauss_logp(const float* mean, int mean_ld, const float* actions, const float* log_std, float* logp, int N,
                  int A, void* stream);
int hs_gauss_logp_grad(const float* mean, int mean_ld, const float* actions, const float* log_std,
                       const float* g_logp, float* g_mean, float* gls_rows, int N, int A, void* stream);
/* SB3 PPO minibatch loss over B samples gathered by idx [B] (int64) from the rollout arrays
 * advantages / returns / old_log_prob [M]: log_prob [B] and values [B] are the policy's on the
 * minibatch.  a = advantages[idx] normalised (mean, unbiased std + 1e-8; not when B == 1, nor when
 * normalize_advantage == 0: SB3's PPO(normalize_advantage=False)),
 * r = exp(log_prob - old_log_prob[idx]); writes policy_loss = -mean(min(a r, a clip(r, 1 -+ clip)))
 * and value_loss = mean((returns[idx] - values)^2) (device scalars).  `workspace` holds
 * hs_ppo_loss_workspace(B) floats: the forward leaves the gathered minibatch and the
 * normalisation there for the backward, which, given the upstream device scalars g_pg, g_vf,
 * writes dL/dlog_prob [B] and dL/dvalues [B] with torch's min/clamp derivative conventions.
 * Fixed reduction order (deterministic); asynchronous on `stream`. */
uint64_t hs_ppo_loss_workspace(int B);
int hs_ppo_loss(const float* log_prob, const float* values, const int64_t* idx, const float* advantages,
                const float* returns, const float* old_log_prob, int B, float clip, int normalize_advantage,
                float* policy_loss, float* value_loss, float* workspace, void* stream);
int hs_ppo_loss_grad(const float* log_prob, const float* values, int B, float clip, const float* workspace,
                     const float* g_pg, const float* g_vf, float* g_log_prob, float* g_values, void* stream);
/* Gradient-norm clipping + one Adam step over nt <= 1024 float32 device tensors: params[i],
 * grads[i], exp_avg[i], exp_avg_sq[i] (numel[i] elements each) and step[i] (a float32 device
 * scalar per tensor, torch's capturable Adam state; all tensors share one step count).  With
 * c = min(1, max_norm / (||grads||_2 + 1e-6)) (max_norm <= 0: c = 1) and t = step + 1:
 * m = b1 m + (1-b1) c g; v = b2 v + (1-b2) (c g)^2; p -= lr / (1 - b1^t) * m / (sqrt(v) /
 * sqrt(1 - b2^t) + eps); step = t (1 - beta rounded to float from double, as torch's scalar
 * arguments are).  Grads are read, not modified.  `workspace` holds
 * hs_adam_workspace(sum numel) floats.  Pointer tables are host arrays (copied into the kernel
 * arguments); asynchronous on `stream`. */
uint64_t hs_adam_workspace(uint64_t total_numel);
int hs_adam_clip(int nt, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const int64_t* numel, float* workspace, float max_norm,
                 double lr, double beta1, double beta2, double eps, void* stream);
/* SB3 PPO.train's controls on the device (ppo/ppo.py, stable_baselines3 2.3.2): every entry below reads
 * the per-iteration hyperparameters from a float32 device block hparams[HS_PPO_HP_SIZE] (refreshed by the
 * host before each train(), so captured graphs follow learning_rate / clip_range schedules), shares the
 * int32 control words control[2] and accumulates into a float32 stats block of
 * hs_ppo_stats_size(n_epochs) = HS_PPO_STAT_KL + 2 n_epochs floats that the host zeroes before train()
 * and reads once after it. */
enum { HS_PPO_HP_LR = 0,              /* Adam learning rate */
       HS_PPO_HP_CLIP_RANGE = 1,      /* clip_range */
       HS_PPO_HP_CLIP_RANGE_VF = 2,   /* clip_range_vf; < 0: no value clipping */
       HS_PPO_HP_KL_STOP = 3,         /* 1.5 * target_kl; < 0: no early stop */
       HS_PPO_HP_SIZE = 4 };
enum { HS_PPO_CTL_STOP = 0,    /* stop word: set by the minibatch whose approx_kl exceeds HS_PPO_HP_KL_STOP */
       HS_PPO_CTL_EPOCH = 1 }; /* index of the current epoch (set by the host between epochs) */
enum { HS_PPO_STAT_POLICY_LOSS = 0, HS_PPO_STAT_VALUE_LOSS = 1, HS_PPO_STAT_CLIP_FRACTION = 2, HS_PPO_STAT_ENTROPY = 3,
       HS_PPO_STAT_LOSS = 4,          /* sums over the minibatches evaluated (count: HS_PPO_STAT_COUNT) */
       HS_PPO_STAT_LOSS_LAST = 5,     /* the last combined loss */
       HS_PPO_STAT_COUNT = 6,
       HS_PPO_STAT_KL_LAST = 7,       /* the last approx_kl a stop decision was taken from */
       HS_PPO_STAT_EXPLAINED_VARIANCE = 8, HS_PPO_STAT_STD = 9,   /* free for the caller (per iteration) */
       HS_PPO_STAT_KL = 10 };         /* [e][2]: sum of approx_kl and minibatch count of epoch e */
uint64_t hs_ppo_stats_size(int n_epochs);
/* hs_ppo_loss with clip = hparams[CLIP_RANGE] and, when hparams[CLIP_RANGE_VF] = c >= 0, SB3's clipped
 * value loss mean((returns[idx] - (ov + clamp(values - ov, -c, c)))^2), ov = old_values[idx] (the rollout
 * buffer's values [M]; read only then).  The same three launches also reduce, in the block order of the
 * two losses, approx_kl = mean((r - 1) - d), d = log_prob - old_log_prob[idx], r = exp(d) (SB3's
 * approx_kl_div as it writes it) and clip_fraction = mean(|r - 1| > clip); policy_loss and value_loss are
 * bitwise hs_ppo_loss's without value clipping.  The final single-wave launch then, unless
 * control[STOP] is already set (then stats and control are left untouched): adds policy_loss,
 * value_loss, clip_fraction, the entropy sum_j (1/2 + log sqrt(2 pi) + log_std[j]) (A <= 32) and
 * loss = policy_loss + vf_coef value_loss - ent_coef entropy to stats (LOSS_LAST = loss, COUNT += 1),
 * adds approx_kl to stats[KL + 2 e] (and 1 to the count beside it), e = control[EPOCH] clamped to
 * [0, n_epochs), and sets control[STOP] = 1 when hparams[KL_STOP] >= 0 and approx_kl > hparams[KL_STOP]
 * (SB3: the tripping minibatch is recorded, it and every later one take no optimizer step).
 * approx_kl_out != NULL defers that decision: the approx_kl is only written there, for hs_ppo_kl_stop
 * to decide from the value all-reduced over ranks.  `workspace`: hs_ppo_loss_workspace_ex(B) floats.
 * hs_ppo_loss_grad_ex is hs_ppo_loss_grad with clip from hparams plus the value-clip derivative
 * (torch's clamp: the closed interval passes, 0 outside); bitwise hs_ppo_loss_grad without value
 * clipping.  Asynchronous on `stream`. */
uint64_t hs_ppo_loss_workspace_ex(int B);
int hs_ppo_loss_ex(const float* log_prob, const float* values, const int64_t* idx, const float* advantages,
                   const float* returns, const float* old_log_prob, const float* old_values, int B,
                   int normalize_advantage, const float* hparams, const float* log_std, int A, float vf_coef,
                   float ent_coef, float* stats, int n_epochs, int* control, float* approx_kl_out, float* policy_loss,
                   float* value_loss, float* workspace, void* stream);
int hs_ppo_loss_grad_ex(const float* log_prob, const float* values, int B, const float* hparams,
                        const float* workspace, const float* g_pg, const float* g_vf, float* g_log_prob,
                        float* g_values, void* stream);
/* The deferred stop decision (one thread): unless control[STOP] is set, records the device scalar
 * approx_kl (the global minibatch's, e.g. the extra element of the all-reduced gradient bucket) in
 * stats[KL + 2 e] / KL_LAST and sets control[STOP] when it exceeds hparams[KL_STOP] >= 0. */
int hs_ppo_kl_stop(const float* approx_kl, const float* hparams, float* stats, int n_epochs, int* control,
                   void* stream);
/* hs_adam_clip with lr = hparams[LR] read on the device and a device predicate: when *skip != 0 (the
 * stop word) no tensor's params, exp_avg, exp_avg_sq or step changes.  With *skip == 0 and the same lr
 * the results are bitwise hs_adam_clip's. */
int hs_adam_clip_ex(int nt, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, float* const* step, const int64_t* numel, float* workspace,
                    float max_norm, const float* hparams, const int* skip, double beta1, double beta2, double eps,
                    void* stream);
/* out[c] = sum_r w[r] x[r][c] over a row-major [rows][cols] float32 device matrix (w = row_weight
 * [rows], or 1 when NULL -- the weighted form is a rank-1 weight gradient g'x), in a fixed
 * summation order (deterministic).  `workspace` must hold hs_colsum_workspace(rows, cols) floats
 * (may be NULL when that is 0).  Asynchronous on `stream`. */
/* ReLU backward fused with the bias gradient's first reduction pass, for a [rows][cols] float32
 * upstream gradient g and the layer's ReLU output y: writes gm = (y > 0) ? g : 0 and per-chunk
 * column sums of gm to partial [hs_colsum_partial_rows(rows, cols)][cols]. */
uint64_t hs_colsum_partial_rows(uint64_t rows, uint64_t cols);
int hs_relu_grad_colsum(const float* g, const float* y, uint64_t rows, uint64_t cols, float* gm, float* partial,
                        void* stream);
/* The same pass for the activation `act` of the layer whose output is y: HS_ACT_RELU as above, HS_ACT_TANH
 * gm = g (1 - y^2) -- threshold_backward / tanh_backward of SB3's loss.backward() through mlp_extractor
 * (policies.py, SB3 2.3.2) with the bias sum's first read.  hs_relu_grad_colsum is this with HS_ACT_RELU. */
int hs_act_grad_colsum(const float* g, const float* y, uint64_t rows, uint64_t cols, int act, float* gm,
                       float* partial, void* stream);
/* Input gradient of a Linear layer fed by an activation, fused with that activation's backward and the
 * first pass of its bias gradient (hs_dgrad_mask: ReLU): GX[B][N] = (G W) masked by X > 0, partial[p][N] = column sums of GX
 * over row block p, p < hs_dgrad_mask_partial_rows(B, K).  G [B][K] (row stride ldg) is the layer's
 * output gradient, W [K][N] its weight as nn.Linear stores it ([out][in], row stride ldw), X [B][N]
 * (ldx) its input = the previous layer's ReLU output; GX is contiguous.  N = 256; K <= 32 (a policy
 * or value head) or K % 16 == 0, K <= 512 (a hidden layer: fp32 MFMA, G rows 16-byte aligned, and
 * `workspace` of hs_dgrad_mask_workspace(K) floats for W transposed; may be NULL when that is 0).
 * Replaces `g @ w` + threshold_backward + the bias sum's first read of SB3's loss.backward() through
 * mlp_extractor (policies.py, SB3 2.3.2).  Asynchronous on `stream`. */
uint64_t hs_dgrad_mask_partial_rows(int B, int K);
uint64_t hs_dgrad_mask_workspace(int K);
int hs_dgrad_mask(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B, int N,
                  float* GX, float* partial, float* workspace, void* stream);
/* The same for a layer fed by the activation `act`: HS_ACT_RELU as above, HS_ACT_TANH GX = (G W) (1 - X^2), X
 * the previous layer's tanh output (nothing else needs to be kept for the backward).  Replaces `g @ w` +
 * tanh_backward + the bias sum's first read of SB3's loss.backward() through a Tanh mlp_extractor
 * (policies.py, SB3 2.3.2).  Same shapes, workspace and partial rows; hs_dgrad_mask is this with HS_ACT_RELU. */
int hs_dgrad_act(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B, int N,
                 int act, float* GX, float* partial, float* workspace, void* stream);
/* Two single-pass column sums in one launch: out0[c] = sum_r x0[r][c] ([rows0][cols0]) and
 * out1[c] = sum_r x1[r][c] ([rows1][cols1]) -- for short matrices (split-K slices, partials). */
int hs_colsum_pair(const float* x0, uint64_t rows0, uint64_t cols0, float* out0, const float* x1, uint64_t rows1,
                   uint64_t cols1, float* out1, void* stream);
uint64_t hs_colsum_workspace(uint64_t rows, uint64_t cols);
int hs_colsum(const float* x, uint64_t rows, uint64_t cols, const float* row_weight, float* workspace, float* out,
              void* stream);
const char* hs_last_error(void);
const char* hs_version(void);

#ifdef __cplusplus
}
#endif
#endif
