// The batch side of the C ABI, shared by its three translation units: the handles' definitions and the few
// helpers that cross units.  hs_api.cpp owns the batch, its memory and the one launch; hs_api_fused.cpp the
// tape, rollout and evaluation launches; hs_api_reward.cpp the rewards, reward programs and termination.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hsim.h"
#include "hs_api_error.h"
#include "hs_kernels.h"
#include "hs_reward_prog.h"
#include "mjcf.h"

struct hs_model {
  hs::HostModel host;
};

struct hs_batch {
  const hs_model* model = nullptr;
  int n = 0, device = 0, precision = HS_FP32, obs_dim = 0;
  bool full_state = false;
  uint64_t seed = 0;
  void* dmodel = nullptr;
  hs_buffers buf{};
  bool owns = false;
  void* dbg = nullptr;
  bool debug = false;
  const void* ar_qpos_noise = nullptr;       // bound auto-reset noise [n][nq] / [n][nv] (null: device RNG)
  const void* ar_qvel_noise = nullptr;
  int* redo = nullptr;                       // wide-tier work list [2 + n] (kernel-managed)
  unsigned long long* redo_total = nullptr;  // cumulative wide-tier re-runs
  void* mid = nullptr;                       // chunk-queue hand-off rows [n][MIDDIM] (kernel-managed)
  void* eval_obs = nullptr;                  // hs_evaluate's obs staging rows [n][obs_dim] f32 (uncached; lazily)
  int* qsync = nullptr;                      // chunk queue claim / exit counters, pair flags (qsync_words)
  hs_env_config cfg{};
  bool ctrl_stale = false;                   // env steps ran with HS_OUT_CTRL off: buf.ctrl is not data.ctrl
  int lose_env1 = 0;                         // hs_debug_lose_handoff test hook (env + 1; 0 = off)
  void* tape_backup = nullptr;               // hs_step_tape / hs_rollout: the state before a tape launch (replay on abort)
  size_t tape_backup_bytes = 0;
  unsigned long long tape_aborts = 0;        // tape launches replayed step by step (resident-tier overflow)
  hipStream_t last_stream = nullptr;         // stream of the batch's previous launch (order_streams)
  bool last_valid = false;
  hipEvent_t order_ev = nullptr;
  unsigned long long stream_orders = 0;      // cross-stream waits inserted (diagnostics)
  hipEvent_t tape_ev[2] = {nullptr, nullptr};   // around the last tape / rollout kernel launch
  float last_tape_ms = -1.f;                 // its duration (hs_last_tape_ms)
  int* kin_envs = nullptr;                   // hs_kinematics_batch: the env-id list on the device (grown on demand)
  int kin_envs_cap = 0;
  uint8_t* prog_done = nullptr;              // hs_step_program: the per-env done bytes, the mask of its reset launch
  // hs_set_termination: the predicate (not owned), its parameters (copied) and the grace period; the per-env
  // grace counter, the episode number it belongs to and the early_terminated bytes (allocated once)
  const hs_reward_program* term_prog = nullptr;
  double term_params[HS_RP_MAX_PARAMS] = {};
  int grace_steps = 1;
  int32_t* grace_count = nullptr;
  int32_t* grace_episode = nullptr;
  uint8_t* early = nullptr;
  // hs_set_termination_builtin: the built-in the predicate was checked against (0: none -- the condition is not
  // fused-capable), and the grace count between an env's steps of a fused launch [n] (uncached, as mid)
  int term_kind = 0;
  double term_min_height = 0.0, term_max_roll_pitch = 0.0;
  int32_t* mid_count = nullptr;
  // hs_set_reward_components: the caller's component rows [comp_n][n] (batch dtype) and the sums' episode tag [n];
  // comp_n = 0: none bound
  int comp_n = 0;
  void* comp = nullptr;
  void* comp_total = nullptr;
  int32_t* comp_episode = nullptr;
  void* term_comp_total = nullptr;
  // hs_set_initial_states: the bank of initial states resets draw from, in the batch precision: init_n rows bound
  // (0: none) of the init_cap rows the two blocks hold.  A rebind that fits writes in place; one that does not
  // allocates anew and retires the old blocks until the batch is destroyed, so a launch recorded into a graph
  // before the rebind still reads memory of this batch.
  void* init_q = nullptr;                    // [init_cap][nq]
  void* init_v = nullptr;                    // [init_cap][nv]
  int init_n = 0, init_cap = 0;
  std::vector<void*> init_retired;
  // hs_set_reference_motion: the reference motion reward and termination programs sample (ref_qpos / ref_qvel), in
  // the batch precision: ref_n rows bound (0: none) of the ref_cap the two blocks hold, key_dt seconds apart, the
  // HS_REF_* flags.  Bound and rebound by the rules of the initial-state bank above.
  void* ref_q = nullptr;                     // [ref_cap][nq]
  void* ref_v = nullptr;                     // [ref_cap][nv]
  int ref_n = 0, ref_cap = 0, ref_flags = 0;
  double ref_key_dt = 0.0;
  std::vector<void*> ref_retired;
};

// a validated reward program (hs_reward_prog.h) and its copies in device memory, one per device it ran on
struct hs_reward_program {
  hs::RpDims dims{};
  std::vector<int32_t> code;
  std::vector<double> consts;
  int n_params = 0;
  hs::RpInfo info;
  struct Dev { int device; int32_t* code; double* consts; };
  std::vector<Dev> dev;
  std::mutex mu;
};

namespace hs {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// f(a zero of the precision's element type): `using T = decltype(zero)` inside a generic lambda
template <typename F>
auto by_precision(int precision, F&& f) {
  return precision == HS_FP64 ? f(0.0) : f(0.0f);
}

// bytes per element of the batch's T* buffers
inline size_t elem_size(const hs_batch* b) { return b->precision == HS_FP64 ? 8 : 4; }

// a step with the ctrl copy on rewrites every env's data.ctrl (commit), one with it off leaves it stale
inline void env_step_committed(hs_batch* b) { b->ctrl_stale = !(b->cfg.outputs & HS_OUT_CTRL); }

// what a fused launch sets beyond its mode and inputs: the tape's step count and per-step outputs, and the
// fused policy's parts as StepLaunch takes them (hs_kernels.h)
struct LaunchExtra {
  int nsteps = 1;
  const hs_tape_out* tape = nullptr;
  FusedArgs fused{};
};

// hs_api.cpp
int order_streams(hs_batch* b, hipStream_t st);
bool uc_alloc(int device, size_t bytes, void** out, const char* what);
void uc_release(int device, size_t bytes, void* ptr);
int launch(hs_batch* b, int mode, const float* act, const uint8_t* mask, const void* nq, const void* nvz, int nsub,
           void* stream, const LaunchExtra& x = {});
int step_launch(hs_batch* b, const float* actions, void* stream);

// hs_api_reward.cpp
int step_outcome_reset(hs_batch* b, const float* actions, const hs_reward_program* prog, const double* params,
                       void* stream);

}  // namespace hs
