// hsim C ABI implementation (product).  See include/hsim.h for the reference interfaces replaced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hsim.h"
#include "hs_act.h"
#include "hs_api_error.h"
#include "hs_kernels.h"
#include "hs_render.h"
#include "hs_reward_prog.h"
#include "hs_term_builtin.h"
#include "mjcf.h"

static_assert(HS_KINDIM == hs::KINDIM, "include/hsim.h HS_KINDIM is the kernels' record size");
static_assert(HS_CAM_BODY == hs::CAM_BODY && HS_CAM_COM == hs::CAM_COM, "include/hsim.h camera modes");
static_assert(HS_RP_MAX_INSTR == hs::RP_MAX_INSTR && HS_RP_MAX_SLOTS == hs::RP_MAX_SLOTS &&
                  HS_RP_MAX_CONSTS == hs::RP_MAX_CONSTS && HS_RP_MAX_PARAMS == hs::RP_MAX_PARAMS &&
                  HS_RP_MAX_OUTPUTS == hs::RP_MAX_OUTPUTS,
              "include/hsim.h reward program limits");
static_assert(sizeof(hs_reward_fields) == hs::RP_NFIELDS * sizeof(void*), "hs_reward_fields: one pointer per field");

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

thread_local std::string hs::g_err;

namespace {
using hs::fail;
using hs::g_err;
using hs::hip_ok;
using hs::hip_rc;

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

// Uncached device memory (the chunk queue's hand-off rows, claim / exit / epoch words and pair
// flags) is recycled only as uncached memory: freed blocks go to a per-device list instead of
// hipFree, for the life of the process.  Round-3 finding: after a batch was destroyed, its hipFree'd
// UNCACHED hand-off rows were handed back out as ordinary memory -- torch tensors of the next batch --
// and a few hundred obs rows of that batch intermittently read back stale values
// (tools/probes/gpu_queue_wide_probe.py: 3 of 3 runs before, none after); keeping UC memory out of the
// general pool removes that path.  Sizes are rounded up to a power of two (>= 64 KB), and a request
// takes a free block of exactly its size class, so batches of any mix of sizes reuse blocks and the
// pool holds at most the peak of concurrently live uncached memory per class -- it never has to
// give a block back (a bounded list did, round 4, and re-opened the hazard for workloads with many
// batch sizes).
struct UcBlock { int device; size_t bytes; void* ptr; };
std::mutex g_uc_mu;
std::vector<UcBlock> g_uc_free;

size_t uc_class(size_t bytes) {
  size_t c = (size_t)64 << 10;
  while (c < bytes) c <<= 1;
  return c;
}

bool uc_alloc(int device, size_t bytes, void** out) {
  const size_t cls = uc_class(bytes);
  {
    std::lock_guard<std::mutex> lk(g_uc_mu);
    for (size_t i = 0; i < g_uc_free.size(); i++)
      if (g_uc_free[i].device == device && g_uc_free[i].bytes == cls) {
        *out = g_uc_free[i].ptr;
        g_uc_free.erase(g_uc_free.begin() + (long)i);
        return true;
      }
  }
  return hipExtMallocWithFlags(out, cls, hipDeviceMallocUncached) == hipSuccess;
}

void uc_release(int device, size_t bytes, void* ptr) {
  if (!ptr) return;
  std::lock_guard<std::mutex> lk(g_uc_mu);
  g_uc_free.push_back({device, uc_class(bytes), ptr});
}

// Launches of one batch are ordered across streams (include/hsim.h): when a call comes on another
// stream than the batch's previous one, the new stream first waits for everything issued on the old
// one (an event recorded there now).  Streams in graph capture are left alone -- the capturing
// framework orders the capture against the streams it forked from, and an event recorded outside a
// capture cannot be waited on inside it.
int order_streams(hs_batch* b, hipStream_t st) {
  if (b->last_valid && st != b->last_stream) {
    hipStreamCaptureStatus cn = hipStreamCaptureStatusNone, co = hipStreamCaptureStatusNone;
    if (!hip_ok(hipStreamIsCapturing(st, &cn), "hipStreamIsCapturing") ||
        !hip_ok(hipStreamIsCapturing(b->last_stream, &co), "hipStreamIsCapturing"))
      return -1;
    if (cn == hipStreamCaptureStatusNone && co == hipStreamCaptureStatusNone) {
      if (!b->order_ev && !hip_ok(hipEventCreateWithFlags(&b->order_ev, hipEventDisableTiming), "hipEventCreate"))
        return -1;
      if (!hip_ok(hipEventRecord(b->order_ev, b->last_stream), "stream order (record)") ||
          !hip_ok(hipStreamWaitEvent(st, b->order_ev, 0), "stream order (wait)"))
        return -1;
      b->stream_orders++;
    }
  }
  b->last_stream = st;
  b->last_valid = true;
  return 0;
}

int obs_dim_of(const hs::HostModel& m) { return (m.nq - 2) + m.nv + 10 * m.nbody + 6 * m.nbody + m.nv; }

template <typename T>
hs::EnvBuffers<T> env_buffers(const hs_batch* b) {
  hs::EnvBuffers<T> e;
  e.qpos = (T*)b->buf.qpos;
  e.qvel = (T*)b->buf.qvel;
  e.qacc_ws = (T*)b->buf.qacc_warmstart;
  e.ctrl = (T*)b->buf.ctrl;
  e.time = (T*)b->buf.time;
  e.step_count = b->buf.step_count;
  e.episode = b->buf.episode;
  e.total_reward = (T*)b->buf.total_reward;
  e.warning = b->buf.warning;
  e.obs = (T*)b->buf.obs;
  e.terminal_obs = (T*)b->buf.terminal_obs;
  e.reward = (T*)b->buf.reward;
  e.terminated = b->buf.terminated;
  e.truncated = b->buf.truncated;
  e.aux = (T*)b->buf.aux;
  e.cfrc_ext = (T*)b->buf.cfrc_ext;
  e.subtree_linvel = (T*)b->buf.subtree_linvel;
  e.term_step_count = b->buf.terminal_step_count;
  e.term_total_reward = (T*)b->buf.terminal_total_reward;
  e.redo = b->redo;
  e.redo_total = b->redo_total;
  e.mid = (T*)b->mid;
  e.qsync = b->qsync;
  e.dbg = b->debug ? (T*)b->dbg : nullptr;
  return e;
}

hs::StepParams params_of(const hs_batch* b, int mode, int nsub) {
  hs::StepParams p{};
  p.mode = mode;
  p.nsub = nsub;
  p.max_steps = b->cfg.max_steps;
  p.reward_id = b->cfg.reward_id;
  p.autoreset = b->cfg.autoreset;
  p.obs_dim = b->obs_dim;
  p.max_newton = b->cfg.max_newton;
  p.full_state = b->full_state ? 1 : 0;
  p.duration = b->cfg.duration;
  p.init_height = b->cfg.init_height;
  p.noise_scale = b->cfg.noise_scale;
  p.seed = b->seed;
  for (int k = 0; k < 9; k++) p.kneel[k] = b->cfg.kneel_params[k];
  p.solver = b->model->host.solver == 1 ? hs::SOLVER_PGS : hs::SOLVER_NEWTON;
  p.outputs = b->cfg.outputs;
  p.schedule = b->cfg.schedule;
  p.dbg_lose_pair1 = b->lose_env1;          // (launch_step maps it to the queue unit)
  return p;
}

int launch(hs_batch* b, int mode, const float* act, const uint8_t* mask, const void* nq, const void* nvz, int nsub,
           void* stream, int nsteps = 1, const hs_tape_out* tape = nullptr, const hs::RolloutArgs* ro = nullptr,
           const hs::EvalArgs* ev = nullptr, const hs::NormArgs* nm = nullptr) {
  if (!b) return fail("null batch");
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  hipError_t e;
  auto p = params_of(b, mode, nsub);
  p.nsteps = nsteps;
  int nv = b->model->host.nv;
  // a tape launch of a batch with a fused-capable termination condition: the TERM instances (the entry points
  // have refused every other tape launch of a batch with a condition)
  hs::TermArgs tm{};
  const bool term = mode == hs::MODE_ENV_STEP && b->term_prog && b->term_kind != 0 && (nsteps > 1 || ro);
  if (term) {
    tm.kind = b->term_kind;
    tm.grace_steps = b->grace_steps;
    tm.min_height = b->term_min_height;
    tm.max_roll_pitch = b->term_max_roll_pitch;
    tm.grace_count = b->grace_count;
    tm.grace_episode = b->grace_episode;
    tm.early = b->early;
    tm.mid_count = b->mid_count;
  }
  if (b->precision == HS_FP64) {
    hs::TapeOut<double> to{tape ? (double*)tape->obs : nullptr, tape ? (double*)tape->reward : nullptr,
                           tape ? tape->terminated : nullptr, tape ? tape->truncated : nullptr};
    e = hs::launch_step<double>((const hs::DevModel<double>*)b->dmodel, nv, env_buffers<double>(b), act, mask,
                                (const double*)nq, (const double*)nvz, p, b->n, (hipStream_t)stream, &to, ro, ev, nm,
                                term ? &tm : nullptr);
  } else {
    if (term) return fail("a fused launch with a termination condition runs on the fp64 Newton engine");
    hs::TapeOut<float> to{tape ? (float*)tape->obs : nullptr, tape ? (float*)tape->reward : nullptr,
                          tape ? tape->terminated : nullptr, tape ? tape->truncated : nullptr};
    e = hs::launch_step<float>((const hs::DevModel<float>*)b->dmodel, nv, env_buffers<float>(b), act, mask,
                               (const float*)nq, (const float*)nvz, p, b->n, (hipStream_t)stream, &to);
  }
  if (e == hipErrorInvalidValue) return fail("no kernel instance for this model's nv (compiled: nv = 27)");
  return hip_rc(e, "step kernel launch");
}

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

int fused_step_cap(const hs_batch* b) {
  return b->term_prog && b->term_kind != 0 ? hs::QTAG_STEPS : std::min(min_episode_len(b), hs::QTAG_STEPS);
}

struct Region { void* p; size_t bytes; };

// the env state a tape launch changes (restored when it aborts on a resident-tier overflow)
std::vector<Region> state_regions(const hs_batch* b) {
  const auto& h = b->model->host;
  const size_t N = (size_t)b->n, es = b->precision == HS_FP64 ? 8 : 4;
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

template <typename T>
bool upload_model(hs_batch* b, std::string& err) {
  auto* d = new hs::DevModel<T>();
  if (!hs::build_dev_model<T>(b->model->host, *d, err)) { delete d; return false; }
  if (!hip_ok(hipMalloc(&b->dmodel, sizeof(hs::DevModel<T>)), "hipMalloc(model)")) { delete d; err = g_err; return false; }
  bool ok = hip_ok(hipMemcpy(b->dmodel, d, sizeof(hs::DevModel<T>), hipMemcpyHostToDevice), "upload model");
  delete d;
  if (!ok) err = g_err;
  return ok;
}

template <typename T>
bool init_state(hs_batch* b) {
  const auto& m = b->model->host;
  int N = b->n;
  std::vector<T> q((size_t)N * m.nq);
  for (int i = 0; i < N; i++)
    for (int k = 0; k < m.nq; k++) q[(size_t)i * m.nq + k] = (T)m.qpos0[k];
  size_t es = sizeof(T);
  return hip_ok(hipMemcpy(b->buf.qpos, q.data(), q.size() * es, hipMemcpyHostToDevice), "init qpos") &&
         hip_ok(hipMemset(b->buf.qvel, 0, (size_t)N * m.nv * es), "init") &&
         hip_ok(hipMemset(b->buf.qacc_warmstart, 0, (size_t)N * m.nv * es), "init") &&
         hip_ok(hipMemset(b->buf.ctrl, 0, (size_t)N * m.nu * es), "init") &&
         hip_ok(hipMemset(b->buf.time, 0, (size_t)N * es), "init") &&
         hip_ok(hipMemset(b->buf.step_count, 0, (size_t)N * 4), "init") &&
         hip_ok(hipMemset(b->buf.episode, 0, (size_t)N * 4), "init") &&
         hip_ok(hipMemset(b->buf.total_reward, 0, (size_t)N * es), "init") &&
         hip_ok(hipMemset(b->buf.warning, 0, (size_t)N * HS_NWARN * 4), "init") &&
         hip_ok(hipMemset(b->buf.obs, 0, (size_t)N * b->obs_dim * es), "init") &&
         hip_ok(hipMemset(b->buf.terminal_obs, 0, (size_t)N * b->obs_dim * es), "init") &&
         hip_ok(hipMemset(b->buf.reward, 0, (size_t)N * es), "init") &&
         hip_ok(hipMemset(b->buf.terminated, 0, (size_t)N), "init") &&
         hip_ok(hipMemset(b->buf.truncated, 0, (size_t)N), "init") &&
         hip_ok(hipMemset(b->buf.aux, 0, (size_t)N * hs::AUXDIM * es), "init") &&
         (!b->buf.cfrc_ext || hip_ok(hipMemset(b->buf.cfrc_ext, 0, (size_t)N * m.nbody * 6 * es), "init")) &&
         (!b->buf.subtree_linvel || hip_ok(hipMemset(b->buf.subtree_linvel, 0, (size_t)N * m.nbody * 3 * es), "init")) &&
         (!b->buf.terminal_step_count || hip_ok(hipMemset(b->buf.terminal_step_count, 0, (size_t)N * 4), "init")) &&
         (!b->buf.terminal_total_reward || hip_ok(hipMemset(b->buf.terminal_total_reward, 0, (size_t)N * es), "init")) &&
         hip_ok(hipMemset(b->redo, 0, (size_t)(N + 2) * sizeof(int)), "init") &&
         hip_ok(hipMemset(b->redo_total, 0, sizeof(unsigned long long)), "init") &&
         hip_ok(hipMemset(b->qsync, 0, hs::qsync_words(N) * sizeof(int)), "init") &&
         // a recycled UC block holds another batch's rows: a lost hand-off reads this row's warning
         // counters and time (hs_env_step.h step_pair), so they start at 0, not at stale bits
         hip_ok(hipMemset(b->mid, 0, (size_t)N * hs::MIDDIM * es), "init");
}

template <typename T>
int state_io(hs_batch* b, int dir, double* qpos, double* qvel, double* warm, double* time, double* ctrl) {
  const auto& m = b->model->host;
  size_t N = (size_t)b->n;
  struct Item { void* dev; double* host; size_t n; } items[] = {
      {b->buf.qpos, qpos, N * m.nq}, {b->buf.qvel, qvel, N * m.nv}, {b->buf.qacc_warmstart, warm, N * m.nv},
      {b->buf.time, time, N}, {b->buf.ctrl, ctrl, N * m.nu}};
  for (auto& it : items) {
    if (!it.host) continue;
    std::vector<T> tmp(it.n);
    if (dir == 0) {
      if (!hip_ok(hipMemcpy(tmp.data(), it.dev, it.n * sizeof(T), hipMemcpyDeviceToHost), "state get")) return -1;
      for (size_t k = 0; k < it.n; k++) it.host[k] = (double)tmp[k];
    } else {
      for (size_t k = 0; k < it.n; k++) tmp[k] = (T)it.host[k];
      if (!hip_ok(hipMemcpy(it.dev, tmp.data(), it.n * sizeof(T), hipMemcpyHostToDevice), "state set")) return -1;
    }
  }
  return 0;
}
template <typename T>
int kinematics_io(hs_batch* b, int env, const double* qpos, double* xpos, double* xmat, double* gxpos,
                  double* gzaxis, double* com) {
  const auto& m = b->model->host;
  T* dq = nullptr;
  T* dout = nullptr;
  int rc = -1;
  std::vector<T> out(hs::KINDIM);
  if (!hip_ok(hipMalloc(&dq, m.nq * sizeof(T)), "kinematics alloc") ||
      !hip_ok(hipMalloc(&dout, hs::KINDIM * sizeof(T)), "kinematics alloc"))
    goto done;
  if (qpos) {
    std::vector<T> q(qpos, qpos + m.nq);
    if (!hip_ok(hipMemcpy(dq, q.data(), m.nq * sizeof(T), hipMemcpyHostToDevice), "kinematics qpos")) goto done;
  } else if (!hip_ok(hipMemcpy(dq, (const T*)b->buf.qpos + (size_t)env * m.nq, m.nq * sizeof(T),
                               hipMemcpyDeviceToDevice), "kinematics qpos")) {
    goto done;
  }
  if (!hip_ok(hs::launch_kinematics<T>((const hs::DevModel<T>*)b->dmodel, m.nv, dq, dout, nullptr), "kinematics launch") ||
      !hip_ok(hipMemcpy(out.data(), dout, hs::KINDIM * sizeof(T), hipMemcpyDeviceToHost), "kinematics out"))
    goto done;
  {
    struct Part { double* dst; int off, n; } parts[] = {
        {xpos, 0, m.nbody * 3}, {xmat, hs::MAXBODY * 3, m.nbody * 9}, {gxpos, hs::MAXBODY * 12, m.ngeom * 3},
        {gzaxis, hs::MAXBODY * 12 + hs::MAXGEOM * 3, m.ngeom * 3}, {com, hs::MAXBODY * 12 + hs::MAXGEOM * 6, 3}};
    for (auto& p : parts)
      if (p.dst)
        for (int k = 0; k < p.n; k++) p.dst[k] = (double)out[p.off + k];
  }
  rc = 0;
done:
  if (dq) (void)hipFree(dq);
  if (dout) (void)hipFree(dout);
  return rc;
}
}  // namespace

namespace {
// f(compiled model) for the precision's DevModel built on the host (no device involved)
template <typename T, typename F>
int with_dev_model(const hs_model* m, F&& f) {
  auto d = std::make_unique<hs::DevModel<T>>();
  std::string err;
  if (!hs::build_dev_model<T>(m->host, *d, err)) return fail(err);
  return f(*d);
}

// the env step's one launch, as the batch's config has it
int step_launch(hs_batch* b, const float* actions, void* stream) {
  int rc = launch(b, hs::MODE_ENV_STEP, actions, nullptr, b->ar_qpos_noise, b->ar_qvel_noise, b->cfg.frame_skip, stream);
  // a step with the ctrl copy on rewrites every env's data.ctrl (commit), one with it off leaves it stale
  if (rc == 0) b->ctrl_stale = !(b->cfg.outputs & HS_OUT_CTRL);
  return rc;
}

// hs_step / hs_step_program on a batch with a termination set, and hs_step_program on any batch: the step
// without auto-reset, the outcome launch, the masked reset (defined with the reward programs below)
int step_outcome_reset(hs_batch* b, const float* actions, const hs_reward_program* prog, const double* params,
                       void* stream);
const char kNoFusedWithTermination[] =
    ": the batch has a termination condition set (hs_set_termination), and a fused launch is bounded by the "
    "shortest possible episode, which a state-dependent end makes unknowable -- step with hs_step / "
    "hs_step_program, or clear the condition";
// the condition keeps the fused launches out unless it is fused-capable (hs_set_termination_builtin)
bool term_blocks_fused(const hs_batch* b) { return b->term_prog && b->term_kind == 0; }
// the most env steps of one fused launch: each env finishes at most one episode in it (min_episode_len), unless
// a fused-capable condition is set -- its instances write nothing once per episode (hs_env_step.h env_outcome)
int fused_step_cap(const hs_batch* b);
}  // namespace

extern "C" {

const char* hs_last_error(void) { return g_err.c_str(); }
const char* hs_version(void) { return "hsim 0.1.0 (gfx950)"; }

hs_model* hs_model_load(const char* xml_path, char* err, int errsz) {
  auto* m = new hs_model();
  std::string e;
  if (!xml_path || !hs::compile_mjcf_file(xml_path, m->host, e)) {
    if (!xml_path) e = "null path";
    g_err = e;
    if (err && errsz > 0) { std::strncpy(err, e.c_str(), errsz - 1); err[errsz - 1] = 0; }
    delete m;
    return nullptr;
  }
  return m;
}

void hs_model_free(hs_model* m) { delete m; }

int hs_model_field(const hs_model* m, const char* name, double* out, int n) {
  if (!m || !name) return fail("null argument");
  int r = hs::model_field(m->host, name, out, n);
  if (r < 0) return fail(std::string("unknown model field '") + name + "'");
  return r;
}

int hs_model_lane_table(const hs_model* m, int precision, void* out, int nbytes) {
  if (!m || (precision != HS_FP32 && precision != HS_FP64)) return fail("hs_model_lane_table: bad argument");
  auto copy = [&](const auto& d) {
    const int sz = (int)sizeof d.lanes;
    if (out && nbytes >= sz) std::memcpy(out, &d.lanes, sz);
    return sz;
  };
  return precision == HS_FP64 ? with_dev_model<double>(m, copy) : with_dev_model<float>(m, copy);
}

int hs_lane_layout(int precision, int i, char* name, int namesz, int* offset, int* count, int* kind) {
  if (precision != HS_FP32 && precision != HS_FP64) return fail("hs_lane_layout: bad precision");
  const hs::LaneEntry* e = nullptr;
  const int n = precision == HS_FP64 ? hs::lane_layout<double>(&e) : hs::lane_layout<float>(&e);
  if (i < 0 || i >= n) return n;
  if (name && namesz > 0) { std::strncpy(name, e[i].name, namesz - 1); name[namesz - 1] = 0; }
  if (offset) *offset = e[i].offset;
  if (count) *count = e[i].count;
  if (kind) *kind = e[i].kind;
  return n;
}

int hs_model_lane_source(const hs_model* m, int precision, const char* name, double* out, int n) {
  if (!m || !name || (precision != HS_FP32 && precision != HS_FP64)) return fail("hs_model_lane_source: bad argument");
  auto get = [&](const auto& d) {
    const int r = hs::lane_source_field(d, name, out, n);
    return r < 0 ? fail(std::string("the lane table has no entry '") + name + "'") : r;
  };
  return precision == HS_FP64 ? with_dev_model<double>(m, get) : with_dev_model<float>(m, get);
}

hs_batch* hs_batch_create(const hs_model* m, int n_envs, int device, uint64_t seed, int precision,
                          const hs_buffers* external) {
  if (!m || n_envs <= 0) { fail("hs_batch_create: null model or n_envs <= 0"); return nullptr; }
  if ((precision & ~HS_FULL_STATE) != HS_FP32 && (precision & ~HS_FULL_STATE) != HS_FP64) {
    fail("precision must be HS_FP32 or HS_FP64 (optionally | HS_FULL_STATE)");
    return nullptr;
  }
  if ((precision & HS_FULL_STATE) && external && (!external->cfrc_ext || !external->subtree_linvel)) {
    fail("HS_FULL_STATE needs external cfrc_ext and subtree_linvel buffers");
    return nullptr;
  }
  int ndev = 0;
  hipError_t de = hipGetDeviceCount(&ndev);
  if (de != hipSuccess || ndev == 0) {
    fail(std::string("no HIP device available (hipGetDeviceCount: ") + hipGetErrorString(de) + ", count " +
         std::to_string(ndev) + ")");
    return nullptr;
  }
  if (device < 0 || device >= ndev) { fail("device index out of range"); return nullptr; }
  DeviceGuard g(device);
  auto* b = new hs_batch();
  b->model = m;
  b->n = n_envs;
  b->device = device;
  b->seed = seed;
  b->full_state = (precision & HS_FULL_STATE) != 0;
  precision &= ~HS_FULL_STATE;
  b->precision = precision;
  b->obs_dim = obs_dim_of(m->host) + (b->full_state ? 6 * (m->host.nbody - 1) : 0);
  b->cfg.frame_skip = 5;
  b->cfg.max_steps = 750;
  b->cfg.reward_id = HS_REWARD_STAND;
  b->cfg.autoreset = 1;
  b->cfg.max_newton = m->host.iterations;     // <option iterations>
  b->cfg.outputs = HS_OUT_AUX | HS_OUT_CTRL;
  b->cfg.duration = 15.0;
  b->cfg.init_height = 1.282;
  b->cfg.noise_scale = 0.01;
  const double kneel[9] = {1.282, 0.85, 3.14159265358979323846 / 6, 0.1, 0.3, 0.3, 0.2, 0.1, 0.1};
  std::memcpy(b->cfg.kneel_params, kneel, sizeof kneel);
  std::string err;
  bool ok = precision == HS_FP64 ? upload_model<double>(b, err) : upload_model<float>(b, err);
  if (!ok) { g_err = err; delete b; return nullptr; }
  size_t es = precision == HS_FP64 ? 8 : 4, N = (size_t)n_envs;
  const auto& h = m->host;
  if (external) {
    b->buf = *external;
    b->owns = false;
  } else {
    b->owns = true;
    auto al = [&](void** p, size_t bytes) { return hip_ok(hipMalloc(p, bytes > 0 ? bytes : 4), "hipMalloc"); };
    ok = al(&b->buf.qpos, N * h.nq * es) && al(&b->buf.qvel, N * h.nv * es) &&
         al(&b->buf.qacc_warmstart, N * h.nv * es) && al(&b->buf.ctrl, N * h.nu * es) && al(&b->buf.time, N * es) &&
         al((void**)&b->buf.step_count, N * 4) && al((void**)&b->buf.episode, N * 4) &&
         al(&b->buf.total_reward, N * es) && al((void**)&b->buf.warning, N * HS_NWARN * 4) &&
         al(&b->buf.obs, N * b->obs_dim * es) && al(&b->buf.terminal_obs, N * b->obs_dim * es) &&
         al(&b->buf.reward, N * es) && al((void**)&b->buf.terminated, N) && al((void**)&b->buf.truncated, N) &&
         al(&b->buf.aux, N * hs::AUXDIM * es) && al(&b->buf.cfrc_ext, N * h.nbody * 6 * es) &&
         al(&b->buf.subtree_linvel, N * h.nbody * 3 * es) && al((void**)&b->buf.terminal_step_count, N * 4) &&
         al(&b->buf.terminal_total_reward, N * es);
    if (!ok) { hs_batch_destroy(b); return nullptr; }
  }
  if (!hip_ok(hipMalloc(&b->dbg, hs::DBGDIM * 8), "hipMalloc(dbg)") ||
      !hip_ok(hipMalloc((void**)&b->redo, (N + 2) * sizeof(int)), "hipMalloc(redo)") ||
      !hip_ok(hipMalloc((void**)&b->redo_total, sizeof(unsigned long long)), "hipMalloc(redo_total)") ||
      !hip_ok(hipMalloc((void**)&b->prog_done, N), "hipMalloc(prog_done)") ||
      // chunk-queue hand-off rows, claim counters and pair flags: UNCACHED device memory from the UC
      // pool above, so a hand-off between waves on different CUs / XCDs needs no L2 write-back or
      // invalidate (hs_env_step.h step_pair)
      !(uc_alloc(device, N * hs::MIDDIM * es, &b->mid) ? true
          : (g_err = "hipExtMallocWithFlags(mid, uncached) failed", false)) ||
      !(uc_alloc(device, hs::qsync_words((int)N) * sizeof(int), (void**)&b->qsync) ? true
          : (g_err = "hipExtMallocWithFlags(qsync, uncached) failed", false))) {
    hs_batch_destroy(b);
    return nullptr;
  }
  ok = precision == HS_FP64 ? init_state<double>(b) : init_state<float>(b);
  if (!ok) { hs_batch_destroy(b); return nullptr; }
  return b;
}

void hs_batch_destroy(hs_batch* b) {
  if (!b) return;
  DeviceGuard g(b->device);
  if (b->owns) {
    void* ptrs[] = {b->buf.qpos, b->buf.qvel, b->buf.qacc_warmstart, b->buf.ctrl, b->buf.time, b->buf.step_count,
                    b->buf.episode, b->buf.total_reward, b->buf.warning, b->buf.obs, b->buf.terminal_obs,
                    b->buf.reward, b->buf.terminated, b->buf.truncated, b->buf.aux, b->buf.cfrc_ext,
                    b->buf.subtree_linvel, b->buf.terminal_step_count, b->buf.terminal_total_reward};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
  }
  if (b->dmodel) (void)hipFree(b->dmodel);
  if (b->dbg) (void)hipFree(b->dbg);
  if (b->redo) (void)hipFree(b->redo);
  if (b->redo_total) (void)hipFree(b->redo_total);
  if (b->prog_done) (void)hipFree(b->prog_done);
  if (b->grace_count) (void)hipFree(b->grace_count);
  if (b->grace_episode) (void)hipFree(b->grace_episode);
  if (b->early) (void)hipFree(b->early);
  uc_release(b->device, (size_t)b->n * sizeof(int32_t), b->mid_count);
  if (b->mid) uc_release(b->device, (size_t)b->n * hs::MIDDIM * (b->precision == HS_FP64 ? 8 : 4), b->mid);
  if (b->qsync) uc_release(b->device, hs::qsync_words(b->n) * sizeof(int), b->qsync);
  if (b->eval_obs) uc_release(b->device, (size_t)b->n * b->obs_dim * sizeof(float), b->eval_obs);
  if (b->tape_backup) (void)hipFree(b->tape_backup);
  if (b->kin_envs) (void)hipFree(b->kin_envs);
  if (b->order_ev) (void)hipEventDestroy(b->order_ev);
  for (auto& e : b->tape_ev)
    if (e) (void)hipEventDestroy(e);
  delete b;
}

int hs_batch_get_info(const hs_batch* b, hs_batch_info* out) {
  if (!b || !out) return fail("null argument");
  const auto& h = b->model->host;
  out->n_envs = b->n;
  out->precision = b->precision;
  out->nq = h.nq; out->nv = h.nv; out->nu = h.nu; out->nbody = h.nbody;
  out->obs_dim = b->obs_dim;
  out->elem_size = b->precision == HS_FP64 ? 8 : 4;
  out->resident_con = b->precision == HS_FP64 ? hs::MAXCON_F64 : hs::MAXCON;
  out->resident_efc = b->precision == HS_FP64 ? hs::MAXEFC_F64 : hs::MAXEFC;
  out->wide_con = hs::MAXCON_WIDE;
  out->wide_efc = hs::MAXEFC_WIDE;
  const hs::ContactBound cb = hs::contact_bound(h);
  out->bound_con_all = cb.con_all;
  out->bound_efc_all = cb.efc_all;
  out->bound_con_floor = cb.con_floor;
  out->bound_efc_floor = cb.efc_floor;
  {
    DeviceGuard g(b->device);
    const bool pgs = b->model->host.solver == 1;
    out->resident_waves = b->precision == HS_FP64 ? hs::resident_waves<double>(pgs) : hs::resident_waves<float>(pgs);
  }
  return 0;
}

int hs_get_buffers(const hs_batch* b, hs_buffers* out) {
  if (!b || !out) return fail("null argument");
  *out = b->buf;
  return 0;
}

int hs_set_config(hs_batch* b, const hs_env_config* cfg) {
  if (!b || !cfg) return fail("null argument");
  if (cfg->frame_skip < 1) return fail("frame_skip must be >= 1");
  if (cfg->max_newton < 1) return fail("max_newton must be >= 1");
  if (cfg->reward_id < HS_REWARD_NONE || cfg->reward_id > HS_REWARD_WALK) return fail("unknown reward id");
  if (cfg->outputs & ~(HS_OUT_AUX | HS_OUT_CTRL)) return fail("unknown output bits");
  if (cfg->schedule != HS_SCHED_AUTO && cfg->schedule != HS_SCHED_DIRECT && cfg->schedule != HS_SCHED_SINGLE &&
      cfg->schedule != HS_SCHED_FIXED_ORDER)
    return fail("unknown schedule");
  b->cfg = *cfg;
  return 0;
}

int hs_set_seed(hs_batch* b, uint64_t seed) {
  if (!b) return fail("null batch");
  b->seed = seed;
  return 0;
}

int hs_get_config(const hs_batch* b, hs_env_config* cfg) {
  if (!b || !cfg) return fail("null argument");
  *cfg = b->cfg;
  return 0;
}

int hs_reset(hs_batch* b, const uint8_t* mask, const void* qpos_noise, const void* qvel_noise, void* stream) {
  int rc = launch(b, hs::MODE_RESET, nullptr, mask, qpos_noise, qvel_noise, 1, stream);
  if (rc == 0 && !mask) b->ctrl_stale = false;     // every env's data.ctrl is 0 again (mj_resetData)
  return rc;
}

int hs_step(hs_batch* b, const float* actions, void* stream) {
  if (!actions) return fail("hs_step: actions must not be NULL");
  if (!b) return fail("null batch");
  // a termination condition: step, outcome launch, masked reset.  Without a device reward the reward is the
  // caller's, and so is the outcome that follows it (hs_apply_termination): the step alone
  if (b->term_prog && b->cfg.reward_id != HS_REWARD_NONE) return step_outcome_reset(b, actions, nullptr, nullptr, stream);
  return step_launch(b, actions, stream);
}

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
  const size_t N = (size_t)b->n, es = b->precision == HS_FP64 ? 8 : 4, nu = (size_t)h.nu;
  hipStream_t st = (hipStream_t)stream;
  // n_steps hs_step calls, each step's outputs copied into its slice (the reference path, and the
  // replay of an aborted tape launch)
  auto per_step = [&]() -> int {
    for (int t = 0; t < n_steps; t++) {
      int rc = hs_step(b, actions + (size_t)t * N * nu, stream);
      if (rc) return rc;
      if (out) {
        const size_t d = (size_t)b->obs_dim;
        if (!hip_ok(hipMemcpyAsync((char*)out->obs + t * N * d * es, b->buf.obs, N * d * es, hipMemcpyDeviceToDevice, st),
                    "tape obs") ||
            !hip_ok(hipMemcpyAsync((char*)out->reward + t * N * es, b->buf.reward, N * es, hipMemcpyDeviceToDevice, st),
                    "tape reward") ||
            !hip_ok(hipMemcpyAsync(out->terminated + t * N, b->buf.terminated, N, hipMemcpyDeviceToDevice, st),
                    "tape terminated") ||
            !hip_ok(hipMemcpyAsync(out->truncated + t * N, b->buf.truncated, N, hipMemcpyDeviceToDevice, st),
                    "tape truncated"))
          return -1;
      }
    }
    return 0;
  };
  const int resident = b->precision == HS_FP64 ? hs::resident_waves<double>(h.solver == 1)
                                               : hs::resident_waves<float>(h.solver == 1);
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
      if (out) {
        sub.obs = (char*)out->obs + (size_t)t0 * N * b->obs_dim * es;
        sub.reward = (char*)out->reward + (size_t)t0 * N * es;
        sub.terminated = out->terminated + (size_t)t0 * N;
        sub.truncated = out->truncated + (size_t)t0 * N;
      }
      int rc = hs_step_tape(b, actions + (size_t)t0 * N * nu, k, out ? &sub : nullptr, stream);
      if (rc) return rc;
    }
    return 0;
  }
  // an env that overflows the resident tier stops the tape launch (QS_ABORT), and the tape is then
  // replayed step by step from the saved state (the wide tier re-runs the overflowing steps) -- the
  // same results, bitwise, as n_steps hs_step calls either way
  int rc = guarded_tape(b, state_regions(b), st, [&] {
    return launch(b, hs::MODE_ENV_STEP, actions, nullptr, b->ar_qpos_noise, b->ar_qvel_noise, b->cfg.frame_skip,
                  stream, n_steps, out);
  });
  if (rc < 0) return rc;
  if (rc == 1) return per_step();
  b->ctrl_stale = !(b->cfg.outputs & HS_OUT_CTRL);
  if (out) {   // the batch's own output buffers hold the last step, as after n_steps hs_step calls
    const size_t d = (size_t)b->obs_dim, t = (size_t)n_steps - 1;
    if (!hip_ok(hipMemcpyAsync(b->buf.obs, (char*)out->obs + t * N * d * es, N * d * es, hipMemcpyDeviceToDevice, st),
                "tape obs") ||
        !hip_ok(hipMemcpyAsync(b->buf.reward, (char*)out->reward + t * N * es, N * es, hipMemcpyDeviceToDevice, st),
                "tape reward") ||
        !hip_ok(hipMemcpyAsync(b->buf.terminated, out->terminated + t * N, N, hipMemcpyDeviceToDevice, st),
                "tape terminated") ||
        !hip_ok(hipMemcpyAsync(b->buf.truncated, out->truncated + t * N, N, hipMemcpyDeviceToDevice, st),
                "tape truncated"))
      return -1;
  }
  return 0;
}

static_assert(HS_ACT_RELU == hs::ACT_RELU && HS_ACT_TANH == hs::ACT_TANH, "activation ids");

int hs_rollout_max_steps(const hs_batch* b) {
  if (!b) return fail("null batch");
  return fused_step_cap(b);
}

int hs_rollout(hs_batch* b, const hs_policy* pol, const hs_rollout_bufs* rb, int t_begin, int n_steps, int t_total,
               void* stream) {
  return hs_rollout_act(b, pol, HS_ACT_RELU, rb, t_begin, n_steps, t_total, stream);
}

namespace {
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

int rollout_impl(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb, int t_begin, int n_steps,
                 int t_total, void* stream, const hs_obs_norm_args* on, bool norm);
int evaluate_impl(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, int t_begin, int n_steps,
                  int t_total, void* stream, const hs_obs_norm_args* on, bool norm);
}  // namespace

int hs_rollout_act(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb, int t_begin, int n_steps,
                   int t_total, void* stream) {
  return rollout_impl(b, pol, act, rb, t_begin, n_steps, t_total, stream, nullptr, false);
}

int hs_rollout_norm(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb,
                    const hs_obs_norm_args* norm, int t_begin, int n_steps, int t_total, void* stream) {
  return rollout_impl(b, pol, act, rb, t_begin, n_steps, t_total, stream, norm, true);
}

int hs_evaluate(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, int t_begin, int n_steps,
                int t_total, void* stream) {
  return evaluate_impl(b, pol, act, eb, t_begin, n_steps, t_total, stream, nullptr, false);
}

int hs_evaluate_norm(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, const hs_obs_norm_args* norm,
                     int t_begin, int n_steps, int t_total, void* stream) {
  return evaluate_impl(b, pol, act, eb, t_begin, n_steps, t_total, stream, norm, true);
}

namespace {
int rollout_impl(hs_batch* b, const hs_policy* pol, int act, const hs_rollout_bufs* rb, int t_begin, int n_steps,
                 int t_total, void* stream, const hs_obs_norm_args* on, bool norm) {
  if (!b || !pol || !rb) return fail("null argument");
  int hidden = 0;
  if (int rc = fused_policy_check(b, pol, act, t_begin, n_steps, t_total, norm ? "hs_rollout_norm" : "hs_rollout",
                                  &hidden))
    return rc;
  hs::NormArgs nm{};
  if (norm)
    if (int rc = norm_args_check(b, on, "hs_rollout_norm", &nm)) return rc;
  for (const void* q : {(const void*)pol->w1, (const void*)pol->b1, (const void*)pol->w2, (const void*)pol->b2,
                        (const void*)pol->w3, (const void*)pol->b3, (const void*)pol->log_std, (const void*)rb->obs,
                        (const void*)rb->obs_last, (const void*)rb->actions, (const void*)rb->log_probs,
                        (const void*)rb->episode_starts, (const void*)rb->rewards, (const void*)rb->dones,
                        (const void*)rb->episode_returns, (const void*)rb->boot, (const void*)rb->terminal_obs,
                        (const void*)rb->ep_acc, (const void*)rb->episode_start, (const void*)rb->actions_clipped,
                        (const void*)rb->counter_base})
    if (!q) return fail("hs_rollout: every policy weight and rollout buffer must be given");
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  const int resident = hs::resident_waves<double>(false);
  if (resident <= 0 || !b->mid || !b->qsync) return fail("hs_rollout: no resident-wave count / queue buffers");
  hs::RolloutArgs ro = policy_args(pol, hidden, act);
  ro.t_begin = t_begin; ro.t_total = t_total;
  ro.obs = rb->obs; ro.obs_last = rb->obs_last; ro.act = rb->actions; ro.logp = rb->log_probs;
  ro.start = rb->episode_starts; ro.rew = rb->rewards; ro.done = rb->dones; ro.epret = rb->episode_returns;
  ro.boot = rb->boot; ro.tobs = rb->terminal_obs; ro.ep_acc = rb->ep_acc; ro.episode_start = rb->episode_start;
  ro.act_clip = rb->actions_clipped; ro.ctr_base = rb->counter_base;
  ro.k0 = (uint32_t)rb->seed; ro.k1 = (uint32_t)(rb->seed >> 32); ro.deterministic = rb->deterministic;
  const size_t N = (size_t)b->n;
  std::vector<Region> regs = state_regions(b);
  regs.push_back({rb->ep_acc, N * sizeof(double)});
  regs.push_back({rb->episode_start, N * sizeof(float)});
  regs.push_back({rb->actions_clipped, N * (size_t)pol->act_dim * sizeof(float)});
  hipStream_t st = (hipStream_t)stream;
  int rc = guarded_tape(b, regs, st, [&] {
    return launch(b, hs::MODE_ENV_STEP, rb->actions_clipped, nullptr, nullptr, nullptr, b->cfg.frame_skip, stream,
                  n_steps, nullptr, &ro, nullptr, norm ? &nm : nullptr);
  });
  if (rc == 0) b->ctrl_stale = !(b->cfg.outputs & HS_OUT_CTRL);
  return rc;
}

int evaluate_impl(hs_batch* b, const hs_policy* pol, int act, const hs_eval_bufs* eb, int t_begin, int n_steps,
                  int t_total, void* stream, const hs_obs_norm_args* on, bool norm) {
  if (!b || !pol || !eb) return fail("null argument");
  int hidden = 0;
  if (int rc = fused_policy_check(b, pol, act, t_begin, n_steps, t_total, norm ? "hs_evaluate_norm" : "hs_evaluate",
                                  &hidden))
    return rc;
  hs::NormArgs nm{};
  if (norm)
    if (int rc = norm_args_check(b, on, "hs_evaluate_norm", &nm)) return rc;
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
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  const int resident = hs::resident_waves<double>(false);
  if (resident <= 0 || !b->mid || !b->qsync) return fail("hs_evaluate: no resident-wave count / queue buffers");
  // the staging rows: one [obs_dim] f32 row per env, rewritten every env step by waves on any XCD, so
  // uncached memory like the hand-off rows (hs_env_step.h step_pair); allocated at the first evaluation
  const size_t N = (size_t)b->n;
  if (!b->eval_obs && !uc_alloc(b->device, N * (size_t)b->obs_dim * sizeof(float), &b->eval_obs)) {
    b->eval_obs = nullptr;
    return fail("hipExtMallocWithFlags(eval obs rows, uncached) failed");
  }
  hs::RolloutArgs ro = policy_args(pol, hidden, act);
  ro.t_begin = t_begin; ro.t_total = t_total;
  ro.obs = (float*)b->eval_obs;
  ro.act_clip = eb->actions_clipped; ro.ctr_base = eb->counter_base;
  ro.k0 = (uint32_t)eb->seed; ro.k1 = (uint32_t)(eb->seed >> 32); ro.deterministic = eb->deterministic;
  hs::EvalArgs ev{};
  ev.episode0 = eb->episode0; ev.max_episodes = eb->max_episodes; ev.n_trace = eb->n_trace;
  ev.ep_return = eb->ep_return; ev.ep_length = eb->ep_length; ev.ep_end_step = eb->ep_end_step;
  ev.tr_qpos = eb->trace_qpos; ev.tr_qvel = eb->trace_qvel; ev.tr_act = eb->trace_actions;
  ev.tr_rew = eb->trace_rewards; ev.tr_done = eb->trace_dones;
  std::vector<Region> regs = state_regions(b);
  regs.push_back({eb->actions_clipped, N * (size_t)pol->act_dim * sizeof(float)});
  int rc = guarded_tape(b, regs, (hipStream_t)stream, [&] {
    return launch(b, hs::MODE_ENV_STEP, eb->actions_clipped, nullptr, nullptr, nullptr, b->cfg.frame_skip, stream,
                  n_steps, nullptr, &ro, &ev, norm ? &nm : nullptr);
  });
  if (rc == 0) b->ctrl_stale = !(b->cfg.outputs & HS_OUT_CTRL);
  return rc;
}
}  // namespace

int hs_debug_lose_handoff(hs_batch* b, int env) {
  if (!b) return fail("null batch");
  if (env < -1 || env >= b->n) return fail("env index out of range");
  b->lose_env1 = env < 0 ? 0 : env + 1;
  return 0;
}

int hs_debug_queue_order(hs_batch* b, int* out, int n) {
  if (!b || (!out && n > 0) || n < 0) return fail("hs_debug_queue_order: bad argument");
  if (!b->qsync || b->cfg.schedule != HS_SCHED_AUTO) return 0;
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  // the queue's unit, as launch_step picks it (a small batch only ever queues tape launches, by env)
  const bool pgs = b->model->host.solver == 1;
  const int resident = b->precision == HS_FP64 ? hs::resident_waves<double>(pgs) : hs::resident_waves<float>(pgs);
  const int nunits = b->n <= resident ? b->n : (b->n + 1) / 2;
  std::vector<int> q(hs::qsync_words(b->n));
  if (!hip_ok(hipMemcpy(q.data(), b->qsync, q.size() * sizeof(int), hipMemcpyDeviceToHost), "qsync")) return -1;
  const int par = q[hs::QS_EPOCH] & 1;   // the parity the next launch reads
  const int* cnt = q.data() + hs::qs_cnt(nunits, par);
  const int* ord = q.data() + hs::qs_ord(nunits, par);
  long long total = 0;
  for (int k = 0; k < hs::QNB; k++) total += cnt[k] < 0 ? (long long)nunits + 1 : cnt[k];
  if (total != nunits) return 0;
  int w = 0;
  for (int k = 0; k < hs::QNB; k++)
    for (int s = 0; s < cnt[k]; s++, w++)
      if (w < n) out[w] = ord[(size_t)k * nunits + s];
  return nunits;
}

int hs_debug_queue_counters(hs_batch* b, int* out) {
  if (!b || !out) return fail("hs_debug_queue_counters: null argument");
  if (!b->qsync) return fail("hs_debug_queue_counters: the batch has no queue buffers");
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  static_assert(hs::QS_HEAD == 0 && hs::QS_EXIT == 1 && hs::QS_EPOCH == 2 && hs::QS_ABORT == 3, "sync word order");
  if (!hip_ok(hipMemcpy(out, b->qsync, 4 * sizeof(int), hipMemcpyDeviceToHost), "qsync")) return -1;
  return 0;
}

int hs_set_autoreset_noise(hs_batch* b, const void* qpos_noise, const void* qvel_noise) {
  if (!b) return fail("null batch");
  if ((qpos_noise == nullptr) != (qvel_noise == nullptr)) return fail("bind both noise arrays or neither");
  b->ar_qpos_noise = qpos_noise;
  b->ar_qvel_noise = qvel_noise;
  return 0;
}

int hs_physics_step(hs_batch* b, const float* ctrl, int nsub, void* stream) {
  if (nsub < 1) return fail("nsub must be >= 1");
  if (!b) return fail("null batch");
  if (!ctrl && b->ctrl_stale)
    return fail("hs_physics_step: ctrl == NULL keeps data.ctrl, but env steps ran with HS_OUT_CTRL off so the "
                "ctrl buffer is stale; pass ctrl, set it with hs_state_io, or enable HS_OUT_CTRL");
  int rc = launch(b, hs::MODE_PHYSICS, ctrl, nullptr, nullptr, nullptr, nsub, stream);
  if (rc == 0 && ctrl) b->ctrl_stale = false;
  return rc;
}

int hs_state_io(hs_batch* b, int dir, double* qpos, double* qvel, double* qacc_warmstart, double* time, double* ctrl) {
  if (!b) return fail("null batch");
  if (dir != 0 && dir != 1) return fail("dir must be 0 (get) or 1 (set)");
  if (dir == 0 && ctrl && b->ctrl_stale)
    return fail("hs_state_io: ctrl requested, but env steps ran with HS_OUT_CTRL off (the ctrl buffer is stale)");
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  int rc = b->precision == HS_FP64 ? state_io<double>(b, dir, qpos, qvel, qacc_warmstart, time, ctrl)
                                   : state_io<float>(b, dir, qpos, qvel, qacc_warmstart, time, ctrl);
  if (rc == 0 && dir == 1 && ctrl) b->ctrl_stale = false;   // only once the new ctrl is on the device
  return rc;
}

int hs_kinematics(hs_batch* b, int env, const double* qpos, double* xpos, double* xmat, double* geom_xpos,
                  double* geom_zaxis, double* com) {
  if (!b) return fail("null batch");
  if (env < 0 || env >= b->n) return fail("env index out of range");
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  return b->precision == HS_FP64 ? kinematics_io<double>(b, env, qpos, xpos, xmat, geom_xpos, geom_zaxis, com)
                                 : kinematics_io<float>(b, env, qpos, xpos, xmat, geom_xpos, geom_zaxis, com);
}

int hs_kinematics_batch(hs_batch* b, int n, const int32_t* envs, const void* qpos_dev, void* kin_dev, void* stream) {
  if (!b) return fail("hs_kinematics_batch: null batch");
  if (!kin_dev) return fail("hs_kinematics_batch: null kin_dev");
  if (n < 1) return fail("hs_kinematics_batch: n must be >= 1");
  if ((envs != nullptr) == (qpos_dev != nullptr))
    return fail("hs_kinematics_batch: exactly one of envs / qpos_dev must be given");
  if (envs)
    for (int i = 0; i < n; i++)
      if (envs[i] < 0 || envs[i] >= b->n)
        return fail("hs_kinematics_batch: env id " + std::to_string(envs[i]) + " out of range [0, " +
                    std::to_string(b->n) + ")");
  DeviceGuard g(b->device);
  hipStream_t st = (hipStream_t)stream;
  if (envs && n > b->kin_envs_cap) {
    // (hipFree waits for the device: no earlier launch still reads the old list)
    if (b->kin_envs) (void)hipFree(b->kin_envs);
    b->kin_envs = nullptr;
    b->kin_envs_cap = 0;
    const int cap = std::max(64, n);
    if (!hip_ok(hipMalloc(&b->kin_envs, (size_t)cap * sizeof(int)), "hipMalloc(kinematics env ids)")) return -1;
    b->kin_envs_cap = cap;
  }
  if (order_streams(b, st)) return -1;
  // pageable host memory: the copy has left `envs` when the call returns, and on the stream it is
  // ordered after the previous launch that read the list
  if (envs && !hip_ok(hipMemcpyAsync(b->kin_envs, envs, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st),
                      "kinematics env ids"))
    return -1;
  const int nv = b->model->host.nv;
  const int* de = envs ? b->kin_envs : nullptr;
  hipError_t e = b->precision == HS_FP64
      ? hs::launch_kinematics_batch<double>((const hs::DevModel<double>*)b->dmodel, nv, n, (const double*)qpos_dev,
                                            (const double*)b->buf.qpos, de, (double*)kin_dev, st)
      : hs::launch_kinematics_batch<float>((const hs::DevModel<float>*)b->dmodel, nv, n, (const float*)qpos_dev,
                                           (const float*)b->buf.qpos, de, (float*)kin_dev, st);
  if (e == hipErrorInvalidValue) return fail("no kernel instance for this model's nv (compiled: nv = 27)");
  return hip_rc(e, "kinematics batch launch");
}

int hs_render_frames(hs_batch* b, int n, const void* kin_dev, const hs_camera* cam, int H, int W, uint8_t* rgb_dev,
                     void* stream) {
  if (!b) return fail("hs_render_frames: null batch");
  if (!kin_dev || !cam || !rgb_dev) return fail("hs_render_frames: null argument");
  if (n < 1) return fail("hs_render_frames: n must be >= 1");
  if (H < 1 || H > 4096 || W < 1 || W > 4096) return fail("hs_render_frames: H and W must lie in [1, 4096]");
  if (!(cam->fovy > 0.0 && cam->fovy < 180.0)) return fail("hs_render_frames: fovy must lie in (0, 180) degrees");
  if (cam->mode != HS_CAM_BODY && cam->mode != HS_CAM_COM) return fail("hs_render_frames: unknown camera mode");
  const auto& h = b->model->host;
  if (cam->mode == HS_CAM_BODY && (cam->body < 0 || cam->body >= h.nbody))
    return fail("hs_render_frames: camera body out of range [0, nbody)");
  hs::RenderScene sc{};
  sc.ngeom = h.ngeom;
  for (int g = 0; g < h.ngeom; g++) {
    sc.geom_type[g] = h.geom_type[g];
    sc.geom_r[g] = h.geom_size[3 * g];
    sc.geom_hl[g] = h.geom_size[3 * g + 1];
  }
  hs::RenderCam rc{};
  rc.mode = cam->mode;
  rc.body = cam->mode == HS_CAM_BODY ? cam->body : 0;
  for (int k = 0; k < 3; k++) rc.pos[k] = cam->pos[k];
  for (int k = 0; k < 9; k++) rc.rot[k] = cam->rot[k];
  rc.f = 0.5 * H / std::tan(cam->fovy * (M_PI / 180.0) / 2);   // render.py: 0.5 H / tan(radians(fovy) / 2)
  DeviceGuard g(b->device);
  hipStream_t st = (hipStream_t)stream;
  if (order_streams(b, st)) return -1;
  hipError_t e = b->precision == HS_FP64 ? hs::launch_render<double>((const double*)kin_dev, n, sc, rc, H, W, rgb_dev, st)
                                         : hs::launch_render<float>((const float*)kin_dev, n, sc, rc, H, W, rgb_dev, st);
  return hip_rc(e, "render launch");
}

int hs_set_debug(hs_batch* b, int enable) {
  if (!b) return fail("null batch");
  b->debug = enable != 0;
  return 0;
}

int hs_get_debug(hs_batch* b, double* out, int n) {
  if (!b || !out) return fail("null argument");
  if (n < hs::DBGDIM) return fail("debug buffer too small");
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  if (b->precision == HS_FP64) return hip_rc(hipMemcpy(out, b->dbg, hs::DBGDIM * 8, hipMemcpyDeviceToHost), "dbg");
  std::vector<float> t(hs::DBGDIM);
  if (!hip_ok(hipMemcpy(t.data(), b->dbg, hs::DBGDIM * 4, hipMemcpyDeviceToHost), "dbg")) return -1;
  for (int k = 0; k < hs::DBGDIM; k++) out[k] = t[k];
  return 0;
}

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
  const double* kn = kneel_params ? kneel_params : kdef;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RewardEvalArgs<T> a{};
    a.reward_id = reward_id;
    a.n = n;
    a.nq = h.nq;
    a.nv = h.nv;
    a.nu = h.nu;
    a.nbody = h.nbody;
    for (int k = 0; k < 9; k++) a.kneel[k] = kn[k];
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
  };
  return prec == HS_FP64 ? run(0.0) : run(0.0f);
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
  const double* kn = kneel_params ? kneel_params : b->cfg.kneel_params;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RewardEvalArgs<T> a{};
    a.reward_id = reward_id;
    a.n = b->n;
    a.nq = h.nq;
    a.nv = h.nv;
    a.nu = h.nu;
    a.nbody = h.nbody;
    for (int k = 0; k < 9; k++) a.kneel[k] = kn[k];
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
  };
  return b->precision == HS_FP64 ? run(0.0) : run(0.0f);
}

// -- reward programs (hs_reward_prog.h) --------------------------------------------------------
}  // extern "C"

namespace {

const char* const kRpFieldNames[hs::RP_NFIELDS] = {"qpos", "qvel", "ctrl", "time", "qfrc_actuator", "cinert", "cvel",
                                                   "subtree_com[0]", "cfrc_ext", "subtree_linvel"};

// the program's code and constants on `device` (uploaded on first use there; hs_reward_program_create
// uploads to the device current at the time, so a later launch -- possibly under graph capture -- allocates nothing)
const hs_reward_program::Dev* rp_resident(hs_reward_program* p, int device) {
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
  const hs_reward_program::Dev* dp = p ? rp_resident(const_cast<hs_reward_program*>(p), b->device) : nullptr;
  const hs_reward_program::Dev* dt = t ? rp_resident(const_cast<hs_reward_program*>(t), b->device) : nullptr;
  if ((p && !dp) || (t && !dt)) return -1;
  auto run = [&](auto zero) -> int {
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
  };
  return b->precision == HS_FP64 ? run(0.0) : run(0.0f);
}

int step_outcome_reset(hs_batch* b, const float* actions, const hs_reward_program* p, const double* params,
                       void* stream) {
  // the predicate's needs once more, in case the config changed after hs_set_termination: before any launch
  if (b->term_prog && rp_check_batch("hs_step", b, b->term_prog, b->term_params, true)) return -1;
  // component rows bound: the program must write exactly that many, or a row would stay stale (or be overrun)
  if (p && b->comp_n > 0 && p->info.n_outputs != b->comp_n)
    return fail("hs_step_program: the program has " + std::to_string(p->info.n_outputs) + " outputs, the batch has " +
                std::to_string(b->comp_n) + " component rows bound (hs_set_reward_components)");
  DeviceGuard g(b->device);
  if ((p && !rp_resident(const_cast<hs_reward_program*>(p), b->device))) return -1;
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

}  // namespace

extern "C" {

int hs_reward_program_create(const hs_model* m, const int32_t* code, int n_instr, const double* consts, int n_consts,
                             int n_params, hs_reward_program** prog) {
  return hs_reward_program_create_components(m, code, n_instr, consts, n_consts, n_params, 0, prog);
}

int hs_reward_program_outputs(const hs_reward_program* p, int* n_outputs) {
  if (!p || !n_outputs) return fail("hs_reward_program_outputs: null argument");
  *n_outputs = p->info.n_outputs;
  return 0;
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

int hs_reward_program_eval_host(const hs_reward_program* p, const double* params, int n, const hs_reward_fields* f,
                                double* out) {
  return hs_reward_program_eval_host_components(p, params, n, f, out, nullptr);
}

int hs_reward_program_eval_host_components(const hs_reward_program* p, const double* params, int n,
                                           const hs_reward_fields* f, double* out, double* comp_out) {
  if (!p || !f) return fail("hs_reward_program_eval_host: null argument");
  if (n < 0) return fail("hs_reward_program_eval_host: negative n");
  if (comp_out && p->info.n_outputs == 0)
    return fail("hs_reward_program_eval_host_components: the program has no outputs, comp_out must be NULL");
  if (n == 0) return 0;
  if (!out || (p->n_params > 0 && !params)) return fail("hs_reward_program_eval_host: null out or params");
  const double* const* fp = reinterpret_cast<const double* const*>(f);
  for (int k = 0; k < hs::RP_NFIELDS; k++)
    if ((p->info.fields & (1u << k)) && !fp[k])
      return fail(std::string("hs_reward_program_eval_host: the program reads ") + kRpFieldNames[k] + ", which is NULL");
  hs::rp_eval_host(p->dims, p->code.data(), (int)(p->code.size() / 5), p->consts.data(), params, n, fp, out, comp_out);
  return 0;
}

int hs_reward_program_eval(const hs_reward_program* p, int precision, const double* params, int n,
                           const hs_reward_fields* f, void* out, void* stream) {
  if (!p || !f) return fail("hs_reward_program_eval: null argument");
  if (n < 0) return fail("hs_reward_program_eval: negative n");
  const int prec = precision & 0xFF;
  if (prec != HS_FP32 && prec != HS_FP64) return fail("hs_reward_program_eval: precision must be HS_FP32 or HS_FP64");
  if (n == 0) return 0;
  if (!out || (p->n_params > 0 && !params)) return fail("hs_reward_program_eval: null out or params");
  const void* const* fp = reinterpret_cast<const void* const*>(f);
  for (int k = 0; k < hs::RP_NFIELDS; k++)
    if ((p->info.fields & (1u << k)) && !fp[k])
      return fail(std::string("hs_reward_program_eval: the program reads ") + kRpFieldNames[k] + ", which is NULL");
  int cur = 0;
  if (!hip_ok(hipGetDevice(&cur), "hipGetDevice")) return -1;
  const auto* d = rp_resident(const_cast<hs_reward_program*>(p), cur);
  if (!d) return -1;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RpArgs<T> a = rp_args<T>(p, d, params, n);
    for (int k = 0; k < hs::RP_NFIELDS; k++) {
      a.field[k] = (const T*)fp[k];
      a.ld[k] = hs::rp_field_len(p->dims, k);
    }
    a.out = (T*)out;
    return hip_rc(hs::launch_reward_program<T>(a, (hipStream_t)stream), "reward_program_kernel");
  };
  return prec == HS_FP64 ? run(0.0) : run(0.0f);
}

int hs_reward_program_batch(hs_batch* b, const hs_reward_program* p, const double* params, void* out, void* stream) {
  return hs_reward_program_batch_components(b, p, params, out, nullptr, stream);
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
  const auto* d = rp_resident(const_cast<hs_reward_program*>(p), b->device);
  if (!d) return -1;
  if (order_streams(b, (hipStream_t)stream)) return -1;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    hs::RpArgs<T> a = rp_args<T>(p, d, params, b->n);
    rp_batch_fields<T>(b, a);
    a.out = (T*)out;
    a.comp = (T*)comp_out;
    a.n_outputs = p->info.n_outputs;
    return hip_rc(hs::launch_reward_program<T>(a, (hipStream_t)stream), "reward_program_kernel");
  };
  return b->precision == HS_FP64 ? run(0.0) : run(0.0f);
}

int hs_step_program(hs_batch* b, const float* actions, const hs_reward_program* p, const double* params, void* stream) {
  if (!actions) return fail("hs_step_program: actions must not be NULL");
  if (rp_check_batch("hs_step_program", b, p, params, true)) return -1;
  return step_outcome_reset(b, actions, p, params, stream);
}

}  // extern "C"

namespace {
// a predicate is read as one truth value: a program with named outputs is a reward, refused as a condition
int term_refuse_outputs(const char* who, const hs_reward_program* pred) {
  if (pred && pred->info.n_outputs > 0)
    return fail(std::string(who) + ": the program has " + std::to_string(pred->info.n_outputs) +
                " outputs; a termination predicate has none (it is read as one truth value)");
  return 0;
}
}  // namespace

extern "C" {

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
  if (!rp_resident(const_cast<hs_reward_program*>(pred), b->device)) return -1;
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

static_assert(HS_TERM_FALLEN == hs::TERM_FALLEN && HS_TERM_LOST_BALANCE == hs::TERM_LOST_BALANCE, "built-in kinds");

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
  if (!b->mid_count && !uc_alloc(b->device, N * sizeof(int32_t), (void**)&b->mid_count)) {
    b->mid_count = nullptr;
    return fail("hipExtMallocWithFlags(grace hand-off counts, uncached) failed");
  }
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
  const double* const* fp = reinterpret_cast<const double* const*>(f);
  for (int k = 0; k < hs::RP_NFIELDS; k++)
    if ((pred->info.fields & (1u << k)) && !fp[k])
      return fail(std::string("hs_termination_eval_host: the predicate reads ") + kRpFieldNames[k] + ", which is NULL");
  hs::rp_termination_eval_host(pred->dims, pred->code.data(), (int)(pred->code.size() / 5), pred->consts.data(), params,
                               grace_steps, n, fp, episode, count, episode_tag, early);
  return 0;
}

int hs_pack_outputs(hs_batch* b, double* out, int ncols, int warnings, void* stream) {
  if (!b || !out) return fail("hs_pack_outputs: null argument");
  if (ncols < 0 || ncols > 7) return fail("hs_pack_outputs: ncols must be in [0, 7]");
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    hs::PackArgs<T> a{};
    a.n = b->n;
    a.obs_dim = b->obs_dim;
    a.ncols = ncols;
    a.nwarn = warnings ? HS_NWARN : 0;
    a.nwarn_stride = HS_NWARN;
    a.obs = (const T*)b->buf.obs;
    a.reward = (const T*)b->buf.reward;
    a.terminated = b->buf.terminated;
    a.truncated = b->buf.truncated;
    a.total_reward = (const T*)b->buf.total_reward;
    a.step_count = b->buf.step_count;
    a.term_step_count = b->buf.terminal_step_count;
    a.term_total_reward = (const T*)b->buf.terminal_total_reward;
    a.warning = b->buf.warning;
    a.out = out;
    return hip_rc(hs::launch_pack<T>(a, (hipStream_t)stream), "pack_kernel");
  };
  return b->precision == HS_FP64 ? run(0.0) : run(0.0f);
}

int hs_batch_counters(const hs_batch* b, uint64_t* wide_reruns) {
  if (!b || !wide_reruns) return fail("null argument");
  DeviceGuard g(b->device);
  unsigned long long v = 0;
  if (!hip_ok(hipDeviceSynchronize(), "sync") ||
      !hip_ok(hipMemcpy(&v, b->redo_total, sizeof v, hipMemcpyDeviceToHost), "counters"))
    return -1;
  *wide_reruns = v;
  return 0;
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

int hs_stream_orders(const hs_batch* b, uint64_t* n) {
  if (!b || !n) return fail("null argument");
  *n = b->stream_orders;
  return 0;
}

int hs_synchronize(hs_batch* b) {
  if (!b) return fail("null batch");
  DeviceGuard g(b->device);
  return hip_rc(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

}  // extern "C"
