// hsim C ABI implementation (product): the model, the batch with its memory and streams, the step and reset
// launches, state I/O, kinematics and rendering.  See include/hsim.h for the reference interfaces replaced;
// hs_api_fused.cpp, hs_api_reward.cpp and hs_api_ops.cpp hold the rest of the ABI.
#include <array>
#include <cmath>
#include <cstring>
#include <memory>

#include "hs_api_batch.h"
#include "hs_render.h"

static_assert(HS_KINDIM == hs::KINDIM, "include/hsim.h HS_KINDIM is the kernels' record size");
static_assert(HS_CAM_BODY == hs::CAM_BODY && HS_CAM_COM == hs::CAM_COM, "include/hsim.h camera modes");

thread_local std::string hs::g_err;

namespace {
using hs::by_precision;
using hs::DeviceGuard;
using hs::fail;
using hs::g_err;
using hs::hip_ok;
using hs::hip_rc;
using hs::order_streams;

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

// The batch's own hs_buffers rows in allocation order: each row's slot, its size in bytes, and whether an
// external batch may leave it out.  hs_batch_create, hs_batch_destroy and init_state walk this one list.
struct BufRow { void** slot; size_t bytes; bool optional; };
std::array<BufRow, 19> buffer_rows(hs_batch* b) {
  const auto& h = b->model->host;
  const size_t N = (size_t)b->n, es = hs::elem_size(b), obs = N * b->obs_dim * es;
  hs_buffers& u = b->buf;
  return {{{&u.qpos, N * h.nq * es, false}, {&u.qvel, N * h.nv * es, false}, {&u.qacc_warmstart, N * h.nv * es, false},
           {&u.ctrl, N * h.nu * es, false}, {&u.time, N * es, false}, {(void**)&u.step_count, N * 4, false},
           {(void**)&u.episode, N * 4, false}, {&u.total_reward, N * es, false},
           {(void**)&u.warning, N * HS_NWARN * 4, false}, {&u.obs, obs, false}, {&u.terminal_obs, obs, false},
           {&u.reward, N * es, false}, {(void**)&u.terminated, N, false}, {(void**)&u.truncated, N, false},
           {&u.aux, N * hs::AUXDIM * es, false}, {&u.cfrc_ext, N * h.nbody * 6 * es, true},
           {&u.subtree_linvel, N * h.nbody * 3 * es, true}, {(void**)&u.terminal_step_count, N * 4, true},
           {&u.terminal_total_reward, N * es, true}}};
}

// qpos = qpos0 in every env, every other row and the kernel-managed words zero
bool init_state(hs_batch* b) {
  const auto& m = b->model->host;
  const size_t N = (size_t)b->n;
  const bool qpos_ok = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    std::vector<T> q(N * m.nq);
    for (size_t i = 0; i < N; i++)
      for (int k = 0; k < m.nq; k++) q[i * m.nq + k] = (T)m.qpos0[k];
    return hip_ok(hipMemcpy(b->buf.qpos, q.data(), q.size() * sizeof(T), hipMemcpyHostToDevice), "init qpos");
  });
  if (!qpos_ok) return false;
  for (const BufRow& r : buffer_rows(b)) {
    if (r.slot == &b->buf.qpos || (r.optional && !*r.slot)) continue;
    if (!hip_ok(hipMemset(*r.slot, 0, r.bytes), "init")) return false;
  }
  return hip_ok(hipMemset(b->redo, 0, (N + 2) * sizeof(int)), "init") &&
         hip_ok(hipMemset(b->redo_total, 0, sizeof(unsigned long long)), "init") &&
         hip_ok(hipMemset(b->qsync, 0, hs::qsync_words((int)N) * sizeof(int)), "init") &&
         // a recycled UC block holds another batch's rows: a lost hand-off reads this row's warning
         // counters and time (hs_env_step.h step_pair), so they start at 0, not at stale bits
         hip_ok(hipMemset(b->mid, 0, N * hs::MIDDIM * hs::elem_size(b)), "init");
}

// the waves of the batch's resident step kernel the device holds at once (<= 0: unknown)
int resident_waves_of(const hs_batch* b) {
  const bool pgs = b->model->host.solver == 1;
  return by_precision(b->precision, [&](auto zero) { return hs::resident_waves<decltype(zero)>(pgs); });
}

// the schedule plan (hs_schedule.h) of an env step of `nsub` substeps, or of a tape launch of n_steps > 1 of them,
// as launch_step will make it for the batch as configured
hs::SchedulePlan plan_of(const hs_batch* b, int nsub, int n_steps) {
  return hs::schedule_plan(b->cfg.schedule, hs::MODE_ENV_STEP, nsub, n_steps, false, b->n, resident_waves_of(b),
                           b->mid && b->qsync, b->lose_env1);
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

// f(compiled model) for the precision's DevModel built on the host (no device involved)
template <typename T, typename F>
int with_dev_model(const hs_model* m, F&& f) {
  auto d = std::make_unique<hs::DevModel<T>>();
  std::string err;
  if (!hs::build_dev_model<T>(m->host, *d, err)) return fail(err);
  return f(*d);
}

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
}  // namespace

namespace hs {

// a block of the pool, or a new one; on failure *out is null and the error names `what`
bool uc_alloc(int device, size_t bytes, void** out, const char* what) {
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
  if (hipExtMallocWithFlags(out, cls, hipDeviceMallocUncached) == hipSuccess) return true;
  *out = nullptr;
  g_err = std::string("hipExtMallocWithFlags(") + what + ", uncached) failed";
  return false;
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

int launch(hs_batch* b, int mode, const float* act, const uint8_t* mask, const void* nq, const void* nvz, int nsub,
           void* stream, const LaunchExtra& x) {
  if (!b) return fail("null batch");
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  // a tape launch of a batch with a fused-capable termination condition: the TERM instances (the entry points
  // have refused every other tape launch of a batch with a condition)
  const bool term = mode == MODE_ENV_STEP && b->term_prog && b->term_kind != 0 && (x.nsteps > 1 || x.fused.ro.obs);
  if (term && b->precision != HS_FP64)
    return fail("a fused launch with a termination condition runs on the fp64 Newton engine");
  // (the rollout, evaluation, norm and termination parts are absent on the fp32 engine: their entry points ask
  // for fp64)
  const hipError_t e = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    StepLaunch<T> s{(const DevModel<T>*)b->dmodel, b->model->host.nv, env_buffers<T>(b), act, mask, (const T*)nq,
                    (const T*)nvz, params_of(b, mode, nsub), b->n};
    s.p.nsteps = x.nsteps;
    if (const hs_tape_out* t = x.tape) s.tape = {(T*)t->obs, (T*)t->reward, t->terminated, t->truncated};
    s.fused = x.fused;
    if (term)
      s.tm = {b->term_kind, b->grace_steps, b->term_min_height, b->term_max_roll_pitch, b->grace_count,
              b->grace_episode, b->early, b->mid_count};
    s.in = {(const T*)b->init_q, (const T*)b->init_v, b->init_n};   // (hs_set_initial_states)
    return launch_step<T>(s, (hipStream_t)stream);
  });
  if (e == hipErrorInvalidValue) return fail("no kernel instance for this model's nv (compiled: nv = 27)");
  return hip_rc(e, "step kernel launch");
}

// the env step's one launch, as the batch's config has it
int step_launch(hs_batch* b, const float* actions, void* stream) {
  int rc = launch(b, MODE_ENV_STEP, actions, nullptr, b->ar_qpos_noise, b->ar_qvel_noise, b->cfg.frame_skip, stream);
  if (rc == 0) env_step_committed(b);
  return rc;
}

}  // namespace hs

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
  return by_precision(precision, [&](auto zero) { return with_dev_model<decltype(zero)>(m, copy); });
}

int hs_lane_layout(int precision, int i, char* name, int namesz, int* offset, int* count, int* kind) {
  if (precision != HS_FP32 && precision != HS_FP64) return fail("hs_lane_layout: bad precision");
  const hs::LaneEntry* e = nullptr;
  const int n = by_precision(precision, [&](auto zero) { return hs::lane_layout<decltype(zero)>(&e); });
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
  return by_precision(precision, [&](auto zero) { return with_dev_model<decltype(zero)>(m, get); });
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
  bool ok = by_precision(precision, [&](auto zero) { return upload_model<decltype(zero)>(b, err); });
  if (!ok) { g_err = err; delete b; return nullptr; }
  size_t es = hs::elem_size(b), N = (size_t)n_envs;
  if (external) {
    b->buf = *external;
    b->owns = false;
  } else {
    b->owns = true;
    for (const BufRow& r : buffer_rows(b))
      if (!hip_ok(hipMalloc(r.slot, r.bytes > 0 ? r.bytes : 4), "hipMalloc")) { hs_batch_destroy(b); return nullptr; }
  }
  if (!hip_ok(hipMalloc(&b->dbg, hs::DBGDIM * 8), "hipMalloc(dbg)") ||
      !hip_ok(hipMalloc((void**)&b->redo, (N + 2) * sizeof(int)), "hipMalloc(redo)") ||
      !hip_ok(hipMalloc((void**)&b->redo_total, sizeof(unsigned long long)), "hipMalloc(redo_total)") ||
      !hip_ok(hipMalloc((void**)&b->prog_done, N), "hipMalloc(prog_done)") ||
      // chunk-queue hand-off rows, claim counters and pair flags: UNCACHED device memory from the UC
      // pool above, so a hand-off between waves on different CUs / XCDs needs no L2 write-back or
      // invalidate (hs_env_step.h step_pair)
      !hs::uc_alloc(device, N * hs::MIDDIM * es, &b->mid, "mid") ||
      !hs::uc_alloc(device, hs::qsync_words((int)N) * sizeof(int), (void**)&b->qsync, "qsync")) {
    hs_batch_destroy(b);
    return nullptr;
  }
  if (!init_state(b)) { hs_batch_destroy(b); return nullptr; }
  return b;
}

void hs_batch_destroy(hs_batch* b) {
  if (!b) return;
  DeviceGuard g(b->device);
  if (b->owns)
    for (const BufRow& r : buffer_rows(b))
      if (*r.slot) (void)hipFree(*r.slot);
  for (void* p : {b->dmodel, b->dbg, (void*)b->redo, (void*)b->redo_total, (void*)b->prog_done, (void*)b->grace_count,
                  (void*)b->grace_episode, (void*)b->early, b->tape_backup, (void*)b->kin_envs, b->init_q, b->init_v,
                  b->ref_q, b->ref_v})
    if (p) (void)hipFree(p);
  for (void* p : b->init_retired) (void)hipFree(p);
  for (void* p : b->ref_retired) (void)hipFree(p);
  hs::uc_release(b->device, (size_t)b->n * sizeof(int32_t), b->mid_count);
  if (b->mid) hs::uc_release(b->device, (size_t)b->n * hs::MIDDIM * hs::elem_size(b), b->mid);
  if (b->qsync) hs::uc_release(b->device, hs::qsync_words(b->n) * sizeof(int), b->qsync);
  if (b->eval_obs) hs::uc_release(b->device, (size_t)b->n * b->obs_dim * sizeof(float), b->eval_obs);
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
  out->elem_size = (int)hs::elem_size(b);
  out->resident_con = b->precision == HS_FP64 ? hs::MAXCON_F64 : hs::MAXCON;
  out->resident_efc = b->precision == HS_FP64 ? hs::MAXEFC_F64 : hs::MAXEFC;
  out->wide_con = hs::MAXCON_WIDE;
  out->wide_efc = hs::MAXEFC_WIDE;
  const hs::ContactBound cb = hs::contact_bound(h);
  out->bound_con_all = cb.con_all;
  out->bound_efc_all = cb.efc_all;
  out->bound_con_floor = cb.con_floor;
  out->bound_efc_floor = cb.efc_floor;
  DeviceGuard g(b->device);
  out->resident_waves = resident_waves_of(b);
  return 0;
}

int hs_batch_schedule(const hs_batch* b, int nsub, int n_steps, int* queue, int* single) {
  if (!b || !queue || !single) return fail("null argument");
  DeviceGuard g(b->device);
  const hs::SchedulePlan plan = plan_of(b, nsub, n_steps);
  if (!plan.valid) return fail("hs_batch_schedule: the batch cannot run a tape launch of n_steps steps");
  *queue = plan.queue;
  *single = plan.single;
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
  int rc = hs::launch(b, hs::MODE_RESET, nullptr, mask, qpos_noise, qvel_noise, 1, stream);
  if (rc == 0 && !mask) b->ctrl_stale = false;     // every env's data.ctrl is 0 again (mj_resetData)
  return rc;
}

int hs_step(hs_batch* b, const float* actions, void* stream) {
  if (!actions) return fail("hs_step: actions must not be NULL");
  if (!b) return fail("null batch");
  // a termination condition: step, outcome launch, masked reset.  Without a device reward the reward is the
  // caller's, and so is the outcome that follows it (hs_apply_termination): the step alone
  if (b->term_prog && b->cfg.reward_id != HS_REWARD_NONE) return hs::step_outcome_reset(b, actions, nullptr, nullptr, stream);
  return hs::step_launch(b, actions, stream);
}

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
  // the queue's unit: a tape launch's (a small batch only ever queues tape launches, by env)
  const hs::SchedulePlan plan = plan_of(b, b->cfg.frame_skip, 2);
  if (!plan.valid) return 0;
  const int nunits = plan.units;
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

int hs_set_initial_states(hs_batch* b, int n_states, const double* qpos, const double* qvel) {
  const std::string who = "hs_set_initial_states";
  if (!b) return fail(who + ": null batch");
  if (n_states < 0 || n_states > HS_MAX_INITIAL_STATES)
    return fail(who + ": n_states " + std::to_string(n_states) + " must lie in [0, HS_MAX_INITIAL_STATES = " +
                std::to_string(HS_MAX_INITIAL_STATES) + "]");
  if (n_states == 0) {   // unbind: the blocks stay for the next bind
    b->init_n = 0;
    return 0;
  }
  if (!qpos) return fail(who + ": qpos must not be NULL with n_states > 0");
  const auto& h = b->model->host;
  const size_t K = (size_t)n_states, nq = (size_t)h.nq, nv = (size_t)h.nv;
  std::vector<double> q(qpos, qpos + K * nq), v(K * nv, 0.0);
  if (qvel) v.assign(qvel, qvel + K * nv);
  for (size_t i = 0; i < q.size(); i++)
    if (!std::isfinite(q[i]))
      return fail(who + ": qpos[" + std::to_string(i / nq) + "][" + std::to_string(i % nq) + "] is not finite");
  for (size_t i = 0; i < v.size(); i++)
    if (!std::isfinite(v[i]))
      return fail(who + ": qvel[" + std::to_string(i / nv) + "][" + std::to_string(i % nv) + "] is not finite");
  // the free joint's quaternion, normalised as mj_normalizeQuat would at the first mj_step; a zero one has no
  // direction to keep
  if (h.njnt > 0 && h.jnt_type[0] == hs::JNT_FREE && nq >= 7)
    for (size_t j = 0; j < K; j++) {
      double* r = q.data() + j * nq;
      const double norm = std::sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]);
      if (!(norm >= 1e-15)) return fail(who + ": row " + std::to_string(j) + " has a zero free-joint quaternion");
      for (int c = 3; c < 7; c++) r[c] /= norm;
    }
  DeviceGuard g(b->device);
  // after the batch's pending launches, whatever stream they are on (they may read the rows written below)
  if (!hip_ok(hipDeviceSynchronize(), "hs_set_initial_states")) return -1;
  const size_t es = hs::elem_size(b);
  if (n_states > b->init_cap) {
    void *nq_blk = nullptr, *nv_blk = nullptr;
    const int cap = std::min(HS_MAX_INITIAL_STATES, std::max(n_states, 2 * b->init_cap));
    if (!hip_ok(hipMalloc(&nq_blk, (size_t)cap * nq * es), "hipMalloc(initial states)") ||
        !hip_ok(hipMalloc(&nv_blk, (size_t)cap * nv * es), "hipMalloc(initial states)")) {
      if (nq_blk) (void)hipFree(nq_blk);
      return -1;
    }
    if (b->init_q) b->init_retired.push_back(b->init_q);
    if (b->init_v) b->init_retired.push_back(b->init_v);
    b->init_n = 0;
    b->init_q = nq_blk;
    b->init_v = nv_blk;
    b->init_cap = cap;
  }
  const bool ok = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    const std::vector<T> tq(q.begin(), q.end()), tv(v.begin(), v.end());
    return hip_ok(hipMemcpy(b->init_q, tq.data(), tq.size() * sizeof(T), hipMemcpyHostToDevice), "initial states qpos") &&
           hip_ok(hipMemcpy(b->init_v, tv.data(), tv.size() * sizeof(T), hipMemcpyHostToDevice), "initial states qvel");
  });
  if (!ok) {
    b->init_n = 0;
    return -1;
  }
  b->init_n = n_states;
  return 0;
}

int hs_get_initial_states(const hs_batch* b, int* n_states) {
  if (!b || !n_states) return fail("hs_get_initial_states: null argument");
  *n_states = b->init_n;
  return 0;
}

int hs_physics_step(hs_batch* b, const float* ctrl, int nsub, void* stream) {
  if (nsub < 1) return fail("nsub must be >= 1");
  if (!b) return fail("null batch");
  if (!ctrl && b->ctrl_stale)
    return fail("hs_physics_step: ctrl == NULL keeps data.ctrl, but env steps ran with HS_OUT_CTRL off so the "
                "ctrl buffer is stale; pass ctrl, set it with hs_state_io, or enable HS_OUT_CTRL");
  int rc = hs::launch(b, hs::MODE_PHYSICS, ctrl, nullptr, nullptr, nullptr, nsub, stream);
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
  int rc = by_precision(b->precision, [&](auto zero) {
    return state_io<decltype(zero)>(b, dir, qpos, qvel, qacc_warmstart, time, ctrl);
  });
  if (rc == 0 && dir == 1 && ctrl) b->ctrl_stale = false;   // only once the new ctrl is on the device
  return rc;
}

int hs_kinematics(hs_batch* b, int env, const double* qpos, double* xpos, double* xmat, double* geom_xpos,
                  double* geom_zaxis, double* com) {
  if (!b) return fail("null batch");
  if (env < 0 || env >= b->n) return fail("env index out of range");
  DeviceGuard g(b->device);
  if (!hip_ok(hipDeviceSynchronize(), "sync")) return -1;
  return by_precision(b->precision, [&](auto zero) {
    return kinematics_io<decltype(zero)>(b, env, qpos, xpos, xmat, geom_xpos, geom_zaxis, com);
  });
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
  const hipError_t e = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    return hs::launch_kinematics_batch<T>((const hs::DevModel<T>*)b->dmodel, nv, n, (const T*)qpos_dev,
                                          (const T*)b->buf.qpos, de, (T*)kin_dev, st);
  });
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
  const hipError_t e = by_precision(b->precision, [&](auto zero) {
    using T = decltype(zero);
    return hs::launch_render<T>((const T*)kin_dev, n, sc, rc, H, W, rgb_dev, st);
  });
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

int hs_pack_outputs(hs_batch* b, double* out, int ncols, int warnings, void* stream) {
  if (!b || !out) return fail("hs_pack_outputs: null argument");
  if (ncols < 0 || ncols > 7) return fail("hs_pack_outputs: ncols must be in [0, 7]");
  DeviceGuard g(b->device);
  if (order_streams(b, (hipStream_t)stream)) return -1;
  return by_precision(b->precision, [&](auto zero) -> int {
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
  });
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
