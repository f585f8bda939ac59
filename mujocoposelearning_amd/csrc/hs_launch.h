// The host side of hs_kernels.hip, included at its end: the wave-count caches, the chunk queue's instance
// dispatch, launch_step and the launchers of the kinematics, reward-evaluation and pack kernels.
#pragma once

namespace hs {

template <typename T>
hipError_t launch_pack(const PackArgs<T>& a, hipStream_t stream) {
  const size_t total = (size_t)a.n * (a.obs_dim + a.ncols + a.nwarn);
  if (total == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL((pack_kernel<T>), dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_reward_eval(const RewardEvalArgs<T>& a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (a.nv < 6 || a.nv > HL || a.nu < 0 || a.nu > HL || a.nbody < 2 || a.nq < 7) return hipErrorInvalidValue;
  const long long threads = (long long)a.n * HL;
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  hipLaunchKernelGGL((reward_eval_kernel<T>), dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// waves of a one-wave-per-block kernel the current device holds at once (occupancy x CUs; 0 if unknown),
// cached per device in the caller's `cache` (0: not yet computed; a racing first call computes the same value
// twice: benign)
constexpr int MAXDEV = 64;
template <typename K>
int waves_held(int (&cache)[MAXDEV], K kernel) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  int* c = dev < MAXDEV ? &cache[dev] : nullptr;
  if (c && *c != 0) return *c > 0 ? *c : 0;
  int per_cu = 0, v = -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WAVE, 0) == hipSuccess && per_cu > 0)
    v = per_cu * prop.multiProcessorCount;
  if (c) *c = v;
  return v > 0 ? v : 0;
}

// waves of the resident step-kernel instance the current device holds at once
template <typename T>
int resident_waves(bool pgs) {
  static int cache[2][MAXDEV] = {};
  return pgs ? waves_held(cache[1], step_kernel<T, 27, true>) : waves_held(cache[0], step_kernel<T, 27, false>);
}

// The chunk-queue instance of a QueueInstance word (hs_kernels.h)
template <typename T, unsigned I>
constexpr auto queue_kernel = step_kernel_queue<T, 27, (I & QI_PGS) != 0, (I & QI_ROLL) != 0, (I & QI_EVAL) != 0,
                                                (I & QI_NORM) != 0, (I & QI_TERM) != 0>;

// waves of a chunk-queue instance the current device holds at once.  The queue's grid must not exceed it: a
// wave's first item is item blockIdx.x, taken without a claim (step_kernel_queue), so every wave of the grid has
// to be running from the start.  It is below resident_waves() where the queue instance's occupancy is below the
// direct kernel's (the fp32 Newton engine: 1 wave per SIMD against 2).
template <typename T, unsigned I>
int queue_waves() {
  static int cache[MAXDEV] = {};
  return waves_held(cache, queue_kernel<T, I>);
}

// The kernels' argument block of a request
template <typename T>
KArgs<T> kernel_args(const StepLaunch<T>& s) {
  return {(MPtr<T>)s.model, s.b, s.actions, s.reset_mask, s.noise_qpos, s.noise_qvel, s.p, s.nenv,
          s.tape, s.fused.ro, s.fused.ev, s.fused.nm, s.tm, s.in};
}

// One queued launch: the instance `instance` names among I..., the instances the caller's pass over
// hs_kernels.hip compiles (in the order they take in its code object), its grid capped at the waves the instance
// holds.  An instance that does not exist (the fp32 engine's fused rollout, ...) is refused here.
template <unsigned... I>
struct QueueInstances {};
template <typename T, unsigned... I>
hipError_t launch_queue(QueueInstances<I...>, const KArgs<T>& args, unsigned instance, unsigned max_grid,
                        hipStream_t stream) {
  hipError_t rc = hipErrorInvalidValue;
  auto go = [&](auto inst) {
    constexpr unsigned J = decltype(inst)::value;
    if (const int held = queue_waves<T, J>(); held > 0) {
      hipLaunchKernelGGL((queue_kernel<T, J>), dim3(std::min(max_grid, (unsigned)held)), dim3(WAVE), 0, stream, args);
      rc = hipGetLastError();
    }
  };
  (void)(... || (instance == I && (go(std::integral_constant<unsigned, I>{}), true)));
  return rc;
}

template <typename T>
hipError_t launch_step(const StepLaunch<T>& req, hipStream_t stream) {
  if (req.nenv <= 0) return hipSuccess;
  if (req.nv != 27) return hipErrorInvalidValue;
  StepLaunch<T> s = req;   // (s.p takes the schedule plan)
  StepParams& p = s.p;
  const FusedArgs& f = s.fused;
  const bool pgs = p.solver == SOLVER_PGS;
  const bool ro = f.ro.obs != nullptr, ev = f.ev.episode0 != nullptr, nm = f.nm.mean != nullptr, tm = s.tm.kind != 0;
  if (s.in.K < 0 || (s.in.K > 0 && (!s.in.q || !s.in.v))) return hipErrorInvalidValue;
  if (nm && (!ro || !f.nm.inv_std || !(f.nm.clip > 0.f))) return hipErrorInvalidValue;
  // fused rollouts: the fp64 Newton engine
  if (ro && (sizeof(T) != 8 || pgs)) return hipErrorInvalidValue;
  // fused evaluation: a rollout launch (the policy, ro.obs = the staging rows) with result slots
  if (ev && (!ro || f.ev.max_episodes < 1 || f.ev.n_trace < 0 || f.ev.n_trace > s.nenv)) return hipErrorInvalidValue;
  // a built-in termination condition: tape launches of the fp64 Newton engine with auto-reset (an early end
  // resets inside the launch)
  if (tm && (sizeof(T) != 8 || pgs || p.mode != MODE_ENV_STEP || !p.autoreset ||
             (s.tm.kind != TERM_FALLEN && s.tm.kind != TERM_LOST_BALANCE) || s.tm.grace_steps < 1 ||
             !s.tm.grace_count || !s.tm.grace_episode || !s.tm.early || !s.tm.mid_count || !(p.nsteps > 1 || ro)))
    return hipErrorInvalidValue;
  const SchedulePlan plan = schedule_plan(p.schedule, p.mode, p.nsub, p.nsteps, ro, s.nenv, resident_waves<T>(pgs),
                                          s.b.mid && s.b.qsync, p.dbg_lose_pair1);
  if (!plan.valid) return hipErrorInvalidValue;
  p.nsteps = plan.nsteps;
  p.queue = plan.queue;
  p.single = plan.single;
  p.qorder = plan.qorder;
  p.qmul = plan.qmul;
  p.dbg_lose_pair1 = plan.dbg_lose_pair1;
  const unsigned instance = (pgs ? QI_PGS : 0u) | (ro ? QI_ROLL : 0u) | (ev ? QI_EVAL : 0u) | (nm ? QI_NORM : 0u) |
                            (tm ? QI_TERM : 0u);
  const KArgs<T> args = kernel_args(s);
  const dim3 grid(plan.grid), wgrid(plan.wide_grid), block(WAVE);
  // the fused instances (tape launches: the chunk queue alone, no wide tier): the TERM and NORM ones live in
  // objects of their own, the rollout and the evaluation here
  if constexpr (sizeof(T) == 8) {
    if (tm) return launch_queue_term(s, instance, grid.x, stream);
    if (nm) return launch_queue_norm(s, instance, grid.x, stream);
    if (ro) return launch_queue(QueueInstances<QI_ROLL | QI_EVAL, QI_ROLL>{}, args, instance, grid.x, stream);
  }
  // one solver's launches: the resident tier (chunk-queue or direct schedule), then the wide tier's re-run of the
  // envs it deferred (a generic lambda, not a function template: the kernel instances then keep their order in
  // the code object)
  auto tiers = [&](auto solver) -> hipError_t {
    constexpr unsigned S = decltype(solver)::value;
    if (plan.queue) {
      const hipError_t rc = launch_queue(QueueInstances<S>{}, args, instance, grid.x, stream);
      if (rc != hipSuccess) return rc;
    } else {
      hipLaunchKernelGGL((step_kernel<T, 27, S != 0>), grid, block, 0, stream, args);
    }
    if (s.b.redo && plan.wide) hipLaunchKernelGGL((step_kernel_wide<T, 27, S != 0>), wgrid, block, 0, stream, args);
    return hipGetLastError();
  };
  return pgs ? tiers(std::integral_constant<unsigned, QI_PGS>{}) : tiers(std::integral_constant<unsigned, 0u>{});
}

template <typename T>
hipError_t launch_kinematics(const DevModel<T>* dmodel, int nv, const T* qpos, T* out, hipStream_t stream) {
  if (nv != 27) return hipErrorInvalidValue;
  hipLaunchKernelGGL((kin_kernel<T, 27>), dim3(1), dim3(WAVE), 0, stream, (MPtr<T>)dmodel, qpos, out);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_kinematics_batch(const DevModel<T>* dmodel, int nv, int n, const T* qpos, const T* state_qpos,
                                   const int* envs, T* out, hipStream_t stream) {
  if (nv != 27 || n < 1 || (envs ? !state_qpos : !qpos)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((kin_batch_kernel<T, 27>), dim3((unsigned)n), dim3(WAVE), 0, stream, (MPtr<T>)dmodel, qpos,
                     state_qpos, envs, out);
  return hipGetLastError();
}

}  // namespace hs
