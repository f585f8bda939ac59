// hsim step kernel for gfx950 (MI355X).  PRODUCT CODE.
//
// Replaces, for a whole batch of envs at once:
//   custom_env.py:152-230  HumanoidEnv.step   (frame_skip x {ctrl = a; mj_step}, obs, reward, done)
//   custom_env.py:97-150   HumanoidEnv.reset  (mj_resetData, noise, one ctrl=0 mj_step, obs)
//   custom_env.py:232-261  _get_state         (352-dim obs, stale derived fields)
//   reward_functions.py:66-261 stand / kneeling / walk rewards (device plug-ins)
//   SB3 SubprocVecEnv auto-reset semantics (train_sb3.py:203)
// and MuJoCo 3.2.5's mj_step pipeline (custom_env.py:121,160): kinematics, com, collision, CRB,
// RNE, actuation, constraint assembly, primal Newton solver (pyramidal cones; MuJoCo's default) or,
// in the <option solver="PGS"> instance, projected Gauss-Seidel on the dual, Euler with implicit
// joint damping.
//
// Execution model: TWO ENVS PER WAVEFRONT.  Lanes 0-31 step env 2w, lanes 32-63 env 2w+1; a
// half-wave maps its 32 lanes to bodies / dofs / geoms / joints / contacts / constraint rows
// stage by stage (humanoid: 17 bodies, 27 dofs, <= 32 contacts), so a wave64 instruction does
// useful work for both envs.  Per-env state lives in LDS (phase-local arrays aliased in a union
// so one wave = 2 envs fits 20 KB: all 4096 envs of configs[1] are resident at once).  Dense
// nv x nv matrices (M, the Newton Hessian, M + h*B) live row-per-lane in VGPRs and are factored
// with per-half v_readlane broadcasts.  The contact part of the Newton Hessian uses the
// tree-structured form H_ij += jp_j' U jp_i (O(nv * ncon), no nefc x nv Jacobian in memory).
// HBM traffic is only the per-env state in/out; the model is read through L1/L2, and its per-lane
// constants, in the fp64 resident-tier instances, from an LDS copy made once per launch (hs_lanes.h).
//
// Source map (private headers, included in definition order):
//   hs_lanes.h        capacity tiers, fences, DPP / half-wave primitives, KArgs, small algebra
//   hs_dense.h        row-per-lane Cholesky / L D L' and triangular solves
//   hs_scratch.h      per-env LDS layouts (Scratch, PgsCache)
//   hs_contacts.h     narrow phase, impedance, J x / J' f, contact aggregates
//   hs_phase_clock.h  per-phase stamps of the HS_TIMING build
//   hs_stepper.h      Stepper: one mj_step, phase by phase
//   hs_reward.h       the reward plug-ins' inputs and formulas, numpy's summation order
//   hs_policy.h       the fused rollout's / evaluation's policy forward (pi net on a wave's two envs)
//   hs_env_step.h     reset, obs, commit, step_pair and its phases (load, outcome, hand-off, next action)
//   this file         the __global__ kernels and, at its end, the explicit instantiations
//   hs_launch.h       the host launchers (included after the kernels): wave counts, queue-instance dispatch,
//                     launch_step
//   hs_schedule.h     the schedule plan launch_step follows (plain C++, no device code; through hs_kernels.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "hs_env_step.h"
#include "hs_kernels.h"
#include "hs_model.h"

namespace hs {
namespace {

// Resident tier: one wave per env pair, all pairs of the batch in one grid.
// 2 waves/SIMD (the VGPR budget of 256) for the fp32 engine; the fp64 parity engine needs more
// registers and runs at 1.  PGS: the <option solver="PGS"> instance (its own LDS cache).
template <typename T, int NV, bool PGS>
__global__ __launch_bounds__(64, (sizeof(T) == 4 && !PGS) ? 2 : 1) void step_kernel(KArgs<T> /* read via kernarg ptr */) {
  __shared__ Scratch<T, Resident<T>> smem[2];
  PgsCache<T, Resident<T>>* pcache = nullptr;
  if constexpr (PGS) {
    __shared__ PgsCache<T, Resident<T>> pgs_smem[2];
    pcache = &pgs_smem[threadIdx.x >= HL ? 1 : 0];
  }
  const KPtr<T> ka = (KPtr<T>)__builtin_amdgcn_kernarg_segment_ptr();
  const bool up = threadIdx.x >= HL;
  // single-env schedule (small batches, p.single): env blockIdx.x on the lower half, its mirror on
  // the upper half (same data, so the same control flow), one env per wave
  const bool single = ka->p.single != 0;
  if constexpr (Resident<T>::LANES) load_lane_table<T>(ka->m);
  step_pair<T, NV, PGS, Resident<T>>(ka, smem, pcache, single ? (int)blockIdx.x : 2 * blockIdx.x + (up ? 1 : 0),
                                     ka->nenv, nullptr, 0, ka->p.nsub, blockIdx.x, single && up);
}

// Resident tier, chunk-queue schedule (launch_step picks it when the env pairs outnumber the waves
// the GPU holds at once -- the fp64 engine at 1 wave per SIMD -- for multi-substep calls).  A
// persistent grid claims items from one counter: first every pair's substeps [0, nsub - 1), then
// every pair's last substep (+ obs / reward / auto-reset), so the launch ends on short items
// instead of a second generation of whole env steps.  Pairs are taken heaviest
// first by the durations the previous queued launch measured (QNB cost buckets, hs_kernels.h), so
// the launch ends on the cheapest last substeps, and ahead of them all the pairs with an env that
// auto-resets in this step (known since the previous step's commit; their last item runs the reset's
// mj_step too); the batch's first queued launch uses a fixed multiplicative permutation (p.qmul).
// The order only decides which wave runs which pair when: results are bitwise the same in any
// order.  Items are claimed only by running waves -- a wave's first item, item blockIdx.x, is its
// own from the start, and the grid is no larger than the waves the GPU holds at once -- and a
// last-substep item waits only on its own pair's first chunk, claimed npairs items earlier by a
// running wave: the launch cannot deadlock.  (Should other work keep part of the grid from starting,
// a wave may wait for the first chunk of a wave that has not started; the wait is bounded as ever.)
// ROLL: the fused-rollout instance (fp64 Newton engine; launch_step picks it for hs_rollout), so the
// policy forward's code and registers stay out of the per-step kernel
// EVAL (with ROLL): the fused-evaluation instance (hs_evaluate): the rollout's loop without the RolloutBuffer
// rows, a kernel of its own so that the rollout instance keeps its code and registers
// NORM (with ROLL): the instances whose policy normalises its obs on load (hs_rollout_norm,
// hs_evaluate_norm; KArgs::nm), kernels of their own so that every other instance keeps its code and registers
// TERM: the instances that evaluate a built-in termination condition after every env step (KArgs::tm,
// hs_set_termination_builtin): the tape, the rollout and the evaluation, kernels of their own likewise
template <typename T, int NV, bool PGS, bool ROLL = false, bool EVAL = false, bool NORM = false, bool TERM = false>
__global__ __launch_bounds__(64, 1) void step_kernel_queue(KArgs<T> /* read via kernarg ptr */) {
  const KPtr<T> ka = (KPtr<T>)__builtin_amdgcn_kernarg_segment_ptr();
  // this launch's epoch (its hand-off tags are qtag(epoch, ...)): the epoch only changes after every
  // wave of the launch has left the claim loop (last wave out, below)
  const uint32_t epoch = __builtin_amdgcn_readfirstlane(
      __hip_atomic_load(ka->b.qsync + QS_EPOCH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __shared__ Scratch<T, Resident<T>> smem[2];
  PgsCache<T, Resident<T>>* pcache = nullptr;
  if constexpr (PGS) {
    __shared__ PgsCache<T, Resident<T>> pgs_smem[2];
    pcache = &pgs_smem[threadIdx.x >= HL ? 1 : 0];
  }
  // claim order: prefix sums of the previous launch's bucket counts (qpre[QNB] == nunits: valid).
  // A unit is an env pair, or one env (upper half-wave a ghost) in the single-env mode of small
  // batches (p.single: every env gets a wave of its own)
  __shared__ int qpre[QNB + 1];
  {
    const int nunits = ka->p.single ? ka->nenv : (ka->nenv + 1) / 2, lane = threadIdx.x;
    int c = (ka->p.qorder && lane < QNB) ? ka->b.qsync[qs_cnt(nunits, epoch & 1) + lane] : 0;
#pragma unroll
    for (int d = 1; d < QNB; d <<= 1) {
      const int y = __shfl_up(c, d);
      if (lane >= d) c += y;
    }
    if (lane < QNB) qpre[lane + 1] = c;
    if (lane == 0) qpre[0] = 0;
    WSYNC();
  }
  // The wave's held claim: the index of the item it runs next, or -1 (one LDS word, so nothing is
  // kept in registers across an item).  Items [0, gridDim.x) are never claimed from the counter:
  // item blockIdx.x is this wave's first, held from the start, so a launch does not open with one
  // returning atomic per wave on the same word (1024 of them: the last is served ~11 us in).  Later
  // claims are gridDim.x + the counter's value.  A held first item counts as claimed by a running
  // wave only if its wave runs: launch_step never makes the grid larger than the waves this
  // instance holds at once (queue_waves).  A wave whose first item lies past the end (a launch with
  // fewer items than waves) leaves like one whose claim does.
  __shared__ int qheld;
  if (threadIdx.x == 0) qheld = (int)blockIdx.x;
  // the model's lane table: one LDS copy per launch serves every item of the wave (hs_lanes.h)
  if constexpr (Resident<T>::LANES) load_lane_table<T>(ka->m);
  WSYNC();
  for (;;) {
    const KPtr<T> k = opaque(ka);       // nothing uniform kept live across items
    const bool single = k->p.single != 0;
    const int nsub = k->p.nsub, npairs = single ? k->nenv : (k->nenv + 1) / 2, K = k->p.nsteps;   // (units)
    int* qs = k->b.qsync;
    int i = __builtin_amdgcn_readfirstlane(qheld);
    WSYNC();
    if (i < 0) {
      if (threadIdx.x == 0) i = (int)gridDim.x + atomicAdd(&qs[QS_HEAD], 1);
      i = __builtin_amdgcn_readfirstlane(i);
    } else if (threadIdx.x == 0) {
      qheld = -1;   // consumed: a wave holds at most one claim
    }
    WSYNC();
    // tape launch: K whole env steps per pair, step-major (step t of every pair, then step t + 1);
    // one env step: every pair's first chunk, then every pair's last substep
    const bool tape = K > 1 || k->ro.obs != nullptr;   // (a fused rollout is a tape launch even for K = 1)
    if (i >= (tape ? K * npairs : 2 * npairs)) break;
    if (tape) {   // an aborted tape launch only drains its claims
      int ab = 0;
      if (threadIdx.x == 0) ab = __hip_atomic_load(qs + QS_ABORT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__builtin_amdgcn_readfirstlane(ab) != 0) continue;
    }
    const int t = tape ? i / npairs : 0;
    const bool last = !tape && i >= npairs;
    const int ii = tape ? i - t * npairs : (last ? i - npairs : i);
    int pair;
    if (qpre[QNB] == npairs) {   // bucket b holds claims [qpre[b], qpre[b + 1])
      const int lane = opaque_v(threadIdx.x);
      const bool hit = lane < QNB && qpre[lane] <= ii && ii < qpre[lane + 1];
      const int b = __builtin_ctzll(__ballot(hit) | (1ull << (QNB - 1)));
      int p = 0;
      if (lane == 0) p = qs[qs_ord(npairs, epoch & 1) + (size_t)b * npairs + (ii - qpre[b])];
      pair = min(max(__builtin_amdgcn_readfirstlane(p), 0), npairs - 1);
    } else {
      pair = (int)((uint64_t)ii * (uint32_t)k->p.qmul % (uint32_t)npairs);
    }
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const bool upper = opaque_v(threadIdx.x) >= HL;
    const int env = single ? pair : 2 * pair + (upper ? 1 : 0);
    // ONE step_pair call site (the whole pipeline is inlined): a tape item is env step t, waiting for
    // the pair's step t - 1 and handing over to its step t + 1; otherwise the first chunk hands over
    // to the last substep
    const int s0 = last ? nsub - 1 : 0, s1 = (tape || last) ? nsub : nsub - 1;
    const int wait_tag = tape ? (t > 0 ? qtag(epoch, t - 1, 1) : 0) : (last ? qtag(epoch, 0, 0) : 0);
    const int set_tag = tape ? (t < K - 1 ? qtag(epoch, t, 1) : 0) : (last ? 0 : qtag(epoch, 0, 0));
    int hint;   // (STEP_* bits, wave-uniform)
    step_pair<T, NV, PGS, Resident<T>, ROLL, true, EVAL, NORM, TERM>(k, smem, pcache, env, k->nenv, nullptr, s0, s1,
                                                                     pair, single && upper, wait_tag, set_tag, t, tape,
                                                                     &hint);
#ifdef HS_TIMING
    // per item (indexed as step_pair's q0 stamps): its claim index within its chunk kind, and whether
    // it ran the reset pass
    if (T* dbg = opaque(ka)->b.dbg; dbg && threadIdx.x == 0 && (last ? npairs : 0) + pair < 4096)
      dbg[28672 + (last ? npairs : 0) + pair] = (T)(2 * ii + ((hint & STEP_DID_RESET) ? 1 : 0));
#endif
    // the pair's duration for the next launch's order: the first chunk's is kept in qcost (its
    // store trails the hand-off, but the last substep reads it ~100 us later; a stale value only
    // makes the order less exact, never the results different); a tape launch times the pair's
    // last env step
    const uint32_t d = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t0);
    if (threadIdx.x == 0) {
      qs = opaque(ka)->b.qsync;
      if (!last && !tape) {
        qs[qs_cost(npairs) + pair] = (int)d;
      } else if (!tape || t == K - 1) {
        const uint32_t tot = tape ? d : d + (uint32_t)qs[qs_cost(npairs) + pair];
        // bucket 0 (claimed first) is kept for the pairs step_pair flags: an env of theirs will
        // auto-reset in the next env step, so that step's last item also runs the reset's mj_step,
        // about two substeps, which no measured duration foretells; claimed late, it would end the
        // launch alone.  The rest go by duration into buckets 1 .. QNB - 1
        int b = QNB - 1 - (int)min(tot / (uint32_t)QBIN, (uint32_t)(QNB - 2));
        if (hint & STEP_WILL_RESET) b = 0;
        const int slot = atomicAdd(&qs[qs_cnt(npairs, (epoch + 1) & 1) + b], 1);
        qs[qs_ord(npairs, (epoch + 1) & 1) + (size_t)b * npairs + slot] = pair;
      }
    }
  }
  // the last wave out resets the counters, clears the bucket counts this launch read, and advances
  // the epoch for the next launch (every wave has made its final claim and read this launch's tag)
  int* qs = ka->b.qsync;
  int lastout = 0;
  if (threadIdx.x == 0) lastout = atomicAdd(&qs[QS_EXIT], 1) == (int)gridDim.x - 1;
  if (__builtin_amdgcn_readfirstlane(lastout)) {
    const int nunits = ka->p.single ? ka->nenv : (ka->nenv + 1) / 2;
    if (threadIdx.x < QNB) qs[qs_cnt(nunits, epoch & 1) + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
      qs[QS_HEAD] = 0;
      qs[QS_EXIT] = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) atomicAdd(&qs[QS_EPOCH], 1);
  }
}

// Wide tier: a small grid that strides over the envs the resident launch deferred (usually none:
// every wave reads the count and leaves), then the last wave out clears the list for the next step.
template <typename T, int NV, bool PGS>
__global__ __launch_bounds__(64, 1) void step_kernel_wide(KArgs<T> /* read via kernarg ptr */) {
  __shared__ Scratch<T, Wide> smem[2];
  PgsCache<T, Wide>* pcache = nullptr;
  if constexpr (PGS) {
    __shared__ PgsCache<T, Wide> pgs_smem[2];
    pcache = &pgs_smem[threadIdx.x >= HL ? 1 : 0];
  }
  const KPtr<T> ka = (KPtr<T>)__builtin_amdgcn_kernarg_segment_ptr();
  int* redo = ka->b.redo;
  const int count = redo[0];
  // nothing deferred (the usual case): every wave reads 0 and leaves; the list and its read counter
  // are already clear, so no fence and no atomic (32 of them on one word cost ~2 us per launch)
  if (count == 0) return;
  for (int base = 2 * blockIdx.x; base < count; base += 2 * gridDim.x)
    step_pair<T, NV, PGS, Wide>(ka, smem, pcache, base + (threadIdx.x >= HL ? 1 : 0), count, redo + 2, 0,
                                ka->p.nsub, 0);
  __threadfence();
  if (threadIdx.x == 0 && atomicAdd(&redo[1], 1) == (int)gridDim.x - 1) {   // every wave has read the list
    redo[0] = 0;
    redo[1] = 0;
  }
}

// mj_kinematics + mj_comPos of ONE state (visualisation / data view, never the step path): one
// wave, the lower half-wave computes, the upper half duplicates it.  out = [xpos MAXBODY*3]
// [xmat MAXBODY*9][geom_xpos MAXGEOM*3][geom z-axis MAXGEOM*3][subtree_com[0] 3].
template <typename T, int NV>
__global__ __launch_bounds__(64) void kin_kernel(MPtr<T> m, const T* __restrict__ qpos, T* __restrict__ out) {
  __shared__ Scratch<T, Resident<T>> smem[2];
  const int lane = threadIdx.x;
  const bool up = lane >= HL;
  const int sl = lane & (HL - 1);
  Scratch<T, Resident<T>>& s = smem[up ? 1 : 0];
  for (int k = sl; k < m->nq; k += HL) s.qpos[k] = qpos[k];
  if constexpr (Resident<T>::LANES) load_lane_table<T>(m);
  WSYNC();
  Stepper<T, NV, Resident<T>> st(m, s, lane);
  st.kinematics();
  if (up) return;
  const int nb = m->nbody, ng = m->ngeom;
  for (int k = sl; k < nb * 3; k += HL) out[k] = s.u.k.xpos[k / 3][k % 3];
  out += MAXBODY * 3;
  for (int k = sl; k < nb * 9; k += HL) out[k] = s.u.k.xmat[k / 9][k % 9];
  out += MAXBODY * 9;
  for (int k = sl; k < ng * 3; k += HL) out[k] = HS_KTAIL(s).gpos[k / 3][k % 3];
  out += MAXGEOM * 3;
  for (int k = sl; k < ng * 3; k += HL) out[k] = HS_KTAIL(s).gax[k / 3][k % 3];
  out += MAXGEOM * 3;
  if (sl < 3) out[sl] = s.com[sl];
}

// The same for n poses in one launch (the device renderer's poses, hs_kinematics_batch): one wave per
// pose, the upper half-wave duplicating the lower as in kin_kernel, so a record is kin_kernel's bit
// for bit and n odd or 1 needs no special case.  Pose i is row i of qpos[n][nq], or, with `envs`,
// row envs[i] of the batch's own state rows (state_qpos); record i goes to out[i][KINDIM].
template <typename T, int NV>
__global__ __launch_bounds__(64) void kin_batch_kernel(MPtr<T> m, const T* __restrict__ qpos,
                                                       const T* __restrict__ state_qpos,
                                                       const int* __restrict__ envs, T* __restrict__ out) {
  __shared__ Scratch<T, Resident<T>> smem[2];
  const int lane = threadIdx.x;
  const bool up = lane >= HL;
  const int sl = lane & (HL - 1);
  Scratch<T, Resident<T>>& s = smem[up ? 1 : 0];
  const size_t pose = blockIdx.x;
  const T* q = envs ? state_qpos + (size_t)envs[pose] * m->nq : qpos + pose * m->nq;
  for (int k = sl; k < m->nq; k += HL) s.qpos[k] = q[k];
  if constexpr (Resident<T>::LANES) load_lane_table<T>(m);
  WSYNC();
  Stepper<T, NV, Resident<T>> st(m, s, lane);
  st.kinematics();
  if (up) return;
  out += pose * KINDIM;
  const int nb = m->nbody, ng = m->ngeom;
  for (int k = sl; k < nb * 3; k += HL) out[k] = s.u.k.xpos[k / 3][k % 3];
  out += MAXBODY * 3;
  for (int k = sl; k < nb * 9; k += HL) out[k] = s.u.k.xmat[k / 9][k % 9];
  out += MAXBODY * 9;
  for (int k = sl; k < ng * 3; k += HL) out[k] = HS_KTAIL(s).gpos[k / 3][k % 3];
  out += MAXGEOM * 3;
  for (int k = sl; k < ng * 3; k += HL) out[k] = HS_KTAIL(s).gax[k / 3][k % 3];
  out += MAXGEOM * 3;
  if (sl < 3) out[sl] = s.com[sl];
}

// hs_reward_eval: the step kernel's reward code (np_sum_half + reward_formula) on caller-supplied
// fields, one env per 32-lane half as in the step kernel.  Not on the step path: it exists so the
// device formulas can be checked against the reference's own outputs on arbitrary states.
template <typename T>
__global__ __launch_bounds__(256) void reward_eval_kernel(RewardEvalArgs<T> a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int sl = lane & (HL - 1);
  const long long env = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / HL;
  const bool ok = env < a.n;
  const int nv = a.nv, nu = a.nu;
  const long long ldc = a.ld_com ? a.ld_com : 3, ldl = a.ld_linv ? a.ld_linv : 3, ldq = a.ld_qfrc ? a.ld_qfrc : nv;
  T e = T(0), cu = T(0);
  if (ok && sl < nv) e = a.qfrc_actuator[env * ldq + sl] * a.qvel[env * nv + sl];
  if (ok && sl < nu) cu = a.ctrl[env * nu + sl];
  const T esum = np_sum_half(e * e, 6, nv - 6, lane);   // every lane of the wave takes part
  const T csum = np_sum_half(cu * cu, 0, nu, lane);
  if (!ok || sl != 0) return;
  const T* q = a.qpos + env * a.nq;
  RewardIn<T> in;
  in.h = q[2];
  in.qw = q[3];
  in.qx = q[4];
  in.qy = q[5];
  in.qz = q[6];
  in.vx = a.qvel[env * nv];
  in.time = a.time[env];
  in.com0 = a.subtree_com0[env * ldc];
  in.com1 = a.subtree_com0[env * ldc + 1];
  {
#pragma clang fp contract(off)
    in.comv = T(0);
    for (int d = 0; d < 3; d++) in.comv += a.subtree_linvel0[env * ldl + d] * a.subtree_linvel0[env * ldl + d];
  }
  const T* cf = a.cfrc_ext + (env * a.nbody + a.nbody - 2) * 6;
  in.lf = T(0);
  in.rf = T(0);
  for (int d = 0; d < 6; d++) { in.lf += fabs(cf[d]); in.rf += fabs(cf[6 + d]); }
  in.energy = esum;
  in.ctrl_sq = csum;
  a.out[env] = reward_formula(a.reward_id, a.kneel, in);
}

// hs_pack_outputs: one step's host-bound outputs as ONE float64 buffer in one launch (the drop-in's
// single device-to-host copy): obs rows, then ncols columns of N values, then the warning rows
// (column-major: kind k of env i at k * N + i).  Grid-stride over the whole buffer: coalesced writes.
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(PackArgs<T> a) {
  const size_t nobs = (size_t)a.n * a.obs_dim, ncol = (size_t)a.ncols * a.n, nw = (size_t)a.nwarn * a.n;
  const size_t total = nobs + ncol + nw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double v;
    if (i < nobs) {
      v = (double)a.obs[i];
    } else if (i < nobs + ncol) {
      const size_t j = i - nobs;
      const int c = (int)(j / a.n);
      const size_t e = j - (size_t)c * a.n;
      switch (c) {
        case 0: v = (double)a.reward[e]; break;
        case 1: v = (double)a.terminated[e]; break;
        case 2: v = (double)a.truncated[e]; break;
        case 3: v = (double)a.total_reward[e]; break;
        case 4: v = (double)a.step_count[e]; break;
        case 5: v = a.term_step_count ? (double)a.term_step_count[e] : 0.0; break;
        default: v = a.term_total_reward ? (double)a.term_total_reward[e] : 0.0; break;
      }
    } else {
      const size_t j = i - nobs - ncol;
      const int kind = (int)(j / a.n);
      const size_t e = j - (size_t)kind * a.n;
      v = (double)a.warning[e * a.nwarn_stride + kind];
    }
    a.out[i] = v;
  }
}

}  // namespace
}  // namespace hs

#include "hs_launch.h"

namespace hs {
// The Makefile compiles this file once per precision (HS_ONLY_F32 / HS_ONLY_F64), so each engine
// gets its own code-generation flags (the fp64 one without MachineLICM), and once more
// (HS_ONLY_NORM, the fp64 flags) for the two fused instances whose policy normalises its obs
// (hs_rollout_norm, hs_evaluate_norm): in a code object of their own they leave the engines' code objects,
// kernel for kernel and byte for byte, what they are without them.
// A fourth pass (HS_ONLY_TERM, the fp64 flags) does the same for the five instances that evaluate a built-in
// termination condition (hs_set_termination_builtin).
#if defined(HS_ONLY_NORM)
hipError_t launch_queue_norm(const StepLaunch<double>& s, unsigned instance, unsigned max_grid, hipStream_t stream) {
  return launch_queue(QueueInstances<QI_ROLL | QI_EVAL | QI_NORM, QI_ROLL | QI_NORM>{}, kernel_args(s), instance, max_grid,
                      stream);
}
#elif defined(HS_ONLY_TERM)
hipError_t launch_queue_term(const StepLaunch<double>& s, unsigned instance, unsigned max_grid, hipStream_t stream) {
  return launch_queue(QueueInstances<QI_TERM, QI_ROLL | QI_EVAL | QI_NORM | QI_TERM, QI_ROLL | QI_EVAL | QI_TERM,
                                      QI_ROLL | QI_NORM | QI_TERM, QI_ROLL | QI_TERM>{},
                      kernel_args(s), instance, max_grid, stream);
}
#else
#ifndef HS_ONLY_F64
template hipError_t launch_step<float>(const StepLaunch<float>&, hipStream_t);
template int resident_waves<float>(bool);
template hipError_t launch_kinematics<float>(const DevModel<float>*, int, const float*, float*, hipStream_t);
template hipError_t launch_kinematics_batch<float>(const DevModel<float>*, int, int, const float*, const float*,
                                                   const int*, float*, hipStream_t);
template hipError_t launch_reward_eval<float>(const RewardEvalArgs<float>&, hipStream_t);
template hipError_t launch_pack<float>(const PackArgs<float>&, hipStream_t);
#endif
#ifndef HS_ONLY_F32
template hipError_t launch_step<double>(const StepLaunch<double>&, hipStream_t);
template int resident_waves<double>(bool);
template hipError_t launch_kinematics<double>(const DevModel<double>*, int, const double*, double*, hipStream_t);
template hipError_t launch_kinematics_batch<double>(const DevModel<double>*, int, int, const double*, const double*,
                                                    const int*, double*, hipStream_t);
template hipError_t launch_reward_eval<double>(const RewardEvalArgs<double>&, hipStream_t);
template hipError_t launch_pack<double>(const PackArgs<double>&, hipStream_t);
#endif
#endif   // HS_ONLY_NORM / HS_ONLY_TERM

}  // namespace hs
