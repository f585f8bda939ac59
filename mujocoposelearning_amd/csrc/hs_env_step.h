// The env layer around mj_step: bad-state checks and reset (custom_env.py:97-150), the 352-dim obs
// (custom_env.py:232-261), the per-env commit, and step_pair -- one env step (custom_env.py:152-230)
// of a wave's env pair, which every step kernel inlines once -- with the phases it calls.  The reward
// plug-ins are in hs_reward.h, the fused rollout's policy forward in hs_policy.h.
#pragma once
#include <cmath>
#include <cstdint>

#include "hs_philox.h"
#include "hs_stepper.h"
#include "hs_reward.h"
#include "hs_policy.h"
#include "hs_term_builtin.h"

namespace hs {
namespace {

// ------------------------------------------------------------------ state helpers
__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
template <typename T>
__device__ __forceinline__ T uniform_pm(uint64_t seed, int env, uint32_t episode, int k, T scale) {
  uint64_t h = splitmix(seed ^ splitmix(((uint64_t)env << 32) ^ ((uint64_t)episode << 8) ^ (uint64_t)k));
  double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);   // [0, 1)
  return (T)(-scale + 2.0 * scale * u);
}

template <typename T, typename C>
__device__ __forceinline__ void reset_state(MPtr<T> m, Scratch<T, C>& s, int sl, T& time, T& xws) {
  if (sl < m->nq) s.qpos[sl] = m->qpos0[sl];
  if (sl + HL < m->nq) s.qpos[sl + HL] = m->qpos0[sl + HL];
  if (sl < m->nv) s.qvel[sl] = 0;
  if (sl < m->nu) s.ctrl[sl] = 0;
  xws = 0;
  time = 0;
  WSYNC();
}

template <typename T, int NV, bool PGS, typename C>
__device__ __forceinline__ void physics_step(Stepper<T, NV, C>& st, KPtr<T> k, T& time, T& xws, int* warn,
                                             PgsCache<T, C>* pc) {
  MPtr<T> m = st.m;
  Scratch<T, C>& s = st.s;
  const int sl = st.sl;
  const bool up = st.up;
  // mj_checkPos / mj_checkVel (auto-reset to qpos0, time 0)
  bool bq = (sl < m->nq && isbad(s.qpos[sl])) || (sl + HL < m->nq && isbad(s.qpos[sl + HL]));
  bool bv = sl < m->nv && isbad(s.qvel[sl]);
  if (hballot(bq, up)) { warn[WARN_BADQPOS]++; reset_state(m, s, sl, time, xws); }
  else if (hballot(bv, up)) { warn[WARN_BADQVEL]++; reset_state(m, s, sl, time, xws); }
  T D[C::RPL], ar[C::RPL], rc[C::RPL], jar0[C::RPL];
  int rd[C::RPL];
  for (int attempt = 0; attempt < 2; attempt++) {
    HS_STAMP(st.clk, 0);
    st.kinematics();
    HS_STAMP(st.clk, 1);
    if constexpr (C::NEAR) {
      if (st.collision_near()) warn[WARN_OVERFLOW]++;
    } else {
      if (st.collision()) warn[WARN_OVERFLOW]++;
    }
    HS_STAMP(st.clk, 4);
    st.mass_matrix();
    HS_STAMP(st.clk, 2);
    st.velocity_forces();
    HS_STAMP(st.clk, 3);
    if (st.template rows<!PGS>(D, ar, rd, rc, xws, jar0)) warn[WARN_OVERFLOW]++;
    HS_STAMP(st.clk, 5);
    if constexpr (PGS)
      st.solve_pgs(xws, opaque(k)->p.max_newton, D, ar, rd, rc, *pc);
    else
      st.solve(xws, opaque(k)->p.max_newton, sizeof(T) == 8 ? T(1e-13) : T(1e-7), D, ar, rd, rc, jar0);
    bool ba = sl < m->nv && isbad(st.qacc);
    bool redo = hballot(ba, up) != 0 && attempt == 0;
    if (__ballot(redo) == 0) break;          // wave-uniform loop control
    if (redo) {                               // mj_checkAcc: reset and redo mj_forward
      warn[WARN_BADQACC]++;
      reset_state(m, s, sl, time, xws);
    }
  }
  if (opaque(k)->p.full_state) st.post_constraint();   // pre-integration state, like cinert / cvel in the obs
  st.euler(time);
  HS_STAMP(st.clk, 13);
  xws = st.qacc;
}

// custom_env.py:232-261 layout; qfrc_actuator comes from registers (sub-lane i holds dof i)
// UC: the row lies in uncached memory and is rewritten every env step (the fused evaluation's staging
// row): agent-scope stores, as the hand-off rows (row_st)
template <bool UC = false, typename T, typename C, typename O>
__device__ __forceinline__ void write_obs(MPtr<T> m, const Scratch<T, C>& s, int sl, T qfa, O* out,
                          int obs_dim) {
  auto put = [&](int i, O v) {
    if constexpr (UC) row_st(out + i, v);
    else out[i] = v;
  };
  int nq = m->nq, nv = m->nv;
  int o1 = nq - 2, o2 = o1 + nv, o3 = o2 + 10 * m->nbody, o4 = o3 + 6 * m->nbody;
  for (int k = sl; k < o4; k += HL) {
    T v;
    if (k < o1) v = s.qpos[2 + k];
    else if (k < o2) v = s.qvel[k - o1];
    else if (k < o3) { int q = k - o2; v = s.cinert[q / 10][q % 10]; }
    else { int q = k - o3; v = s.cvel[q / 6][q % 6]; }
    put(k, (O)v);
  }
  if (sl < nv && o4 + sl < obs_dim) put(o4 + sl, (O)qfa);
  const int o5 = o4 + nv, nf = 6 * (m->nbody - 1);
  if (obs_dim >= o5 + nf)    // full_state: + cfrc_ext[1:] (custom_env.py:247,255, commented out there)
    for (int k = sl; k < nf; k += HL) put(o5 + k, (O)s.u.n.cfrc[1 + k / 6][k % 6]);
}

template <typename T, int NV, typename C>
__device__ __forceinline__ void dump_debug(const Stepper<T, NV, C>& st, T* dbg) {
  const Scratch<T, C>& s = st.s;
  int sl = st.sl;
  for (int k = sl; k < MAXBODY * 10; k += HL) dbg[200 + k] = s.cinert[k / 10][k % 10];
  for (int k = sl; k < MAXDOF * 6; k += HL) dbg[500 + k] = s.cdof[k / 6][k % 6];
  if (sl < NV)
    for (int j = 0; j < NV; j++) dbg[700 + sl * MAXDOF + j] = st.Mr[j];
  for (int k = sl; k < MAXBODY * 6; k += HL) dbg[1800 + k] = s.cvel[k / 6][k % 6];
  if (sl < NV) {
    dbg[2280 + sl] = st.qfa;
    dbg[2320 + sl] = st.fsmooth;
    dbg[2360 + sl] = st.fcon;
    dbg[2400 + sl] = st.qacc;
  }
  if (sl == 0) {
    dbg[2500] = s.com[0]; dbg[2501] = s.com[1]; dbg[2502] = s.com[2];
    dbg[2503] = s.ncon; dbg[2504] = s.nefc; dbg[2505] = st.niter; dbg[2506] = s.nlim;
  }
  for (int c = sl; c < s.ncon; c += HL) {
    T* o = dbg + 2600 + 11 * c;
    for (int k = 0; k < 3; k++) { o[k] = s.con_pos[c][k]; o[3 + k] = s.con_n[c][k]; o[6 + k] = s.con_t1[c][k]; }
    o[9] = s.con_dist[c];
    o[10] = s.con_pair[c];
  }
  for (int r = sl; r < s.nefc; r += HL) {
    T* o = dbg + 4000 + 6 * r;     // contacts above end at 2600 + 11 * 64
    o[0] = rk_kind(s.row_kid[r]); o[1] = rk_id(s.row_kid[r]); o[2] = s.row_D[r]; o[4] = s.row_f[r];
  }
}

// per-env commit of state (+ the optional aux row / ctrl copy) for one half-wave
template <typename T, int NV, typename C>
__device__ __forceinline__ void commit(MPtr<T> m, KPtr<T> k, const Stepper<T, NV, C>& st,
                       int env, T time, T xws, int step_count, uint32_t episode, T total, const int* warn,
                       bool full) {
  const Scratch<T, C>& s = st.s;
  const int sl = st.sl, nq = m->nq, nv = m->nv, nu = m->nu;
  const int outputs = k->p.outputs;
  if (sl < nq) k->b.qpos[(size_t)env * nq + sl] = s.qpos[sl];
  if (sl + HL < nq) k->b.qpos[(size_t)env * nq + sl + HL] = s.qpos[sl + HL];
  if (sl < nv) {
    k->b.qvel[(size_t)env * nv + sl] = s.qvel[sl];
    k->b.qacc_ws[(size_t)env * nv + sl] = xws;
    if (outputs & OUT_AUX) k->b.aux[(size_t)env * AUXDIM + sl] = st.qacc;
  }
  // data.ctrl: always for resets and raw physics calls (rare); for env steps only with OUT_CTRL
  // (the host marks the buffer stale otherwise, hs_api.cpp)
  if (sl < nu && ((outputs & OUT_CTRL) || k->p.mode != MODE_ENV_STEP)) k->b.ctrl[(size_t)env * nu + sl] = s.ctrl[sl];
  if (sl == 0) {
    k->b.time[env] = time;
    k->b.step_count[env] = step_count;
    k->b.episode[env] = episode;
    k->b.total_reward[env] = total;
    if (outputs & OUT_AUX) {
      T* a = k->b.aux + (size_t)env * AUXDIM;
      a[MAXDOF + 0] = s.com[0]; a[MAXDOF + 1] = s.com[1]; a[MAXDOF + 2] = s.com[2];
      a[MAXDOF + 3] = (T)s.ncon; a[MAXDOF + 4] = (T)s.nefc; a[MAXDOF + 5] = (T)st.niter;
    }
    for (int w = 0; w < NWARN; w++)   // read-modify-write only when set (a load here would wait for
      if (warn[w]) k->b.warning[(size_t)env * NWARN + w] += warn[w];   // every store issued above)
  }
  if (full) {   // data.cfrc_ext / data.subtree_linvel of the last substep (pre-integration)
    const int nb = m->nbody;
    for (int q = sl; q < 6 * nb; q += HL) k->b.cfrc_ext[(size_t)env * 6 * nb + q] = s.u.n.cfrc[q / 6][q % 6];
    for (int q = sl; q < 3 * nb; q += HL) k->b.subtree_linvel[(size_t)env * 3 * nb + q] = s.u.n.linv[q / 3][q % 3];
  }
}

// ------------------------------------------------------------------ one env step of an env pair
// step_pair's hint bits (wave-uniform): an env of the pair will auto-reset in its next env step / the
// wave ran the reset pass in this one.  Scheduling hints for the chunk queue, never results.
constexpr int STEP_WILL_RESET = 1, STEP_DID_RESET = 2;

// Will an env that commits (time, step_count) end its episode in the next env step and auto-reset?
// The next step's own tests (below) on the values it will see: its clock after nsub more substeps
// and its step count + 1.  A prediction only: set_state / reset / configure between the launches,
// a bad-state reset, or the rounding of time + nsub * dt against nsub additions can make it wrong.
template <typename T>
__device__ __forceinline__ bool resets_next(KPtr<T> k, MPtr<T> m, T time, int step_count) {
  return k->p.autoreset && ((double)(time + (T)k->p.nsub * m->timestep) >= k->p.duration ||
                            step_count + 1 >= k->p.max_steps);
}

// ---- step_pair's phases, in the order it runs them.  Each is inlined into its one caller; `sl` is the
// lane's sub-lane of its half, `env` / `env_id` the env its half steps.

// load from batch: the env's state as the previous launch committed it
// TERM: also the env's effective grace count (the stored one belongs to the episode it is tagged with)
template <bool EVAL, bool TERM = false, typename T, typename C>
__device__ __forceinline__ void load_batch_state(KPtr<T> ka, Scratch<T, C>& s, int sl, int nq, int nv, int env_id,
                                                 bool rollout, T& time, T& xws, int& step_count, uint32_t& episode,
                                                 T& total, double& epacc, int32_t& grace) {
  time = ka->b.time[env_id];
  xws = (sl < nv) ? ka->b.qacc_ws[(size_t)env_id * nv + sl] : T(0);
  if (sl < nq) s.qpos[sl] = ka->b.qpos[(size_t)env_id * nq + sl];
  if (sl + HL < nq) s.qpos[sl + HL] = ka->b.qpos[(size_t)env_id * nq + sl + HL];
  if (sl < nv) s.qvel[sl] = ka->b.qvel[(size_t)env_id * nv + sl];
  step_count = ka->b.step_count[env_id];
  episode = ka->b.episode[env_id];
  total = ka->b.total_reward[env_id];
  if constexpr (!EVAL)
    if (rollout) epacc = ka->ro.ep_acc[env_id];
  if constexpr (TERM)
    grace = ka->tm.grace_episode[env_id] == (int32_t)episode ? ka->tm.grace_count[env_id] : 0;
}

// Queued schedule (launch_step sets p.queue when the pairs outnumber the resident waves): the
// pair's substeps [s0, s1) only.  A chunk that ends before the last substep hands the state over
// through b.mid and sets the pair's flag := this launch's tag; the last-substep chunk waits for the
// tag and starts from that row.  b.mid and the flags live in UNCACHED device memory (hs_api.cpp; its
// blocks are recycled only as uncached memory), so the stores are in memory once `s_waitcnt
// vmcnt(0)` returns and the consumer's loads cannot hit a stale L1 / L2 line: no cache invalidate or
// write-back on either side.  Every chunk recomputes the whole mj_step pipeline from (qpos, qvel,
// qacc_warmstart, time), so the hand-off is exact: results are bitwise those of one wave running all
// substeps.

// load from hand-off row: wait for the pair's previous chunk (or tape step) to hand the state over, then
// read the row.  false: the tape launch aborted, the caller leaves (results discarded: the host replays).
// TERM: the grace count comes beside the row (tm.mid_count).
template <bool EVAL, bool TERM = false, typename T, typename C>
__device__ __forceinline__ bool load_handoff_state(KPtr<T> ka, Scratch<T, C>& s, int lane, int nq, int nv, int nu,
                                                   int env_id, int pair, int wait_tag, int tstep, bool rollout,
                                                   T& time, T& xws, int& step_count, uint32_t& episode, T& total,
                                                   int (&warn)[NWARN], T& act_row, double& epacc, int32_t& grace) {
  const int sl = lane & (HL - 1);
  int* flag = ka->b.qsync + QS_FLAG + pair;
  int seen = 0, abort = 0;
  if (lane == 0) {   // bounded (~0.5 s): a broken hand-off must not hang the GPU
    int w = 0;
    if (pair + 1 != ka->p.dbg_lose_pair1)   // test hook: treat this unit's hand-off as lost
      while ((seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != wait_tag &&
             ++w < (1 << 22)) {
        // a tape launch that aborted (overflow) never hands this pair over: leave at once
        if (tstep > 0 && (abort = __hip_atomic_load(ka->b.qsync + QS_ABORT, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT)) != 0)
          break;
        __builtin_amdgcn_s_sleep(2);
      }
  }
  if (__builtin_amdgcn_readfirstlane(abort) != 0) return false;
  const bool lost = __builtin_amdgcn_readfirstlane(seen) != wait_tag;
  WSYNC();   // (compiler order: the row loads stay behind the poll)
  const T* r = ka->b.mid + (size_t)env_id * MIDDIM;
  time = row_ld(r + MID_TIME);
  xws = (sl < nv) ? row_ld(r + MID_WS + sl) : T(0);
  if (sl < nq) s.qpos[sl] = row_ld(r + MID_Q + sl);
  if (sl + HL < nq) s.qpos[sl + HL] = row_ld(r + MID_Q + sl + HL);
  if (sl < nv) s.qvel[sl] = row_ld(r + MID_V + sl);
#pragma unroll
  for (int w = 0; w < NWARN; w++) warn[w] = (int)row_ld(r + MID_W + w);
  step_count = (int)row_ld(r + MID_SC);
  episode = (uint32_t)row_ld(r + MID_EP);
  total = row_ld(r + MID_TOT);
  if (rollout) {
    if (sl < nu) act_row = row_ld(r + MID_ACT + sl);
    if constexpr (!EVAL) epacc = (double)row_ld(r + MID_EPACC);
  }
  if constexpr (TERM) grace = row_ld(ka->tm.mid_count + env_id);
  // never seen in practice; if it were, the state is poisoned so that the substep's mj_checkPos
  // resets the env (mj_resetData, ctrl 0 for that substep) -- counted in its own slot,
  // HS_WARN_HANDOFF, not as a bad state (the -1 cancels the HS_WARN_BADQPOS count the poisoned
  // qpos draws); the trainer raises on it: loud, never silent
  if (lost) {
    warn[WARN_HANDOFF]++;
    warn[WARN_BADQPOS]--;
    if (sl == 2) s.qpos[2] = T(NAN);
  }
  return true;
}

// store hand-off row: the state and the warning counters accumulated so far, for the pair's next chunk
// (or next tape step).  The caller publishes it (publish, below).  TERM: and the grace count beside it.
template <bool TERM = false, typename T, typename C>
__device__ __forceinline__ void store_handoff_state(KPtr<T> k, const Scratch<T, C>& s, int sl, int nq, int nv, int env,
                                                    T time, T xws, int step_count, uint32_t episode, T total,
                                                    const int* warn, int32_t grace = 0) {
  T* r = k->b.mid + (size_t)env * MIDDIM;
  if (sl < nq) row_st(r + MID_Q + sl, s.qpos[sl]);
  if (sl + HL < nq) row_st(r + MID_Q + sl + HL, s.qpos[sl + HL]);
  if (sl < nv) { row_st(r + MID_V + sl, s.qvel[sl]); row_st(r + MID_WS + sl, xws); }
  if (sl == 0) {
    row_st(r + MID_TIME, time);
#pragma unroll
    for (int w = 0; w < NWARN; w++) row_st(r + MID_W + w, (T)warn[w]);
    row_st(r + MID_SC, (T)step_count);
    row_st(r + MID_EP, (T)episode);
    row_st(r + MID_TOT, total);
    if constexpr (TERM) row_st(k->tm.mid_count + env, grace);
  }
}

// a word of b.qsync (a pair's flag, the abort word) := value, once every store this wave issued (its
// hand-off rows) is in memory
__device__ __forceinline__ void publish(int* word, int value, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// this env step's output rows: the tape's slice tstep, or the batch's own buffers (null: an
// intermediate step of a tape launch without per-step outputs writes none)
template <typename T>
__device__ __forceinline__ T* step_obs_row(KPtr<T> k, int env, int obs_dim, int tstep, bool tape_final) {
  if (k->tape.obs) return k->tape.obs + ((size_t)tstep * k->nenv + env) * obs_dim;
  return tape_final ? k->b.obs + (size_t)env * obs_dim : nullptr;
}
// fused rollout: the rollout buffer's obs row of step g + 1 (the obs this step returns)
template <typename T>
__device__ __forceinline__ float* ro_next_obs(KPtr<T> k, int env, int tstep) {
  const int g = k->ro.t_begin + tstep;
  return g + 1 < k->ro.t_total ? k->ro.obs + ((size_t)(g + 1) * k->nenv + env) * k->ro.D
                               : k->ro.obs_last + (size_t)env * k->ro.D;
}

// fused rollout: SB3 collect_rollouts' bookkeeping of this step (ppo_post_kernel): reward and
// done rows, the episode return, TimeLimit.truncated envs' terminal obs for the bootstrap,
// and the returned obs (an env that auto-resets returns its reset obs, written after the reset pass)
template <typename T, int NV, typename C>
__device__ __forceinline__ void rollout_rows(KPtr<T> k, const Stepper<T, NV, C>& st, int sl, int env, int tstep,
                                             int obs_dim, T r, bool term, bool trunc, double& epacc) {
  const float rf = (float)r;
  const double acc = epacc + (double)rf;
  const bool rdone = term || trunc;
  const size_t gi = (size_t)(k->ro.t_begin + tstep) * k->nenv + env;
  if (sl == 0) {
    k->ro.rew[gi] = rf;
    k->ro.done[gi] = rdone;
    k->ro.epret[gi] = acc;
    k->ro.boot[gi] = trunc && !term;
  }
  epacc = rdone ? 0.0 : acc;
  if (trunc && !term) write_obs(st.m, st.s, sl, st.qfa, k->ro.tobs + gi * obs_dim, obs_dim);
  if (!rdone) write_obs(st.m, st.s, sl, st.qfa, ro_next_obs(k, env, tstep), obs_dim);
}

// fused evaluation: no RolloutBuffer rows.  A finished episode's result slots (one address per
// episode, written once), a traced env's row of this step (written once), and the step's obs
// into the env's staging row for the policy forward (next_action)
template <typename T, int NV, typename C>
__device__ __forceinline__ void eval_rows(KPtr<T> k, const Stepper<T, NV, C>& st, int sl, int nq, int nv, int nu,
                                          int env, int tstep, int obs_dim, T r, bool rdone, T act, int step_count,
                                          uint32_t episode, T total) {
  const Scratch<T, C>& s = st.s;
  const int g = k->ro.t_begin + tstep;
  if (rdone && sl == 0) {
    const uint32_t e = episode - k->ev.episode0[env];
    if (e < (uint32_t)k->ev.max_episodes) {
      const size_t o = (size_t)e * k->nenv + env;
      k->ev.ep_return[o] = (double)total;
      k->ev.ep_length[o] = step_count;
      k->ev.ep_end_step[o] = g;
    }
  }
  if (env < k->ev.n_trace) {   // the state the reward was computed from (terminal on a done step)
    const size_t row = (size_t)g * k->ev.n_trace + env;
    T* tq = (T*)k->ev.tr_qpos + row * nq;
    if (sl < nq) tq[sl] = s.qpos[sl];
    if (sl + HL < nq) tq[sl + HL] = s.qpos[sl + HL];
    if (sl < nv) ((T*)k->ev.tr_qvel)[row * nv + sl] = s.qvel[sl];
    if (sl < nu) k->ev.tr_act[row * nu + sl] = (float)act;
    if (sl == 0) {
      ((T*)k->ev.tr_rew)[row] = r;
      k->ev.tr_done[row] = rdone;
    }
  }
  if (!rdone) write_obs<true>(st.m, s, sl, st.qfa, k->ro.obs + (size_t)env * k->ro.D, obs_dim);
}

// env-step outcome, after the last substep (custom_env.py:163-230): the obs row, and for an env step the
// reward, the done flags, a finished episode's info and terminal obs, the fused rollout's or evaluation's
// rows, and whether this half resets now (do_reset) or, HINTS, some half will in its next env step
// TERM: the built-in termination condition on the post-step state joins `term` (hs_term_builtin.h), and the
// per-env terminal rows are the launch's last step's alone (an env may end several episodes in one launch)
template <bool HINTS, bool EVAL, bool TERM = false, typename T, int NV, typename C>
__device__ __forceinline__ void env_outcome(KPtr<T> k, Stepper<T, NV, C>& st, int lane, int nq, int nv, int nu,
                                            int env, int tstep, bool tape_final, bool rollout, bool active, T act,
                                            T time, uint32_t episode, int& step_count, T& total, double& epacc,
                                            bool& rdone, bool& do_reset, bool& will_reset_next, int32_t& grace) {
  const Scratch<T, C>& s = st.s;
  const int sl = lane & (HL - 1);
  const int obs_dim = k->p.obs_dim;
  HS_STAMP(st.clk, 22);
  T* orow = step_obs_row(k, env, obs_dim, tstep, tape_final);
  if (active && orow) write_obs(st.m, s, sl, st.qfa, orow, obs_dim);
  HS_STAMP(st.clk, 23);
  if (k->p.mode != MODE_ENV_STEP) return;
  step_count += 1;
  bool trunc = step_count >= k->p.max_steps;
  // np.sum(np.square(qfrc_actuator[-nj:] * qvel[6:])) and np.sum(np.square(ctrl)) in numpy's order
  // (each sum only for the reward that reads it: kneeling the energy, stand / walk the torque;
  // the launch's reward id is wave-uniform)
  const int rid = opaque(k)->p.reward_id;
  const T e = sl < nv ? st.qfa * s.qvel[sl] : T(0);
  const T esum = rid == REWARD_KNEELING ? np_sum_half(e * e, 6, nv - 6, lane) : T(0);
  const T cu = sl < st.m->nu ? s.ctrl[sl] : T(0);
  const T csum = (rid == REWARD_STAND || rid == REWARD_WALK) ? np_sum_half(cu * cu, 0, st.m->nu, lane) : T(0);
  HS_STAMP(st.clk, 24);
  T r = trunc ? T(0) : compute_reward(st.m, s, k, time, esum, csum);
  HS_STAMP(st.clk, 25);
  total += r;
  bool term = (double)time >= k->p.duration;
  if constexpr (TERM) {
    // the episode also ends when the condition has held for grace_steps consecutive env steps of it
    // (custom_env.py:167-200), whether or not the step is truncated; the count, the episode it belongs to and
    // the early byte are committed by the launch's last step, as the state is
    const bool holds = term_builtin_holds<T>(k->tm.kind, (T)k->tm.min_height, (T)k->tm.max_roll_pitch, s.qpos);
    bool early = false;
    grace = rp_grace_update(grace, (int32_t)episode, (int32_t)episode, holds, k->tm.grace_steps, &early);
    term |= early;
    if (tape_final && active && sl == 0) {
      k->tm.grace_count[env] = grace;
      k->tm.grace_episode[env] = (int32_t)episode;
      k->tm.early[env] = early;
    }
  }
  if (sl == 0 && active && (k->tape.reward || tape_final)) {
    const size_t o = k->tape.reward ? (size_t)tstep * k->nenv : 0;
    (k->tape.reward ? k->tape.reward : k->b.reward)[o + env] = r;
    (k->tape.terminated ? k->tape.terminated : k->b.terminated)[o + env] = term;
    (k->tape.truncated ? k->tape.truncated : k->b.truncated)[o + env] = trunc;
  }
  // the final step's info of a finished episode (SubprocVecEnv returns its step_count /
  // total_reward before resetting, custom_env.py:216-224), with or without auto-reset
  if ((term || trunc) && active && sl == 0 && (!TERM || tape_final)) {
    if (k->b.term_step_count) k->b.term_step_count[env] = step_count;
    if (k->b.term_total_reward) k->b.term_total_reward[env] = total;
  }
  if (rollout && active) {
    rdone = term || trunc;
    if constexpr (EVAL) eval_rows(k, st, sl, nq, nv, nu, env, tstep, obs_dim, r, rdone, act, step_count, episode, total);
    else rollout_rows(k, st, sl, env, tstep, obs_dim, r, term, trunc, epacc);
  }
  if ((term || trunc) && k->p.autoreset && active) {
    if (!TERM || tape_final) write_obs(st.m, s, sl, st.qfa, k->b.terminal_obs + (size_t)env * obs_dim, obs_dim);
    do_reset = true;
  }
  // (an env that resets below restarts at time = dt, step 0: not flagged)
  if constexpr (HINTS)
    will_reset_next = __ballot(active && !do_reset && resets_next(k, st.m, time, step_count)) != 0;
}

// resident tier: an overflowing env is deferred to the wide tier instead of committed
template <typename T, typename C>
__device__ __forceinline__ bool defer_to_wide(KPtr<T> k, const int* warn, int sl, int env) {
  if constexpr (C::WIDE) {
    return false;
  } else {
    if (!k->b.redo || warn[WARN_OVERFLOW] == 0) return false;
    if (sl == 0) {
      const int slot = atomicAdd(&k->b.redo[0], 1);
      k->b.redo[2 + slot] = env;
      atomicAdd(k->b.redo_total, 1ull);
    }
    return true;
  }
}

// commit, defer or hand off: where the state of an env that has finished its env step (or its reset
// pass) goes, as (step_count, total) of the calling site.  true: deferred to the wide tier, nothing written.
// Tape launch (set_tag on a whole-step item): the state goes on to the pair's next env step only
// through its hand-off row (uncached), together with the warning counters accumulated so far.
// Only the tape's LAST step commits to the batch buffers: consecutive steps of one env may run on
// different XCDs, whose L2s are not coherent with each other, so two steps writing the same
// batch address would leave whichever dirty line is written back last.  For the same reason the
// batch's obs / reward / done rows are written by the last step only when the tape has no
// per-step outputs, and the host keeps each env to at most one finished episode per tape launch
// (hs_step_tape), so its terminal obs / info rows are written once.  A TERM instance, in which an env may
// finish several episodes, writes those rows on the tape's last step only (env_outcome).
template <bool TERM = false, typename T, int NV, typename C>
__device__ __forceinline__ bool commit_or_handoff(KPtr<T> k, const Stepper<T, NV, C>& st, int sl, int nq, int nv,
                                                  int env, T time, T xws, int step_count, uint32_t episode, T total,
                                                  const int* warn, bool tape_final, bool tape_handoff,
                                                  int32_t grace = 0) {
  if (defer_to_wide<T, C>(k, warn, sl, env)) return true;
  if (tape_final) commit(st.m, k, st, env, time, xws, step_count, episode, total, warn, k->p.full_state != 0);
  if (tape_handoff)
    store_handoff_state<TERM>(k, st.s, sl, nq, nv, env, time, xws, step_count, episode, total, warn, grace);
  return false;
}

// reset draw: custom_env.py:97-130: mj_resetData; qpos = init (z=1.282, upright); += U(+-0.01) noise
// with z noise x0.1 and no quaternion noise; qvel = U(+-0.01); one mj_step with ctrl = 0 (the caller's
// next substep).
// With a bank of initial states bound (KArgs::in, hs_set_initial_states) the episode starts from one of its
// rows instead: row j = min(K - 1, floor(u K)), u the [0, 1) value of the counter hash at (seed, env, new
// episode, INIT_SLOT) -- a slot no noise draw uses (qpos 0..nq-1, qvel 64..64+nv-1) -- whichever noise source
// is bound; qpos = row + noise, qvel = row + noise, the free-joint rules on the noise alone (the row supplies
// the height and the orientation).  One coalesced read of the row per reset: lane sl reads elements sl and
// sl + HL.  K is wave-uniform, j the same in all lanes of a half-wave.
constexpr int INIT_SLOT = 128;
// the bank row of (seed, env, episode): scalar arithmetic on a half-wave's uniform values
__device__ __forceinline__ int bank_row(uint64_t seed, int env, uint32_t ep, int K) {
  const uint64_t h = splitmix(seed ^ splitmix(((uint64_t)env << 32) ^ ((uint64_t)ep << 8) ^ (uint64_t)INIT_SLOT));
  const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);   // [0, 1), as uniform_pm
  return min(K - 1, (int)(u * (double)K));
}
template <typename T, typename C>
__device__ __forceinline__ void reset_draw(KPtr<T> k, MPtr<T> m, Scratch<T, C>& s, int sl, int nq, int nv, int nu,
                                           int env, uint32_t& episode, T& time, T& xws) {
  T sc = (T)k->p.noise_scale;
  const uint64_t seed = k->p.seed;
  const T* nz_q = k->nz_q;
  const T* nz_v = k->nz_v;
  uint32_t ep = episode + 1;
  // a bank bound: each half's row index from its own (env, episode), computed on the scalar unit from the halves'
  // first lanes, so that nothing of it occupies a vector register; the rows are read relative to the uniform base
  const int K = k->in.K;
  uint32_t row = 0;
  if (K > 0) {
    const int j0 = bank_row(seed, __builtin_amdgcn_readfirstlane(env), __builtin_amdgcn_readfirstlane(ep), K);
    const int j1 = bank_row(seed, __builtin_amdgcn_readlane(env, HL), __builtin_amdgcn_readlane(ep, HL), K);
    row = (uint32_t)(threadIdx.x >= HL ? j1 : j0);
  }
  for (int q = sl; q < nq; q += HL) {
    T v = K > 0 ? k->in.q[row * (uint32_t)nq + (uint32_t)q] : m->qpos0[q];
    T nzq = nz_q ? nz_q[(size_t)env * nq + q] : uniform_pm<T>(seed, env, ep, q, sc);
    if (m->jnt_type[0] == JNT_FREE) {
      if (q == 2) { if (K <= 0) v = (T)k->p.init_height; nzq *= T(0.1); }
      if (q >= 3 && q < 7) { if (K <= 0) v = q == 3 ? T(1) : T(0); nzq = 0; }
    }
    s.qpos[q] = v + nzq;
  }
  if (sl < nv) {
    const T nzv = nz_v ? nz_v[(size_t)env * nv + sl] : uniform_pm<T>(seed, env, ep, 64 + sl, sc);
    s.qvel[sl] = K > 0 ? k->in.v[row * (uint32_t)nv + (uint32_t)sl] + nzv : nzv;
  }
  if (sl < nu) s.ctrl[sl] = 0;
  xws = 0;
  time = 0;
  episode = ep;
  WSYNC();
}

// next action (fused rollout and evaluation): the policy acts on the step's obs: step g + 1's action, the
// mean or the draw of counter g + 1 + *ctr_base as ppo_act_kernel makes it, clipped, into the hand-off row
// (or act_clip after the launch's last step).  The rollout also writes step g + 1's RolloutBuffer rows and
// carries the episode return.
// EVAL: the obs is in the env's staging row.  The row is uncached memory, written by env_outcome or after
// the reset pass with agent-scope stores by this wave (both halves' rows; a ghost half reads its partner's)
// and read back at agent scope after the wait below: no L1 / L2 line of an earlier step of this env, on
// whatever XCD it ran, can be returned.
// NORM: the policy reads the obs normalised with the launch's moments (hs_policy.h).
template <bool EVAL, bool NORM = false, typename T, typename C>
__device__ __forceinline__ void next_action(KPtr<T> k, Scratch<T, C>* smem, int lane, int env_id, int tstep, bool real,
                                            T act, double epacc, bool rdone) {
  const int sl = lane & (HL - 1);
  const int g = k->ro.t_begin + tstep, A = k->ro.A;
  const bool last_of_launch = tstep == k->p.nsteps - 1;
  T* r = k->b.mid + (size_t)env_id * MIDDIM;
  if (g + 1 < k->ro.t_total) {
    [[maybe_unused]] const size_t gi = (size_t)(g + 1) * k->nenv + env_id;   // the rollout's rows of step g + 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's obs row is written before it is read
    float mean;
    if constexpr (EVAL) mean = policy_mean<true, NORM>(k, k->ro.obs + (size_t)env_id * k->ro.D, smem, lane);
    else mean = policy_mean<false, NORM>(k, k->ro.obs + gi * k->ro.D, smem, lane);
    const float ls = sl < A ? k->ro.log_std[sl] : 0.f;
    float z = 0.f;
    if (!k->ro.deterministic && sl < A)
      z = policy_noise((uint32_t)env_id, (uint32_t)sl, (uint64_t)(g + 1) + *k->ro.ctr_base, k->ro.k0, k->ro.k1);
    const float a = mean + __expf(ls) * z;
    const float ac = fminf(fmaxf(a, -1.f), 1.f);
    if (real && sl < A) {
      if constexpr (!EVAL) k->ro.act[gi * A + sl] = a;
      if (last_of_launch) k->ro.act_clip[(size_t)env_id * A + sl] = ac;
      else row_st(r + MID_ACT + sl, (T)ac);
    }
    if constexpr (!EVAL) {
      const float lp = half_sum(sl < A ? -0.5f * z * z - ls - 0.91893853320467274f : 0.f);
      if (real && sl == 0) {
        k->ro.logp[gi] = lp;
        k->ro.start[gi] = rdone ? 1.f : 0.f;
      }
    }
  }
  // the rollout's last step: act_clip ends as the action that step ran with (as the per-step path)
  // (its own test, not the else of the one above: as an else the rollout instance took 256 AGPRs and
  // 16 B/lane of scratch, against 254 and none, profiles/step_pair_split.md)
  if (real && last_of_launch && g + 1 >= k->ro.t_total && sl < A) k->ro.act_clip[(size_t)env_id * A + sl] = (float)act;
  if constexpr (!EVAL) {
    if (real && sl == 0) {
      if (last_of_launch) {
        k->ro.ep_acc[env_id] = epacc;
        k->ro.episode_start[env_id] = rdone ? 1.f : 0.f;
      } else {
        row_st(r + MID_EPACC, (T)epacc);
      }
    }
  }
}

// signal: a tape launch never runs the wide tier, so an env deferred on ANY of its steps -- the last one
// included, which hands nothing over -- stops the launch: the host restores the saved state and
// replays the tape step by step (hs_api.cpp guarded_tape).  Otherwise the pair's next env step may
// start: rows in memory, then the flag.
template <typename T>
__device__ __forceinline__ void signal_next_step(KPtr<T> k, int lane, int pair, int set_tag, bool tape_handoff,
                                                 bool deferred) {
  const bool any_deferred = __ballot(deferred) != 0;
  if (any_deferred) publish(k->b.qsync + QS_ABORT, 1, lane);
  else if (tape_handoff) publish(k->b.qsync + QS_FLAG + pair, set_tag, lane);
}

// One env step (or reset / raw physics call) of the env pair (index, index + 1) of one wave.
// `list` (wide tier): indices map to env ids through it; resident tier: indices are env ids.
// In the resident tier an env whose contacts / rows overflowed the resident capacity in any
// substep is NOT committed: it is appended to the wide tier's work list instead, and the wide
// launch that follows re-runs its whole step from the same (untouched) inputs.
// Queued schedule: the pair's substeps [s0, s1) only, the state arriving (wait_tag) and leaving
// (set_tag) through the pair's hand-off row (load_handoff_state above).
// ghost: this half-wave mirrors env idx (the single-env schedule's upper half) and commits nothing.
// HINTS (the chunk queue): *hint = STEP_* bits of this call.
// EVAL (with ROLL): the fused evaluation (hs_evaluate, EvalArgs) -- the rollout's loop without the
// RolloutBuffer: the step's obs goes to the env's one staging row (ro.obs, [N][D], uncached), the policy
// reads it back, the clipped action goes to the pair's next step; a finished episode writes its three
// result slots, a traced env one trace row.
// NORM (with ROLL): the instances of hs_rollout_norm / hs_evaluate_norm, whose policy normalises its obs.
// TERM (tape launches of the fp64 Newton engine): the instances that evaluate a built-in termination condition
// themselves (KArgs::tm, hs_set_termination_builtin).
template <typename T, int NV, bool PGS, typename C, bool ROLL = false, bool HINTS = false, bool EVAL = false,
          bool NORM = false, bool TERM = false>
__device__ __forceinline__ void step_pair(KPtr<T> ka, Scratch<T, C>* smem, PgsCache<T, C>* pcache, int idx,
                                          int nidx, const int* list, int s0, int s1, int pair, bool ghost = false,
                                          int wait_tag = 0, int set_tag = 0, int tstep = 0, bool tape_launch = false,
                                          int* hint = nullptr) {
  if constexpr (HINTS) *hint = 0;
  [[maybe_unused]] constexpr bool WIDE = C::WIDE;   // (HS_FLUSH)
  const int lane = opaque_v(threadIdx.x);   // (no lane-derived value hoisted out of the chunk-queue loop)
  const bool up = lane >= HL;
  const int sl = lane & (HL - 1);
  bool active = idx < nidx && !ghost;                 // ghost half: odd count, or the single-env schedule
  const int ei = idx < nidx ? idx : nidx - 1;
  const int env_id = list ? list[ei] : ei;
  const int mode = ka->p.mode;
  if (mode == MODE_RESET && ka->reset_mask && !ka->reset_mask[env_id]) active = false;
  if (__ballot(active) == 0) return;                  // wave-uniform exit
  const bool real = active;                           // this half steps (and commits) a real env
  // fused rollout (fp64 engine): the episode return so far and the step's done flag, carried to the
  // policy forward after the step; the action of steps after the launch's first comes in the row
  const bool rollout = ROLL && ka->ro.obs != nullptr;
  double epacc = 0.0;
  bool rdone = false;
  T act_row = T(0);
  Scratch<T, C>& s = smem[up ? 1 : 0];
  MPtr<T> m = ka->m;
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  Stepper<T, NV, C> st(m, s, lane);
  if (ka->b.dbg && env_id == 0 && active) st.dbg = ka->b.dbg;
  int warn[NWARN] = {0, 0, 0, 0, 0};
  T time, xws;
  int step_count;
  uint32_t episode;
  T total, act;
  [[maybe_unused]] int32_t grace = 0;   // (TERM) consecutive env steps of the episode the condition has held
  if (wait_tag != 0) {   // queued: the pair's previous chunk (or tape step) hands the state over
    if (!load_handoff_state<EVAL, TERM>(ka, s, lane, nq, nv, nu, env_id, pair, wait_tag, tstep, rollout, time, xws,
                                        step_count, episode, total, warn, act_row, epacc, grace))
      return;
  } else {
    load_batch_state<EVAL, TERM>(ka, s, sl, nq, nv, env_id, rollout, time, xws, step_count, episode, total, epacc,
                                 grace);
  }
  {
    // data.ctrl is an input only to a raw physics call that keeps the current ctrl; env steps set
    // it from the action, resets zero it
    const float* actions = ka->actions;
    if (sl < nu) s.ctrl[sl] = (mode == MODE_PHYSICS && !actions) ? ka->b.ctrl[(size_t)env_id * nu + sl] : T(0);
    // the action is the same for all substeps: one load, issued with the state loads (a tape
    // launch's step tstep reads its own [N][nu] slice)
    // (a rollout's `actions` is its first step's, ro.act_clip; later steps' come in the row)
    act = (rollout && tstep > 0) ? act_row
        : (actions && sl < nu) ? (T)actions[((size_t)tstep * ka->nenv + env_id) * nu + sl] : T(0);
  }
  WSYNC();
  st.clk.start();
  st.qfa = 0;
  st.qacc = 0;
  st.niter = 0;
  // tape launch: a whole-step item hands over to the pair's next env step, and only the tape's last
  // step commits to the batch (commit_or_handoff)
  const bool tape_handoff = set_tag != 0 && s1 == ka->p.nsub;
  const bool tape_final = !(ka->p.nsteps > 1 && tstep < ka->p.nsteps - 1);
  bool deferred = false;

  // Both halves always run the same instruction stream; a half that is inactive (ghost env,
  // masked reset) or not resetting while its partner resets computes on scratch but commits
  // nothing (its real state was committed before the shared reset pass).
  bool do_reset = mode == MODE_RESET && active;
  const int nsub = (mode == MODE_RESET) ? 0 : ka->p.nsub;
  bool in_reset = false;
  // wave-uniform: some env of the pair will auto-reset in its NEXT env step (the clock or the step
  // count it commits here already says so); the chunk queue claims such pairs first (step_kernel_queue)
  bool will_reset_next = false;
#ifdef HS_TIMING
  int tot_iter = 0;
  const int titem = (ka->p.queue ? (s0 > 0 ? (nidx + 1) / 2 : 0) + pair : -1);
#endif
  // One loop, ONE inlined physics_step call site: substeps 0..nsub-1 apply the action; after the
  // last one the env bookkeeping runs; if any half of the wave must reset, one more substep
  // runs with the reset state (a half that is not resetting has already committed and computes
  // on scratch only).  Launch arguments are re-read through k = opaque(ka) at each use.
  for (int sub = s0;; sub++) {
    st.m = opaque(st.m);
    st.sl = opaque_v(st.sl);
    const int env = opaque_v(env_id);   // per-env addresses recomputed at each use, not kept live
    if (sub == s1 && s1 < nsub) {         // queued chunk ends before the last substep: hand over
      KPtr<T> k = opaque(ka);
      if (active) store_handoff_state<TERM>(k, s, sl, nq, nv, env, time, xws, step_count, episode, total, warn, grace);
      publish(k->b.qsync + QS_FLAG + pair, set_tag, lane);   // the row is in memory before the flag is
      HS_FLUSH();
      break;
    }
    if (sub == nsub && !in_reset) {       // after the last substep: the env step's outcome
      if (nsub > 0) {
        KPtr<T> k = opaque(ka);
        env_outcome<HINTS, EVAL, TERM>(k, st, lane, nq, nv, nu, env, tstep, tape_final, rollout, active, act, time,
                                       episode, step_count, total, epacc, rdone, do_reset, will_reset_next, grace);
        if (active && !do_reset) {
          if (commit_or_handoff<TERM>(k, st, sl, nq, nv, env, time, xws, step_count, episode, total, warn, tape_final,
                                      tape_handoff, grace))
            deferred = true;
          active = false;   // committed (or deferred); a reset pass below is scratch work for this half
        }
      }
      if (__ballot(do_reset) == 0) { HS_FLUSH(); break; }
      in_reset = true;
      st.dbg = nullptr;
      reset_draw(opaque(ka), m, s, sl, nq, nv, nu, env, episode, time, xws);
      if constexpr (TERM) grace = 0;   // the count belongs to the episode that ended
    } else if (sub > nsub) {              // after the reset's substep: the reset obs, the new episode's state
      if (do_reset && active) {
        KPtr<T> k = opaque(ka);
        if (k->b.dbg && env == 0) dump_debug(st, k->b.dbg);
        const int obs_dim = k->p.obs_dim;
        T* orow = step_obs_row(k, env, obs_dim, tstep, tape_final);
        if (orow) write_obs(st.m, s, sl, st.qfa, orow, obs_dim);
        if constexpr (EVAL) {
          if (rollout) write_obs<true>(st.m, s, sl, st.qfa, k->ro.obs + (size_t)env * k->ro.D, obs_dim);
        } else if (rollout) write_obs(st.m, s, sl, st.qfa, ro_next_obs(k, env, tstep), obs_dim);   // the reset obs
        if (commit_or_handoff<TERM>(k, st, sl, nq, nv, env, time, xws, 0, episode, T(0), warn, tape_final, tape_handoff,
                                    grace))
          deferred = true;
      }
      HS_FLUSH();
      break;
    } else {
      // data.ctrl[:] = action each substep (custom_env.py:159); mj_resetData may have zeroed it
      if (sl < nu && opaque(ka)->actions) s.ctrl[sl] = act;
      WSYNC();
    }
    physics_step<T, NV, PGS>(st, ka, time, xws, warn, pcache);
#ifdef HS_TIMING
    tot_iter += st.niter;
#endif
    if (st.dbg && active && !in_reset) dump_debug(st, st.dbg);
  }
  if constexpr (ROLL) {
    if (rollout) next_action<EVAL, NORM>(opaque(ka), smem, lane, env_id, tstep, real, act, epacc, rdone);
  }
  if (tape_handoff || tape_launch) signal_next_step(opaque(ka), lane, pair, set_tag, tape_handoff, deferred);
  if constexpr (HINTS) *hint = (will_reset_next ? STEP_WILL_RESET : 0) | (in_reset ? STEP_DID_RESET : 0);
}

}  // namespace
}  // namespace hs
