// reward_program_kernel: a traced reward function and / or a termination predicate (hs_reward_prog.h)
// evaluated for every env of a batch.
// A translation unit of its own: the step kernels' source, flags and code objects do not know it.
//
// One env per lane, one wave per workgroup.  The instruction stream is wave-uniform (scalar loads of
// the five words, a uniform switch), so every lane runs the same op and the wave never diverges:
// selects stand in for branches.  Values are T, the batch's dtype.  The value slots are in LDS,
// slot-major -- slot s of lane l at (s * 64 + l) * sizeof(T) -- so the dynamic slot index is an
// address, not a register index: no per-lane scratch memory.  Each lane reads and writes only its own
// column, so no barrier is needed.  Bank conflicts: none -- one access of a slot touches 64 consecutive
// values; ds_read/write_b32 and _b64 are serviced per 32-lane half, whose 32 x 4 B (fp32) or 32 x 8 B
// (fp64) are 32 or 64 distinct dwords = distinct banks of the 64.
// Field loads are per-lane gathers at env * ld + index: strided and small (a reward reads tens of
// values per env against the step's thousands); left as they are.
// A reward program and a predicate run through the same interpreter (rp_run), one after the other over
// the same slots: the LDS is sized to the larger of the two.
// A program's named components (RP_OUT) leave through component-major rows [C][n]: each RP_OUT is one
// coalesced store per wave (env-major rows would be strided by C).  See RpSink.
// Reference fields (ref_qpos / ref_qvel, hs_reward_prog.h "reference motion"): when the launch's programs read
// one (RpRef::K > 0, set by the host from their field masks) the REF instance of the kernel runs: the lane
// computes its two rows and the weight ONCE, ahead of rp_run, and keeps them in registers (RpLanePhase); a load
// of such a field is then the two row gathers, issued together, and the interpolation -- no second pass over the
// program.  The rows are a few KB that every lane of the launch reads: they stay in L2.  Every other launch runs
// the instance without REF, which compiles to the code it was before: a first version that tested K in one
// kernel cost the stand program's launch 3.5 us of 64 (profiles/reference_motion.md).
#include <hip/hip_runtime.h>

#include "hs_reward_prog.h"

namespace hs {
namespace {

constexpr int RP_BLOCK = 64;   // one wave
// The interpreter loop: program `c` on env `e`'s fields, the lane's slot column at `v`.
// One dependent chain per wave (fetch, slot reads, op or gather, slot write), and 4096 envs are 64 waves:
// the kernel is latency-bound, mostly on the gathers.  Fetching the next instruction's words ahead by
// hand changed nothing (profiles/reward_programs.md).
//
// RP_OUT goes to the lane's sink.  The rows are component-major, so one RP_OUT is one store of 64 consecutive
// values per wave.  `comp` NULL (a kernel argument: the branch is wave-uniform) makes RP_OUT a no-op; a lane
// past the end (`live` false) stores nothing.  In outcome mode the value is 0 for a truncated env, as the
// reward is, and joins the episode's running sum (prev + value, rounded in T; prev reads as 0 when the sums
// belong to another episode).
template <typename T>
struct RpSink {
  T* comp = nullptr;       // [C][n] this evaluation's values
  T* total = nullptr;      // [C][n] the episode's sums (outcome mode), or NULL
  long long n = 0, env = 0;
  bool live = false, zero = false, fresh = false;
};

// the lane's phase on the reference motion: the two rows, packed into one register (i | i1 << 16; both are below
// RP_REF_MAX_ROWS = 2^12), and the second row's weight
template <typename T>
struct RpLanePhase {
  uint32_t rows = 0;
  T w = T(0);
};
static_assert(RP_REF_MAX_ROWS <= 1 << 16, "RpLanePhase packs two row indices into 32 bits");

template <typename T>
__device__ __forceinline__ RpLanePhase<T> rp_lane_phase(const RpRef<T>& r, long long e) {
  RpLanePhase<T> ph;
  const int32_t ep = r.episode[e];
  const int j0 = rp_ref_start(r.flags, r.seed, (int)e, ep, r.K);
  int i = 0, i1 = 0;
  ph.w = (T)rp_ref_phase(r.K, r.flags, j0, (double)r.time[e], r.key_dt, &i, &i1);
  ph.rows = (uint32_t)i | ((uint32_t)i1 << 16);
  return ph;
}

template <typename T, bool REF>
__device__ __forceinline__ T rp_run(const RpCode& c, const RpArgs<T>& a, long long e, T* v, const RpSink<T>& s,
                                    const RpLanePhase<T>& ph) {
  T res = T(0);
  for (int i = 0; i < c.n_instr; i++) {
    const int32_t* in = c.code + 5 * (size_t)i;
    const int op = in[0], dst = in[1], x = in[2], y = in[3], z = in[4];
    T r;
    // (RP_OUT is tested ahead of the chain: one more scalar compare per instruction, +0.5 µs on the 167
    // instructions of stand_program.  Folding it into one `op >= RP_RESULT` test with RP_RESULT, so that the
    // arithmetic ops pass no more compares than before, measured 4.5 µs SLOWER: profiles/reward_programs.md)
    if (op == RP_OUT) {
      if (s.comp && s.live) {
        const long long at = (long long)y * s.n + s.env;
        const T val = s.zero ? T(0) : v[x * RP_BLOCK];
        s.comp[at] = val;
        if (s.total) {
          const T prev = s.fresh ? T(0) : s.total[at];
          s.total[at] = prev + val;
        }
      }
      continue;
    }
    if (op == RP_CONST) {
      r = (T)c.consts[x];
    } else if (op == RP_PARAM) {
      r = (T)c.params[x];
    } else if (op == RP_LOAD) {
      if (!REF || x < RP_NFIELDS) {
        const T* f = a.field[x];
        r = f ? f[e * a.ld[x] + y] : T(0);
      } else {   // a reference field (x is wave-uniform): the two rows' values, then a + w (b - a)
        const bool pos = x == RP_F_REF_QPOS;
        const T* f = pos ? a.ref.q : a.ref.v;
        const size_t ld = (size_t)(pos ? a.ref.nq : a.ref.nv);
        const T lo = f[(size_t)(ph.rows & 0xFFFFu) * ld + (size_t)y];
        const T hi = f[(size_t)(ph.rows >> 16) * ld + (size_t)y];
        r = rp_ref_value<T>(lo, hi, ph.w);
      }
    } else if (op == RP_RESULT) {
      res = v[x * RP_BLOCK];
      break;
    } else {
      const int ar = rp_arity(op);
      const T p = v[x * RP_BLOCK];
      const T q = ar > 1 ? v[y * RP_BLOCK] : T(0);
      const T w = ar > 2 ? v[z * RP_BLOCK] : T(0);
      r = rp_op<T>(op, p, q, w);
    }
    v[dst * RP_BLOCK] = r;
  }
  return res;
}

template <typename T, bool REF>
__global__ __launch_bounds__(RP_BLOCK) void reward_program_kernel(RpArgs<T> a) {
  extern __shared__ double rp_lds[];
  T* v = reinterpret_cast<T*>(rp_lds) + threadIdx.x;
  const long long env = (long long)blockIdx.x * RP_BLOCK + threadIdx.x;
  const bool ok = env < a.n;
  const long long e = ok ? env : a.n - 1;   // a lane past the end mirrors the last env and writes nothing
  const bool has_prog = a.prog.n_instr > 0, has_pred = a.pred.n_instr > 0;   // wave-uniform
  // the reward program's component sink; a predicate has no outputs (hs_set_termination refuses them)
  RpSink<T> sink, none;
  int32_t ep = 0;
  if (a.comp) {
    sink.comp = a.comp;
    sink.n = a.n;
    sink.env = e;
    sink.live = ok;
    if (a.outcome) {
      ep = a.episode[e];
      sink.total = a.comp_total;
      sink.zero = a.truncated[e] != 0;
      sink.fresh = a.comp_episode[e] != ep;
    }
  }
  RpLanePhase<T> ph;
  if constexpr (REF) ph = rp_lane_phase<T>(a.ref, e);
  T res = T(0);
  if (has_prog) res = rp_run<T, REF>(a.prog, a, e, v, sink, ph);
  if (!a.outcome) {
    if (ok) a.out[env] = res;
    return;
  }
  T held = T(0);
  if (has_pred) held = rp_run<T, REF>(a.pred, a, e, v, none, ph);
  // The env step's outcome on the post-step, pre-reset state (custom_env.py:201-224), as the step kernel's
  // env_outcome writes it for a built-in reward: a truncated env is rewarded 0, the reward joins the
  // episode's total, a finished env leaves its final info and obs in the terminal rows, and its done byte
  // is the mask of the reset launch that follows.  Without a reward program the reward and the total are
  // the step kernel's.  With a predicate the episode also ends when it has held for grace_steps consecutive
  // env steps (custom_env.py:167-200): terminated |= early, whether or not the env is truncated.
  bool done = false;
  if (ok) {
    const bool trunc = a.truncated[env] != 0;
    bool term = a.terminated[env] != 0;
    T total = a.total_reward[env];
    if (has_prog) {
      const T r = trunc ? T(0) : res;
      total = total + r;
      a.reward[env] = r;
      a.total_reward[env] = total;
    }
    if (has_pred) {
      const int32_t ep = a.episode[env];
      bool early = false;
      a.grace_count[env] = rp_grace_update(a.grace_count[env], a.grace_episode[env], ep, rp_truth<T>(held),
                                           a.grace_steps, &early);
      a.grace_episode[env] = ep;
      a.early[env] = early;
      if (early && !term) a.terminated[env] = 1;
      term = term || early;
    }
    done = term || trunc;
    a.done[env] = done;
    if (done) {
      if (a.term_step_count) a.term_step_count[env] = a.step_count[env];
      if (a.term_total_reward) a.term_total_reward[env] = total;
    }
    // the component sums now belong to this episode; a finished env leaves them beside its total reward
    // (the lane reads back what it stored itself at its RP_OUTs)
    if (a.comp) {
      a.comp_episode[env] = ep;
      if (done)
        for (int c = 0; c < a.n_outputs; c++) {
          const long long at = (long long)c * a.n + env;
          a.term_comp_total[at] = a.comp_total[at];
        }
    }
  }
  // terminal obs rows: the wave copies each finished env's row together (coalesced; finished envs are few)
  unsigned long long m = __ballot(done);
  while (m) {
    const int l = __ffsll((long long)m) - 1;
    m &= m - 1;
    const size_t row = ((size_t)blockIdx.x * RP_BLOCK + l) * a.obs_dim;
    for (int k = threadIdx.x; k < a.obs_dim; k += RP_BLOCK) a.terminal_obs[row + k] = a.obs[row + k];
  }
}

}  // namespace

template <typename T>
hipError_t launch_reward_program(const RpArgs<T>& a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  const int ni = a.prog.n_instr, np = a.pred.n_instr;
  if (a.n_slots < 1 || a.n_slots > RP_MAX_SLOTS || ni < 0 || ni > RP_MAX_INSTR || np < 0 || np > RP_MAX_INSTR)
    return hipErrorInvalidValue;
  if (a.outcome ? (ni == 0 && np == 0) : (ni == 0 || np != 0)) return hipErrorInvalidValue;
  if (np > 0 && (!a.episode || !a.grace_count || !a.grace_episode || !a.early || a.grace_steps < 1))
    return hipErrorInvalidValue;
  if (a.comp && (ni == 0 || a.n_outputs < 1 || a.n_outputs > RP_MAX_OUTPUTS ||
                 (a.outcome && (!a.comp_total || !a.comp_episode || !a.term_comp_total || !a.episode))))
    return hipErrorInvalidValue;
  if (a.ref.K < 0 || a.ref.K > RP_REF_MAX_ROWS ||
      (a.ref.K > 0 && (!a.ref.q || !a.ref.v || !a.ref.time || !a.ref.episode || a.ref.nq < 1 || a.ref.nv < 1 ||
                       (a.ref.K > 1 && !(a.ref.key_dt > 0)))))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)(((long long)a.n + RP_BLOCK - 1) / RP_BLOCK);
  const size_t lds = (size_t)a.n_slots * RP_BLOCK * sizeof(T);   // <= 64 * 64 * 8 = 32 KB
  if (a.ref.K > 0)
    hipLaunchKernelGGL((reward_program_kernel<T, true>), dim3(blocks), dim3(RP_BLOCK), lds, stream, a);
  else
    hipLaunchKernelGGL((reward_program_kernel<T, false>), dim3(blocks), dim3(RP_BLOCK), lds, stream, a);
  return hipGetLastError();
}

template hipError_t launch_reward_program<float>(const RpArgs<float>&, hipStream_t);
template hipError_t launch_reward_program<double>(const RpArgs<double>&, hipStream_t);

}  // namespace hs
