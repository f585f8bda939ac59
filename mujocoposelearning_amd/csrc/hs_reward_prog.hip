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
#include <hip/hip_runtime.h>

#include "hs_reward_prog.h"

namespace hs {
namespace {

constexpr int RP_BLOCK = 64;   // one wave

// The interpreter loop: program `c` on env `e`'s fields, the lane's slot column at `v`.
// One dependent chain per wave (fetch, slot reads, op or gather, slot write), and 4096 envs are 64 waves:
// the kernel is latency-bound, mostly on the gathers.  Fetching the next instruction's words ahead by
// hand changed nothing (profiles/reward_programs.md).
template <typename T>
__device__ __forceinline__ T rp_run(const RpCode& c, const RpArgs<T>& a, long long e, T* v) {
  T res = T(0);
  for (int i = 0; i < c.n_instr; i++) {
    const int32_t* in = c.code + 5 * (size_t)i;
    const int op = in[0], dst = in[1], x = in[2], y = in[3], z = in[4];
    T r;
    if (op == RP_CONST) {
      r = (T)c.consts[x];
    } else if (op == RP_PARAM) {
      r = (T)c.params[x];
    } else if (op == RP_LOAD) {
      const T* f = a.field[x];
      r = f ? f[e * a.ld[x] + y] : T(0);
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

template <typename T>
__global__ __launch_bounds__(RP_BLOCK) void reward_program_kernel(RpArgs<T> a) {
  extern __shared__ double rp_lds[];
  T* v = reinterpret_cast<T*>(rp_lds) + threadIdx.x;
  const long long env = (long long)blockIdx.x * RP_BLOCK + threadIdx.x;
  const bool ok = env < a.n;
  const long long e = ok ? env : a.n - 1;   // a lane past the end mirrors the last env and writes nothing
  const bool has_prog = a.prog.n_instr > 0, has_pred = a.pred.n_instr > 0;   // wave-uniform
  T res = T(0);
  if (has_prog) res = rp_run<T>(a.prog, a, e, v);
  if (!a.outcome) {
    if (ok) a.out[env] = res;
    return;
  }
  T held = T(0);
  if (has_pred) held = rp_run<T>(a.pred, a, e, v);
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
  const unsigned blocks = (unsigned)(((long long)a.n + RP_BLOCK - 1) / RP_BLOCK);
  const size_t lds = (size_t)a.n_slots * RP_BLOCK * sizeof(T);   // <= 64 * 64 * 8 = 32 KB
  hipLaunchKernelGGL((reward_program_kernel<T>), dim3(blocks), dim3(RP_BLOCK), lds, stream, a);
  return hipGetLastError();
}

template hipError_t launch_reward_program<float>(const RpArgs<float>&, hipStream_t);
template hipError_t launch_reward_program<double>(const RpArgs<double>&, hipStream_t);

}  // namespace hs
