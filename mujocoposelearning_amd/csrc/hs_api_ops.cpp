// hsim C ABI, stateless operators (see include/hsim.h): the PPO rollout / update operators, the policy
// MLP forward and backward pieces, column sums and GAE -- entry points that validate their arguments and
// launch on the caller's stream, and never touch an hs_batch (those are the batch side's: hs_api_batch.h).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hsim.h"
#include "hs_act.h"
#include "hs_api_error.h"
#include "hs_kernels.h"

using hs::fail;
using hs::hip_rc;

extern "C" {

int hs_ppo_act(const float* mean, int mean_ld, const float* value, int value_ld, const float* log_std,
               const float* episode_start, uint64_t seed, uint64_t counter, const uint64_t* counter_base,
               int deterministic, float* actions,
               float* actions_clipped, float* log_prob, float* values, float* episode_starts_out, int N, int A,
               void* stream) {
  if (N < 0 || A < 1 || A > 32) return fail("hs_ppo_act: need N >= 0 and 1 <= A <= 32");
  if (mean_ld < A || value_ld < 1) return fail("hs_ppo_act: bad leading dimension");
  if (N == 0) return 0;
  if (!mean || !value || !log_std || !episode_start || !actions || !actions_clipped || !log_prob || !values ||
      !episode_starts_out)
    return fail("hs_ppo_act: null buffer");
  return hip_rc(hs::launch_ppo_act(mean, mean_ld, value, value_ld, log_std, episode_start, seed, counter, counter_base,
                                   deterministic,
                                   actions, actions_clipped, log_prob, values, episode_starts_out, N, A,
                                   (hipStream_t)stream),
                "ppo_act_kernel");
}

int hs_ppo_post(const float* reward, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value,
                const float* terminal_obs, float* boot_obs_out, uint8_t* boot_out, int obs_dim, float gamma,
                const float* obs, float* obs_out, uint64_t obs_floats, float* reward_out, uint8_t* done_out,
                double* ep_acc, double* ep_return_out, float* episode_start, int N, void* stream) {
  if (N < 0) return fail("hs_ppo_post: negative size");
  if (N == 0) return 0;
  if (!reward || !terminated || !truncated || !reward_out || !done_out || !ep_acc || !ep_return_out || !episode_start)
    return fail("hs_ppo_post: null buffer");
  if (!terminal_value && (!terminal_obs || !boot_obs_out || !boot_out || obs_dim < 1))
    return fail("hs_ppo_post: need terminal_value, or terminal_obs + boot_obs_out + boot_out + obs_dim (deferred)");
  if (!obs) obs_floats = 0;
  if (obs_floats && !obs_out) return fail("hs_ppo_post: null obs_out");
  return hip_rc(hs::launch_ppo_post(reward, terminated, truncated, terminal_value, terminal_obs, boot_obs_out, boot_out,
                                    obs_dim, gamma, obs, obs_out, (size_t)obs_floats, reward_out, done_out, ep_acc,
                                    ep_return_out, episode_start, N, (hipStream_t)stream),
                "ppo_post_kernel");
}

int hs_gauss_logp(const float* mean, int mean_ld, const float* actions, const float* log_std, float* logp, int N,
                  int A, void* stream) {
  if (N < 0 || A < 1 || A > 32 || mean_ld < A) return fail("hs_gauss_logp: need N >= 0, 1 <= A <= 32, mean_ld >= A");
  if (N == 0) return 0;
  if (!mean || !actions || !log_std || !logp) return fail("hs_gauss_logp: null buffer");
  return hip_rc(hs::launch_gauss_logp(mean, mean_ld, actions, log_std, logp, N, A, (hipStream_t)stream),
                "gauss_logp_kernel");
}

int hs_gauss_logp_grad(const float* mean, int mean_ld, const float* actions, const float* log_std,
                       const float* g_logp, float* g_mean, float* gls_rows, int N, int A, void* stream) {
  if (N < 0 || A < 1 || mean_ld < A) return fail("hs_gauss_logp_grad: need N >= 0, A >= 1, mean_ld >= A");
  if (N == 0) return 0;
  if (!mean || !actions || !log_std || !g_logp || !g_mean || !gls_rows) return fail("hs_gauss_logp_grad: null buffer");
  return hip_rc(hs::launch_gauss_logp_grad(mean, mean_ld, actions, log_std, g_logp, g_mean, gls_rows, N, A,
                                           (hipStream_t)stream),
                "gauss_logp_grad_kernel");
}

uint64_t hs_ppo_loss_workspace(int B) { return B > 0 ? hs::ppo_loss_workspace(B) : 0; }

int hs_ppo_loss(const float* log_prob, const float* values, const int64_t* idx, const float* advantages,
                const float* returns, const float* old_log_prob, int B, float clip, int normalize_advantage,
                float* policy_loss, float* value_loss, float* workspace, void* stream) {
  if (B < 0) return fail("hs_ppo_loss: negative size");
  if (B == 0) return 0;
  if (!log_prob || !values || !idx || !advantages || !returns || !old_log_prob || !policy_loss || !value_loss ||
      !workspace)
    return fail("hs_ppo_loss: null buffer");
  return hip_rc(hs::launch_ppo_loss_fwd(log_prob, values, idx, advantages, returns, old_log_prob, B, clip,
                                        normalize_advantage, policy_loss, value_loss, workspace, (hipStream_t)stream),
                "ppo loss kernels");
}

int hs_ppo_loss_grad(const float* log_prob, const float* values, int B, float clip, const float* workspace,
                     const float* g_pg, const float* g_vf, float* g_log_prob, float* g_values, void* stream) {
  if (B < 0) return fail("hs_ppo_loss_grad: negative size");
  if (B == 0) return 0;
  if (!log_prob || !values || !workspace || !g_pg || !g_vf || !g_log_prob || !g_values)
    return fail("hs_ppo_loss_grad: null buffer");
  return hip_rc(hs::launch_ppo_loss_bwd(log_prob, values, B, clip, workspace, g_pg, g_vf, g_log_prob, g_values,
                                        (hipStream_t)stream),
                "ppo_loss_bwd_kernel");
}

uint64_t hs_adam_workspace(uint64_t total_numel) { return (uint64_t)hs::adam_partials((long long)total_numel); }

int hs_adam_clip(int nt, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const int64_t* numel, float* workspace, float max_norm,
                 double lr, double beta1, double beta2, double eps, void* stream) {
  if (nt < 1 || nt > 1024) return fail("hs_adam_clip: need 1 <= nt <= 1024 tensors");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !numel || !workspace)
    return fail("hs_adam_clip: null argument");
  std::vector<long long> n(nt);
  for (int t = 0; t < nt; t++) {
    if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || !step[t] || numel[t] < 0)
      return fail("hs_adam_clip: null tensor or negative size");
    n[t] = (long long)numel[t];
  }
  return hip_rc(hs::launch_adam_clip(nt, params, grads, exp_avg, exp_avg_sq, step, n.data(), workspace, max_norm, lr,
                                     beta1, beta2, eps, (hipStream_t)stream),
                "adam kernels");
}

static_assert(HS_PPO_HP_LR == hs::HP_LR && HS_PPO_HP_CLIP_RANGE == hs::HP_CLIP && HS_PPO_HP_CLIP_RANGE_VF == hs::HP_CLIP_VF &&
                  HS_PPO_HP_KL_STOP == hs::HP_KL_STOP && HS_PPO_HP_SIZE == 4,
              "hyperparameter block layout");
static_assert(HS_PPO_CTL_STOP == hs::CTL_STOP && HS_PPO_CTL_EPOCH == hs::CTL_EPOCH, "control words");
static_assert(HS_PPO_STAT_POLICY_LOSS == hs::ST_PG && HS_PPO_STAT_VALUE_LOSS == hs::ST_VF &&
                  HS_PPO_STAT_CLIP_FRACTION == hs::ST_CLIPFRAC && HS_PPO_STAT_ENTROPY == hs::ST_ENT &&
                  HS_PPO_STAT_LOSS == hs::ST_LOSS && HS_PPO_STAT_LOSS_LAST == hs::ST_LOSS_LAST &&
                  HS_PPO_STAT_COUNT == hs::ST_COUNT && HS_PPO_STAT_KL_LAST == hs::ST_KL_LAST &&
                  HS_PPO_STAT_EXPLAINED_VARIANCE == hs::ST_EXPL_VAR && HS_PPO_STAT_STD == hs::ST_STD &&
                  HS_PPO_STAT_KL == hs::ST_KL,
              "stats block layout");

uint64_t hs_ppo_stats_size(int n_epochs) { return (uint64_t)HS_PPO_STAT_KL + 2 * (uint64_t)(n_epochs > 0 ? n_epochs : 0); }

uint64_t hs_ppo_loss_workspace_ex(int B) { return B > 0 ? hs::ppo_loss_workspace_ex(B) : 0; }

int hs_ppo_loss_ex(const float* log_prob, const float* values, const int64_t* idx, const float* advantages,
                   const float* returns, const float* old_log_prob, const float* old_values, int B,
                   int normalize_advantage, const float* hparams, const float* log_std, int A, float vf_coef,
                   float ent_coef, float* stats, int n_epochs, int* control, float* approx_kl_out, float* policy_loss,
                   float* value_loss, float* workspace, void* stream) {
  if (B < 0) return fail("hs_ppo_loss_ex: negative size");
  if (A < 0 || A > 32 || n_epochs < 1) return fail("hs_ppo_loss_ex: need 0 <= A <= 32 and n_epochs >= 1");
  if (B == 0) return 0;
  if (!log_prob || !values || !idx || !advantages || !returns || !old_log_prob || !old_values || !hparams ||
      (A > 0 && !log_std) || !stats || !control || !policy_loss || !value_loss || !workspace)
    return fail("hs_ppo_loss_ex: null buffer");
  const hs::PpoLossEx x{hparams, log_std, A, vf_coef, ent_coef, stats, n_epochs, control, approx_kl_out};
  return hip_rc(hs::launch_ppo_loss_fwd_ex(log_prob, values, idx, advantages, returns, old_log_prob, old_values, B,
                                           normalize_advantage, x, policy_loss, value_loss, workspace,
                                           (hipStream_t)stream),
                "ppo loss kernels (ex)");
}

int hs_ppo_loss_grad_ex(const float* log_prob, const float* values, int B, const float* hparams,
                        const float* workspace, const float* g_pg, const float* g_vf, float* g_log_prob,
                        float* g_values, void* stream) {
  if (B < 0) return fail("hs_ppo_loss_grad_ex: negative size");
  if (B == 0) return 0;
  if (!log_prob || !values || !hparams || !workspace || !g_pg || !g_vf || !g_log_prob || !g_values)
    return fail("hs_ppo_loss_grad_ex: null buffer");
  return hip_rc(hs::launch_ppo_loss_bwd_ex(log_prob, values, B, hparams, workspace, g_pg, g_vf, g_log_prob, g_values,
                                           (hipStream_t)stream),
                "ppo_loss_bwd_kernel (ex)");
}

int hs_ppo_kl_stop(const float* approx_kl, const float* hparams, float* stats, int n_epochs, int* control,
                   void* stream) {
  if (n_epochs < 1) return fail("hs_ppo_kl_stop: need n_epochs >= 1");
  if (!approx_kl || !hparams || !stats || !control) return fail("hs_ppo_kl_stop: null buffer");
  return hip_rc(hs::launch_ppo_kl_stop(approx_kl, hparams, stats, n_epochs, control, (hipStream_t)stream),
                "kl_stop_kernel");
}

int hs_adam_clip_ex(int nt, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, float* const* step, const int64_t* numel, float* workspace,
                    float max_norm, const float* hparams, const int* skip, double beta1, double beta2, double eps,
                    void* stream) {
  if (nt < 1 || nt > 1024) return fail("hs_adam_clip_ex: need 1 <= nt <= 1024 tensors");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !numel || !workspace || !hparams || !skip)
    return fail("hs_adam_clip_ex: null argument");
  std::vector<long long> n(nt);
  for (int t = 0; t < nt; t++) {
    if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || !step[t] || numel[t] < 0)
      return fail("hs_adam_clip_ex: null tensor or negative size");
    n[t] = (long long)numel[t];
  }
  return hip_rc(hs::launch_adam_clip(nt, params, grads, exp_avg, exp_avg_sq, step, n.data(), workspace, max_norm, 0.0,
                                     beta1, beta2, eps, (hipStream_t)stream, hparams, skip),
                "adam kernels (ex)");
}

int hs_mlp2_forward_act(const float* X, int ldx, int D, int N, int H, int act, const float* W1, int ld1,
                        const float* b1, const float* W2, int ld2, const float* b2, const float* W3, int ld3,
                        const float* b3, int A, float* out, int ldo, void* stream) {
  if (act != HS_ACT_RELU && act != HS_ACT_TANH)
    return fail("hs_mlp2_forward: activation " + std::to_string(act) +
                " is neither HS_ACT_RELU (0) nor HS_ACT_TANH (1)");
  if (H != 64 && H != 128 && H != 256) return fail("hs_mlp2_forward: need H = 64, 128 or 256");
  if (N < 0 || D < 1 || D > 512 || A < 1 || A > 32 || ld1 < D || ld2 < H || ld3 < H || ldx < D || ldo < A)
    return fail("hs_mlp2_forward: need N >= 0, 1 <= D <= 512, 1 <= A <= 32, ld1 >= D, ld2 >= " + std::to_string(H) +
                ", ld3 >= " + std::to_string(H) + ", ldx >= D, ldo >= A");
  if (N == 0) return 0;
  if (!X || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !out) return fail("hs_mlp2_forward: null buffer");
  return hip_rc(hs::launch_mlp2_fwd(X, ldx, D, N, H, act, W1, ld1, b1, W2, ld2, b2, W3, ld3, b3, A, out, ldo,
                                    (hipStream_t)stream),
                "mlp2_fwd_kernel");
}

int hs_mlp2_forward_h(const float* X, int ldx, int D, int N, int H, const float* W1, int ld1, const float* b1,
                      const float* W2, int ld2, const float* b2, const float* W3, int ld3, const float* b3, int A,
                      float* out, int ldo, void* stream) {
  return hs_mlp2_forward_act(X, ldx, D, N, H, HS_ACT_RELU, W1, ld1, b1, W2, ld2, b2, W3, ld3, b3, A, out, ldo, stream);
}

int hs_mlp2_forward(const float* X, int ldx, int D, int N, const float* W1, int ld1, const float* b1, const float* W2,
                    int ld2, const float* b2, const float* W3, int ld3, const float* b3, int A, float* out, int ldo,
                    void* stream) {
  return hs_mlp2_forward_h(X, ldx, D, N, 256, W1, ld1, b1, W2, ld2, b2, W3, ld3, b3, A, out, ldo, stream);
}

uint64_t hs_colsum_partial_rows(uint64_t rows, uint64_t cols) { return hs::colsum_partial_rows(rows, cols); }

int hs_act_grad_colsum(const float* g, const float* y, uint64_t rows, uint64_t cols, int act, float* gm,
                       float* partial, void* stream) {
  if (act != HS_ACT_RELU && act != HS_ACT_TANH)
    return fail("hs_act_grad_colsum: activation " + std::to_string(act) +
                " is neither HS_ACT_RELU (0) nor HS_ACT_TANH (1)");
  if (!rows || !cols) return 0;
  if (!g || !y || !gm || !partial) return fail("hs_act_grad_colsum: null buffer");
  return hip_rc(hs::launch_relu_colsum(g, y, rows, cols, act, gm, partial, (hipStream_t)stream),
                "relu_colsum_kernel");
}

int hs_relu_grad_colsum(const float* g, const float* y, uint64_t rows, uint64_t cols, float* gm, float* partial,
                        void* stream) {
  return hs_act_grad_colsum(g, y, rows, cols, HS_ACT_RELU, gm, partial, stream);
}

uint64_t hs_dgrad_mask_partial_rows(int B, int K) { return hs::dgrad_mask_partial_rows(B, K); }
uint64_t hs_dgrad_mask_workspace(int K) { return hs::dgrad_mask_workspace(K); }

int hs_dgrad_mask(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B, int N,
                  float* GX, float* partial, float* workspace, void* stream) {
  return hs_dgrad_act(G, ldg, K, W, ldw, X, ldx, B, N, HS_ACT_RELU, GX, partial, workspace, stream);
}

int hs_dgrad_act(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B, int N,
                 int act, float* GX, float* partial, float* workspace, void* stream) {
  if (act != HS_ACT_RELU && act != HS_ACT_TANH)
    return fail("hs_dgrad_act: activation " + std::to_string(act) + " is neither HS_ACT_RELU (0) nor HS_ACT_TANH (1)");
  if (B < 0 || N != 256 || K < 1 || (K > 32 && (K % 16 != 0 || K > 512)) || ldg < K || ldw < N || ldx < N)
    return fail("hs_dgrad_mask: need B >= 0, N == 256, K <= 32 or K % 16 == 0 with K <= 512, ldg >= K, ldw >= N, "
                "ldx >= N");
  if (B == 0) return 0;
  if (!G || !W || !X || !GX || !partial) return fail("hs_dgrad_mask: null buffer");
  if (K > 32 && (((uintptr_t)G & 15) || (ldg & 3))) return fail("hs_dgrad_mask: K > 32 needs 16-byte aligned G rows");
  if (hs::dgrad_mask_workspace(K) && !workspace) return fail("hs_dgrad_mask: workspace required");
  return hip_rc(hs::launch_dgrad_mask(G, ldg, K, W, ldw, X, ldx, B, N, act, GX, partial, workspace, (hipStream_t)stream),
                "dgrad_mask kernel");
}

int hs_colsum_pair(const float* x0, uint64_t rows0, uint64_t cols0, float* out0, const float* x1, uint64_t rows1,
                   uint64_t cols1, float* out1, void* stream) {
  if ((cols0 && (!x0 || !out0)) || (cols1 && (!x1 || !out1))) return fail("hs_colsum_pair: null buffer");
  return hip_rc(hs::launch_colsum_pair(x0, rows0, cols0, out0, x1, rows1, cols1, out1, (hipStream_t)stream),
                "colsum_pair_kernel");
}

uint64_t hs_colsum_workspace(uint64_t rows, uint64_t cols) { return hs::colsum_workspace(rows, cols); }

int hs_colsum(const float* x, uint64_t rows, uint64_t cols, const float* row_weight, float* workspace, float* out,
              void* stream) {
  if (cols == 0) return 0;
  if (!out || (rows && !x)) return fail("hs_colsum: null buffer");
  if (hs::colsum_workspace(rows, cols) && !workspace) return fail("hs_colsum: workspace required");
  return hip_rc(hs::launch_colsum(x, rows, cols, row_weight, workspace, out, (hipStream_t)stream), "colsum_kernel");
}

uint64_t hs_obs_norm_workspace(uint64_t rows, int obs_dim) {
  return obs_dim > 0 ? hs::obs_norm_workspace((size_t)rows, obs_dim) : 0;
}

int hs_obs_norm(const float* X, uint64_t ldx, uint64_t rows, int obs_dim, const float* mean, const float* inv_std,
                float clip, float* out, uint64_t ldo, double* moments, void* workspace, void* stream) {
  if (obs_dim < 1 || obs_dim > 512) return fail("hs_obs_norm: need 1 <= obs_dim <= 512");
  if (ldx < (uint64_t)obs_dim || ldo < (uint64_t)obs_dim) return fail("hs_obs_norm: need ldx >= obs_dim and ldo >= obs_dim");
  if (!(clip > 0.f)) return fail("hs_obs_norm: need clip > 0");
  if (rows == 0) return 0;
  if (!X || !mean || !inv_std || !out) return fail("hs_obs_norm: null buffer");
  if (moments && !workspace) return fail("hs_obs_norm: moments need the workspace of hs_obs_norm_workspace bytes");
  return hip_rc(hs::launch_obs_norm(X, (size_t)ldx, (size_t)rows, obs_dim, mean, inv_std, clip, out, (size_t)ldo,
                                    moments, workspace, (hipStream_t)stream),
                "obs_norm_kernel");
}

int hs_rms_merge(double* state, int dim, const double* sets, int n_sets, uint64_t set_stride, double epsilon,
                 float* mean_f32, float* inv_std_f32, void* stream) {
  if (dim < 1 || n_sets < 0) return fail("hs_rms_merge: need dim >= 1 and n_sets >= 0");
  if (n_sets > 0 && set_stride < (uint64_t)(1 + 2 * dim)) return fail("hs_rms_merge: need set_stride >= 1 + 2 dim");
  if (!state || (n_sets > 0 && !sets)) return fail("hs_rms_merge: null buffer");
  return hip_rc(hs::launch_rms_merge(state, dim, sets, n_sets, (size_t)set_stride, epsilon, mean_f32, inv_std_f32,
                                     (hipStream_t)stream),
                "rms_merge_kernel");
}

int hs_return_moments(const float* rewards, const uint8_t* dones, int T, int N, double gamma, double* returns_carry,
                      double* workspace, double* moments, void* stream) {
  if (T < 0 || N < 0) return fail("hs_return_moments: negative size");
  if (T == 0 || N == 0) return 0;
  if (!rewards || !dones || !returns_carry || !workspace || !moments) return fail("hs_return_moments: null buffer");
  return hip_rc(hs::launch_return_moments(rewards, dones, T, N, gamma, returns_carry, workspace, moments,
                                          (hipStream_t)stream),
                "return moments kernels");
}

int hs_reward_scale(float* rewards, int T, int N, double* state, const double* moments, int n_sets,
                    uint64_t set_stride, double epsilon, double clip, double* workspace, void* stream) {
  if (T < 0 || N < 0) return fail("hs_reward_scale: negative size");
  if (n_sets < 1 || set_stride < (uint64_t)3 * (uint64_t)(T > 0 ? T : 0))
    return fail("hs_reward_scale: need n_sets >= 1 and set_stride >= 3 T");
  if (!(clip > 0.0)) return fail("hs_reward_scale: need clip > 0");
  if (T == 0 || N == 0) return 0;
  if (!rewards || !state || !moments || !workspace) return fail("hs_reward_scale: null buffer");
  return hip_rc(hs::launch_reward_scale(rewards, T, N, state, moments, n_sets, (size_t)set_stride, epsilon, clip,
                                        workspace, (hipStream_t)stream),
                "reward scale kernels");
}

int hs_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
           const float* last_dones, float* advantages, float* returns, int T, int N, float gamma, float gae_lambda,
           void* stream) {
  if (T < 0 || N < 0) return fail("hs_gae: negative size");
  if (T == 0 || N == 0) return 0;
  if (!rewards || !values || !episode_starts || !last_values || !last_dones || !advantages || !returns)
    return fail("hs_gae: null buffer");
  {  // the T >= 256 path keeps per-chunk maps / carries in the output rows: outputs must not overlap inputs
    const size_t tn = (size_t)T * (size_t)N * sizeof(float);
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
      const char *pa = (const char*)a, *pb = (const char*)b;
      return pa < pb + nb && pb < pa + na;
    };
    const void* outs[2] = {advantages, returns};
    const void* ins[3] = {rewards, values, episode_starts};
    if (overlap(advantages, tn, returns, tn)) return fail("hs_gae: advantages and returns overlap");
    for (const void* o : outs) {
      for (const void* in : ins)
        if (overlap(o, tn, in, tn)) return fail("hs_gae: an output ([T][N] advantages / returns) overlaps an input");
      if (overlap(o, tn, last_values, (size_t)N * sizeof(float)) || overlap(o, tn, last_dones, (size_t)N * sizeof(float)))
        return fail("hs_gae: an output overlaps last_values / last_dones");
    }
  }
  return hip_rc(hs::launch_gae(rewards, values, episode_starts, last_values, last_dones, advantages, returns, T, N,
                               gamma, gae_lambda, (hipStream_t)stream),
                "gae_kernel");
}

}  // extern "C"
