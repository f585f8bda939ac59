// hsim PPO update kernels for gfx950 (MI355X): deterministic column sums.  PRODUCT CODE.
//
// Column sums of a row-major [rows][cols] float32 matrix: out[c] = sum_r x[r][c].  The PPO
// update's bias gradients (sum of the output gradient over the minibatch, [32768][256]) and the
// split-K weight-gradient finish (sum over S slices of [S][out*in]).  A workgroup is a tile of
// 64 columns (a wave reads 256 contiguous bytes of a row per load) x 16 row phases (waves); each
// lane runs 4 independent accumulation chains over its rows, then the 16 phases are combined
// through LDS.  grid.y splits the rows into chunks whose partial rows a second launch
// (grid.y = 1) sums: fixed summation order, so results are run-to-run deterministic (no float
// atomics), and every lane's dependent-load chain stays short.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "hs_act.h"
#include "hs_kernels.h"
#include "ppo_launch.h"

namespace hs {
namespace {

constexpr int CS_COLS = 64, CS_PHASES = 16, CS_PAIR_COLS1 = 16;

__global__ __launch_bounds__(CS_COLS* CS_PHASES) void colsum_kernel(const float* __restrict__ x, size_t rows,
                                                                     size_t cols, size_t rows_per_chunk,
                                                                     const float* __restrict__ rw,
                                                                     float* __restrict__ out) {
  __shared__ float part[CS_PHASES][CS_COLS];
  const int lane = threadIdx.x, ph = threadIdx.y;
  const size_t c = (size_t)blockIdx.x * CS_COLS + lane;
  const size_t r0 = (size_t)blockIdx.y * rows_per_chunk;
  const size_t r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < cols) {
    const float* __restrict__ p = x + c;
    const size_t step = (size_t)CS_PHASES * cols;
    size_t r = r0 + ph;
    if (rw) {     // weighted rows: out[c] = sum_r rw[r] x[r][c] (a rank-1 weight gradient g' x)
      for (; r + 3 * CS_PHASES < r1; r += 4 * CS_PHASES) {
        const float* q = p + r * cols;
        a0 += rw[r] * q[0];
        a1 += rw[r + CS_PHASES] * q[step];
        a2 += rw[r + 2 * CS_PHASES] * q[2 * step];
        a3 += rw[r + 3 * CS_PHASES] * q[3 * step];
      }
      for (; r < r1; r += CS_PHASES) a0 += rw[r] * p[r * cols];
    } else {
      for (; r + 3 * CS_PHASES < r1; r += 4 * CS_PHASES) {
        const float* q = p + r * cols;
        a0 += q[0];
        a1 += q[step];
        a2 += q[2 * step];
        a3 += q[3 * step];
      }
      for (; r < r1; r += CS_PHASES) a0 += p[r * cols];
    }
  }
  part[ph][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (ph == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < CS_PHASES; k++) t += part[k][lane];
    out[(size_t)blockIdx.y * cols + c] = t;
  }
}

// Activation backward fused with the bias gradient's first reduction pass: gm = (y > 0) ? g : 0
// (ReLU) or g (1 - y^2) (Tanh; y is the activation's output either way, hs_act_grad) is
// written for the GEMMs that follow, and its per-chunk column sums go to `partial`
// ([gridDim.y][cols], the same tiling as colsum_kernel), finished by colsum_pair_kernel together
// with the split-K weight-gradient slices -- one pass over g instead of threshold_backward + a
// separate colsum read.
// gm of element i: the ReLU form reads g[i] under the y[i] > 0 select
template <int ACT>
__device__ __forceinline__ float act_grad_at(const float* __restrict__ g, const float* __restrict__ y, size_t i) {
  if constexpr (ACT == ACT_RELU) return y[i] > 0.f ? g[i] : 0.f;
  else return hs_act_grad<ACT>(g[i], y[i]);
}

template <int ACT>
__global__ __launch_bounds__(CS_COLS* CS_PHASES) void relu_colsum_kernel(const float* __restrict__ g,
                                                                          const float* __restrict__ y,
                                                                          size_t rows, size_t cols,
                                                                          size_t rows_per_chunk,
                                                                          float* __restrict__ gm,
                                                                          float* __restrict__ partial) {
  __shared__ float part[CS_PHASES][CS_COLS];
  const int lane = threadIdx.x, ph = threadIdx.y;
  const size_t c = (size_t)blockIdx.x * CS_COLS + lane;
  const size_t r0 = (size_t)blockIdx.y * rows_per_chunk;
  const size_t r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
  float a0 = 0.f, a1 = 0.f;
  if (c < cols) {
    size_t r = r0 + ph;
    for (; r + CS_PHASES < r1; r += 2 * CS_PHASES) {
      const size_t i0 = r * cols + c, i1 = (r + CS_PHASES) * cols + c;
      const float v0 = act_grad_at<ACT>(g, y, i0), v1 = act_grad_at<ACT>(g, y, i1);
      gm[i0] = v0;
      gm[i1] = v1;
      a0 += v0;
      a1 += v1;
    }
    for (; r < r1; r += CS_PHASES) {
      const size_t i = r * cols + c;
      const float v = act_grad_at<ACT>(g, y, i);
      gm[i] = v;
      a0 += v;
    }
  }
  part[ph][lane] = a0 + a1;
  __syncthreads();
  if (ph == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < CS_PHASES; k++) t += part[k][lane];
    partial[(size_t)blockIdx.y * cols + c] = t;
  }
}

// Two single-pass column sums in one launch (blocks [0, tiles0) do x0, the rest x1): a layer's
// split-K weight-gradient finish (S rows, many columns: 64 columns x 16 row phases per block) and its
// bias-gradient finish (hundreds of partial rows of 256 columns: 16 columns x 64 row phases per
// block, so that 16 blocks share the rows instead of 4 walking them).  Four independent
// accumulators per thread keep four loads in flight.
__global__ __launch_bounds__(CS_COLS* CS_PHASES) void colsum_pair_kernel(const float* __restrict__ x0, size_t rows0,
                                                                          size_t cols0, float* __restrict__ out0,
                                                                          const float* __restrict__ x1, size_t rows1,
                                                                          size_t cols1, float* __restrict__ out1,
                                                                          unsigned tiles0) {
  __shared__ float part[CS_COLS * CS_PHASES];
  const bool second = blockIdx.x >= tiles0;
  const float* __restrict__ x = second ? x1 : x0;
  const size_t rows = second ? rows1 : rows0, cols = second ? cols1 : cols0;
  float* __restrict__ out = second ? out1 : out0;
  const int t = threadIdx.y * CS_COLS + threadIdx.x;
  const int w = second ? CS_PAIR_COLS1 : CS_COLS, nph = CS_COLS * CS_PHASES / w;   // columns, row phases per block
  const int lane = t % w, ph = t / w;
  const size_t c = (size_t)(second ? blockIdx.x - tiles0 : blockIdx.x) * w + lane;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < cols) {
    size_t r = ph;
    for (; r + 3 * nph < rows; r += 4 * nph) {
      a0 += x[r * cols + c];
      a1 += x[(r + nph) * cols + c];
      a2 += x[(r + 2 * nph) * cols + c];
      a3 += x[(r + 3 * nph) * cols + c];
    }
    for (; r < rows; r += nph) a0 += x[r * cols + c];
  }
  part[ph * w + lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (ph == 0 && c < cols) {
    float s = 0.f;
    for (int k = 0; k < nph; k++) s += part[k * w + lane];
    out[c] = s;
  }
}

}  // namespace

// row chunks for colsum: enough workgroups to fill the chip (~1024) with >= 32 rows each;
// one chunk (a single launch) when the column tiles alone give that parallelism
static size_t colsum_chunks(size_t rows, size_t cols) {
  const size_t ctiles = (cols + CS_COLS - 1) / CS_COLS;
  if (ctiles >= 512 || rows <= 4 * CS_PHASES) return 1;
  size_t chunks = 512 / ctiles;                 // ~512 workgroups of 16 waves
  const size_t maxc = rows / (4 * CS_PHASES);   // >= 4 rows per lane
  if (chunks > maxc) chunks = maxc;
  return chunks < 1 ? 1 : chunks;
}

size_t colsum_workspace(size_t rows, size_t cols) {
  const size_t chunks = colsum_chunks(rows, cols);
  return chunks > 1 ? chunks * cols : 0;
}

hipError_t launch_colsum(const float* x, size_t rows, size_t cols, const float* row_weight, float* workspace,
                         float* out, hipStream_t stream) {
  if (cols == 0) return hipSuccess;
  const dim3 block(CS_COLS, CS_PHASES);
  const unsigned ctiles = (unsigned)((cols + CS_COLS - 1) / CS_COLS);
  const size_t chunks = colsum_chunks(rows, cols);
  if (rows == 0) return hipMemsetAsync(out, 0, cols * sizeof(float), stream);
  if (chunks <= 1) {
    hipLaunchKernelGGL(colsum_kernel, dim3(ctiles, 1), block, 0, stream, x, rows, cols, rows, row_weight, out);
    return hipGetLastError();
  }
  const size_t rpc = (rows + chunks - 1) / chunks;
  hipLaunchKernelGGL(colsum_kernel, dim3(ctiles, (unsigned)chunks), block, 0, stream, x, rows, cols, rpc,
                     row_weight, workspace);
  hipLaunchKernelGGL(colsum_kernel, dim3(ctiles, 1), block, 0, stream, (const float*)workspace, chunks, cols,
                     chunks, (const float*)nullptr, out);
  return hipGetLastError();
}

size_t colsum_partial_rows(size_t rows, size_t cols) { return colsum_chunks(rows, cols); }

hipError_t launch_relu_colsum(const float* g, const float* y, size_t rows, size_t cols, int act, float* gm,
                              float* partial, hipStream_t stream) {
  if (act != ACT_RELU && act != ACT_TANH) return hipErrorInvalidValue;
  if (cols == 0 || rows == 0) return hipSuccess;
  const size_t chunks = colsum_chunks(rows, cols);
  const size_t rpc = (rows + chunks - 1) / chunks;
  const unsigned ctiles = (unsigned)((cols + CS_COLS - 1) / CS_COLS);
  return with_act(act, [&](auto ac) {
    hipLaunchKernelGGL(relu_colsum_kernel<decltype(ac)::value>, dim3(ctiles, (unsigned)chunks),
                       dim3(CS_COLS, CS_PHASES), 0, stream, g, y, rows, cols, rpc, gm, partial);
    return hipGetLastError();
  });
}

hipError_t launch_colsum_pair(const float* x0, size_t rows0, size_t cols0, float* out0, const float* x1, size_t rows1,
                              size_t cols1, float* out1, hipStream_t stream) {
  const unsigned t0 = (unsigned)((cols0 + CS_COLS - 1) / CS_COLS),
                 t1 = (unsigned)((cols1 + CS_PAIR_COLS1 - 1) / CS_PAIR_COLS1);
  if (t0 + t1 == 0) return hipSuccess;
  hipLaunchKernelGGL(colsum_pair_kernel, dim3(t0 + t1), dim3(CS_COLS, CS_PHASES), 0, stream, x0, rows0, cols0, out0, x1,
                     rows1, cols1, out1, t0);
  return hipGetLastError();
}

}  // namespace hs
