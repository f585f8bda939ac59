// Register-resident dense algebra: an nv x nv SPD matrix held row-per-lane in each half-wave,
// factored (L L' or L D L') and solved with lane broadcasts.  Restates mju_cholFactor /
// mju_cholSolve for the Newton Hessian, the PGS dual and the implicit-damping Euler step.
#pragma once
#include "hs_lanes.h"

namespace hs {
namespace {

// Cholesky A = L L' of an NV x NV SPD matrix held row-per-lane in each half (sub-lane i: row i);
// on return A holds L's strictly lower part (diagonal and upper part zeroed, so the substitutions
// below need no lane selects) and dinv (sub-lane i) = 1 / L_ii.  Step k
// publishes column k (a_ik, one ds_write) in the env's LDS vector `col`; every lane reads the
// pivot and a_jk (j > k) back as broadcast ds_reads, so the update is pure FMAs:
//   A_ij -= (a_ik / a_kk) a_jk.

// LDL: return the factor as L D L' instead (unit lower L's strictly lower part in A, dinv = 1/d_i,
// *diag = d_i): the same elimination, each finished column scaled by its pivot's 1/L_kk on the way.
template <int NV, typename T, bool LDL = false>
__device__ __forceinline__ void chol_rows(T (&A)[NV], T& dinv, int sl, T (*cb)[2], T* diag = nullptr) {
  // pivot block by DPP broadcast instead of LDS read-back: the fp64 engine only.  A/B, ms per
  // configs[1] launch: fp64 0.720 -> 0.714; fp32 0.423 -> 0.433 (2 waves per SIMD hide the LDS round
  // trip, and the extra VALU ops cost issue slots)
  constexpr bool CDPP = sizeof(T) == 8;
  // two columns per LDS round trip: every lane publishes (a_ik, a_i,k+1) as one ds_write and reads
  // the 2x2 pivot block and (a_jk, a_j,k+1) back as broadcasts.  With L_P the pivot block's
  // Cholesky factor (1/L_kk = r1, L_k+1,k = l10, 1/L_k+1,k+1 = r2), row i gets
  //   z = L_P^-1 (a_ik, a_i,k+1)   (its L entries)    f = L_P^-T z   (its Schur coefficients)
  //   A_ij -= f0 a_jk + f1 a_j,k+1   (j >= k+2)
  // and the pivot rows' own z are their L entries (L_kk, and l10, L_k+1,k+1).
  static_for<0, NV / 2>([&](auto bc) {
    constexpr int k = 2 * decltype(bc)::value;
    const int sl_k = opaque_v(sl);     // fresh compare per step (no 64-bit mask kept live)
    cb[sl_k][0] = A[k];
    cb[sl_k][1] = A[k + 1];
    T p, q, t;
    if constexpr (CDPP) {   // the pivot block by DPP broadcast from lanes k, k+1: the LDS round trip
      // of the column publish leaves the pivot chain (the trailing update still reads a_jk from LDS);
      // the pivot is clamped before the broadcast (an FMA result: no NaN canonicalization for v_max)
      p = bcast<k>(A[k] > T(1e-30) ? A[k] : T(1e-30));
      q = bcast<k + 1>(A[k]);
      t = bcast<k + 1>(A[k + 1]);
    } else {
      p = cb[k][0];
      q = cb[k + 1][0];
      t = cb[k + 1][1];
      p = p > T(1e-30) ? p : T(1e-30);
    }
    // the trailing columns' broadcast reads issued before the pivot math (fenced), so their LDS round
    // trip overlaps the pivot chain instead of following it (the machine scheduler otherwise sinks the
    // column publish and its read-back below the pivot chain): 0.691 -> 0.682 ms per fp64 configs[1]
    // launch; fp32 (pivots from LDS too, so one round trip instead of two) 0.390 -> 0.387 ms
    T cj[NV][2];
    static_for<k + 2, NV>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      cj[j][0] = cb[j][0];
      cj[j][1] = cb[j][1];
    });
    SCHED_FENCE();
    T r1 = rsqrt_t(p);
    T l10 = q * r1;
    T s11 = t - l10 * l10;
    s11 = s11 > T(1e-30) ? s11 : T(1e-30);
    T r2 = rsqrt_t(s11);
    T z0 = A[k] * r1;
    T z1 = (sl_k == k + 1) ? s11 * r2 : (A[k + 1] - l10 * z0) * r2;
    T f1 = z1 * r2;
    T f0 = (z0 - l10 * f1) * r1;
    if constexpr (LDL) {   // L~_ik = L_ik / L_kk, d = L_kk^2 (the pivots' own entries are zeroed below)
      A[k] = z0 * r1;
      A[k + 1] = z1 * r2;
      dinv = (sl_k == k) ? r1 * r1 : ((sl_k == k + 1) ? r2 * r2 : dinv);
      *diag = (sl_k == k) ? p : ((sl_k == k + 1) ? s11 : *diag);
    } else {
      A[k] = (sl_k == k) ? p * r1 : z0;
      A[k + 1] = z1;
      dinv = (sl_k == k) ? r1 : ((sl_k == k + 1) ? r2 : dinv);
    }
    static_for<k + 2, NV>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      A[j] = fma(-f0, cj[j][0], fma(-f1, cj[j][1], A[j]));
    });
    SCHED_FENCE();
  });
  if constexpr (NV % 2 == 1) {         // trailing single column
    constexpr int k = NV - 1;
    const int sl_k = opaque_v(sl);
    T akk;
    if constexpr (CDPP) {
      akk = bcast<k>(A[k]);
    } else {
      cb[sl_k][0] = A[k];
      akk = cb[k][0];
    }
    akk = akk > T(1e-30) ? akk : T(1e-30);
    if constexpr (LDL) {
      const T r = rsqrt_t(akk);
      A[k] = A[k] * r * r;
      dinv = (sl_k == k) ? r * r : dinv;
      *diag = (sl_k == k) ? akk : *diag;
    } else {
      const T r = rsqrt_t(akk);
      A[k] = (sl_k == k) ? akk * r : A[k] * r;
      dinv = (sl_k == k) ? r : dinv;
    }
  }
  const int sl_z = opaque_v(sl);
  static_for<0, NV>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    A[j] = sl_z > j ? A[j] : T(0);
  });
}
// solve (L L') x = b (L from chol_rows: strictly lower part, 1/L_ii in dinv); sub-lane i holds b_i;
// returns x_i.  Forward: at step k every lane subtracts L_ik y_k (zero unless i > k), so lane k's b
// stops changing once y_k = b_k / L_kk is broadcast, and y = b / L_ii at the end.
// UNIT: L D L' form instead (unit lower L, 1/d_i in dinv): forward with L, scale by 1/d, back with L'.
template <int NV, typename T, bool UNIT = false>
__device__ __forceinline__ T chol_solve(const T (&L)[NV], T dinv, T b, int sl) {
  static_for<0, NV - 1>([&](auto kc) {      // column NV - 1 has no row below it: skipped
    constexpr int k = decltype(kc)::value;
    b = fma(-L[k], bcast<k>(UNIT ? b : b * dinv), b);
  });
  b *= dinv;
  // back substitution x_k = (y_k - sum_{i>k} L_ik x_i) / L_kk in blocks of BS columns, top block
  // first: the sums over the rows below the block are BS independent half-wave sums (their latencies
  // overlap), the block's own rows follow as a short chain of broadcasts of L_ik x_i from lane i
  // (block size A/B, fp64 configs[1] ms per launch: BS 1 0.726, 2 0.728, 3 0.731, 4 0.738,
  // 5 0.747; fp32: BS 2 0.424 vs 3 0.426, BS 1 within noise of 2)
  constexpr int BS = sizeof(T) == 8 ? 1 : 2;
  T x = 0;
  static_for<0, (NV + BS - 1) / BS>([&](auto bc) {
    constexpr int hi = NV - BS * decltype(bc)::value;        // block = columns [lo, hi)
    constexpr int lo = hi - BS > 0 ? hi - BS : 0;
    const int sl_k = opaque_v(sl);
    T ssum[BS];
    static_for<lo, hi>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      ssum[c - lo] = hsum(L[c] * x);                           // x = 0 on lanes < hi still
    });
    static_for<0, hi - lo>([&](auto tc) {
      constexpr int c = hi - 1 - decltype(tc)::value;         // top of the block down
      T xc = UNIT ? b - ssum[c - lo] : (b - ssum[c - lo]) * dinv;   // lane c's value is x_c
      x = (sl_k == c) ? xc : x;
      static_for<lo, c>([&](auto dc) {                       // lane c's L_cd x_c to the block's lanes d < c
        constexpr int d = decltype(dc)::value;
        ssum[d - lo] += bcast<c>(L[d] * x);
      });
    });
  });
  return x;
}
// forward substitution y = L^-1 b for G right-hand sides at once (sub-lane i holds b_i of each; the
// G broadcast chains are independent, so their latencies overlap); returns y_i in place (0 on
// sub-lanes >= NV, where dinv = 0)
template <int NV, int G, typename T>
__device__ __forceinline__ void chol_fwd_multi(const T (&L)[NV], T dinv, T (&b)[G], int sl) {
  static_for<0, NV - 1>([&](auto kc) {      // the last column changes no row: skipped
    constexpr int k = decltype(kc)::value;
    static_for<0, G>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      b[g] = fma(-L[k], bcast<k>(b[g] * dinv), b[g]);
    });
  });
  static_for<0, G>([&](auto gc) { b[decltype(gc)::value] *= dinv; });
}
template <int NV, typename T>
__device__ __forceinline__ T chol_fwd(const T (&L)[NV], T dinv, T b, int sl) {
  T bb[1] = {b};
  chol_fwd_multi<NV, 1>(L, dinv, bb, sl);
  return bb[0];
}
// (A v)_i for a row-per-lane matrix and a vector in LDS (broadcast ds_reads); two accumulators
// measured no change
template <int NV, typename T>
__device__ __forceinline__ T matvec_lds(const T (&A)[NV], const T* v) {
  T acc = 0;
  static_for<0, NV>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    acc = fma(A[j], v[j], acc);
  });
  return acc;
}

}  // namespace
}  // namespace hs
