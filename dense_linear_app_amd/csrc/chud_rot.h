// The arithmetic of chol_chud_tile / chol_chdd_tile (chud.hip), spelled once: one rotation of column j of L against
// one vector v, and what it does to a row i > j.  Every kernel of the family calls these two functions and nothing
// else touches L or V, so a row takes the same operations whichever kernel handles it: the result depends neither on
// the tile size nor on the launch geometry.  tests/chud_model.py is the same arithmetic in numpy (without the fused
// multiply-adds).
#pragma once
#include <hip/hip_runtime.h>

namespace cholmi {

// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every global load and store in
// flight, which would put the latency of the prefetched columns and of the stores behind them on every step of the
// chain.  The kernels of chud.hip and chex.hip exchange data between lanes through LDS alone: a lane reads and writes
// only its own rows of L and V in global memory, and a table is written by one kernel and read by the next.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// what a row needs of the rotation (column j, vector t): the appliers read it as four consecutive values
template <typename T>
struct ChudRot {
  T c, s, ci, ss;  // rr / L_jj, v_j / L_jj, L_jj / rr, sigma s
};

template <typename T>
__device__ __forceinline__ T chud_fma(T a, T b, T c);
template <>
__device__ __forceinline__ double chud_fma<double>(double a, double b, double c) {
  return fma(a, b, c);
}
template <>
__device__ __forceinline__ float chud_fma<float>(float a, float b, float c) {
  return fmaf(a, b, c);
}
template <typename T>
__device__ __forceinline__ T chud_sqrt(T x);
template <>
__device__ __forceinline__ double chud_sqrt<double>(double x) {
  return sqrt(x);
}
template <>
__device__ __forceinline__ float chud_sqrt<float>(float x) {
  return sqrtf(x);
}

// the pivot of the rotation that takes (L_jj, v_j) to (rr, 0): rr^2 = L_jj^2 + sigma v_j^2 (sigma = +1 update, -1
// downdate).  -> false when rr^2 is not positive (or NaN): then rr = L_jj and vj = 0, the identity rotation
template <typename T>
__device__ __forceinline__ bool chud_pivot(T ljj, T &vj, T sigma, T &rr) {
  const T d2 = chud_fma<T>(sigma * vj, vj, ljj * ljj);
  if (!(d2 > T(0))) {
    rr = ljj;
    vj = T(0);
    return false;
  }
  rr = chud_sqrt<T>(d2);
  return true;
}

// one of the three quotients of that rotation: q = 0: c = rr / L_jj, 1: s = v_j / L_jj, 2: ci = L_jj / rr (they do
// not depend on each other: the generator gives each to a lane of its own)
template <typename T>
__device__ __forceinline__ T chud_quotient(int q, T ljj, T vj, T rr) {
  const T num = q == 0 ? rr : q == 1 ? vj : ljj, den = q == 2 ? rr : ljj;
  return num / den;
}

// row i > j: L_ij <- (L_ij + sigma s v_i) ci, then v_i <- c v_i - s L_ij with the new L_ij
template <typename T>
__device__ __forceinline__ void chud_apply(T &lij, T &vi, const ChudRot<T> &rot) {
  lij = chud_fma<T>(rot.ss, vi, lij) * rot.ci;
  vi = chud_fma<T>(-rot.s, lij, rot.c * vi);
}

}  // namespace cholmi
