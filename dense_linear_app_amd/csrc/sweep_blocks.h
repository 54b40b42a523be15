// Device helpers shared by condest.hip (the one-vector sweeps of pocon) and refine.hip (the multi-vector sweeps and
// the residual of porfs): the cut of a single-process tile image into 128 x 128 blocks of stored rows, and the
// one-block product.  See condest.hip for the geometry.
#pragma once
#include "cholmi_internal.h"

namespace cholmi {

namespace {

constexpr int CB = 128;  // block edge

template <typename T>
struct V2;
template <>
struct V2<double> {
  using t = double2;
};
template <>
struct V2<float> {
  using t = float2;
};

__device__ __forceinline__ int bpt_of(const TileGeo &g) { return (g.mbs + CB - 1) / CB; }

// rows of block row b that lie inside the matrix (0 ... 128)
__device__ __forceinline__ int block_valid(const TileGeo &g, int b) {
  const int bpt = bpt_of(g), t = b / bpt, r0 = (b % bpt) * CB;
  const long left = min((long)g.mbu, g.m - (long)t * g.mbu) - r0;
  return (int)max(0L, min((long)CB, left));
}

// global row of vector entry (block b, t)
__device__ __forceinline__ long global_row(const TileGeo &g, long b, int t) {
  const int bpt = bpt_of(g);
  return (b / bpt) * g.mbu + (b % bpt) * CB + t;
}

// the stored block (P, Q) of the image (block row P, block column Q)
template <typename T>
__device__ __forceinline__ const T *block_at(const TileGeo &g, const T *A, int P, int Q) {
  const int bpt = bpt_of(g);
  return A + ((long)(P / bpt) + (long)(Q / bpt) * g.lmt) * g.mbs * g.mbs + (long)(P % bpt) * CB +
         (long)(Q % bpt) * CB * g.mbs;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (P, Q), P >= Q, of pair index P (P + 1) / 2 + Q
__device__ __forceinline__ void pair_of(long pair, int &P, int &Q) {
  int p = (int)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((long)p * (p + 1) / 2 > pair) --p;
  while ((long)(p + 1) * (p + 2) / 2 <= pair) ++p;
  P = p;
  Q = (int)(pair - (long)p * (p + 1) / 2);
}

// lane l's entries (rows 2l, 2l+1) of column c of a stored block, zero outside vr x vc and, with LOWER, above the
// diagonal; nothing masked is loaded
template <typename T>
__device__ __forceinline__ void load_pair(const T *S, int ld, int r, int c, int vr, int vc, bool lower, T &a0,
                                          T &a1) {
  const T *p = S + (long)c * ld + r;
  if (vr == CB && vc == CB && !lower) {
    const typename V2<T>::t a = *reinterpret_cast<const typename V2<T>::t *>(p);
    a0 = a.x;
    a1 = a.y;
    return;
  }
  const bool in = c < vc;
  a0 = (in && r < vr && (!lower || r >= c)) ? p[0] : T(0);
  a1 = (in && r + 1 < vr && (!lower || r + 1 >= c)) ? p[1] : T(0);
}

// out[t] = sum_c S(t, c) v[c] (TRANS: sum_r S(r, t) v[r]) for the 128 x 128 block S (ld), 256 threads; v and out in
// LDS (128 each), red: LDS scratch [4][128].  Fixed summation order.
template <typename T, bool TRANS>
__device__ __forceinline__ void block_product(const T *S, int ld, int vr, int vc, bool lower, const T *v, T *out,
                                              T (*red)[CB]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = 2 * lane;
  if (!TRANS) {
    T acc0 = 0, acc1 = 0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1;
      load_pair<T>(S, ld, r, c, vr, vc, lower, a0, a1);
      acc0 = fma(a0, v[c], acc0);
      acc1 = fma(a1, v[c], acc1);
    }
    red[w][r] = acc0;
    red[w][r + 1] = acc1;
    __syncthreads();
    if (tid < CB) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  } else {
    const T u0 = v[r], u1 = v[r + 1];
    T mine = 0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1;
      load_pair<T>(S, ld, r, c, vr, vc, lower, a0, a1);
      const T s = wave_sum<T>(fma(a1, u1, a0 * u0));
      if (lane == k) mine = s;
    }
    if (lane < 32) out[w * 32 + lane] = mine;
  }
  __syncthreads();
}

}  // namespace

}  // namespace cholmi
