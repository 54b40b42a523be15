// Device helpers shared by condest.hip (lansy and the triangular sweeps), refine.hip (the residual of porfs), trmm.hip
// (the products with a triangle), mixed.hip (the symmetric residual of dsposv) and symm.hip: the cut of a
// single-process tile image into 128 x 128 blocks of stored rows, where a vector entry lies in an image, the stored
// block of a pair of the triangle, the fixed order in which a row block's partial sums are added, the wave reductions
// and the one-block product.  See condest.hip for the geometry.
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

// storage index of vector entry (block b, t) of column j of an n x ncols image with the matrix's row tiling
__device__ __forceinline__ long desc_index(const TileGeo &g, long b, int t, int j) {
  const int bpt = bpt_of(g);
  return ((b / bpt) + (long)(j / g.mbu) * g.lmt) * (long)g.mbs * g.mbs + (b % bpt) * CB + t + (long)(j % g.mbu) * g.mbs;
}

// storage index of global row i, column j of an n x ncols image / of column 0 (the S vector) / of the diagonal entry
// A(i, i)
__device__ __forceinline__ long image_index(const TileGeo &g, long i, int j) {
  return ((i / g.mbu) + (long)(j / g.mbu) * g.lmt) * (long)g.mbs * g.mbs + i % g.mbu + (long)(j % g.mbu) * g.mbs;
}
__device__ __forceinline__ long col0_index(const TileGeo &g, long i) {
  return (i / g.mbu) * (long)g.mbs * g.mbs + i % g.mbu;
}
__device__ __forceinline__ long diag_index(const TileGeo &g, long i) {
  const long t = i / g.mbu, r = i % g.mbu;
  return t * (g.lmt + 1) * (long)g.mbs * g.mbs + r + r * g.mbs;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v[0..N) of every lane summed over the 64 lanes, N in {1, 2, 4, 8}: the first log2 N exchange steps halve the values a
// lane holds (at offset 32 the lanes with bit 5 set keep the upper half and send the lower one, and so on), the rest
// is a plain butterfly.  log2 N + (6 - log2 N) ... = N - 1 + 6 - log2 N exchanges instead of 6 N.  Returns the total of
// vector *j in every lane (the lanes that share bits 5 .. 6 - log2 N of their index hold the same one); fixed order.
template <typename T, int N>
__device__ __forceinline__ T wave_sum_n(const T (&v)[N], int lane, int *j) {
  T w[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = v[i];
  int jb = 0, off = 32;
#pragma unroll
  for (int cnt = N; cnt > 1; cnt >>= 1, off >>= 1) {
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < cnt / 2; ++i) {
      const T keep = hi ? w[i + cnt / 2] : w[i], send = hi ? w[i] : w[i + cnt / 2];
      w[i] = keep + __shfl_xor(send, off, 64);
    }
    if (hi) jb += cnt / 2;
  }
#pragma unroll
  for (; off > 0; off >>= 1) w[0] += __shfl_xor(w[0], off, 64);
  *j = jb;
  return w[0];
}

// (P, Q), P >= Q, of pair index P (P + 1) / 2 + Q
__device__ __forceinline__ void pair_of(long pair, int &P, int &Q) {
  int p = (int)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((long)p * (p + 1) / 2 > pair) --p;
  while ((long)(p + 1) * (p + 2) / 2 <= pair) ++p;
  P = p;
  Q = (int)(pair - (long)p * (p + 1) / 2);
}

// The stored block of pair (P, Q), P >= Q, of the triangle: Lower at block (P, Q), Upper at (Q, P); its rows are block
// row br (vr of them inside the matrix), its columns block column bc (vc); tri: what load_pair may read of it (a
// diagonal block: only its stored half, the diagonal included)
template <typename T>
struct TriBlock {
  int P, Q, br, bc;
  const T *S;
  int vr, vc, tri;
};
template <typename T>
__device__ __forceinline__ TriBlock<T> tri_block(const TileGeo &g, const T *A, int upper, long pair) {
  TriBlock<T> b;
  pair_of(pair, b.P, b.Q);
  b.br = upper ? b.Q : b.P;
  b.bc = upper ? b.P : b.Q;
  b.S = block_at<T>(g, A, b.br, b.bc);
  b.vr = block_valid(g, b.br);
  b.vc = block_valid(g, b.bc);
  b.tri = b.P != b.Q ? 0 : upper ? 2 : 1;
  return b;
}

// The partial sums that belong to row block P of NB, in the one order every routine adds them (what makes a result
// bit-identical from run to run): f(pair, 0) for the blocks (P, q), q = 0 .. P, then f(pair, 1) for (k, P),
// k = P .. NB-1; kinds: bit 0 / bit 1 selects the halves to visit
template <typename F>
__device__ __forceinline__ void for_row_partials(int P, int NB, F f, int kinds = 3) {
  if (kinds & 1)
    for (int q = 0; q <= P; ++q) f((long)P * (P + 1) / 2 + q, 0);
  if (kinds & 2)
    for (int k = P; k < NB; ++k) f((long)k * (k + 1) / 2 + P, 1);
}

// lane l's entries (rows 2l, 2l+1) of column c of a stored block, zero outside vr x vc and outside tri: 0 the whole
// block, 1 its entries on or below the diagonal, 2 those on or above; nothing masked is loaded.  UPPER = false: for
// callers that only ever pass 0 or 1 (the sweeps: the staged diagonal tiles are Lower); the test for 2 is compiled
// out, and passing 2 there would be the caller's error (it would mask as 1)
template <typename T, bool UPPER = true>
__device__ __forceinline__ void load_pair(const T *S, int ld, int r, int c, int vr, int vc, int tri, T &a0, T &a1) {
  const T *p = S + (long)c * ld + r;
  const bool part = tri != 0, up = UPPER && tri == 2;
  if (vr == CB && vc == CB && !part) {
    const typename V2<T>::t a = *reinterpret_cast<const typename V2<T>::t *>(p);
    a0 = a.x;
    a1 = a.y;
    return;
  }
  const bool in = c < vc;
  a0 = (in && r < vr && (!part || (up ? r <= c : r >= c))) ? p[0] : T(0);
  a1 = (in && r + 1 < vr && (!part || (up ? r + 1 <= c : r + 1 >= c))) ? p[1] : T(0);
}

// load_pair for a block whose entries are used once (the products of trmm.hip): nontemporal loads; tri: 0 the whole
// block, 1 its entries on or below the diagonal, 2 those on or above; nothing masked is loaded
template <typename T>
struct V2N;
template <>
struct V2N<double> {
  typedef double t __attribute__((ext_vector_type(2)));
};
template <>
struct V2N<float> {
  typedef float t __attribute__((ext_vector_type(2)));
};
template <typename T>
__device__ __forceinline__ void load_pair_nt(const T *S, int ld, int r, int c, int vr, int vc, int tri, T &a0, T &a1) {
  const T *p = S + (long)c * ld + r;
  if (vr == CB && vc == CB && tri == 0) {
    const typename V2N<T>::t a = __builtin_nontemporal_load(reinterpret_cast<const typename V2N<T>::t *>(p));
    a0 = a.x;
    a1 = a.y;
    return;
  }
  const bool in = c < vc;
  const bool k0 = in && r < vr && (tri == 0 || (tri == 1 ? r >= c : r <= c));
  const bool k1 = in && r + 1 < vr && (tri == 0 || (tri == 1 ? r + 1 >= c : r + 1 <= c));
  a0 = k0 ? __builtin_nontemporal_load(p) : T(0);
  a1 = k1 ? __builtin_nontemporal_load(p + 1) : T(0);
}

// The one-vector product of pocon's own sweep kernels (kept beside block_product_nv: folded onto its NV = 1 form,
// pocon's application measured about 1 % slower at 16384 / 512 and 65536 / 1024 in fp64).
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
      load_pair<T, false>(S, ld, r, c, vr, vc, lower ? 1 : 0, a0, a1);
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
      load_pair<T, false>(S, ld, r, c, vr, vc, lower ? 1 : 0, a0, a1);
      const T s = wave_sum<T>(fma(a1, u1, a0 * u0));
      if (lane == k) mine = s;
    }
    if (lane < 32) out[w * 32 + lane] = mine;
  }
  __syncthreads();
}

// out[j][t] = sum_c S(t, c) v[j][c] (TRANS: sum_r S(r, t) v[j][r]) for the 128 x 128 block S (ld; tri, UPPER: load_pair)
// and NV vectors, 256 threads; v and out in LDS, red: LDS scratch.  The transposed form reduces its NV column products
// at once (wave_sum_n).  Fixed summation order.
template <typename T, bool TRANS, int NV, bool UPPER = true>
__device__ __forceinline__ void block_product_nv(const T *S, int ld, int vr, int vc, int tri, const T (*v)[CB],
                                                 T (*out)[CB], T (*red)[NV][CB]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = 2 * lane;
  if (!TRANS) {
    T acc0[NV], acc1[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc0[j] = acc1[j] = T(0);
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1;
      load_pair<T, UPPER>(S, ld, r, c, vr, vc, tri, a0, a1);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        acc0[j] = fma(a0, v[j][c], acc0[j]);
        acc1[j] = fma(a1, v[j][c], acc1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      red[w][j][r] = acc0[j];
      red[w][j][r + 1] = acc1[j];
    }
    __syncthreads();
    for (int e = tid; e < NV * CB; e += 256) {
      const int j = e / CB, t = e % CB;
      out[j][t] = ((red[0][j][t] + red[1][j][t]) + red[2][j][t]) + red[3][j][t];
    }
  } else {
    T u0[NV], u1[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) u0[j] = v[j][r], u1[j] = v[j][r + 1];
#pragma unroll 4
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1, p[NV];
      load_pair<T, UPPER>(S, ld, r, c, vr, vc, tri, a0, a1);
#pragma unroll
      for (int j = 0; j < NV; ++j) p[j] = fma(a1, u1[j], a0 * u0[j]);
      int js;
      const T s = wave_sum_n<T, NV>(p, lane, &js);
      if (lane % (64 / NV) == 0) out[js][c] = s;
    }
  }
  __syncthreads();
}

}  // namespace

}  // namespace cholmi
