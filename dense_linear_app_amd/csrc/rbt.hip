// The kernels of the symmetric random butterfly transformation behind chol_sytrf_rbt_tile / chol_sytrs_rbt_tile /
// chol_sysv_rbt_tile / chol_rbt_apply_tile (spd.hip): A <- W^T A W on the stored Lower triangle, in place, one level of
// the recursive butterfly per pass, and B <- W^T B / X <- W X on an n x nrhs image.
//
// A butterfly of order 2h over the rows o .. o+2h-1 is B = 2^(-1/2) [[R0, R1], [R0, -R1]], R0 = diag(w(o .. o+h-1)),
// R1 = diag(w(o+h .. o+2h-1)), w the column of the descriptor W that belongs to the level.  Level k has 2^k butterflies
// of order n / 2^k side by side.  For the row butterfly p and the column butterfly q of one level the block
// A(p,q) = [[a11, a12], [a21, a22]] (h x h each) becomes B_p^T A(p,q) B_q; entry (i,j) of the four quarters maps to
// the same four places:
//     s1 = a11 + a21   d1 = a11 - a21   s2 = a12 + a22   d2 = a12 - a22
//     c11 = (r0p_i r0q_j) ((s1 + s2) / 2)      c12 = (r0p_i r1q_j) ((s1 - s2) / 2)
//     c21 = (r1p_i r0q_j) ((d1 + d2) / 2)      c22 = (r1p_i r1q_j) ((d1 - d2) / 2)
// (the two factors 2^(-1/2) are the exact 1/2).  One work item owns one such group, so a pass needs no copy of A and no
// atomics.  p > q: all four numbers lie in the stored triangle (k_rbt_pass<T, false>).  p == q: a12(i,j) is stored as
// a21(j,i), so the items i >= j cover the stored triangle: i > j owns a11(i,j), a21(i,j), a21(j,i), a22(i,j), i == j
// owns three numbers and writes c21 (k_rbt_pass<T, true>).  A workgroup takes a 64 x 64 block of (i,j); lanes walk down
// a column.  The transposed quarter-block a21(j,i) goes through LDS: it is read and written back along its own
// columns.  Entries are addressed one by one through the tile geometry, so neither h nor o is tied to the tile edge;
// the padding of the image is never touched.  Every element of the triangle is read once and written once per level:
// streaming (nontemporal) accesses.  Built with floating-point contraction off: the operation order above is the
// order of tests/rbt_model.py, bit for bit.
#include "cholmi_internal.h"

namespace cholmi {

namespace {

constexpr int RT = 64;  // edge of a workgroup's block of groups

// entry (r, c) of an image at rbt_row(g, r) + rbt_col(g, c)
__device__ __forceinline__ long rbt_row(const TileGeo &g, int r) {
  const int t = r / g.mbu;
  return (long)t * g.mbs * g.mbs + (r - t * g.mbu);
}
__device__ __forceinline__ long rbt_col(const TileGeo &g, int c) {
  const int t = c / g.mbu;
  return (long)t * g.lmt * g.mbs * g.mbs + (long)(c - t * g.mbu) * g.mbs;
}

template <typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
  return __builtin_nontemporal_load(p);
}
template <typename T>
__device__ __forceinline__ void st_stream(T *p, T v) {
  __builtin_nontemporal_store(v, p);
}

// (P, Q), P >= Q, of index P (P + 1) / 2 + Q
__device__ __forceinline__ void tri_pair(long x, int &P, int &Q) {
  int p = (int)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
  while ((long)p * (p + 1) / 2 > x) --p;
  while ((long)(p + 1) * (p + 2) / 2 <= x) ++p;
  P = p;
  Q = (int)(x - (long)p * (p + 1) / 2);
}

// One level (column `level` of W, half order h, nbf butterflies) on the blocks p == q (DIAG) or p > q of the level's
// partition.  Work item: blocks of 64 x 64 groups, nb = ceil(h / 64) per side; per_bf of them per butterfly (pair),
// `total` in all, taken by the grid in a stride loop.
template <typename T, bool DIAG>
__global__ __launch_bounds__(256) void k_rbt_pass(TileGeo ga, T *A, TileGeo gw, const T *__restrict__ W, int level,
                                                  int h, int nb, long per_bf, long total) {
  __shared__ T sh[DIAG ? RT : 1][RT + 1];  // the transposed quarter-block: sh[ii][jj] = a21(j0 + jj, i0 + ii)
  __shared__ long colJ[RT], colJh[RT], colI[DIAG ? RT : 1];
  __shared__ T wj0[RT], wj1[RT];
  const int tid = threadIdx.x, r = tid & 63, cg = (tid >> 6) * 16;
  const long wcol = rbt_col(gw, level);
  const T half = T(0.5);
  for (long wk = blockIdx.x; wk < total; wk += gridDim.x) {
    const long bf = wk / per_bf, in = wk - bf * per_bf;
    int p, q, bi, bj;
    if (DIAG) {
      p = q = (int)bf;
      tri_pair(in, bi, bj);
    } else {
      tri_pair(bf, p, q);  // strictly lower pairs: (p + 1, q)
      ++p;
      bi = (int)(in % nb);
      bj = (int)(in / nb);
    }
    const int op = p * 2 * h, oq = q * 2 * h, i0 = bi * RT, j0 = bj * RT;
    const bool same = DIAG && bi == bj;
    __syncthreads();  // (the tables and sh of the previous block are no longer read)
    if (tid < RT) {
      const int j = j0 + tid;
      if (j < h) {
        colJ[tid] = rbt_col(ga, oq + j);
        colJh[tid] = rbt_col(ga, oq + h + j);
        wj0[tid] = W[rbt_row(gw, oq + j) + wcol];
        wj1[tid] = W[rbt_row(gw, oq + h + j) + wcol];
      }
      if (DIAG && i0 + tid < h) colI[tid] = rbt_col(ga, op + i0 + tid);
    }
    __syncthreads();
    const int i = i0 + r;
    const bool irow = i < h;
    long rowI = 0, rowIh = 0, rowJh = 0;
    T r0i = T(0), r1i = T(0);
    if (irow) {
      rowI = rbt_row(ga, op + i);
      rowIh = rbt_row(ga, op + h + i);
      r0i = W[rbt_row(gw, op + i) + wcol];
      r1i = W[rbt_row(gw, op + h + i) + wcol];
    }
    if (DIAG) {
      const bool jrow = j0 + r < h;
      if (jrow) rowJh = rbt_row(ga, op + h + j0 + r);
#pragma unroll 4
      for (int k = 0; k < 16; ++k) {
        const int c = cg + k;
        if (jrow && i0 + c < h) sh[c][r] = ld_stream(A + rowJh + colI[c]);
      }
      __syncthreads();
    }
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int c = cg + k, j = j0 + c;
      if (!irow || j >= h || (DIAG && i < j)) continue;
      T *p11 = A + rowI + colJ[c], *p22 = A + rowIh + colJh[c], *p21 = A + rowIh + colJ[c];
      T *p12 = A + rowI + colJh[c];  // (p > q only: above the diagonal otherwise)
      const T a11 = ld_stream(p11), a22 = ld_stream(p22);
      T a21, a12;
      if (DIAG) {
        a21 = same ? sh[c][r] : ld_stream(p21);
        a12 = sh[r][c];
      } else {
        a21 = ld_stream(p21);
        a12 = ld_stream(p12);
      }
      const T s1 = a11 + a21, d1 = a11 - a21, s2 = a12 + a22, d2 = a12 - a22;
      const T r0j = wj0[c], r1j = wj1[c];
      const T c11 = (r0i * r0j) * ((s1 + s2) * half);
      const T c21 = (r1i * r0j) * ((d1 + d2) * half);
      const T c12 = (r0i * r1j) * ((s1 - s2) * half);
      const T c22 = (r1i * r1j) * ((d1 - d2) * half);
      st_stream(p11, c11);
      st_stream(p22, c22);
      if (DIAG) {
        if (same)
          sh[c][r] = c21;
        else
          st_stream(p21, c21);
        if (i > j) sh[r][c] = c12;
      } else {
        st_stream(p21, c21);
        st_stream(p12, c12);
      }
    }
    if (DIAG) {
      __syncthreads();
      if (j0 + r < h)
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
          const int c = cg + k;
          if (i0 + c < h) st_stream(A + rowJh + colI[c], sh[c][r]);
        }
    }
  }
}

// One level on the rows of an n x ncols image: the pair (i, i + h) of every butterfly and column.  trans: B^T x
// (y1 = r0 ((x1 + x2) c), y2 = r1 ((x1 - x2) c)), else B x (t1 = r0 x1, t2 = r1 x2, y1 = (t1 + t2) c, y2 = (t1 - t2) c),
// c = 2^(-1/2) rounded to T.
template <typename T>
__global__ __launch_bounds__(256) void k_rbt_vec(TileGeo gx, T *X, TileGeo gw, const T *__restrict__ W, int level, int h,
                                                 int trans, long half_n, long total) {
  const long wcol = rbt_col(gw, level);
  const T c = T(0.70710678118654752440);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int col = (int)(e / half_n), pr = (int)(e - (long)col * half_n);
    const int bf = pr / h, r1 = bf * 2 * h + (pr - bf * h), r2 = r1 + h;
    const long xc = rbt_col(gx, col);
    T *p1 = X + rbt_row(gx, r1) + xc, *p2 = X + rbt_row(gx, r2) + xc;
    const T x1 = *p1, x2 = *p2, w0 = W[rbt_row(gw, r1) + wcol], w1 = W[rbt_row(gw, r2) + wcol];
    T y1, y2;
    if (trans) {
      y1 = w0 * ((x1 + x2) * c);
      y2 = w1 * ((x1 - x2) * c);
    } else {
      const T t1 = w0 * x1, t2 = w1 * x2;
      y1 = (t1 + t2) * c;
      y2 = (t1 - t2) * c;
    }
    *p1 = y1;
    *p2 = y2;
  }
}

// W(r, k) <- src[r + k n] for the n x depth entries generated on the host
template <typename T>
__global__ __launch_bounds__(256) void k_rbt_put(TileGeo gw, T *W, const T *__restrict__ src, long n, long total) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int k = (int)(e / n), r = (int)(e - (long)k * n);
    W[rbt_row(gw, r) + rbt_col(gw, k)] = src[e];
  }
}

unsigned rbt_grid(long items) { return (unsigned)std::max(1L, std::min(items, 8192L)); }

}  // namespace

template <typename T>
void launch_rbt_sym(hipStream_t s, const TileGeo &ga, T *A, const TileGeo &gw, const T *W, int level) {
  const int nbf = 1 << level, h = (int)(ga.m / nbf / 2), nb = (h + RT - 1) / RT;
  if (h <= 0) return;
  const long per_d = (long)nb * (nb + 1) / 2, tot_d = per_d * nbf;
  k_rbt_pass<T, true><<<rbt_grid(tot_d), 256, 0, s>>>(ga, A, gw, W, level, h, nb, per_d, tot_d);
  const long pairs = (long)nbf * (nbf - 1) / 2, per_g = (long)nb * nb, tot_g = per_g * pairs;
  if (tot_g > 0) k_rbt_pass<T, false><<<rbt_grid(tot_g), 256, 0, s>>>(ga, A, gw, W, level, h, nb, per_g, tot_g);
}

template <typename T>
void launch_rbt_vec(hipStream_t s, const TileGeo &gx, T *X, const TileGeo &gw, const T *W, int level, bool trans) {
  const int nbf = 1 << level, h = (int)(gx.m / nbf / 2);
  const long half_n = gx.m / 2, total = half_n * gx.n;
  if (h <= 0 || total <= 0) return;
  k_rbt_vec<T><<<rbt_grid((total + 255) / 256), 256, 0, s>>>(gx, X, gw, W, level, h, trans ? 1 : 0, half_n, total);
}

template <typename T>
void launch_rbt_put(hipStream_t s, const TileGeo &gw, T *W, const T *src, long n, int depth) {
  const long total = n * depth;
  if (total > 0) k_rbt_put<T><<<rbt_grid((total + 255) / 256), 256, 0, s>>>(gw, W, src, n, total);
}

#define INSTANTIATE_RBT(T)                                                                               \
  template void launch_rbt_sym<T>(hipStream_t, const TileGeo &, T *, const TileGeo &, const T *, int);  \
  template void launch_rbt_vec<T>(hipStream_t, const TileGeo &, T *, const TileGeo &, const T *, int, bool); \
  template void launch_rbt_put<T>(hipStream_t, const TileGeo &, T *, const T *, long, int);
INSTANTIATE_RBT(double)
INSTANTIATE_RBT(float)

}  // namespace cholmi
