// The pivoted panel of the Cholesky factorisation with complete pivoting (spd.hip: chol_pstrf_tile, LAPACK DPSTRF)
// on a single-process, device-resident tile image: stored tiles of mbi x mbi elements of which the caller's tile is
// the leading mb x mb part (PsGeo, cholmi_internal.h).  Every kernel addresses the matrix by its global row and column
// (0 .. n-1), so the padding of the image (a ragged last tile, a tile edge that is not a multiple of 128) is never read
// or written here; only entries on or below the diagonal are.
//
// One pivot step j of tile column k (columns k0 .. k1-1) is two launches:
//   pivot:  p = argmax_{i >= j} d(i) from the column launch's per-chunk partial maxima (every workgroup reduces them
//           itself, in the same fixed order); stop when d(p) <= dstop or is NaN; otherwise the symmetric interchange
//           j <-> p of the trailing lower triangle, rows j and p of the tile column's finished columns, d(j) <-> d(p)
//   column: L(j,j) = sqrt(d(j)); L(i,j) = (A(i,j) - L(i,k0:j-1) L(j,k0:j-1)^T) * (1 / L(j,j)) for i > j (the GEMV
//           split over four waves, added in a fixed order); w(i) += L(i,j)^2, d(i) = dg(i) - w(i); the partial
//           maxima of d per 64-row chunk
// d is kept in LAPACK's form: dg(i) = A(i,i) at the start of the tile column, w(i) = the accumulated sum of squares
// since then.  Maxima: NaN above everything, then the larger value, then the smaller index (LAPACK's MAXLOC among
// equal values), so the result does not depend on the reduction order; no floating-point atomics anywhere, so runs
// are bit-identical.  A stop is recorded in ctl[0] (step + 1); every later launch of the tile column sees it and
// returns at once.
#include <cfloat>

#include "cholmi_internal.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libcholmi's kernels target gfx950 (MI355X) only: build with --offload-arch=gfx950"
#endif

namespace cholmi {

namespace {

constexpr int PS_CHUNK = 64;   // rows per partial maximum (one wave)
constexpr int PS_PIVOT_WGS = 64;  // workgroups of a pivot launch (the interchange is O(n))

__device__ __forceinline__ long ps_row(const PsGeo &g, long r) { return (r / g.mb) * g.bsiz + r % g.mb; }
__device__ __forceinline__ long ps_col(const PsGeo &g, long c) {
  return (c / g.mb) * (long)g.lmt * g.bsiz + (c % g.mb) * (long)g.mbi;
}
__device__ __forceinline__ long ps_at(const PsGeo &g, long r, long c) { return ps_row(g, r) + ps_col(g, c); }

// unfused products and sums: w(i) + L(i,j)^2 rounds as LAPACK's WORK(I) + A(I,J-1)**2
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }

// (av, ai) ranks before (bv, bi): an index < 0 is empty; NaN first, then the larger value, then the smaller index
template <typename T>
__device__ __forceinline__ bool ps_better(T av, int ai, T bv, int bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

// the best of one wave's 64 (v, i), in every lane
template <typename T>
__device__ __forceinline__ void ps_wave_best(T &v, int &i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ps_better(ov, oi, v, i)) v = ov, i = oi;
  }
}

// the best of the partials of chunks c0 .. nch-1, in every thread of a 256-thread workgroup
template <typename T>
__device__ __forceinline__ void ps_block_best(const T *pval, const int *pidx, long c0, long nch, T &v, int &i) {
  __shared__ T sv[4];
  __shared__ int si[4];
  v = T(0), i = -1;
  for (long c = c0 + threadIdx.x; c < nch; c += 256) {
    const T cv = pval[c];
    const int ci = pidx[c];
    if (ps_better(cv, ci, v, i)) v = cv, i = ci;
  }
  ps_wave_best(v, i);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sv[w] = v, si[w] = i;
  __syncthreads();
  v = sv[0], i = si[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (ps_better(sv[k], si[k], v, i)) v = sv[k], i = si[k];
}

// dg(i) = A(i,i), w(i) = 0 for k0 <= i < n, and the partial maxima of d = dg per chunk (one wave per chunk)
template <typename T>
__global__ __launch_bounds__(64) void k_pstrf_init(PsGeo g, const T *__restrict__ A, long k0, T *dg, T *w, T *pval,
                                                  int *pidx) {
  const long chunk = k0 / PS_CHUNK + blockIdx.x, i = chunk * PS_CHUNK + threadIdx.x;
  T v = T(0);
  int vi = -1;
  if (i >= k0 && i < g.n) {
    v = A[ps_at(g, i, i)];
    vi = (int)i;
    dg[i] = v;
    w[i] = T(0);
  }
  ps_wave_best(v, vi);
  if (threadIdx.x == 0) pval[chunk] = v, pidx[chunk] = vi;
}

// out <- the best of the partials of chunks c0 .. (one workgroup)
template <typename T>
__global__ __launch_bounds__(256) void k_pstrf_max(long c0, long nch, const T *pval, const int *pidx, T *outv,
                                                   int *outi) {
  T v;
  int i;
  ps_block_best(pval, pidx, c0, nch, v, i);
  if (threadIdx.x == 0) *outv = v, *outi = i;
}

template <typename T>
__device__ __forceinline__ void ps_swap(T *A, long a, long b) {
  const T t = A[a];
  A[a] = A[b];
  A[b] = t;
}

// pivot step j: the choice, the stop test, the interchange
template <typename T>
__global__ __launch_bounds__(256) void k_pstrf_pivot(PsGeo g, T *A, long j, long k0, T dstop, T *dg, T *w,
                                                     const T *pval, const int *pidx, int *ctl, int *pj, T *ajj) {
  // (stopped at an earlier step; read once per workgroup: workgroup 0 of this launch may set it while others start)
  __shared__ int stopped;
  if (threadIdx.x == 0) stopped = ctl[0];
  __syncthreads();
  if (stopped != 0) return;
  const long nch = (g.n + PS_CHUNK - 1) / PS_CHUNK;
  T v;
  int pi;
  ps_block_best(pval, pidx, j / PS_CHUNK, nch, v, pi);
  if (j > 0 && !(v > dstop)) {  // (a NaN candidate stops too)
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[0] = (int)(j + 1);
    return;
  }
  const long p = pi;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    pj[j] = (int)p;
    *ajj = v;
    if (p != j) {
      T t = dg[j];
      dg[j] = dg[p], dg[p] = t;
      t = w[j];
      w[j] = w[p], w[p] = t;
      A[ps_at(g, p, p)] = A[ps_at(g, j, j)];  // (A(j,j) is overwritten by the column launch)
    }
  }
  if (p == j) return;
  // the disjoint pairs: row j <-> row p of the finished columns k0 .. j-1; A(m,j) <-> A(p,m), j < m < p;
  // A(m,j) <-> A(m,p), m > p
  const long nd = j - k0, nb = p - j - 1, total = nd + nb + (g.n - p - 1);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    if (t < nd) {
      const long co = ps_col(g, k0 + t);
      ps_swap(A, ps_row(g, j) + co, ps_row(g, p) + co);
    } else if (t < nd + nb) {
      const long m = j + 1 + (t - nd);
      ps_swap(A, ps_at(g, m, j), ps_at(g, p, m));
    } else {
      const long m = p + 1 + (t - nd - nb), r = ps_row(g, m);
      ps_swap(A, r + ps_col(g, j), r + ps_col(g, p));
    }
  }
}

// column j (left-looking inside the tile column), then the candidates and their partial maxima: one 64-row chunk
// per workgroup, the GEMV's columns split over its four waves
template <typename T>
__global__ __launch_bounds__(256) void k_pstrf_column(PsGeo g, T *A, long j, long k0, const T *dg, T *w, T *pval,
                                                      int *pidx, const int *ctl, const T *ajjp) {
  if (ctl[0] != 0) return;
  __shared__ T red[4][PS_CHUNK];
  const T ljj = sqrt(*ajjp);
  const long cj = ps_col(g, j), rj = ps_row(g, j);
  if (blockIdx.x == 0 && threadIdx.x == 0) A[rj + cj] = ljj;
  const long nch = (g.n + PS_CHUNK - 1) / PS_CHUNK, chunk = (j + 1) / PS_CHUNK + blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long i = chunk * PS_CHUNK + lane;
  const bool live = i > j && i < g.n;
  const long ri = live ? ps_row(g, i) : 0;
  // columns k0 .. j-1 lie in one tile column: column c at cbase + (c - k0) mbi
  const long ncol = j - k0, q = (ncol + 3) / 4, c_lo = wv * q, c_hi = ncol < c_lo + q ? ncol : c_lo + q;
  const long cbase = ps_col(g, k0);
  T s = T(0);
  if (live) {
    const T *pa = A + ri + cbase, *pb = A + rj + cbase;
#pragma unroll 8
    for (long c = c_lo; c < c_hi; ++c) s += pa[c * g.mbi] * pb[c * g.mbi];
  }
  red[wv][lane] = s;
  __syncthreads();
  if (wv != 0) return;
  T v = T(0);
  int vi = -1;
  if (live) {
    const T dot = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    T *pij = A + ri + cj;
    const T l = mul_rn(sub_rn(*pij, dot), T(1) / ljj);
    *pij = l;
    const T wi = add_rn(w[i], mul_rn(l, l));
    w[i] = wi;
    v = sub_rn(dg[i], wi);
    vi = (int)i;
  }
  ps_wave_best(v, vi);
  if (lane == 0 && chunk < nch) pval[chunk] = v, pidx[chunk] = vi;
}

// the interchanges of one tile column applied to columns 0 .. ncols-1 at once: row rows[t] <- row rows[m + t] (the
// composed permutation; both lists name the same m rows), one workgroup per column
template <typename T>
__global__ __launch_bounds__(256) void k_pstrf_laswp(PsGeo g, T *A, const int *rows, int m) {
  extern __shared__ unsigned char ps_smem[];
  T *buf = reinterpret_cast<T *>(ps_smem);
  const long co = ps_col(g, blockIdx.x);
  for (int t = threadIdx.x; t < m; t += 256) buf[t] = A[ps_row(g, rows[m + t]) + co];
  __syncthreads();
  for (int t = threadIdx.x; t < m; t += 256) A[ps_row(g, rows[t]) + co] = buf[t];
}

// A(r,c) <-> A(c,r) for every r > c (an image whose tile edge is not a multiple of 64: a single tile)
template <typename T>
__global__ __launch_bounds__(256) void k_pstrf_transpose(PsGeo g, T *A) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, r = e % g.n, c = e / g.n;
  if (c < g.n && r > c) ps_swap(A, ps_at(g, r, c), ps_at(g, c, r));
}

}  // namespace

long pstrf_chunks(long n) { return (n + PS_CHUNK - 1) / PS_CHUNK; }

template <typename T>
void launch_pstrf_init(hipStream_t s, const PsGeo &g, const T *A, long k0, T *dg, T *w, T *pval, int *pidx) {
  const long nb = pstrf_chunks(g.n) - k0 / PS_CHUNK;
  if (nb > 0) k_pstrf_init<T><<<dim3((unsigned)nb), dim3(64), 0, s>>>(g, A, k0, dg, w, pval, pidx);
}

template <typename T>
void launch_pstrf_max(hipStream_t s, const PsGeo &g, long c0, const T *pval, const int *pidx, T *outv, int *outi) {
  k_pstrf_max<T><<<1, 256, 0, s>>>(c0, pstrf_chunks(g.n), pval, pidx, outv, outi);
}

template <typename T>
void launch_pstrf_step(hipStream_t s, const PsGeo &g, T *A, long j, long k0, T dstop, T *dg, T *w, T *pval, int *pidx,
                       int *ctl, int *pj, T *ajj) {
  // the interchange has at most (j - k0) + (n - j - 2) pairs
  const long pairs = (j - k0) + g.n - j, wgs = std::min<long>(PS_PIVOT_WGS, std::max<long>(1, (pairs + 255) / 256));
  k_pstrf_pivot<T><<<dim3((unsigned)wgs), dim3(256), 0, s>>>(g, A, j, k0, dstop, dg, w, pval, pidx, ctl, pj, ajj);
  const long cols = std::max<long>(1, pstrf_chunks(g.n) - (j + 1) / PS_CHUNK);
  k_pstrf_column<T><<<dim3((unsigned)cols), dim3(256), 0, s>>>(g, A, j, k0, dg, w, pval, pidx, ctl, ajj);
}

template <typename T>
void launch_pstrf_laswp(hipStream_t s, const PsGeo &g, T *A, long ncols, const int *rows, int m) {
  if (ncols > 0 && m > 0)
    k_pstrf_laswp<T><<<dim3((unsigned)ncols), dim3(256), (size_t)m * sizeof(T), s>>>(g, A, rows, m);
}

template <typename T>
void launch_pstrf_transpose(hipStream_t s, const PsGeo &g, T *A) {
  const long e = g.n * g.n;
  if (e > 0) k_pstrf_transpose<T><<<dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s>>>(g, A);
}

#define PSTRF_INST(T)                                                                                                  \
  template void launch_pstrf_init<T>(hipStream_t, const PsGeo &, const T *, long, T *, T *, T *, int *);              \
  template void launch_pstrf_max<T>(hipStream_t, const PsGeo &, long, const T *, const int *, T *, int *);            \
  template void launch_pstrf_step<T>(hipStream_t, const PsGeo &, T *, long, long, T, T *, T *, T *, int *, int *,     \
                                     int *, T *);                                                                     \
  template void launch_pstrf_laswp<T>(hipStream_t, const PsGeo &, T *, long, const int *, int);                       \
  template void launch_pstrf_transpose<T>(hipStream_t, const PsGeo &, T *);
PSTRF_INST(double)
PSTRF_INST(float)
#undef PSTRF_INST

}  // namespace cholmi
