// The SPD expert solve (api.hip: chol_poequ_tile, chol_laqsy_tile, chol_porfs_tile, chol_posvx_tile; LAPACK DPOEQU,
// DLAQSY, DPORFS, DPOSVX) on a single-process, device-resident tile image, in the geometry of condest.hip: stored
// tiles of mbs x mbs elements of which the caller's tile is the leading mbu x mbu part, cut into 128 x 128 blocks of
// stored rows (sweep_blocks.h); entries outside the matrix are masked before they are loaded.  Every kernel is
// templated on T: the fp32 path is LAPACK's S-routine, in single precision throughout.
//
// The residual of porfs: one workgroup per stored block of the triangle (as mixed.hip's k_sym_resid) reads the block
// once and forms four products for up to 8 columns: A X and A^T X, |A| |X| and |A|^T |X| (a diagonal block made
// symmetric from its stored half).  A second pass adds the per-block partials in a fixed order, forms R = B - A X and
// W = |A||X| + |B|, the componentwise backward error of each column (an order-independent max) and the FERR weight
// vector |R| + nz eps W, both written as condest-layout vectors (v[128 b + t], zero outside the matrix).  The
// applications of A^{-1} between two residuals are condest.hip's sweeps.
#include <cfloat>

#include "cholmi_internal.h"
#include "sweep_blocks.h"

namespace cholmi {

namespace {

template <typename T>
struct Bits;
template <>
struct Bits<double> {
  __device__ static unsigned long long of(double v) { return (unsigned long long)__double_as_longlong(v); }
};
template <>
struct Bits<float> {
  __device__ static unsigned long long of(float v) { return (unsigned long long)__double_as_longlong((double)v); }
};

// IEEE 1/sqrt(d), as LAPACK's ONE / SQRT( D ).  fp32: each step in fp64, then rounded to fp32 -- for sqrt and division
// that is the correctly rounded fp32 result (53 >= 2 * 24 + 2), which the fp32 device instructions do not guarantee
__device__ __forceinline__ double inv_sqrt_rn(double d) { return __ddiv_rn(1.0, __dsqrt_rn(d)); }
__device__ __forceinline__ float inv_sqrt_rn(float d) {
  const float s = (float)__dsqrt_rn((double)d);
  return (float)__ddiv_rn(1.0, (double)s);
}

// ---------------------------------------------------------------- poequ / the range of S
constexpr int SCAN_WG = 256;

// mode 0: d = A(i,i), S(i) <- 1/sqrt(d) where d > 0; mode 1: d = S(i).  part[wg * 3 + ...] <- min d, max d, the first
// i with d <= 0 (or -1) of the workgroup's range of rows
template <typename T>
__global__ __launch_bounds__(256) void k_diag_scan(TileGeo g, const T *__restrict__ A, T *__restrict__ S, int mode,
                                                   double *__restrict__ part) {
  const long n = g.m, per = (n + SCAN_WG - 1) / SCAN_WG, lo = blockIdx.x * per, hi = min(n, lo + per);
  __shared__ T smin[256], smax[256];
  __shared__ long sbad[256];
  T mn = T(INFINITY), mx = T(-INFINITY);
  long bad = -1;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const T d = mode == 0 ? A[diag_index(g, i)] : S[col0_index(g, i)];
    mn = fmin(mn, d);
    mx = fmax(mx, d);
    if (d <= T(0) && bad < 0) bad = i;  // (ascending i per thread: its first)
    if (mode == 0) S[col0_index(g, i)] = d > T(0) ? inv_sqrt_rn(d) : d;
  }
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  sbad[threadIdx.x] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    const int t = threadIdx.x;
    if (t < o) {
      smin[t] = fmin(smin[t], smin[t + o]);
      smax[t] = fmax(smax[t], smax[t + o]);
      const long b2 = sbad[t + o];
      if (b2 >= 0 && (sbad[t] < 0 || b2 < sbad[t])) sbad[t] = b2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x * 3 + 0] = (double)smin[0];
    part[blockIdx.x * 3 + 1] = (double)smax[0];
    part[blockIdx.x * 3 + 2] = (double)sbad[0];
  }
}

// ---------------------------------------------------------------- laqsy and the row scaling
// the stored triangle of A <- (S(j) S(i)) A(i,j), LAPACK's order; tile pair blockIdx.y (I >= J: Lower tile (I, J),
// Upper tile (J, I)); nothing outside the matrix or the triangle is read or written
template <typename T>
__global__ __launch_bounds__(256) void k_laqsy(TileGeo g, int upper, T *__restrict__ A, const T *__restrict__ S) {
  int I, J;
  pair_of(blockIdx.y, I, J);
  const int ti = upper ? J : I, tj = upper ? I : J;
  T *tile = A + ((long)ti + (long)tj * g.lmt) * g.mbs * g.mbs;
  const long total = (long)g.mbu * g.mbu;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int rr = (int)(e % g.mbu), cc = (int)(e / g.mbu);
    const long gr = (long)ti * g.mbu + rr, gc = (long)tj * g.mbu + cc;
    if (gr >= g.m || gc >= g.m || (upper ? gr > gc : gr < gc)) continue;
    T *p = tile + rr + (long)cc * g.mbs;
    *p = (S[col0_index(g, gc)] * S[col0_index(g, gr)]) * *p;
  }
}

// D(i, j) <- S(i) D(i, j) over the n x ncols entries
template <typename T>
__global__ __launch_bounds__(256) void k_row_scale(TileGeo gx, T *__restrict__ D, const T *__restrict__ S) {
  const long total = gx.m * gx.n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long gi = e % gx.m;
    const int j = (int)(e / gx.m);
    const long idx = image_index(gx, gi, j);
    D[idx] = S[col0_index(gx, gi)] * D[idx];
  }
}

// ---------------------------------------------------------------- descriptor columns <-> condest-layout vectors
// V[cols.v[j] nv + e] <- D(row of e, cols.d[j]), zero outside the matrix
template <typename T>
__global__ __launch_bounds__(256) void k_gather(TileGeo gx, const T *__restrict__ D, VecCols cols, T *__restrict__ V,
                                                long nv) {
  const int j = blockIdx.y;
  T *v = V + (long)cols.v[j] * nv;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long)gridDim.x * 256) {
    const long b = e / CB;
    const int t = (int)(e % CB);
    v[e] = t < block_valid(gx, (int)b) ? D[desc_index(gx, b, t, cols.d[j])] : T(0);
  }
}

// D(row of e, cols.d[j]) <- (add: D +) V[cols.v[j] nv + e], inside the matrix only
template <typename T>
__global__ __launch_bounds__(256) void k_scatter(TileGeo gx, T *__restrict__ D, VecCols cols, const T *__restrict__ V,
                                                 long nv, int add) {
  const int j = blockIdx.y;
  const T *v = V + (long)cols.v[j] * nv;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long)gridDim.x * 256) {
    const long b = e / CB;
    const int t = (int)(e % CB);
    if (t >= block_valid(gx, (int)b)) continue;
    T *p = D + desc_index(gx, b, t, cols.d[j]);
    *p = add ? *p + v[e] : v[e];
  }
}

// V[c] <- W[c] .* V[c] for the columns c = cols.v[j] whose bit j of `mask` is set (DPORFS's diag(W))
template <typename T>
__global__ __launch_bounds__(256) void k_vec_weight(T *__restrict__ V, const T *__restrict__ W, VecCols cols,
                                                    unsigned mask, long nv) {
  const int j = blockIdx.y;
  if (!((mask >> j) & 1u)) return;
  const long off = (long)cols.v[j] * nv;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long)gridDim.x * 256)
    V[off + e] = W[off + e] * V[off + e];
}

// ---------------------------------------------------------------- the residual of porfs
// part[(((pair * 2 + kind) * 2 + q) * NR + j) * 128 + t]: kind 0 -> rows of block row P, 1 -> rows of block row Q;
// q 0 -> A X, 1 -> |A| |X|; column cols.d[j]
template <typename T, int NR>
__global__ __launch_bounds__(256) void k_porfs_resid(TileGeo ga, int upper, const T *__restrict__ A, TileGeo gx,
                                                     const T *__restrict__ X, VecCols cols, T *__restrict__ part) {
  const long pair = blockIdx.x;
  const TriBlock<T> b = tri_block<T>(ga, A, upper, pair);
  const int br = b.br, bc = b.bc, vr = b.vr, vc = b.vc;
  const bool diag = b.tri != 0;
  const int nr = cols.n;
  __shared__ T sv[NR][CB];         // X rows of the block's columns
  __shared__ T srow[4][NR][CB];    // per-wave row products (A X, then |A| |X|)
  __shared__ T scol[2][NR][CB];    // the column products (A^T X, |A|^T |X|)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = 2 * lane;
  for (int e = tid; e < NR * CB; e += 256) {
    const int j = e / CB, c = e % CB;
    sv[j][c] = (c < vc && j < nr) ? X[desc_index(gx, bc, c, cols.d[j])] : T(0);
  }
  T u[2][NR];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < NR; ++j) u[k][j] = (r + k < vr && j < nr) ? X[desc_index(gx, br, r + k, cols.d[j])] : T(0);
  __syncthreads();
  T racc[2][NR], aacc[2][NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) racc[0][j] = racc[1][j] = aacc[0][j] = aacc[1][j] = T(0);
  constexpr int GRP = 64 / NR;  // lanes that end with the same column product
#pragma unroll 4
  for (int k = 0; k < 32; ++k) {
    const int c = w * 32 + k;
    T t0, t1;
    load_pair<T>(b.S, ga.mbs, r, c, vr, vc, b.tri, t0, t1);
    // the row products take the stored half with the diagonal, the column products the strict half
    const T ca0 = (diag && r == c) ? T(0) : t0, ca1 = (diag && r + 1 == c) ? T(0) : t1;
    T ps[NR], pa[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const T v = sv[j][c];
      racc[0][j] = fma(t0, v, racc[0][j]);
      racc[1][j] = fma(t1, v, racc[1][j]);
      aacc[0][j] = fma(fabs(t0), fabs(v), aacc[0][j]);
      aacc[1][j] = fma(fabs(t1), fabs(v), aacc[1][j]);
      ps[j] = fma(ca1, u[1][j], ca0 * u[0][j]);
      pa[j] = fma(fabs(ca1), fabs(u[1][j]), fabs(ca0) * fabs(u[0][j]));
    }
    int js, ja;
    const T s = wave_sum_n<T, NR>(ps, lane, &js), sa = wave_sum_n<T, NR>(pa, lane, &ja);
    if (lane % GRP == 0) scol[0][js][c] = s, scol[1][ja][c] = sa;
  }
  // Lower: the row products go to the rows of P (kind 0), the column products to those of Q; Upper the other way round
  const int krow = upper ? 1 : 0, kcol = 1 - krow;
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      srow[w][j][r] = q ? aacc[0][j] : racc[0][j];
      srow[w][j][r + 1] = q ? aacc[1][j] : racc[1][j];
    }
    __syncthreads();
    T *prow = part + ((pair * 2 + krow) * 2 + q) * NR * CB;
    for (int e = tid; e < NR * CB; e += 256) {
      const int j = e / CB, t = e % CB;
      prow[e] = ((srow[0][j][t] + srow[1][j][t]) + srow[2][j][t]) + srow[3][j][t];
    }
    __syncthreads();
  }
  T *pcol = part + ((pair * 2 + kcol) * 2) * NR * CB;  // (scol is complete: the loop above ends on a barrier)
  for (int e = tid; e < NR * CB; e += 256) {
    pcol[e] = scol[0][e / CB][e % CB];
    pcol[NR * CB + e] = scol[1][e / CB][e % CB];
  }
}

// R = B - A X and W = |B| + |A| |X| per stored row, the partials added in the fixed order of for_row_partials;
// R[v nv + s] <- R, F[v nv + s] <- the FERR weight, berr[v] <- max of the
// componentwise ratio (bits of a non-negative double: order-independent), v = cols.v[j]
template <typename T, int NR>
__global__ __launch_bounds__(256) void k_porfs_reduce(TileGeo ga, TileGeo gx, const T *__restrict__ part, VecCols cols,
                                                      const T *__restrict__ B, T *__restrict__ R, T *__restrict__ F,
                                                      long nv, T nzeps, T safe1, T safe2,
                                                      unsigned long long *berr) {
  const int NB = ga.lmt * bpt_of(ga);
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (s >= (long)NB * CB) return;
  const int P = (int)(s / CB), t = (int)(s % CB);
  const long vo = (long)cols.v[j] * nv + s;
  if (t >= block_valid(ga, P)) {
    R[vo] = T(0);
    F[vo] = T(0);
    return;
  }
  T sum = 0, asum = 0;
  for_row_partials(P, NB, [&](long pair, int kind) {
    const T *p = part + ((pair * 2 + kind) * 2) * NR * CB + j * CB + t;
    sum += p[0];
    asum += p[NR * CB];
  });
  const T b = B[desc_index(gx, P, t, cols.d[j])];
  const T rv = b - sum, wv = fabs(b) + asum, ar = fabs(rv);
  const T ratio = wv > safe2 ? ar / wv : (ar + safe1) / (wv + safe1);
  atomicMax(berr + cols.v[j], Bits<T>::of(ratio));
  R[vo] = rv;
  F[vo] = wv > safe2 ? ar + nzeps * wv : ar + nzeps * wv + safe1;
}

template <typename T, int NR>
void porfs_pass(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gx, const T *X, const T *B,
                const VecCols &cols, T *part, T *R, T *F, double eps, double safe1, double safe2,
                unsigned long long *berr) {
  const long NB = block_rows(ga), pairs = tri_pairs(ga);
  const long nv = (long)condest_vec_elems(ga);
  if (!pairs) return;
  hipLaunchKernelGGL((k_porfs_resid<T, NR>), dim3((unsigned)pairs), dim3(256), 0, s, ga, upper, A, gx, X, cols, part);
  const T nz = T(ga.m + 1);
  hipLaunchKernelGGL((k_porfs_reduce<T, NR>), dim3((unsigned)((NB * CB + 255) / 256), (unsigned)cols.n), dim3(256), 0, s,
                     ga, gx, part, cols, B, R, F, nv, T(nz * T(eps)), T(safe1), T(safe2), berr);
}

unsigned grid_over(long total) { return (unsigned)std::max(1L, std::min((total + 255) / 256, 4096L)); }

}  // namespace

// ---------------------------------------------------------------- launchers
int refine_width(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

size_t porfs_part_elems(const TileGeo &ga, int width) { return (size_t)tri_pairs(ga) * 4 * CB * width; }

size_t diag_scan_part_bytes() { return (size_t)SCAN_WG * 3 * sizeof(double); }

template <typename T>
void launch_diag_scan(hipStream_t s, const TileGeo &g, const T *A, T *S, int mode, double *part) {
  hipLaunchKernelGGL(k_diag_scan<T>, dim3(SCAN_WG), dim3(256), 0, s, g, A, S, mode, part);
}

template <typename T>
void launch_laqsy(hipStream_t s, const TileGeo &g, int upper, T *A, const T *S) {
  const long nt = g.lmt, pairs = nt * (nt + 1) / 2;
  if (!pairs) return;
  const unsigned gx = grid_over((long)g.mbu * g.mbu) > 64 ? 64 : grid_over((long)g.mbu * g.mbu);
  hipLaunchKernelGGL(k_laqsy<T>, dim3(gx, (unsigned)pairs), dim3(256), 0, s, g, upper, A, S);
}

template <typename T>
void launch_row_scale(hipStream_t s, const TileGeo &gx, T *D, const T *S) {
  if (gx.m * gx.n > 0) hipLaunchKernelGGL(k_row_scale<T>, dim3(grid_over(gx.m * gx.n)), dim3(256), 0, s, gx, D, S);
}

template <typename T>
void launch_gather(hipStream_t s, const TileGeo &gx, const T *D, const VecCols &cols, T *V) {
  const long nv = (long)condest_vec_elems(gx);
  if (cols.n > 0) hipLaunchKernelGGL(k_gather<T>, dim3(grid_over(nv), (unsigned)cols.n), dim3(256), 0, s, gx, D, cols, V, nv);
}

template <typename T>
void launch_scatter(hipStream_t s, const TileGeo &gx, T *D, const VecCols &cols, const T *V, bool add) {
  const long nv = (long)condest_vec_elems(gx);
  if (cols.n > 0)
    hipLaunchKernelGGL(k_scatter<T>, dim3(grid_over(nv), (unsigned)cols.n), dim3(256), 0, s, gx, D, cols, V, nv, add ? 1 : 0);
}

template <typename T>
void launch_vec_weight(hipStream_t s, const TileGeo &g, T *V, const T *W, const VecCols &cols, unsigned mask) {
  const long nv = (long)condest_vec_elems(g);
  if (cols.n > 0 && mask)
    hipLaunchKernelGGL(k_vec_weight<T>, dim3(grid_over(nv), (unsigned)cols.n), dim3(256), 0, s, V, W, cols, mask, nv);
}

template <typename T>
void launch_porfs_resid(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gx, const T *X,
                        const T *B, const VecCols &cols, T *part, T *R, T *F, double eps, double safe1, double safe2,
                        unsigned long long *berr) {
  with_width(cols.n, [&](auto w) {
    porfs_pass<T, decltype(w)::value>(s, ga, upper, A, gx, X, B, cols, part, R, F, eps, safe1, safe2, berr);
  });
}

#define INSTANTIATE_REFINE(T)                                                                                        \
  template void launch_diag_scan<T>(hipStream_t, const TileGeo &, const T *, T *, int, double *);                    \
  template void launch_laqsy<T>(hipStream_t, const TileGeo &, int, T *, const T *);                                  \
  template void launch_row_scale<T>(hipStream_t, const TileGeo &, T *, const T *);                                   \
  template void launch_gather<T>(hipStream_t, const TileGeo &, const T *, const VecCols &, T *);                     \
  template void launch_scatter<T>(hipStream_t, const TileGeo &, T *, const VecCols &, const T *, bool);              \
  template void launch_vec_weight<T>(hipStream_t, const TileGeo &, T *, const T *, const VecCols &, unsigned);       \
  template void launch_porfs_resid<T>(hipStream_t, const TileGeo &, int, const T *, const TileGeo &, const T *,      \
                                      const T *, const VecCols &, T *, T *, T *, double, double, double,            \
                                      unsigned long long *);
INSTANTIATE_REFINE(double)
INSTANTIATE_REFINE(float)

}  // namespace cholmi
