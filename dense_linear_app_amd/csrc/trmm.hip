// The product with one triangle of a factor (spd.hip: chol_trmm_tile, BLAS DTRMM side Left) for a few vectors, and the
// log-determinant from a factor's diagonal (chol_logdet_tile), on a single-process, device-resident tile image in the
// geometry of condest.hip: stored tiles of mbs x mbs elements of which the caller's tile is the leading mbu x mbu part,
// cut into 128 x 128 blocks of stored rows (sweep_blocks.h); entries outside the matrix and, in a diagonal block,
// outside the stored half are masked before they are loaded, so the other strict triangle may hold anything.
//
// The product is the residual pass of mixed.hip / refine.hip cut in two: one workgroup per stored block (P, Q),
// P >= Q, of the triangle reads the block once -- nontemporal, each entry is used once -- for up to 8 vectors and
// forms ONE product: the forward kind T(P,Q) x_Q, which belongs to row block P, or the transposed kind T(P,Q)^T x_P,
// which belongs to row block Q.  The products are written as per-block partial sums, every one of them on every call,
// and a second kernel adds those of a row block in ascending order of the other block index, applies alpha and
// writes B's columns: no floating-point atomics, a repeated call returns the same bits, and a column's result does
// not depend on which columns share its group.  B's columns are gathered into vectors first (refine.hip), so the
// product is safe in place.
#include "cholmi_internal.h"
#include "sweep_blocks.h"

namespace cholmi {

namespace {

// (The block product is block_product_nv of sweep_blocks.h with nontemporal loads, spelled out here: through the shared
// body three instantiations were allocated 8 VGPRs more, one wave per SIMD less.)
// part[(pair NV + j) 128 + t] <- row / column t of the product of stored block `pair` with vector j (x + j nv).
// TRANS: the block's transpose times the vector's entries of the block's rows; else the block times those of its columns
template <typename T, bool TRANS, int NV>
__global__ __launch_bounds__(256) void k_trmm_block(TileGeo g, int upper, const T *__restrict__ A,
                                                    const T *__restrict__ x, long nv, T *__restrict__ part) {
  int P, Q;
  pair_of(blockIdx.x, P, Q);
  const int br = upper ? Q : P, bc = upper ? P : Q;  // the stored block's block row and column
  const T *S = block_at<T>(g, A, br, bc);
  const int vr = block_valid(g, br), vc = block_valid(g, bc);
  const int tri = P != Q ? 0 : upper ? 2 : 1;  // a diagonal block: its stored half, the diagonal included
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = 2 * lane;
  __shared__ T so[NV][CB];
  if (!TRANS) {
    __shared__ T sv[NV][CB];
    __shared__ T red[4][NV][CB];
    for (int e = tid; e < NV * CB; e += 256) sv[e / CB][e % CB] = x[(e / CB) * nv + (long)bc * CB + e % CB];
    __syncthreads();
    T acc0[NV], acc1[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc0[j] = acc1[j] = T(0);
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1;
      load_pair_nt<T>(S, g.mbs, r, c, vr, vc, tri, a0, a1);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        acc0[j] = fma(a0, sv[j][c], acc0[j]);
        acc1[j] = fma(a1, sv[j][c], acc1[j]);
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
      so[j][t] = ((red[0][j][t] + red[1][j][t]) + red[2][j][t]) + red[3][j][t];
    }
  } else {
    T u0[NV], u1[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      u0[j] = x[j * nv + (long)br * CB + r];
      u1[j] = x[j * nv + (long)br * CB + r + 1];
    }
#pragma unroll 4
    for (int k = 0; k < 32; ++k) {
      const int c = w * 32 + k;
      T a0, a1, p[NV];
      load_pair_nt<T>(S, g.mbs, r, c, vr, vc, tri, a0, a1);
#pragma unroll
      for (int j = 0; j < NV; ++j) p[j] = fma(a1, u1[j], a0 * u0[j]);
      int js;
      const T s = wave_sum_n<T, NV>(p, lane, &js);
      if (lane % (64 / NV) == 0) so[js][c] = s;
    }
  }
  __syncthreads();
  T *out = part + (long)blockIdx.x * NV * CB;
  for (int e = tid; e < NV * CB; e += 256) out[e] = so[e / CB][e % CB];
}

// B(row t of block P, cols.d[j]) <- alpha (the sum of row block P's partials of vector j): fwd, those of the blocks
// (P, q), q = 0 .. P; else those of (k, P), k = P .. NB-1.  Rows outside the matrix are not written
template <typename T>
__global__ __launch_bounds__(256) void k_trmm_reduce(TileGeo ga, TileGeo gx, const T *__restrict__ part, int NV, int fwd,
                                                     T alpha, VecCols cols, T *__restrict__ B) {
  const int NB = ga.lmt * bpt_of(ga);
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (s >= (long)NB * CB) return;
  const int P = (int)(s / CB), t = (int)(s % CB);
  if (t >= block_valid(ga, P)) return;
  const T *p = part + (long)j * CB + t;
  T sum = 0;
  if (fwd)
    for (int q = 0; q <= P; ++q) sum += p[((long)P * (P + 1) / 2 + q) * NV * CB];
  else
    for (int k = P; k < NB; ++k) sum += p[((long)k * (k + 1) / 2 + P) * NV * CB];
  B[desc_index(gx, P, t, cols.d[j])] = alpha * sum;
}

template <typename T, int NV>
void trmm_pass(hipStream_t s, const TileGeo &ga, int upper, int trans, const T *A, const TileGeo &gx, T *B,
               const VecCols &cols, T alpha, const T *x, T *part) {
  const long NB = block_rows(ga), pairs = tri_pairs(ga), nv = (long)condest_vec_elems(ga);
  if (!pairs) return;
  if (trans)
    hipLaunchKernelGGL((k_trmm_block<T, true, NV>), dim3((unsigned)pairs), dim3(256), 0, s, ga, upper, A, x, nv, part);
  else
    hipLaunchKernelGGL((k_trmm_block<T, false, NV>), dim3((unsigned)pairs), dim3(256), 0, s, ga, upper, A, x, nv, part);
  // the forward kind (the product belongs to row block P): L x and U^T x
  const int fwd = (upper != 0) == (trans != 0);
  hipLaunchKernelGGL(k_trmm_reduce<T>, dim3((unsigned)((NB * CB + 255) / 256), (unsigned)cols.n), dim3(256), 0, s, ga, gx,
                     part, NV, fwd, alpha, cols, B);
}

// out tile z (mb x mb) <- the lower triangle of the tile A + z tstride, zero above the diagonal (transposed: its transpose)
template <typename T>
__global__ __launch_bounds__(256) void k_tri_tiles(const T *__restrict__ A, long tstride, int mb, int transposed,
                                                   T *__restrict__ out) {
  const T *src = A + (long)blockIdx.y * tstride;
  T *dst = out + (long)blockIdx.y * mb * mb;
  const long total = (long)mb * mb;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int r = (int)(e % mb), c = (int)(e / mb);
    const T v = r >= c ? src[e] : T(0);  // (nothing above the diagonal is loaded)
    dst[transposed ? c + (long)r * mb : e] = v;
  }
}

// v <- alpha v over `total` entries (the wide product's alpha: one multiplication of every finished sum, as the narrow
// path's second kernel applies it)
template <typename T>
__global__ __launch_bounds__(256) void k_scale(T *__restrict__ v, long total, T alpha) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) v[e] = alpha * v[e];
}

// ---------------------------------------------------------------- logdet
constexpr int LOGDET_WG = 256;

// part[2 wg], part[2 wg + 1] <- the sum of log A(i,i) over the workgroup's range of rows (entries <= 0 or NaN left
// out) and the first such i (or -1); fixed order: a thread's rows ascending, then a tree over the threads
template <typename T>
__global__ __launch_bounds__(256) void k_logdet_part(TileGeo g, const T *__restrict__ A, double *__restrict__ part) {
  const long n = g.m, per = (n + LOGDET_WG - 1) / LOGDET_WG, lo = blockIdx.x * per, hi = min(n, lo + per);
  __shared__ double ssum[256];
  __shared__ long sbad[256];
  double sum = 0.0;
  long bad = -1;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const double d = (double)A[diag_index(g, i)];
    if (d > 0.0)
      sum += log(d);
    else if (bad < 0)
      bad = i;
  }
  ssum[threadIdx.x] = sum;
  sbad[threadIdx.x] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    const int t = threadIdx.x;
    if (t < o) {
      ssum[t] += ssum[t + o];
      const long b2 = sbad[t + o];
      if (b2 >= 0 && (sbad[t] < 0 || b2 < sbad[t])) sbad[t] = b2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = ssum[0];
    part[2 * blockIdx.x + 1] = (double)sbad[0];
  }
}

// out[0] <- twice the partial sums added in ascending order, out[1] <- the first bad index (the ranges ascend)
__global__ void k_logdet_sum(const double *__restrict__ part, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0, bad = -1.0;
  for (int w = 0; w < LOGDET_WG; ++w) {
    sum += part[2 * w];
    if (bad < 0 && part[2 * w + 1] >= 0) bad = part[2 * w + 1];
  }
  out[0] = 2.0 * sum;
  out[1] = bad;
}

}  // namespace

// ---------------------------------------------------------------- launchers
size_t trmm_part_elems(const TileGeo &ga, int width) { return (size_t)tri_pairs(ga) * CB * width; }

template <typename T>
void launch_trmm_narrow(hipStream_t s, const TileGeo &ga, int upper, int trans, const T *A, const TileGeo &gx, T *B,
                        const VecCols &cols, T alpha, T *x, T *part) {
  if (cols.n <= 0) return;
  launch_gather<T>(s, gx, B, cols, x);
  with_width(cols.n, [&](auto w) { trmm_pass<T, decltype(w)::value>(s, ga, upper, trans, A, gx, B, cols, alpha, x, part); });
}

template <typename T>
void launch_tri_tiles(hipStream_t s, const T *A, long tstride, int mb, int nt, bool transposed, T *out) {
  if (nt <= 0) return;
  const unsigned gx = (unsigned)std::min(((long)mb * mb + 255) / 256, 256L);
  hipLaunchKernelGGL(k_tri_tiles<T>, dim3(gx, (unsigned)nt), dim3(256), 0, s, A, tstride, mb, transposed ? 1 : 0, out);
}

template <typename T>
void launch_scale(hipStream_t s, T *v, long total, T alpha) {
  if (total > 0)
    hipLaunchKernelGGL(k_scale<T>, dim3((unsigned)std::min((total + 255) / 256, 4096L)), dim3(256), 0, s, v, total, alpha);
}

size_t logdet_part_bytes() { return (size_t)LOGDET_WG * 2 * sizeof(double); }

template <typename T>
void launch_logdet(hipStream_t s, const TileGeo &g, const T *A, double *part, double *out) {
  hipLaunchKernelGGL(k_logdet_part<T>, dim3(LOGDET_WG), dim3(256), 0, s, g, A, part);
  hipLaunchKernelGGL(k_logdet_sum, dim3(1), dim3(64), 0, s, part, out);
}

#define INSTANTIATE_TRMM(T)                                                                                          \
  template void launch_trmm_narrow<T>(hipStream_t, const TileGeo &, int, int, const T *, const TileGeo &, T *,      \
                                      const VecCols &, T, T *, T *);                                                 \
  template void launch_tri_tiles<T>(hipStream_t, const T *, long, int, int, bool, T *);                              \
  template void launch_scale<T>(hipStream_t, T *, long, T);                                                          \
  template void launch_logdet<T>(hipStream_t, const TileGeo &, const T *, double *, double *);
INSTANTIATE_TRMM(double)
INSTANTIATE_TRMM(float)

}  // namespace cholmi
