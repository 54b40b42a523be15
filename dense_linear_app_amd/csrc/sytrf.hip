// The kernels of chol_sytrf_nopiv_tile / chol_sytrs_nopiv_tile (spd.hip: A = L D L^T without pivoting, Lower) that are
// not the trailing update's: the factorisation of one diagonal tile in 128-block steps, the scaling of a solved panel
// by D^{-1}, the staging of the diagonal tiles for the solve, and the reductions behind chol_last_sytrf_stats.
//
// Block step s of a diagonal tile (e x e, ld e; r: the 128-blocks below s inside the tile):
//   k_ldl_block   A(s,s) = L D L^T in place, one workgroup, the block in LDS.  Column j, left-looking:
//                     w(i,j) = a(i,j) - sum_{p<j} w(i,p) l(j,p),  d_j = w(j,j),  l(i,j) = w(i,j) (1 / d_j)
//                 (the reciprocal is formed once per pivot and multiplied, as LAPACK DSYTF2's r1 = 1 / d).  Also
//                 leaves the unit lower triangular L of the block in a compact 128 x 128 image for its inversion.
//   (launch_invert_diag on that image: X = L(s,s)^{-1})
//   k_ldl_rows    W(r,s) = A(r,s) X^T into scratch, A(r,s) <- L(r,s) = W(r,s) D_s^{-1}
//   k_ldl_intile  A(r,c) -= W(r,s) L(c,s)^T for s < c <= r (the lower triangle only of the blocks r == c)
// The products are NT forms of inverse.hip's register block core (nn_blocks.h): one workgroup sums a 128 x 128 block
// in a fixed order, so a repeated call returns the same bits.  Nothing here uses a floating-point atomic.
#include "nn_blocks.h"

namespace cholmi {

namespace {

constexpr int LDL_SLOTS = 2048;  // partial maxima of |L| kept by the panel scaling (one per workgroup)
constexpr int LDL_TSLOTS = 4096;  // ... and by the diagonal tiles (one per tile column of entries; tiles up to 4096)

// acc += A(i0 .. i0+63, kb .. ke) B(j0 .. j0+63, kb .. ke)^T; A(r,k) at A[r + k lda], B(c,k) at B[c + k ldb]; kb, ke
// multiples of 16.  TRB: B is lower triangular (B(c,k) = 0 for k > c), whatever its other triangle holds.
template <typename T, bool TRB>
__device__ __forceinline__ void nt_acc(const T *__restrict__ A, int lda, const T *__restrict__ B, int ldb, int i0,
                                       int j0, int kb, int ke, Acc<T> &acc) {
  const int lane = threadIdx.x & 63, c = lane & 15, g4 = (lane >> 4) * 4;
  for (int k0 = kb; k0 < ke; k0 += 16) {
    T xa[4][4], xb[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int s = 0; s < 4; ++s) xa[a][s] = A[(i0 + 16 * a + c) + (long)(k0 + g4 + s) * lda];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = j0 + 16 * b + c;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + g4 + s;
        xb[b][s] = B[col + (long)k * ldb];
        if (TRB && k > col) xb[b][s] = T(0);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = Tr<T>::mfma(xb[b][s], xa[a][s], acc[a][b]);
  }
}

// the largest value of a workgroup's threads (256 or fewer), in thread 0; NaNs are ignored
template <typename T>
__device__ __forceinline__ T block_max(T v, T *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < nw; ++i) v = fmax(v, red[i]);
  return v;
}

// One 128 x 128 diagonal block: A = L D L^T in place (D on the diagonal, L below it, the strict upper triangle not
// touched).  Lc (ld 128) <- the unit lower triangular L, zeros above; dv, rv <- d_j and 1 / d_j.  *info <- info_base + j
// (1-based) at the first pivot that is zero or not finite, unless an earlier block raised it; a block that fails, or
// that follows a failure, leaves the identity in Lc (what follows in the tile is arithmetic on unspecified data).
template <typename T>
__global__ __launch_bounds__(128) void k_ldl_block(T *A, int ld, T *__restrict__ Lc, T *__restrict__ dv,
                                                   T *__restrict__ rv, int *info, int info_base) {
  extern __shared__ __align__(16) unsigned char ldl_lds[];
  T *S = reinterpret_cast<T *>(ldl_lds), *u = S + MACRO * MACRO, *r = u + MACRO;
  __shared__ int bad;
  const int i = threadIdx.x;
  if (*info != 0) {
    for (int c = 0; c < MACRO; ++c) Lc[i + c * MACRO] = i == c ? T(1) : T(0);
    dv[i] = rv[i] = T(1);
    return;
  }
  if (i == 0) bad = 0;
#pragma unroll 16
  for (int c = 0; c < MACRO; ++c) S[i + c * MACRO] = i >= c ? A[i + (long)c * ld] : T(0);
  __syncthreads();
  for (int j = 0; j < MACRO; ++j) {
    if (i < j) u[i] = S[j + i * MACRO] * r[i];  // l(j,i)
    __syncthreads();
    if (i >= j) {
      T a0 = S[i + j * MACRO], a1 = T(0);
      int p = 0;
      for (; p + 1 < j; p += 2) {
        a0 -= S[i + p * MACRO] * u[p];
        a1 -= S[i + (p + 1) * MACRO] * u[p + 1];
      }
      if (p < j) a0 -= S[i + p * MACRO] * u[p];
      const T v = a0 + a1;
      S[i + j * MACRO] = v;
      if (i == j) {
        r[j] = T(1) / v;
        if (!(v != T(0) && isfinite(v)) && bad == 0) bad = j + 1;
      }
    }
    __syncthreads();
  }
  const bool ok = bad == 0;
  if (!ok && i == 0) atomicCAS(info, 0, info_base + bad);
#pragma unroll 8
  for (int c = 0; c < MACRO; ++c) {
    const T w = S[i + c * MACRO], l = w * r[c] + T(0);  // (+ 0: a zero of the padding times a negative 1 / d stays +0)
    if (i >= c) A[i + (long)c * ld] = i == c ? w : l;
    Lc[i + c * MACRO] = i == c ? T(1) : (ok && i > c ? l : T(0));
  }
  dv[i] = S[i + i * MACRO];
  rv[i] = r[i];
}

// the 64 x 64 quarter of wave w of a 128 x 128 block
__device__ __forceinline__ void ldl_quarter(int &i0, int &j0) {
  const int w = threadIdx.x >> 6;
  i0 = 64 * (w & 1);
  j0 = 64 * (w >> 1);
}

// W(r,s) = A(r,s) X^T for the blocks r = s + 1 + blockIdx.x of the tile (ld e), X (ld 128) lower triangular; W into the
// same place of the scratch tile Wt, A(r,s) <- W(r,s) diag(rv): L
template <typename T>
__global__ __launch_bounds__(256, 2) void k_ldl_rows(T *tile, int e, int s, const T *__restrict__ X,
                                                     const T *__restrict__ rv, T *__restrict__ Wt) {
  int i0, j0;
  ldl_quarter(i0, j0);
  const long at0 = (long)(s + 1 + blockIdx.x) * MACRO + (long)s * MACRO * e;
  Acc<T> acc;
  acc_zero<T>(acc);
  nt_acc<T, true>(tile + at0, e, X, MACRO, i0, j0, 0, j0 + 64, acc);  // (columns j0 .. j0+63 of X^T end at row j0 + 63)
  __syncthreads();  // every wave has read the block before any of it is overwritten
  const int lane = threadIdx.x & 63, c = lane & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = j0 + 16 * b + Tr<T>::drow(lane, q);
        const long at = at0 + (i0 + 16 * a + c) + (long)col * e;
        Wt[at] = acc[a][b][q];
        tile[at] = acc[a][b][q] * rv[col] + T(0);  // (+ 0: the zeros of the padding stay +0)
      }
}

// A(r,c) -= W(r,s) L(c,s)^T for the pairs s < c <= r of the tile, pair blockIdx.x in the order (s+1,s+1), (s+2,s+1),
// (s+2,s+2), ...; W from the scratch tile, L from the tile itself
template <typename T>
__global__ __launch_bounds__(256, 2) void k_ldl_intile(T *tile, int e, int s, const T *__restrict__ Wt) {
  int r = 0, cc = blockIdx.x;
  while (cc > r) {
    cc -= r + 1;
    ++r;
  }
  r += s + 1;
  cc += s + 1;
  int i0, j0;
  ldl_quarter(i0, j0);
  if (r == cc && i0 + 63 < j0) return;  // (wholly above the diagonal)
  const long sc = (long)s * MACRO * e;
  Acc<T> acc;
  acc_zero<T>(acc);
  nt_acc<T, false>(Wt + (long)r * MACRO + sc, e, tile + (long)cc * MACRO + sc, e, i0, j0, 0, MACRO, acc);
  T *C = tile + (long)r * MACRO + (long)cc * MACRO * e;
  const int lane = threadIdx.x & 63, c = lane & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = i0 + 16 * a + c, col = j0 + 16 * b + Tr<T>::drow(lane, q);
        if (r == cc && row < col) continue;
        C[row + (long)col * e] -= acc[a][b][q];
      }
}

// pm[column] <- max(pm[column], the largest |L| of the column below the diagonal) for the e columns of a factored tile
template <typename T>
__global__ __launch_bounds__(256) void k_ldl_tile_lmax(const T *__restrict__ tile, int e, double *pm) {
  __shared__ T red[4];
  const int col = blockIdx.x;
  T v = T(0);
  for (int row = col + 1 + threadIdx.x; row < e; row += 256) v = fmax(v, fabs(tile[row + (long)col * e]));
  v = block_max<T>(v, red);
  if (threadIdx.x == 0) pm[col] = fmax(pm[col], (double)v);
}

// the solved panel W (total elements: whole tiles of bs, ld e) -> Wscr, and W diag(rv) -> W in place: L.  16-byte
// accesses; pm[workgroup] <- max(pm[workgroup], the largest |L| it wrote)
template <typename T>
__global__ __launch_bounds__(256) void k_ldl_scale(T *__restrict__ W, T *__restrict__ Wscr, long total, long bs, int e,
                                                   const T *__restrict__ rv, double *pm) {
  using vec_t = T __attribute__((ext_vector_type(16 / sizeof(T))));
  constexpr int V = 16 / sizeof(T);
  __shared__ T red[4];
  T m = T(0);
  for (long x = ((long)blockIdx.x * 256 + threadIdx.x) * V; x < total; x += (long)gridDim.x * 256 * V) {
    vec_t w = *reinterpret_cast<const vec_t *>(W + x);
    *reinterpret_cast<vec_t *>(Wscr + x) = w;
    const T rr = rv[(x % bs) / e];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      w[q] = w[q] * rr + T(0);  // (+ 0: the zeros of the padding stay +0 under a negative 1 / d)
      m = fmax(m, fabs(w[q]));
    }
    *reinterpret_cast<vec_t *>(W + x) = w;
  }
  m = block_max<T>(m, red);
  if (threadIdx.x == 0) pm[blockIdx.x] = fmax(pm[blockIdx.x], (double)m);
}

// out[0..4] <- the number of positive and of negative pivots, min |d|, max |d| over the rows 0 .. n-1 (row g at
// dv[(g / mb) e + g % mb]: the padding is not counted), and the largest of the npm partial maxima; one workgroup, a
// fixed tree
template <typename T>
__global__ __launch_bounds__(256) void k_ldl_stats(const T *__restrict__ dv, long n, int mb, int e,
                                                   const double *__restrict__ pm, int npm, double *out) {
  __shared__ double sp[256], sn[256], smin[256], smax[256], sl[256];
  const int t = threadIdx.x;
  double np = 0, nn = 0, dmin = INFINITY, dmax = 0, lm = 0;
  for (long g = t; g < n; g += 256) {
    const double d = (double)dv[(g / mb) * e + g % mb];
    np += d > 0;
    nn += d < 0;
    dmin = fmin(dmin, fabs(d));
    dmax = fmax(dmax, fabs(d));
  }
  for (int i = t; i < npm; i += 256) lm = fmax(lm, pm[i]);
  sp[t] = np, sn[t] = nn, smin[t] = dmin, smax[t] = dmax, sl[t] = lm;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      sp[t] += sp[t + h];
      sn[t] += sn[t + h];
      smin[t] = fmin(smin[t], smin[t + h]);
      smax[t] = fmax(smax[t], smax[t + h]);
      sl[t] = fmax(sl[t], sl[t + h]);
    }
    __syncthreads();
  }
  if (t == 0) out[0] = sp[0], out[1] = sn[0], out[2] = smin[0], out[3] = smax[0], out[4] = sl[0];
}

// U(t) <- the diagonal tile t of the factor with a unit diagonal and zeros above it, rv <- 1 / d; tile t = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256) void k_ldl_stage(const T *__restrict__ A, long dstride, long bs, int e,
                                                   T *__restrict__ U, T *__restrict__ rv) {
  const int t = blockIdx.y;
  const T *D = A + t * dstride;
  for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < bs; x += (long)gridDim.x * 256) {
    const int i = (int)(x % e), j = (int)(x / e);
    const T v = i >= j ? D[x] : T(0);
    U[t * bs + x] = i == j ? T(1) : v;
    if (i == j) rv[(long)t * e + i] = T(1) / v;
  }
}

// Z (tiles of bs, ld e; tile row r of tile column i at (r + i nr) bs) <- Z diag(rv(i)): the row scaling of the
// right-hand sides on potrs's transposed image
template <typename T>
__global__ __launch_bounds__(256) void k_ldl_zscale(T *__restrict__ Z, long total, long bs, int e, int nr,
                                                    const T *__restrict__ rv) {
  for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
    const long tile = x / bs;
    Z[x] *= rv[(tile / nr) * e + (x % bs) / e];
  }
}

template <typename T>
int ldl_block_lds() {
  static const int bytes = [] {
    const int b = (MACRO * MACRO + 2 * MACRO) * (int)sizeof(T);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ldl_block<T>), hipFuncAttributeMaxDynamicSharedMemorySize, b);
    return b;
  }();
  return bytes;
}

unsigned flat_grid(long items, int cap) { return (unsigned)std::max<long>(1, std::min<long>(cap, (items + 255) / 256)); }

}  // namespace

int ldl_partials() { return LDL_SLOTS + LDL_TSLOTS; }

template <typename T>
void launch_ldl_tile(hipStream_t s, T *tile, int e, T *Wt, T *Lc, T *winv, T *dv, T *rv, int *info, int info_base,
                     double *pm) {
  const int nbm = e / MACRO, lds = ldl_block_lds<T>();
  const long blk = (long)MACRO * MACRO;
  for (int st = 0; st < nbm; ++st) {
    k_ldl_block<T><<<1, 128, lds, s>>>(tile + (long)st * MACRO * (e + 1), e, Lc + st * blk, dv + st * MACRO, rv + st * MACRO,
                                       info, info_base + st * MACRO);
    launch_invert_diag<T>(s, Lc + st * blk, MACRO, winv + st * blk);
    const int nr = nbm - 1 - st;
    if (nr > 0) {
      k_ldl_rows<T><<<nr, 256, 0, s>>>(tile, e, st, winv + st * blk, rv + st * MACRO, Wt);
      k_ldl_intile<T><<<nr * (nr + 1) / 2, 256, 0, s>>>(tile, e, st, Wt);
    }
  }
  k_ldl_tile_lmax<T><<<e, 256, 0, s>>>(tile, e, pm + LDL_SLOTS);
}

template <typename T>
void launch_ldl_scale(hipStream_t s, T *W, T *Wscr, long total, long bs, int e, const T *rv, double *pm) {
  if (total <= 0) return;
  k_ldl_scale<T><<<flat_grid(total / (16 / (long)sizeof(T)), LDL_SLOTS), 256, 0, s>>>(W, Wscr, total, bs, e, rv, pm);
}

template <typename T>
void launch_ldl_stats(hipStream_t s, const T *dv, long n, int mb, int e, const double *pm, double *out) {
  k_ldl_stats<T><<<1, 256, 0, s>>>(dv, n, mb, e, pm, LDL_SLOTS + LDL_TSLOTS, out);
}

template <typename T>
void launch_ldl_stage(hipStream_t s, const T *A, long dstride, long bs, int e, int nt, T *U, T *rv) {
  if (nt > 0) k_ldl_stage<T><<<dim3(flat_grid(bs, 256), (unsigned)nt), 256, 0, s>>>(A, dstride, bs, e, U, rv);
}

template <typename T>
void launch_ldl_zscale(hipStream_t s, T *Z, long total, long bs, int e, int nr, const T *rv) {
  if (total > 0) k_ldl_zscale<T><<<flat_grid(total, 4096), 256, 0, s>>>(Z, total, bs, e, nr, rv);
}

#define INSTANTIATE_LDL(T)                                                                                        \
  template void launch_ldl_tile<T>(hipStream_t, T *, int, T *, T *, T *, T *, T *, int *, int, double *);        \
  template void launch_ldl_scale<T>(hipStream_t, T *, T *, long, long, int, const T *, double *);                \
  template void launch_ldl_stats<T>(hipStream_t, const T *, long, int, int, const double *, double *);           \
  template void launch_ldl_stage<T>(hipStream_t, const T *, long, long, int, int, T *, T *);                     \
  template void launch_ldl_zscale<T>(hipStream_t, T *, long, long, int, int, const T *);
INSTANTIATE_LDL(double)
INSTANTIATE_LDL(float)

}  // namespace cholmi
