// The kernels of chol_sygst_tile (spd.hip: LAPACK DSYGST, itype 1, Lower) that are not the trailing update's: the
// product on one diagonal tile, A(k,k) <- X A(k,k) X^T with X = L(k,k)^{-1}, and the deferred left solve
//     X(m,k) = Xd(m) (P(m,k) - sum_{k<j<m} L(m,j) X(j,k)),   k < m,   Xd(m) = L(m,m)^{-1},
// one tile row m per launch pair: Y(k) = P(m,k) - sum ... for every k (k_sg_row_y), then X(m,k) = Xd(m) Y(k) in
// place over P(m,k) (k_sg_trmm).  Row m reads only the rows above it, which earlier launch pairs finished.  Both are
// NN products on inverse.hip's block core (nn_blocks.h): one workgroup sums one 128 x 128 output block in registers,
// in a fixed order, so a repeated call returns the same bits.
#include "nn_blocks.h"

namespace cholmi {

namespace {

// the output block of a workgroup: block blockIdx.x of a job's nbe x nbe blocks, this wave's 64 x 64 quarter
__device__ __forceinline__ void sg_block(int nbe, int &i0, int &j0) {
  const int blk = blockIdx.x, w = threadIdx.x >> 6;
  i0 = (blk % nbe) * 128 + 64 * (w & 1);
  j0 = (blk / nbe) * 128 + 64 * (w >> 1);
}

// S (E x E, ld E) <- the symmetric expansion of the lower triangle of the tile D (e x e, ld e), the identity beyond e
template <typename T>
__global__ __launch_bounds__(128) void k_sg_expand(const T *__restrict__ D, int e, T *__restrict__ S, int E) {
  const int r = blockIdx.x * 128 + threadIdx.x, c = blockIdx.y;
  T v = r == c ? T(1) : T(0);
  if (r < e && c < e) v = r >= c ? D[r + (long)c * e] : D[c + (long)r * e];
  S[r + (long)c * E] = v;
}

// the lower triangle of C (E x E, ld E) into the tile D (ld e) for rows and columns < nv; then C's strict upper
// triangle <- its lower one (C symmetric: the A(k,k) that the two SYMMs of the step read)
template <typename T>
__global__ __launch_bounds__(128) void k_sg_put_diag(T *__restrict__ C, int E, T *__restrict__ D, int e, int nv) {
  const int r = blockIdx.x * 128 + threadIdx.x, c = blockIdx.y;
  if (r < c) return;
  const T v = C[r + (long)c * E];
  if (r < nv && c < nv) D[r + (long)c * e] = v;
  if (r > c) C[c + (long)r * E] = v;
}

// out(z) = X Y(z) for the E x E blocks z = blockIdx.y, X lower triangular (its strict upper triangle never read)
template <typename T>
__global__ __launch_bounds__(256, 2) void k_sg_trmm(const T *X, int ldx, const T *Y, long sy, int ldy, T *out, long so,
                                                    int ldo, int E) {
  int i0, j0;
  sg_block(E / 128, i0, j0);
  const int z = blockIdx.y;
  Acc<T> acc;
  acc_zero<T>(acc);
  // rows i0 .. i0+63 of X end at column i0 + 63
  nn_acc<T, true, false>(X, ldx, Y + z * sy, ldy, i0, j0, 0, i0 + 64, acc);
  acc_store<T>(out + z * so, ldo, i0, j0, acc, T(1));
}

// Y(k) = P(m,k) - sum_{k<j<m} L(m,j) X(j,k), k = blockIdx.y < m (the longest sums first); tile (i,j) of A and L at
// + (i + j lmt) bs, ld E; Y(k) at y + k bs
template <typename T>
__global__ __launch_bounds__(256, 2) void k_sg_row_y(const T *A, const T *L, long bs, int lmt, int E, int m, T *y) {
  int i0, j0;
  sg_block(E / 128, i0, j0);
  const int k = blockIdx.y;
  const long sj = (long)lmt * bs;
  const T *Lrow = L + m * bs;
  Acc<T> acc;
  acc_zero<T>(acc);
  for (int j = k + 1; j < m; ++j) nn_acc<T, false, false>(Lrow + j * sj, E, A + j * bs + k * sj, E, i0, j0, 0, E, acc);
  const T *P = A + m * bs + k * sj;
  T *Y = y + k * bs;
  const int lane = threadIdx.x & 63, c = lane & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long at = (i0 + 16 * a + c) + (long)(j0 + 16 * b + Tr<T>::drow(lane, r)) * E;
        Y[at] = P[at] - acc[a][b][r];
      }
}

}  // namespace

template <typename T>
void launch_sygst_diag(hipStream_t s, T *D, int e, int nv, const T *X, int E, T *S, T *W, T *C) {
  const dim3 g1((unsigned)(E / 128), (unsigned)E);
  k_sg_expand<T><<<g1, 128, 0, s>>>(D, e, S, E);
  launch_gemm_nt_batch<T>(s, S, 0, 1, X, 0, 1, W, 0, 0, E, T(1), T(0));  // W = S X^T
  const int nbe = E / 128;
  k_sg_trmm<T><<<dim3((unsigned)(nbe * nbe), 1), 256, 0, s>>>(X, E, W, 0, E, C, 0, E, E);  // C = X W
  k_sg_put_diag<T><<<g1, 128, 0, s>>>(C, E, D, e, nv);
}

template <typename T>
void launch_sygst_solve_row(hipStream_t s, T *A, const T *L, long bs, int lmt, int E, int m, const T *Xd, T *y) {
  if (m <= 0) return;
  const int nbe = E / 128;
  const dim3 grid((unsigned)(nbe * nbe), (unsigned)m);
  k_sg_row_y<T><<<grid, 256, 0, s>>>(A, L, bs, lmt, E, m, y);
  k_sg_trmm<T><<<grid, 256, 0, s>>>(Xd, E, y, bs, E, A + m * bs, (long)lmt * bs, E, E);
}

#define INSTANTIATE_SG(T)                                                                                  \
  template void launch_sygst_diag<T>(hipStream_t, T *, int, int, const T *, int, T *, T *, T *);          \
  template void launch_sygst_solve_row<T>(hipStream_t, T *, const T *, long, int, int, int, const T *, T *);
INSTANTIATE_SG(double)
INSTANTIATE_SG(float)

}  // namespace cholmi
