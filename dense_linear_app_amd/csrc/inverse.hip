// The tiled triangular inverse X = L^{-1} of chol_trtri_tile / chol_potri_tile / chol_poinv_tile (api.hip), in place
// over the lower tiles of a single-process stored tile image.
//
// One recursion serves two levels.  For a lower block-triangular matrix with n blocks of edge E whose diagonal
// blocks are already inverted (Xd(i) = L(i,i)^{-1}), column c of the inverse below the diagonal is
//     X(i,c) = - sum_{c < m <= i} X(i,m) Y(m),   Y(m) = L(m,c) Xd(c),     i > c,
// which needs only the columns to its right: the columns are done from c = n - 2 down to 0 (LAPACK dtrtri's
// order), each in two batched launches, Y for every m of the column (k_tri_y) and then X for every i (k_tri_x,
// in place over L(i,c), which no product reads any more once Y is formed).
//   - inner level, E = 128: the blocks of every diagonal tile, all tiles in one launch per column; Xd from the
//     128 x 128 inverses the diagonal-block kernel leaves (launch_invert_diag_batch), copied in at the end;
//   - tile level, E = mb: the tiles, Xd(i) the finished diagonal tiles themselves (their strict upper triangle
//     holds the caller's data: masked on read, never written).
// Both products are NN.  One workgroup owns a 128 x 128 block of the output, one wave 64 x 64 of it (4 x 4 tiles of
// the fp64 / fp32 16x16x4 MFMA, 16 accumulators).  The operands are read from L2 straight into registers, as
// verify_ops.hip's LAUUM does: per 16-deep k-chunk, lane l holds A's row (l & 15) at the four k = 4 (l >> 4) .. +3
// (four coalesced 16-lane column reads) and B's column (l & 15) at the same four k (one 16 / 32-byte vector load),
// and MFMA step s multiplies k = 4 (l >> 4) + s of both: the k order inside a chunk is permuted identically on both
// sides.  Operands are swapped (B's fragment in the MFMA's A slot), so a lane's accumulator registers hold
// consecutive ROWS of the output in consecutive lanes: the column-major stores are contiguous per 16 lanes.
// Every output element is summed by one lane in a fixed order: the result is bit-identical from run to run.
#include "nn_blocks.h"

namespace cholmi {

namespace {

// (q, 128-block) of a launch: blockIdx.x = q nb2 + blk, the longest sums (largest q) first
__device__ __forceinline__ void tri_job(int cnt, int nbe, int &q, int &i0, int &j0) {
  const int nb2 = nbe * nbe, blk = blockIdx.x % nb2, w = threadIdx.x >> 6;
  q = cnt - 1 - (int)(blockIdx.x / nb2);
  i0 = (blk % nbe) * 128 + 64 * (w & 1);
  j0 = (blk / nbe) * 128 + 64 * (w >> 1);
}

// Y(m) = L(m,c) Xd(c), m = c + 1 .. c + cnt, problem z = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256, 2) void k_tri_y(TriLevel<T> L, int c, int cnt) {
  int q, i0, j0;
  tri_job(cnt, L.E / 128, q, i0, j0);
  const int m = c + 1 + q, z = blockIdx.y;
  Acc<T> acc;
  acc_zero<T>(acc);
  nn_acc<T, false, true>(L.base + z * L.sz + m * L.si + c * L.sj, L.ld, L.dg + z * L.dsz + c * L.dsi, L.dld, i0, j0,
                         j0, L.E, acc);
  acc_store<T>(L.y + z * L.ysz + m * L.ysi, L.E, i0, j0, acc, T(1));
}

// X(i,c) = - sum_{c < m <= i} X(i,m) Y(m), i = c + 1 .. c + cnt, in place over L(i,c)
template <typename T>
__global__ __launch_bounds__(256, 2) void k_tri_x(TriLevel<T> L, int c, int cnt) {
  int q, i0, j0;
  tri_job(cnt, L.E / 128, q, i0, j0);
  const int i = c + 1 + q, z = blockIdx.y;
  T *row = L.base + z * L.sz + i * L.si;
  const T *y = L.y + z * L.ysz;
  Acc<T> acc;
  acc_zero<T>(acc);
  for (int m = c + 1; m < i; ++m) nn_acc<T, false, false>(row + m * L.sj, L.ld, y + m * L.ysi, L.E, i0, j0, 0, L.E, acc);
  // the diagonal term: Xd(i) lower triangular, rows i0 .. i0+63 end at column i0 + 63
  nn_acc<T, true, false>(L.dg + z * L.dsz + i * L.dsi, L.dld, y + i * L.ysi, L.E, i0, j0, 0, i0 + 64, acc);
  acc_store<T>(row + c * L.sj, L.ld, i0, j0, acc, T(-1));
}

// the lower triangle (diagonal included) of the 128 x 128 inverses into the diagonal blocks of every diagonal tile
template <typename T>
__global__ __launch_bounds__(256) void k_tri_put_diag(T *A, long tstride, int mb, const T *__restrict__ winv) {
  const int nbm = mb / 128, t = blockIdx.x / nbm, s = blockIdx.x % nbm;
  const T *w = winv + ((long)t * nbm + s) * 128 * 128;
  T *d = A + t * tstride + (long)s * 128 * (mb + 1);
  const int r = threadIdx.x & 127;
  for (int c = threadIdx.x >> 7; c < 128; c += 2)
    if (r >= c) d[r + (long)c * mb] = w[r + c * 128];
}

// *first = min over the matrix's diagonal of (1-based index where A(i,i) == 0); *first preset above any order
template <typename T>
__global__ __launch_bounds__(256) void k_diag_zero(const T *A, long tstride, int mbs, int mbu, long n, int *first) {
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n; g += (long)gridDim.x * 256) {
    const long t = g / mbu, r = g % mbu;
    if (A[t * tstride + r * (mbs + 1)] == T(0)) atomicMin(first, (int)(g + 1));
  }
}

}  // namespace

template <typename T>
void launch_tri_column(hipStream_t s, const TriLevel<T> &L, int n, int nbatch, int c) {
  const int cnt = n - 1 - c, nbe = L.E / 128;
  if (cnt <= 0 || nbatch <= 0) return;
  const dim3 grid((unsigned)(cnt * nbe * nbe), (unsigned)nbatch);
  k_tri_y<T><<<grid, 256, 0, s>>>(L, c, cnt);
  k_tri_x<T><<<grid, 256, 0, s>>>(L, c, cnt);
}

template <typename T>
void launch_tri_put_diag(hipStream_t s, T *A, long tstride, int mb, int nt, const T *winv) {
  if (nt > 0) k_tri_put_diag<T><<<(unsigned)(nt * (mb / 128)), 256, 0, s>>>(A, tstride, mb, winv);
}

template <typename T>
void launch_diag_zero(hipStream_t s, const T *A, long tstride, int mbs, int mbu, long n, int *first) {
  (void)hipMemsetAsync(first, 0x7f, sizeof(int), s);  // 0x7f7f7f7f: above any order
  if (n > 0) k_diag_zero<T><<<(unsigned)std::min<long>(1024, (n + 255) / 256), 256, 0, s>>>(A, tstride, mbs, mbu, n, first);
}

#define INSTANTIATE_I(T)                                                                     \
  template void launch_tri_column<T>(hipStream_t, const TriLevel<T> &, int, int, int);       \
  template void launch_tri_put_diag<T>(hipStream_t, T *, long, int, int, const T *);         \
  template void launch_diag_zero<T>(hipStream_t, const T *, long, int, int, long, int *);
INSTANTIATE_I(double)
INSTANTIATE_I(float)

}  // namespace cholmi
