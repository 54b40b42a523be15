// The symmetric matrix product from one stored triangle (spd.hip: chol_symm_tile, BLAS DSYMM / SSYMM side Left):
// C <- alpha A B + beta C for the n x n symmetric A of which only the `upper` / lower triangle is stored, on
// single-process, device-resident tile images in the geometry of condest.hip (sweep_blocks.h): stored tiles of
// mbs x mbs elements cut into 128 x 128 blocks of stored rows, padding masked per entry.
//
// Owner computes: a workgroup of four waves owns one block of C -- the 128 rows of block row P and W = 16 WT columns
// -- and walks the NB blocks Q of block row P of A in ascending order, 16 values of k (one K-slice) at a time, on the
// 16x16x4 MFMA.  A(P,Q) is the stored block (P,Q) where that lies in the stored triangle and the transpose of the
// stored block (Q,P) otherwise; the diagonal block is made symmetric from its stored half.  Every entry of C is summed
// by one lane over k = 0 .. n-1 in that one order, whatever nrhs and W are: no partial buffers, no atomics, the same
// bits on every call, and every workgroup has the same length.
//
// A slice goes global -> registers -> LDS as it is stored (no transposing copy); the slice after it is in flight in
// registers while the current one is multiplied.  The two orientations differ in the LDS read map alone:
//   direct    the slice is 128 rows x 16 columns of the stored block, kept as [column][row] with pitch 128 + 16: the 32
//             lanes of one LDS cycle read rows r .. r+15 of two neighbouring columns, 16 consecutive elements and the
//             16 that lie 144 = 16 (mod 32) further on: 32 different banks (pairs of banks in fp64)
//   mirrored  the slice is 16 rows x 128 columns of the stored block (Q,P), kept as [column][row] with pitch 16 + 2:
//             the lanes read rows k, k+1 of 16 neighbouring columns, 18 c + {0, 1} (mod 32): 32 different banks again
// The slice of B (16 rows x W columns) is kept and read like a mirrored one.
//
// Masked BY SELECTION while a slice is fetched, so that nothing masked is loaded and a NaN there cannot reach an MFMA:
// entries of A outside the matrix, the unreferenced half of the diagonal block, rows of B beyond n and columns of B
// beyond nrhs.  Rows of C outside the matrix and columns beyond nrhs are not stored.
#include "cholmi_internal.h"
#include "mfma_traits.h"
#include "sweep_blocks.h"

namespace cholmi {

namespace {

constexpr int SY_KS = 16;       // the K-slice
constexpr int SY_PD = CB + 16;  // LDS pitch of a direct slice of A: [16][128 + 16]
constexpr int SY_PT = SY_KS + 2;  // ... of a mirrored slice of A and of the slice of B: [128 or W][16 + 2]
enum { SY_DIRECT = 0, SY_MIRROR = 1, SY_DIAG = 2 };

template <typename T>
__device__ __forceinline__ void load2(const T *p, T &a0, T &a1) {
  const typename V2<T>::t a = *reinterpret_cast<const typename V2<T>::t *>(p);
  a0 = a.x;
  a1 = a.y;
}

// K-slice k0 .. k0+15 of block Q: A(P, Q)'s part into va, B's rows (columns j0 .. j0+W-1) into vb.  -> how va is laid
// out: SY_DIRECT / SY_DIAG: va[2i+e] = A(row 2 (tid & 63) + e, k0 + (tid >> 6) + 4i); SY_MIRROR: va[2i+e] =
// A(row (tid >> 3) + 32i, k0 + 2 (tid & 7) + e); vb[2i+e] = B(k0 + 2 (tid & 7) + e, j0 + (tid >> 3) + 32i)
template <typename T, int W>
__device__ __forceinline__ int symm_fetch(const TileGeo &ga, const TileGeo &gb, int upper, const T *__restrict__ A,
                                          const T *__restrict__ B, int P, int Q, int k0, int vp, int vq, int j0,
                                          T (&va)[8], T (&vb)[2 * ((W + 31) / 32)]) {
  const int tid = threadIdx.x, ld = ga.mbs, nrhs = (int)gb.n;
  const int kk = k0 + 2 * (tid & 7), c8 = tid >> 3;
#pragma unroll
  for (int i = 0; i < (W + 31) / 32; ++i) {
    const int c = c8 + 32 * i, col = j0 + c;
    vb[2 * i] = vb[2 * i + 1] = T(0);
    if (c < W && col < nrhs) {
      const T *p = B + desc_index(gb, Q, kk, col);
      if (vq == CB) {
        load2<T>(p, vb[2 * i], vb[2 * i + 1]);
      } else {
        if (kk < vq) vb[2 * i] = p[0];
        if (kk + 1 < vq) vb[2 * i + 1] = p[1];
      }
    }
  }
  if (P == Q) {
    const T *S = block_at<T>(ga, A, P, P);
    const int r = 2 * (tid & 63);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = k0 + (tid >> 6) + 4 * i;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int rr = r + e;
        const bool own = upper ? rr <= c : rr >= c;  // (rr, c) lies in the stored half
        T v = T(0);
        if (rr < vp && c < vp) v = own ? S[rr + (long)c * ld] : S[c + (long)rr * ld];
        va[2 * i + e] = v;
      }
    }
    return SY_DIAG;
  }
  if (upper ? Q > P : Q < P) {
    const T *S = block_at<T>(ga, A, P, Q);
    const int r = 2 * (tid & 63);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = k0 + (tid >> 6) + 4 * i;
      const T *p = S + r + (long)c * ld;
      if (vp == CB && vq == CB) {
        load2<T>(p, va[2 * i], va[2 * i + 1]);
      } else {
        va[2 * i] = (r < vp && c < vq) ? p[0] : T(0);
        va[2 * i + 1] = (r + 1 < vp && c < vq) ? p[1] : T(0);
      }
    }
    return SY_DIRECT;
  }
  const T *S = block_at<T>(ga, A, Q, P);  // rows: k, columns: the rows of block row P
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c8 + 32 * i;
    const T *p = S + kk + (long)c * ld;
    if (vp == CB && vq == CB) {
      load2<T>(p, va[2 * i], va[2 * i + 1]);
    } else {
      va[2 * i] = (kk < vq && c < vp) ? p[0] : T(0);
      va[2 * i + 1] = (kk + 1 < vq && c < vp) ? p[1] : T(0);
    }
  }
  return SY_MIRROR;
}

// the fetched slice into LDS, as it is stored
template <typename T, int W>
__device__ __forceinline__ void symm_put(int kind, const T (&va)[8], const T (&vb)[2 * ((W + 31) / 32)], T *sA, T *sB) {
  using v2 = typename V2<T>::t;
  const int tid = threadIdx.x, k2 = 2 * (tid & 7), c8 = tid >> 3;
#pragma unroll
  for (int i = 0; i < (W + 31) / 32; ++i) {
    const int c = c8 + 32 * i;
    if (c < W) {
      v2 v;
      v.x = vb[2 * i], v.y = vb[2 * i + 1];
      *reinterpret_cast<v2 *>(sB + c * SY_PT + k2) = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v2 v;
    v.x = va[2 * i], v.y = va[2 * i + 1];
    if (kind == SY_MIRROR)
      *reinterpret_cast<v2 *>(sA + (c8 + 32 * i) * SY_PT + k2) = v;
    else
      *reinterpret_cast<v2 *>(sA + ((tid >> 6) + 4 * i) * SY_PD + 2 * (tid & 63)) = v;
  }
}

// acc += the slice in LDS: this wave's rows 32 w .. 32 w + 31 of the block against the W columns.  One body for both
// read maps of A: entry (row, k) at row SY_PT + k (mirrored) or k SY_PD + row (direct)
template <typename T, int WT>
__device__ __forceinline__ void symm_mac(bool mirror, const T *sA, const T *sB, typename Tr<T>::acc_t (&acc)[2][WT]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int row = 32 * w + c;
  const T *pa = sA + (mirror ? row * SY_PT + g : g * SY_PD + row);
  const int sk = mirror ? 4 : 4 * SY_PD, sr = mirror ? 16 * SY_PT : 16;  // the steps of 4 k and of 16 rows
  const T *pb = sB + c * SY_PT + g;
#pragma unroll
  for (int s = 0; s < SY_KS / 4; ++s) {
    T xa[2], xb[WT];
#pragma unroll
    for (int a = 0; a < 2; ++a) xa[a] = pa[s * sk + a * sr];
#pragma unroll
    for (int b = 0; b < WT; ++b) xb[b] = pb[16 * b * SY_PT + 4 * s];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < WT; ++b) acc[a][b] = Tr<T>::mfma(xb[b], xa[a], acc[a][b]);
  }
}

// grid: (column blocks of W = 16 WT, NB block rows)
template <typename T, int WT>
__global__ __launch_bounds__(256) void k_symm(TileGeo ga, TileGeo gb, TileGeo gc, int upper, const T *__restrict__ A,
                                              const T *__restrict__ B, T *__restrict__ C, T alpha, T beta) {
  constexpr int W = 16 * WT;
  const int P = blockIdx.y, j0 = blockIdx.x * W;
  const int NB = ga.lmt * bpt_of(ga), nrhs = (int)gb.n;
  const int vp = block_valid(ga, P);
  if (vp == 0) return;  // (a block of padding alone: nothing of C lies in it)
  __shared__ __attribute__((aligned(16))) T sA[SY_KS * SY_PD];
  __shared__ __attribute__((aligned(16))) T sB[W * SY_PT];
  typename Tr<T>::acc_t acc[2][WT];
  acc_zero<T, 2, WT>(acc);
  T va[8], vb[2 * ((W + 31) / 32)];
  int Q = 0, k0 = 0, vq = block_valid(ga, 0);  // (block 0 holds rows of the matrix: n >= 1)
  int kind = symm_fetch<T, W>(ga, gb, upper, A, B, P, Q, k0, vp, vq, j0, va, vb);
  for (;;) {
    __syncthreads();  // every wave is done with the slice in LDS
    symm_put<T, W>(kind, va, vb, sA, sB);
    const bool mirror = kind == SY_MIRROR;
    __syncthreads();
    // the next slice that holds rows of the matrix, ascending
    k0 += SY_KS;
    if (k0 >= vq) {
      k0 = 0;
      do {
        ++Q;
      } while (Q < NB && (vq = block_valid(ga, Q)) == 0);
    }
    const bool more = Q < NB;
    if (more) kind = symm_fetch<T, W>(ga, gb, upper, A, B, P, Q, k0, vp, vq, j0, va, vb);
    symm_mac<T, WT>(mirror, sA, sB, acc);
    if (!more) break;
  }
  // C(row, col) <- alpha sum + beta C(row, col), one fixed formula; beta == 0: C is not read
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int row = 32 * w + 16 * a + c;
    if (row >= vp) continue;
#pragma unroll
    for (int b = 0; b < WT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = j0 + 16 * b + Tr<T>::drow(lane, r);
        if (col >= nrhs) continue;
        T *p = C + desc_index(gc, P, row, col);
        const T s = acc[a][b][r];
        *p = beta == T(0) ? alpha * s : fma(alpha, s, beta * *p);
      }
  }
}

// alpha == 0: C <- beta C on the entries of the matrix (beta == 0: C <- 0, C is not read).  grid: (chunks of 64
// columns, NB block rows)
template <typename T>
__global__ __launch_bounds__(256) void k_symm_scale(TileGeo gc, T *__restrict__ C, T beta) {
  const int P = blockIdx.y, t = threadIdx.x & 127, vp = block_valid(gc, P), nrhs = (int)gc.n;
  if (t >= vp) return;
  const int hi = min(nrhs, ((int)blockIdx.x + 1) * 64);
  for (int col = blockIdx.x * 64 + (threadIdx.x >> 7); col < hi; col += 2) {
    T *p = C + desc_index(gc, P, t, col);
    *p = beta == T(0) ? T(0) : beta * *p;
  }
}

template <typename T, int WT>
void symm_launch(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gb, const T *B,
                 const TileGeo &gc, T *C, T alpha, T beta, unsigned NB) {
  const unsigned nx = (unsigned)((gb.n + 16 * WT - 1) / (16 * WT));
  hipLaunchKernelGGL((k_symm<T, WT>), dim3(nx, NB), dim3(256), 0, s, ga, gb, gc, upper, A, B, C, alpha, beta);
}

}  // namespace

// ---------------------------------------------------------------- launchers
int symm_width(long nrhs) { return nrhs <= 16 ? 16 : nrhs <= 32 ? 32 : nrhs <= 64 ? 64 : 128; }

template <typename T>
long launch_symm(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gb, const T *B,
                 const TileGeo &gc, T *C, T alpha, T beta) {
  const unsigned NB = (unsigned)(ga.lmt * (condest_edge(ga) / CB));
  if (!NB || gb.n <= 0) return 0;
  if (alpha == T(0)) {
    const unsigned nx = (unsigned)((gc.n + 63) / 64);
    hipLaunchKernelGGL(k_symm_scale<T>, dim3(nx, NB), dim3(256), 0, s, gc, C, beta);
    return (long)nx * NB;
  }
  const int W = symm_width(gb.n);
  switch (W) {
    case 16: symm_launch<T, 1>(s, ga, upper, A, gb, B, gc, C, alpha, beta, NB); break;
    case 32: symm_launch<T, 2>(s, ga, upper, A, gb, B, gc, C, alpha, beta, NB); break;
    case 64: symm_launch<T, 4>(s, ga, upper, A, gb, B, gc, C, alpha, beta, NB); break;
    default: symm_launch<T, 8>(s, ga, upper, A, gb, B, gc, C, alpha, beta, NB); break;
  }
  return (long)((gb.n + W - 1) / W) * NB;
}

#define INSTANTIATE_SYMM(T)                                                                                      \
  template long launch_symm<T>(hipStream_t, const TileGeo &, int, const T *, const TileGeo &, const T *,         \
                               const TileGeo &, T *, T, T);
INSTANTIATE_SYMM(double)
INSTANTIATE_SYMM(float)

}  // namespace cholmi
