// The kernels of chol_chud_tile / chol_chdd_tile (spd.hip: LINPACK DCHUD / DCHDD, Lower): the factor of
// L L^T + sigma V V^T from L, column by column, each column rotated against every vector (chud_rot.h).  Two kernels,
// both bandwidth-bound VALU work with one lane per row:
//   k_chud_gen    one workgroup on the diagonal block of (at most) 128 columns: row j's lane makes the pivots of column
//                 j from L_jj and row j of V, one after another; the three quotients of every rotation are divided
//                 on a lane each; the lanes of the rows below apply the rotations, broadcast through LDS.  The
//                 rotations also go to a table for the appliers.
//   k_chud_apply  the rows below such a block (the rest of the diagonal tile), or every row below the diagonal tile for
//                 all of its columns at once: a lane keeps its row of V in registers and streams its row of L column
//                 by column (consecutive lanes are consecutive rows of a column-major tile: full segments); the
//                 table is the same for every lane, and goes through LDS.
// Rows and columns outside the matrix (the padding of a ragged order or of a rounded-up tile edge) are skipped: they
// come back bit for bit.  No atomics, no reductions: a repeated call returns the same bits.
#include "cholmi_internal.h"
#include "chud_rot.h"

namespace cholmi {

namespace {

// vector t of the image, stored row r of tile row I
template <typename T>
__device__ __forceinline__ T *chud_vec(const ChudVecs<T> &V, int t, int I, int r) {
  return V.p + ((long)(t / V.mb) * V.lmt + I) * V.bs + (long)(t % V.mb) * V.ld + r;
}

// Columns c0 .. c0+nc-1 (nc <= 128) of the diagonal tile D (ld e) against the vectors V.g0 .. V.g0+rg-1: the lower
// triangle of the nc x nc diagonal block and its rows of V (tile row I); tab[(c0 + j) rg + t] <- the rotation of
// column c0 + j and vector V.g0 + t.  Column j: row j's lane makes the rg pivots one after another (each needs the
// L_jj the one before left); lane 3 t + q makes quotient q of vector t (chud_quotient) -- with a single vector row
// j's lane makes the three itself, which saves a barrier; the lanes of the rows below apply the rotations.  A pivot
// that cannot be made is recorded in info when its column (1-based, col1 + j) comes before the one already there:
// info[0] the column, info[1] the vector.  The block's entries of L are read eight columns at a time, the next eight
// while these are worked on.
template <typename T, int RG>
__global__ __launch_bounds__(128) void k_chud_gen(T *__restrict__ D, int e, int c0, int nc, ChudVecs<T> V, int I,
                                                  int rg, T sigma, T *__restrict__ tab, int *info, int col1) {
  static_assert(3 * RG <= 128, "one lane per quotient");
  constexpr bool SELF = RG == 1;
  __shared__ T piv[RG][3];  // L_jj before the rotation, v_j, rr
  __shared__ T rot[2][RG][4];  // c, s, ci, sigma s (ChudRot); SELF: the columns alternate between the halves
  __shared__ unsigned long long stop;  // the first pivot of this block that could not be made: column << 32 | vector
  const int i = threadIdx.x;
  const bool act = i < nc;
  unsigned long long bad = ~0ull;  // (this lane's)
  if (i == 0) stop = ~0ull;
  T *a = D + (c0 + i) + (long)c0 * e;
  T v[RG];
#pragma unroll
  for (int t = 0; t < RG; ++t) v[t] = act && t < rg ? *chud_vec(V, V.g0 + t, I, c0 + i) : T(0);
  T l[8], nx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) l[u] = act && u <= i ? a[(long)u * e] : T(0);
  // Every load so far has landed (s_waitcnt vmcnt(0) alone).  Without it the compiler, which cannot count the memory
  // operations in flight across the branches of the column loop, waits for all of them -- the table's stores
  // included -- at every use of v and l, on every column of the chain.
  __builtin_amdgcn_s_waitcnt(0x0f70);
  lds_barrier();
  for (int j0 = 0; j0 < nc; j0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) nx[u] = act && j0 + 8 + u <= i ? a[(long)(j0 + 8 + u) * e] : T(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u, half = SELF ? j & 1 : 0;
      if (j < nc) {  // (the same in every lane)
        if (i == j) {
#pragma unroll
          for (int t = 0; t < RG; ++t)
            if (t < rg) {
              const T ljj = l[u];
              T rr;
              if (!chud_pivot<T>(ljj, v[t], sigma, rr) && bad == ~0ull)
                bad = (unsigned long long)(col1 + j) << 32 | (unsigned)(V.g0 + t);
              l[u] = rr;
              if (SELF) {
                T *out = tab + ((long)(c0 + j) * rg + t) * 4;
#pragma unroll
                for (int q = 0; q < 3; ++q) rot[half][t][q] = out[q] = chud_quotient<T>(q, ljj, v[t], rr);
                rot[half][t][3] = out[3] = sigma * rot[half][t][1];
              } else {
                piv[t][0] = ljj, piv[t][1] = v[t], piv[t][2] = rr;
              }
            }
        }
        lds_barrier();
        if (!SELF) {
          if (i < 3 * rg) {
            const int t = i / 3, q = i - 3 * t;
            const T x = chud_quotient<T>(q, piv[t][0], piv[t][1], piv[t][2]);
            T *out = tab + ((long)(c0 + j) * rg + t) * 4;
            rot[0][t][q] = out[q] = x;
            if (q == 1) rot[0][t][3] = out[3] = sigma * x;
          }
          lds_barrier();
        }
        if (act && i > j) {
#pragma unroll
          for (int t = 0; t < RG; ++t)
            if (t < rg) chud_apply<T>(l[u], v[t], *reinterpret_cast<const ChudRot<T> *>(rot[half][t]));
        }
        // (two barriers a column: the next column's pivots and quotients are written behind the barriers that follow
        // these reads.  SELF, one barrier: column j + 1 writes the other half, and column j + 2 is made only after
        // every lane has passed the barrier of column j + 1, behind its reads of this half)
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (act && j0 + u <= i) a[(long)(j0 + u) * e] = l[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) l[u] = nx[u];
  }
  // (row j's entries of V were consumed by its own rotations: what is left of them is not part of the result)
#pragma unroll
  for (int t = 0; t < RG; ++t)
    if (act && t < rg) *chud_vec(V, V.g0 + t, I, c0 + i) = v[t];
  if (bad != ~0ull) atomicMin(&stop, bad);
  lds_barrier();
  if (i == 0 && stop != ~0ull && (info[0] == 0 || (int)(stop >> 32) < info[0]))
    info[0] = (int)(stop >> 32), info[1] = (int)(stop & 0xffffffffu);
}

// Stored rows [r0, r1) below the top of the diagonal tile of tile column k (row R: tile k + R / e, its row R % e;
// tile (k + i, k) at Acol + i bs, ld e), columns c0 .. c0+nc-1 of that tile column: the rotations tab[col rg + t]
// applied in column order.  One lane per row.  The rotations go through LDS, CHUD_STAGE columns at a time (every lane
// reads the same one), the next stage loaded while this one is used; a lane's entries of L are read UC columns at a
// time, the next UC while these are worked on: the fewer the vectors, the more columns in flight.
constexpr int CHUD_STAGE = 32;
template <typename T, int RG>
__global__ __launch_bounds__(256) void k_chud_apply(T *__restrict__ Acol, long bs, int e, int mb, long n, int k, long r0,
                                                    long r1, int c0, int nc, const T *__restrict__ tab, ChudVecs<T> V,
                                                    int rg) {
  constexpr int UC = RG <= 2 ? 32 : RG <= 8 ? 16 : 8;
  constexpr int PT = (CHUD_STAGE * RG * 4 + 255) / 256;  // table entries per lane and stage
  static_assert(CHUD_STAGE % UC == 0, "whole groups of columns per stage");
  __shared__ T rots[2][CHUD_STAGE * RG * 4];
  const long R = r0 + (long)blockIdx.x * 256 + threadIdx.x;
  const int ti = (int)(R / e), r = (int)(R - (long)ti * e), I = k + ti;
  const bool on = R < r1 && r < mb && (long)I * mb + r < n;  // (padding: not read, not written)
  T *a = Acol + ti * bs + r + (long)c0 * e;
  tab += (long)c0 * rg * 4;
  T stage[PT];
  auto load_stage = [&](int s0) {  // (beyond the last column: nothing)
    const int cnt = min(CHUD_STAGE, nc - s0) * rg * 4;
#pragma unroll
    for (int p = 0; p < PT; ++p) {
      const int x = threadIdx.x + 256 * p;
      stage[p] = x < cnt ? tab[(long)s0 * rg * 4 + x] : T(0);
    }
  };
  load_stage(0);
  T v[RG];
#pragma unroll
  for (int t = 0; t < RG; ++t) v[t] = on && t < rg ? *chud_vec(V, V.g0 + t, I, r) : T(0);
  T l[UC], nx[UC];
#pragma unroll
  for (int u = 0; u < UC; ++u) l[u] = on && u < nc ? a[(long)u * e] : T(0);
  for (int s0 = 0, half = 0; s0 < nc; s0 += CHUD_STAGE, half ^= 1) {
    const int ns = min(CHUD_STAGE, nc - s0);
    T *rs = rots[half];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
      const int x = threadIdx.x + 256 * p;
      if (x < CHUD_STAGE * RG * 4) rs[x] = stage[p];
    }
    // (one barrier per stage: the next stage goes to the other half, and the one after it is written only behind the
    // next barrier, which every lane reaches with this stage read)
    lds_barrier();
    load_stage(s0 + CHUD_STAGE);
    for (int j0 = 0; j0 < ns; j0 += UC) {
      const int j = s0 + j0;
#pragma unroll
      for (int u = 0; u < UC; ++u) nx[u] = on && j + UC + u < nc ? a[(long)(j + UC + u) * e] : T(0);
#pragma unroll
      for (int u = 0; u < UC; ++u)
        if (j0 + u < ns) {
#pragma unroll
          for (int t = 0; t < RG; ++t)
            if (t < rg) chud_apply<T>(l[u], v[t], *reinterpret_cast<const ChudRot<T> *>(&rs[((j0 + u) * rg + t) * 4]));
        }
#pragma unroll
      for (int u = 0; u < UC; ++u)
        if (on && j + u < nc) a[(long)(j + u) * e] = l[u];
#pragma unroll
      for (int u = 0; u < UC; ++u) l[u] = nx[u];
    }
  }
#pragma unroll
  for (int t = 0; t < RG; ++t)
    if (on && t < rg) *chud_vec(V, V.g0 + t, I, r) = v[t];
}

// f(the smallest instantiated register group that holds rg vectors)
template <typename F>
void chud_with_group(int rg, F f) {
  if (rg <= 1) f(std::integral_constant<int, 1>());
  else if (rg <= 2) f(std::integral_constant<int, 2>());
  else if (rg <= 4) f(std::integral_constant<int, 4>());
  else if (rg <= 8) f(std::integral_constant<int, 8>());
  else f(std::integral_constant<int, CHUD_GROUP>());
}

}  // namespace

template <typename T>
void launch_chud_gen(hipStream_t s, T *D, int e, int c0, int nc, const ChudVecs<T> &V, int I, int rg, T sigma, T *tab,
                     int *info, int col1) {
  chud_with_group(rg, [&](auto G) {
    k_chud_gen<T, decltype(G)::value>
        <<<1, 128, 0, s>>>(D, e, c0, nc, V, I, rg, sigma, tab, info, col1);
  });
}

template <typename T>
void launch_chud_apply(hipStream_t s, T *Acol, long bs, int e, int mb, long n, int k, long r0, long r1, int c0, int nc,
                       const T *tab, const ChudVecs<T> &V, int rg) {
  if (r1 <= r0 || nc <= 0) return;
  const unsigned blocks = (unsigned)((r1 - r0 + 255) / 256);
  chud_with_group(rg, [&](auto G) {
    k_chud_apply<T, decltype(G)::value><<<blocks, 256, 0, s>>>(Acol, bs, e, mb, n, k, r0, r1, c0, nc, tab, V, rg);
  });
}

#define INSTANTIATE_CHUD(T)                                                                                         \
  template void launch_chud_gen<T>(hipStream_t, T *, int, int, int, const ChudVecs<T> &, int, int, T, T *, int *, int); \
  template void launch_chud_apply<T>(hipStream_t, T *, long, int, int, long, int, long, long, int, int, const T *,     \
                                     const ChudVecs<T> &, int);
INSTANTIATE_CHUD(double)
INSTANTIATE_CHUD(float)

}  // namespace cholmi
