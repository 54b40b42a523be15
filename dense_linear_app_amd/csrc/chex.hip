// The kernels of chol_chex_tile (spd.hip: LINPACK DCHEX without Z, Lower): the factor after a circular shift of the
// variables k..l.  Both jobs move the window of the factor by one row and one column along the diagonal, so a lane's
// source is another lane's destination: the host saves each tile column (ChexStage) before it is written, and every
// kernel here reads L from those copies and writes A.  Rows are 0-based below.
//   k_chex_vec    the work vector over the rows k..n-1: job 2: the moved variable's old column in the new row order
//                 (chud's vector); job 1: what each row carries into the rotations (its entry of column l, or +0)
//   k_chex_move   plain copies, one lane per row and eight columns: the rows k..l of the columns before k permuted
//                 (both jobs), and job 2's window: new column j = old column j + 1 moved up by one row, a zero in
//                 the moved variable's new row.  The rotations of job 2 are chud.hip's, on the window's columns.
//   k_chex_setcol job 2: the rotated vector becomes column l
//   k_chex_coef   job 1: the rotations from the moved row (chex_rot.h), right to left: one workgroup, 256 columns at a
//                 time; lane 0 makes the pivots one after another, then a lane per column divides the two quotients
//   k_chex_apply  job 1: one lane per row streams its row of the staged window right to left and writes it rotated
//                 one column to the right (and one row down, above l) -- the window is read once and written once;
//                 the table goes through LDS as k_chud_apply's does, what a row carries on in the work vector
// Lanes are consecutive rows of a column-major tile: full segments but for the one-row offset.  Rows and columns
// outside the matrix are neither read nor written.  No atomics on data, no reductions: the same bits on every call.
#include "cholmi_internal.h"
#include "chex_rot.h"

namespace cholmi {

namespace {

template <typename T>
__device__ __forceinline__ T *chex_at(const ChexMat<T> &M, int row, int col) {
  const int I = row / M.mb, J = col / M.mb;
  return M.A + ((long)I + (long)J * M.lmt) * M.bs + (row - I * M.mb) + (long)(col - J * M.mb) * M.e;
}
template <typename T>
__device__ __forceinline__ T *chex_w(const ChexMat<T> &M, T *w, int row) {
  const int I = row / M.mb;
  return w + (long)I * M.e + (row - I * M.mb);
}

template <typename T>
__global__ __launch_bounds__(256) void k_chex_vec(ChexMat<T> M, int k0, int l0, int job, T *__restrict__ w) {
  const long x = (long)k0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= M.n) return;
  const int i = (int)x;
  T val;
  if (job == 2) {
    val = *chex_at(M, i < l0 ? i + 1 : i == l0 ? k0 : i, k0);
  } else {
    if (i == k0) return;  // (the last pivot: k_chex_coef)
    val = i <= l0 ? T(0) : *chex_at(M, i, l0);
  }
  *chex_w(M, w, i) = val;
}

template <typename T>
__global__ __launch_bounds__(256) void k_chex_setcol(ChexMat<T> M, int l0, const T *__restrict__ w) {
  const long x = (long)l0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= M.n) return;
  *chex_at(M, (int)x, l0) = *chex_w(M, const_cast<T *>(w), (int)x);
}

// Tile column J, its columns c < c1, the stored rows [0, rows) from the top of tile row I0.  S0: the copy of tile
// column J, S1: of J + 1 (job 2's last column of a tile takes the first of the next)
constexpr int CHEX_CPT = 8;  // columns per lane
template <typename T>
__global__ __launch_bounds__(256) void k_chex_move(ChexMat<T> M, int J, int c1, int I0, int rows, int k0, int l0, int job,
                                                   ChexStage<T> S0, ChexStage<T> S1) {
  const int R = blockIdx.x * 256 + threadIdx.x;
  const int ti = R / M.e, rr = R - ti * M.e, I = I0 + ti;
  const long in = (long)I * M.mb + rr;
  if (R >= rows || rr >= M.mb || in >= M.n) return;
  const int i = (int)in;
  const bool inwin = i >= k0 && i <= l0;
  // the source row: of a column before k (a row of the window only), and of a column of job 2's window
  const int ra = job == 2 ? (i < l0 ? i + 1 : k0) : (i == k0 ? l0 : i - 1);
  const int rw = i < l0 ? i + 1 : i;
  const int Ia = ra / M.mb, Iw = rw / M.mb;
  const T *pa = S0.p + (long)(Ia - S0.row0) * M.bs + (ra - Ia * M.mb);
  const T *pw0 = S0.p + (long)(Iw - S0.row0) * M.bs + (rw - Iw * M.mb);
  const T *pw1 = S1.p + (long)(Iw - S1.row0) * M.bs + (rw - Iw * M.mb);
  T *dst = M.A + ((long)I + (long)J * M.lmt) * M.bs + rr;
  const int cbase = blockIdx.y * CHEX_CPT;
  T x[CHEX_CPT];
  bool wr[CHEX_CPT];
#pragma unroll
  for (int q = 0; q < CHEX_CPT; ++q) {
    const int c = cbase + q;
    const long j = (long)J * M.mb + c;
    x[q] = T(0);
    wr[q] = false;
    if (c >= c1) continue;
    if (j < k0) {
      wr[q] = inwin;
      if (inwin) x[q] = pa[(long)c * M.e];
    } else if (job == 2 && j < l0 && i >= j) {
      wr[q] = true;
      if (i != l0) x[q] = c + 1 < M.mb ? pw0[(long)(c + 1) * M.e] : *pw1;
    }
  }
#pragma unroll
  for (int q = 0; q < CHEX_CPT; ++q)
    if (wr[q]) dst[(long)(cbase + q) * M.e] = x[q];
}

// tab[2 (i - k0) ..] <- (cc_i, ss_i) for i = l0-1 down to k0, w[k0] <- the last pivot (the new L(k,k)); info[0] <-
// the 1-based new column i + 2 of the first rotation (in that order) whose rho^2 is not positive.  Reads row l0 of A.
template <typename T>
__global__ __launch_bounds__(256) void k_chex_coef(ChexMat<T> M, int k0, int l0, T *__restrict__ tab, T *__restrict__ w,
                                                   int *info) {
  __shared__ T xs[256], ys[256], rs[256];
  const int t = threadIdx.x;
  T y = *chex_at(M, l0, l0);  // (used by lane 0)
  int bad = 0;
  T nx = l0 - 1 - t >= k0 ? *chex_at(M, l0, l0 - 1 - t) : T(0);
  for (int hi = l0 - 1; hi >= k0; hi -= 256) {
    const int cnt = min(256, hi - k0 + 1);
    xs[t] = nx;
    lds_barrier();
    nx = hi - 256 - t >= k0 ? *chex_at(M, l0, hi - 256 - t) : T(0);
    if (t == 0) {
      for (int u = 0; u < cnt; ++u) {
        T rho;
        if (!chex_pivot<T>(xs[u], y, rho) && !bad) bad = hi - u + 2;
        ys[u] = y;
        rs[u] = rho;
        y = rho;
      }
    }
    lds_barrier();
    if (t < cnt) {
      T *out = tab + 2 * (long)(hi - t - k0);
      out[0] = chex_quotient<T>(0, xs[t], ys[t], rs[t]);
      out[1] = chex_quotient<T>(1, xs[t], ys[t], rs[t]);
    }
    // (the next chunk's xs are written behind these reads: lane 0's loop lies behind the barrier that follows them)
    lds_barrier();
  }
  if (t == 0) {
    *chex_w(M, w, k0) = y;
    if (bad) info[0] = bad;
  }
}

// The new columns jlo..jhi of tile column J (k0 <= jlo, jhi <= l0), right to left, for every stored row from the top
// of tile row J down: new row i >= j takes a = L(r, j-1) from the staged copies (r = i - 1 inside the window, i below
// it; S0: tile column J, S1: J - 1, for j - 1 its last column), A(i, j) <- the rotated entry; column k0 <- what the
// row carried out of its last rotation (row k0: the last pivot).  w: what a row carries between the launches.
constexpr int CHEX_STAGE = 32, CHEX_UC = 16;
template <typename T>
__global__ __launch_bounds__(256) void k_chex_apply(ChexMat<T> M, int J, int jlo, int jhi, int k0, int l0,
                                                    ChexStage<T> S0, ChexStage<T> S1, const T *__restrict__ tab,
                                                    T *__restrict__ w) {
  constexpr int UC = CHEX_UC;
  static_assert(CHEX_STAGE % UC == 0 && 2 * CHEX_STAGE <= 256, "whole groups of columns per stage, a lane per value");
  __shared__ T cs[2][CHEX_STAGE * 2];
  const int R = blockIdx.x * 256 + threadIdx.x;
  const int ti = R / M.e, rr = R - ti * M.e, I = J + ti;
  const long in = (long)I * M.mb + rr;
  const bool on = rr < M.mb && in < M.n && in >= k0;  // (padding, and the rows before k: not read, not written)
  const int i = on ? (int)in : k0;
  const int r = i - (i > k0 && i <= l0 ? 1 : 0);
  const int Ir = r / M.mb;
  const T *src0 = S0.p + (long)(Ir - S0.row0) * M.bs + (r - Ir * M.mb);
  const T *src1 = S1.p + (long)(Ir - S1.row0) * M.bs + (r - Ir * M.mb) + (long)(M.mb - 1) * M.e;
  T *dst = M.A + ((long)I + (long)J * M.lmt) * M.bs + rr;
  T *wi = w + (long)I * M.e + rr;
  const int ncol = jhi - jlo + 1, cJ = J * M.mb;  // column u of the launch: j = jhi - u
  auto load_coef = [&](int s0) -> T {  // (beyond the last column, and for column k0: nothing)
    const int j = jhi - (s0 + (int)threadIdx.x / 2);
    return threadIdx.x < 2 * CHEX_STAGE && j >= jlo && j > k0 ? tab[2 * (long)(j - 1 - k0) + (threadIdx.x & 1)] : T(0);
  };
  auto load_a = [&](int u) -> T {
    const int j = jhi - u;
    if (!(on && u < ncol && j > k0 && i >= j)) return T(0);
    const int c = j - 1 - cJ;
    return c >= 0 ? src0[(long)c * M.e] : *src1;
  };
  T st = load_coef(0);
  T b = on ? *wi : T(0);
  T a[UC], nx[UC];
#pragma unroll
  for (int u = 0; u < UC; ++u) a[u] = load_a(u);
  for (int s0 = 0, half = 0; s0 < ncol; s0 += CHEX_STAGE, half ^= 1) {
    const int ns = min(CHEX_STAGE, ncol - s0);
    if (threadIdx.x < 2 * CHEX_STAGE) cs[half][threadIdx.x] = st;
    // (one barrier per stage: the next stage goes to the other half, and the one after it is written only behind the
    // next barrier, which every lane reaches with this stage read)
    lds_barrier();
    st = load_coef(s0 + CHEX_STAGE);
    for (int j0 = 0; j0 < ns; j0 += UC) {
      const int u0 = s0 + j0;
#pragma unroll
      for (int u = 0; u < UC; ++u) nx[u] = load_a(u0 + UC + u);
#pragma unroll
      for (int u = 0; u < UC; ++u)
        if (j0 + u < ns) {
          const int j = jhi - (u0 + u);
          if (j > k0) {
            if (on && i >= j) a[u] = chex_apply<T>(a[u], b, cs[half][2 * (j0 + u)], cs[half][2 * (j0 + u) + 1]);
          } else {
            a[u] = b;
          }
        }
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        const int j = jhi - (u0 + u);
        if (on && u0 + u < ncol && i >= j) dst[(long)(j - cJ) * M.e] = a[u];
      }
#pragma unroll
      for (int u = 0; u < UC; ++u) a[u] = nx[u];
    }
  }
  if (on) *wi = b;
}

}  // namespace

template <typename T>
void launch_chex_vec(hipStream_t s, const ChexMat<T> &M, int k0, int l0, int job, T *w) {
  k_chex_vec<T><<<(unsigned)((M.n - k0 + 255) / 256), 256, 0, s>>>(M, k0, l0, job, w);
}

template <typename T>
void launch_chex_setcol(hipStream_t s, const ChexMat<T> &M, int l0, const T *w) {
  k_chex_setcol<T><<<(unsigned)((M.n - l0 + 255) / 256), 256, 0, s>>>(M, l0, w);
}

template <typename T>
void launch_chex_move(hipStream_t s, const ChexMat<T> &M, int J, int c1, int I0, int I1, int k0, int l0, int job,
                      const ChexStage<T> &S0, const ChexStage<T> &S1) {
  if (c1 <= 0 || I1 <= I0) return;
  const int rows = (I1 - I0) * M.e;
  const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)((c1 + CHEX_CPT - 1) / CHEX_CPT));
  k_chex_move<T><<<grid, 256, 0, s>>>(M, J, c1, I0, rows, k0, l0, job, S0, S1);
}

template <typename T>
void launch_chex_coef(hipStream_t s, const ChexMat<T> &M, int k0, int l0, T *tab, T *w, int *info) {
  k_chex_coef<T><<<1, 256, 0, s>>>(M, k0, l0, tab, w, info);
}

template <typename T>
void launch_chex_apply(hipStream_t s, const ChexMat<T> &M, int nt, int J, int jlo, int jhi, int k0, int l0,
                       const ChexStage<T> &S0, const ChexStage<T> &S1, const T *tab, T *w) {
  if (jhi < jlo) return;
  const long rows = (long)(nt - J) * M.e;
  k_chex_apply<T><<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(M, J, jlo, jhi, k0, l0, S0, S1, tab, w);
}

#define INSTANTIATE_CHEX(T)                                                                                        \
  template void launch_chex_vec<T>(hipStream_t, const ChexMat<T> &, int, int, int, T *);                            \
  template void launch_chex_setcol<T>(hipStream_t, const ChexMat<T> &, int, const T *);                             \
  template void launch_chex_move<T>(hipStream_t, const ChexMat<T> &, int, int, int, int, int, int, int,             \
                                    const ChexStage<T> &, const ChexStage<T> &);                                    \
  template void launch_chex_coef<T>(hipStream_t, const ChexMat<T> &, int, int, T *, T *, int *);                    \
  template void launch_chex_apply<T>(hipStream_t, const ChexMat<T> &, int, int, int, int, int, int,                 \
                                     const ChexStage<T> &, const ChexStage<T> &, const T *, T *);
INSTANTIATE_CHEX(double)
INSTANTIATE_CHEX(float)

}  // namespace cholmi
