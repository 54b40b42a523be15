// Batched Cholesky of small matrices (include/cholmi.h: chol_potrf_batched, chol_potrs_batched, chol_posv_batched):
// 10^3 .. 10^6 independent SPD matrices of order n <= 64, column-major images at a fixed stride.  One kernel, three
// modes (factor, solve, factor + solve in one pass); the entry points follow it.
//
// Lane = row.  A sub-group of NP = 8 / 16 / 32 / 64 lanes (the padded order) owns one matrix, 64 / NP matrices share a
// wavefront; lane i keeps row i of the lower triangle in registers (a[m] = A(i,m), m <= i; every index of a[] is a
// compile-time constant: the loops over the padded order are unrolled, the actual order only guards them with
// wave-uniform branches).  The factorisation is right-looking: step j broadcasts the pivot, scales column j, and
// updates a[m] <- fma(-a[j], L(m,j), a[m]) with L(m,j) broadcast from lane m -- for entry (i,m) that is the chain
// k = 0 .. m-1 ascending of the header.  A broadcast is v_readlane with a compile-time lane at NP = 64 and a shuffle
// inside the sub-group below it.  No LDS, no barrier, no atomics on data; a matrix that fails only sets its own flag
// and keeps its own stores back, so its neighbours in the wavefront see nothing of it.
// `uplo` only chooses the loads and stores: Lower reads A(i,m) at i + m lda (a wave reads whole columns); Upper holds
// U = L^T, so lane i reads its row m = 0 .. i at consecutive addresses, with 16-byte loads where the image allows
// them (base, lda and stride all multiples of 16 bytes) and the chunk lies inside the triangle.
// The solve keeps the same rows: forward y_j = b_j r_j (r_j = 1 / L(j,j)), b_i <- fma(-L(i,j), y_j, b_i) for i > j;
// backward, j descending, x_j = (y_j - S_j) r_j with S_j the sum over the sub-group of t_i = L(i,j) x_i (i > j, else
// +0) by the butterfly t <- t + t[lane ^ off], off = NP/2 .. 1: a fixed tree per padded order, whatever uplo, nrhs or
// the position in the batch.  One right-hand column at a time, each on its own.
// The rank-r update and downdate of such factors (chol_chud_batched, chol_chdd_batched) is a second kernel on the same
// rows, k_chud_rows: the rotated vector is one more register per lane, a rotation two broadcasts and one chud_apply
// (chud_rot.h, the arithmetic of chol_chud_tile), vectors outer and columns inner, one store after the last vector.
// One half of such a factor alone (chol_trtrs_batched, chol_trmm_batched, chol_logdet_batched) is a third family on the
// same rows, k_half_rows: the forward or the backward sweep of the solve on its own, the two products with L and L^T,
// and a small kernel that reads the diagonal alone for the log-determinant.
// The explicit inverses (chol_trtri_batched, chol_potri_batched, chol_poinv_batched, chol_invdiag_batched) are a fourth
// family on the same rows, k_inv_rows: inv(L) and then inv(L)^T inv(L) built in place in the one register array, by
// broadcasts alone.
// (compiled with -ffp-contract=off: only the fma() calls below fuse)
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "api_internal.h"
#include "chud_rot.h"

using namespace cholmi;

namespace {

enum { MODE_POTRF = 0, MODE_POTRS = 1, MODE_POSV = 2, MODE_CHUD = 3, MODE_CHDD = 4 };  // (k_batched has the first three)
constexpr int BATCHED_THREADS = 256;  // four wavefronts, nothing shared between them
constexpr int NO_FAILURE = 0x7f7f7f7f;  // (what hipMemset of 0x7f leaves in the first-failure word)

template <typename T>
struct BatchedArgs {
  T *A, *B;
  long lda, strideA, ldb, strideB;
  int n, nrhs, batch;
  int vec;     // A's image allows 16-byte accesses of whole rows (Upper)
  int *info;   // batch words
  int *first;  // min over the failing matrices of b + 1
};

__device__ __forceinline__ float readlane(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}
__device__ __forceinline__ double readlane(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                          __builtin_amdgcn_readlane(__double2loint(x), l));
}
// x of lane `src` of this lane's sub-group (src a compile-time constant after unrolling)
template <typename T, int NP>
__device__ __forceinline__ T bcast(T x, int src) {
  if constexpr (NP == 64) return readlane(x, src);
  else return __shfl(x, src, NP);
}
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_(double a) { return __builtin_sqrt(a); }

template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  using type = float4;
};
template <>
struct Vec16<double> {
  using type = double2;
};

// Row i of the `uplo` triangle into a[] (live: this lane has a row; entries beyond the triangle: +0).  Every a[m] is
// assigned once, from a value of its own: zeroing the array first and loading under a branch makes the compiler keep
// a[] as one vector, copied whole at every branch, which spills at NP = 16 and 32.
template <typename T, int NP, bool UPPER>
__device__ __forceinline__ void load_rows(T (&a)[NP], const T *Ab, long lda, int n, int i, bool live, bool vec) {
  if constexpr (!UPPER) {
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      T v = T(0);
      if (m < n && live && i >= m) v = Ab[i + (long)m * lda];
      a[m] = v;
    }
  } else {
    constexpr int W = 16 / (int)sizeof(T);
    using V = typename Vec16<T>::type;
    const T *row = Ab + (long)i * lda;
#pragma unroll
    for (int c = 0; c < NP; c += W) {
      V v = {};
      T *e = reinterpret_cast<T *>(&v);
      if (c < n && live) {
        if (vec && c + W - 1 <= i) {
          v = *reinterpret_cast<const V *>(row + c);
        } else {
#pragma unroll
          for (int q = 0; q < W; ++q)
            if (c + q <= i) e[q] = row[c + q];
        }
      }
#pragma unroll
      for (int q = 0; q < W; ++q) a[c + q] = e[q];
    }
  }
}

// The columns < cols of row i back into the triangle
template <typename T, int NP, bool UPPER>
__device__ __forceinline__ void store_rows(const T (&a)[NP], T *Ab, long lda, int cols, int i, bool live, bool vec) {
  if constexpr (!UPPER) {
#pragma unroll
    for (int m = 0; m < NP; ++m)
      if (m < cols && live && i >= m) Ab[i + (long)m * lda] = a[m];
  } else {
    constexpr int W = 16 / (int)sizeof(T);
    using V = typename Vec16<T>::type;
    T *row = Ab + (long)i * lda;
#pragma unroll
    for (int c = 0; c < NP; c += W) {
      if (c < cols && live) {
        if (vec && c + W - 1 <= i && c + W <= cols) {
          V v;
          T *e = reinterpret_cast<T *>(&v);
#pragma unroll
          for (int q = 0; q < W; ++q) e[q] = a[c + q];
          *reinterpret_cast<V *>(row + c) = v;
        } else {
#pragma unroll
          for (int q = 0; q < W; ++q)
            if (c + q <= i && c + q < cols) row[c + q] = a[c + q];
        }
      }
    }
  }
}

// The right-looking factorisation of the rows in a[] for k_inv_rows: the loop of k_batched below, statement for
// statement (k_batched keeps its own copy: called from there, this function changes its register allocation, to 106
// from 56 VGPRs at fp64 and order 16).  -> LAPACK's info of this lane's matrix, the same in every lane of the
// sub-group; r: 1 / L(i,i)
template <typename T, int NP>
__device__ __forceinline__ int factor_rows(T (&a)[NP], int n, int i, T &r) {
  int bad = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (j < n) {
      const T d = bcast<T, NP>(a[j], j);
      if (!bad && !(d > T(0))) bad = j + 1;
      const T piv = sqrt_(d), rj = T(1) / piv;
      a[j] = i == j ? piv : a[j] * rj;
      if (i == j) r = rj;
#pragma unroll
      for (int m = j + 1; m < NP; ++m)
        if ((m & ~7) < n) a[m] = fma_(-a[j], bcast<T, NP>(a[j], m), a[m]);
    }
  }
  return bad;
}

// The first exact zero on the diagonal of the factor in a[] (1-based, 0: none), the same in every lane of the
// sub-group; r: 1 / L(i,i) (+0 in a lane without a row).  (k_batched's and k_half_rows' check, for k_inv_rows)
template <typename T, int NP>
__device__ __forceinline__ int diagonal_of_rows(const T (&a)[NP], int sub, int i, bool live, T &r) {
  T d = T(1);
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (i == k) d = a[k];
  const unsigned long long z = __ballot(live && d == T(0)) >> (sub * NP) & (NP == 64 ? ~0ull : (1ull << NP) - 1);
  r = live ? T(1) / d : T(0);
  return z ? __ffsll((long long)z) : 0;
}

// Registers: the row is NP sizeof(T) / 4 VGPRs -- 128 at fp64 and order 64, which with the solve's values stays under
// 168 (three wavefronts per SIMD).  The launch bound of 256 lanes allows all 512 registers; no kernel takes AGPRs or
// scratch (DESIGN.md 3m has the table).
template <typename T, int NP, bool UPPER, int MODE>
__global__ __launch_bounds__(BATCHED_THREADS) void k_batched(BatchedArgs<T> p) {
  constexpr int M = 64 / NP;  // matrices per wavefront
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  if (wave * M >= p.batch) return;  // (a whole wavefront: the shuffles below never see a partly exited one)
  const int sub = lane / NP, i = lane % NP, n = p.n;
  const long b = wave * M + sub;
  const bool live = b < p.batch && i < n;
  T *Ab = p.A + (live ? b : 0) * p.strideA;

  T a[NP];
  load_rows<T, NP, UPPER>(a, Ab, p.lda, n, i, live, p.vec != 0);

  int bad = 0;  // LAPACK's info of this lane's matrix: the same in every lane of the sub-group
  T r = T(0);   // 1 / L(i,i)
  if constexpr (MODE != MODE_POTRS) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (j < n) {
        const T d = bcast<T, NP>(a[j], j);
        if (!bad && !(d > T(0))) bad = j + 1;
        const T piv = sqrt_(d), rj = T(1) / piv;
        a[j] = i == j ? piv : a[j] * rj;
        if (i == j) r = rj;
#pragma unroll
        for (int m = j + 1; m < NP; ++m)
          if ((m & ~7) < n) a[m] = fma_(-a[j], bcast<T, NP>(a[j], m), a[m]);
      }
    }
    // (a failed matrix: the columns before the failing one are final and stored, the rest stays as it was given)
    store_rows<T, NP, UPPER>(a, Ab, p.lda, bad ? bad - 1 : n, i, live, p.vec != 0);
  } else {
    T d = T(1);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (i == k) d = a[k];
    const unsigned long long z = __ballot(live && d == T(0)) >> (sub * NP) & (NP == 64 ? ~0ull : (1ull << NP) - 1);
    if (z) bad = __ffsll((long long)z);
    r = live ? T(1) / d : T(0);
  }
  if (live && i == 0) {
    p.info[b] = bad;
    if (bad) atomicMin(p.first, (int)(b < INT_MAX ? b + 1 : INT_MAX));
  }

  if constexpr (MODE != MODE_POTRF) {
    const bool wr = live && !bad;  // (a failed matrix computes on, in its own lanes, and stores nothing)
    T *Bb = p.B + (live ? b : 0) * p.strideB + i;
    for (int c = 0; c < p.nrhs; ++c) {
      T *at = Bb + (long)c * p.ldb;
      T v = wr ? *at : T(0);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (j < n) {
          const T yj = bcast<T, NP>(v * r, j);
          if (i > j) v = fma_(-a[j], yj, v);
        }
      }
      const T y = v * r;
      T x = T(0);
#pragma unroll
      for (int j = NP - 1; j >= 0; --j) {
        if (j < n) {
          T t = i > j ? a[j] * x : T(0);
#pragma unroll
          for (int off = NP / 2; off >= 1; off >>= 1) t = t + __shfl_xor(t, off, NP);
          const T cand = (y - t) * r;
          if (i == j) x = cand;
        }
      }
      if (wr) *at = x;
    }
  }
}

template <typename T, int NP, bool UPPER>
void launch_mode(int mode, hipStream_t s, unsigned grid, const BatchedArgs<T> &p) {
  if (mode == MODE_POTRF) k_batched<T, NP, UPPER, MODE_POTRF><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else if (mode == MODE_POTRS) k_batched<T, NP, UPPER, MODE_POTRS><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else k_batched<T, NP, UPPER, MODE_POSV><<<grid, BATCHED_THREADS, 0, s>>>(p);
}
template <typename T, int NP>
void launch_uplo(bool upper, int mode, hipStream_t s, unsigned grid, const BatchedArgs<T> &p) {
  if (upper) launch_mode<T, NP, true>(mode, s, grid, p);
  else launch_mode<T, NP, false>(mode, s, grid, p);
}
inline int padded_order(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }
template <typename T>
void launch_batched(bool upper, int mode, hipStream_t s, unsigned grid, const BatchedArgs<T> &p) {
  switch (padded_order(p.n)) {
    case 8: return launch_uplo<T, 8>(upper, mode, s, grid, p);
    case 16: return launch_uplo<T, 16>(upper, mode, s, grid, p);
    case 32: return launch_uplo<T, 32>(upper, mode, s, grid, p);
    default: return launch_uplo<T, 64>(upper, mode, s, grid, p);
  }
}

// ---------------------------------------------------------------- rank-r update and downdate
template <typename T>
struct ChudRowsArgs {
  T *A;
  const T *V;
  long lda, strideA, ldv, strideV;
  int n, r, batch;
  int vec;    // as BatchedArgs
  T sigma;    // +1 update, -1 downdate
  int *info;  // batch words
  int *first;
};

// The factor of L L^T + sigma V V^T in the rows k_batched keeps.  Vector t: lane i holds v = V(i,t); column j takes
// L_jj and v_j from lane j, every lane makes the pivot for itself (it is the same in the whole sub-group), lanes 0, 1
// and 2 of the sub-group divide one of the three quotients each and broadcast it (one division per column instead of
// three: 0.66 to 0.85 of the time at r >= 4), lane j keeps rr and the lanes below apply the rotation.
// The lanes i < j apply it too, to registers nobody reads again (a[j] beyond the triangle, a v_i whose column is
// past), which saves the selects.
// Running the vectors outside gives the bits and the info of the header's order (columns outer): the rotation of
// (j, t) needs column j after the vectors before t and vector t after the columns before j, in either order; a
// rotation that cannot be made is the identity (chud_pivot), so the columns before the first such column -- the
// header's info, the least over the vectors -- are the same in both orders, and nothing of that matrix is stored.
// Registers: the row, v, the pivot's and the rotation's values: fp64 at order 64 stays under 168.
template <typename T, int NP, bool UPPER>
__global__ __launch_bounds__(BATCHED_THREADS) void k_chud_rows(ChudRowsArgs<T> p) {
  constexpr int M = 64 / NP;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  if (wave * M >= p.batch) return;
  const int sub = lane / NP, i = lane % NP, n = p.n;
  const long b = wave * M + sub;
  const bool live = b < p.batch && i < n;
  T *Ab = p.A + (live ? b : 0) * p.strideA;
  const T *Vb = p.V + (live ? b : 0) * p.strideV + i;

  T a[NP];
  load_rows<T, NP, UPPER>(a, Ab, p.lda, n, i, live, p.vec != 0);

  T d = T(1);
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (i == k) d = a[k];
  const unsigned long long z = __ballot(live && d == T(0)) >> (sub * NP) & (NP == 64 ? ~0ull : (1ull << NP) - 1);
  const int zero = z ? __ffsll((long long)z) : 0;  // an exact zero on the diagonal comes before everything else
  int stop = NP + 1;  // the first column (1-based) at which some vector's rotation cannot be made

  for (int t = 0; t < p.r; ++t) {
    T v = live ? Vb[(long)t * p.ldv] : T(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (j < n) {
        const T ljj = bcast<T, NP>(a[j], j);
        T vj = bcast<T, NP>(v, j), rr;
        if (!chud_pivot<T>(ljj, vj, p.sigma, rr) && j + 1 < stop) stop = j + 1;
        ChudRot<T> rot;
        const T q = chud_quotient<T>(i, ljj, vj, rr);  // (lanes 0, 1, 2: c, s, ci; the others divide for nothing)
        rot.c = bcast<T, NP>(q, 0);
        rot.s = bcast<T, NP>(q, 1);
        rot.ci = bcast<T, NP>(q, 2);
        rot.ss = p.sigma * rot.s;
        T l = a[j];
        chud_apply<T>(l, v, rot);
        a[j] = i == j ? rr : l;
      }
    }
  }

  const int bad = zero ? zero : stop <= NP ? stop : 0;
  // (a failed matrix has computed on, in its own lanes, and stores nothing)
  store_rows<T, NP, UPPER>(a, Ab, p.lda, n, i, live && !bad, p.vec != 0);
  if (live && i == 0) {
    p.info[b] = bad;
    if (bad) atomicMin(p.first, (int)(b < INT_MAX ? b + 1 : INT_MAX));
  }
}

template <typename T, int NP>
void launch_chud_uplo(bool upper, hipStream_t s, unsigned grid, const ChudRowsArgs<T> &p) {
  if (upper) k_chud_rows<T, NP, true><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else k_chud_rows<T, NP, false><<<grid, BATCHED_THREADS, 0, s>>>(p);
}
template <typename T>
void launch_chud_rows(bool upper, hipStream_t s, unsigned grid, const ChudRowsArgs<T> &p) {
  switch (padded_order(p.n)) {
    case 8: return launch_chud_uplo<T, 8>(upper, s, grid, p);
    case 16: return launch_chud_uplo<T, 16>(upper, s, grid, p);
    case 32: return launch_chud_uplo<T, 32>(upper, s, grid, p);
    default: return launch_chud_uplo<T, 64>(upper, s, grid, p);
  }
}

// ---------------------------------------------------------------- one half of the factor: trtrs, trmm, logdet
enum { HALF_SOLVE_FWD = 0, HALF_SOLVE_BWD = 1, HALF_MUL_FWD = 2, HALF_MUL_BWD = 3 };

template <typename T>
struct HalfArgs {
  const T *A;
  T *B;
  long lda, strideA, ldb, strideB;
  int n, nrhs, batch;
  int vec;     // as BatchedArgs
  T alpha;     // (the products)
  int *info;   // batch words (the solves)
  int *first;
};

// One sweep with the lower factor L in the rows k_batched keeps (UPPER: the image holds U = L^T; which of op(T) is the
// forward and which the backward half the host decides).  The solves are the two halves of k_batched's MODE_POTRS,
// statement for statement, so forward then backward returns its bits.  The products: forward x_i = sum over k <= i of
// L(i,k) z_k, z_k broadcast from lane k, k ascending; backward x_j = sum over i >= j of L(i,j) z_i by the backward
// solve's butterfly.  Both select the terms of the triangle instead of multiplying by the +0 that load_rows left
// beyond it: a NaN in z_k reaches only the rows that depend on it.
// Registers: the row and four or five values, the budget of MODE_POTRS (DESIGN.md 3o has the table).
template <typename T, int NP, bool UPPER, int OP>
__global__ __launch_bounds__(BATCHED_THREADS) void k_half_rows(HalfArgs<T> p) {
  constexpr int M = 64 / NP;
  constexpr bool SOLVE = OP == HALF_SOLVE_FWD || OP == HALF_SOLVE_BWD;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  if (wave * M >= p.batch) return;
  const int sub = lane / NP, i = lane % NP, n = p.n;
  const long b = wave * M + sub;
  const bool live = b < p.batch && i < n;
  const T *Ab = p.A + (live ? b : 0) * p.strideA;

  T a[NP];
  load_rows<T, NP, UPPER>(a, Ab, p.lda, n, i, live, p.vec != 0);

  int bad = 0;
  T r = T(0);  // 1 / L(i,i)
  if constexpr (SOLVE) {
    T d = T(1);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (i == k) d = a[k];
    const unsigned long long z = __ballot(live && d == T(0)) >> (sub * NP) & (NP == 64 ? ~0ull : (1ull << NP) - 1);
    if (z) bad = __ffsll((long long)z);
    r = live ? T(1) / d : T(0);
    if (live && i == 0) {
      p.info[b] = bad;
      if (bad) atomicMin(p.first, (int)(b < INT_MAX ? b + 1 : INT_MAX));
    }
  }

  const bool wr = live && !bad;  // (a failed matrix computes on, in its own lanes, and stores nothing)
  T *Bb = p.B + (live ? b : 0) * p.strideB + i;
  for (int c = 0; c < p.nrhs; ++c) {
    T *at = Bb + (long)c * p.ldb;
    T v = wr ? *at : T(0);
    T x = T(0);
    if constexpr (OP == HALF_SOLVE_FWD) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (j < n) {
          const T yj = bcast<T, NP>(v * r, j);
          if (i > j) v = fma_(-a[j], yj, v);
        }
      }
      x = v * r;
    } else if constexpr (OP == HALF_SOLVE_BWD) {
#pragma unroll
      for (int j = NP - 1; j >= 0; --j) {
        if (j < n) {
          T t = i > j ? a[j] * x : T(0);
#pragma unroll
          for (int off = NP / 2; off >= 1; off >>= 1) t = t + __shfl_xor(t, off, NP);
          const T cand = (v - t) * r;
          if (i == j) x = cand;
        }
      }
    } else if constexpr (OP == HALF_MUL_FWD) {
      T s = T(0);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        if (k < n) {
          const T zk = bcast<T, NP>(v, k);
          if (i >= k) s = fma_(a[k], zk, s);
        }
      }
      x = p.alpha * s;
    } else {
#pragma unroll
      for (int j = NP - 1; j >= 0; --j) {
        if (j < n) {
          T t = i >= j ? a[j] * v : T(0);  // (+0 in the lanes from n on: a[j] and v are +0 there)
#pragma unroll
          for (int off = NP / 2; off >= 1; off >>= 1) t = t + __shfl_xor(t, off, NP);
          if (i == j) x = p.alpha * t;
        }
      }
    }
    if (wr) *at = x;
  }
}

template <typename T, int NP, bool UPPER>
void launch_half_op(int op, hipStream_t s, unsigned grid, const HalfArgs<T> &p) {
  if (op == HALF_SOLVE_FWD) k_half_rows<T, NP, UPPER, HALF_SOLVE_FWD><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else if (op == HALF_SOLVE_BWD) k_half_rows<T, NP, UPPER, HALF_SOLVE_BWD><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else if (op == HALF_MUL_FWD) k_half_rows<T, NP, UPPER, HALF_MUL_FWD><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else k_half_rows<T, NP, UPPER, HALF_MUL_BWD><<<grid, BATCHED_THREADS, 0, s>>>(p);
}
template <typename T, int NP>
void launch_half_uplo(bool upper, int op, hipStream_t s, unsigned grid, const HalfArgs<T> &p) {
  if (upper) launch_half_op<T, NP, true>(op, s, grid, p);
  else launch_half_op<T, NP, false>(op, s, grid, p);
}
template <typename T>
void launch_half_rows(bool upper, int op, hipStream_t s, unsigned grid, const HalfArgs<T> &p) {
  switch (padded_order(p.n)) {
    case 8: return launch_half_uplo<T, 8>(upper, op, s, grid, p);
    case 16: return launch_half_uplo<T, 16>(upper, op, s, grid, p);
    case 32: return launch_half_uplo<T, 32>(upper, op, s, grid, p);
    default: return launch_half_uplo<T, 64>(upper, op, s, grid, p);
  }
}

// trmm with alpha == 0: B <- +0 in the lanes of k_half_rows, neither A nor B read (NP: the padded order)
template <typename T>
__global__ __launch_bounds__(BATCHED_THREADS) void k_zero_rows(T *B, long ldb, long strideB, int n, int nrhs,
                                                               int batch, int NP) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  const int i = lane % NP;
  const long b = wave * (64 / NP) + lane / NP;
  if (b >= batch || i >= n) return;
  T *Bb = B + b * strideB + i;
  for (int c = 0; c < nrhs; ++c) Bb[(long)c * ldb] = T(0);
}

// logdet[b] = 2 (((log d_0 + log d_1) + log d_2) + ..): the sub-groups of k_half_rows with lane = j, which loads d_j
// alone and takes its logarithm in fp64; the chain then runs in every lane of the sub-group, log d_j shuffled from
// lane j.  The first d_j <= 0 or NaN is info and makes the value NaN.
template <typename T>
__global__ __launch_bounds__(BATCHED_THREADS) void k_diag_logdet(const T *A, long lda, long strideA, int n, int batch,
                                                            int NP, double *out, int *info, int *first) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  const int M = 64 / NP;
  if (wave * M >= batch) return;  // (a whole wavefront)
  const int sub = lane / NP, j = lane % NP;
  const long b = wave * M + sub;
  const bool live = b < batch && j < n;
  const double d = live ? (double)A[b * strideA + j * (lda + 1)] : 1.0;
  const unsigned long long z = __ballot(live && !(d > 0.0)) >> (sub * NP) & (NP == 64 ? ~0ull : (1ull << NP) - 1);
  const int bad = z ? __ffsll((long long)z) : 0;
  const double lg = log(d);
  double s = 0.0;
  for (int k = 0; k < n; ++k) s = s + __shfl(lg, k, NP);
  if (live && j == 0) {
    out[b] = bad ? __builtin_nan("") : 2.0 * s;
    info[b] = bad;
    if (bad) atomicMin(first, (int)(b < INT_MAX ? b + 1 : INT_MAX));
  }
}

// ---------------------------------------------------------------- the inverses: trtri, potri, poinv, invdiag
enum { INV_TRTRI = 0, INV_POTRI = 1, INV_POINV = 2, INV_DIAG = 3 };

template <typename T>
struct InvArgs {
  T *A;
  T *D;  // (invdiag: n elements per matrix; A is only read then)
  long lda, strideA, strideD;
  int n, batch;
  int vec;    // as BatchedArgs
  int *info;  // batch words
  int *first;
};

// Column i of W = inv(L) from lane i, whose t[k] = W(k,i), k >= i, into the `uplo` triangle: Lower stores the column
// as it is (a run of consecutive addresses per lane, in 16-byte pieces where the image allows them and the piece lies
// inside the triangle: load_rows<UPPER> mirrored), Upper stores it as row i of inv(U) = W^T (a wave writes whole
// columns)
template <typename T, int NP, bool UPPER>
__device__ __forceinline__ void store_cols(const T (&t)[NP], T *Ab, long lda, int n, int i, bool live, bool vec) {
  if constexpr (UPPER) {
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (k < n && live && k >= i) Ab[i + (long)k * lda] = t[k];
  } else {
    constexpr int W = 16 / (int)sizeof(T);
    using V = typename Vec16<T>::type;
    T *col = Ab + (long)i * lda;
#pragma unroll
    for (int c = 0; c < NP; c += W) {
      if (c < n && live) {
        if (vec && c >= i && c + W <= n) {
          V v;
          T *e = reinterpret_cast<T *>(&v);
#pragma unroll
          for (int q = 0; q < W; ++q) e[q] = t[c + q];
          *reinterpret_cast<V *>(col + c) = v;
        } else {
#pragma unroll
          for (int q = 0; q < W; ++q)
            if (c + q >= i && c + q < n) col[c + q] = t[c + q];
        }
      }
    }
  }
}

// The inverses in the rows k_batched keeps, in ONE register array.  Lane i loads row i of L into t[m], m <= i, with +0
// beyond the triangle; column i of W = inv(L) needs the slots k >= i, the complement but for the diagonal, whose
// L(i,i) lives on as r = 1 / L(i,i).  So the column is built in place, right-looking (the header's chain, which is the
// forward sweep of k_half_rows applied to e_i and started at step i): t[i] = 1, and at step j the lanes i <= j make
// y = t[j] r_j final and update t[k] <- fma(-L(k,j), y, t[k]), k > j, with L(k,j) = t[j] of lane k, which lane k
// (k > j: not yet started) still holds.  The lanes i > j are left alone by a select, not by a product with the +0 they
// hold: their slots are L's, and a NaN or Inf in column j of L must not reach the columns of W after j.
// The product X = W^T W is built in place as well: row i of X needs the slots m <= i, which hold L (dead by now) and
// are set to +0, the diagonal slot too (W(i,i) is r).  Step k, ascending, adds W(k,i) W(k,m) to t[m] for m <= k in
// the lanes i <= k, W(k,m) = t[k] of lane m; slot k is written last in its step, after every lane has read it.  The
// slots m > i of a lane receive sums that belong to nothing; they are dead (column entries of the steps before) and
// never stored.  The diagonal of X alone (invdiag) needs no broadcast: x_i = sum over k >= i of W(k,i)^2.
// No reduction anywhere: n^2 / 2 broadcasts per phase.  Registers: one row, as k_batched (DESIGN.md 3p has the table).
template <typename T, int NP, bool UPPER, int MODE>
__global__ __launch_bounds__(BATCHED_THREADS) void k_inv_rows(InvArgs<T> p) {
  constexpr int M = 64 / NP;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (BATCHED_THREADS / 64) + (threadIdx.x >> 6);
  if (wave * M >= p.batch) return;  // (a whole wavefront)
  const int sub = lane / NP, i = lane % NP, n = p.n;
  const long b = wave * M + sub;
  const bool live = b < p.batch && i < n;
  T *Ab = p.A + (live ? b : 0) * p.strideA;

  T t[NP];
  load_rows<T, NP, UPPER>(t, Ab, p.lda, n, i, live, p.vec != 0);

  int bad;
  T r = T(0);  // 1 / L(i,i)
  if constexpr (MODE == INV_POINV) {
    bad = factor_rows<T, NP>(t, n, i, r);
    // (a failed matrix is left as potrf leaves it; the others keep the factor in registers)
    store_rows<T, NP, UPPER>(t, Ab, p.lda, bad - 1, i, live && bad, p.vec != 0);
  } else {
    bad = diagonal_of_rows<T, NP>(t, sub, i, live, r);
  }
  if (live && i == 0) {
    p.info[b] = bad;
    if (bad) atomicMin(p.first, (int)(b < INT_MAX ? b + 1 : INT_MAX));
  }
  const bool wr = live && !bad;  // (a failed matrix computes on, in its own lanes, and stores nothing more)

  // W = inv(L): t[k] = W(k,i), k >= i, from e_i (factor_rows leaves its updates beyond the triangle, not +0)
#pragma unroll
  for (int k = 0; k < NP; ++k) t[k] = i == k ? T(1) : i < k ? T(0) : t[k];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (j < n) {
      const bool on = i <= j;
      const T lj = t[j];  // (the lanes k > j: L(k,j))
      const T y = lj * bcast<T, NP>(r, j);
      t[j] = on ? y : lj;
#pragma unroll
      for (int k = j + 1; k < NP; ++k) {
        if ((k & ~7) < n) {
          const T u = fma_(-bcast<T, NP>(lj, k), y, t[k]);
          t[k] = on ? u : t[k];
        }
      }
    }
  }
  if constexpr (MODE == INV_TRTRI) {
    store_cols<T, NP, UPPER>(t, Ab, p.lda, n, i, wr, p.vec != 0);
    return;
  }

  if constexpr (MODE == INV_DIAG) {
    T s = T(0);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      if (k < n) {
        const T u = fma_(t[k], t[k], s);
        s = i <= k ? u : s;
      }
    }
    if (wr) p.D[b * p.strideD + i] = s;
    return;
  }

  // X = W^T W: t[m] = X(i,m), m <= i
#pragma unroll
  for (int m = 0; m < NP; ++m) t[m] = i >= m ? T(0) : t[m];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (k < n) {
      const bool on = i <= k;
      const T wk = t[k];                // (the lanes m < k: W(k,m))
      const T ck = i == k ? r : wk;     // W(k,i)
#pragma unroll
      for (int m = 0; m < k; ++m) {
        const T u = fma_(ck, bcast<T, NP>(wk, m), t[m]);
        t[m] = on ? u : t[m];
      }
      const T u = fma_(ck, bcast<T, NP>(r, k), wk);  // (lane k: r r + 0)
      t[k] = on ? u : wk;
    }
  }
  store_rows<T, NP, UPPER>(t, Ab, p.lda, n, i, wr, p.vec != 0);
}

template <typename T, int NP, bool UPPER>
void launch_inv_mode(int mode, hipStream_t s, unsigned grid, const InvArgs<T> &p) {
  if (mode == INV_TRTRI) k_inv_rows<T, NP, UPPER, INV_TRTRI><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else if (mode == INV_POTRI) k_inv_rows<T, NP, UPPER, INV_POTRI><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else if (mode == INV_POINV) k_inv_rows<T, NP, UPPER, INV_POINV><<<grid, BATCHED_THREADS, 0, s>>>(p);
  else k_inv_rows<T, NP, UPPER, INV_DIAG><<<grid, BATCHED_THREADS, 0, s>>>(p);
}
template <typename T, int NP>
void launch_inv_uplo(bool upper, int mode, hipStream_t s, unsigned grid, const InvArgs<T> &p) {
  if (upper) launch_inv_mode<T, NP, true>(mode, s, grid, p);
  else launch_inv_mode<T, NP, false>(mode, s, grid, p);
}
template <typename T>
void launch_inv_rows(bool upper, int mode, hipStream_t s, unsigned grid, const InvArgs<T> &p) {
  switch (padded_order(p.n)) {
    case 8: return launch_inv_uplo<T, 8>(upper, mode, s, grid, p);
    case 16: return launch_inv_uplo<T, 16>(upper, mode, s, grid, p);
    case 32: return launch_inv_uplo<T, 32>(upper, mode, s, grid, p);
    default: return launch_inv_uplo<T, 64>(upper, mode, s, grid, p);
  }
}

// ---------------------------------------------------------------- host
ScratchPool<1> bt;  // [0]: the first-failure word, then (at 16 bytes) the batch words of info
hipEvent_t bt_ev[4] = {};
double bt_stats[8] = {};

// the position of each argument in an entry point's signature (0: it has none)
struct ArgPos {
  int uplo, dtype, n, nrhs, A, lda, strideA, B, ldb, strideB, batch, trans;
};
constexpr ArgPos POS_POTRF = {1, 2, 3, 0, 4, 5, 6, 0, 0, 0, 7, 0};
constexpr ArgPos POS_SOLVE = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0};
constexpr ArgPos POS_TRTRS = {1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 2};
constexpr ArgPos POS_TRMM = {1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 2};  // (6: alpha)
constexpr ArgPos POS_LOGDET = {0, 1, 2, 0, 3, 4, 5, 0, 0, 0, 6, 0};    // (7: logdet)
constexpr ArgPos POS_INVDIAG = {1, 2, 3, 0, 4, 5, 6, 7, 0, 8, 9, 0};   // (D: an n x 1 image in B's place)

// what the messages call B and its arguments, and where n > 64 sends the caller
struct ArgNames {
  const char *B, *ldb, *nrhs, *beyond;
};
constexpr ArgNames NAMES_POTRF = {"B", "ldb", "nrhs",
                                  "use chol_potrf_batch (tiles that are multiples of 128) or the descriptor routines "
                                  "(chol_potrf_tile, chol_potrs_tile, chol_posv_tile)"};
constexpr ArgNames NAMES_CHUD = {"V", "ldv", "r",
                                 "use the descriptor routines (chol_chud_tile, chol_chdd_tile), which take any order"};
constexpr ArgNames NAMES_HALF = {"B", "ldb", "nrhs",
                                 "use the descriptor routines (chol_trtrs_tile, chol_trmm_tile, chol_logdet_tile), "
                                 "which take any order"};
constexpr ArgNames NAMES_INV = {"D", "n", "1",
                                "use the descriptor routines (chol_trtri_tile, chol_potri_tile, chol_poinv_tile), "
                                "which take any order"};

// bytes from the base to the end of the last element of `batch` images of rows x cols
inline unsigned long long span_bytes(long long rows, long long cols, long long ld, long long stride, long long batch,
                                     size_t es) {
  if (!rows || !cols || !batch) return 0;
  return ((unsigned long long)(batch - 1) * stride + (unsigned long long)(cols - 1) * ld + rows) * es;
}

// The argument rules that every entry point shares, in the order of the checks (pos.B == 0: the routine has no B;
// empty_rhs: nrhs == 0 leaves nothing to do).  -> negative: the error; 1: a zero size, info zeroed, nothing to do;
// 0: go on.
int check_images(const char *what, const ArgPos &pos, const ArgNames &nm, int uplo, int trans, int dtype, int n,
                 int nrhs, const void *A, int lda, long long strideA, const void *B, int ldb, long long strideB,
                 int batch, bool empty_rhs, int *info) {
  if (!ctx_inited()) return failf(CHOL_ERR_NOT_INITIALIZED, "%s before chol_init", what);
  if (pos.uplo && uplo != CHOL_LOWER && uplo != CHOL_UPPER) return failf(-pos.uplo, "%s: uplo", what);
  if (pos.trans && trans != CHOL_NOTRANS && trans != CHOL_TRANS)
    return failf(-pos.trans, "%s: trans must be CHOL_NOTRANS or CHOL_TRANS", what);
  if (dtype != CHOL_REAL_DOUBLE && dtype != CHOL_REAL_FLOAT)
    return failf(-pos.dtype, "%s: dtype must be fp64 or fp32", what);
  if (n < 0) return failf(-pos.n, "%s: n < 0", what);
  if (pos.B && nrhs < 0) return failf(-pos.nrhs, "%s: %s < 0", what, nm.nrhs);
  if (batch < 0) return failf(-pos.batch, "%s: batch < 0", what);
  if (n > 64) return failf(CHOL_ERR_NOT_SUPPORTED, "%s: n > 64; %s", what, nm.beyond);
  if (lda < (n > 1 ? n : 1)) return failf(-pos.lda, "%s: lda < max(1, n)", what);
  if (strideA < (long long)lda * n) return failf(-pos.strideA, "%s: strideA < lda * n", what);
  if (pos.B) {
    if (ldb < (n > 1 ? n : 1)) return failf(-pos.ldb, "%s: %s < max(1, n)", what, nm.ldb);
    if (strideB < (long long)ldb * nrhs)
      return failf(-pos.strideB, "%s: stride%s < %s * %s", what, nm.B, nm.ldb, nm.nrhs);
  }
  if (n == 0 || batch == 0 || (empty_rhs && nrhs == 0)) {
    for (int b = 0; info && b < batch; ++b) info[b] = 0;
    return 1;
  }
  const size_t es = dtype == CHOL_REAL_DOUBLE ? sizeof(double) : sizeof(float);
  if (!A || !is_device_ptr(A)) return failf(-pos.A, "%s: A must be a device pointer", what);
  if (pos.B && nrhs > 0) {
    if (!B || !is_device_ptr(B)) return failf(-pos.B, "%s: %s must be a device pointer", what, nm.B);
    const uintptr_t a0 = (uintptr_t)A, b0 = (uintptr_t)B;
    const uintptr_t a1 = a0 + span_bytes(n, n, lda, strideA, batch, es);
    const uintptr_t b1 = b0 + span_bytes(n, nrhs, ldb, strideB, batch, es);
    if (a0 < b1 && b0 < a1) return failf(-pos.B, "%s: the address ranges of A and %s overlap", what, nm.B);
  }
  return 0;
}

// A's image allows 16-byte accesses of whole rows
inline bool rows_vec(const void *A, int lda, long long strideA, size_t es) {
  return (uintptr_t)A % 16 == 0 && (size_t)lda * es % 16 == 0 && (unsigned long long)strideA * es % 16 == 0;
}

// One call on the main stream between the library's events: the first-failure word reset, launch(s, grid, dinfo,
// first) for `batch` matrices in sub-groups of the padded order of n, the word and info back, the statistics.
// -> 0, or b + 1 of the first failing matrix
int run_timed(const char *what, int n, int batch, int *info, double bytes,
              const std::function<void(hipStream_t, unsigned, int *, int *)> &launch) {
  return with_views({}, [&]() -> int {
    hipStream_t s = main_rank_ctx()->st[ST_MAIN];
    if (int rc = bt.ensure_bytes(0, 16 + (size_t)batch * sizeof(int), what)) return rc;
    for (hipEvent_t &e : bt_ev)
      if (!e) HIPCHECK(hipEventCreate(&e));
    int *first = bt.as<int>(0), *dinfo = first + 4;
    const int NP = padded_order(n), per_wave = 64 / NP;
    const long long waves = ((long long)batch + per_wave - 1) / per_wave;
    const unsigned grid = (unsigned)((waves + BATCHED_THREADS / 64 - 1) / (BATCHED_THREADS / 64));

    // events: the whole call [0] .. [3], the kernel [1] .. [2]
    HIPCHECK(hipEventRecord(bt_ev[0], s));
    HIPCHECK(hipMemsetAsync(first, 0x7f, sizeof(int), s));
    HIPCHECK(hipEventRecord(bt_ev[1], s));
    launch(s, grid, dinfo, first);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(bt_ev[2], s));
    int head = NO_FAILURE;
    HIPCHECK(hipMemcpyAsync(&head, first, sizeof(int), hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, dinfo, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipEventRecord(bt_ev[3], s));
    HIPCHECK(hipStreamSynchronize(s));
    float total = 0, kern = 0;
    HIPCHECK(hipEventElapsedTime(&total, bt_ev[0], bt_ev[3]));
    HIPCHECK(hipEventElapsedTime(&kern, bt_ev[1], bt_ev[2]));
    const double st[8] = {total, kern, (double)batch, (double)n, (double)per_wave, (double)grid, bytes, 0.0};
    std::copy(st, st + 8, bt_stats);
    return head == NO_FAILURE ? 0 : head;
  });
}

// potrf, potrs, posv, chud and chdd.  MODE_CHUD / MODE_CHDD: B is the n x nrhs block of vectors V (only read), nrhs
// is r.
int run_batched(const char *what, int mode, const ArgPos &pos, int uplo, int dtype, int n, int nrhs, void *A, int lda,
                long long strideA, void *B, int ldb, long long strideB, int batch, int *info) {
  const bool chud = mode == MODE_CHUD || mode == MODE_CHDD;
  if (int rc = check_images(what, pos, chud ? NAMES_CHUD : NAMES_POTRF, uplo, 0, dtype, n, nrhs, A, lda, strideA, B,
                            ldb, strideB, batch, mode == MODE_POTRS || chud, info))
    return rc < 0 ? rc : 0;
  const bool rhs = mode != MODE_POTRF && nrhs > 0;
  const size_t es = dtype == CHOL_REAL_DOUBLE ? sizeof(double) : sizeof(float);
  const bool vec = rows_vec(A, lda, strideA, es);
  const double tri = 0.5 * n * (n + 1.0), rhs_el = chud ? 1.0 * n * nrhs : rhs ? 2.0 * n * nrhs : 0.0;  // (V: read)
  const double el = (mode == MODE_POTRS ? tri : 2.0 * tri) + rhs_el;
  return run_timed(what, n, batch, info, el * es * batch, [&](hipStream_t s, unsigned grid, int *dinfo, int *first) {
    const int kmode = rhs ? mode : MODE_POTRF;  // (posv without a right-hand side factors)
    if (chud) {
      const double sigma = mode == MODE_CHUD ? 1.0 : -1.0;
      if (dtype == CHOL_REAL_DOUBLE) {
        const ChudRowsArgs<double> p = {(double *)A, (const double *)B, lda, strideA, ldb,   strideB, n,
                                        nrhs,        batch,             vec, sigma,   dinfo, first};
        launch_chud_rows<double>(uplo == CHOL_UPPER, s, grid, p);
      } else {
        const ChudRowsArgs<float> p = {(float *)A, (const float *)B, lda, strideA,      ldb,   strideB, n,
                                       nrhs,       batch,            vec, (float)sigma, dinfo, first};
        launch_chud_rows<float>(uplo == CHOL_UPPER, s, grid, p);
      }
    } else if (dtype == CHOL_REAL_DOUBLE) {
      const BatchedArgs<double> p = {(double *)A, (double *)B, lda,   strideA, ldb,   strideB,
                                     n,           nrhs,        batch, vec,     dinfo, first};
      launch_batched<double>(uplo == CHOL_UPPER, kmode, s, grid, p);
    } else {
      const BatchedArgs<float> p = {(float *)A, (float *)B, lda,   strideA, ldb,   strideB,
                                    n,          nrhs,       batch, vec,     dinfo, first};
      launch_batched<float>(uplo == CHOL_UPPER, kmode, s, grid, p);
    }
  });
}

// trtrs (solve) and trmm.  The forward half is L, the backward half L^T, L the lower factor however it is stored:
// (Lower, NoTrans) and (Upper, Trans) are forward.
int run_half(const char *what, bool solve, const ArgPos &pos, int uplo, int trans, int dtype, int n, int nrhs,
             double alpha, const void *A, int lda, long long strideA, void *B, int ldb, long long strideB, int batch,
             int *info) {
  if (int rc = check_images(what, pos, NAMES_HALF, uplo, trans, dtype, n, nrhs, A, lda, strideA, B, ldb, strideB,
                            batch, true, info))
    return rc < 0 ? rc : 0;
  const size_t es = dtype == CHOL_REAL_DOUBLE ? sizeof(double) : sizeof(float);
  const bool forward = (uplo == CHOL_LOWER) == (trans == CHOL_NOTRANS);
  const int op = solve ? (forward ? HALF_SOLVE_FWD : HALF_SOLVE_BWD) : (forward ? HALF_MUL_FWD : HALF_MUL_BWD);
  const bool zero = !solve && (dtype == CHOL_REAL_DOUBLE ? alpha == 0.0 : (float)alpha == 0.0f);
  const double el = zero ? 1.0 * n * nrhs : 0.5 * n * (n + 1.0) + 2.0 * n * nrhs;  // (alpha == 0: B written)
  return run_timed(what, n, batch, info, el * es * batch, [&](hipStream_t s, unsigned grid, int *dinfo, int *first) {
    const int NP = padded_order(n);
    const bool vec = rows_vec(A, lda, strideA, es);
    if (dtype == CHOL_REAL_DOUBLE) {
      const HalfArgs<double> p = {(const double *)A, (double *)B, lda, strideA, ldb,   strideB, n,
                                  nrhs,              batch,       vec, alpha,   dinfo, first};
      if (zero) k_zero_rows<double><<<grid, BATCHED_THREADS, 0, s>>>(p.B, ldb, strideB, n, nrhs, batch, NP);
      else launch_half_rows<double>(uplo == CHOL_UPPER, op, s, grid, p);
    } else {
      const HalfArgs<float> p = {(const float *)A, (float *)B, lda, strideA,      ldb,   strideB, n,
                                 nrhs,             batch,      vec, (float)alpha, dinfo, first};
      if (zero) k_zero_rows<float><<<grid, BATCHED_THREADS, 0, s>>>(p.B, ldb, strideB, n, nrhs, batch, NP);
      else launch_half_rows<float>(uplo == CHOL_UPPER, op, s, grid, p);
    }
  });
}

// logdet: the diagonal alone, the values to a device array
int run_logdet(int dtype, int n, const void *A, int lda, long long strideA, int batch, double *logdet, int *info) {
  const char *what = "logdet_batched";
  const int rc = check_images(what, POS_LOGDET, NAMES_HALF, 0, 0, dtype, n, 0, A, lda, strideA, nullptr, 1, 0, batch,
                              false, info);
  if (rc < 0) return rc;
  if (batch == 0) return 0;
  if (!logdet || !is_device_ptr(logdet)) return failf(-7, "%s: logdet must be a device pointer", what);
  if (rc) {  // n = 0: the determinant of the empty matrix is 1
    return with_views({}, [&]() -> int {
      hipStream_t s = main_rank_ctx()->st[ST_MAIN];
      HIPCHECK(hipMemsetAsync(logdet, 0, (size_t)batch * sizeof(double), s));
      HIPCHECK(hipStreamSynchronize(s));
      return 0;
    });
  }
  const size_t es = dtype == CHOL_REAL_DOUBLE ? sizeof(double) : sizeof(float);
  const double bytes = (1.0 * n * es + sizeof(double)) * batch;
  return run_timed(what, n, batch, info, bytes, [&](hipStream_t s, unsigned grid, int *dinfo, int *first) {
    const int NP = padded_order(n);
    if (dtype == CHOL_REAL_DOUBLE)
      k_diag_logdet<double>
          <<<grid, BATCHED_THREADS, 0, s>>>((const double *)A, lda, strideA, n, batch, NP, logdet, dinfo, first);
    else
      k_diag_logdet<float>
          <<<grid, BATCHED_THREADS, 0, s>>>((const float *)A, lda, strideA, n, batch, NP, logdet, dinfo, first);
  });
}

// trtri, potri, poinv (D == nullptr, pos = POS_POTRF) and invdiag (D: n elements per matrix at strideD, A only read)
int run_inv(const char *what, int mode, const ArgPos &pos, int uplo, int dtype, int n, void *A, int lda,
            long long strideA, void *D, long long strideD, int batch, int *info) {
  // (D is checked as an n x 1 image of leading dimension max(1, n): strideD >= n, also for n = 0)
  if (int rc = check_images(what, pos, NAMES_INV, uplo, 0, dtype, n, n ? 1 : 0, A, lda, strideA, D, n > 1 ? n : 1,
                            strideD, batch, false, info))
    return rc < 0 ? rc : 0;
  const size_t es = dtype == CHOL_REAL_DOUBLE ? sizeof(double) : sizeof(float);
  const bool vec = rows_vec(A, lda, strideA, es);
  const double tri = 0.5 * n * (n + 1.0), el = mode == INV_DIAG ? tri + n : 2.0 * tri;
  return run_timed(what, n, batch, info, el * es * batch, [&](hipStream_t s, unsigned grid, int *dinfo, int *first) {
    if (dtype == CHOL_REAL_DOUBLE) {
      const InvArgs<double> p = {(double *)A, (double *)D, lda, strideA, strideD, n, batch, vec, dinfo, first};
      launch_inv_rows<double>(uplo == CHOL_UPPER, mode, s, grid, p);
    } else {
      const InvArgs<float> p = {(float *)A, (float *)D, lda, strideA, strideD, n, batch, vec, dinfo, first};
      launch_inv_rows<float>(uplo == CHOL_UPPER, mode, s, grid, p);
    }
  });
}

}  // namespace

void cholmi::batched_release() {
  bt.release();
  for (hipEvent_t &e : bt_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

// ---------------------------------------------------------------- the entry points (C linkage: include/cholmi.h)
int chol_potrf_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info) {
  return run_batched("potrf_batched", MODE_POTRF, POS_POTRF, uplo, dtype, n, 0, A, lda, strideA, nullptr, 1, 0, batch,
                     info);
}

int chol_potrs_batched(int uplo, int dtype, int n, int nrhs, const void *A, int lda, long long strideA, void *B,
                       int ldb, long long strideB, int batch, int *info) {
  return run_batched("potrs_batched", MODE_POTRS, POS_SOLVE, uplo, dtype, n, nrhs, const_cast<void *>(A), lda, strideA,
                     B, ldb, strideB, batch, info);
}

int chol_posv_batched(int uplo, int dtype, int n, int nrhs, void *A, int lda, long long strideA, void *B, int ldb,
                      long long strideB, int batch, int *info) {
  return run_batched("posv_batched", MODE_POSV, POS_SOLVE, uplo, dtype, n, nrhs, A, lda, strideA, B, ldb, strideB,
                     batch, info);
}

int chol_chud_batched(int uplo, int dtype, int n, int r, void *A, int lda, long long strideA, const void *V, int ldv,
                      long long strideV, int batch, int *info) {
  return run_batched("chud_batched", MODE_CHUD, POS_SOLVE, uplo, dtype, n, r, A, lda, strideA, const_cast<void *>(V),
                     ldv, strideV, batch, info);
}

int chol_chdd_batched(int uplo, int dtype, int n, int r, void *A, int lda, long long strideA, const void *V, int ldv,
                      long long strideV, int batch, int *info) {
  return run_batched("chdd_batched", MODE_CHDD, POS_SOLVE, uplo, dtype, n, r, A, lda, strideA, const_cast<void *>(V),
                     ldv, strideV, batch, info);
}

int chol_trtrs_batched(int uplo, int trans, int dtype, int n, int nrhs, const void *A, int lda, long long strideA,
                       void *B, int ldb, long long strideB, int batch, int *info) {
  return run_half("trtrs_batched", true, POS_TRTRS, uplo, trans, dtype, n, nrhs, 1.0, A, lda, strideA, B, ldb, strideB,
                  batch, info);
}

int chol_trmm_batched(int uplo, int trans, int dtype, int n, int nrhs, double alpha, const void *A, int lda,
                      long long strideA, void *B, int ldb, long long strideB, int batch) {
  return run_half("trmm_batched", false, POS_TRMM, uplo, trans, dtype, n, nrhs, alpha, A, lda, strideA, B, ldb,
                  strideB, batch, nullptr);
}

int chol_logdet_batched(int dtype, int n, const void *A, int lda, long long strideA, int batch, double *logdet,
                        int *info) {
  return run_logdet(dtype, n, A, lda, strideA, batch, logdet, info);
}

int chol_trtri_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info) {
  return run_inv("trtri_batched", INV_TRTRI, POS_POTRF, uplo, dtype, n, A, lda, strideA, nullptr, 0, batch, info);
}

int chol_potri_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info) {
  return run_inv("potri_batched", INV_POTRI, POS_POTRF, uplo, dtype, n, A, lda, strideA, nullptr, 0, batch, info);
}

int chol_poinv_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info) {
  return run_inv("poinv_batched", INV_POINV, POS_POTRF, uplo, dtype, n, A, lda, strideA, nullptr, 0, batch, info);
}

int chol_invdiag_batched(int uplo, int dtype, int n, const void *A, int lda, long long strideA, void *D,
                         long long strideD, int batch, int *info) {
  return run_inv("invdiag_batched", INV_DIAG, POS_INVDIAG, uplo, dtype, n, const_cast<void *>(A), lda, strideA, D,
                 strideD, batch, info);
}

int chol_last_batched_stats(double *out8) {
  if (!ctx_inited()) return fail(CHOL_ERR_NOT_INITIALIZED, "last_batched_stats before chol_init");
  if (!out8) return fail(-1, "last_batched_stats: NULL");
  std::lock_guard<std::recursive_mutex> lk(ctx_mutex());
  std::copy(bt_stats, bt_stats + 8, out8);
  return 0;
}
