// The condition estimate from the factor (api.hip: chol_lansy_tile, chol_pocon_tile, LAPACK DLANSY / DPOCON) on a
// single-process, device-resident tile image: stored tiles of mbs x mbs elements of which the caller's tile is the
// leading mbu x mbu part (TileGeo, cholmi_internal.h).  Every kernel reads only the stored triangle.
//
// Geometry.  The image is cut into 128 x 128 blocks of STORED rows / columns: block row b is stored rows
// [128 (b % bpt), +128) of tile row b / bpt, bpt = ceil(mbs / 128), so every block lies inside one tile.  Entries
// outside the matrix (a ragged last tile, a tile edge mbu < mbs) are masked BEFORE they are loaded: their storage
// may hold anything, and for an edge that is not a multiple of 128 it may not exist.  The N-vectors use the same
// cut: entry t of block b at v[128 b + t], zero outside the matrix; in that order the entries inside the matrix
// are in global row order, so "the first index" of idamax is the first in storage order.
//
// lansy: one workgroup per stored block of the triangle, as mixed.hip's residual: the row sums of |A| of the
// block's rows and its column sums (the strict half of a diagonal block) go to per-block partials that a second
// pass adds up per row in a fixed order; the max and the weighted sum of squares of each block are reduced
// order-independently (integer max on the bits of a non-negative double) or in a fixed order.
//
// The sweeps: L y = b and then L^T x = y, one tile column per step.  Two forms of one scheme live here: pocon's own
// one-vector kernels (k_sweep_*) and the multi-vector kernels (k_msweep_*) of porfs, posvx and trtrs for NV = 1, 2, 4
// or 8 vectors, each 128 x 128 block of the factor read once per launch for all of them.  pocon does not run the
// NV = 1 instantiation: its application measured about 1 % slower so in fp64 (profiles/fold_blocks_ab.txt).
// The diagonal tiles are inverted once per call (their 128-blocks by kernels.hip's diagonal-block kernel, then
// the tile by inverse.hip's inner level), so that the step's serial part is a product, not a chain of solves.
// Step k is two launches, each spread over 128 x 128 blocks, one workgroup per block:
//   diag:  partial (rho, kappa) = Dinv_k(rho, kappa) r_k(kappa)    (forward; the transposed block backward)
//   rect:  y_k = the diag partials of the block, added in a fixed order (the workgroups of row 0 store it)
//          partial (rho, kappa) = L(rho, kappa) y_k(kappa) for every block row rho of the tiles still to come
// A rect launch's partials are subtracted from r where they are next needed: by the next diag launch for the rows
// of its tile (on the fly) and by the next rect launch for all other rows (its kappa = 0 workgroup of each row
// folds them into r).  Every element is thus summed by one lane in a fixed order, with no floating-point atomics
// and no hand-off inside a launch: the result is bit-identical from run to run.
#include <cfloat>

#include "cholmi_internal.h"
#include "sweep_blocks.h"

namespace cholmi {

namespace {

// ---------------------------------------------------------------- lansy
// part[(pair * 2 + kind) * 128 + t]: kind 0 -> rows of block row P, kind 1 -> rows of block row Q (the row sums of
// |A| of the symmetric matrix); ssq[pair]: the block's share of the sum of squares (off-diagonal entries twice);
// res[0]: bits of max |a|
template <typename T>
__global__ __launch_bounds__(256) void k_lansy_blocks(TileGeo g, int upper, const T *__restrict__ A,
                                                      double *__restrict__ part, double *__restrict__ ssq,
                                                      unsigned long long *res) {
  const long pair = blockIdx.x;
  const TriBlock<T> b = tri_block<T>(g, A, upper, pair);
  const bool diag = b.tri != 0;
  __shared__ double srow[4][CB];
  __shared__ double sred[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = 2 * lane;
  double racc0 = 0, racc1 = 0, cres = 0, amax = 0, sqs = 0, sqd = 0;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    const int c = w * 32 + k;
    T t0, t1;
    load_pair<T>(b.S, g.mbs, r, c, b.vr, b.vc, b.tri, t0, t1);
    const double a0 = fabs((double)t0), a1 = fabs((double)t1);
    // the row sums take the stored half with the diagonal, the column sums the strict half
    const bool d0 = diag && r == c, d1 = diag && r + 1 == c;
    const double ca0 = d0 ? 0.0 : a0, ca1 = d1 ? 0.0 : a1;
    const double da0 = d0 ? a0 : 0.0, da1 = d1 ? a1 : 0.0;  // (selected, not a0 - ca0: Inf - Inf would be a NaN)
    racc0 += a0;
    racc1 += a1;
    const double s = wave_sum<double>(ca0 + ca1);
    if (lane == k) cres = s;
    amax = nan_max(amax, nan_max(a0, a1));
    sqs = fma(ca1, ca1, fma(ca0, ca0, sqs));                   // strict entries: twice (the other triangle)
    sqd = fma(da1, da1, fma(da0, da0, sqd));                   // the diagonal: once
  }
  srow[w][r] = racc0;
  srow[w][r + 1] = racc1;
  // max: order-independent; sum of squares: a fixed tree
  double m = amax;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  const double wsq = wave_sum<double>(2.0 * sqs + sqd);
  if (lane == 0) {
    sred[0][w] = m;
    sred[1][w] = wsq;
  }
  __syncthreads();
  const int krow = upper ? 1 : 0, kcol = 1 - krow;
  double *prow = part + (pair * 2 + krow) * CB, *pcol = part + (pair * 2 + kcol) * CB;
  if (tid < CB) prow[tid] = ((srow[0][tid] + srow[1][tid]) + srow[2][tid]) + srow[3][tid];
  if (lane < 32) pcol[w * 32 + lane] = cres;
  if (tid == 0) {
    const double bm = nan_max(nan_max(sred[0][0], sred[0][1]), nan_max(sred[0][2], sred[0][3]));
    atomicMax(res, (unsigned long long)__double_as_longlong(bm));
    ssq[pair] = ((sred[1][0] + sred[1][1]) + sred[1][2]) + sred[1][3];
  }
}

// the row sums, added in the fixed order of for_row_partials; res[1]: bits of their max
__global__ __launch_bounds__(256) void k_lansy_rows(TileGeo g, const double *__restrict__ part,
                                                    unsigned long long *res) {
  const int NB = g.lmt * bpt_of(g);
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= (long)NB * CB) return;
  const int P = (int)(s / CB), t = (int)(s % CB);
  if (t >= block_valid(g, P)) return;
  double sum = 0.0;
  for_row_partials(P, NB, [&](long pair, int kind) { sum += part[(pair * 2 + kind) * CB + t]; });
  atomicMax(res + 1, (unsigned long long)__double_as_longlong(sum));
}

// res[2] <- the sum of ssq[0 .. n), in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_lansy_ssq(const double *__restrict__ ssq, long n, double *res) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) acc += ssq[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) res[2] = sh[0];
}

// ---------------------------------------------------------------- the diagonal tiles' inverses
// Dv tile k (E x E, ld E) <- the lower triangle of L(k,k) (Upper: U(k,k)^T), zero above the diagonal, the identity
// outside the matrix.  One 64 x 64 block per workgroup, through LDS so that Upper is read coalesced.
template <typename T>
__global__ __launch_bounds__(256) void k_stage_diag(TileGeo g, int upper, const T *__restrict__ A, T *__restrict__ Dv,
                                                    int E) {
  const int k = blockIdx.y, nb = E / 64, rb = blockIdx.x % nb, cb = blockIdx.x / nb;
  const int vk = (int)min((long)g.mbu, g.m - (long)k * g.mbu);
  const T *Ak = A + (long)k * (g.lmt + 1) * g.mbs * g.mbs;
  T *dst = Dv + (long)k * E * E + (long)rb * 64 + (long)cb * 64 * E;
  __shared__ T sh[64][65];
  if (rb >= cb) {
    // source rows sr0.., columns sc0.. of the stored tile, read down its columns
    const int sr0 = (upper ? cb : rb) * 64, sc0 = (upper ? rb : cb) * 64;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
      const int rr = e % 64, cc = e / 64, sr = sr0 + rr, sc = sc0 + cc;
      const bool ref = upper ? sr <= sc : sr >= sc;
      sh[cc][rr] = (sr < vk && sc < vk && ref) ? Ak[sr + (long)sc * g.mbs] : T(0);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int rr = e % 64, cc = e / 64, r = rb * 64 + rr, c = cb * 64 + cc;
    T v;
    if (r >= vk || c >= vk) v = r == c ? T(1) : T(0);
    else if (r < c) v = T(0);
    else v = upper ? sh[rr][cc] : sh[cc][rr];
    dst[rr + (long)cc * E] = v;
  }
}

// ---------------------------------------------------------------- the sweeps
// The input block kappa (local to tile k) of the diag launch: r - the pending partials of the previous rect launch
template <typename T>
__device__ __forceinline__ T pending_sub(const T *r, const T *pg, long rho, int bpt, int t) {
  T v = r[rho * CB + t];
  if (pg) {
    T s = 0;
    for (int c = 0; c < bpt; ++c) s += pg[(rho * bpt + c) * CB + t];
    v -= s;
  }
  return v;
}

// step k, diagonal part: workgroup (P, Q), P >= Q, of Dinv_k; forward partial (P, Q) = Dinv(P,Q) v_Q, backward
// partial (Q, P) = Dinv(P,Q)^T v_P; pd[(rho * bpt + kappa) * 128 + t]
template <typename T, bool FWD>
__global__ __launch_bounds__(256) void k_sweep_diag(TileGeo g, const T *__restrict__ Dk, int E, int k,
                                                    const T *__restrict__ r, const T *__restrict__ pg,
                                                    T *__restrict__ pd) {
  int P, Q;
  pair_of(blockIdx.x, P, Q);
  const int bpt = E / CB;
  const long kb0 = (long)k * bpt;
  const int rho = FWD ? P : Q, kap = FWD ? Q : P;
  __shared__ T sv[CB], so[CB];
  __shared__ T red[4][CB];
  if (threadIdx.x < CB) sv[threadIdx.x] = pending_sub<T>(r, pg, kb0 + kap, bpt, threadIdx.x);
  __syncthreads();
  const int vr = block_valid(g, (int)kb0 + P), vc = block_valid(g, (int)kb0 + Q);
  block_product<T, !FWD>(Dk + (long)P * CB + (long)Q * CB * E, E, vr, vc, P == Q, sv, so, red);
  if (threadIdx.x < CB) pd[((long)rho * bpt + kap) * CB + threadIdx.x] = so[threadIdx.x];
}

// step k, the blocks below (forward) / above (backward) tile k: workgroup (i, kappa) of block row rho = row0 + i and
// block column kb0 + kappa.  y_k(kappa) from the diag partials; nrows == 0: only y_k is stored.
template <typename T, bool FWD>
__global__ __launch_bounds__(256) void k_sweep_rect(TileGeo g, int upper, const T *__restrict__ A, int k, int row0,
                                                    int nrows, T *__restrict__ r, const T *__restrict__ pg_prev,
                                                    T *__restrict__ pg, const T *__restrict__ pd, T *__restrict__ yout) {
  const int bpt = bpt_of(g), i = blockIdx.x / bpt, kap = blockIdx.x % bpt, t = threadIdx.x;
  const long kb0 = (long)k * bpt, rho = row0 + i;
  __shared__ T sv[CB], so[CB];
  __shared__ T red[4][CB];
  if (t < CB) {
    // y_k(kappa): forward the partials (kappa, c), c <= kappa; backward (kappa, c), c >= kappa
    T y = 0;
    for (int c = FWD ? 0 : kap; c <= (FWD ? kap : bpt - 1); ++c) y += pd[((long)kap * bpt + c) * CB + t];
    sv[t] = y;
    if (i == 0) yout[(kb0 + kap) * CB + t] = y;
    // the previous rect launch's partials of this row (every row of this launch was one of its rows)
    if (nrows > 0 && kap == 0 && pg_prev) {
      T s = 0;
      for (int c = 0; c < bpt; ++c) s += pg_prev[(rho * bpt + c) * CB + t];
      r[rho * CB + t] -= s;
    }
  }
  if (nrows == 0) return;
  __syncthreads();
  // forward L(rho, kappa) y: Lower the stored block (rho, kappa), Upper U(kappa, rho)^T; backward L(kappa, rho)^T y:
  // Lower the stored block (kappa, rho) transposed, Upper U(rho, kappa)
  const int kg = (int)(kb0 + kap);
  const bool trans = FWD ? upper : !upper;
  const int sr = trans ? kg : (int)rho, sc = trans ? (int)rho : kg;
  const T *S = block_at<T>(g, A, sr, sc);
  const int vr = block_valid(g, sr), vc = block_valid(g, sc);
  if (trans)
    block_product<T, true>(S, g.mbs, vr, vc, false, sv, so, red);
  else
    block_product<T, false>(S, g.mbs, vr, vc, false, sv, so, red);
  if (t < CB) pg[(rho * bpt + kap) * CB + t] = so[t];
}

// ---------------------------------------------------------------- the multi-vector sweeps (porfs, posvx, trtrs)
template <typename T>
struct Vec8 {
  T *p[8];
};

// step k, diagonal part, NV vectors: workgroup (P, Q), P >= Q, of Dinv_k; forward partial (P, Q) = Dinv(P,Q) v_Q,
// backward partial (Q, P) = Dinv(P,Q)^T v_P; vector j's pending partials at pg + j pgn, its diag partials at
// pd + j pdn + (rho * bpt + kappa) * 128 + t
template <typename T, bool FWD, int NV>
__global__ __launch_bounds__(256) void k_msweep_diag(TileGeo g, const T *__restrict__ Dk, int E, int k, Vec8<T> r,
                                                     const T *__restrict__ pg, long pgn, T *__restrict__ pd, long pdn) {
  int P, Q;
  pair_of(blockIdx.x, P, Q);
  const int bpt = E / CB;
  const long kb0 = (long)k * bpt;
  const int rho = FWD ? P : Q, kap = FWD ? Q : P;
  __shared__ T sv[NV][CB], so[NV][CB];
  __shared__ T red[4][NV][CB];
  for (int e = threadIdx.x; e < NV * CB; e += 256) {
    const int j = e / CB, t = e % CB;
    // the input block kappa (local to tile k): r - the pending partials of the previous rect launch
    T v = r.p[j][(kb0 + kap) * CB + t];
    if (pg) {
      T sp = 0;
      for (int c = 0; c < bpt; ++c) sp += pg[j * pgn + ((kb0 + kap) * bpt + c) * CB + t];
      v -= sp;
    }
    sv[j][t] = v;
  }
  __syncthreads();
  const int vr = block_valid(g, (int)kb0 + P), vc = block_valid(g, (int)kb0 + Q);
  // (the staged tiles are Lower: a diagonal block's half on or below the diagonal, never the upper one)
  const T *S = Dk + (long)P * CB + (long)Q * CB * E;
  block_product_nv<T, !FWD, NV, false>(S, E, vr, vc, P == Q ? 1 : 0, sv, so, red);
  for (int e = threadIdx.x; e < NV * CB; e += 256) {
    const int j = e / CB, t = e % CB;
    pd[j * pdn + ((long)rho * bpt + kap) * CB + t] = so[j][t];
  }
}

// step k, the blocks below (forward) / above (backward) tile k, NV vectors: workgroup (i, kappa) of block row
// rho = row0 + i and block column kb0 + kappa.  y_k(kappa) from the diag partials; nrows == 0: only y_k is stored.
template <typename T, bool FWD, int NV>
__global__ __launch_bounds__(256) void k_msweep_rect(TileGeo g, int upper, const T *__restrict__ A, int k, int row0,
                                                     int nrows, Vec8<T> r, const T *__restrict__ pg_prev,
                                                     T *__restrict__ pg, long pgn, const T *__restrict__ pd, long pdn,
                                                     Vec8<T> yout) {
  const int bpt = bpt_of(g), i = blockIdx.x / bpt, kap = blockIdx.x % bpt;
  const long kb0 = (long)k * bpt, rho = row0 + i;
  __shared__ T sv[NV][CB], so[NV][CB];
  __shared__ T red[4][NV][CB];
  for (int e = threadIdx.x; e < NV * CB; e += 256) {
    const int j = e / CB, t = e % CB;
    // y_k(kappa): forward the partials (kappa, c), c <= kappa; backward (kappa, c), c >= kappa
    T y = 0;
    for (int c = FWD ? 0 : kap; c <= (FWD ? kap : bpt - 1); ++c) y += pd[j * pdn + ((long)kap * bpt + c) * CB + t];
    sv[j][t] = y;
    if (i == 0) yout.p[j][(kb0 + kap) * CB + t] = y;
    // the previous rect launch's partials of this row (every row of this launch was one of its rows)
    if (nrows > 0 && kap == 0 && pg_prev) {
      T s = 0;
      for (int c = 0; c < bpt; ++c) s += pg_prev[j * pgn + (rho * bpt + c) * CB + t];
      r.p[j][rho * CB + t] -= s;
    }
  }
  if (nrows == 0) return;
  __syncthreads();
  // forward L(rho, kappa) y: Lower the stored block (rho, kappa), Upper U(kappa, rho)^T; backward L(kappa, rho)^T y:
  // Lower the stored block (kappa, rho) transposed, Upper U(rho, kappa)
  const int kg = (int)(kb0 + kap);
  const bool trans = FWD ? upper : !upper;
  const int sr = trans ? kg : (int)rho, sc = trans ? (int)rho : kg;
  const T *S = block_at<T>(g, A, sr, sc);
  const int vr = block_valid(g, sr), vc = block_valid(g, sc);
  if (trans)
    block_product_nv<T, true, NV, false>(S, g.mbs, vr, vc, 0, sv, so, red);
  else
    block_product_nv<T, false, NV, false>(S, g.mbs, vr, vc, 0, sv, so, red);
  for (int e = threadIdx.x; e < NV * CB; e += 256) {
    const int j = e / CB, t = e % CB;
    pg[j * pgn + (rho * bpt + kap) * CB + t] = so[j][t];
  }
}

// which: SWEEP_BOTH x <- A^{-1} x; SWEEP_FORWARD / SWEEP_BACKWARD that half alone, its result left in the y vectors
// (b.y + j nv) and x used up
template <typename T, int NV>
void msweep(hipStream_t s, const TileGeo &g, int upper, const T *A, const T *Dv, const Vec8<T> &x, const MSweepBufs<T> &b,
            int which) {
  const int E = condest_edge(g), bpt = E / CB, nt = g.lmt, NB = nt * bpt;
  const unsigned dwg = (unsigned)(bpt * (bpt + 1) / 2);
  const long nv = (long)condest_vec_elems(g), pgs = (long)NB * bpt * CB, pgn = 2 * pgs, pdn = (long)bpt * bpt * CB;
  Vec8<T> y{};
  for (int j = 0; j < NV; ++j) y.p[j] = b.y + j * nv;
  const bool half = which != SWEEP_BOTH;
  for (int pass = which == SWEEP_BACKWARD ? 1 : 0; pass < (which == SWEEP_FORWARD ? 1 : 2); ++pass) {
    const bool fwd = pass == 0;
    // forward: b = x -> y; backward: y -> x (r: in place); one half alone: x -> y
    const Vec8<T> r = fwd || half ? x : y, out = fwd || half ? y : x;
    const T *pg_prev = nullptr;
    for (int step = 0; step < nt; ++step) {
      const int k = fwd ? step : nt - 1 - step;
      T *pg = b.pg + (step % 2) * pgs;
      const T *Dk = Dv + (long)k * E * E;
      if (fwd)
        hipLaunchKernelGGL((k_msweep_diag<T, true, NV>), dim3(dwg), dim3(256), 0, s, g, Dk, E, k, r, pg_prev, pgn, b.pd,
                           pdn);
      else
        hipLaunchKernelGGL((k_msweep_diag<T, false, NV>), dim3(dwg), dim3(256), 0, s, g, Dk, E, k, r, pg_prev, pgn, b.pd,
                           pdn);
      const int row0 = fwd ? (k + 1) * bpt : 0, nrows = fwd ? NB - (k + 1) * bpt : k * bpt;
      const unsigned rwg = (unsigned)(std::max(nrows, 1) * bpt);
      if (fwd)
        hipLaunchKernelGGL((k_msweep_rect<T, true, NV>), dim3(rwg), dim3(256), 0, s, g, upper, A, k, row0, nrows, r,
                           pg_prev, pg, pgn, b.pd, pdn, out);
      else
        hipLaunchKernelGGL((k_msweep_rect<T, false, NV>), dim3(rwg), dim3(256), 0, s, g, upper, A, k, row0, nrows, r,
                           pg_prev, pg, pgn, b.pd, pdn, out);
      pg_prev = pg;
    }
  }
}

// ---------------------------------------------------------------- the estimator's vector operations
// x over the NB * 128 entries: mode 0 -> 1/n, 1 -> e_j (j a storage index), 2 -> the alternating-sign vector
// (-1)^i (1 + i / (n - 1)) of DLACN2's last step (i the 0-based global row); zero outside the matrix
template <typename T>
__global__ __launch_bounds__(256) void k_vec_fill(TileGeo g, T *__restrict__ x, int mode, long j) {
  const long total = (long)g.lmt * bpt_of(g) * CB;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long b = e / CB;
    const int t = (int)(e % CB);
    T v = 0;
    if (t < block_valid(g, (int)b)) {
      const long gi = global_row(g, b, t);
      if (mode == 0) v = T(1) / T(g.m);
      else if (mode == 1) v = e == j ? T(1) : T(0);
      else v = (gi % 2 ? T(-1) : T(1)) * (T(1) + T(gi) / T(g.m - 1));
    }
    x[e] = v;
  }
}

constexpr int STAT_WG = 256;  // workgroups of the statistics pass

// per workgroup (a fixed range of entries): sum |x|, max |x| and its first storage index, a non-finite entry;
// sign != 0: x <- sign(x) (x >= 0 -> +1) and isgn <- the same, *differ = 1 where it changes isgn
template <typename T>
__global__ __launch_bounds__(256) void k_vec_stats(TileGeo g, T *__restrict__ x, int *__restrict__ isgn, int sign,
                                                   double *__restrict__ part, int *differ) {
  const long total = (long)g.lmt * bpt_of(g) * CB;
  const long per = (total + STAT_WG - 1) / STAT_WG, lo = blockIdx.x * per, hi = min(total, lo + per);
  __shared__ T ssum[256], smax[256];
  __shared__ long sidx[256];
  __shared__ int sbad[256];
  T asum = 0, amax = -1;
  long imax = -1;
  int bad = 0, dif = 0;
  for (long e = lo + threadIdx.x; e < hi; e += 256) {
    if ((int)(e % CB) >= block_valid(g, (int)(e / CB))) continue;
    const T v = x[e], a = fabs(v);
    if (!isfinite(v)) bad = 1;
    asum += a;
    if (a > amax) amax = a, imax = e;  // (ascending e per thread: the first on ties)
    if (sign) {
      const int s = v >= T(0) ? 1 : -1;
      if (isgn[e] != s) dif = 1;
      isgn[e] = s;
      x[e] = T(s);
    }
  }
  if (dif) atomicOr(differ, 1);
  ssum[threadIdx.x] = asum;
  smax[threadIdx.x] = amax;
  sidx[threadIdx.x] = imax;
  sbad[threadIdx.x] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    const int t = threadIdx.x;
    if (t < o) {
      ssum[t] += ssum[t + o];
      sbad[t] |= sbad[t + o];
      const T m2 = smax[t + o];
      const long i2 = sidx[t + o];
      if (m2 > smax[t] || (m2 == smax[t] && i2 >= 0 && (sidx[t] < 0 || i2 < sidx[t]))) smax[t] = m2, sidx[t] = i2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *p = part + blockIdx.x * 4;
    p[0] = (double)ssum[0];
    p[1] = (double)smax[0];
    p[2] = (double)sidx[0];
    p[3] = (double)sbad[0];
  }
}

// out[0..5] <- sum |x| (in T, the workgroups in order), max |x|, its first storage index, non-finite, x[jlast]
// (jlast >= 0), the sign-change flag
template <typename T>
__global__ __launch_bounds__(64) void k_vec_final(const double *__restrict__ part, const T *__restrict__ x, long jlast,
                                                  const int *differ, double *out) {
  if (threadIdx.x != 0) return;
  T asum = 0;
  double amax = -1, imax = -1, bad = 0;
  for (int w = 0; w < STAT_WG; ++w) {
    const double *p = part + w * 4;
    asum += (T)p[0];
    if (p[2] >= 0 && p[1] > amax) amax = p[1], imax = p[2];  // (workgroups in ascending ranges: first on ties)
    if (p[3] != 0) bad = 1;
  }
  out[0] = (double)asum;
  out[1] = amax;
  out[2] = imax;
  out[3] = bad;
  out[4] = jlast >= 0 ? (double)x[jlast] : 0.0;
  out[5] = (double)*differ;
}

}  // namespace

// ---------------------------------------------------------------- launchers
size_t lansy_part_bytes(const TileGeo &g) { return (size_t)tri_pairs(g) * (2 * CB + 1) * sizeof(double); }

template <typename T>
void launch_lansy(hipStream_t s, const TileGeo &g, int upper, const T *A, double *part, double *res) {
  const long NB = block_rows(g), pairs = tri_pairs(g);
  double *ssq = part + pairs * 2 * CB;
  auto *bits = reinterpret_cast<unsigned long long *>(res);
  (void)hipMemsetAsync(res, 0, 3 * sizeof(double), s);
  if (!pairs) return;
  hipLaunchKernelGGL(k_lansy_blocks<T>, dim3((unsigned)pairs), dim3(256), 0, s, g, upper, A, part, ssq, bits);
  hipLaunchKernelGGL(k_lansy_rows, dim3((unsigned)((NB * CB + 255) / 256)), dim3(256), 0, s, g, part, bits);
  hipLaunchKernelGGL(k_lansy_ssq, dim3(1), dim3(256), 0, s, ssq, pairs, res);
}

int condest_edge(const TileGeo &g) { return (g.mbs + CB - 1) / CB * CB; }

size_t condest_vec_elems(const TileGeo &g) { return (size_t)block_rows(g) * CB; }

template <typename T>
void launch_stage_diag(hipStream_t s, const TileGeo &g, int upper, const T *A, T *Dv) {
  const int E = condest_edge(g), nb = E / 64;
  if (g.lmt > 0)
    hipLaunchKernelGGL(k_stage_diag<T>, dim3((unsigned)(nb * nb), (unsigned)g.lmt), dim3(256), 0, s, g, upper, A, Dv, E);
}

template <typename T>
void launch_sweep(hipStream_t s, const TileGeo &g, int upper, const T *A, const T *Dv, const SweepBufs<T> &b) {
  const int E = condest_edge(g), bpt = E / CB, nt = g.lmt, NB = nt * bpt;
  const unsigned dwg = (unsigned)(bpt * (bpt + 1) / 2);
  const long pgs = (long)NB * bpt * CB;
  for (int pass = 0; pass < 2; ++pass) {
    const bool fwd = pass == 0;
    T *r = fwd ? b.x : b.y, *out = fwd ? b.y : b.x;  // forward: b = x -> y; backward: y -> x (r: in place)
    const T *pg_prev = nullptr;
    for (int step = 0; step < nt; ++step) {
      const int k = fwd ? step : nt - 1 - step;
      T *pg = b.pg + (step % 2) * pgs;
      const T *Dk = Dv + (long)k * E * E;
      if (fwd)
        hipLaunchKernelGGL((k_sweep_diag<T, true>), dim3(dwg), dim3(256), 0, s, g, Dk, E, k, r, pg_prev, b.pd);
      else
        hipLaunchKernelGGL((k_sweep_diag<T, false>), dim3(dwg), dim3(256), 0, s, g, Dk, E, k, r, pg_prev, b.pd);
      const int row0 = fwd ? (k + 1) * bpt : 0, nrows = fwd ? NB - (k + 1) * bpt : k * bpt;
      const unsigned rwg = (unsigned)(std::max(nrows, 1) * bpt);
      if (fwd)
        hipLaunchKernelGGL((k_sweep_rect<T, true>), dim3(rwg), dim3(256), 0, s, g, upper, A, k, row0, nrows, r, pg_prev,
                           pg, b.pd, out);
      else
        hipLaunchKernelGGL((k_sweep_rect<T, false>), dim3(rwg), dim3(256), 0, s, g, upper, A, k, row0, nrows, r, pg_prev,
                           pg, b.pd, out);
      pg_prev = pg;
    }
  }
}

size_t msweep_scratch_elems(const TileGeo &g) {
  const long bpt = (condest_edge(g) / CB), NB = block_rows(g), nv = (long)condest_vec_elems(g);
  return (size_t)8 * (nv + 2 * NB * bpt * CB + bpt * bpt * CB);
}

template <typename T>
void launch_msweep(hipStream_t s, const TileGeo &g, int upper, const T *A, const T *Dv, T *const *x, int count,
                   T *pad, const MSweepBufs<T> &b, int which) {
  const long nv = (long)condest_vec_elems(g);
  with_width(count, [&](auto width) {
    constexpr int NV = decltype(width)::value;
    Vec8<T> v{};
    for (int j = 0; j < NV; ++j) v.p[j] = j < count ? x[j] : pad + (long)(j - count) * nv;  // (padding: results unused)
    msweep<T, NV>(s, g, upper, A, Dv, v, b, which);
  });
}

template <typename T>
void launch_vec_fill(hipStream_t s, const TileGeo &g, T *x, int mode, long j) {
  const long total = (long)condest_vec_elems(g);
  const unsigned grid = (unsigned)std::max(1L, std::min((total + 255) / 256, 4096L));
  hipLaunchKernelGGL(k_vec_fill<T>, dim3(grid), dim3(256), 0, s, g, x, mode, j);
}

size_t vec_stats_part_bytes() { return (size_t)STAT_WG * 4 * sizeof(double) + 64; }

template <typename T>
void launch_vec_stats(hipStream_t s, const TileGeo &g, T *x, int *isgn, int sign, long jlast, double *part,
                      double *out) {
  int *differ = reinterpret_cast<int *>(part + STAT_WG * 4);
  (void)hipMemsetAsync(differ, 0, sizeof(int), s);
  hipLaunchKernelGGL(k_vec_stats<T>, dim3(STAT_WG), dim3(256), 0, s, g, x, isgn, sign, part, differ);
  hipLaunchKernelGGL(k_vec_final<T>, dim3(1), dim3(64), 0, s, part, x, jlast, differ, out);
}

#define INSTANTIATE_CONDEST(T)                                                                               \
  template void launch_lansy<T>(hipStream_t, const TileGeo &, int, const T *, double *, double *);           \
  template void launch_stage_diag<T>(hipStream_t, const TileGeo &, int, const T *, T *);                     \
  template void launch_sweep<T>(hipStream_t, const TileGeo &, int, const T *, const T *, const SweepBufs<T> &); \
  template void launch_msweep<T>(hipStream_t, const TileGeo &, int, const T *, const T *, T *const *, int, T *, \
                                 const MSweepBufs<T> &, int);                                                \
  template void launch_vec_fill<T>(hipStream_t, const TileGeo &, T *, int, long);                            \
  template void launch_vec_stats<T>(hipStream_t, const TileGeo &, T *, int *, int, long, double *, double *);
INSTANTIATE_CONDEST(double)
INSTANTIATE_CONDEST(float)

}  // namespace cholmi
