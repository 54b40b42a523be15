// The fp64 side of the mixed-precision SPD solve (api.hip: chol_dsposv_tile, LAPACK DSPOSV): the symmetric
// residual R = B - A X read from ONE stored triangle of A, the fp64 -> fp32 conversions with overflow detection,
// and the fp64 update X += C.  Single-process, device-resident tile images: stored tiles of mbs x mbs elements
// (mbs a multiple of 128) of which the caller's tile is the leading mbu x mbu part (TileGeo, cholmi_internal.h).
//
// The residual works on the 128 x 128 blocks of the stored image (sweep_blocks.h; see condest.hip for the geometry):
// every block lies inside one tile and padding is masked per entry.
// One workgroup per stored block of the triangle (pair (P, Q), P >= Q, of the symmetric matrix) reads the block
// once and produces both of its products: A(P,Q) X_Q (goes to R_P) and A(P,Q)^T X_P (goes to R_Q); a diagonal
// block is made symmetric from its stored half (the diagonal counted once).  The products are written as
// per-block partial sums and a second pass adds them up in a fixed order -- no floating-point atomics, so the
// residual is bit-identical from run to run.  The column max-abs values of R and X are by-products of that pass
// (integer atomicMax on the bit pattern of a non-negative double: order-independent).
#include <cfloat>
#include <type_traits>

#include "cholmi_internal.h"
#include "sweep_blocks.h"

namespace cholmi {

namespace {

__device__ __forceinline__ void atomic_max_abs(unsigned long long *addr, double v) {
  atomicMax(addr, (unsigned long long)__double_as_longlong(fabs(v)));
}

// One stored block of the triangle per workgroup (4 waves, 32 columns each; lane l holds rows 2l, 2l+1).
// part[((pair * 2 + kind) * NR + j) * 128 + t]: kind 0 -> row t of R_P, kind 1 -> row t of R_Q, rhs column j0 + j.
// ABS: |A| times a vector of ones (the row sums of |A|: the infinity norm of the symmetric matrix).
template <int NR, bool ABS>
__global__ __launch_bounds__(256) void k_sym_resid(TileGeo ga, int upper, const double *__restrict__ A, TileGeo gx,
                                                   const double *__restrict__ X, int j0, int nr,
                                                   double *__restrict__ part) {
  const long pair = blockIdx.x;
  const TriBlock<double> b = tri_block<double>(ga, A, upper, pair);
  const double *S = b.S;
  const int br = b.br, bc = b.bc, vr = b.vr, vc = b.vc;
  const bool diag = b.tri != 0;
  __shared__ double sv[NR][CB];        // X rows of the block's columns
  __shared__ double srow[4][NR][CB];   // per-wave row products
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int e = tid; e < NR * CB; e += 256) {
    const int j = e / CB, c = e % CB;
    double v = 0.0;
    if (c < vc && j < nr) v = ABS ? 1.0 : X[desc_index(gx, bc, c, j0 + j)];
    sv[j][c] = v;
  }
  double u[2][NR];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int r = 2 * lane + k;
      u[k][j] = (r < vr && j < nr) ? (ABS ? 1.0 : X[desc_index(gx, br, r, j0 + j)]) : 0.0;
    }
  __syncthreads();
  double racc[2][NR], cres[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) racc[0][j] = racc[1][j] = cres[j] = 0.0;
  const int r = 2 * lane;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    const int c = w * 32 + k;
    const double2 a = *reinterpret_cast<const double2 *>(S + (long)c * ga.mbs + r);
    // entries outside the matrix (and, in a diagonal block, the unreferenced half) by selection: they may hold NaN
    double a0 = (r < vr && c < vc) ? a.x : 0.0, a1 = (r + 1 < vr && c < vc) ? a.y : 0.0;
    if (ABS) a0 = fabs(a0), a1 = fabs(a1);
    // the row product takes the stored half with the diagonal, the column product the strict half
    double ra0 = a0, ra1 = a1, ca0 = a0, ca1 = a1;
    if (diag) {
      ra0 = (upper ? r <= c : r >= c) ? a0 : 0.0;
      ra1 = (upper ? r + 1 <= c : r + 1 >= c) ? a1 : 0.0;
      ca0 = (upper ? r < c : r > c) ? a0 : 0.0;
      ca1 = (upper ? r + 1 < c : r + 1 > c) ? a1 : 0.0;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const double v = sv[j][c];
      racc[0][j] = fma(ra0, v, racc[0][j]);
      racc[1][j] = fma(ra1, v, racc[1][j]);
      const double s = wave_sum<double>(fma(ca1, u[1][j], ca0 * u[0][j]));
      if (lane == k) cres[j] = s;
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    srow[w][j][r] = racc[0][j];
    srow[w][j][r + 1] = racc[1][j];
  }
  __syncthreads();
  // Lower: the row product is A(P,Q) X_Q (-> R_P), the column product A(P,Q)^T X_P (-> R_Q); Upper the other way round
  const int krow = upper ? 1 : 0, kcol = 1 - krow;
  double *prow = part + (pair * 2 + krow) * NR * CB, *pcol = part + (pair * 2 + kcol) * NR * CB;
  for (int e = tid; e < NR * CB; e += 256) {
    const int j = e / CB, t = e % CB;
    prow[e] = ((srow[0][j][t] + srow[1][j][t]) + srow[2][j][t]) + srow[3][j][t];
  }
  if (lane < 32)
#pragma unroll
    for (int j = 0; j < NR; ++j) pcol[j * CB + w * 32 + lane] = cres[j];
}

// R(s, j0 + j) = B - (sum of the partial products of stored row s), added in the fixed order of for_row_partials.
// Rf (may be null): R rounded to fp32, *flag raised where |R| > FLT_MAX
// -- or, RO = double, R itself.  colmax[j]: max |R(:,j)|, colmax[ncols + j]: max |X(:,j)| (X may be null).
template <int NR, typename RO>
__global__ __launch_bounds__(256) void k_sym_resid_reduce(TileGeo ga, TileGeo gx, const double *__restrict__ part,
                                                          int j0, const double *__restrict__ B,
                                                          const double *__restrict__ X, RO *__restrict__ Rf,
                                                          unsigned long long *colmax, int *flag) {
  const int NB = ga.lmt * bpt_of(ga);
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (s >= (long)NB * CB) return;
  const int P = (int)(s / CB), t = (int)(s % CB);
  if (t >= block_valid(ga, P)) return;
  double sum = 0.0;
  for_row_partials(P, NB, [&](long pair, int kind) { sum += part[(pair * 2 + kind) * NR * CB + j * CB + t]; });
  const long idx = desc_index(gx, P, t, j0 + j);
  const double rv = (B ? B[idx] : 0.0) - sum;
  if (Rf) {
    if (std::is_same<RO, float>::value && fabs(rv) > (double)FLT_MAX) atomicOr(flag, 1);
    Rf[idx] = (RO)rv;
  }
  atomic_max_abs(colmax + j0 + j, rv);
  if (X) atomic_max_abs(colmax + gx.n + j0 + j, X[idx]);
}

// The stored triangle of A -> the Lower fp32 tile image chol_potrf_tile factors: one 64 x 64 block of a lower tile
// (I >= J) per workgroup, staged through LDS so that Upper is read coalesced and transposed on the fly.  The
// unreferenced half of a diagonal tile is written as zeros, positions outside the matrix as the identity.
__global__ __launch_bounds__(256) void k_sym_to_f32(TileGeo ga, int upper, const double *__restrict__ A,
                                                    float *__restrict__ Af, int *flag) {
  const long tp = blockIdx.y;  // lower tile pair
  int I, J;
  pair_of(tp, I, J);
  const int bpt = ga.mbs / 64, rb = blockIdx.x % bpt, cb = blockIdx.x / bpt;
  const long ts = (long)ga.mbs * ga.mbs;
  __shared__ double sh[64][65];
  // source block: Lower (I, J) block (rb, cb); Upper (J, I) block (cb, rb), read in its own orientation
  const int si = upper ? J : I, sj = upper ? I : J, sr = upper ? cb : rb, sc = upper ? rb : cb;
  const double *src = A + ((long)si + (long)sj * ga.lmt) * ts + (long)sr * 64 + (long)sc * 64 * ga.mbs;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int rr = e % 64, cc = e / 64;
    sh[cc][rr] = src[rr + (long)cc * ga.mbs];
  }
  __syncthreads();
  float *dst = Af + ((long)I + (long)J * ga.lmt) * ts + (long)rb * 64 + (long)cb * 64 * ga.mbs;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int rr = e % 64, cc = e / 64;
    const int r = rb * 64 + rr, c = cb * 64 + cc;  // in-tile position of the destination entry
    const bool inside = r < ga.mbu && c < ga.mbu && (long)I * ga.mbu + r < ga.m && (long)J * ga.mbu + c < ga.m;
    float v;
    if (I == J && r < c) {
      v = 0.0f;
    } else if (!inside) {
      v = (I == J && r == c) ? 1.0f : 0.0f;
    } else {
      const double a = upper ? sh[rr][cc] : sh[cc][rr];
      if (fabs(a) > (double)FLT_MAX) atomicOr(flag, 1);
      v = (float)a;
    }
    dst[rr + (long)cc * ga.mbs] = v;
  }
}

// the n x ncols entries of an fp64 image -> fp32 (same positions), *flag raised where |x| > FLT_MAX
__global__ __launch_bounds__(256) void k_vec_to_f32(TileGeo gx, const double *__restrict__ B, float *__restrict__ Bf,
                                                    int *flag) {
  const long total = gx.m * gx.n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long gi = e % gx.m;
    const int j = (int)(e / gx.m);
    const long idx = image_index(gx, gi, j);
    const double b = B[idx];
    if (fabs(b) > (double)FLT_MAX) atomicOr(flag, 1);
    Bf[idx] = (float)b;
  }
}

// X := (double) C (assign) or X += (double) C over the n x ncols entries
__global__ __launch_bounds__(256) void k_vec_update(TileGeo gx, const float *__restrict__ C, double *__restrict__ X,
                                                    int assign) {
  const long total = gx.m * gx.n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long gi = e % gx.m;
    const int j = (int)(e / gx.m);
    const long idx = image_index(gx, gi, j);
    const double c = (double)C[idx];
    X[idx] = assign ? c : X[idx] + c;
  }
}

int grid_of(long total) { return (int)std::max(1L, std::min((total + 255) / 256, 8192L)); }

template <int NR, typename RO>
void resid_pass(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx, const double *X,
                const double *B, int j0, int nr, double *part, RO *Rf, unsigned long long *colmax, int *flag,
                bool abs_mode) {
  const long NB = block_rows(ga), pairs = tri_pairs(ga);
  if (abs_mode)
    hipLaunchKernelGGL((k_sym_resid<NR, true>), dim3((unsigned)pairs), dim3(256), 0, s, ga, upper, A, gx, X, j0, nr, part);
  else
    hipLaunchKernelGGL((k_sym_resid<NR, false>), dim3((unsigned)pairs), dim3(256), 0, s, ga, upper, A, gx, X, j0, nr, part);
  hipLaunchKernelGGL((k_sym_resid_reduce<NR, RO>), dim3((unsigned)((NB * CB + 255) / 256), (unsigned)nr), dim3(256), 0, s,
                     ga, gx, part, j0, B, X, Rf, colmax, flag);
}

}  // namespace

size_t sym_resid_part_bytes(const TileGeo &ga, int nrhs) {
  return (size_t)tri_pairs(ga) * 2 * CB * refine_width(nrhs) * sizeof(double);
}

template <typename RO>
void sym_resid_blocks(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx, const double *X,
                      const double *B, double *part, RO *Rf, unsigned long long *colmax, int *flag) {
  // column blocks of X of up to 8 right-hand sides, each one pass over the stored triangle
  for (int j0 = 0; j0 < gx.n; j0 += 8) {
    const int nr = (int)std::min<long>(8, gx.n - j0);
    with_width(nr, [&](auto w) {
      resid_pass<decltype(w)::value, RO>(s, ga, upper, A, gx, X, B, j0, nr, part, Rf, colmax, flag, false);
    });
  }
}

void launch_sym_resid(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx,
                      const double *X, const double *B, double *part, float *Rf, unsigned long long *colmax, int *flag) {
  sym_resid_blocks<float>(s, ga, upper, A, gx, X, B, part, Rf, colmax, flag);
}

void launch_sym_resid_f64(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx,
                          const double *X, const double *B, double *part, double *R, unsigned long long *colmax) {
  sym_resid_blocks<double>(s, ga, upper, A, gx, X, B, part, R, colmax, nullptr);
}

void launch_sym_inf_norm(hipStream_t s, const TileGeo &ga, int upper, const double *A, double *part,
                         unsigned long long *colmax) {
  TileGeo g1 = ga;
  g1.n = 1;
  resid_pass<1, float>(s, ga, upper, A, g1, nullptr, nullptr, 0, 1, part, nullptr, colmax, nullptr, true);
}

void launch_sym_to_f32(hipStream_t s, const TileGeo &ga, int upper, const double *A, float *Af, int *flag) {
  const long nt = ga.lmt, bpt = ga.mbs / 64;
  hipLaunchKernelGGL(k_sym_to_f32, dim3((unsigned)(bpt * bpt), (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, ga,
                     upper, A, Af, flag);
}

void launch_vec_to_f32(hipStream_t s, const TileGeo &gx, const double *B, float *Bf, int *flag) {
  hipLaunchKernelGGL(k_vec_to_f32, dim3(grid_of(gx.m * gx.n)), dim3(256), 0, s, gx, B, Bf, flag);
}

void launch_vec_update(hipStream_t s, const TileGeo &gx, const float *C, double *X, bool assign) {
  hipLaunchKernelGGL(k_vec_update, dim3(grid_of(gx.m * gx.n)), dim3(256), 0, s, gx, C, X, assign ? 1 : 0);
}

}  // namespace cholmi
