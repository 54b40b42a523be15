// The routines of libcholmi.so that work from a factor (include/cholmi.h), one section each below: the SPD solve, the
// mixed-precision solve, the inverse, the condition estimate, the expert solve with error bounds, the pivoted
// factorisation, the reduction of the generalized symmetric-definite eigenproblem, the L D L^T factorisation without
// pivoting with its solve, their butterfly-randomised forms, the rank-r update and downdate of a factor, the circular
// shift of a factor's variables, the halves of a factor alone, and the symmetric product from one stored triangle; the
// entry points come last.  All run on the main stream of the context that api.hip keeps (api_internal.h), inside a
// with_views body and so under the context lock; this file owns only its scratch and the statistics of the last call
// of each family.  What the routines repeat is said once: the element type by by_dtype (api_internal.h), a timed
// stretch by timed(), the look for a zero pivot and the Lower path with its launch check by lower_run(), an entry
// point's name and its first refusals by Entry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

#include "api_internal.h"

using namespace cholmi;

namespace {

// Scratch, grown on demand and kept until chol_finalize: one pool per family, because a family's buffers are live
// while it calls into another's (porfs / posvx hold cn[0] and rf while they call potrs_impl, which grows `work`).
// What each buffer holds is said where it is sized.
ScratchPool<1> work;      // potrs_impl
ScratchPool<4, true> mx;  // dsposv
ScratchPool<4> iv;        // trtri / potri; iv[3]: diag_zero's word, for every family that looks for a zero pivot first
ScratchPool<7> cn;        // lansy / pocon, and the staged factor diagonal that porfs / posvx share with them
ScratchPool<8, true> rf;  // poequ / porfs / posvx
ScratchPool<3> ps;        // pstrf
ScratchPool<3> sg;        // sygst
ScratchPool<2> cu;        // chud / chdd
ScratchPool<4> cx;        // chex
ScratchPool<4> sy;        // sytrf_nopiv / sytrs_nopiv
// sytrf_rbt / sysv_rbt.  Not cleared when it grows (a clear on the null stream would race with the main stream's upload
// of W): every buffer is written before it is read
ScratchPool<4> rb;
// trtrs / trmm / logdet: [0] the narrow paths' vectors and partials, [1] the wide product's clean diagonal tiles (in
// `work`, see ZSweeps), [2] the padded copy of a one-tile factor, [3] logdet's partials and result.  Cleared when it
// grows: the sweeps' unused vector slots then hold numbers
ScratchPool<4, true> tr;

// The statistics of a family's last call: written by the routine under the context lock, read by chol_last_*_stats
// (which is no with_views body and takes the lock itself)
struct LastStats {
  double v[8] = {};
  void clear() { std::fill(v, v + 8, 0.0); }
  // the accessor chol_last_<name>_stats: the first n values into out
  int read(const char *name, double *out, int n = 8) const {
    if (!ctx_inited()) return failf(CHOL_ERR_NOT_INITIALIZED, "last_%s_stats before chol_init", name);
    if (!out) return failf(-1, "last_%s_stats: NULL", name);
    std::lock_guard<std::recursive_mutex> lk(ctx_mutex());
    std::copy(v, v + n, out);
    return 0;
  }
};
LastStats mx_stats, cn_stats, rf_stats, ps_stats, sg_stats, cu_stats, cx_stats, sy_stats, rb_stats, tr_stats, sm_stats;

hipStream_t main_stream() { return main_rank_ctx()->st[ST_MAIN]; }

// An entry point's name, its refusals "<what>: <why>", and what the entry points begin with: the refusal before
// chol_init, then (given an uplo) the uplo rule at argument position pos.  Where another argument's rule stands
// between the two, the entry point calls begin() and uplo_at() apart; each check stays on its side of with_views
struct Entry {
  const char *what;
  int bad(int code, const char *why) const { return failf(code, "%s: %s", what, why); }
  int begin() const { return ctx_inited() ? 0 : failf(CHOL_ERR_NOT_INITIALIZED, "%s before chol_init", what); }
  int uplo_at(int uplo, int pos) const { return uplo == CHOL_LOWER || uplo == CHOL_UPPER ? 0 : bad(-pos, "uplo"); }
  int begin(int uplo, int pos = 1) const {
    const int rc = begin();
    return rc ? rc : uplo_at(uplo, pos);
  }
};

// one of the trailing updates (launch_trail_update, launch_syr2k_update, launch_ldl_update) on the tiles of d's columns
// [jlo, jhi), from the given panels
template <typename Launch, typename... Panels>
void update_cols(Launch launch, const chol_desc *d, int jlo, int jhi, const Panels &...pans) {
  const ColRange rr = col_range(d, jlo, jhi);
  launch(main_stream(), whole_local_mat(d), d->d_list, rr.off, rr.na, rr.offb, rr.nb, pans...);
}

// The time between two events on the main stream, added to a statistic; the events are made on first use
struct EventTimer {
  hipEvent_t e[2] = {nullptr, nullptr};
  ~EventTimer() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int start() {
    for (hipEvent_t &x : e)
      if (!x) HIPCHECK(hipEventCreate(&x));
    HIPCHECK(hipEventRecord(e[0], main_stream()));
    return 0;
  }
  int mark() {
    HIPCHECK(hipEventRecord(e[1], main_stream()));
    return 0;
  }
  int add(double *acc) {  // (after the end mark has run)
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, e[0], e[1]));
    *acc += ms;
    return 0;
  }
  int stop(double *acc) {  // (the phases end with a stream synchronisation of their own or are followed by one)
    if (int rc = mark()) return rc;
    HIPCHECK(hipEventSynchronize(e[1]));
    return add(acc);
  }
};

// body() between the two events of a timer of its own, the time added to *acc; a body that returns non-zero (an
// error, or an info it found before it wrote anything) returns before the timer is stopped
template <typename Body>
int timed(double *acc, const Body &body) {
  EventTimer tt;
  if (int rc = tt.start()) return rc;
  if (int rc = body()) return rc;
  return tt.stop(acc);
}

// ---------------------------------------------------------------- solve with the factor
// X <- A^{-1} B for A = L L^T already factored (CHAMELEON_dpotrs_Tile(ChamLower, A, B)).
// The kernels of this library are the right-sided NT forms the factorisation needs
// (X = A L^{-T}, C -= A B^T), so the solve runs on Z = B^T:
//   forward   Z(:,k) <- Z(:,k) L(k,k)^{-T};  Z(:,i) -= Z(:,k) L(i,k)^T, i > k      (L Y = B)
//   backward  Z(:,k) <- Z(:,k) L(k,k)^{-1};  Z(:,i) -= Z(:,k) L(k,i),   i < k      (L^T X = Y)
// the backward sweep's operands being transposed tiles (L(k,k)^{-T} from a TRSM of the identity,
// L(k,i)^T from a tile transpose) so that every product is again A B^T.
// udiag, rdiag (both or neither): the solve with an L D L^T factor (sytrs_nopiv) -- udiag holds the nt diagonal tiles
// with unit diagonals (read in place of A's), rdiag the reciprocals 1 / d (tile t at + t mb), by which the right-hand
// sides are scaled between the two sweeps
// The two sweeps apart (chol_trtrs_tile runs one of them), on the image Z that `load` makes and `store` writes back
template <typename T>
struct ZSweeps {
  chol_desc *A, *B;
  const T *udiag;
  int nt, nr, mb;
  long bs;
  size_t tb;
  T *La, *Bm, *Z, *Wt, *Tt, *tmp, *winv;  // Tt: nt tiles, tmp: nr tiles
  hipStream_t s;
  // extra: tiles of scratch beyond the sweeps' own, at `more` (chol_trmm_tile's clean diagonal tiles)
  T *more;
  int init(chol_desc *A_, chol_desc *B_, const T *udiag_, const char *what, size_t extra = 0) {
    A = A_, B = B_, udiag = udiag_;
    nt = A->nt, nr = B->nt, mb = A->mbi;
    bs = A->bsizi;
    tb = (size_t)bs * sizeof(T);
    La = reinterpret_cast<T *>(A->mat), Bm = reinterpret_cast<T *>(B->mat);
    if (int rc = work.ensure_bytes(0, ((size_t)nr * nt + 2 + (size_t)nr + (size_t)nt + extra) * tb, what)) return rc;
    T *scr = work.as<T>(0);
    Z = scr, Wt = scr + (size_t)nr * nt * bs, Tt = Wt + bs, tmp = Tt + (size_t)nt * bs, more = tmp + (size_t)nr * bs;
    s = main_stream();
    winv = reinterpret_cast<T *>(main_rank_ctx()->winv);
    return 0;
  }
  T *Ltile(int i, int j) const { return La + ((long)i + (long)j * A->lmt) * bs; }
  T *Ztile(int r, int i) const { return Z + ((long)r + (long)i * nr) * bs; }
  const T *Dtile(int k) const { return udiag ? udiag + (long)k * bs : Ltile(k, k); }
  void load() const {  // Z(r,i) = B(i,r)^T
    for (int r = 0; r < nr; ++r)
      launch_tiles_transpose<T>(s, Bm + (long)r * B->lmt * bs, bs, Ztile(r, 0), (long)nr * bs, mb, nt);
  }
  void store() const {  // B(i,r) = Z(r,i)^T
    for (int r = 0; r < nr; ++r)
      launch_tiles_transpose<T>(s, Ztile(r, 0), (long)nr * bs, Bm + (long)r * B->lmt * bs, bs, mb, nt);
  }
  void forward() const {
    for (int k = 0; k < nt; ++k) {
      launch_invert_diag<T>(s, Dtile(k), mb, winv);
      launch_trsm_panel<T>(s, Ztile(0, k), bs, nr, Dtile(k), winv, mb, T(1));
      // Z(r,i) -= Z(r,k) L(i,k)^T for every r and i > k: one launch
      launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Ltile(k + 1, k), bs, nt - 1 - k, Ztile(0, k + 1), bs, (long)nr * bs,
                              mb, T(-1), T(1));
    }
  }
  int backward() const {
    for (int k = nt - 1; k >= 0; --k) {
      HIPCHECK(hipMemsetAsync(Wt, 0, tb, s));
      launch_pad_identity<T>(s, Wt, 0, mb);
      launch_invert_diag<T>(s, Dtile(k), mb, winv);
      launch_trsm_panel<T>(s, Wt, bs, 1, Dtile(k), winv, mb, T(1));  // Wt = L(k,k)^{-T}
      // Z(r,k) <- Z(r,k) L(k,k)^{-1} for every r (out of place, then back: the tiles of a column are contiguous)
      launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Wt, 0, 1, tmp, bs, 0, mb, T(1), T(0));
      HIPCHECK(hipMemcpyAsync(Ztile(0, k), tmp, (size_t)nr * tb, hipMemcpyDeviceToDevice, s));
      // Z(r,i) -= Z(r,k) L(k,i) for every r and i < k: the k tiles L(k,i)^T in one transpose launch, one product launch
      if (k > 0) {
        launch_tiles_transpose<T>(s, Ltile(k, 0), (long)A->lmt * bs, Tt, bs, mb, k);
        launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Tt, bs, k, Ztile(0, 0), bs, (long)nr * bs, mb, T(-1), T(1));
      }
    }
    return 0;
  }
  // Z <- alpha Z L^T (B <- alpha L B), or with trans Z <- alpha Z L (B <- alpha L^T B); Dc: the diagonal tiles with
  // zeros above the diagonal (trans: transposed), nt tiles of bs.  Tile column k of Z is multiplied into the columns
  // that are already final before it is overwritten, so the order is from the last column down (trans: from the first
  // up); alpha multiplies the finished sums
  int product(bool trans, T alpha, const T *Dc) const {
    for (int step = 0; step < nt; ++step) {
      const int k = trans ? step : nt - 1 - step;
      if (!trans) {
        // Z(r,i) += Z(r,k) L(i,k)^T for every r and i > k
        launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Ltile(k + 1, k), bs, nt - 1 - k, Ztile(0, k + 1), bs,
                                (long)nr * bs, mb, T(1), T(1));
      } else if (k > 0) {
        // Z(r,i) += Z(r,k) L(k,i) for every r and i < k, on the transposed tiles as the backward sweep
        launch_tiles_transpose<T>(s, Ltile(k, 0), (long)A->lmt * bs, Tt, bs, mb, k);
        launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Tt, bs, k, Ztile(0, 0), bs, (long)nr * bs, mb, T(1), T(1));
      }
      // Z(r,k) <- Z(r,k) D_k^T (trans: D_k), out of place and back
      launch_gemm_nt_batch<T>(s, Ztile(0, k), bs, nr, Dc + (long)k * bs, 0, 1, tmp, bs, 0, mb, T(1), T(0));
      HIPCHECK(hipMemcpyAsync(Ztile(0, k), tmp, (size_t)nr * tb, hipMemcpyDeviceToDevice, s));
    }
    if (alpha != T(1)) launch_scale<T>(s, Z, (long)nr * nt * bs, alpha);
    return 0;
  }
  int finish() const {
    HIPCHECK(hipGetLastError());  // (a refused launch configuration must not come back as a wrong solution)
    HIPCHECK(hipStreamSynchronize(s));
    return 0;
  }
};

template <typename T>
int potrs_impl(chol_desc *A, chol_desc *B, const T *udiag = nullptr, const T *rdiag = nullptr) {
  ZSweeps<T> z;
  if (int rc = z.init(A, B, udiag, "potrs_tile")) return rc;
  z.load();
  z.forward();
  if (rdiag) launch_ldl_zscale<T>(z.s, z.Z, (long)z.nr * z.nt * z.bs, z.bs, z.mb, z.nr, rdiag);  // (D^{-1} between the sweeps)
  if (int rc = z.backward()) return rc;
  z.store();
  return z.finish();
}

// potrs_impl for either orientation of the factor.  No synchronisation after the second transpose: the caller's next
// work on the stream follows it.
template <typename T>
int potrs_uplo(int upper, chol_desc *A, chol_desc *B) {
  return through_lower(upper, {A}, [&] { return potrs_impl<T>(A, B); }, /*wait=*/false);
}

// ---------------------------------------------------------------- mixed-precision solve (LAPACK DSPOSV)
// Factor an fp32 copy of A, solve in fp32, refine X in fp64 with residuals R = B - A X read from the stored triangle
// (mixed.hip) until every column satisfies max|R(:,j)| <= max|X(:,j)| anrm eps sqrt(n); A and B are only read.
// *iter < 0 (no convergence, an entry that does not fit in fp32, fp32 factor not SPD): X <- B and dposv on A, X.
constexpr int DSPOSV_ITMAX = 30;

// What this refinement and sysv_rbt_impl's share.  A descriptor over scratch: d's geometry on `mat`, owning nothing and
// without a work list
chol_desc scratch_view(const chol_desc *d, void *mat) {
  chol_desc v = *d;
  v.mat = mat;
  v.user_mat = nullptr;
  v.owns = false;
  v.version = 0;
  v.d_list = nullptr;
  return v;
}

// the residual passes' `colmax` (mixed.hip): max |R(:,j)|, then max |X(:,j)|, each the bits of a non-negative double,
// then the overflow flag's word and a spare; launch_sym_inf_norm leaves anrm in the first word
size_t colmax_bytes(int nrhs) { return (size_t)(2 * nrhs + 2) * sizeof(unsigned long long); }

// LAPACK DSPOSV's stopping rule: max |R(:,j)| <= max |X(:,j)| cte for every column, cte = anrm eps sqrt(n)
struct RefineTol {
  double anrm, cte;
  RefineTol(unsigned long long anrm_bits, long n) {
    memcpy(&anrm, &anrm_bits, sizeof anrm);
    cte = anrm * std::ldexp(1.0, -53) * std::sqrt((double)n);
  }
  // hmax: colmax read back; berr (or null)[j] <- max |R(:,j)| / (anrm max |X(:,j)|)
  bool converged(const unsigned long long *hmax, int nrhs, double *berr = nullptr) const {
    bool done = true;
    for (int j = 0; j < nrhs; ++j) {
      double rn, xn;
      memcpy(&rn, &hmax[j], sizeof rn);
      memcpy(&xn, &hmax[nrhs + j], sizeof xn);
      if (berr) berr[j] = rn == 0 ? 0.0 : rn / (anrm * xn);
      if (!(rn <= xn * cte)) done = false;  // (a NaN residual does not converge)
    }
    return done;
  }
};

// -> *iter (>= 0: refinement steps; or -2 / -3 / -31 for the fallback), or a negative status
int dsposv_mixed(int uplo, chol_desc *A, chol_desc *B, chol_desc *X, int *iter) {
  hipStream_t s = main_stream();
  const int up = uplo == CHOL_UPPER ? 1 : 0, nrhs = B->ln;
  const TileGeo ga = geo_of(A), gx = geo_of(B);
  mx_stats.clear();
  double *st = mx_stats.v;  // total, conversions + norm, fp32 factor, fp32 solves, residual passes, #solves, #passes, -
  const size_t rf_bytes = (size_t)B->lmt * B->lnt * B->bsizi * sizeof(float);
  const char *what = "dsposv_tile";
  // the fp32 factor (A's tile image), the fp32 right-hand side / correction (B's), the residual's per-block partial
  // sums, colmax
  int rc = mx.ensure_bytes(0, (size_t)A->lmt * A->lnt * A->bsizi * sizeof(float), what);
  if (!rc) rc = mx.ensure_bytes(1, rf_bytes, what);
  if (!rc) rc = mx.ensure_bytes(2, sym_resid_part_bytes(ga, nrhs), what);
  if (!rc) rc = mx.ensure_bytes(3, colmax_bytes(nrhs), what);
  if (rc) return rc;
  float *Af = mx.as<float>(0), *Rf = mx.as<float>(1);
  double *part = mx.as<double>(2);
  unsigned long long *colmax = mx.as<unsigned long long>(3);
  int *flag = reinterpret_cast<int *>(colmax + 2 * nrhs);
  std::vector<unsigned long long> hmax(2 * nrhs + 1);
  // fp32 descriptors over the scratch: A's and B's geometry
  chol_desc Ad = scratch_view(A, Af), Rd = scratch_view(B, Rf);
  Ad.dtype = Rd.dtype = CHOL_REAL_FLOAT;
  Ad.esize = Rd.esize = sizeof(float);
  Ad.d_list = A->d_list;  // (potrf_run walks A's work list)
  EventTimer tt, tp;
  if ((rc = tt.start())) return rc;
  // anrm, then B and A to fp32 (-2 where an entry does not fit)
  if ((rc = tp.start())) return rc;
  HIPCHECK(hipMemsetAsync(colmax, 0, colmax_bytes(nrhs), s));
  HIPCHECK(hipMemsetAsync(Rf, 0, rf_bytes, s));  // (the solve runs on whole tiles: padding must be finite)
  launch_sym_inf_norm(s, ga, up, (const double *)A->mat, part, colmax);
  launch_vec_to_f32(s, gx, (const double *)B->mat, Rf, flag);
  launch_sym_to_f32(s, ga, up, (const double *)A->mat, Af, flag);
  HIPCHECK(hipGetLastError());
  unsigned long long anrm_bits = 0;
  int hflag = 0;
  HIPCHECK(hipMemcpyAsync(&anrm_bits, colmax, sizeof anrm_bits, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&hflag, flag, sizeof hflag, hipMemcpyDeviceToHost, s));
  if ((rc = tp.stop(&st[1]))) return rc;
  const RefineTol tol(anrm_bits, A->lm);
  auto finish = [&](int it) {
    *iter = it;
    return tt.stop(&st[0]);
  };
  if (hflag) return finish(-2);
  // the fp32 factor: info > 0 -> -3; an error (CHOL_ERR_DEVICE_WAIT, HIP) is returned as it is
  if ((rc = tp.start())) return rc;
  rc = potrf_run(CHOL_LOWER, &Ad);
  if (rc < 0) return rc;
  if (int r2 = tp.stop(&st[2])) return r2;
  if (rc > 0) return finish(-3);
  auto solve = [&]() -> int {  // Rf <- A^{-1} Rf in fp32
    int r = tp.start();
    if (!r) r = potrs_impl<float>(&Ad, &Rd);
    if (!r) r = tp.stop(&st[3]);
    st[5] += 1;
    return r;
  };
  if ((rc = solve())) return rc;
  launch_vec_update(s, gx, Rf, (double *)X->mat, /*assign=*/true);
  for (int it = 0;; ++it) {
    // R = B - A X in fp64, rounded into Rf; the column maxima of R and X
    if ((rc = tp.start())) return rc;
    HIPCHECK(hipMemsetAsync(colmax, 0, colmax_bytes(nrhs), s));
    launch_sym_resid(s, ga, up, (const double *)A->mat, gx, (const double *)X->mat, (const double *)B->mat, part, Rf,
                     colmax, flag);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hmax.data(), colmax, (2 * nrhs + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = tp.stop(&st[4]))) return rc;
    st[6] += 1;
    if (tol.converged(hmax.data(), nrhs)) return finish(it);
    if (it == DSPOSV_ITMAX) return finish(-DSPOSV_ITMAX - 1);
    if (hmax[2 * nrhs] & 0xffffffffull) return finish(-2);  // (the flag: the low word on a little-endian device)
    if ((rc = solve())) return rc;
    launch_vec_update(s, gx, Rf, (double *)X->mat, /*assign=*/false);
  }
}

// ---------------------------------------------------------------- inverse from the factor (LAPACK DTRTRI / DPOTRI)
// X = L^{-1} in place over the lower tiles (inverse.hip: the 128-blocks of every diagonal tile, then the tiles, each
// level column by column from the right), then for potri X^T X into the lower triangle (verify_ops.hip's LAUUM).
// ChamUpper flips the storage around the Lower path, as potrf and potrs do.  A stored image whose padding is the
// identity (a ragged order, a tile edge that is not a multiple of 128) is inverted as a whole: its padding stays the
// identity and its matrix part is the inverse of the caller's matrix.
template <typename T>
struct InvImg {  // nt x nt tiles of mbs x mbs (mbs % 128 == 0), tile (i,j) at p + (i + j lmt) mbs^2
  T *p;
  int nt, lmt, mbs;
};

template <typename T>
int trtri_img(const InvImg<T> &A) {
  hipStream_t s = main_stream();
  const int nt = A.nt, mb = A.mbs, nbm = mb / MACRO;
  const long bs = (long)mb * mb, tstride = (long)(A.lmt + 1) * bs, blk = (long)MACRO * MACRO;
  // Y: nt tiles (tile level) or nt * nbm blocks (inner level); the 128 x 128 inverses of every diagonal tile
  if (int rc = iv.ensure_bytes(0, (size_t)nt * bs * sizeof(T), "trtri_tile")) return rc;
  if (int rc = iv.ensure_bytes(1, (size_t)nt * nbm * blk * sizeof(T), "trtri_tile")) return rc;
  T *Y = iv.as<T>(0), *W = iv.as<T>(1);
  launch_invert_diag_batch<T>(s, A.p, tstride, nt, mb, W);
  // the diagonal tiles, all at once: blocks (i,j) of tile z at p + z tstride + i 128 + j 128 mb
  const TriLevel<T> in{A.p, MACRO, (long)MACRO * mb, tstride, mb, W, blk, nbm * blk, MACRO, Y, blk, nbm * blk, MACRO};
  for (int c = nbm - 2; c >= 0; --c) launch_tri_column<T>(s, in, nbm, nt, c);
  launch_tri_put_diag<T>(s, A.p, tstride, mb, nt, W);
  // the tiles below the diagonal
  const TriLevel<T> top{A.p, bs, (long)A.lmt * bs, 0, mb, A.p, tstride, 0, mb, Y, bs, 0, mb};
  for (int c = nt - 2; c >= 0; --c) launch_tri_column<T>(s, top, nt, 1, c);
  HIPCHECK(hipGetLastError());
  return 0;
}

// lower triangle of A <- X^T X, X the lower triangle of A (padding included: the identity stays)
template <typename T>
int lauum_img(const InvImg<T> &A) {
  hipStream_t s = main_stream();
  if (int rc = iv.ensure_bytes(0, (size_t)A.nt * A.nt * A.mbs * A.mbs * sizeof(T), "potri_tile")) return rc;
  T *out = iv.as<T>(0);
  launch_lauum_lower<T>(s, A.p, out, A.nt, A.mbs);
  TileGeo ge;
  ge.lmt = ge.lnt = A.nt;
  ge.mbs = ge.mbu = A.mbs;
  ge.m = ge.n = (long)A.nt * A.mbs;
  launch_lacpy<T>(s, ge, 1, out, A.p);
  HIPCHECK(hipGetLastError());
  return 0;
}

// A (Lower orientation, already checked) <- L^{-1}, or inv(L L^T) for potri
template <typename T>
int inverse_impl(chol_desc *A, bool potri) {
  hipStream_t s = main_stream();
  forget_winv(A->mat);  // (A is overwritten)
  // potri: its LAUUM image first (trtri's Y blocks fit in it): no scratch is reallocated between the launches
  const int ep = roundup(A->mbi, MACRO), nt = A->mbi % MACRO ? 1 : A->nt;
  if (potri) {
    if (int rc = iv.ensure_bytes(0, (size_t)nt * nt * ep * ep * sizeof(T), "potri_tile")) return rc;
  }
  if (A->mbi % MACRO == 0) {
    const InvImg<T> im{reinterpret_cast<T *>(A->mat), A->nt, A->lmt, A->mbi};
    int rc = trtri_img<T>(im);
    if (!rc && potri) rc = lauum_img<T>(im);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize(s));
    return 0;
  }
  // a single tile whose edge is an odd multiple of 64: staged into a multiple of 128 with the identity beyond it
  const int e = A->mbi;
  if (int rc = iv.ensure_bytes(2, (size_t)ep * ep * sizeof(T), "trtri_tile")) return rc;
  T *S = iv.as<T>(2);
  HIPCHECK(hipMemsetAsync(S, 0, (size_t)ep * ep * sizeof(T), s));
  HIPCHECK(hipMemcpy2DAsync(S, (size_t)ep * sizeof(T), A->mat, (size_t)e * sizeof(T), (size_t)e * sizeof(T), e,
                            hipMemcpyDeviceToDevice, s));
  launch_pad_identity<T>(s, S, e, ep);
  const InvImg<T> im{S, 1, 1, ep};
  int rc = trtri_img<T>(im);
  if (!rc && potri) rc = lauum_img<T>(im);
  if (rc) return rc;
  // (the strict upper triangle goes back as it came: no kernel writes it)
  HIPCHECK(hipMemcpy2DAsync(A->mat, (size_t)e * sizeof(T), S, (size_t)ep * sizeof(T), (size_t)e * sizeof(T), e,
                            hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

// the descriptor rules of chol_trtri_tile / chol_potri_tile / chol_poinv_tile (apos: A's argument position)
int inverse_check(const char *what, chol_desc *A, int apos) {
  int rc = resident_whole(what, A);
  if (rc) return rc;
  if (A->mt != A->nt || A->lm != A->ln) return failf(-apos, "%s: A is not square", what);
  if (A->mbi % 64) return failf(CHOL_ERR_NOT_SUPPORTED, "%s: stored tile edge must be a multiple of 64", what);
  return 0;
}

// the first exact zero on the diagonal (1-based), or 0; read before anything is written (what: the calling routine)
int diag_zero(const chol_desc *A, int *info, const char *what) {
  hipStream_t s = main_stream();
  if (int rc = iv.ensure_bytes(3, sizeof(int), what)) return rc;
  int *first = iv.as<int>(3);
  by_dtype(A->dtype, [&](auto t) {
    using T = decltype(t);
    launch_diag_zero<T>(s, reinterpret_cast<const T *>(A->mat), (long)(A->lmt + 1) * A->bsizi, A->mbi, A->mb, A->lm, first);
  });
  HIPCHECK(hipGetLastError());
  int v = 0;
  HIPCHECK(hipMemcpyAsync(&v, first, sizeof v, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *info = v <= A->lm ? v : 0;
  return 0;
}

// The look for a zero pivot and the Lower path that sygst, chud, chex and sytrf share: an exact zero on `scan`'s
// diagonal returns its 1-based index before anything is written (scan null: no look); then body() on the Lower
// orientation of `ds` (through_lower), the launch check and the wait for the main stream -> the body's status
int lower_run(const char *what, const chol_desc *scan, int uplo, std::initializer_list<chol_desc *> ds,
              const std::function<int()> &body) {
  int info = 0;
  if (scan)
    if (int rc = diag_zero(scan, &info, what)) return rc;
  if (info) return info;
  const int rc = through_lower(uplo == CHOL_UPPER, ds, body);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(main_stream()));
  return rc;
}

// (not lower_run: inverse_impl ends with its own wait, and no launch check follows the second transpose)
int inverse_run(int uplo, chol_desc *A, bool potri) {
  int info = 0;
  if (int rc = diag_zero(A, &info, potri ? "potri_tile" : "trtri_tile")) return rc;
  if (info) return info;  // (LAPACK: A is unchanged)
  // ChamUpper: U = L^T; inv(U) = inv(L)^T and inv(U^T U) = inv(L L^T) -- the Lower path on the transposed storage
  return through_lower(uplo == CHOL_UPPER, {A},
                       [&] { return by_dtype(A->dtype, [&](auto t) { return inverse_impl<decltype(t)>(A, potri); }); });
}

// ---------------------------------------------------------------- condition estimate (LAPACK DLANSY / DPOCON)
// lansy: one pass over the stored triangle (condest.hip).  pocon: LAPACK DLACN2's state machine on the host, which
// reads back six scalars after each application of A^{-1}; the applications (two narrow triangular sweeps over the
// stored triangle) and every operation on an N-vector run on the device (condest.hip).

// v <- the max, the one (= inf) norm and the sum of squares of the stored triangle
template <typename T>
int lansy_impl(const chol_desc *A, int upper, const char *what, double v[3]) {
  hipStream_t s = main_stream();
  const TileGeo ge = geo_of(A);
  const size_t pb = lansy_part_bytes(ge);
  if (int rc = cn.ensure_bytes(6, pb + 4 * sizeof(double), what)) return rc;
  double *part = cn.as<double>(6), *res = part + pb / sizeof(double);
  launch_lansy<T>(s, ge, upper, reinterpret_cast<const T *>(A->mat), part, res);
  HIPCHECK(hipGetLastError());
  v[0] = v[1] = v[2] = 0;  // (the max and the row-sum max are the bits of non-negative doubles: read as doubles)
  HIPCHECK(hipMemcpyAsync(v, res, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

// LAPACK DLACN2's control flow for one vector (Higham's estimator, as LAPACK has it): what the device does before the
// next application of the operator (fill x: -1 nothing, 0 1/n, 1 e_j, 2 the alternating-sign vector; kase 1 / 2), the
// statistics after it (condest.hip: launch_vec_stats with `sign`, `jlast`), and the estimate.  pocon applies A^{-1}
// for both kases; porfs applies diag(W) A^{-1} (kase 1) and A^{-1} diag(W) (kase 2).
struct Lacn2 {
  static constexpr int ITMAX = 5;
  long n = 0;
  int isave = 0, iter = 0;
  long j = 0;
  double est = 0;
  bool done = false, finite = true;
  int fill = 0, kase = 1, sign = 1;
  long fill_j = 0, jlast = -1;
  void next(int isave_, int fill_, long fill_j_, int kase_, int sign_, long jlast_) {
    isave = isave_, fill = fill_, fill_j = fill_j_, kase = kase_, sign = sign_, jlast = jlast_;
  }
  void start(long n_) {
    n = n_, iter = 0, j = 0, est = 0, done = false, finite = true;
    next(1, 0, 0, 1, 1, -1);  // x = 1/n; after it est = ||x||_1, x = isgn = sign(x)
  }
  // st: launch_vec_stats' out[0..5] after the application (sum |x|, max |x|, its index, non-finite, x[jlast], changed)
  template <typename T>
  void take(const double *st) {
    if (st[3] != 0) {  // (no dlatrs scaling: a non-finite entry ends the estimate)
      finite = false;
      done = true;
      return;
    }
    switch (isave) {
      case 1:
        est = st[0];
        if (n <= 1) {
          done = true;
          return;
        }
        return next(2, -1, 0, 2, 0, -1);  // then j = idamax(x)
      case 2:
        j = (long)st[2];
        iter = 2;
        return next(3, 1, j, 1, 1, -1);  // x = e_j; then est = ||x||_1, x = isgn = sign(x), changed?
      case 3: {
        const double estold = est;
        est = st[0];
        if (st[5] == 0 || est <= estold) break;  // a repeated sign vector, or no increase: converged
        return next(4, -1, 0, 2, 0, j);          // then j = idamax(x), x(jlast) against |x(j)|
      }
      case 4:
        if (st[4] != st[1] && iter < ITMAX) {
          ++iter;
          j = (long)st[2];
          return next(3, 1, j, 1, 1, -1);
        }
        break;
      default: {  // 5: the alternating-sign test vector
        const T temp = T(2) * (T(st[0]) / T(3 * n));
        if ((double)temp > est) est = (double)temp;
        done = true;
        return;
      }
    }
    next(5, 2, 0, 1, 0, -1);
  }
};

// the diagonal tiles of the factor, inverted once per call: their 128-blocks (as potrs) into W, then the tiles
// (trtri's inner level) into Dv (nt tiles of E x E, E = condest_edge); Y: the products' scratch.  W and Y hold
// nt (E / 128) blocks of 128 x 128 each; W keeps the 128-block inverses (potrs's winv, tile t at W + t (E / 128) 128^2).
template <typename T>
void stage_factor_diag_into(chol_desc *A, int upper, T *Dv, T *W, T *Y) {
  hipStream_t s = main_stream();
  const TileGeo ge = geo_of(A);
  const int E = condest_edge(ge), nbm = E / MACRO, nt = A->nt;
  const long blk = (long)MACRO * MACRO;
  launch_stage_diag<T>(s, ge, upper, reinterpret_cast<const T *>(A->mat), Dv);
  launch_invert_diag_batch<T>(s, Dv, (long)E * E, nt, E, W);
  const TriLevel<T> in{Dv, MACRO, (long)MACRO * E, (long)E * E, E, W, blk, nbm * blk, MACRO, Y, blk, nbm * blk, MACRO};
  for (int c = nbm - 2; c >= 0; --c) launch_tri_column<T>(s, in, nbm, nt, c);
  launch_tri_put_diag<T>(s, Dv, (long)E * E, E, nt, W);
}

// ... into cn[0] (cn[1], cn[2]: W, Y)
template <typename T>
int stage_factor_diag(chol_desc *A, int upper, const char *what) {
  const TileGeo ge = geo_of(A);
  const int E = condest_edge(ge), nbm = E / MACRO, nt = A->nt;
  const long blk = (long)MACRO * MACRO;
  int rc = cn.ensure_bytes(0, (size_t)nt * E * E * sizeof(T), what);
  if (!rc) rc = cn.ensure_bytes(1, (size_t)nt * nbm * blk * sizeof(T), what);
  if (!rc) rc = cn.ensure_bytes(2, (size_t)nt * nbm * blk * sizeof(T), what);
  if (rc) return rc;
  stage_factor_diag_into<T>(A, upper, cn.as<T>(0), cn.as<T>(1), cn.as<T>(2));
  HIPCHECK(hipGetLastError());
  return 0;
}

// staged: cn[0] already holds the inverted diagonal tiles of this factor (posvx)
template <typename T>
int pocon_impl(chol_desc *A, int upper, double anorm, double *rcond, bool staged = false) {
  hipStream_t s = main_stream();
  const TileGeo ge = geo_of(A);
  const long n = A->lm;
  cn_stats.clear();
  *rcond = 0;
  if (n == 0) {
    *rcond = 1;
    return 0;
  }
  if (anorm == 0 || std::isinf(anorm)) return 0;
  EventTimer tt, tsweep;  // the whole call; each application (read after the synchronisation that follows it)
  int rc = tt.start();
  if (rc) return rc;
  int info = 0;
  rc = diag_zero(A, &info, "pocon_tile");
  if (rc) return rc;
  if (info) return 0;  // a zero on the factor's diagonal: rcond = 0, no sweep
  // scratch: the diagonal tiles, their 128-block inverses, the products' Y blocks (stage_factor_diag), the vectors,
  // the sign vector, the statistics
  const int E = condest_edge(ge), nt = A->nt, bpt = E / MACRO;
  const long NB = (long)nt * bpt;
  const size_t nv = condest_vec_elems(ge), npg = 2 * (size_t)NB * bpt * MACRO, npd = (size_t)bpt * bpt * MACRO;
  if (!staged && (rc = stage_factor_diag<T>(A, upper, "pocon_tile"))) return rc;
  rc = cn.ensure_bytes(3, (2 * nv + npg + npd) * sizeof(T), "pocon_tile");
  if (!rc) rc = cn.ensure_bytes(4, nv * sizeof(int), "pocon_tile");
  if (!rc) rc = cn.ensure_bytes(5, vec_stats_part_bytes() + 8 * sizeof(double), "pocon_tile");
  if (rc) return rc;
  const T *Dv = cn.as<const T>(0);
  T *vx = cn.as<T>(3);
  const SweepBufs<T> bufs{vx, vx + nv, vx + 2 * nv, vx + 2 * nv + npg};
  int *isgn = cn.as<int>(4);
  double *spart = cn.as<double>(5), *sout = spart + vec_stats_part_bytes() / sizeof(double);
  const T *Am = reinterpret_cast<const T *>(A->mat);
  int apps = 0;
  double sweep_ms = 0, st[6] = {0, 0, 0, 0, 0, 0};
  // x <- A^{-1} x, then the statistics of x (DLACN2's kase != 0 round trip)
  auto apply = [&](int sign, long jlast) -> int {
    if (int r = tsweep.start()) return r;
    launch_sweep<T>(s, ge, upper, Am, Dv, bufs);
    if (int r = tsweep.mark()) return r;
    launch_vec_stats<T>(s, ge, bufs.x, isgn, sign, jlast, spart, sout);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(st, sout, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (int r = tsweep.add(&sweep_ms)) return r;
    ++apps;
    return 0;
  };
  // DLACN2; A is symmetric, so kase 1 and kase 2 apply the same A^{-1}
  Lacn2 est;
  est.start(n);
  while (!est.done) {
    if (est.fill >= 0) launch_vec_fill<T>(s, ge, bufs.x, est.fill, est.fill_j);
    if ((rc = apply(est.sign, est.jlast))) return rc;
    est.take<T>(st);
  }
  // (no dlatrs scaling: a sweep that overflows gives rcond = 0)
  if (est.finite && est.est != 0) *rcond = (1.0 / est.est) / anorm;
  if ((rc = tt.stop(&cn_stats.v[0]))) return rc;
  cn_stats.v[1] = sweep_ms;
  cn_stats.v[2] = apps;
  return 0;
}

// ---------------------------------------------------------------- the SPD expert solve (LAPACK DPOEQU, DLAQSY, DPORFS, DPOSVX)
// poequ / laqsy: one pass over the diagonal / the stored triangle (refine.hip).  porfs: every column in lockstep, each
// with its own refinement count, lstres and DLACN2 state; each step applies A^{-1} only to the columns still active,
// either with the multi-vector sweeps (at most K_X columns: ceil(k / 8) sweeps of up to 8 vectors) or with potrs_impl
// on a scratch n x k image (wider steps).  posvx composes them in DPOSVX's order.

// the widest application of A^{-1} that runs as multi-vector sweeps; wider ones go through potrs_impl.  Measured
// crossover: about 47 columns at N = 65536 / 1024, about 30 at 16384 / 512
constexpr int POSVX_KX = 40;
constexpr int PORFS_ITMAX = 5;

template <typename T>
struct Lam;  // LAPACK xLAMCH: 'E'psilon (rounding), 'S'afe minimum, 'P'recision = eps * base
template <>
struct Lam<double> {
  static constexpr double eps = 0x1p-53, safmin = 0x1p-1022, prec = 0x1p-52;
};
template <>
struct Lam<float> {
  static constexpr double eps = 0x1p-24, safmin = 0x1p-126, prec = 0x1p-23;
};

// porfs / posvx's scratch (rf): the residual / estimator vectors, the FERR weights, the sign vectors (one
// condest-layout vector per column each), the residual partials, the sweeps' scratch and padding vectors, the
// backward errors and statistics, and the n x k image of the potrs path
template <typename T>
struct RfBufs {
  T *R, *F, *part, *sw, *pad;
  int *isgn;
  unsigned long long *berr;
  double *spart, *sout;
  long nv;
};

template <typename T>
int rf_buffers(const TileGeo &ga, int nrhs, RfBufs<T> *b, const char *what) {
  const long nv = (long)condest_vec_elems(ga);
  const size_t vb = (size_t)nrhs * nv * sizeof(T);
  const size_t sb = vec_stats_part_bytes() + (size_t)(nrhs + 1) * 8 * sizeof(double);
  int rc = rf.ensure_bytes(0, vb, what);
  if (!rc) rc = rf.ensure_bytes(1, vb, what);
  if (!rc) rc = rf.ensure_bytes(2, (size_t)nrhs * nv * sizeof(int), what);
  if (!rc) rc = rf.ensure_bytes(3, porfs_part_elems(ga, refine_width(std::min(nrhs, 8))) * sizeof(T), what);
  if (!rc) rc = rf.ensure_bytes(4, (msweep_scratch_elems(ga) + 8 * (size_t)nv) * sizeof(T), what);
  if (!rc) rc = rf.ensure_bytes(5, (size_t)nrhs * sizeof(unsigned long long) + sb, what);
  if (rc) return rc;
  b->nv = nv;
  b->R = rf.as<T>(0);
  b->F = rf.as<T>(1);
  b->isgn = rf.as<int>(2);
  b->part = rf.as<T>(3);
  b->sw = rf.as<T>(4);
  b->pad = b->sw + msweep_scratch_elems(ga);
  b->berr = rf.as<unsigned long long>(5);
  b->spart = reinterpret_cast<double *>(b->berr + nrhs);
  b->sout = b->spart + vec_stats_part_bytes() / sizeof(double);
  return 0;
}

// `cols` in groups of up to 8 (VecCols): vector slot v[j] = column d[j] of the matrix; packed: d[j] is the position
// in `cols` instead (a compact n x k image)
std::vector<VecCols> groups_of(const std::vector<int> &cols, bool packed = false) {
  std::vector<VecCols> out;
  for (size_t c0 = 0; c0 < cols.size(); c0 += 8) {
    VecCols vc{(int)std::min<size_t>(8, cols.size() - c0), {}, {}};
    for (int j = 0; j < vc.n; ++j) vc.v[j] = cols[c0 + j], vc.d[j] = packed ? (int)c0 + j : cols[c0 + j];
    out.push_back(vc);
  }
  return out;
}

// the columns 0 .. k-1
std::vector<int> all_cols(int k) {
  std::vector<int> v(k);
  std::iota(v.begin(), v.end(), 0);
  return v;
}

// V[c] <- A^{-1} V[c] for the slots c in `cols` (AF: the factor, its diagonal tiles staged in cn[0]); st: posvx stats;
// path: 0 the path rule, 1 the sweeps, 2 potrs (chol_bench_refine)
template <typename T>
int apply_inv(int upper, chol_desc *AF, const RfBufs<T> &b, T *V, const std::vector<int> &cols, double *st,
              int path = 0) {
  hipStream_t s = main_stream();
  const TileGeo ga = geo_of(AF);
  const int k = (int)cols.size();
  if (!k) return 0;
  if (path == 1 || (path == 0 && k <= POSVX_KX)) {
    const long NB = (long)ga.lmt * (condest_edge(ga) / MACRO);
    const long nv = b.nv, pgn = 2 * NB * (condest_edge(ga) / MACRO) * MACRO;
    const MSweepBufs<T> mb{b.sw, b.sw + 8 * nv, b.sw + 8 * nv + 8 * pgn};
    for (int c0 = 0; c0 < k; c0 += 8) {
      const int m = std::min(8, k - c0);
      T *x[8];
      for (int j = 0; j < m; ++j) x[j] = V + (long)cols[c0 + j] * nv;
      launch_msweep<T>(s, ga, upper, reinterpret_cast<const T *>(AF->mat), cn.as<const T>(0), x, m,
                       b.pad, mb);
      st[6] += m;
    }
    HIPCHECK(hipGetLastError());
    return 0;
  }
  // wide: potrs_impl on an n x k scratch image with AF's row tiling (the solve runs on whole tiles: zero padding)
  chol_desc Td = scratch_view(AF, nullptr);
  Td.ln = Td.n = k;
  Td.nt = Td.lnt = (k + AF->mb - 1) / AF->mb;
  const size_t tb = (size_t)Td.lmt * Td.lnt * Td.bsizi * sizeof(T);
  if (int rc = rf.ensure_bytes(6, tb, "porfs_tile")) return rc;
  Td.mat = rf.p[6];
  HIPCHECK(hipMemsetAsync(Td.mat, 0, tb, s));
  const TileGeo gt = geo_of(&Td);
  const std::vector<VecCols> gr = groups_of(cols, /*packed=*/true);
  for (const VecCols &vc : gr) launch_scatter<T>(s, gt, reinterpret_cast<T *>(Td.mat), vc, V, false);
  if (int rc = potrs_uplo<T>(upper, AF, &Td)) return rc;
  for (const VecCols &vc : gr) launch_gather<T>(s, gt, reinterpret_cast<const T *>(Td.mat), vc, V);
  HIPCHECK(hipGetLastError());
  st[7] += k;
  return 0;
}

// LAPACK DPORFS on device images; AF's diagonal tiles staged in cn[0]; st: posvx stats ([5] total porfs ms,
// [6] / [7] columns through the sweeps / through potrs)
template <typename T>
int porfs_impl(int upper, chol_desc *A, chol_desc *AF, chol_desc *B, chol_desc *X, double *ferr, double *berr,
               double *st) {
  hipStream_t s = main_stream();
  const TileGeo ga = geo_of(A), gx = geo_of(B);
  const long n = A->lm;
  const int nrhs = B->ln;
  if (n == 0 || nrhs == 0) {
    std::fill(ferr, ferr + nrhs, 0.0);
    std::fill(berr, berr + nrhs, 0.0);
    return 0;
  }
  EventTimer tt;
  int rc = tt.start();
  if (rc) return rc;
  RfBufs<T> b;
  if ((rc = rf_buffers<T>(ga, nrhs, &b, "porfs_tile"))) return rc;
  const double eps = Lam<T>::eps, safe1 = (double)(T(n + 1) * T(Lam<T>::safmin)), safe2 = (double)(T(safe1) / T(eps));
  const T *Am = reinterpret_cast<const T *>(A->mat);
  std::vector<int> count(nrhs, 1), active = all_cols(nrhs);
  std::vector<double> lstres(nrhs, 3.0);
  std::vector<unsigned long long> hb(nrhs);
  // refinement: R = B - A X, BERR; X += A^{-1} R for the columns that go on
  while (!active.empty()) {
    HIPCHECK(hipMemsetAsync(b.berr, 0, (size_t)nrhs * sizeof(unsigned long long), s));
    for (const VecCols &vc : groups_of(active))
      launch_porfs_resid<T>(s, ga, upper, Am, gx, reinterpret_cast<const T *>(X->mat), reinterpret_cast<const T *>(B->mat),
                            vc, b.part, b.R, b.F, eps, safe1, safe2, b.berr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hb.data(), b.berr, (size_t)nrhs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::vector<int> next;
    for (int j : active) {
      double bj;
      memcpy(&bj, &hb[j], sizeof bj);
      berr[j] = bj;
      if (bj > eps && 2 * bj <= lstres[j] && count[j] <= PORFS_ITMAX) {
        next.push_back(j);
        lstres[j] = bj;
        ++count[j];
      }
    }
    if ((rc = apply_inv<T>(upper, AF, b, b.R, next, st))) return rc;
    for (const VecCols &vc : groups_of(next)) launch_scatter<T>(s, gx, reinterpret_cast<T *>(X->mat), vc, b.R, true);
    active.swap(next);
  }
  // FERR: DLACN2 on diag(F) A^{-1} (kase 1) / A^{-1} diag(F) (kase 2), every column in lockstep, x in the R slots
  std::vector<Lacn2> est(nrhs);
  for (int j = 0; j < nrhs; ++j) est[j].start(n), active.push_back(j);
  std::vector<double> hs((size_t)nrhs * 8);
  while (!active.empty()) {
    const std::vector<VecCols> gr = groups_of(active);
    for (int j : active)
      if (est[j].fill >= 0) launch_vec_fill<T>(s, ga, b.R + (long)j * b.nv, est[j].fill, est[j].fill_j);
    auto weight = [&](int kase) {
      for (const VecCols &vc : gr) {
        unsigned mask = 0;
        for (int i = 0; i < vc.n; ++i) mask |= (est[vc.v[i]].kase == kase ? 1u : 0u) << i;
        launch_vec_weight<T>(s, ga, b.R, b.F, vc, mask);
      }
    };
    weight(2);
    if ((rc = apply_inv<T>(upper, AF, b, b.R, active, st))) return rc;
    weight(1);
    for (size_t i = 0; i < active.size(); ++i) {
      const int j = active[i];
      launch_vec_stats<T>(s, ga, b.R + (long)j * b.nv, b.isgn + (long)j * b.nv, est[j].sign, est[j].jlast, b.spart,
                          b.sout + 8 * i);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hs.data(), b.sout, active.size() * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    std::vector<int> next;
    for (size_t i = 0; i < active.size(); ++i) {
      const int j = active[i];
      est[j].take<T>(&hs[8 * i]);
      if (!est[j].done) next.push_back(j);
    }
    active.swap(next);
  }
  // normalise by max |X(:,j)| (gathered into a padding vector, then launch_vec_stats)
  for (int j = 0; j < nrhs; ++j) {
    const VecCols vc{1, {0}, {j}};
    launch_gather<T>(s, gx, reinterpret_cast<const T *>(X->mat), vc, b.pad);
    launch_vec_stats<T>(s, ga, b.pad, b.isgn, 0, -1, b.spart, b.sout + 8 * j);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(hs.data(), b.sout, (size_t)nrhs * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  for (int j = 0; j < nrhs; ++j) {
    T f = est[j].finite ? T(est[j].est) : T(INFINITY);
    const T xm = T(hs[8 * j + 1]);
    if (xm != T(0)) f = f / xm;
    ferr[j] = (double)f;
  }
  return tt.stop(&st[5]);
}

// the descriptor rules shared by porfs / posvx: an n x nrhs image d with A's dtype, order and tile size
int rhs_check(const char *what, const chol_desc *A, const chol_desc *d, int pos, const char *name) {
  if (!d) return failf(-pos, "%s: %s is NULL", what, name);
  if (int rc = resident_whole(what, d)) return rc;
  if (!same_rows(A, d)) return failf(-pos, "%s: %s must have A's dtype, order and tile size", what, name);
  return 0;
}

int square_check(const char *what, chol_desc *A, int pos) {
  if (!A) return failf(-pos, "%s: NULL descriptor", what);
  return inverse_check(what, A, pos);
}

// launch_diag_scan (mode 0: S <- 1/sqrt(diag(A)); 1: S alone) reduced on the host: the smallest and the largest
// value scanned, and the first 0-based index of one <= 0 (or -1)
template <typename T>
int diag_scan(const chol_desc *A, chol_desc *S, int mode, const char *what, T *smin, T *smax, long *bad) {
  hipStream_t s = main_stream();
  const long n = A->lm;
  if (int rc = rf.ensure_bytes(7, diag_scan_part_bytes(), what)) return rc;
  double *part = rf.as<double>(7);
  launch_diag_scan<T>(s, geo_of(A), mode == 0 ? reinterpret_cast<const T *>(A->mat) : nullptr,
                      reinterpret_cast<T *>(S->mat), mode, part);
  HIPCHECK(hipGetLastError());
  std::vector<double> h(diag_scan_part_bytes() / sizeof(double));
  HIPCHECK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  const long per = (n + 255) / 256;
  *smin = T(INFINITY), *smax = T(-INFINITY), *bad = -1;
  for (long w = 0; w < 256 && w * per < n; ++w) {
    *smin = std::min(*smin, T(h[3 * w]));
    *smax = std::max(*smax, T(h[3 * w + 1]));
    if (h[3 * w + 2] >= 0 && *bad < 0) *bad = (long)h[3 * w + 2];
  }
  return 0;
}

// LAPACK DPOEQU on the device: S <- 1/sqrt(diag), *scond, *amax; info > 0: the first non-positive diagonal entry
template <typename T>
int poequ_impl(chol_desc *A, chol_desc *S, double *scond, double *amax, int *info) {
  *info = 0;
  if (A->lm == 0) {
    *scond = 1, *amax = 0;
    return 0;
  }
  T smin, smax;
  long bad;
  if (int rc = diag_scan<T>(A, S, 0, "poequ_tile", &smin, &smax, &bad)) return rc;
  *amax = (double)smax;
  if (smin <= T(0)) {
    *info = (int)(bad + 1);
    return 0;
  }
  *scond = (double)(T(std::sqrt(smin)) / T(std::sqrt(smax)));
  return 0;
}

// LAPACK DLAQSY's decision and scaling; *equed <- 1 ('Y') or 0 ('N')
template <typename T>
int laqsy_impl(int upper, chol_desc *A, chol_desc *S, double scond, double amax, int *equed) {
  const double small = Lam<T>::safmin / Lam<T>::prec, large = 1.0 / small;
  *equed = 0;
  if (A->lm == 0) return 0;
  if (scond >= 0.1 && amax >= small && amax <= large) return 0;
  launch_laqsy<T>(main_stream(), geo_of(A), upper, reinterpret_cast<T *>(A->mat), reinterpret_cast<const T *>(S->mat));
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(main_stream()));
  *equed = 1;
  return 0;
}

// the checks of porfs (apos: A's position; B, X follow AF)
int porfs_args(const char *what, chol_desc *A, chol_desc *AF, chol_desc *B, chol_desc *X, int apos, int bpos,
               int xpos) {
  int rc = square_check(what, A, apos);
  if (rc) return rc;
  if ((rc = square_check(what, AF, apos + 1))) return rc;
  if (!same_geometry(A, AF) || AF->mat == A->mat)
    return failf(-(apos + 1), "%s: AF must have A's shape, tile size and type, in storage of its own", what);
  if ((rc = rhs_check(what, A, B, bpos, "B"))) return rc;
  if ((rc = rhs_check(what, A, X, xpos, "X"))) return rc;
  if (!same_geometry(B, X)) return failf(-xpos, "%s: X must have B's shape, tile size and type", what);
  if (X->mat == A->mat || X->mat == AF->mat || X->mat == B->mat || B->mat == A->mat || B->mat == AF->mat)
    return failf(-xpos, "%s: X aliases A, AF or B", what);
  // (the wide steps solve with potrs_impl)
  if (!winv_fits(AF)) return failf(CHOL_ERR_NOT_SUPPORTED, "%s: tile size above 4096", what);
  return 0;
}

template <typename T>
int posvx_impl(int fact, int upper, chol_desc *A, chol_desc *AF, int *equed, chol_desc *S, chol_desc *B,
               chol_desc *X, double *rcond, double *ferr, double *berr) {
  hipStream_t s = main_stream();
  rf_stats.clear();
  double *st = rf_stats.v;  // total, equilibrate + scale B, factor, lansy + pocon, solve, porfs, #sweep / #potrs columns
  const long n = A->lm;
  const int nrhs = B->ln, uplo = upper ? CHOL_UPPER : CHOL_LOWER;
  EventTimer tt, tp;
  int rc = tt.start();
  if (rc) return rc;
  bool rcequ = false;
  double scond = 1;
  if ((rc = tp.start())) return rc;
  if (fact == CHOL_FACT_FACTORED) {
    rcequ = *equed == 1;
    if (rcequ && n > 0) {  // DPOSVX: scond from S itself
      T smin, smax;
      long bad;
      if ((rc = diag_scan<T>(A, S, 1, "posvx_tile", &smin, &smax, &bad))) return rc;
      if (!(smin > T(0))) return fail(-6, "posvx_tile: S has an entry <= 0");
      const T smlnum = T(Lam<T>::safmin), bignum = T(1) / smlnum;
      scond = (double)(std::max(smin, smlnum) / std::min(smax, bignum));
    }
  } else {
    *equed = 0;
    if (fact == CHOL_FACT_EQUILIBRATE) {
      int infequ = 0;
      double amax = 0;
      if ((rc = poequ_impl<T>(A, S, &scond, &amax, &infequ))) return rc;
      if (infequ == 0) {
        if ((rc = laqsy_impl<T>(upper, A, S, scond, amax, equed))) return rc;
        rcequ = *equed == 1;
      }
    }
  }
  const TileGeo ga = geo_of(A), gx = geo_of(B);
  if (rcequ) launch_row_scale<T>(s, gx, reinterpret_cast<T *>(B->mat), reinterpret_cast<const T *>(S->mat));
  HIPCHECK(hipGetLastError());
  if ((rc = tp.stop(&st[1]))) return rc;
  if (fact != CHOL_FACT_FACTORED) {
    if ((rc = tp.start())) return rc;
    launch_lacpy<T>(s, ga, upper ? 2 : 1, reinterpret_cast<const T *>(A->mat), reinterpret_cast<T *>(AF->mat));
    HIPCHECK(hipGetLastError());
    const int info = potrf_run(uplo, AF);
    if (info < 0) return info;
    if ((rc = tp.stop(&st[2]))) return rc;
    if (info > 0) {
      *rcond = 0;
      return tt.stop(&st[0]) ? CHOL_ERR_HIP : info;
    }
  }
  // rcond: anorm = ||A||_1 of the (equilibrated) A, the estimate on AF's sweeps
  if ((rc = tp.start())) return rc;
  double lv[3];
  if ((rc = lansy_impl<T>(A, upper, "posvx_tile", lv))) return rc;
  if ((rc = stage_factor_diag<T>(AF, upper, "posvx_tile"))) return rc;
  if ((rc = pocon_impl<T>(AF, upper, lv[1], rcond, /*staged=*/true))) return rc;
  if ((rc = tp.stop(&st[3]))) return rc;
  // X <- A^{-1} B: the sweeps on B's columns gathered into the R slots, or lacpy and potrs_impl when wide
  if ((rc = tp.start())) return rc;
  if (nrhs > 0 && n > 0) {
    if (nrhs <= POSVX_KX) {
      RfBufs<T> b;
      if ((rc = rf_buffers<T>(ga, nrhs, &b, "posvx_tile"))) return rc;
      const std::vector<int> all = all_cols(nrhs);
      const std::vector<VecCols> gr = groups_of(all);
      for (const VecCols &vc : gr) launch_gather<T>(s, gx, reinterpret_cast<const T *>(B->mat), vc, b.R);
      if ((rc = apply_inv<T>(upper, AF, b, b.R, all, st))) return rc;
      for (const VecCols &vc : gr) launch_scatter<T>(s, gx, reinterpret_cast<T *>(X->mat), vc, b.R, false);
    } else {
      launch_lacpy<T>(s, gx, 0, reinterpret_cast<const T *>(B->mat), reinterpret_cast<T *>(X->mat));
      if ((rc = potrs_uplo<T>(upper, AF, X))) return rc;
      st[7] += nrhs;
    }
    HIPCHECK(hipGetLastError());
  }
  if ((rc = tp.stop(&st[4]))) return rc;
  if ((rc = porfs_impl<T>(upper, A, AF, B, X, ferr, berr, st))) return rc;
  // the solution of the original system, its error bound
  if (rcequ) {
    launch_row_scale<T>(s, gx, reinterpret_cast<T *>(X->mat), reinterpret_cast<const T *>(S->mat));
    HIPCHECK(hipGetLastError());
    for (int j = 0; j < nrhs; ++j) ferr[j] = (double)(T(ferr[j]) / T(scond));
  }
  if ((rc = tt.stop(&st[0]))) return rc;
  return *rcond < Lam<T>::eps ? (int)(n + 1) : 0;
}

// the parts of porfs alone, for scripts/posvx_time.py: path 0 the residual pass over X's columns (B = X), 1 one
// application of A^{-1} to them by the multi-vector sweeps, 2 the same by potrs_impl; *ms <- the fastest of reps
template <typename T>
int bench_refine_impl(int upper, chol_desc *A, chol_desc *AF, chol_desc *X, int path, int reps, double *ms) {
  hipStream_t s = main_stream();
  const TileGeo ga = geo_of(A), gx = geo_of(X);
  const int k = X->ln;
  RfBufs<T> b;
  int rc = rf_buffers<T>(ga, k, &b, "bench_refine");
  if (rc) return rc;
  if ((rc = stage_factor_diag<T>(AF, upper, "bench_refine"))) return rc;
  const std::vector<int> all = all_cols(k);
  for (const VecCols &vc : groups_of(all)) launch_gather<T>(s, gx, reinterpret_cast<const T *>(X->mat), vc, b.R);
  double st[8] = {};
  *ms = 1e30;
  for (int r = 0; r <= reps; ++r) {
    EventTimer tt;
    if ((rc = tt.start())) return rc;
    if (path == 0) {
      for (const VecCols &vc : groups_of(all))
        launch_porfs_resid<T>(s, ga, upper, reinterpret_cast<const T *>(A->mat), gx, reinterpret_cast<const T *>(X->mat),
                              reinterpret_cast<const T *>(X->mat), vc, b.part, b.R, b.F, Lam<T>::eps, 0.0, 0.0, b.berr);
    } else {
      if ((rc = apply_inv<T>(upper, AF, b, b.R, all, st, path))) return rc;
    }
    HIPCHECK(hipGetLastError());
    double t = 0;
    if ((rc = tt.stop(&t))) return rc;
    if (r > 0) *ms = std::min(*ms, t);
  }
  return 0;
}

// ---------------------------------------------------------------- pivoted Cholesky (LAPACK DPSTRF)
// Right-looking between tile columns, left-looking inside one (pstrf.hip).  Tile column k (columns k0 .. k1-1) at
// update level k-1: the candidates d(i) = A(i,i) - (sum of squares of this tile column's finished L(i,:)), then
// one pivot step per column (two launches); then this tile column's interchanges applied at once to the rows of the
// earlier tile columns (also after a stop inside the tile column: the rows of L must match piv), then, unless the
// factorisation stopped, the walker's trailing update of the tiles (i, j >= k+1) by tile column k.  The padded rows
// of the image are not candidates: the kernels address only rows and columns 0 .. n-1.
template <typename T>
int pstrf_impl(chol_desc *A, int *piv, int *rank, double tol) {
  hipStream_t s = main_stream();
  const long n = A->lm;
  const int mb = A->mb;
  ps_stats.clear();
  double *st = ps_stats.v;  // total, pivot steps, row interchanges, trailing updates, #steps
  for (long i = 0; i < n; ++i) piv[i] = (int)(i + 1);
  *rank = 0;
  if (n == 0) return 0;
  const PsGeo g{n, mb, A->mbi, A->lmt, (long)A->bsizi};
  const long nch = pstrf_chunks(n);
  const char *what = "pstrf_tile";
  // ps[0]: dg, w; ps[1]: pval, ajj, the maximum; ps[2]: pidx, ctl, the maximum's index, pj, the interchange list
  int rc = ps.ensure_bytes(0, 2 * (size_t)n * sizeof(T), what);
  if (!rc) rc = ps.ensure_bytes(1, ((size_t)nch + 2) * sizeof(T), what);
  if (!rc) rc = ps.ensure_bytes(2, ((size_t)nch + 2 + (size_t)n + 4 * (size_t)mb) * sizeof(int), what);
  if (rc) return rc;
  T *dg = ps.as<T>(0), *w = dg + n, *pval = ps.as<T>(1), *ajj = pval + nch, *mval = ajj + 1;
  int *pidx = ps.as<int>(2), *ctl = pidx + nch, *midx = ctl + 1, *pj = midx + 1, *rows = pj + n;
  T *Am = reinterpret_cast<T *>(A->mat);
  EventTimer tt, tp;
  if ((rc = tt.start())) return rc;
  forget_winv(A->mat);  // (A is overwritten)
  // the largest diagonal entry: <= 0 or NaN -> rank 0, A unchanged; else the stopping value
  launch_pstrf_init<T>(s, g, Am, 0, dg, w, pval, pidx);
  launch_pstrf_max<T>(s, g, 0, pval, pidx, mval, midx);
  HIPCHECK(hipMemsetAsync(ctl, 0, sizeof(int), s));
  HIPCHECK(hipGetLastError());
  T amax = T(0);
  HIPCHECK(hipMemcpyAsync(&amax, mval, sizeof amax, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (!(amax > T(0))) {
    *rank = 0;
    return tt.stop(&st[0]) ? CHOL_ERR_HIP : 1;
  }
  const T dstop = tol < 0 ? T(n) * T(Lam<T>::eps) * amax : T(tol);
  std::vector<int> hp((size_t)mb), hrows;
  std::map<long, long> at;  // row -> the row whose content it holds after the interchanges so far
  long stop = 0;
  for (int k = 0; k < A->nt && !stop; ++k) {
    const long k0 = (long)k * mb, k1 = std::min<long>(k0 + mb, n);
    if ((rc = tp.start())) return rc;
    if (k > 0) launch_pstrf_init<T>(s, g, Am, k0, dg, w, pval, pidx);
    for (long j = k0; j < k1; ++j) launch_pstrf_step<T>(s, g, Am, j, k0, dstop, dg, w, pval, pidx, ctl, pj, ajj);
    HIPCHECK(hipGetLastError());
    int hctl = 0;
    HIPCHECK(hipMemcpyAsync(&hctl, ctl, sizeof hctl, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(hp.data(), pj + k0, (size_t)(k1 - k0) * sizeof(int), hipMemcpyDeviceToHost, s));
    if ((rc = tp.stop(&st[1]))) return rc;
    stop = hctl;
    const long jend = stop ? stop - 1 : k1;
    st[4] += (double)(jend - k0);
    // piv, and the composed interchanges of this tile column for the earlier ones
    at.clear();
    auto cur = [&](long r) {
      auto it = at.find(r);
      return it == at.end() ? r : it->second;
    };
    for (long j = k0; j < jend; ++j) {
      const long p = hp[j - k0];
      std::swap(piv[j], piv[p]);
      const long a = cur(j), b = cur(p);
      at[j] = b;
      at[p] = a;
    }
    if (k0 > 0) {
      hrows.clear();
      for (const auto &e : at)
        if (e.first != e.second) hrows.push_back((int)e.first);
      const int m = (int)hrows.size();
      for (int t = 0; t < m; ++t) hrows.push_back((int)at[hrows[t]]);
      if (m > 0) {
        if ((rc = tp.start())) return rc;
        HIPCHECK(hipMemcpyAsync(rows, hrows.data(), 2 * (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
        launch_pstrf_laswp<T>(s, g, Am, k0, rows, m);
        HIPCHECK(hipGetLastError());
        if ((rc = tp.stop(&st[2]))) return rc;
      }
    }
    if (stop || k + 1 >= A->nt) continue;
    // the trailing update by tile column k (chol_bench_update's call)
    if ((rc = tp.start())) return rc;
    update_cols(launch_trail_update<T>, A, k + 1, A->nt, one_panel(Am + (size_t)k * A->lmt * A->bsizi), /*yield=*/false,
                /*pan2=*/nullptr);
    HIPCHECK(hipGetLastError());
    if ((rc = tp.stop(&st[3]))) return rc;
  }
  *rank = stop ? (int)(stop - 1) : (int)n;
  if ((rc = tt.stop(&st[0]))) return rc;
  return *rank < n ? 1 : 0;
}

// pstrf's transpose of the storage: a single tile whose edge is not a multiple of 64 element by element
void pstrf_flip(chol_desc *A) {
  if (A->mbi % 64 == 0) return transpose_storage(A);
  const PsGeo g{A->lm, A->mb, A->mbi, A->lmt, (long)A->bsizi};
  by_dtype(A->dtype, [&](auto t) { launch_pstrf_transpose<decltype(t)>(main_stream(), g, (decltype(t) *)A->mat); });
}

// (not lower_run: no look for a zero pivot, its own flip, and the launch check follows the Upper path alone.  The two
// arms are written out: called through by_dtype, pstrf_impl is inlined otherwise and the library's dynamic symbols
// lose the weak std::vector<int>::push_back they have had)
int pstrf_run(int uplo, chol_desc *A, int *piv, int *rank, double tol) {
  const bool up = uplo == CHOL_UPPER;
  const int rc = through_lower(up, {A}, [&] {
    return A->dtype == CHOL_REAL_DOUBLE ? pstrf_impl<double>(A, piv, rank, tol) : pstrf_impl<float>(A, piv, rank, tol);
  }, /*wait=*/true, pstrf_flip);
  if (up) HIPCHECK(hipGetLastError());
  return rc;
}

// ---------------------------------------------------------------- generalized eigenproblem reduction (LAPACK DSYGST)
// itype 1, Lower: A <- inv(L) A inv(L)^T, B = L L^T.  LAPACK's blocked DSYGST with the tile as the block; step k (T: the
// tiles after k):
//   1. A(k,k) <- X A(k,k) X^T, X = L(k,k)^{-1} (sygst.hip; the symmetric result stays in scratch for 3 and 5)
//   2. A(T,k) <- A(T,k) L(k,k)^{-T}                       (the panel TRSM)
//   3. A(T,k) -= 1/2 L(T,k) A(k,k)                        (the batched NT product against the symmetric copy)
//   4. A(T,T) -= A(T,k) L(T,k)^T + L(T,k) A(T,k)^T        (the rank-2k update on the walker's work list)
//   5. step 3 again
// LAPACK's sixth step, A(T,k) <- inv(L(T,T)) A(T,k), is deferred: no later step reads column k, so after the walk one
// pass over the tile rows solves every column at once (sygst.hip: launch_sygst_solve_row).  The diagonal tiles of L
// are inverted once, up front (stage_factor_diag_into); their 128-block inverses are the panel TRSM's.  One stream,
// in program order; the phases are timed by events recorded between them, read after the last.
struct PhaseMarks {
  std::vector<hipEvent_t> ev;
  std::vector<int> ph;
  ~PhaseMarks() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  // the end of a stretch of phase `p` (the first mark: the start)
  int mark(int p) {
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    ev.push_back(e);
    ph.push_back(p);
    HIPCHECK(hipEventRecord(e, main_stream()));
    return 0;
  }
  // st[0] += the whole span, st[ph] += every stretch
  int sum(double *st) {
    if (ev.size() < 2) return 0;
    HIPCHECK(hipEventSynchronize(ev.back()));
    for (size_t i = 1; i < ev.size(); ++i) {
      float ms = 0;
      HIPCHECK(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
      st[ph[i]] += ms;
    }
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ev.front(), ev.back()));
    st[0] += ms;
    return 0;
  }
};

template <typename T>
int sygst_impl(chol_desc *A, chol_desc *B) {
  hipStream_t s = main_stream();
  sg_stats.clear();
  double *st = sg_stats.v;  // total, diagonal-tile inverses, chain, rank-2k updates, deferred solve, #steps
  const long n = A->lm;
  if (n == 0) return 0;
  const int nt = A->nt, mb = A->mb, e = A->mbi, lmt = A->lmt;
  const int E = condest_edge(geo_of(A)), nbm = E / MACRO;
  if (nt > 1 && e != E) return fail(CHOL_ERR_NOT_SUPPORTED, "sygst_tile: stored tile edge");  // (not made by desc_create)
  const long bs = A->bsizi, blk = (long)MACRO * MACRO, EE = (long)E * E;
  const char *what = "sygst_tile";
  // sg[0]: the inverted diagonal tiles; sg[1]: their 128-block inverses and the inversion's products; sg[2]: the
  // diagonal step's three E x E tiles and one tile row of the deferred solve
  int rc = sg.ensure_bytes(0, (size_t)nt * EE * sizeof(T), what);
  if (!rc) rc = sg.ensure_bytes(1, 2 * (size_t)nt * nbm * blk * sizeof(T), what);
  if (!rc) rc = sg.ensure_bytes(2, (3 * (size_t)EE + (size_t)(nt - 1) * bs) * sizeof(T), what);
  if (rc) return rc;
  T *Dv = sg.as<T>(0), *W = sg.as<T>(1), *Yi = W + (size_t)nt * nbm * blk;
  T *S = sg.as<T>(2), *W2 = S + EE, *Cs = W2 + EE, *yrow = Cs + EE;
  T *Am = reinterpret_cast<T *>(A->mat);
  const T *Bm = reinterpret_cast<const T *>(B->mat);
  auto tile = [&](const T *p, int i, int j) { return const_cast<T *>(p) + ((long)i + (long)j * lmt) * bs; };
  forget_winv(A->mat);  // (A is overwritten)
  PhaseMarks pm;
  enum { P_DIAG = 1, P_CHAIN, P_SYR2K, P_SOLVE };
  if ((rc = pm.mark(0))) return rc;
  stage_factor_diag_into<T>(B, 0, Dv, W, Yi);
  if ((rc = pm.mark(P_DIAG))) return rc;
  for (int k = 0; k < nt; ++k) {
    const int nv = (int)std::min<long>(mb, n - (long)k * mb);
    launch_sygst_diag<T>(s, tile(Am, k, k), e, nv, Dv + k * EE, E, S, W2, Cs);
    st[5] += 1;
    if (k + 1 < nt) {
      const int nr = nt - 1 - k;
      T *P = tile(Am, k + 1, k);
      T *Lt = tile(Bm, k + 1, k);
      launch_trsm_panel<T>(s, P, bs, nr, tile(Bm, k, k), W + (long)k * nbm * blk, e, T(1));
      launch_gemm_nt_batch<T>(s, Lt, bs, nr, Cs, 0, 1, P, bs, 0, e, T(-0.5), T(1));
      if ((rc = pm.mark(P_CHAIN))) return rc;
      update_cols(launch_syr2k_update<T>, A, k + 1, nt, one_panel(tile(Am, 0, k)), one_panel(tile(Bm, 0, k)));
      if ((rc = pm.mark(P_SYR2K))) return rc;
      launch_gemm_nt_batch<T>(s, Lt, bs, nr, Cs, 0, 1, P, bs, 0, e, T(-0.5), T(1));
    }
    HIPCHECK(hipGetLastError());
    if ((rc = pm.mark(P_CHAIN))) return rc;
  }
  for (int m = 1; m < nt; ++m) launch_sygst_solve_row<T>(s, Am, Bm, bs, lmt, E, m, Dv + m * EE, yrow);
  HIPCHECK(hipGetLastError());
  if ((rc = pm.mark(P_SOLVE))) return rc;
  return pm.sum(st);
}

// the Lower path, or Upper between transposes of both storages (U^T U = L L^T with L = U^T, and inv(U^T) A inv(U) is
// the Lower result); a zero on B's diagonal returns its index before anything is written
int sygst_run(int uplo, chol_desc *A, chol_desc *B) {
  return lower_run("sygst_tile", B, uplo, {A, B},
                   [&] { return by_dtype(A->dtype, [&](auto t) { return sygst_impl<decltype(t)>(A, B); }); });
}

// ---------------------------------------------------------------- rank-r update / downdate (LINPACK DCHUD / DCHDD)
// Lower: L <- the factor of L L^T + sigma V V^T, sigma = +1 (chud) or -1 (chdd).  Column j of L is rotated against
// every vector in turn (chud_rot.h), columns outer, vectors inner; a vector sees the columns in order and a column
// sees the vectors in order, and any schedule that keeps those two orders gives the same values.  This one walks the
// tile columns; in tile column k, for each block of 128 columns of the diagonal tile: the generator (chud.hip) on the
// diagonal block, which also leaves the rotations in a table, then the applier on the rows of the diagonal tile below
// the block; then one applier launch on every row below the diagonal tile for all the columns of k.  More than
// CHUD_GROUP vectors run as several such passes over the matrix, CHUD_GROUP vectors each.  One stream, in program
// order; the phases are timed as sygst's are.
// *info <- 0, or the 1-based column of the first rotation in that order whose rr^2 is not positive (or is NaN)
template <typename T>
int chud_impl(chol_desc *A, chol_desc *V, T sigma, int *info) {
  hipStream_t s = main_stream();
  cu_stats.clear();
  double *st = cu_stats.v;  // total, chain (generators, in-tile appliers), bulk appliers, r, #passes, stop vector
  const long n = A->lm;
  const int r = V->ln, nt = A->nt, mb = A->mb, e = A->mbi;
  const long bs = A->bsizi;
  *info = 0;
  st[3] = r;
  st[5] = -1;
  if (n == 0 || r == 0) return 0;
  // cu[0]: the rotations of one tile column (mb columns x CHUD_GROUP vectors x 4 values); cu[1]: the stop word
  int rc = cu.ensure_bytes(0, (size_t)mb * CHUD_GROUP * 4 * sizeof(T), "chud_tile");
  if (!rc) rc = cu.ensure_bytes(1, 2 * sizeof(int), "chud_tile");
  if (rc) return rc;
  T *tab = cu.as<T>(0);
  int *stop = cu.as<int>(1);
  T *Am = reinterpret_cast<T *>(A->mat);
  forget_winv(A->mat);  // (A is overwritten)
  HIPCHECK(hipMemsetAsync(stop, 0, 2 * sizeof(int), s));
  PhaseMarks pm;
  enum { P_CHAIN = 1, P_BULK };
  if ((rc = pm.mark(0))) return rc;
  for (int g0 = 0; g0 < r; g0 += CHUD_GROUP) {
    const int rg = std::min(CHUD_GROUP, r - g0);
    const ChudVecs<T> vec{reinterpret_cast<T *>(V->mat), (long)V->bsizi, V->mbi, V->lmt, V->mb, g0};
    st[4] += 1;
    for (int k = 0; k < nt; ++k) {
      const int nv = (int)std::min<long>(mb, n - (long)k * mb);  // (the columns of the tile beyond nv are padding)
      T *Acol = Am + ((long)k + (long)k * A->lmt) * bs;
      for (int c0 = 0; c0 < nv; c0 += MACRO) {
        const int nc = std::min(MACRO, nv - c0);
        launch_chud_gen<T>(s, Acol, e, c0, nc, vec, k, rg, sigma, tab, stop, k * mb + c0 + 1);
        launch_chud_apply<T>(s, Acol, bs, e, mb, n, k, c0 + nc, nv, c0, nc, tab, vec, rg);
      }
      if ((rc = pm.mark(P_CHAIN))) return rc;
      if (k + 1 < nt) {
        launch_chud_apply<T>(s, Acol, bs, e, mb, n, k, e, (long)(nt - k) * e, 0, nv, tab, vec, rg);
        if ((rc = pm.mark(P_BULK))) return rc;
      }
    }
    HIPCHECK(hipGetLastError());
  }
  int hstop[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(hstop, stop, sizeof hstop, hipMemcpyDeviceToHost, s));
  if ((rc = pm.sum(st))) return rc;
  HIPCHECK(hipStreamSynchronize(s));
  if (hstop[0]) *info = hstop[0], st[5] = hstop[1];
  return 0;
}

// the Lower path, or Upper between two transposes of A's storage (U^T U + sigma V V^T = L L^T + sigma V V^T with
// L = U^T); a zero on the factor's diagonal returns its index before anything is written
int chud_run(int uplo, chol_desc *A, chol_desc *V, double sigma, const char *what) {
  int info = 0;
  const int rc = lower_run(what, A, uplo, {A}, [&] {
    return by_dtype(A->dtype, [&](auto t) { return chud_impl<decltype(t)>(A, V, (decltype(t))sigma, &info); });
  });
  return rc ? rc : info;
}

// chol_chud_tile / chol_chdd_tile
int chud_entry(const Entry &e, int uplo, chol_desc *A, chol_desc *V, double sigma) {
  const char *what = e.what;
  if (int rc = e.begin(uplo)) return rc;
  if (!A) return e.bad(-2, "NULL A");
  if (!V) return e.bad(-3, "NULL V");
  if (A == V || (A->mat && A->mat == V->mat)) return e.bad(-3, "V aliases A");
  // (V is workspace: the image of a view of V is not written back)
  return with_views({{A, true}, {V, false}}, [&]() -> int {
    int rc = inverse_check(what, A, 2);
    if (rc) return rc;
    if ((rc = resident_whole(what, V))) return rc;
    // (A's rows, not same_rows: a one-tile A of order mb keeps its tile edge, an n x r image of it is padded to 128)
    if (V->lm != A->lm || V->mb != A->mb || V->dtype != A->dtype)
      return failf(-3, "%s: V must have A's dtype, order and tile size", what);
    return chud_run(uplo, A, V, sigma, what);
  });
}

// ---------------------------------------------------------------- circular shift of the variables (LINPACK DCHEX)
// Lower, rows and columns 0-based: L <- the factor of P^T L L^T P, P the circular shift of the variables k0..l0.  Both
// jobs move the window (rows >= k0 of the columns k0..l0) by one row and one column along the diagonal and permute the
// rows k0..l0 of the columns before k0; the rows before k0 and the columns after l0 are not touched.  A lane's source
// is another lane's destination, so the walk goes tile column by tile column and copies each one (from tile row kt down;
// before kt: its tile rows kt..lt) into a ring of two buffers before it is written; the kernels read L from the copies.
//   job 2 (k0 moves down to l0), tile columns ascending: the move (chex.hip: new column j <- old column j + 1, so tile
//     column J needs the copies of J and J + 1), then chud's generator and appliers with sigma = +1 on the window's
//     columns of J alone, against the one vector that launch_chex_vec made of the old column k0; at the end the rotated
//     vector becomes column l0.
//   job 1 (l0 moves up to k0): the rotations come from row l0 alone (launch_chex_coef, a chain of l0 - k0 pivots);
//     then tile columns descending, the applier reads the copies of J and J - 1 and writes column J rotated and moved
//     in one pass; what a row carries from one tile column to the next is in the work vector.
// One stream, in program order; the phases are timed as sygst's are.
// *info <- 0, or the 1-based new column of the first rotation whose squared pivot is not positive (or is NaN)
template <typename T>
int chex_impl(chol_desc *A, int k0, int l0, int job, int *info) {
  hipStream_t s = main_stream();
  double *st = cx_stats.v;  // total, data movement, chain, bulk appliers, job, l - k
  const long n = A->lm;
  const int nt = A->nt, mb = A->mb, e = A->mbi, lmt = A->lmt, kt = k0 / mb, lt = l0 / mb;
  const long bs = A->bsizi;
  const char *what = "chex_tile";
  *info = 0;
  // cx[0], cx[1]: the ring; cx[2]: the work vector (nt e) and the table behind it (job 1: two values a column of the
  // window; job 2: chud's four a column of a tile); cx[3]: the stop word
  const size_t tabn = job == 1 ? 2 * (size_t)(l0 - k0) : 4 * (size_t)mb;
  int rc = cx.ensure_bytes(0, (size_t)(nt - kt) * bs * sizeof(T), what);
  if (!rc) rc = cx.ensure_bytes(1, (size_t)(nt - kt) * bs * sizeof(T), what);
  if (!rc) rc = cx.ensure_bytes(2, ((size_t)nt * e + tabn) * sizeof(T), what);
  if (!rc) rc = cx.ensure_bytes(3, 2 * sizeof(int), what);
  if (rc) return rc;
  T *w = cx.as<T>(2), *tab = w + (size_t)nt * e;
  int *stop = cx.as<int>(3);
  T *Am = reinterpret_cast<T *>(A->mat);
  const ChexMat<T> M{Am, bs, lmt, e, mb, n};
  ChexStage<T> S[2];
  // tile column X saved into buffer `slot`
  auto stage = [&](int X, int slot) -> int {
    const int row0 = std::max(X, kt), cnt = (X < kt ? lt + 1 : nt) - row0;
    HIPCHECK(hipMemcpyAsync(cx.p[slot], Am + ((long)row0 + (long)X * lmt) * bs, (size_t)cnt * bs * sizeof(T),
                            hipMemcpyDeviceToDevice, s));
    S[slot] = ChexStage<T>{cx.as<T>(slot), row0};
    return 0;
  };
  forget_winv(A->mat);  // (A is overwritten)
  HIPCHECK(hipMemsetAsync(stop, 0, 2 * sizeof(int), s));
  PhaseMarks pm;
  enum { P_MOVE = 1, P_CHAIN, P_BULK };
  if ((rc = pm.mark(0))) return rc;
  if (job == 2) {
    const ChudVecs<T> vec{w, (long)e, e, nt, mb, 0};
    launch_chex_vec<T>(s, M, k0, l0, 2, w);
    for (int J = 0; J < kt; ++J) {
      if ((rc = stage(J, 0))) return rc;
      launch_chex_move<T>(s, M, J, mb, kt, lt + 1, k0, l0, 2, S[0], S[0]);
    }
    if ((rc = stage(kt, kt & 1))) return rc;
    for (int J = kt; J <= lt; ++J) {
      if (J < lt && (rc = stage(J + 1, (J + 1) & 1))) return rc;
      const int ca = std::max(k0 - J * mb, 0), cb = std::min(mb, l0 - J * mb);  // the window's columns of J before l0
      launch_chex_move<T>(s, M, J, cb, J, nt, k0, l0, 2, S[J & 1], S[J < lt ? (J + 1) & 1 : J & 1]);
      if ((rc = pm.mark(P_MOVE))) return rc;
      if (cb <= ca) continue;
      const int nv = (int)std::min<long>(mb, n - (long)J * mb);
      T *Acol = Am + ((long)J + (long)J * lmt) * bs;
      for (int c0 = ca; c0 < cb; c0 += MACRO) {
        const int nc = std::min(MACRO, cb - c0);
        launch_chud_gen<T>(s, Acol, e, c0, nc, vec, J, 1, T(1), tab, stop, J * mb + c0 + 1);
        launch_chud_apply<T>(s, Acol, bs, e, mb, n, J, c0 + nc, nv, c0, nc, tab, vec, 1);
      }
      if ((rc = pm.mark(P_CHAIN))) return rc;
      if (J + 1 < nt) {
        launch_chud_apply<T>(s, Acol, bs, e, mb, n, J, e, (long)(nt - J) * e, ca, cb - ca, tab, vec, 1);
        if ((rc = pm.mark(P_BULK))) return rc;
      }
    }
    launch_chex_setcol<T>(s, M, l0, w);
    HIPCHECK(hipGetLastError());
    if ((rc = pm.mark(P_MOVE))) return rc;
  } else {
    launch_chex_coef<T>(s, M, k0, l0, tab, w, stop);
    if ((rc = pm.mark(P_CHAIN))) return rc;
    launch_chex_vec<T>(s, M, k0, l0, 1, w);
    if ((rc = stage(lt, lt & 1))) return rc;
    for (int J = lt; J >= kt; --J) {
      if (J > kt && (rc = stage(J - 1, (J - 1) & 1))) return rc;
      if ((rc = pm.mark(P_MOVE))) return rc;
      launch_chex_apply<T>(s, M, nt, J, std::max(k0, J * mb), std::min(l0, (J + 1) * mb - 1), k0, l0, S[J & 1],
                           S[J > kt ? (J - 1) & 1 : J & 1], tab, w);
      if ((rc = pm.mark(P_BULK))) return rc;
    }
    launch_chex_move<T>(s, M, kt, k0 - kt * mb, kt, lt + 1, k0, l0, 1, S[kt & 1], S[kt & 1]);
    for (int J = 0; J < kt; ++J) {
      if ((rc = stage(J, 0))) return rc;
      launch_chex_move<T>(s, M, J, mb, kt, lt + 1, k0, l0, 1, S[0], S[0]);
    }
    HIPCHECK(hipGetLastError());
    if ((rc = pm.mark(P_MOVE))) return rc;
  }
  int hstop[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(hstop, stop, sizeof hstop, hipMemcpyDeviceToHost, s));
  if ((rc = pm.sum(st))) return rc;
  HIPCHECK(hipStreamSynchronize(s));
  *info = hstop[0];
  return 0;
}

// the Lower path, or Upper between two transposes of A's storage (the shift of U^T U's variables is that of L L^T's
// with L = U^T); a zero on the factor's diagonal returns its index before anything is written
int chex_run(int uplo, chol_desc *A, int k, int l, int job) {
  cx_stats.clear();
  cx_stats.v[4] = job;
  cx_stats.v[5] = l - k;
  if (A->lm == 0 || k == l) return 0;
  int info = 0;
  const int rc = lower_run("chex_tile", A, uplo, {A}, [&] {
    return by_dtype(A->dtype, [&](auto t) { return chex_impl<decltype(t)>(A, k - 1, l - 1, job, &info); });
  });
  return rc ? rc : info;
}

// ---------------------------------------------------------------- L D L^T without pivoting (MAGMA dsytrf_nopiv)
// Lower: A = L D L^T, L unit lower triangular, D diagonal; on return D on the diagonal and L below it.  Right-looking
// with the tile as the block; tile column k (T: the tiles below k):
//   1. A(k,k) = L_kk D_k L_kk^T in place, by 128-block steps (sytrf.hip), which also leaves the inverses of the unit
//      diagonal 128-blocks of L_kk and raises the device info word at the first zero or non-finite pivot
//   2. W(T) = A(T,k) L_kk^{-T}                            (the panel TRSM; L_kk's diagonal blocks enter through the inverses)
//   3. Wscr(T) <- W(T), A(T,k) <- L(T,k) = W(T) D_k^{-1}  (one pass; a multiplication by the reciprocal 1 / d_j)
//   4. A(T,T) -= Wscr(T) L(T,k)^T                         (the one-pass two-panel update on the walker's work list)
// One stream, in program order.  The host reads the info word once per tile column, behind the chain: the update of
// the column is already queued by then, so the device does not wait for the host.
template <typename T>
int sytrf_impl(chol_desc *A, int *info) {
  hipStream_t s = main_stream();
  // total, chain, updates [ms]; positive and negative pivots; min |d|, max |d|, max |L|
  sy_stats.clear();
  double *st = sy_stats.v;
  *info = 0;
  const long n = A->lm;
  if (n == 0) return 0;
  const int nt = A->nt, mb = A->mb, e = A->mbi, lmt = A->lmt, nbm = e / MACRO;
  const long bs = A->bsizi, blk = (long)MACRO * MACRO;
  const char *what = "sytrf_nopiv_tile";
  const int npm = ldl_partials();
  // sy[0]: the unscaled panel (one tile column); sy[1]: the diagonal tile's scratch tile, its unit 128-blocks with their
  // inverses, d and 1 / d; sy[2]: the partial maxima with the statistics and the info word
  int rc = sy.ensure_bytes(0, (size_t)std::max(1, nt - 1) * bs * sizeof(T), what);
  if (!rc) rc = sy.ensure_bytes(1, ((size_t)bs + 2 * (size_t)nbm * blk + 2 * (size_t)nt * e) * sizeof(T), what);
  if (!rc) rc = sy.ensure_bytes(2, ((size_t)npm + 8) * sizeof(double) + sizeof(int), what);
  if (rc) return rc;
  T *Wscr = sy.as<T>(0), *Wt = sy.as<T>(1), *Lc = Wt + bs, *winv = Lc + nbm * blk, *dv = winv + nbm * blk, *rv = dv + (long)nt * e;
  double *pmax = sy.as<double>(2), *out = pmax + npm;
  int *d_info = reinterpret_cast<int *>(out + 8);
  T *Am = reinterpret_cast<T *>(A->mat);
  auto tile = [&](int i, int j) { return Am + ((long)i + (long)j * lmt) * bs; };
  forget_winv(A->mat);  // (A is overwritten)
  HIPCHECK(hipMemsetAsync(pmax, 0, ((size_t)npm + 8) * sizeof(double) + sizeof(int), s));
  PhaseMarks pm;
  enum { P_CHAIN = 1, P_UPDATE };
  if ((rc = pm.mark(0))) return rc;
  int hinfo = 0;
  for (int k = 0; k < nt && !hinfo; ++k) {
    const int nr = nt - 1 - k;
    launch_ldl_tile<T>(s, tile(k, k), e, Wt, Lc, winv, dv + (long)k * e, rv + (long)k * e, d_info, k * mb, pmax);
    if (nr > 0) {
      launch_trsm_panel<T>(s, tile(k + 1, k), bs, nr, tile(k, k), winv, e, T(1));
      launch_ldl_scale<T>(s, tile(k + 1, k), Wscr, (long)nr * bs, bs, e, rv + (long)k * e, pmax);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(&hinfo, d_info, sizeof hinfo, hipMemcpyDeviceToHost, s));
    if ((rc = pm.mark(P_CHAIN))) return rc;
    const hipEvent_t chain_end = pm.ev.back();
    if (nr > 0) {
      update_cols(launch_ldl_update<T>, A, k + 1, nt, one_panel(Wscr, k + 1), one_panel(tile(0, k)));
      HIPCHECK(hipGetLastError());
      if ((rc = pm.mark(P_UPDATE))) return rc;
    }
    HIPCHECK(hipEventSynchronize(chain_end));
  }
  launch_ldl_stats<T>(s, dv, n, mb, e, pmax, out);
  HIPCHECK(hipGetLastError());
  double h[5] = {};
  HIPCHECK(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, s));
  if ((rc = pm.mark(P_CHAIN))) return rc;
  if ((rc = pm.sum(st))) return rc;
  HIPCHECK(hipStreamSynchronize(s));
  for (int i = 0; i < 5; ++i) st[3 + i] = h[i];
  *info = hinfo;
  return 0;
}

// the Lower path, or Upper between two transposes of the storage (U^T D U = L D L^T with L = U^T); -> info
int sytrf_run(int uplo, chol_desc *A) {
  if (A->mbi % MACRO) return fail(CHOL_ERR_NOT_SUPPORTED, "sytrf_nopiv_tile: stored tile edge must be a multiple of 128");
  int info = 0;
  const int rc = lower_run("sytrf_nopiv_tile", /*scan=*/nullptr, uplo, {A}, [&] {
    return by_dtype(A->dtype, [&](auto t) { return sytrf_impl<decltype(t)>(A, &info); });
  });
  return rc ? rc : info;
}

// B <- A^{-1} B from that factor: potrs_impl's sweeps over the diagonal tiles staged with unit diagonals, the
// right-hand sides scaled by 1 / d in between.  A zero on the stored diagonal returns its index before B is written.
template <typename T>
int sytrs_impl(int upper, chol_desc *A, chol_desc *B, bool diag_checked = false) {
  int info = 0;
  // (sytrs_rbt has looked before its butterflies wrote B)
  int rc = diag_checked ? 0 : diag_zero(A, &info, "sytrs_nopiv_tile");
  if (rc) return rc;
  if (info) return info;
  const int nt = A->nt, e = A->mbi;
  const long bs = A->bsizi;
  // sy[3]: the staged diagonal tiles, then 1 / d
  if ((rc = sy.ensure_bytes(3, ((size_t)nt * bs + (size_t)nt * e) * sizeof(T), "sytrs_nopiv_tile"))) return rc;
  T *U = sy.as<T>(3), *rv = U + (long)nt * bs;
  return through_lower(upper, {A}, [&] {
    launch_ldl_stage<T>(main_stream(), reinterpret_cast<const T *>(A->mat), (long)(A->lmt + 1) * bs, bs, e, nt, U, rv);
    return potrs_impl<T>(A, B, U, rv);
  });
}

// ---------------------------------------------------------------- the symmetric random butterfly transformation
// (Baboulin, Becker, Dongarra 2012; MAGMA's *_rbt): A_r = W^T A W with the recursive butterfly W = D_(d-1) ... D_0 of
// depth d (D_0 one butterfly of order n, D_k block diagonal with 2^k butterflies of order n / 2^k), then L D L^T of A_r
// without pivoting, A^{-1} = W (L D L^T)^{-1} W^T, and for sysv_rbt iterative refinement against the original A.  W is the
// n x d descriptor of the butterflies' diagonal entries (rbt.hip); W^T A W applies the level of the smallest
// butterflies first.  rb_stats [ms]: total, generation + upload of W, the transformation, the factorisation, the
// solves, the residual passes, the vector butterflies; then the refinement steps.
enum { RB_TOTAL = 0, RB_GEN, RB_XFORM, RB_FACT, RB_SOLVE, RB_RESID, RB_VEC, RB_STEPS };
constexpr int RBT_ITMAX = 10;

// the entries exp(r / 10), r uniform in [-1/2, 1/2]: the 64-bit LCG of chol_plgsy_tile stepped once per entry from the
// seed, level by level and row by row, on the host (libm's exp, rounded to T), so that (n, depth, seed, dtype) names W
template <typename T>
int rbt_generate(chol_desc *W, long n, int depth, unsigned long long seed) {
  hipStream_t s = main_stream();
  std::vector<T> h((size_t)n * depth);
  unsigned long long ran = seed;
  for (size_t x = 0; x < h.size(); ++x) {
    ran = 6364136223846793005ULL * ran + 1ULL;
    const double r = 0.5 - (double)ran * 5.4210108624275222e-20;
    h[x] = (T)std::exp(r / 10.0);
  }
  if (int rc = rb.ensure_bytes(0, h.size() * sizeof(T), "sytrf_rbt_tile")) return rc;
  HIPCHECK(hipMemcpyAsync(rb.p[0], h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
  launch_rbt_put<T>(s, geo_of(W), reinterpret_cast<T *>(W->mat), rb.as<T>(0), n, depth);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));  // (h goes out of scope)
  return 0;
}

// A <- W^T A W on the Lower stored triangle
template <typename T>
void rbt_transform(chol_desc *A, const chol_desc *W, int depth) {
  for (int k = depth - 1; k >= 0; --k)
    launch_rbt_sym<T>(main_stream(), geo_of(A), reinterpret_cast<T *>(A->mat), geo_of(W), reinterpret_cast<const T *>(W->mat), k);
}

// X <- W^T X (the smallest butterflies first) or W X (the full-order butterfly first)
template <typename T>
int rbt_vectors(chol_desc *X, const chol_desc *W, int depth, bool trans, double *st) {
  return timed(&st[RB_VEC], [&]() -> int {
    for (int x = 0; x < depth; ++x)
      launch_rbt_vec<T>(main_stream(), geo_of(X), reinterpret_cast<T *>(X->mat), geo_of(W),
                        reinterpret_cast<const T *>(W->mat), trans ? depth - 1 - x : x, trans);
    HIPCHECK(hipGetLastError());
    return 0;
  });
}

// W filled (seed != 0), A <- W^T A W on the `uplo` triangle, then sytrf_impl on it -> *info.  Upper: one transpose of
// the storage before the transformation and one after the factorisation, inside the two phases' times.
template <typename T>
int sytrf_rbt_impl(int uplo, chol_desc *A, chol_desc *W, int depth, unsigned long long seed, int *info, double *st) {
  EventTimer tp;
  int rc;
  if (seed) {
    if ((rc = tp.start())) return rc;
    if ((rc = rbt_generate<T>(W, A->lm, depth, seed))) return rc;
    if ((rc = tp.stop(&st[RB_GEN]))) return rc;
  }
  if ((rc = tp.start())) return rc;
  rc = through_lower(uplo == CHOL_UPPER, {A}, [&]() -> int {
    rbt_transform<T>(A, W, depth);
    HIPCHECK(hipGetLastError());
    if (int r = tp.stop(&st[RB_XFORM])) return r;
    if (int r = tp.start()) return r;
    return sytrf_impl<T>(A, info);
  }, /*wait=*/false);
  HIPCHECK(hipGetLastError());
  if (int r2 = tp.stop(&st[RB_FACT])) return r2;
  return rc;
}

// B <- W (L D L^T)^{-1} W^T B; a zero on the factor's stored diagonal returns its index before B is written
template <typename T>
int sytrs_rbt_impl(int upper, chol_desc *A, const chol_desc *W, int depth, chol_desc *B, double *st,
                   bool diag_checked = false) {
  int info = 0;
  // (the refinement steps solve with the factor the first solve saw)
  int rc = diag_checked ? 0 : diag_zero(A, &info, "sytrs_rbt_tile");
  if (rc) return rc;
  if (info) return info;
  if ((rc = rbt_vectors<T>(B, W, depth, true, st))) return rc;
  EventTimer tp;
  if ((rc = tp.start())) return rc;
  if ((rc = sytrs_impl<T>(upper, A, B, /*diag_checked=*/true))) return rc;
  if ((rc = tp.stop(&st[RB_SOLVE]))) return rc;
  return rbt_vectors<T>(B, W, depth, false, st);
}

// chol_sysv_rbt_tile in fp64 after its argument checks
int sysv_rbt_impl(int uplo, chol_desc *A, chol_desc *AF, chol_desc *W, int depth, unsigned long long seed, chol_desc *B,
                  chol_desc *X, int *iter, double *berr) {
  hipStream_t s = main_stream();
  double *st = rb_stats.v;
  const int up = uplo == CHOL_UPPER ? 1 : 0, nrhs = B->ln;
  const TileGeo ga = geo_of(A), gx = geo_of(B);
  const char *what = "sysv_rbt_tile";
  const size_t img = (size_t)B->lmt * B->lnt * B->bsizi * sizeof(double);
  // the residual / correction (B's tile image), the residual's per-block partial sums, colmax
  int rc = rb.ensure_bytes(1, img, what);
  if (!rc) rc = rb.ensure_bytes(2, sym_resid_part_bytes(ga, nrhs), what);
  if (!rc) rc = rb.ensure_bytes(3, colmax_bytes(nrhs), what);
  if (rc) return rc;
  double *R = rb.as<double>(1), *part = rb.as<double>(2);
  unsigned long long *colmax = rb.as<unsigned long long>(3);
  std::vector<unsigned long long> hmax(2 * nrhs);
  chol_desc Rd = scratch_view(B, R);
  EventTimer tt, tp;
  if ((rc = tt.start())) return rc;
  // anrm (counted with the residual passes: the same kernel), AF <- the triangle of A
  if ((rc = tp.start())) return rc;
  HIPCHECK(hipMemsetAsync(colmax, 0, colmax_bytes(nrhs), s));
  HIPCHECK(hipMemsetAsync(R, 0, img, s));  // (the solve runs on whole tiles: the padding must be finite)
  launch_sym_inf_norm(s, ga, up, (const double *)A->mat, part, colmax);
  launch_lacpy<double>(s, ga, up ? 2 : 1, (const double *)A->mat, (double *)AF->mat);
  HIPCHECK(hipGetLastError());
  unsigned long long anrm_bits = 0;
  HIPCHECK(hipMemcpyAsync(&anrm_bits, colmax, sizeof anrm_bits, hipMemcpyDeviceToHost, s));
  if ((rc = tp.stop(&st[RB_RESID]))) return rc;
  const RefineTol tol(anrm_bits, A->lm);
  auto finish = [&](int it, int ret) {
    *iter = it;
    const int r = tt.stop(&st[RB_TOTAL]);
    return r ? r : ret;
  };
  int info = 0;
  rc = sytrf_rbt_impl<double>(uplo, AF, W, depth, seed, &info, st);
  if (rc) return rc;
  if (info) return finish(-3, info);  // (X untouched)
  launch_lacpy<double>(s, gx, 0, (const double *)B->mat, (double *)X->mat);
  HIPCHECK(hipGetLastError());
  rc = sytrs_rbt_impl<double>(up, AF, W, depth, X, st);
  if (rc < 0) return rc;
  if (rc > 0) return finish(-3, rc);
  for (int it = 0;; ++it) {
    // R = B - A X from the stored triangle of the untouched A; the column maxima of R and X
    if ((rc = tp.start())) return rc;
    HIPCHECK(hipMemsetAsync(colmax, 0, colmax_bytes(nrhs), s));
    launch_sym_resid_f64(s, ga, up, (const double *)A->mat, gx, (const double *)X->mat, (const double *)B->mat, part, R,
                         colmax);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hmax.data(), colmax, 2 * nrhs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = tp.stop(&st[RB_RESID]))) return rc;
    if (tol.converged(hmax.data(), nrhs, berr)) return finish(it, 0);
    if (it == RBT_ITMAX) return finish(-31, A->lm + 1);
    rc = sytrs_rbt_impl<double>(up, AF, W, depth, &Rd, st, /*diag_checked=*/true);
    if (rc) return rc;
    launch_geadd<double>(s, gx, 1.0, R, 1.0, (double *)X->mat);
    HIPCHECK(hipGetLastError());
    st[RB_STEPS] += 1;
  }
}

// ---------------------------------------------------------------- one half of the factor alone (LAPACK DTRTRS, BLAS DTRMM, log det)
// trtrs: B <- inv(op(T)) B, T the `uplo` triangle.  (Lower, NoTrans) and (Upper, Trans) are potrs's forward half,
// L Y = B; the other two its backward half, L^T X = Y.  Up to TRTRS_KX columns run as one pass of the multi-vector
// sweeps (condest.hip) in groups of 8 on the gathered columns, the diagonal tiles staged and inverted once per call;
// more columns run as one sweep of potrs_impl's on Z = B^T (Upper between two transposes of the storage, as potrs).
// trmm: B <- alpha op(T) B.  Up to TRMM_KX columns in groups of 8 by trmm.hip's block products; more columns as
// products of whole tiles on Z = B^T (ZSweeps::product), with the diagonal tiles staged as clean triangles.
// The limits: apply_inv's rule (POSVX_KX).  Measured: the forward solve crosses at about 72 columns at
// N = 65536 / 1024 and 43 at 16384 / 512, the backward solve at about 36 and 24, the product beyond 70 in every case
constexpr int TRTRS_KX = POSVX_KX, TRMM_KX = POSVX_KX;
int trtrs_kx = TRTRS_KX, trmm_kx = TRMM_KX;  // (chol_debug_half_limits moves them for scripts/trtrs_time.py)

// the factor the wide paths work on: A's own image, or, for a one-tile A whose edge is not a multiple of 128 (its
// n x nrhs image has that tile padded to one), a copy with B's tile edge and the identity beyond A's (tr[2])
template <typename T>
int wide_factor(chol_desc *A, const chol_desc *B, chol_desc *Aw, const char *what) {
  *Aw = scratch_view(A, A->mat);
  if (A->mbi == B->mbi) return 0;
  hipStream_t s = main_stream();
  const int e = A->mbi, ep = B->mbi;
  if (int rc = tr.ensure_bytes(2, (size_t)ep * ep * sizeof(T), what)) return rc;
  T *S = tr.as<T>(2);
  HIPCHECK(hipMemsetAsync(S, 0, (size_t)ep * ep * sizeof(T), s));
  HIPCHECK(hipMemcpy2DAsync(S, (size_t)ep * sizeof(T), A->mat, (size_t)e * sizeof(T), (size_t)e * sizeof(T), e,
                            hipMemcpyDeviceToDevice, s));
  launch_pad_identity<T>(s, S, e, ep);
  Aw->mat = S;
  Aw->mbi = ep;
  Aw->bsizi = ep * ep;
  return 0;
}

// st: total, staging of the diagonal tiles, sweeps or products [ms]; columns through the narrow / the wide path
template <typename T>
int trtrs_impl(int upper, int trans, chol_desc *A, chol_desc *B, double *st) {
  hipStream_t s = main_stream();
  const char *what = "trtrs_tile";
  const int nrhs = B->ln;
  if (A->lm == 0 || nrhs == 0) return 0;
  const bool fwd = (upper != 0) == (trans != 0);
  EventTimer tp;
  int rc = 0;
  if (nrhs <= trtrs_kx) {
    const TileGeo ga = geo_of(A), gx = geo_of(B);
    const int bpt = condest_edge(ga) / MACRO;
    const long nv = (long)condest_vec_elems(ga), pgn = 2 * (long)ga.lmt * bpt * bpt * MACRO;
    if ((rc = tp.start())) return rc;
    if ((rc = stage_factor_diag<T>(A, upper, what))) return rc;
    if ((rc = tp.stop(&st[1]))) return rc;
    // the gathered columns, the padding vectors, the sweeps' scratch (whose first 8 vectors take the results)
    if ((rc = tr.ensure_bytes(0, (16 * (size_t)nv + msweep_scratch_elems(ga)) * sizeof(T), what))) return rc;
    T *x = tr.as<T>(0), *pad = x + 8 * nv, *sw = pad + 8 * nv;
    const MSweepBufs<T> mb{sw, sw + 8 * nv, sw + 8 * nv + 8 * pgn};
    if ((rc = tp.start())) return rc;
    for (const VecCols &vc : groups_of(all_cols(nrhs))) {
      VecCols in = vc;  // (slot j of the group <- column d[j])
      T *xs[8];
      for (int j = 0; j < vc.n; ++j) in.v[j] = j, xs[j] = x + (long)j * nv;
      launch_gather<T>(s, gx, reinterpret_cast<const T *>(B->mat), in, x);
      launch_msweep<T>(s, ga, upper, reinterpret_cast<const T *>(A->mat), cn.as<const T>(0), xs, vc.n, pad, mb,
                       fwd ? SWEEP_FORWARD : SWEEP_BACKWARD);
      launch_scatter<T>(s, gx, reinterpret_cast<T *>(B->mat), in, mb.y, false);
    }
    HIPCHECK(hipGetLastError());
    if ((rc = tp.stop(&st[2]))) return rc;
    st[3] = nrhs;
    return 0;
  }
  chol_desc Aw;
  if ((rc = wide_factor<T>(A, B, &Aw, what))) return rc;
  if ((rc = tp.start())) return rc;
  rc = through_lower(upper, {&Aw}, [&]() -> int {
    ZSweeps<T> z;
    if (int r = z.init(&Aw, B, nullptr, what)) return r;
    z.load();
    if (fwd)
      z.forward();
    else if (int r = z.backward())
      return r;
    z.store();
    return z.finish();
  });
  if (rc) return rc;
  if ((rc = tp.stop(&st[2]))) return rc;
  st[4] = nrhs;
  return 0;
}

template <typename T>
int trmm_impl(int upper, int trans, double alpha, chol_desc *A, chol_desc *B, double *st) {
  hipStream_t s = main_stream();
  const char *what = "trmm_tile";
  const int nrhs = B->ln;
  if (A->lm == 0 || nrhs == 0) return 0;
  EventTimer tp;
  int rc = 0;
  if (nrhs <= trmm_kx) {
    const TileGeo ga = geo_of(A), gx = geo_of(B);
    const long nv = (long)condest_vec_elems(ga);
    const size_t pe = trmm_part_elems(ga, refine_width(std::min(nrhs, 8)));
    if ((rc = tr.ensure_bytes(0, (8 * (size_t)nv + pe) * sizeof(T), what))) return rc;
    T *x = tr.as<T>(0), *part = x + 8 * nv;
    if ((rc = tp.start())) return rc;
    for (const VecCols &vc : groups_of(all_cols(nrhs))) {
      VecCols in = vc;
      for (int j = 0; j < vc.n; ++j) in.v[j] = j;
      launch_trmm_narrow<T>(s, ga, upper, trans, reinterpret_cast<const T *>(A->mat), gx, reinterpret_cast<T *>(B->mat),
                            in, T(alpha), x, part);
    }
    HIPCHECK(hipGetLastError());
    if ((rc = tp.stop(&st[2]))) return rc;
    st[3] = nrhs;
    return 0;
  }
  chol_desc Aw;
  if ((rc = wide_factor<T>(A, B, &Aw, what))) return rc;
  // on the Lower orientation: Upper NoTrans is L^T B, Upper Trans is L B
  const bool ltrans = (upper != 0) != (trans != 0);
  rc = through_lower(upper, {&Aw}, [&]() -> int {
    ZSweeps<T> z;
    if (int r = z.init(&Aw, B, nullptr, what, (size_t)Aw.nt)) return r;
    if (int r = tp.start()) return r;
    launch_tri_tiles<T>(s, z.La, (long)(Aw.lmt + 1) * z.bs, z.mb, z.nt, ltrans, z.more);
    if (int r = tp.stop(&st[1])) return r;
    if (int r = tp.start()) return r;
    z.load();
    if (int r = z.product(ltrans, T(alpha), z.more)) return r;
    z.store();
    if (int r = z.finish()) return r;
    return tp.stop(&st[2]);
  });
  if (rc) return rc;
  st[4] = nrhs;
  return 0;
}

// ---------------------------------------------------------------- the symmetric product (BLAS DSYMM, side Left)
// C <- alpha A B + beta C from the `upper` / lower triangle of A, by symm.hip's one kernel for every nrhs; no scratch.
// st: total, kernel [ms], nrhs, the column width of a workgroup's block (0: alpha == 0, A and B are not read), the
// workgroups launched, 2 n^2 nrhs
template <typename T>
int symm_impl(int upper, double alpha, const chol_desc *A, const chol_desc *B, double beta, chol_desc *C, double *st) {
  const int nrhs = B->ln;
  st[2] = nrhs;
  st[5] = 2.0 * (double)A->lm * (double)A->lm * nrhs;
  if (A->lm == 0 || nrhs == 0) return 0;
  EventTimer tp;
  if (int rc = tp.start()) return rc;
  const long wgs = launch_symm<T>(main_stream(), geo_of(A), upper, reinterpret_cast<const T *>(A->mat), geo_of(B),
                                  reinterpret_cast<const T *>(B->mat), geo_of(C), reinterpret_cast<T *>(C->mat), T(alpha),
                                  T(beta));
  HIPCHECK(hipGetLastError());
  st[3] = T(alpha) == T(0) ? 0 : symm_width(nrhs);
  st[4] = (double)wgs;
  return tp.stop(&st[1]);
}

// the rule for an n x nrhs operand X of chol_symm_tile (pos: its argument position): chol_trmm_tile's rule for its B
int symm_operand(const chol_desc *A, const chol_desc *X, int pos, const char *name) {
  if (int rc = resident_whole("symm_tile", X)) return rc;
  if (X->lm != A->lm || X->mb != A->mb || X->dtype != A->dtype ||
      (X->mbi != A->mbi && !(A->nt == 1 && X->mbi == roundup(A->mbi, MACRO))))
    return failf(-pos, "symm_tile: %s must have A's dtype, order and tile size", name);
  return 0;
}

// *logdet <- 2 sum log A(j,j); -> info: the first j (1-based) with A(j,j) <= 0 or NaN
template <typename T>
int logdet_impl(const chol_desc *A, double *logdet, int *info) {
  hipStream_t s = main_stream();
  *info = 0;
  *logdet = 0;
  if (A->lm == 0) return 0;
  if (int rc = tr.ensure_bytes(3, logdet_part_bytes() + 2 * sizeof(double), "logdet_tile")) return rc;
  double *part = tr.as<double>(3), *out = part + logdet_part_bytes() / sizeof(double);
  launch_logdet<T>(s, geo_of(A), reinterpret_cast<const T *>(A->mat), part, out);
  HIPCHECK(hipGetLastError());
  double h[2] = {0, -1};
  HIPCHECK(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *logdet = h[0];
  if (h[1] >= 0) *info = (int)h[1] + 1;
  return 0;
}

// the argument rules chol_trtrs_tile and chol_trmm_tile share (apos, bpos: the positions of A and B)
int half_args(const char *what, chol_desc *A, int apos, chol_desc *B, int bpos) {
  if (!A) return failf(-apos, "%s: NULL A", what);
  if (!B) return failf(-bpos, "%s: NULL B", what);
  if (A == B || (A->mat && A->mat == B->mat)) return failf(-bpos, "%s: B aliases A", what);
  int rc = inverse_check(what, A, apos);
  if (rc) return rc;
  if ((rc = resident_whole(what, B))) return rc;
  // (A's rows, but not same_rows: a one-tile A of order mb keeps its tile edge, an n x nrhs image of it is padded to 128)
  if (B->lm != A->lm || B->mb != A->mb || B->dtype != A->dtype ||
      (B->mbi != A->mbi && !(A->nt == 1 && B->mbi == roundup(A->mbi, MACRO))))
    return failf(-bpos, "%s: B must have A's dtype, order and tile size", what);
  if (!winv_fits(B)) return failf(CHOL_ERR_NOT_SUPPORTED, "%s: tile size above 4096", what);
  return 0;
}

// the argument rules the butterfly routines share: A square, device-resident, single process, stored tile edge a
// multiple of 128; depth 1 or 2; the order a multiple of 2^depth; W n x depth or wider with A's dtype and row tiling
int rbt_args(const char *what, int uplo, chol_desc *A, int apos, chol_desc *W, int wpos, int depth, int dpos) {
  auto bad = [&](int code, const char *why) { return failf(code, "%s: %s", what, why); };
  if (uplo != CHOL_LOWER && uplo != CHOL_UPPER) return bad(-1, "uplo");
  if (!A) return bad(-apos, "NULL A");
  int rc = inverse_check(what, A, apos);
  if (rc) return rc;
  if (A->mbi % MACRO) return bad(CHOL_ERR_NOT_SUPPORTED, "stored tile edge must be a multiple of 128");
  if (!W) return bad(-wpos, "NULL W");
  if (W->p * W->q != 1 || !W->on_device) return bad(CHOL_ERR_NOT_SUPPORTED, "W must be a device-resident single-process descriptor");
  if (depth != 1 && depth != 2) return bad(-dpos, "depth must be 1 or 2");
  if (!same_rows(A, W) || W->nb != A->nb || W->ln < depth || W == A || W->mat == A->mat)
    return bad(-wpos, "W must be an n x depth descriptor of its own with A's order, tile size and type");
  if (A->lm % (1 << depth))
    return bad(CHOL_ERR_NOT_SUPPORTED, "the order must be a multiple of 2^depth (border A with an identity row)");
  if (!winv_fits(A)) return bad(CHOL_ERR_NOT_SUPPORTED, "tile size above 4096");
  return 0;
}

}  // namespace

void cholmi::spd_release() {
  work.release();
  mx.release();
  iv.release();
  cn.release();
  rf.release();
  ps.release();
  sg.release();
  cu.release();
  cx.release();
  sy.release();
  rb.release();
  tr.release();
}

// ---------------------------------------------------------------- the entry points (C linkage: include/cholmi.h)
int chol_potrs_tile(int uplo, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"potrs_tile"};
  return with_views({{A, false}, {B, true}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = resident_whole(e.what, A);
  if (!rc) rc = resident_whole(e.what, B);
  if (rc) return rc;
  if (A->mt != A->nt || A->lm != A->ln) return e.bad(-2, "A is not square");
  if (!same_rows(A, B)) return e.bad(-3, "B must have A's order, tile size and type");
  if (A->mbi % 64) return e.bad(CHOL_ERR_NOT_SUPPORTED, "stored tile edge must be a multiple of 64");
  CHECK_WINV(A, e.what);
  const int up = uplo == CHOL_UPPER;
  rc = by_dtype(A->dtype, [&](auto t) { return potrs_uplo<decltype(t)>(up, A, B); });
  if (up) HIPCHECK(hipStreamSynchronize(main_stream()));
  return rc;
  });
}

// The composite entry points (posv, poinv, sysv_nopiv, and dsposv's fallback) keep every check of their own: the
// routines they call repeat none of them with the same text, since each text begins with its routine's name
int chol_posv_tile(int uplo, chol_desc_t *A, chol_desc_t *B) {
  if (uplo != CHOL_LOWER && uplo != CHOL_UPPER) return fail(-1, "posv_tile: uplo");
  const int info = chol_potrf_tile(uplo, A);
  if (info != 0) return info;  // > 0: not positive definite, B untouched (LAPACK dposv)
  return chol_potrs_tile(uplo, A, B);
}

int chol_dsposv_tile(int uplo, chol_desc_t *A, chol_desc_t *B, chol_desc_t *X, int *iter) {
  const Entry e{"dsposv_tile"};
  return with_views({{A, false}, {B, false}, {X, false}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = resident_whole(e.what, A);
  if (rc) return rc;
  if (A->dtype != CHOL_REAL_DOUBLE) return e.bad(-2, "A must be fp64");
  if (A->mt != A->nt || A->lm != A->ln) return e.bad(-2, "A is not square");
  if (!B) return e.bad(-3, "B is NULL");
  if ((rc = resident_whole(e.what, B))) return rc;
  if (!same_rows(A, B) || B->mat == A->mat) return e.bad(-3, "B must be fp64 with A's order and tile size");
  if (!X) return e.bad(-4, "X is NULL");
  if ((rc = resident_whole(e.what, X))) return rc;
  if (!same_geometry(B, X)) return e.bad(-4, "X must have B's shape, tile size and type");
  if (X->mat == A->mat || X->mat == B->mat) return e.bad(-4, "X aliases A or B");
  if (!iter) return e.bad(-5, "iter is NULL");
  if (A->user_mat || B->user_mat || X->user_mat)
    return e.bad(CHOL_ERR_NOT_SUPPORTED, "sub-matrix views over a user buffer");
  if (A->mbi % MACRO) return e.bad(CHOL_ERR_NOT_SUPPORTED, "stored tile edge must be a multiple of 128");
  CHECK_WINV(A, e.what);
  rc = dsposv_mixed(uplo, A, B, X, iter);
  if (rc < 0) return rc;
  if (*iter >= 0) return 0;
  // fallback (LAPACK dsposv): X <- B, then dposv in fp64 -- A then holds the fp64 factor
  launch_lacpy<double>(main_stream(), geo_of(B), 0, (const double *)B->mat, (double *)X->mat);
  HIPCHECK(hipStreamSynchronize(main_stream()));
  const int info = chol_potrf_tile(uplo, A);
  if (info != 0) return info;
  return chol_potrs_tile(uplo, A, X);
  });
}

int chol_last_dsposv_stats(double *out8) { return mx_stats.read("dsposv", out8); }

int chol_trtri_tile(int uplo, int diag, chol_desc_t *A) {
  const Entry e{"trtri_tile"};
  return with_views({{A, true}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (rc) return rc;
  if (diag != CHOL_NONUNIT && diag != CHOL_UNIT) return e.bad(-2, "diag");
  if (diag == CHOL_UNIT)
    return e.bad(CHOL_ERR_NOT_SUPPORTED, "ChamUnit (a Cholesky factor has no unit diagonal)");
  if ((rc = inverse_check(e.what, A, 3))) return rc;
  return inverse_run(uplo, A, false);
  });
}

int chol_potri_tile(int uplo, chol_desc_t *A) {
  const Entry e{"potri_tile"};
  return with_views({{A, true}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = inverse_check(e.what, A, 2);
  return rc ? rc : inverse_run(uplo, A, true);
  });
}

int chol_poinv_tile(int uplo, chol_desc_t *A) {
  const Entry e{"poinv_tile"};
  int rc = e.begin(uplo);
  if (!rc) rc = inverse_check(e.what, A, 2);  // (before the factorisation writes anything)
  if (rc) return rc;
  const int info = chol_potrf_tile(uplo, A);
  if (info != 0) return info;  // > 0: not positive definite, A as potrf leaves it
  return chol_potri_tile(uplo, A);
}

int chol_lansy_tile(int norm, int uplo, chol_desc_t *A, double *value) {
  const Entry e{"lansy_tile"};
  return with_views({{A, false}}, [&]() -> int {
  int rc = e.begin();
  if (rc) return rc;
  int kind;
  switch (norm) {
    case CHOL_MAX_NORM: kind = 0; break;
    case CHOL_ONE_NORM:
    case CHOL_INF_NORM: kind = 1; break;  // (symmetric: one value for both)
    case CHOL_FROBENIUS_NORM: kind = 2; break;
    default: return e.bad(-1, "norm");
  }
  if ((rc = e.uplo_at(uplo, 2))) return rc;
  if ((rc = inverse_check(e.what, A, 3))) return rc;
  if (!value) return e.bad(-4, "NULL value");
  const int up = uplo == CHOL_UPPER;
  double v[3];
  if ((rc = by_dtype(A->dtype, [&](auto t) { return lansy_impl<decltype(t)>(A, up, e.what, v); }))) return rc;
  *value = kind == 2 ? std::sqrt(v[2]) : v[kind];
  return 0;
  });
}

int chol_pocon_tile(int uplo, chol_desc_t *A, double anorm, double *rcond) {
  const Entry e{"pocon_tile"};
  return with_views({{A, false}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = inverse_check(e.what, A, 2);
  if (rc) return rc;
  if (!(anorm >= 0)) return e.bad(-3, "anorm is negative or NaN");
  if (!rcond) return e.bad(-4, "NULL rcond");
  const int up = uplo == CHOL_UPPER;
  return by_dtype(A->dtype, [&](auto t) { return pocon_impl<decltype(t)>(A, up, anorm, rcond); });
  });
}

int chol_last_pocon_stats(double *out4) { return cn_stats.read("pocon", out4, 4); }

int chol_poequ_tile(chol_desc_t *A, chol_desc_t *S, double *scond, double *amax) {
  const Entry e{"poequ_tile"};
  return with_views({{A, false}, {S, true}}, [&]() -> int {
  int rc = e.begin();
  if (!rc) rc = square_check(e.what, A, 1);
  if (!rc) rc = rhs_check(e.what, A, S, 2, "S");
  if (rc) return rc;
  if (S->ln != 1 || S->mat == A->mat) return e.bad(-2, "S must be an n x 1 descriptor of its own");
  if (!scond) return e.bad(-3, "NULL scond");
  if (!amax) return e.bad(-4, "NULL amax");
  int info = 0;
  rc = by_dtype(A->dtype, [&](auto t) { return poequ_impl<decltype(t)>(A, S, scond, amax, &info); });
  return rc ? rc : info;
  });
}

int chol_laqsy_tile(int uplo, chol_desc_t *A, chol_desc_t *S, double scond, double amax, int *equed) {
  const Entry e{"laqsy_tile"};
  return with_views({{A, true}, {S, false}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = square_check(e.what, A, 2);
  if (!rc) rc = rhs_check(e.what, A, S, 3, "S");
  if (rc) return rc;
  if (S->ln != 1 || S->mat == A->mat) return e.bad(-3, "S must be an n x 1 descriptor of its own");
  if (!(scond >= 0)) return e.bad(-4, "scond is negative or NaN");
  if (!(amax >= 0)) return e.bad(-5, "amax is negative or NaN");
  if (!equed) return e.bad(-6, "NULL equed");
  const int up = uplo == CHOL_UPPER;
  return by_dtype(A->dtype, [&](auto t) { return laqsy_impl<decltype(t)>(up, A, S, scond, amax, equed); });
  });
}

int chol_porfs_tile(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *B, chol_desc_t *X, double *ferr,
                    double *berr) {
  const Entry e{"porfs_tile"};
  return with_views({{A, false}, {AF, false}, {B, false}, {X, true}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = porfs_args(e.what, A, AF, B, X, 2, 4, 5);
  if (rc) return rc;
  if (!ferr) return e.bad(-6, "NULL ferr");
  if (!berr) return e.bad(-7, "NULL berr");
  const int up = uplo == CHOL_UPPER;
  rf_stats.clear();
  return timed(&rf_stats.v[0], [&] {
    return by_dtype(A->dtype, [&](auto t) {
      using T = decltype(t);
      const int r = stage_factor_diag<T>(AF, up, e.what);
      return r ? r : porfs_impl<T>(up, A, AF, B, X, ferr, berr, rf_stats.v);
    });
  });
  });
}

int chol_posvx_tile(int fact, int uplo, chol_desc_t *A, chol_desc_t *AF, int *equed, chol_desc_t *S, chol_desc_t *B,
                    chol_desc_t *X, double *rcond, double *ferr, double *berr) {
  const Entry e{"posvx_tile"};
  return with_views({{A, true}, {AF, true}, {S, true}, {B, true}, {X, true}}, [&]() -> int {
  int rc = e.begin();
  if (rc) return rc;
  if (fact != CHOL_FACT_NONE && fact != CHOL_FACT_EQUILIBRATE && fact != CHOL_FACT_FACTORED) return e.bad(-1, "fact");
  if ((rc = e.uplo_at(uplo, 2))) return rc;
  if ((rc = porfs_args(e.what, A, AF, B, X, 3, 7, 8))) return rc;
  if (!equed) return e.bad(-5, "NULL equed");
  if (fact == CHOL_FACT_FACTORED && *equed != 0 && *equed != 1) return e.bad(-5, "equed must be 0 or 1");
  const bool need_s = fact == CHOL_FACT_EQUILIBRATE || (fact == CHOL_FACT_FACTORED && *equed == 1);
  if (need_s || S) {
    if ((rc = rhs_check(e.what, A, S, 6, "S"))) return rc;
    if (S->ln != 1 || S->mat == A->mat || S->mat == AF->mat || S->mat == B->mat || S->mat == X->mat)
      return e.bad(-6, "S must be an n x 1 descriptor of its own");
  }
  if (!rcond) return e.bad(-9, "NULL rcond");
  if (!ferr) return e.bad(-10, "NULL ferr");
  if (!berr) return e.bad(-11, "NULL berr");
  const int up = uplo == CHOL_UPPER;
  return by_dtype(A->dtype, [&](auto t) {
    return posvx_impl<decltype(t)>(fact, up, A, AF, equed, S, B, X, rcond, ferr, berr);
  });
  });
}

int chol_bench_refine(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *X, int path, int reps, double *ms) {
  const Entry e{"bench_refine"};
  return with_views({{A, false}, {AF, false}, {X, false}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (!rc) rc = square_check(e.what, A, 2);
  if (!rc) rc = square_check(e.what, AF, 3);
  if (!rc) rc = rhs_check(e.what, A, X, 4, "X");
  if (rc) return rc;
  if (path < 0 || path > 2 || reps < 1 || !ms) return e.bad(-5, "path, reps or ms");
  const int up = uplo == CHOL_UPPER;
  return by_dtype(A->dtype, [&](auto t) { return bench_refine_impl<decltype(t)>(up, A, AF, X, path, reps, ms); });
  });
}

int chol_last_posvx_stats(double *out8) { return rf_stats.read("posvx", out8); }

int chol_pstrf_tile(int uplo, chol_desc_t *A, int *piv, int *rank, double tol) {
  const Entry e{"pstrf_tile"};
  return with_views({{A, true}}, [&]() -> int {
  int rc = e.begin(uplo);
  if (rc) return rc;
  if (!A) return e.bad(-2, "NULL descriptor");
  if ((rc = resident_whole(e.what, A))) return rc;
  if (A->mt != A->nt || A->lm != A->ln) return e.bad(-2, "A is not square");
  if (!piv) return e.bad(-3, "NULL piv");
  if (!rank) return e.bad(-4, "NULL rank");
  if (std::isnan(tol)) return e.bad(-5, "tol is NaN");
  return pstrf_run(uplo, A, piv, rank, tol);
  });
}

int chol_last_pstrf_stats(double *out8) { return ps_stats.read("pstrf", out8); }

int chol_sygst_tile(int itype, int uplo, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"sygst_tile"};
  int rc = e.begin();
  if (rc) return rc;
  if (itype < 1 || itype > 3) return e.bad(-1, "itype");
  if ((rc = e.uplo_at(uplo, 2))) return rc;
  if (!A) return e.bad(-3, "NULL A");
  if (!B) return e.bad(-4, "NULL B");
  if (A == B || (A->mat && A->mat == B->mat)) return e.bad(-4, "B aliases A");
  return with_views({{A, true}, {B, false}}, [&]() -> int {
  int rc = inverse_check(e.what, A, 3);
  if (!rc) rc = inverse_check(e.what, B, 4);
  if (rc) return rc;
  if (!same_geometry(A, B)) return e.bad(-4, "B's dtype or geometry differs from A's");
  if (itype != 1) return e.bad(CHOL_ERR_NOT_SUPPORTED, "itype 2 and 3 (C = L^T A L)");
  CHECK_WINV(A, e.what);
  return sygst_run(uplo, A, B);
  });
}

int chol_last_sygst_stats(double *out8) { return sg_stats.read("sygst", out8); }

int chol_chud_tile(int uplo, chol_desc_t *A, chol_desc_t *V) {
  return chud_entry(Entry{"chud_tile"}, uplo, A, V, 1.0);
}

int chol_chdd_tile(int uplo, chol_desc_t *A, chol_desc_t *V) {
  return chud_entry(Entry{"chdd_tile"}, uplo, A, V, -1.0);
}

int chol_last_chud_stats(double *out8) { return cu_stats.read("chud", out8); }

int chol_chex_tile(int uplo, chol_desc_t *A, int k, int l, int job) {
  const Entry e{"chex_tile"};
  if (int rc = e.begin(uplo)) return rc;
  if (!A) return e.bad(-2, "NULL A");
  return with_views({{A, true}}, [&]() -> int {
    if (int rc = inverse_check(e.what, A, 2)) return rc;
    const int n = A->lm;
    if (n > 0 && (k < 1 || k > n)) return e.bad(-3, "k outside 1..n");
    if (n > 0 && (l < k || l > n)) return e.bad(-4, "l outside k..n");
    if (job != 1 && job != 2) return e.bad(-5, "job must be 1 (right shift) or 2 (left shift)");
    return chex_run(uplo, A, k, l, job);
  });
}

int chol_last_chex_stats(double *out8) { return cx_stats.read("chex", out8); }

int chol_trtrs_tile(int uplo, int trans, int diag, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"trtrs_tile"};
  if (int rc = e.begin(uplo)) return rc;
  if (trans != CHOL_NOTRANS && trans != CHOL_TRANS) return e.bad(-2, "trans");
  if (diag != CHOL_NONUNIT && diag != CHOL_UNIT) return e.bad(-3, "diag");
  if (!A) return e.bad(-4, "NULL A");
  if (!B) return e.bad(-5, "NULL B");
  if (A == B || (A->mat && A->mat == B->mat)) return e.bad(-5, "B aliases A");
  return with_views({{A, false}, {B, true}}, [&]() -> int {
  if (int rc = half_args(e.what, A, 4, B, 5)) return rc;
  if (diag == CHOL_UNIT)
    return e.bad(CHOL_ERR_NOT_SUPPORTED, "ChamUnit (a Cholesky factor has no unit diagonal)");
  const int up = uplo == CHOL_UPPER, tr_ = trans == CHOL_TRANS;
  tr_stats.clear();
  // (not lower_run: the Lower path is inside trtrs_impl, around its wide sweep alone, and the time is taken around both)
  return timed(&tr_stats.v[0], [&]() -> int {
    int info = 0;
    if (int rc = diag_zero(A, &info, e.what)) return rc;
    if (info) return info;  // (LAPACK: B is unchanged)
    return by_dtype(A->dtype, [&](auto t) { return trtrs_impl<decltype(t)>(up, tr_, A, B, tr_stats.v); });
  });
  });
}

int chol_trmm_tile(int side, int uplo, int trans, int diag, double alpha, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"trmm_tile"};
  if (int rc = e.begin()) return rc;
  if (side != CHOL_LEFT && side != CHOL_RIGHT) return e.bad(-1, "side");
  if (int rc = e.uplo_at(uplo, 2)) return rc;
  if (trans != CHOL_NOTRANS && trans != CHOL_TRANS) return e.bad(-3, "trans");
  if (diag != CHOL_NONUNIT && diag != CHOL_UNIT) return e.bad(-4, "diag");
  if (!A) return e.bad(-6, "NULL A");
  if (!B) return e.bad(-7, "NULL B");
  if (A == B || (A->mat && A->mat == B->mat)) return e.bad(-7, "B aliases A");
  return with_views({{A, false}, {B, true}}, [&]() -> int {
  if (int rc = half_args(e.what, A, 6, B, 7)) return rc;
  if (side == CHOL_RIGHT) return e.bad(CHOL_ERR_NOT_SUPPORTED, "ChamRight");
  if (diag == CHOL_UNIT)
    return e.bad(CHOL_ERR_NOT_SUPPORTED, "ChamUnit (a Cholesky factor has no unit diagonal)");
  const int up = uplo == CHOL_UPPER, tr_ = trans == CHOL_TRANS;
  tr_stats.clear();
  return timed(&tr_stats.v[0], [&] {
    return by_dtype(A->dtype, [&](auto t) { return trmm_impl<decltype(t)>(up, tr_, alpha, A, B, tr_stats.v); });
  });
  });
}

int chol_symm_tile(int side, int uplo, double alpha, chol_desc_t *A, chol_desc_t *B, double beta, chol_desc_t *C) {
  const Entry e{"symm_tile"};
  if (int rc = e.begin()) return rc;
  if (side != CHOL_LEFT && side != CHOL_RIGHT) return e.bad(-1, "side");
  if (int rc = e.uplo_at(uplo, 2)) return rc;
  if (!A) return e.bad(-4, "NULL A");
  if (!B) return e.bad(-5, "NULL B");
  if (!C) return e.bad(-7, "NULL C");
  if (C == A || C == B || (C->mat && (C->mat == A->mat || C->mat == B->mat))) return e.bad(-7, "C aliases A or B");
  return with_views({{A, false}, {B, false}, {C, true}}, [&]() -> int {
  int rc = inverse_check(e.what, A, 4);
  if (!rc) rc = symm_operand(A, B, 5, "B");
  if (!rc) rc = symm_operand(A, C, 7, "C");
  if (rc) return rc;
  if (C->ln != B->ln || C->mbi != B->mbi) return e.bad(-7, "C must have B's width");
  if (side == CHOL_RIGHT) return e.bad(CHOL_ERR_NOT_SUPPORTED, "ChamRight");
  sm_stats.clear();
  const int up = uplo == CHOL_UPPER;
  return timed(&sm_stats.v[0], [&] {
    return by_dtype(A->dtype, [&](auto t) { return symm_impl<decltype(t)>(up, alpha, A, B, beta, C, sm_stats.v); });
  });
  });
}

int chol_last_symm_stats(double *out8) { return sm_stats.read("symm", out8); }

int chol_logdet_tile(chol_desc_t *A, double *logdet) {
  const Entry e{"logdet_tile"};
  if (int rc = e.begin()) return rc;
  if (!A) return e.bad(-1, "NULL A");
  return with_views({{A, false}}, [&]() -> int {
  int rc = inverse_check(e.what, A, 1);
  if (rc) return rc;
  if (!logdet) return e.bad(-2, "NULL logdet");
  int info = 0;
  rc = by_dtype(A->dtype, [&](auto t) { return logdet_impl<decltype(t)>(A, logdet, &info); });
  return rc ? rc : info;
  });
}

int chol_last_trtrs_stats(double *out8) { return tr_stats.read("trtrs", out8); }

int chol_debug_half_limits(int trtrs_cols, int trmm_cols) {
  std::lock_guard<std::recursive_mutex> lk(ctx_mutex());  // (no with_views body)
  trtrs_kx = trtrs_cols < 0 ? TRTRS_KX : trtrs_cols;
  trmm_kx = trmm_cols < 0 ? TRMM_KX : trmm_cols;
  return 0;
}

int chol_sytrf_nopiv_tile(int uplo, chol_desc_t *A) {
  const Entry e{"sytrf_nopiv_tile"};
  if (int rc = e.begin(uplo)) return rc;
  if (!A) return e.bad(-2, "NULL A");
  return with_views({{A, true}}, [&]() -> int {
  if (int rc = inverse_check(e.what, A, 2)) return rc;
  CHECK_WINV(A, e.what);
  return sytrf_run(uplo, A);
  });
}

int chol_sytrs_nopiv_tile(int uplo, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"sytrs_nopiv_tile"};
  if (int rc = e.begin(uplo)) return rc;
  if (!A) return e.bad(-2, "NULL A");
  if (!B) return e.bad(-3, "NULL B");
  if (A == B || (A->mat && A->mat == B->mat)) return e.bad(-3, "B aliases A");
  return with_views({{A, false}, {B, true}}, [&]() -> int {
  int rc = inverse_check(e.what, A, 2);
  if (!rc) rc = resident_whole(e.what, B);
  if (rc) return rc;
  if (!same_rows(A, B)) return e.bad(-3, "B must have A's order, tile size and type");
  CHECK_WINV(A, e.what);
  const int up = uplo == CHOL_UPPER;
  return by_dtype(A->dtype, [&](auto t) { return sytrs_impl<decltype(t)>(up, A, B); });
  });
}

int chol_sysv_nopiv_tile(int uplo, chol_desc_t *A, chol_desc_t *B) {
  const Entry e{"sysv_nopiv_tile"};
  if (int rc = e.begin(uplo)) return rc;
  if (!A) return e.bad(-2, "NULL A");
  if (!B) return e.bad(-3, "NULL B");
  const int info = chol_sytrf_nopiv_tile(uplo, A);
  if (info != 0) return info;  // > 0: a zero or non-finite pivot, B untouched
  return chol_sytrs_nopiv_tile(uplo, A, B);
}

int chol_last_sytrf_stats(double *out8) { return sy_stats.read("sytrf", out8); }

int chol_rbt_apply_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth) {
  const Entry e{"rbt_apply_tile"};
  if (int rc = e.begin()) return rc;
  return with_views({{A, true}, {W, false}}, [&]() -> int {
  int rc = rbt_args(e.what, uplo, A, 2, W, 3, depth, 4);
  if (rc) return rc;
  if (A->lm == 0) return 0;
  forget_winv(A->mat);  // (A is overwritten)
  // (not lower_run: a failed wait after the second transpose returns before the launch check)
  rc = through_lower(uplo == CHOL_UPPER, {A}, [&] {
    by_dtype(A->dtype, [&](auto t) { rbt_transform<decltype(t)>(A, W, depth); });
    return 0;
  });
  if (rc) return rc;
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(main_stream()));
  return 0;
  });
}

int chol_sytrf_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth, unsigned long long seed) {
  const Entry e{"sytrf_rbt_tile"};
  if (int rc = e.begin()) return rc;
  return with_views({{A, true}, {W, true}}, [&]() -> int {
  int rc = rbt_args(e.what, uplo, A, 2, W, 3, depth, 4);
  if (rc) return rc;
  rb_stats.clear();
  if (A->lm == 0) return 0;  // (after the clear, before the timer starts)
  int info = 0;  // (a positive info is returned with the timer stopped)
  rc = timed(&rb_stats.v[RB_TOTAL], [&] {
    return by_dtype(A->dtype, [&](auto t) {
      return sytrf_rbt_impl<decltype(t)>(uplo, A, W, depth, seed, &info, rb_stats.v);
    });
  });
  return rc ? rc : info;
  });
}

int chol_sytrs_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth, chol_desc_t *B) {
  const Entry e{"sytrs_rbt_tile"};
  if (int rc = e.begin()) return rc;
  return with_views({{A, false}, {W, false}, {B, true}}, [&]() -> int {
  int rc = rbt_args(e.what, uplo, A, 2, W, 3, depth, 4);
  if (rc) return rc;
  if (!B) return e.bad(-5, "NULL B");
  if ((rc = resident_whole(e.what, B))) return rc;
  if (!same_rows(A, B) || B == A || B == W || B->mat == A->mat || B->mat == W->mat)
    return e.bad(-5, "B must be a descriptor of its own with A's order, tile size and type");
  rb_stats.clear();
  if (A->lm == 0) return 0;
  const int up = uplo == CHOL_UPPER;
  return timed(&rb_stats.v[RB_TOTAL], [&] {
    return by_dtype(A->dtype, [&](auto t) { return sytrs_rbt_impl<decltype(t)>(up, A, W, depth, B, rb_stats.v); });
  });
  });
}

int chol_sysv_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *W, int depth, unsigned long long seed,
                       chol_desc_t *B, chol_desc_t *X, int *iter, double *berr) {
  const Entry e{"sysv_rbt_tile"};
  if (int rc = e.begin()) return rc;
  return with_views({{A, false}, {AF, true}, {W, true}, {B, false}, {X, true}}, [&]() -> int {
  int rc = e.uplo_at(uplo, 1);
  if (rc) return rc;
  if (!A) return e.bad(-2, "NULL A");
  if ((rc = inverse_check(e.what, A, 2))) return rc;
  if (!AF) return e.bad(-3, "NULL AF");
  if ((rc = resident_whole(e.what, AF))) return rc;
  if (!same_geometry(A, AF) || AF == A || AF->mat == A->mat)
    return e.bad(-3, "AF must be a descriptor of its own with A's geometry and type");
  if ((rc = rbt_args(e.what, uplo, AF, 3, W, 4, depth, 5))) return rc;
  if (W->mat == A->mat) return e.bad(-4, "W aliases A");
  if (!B) return e.bad(-7, "NULL B");
  if ((rc = resident_whole(e.what, B))) return rc;
  if (!same_rows(A, B) || B->mat == A->mat || B->mat == AF->mat || B->mat == W->mat)
    return e.bad(-7, "B must be a descriptor of its own with A's order, tile size and type");
  if (!X) return e.bad(-8, "NULL X");
  if ((rc = resident_whole(e.what, X))) return rc;
  if (!same_geometry(B, X) || X == B || X->mat == B->mat || X->mat == A->mat || X->mat == AF->mat || X->mat == W->mat)
    return e.bad(-8, "X must be a descriptor of its own with B's shape, tile size and type");
  if (!iter) return e.bad(-9, "NULL iter");
  if (A->dtype != CHOL_REAL_DOUBLE)
    return e.bad(CHOL_ERR_NOT_SUPPORTED, "fp32 (the residual pass is fp64: use sytrf_rbt / sytrs_rbt)");
  rb_stats.clear();
  *iter = 0;
  if (A->lm == 0 || B->ln == 0) return 0;
  return sysv_rbt_impl(uplo, A, AF, W, depth, seed, B, X, iter, berr);
  });
}

int chol_last_rbt_stats(double *out8) { return rb_stats.read("rbt", out8); }
