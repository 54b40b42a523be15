/*
 * cholmi.h -- C ABI of libcholmi.so: the MI355X (gfx950) replacement for the
 * Chameleon calls on the reference's tiled-Cholesky path.
 *
 * Every entry point is `extern "C"`, takes plain ints / doubles / pointers, and
 * replaces exactly one call the reference makes into libchameleon.so.  Citations
 * are relative to /root/reference/ :
 *   W2 = cholesky_armonik/w_c_cons_v2/worker_construction2/src/worker_distrib.cpp
 *   C2 = cholesky_armonik/w_c_cons_v2/client_construction2/client/src/client_distrib.cpp
 *   V6 = Cholesky_chameleon_VM/cho/docker_installation_and_bench_files/v6_test.c
 *
 * Conventions
 *   - All tile operations are synchronous at this boundary (they return after
 *     the result is visible in the descriptor's memory), as Chameleon's
 *     non-_Async API is.
 *   - Return value: 0 on success; > 0 a LAPACK-style `info` (POTRF: 1-based
 *     global index of the first non-positive pivot); < 0 the negated 1-based
 *     position of the first invalid argument; <= -100 a runtime failure
 *     (CHOL_ERR_*).  The reference treats any value != 0 as failure
 *     (W2:243, 327, 420).
 *   - There is NO CPU backend.  chol_init(ncpu, 0) fails with CHOL_ERR_NO_GPU:
 *     the product path never falls back to host arithmetic.
 *   - Storage: a descriptor's `mat` may be NULL (the library allocates HBM in
 *     Chameleon tile layout, V6:44), a device pointer (wrapped in place, tiles
 *     stay resident) or a host pointer (W2:78: staged H2D/D2H around every
 *     call, which is what the reference's worker does with its blobs).
 *   - Tile layout (Chameleon descriptor): tile (I,J) of an lmt x lnt tile grid
 *     is `bsiz` contiguous elements at offset (I + J*lmt)*bsiz, column-major
 *     inside with leading dimension mb.  With p*q > 1 each process holds the
 *     tiles with (I mod p, J mod q) == its grid coordinates, packed the same
 *     way over local tile indices (I/p, J/q).
 */
#ifndef CHOLMI_H
#define CHOLMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Chameleon / PLASMA enum values (ChamRealDouble etc. are referenced at W2:78,
 * 238, 323, 416, 511; chameleon.h itself is not in the reference tree). */
enum {
  CHOL_REAL_FLOAT = 2,  /* ChamRealFloat  */
  CHOL_REAL_DOUBLE = 3, /* ChamRealDouble */
  CHOL_NOTRANS = 111,   /* ChamNoTrans */
  CHOL_TRANS = 112,     /* ChamTrans   */
  CHOL_UPPER = 121,     /* ChamUpper   */
  CHOL_LOWER = 122,     /* ChamLower   */
  CHOL_UPPER_LOWER = 123, /* ChamUpperLower (V6:51) */
  CHOL_NONUNIT = 131,   /* ChamNonUnit */
  CHOL_UNIT = 132,      /* ChamUnit    */
  CHOL_LEFT = 141,      /* ChamLeft    */
  CHOL_RIGHT = 142,     /* ChamRight   */
  CHOL_ONE_NORM = 171,       /* ChamOneNorm       */
  CHOL_FROBENIUS_NORM = 174, /* ChamFrobeniusNorm */
  CHOL_INF_NORM = 175,       /* ChamInfNorm (V6:74) */
  CHOL_MAX_NORM = 177        /* ChamMaxNorm       */
};

enum {
  CHOL_SUCCESS = 0,
  CHOL_ERR_NOT_INITIALIZED = -101,
  CHOL_ERR_NO_GPU = -102,        /* no HIP device / ngpu == 0 requested */
  CHOL_ERR_HIP = -103,           /* a HIP runtime call failed (see chol_last_error) */
  CHOL_ERR_NOT_SUPPORTED = -104, /* valid Chameleon usage this build does not cover */
  CHOL_ERR_OUT_OF_MEMORY = -105,
  CHOL_ERR_DEVICE_WAIT = -106    /* a bounded device-side wait inside the library gave up: the result is invalid */
};

typedef struct chol_desc chol_desc_t;

/* CHAMELEON_Init(ncpu, ngpu) W2:589, V6:41 / CHAMELEON_Finalize() V6:93.
 * Process-global and idempotent.  `ncpu` is accepted for signature parity and
 * ignored (host threads do no arithmetic); `ngpu` must be >= 1: this process
 * drives HIP device `chol_set_device`'s value (default: $LOCAL_RANK or 0). */
int chol_init(int ncpu, int ngpu);
int chol_finalize(void);
int chol_set_device(int device); /* call before chol_init */
const char *chol_last_error(void);
const char *chol_version(void);

/* One process per GPU: position of this process in the p x q grid that
 * descriptors with p*q > 1 refer to (Chameleon takes it from MPI).  rank =
 * prow*q + pcol, i.e. tile (I,J) belongs to rank (I mod p)*q + (J mod q). */
int chol_set_rank(int rank, int nranks);

/* CHAMELEON_Desc_Create(&d, mat, dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q)
 * W2:78 (1-tile wrap of a user buffer), V6:44 (mat = NULL: library-owned tile
 * storage) / CHAMELEON_Desc_Destroy W2:256, V6:90-91.
 * Sub-matrix views (i, j, m, n) != (0, 0, lm, ln), any offset: with mat = NULL the view is a matrix of its
 * own; over a user buffer (a matrix of whole mb = nb tiles) the library mirrors the view through a device
 * image around every operation -- entries outside the view are never touched. */
int chol_desc_create(chol_desc_t **desc, void *mat, int dtype, int mb, int nb, int bsiz, int lm,
                     int ln, int i, int j, int m, int n, int p, int q);
int chol_desc_destroy(chol_desc_t **desc);

/* Names the CONTENT behind a 1-tile descriptor's device buffer (the worker: a hash of the write-once result id
 * its blob belongs to; 0 = unnamed).  chol_potrf_tile on a tagged in-place device tile keeps the tile's block
 * inverses; chol_trsm_tile with an L of the same buffer AND tag reuses them instead of re-inverting L(k,k) for
 * every TRSM task of the wave (W2:323 is called once per panel tile with the same L). */
int chol_desc_set_version(chol_desc_t *desc, unsigned long long version);

/* CHAMELEON_dpotrf_Tile(uplo, A) W2:238, V6:56 (spotrf by descriptor dtype).
 * Works on a 1-tile descriptor (worker path), on a whole tiled matrix (driver path: the full wave
 * DAG of C2:506-565 runs on the device) and on a p x q block-cyclic descriptor (one process per GPU,
 * ChamLower; needs a transport, see chol_set_transport below).  ChamUpper is served for device-resident
 * matrices by transposing the storage in place around the Lower factorisation (the strict
 * lower triangle is returned untouched).
 * Returns LAPACK's info (0, or the 1-based index of the first non-positive pivot) or a negative CHOL_ERR_*;
 * CHOL_ERR_DEVICE_WAIT -- never expected -- says that a bounded device-side wait inside the library gave
 * up (the matrix is then left partly factored; the context falls back to stream events for later calls;
 * DESIGN.md, section 4). */
int chol_potrf_tile(int uplo, chol_desc_t *A);

/* CHAMELEON_dtrsm_Tile(side, uplo, trans, diag, alpha, A, B) W2:323.
 * Supported: (Right, Lower, Trans, NonUnit), any alpha; 1-tile descriptors. */
int chol_trsm_tile(int side, int uplo, int trans, int diag, double alpha, chol_desc_t *A,
                   chol_desc_t *B);

/* CHAMELEON_dsyrk_Tile(uplo, trans, alpha, A, beta, C) W2:416.
 * Supported: (Lower, NoTrans), any alpha/beta; the strict upper triangle of C
 * is never read or written. 1-tile descriptors. */
int chol_syrk_tile(int uplo, int trans, double alpha, chol_desc_t *A, double beta, chol_desc_t *C);

/* CHAMELEON_dgemm_Tile(transA, transB, alpha, A, B, beta, C) W2:511.
 * Supported: (NoTrans, Trans), any alpha/beta. 1-tile descriptors. */
int chol_gemm_tile(int transA, int transB, double alpha, chol_desc_t *A, chol_desc_t *B,
                   double beta, chol_desc_t *C);

/* The tasks of ONE op class of a wave in one grouped launch ("submit a whole wave, one wait per
 * wave"; W2:323 / 416 / 511 executed for n tasks at once), on HBM-resident mb x mb tiles (mb a multiple of 128):
 *   CHOL_BATCH_TRSM    c_out[t] = c_in[t] * a[t]^{-T}           (Right, Lower, Trans, NonUnit; a[t] = L(k,k))
 *   CHOL_BATCH_SYRK    c_out[t] = c_in[t] - a[t] a[t]^T, lower triangle (the strict upper triangle is copied)
 *   CHOL_BATCH_GEMM    c_out[t] = c_in[t] - a[t] b[t]^T
 *   CHOL_BATCH_UPDATE  the SYRK and GEMM tasks of a wave together: b[t] == NULL marks a SYRK task
 * c_in / a / b / c_out: HOST arrays of n device pointers (b ignored for TRSM / SYRK).  c_out[t] must not alias an
 * input: every task writes its private copy (W2:212-213) -- SYRK / GEMM / UPDATE in ONE out-of-place launch of the
 * trailing-update kernel (the copy IS the kernel's write: no copy pass), TRSM after a copy launch.  Results agree
 * with n calls of chol_trsm_tile / chol_syrk_tile / chol_gemm_tile to rounding (same products, same K order; the
 * kernels differ, so bit-identity is not promised).
 * a_versions (may be NULL): content tags of the a[t] buffers (chol_desc_set_version's meaning) -- TRSM reuses
 * the block inverses kept for (a[t], tag) by the POTRF batch instead of re-inverting L(k,k).
 * flags: CHOL_BATCH_ASYNC -- return once the work is enqueued (later batches are ordered behind it by what they
 *        read: see below; chol_sync() waits for everything).
 *        CHOL_BATCH_URGENT -- (SYRK / GEMM / UPDATE) the tasks feed the panel chain: column k+1 of wave k.
 * Execution is dependency-driven on two streams: POTRF and TRSM batches and URGENT updates run on a high-priority
 * chain stream, other updates on the bulk stream; a batch that reads a tile written by a batch of the other stream
 * waits for exactly that batch (tile pointers are the keys: results are write-once buffers).  So POTRF / TRSM of
 * wave k+1 run beside the bulk update of wave k, as in the whole-matrix walker, whenever the caller submits column
 * k+1's tasks URGENT and ahead of the rest (the reference's TaskOptions.priority, C2:335, is the natural carrier). */
enum { CHOL_BATCH_TRSM = 1, CHOL_BATCH_SYRK = 2, CHOL_BATCH_GEMM = 3, CHOL_BATCH_UPDATE = 4 };
enum { CHOL_BATCH_ASYNC = 1, CHOL_BATCH_URGENT = 2 };
int chol_tile_batch(int op, int dtype, int mb, int n, const void *const *c_in, const void *const *a,
                    const void *const *b, void *const *c_out, const unsigned long long *a_versions, int flags);
/* Waits for everything enqueued by the batch calls (both streams) and for the library's main stream. */
int chol_sync(void);
/* The POTRF tasks of a wave the same way: a_out[t] <- a_in[t] (private copy), factored Lower in place.  versions
 * (may be NULL) tags a_out[t]'s content, so that its block inverses serve the TRSM batch that follows.  The
 * LAPACK info of task t lands in a device slot: slots[t] (host array of n ints) receives its index, and
 * chol_batch_info(slot, &info) reads it (after waiting for the library's stream).  With CHOL_BATCH_ASYNC the call
 * returns at once: a failing factorisation is discovered when the caller asks. */
int chol_potrf_batch(int dtype, int mb, int n, const void *const *a_in, void *const *a_out,
                     const unsigned long long *versions, int *slots, int flags);
int chol_batch_info(int slot, int *info);
/* A mark = the batches enqueued so far (mark2: two sequence numbers, chain and bulk stream); chol_batch_wait blocks
 * until everything up to a mark has run WITHOUT draining what was enqueued after it -- what a client that releases
 * superseded tile versions needs: the readers of a version were all enqueued before the mark taken after them. */
int chol_batch_mark(unsigned long long *mark2);
int chol_batch_wait(const unsigned long long *mark2);
/* Executor statistics since chol_init: out4 = {batches on the chain stream, batches on the bulk stream, event waits
 * between the two, tile pointers currently remembered} (bench.py / tests: the overlap is really there). */
int chol_batch_stats(long long *out4);

/* CHAMELEON_dplgsy_Tile(bump, uplo, A, seed) V6:46: Chameleon's generator (published
 * core_dplgsy: 64-bit LCG with jump-ahead, entry (i,j), i >= j, = 0.5 - ran_{i + j*m} / 2^64,
 * symmetric, `bump` added to the diagonal), directly in tile layout on the device.  Values
 * depend only on (global row, global col, matrix order m, seed): independent of tile size
 * and process grid.  uplo = ChamLower / ChamUpper: the tiles on that side and the diagonal
 * tiles in full, the other tiles are left as they are (Chameleon's rule; library-allocated
 * storage starts at zero); ChamUpperLower: every tile. */
int chol_plgsy_tile(double bump, int uplo, chol_desc_t *A, unsigned long long seed);

/* The validation block of the reference driver, V6:51 and V6:72-86, on device-resident
 * single-process descriptors of identical geometry:
 *   CHAMELEON_dlacpy_Tile(uplo, A, B)            V6:51, 79   B <- A on the uplo part
 *   CHAMELEON_dlange_Tile(norm, A)               V6:74, 85   *value <- the norm
 *   CHAMELEON_dlauum_Tile(ChamLower, A)          V6:80       tril(A) <- tril(L^T L), L = tril(A)
 *   CHAMELEON_dgeadd_Tile(ChamNoTrans, a, A, b, B) V6:83     B <- a A + b B
 * (s-precision by descriptor dtype).  dlauum takes a scratch copy of the matrix.
 * dlange follows LAPACK DLANGE on non-finite entries, in all four norms: a NaN anywhere inside the m x n matrix
 * gives NaN; otherwise a +-Inf gives +Inf.  The stored padding outside the matrix is never read. */
int chol_lacpy_tile(int uplo, chol_desc_t *A, chol_desc_t *B);
int chol_lange_tile(int norm, chol_desc_t *A, double *value);
int chol_lauum_tile(int uplo, chol_desc_t *A);
int chol_geadd_tile(int trans, double alpha, chol_desc_t *A, double beta, chol_desc_t *B);

/* The step after the factor (not called by the reference):
 *   CHAMELEON_dpotrs_Tile(ChamLower, A, B)   B <- A^{-1} B with A = L L^T already factored
 *   CHAMELEON_dposv_Tile(ChamLower, A, B)    factor A, then solve; info > 0: A not SPD, B untouched
 * A: n x n, B: n x nrhs, device-resident single-process descriptors with the same tile size. */
int chol_potrs_tile(int uplo, chol_desc_t *A, chol_desc_t *B);
int chol_posv_tile(int uplo, chol_desc_t *A, chol_desc_t *B);

/* CHAMELEON_dsposv_Tile(uplo, A, B, X, &iter) -- LAPACK DSPOSV semantics on device-resident single-process
 * descriptors (the descriptor rules of chol_potrs_tile; A: n x n fp64, B and X: n x nrhs fp64, same tile size).
 * Factors an fp32 copy of A, solves in fp32 and refines X with fp64 residuals R = B - A X until every column
 * satisfies max|R(:,j)| <= max|X(:,j)| * anrm * eps * sqrt(n) (anrm = ||A||_inf, eps = 2^-53), at most 30 steps.
 * Only the `uplo` triangle of A is read; B is never written.  *iter on return:
 *   >= 0  refinement steps taken; A is unchanged
 *   -2    an entry of A, B or a residual does not fit in fp32
 *   -3    the fp32 factorisation reported info > 0
 *   -31   no convergence in 30 steps
 * On every negative *iter, X <- B and chol_posv_tile(uplo, A, X) run in fp64: A then holds the fp64 factor and the
 * return value is that factorisation's info (> 0: A is not SPD, X unspecified).
 * Argument errors return negative positions (A not fp64, B / X not matching A, X aliasing A or B, iter NULL). */
int chol_dsposv_tile(int uplo, chol_desc_t *A, chol_desc_t *B, chol_desc_t *X, int *iter);
/* Phases of the last chol_dsposv_tile [ms]: total, conversions + ||A||_inf, fp32 factor, fp32 solves (all),
 * residual passes (all), then the number of fp32 solves and of residual passes; out8[7] is 0. */
int chol_last_dsposv_stats(double *out8);

/* Inverse from the Cholesky factor, on device-resident single-process descriptors (the descriptor rules of
 * chol_potrs_tile: A square, stored tile edge a multiple of 64, views allowed; a p x q block-cyclic descriptor
 * returns CHOL_ERR_NOT_SUPPORTED).  fp64 or fp32 by A's dtype; only the `uplo` triangle of A is read or written,
 * the other strict triangle comes back bit-for-bit as it was.
 *
 * CHAMELEON_dtrtri_Tile(uplo, diag, A) -- LAPACK DTRTRI: A <- inv(A), A triangular, in place.  diag must be
 * CHOL_NONUNIT: a Cholesky factor never has a unit diagonal, so CHOL_UNIT returns CHOL_ERR_NOT_SUPPORTED.
 * Returns info = i > 0 (1-based) for the first exact zero A(i,i), found before anything is written: A is then
 * unchanged, as in LAPACK. */
int chol_trtri_tile(int uplo, int diag, chol_desc_t *A);
/* CHAMELEON_dpotri_Tile(uplo, A) -- LAPACK DPOTRI: A holds the factor L (or U) of chol_potrf_tile; the `uplo`
 * triangle of A becomes that of inv(L L^T) (inv(U^T U)).  info = i > 0 as chol_trtri_tile (A unchanged). */
int chol_potri_tile(int uplo, chol_desc_t *A);
/* CHAMELEON_dpoinv_Tile(uplo, A) -- Chameleon poinv: chol_potrf_tile followed by chol_potri_tile.  Returns potrf's
 * info > 0 when A is not positive definite, A then in the state potrf leaves it. */
int chol_poinv_tile(int uplo, chol_desc_t *A);

/* Condition estimate from the Cholesky factor, on device-resident single-process descriptors (the descriptor rules
 * of chol_potrs_tile: A square, stored tile edge a multiple of 64, views allowed; a p x q block-cyclic descriptor
 * returns CHOL_ERR_NOT_SUPPORTED).  fp64 or fp32 by A's dtype (the fp32 estimate runs in fp32, as LAPACK SPOCON);
 * A is only read, and only its `uplo` triangle.
 *
 * CHAMELEON_dlansy_Tile(norm, uplo, A) -- LAPACK DLANSY: *value <- the norm of the symmetric matrix whose `uplo`
 * triangle A stores.  CHOL_MAX_NORM, CHOL_ONE_NORM, CHOL_INF_NORM (equal to ONE, bit for bit) or
 * CHOL_FROBENIUS_NORM (the sum of squares in fp64, off-diagonal entries twice, then its square root, as
 * chol_lange_tile).  Sums run in a fixed order: a repeated call returns the same bits.  Non-finite entries as in
 * chol_lange_tile: a NaN inside the `uplo` triangle gives NaN in every norm, otherwise a +-Inf gives +Inf; the other
 * triangle is never read. */
int chol_lansy_tile(int norm, int uplo, chol_desc_t *A, double *value);
/* LAPACK DPOCON: A holds the factor of chol_potrf_tile(uplo, .); anorm = ||A_original||_1 (chol_lansy_tile).
 * *rcond <- 1 / (anorm * est(||A^{-1}||_1)), est from LAPACK DLACN2 (Higham's estimator, at most 11 applications of
 * A^{-1} = L^{-T} L^{-1}, each two triangular sweeps on one vector).  Argument errors: -1 uplo, -2 A, -3 anorm < 0
 * or NaN, -4 rcond NULL.  rcond = 0 for anorm = 0 or +Inf and for an exact zero on the factor's diagonal (found
 * before any sweep).  Unlike LAPACK, the sweeps do not rescale against overflow (no DLATRS): if a sweep produces a
 * non-finite value, rcond = 0.  Bit-identical from run to run. */
int chol_pocon_tile(int uplo, chol_desc_t *A, double anorm, double *rcond);
/* The last chol_pocon_tile: total ms, sweep ms (the applications alone), the number of applications, 0. */
int chol_last_pocon_stats(double *out4);

/* The SPD expert solve with error bounds (LAPACK DPOEQU, DLAQSY, DPORFS, DPOSVX), on device-resident single-process
 * descriptors with the rules of chol_pocon_tile (A square, stored tile edge a multiple of 64, views allowed; a p x q
 * block-cyclic descriptor returns CHOL_ERR_NOT_SUPPORTED).  fp64 or fp32 by A's dtype (fp32 follows LAPACK's
 * S-routines, in single precision throughout).  Only the `uplo` triangle of A and AF is read or written; the other
 * strict triangle comes back bit for bit as it was.  S is an n x 1 descriptor, B and X n x nrhs ones, all with A's
 * dtype and tile size.  No floating-point atomics and fixed summation orders: repeated calls give the same bits.
 * Argument errors return the negative position of the argument. */
enum {
  CHOL_FACT_NONE = 0,        /* 'N': factor A (a copy in AF)                            */
  CHOL_FACT_EQUILIBRATE = 1, /* 'E': equilibrate A if that helps, then factor it        */
  CHOL_FACT_FACTORED = 2     /* 'F': AF holds the factor; *equed and S are inputs      */
};
/* LAPACK DPOEQU: S <- 1/sqrt(A(i,i)) (IEEE, as LAPACK), *scond = sqrt(min A(i,i)) / sqrt(max A(i,i)),
 * *amax = max A(i,i).  Reads the diagonal only.  Returns info = i > 0 for the first A(i,i) <= 0 (S then unspecified). */
int chol_poequ_tile(chol_desc_t *A, chol_desc_t *S, double *scond, double *amax);
/* LAPACK DLAQSY: if scond < 0.1 or amax outside [small, large] (small = safmin / prec, large = 1 / small), the `uplo`
 * triangle of A <- (S(j) * S(i)) * A(i,j) in place and *equed = 1 ('Y'); else A untouched and *equed = 0 ('N'). */
int chol_laqsy_tile(int uplo, chol_desc_t *A, chol_desc_t *S, double scond, double amax, int *equed);
/* LAPACK DPORFS: A the matrix, AF its factor (chol_potrf_tile(uplo, .)), B the right-hand sides, X the solution,
 * refined in place (at most 5 steps per column; a column stops when berr <= eps or berr no longer halves).
 * ferr[nrhs] <- forward error bounds (DLACN2 on diag(W) A^-1, W = |R| + (n+1) eps (|A||X| + |B|)), berr[nrhs] <-
 * componentwise backward errors; host arrays.  A sweep that overflows (no DLATRS scaling) gives ferr = +Inf. */
int chol_porfs_tile(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *B, chol_desc_t *X, double *ferr,
                    double *berr);
/* LAPACK DPOSVX: equilibrate (CHOL_FACT_EQUILIBRATE), factor A into AF (NONE / EQUILIBRATE), rcond from lansy(One)
 * of the equilibrated A and pocon, X <- A^-1 B, porfs, then X <- diag(S) X and ferr /= scond when *equed = 1.  With
 * *equed = 1, A comes back equilibrated and B as diag(S) B.  CHOL_FACT_FACTORED takes A as already equilibrated, AF as
 * its factor and *equed / S as inputs (scond from S as DPOSVX: max(smin, safmin) / min(smax, 1 / safmin)); S may be
 * NULL when it is not used.  Returns 0; i in 1..n: the leading minor of order i is not positive definite (rcond = 0,
 * X, ferr, berr untouched); n + 1: rcond < eps (X, ferr and berr still computed).  Argument errors: -1 fact, -2 uplo,
 * -3 A, -4 AF, -5 equed, -6 S, -7 B, -8 X (or X aliasing A, AF or B), -9 rcond, -10 ferr, -11 berr NULL. */
int chol_posvx_tile(int fact, int uplo, chol_desc_t *A, chol_desc_t *AF, int *equed, chol_desc_t *S,
                    chol_desc_t *B, chol_desc_t *X, double *rcond, double *ferr, double *berr);
/* The last chol_posvx_tile / chol_porfs_tile: [0] total ms, [1] equilibration and the scaling of B, [2] lacpy + potrf,
 * [3] lansy + pocon, [4] the solve, [5] porfs (ms); [6] columns to which A^-1 was applied by the multi-vector sweeps,
 * [7] columns to which it was applied by potrs.  Phases a call did not run are 0. */
int chol_last_posvx_stats(double *out8);
/* The parts of chol_porfs_tile alone (scripts/posvx_time.py), on X's columns: path 0 the residual pass (B = X), 1 one
 * application of A^-1 by the multi-vector sweeps (groups of up to 8), 2 the same by potrs on an n x nrhs image.
 * AF holds the factor of A; X is only read.  *ms <- the fastest of `reps` calls after a warm-up one. */
int chol_bench_refine(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *X, int path, int reps, double *ms);

/* LAPACK DPSTRF: P^T A P = L L^T (Lower) or U^T U (Upper) with complete pivoting, stopping when the largest
 * remaining pivot is <= tol (tol < 0: n * eps * max_i A(i,i), eps = LAPACK's DLAMCH('Epsilon'), 2^-53 / 2^-24).
 * piv: HOST array of n ints, 1-based (LAPACK's PIV: column j of P is column piv[j] of the identity).
 * *rank: the number of pivots taken.  Returns 0 (rank = n), 1 (rank < n: semidefinite or rank deficient, as
 * LAPACK's INFO = 1) or a negative argument position / CHOL_ERR_*.
 *
 * Device-resident single-process descriptors that chol_potrf_tile factors (ragged orders, tile edges that are not
 * multiples of 128, sub-matrix views); a p x q block-cyclic descriptor returns CHOL_ERR_NOT_SUPPORTED.  fp64 or fp32
 * by A's dtype (fp32 runs in single precision throughout, as SPSTRF).  Only the `uplo` triangle is read or written:
 * the other strict triangle comes back bit for bit.  On return the first `rank` columns of the triangle hold L (Upper:
 * the first `rank` rows hold U = L^T), its rows in pivoted order, those of columns finished before a later pivot
 * included; with info = 1 columns rank+1 .. n are unspecified, as in LAPACK.  The largest diagonal entry <= 0 or NaN:
 * rank = 0, info = 1, A unchanged and piv the identity.  As in LAPACK the first pivot is taken whatever tol is; a
 * later step stops when its largest candidate is <= the stopping value or when any candidate is NaN (a NaN ranks
 * above every number).  Among equal candidates the smallest index wins (LAPACK's MAXLOC).  No floating-point atomics
 * and fixed reduction orders: a repeated call returns the same bits.  Argument errors: -1 uplo, -2 A, -3 piv NULL,
 * -4 rank NULL, -5 tol NaN. */
int chol_pstrf_tile(int uplo, chol_desc_t *A, int *piv, int *rank, double tol);
/* The last chol_pstrf_tile [ms]: total, pivot steps, row interchanges of the finished columns, trailing updates,
 * then the number of pivot steps; the rest 0. */
int chol_last_pstrf_stats(double *out8);

/* LAPACK DSYGST / SSYGST with itype 1: the generalized symmetric-definite eigenproblem A x = lambda B x reduced to
 * the standard form C y = lambda y.  B holds the Cholesky factor that chol_potrf_tile(uplo, B) returned.  Lower
 * (B = L L^T): the lower triangle of A becomes that of C = inv(L) A inv(L)^T.  Upper (B = U^T U): the upper triangle
 * of A becomes that of C = inv(U^T) A inv(U).  Only the `uplo` triangle of A is read or written: the other strict
 * triangle comes back bit for bit.  Only the `uplo` triangle of B is read, and all of B comes back bit for bit.
 * itype 2 and 3 (C = L^T A L) return CHOL_ERR_NOT_SUPPORTED.
 *
 * The descriptor rules of chol_trtri_tile: device-resident single-process square descriptors (ragged orders and
 * sub-matrix views included) whose stored tile edge is a multiple of 64, tiles up to 4096; a p x q block-cyclic
 * descriptor returns CHOL_ERR_NOT_SUPPORTED.  A and B of the same geometry and dtype; fp64 or fp32 by the dtype.
 * Deviation from LAPACK (which does not check): an exact zero on the diagonal of B returns its 1-based index
 * (info > 0) before anything is written, A unchanged.  No floating-point atomics and fixed reduction orders: a
 * repeated call returns the same bits.  Argument errors: -1 itype not in {1, 2, 3}, -2 uplo, -3 A, -4 B (NULL, a
 * dtype or geometry that differs from A's, or B aliasing A). */
int chol_sygst_tile(int itype, int uplo, chol_desc_t *A, chol_desc_t *B);
/* The last chol_sygst_tile [ms]: total, the inverses of B's diagonal tiles, the chain (diagonal tiles, panel TRSM,
 * the two SYMMs), the rank-2k updates, the deferred left solve; then the number of steps; the rest 0. */
int chol_last_sygst_stats(double *out8);

/* LINPACK DCHUD / DCHDD (MATLAB cholupdate) for r vectors at once: A holds the Cholesky factor that
 * chol_potrf_tile(uplo, A) returned, A = L L^T (Lower) or U^T U (Upper); on return it holds the factor of
 * L L^T + V V^T (chol_chud_tile) or of L L^T - V V^T (chol_chdd_tile), V an n x r descriptor, any r >= 0.  O(n^2 r)
 * operations and one read and one write of the stored triangle per 16 vectors, against the O(n^3) of a new
 * factorisation.  Only the `uplo` triangle of A is read or written: the other strict triangle (and the padding of a
 * ragged order) comes back bit for bit.  V IS WORKSPACE: it is overwritten and its content on return is unspecified.
 *
 * The arithmetic is fixed (sigma = +1 update, -1 downdate; columns j outer, vectors v inner):
 *     d2 = L_jj L_jj + sigma v_j v_j;   rr = sqrt(d2);   c = rr / L_jj;   s = v_j / L_jj;   ci = L_jj / rr;   L_jj = rr
 *     i > j:   L_ij = (L_ij + sigma s v_i) ci;   v_i = c v_i - s L_ij  (the new L_ij)
 * each sum of a product and a term one fused multiply-add.  No floating-point atomics and no reductions: a repeated
 * call returns the same bits, and the result does not depend on the tile size.
 *
 * The descriptor rules of chol_potrs_tile: device-resident single-process square A (ragged orders and sub-matrix
 * views included) whose stored tile edge is a multiple of 64; V with A's dtype, order and tile size; a p x q
 * block-cyclic descriptor returns CHOL_ERR_NOT_SUPPORTED.  fp64 or fp32 by the dtype, fp32 in single precision
 * throughout.  Cached block inverses of the old factor (chol_desc_set_version) are dropped.
 *
 * Returns 0, or j > 0 (1-based):
 *   - an exact zero at L_jj, found before anything is written: A and V unchanged;
 *   - the first column j, in the order above, at which some vector gives d2 <= 0 or NaN (for finite data only
 *     chol_chdd_tile can): the leading minor of order j of A - V V^T is not positive definite, chol_potrf_tile's
 *     meaning of info.  A and V are then unspecified, as A is after a failed chol_potrf_tile: a caller who needs the
 *     old factor keeps a copy (chol_lacpy_tile).
 * Argument errors: -1 uplo, -2 A, -3 V (NULL, another dtype, order or tile size, or V aliasing A). */
int chol_chud_tile(int uplo, chol_desc_t *A, chol_desc_t *V);
int chol_chdd_tile(int uplo, chol_desc_t *A, chol_desc_t *V);
/* The last chol_chud_tile / chol_chdd_tile: total, chain (the diagonal blocks' generators and the appliers inside
 * the diagonal tiles) and bulk applier time [ms]; r; the number of passes over the matrix (16 vectors each); the
 * 0-based index of the vector at which a downdate stopped (-1: none); the rest 0. */
int chol_last_chud_stats(double *out8);

/* LINPACK DCHEX without Z: A holds the Cholesky factor that chol_potrf_tile(uplo, A) returned, of a matrix M.  On
 * return it holds the factor of P^T M P, P the circular shift of the variables k..l (1-based, 1 <= k <= l <= n):
 *   job 1 (right shift): new order 1..k-1, l, k, k+1, .., l-1, l+1..n     (variable l moves up to position k)
 *   job 2 (left shift):  new order 1..k-1, k+1, .., l, k, l+1..n          (variable k moves down to position l)
 * O(n (l-k)) operations; only the columns <= l of the rows >= k are touched, one tile column at a time through a
 * staged copy (two buffers of a tile column each).  To delete variable k: job 2 with l = n, then the leading
 * (n-1) x (n-1) sub-matrix view holds the factor without it.
 *
 * The arithmetic is fixed (Lower form, L the old and L' the new factor; each a b + c one fused multiply-add):
 *   job 2: chol_chud_tile's rotations of ONE vector, sigma = +1, on the columns k..l-1 alone: the vector is
 *     v_i = L(i+1,k) (k <= i < l), v_l = L(k,k), v_i = L(i,k) (i > l); column j is the old column j+1 moved up by one
 *     row, W(i,j) = L(i+1,j+1) (j <= i < l), W(l,j) = 0, W(i,j) = L(i,j+1) (i > l); afterwards L'(i,l) = v_i, i >= l.
 *   job 1: y = L(l,l); for i = l-1 down to k: x = L(l,i), rho_i = sqrt(x x + y y), cc_i = y / rho_i,
 *     ss_i = x / rho_i, y = rho_i.  Every other old row r >= k, new row r' = r+1 (r < l) or r (r > l):
 *     b = L(r,l) (r > l) or +0; for i = min(r,l-1) down to k: a = L(r,i), L'(r',i+1) = cc_i a - (ss_i b),
 *     b = ss_i a + cc_i b; finally L'(r',k) = b.  L'(k,k) = rho_k.
 *   both: in the columns before k the rows k..l are permuted, every entry a bit-for-bit copy.
 * No floating-point atomics and no reductions: a repeated call returns the same bits, and the result does not depend
 * on the tile size.  Only the `uplo` triangle is read or written; the other strict triangle, the padding, the rows
 * before k and the columns after l are not written at all.
 *
 * chol_chud_tile's descriptor rules for A: device-resident single-process square A (ragged orders and sub-matrix views
 * included), stored tile edge a multiple of 64, fp64 or fp32 by the dtype; a p x q block-cyclic descriptor returns
 * CHOL_ERR_NOT_SUPPORTED.  Cached block inverses of the old factor (chol_desc_set_version) are dropped.
 *
 * Returns 0 (also for n = 0 or k = l, with nothing written), or j > 0 (1-based):
 *   - an exact zero at L_jj, found before anything is written: A unchanged;
 *   - the new column j that the first rotation with a squared pivot <= 0 or NaN would have written (non-finite data
 *     only).  A is then unspecified.
 * Argument errors: -1 uplo, -2 A, -3 k (outside 1..n), -4 l (outside k..n), -5 job. */
int chol_chex_tile(int uplo, chol_desc_t *A, int k, int l, int job);
/* The last chol_chex_tile: total, data movement (staging copies and plain moves), chain (job 2: chud's generators and
 * in-tile appliers; job 1: the coefficient chain) and bulk applier time [ms]; job; l - k; the rest 0. */
int chol_last_chex_stats(double *out8);

/* Batched Cholesky of small matrices: `batch` independent SPD matrices of order 0 <= n <= 64 (10^3 .. 10^6 of them is
 * the regime), without descriptors.  Matrix b is column-major at A + b strideA elements with leading dimension
 * lda >= max(1,n), strideA >= lda n; B likewise, n x nrhs, ldb >= max(1,n), strideB >= ldb nrhs.  A and B are device
 * pointers (a host pointer is an argument error); nothing beyond element alignment is assumed (lda may be odd, the
 * base may sit one element past a 16-byte boundary); every offset is computed in 64 bits.  fp64 or fp32 by dtype
 * (CHOL_REAL_DOUBLE / CHOL_REAL_FLOAT), fp32 in single precision throughout; CHOL_LOWER and CHOL_UPPER.  Only the
 * `uplo` triangle of each matrix is read or written: the other strict triangle, the lda - n rows under each column,
 * the gap between matrices, and the same places of B come back bit for bit and may hold NaN.  n > 64 returns
 * CHOL_ERR_NOT_SUPPORTED (chol_potrf_batch takes tiles that are multiples of 128, the descriptor routines any order).
 * Zero sizes (n, batch; nrhs for potrs) return 0 with nothing written on the device.
 *
 * The calls are synchronous and run on the library's main stream.  info: a host array of `batch` ints, or NULL;
 * info[b] is LAPACK's info of matrix b.  Returns 0 when every info[b] is 0, else b + 1 (1-based) of the first matrix
 * with info[b] > 0; negative: the position of a bad argument in the signature (lda, ldb or a stride too small, the
 * address ranges of A and B overlapping (B's position) included) or CHOL_ERR_*.  A failing matrix never disturbs
 * another one, also not one that shares its wavefront.
 *
 * potrf, the arithmetic fixed (uplo only says where L is stored, Upper holds U = L^T; each a b + c one fused
 * multiply-add, sqrt and the division correctly rounded):
 *   for j = 0..n-1:  s_i = A(i,j) (i >= j);  for k = 0..j-1 ascending: s_i = fma(-L(i,k), L(j,k), s_i);
 *     if !(s_j > 0): info = j+1, stop;  L(j,j) = sqrt(s_j);  r_j = 1 / L(j,j);  L(i,j) = s_i r_j (i > j).
 *   On info = j+1 the columns before j+1 hold the factor's, the rest of the triangle is as it was given.
 * potrs, B <- inv(L L^T) B from the factor, one column of B at a time and each on its own (r_j = 1 / L(j,j), P = 8,
 * 16, 32 or 64 the least of them >= n):
 *   forward   for j = 0..n-1:  y_j = b_j r_j;  b_i = fma(-L(i,j), y_j, b_i) (i > j)
 *   backward  for j = n-1..0:  t_i = L(i,j) x_i (j < i < n), +0 for the other i < P;
 *             for off = P/2, P/4, .., 1: t_i = t_i + t_(i xor off) (all i at once);  x_j = (y_j - t_j) r_j
 *   The order depends on n alone: not on uplo, nrhs, the matrix's place in the batch or its wavefront's other matrices.
 *   An exact zero on the stored diagonal gives info[b] = j (1-based, the first) and leaves that matrix's B untouched,
 *   as chol_trtrs_tile does.
 * posv: potrf then potrs in one pass, the factor never read back from memory; the same bits as the two calls.  With
 * info[b] > 0 that matrix's B is untouched.
 *
 * Argument positions: potrf 1 uplo, 2 dtype, 3 n, 4 A, 5 lda, 6 strideA, 7 batch; potrs and posv 1 uplo, 2 dtype, 3 n,
 * 4 nrhs, 5 A, 6 lda, 7 strideA, 8 B, 9 ldb, 10 strideB, 11 batch. */
int chol_potrf_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info);
int chol_potrs_batched(int uplo, int dtype, int n, int nrhs, const void *A, int lda, long long strideA, void *B,
                       int ldb, long long strideB, int batch, int *info);
int chol_posv_batched(int uplo, int dtype, int n, int nrhs, void *A, int lda, long long strideA, void *B, int ldb,
                      long long strideB, int batch, int *info);
/* The rank-r update and downdate of such factors (LINPACK DCHUD / DCHDD without Z and RHO, for r vectors): matrix b's
 * `uplo` triangle, as chol_potrf_batched(uplo, ..) left it, becomes the factor of L L^T + V V^T (chol_chud_batched) or
 * of L L^T - V V^T (chol_chdd_batched), V its n x r block of vectors.  The storage rules of chol_potrs_batched with V
 * in B's place: column-major at V + b strideV, ldv >= max(1,n), strideV >= ldv r; device pointers, fp64 or fp32, Lower
 * and Upper, element alignment alone, 64-bit offsets, 0 <= n <= 64 (n > 64: CHOL_ERR_NOT_SUPPORTED; chol_chud_tile and
 * chol_chdd_tile take any order).  Zero sizes (n, r, batch) return 0 with nothing written on the device.
 *
 * The arithmetic is chol_chud_tile's block above, each a b + c one fused multiply-add; for every matrix with info 0
 * the bits are those chol_chud_tile / chol_chdd_tile return for the same L and V.  They depend neither on uplo, the
 * layout, the matrix's place in the batch or its wavefront's other matrices, nor on how the vectors are grouped into
 * calls: r vectors in one call give the bits of r calls with one vector each.
 *
 * V IS ONLY READ (unlike the tile routine's workspace) and comes back bit for bit.  Only the `uplo` triangle of A is
 * read or written; the other strict triangle, the lda - n rows under a column, the gaps between the matrices and V's
 * padding come back bit for bit and may hold NaN.
 *
 * info[b] (a host array of `batch` ints, or NULL): 0; or j (1-based) of the first exact zero L_jj, found before any
 * rotation and ahead of everything else; or the first column j, columns outer and vectors inner, at which some vector
 * gives d2 <= 0 or NaN (a NaN or Inf in V or on the diagonal ends here): the leading minor of order j of
 * L L^T - V V^T is not positive definite.  Whenever info[b] > 0 matrix b's A IS UNTOUCHED, bit for bit (stronger than
 * the tile routine), and no other matrix is disturbed.  Returns 0, or b + 1 of the first matrix with info[b] > 0;
 * negative: the position of a bad argument (a host pointer, lda, ldv or a stride too small, the address ranges of A
 * and V overlapping (V's position) included) or CHOL_ERR_*.
 *
 * Z and RHO of LINPACK (a recursive least-squares step): border the matrix with the right-hand side,
 * [A b; b^T c], order n + 1 <= 64, and update its factor with (x, y): the last row of the factor is z^T and rho.
 *
 * Argument positions: 1 uplo, 2 dtype, 3 n, 4 r, 5 A, 6 lda, 7 strideA, 8 V, 9 ldv, 10 strideV, 11 batch. */
int chol_chud_batched(int uplo, int dtype, int n, int r, void *A, int lda, long long strideA, const void *V, int ldv,
                      long long strideV, int batch, int *info);
int chol_chdd_batched(int uplo, int dtype, int n, int r, void *A, int lda, long long strideA, const void *V, int ldv,
                      long long strideV, int batch, int *info);
/* One half of such a factor alone (what chol_trtrs_tile, chol_trmm_tile and chol_logdet_tile are to the tiled side):
 * B <- inv(op(T)) B (chol_trtrs_batched), B <- alpha op(T) B (chol_trmm_batched) and log det(L L^T)
 * (chol_logdet_batched).  The storage rules are chol_potrs_batched's: column-major images at a fixed stride,
 * lda >= max(1,n), strideA >= lda n, B likewise (n x nrhs, ldb >= max(1,n), strideB >= ldb nrhs); device pointers
 * only; element alignment alone; 64-bit offsets; 0 <= n <= 64 (n > 64: CHOL_ERR_NOT_SUPPORTED; chol_trtrs_tile,
 * chol_trmm_tile and chol_logdet_tile take any order); fp64 or fp32 by dtype, fp32 in single precision throughout;
 * zero sizes (n, nrhs, batch) return 0 with nothing written on the device (but see logdet for n = 0); overlapping
 * address ranges of A and B are an argument error at B's position; synchronous, on the library's main stream.
 *
 * T is the `uplo` triangle of each image, op(T) = T (CHOL_NOTRANS) or T^T (CHOL_TRANS): all four combinations.  uplo
 * only chooses the loads: L below is the lower factor however it is stored (Upper holds U = L^T), so (Lower, NoTrans)
 * and (Upper, Trans) are the FORWARD half, op(T) = L, and (Lower, Trans) and (Upper, NoTrans) the BACKWARD half,
 * op(T) = L^T.  A IS ONLY READ: the whole buffer comes back bit for bit; the other strict triangle, the lda - n rows
 * under a column and the gaps may hold NaN and none of it reaches B.  Of B only the n x nrhs entries are written.
 *
 * The arithmetic, fixed (each a b + c one fused multiply-add; r_j = 1 / L(j,j); P = 8, 16, 32 or 64, the least of them
 * >= n; one column of B at a time and each on its own):
 *   trtrs forward   for j = 0..n-1:  y_j = b_j r_j;  b_i = fma(-L(i,j), y_j, b_i) (i > j)
 *   trtrs backward  for j = n-1..0:  t_i = L(i,j) x_i (j < i < n), +0 for the other i < P;
 *                   for off = P/2, P/4, .., 1: t_i = t_i + t_(i xor off) (all i at once);  x_j = (b_j - t_j) r_j
 *     These are the two halves of chol_potrs_batched: the forward call followed by the backward call on the same B
 *     returns its bits.  An exact zero on the stored diagonal gives info[b] = j (1-based, the first): that matrix's B
 *     is untouched and no other matrix is disturbed, also not one that shares its wavefront.  info is a host array of
 *     `batch` ints or NULL; the return value is 0, or b + 1 of the first such matrix.
 *   trmm forward    s_i = +0;  for k = 0..i ascending: s_i = fma(L(i,k), z_k, s_i);  B(i) = alpha s_i
 *   trmm backward   for j = n-1..0:  t_i = L(i,j) z_i (j <= i < n), +0 for the other i < P;  the same butterfly;
 *                   B(j) = alpha t_j
 *     The terms outside the triangle are left out, not multiplied by a stored zero: a NaN in z_k reaches the rows
 *     i >= k (forward) or i <= k (backward) and no other.  alpha is rounded to the dtype; with alpha == 0 neither A nor
 *     B is read and B <- +0, as BLAS does (a NaN in B does not survive).  A zero on the diagonal is no failure: trmm
 *     has no info and returns 0.
 *   logdet          only the diagonal is read, so there is no uplo.  `logdet` is a DEVICE array of `batch` doubles
 *     for both dtypes (a host pointer is an argument error):
 *     logdet[b] = 2 (((log d_0 + log d_1) + log d_2) + ..), d_j = L(j,j) converted to fp64, the device's fp64 log, a
 *     plain ascending chain.  info[b] = j (1-based) for the first d_j <= 0 or NaN, and logdet[b] is then NaN; the
 *     return value is 0, or b + 1 of the first such matrix.  n = 0 gives logdet[b] = 0 (the one write of a zero size).
 * For every routine the bits depend on n and that matrix's data alone: not on uplo, the layout, nrhs, the matrix's
 * place in the batch, its wavefront's other matrices, or whether the call is repeated.
 *
 * Argument positions: trtrs 1 uplo, 2 trans, 3 dtype, 4 n, 5 nrhs, 6 A, 7 lda, 8 strideA, 9 B, 10 ldb, 11 strideB,
 * 12 batch; trmm 1 uplo, 2 trans, 3 dtype, 4 n, 5 nrhs, 6 alpha, 7 A, 8 lda, 9 strideA, 10 B, 11 ldb, 12 strideB,
 * 13 batch; logdet 1 dtype, 2 n, 3 A, 4 lda, 5 strideA, 6 batch, 7 logdet. */
int chol_trtrs_batched(int uplo, int trans, int dtype, int n, int nrhs, const void *A, int lda, long long strideA,
                       void *B, int ldb, long long strideB, int batch, int *info);
int chol_trmm_batched(int uplo, int trans, int dtype, int n, int nrhs, double alpha, const void *A, int lda,
                      long long strideA, void *B, int ldb, long long strideB, int batch);
int chol_logdet_batched(int dtype, int n, const void *A, int lda, long long strideA, int batch, double *logdet,
                        int *info);
/* The explicit inverses of such factors (what chol_trtri_tile, chol_potri_tile and chol_poinv_tile are to the tiled
 * side), in place: the stored triangle T becomes inv(T) (chol_trtri_batched), the triangle of inv(L L^T)
 * (chol_potri_batched), or the `uplo` triangle of an SPD matrix becomes that of its inverse (chol_poinv_batched);
 * chol_invdiag_batched returns the diagonal of inv(L L^T) alone (marginal variances, leave-one-out residuals).  The
 * storage and argument rules are chol_potrf_batched's: column-major images at a fixed stride, lda >= max(1,n),
 * strideA >= lda n; device pointers only; element alignment alone; 64-bit offsets; 0 <= n <= 64 (n > 64:
 * CHOL_ERR_NOT_SUPPORTED; chol_trtri_tile, chol_potri_tile and chol_poinv_tile take any order); fp64 or fp32 by dtype,
 * fp32 in single precision throughout; Lower and Upper; zero sizes (n, batch) return 0 with nothing written on the
 * device; synchronous, on the library's main stream.  Only the `uplo` triangle is read or written: the other strict
 * triangle, the lda - n rows under a column and the gaps come back bit for bit and may hold NaN.
 * invdiag: A IS ONLY READ; D + b strideD receives the n diagonal entries of matrix b's inverse in A's dtype,
 * strideD >= n, a device pointer; the address ranges of A and D overlapping are an argument error at D's position.
 *
 * The arithmetic, fixed (L the lower factor however it is stored, Upper holds U = L^T; r_j = 1 / L(j,j); each a b + c
 * one fused multiply-add; W = inv(L)):
 *   trtri  column c of W on its own:  b_c = 1, b_i = +0 (i > c);
 *          for j = c..n-1 ascending:  W(j,c) = b_j r_j;  b_i = fma(-L(i,j), W(j,c), b_i) (i > j)
 *          Lower receives W, Upper inv(U) = W^T.  This is the forward sweep of chol_trtrs_batched applied to e_c and
 *          started at step c: for a finite factor the bits are those of the lower triangle of trtrs_batched(F, I).
 *   potri  X(i,m), i >= m:  s = +0;  for k = i..n-1 ascending:  s = fma(W(k,i), W(k,m), s)
 *          X = W^T W = inv(L L^T); Lower receives its lower triangle, Upper the upper one (the same bits, mirrored).
 *   poinv  potrf (the chain of chol_potrf_batched) then potri in one pass, the factor never stored: the bits of the
 *          two calls.
 *   invdiag  D(i) = X(i,i) of potri, bit for bit.
 *   The terms outside an entry's sum are left out, not multiplied by a stored zero: a NaN at L(p,q) reaches exactly
 *   the entries W(k,c) with c <= q and k >= p, and of X the entries X(i,m) with m <= q; every other entry keeps its
 *   bits.  The order depends on n and that matrix's data alone: not on uplo, the layout, the matrix's place in the
 *   batch, its wavefront's other matrices, or whether the call is repeated.
 *
 * info (a host array of `batch` ints, or NULL).  trtri, potri, invdiag: info[b] = j (1-based) is the first exact zero
 * on the stored diagonal; that matrix's A (invdiag: D) is then untouched, as chol_trtri_tile and chol_trtrs_batched
 * leave it.  poinv: potrf's info, and that matrix is left as chol_potrf_batched leaves it (the columns before the
 * failing one hold the factor's, the rest is as it was given).  A failing matrix never disturbs another one, also not
 * one that shares its wavefront.  Returns 0, or b + 1 of the first matrix with info[b] > 0; negative: the position of
 * a bad argument or CHOL_ERR_*.
 *
 * Argument positions: trtri, potri and poinv 1 uplo, 2 dtype, 3 n, 4 A, 5 lda, 6 strideA, 7 batch; invdiag 1 uplo,
 * 2 dtype, 3 n, 4 A, 5 lda, 6 strideA, 7 D, 8 strideD, 9 batch. */
int chol_trtri_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info);
int chol_potri_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info);
int chol_poinv_batched(int uplo, int dtype, int n, void *A, int lda, long long strideA, int batch, int *info);
int chol_invdiag_batched(int uplo, int dtype, int n, const void *A, int lda, long long strideA, void *D,
                         long long strideD, int batch, int *info);
/* The last batched call: total time and kernel time [ms] (the library's own events); batch; n; matrices per wavefront;
 * workgroups launched; the bytes the algorithm must move (the stored triangles read and written, plus B read and
 * written; chud and chdd: the triangles read and written, plus V read; trtrs and trmm: the triangle read, plus B read
 * and written -- B written alone with alpha == 0; logdet: n diagonal elements read and 8 bytes written; trtri, potri
 * and poinv: the triangles read and written; invdiag: the triangles read and n elements written); 0. */
int chol_last_batched_stats(double *out8);

/* One half of a Cholesky factor alone: the triangular solve, the triangular product and the log-determinant, on
 * device-resident single-process descriptors with the rules of chol_potrs_tile: A square (ragged orders and
 * sub-matrix views included), stored tile edge a multiple of 64; B n x nrhs with A's dtype, order and tile size, any
 * nrhs >= 0; a p x q block-cyclic descriptor returns CHOL_ERR_NOT_SUPPORTED.  fp64 or fp32 by the dtype, fp32 in
 * single precision throughout.  T is the `uplo` triangle of A (what chol_potrf_tile(uplo, .) returned), op(T) = T
 * (CHOL_NOTRANS) or T^T (CHOL_TRANS): all four combinations.  diag must be CHOL_NONUNIT: CHOL_UNIT returns
 * CHOL_ERR_NOT_SUPPORTED, as chol_trtri_tile.  A IS ONLY READ and comes back bit for bit, all of it; the other strict
 * triangle may hold anything, NaN included, and does not reach B.  No floating-point atomics and fixed summation
 * orders: a repeated call returns the same bits.
 *
 * CHAMELEON_dtrtrs_Tile(uplo, trans, diag, A, B) -- LAPACK DTRTRS: B <- inv(op(T)) B.  (Lower, NoTrans) and (Upper,
 * Trans) are the forward half of chol_potrs_tile, (Lower, Trans) and (Upper, NoTrans) its backward half: x = L^-T y
 * takes the eigenvectors of chol_sygst_tile's standard problem back to the generalized one, |L^-1 y|^2 is the
 * quadratic form of a Gaussian likelihood, L^-1 B whitens.  Up to 40 columns run as one pass of the narrow sweeps of
 * chol_pocon_tile / chol_porfs_tile over the stored triangle, 8 columns at a time (a column's result does not depend
 * on which columns share its pass); more columns run as one sweep of chol_potrs_tile's.  Returns info = i > 0
 * (1-based) for the first exact zero T(i,i), found before B is written (B unchanged), as LAPACK.
 * Argument errors: -1 uplo, -2 trans, -3 diag, -4 A, -5 B (NULL, another dtype, order or tile size, or B aliasing A). */
int chol_trtrs_tile(int uplo, int trans, int diag, chol_desc_t *A, chol_desc_t *B);
/* CHAMELEON_dtrmm_Tile(side, uplo, trans, diag, alpha, A, B) -- BLAS DTRMM: B <- alpha op(T) B, in place (x = L z is
 * a sample with covariance L L^T).  side must be CHOL_LEFT: CHOL_RIGHT returns CHOL_ERR_NOT_SUPPORTED.  Up to 40
 * columns run 8 at a time, each pass reading the stored triangle once; more columns run as products of whole tiles.
 * Argument errors (chol_trsm_tile's positions): -1 side, -2 uplo, -3 trans, -4 diag, -6 A, -7 B (as above). */
int chol_trmm_tile(int side, int uplo, int trans, int diag, double alpha, chol_desc_t *A, chol_desc_t *B);
/* *logdet <- 2 sum_j log A(j,j): log det(L L^T) from the diagonal of the factor, which alone is read (either uplo).
 * Logs and the sum in fp64 for both dtypes, as chol_lansy_tile's Frobenius sum, in a fixed order.  n = 0 gives 0.
 * Returns info = j > 0 for the first A(j,j) that is <= 0 or NaN (*logdet is unspecified then).
 * Argument errors: -1 A, -2 logdet NULL. */
int chol_logdet_tile(chol_desc_t *A, double *logdet);
/* The last chol_trtrs_tile / chol_trmm_tile: total, staging of the diagonal tiles, sweeps or products [ms]; the
 * columns that went through the narrow path, those that went through the wide path; the rest 0. */
int chol_last_trtrs_stats(double *out8);
/* Diagnostic (scripts/trtrs_time.py measures the crossovers with it): the widest chol_trtrs_tile / chol_trmm_tile call
 * that takes the narrow path; a negative value restores the built-in limit (40). */
int chol_debug_half_limits(int trtrs_cols, int trmm_cols);

/* The symmetric matrix product from one stored triangle: CHAMELEON_dsymm_Tile(side, uplo, alpha, A, B, beta, C) --
 * BLAS DSYMM / SSYMM: C <- alpha A B + beta C.  A is n x n symmetric and only its `uplo` triangle is read: the other
 * strict triangle may hold anything, NaN included, and does not reach C.  B and C are n x nrhs with A's dtype, order
 * and tile size (chol_trmm_tile's rule for its B), any nrhs >= 1, also across several tile columns.  Device-resident
 * single-process descriptors; ragged orders, tile edges that are no multiple of 128 and sub-matrix views (C writable)
 * are served; a p x q block-cyclic descriptor returns CHOL_ERR_NOT_SUPPORTED.  side must be CHOL_LEFT: CHOL_RIGHT
 * returns CHOL_ERR_NOT_SUPPORTED.  fp64 or fp32 by the dtype; fp32 runs in single precision throughout, alpha and beta
 * rounded to float.
 * A and B ARE ONLY READ: their stored images come back bit for bit, padding and the unreferenced triangle included.  B
 * may be A itself; C must not alias A or B.  Of C only the entries of the matrix are written, its padding comes back
 * bit for bit.
 * The scalars follow BLAS: with beta == 0 C is not read (a NaN in C does not survive); with alpha == 0 A and B are not
 * read and C <- beta C (C <- 0 when beta == 0 too).
 * Arithmetic: one lane forms s = sum_k A(i,k) B(k,j) over k = 0 .. n-1 in ascending steps of four on the 16x16x4 MFMA,
 * in the same order whatever nrhs is and whichever columns share its workgroup, then stores
 *     C(i,j) <- fma(alpha, s, beta * C(i,j))      (beta != 0)        C(i,j) <- alpha * s      (beta == 0)
 * and, with alpha == 0, C(i,j) <- beta * C(i,j) or 0.  No floating-point atomics, no partial sums: a repeated call
 * returns the same bits, and a column's result depends neither on nrhs nor on its neighbours.
 * One kernel serves every nrhs: a workgroup owns 128 rows of C and 16, 32, 64 or 128 columns (the smallest of these
 * that holds nrhs, else 128) and reads its block row of A once, so the whole of A is read once per block of columns:
 * twice the stored triangle, where the residual pass inside chol_dsposv_tile / chol_porfs_tile reads the triangle once
 * per 8 columns.  Measured at N=65536 / 1024 and 16384 / 512, fp64: that pass is faster at one column (0.81 /
 * 0.35 of this routine's time), this routine from 8 columns on (4.5 x / 1.7 x at 8, 12 x at 128 and 1024): the crossover
 * lies between 1 and 8 columns.
 * Argument errors (Chameleon's positions): -1 side, -2 uplo, -4 A (NULL or not square), -5 B (NULL, another dtype,
 * order or tile size), -7 C (as B, a width that differs from B's, or C aliasing A or B). */
int chol_symm_tile(int side, int uplo, double alpha, chol_desc_t *A, chol_desc_t *B, double beta, chol_desc_t *C);
/* The last chol_symm_tile: total, kernel [ms] (the library's own events), nrhs, the column width of a workgroup's
 * block (0 when alpha == 0), the number of workgroups, 2 n^2 nrhs; the rest 0. */
int chol_last_symm_stats(double *out8);

/* The L D L^T factorisation WITHOUT pivoting of a symmetric matrix (MAGMA dsytrf_nopiv / ssytrf_nopiv; LAPACK
 * DSYTF2's storage for 1 x 1 pivots): A = L D L^T (Lower) or U^T D U (Upper, U = L^T), L unit lower triangular, D
 * diagonal.  On return the diagonal of A holds D and the strict `uplo` triangle holds L (U); the unit diagonal is not
 * stored.  Only the `uplo` triangle is read or written: the other strict triangle comes back bit for bit.  For
 * matrices whose factorisation needs no pivoting: symmetric quasi-definite [[H, J^T], [J, -C]] with H and C positive
 * definite (under any symmetric permutation), symmetric diagonally dominant with diagonal entries of either sign,
 * shifted matrices C - sigma I whose inertia is wanted.  Nothing bounds the growth of L on other matrices:
 * chol_last_sytrf_stats reports min |d|, max |d| and max |L| so that a caller can judge the run.
 *
 * A column of L is its unscaled column times the reciprocal of the pivot, l(i,j) = w(i,j) * (1 / d_j), the
 * reciprocal formed once per pivot (DSYTF2's r1 = 1 / d), not a division per entry.
 *
 * Returns 0, or j > 0: the 1-based index of the first pivot d_j that is exactly zero or not finite (NaN, +-Inf); then
 * the tile columns before the one that holds j are final and the rest of the triangle is unspecified (LAPACK leaves a
 * partly factored matrix in the same way).  A negative pivot is NOT an error.
 *
 * The descriptor rules of chol_sygst_tile: device-resident single-process square descriptors (ragged orders and
 * sub-matrix views included), tiles up to 4096, the stored tile edge a multiple of 128 (what chol_desc_create
 * allocates; a caller's buffer with another edge returns CHOL_ERR_NOT_SUPPORTED); a p x q block-cyclic descriptor
 * returns CHOL_ERR_NOT_SUPPORTED.  fp64 or fp32 by the dtype, fp32 in single precision throughout.  No floating-point
 * atomics and fixed reduction orders: a repeated call returns the same bits.  Argument errors: -1 uplo, -2 A. */
int chol_sytrf_nopiv_tile(int uplo, chol_desc_t *A);
/* B <- inv(A) B from the factor chol_sytrf_nopiv_tile(uplo, A) returned: L Y = B, Z = D^{-1} Y (a multiplication by
 * 1 / d_j), L^T X = Z.  Any number of right-hand sides; B with A's order, row tiling and dtype (the rules of
 * chol_potrs_tile).  A is only read and comes back bit for bit.  A zero on the stored diagonal returns its 1-based
 * index (info > 0) before B is written.  Argument errors: -1 uplo, -2 A, -3 B (NULL, another order, tile size or
 * dtype than A's, or B aliasing A). */
int chol_sytrs_nopiv_tile(int uplo, chol_desc_t *A, chol_desc_t *B);
/* chol_sytrf_nopiv_tile then chol_sytrs_nopiv_tile; with info > 0 from the factorisation B is not touched. */
int chol_sysv_nopiv_tile(int uplo, chol_desc_t *A, chol_desc_t *B);
/* The last chol_sytrf_nopiv_tile: total, chain (diagonal tiles, panel TRSM, scaling) and trailing-update time [ms];
 * the number of positive and of negative pivots (the inertia; by Sylvester's law the number of positive and negative
 * eigenvalues), min |d_j|, max |d_j|, max |L(i,j)| over the strict triangle -- over rows and columns 0 .. n-1 only:
 * the identity padding of a ragged order is not counted.  From fixed-order reductions. */
int chol_last_sytrf_stats(double *out8);

/* The butterfly-randomised solve of a general symmetric INDEFINITE system (Baboulin, Becker, Dongarra, IPDPS 2012;
 * MAGMA's *_rbt routines): A_r = W^T A W with a random recursive butterfly W, then A_r = L D L^T WITHOUT pivoting (the
 * routine above), A^{-1} = W (L D L^T)^{-1} W^T, and in chol_sysv_rbt_tile iterative refinement against the original A.
 * For the matrices on which chol_sytrf_nopiv_tile stops or loses accuracy: a zero diagonal, a saddle point with a
 * zero block, a shift next to an eigenvalue of a leading block.  The randomisation makes a zero or tiny pivot
 * improbable; it does not bound the growth, so chol_sysv_rbt_tile refines and returns the backward error it reached.
 *
 * A butterfly of order m = 2h is 2^(-1/2) [[R0, R1], [R0, -R1]], R0 and R1 diagonal of order h.  W = D_(depth-1) ...
 * D_0: D_0 one butterfly of order n, D_k block diagonal with 2^k butterflies of order n / 2^k.  W is an n x depth (or
 * wider) descriptor with A's dtype and tile size: column k holds the diagonal entries of level k in row order (rows o
 * .. o+h-1 of a butterfly over the rows o .. o+2h-1 hold R0, the next h hold R1).  seed != 0: the library fills W with
 * exp(r / 10), r uniform in [-1/2, 1/2] from the 64-bit generator of chol_plgsy_tile run on the host, so that (n,
 * depth, seed, dtype) gives the same W everywhere.  seed == 0: W is an input.
 *
 * depth is 1 or 2.  n MUST be a multiple of 2^depth (CHOL_ERR_NOT_SUPPORTED otherwise): border A with a row and column
 * of the identity; the library does not pad.  The other descriptor rules are chol_sytrf_nopiv_tile's (device-resident,
 * single process, sub-matrix views allowed, stored tile edge a multiple of 128; p x q: CHOL_ERR_NOT_SUPPORTED).  Only
 * the `uplo` triangle is read or written; the other strict triangle and all padding come back bit for bit.  Fixed
 * formulas and no reductions in the transformation: a repeated call returns the same bits.
 *
 * chol_rbt_apply_tile: A <- W^T A W alone (W is read).  Argument errors: -1 uplo, -2 A, -3 W, -4 depth. */
int chol_rbt_apply_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth);
/* W filled (seed != 0), A <- W^T A W, then the factorisation of chol_sytrf_nopiv_tile.  Returns what that returns: 0,
 * or the 1-based index of the first zero or non-finite pivot of A_r.  chol_last_sytrf_stats reports the growth and
 * the inertia (that of A, by Sylvester's law).  Argument errors: -1 uplo, -2 A, -3 W, -4 depth. */
int chol_sytrf_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth, unsigned long long seed);
/* B <- W (L D L^T)^{-1} W^T B from what chol_sytrf_rbt_tile left in A and W; both are only read.  A zero on the stored
 * diagonal returns its index (info > 0) before B is written.  Argument errors: -1 uplo, -2 A, -3 W, -4 depth, -5 B. */
int chol_sytrs_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *W, int depth, chol_desc_t *B);
/* A X = B: AF <- the `uplo` triangle of A, chol_sytrf_rbt_tile on AF, X <- the solve of B, then refinement in fp64
 * against the untouched A: R = B - A X from the stored triangle, X += W (L D L^T)^{-1} W^T R, until every column has
 * max |R(:,j)| <= max |X(:,j)| ||A||_inf eps sqrt(n) (LAPACK DSPOSV's criterion, eps = 2^-53), at most 10 steps.  A and
 * B are only read.  *iter: the steps taken; -3: the factorisation stopped (the return value is its info, X untouched);
 * -31: no convergence in 10 steps (the return value is n + 1, X holds the last iterate).  berr (nrhs host doubles,
 * may be NULL): the final max |R(:,j)| / (||A||_inf max |X(:,j)|) of every column; a column of X that is all zeros
 * gives 0 when its residual is zero too and +Inf otherwise.  fp64 only: an fp32 A returns
 * CHOL_ERR_NOT_SUPPORTED (chol_sytrf_rbt_tile / chol_sytrs_rbt_tile / chol_rbt_apply_tile serve both dtypes).
 * Argument errors: -1 uplo, -2 A, -3 AF, -4 W, -5 depth, -7 B, -8 X, -9 iter. */
int chol_sysv_rbt_tile(int uplo, chol_desc_t *A, chol_desc_t *AF, chol_desc_t *W, int depth, unsigned long long seed,
                       chol_desc_t *B, chol_desc_t *X, int *iter, double *berr);
/* The last chol_sytrf_rbt_tile / chol_sytrs_rbt_tile / chol_sysv_rbt_tile [ms]: total, generation and upload of W, the
 * transformation of A, the factorisation, all solves, all residual passes (with ||A||_inf), all vector butterflies;
 * then the number of refinement steps. */
int chol_last_rbt_stats(double *out8);

/* CHAMELEON_Lapack_to_Tile / Tile_to_Lapack equivalents (host LAPACK layout
 * <-> descriptor storage); single-process descriptors only. */
int chol_lapack_to_tile(const void *A, int lda, chol_desc_t *desc);
int chol_tile_to_lapack(chol_desc_t *desc, void *A, int lda);

/* Single-tile transfer for any descriptor this process owns tile (I,J) of. */
int chol_tile_upload(chol_desc_t *desc, int I, int J, const void *host_tile);
int chol_tile_download(chol_desc_t *desc, int I, int J, void *host_tile);

/* ||tril(L) tril(L)^T - A||_F / ||A||_F with A regenerated by the plgsy rule
 * (the check V6:72-87 intended).  L = factored descriptor.  Only tril(L) is read.  A NaN in tril(L) gives NaN
 * and a +-Inf there a non-finite value, never a finite number: the verdict cannot hide a non-finite factor. */
int chol_residual_plgsy(chol_desc_t *L, double bump, unsigned long long seed, double *rel);
/* The quantity v6_test.c:72-86 prints, computed correctly: ||A - L L^T||_inf / ||A||_inf, over the full symmetric
 * matrices.  Non-finite entries of tril(L) as in chol_residual_plgsy (the maximum over the row sums keeps a NaN). */
int chol_residual_plgsy_inf(chol_desc_t *L, double bump, unsigned long long seed, double *rel_inf);

/* ---- client-side host helpers (pure host code, usable without a GPU) ------ */
/* make_spd_like_chameleon C2:224-252 + enforce_strict_diag_dominance C2:255-264 */
void chol_make_spd_like_chameleon(double *A, int N, int LDA, double bump, char uplo,
                                  unsigned long long seed);
void chol_enforce_strict_diag_dominance(double *A, int N, int LDA, double eps);
/* handle_json W2:47-69 for the n payloads of a wave in one call (the worker's wave-level execution):
 * buf = the payloads back to back, payload t = buf[off[t] .. off[t+1]).  op[t]: 1 TRSM, 2 SYRK, 3 GEMM, 4 POTRF, B[t],
 * and id_off / id_len [3 t + r]: where the op's tile ids sit in buf, in the order chol_tile_batch takes them (TRSM
 * {inA, inL}, SYRK {inC, inA}, GEMM {inC, inAi, inAj}, POTRF {in}).  op[t] = 0: not a flat payload of these four ops
 * -- the caller's general JSON parser decides about it, with the reference's messages.  Host only. */
int chol_parse_payloads(const char *buf, const long long *off, int n, int *op, int *B, long long *id_off, int *id_len);
/* extract_block_from_spd_matrix_colmajor C2:280-309 */
void chol_extract_block(const double *A, int N, int LDA, int B, int bi, int bj, double *block);

/* ---- instrumentation ------------------------------------------------------ */
/* Device time (HIP events on the library's own streams) of the last whole-matrix
 * chol_potrf_tile: total ms and the trailing-update kernel's launch count / ms. */
int chol_last_potrf_stats(double *total_ms, double *update_ms, int *update_launches,
                          double *update_flops);
/* The schedule the last whole-matrix chol_potrf_tile actually ran -- the walker picks a regime per wave from speeds
 * measured at chol_init (chol_debug_calibration), so two boxes may run two schedules; with this a number can be tied
 * to its schedule afterwards.  out8: waves that were {0 paired, 1 plain (one far launch), 2 near / far halves,
 * 3 counter-linked chain, 4 ... with the near column, 5 ... with the tile POTRF as a flow, 6 update yields CUs to the
 * chain, 7 column k+1 in the latency form}; 0-2 and 4 partition the waves with an update, 3 / 5-7 are attributes.
 * *nt (may be NULL): the number of waves. */
int chol_last_potrf_regimes(int *out8, int *nt);
/* 1 = bracket the trailing-update launches of every wave (pair of waves) with HIP events
 * on the stream the big launch runs on; the wait that closes a bracket joins launches the
 * next wave's big launch depends on anyway, so no dependency is added (walker.h) -- what
 * remains is the cost of the event records, which bench.py puts on record beside the
 * bracketed steps ("unprofiled_ms").  For bench.py's roofline leg; 0 = off (default). */
int chol_set_profiling(int on);

/* Diagnostic: time the trailing-update launch of wave k alone (best of `reps`), on whatever
 * data the descriptor holds (the matrix is modified).  ablate must be 0 (the ablation twin of rounds 1-4 left the
 * library in round 5: CHOL_ERR_NOT_SUPPORTED). */
int chol_bench_update(chol_desc_t *desc, int k, int ablate, int reps, double *ms, double *flops);

/* Diagnostic: enable = 1 starts recording, per diagonal-block workgroup, 8 words of 100 MHz
 * realtime ticks {start, end, loaded, sum phase A, sum phase B, L stored, block inverses done,
 * factor inverse done}; enable = 0 stops, copies up to max_pairs records (8 words each) to
 * `out` and returns their number. */
int chol_debug_stamps(int enable, unsigned long long *out, int max_pairs);

/* Register-only 16x16x4 MFMA stream on every CU (waves_per_simd = 1..8): the matrix-core
 * rate this chip sustains under load, to quote beside the datasheet peak. */
int chol_mfma_probe(int dtype, int waves_per_simd, double *tflops);

/* Diagnostic: how many waves of the last whole-matrix chol_potrf_tile factored their diagonal tile in the flow form
 * (two persistent launches handing 16-column panels to each other through polled counters). */
int chol_debug_flow_waves(void);

/* Test hook, no GPU needed: the wave walker (one GPU, nt x nt tiles of edge mb) run over an engine that executes nothing and
 * records every launch with the tiles it reads and writes, every event record / wait and every counter a stream is gated
 * on; then every pair of launches that touch the same tile (or block-inverse workspace), one of them writing, must be
 * ordered by a stream, an event or a counter.  t_tile / t_panel [s]: the speeds the walker picks its regimes from (the
 * CHOLMI_* schedule switches apply as in the product); profiling: with the per-wave event brackets.  Returns the number of
 * findings (0 = every conflict ordered; < 0: the walker failed); `report` (cap bytes) receives them, one per line, and a
 * last line "<launches> launches, <w> event waits, <c> counter edges, <n> flow-form waves, <m> findings".
 * CHOLMI_CHECK_DROP_WAIT / CHOLMI_CHECK_DROP_GATE = n: the checker's self-test -- it ignores the n-th event wait / counter
 * edge the walker asks for, i.e. checks a schedule with that dependency missing. */
int chol_debug_schedule_check(int nt, int mb, double t_tile, double t_panel, int profiling, char *report, int cap);
/* ... and rank `rank`'s share of the same factorisation on a p x q grid: its sends read and its receives write (tiles, the
 * diagonal / head tile buffers by wave parity, the panel buffers by wave mod 4) on the streams they are issued on. */
int chol_debug_schedule_check_grid(int nt, int mb, int p, int q, int rank, double t_tile, double t_panel, int profiling,
                                   char *report, int cap);
/* ... and that rank's whole launch graph as text, one launch per line in issue order:
 * "<id> <channel or -1> <S|R|-> <peer> <bytes> <group> <dep,dep,...|-> <kind> <seconds>" (kernel launches: channel -1, kind
 * P / T / U / Y / L and a rough duration from t_tile / t_panel -- scripts/predict_scale.py; transport calls: channel
 * 0 = diagonal and head tiles, 1 = panels, the peer, the size, the group of that channel they were issued in; deps = the
 * launches it is ordered behind by stream order, events and counters).  Returns the checker's findings, < 0 on error. */
int chol_debug_comm_trace(int nt, int mb, int p, int q, int rank, double t_tile, double t_panel, char *out, int cap);

/* The ordering of the task executor (chol_tile_batch / chol_potrf_batch) checked WITHOUT a GPU.
 * chol_debug_task_record(1, mutate) -- only before chol_init -- puts the executor into recording mode: the grouped-launch
 * entry points (and chol_batch_mark / _wait / _info, chol_sync) run their real dependency tracking on whatever pointer
 * values the caller passes (they are never dereferenced), skip every HIP call and log each batch with the tiles it reads
 * and writes, its stream, its event waits and what the host knew to be complete.  mutate >= 0 drops that one event wait
 * (self-test).  chol_debug_task_check(out5) then examines every pair of batches that touch the same tile, one of them
 * writing: out5 = {batches, event waits, pairs examined, pairs NOT ordered, pairs ordered by a host-side wait};
 * chol_last_error() describes the first unordered pair.  chol_debug_task_record(0, -1) leaves the mode. */
int chol_debug_task_record(int on, int mutate);
int chol_debug_task_check(long long *out5);

/* What the walker's regime switches (pairs / halves / counter-linked chain / CU hand-over) are measured in,
 * taken once at chol_init (or from CHOLMI_CALIB="tf64,us64,tf32,us32"): out8[0..3] = fp64 MFMA probe
 * [TFLOP/s], fp64 128 x 128 diagonal-block step alone [us], the same for fp32; out8[4..7] = the derived
 * update rate inside the DAG [TFLOP/s] and panel-chain step [us] per dtype that the thresholds use. */
int chol_debug_calibration(double *out8);
/* Name of the trailing-update kernel launched for `dtype`, as a profiler prints it (bench.py's roofline.kernel). */
int chol_debug_update_kernel(int dtype, char *buf, int buflen);
/* 1 if chain-bound waves can use device-side counters (chol_init's probe found the panel streams on independent
 * hardware queues, and no device-side wait has timed out since), 0 if every dependency is a stream event -- e.g.
 * under a profiler that serialises kernels, where the probe fails by design. */
int chol_debug_device_counters(void);

/* ---- local storage of a descriptor ---------------------------------------- */
void *chol_desc_local_ptr(chol_desc_t *desc, size_t *bytes);
int chol_desc_local_tiles(chol_desc_t *desc, int *lmt, int *lnt);

/* ---- distributed factorisation behind chol_potrf_tile --------------------- */
/* chol_potrf_tile(ChamLower, A) on a descriptor with p*q > 1 (the reference passes p, q from argv
 * straight into CHAMELEON_Desc_Create, V6:26-27, 44-45) runs the 2D block-cyclic wave DAG of all
 * p*q processes inside the library -- the SAME wave walker as on one GPU (csrc/walker.h; p = q = 1 is its
 * instance without transport calls): paired panels, near / far halves, the POTRF steps pipelined with the
 * owner's TRSM steps.  What moves per wave, point to point, nobody receiving a tile it does not use:
 * L(k,k) with its block inverses from its owner to the other ranks of its process column; the head tile
 * L(k+1,k) ahead of everything else to the owner of (k+1,k+1); every panel tile L(i,k) along process row
 * i mod p (whole contiguous parts) and to the ranks of process column i mod q (tile by tile).
 *
 * A transport is a table of stream-ordered point-to-point operations.  `stream` is a hipStream_t;
 * everything issued between group_begin and group_end progresses together (ncclGroupStart /
 * ncclGroupEnd semantics: sends and receives of one group may be matched in any order).
 * allreduce_max is a blocking host-value reduction (the final LAPACK info).
 * The walker drives TWO channels from two streams of its own: channel 0 carries the small latency-critical
 * messages (diagonal tile, head tile), channel 1 the panel exchange -- so that a communicator which executes
 * its operations in issue order (RCCL does) never queues the next diagonal tile behind a panel. */
typedef struct chol_transport {
  void *ctx;
  int (*group_begin)(void *ctx);
  int (*send)(void *ctx, const void *buf, size_t bytes, int peer, void *stream);
  int (*recv)(void *ctx, void *buf, size_t bytes, int peer, void *stream);
  int (*group_end)(void *ctx);
  int (*allreduce_max)(void *ctx, long long *value);
} chol_transport_t;
/* Install (copy) a transport for both channels; NULL removes it.  Ranks are those of chol_set_rank.
 * chol_set_transport_channel replaces the table of one channel (0 or 1) afterwards. */
int chol_set_transport(const chol_transport_t *t);
int chol_set_transport_channel(int channel, const chol_transport_t *t);
/* The RCCL transport (xGMI inside a node): rank 0 creates the id blob (CHOL_RCCL_ID_BYTES: one ncclUniqueId
 * per channel), the application shares it out of band (MPI, torch.distributed store, a file), every rank calls
 * _init -- which builds one communicator per channel on this process's device and installs the transport
 * (ncclSend / ncclRecv in ncclGroupStart / ncclGroupEnd).  librccl is loaded at this call, not at link
 * time; its version (ncclGetVersion) must match the major version of the rccl.h this library was compiled
 * against and be >= 2.7 (point-to-point operations); _version returns the code (0: not loadable). */
#define CHOL_RCCL_ID_BYTES 256
int chol_transport_rccl_unique_id(void *id256);
int chol_transport_rccl_init(const void *id256, int rank, int nranks);
int chol_transport_rccl_finalize(void);
int chol_transport_rccl_version(void);
/* Host time spent issuing the last distributed factorisation (everything but the final
 * synchronisation), in microseconds per wave, and the number of transport operations it posted. */
int chol_dist_last_stats(double *issue_us_per_wave, long long *sends, long long *recvs, long long *bytes_sent);

/* Collect the lower tiles of a p x q descriptor on rank `root` into a device-resident single-process
 * descriptor of the same order, tile size and type (`dst` is ignored on the other ranks): lets the
 * root verify a distributed factorisation with chol_residual_plgsy.  Collective over the p*q ranks. */
int chol_dist_gather_lower(chol_desc_t *src, chol_desc_t *dst, int root);

/* ---- test hooks of the distributed path (never used by chol_potrf_tile) --- */
/* A transport that moves nothing: sends vanish, receives deliver zeros (stream-ordered).  Lets one process play
 * any single rank of a p x q grid on a one-GPU box and time that rank's schedule with communication taken as
 * free; the numerical result is meaningless. */
int chol_set_transport_null(void);

/* One message of `bytes` bytes (a positive multiple of 8) from this rank to itself on EACH channel of the
 * installed transport, both groups in flight together on the walker's two communication streams,
 * byte-compared.  On a one-rank RCCL communicator: ncclSend / ncclRecv to self inside one group. */
int chol_transport_selftest(int self_rank, size_t bytes);

/* The wave walker over caller-supplied tile kernels, so that the distribution logic (ownership,
 * addressing, matching of sends and receives, buffer reuse, the paired / halves regimes) can run without
 * a GPU under any transport.  Tiles are addressed as in a descriptor: local tile (il, jl) of an
 * lmt x lnt local grid at store + (il + jl*lmt) * B*B elements.  All callbacks are synchronous and are
 * called in a valid sequential order.  mode: 0 every wave plain and split, 1 mixed (panels in pairs while a
 * rank has >= 6 tiles to update), 2 every wave in pairs -- the regimes the product picks by measured speed. */
typedef struct chol_test_engine {
  void *ctx;
  void *store;      /* this rank's tiles */
  size_t esize;     /* bytes per element */
  void *(*alloc)(void *ctx, size_t bytes);                       /* receive buffers */
  int (*potrf)(void *ctx, int k, void *lkk);
  int (*trsm)(void *ctx, int k, const void *lkk);
  int (*update)(void *ctx, int k, int jlo, int jhi, const void *const *bases, const int *firsts, int skip_diag);
  int (*update_diag)(void *ctx, int k, int j, const void *const *bases, const int *firsts);
  int (*info)(void *ctx);
} chol_test_engine_t;
int chol_dist_factorize_with(const chol_test_engine_t *engine, const chol_transport_t *transport, int N, int B,
                             int p, int q, int rank, int mode);

/* A p x q factorisation rehearsed on ONE GPU: p*q ranks as threads of this process, each with its own
 * streams, workspaces and local tiles, the real kernels, and an in-process transport whose sends and receives
 * are stream-ordered device copies (no device synchronisation anywhere: the stream / event ordering and the
 * buffer reuse of the multi-GPU schedule are what is exercised).  The matrix is plgsy(bump, seed) of order N
 * (a multiple of mb, mb a multiple of 128); the factor's lower tiles are gathered into `full`, a
 * device-resident 1 x 1 descriptor of the same order, tile size and type.  *ms: wall time (the ranks share the
 * GPU: a stress figure, not a scaling figure).  Returns the LAPACK info the ranks agreed on. */
int chol_dist_rehearse(int dtype, int N, int mb, int p, int q, double bump, unsigned long long seed,
                       chol_desc_t *full, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* CHOLMI_H */
