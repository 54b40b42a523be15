// Internal declarations shared by the kernel and API translation units of
// libcholmi.so.  Not part of the ABI (that is include/cholmi.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/cholmi.h"

// The descriptor behind chol_desc_t (include/cholmi.h): Chameleon's CHAM_desc_t arguments plus what
// this library derives from them.
struct chol_desc {
  int dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q;
  int mbi, bsizi;    // stored tile edge / size: mb rounded up to 128 when the library owns a padded image
  bool padded;       // stored tiles are larger than (mb, nb) and/or the last tile row/column is ragged
  int mt, nt;        // global tile grid
  int prow, pcol;    // this process's grid coordinates
  int lmt, lnt;      // local tile grid
  size_t esize;
  void *mat;         // storage as seen by the caller (host or device)
  bool on_device;    // mat is device memory
  bool owns;         // library allocated mat
  // static work list of the trailing updates: the local strictly-lower tiles sorted by column
  // descending (rows ascending inside a column), entries with column >= j in [0, ge[j]); then,
  // from n_off on, the local diagonal tiles sorted by column descending, [n_off, n_off + gd[j])
  int2 *d_list = nullptr;
  std::vector<int> ge, gd;
  int n_off = 0;
  // chol_desc_set_version: names the CONTENT behind `mat` (the worker: a hash of the write-once result id the
  // blob belongs to); lets the library keep the block inverses of a factored tile for the TRSM tasks that follow
  unsigned long long version = 0;
  // A sub-matrix view (i, j, m, n) over a USER buffer (tile-aligned offsets, whole tiles): `mat` is a library-owned
  // compact image of the view's tiles, refreshed from the user's tile matrix before every operation on this
  // descriptor and written back after every operation that modifies it (api.hip: with_views).
  void *user_mat = nullptr;
  int user_lmt = 0;              // tile rows of the user's matrix
  int user_i = 0, user_j = 0;    // the view's first ROW / COLUMN in it (any offset: a view may start inside a tile)
};

extern "C" int chol_internal_fail(int code, const char *msg);  // api.hip: sets chol_last_error, returns code

// the segments of a descriptor's work list that hold the tiles of columns [jlo, jhi) (clamped to the matrix):
// `na` off-diagonal entries from `off`, `nb` diagonal ones from `offb`
struct ColRange {
  int off, na, offb, nb;
};
inline ColRange col_range(const chol_desc *d, int jlo, int jhi) {
  jlo = std::min(jlo, d->nt), jhi = std::min(jhi, d->nt);
  return ColRange{d->ge[jhi], d->ge[jlo] - d->ge[jhi], d->n_off + d->gd[jhi], d->gd[jlo] - d->gd[jhi]};
}

namespace cholmi {

// streams of one rank's factorisation (walker.h)
enum { ST_MAIN = 0, ST_PANEL, ST_TRSM, ST_U1, ST_CX, ST_PX, ST_COUNT };

constexpr int SEM_SLOTS = 65536;   // device-side counters: 3 mb/128 + 1 per tile column (+ the flow's control block) ...
constexpr int TILE_SEM_SETS = 8;   // ... plus rotating sets of 32 for the single-tile POTRF's fused in-tile steps
constexpr int SEM_INTS = (SEM_SLOTS + TILE_SEM_SETS * 32) * 32;  // ... each on a 128-byte line of its own

// device buffers that live as long as the context (receive buffers of the distributed walker)
struct DevPool {
  struct Blk {
    void *p;
    size_t bytes;
    bool used;
  };
  std::vector<Blk> blks;
  void *get(size_t bytes);
  void release_all() {
    for (auto &b : blks) b.used = false;
  }
  void free_all();
};

// Everything one rank's factorisation runs on: its streams, workspaces, counters, events, timings.  The process
// has one (api.hip: the context behind the C ABI); the one-GPU rehearsal of the distributed walker makes more.
struct RankCtx {
  int device = -1;
  hipStream_t st[ST_COUNT] = {};
  void *winv = nullptr;  // inverses of the 128x128 diagonal blocks of L(k,k), two sets (wave parity)
  size_t winv_bytes = 0;
  int *d_info = nullptr;
  int *d_sem = nullptr;  // device-side dependency counters of the panel chain (kernels.hip: sem_wait), or null
  bool flow_ok = false;  // ... and ST_CX / ST_PANEL have queues of their own: the flow form of the tile POTRF may be used
  unsigned tile_sem_next = 0;
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> retired;  // streams chol_init replaced because an update stream's launches held theirs back
  int stream_swaps = 0;          // ... how many, and pairs that still collide after the attempts
  int stream_collisions = 0;
  hipEvent_t ev_flow = nullptr;  // joins ST_CX to ST_PANEL once, at the first flow-form wave of a factorisation
  bool profiling = false;
  // stats of the last whole-matrix potrf
  double total_ms = 0, update_ms = 0, update_flops = 0, issue_us = 0;
  int update_launches = 0;
  int flow_waves = 0;  // waves of the last whole-matrix potrf whose tile POTRF ran in flow form (kernels.hip: k_flow_factor)
  int regimes[8] = {};  // ... and its waves per regime (walker.h: Walker::R_*), of regimes_nt waves (chol_last_potrf_regimes)
  int regimes_nt = 0;
  long long sends = 0, recvs = 0, bytes_sent = 0;
  DevPool pool;
  // measured once at creation, by dtype (0 = f64, 1 = f32): the register-only MFMA stream's rate [TFLOP/s]
  // and one 128 x 128 diagonal-block step of the panel chain alone [us]; what the walker's regime switches use
  double probe_tflops[2] = {0, 0}, diag_us[2] = {0, 0};
};
int rank_ctx_create(RankCtx *r, int device, const RankCtx *calib_from);  // api.hip
void rank_ctx_destroy(RankCtx *r);
RankCtx *main_rank_ctx();
int main_rank(int *nranks);

// The trailing update inside the DAG runs at about this fraction of the register-only MFMA stream, and one
// 128-step of the panel chain (diagonal block, in-tile solve and update, launch gaps) takes about this many
// times the diagonal-block kernel alone (rounds 1-2, fp64: 65 of 76.4 TFLOP/s; 130 of 49 us): the units the
// walker's regime thresholds were tuned in, now derived from what chol_init measures per dtype.
constexpr double CHOLMI_UPDATE_EFF = 0.85, CHOLMI_STEP_FACTOR = 2.65;

constexpr int MACRO = 128;  // macro-tile edge: one workgroup's C block, and the
                            // diagonal-block size of the in-tile POTRF/TRSM
constexpr int MAXP = 8;     // max process-grid rows a panel reference can address

// Where the panel tiles L(i,k) of the current wave live.  Tile i is at
// base[i % P] + (i / P - first[i % P]) * bsiz  (elements).  Single GPU: P = 1,
// base[0] = column k of the matrix itself, first[0] = 0 (no copy).
struct PanelRef {
  const void *base[MAXP];
  int first[MAXP];
  int P;
};

// This process's part of a 2D block-cyclic tile matrix.
struct LocalMat {
  void *base;
  int lmt;   // local tile rows (leading dimension of the local tile grid)
  int P, Q;  // process grid
  int mb;    // tile edge (= ld inside a tile)
  long bsiz; // elements per tile
};

extern int g_trsm_small_max;
extern int g_poll_max_wgs;
// the flow form of a counter-linked wave's tile POTRF (kernels.hip: k_flow_factor): does it apply to tiles of nbm 128-blocks
bool flow_applies(int nbm);
extern int g_flow;
extern int g_flow_min_nbm;
extern int g_flow_max_nbm;
extern int g_flow_fences;
extern int g_intile_fused;
extern int g_min_units;
extern unsigned long long *g_dbg;
extern int *g_ytab;
constexpr int YTAB_ENTRIES = 2048;

// ---- launchers (kernels.hip) ---------------------------------------------
// C(i,j) -= L(i,k) L(j,k)^T for the (i,j) pairs in d_list[off .. off+na) followed by
// d_list[offb .. offb+nb) (off-diagonal tiles first, the diagonal tiles -- whose blocks above the
// diagonal exit at once -- last, so that they do not split the 64-block cohorts of an XCD);
// yield: the update's waves give their CU to guest workgroups of the panel chain (kernels.hip);
// pan2 != null: the updates by two panels in one pass (C -= L L^T of `pan`, then of `pan2`)
template <typename T>
void launch_trail_update(hipStream_t s, const LocalMat &C, const int2 *d_list, int off, int na, int offb,
                         int nb, const PanelRef &pan, bool yield = false, const PanelRef *pan2 = nullptr);

// sygst's rank-2k update (LAPACK DSYR2K, Lower): C(i,j) -= P(i) Q(j)^T + Q(i) P(j)^T for the same (i,j) list and
// with the same block map as launch_trail_update; P = pan, Q = qan (kernels.hip: k_syr2k_w8, k_syr2k_w8f)
template <typename T>
void launch_syr2k_update(hipStream_t s, const LocalMat &C, const int2 *d_list, int off, int na, int offb, int nb,
                         const PanelRef &pan, const PanelRef &qan);

// sytrf_nopiv's one-pass two-panel update: C(i,j) -= P(i) Q(j)^T for the same (i,j) list and with the same block map
// as launch_trail_update; P = pan (the unscaled panel W = L D, in scratch: PanelRef::first), Q = qan (L, the matrix's
// own column) -- kernels.hip: k_ldl_update_w8, k_ldl_update_w8f
template <typename T>
void launch_ldl_update(hipStream_t s, const LocalMat &C, const int2 *d_list, int off, int na, int offb, int nb,
                       const PanelRef &pan, const PanelRef &qan);

// In-tile blocked POTRF of one mb x mb tile (device pointer, ld = mb).  Writes the
// inverses of the MACRO x MACRO diagonal blocks of L to winv (mb/MACRO blocks of
// MACRO*MACRO elements, ld = MACRO).  info: device int, set to info_base + j (1-based)
// at the first non-positive pivot (first writer wins).
template <typename T>
void launch_potrf_tile(hipStream_t s, T *tile, int mb, T *winv, int *d_info, int info_base, int *sem = nullptr);

// C (mb x mb tile, lower part) -= A A^T, A one tile: 64 x 64 blocks, one workgroup each (critical chain)
template <typename T>
void launch_diag_syrk(hipStream_t s, T *C, const T *A, int mb);

// POTRF(tile) on stream sp with the TRSM of `ntiles` contiguous tiles pipelined behind it on
// stream st (ev: mb/MACRO + 1 events).  ev_head (may be null): recorded once the panel is solved.
// chol_init's probe: the consumer kernel goes first, polls *sem (zeroed) for <= ~20 ms and writes 1 (seen) or
// 2 (gave up) to *result; the producer kernel raises *sem
void launch_sem_probe(hipStream_t consumer, hipStream_t producer, int *sem, int *result);
// chol_init's probe of two streams' dispatch paths (kernels.hip: k_pipe_big): t[0] / t[1] = start of the many-round launch on
// `big` / of the one-wave kernel launched right behind it on `small` (100 MHz ticks)
void launch_pipe_probe(hipStream_t big, hipStream_t small, unsigned long long *t, int cus);

// The chain-bound form of a wave (device-side edges, kernels.hip: sem_wait).  The SYRK on the next diagonal
// tile, C(k+1,k+1) -= L(k+1,k) L(k+1,k)^T, is cut into the K = 128 slices of the head tile's block columns
// and issued on `su`; the TRSM steps go to the TRSM stream as before -- but every kernel of the three
// streams is launched ahead of time, without a stream operation, and polls the counter of what it needs:
//   diagonal-block step s  -->  TRSM step s: solve  -->  slice s          in-tile solve s  -->  TRSM step s: update
//   last slice  -->  POTRF(k+1)'s first diagonal-block step (launch_panel_pipelined's wait_sem / wait_target)
struct SyrkPipe {
  void *c;         // tile (k+1,k+1)
  hipStream_t su;  // has already waited for the earlier writers of that tile
  int *sem;        // 3 nbm + 1 zeroed counters of this wave, 32 ints (one 128-byte line) apart; the last one
                   // counts the last slice's workgroups: n (n + 1) / 2, n = mb / 64
  // the tile POTRF as a flow (kernels.hip: k_flow_factor / k_flow_rows), or null: its zeroed control block
  // (flow_lines(nbm, nbm) lines), the stream the row-slab waves run on, an event to join it once
  int *fc = nullptr;
  hipStream_t sflow = nullptr;
  hipEvent_t ev_flow = nullptr;
  bool join_flow = false;  // the flow stream has to join the POTRF stream's order by an event (walker.h)
};
inline int flow_ctl_lines(int nbm) { return nbm >= 2 && nbm <= 8 ? 1 + nbm + 2 * nbm * nbm : 0; }

template <typename T>
void launch_panel_pipelined(hipStream_t sp, hipStream_t st, hipEvent_t *ev, T *lkk, int mb, T *winv,
                            int *d_info, int info_base, T *tiles, long bsiz, int ntiles,
                            hipEvent_t ev_head = nullptr, const SyrkPipe *sy = nullptr, const int *wait_sem = nullptr,
                            int wait_target = 0, int *tile_sem = nullptr);

template <typename T>
void launch_col_update_small(hipStream_t s, T *C, const T *A, const T *B, int mb, int ntiles, long bsiz, int *done);

// winv from an already factored tile
template <typename T>
void launch_invert_diag(hipStream_t s, const T *tile, int mb, T *winv);
// the same for the nt tiles A + t tstride in one launch: the inverses of tile t at winv + t (mb/MACRO) MACRO^2
template <typename T>
void launch_invert_diag_batch(hipStream_t s, const T *A, long tstride, int nt, int mb, T *winv);

// tiles[t] := alpha * tiles[t] * L^{-T}, t < ntiles, tiles contiguous (stride bsiz)
template <typename T>
void launch_trsm_panel(hipStream_t s, T *tiles, long bsiz, int ntiles, const T *lkk, const T *winv,
                       int mb, T alpha);

// generic 1-tile C := alpha A B^T + beta C (lower_only: SYRK semantics)
template <typename T>
void launch_gemm_nt_tile(hipStream_t s, const T *A, const T *B, T *C, int mb, T alpha, T beta,
                         bool lower_only);

// the same product for nz1 x nz2 tiles in one launch: A + z1 sA, B + z2 sB, C + z1 sC1 + z2 sC2
template <typename T>
void launch_gemm_nt_batch(hipStream_t s, const T *A, long sA, int nz1, const T *B, long sB, int nz2, T *C, long sC1,
                          long sC2, int mb, T alpha, T beta);

// cout[z] = cin[z] - a[z] b[z]^T for n tasks given as device arrays of device tile pointers, out of place; b[z] == null:
// a SYRK task (b = a, the lower triangle updated, the strict upper one copied) -- kernels.hip: k_update_ptrs_w8
template <typename T>
void launch_update_ptrs(hipStream_t s, const T *const *cin, const T *const *a, const T *const *b, T *const *cout, int n, int mb,
                        bool yield);
// dst[z] <- src[z], z < n, `bytes` (a multiple of 16) each; src / dst: device arrays of device pointers
void launch_copy_ptrs(hipStream_t s, const void *const *src, void *const *dst, int n, long bytes);

template <typename T>
void launch_plgsy(hipStream_t s, const LocalMat &A, int lnt, int prow, int pcol, double bump,
                  unsigned long long seed, int mbu, long nglob, int side);

// accumulates sum((LL^T - A)^2) and sum(A^2) over the lower triangle (strict part
// counted twice) into acc[0], acc[1] (device doubles).  Single process only.
template <typename T>
void launch_residual(hipStream_t s, const T *Lbase, int Nb, int mb, double bump,
                     unsigned long long seed, double *d_acc, int mbu, long nglob,
                     double *rowsum = nullptr);  // rowsum: 2*nglob doubles (|R| rows, then |A| rows), zeroed

// pad helpers for the staged 1-tile path: dst is ldp x ldp (zeroed), identity on
// the padded part of the diagonal when `unit_pad`.
template <typename T>
void launch_pad_identity(hipStream_t s, T *dst, int n, int ldp);

// in-place transpose of a whole nt x nt tile matrix (mb multiple of 64)
template <typename T>
void launch_transpose_inplace(hipStream_t s, T *M, int nt, int mb);

// The maximum that LAPACK's norms take (DLANGE, DLANSY: `IF (VALUE < TEMP .OR. DISNAN(TEMP))`): a NaN on either side
// gives a NaN, where fmax and std::max drop it.  Every max of the norms and of the residual's row sums goes through
// it, so a NaN in the matrix is a NaN in the verdict.
__host__ __device__ inline double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// ---- launchers (verify_ops.hip): the driver's validation block, v6_test.c:51, 74-85 ----
// Geometry of a single-process stored tile image: lmt x lnt tiles of mbs x mbs elements, of
// which the caller's tile is the leading mbu x mbu part; the matrix is m x n.
struct TileGeo {
  int lmt, lnt, mbs, mbu;
  long m, n;
};
// The image cut into 128 x 128 blocks of stored rows (condest.hip): its block rows, and the blocks (P, Q), P >= Q, of
// one triangle
inline long block_rows(const TileGeo &g) { return (long)g.lmt * ((g.mbs + MACRO - 1) / MACRO); }
inline long tri_pairs(const TileGeo &g) { return block_rows(g) * (block_rows(g) + 1) / 2; }
// The group size 1, 2, 4 or 8 that takes k <= 8 columns (more: 8), and f called with it as a
// std::integral_constant: the kernels of a column group are instantiated for these four widths
int refine_width(int k);
template <typename F>
void with_width(int k, F f) {
  switch (refine_width(k)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}
// side: 0 all, 1 on or below the diagonal, 2 on or above
template <typename T>
void launch_lacpy(hipStream_t s, const TileGeo &g, int side, const T *A, T *B);
template <typename T>
void launch_geadd(hipStream_t s, const TileGeo &g, double alpha, const T *A, double beta, T *B);
// work: max(m, n) + 2 device doubles; result in work[0] (kind 0 max, 1 one, 2 inf, 3 sum of squares)
template <typename T>
void launch_lange(hipStream_t s, const TileGeo &g, int kind, const T *A, double *work);
// out(I,J) = sum_{K>=I} L(K,I)^T L(K,J), I >= J (lower part only; out != L)
template <typename T>
void launch_lauum_lower(hipStream_t s, const T *L, T *out, int nt, int mbs);

// ---- launchers (mixed.hip): the fp64 side of chol_dsposv_tile on a single-process image (mbs % 128 == 0) ----
// ga: the n x n matrix (only the Lower / Upper stored triangle is read), gx: the n x nrhs images (same mbs / mbu).
// part: sym_resid_part_bytes(ga, nrhs) of scratch; colmax: 2 nrhs zeroed words, max |R(:,j)| then max |X(:,j)| as
// double bit patterns; Rf: R rounded to fp32 at the same positions; *flag |= 1 where an entry does not fit in fp32.
size_t sym_resid_part_bytes(const TileGeo &ga, int nrhs);
void launch_sym_resid(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx, const double *X,
                      const double *B, double *part, float *Rf, unsigned long long *colmax, int *flag);
// the same pass with the residual kept in fp64: R (an n x nrhs image like X; only the rows of the matrix are written)
void launch_sym_resid_f64(hipStream_t s, const TileGeo &ga, int upper, const double *A, const TileGeo &gx,
                          const double *X, const double *B, double *part, double *R, unsigned long long *colmax);
// colmax[0] <- bits of the infinity norm of the symmetric matrix (row sums of |A| from the stored triangle)
void launch_sym_inf_norm(hipStream_t s, const TileGeo &ga, int upper, const double *A, double *part,
                         unsigned long long *colmax);
// the stored triangle -> the Lower fp32 tile image (every tile I >= J written; zeros in the unreferenced half of the
// diagonal tiles, the identity outside the matrix)
void launch_sym_to_f32(hipStream_t s, const TileGeo &ga, int upper, const double *A, float *Af, int *flag);
void launch_vec_to_f32(hipStream_t s, const TileGeo &gx, const double *B, float *Bf, int *flag);
// X := (double) C (assign) or X += (double) C
void launch_vec_update(hipStream_t s, const TileGeo &gx, const float *C, double *X, bool assign);

// ---- launchers (inverse.hip): the triangular inverse of chol_trtri_tile / chol_potri_tile ----
// A lower block-triangular matrix of n blocks of edge E (a multiple of 128), nbatch independent problems:
// block (i,j) of problem z at base + z sz + i si + j sj (ld), the inverses Xd(i) of its diagonal blocks at
// dg + z dsz + i dsi (ld dld; read as lower triangular), scratch for n blocks E x E at y + z ysz + m ysi (ld E).
template <typename T>
struct TriLevel {
  T *base;
  long si, sj, sz;
  int ld;
  const T *dg;
  long dsi, dsz;
  int dld;
  T *y;
  long ysi, ysz;
  int E;
};
// column c of the inverse below the diagonal, every problem: X(i,c) = -sum_{c<m<=i} X(i,m) L(m,c) Xd(c), in place
// (needs the columns right of c done; two launches)
template <typename T>
void launch_tri_column(hipStream_t s, const TriLevel<T> &L, int n, int nbatch, int c);
// the lower triangles of the nt * mb/128 inverses winv (128 x 128 each, tile by tile) into the diagonal
// 128-blocks of the diagonal tiles A + t tstride (ld mb)
template <typename T>
void launch_tri_put_diag(hipStream_t s, T *A, long tstride, int mb, int nt, const T *winv);
// *first <- the smallest 1-based i <= n with A(i,i) == 0 (diagonal tile t at A + t tstride, ld mbs, mbu of its rows
// inside the matrix), or a value above n
template <typename T>
void launch_diag_zero(hipStream_t s, const T *A, long tstride, int mbs, int mbu, long n, int *first);

// ---- launchers (condest.hip): chol_lansy_tile and chol_pocon_tile on a single-process image (any mbs) ----
// and the triangular sweeps that chol_pocon_tile, chol_porfs_tile, chol_posvx_tile and chol_trtrs_tile share.
// The image in 128 x 128 blocks of stored rows (bpt = ceil(mbs / 128) per tile); N-vectors of condest_vec_elems
// entries in that order, zero outside the matrix.
int condest_edge(const TileGeo &g);           // bpt 128: the edge of the staged diagonal tiles
size_t condest_vec_elems(const TileGeo &g);
// part: lansy_part_bytes(g) of scratch; res[0..2] <- max |a|, the largest row sum of |A|, the sum of squares
// (off-diagonal entries twice) of the symmetric matrix stored in the `upper` triangle
size_t lansy_part_bytes(const TileGeo &g);
template <typename T>
void launch_lansy(hipStream_t s, const TileGeo &g, int upper, const T *A, double *part, double *res);
// Dv (lmt tiles of condest_edge^2): the diagonal tiles of the factor as Lower (U^T for Upper), zero above the
// diagonal, the identity outside the matrix
template <typename T>
void launch_stage_diag(hipStream_t s, const TileGeo &g, int upper, const T *A, T *Dv);
// pocon's own one-vector form: one application of A^{-1} = L^{-T} L^{-1} (U^{-1} U^{-T}): x <- A^{-1} x; Dv: the
// inverted diagonal tiles; y, pd (bpt^2 blocks of 128), pg (2 NB bpt blocks of 128): scratch
template <typename T>
struct SweepBufs {
  T *x, *y, *pg, *pd;
};
template <typename T>
void launch_sweep(hipStream_t s, const TileGeo &g, int upper, const T *A, const T *Dv, const SweepBufs<T> &b);
// count <= 8 applications of A^{-1} = L^{-T} L^{-1} (U^{-1} U^{-T}) at once, in the NV = refine_width(count) form:
// x[j] <- A^{-1} x[j], each block of the factor read once per launch for all vectors; Dv: the inverted diagonal tiles;
// pad: NV - count vectors of scratch for the unused places (none for count = 1, 2, 4, 8); scratch per vector: y, pd
// (bpt^2 blocks of 128), pg (2 NB bpt blocks of 128), vector j's at y + j nv, pg + j 2 NB bpt 128, pd + j bpt^2 128:
// msweep_scratch_elems(g) elements of T hold them for 8 vectors.
// which = SWEEP_FORWARD / SWEEP_BACKWARD: one half alone, L y = x (U^T y = x) / L^T y = x (U y = x): vector j's
// result is left at b.y + j condest_vec_elems(g) and x[j] is used up
enum { SWEEP_BOTH = 0, SWEEP_FORWARD = 1, SWEEP_BACKWARD = 2 };
template <typename T>
struct MSweepBufs {
  T *y, *pg, *pd;
};
size_t msweep_scratch_elems(const TileGeo &g);
template <typename T>
void launch_msweep(hipStream_t s, const TileGeo &g, int upper, const T *A, const T *Dv, T *const *x, int count,
                   T *pad, const MSweepBufs<T> &b, int which = SWEEP_BOTH);
// x <- 1/n (mode 0), e_j (1; j a vector index), the alternating-sign vector of DLACN2 (2)
template <typename T>
void launch_vec_fill(hipStream_t s, const TileGeo &g, T *x, int mode, long j);
// out[0..5] <- sum |x|, max |x|, its first vector index, a non-finite entry (0 / 1), x[jlast] (jlast >= 0), a sign
// change; sign != 0: x and isgn <- sign(x) (x >= 0 -> +1), the change flag set where isgn changes.
// part: vec_stats_part_bytes() of scratch.
size_t vec_stats_part_bytes();
template <typename T>
void launch_vec_stats(hipStream_t s, const TileGeo &g, T *x, int *isgn, int sign, long jlast, double *part,
                      double *out);

// ---- launchers (refine.hip): chol_poequ_tile, chol_laqsy_tile, chol_porfs_tile, chol_posvx_tile (condest.hip's
// geometry and vector layout).  An n x ncols image (B, X, S) has the matrix's row tiling (same mbs, mbu, lmt).
// Up to 8 columns of an image and the condest-layout vector slots they go with: slot v[j] <-> image column d[j].
struct VecCols {
  int n;
  int v[8], d[8];
};
// mode 0: S(i) <- 1/sqrt(A(i,i)) (IEEE) where A(i,i) > 0; mode 1: only scan S.  part (diag_scan_part_bytes): per
// workgroup min, max, the first 0-based i with a value <= 0 (or -1) of the scanned values
size_t diag_scan_part_bytes();
template <typename T>
void launch_diag_scan(hipStream_t s, const TileGeo &g, const T *A, T *S, int mode, double *part);
// the stored triangle of A <- (S(j) S(i)) A(i,j) (LAPACK DLAQSY's order); S an n x 1 image
template <typename T>
void launch_laqsy(hipStream_t s, const TileGeo &g, int upper, T *A, const T *S);
// D <- diag(S) D for the n x ncols image D
template <typename T>
void launch_row_scale(hipStream_t s, const TileGeo &gx, T *D, const T *S);
// V[v nv ...] <- image column d (zero outside the matrix); image column d <- (add: += ) V[v nv ...]
template <typename T>
void launch_gather(hipStream_t s, const TileGeo &gx, const T *D, const VecCols &cols, T *V);
template <typename T>
void launch_scatter(hipStream_t s, const TileGeo &gx, T *D, const VecCols &cols, const T *V, bool add);
// V[v] <- W[v] .* V[v] for the slots v = cols.v[j] whose bit j of mask is set
template <typename T>
void launch_vec_weight(hipStream_t s, const TileGeo &g, T *V, const T *W, const VecCols &cols, unsigned mask);
// DPORFS's residual pass for the columns d[j] (at most 8) of X and B: R[v] <- B - A X, F[v] <- the FERR weight
// |R| + (n+1) eps W (+ safe1 where W <= safe2), W = |B| + |A||X|; berr[v] (zeroed) <- bits of the column's
// componentwise backward error as a double.  part: porfs_part_elems(ga, refine_width(n)) elements of T.
size_t porfs_part_elems(const TileGeo &ga, int width);
template <typename T>
void launch_porfs_resid(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gx, const T *X,
                        const T *B, const VecCols &cols, T *part, T *R, T *F, double eps, double safe1, double safe2,
                        unsigned long long *berr);

// ---- launchers (trmm.hip): chol_trmm_tile's narrow path and chol_logdet_tile (condest.hip's geometry) ----
// B(:, cols.d[j]) <- alpha op(T) B(:, cols.d[j]) for at most 8 columns of the n x ncols image B (gx), T the `upper`
// triangle of the n x n image A (ga; the other strict triangle is not read), op the transpose when trans.  x: 8
// vectors (condest_vec_elems each) that take the gathered columns; part: trmm_part_elems(ga, refine_width(cols.n))
// elements, the per-block products that a second kernel adds in a fixed order
size_t trmm_part_elems(const TileGeo &ga, int width);
template <typename T>
void launch_trmm_narrow(hipStream_t s, const TileGeo &ga, int upper, int trans, const T *A, const TileGeo &gx, T *B,
                        const VecCols &cols, T alpha, T *x, T *part);
// out (nt tiles of mb x mb) <- the lower triangles of the diagonal tiles A + t tstride (ld mb), zero above the
// diagonal; transposed: each written as its transpose
template <typename T>
void launch_tri_tiles(hipStream_t s, const T *A, long tstride, int mb, int nt, bool transposed, T *out);
// v <- alpha v, `total` entries
template <typename T>
void launch_scale(hipStream_t s, T *v, long total, T alpha);
// out[0] <- 2 sum_i log A(i,i) (logs and sum in fp64, fixed order), out[1] <- the first 0-based i whose A(i,i) is
// <= 0 or NaN, or -1; part: logdet_part_bytes() of scratch
size_t logdet_part_bytes();
template <typename T>
void launch_logdet(hipStream_t s, const TileGeo &g, const T *A, double *part, double *out);

// ---- launcher (symm.hip): chol_symm_tile (condest.hip's geometry) ----
// C <- alpha A B + beta C: A the n x n image ga of which only the `upper` / lower triangle is read, B (gb) and C (gc)
// n x nrhs images with A's row tiling (their stored tile edge may be A's rounded up to 128); one MFMA kernel for every
// nrhs, a workgroup owning 128 rows x symm_width(nrhs) columns of C; alpha == 0: A and B are not read.  -> the number
// of workgroups launched
int symm_width(long nrhs);
template <typename T>
long launch_symm(hipStream_t s, const TileGeo &ga, int upper, const T *A, const TileGeo &gb, const T *B,
                 const TileGeo &gc, T *C, T alpha, T beta);

// ---- launchers (pstrf.hip): the pivoted panel of chol_pstrf_tile (LAPACK DPSTRF, Lower) on a single-process image.
// Entry (r, c) of the n x n matrix at (r / mb + (c / mb) lmt) bsiz + r % mb + (c % mb) mbi; the padding is never
// touched.  Scratch: dg, w (n each), pval, pidx (pstrf_chunks(n) each: the partial maxima of the candidates
// d = dg - w per 64-row chunk), ctl (one zeroed int: the step + 1 at which the factorisation stopped), pj (n: the
// pivot of every step), ajj (one element).
struct PsGeo {
  long n;
  int mb, mbi, lmt;
  long bsiz;
};
long pstrf_chunks(long n);
// the start of tile column k0 / mb: dg(i) <- A(i,i), w(i) <- 0 for i >= k0, and their partial maxima
template <typename T>
void launch_pstrf_init(hipStream_t s, const PsGeo &g, const T *A, long k0, T *dg, T *w, T *pval, int *pidx);
// *outv, *outi <- the largest partial of the chunks c0 .. (NaN above all, ties to the smaller index)
template <typename T>
void launch_pstrf_max(hipStream_t s, const PsGeo &g, long c0, const T *pval, const int *pidx, T *outv, int *outi);
// pivot step j of the tile column that starts at k0 (two launches): the choice of p (or the stop, for j > 0, when
// d(p) <= dstop or is NaN), the symmetric interchange j <-> p, then column j of L and the next partial maxima
template <typename T>
void launch_pstrf_step(hipStream_t s, const PsGeo &g, T *A, long j, long k0, T dstop, T *dg, T *w, T *pval, int *pidx,
                       int *ctl, int *pj, T *ajj);
// rows[t] <- rows[m + t] (t < m) in columns 0 .. ncols-1: the composed interchanges of one tile column (LAPACK laswp)
template <typename T>
void launch_pstrf_laswp(hipStream_t s, const PsGeo &g, T *A, long ncols, const int *rows, int m);
// A(r,c) <-> A(c,r) for r > c, any tile geometry (the Upper path of a single tile whose edge is not a multiple of 64)
template <typename T>
void launch_pstrf_transpose(hipStream_t s, const PsGeo &g, T *A);

// ---- launchers (sygst.hip): chol_sygst_tile (LAPACK DSYGST, itype 1, Lower) on a single-process image ----
// one diagonal tile D (e x e, ld e) <- the lower triangle of X S X^T on its rows and columns < nv, S the symmetric
// expansion of D's lower triangle (the identity beyond e), X (E x E, ld E; E >= e, a multiple of 128) lower
// triangular: L(k,k)^{-1}.  S, W, C: E x E scratch each; afterwards C holds the symmetric X S X^T (its lower
// triangle mirrored), the A(k,k) of the step's two SYMMs.
template <typename T>
void launch_sygst_diag(hipStream_t s, T *D, int e, int nv, const T *X, int E, T *S, T *W, T *C);
// tile row m of the deferred left solve, two launches: X(m,k) = Xd(m) (A(m,k) - sum_{k<j<m} L(m,j) X(j,k)) in
// place over A(m,k) for every k < m.  Tile (i,j) of A and L at + (i + j lmt) bs, ld E (E % 128 == 0); the
// inverted diagonal tile Xd(m) at Xd (ld E); y: m tiles of scratch
template <typename T>
void launch_sygst_solve_row(hipStream_t s, T *A, const T *L, long bs, int lmt, int E, int m, const T *Xd, T *y);

// ---- launchers (chud.hip): chol_chud_tile / chol_chdd_tile (LINPACK DCHUD / DCHDD, Lower) on a single-process image ----
constexpr int CHUD_GROUP = 16;  // the vectors of one pass: a lane of the appliers keeps that many entries of V in registers
// the vectors g0 .. of an n x r image with the factor's row tiling: vector t, stored row r of tile row I at
// p + ((t / mb) lmt + I) bs + (t % mb) ld + r
template <typename T>
struct ChudVecs {
  T *p;
  long bs;
  int ld, lmt, mb, g0;
};
// columns c0 .. c0+nc-1 (nc <= 128) of the diagonal tile D (ld e; tile row I of V) against rg <= CHUD_GROUP vectors:
// the nc x nc diagonal block and its rows of V rotated in place, tab[((c0 + j) rg + t) 4 ..] <- (c, s, ci, sigma s) of
// column c0 + j and vector g0 + t (chud_rot.h).  info[0..1] <- (col1 + j, g0 + t) at a rotation whose rr^2 is not
// positive, when that column comes before the one already recorded (0: none)
template <typename T>
void launch_chud_gen(hipStream_t s, T *D, int e, int c0, int nc, const ChudVecs<T> &V, int I, int rg, T sigma, T *tab,
                     int *info, int col1);
// the rotations of columns c0 .. c0+nc-1 of tile column k applied to the stored rows [r0, r1) counted from the top of
// the diagonal tile (tile (k + i, k) at Acol + i bs, ld e); rows outside the matrix (beyond mb in a tile, beyond n)
// are neither read nor written
template <typename T>
void launch_chud_apply(hipStream_t s, T *Acol, long bs, int e, int mb, long n, int k, long r0, long r1, int c0, int nc,
                       const T *tab, const ChudVecs<T> &V, int rg);

// ---- launchers (chex.hip): chol_chex_tile (LINPACK DCHEX, Lower) on a single-process image; rows and columns 0-based ----
// the image: tile (I, J) at A + (I + J lmt) bs, ld e, mb used rows and columns a tile, order n
template <typename T>
struct ChexMat {
  T *A;
  long bs;
  int lmt, e, mb;
  long n;
};
// the saved copy of a tile column from tile row row0 down, tile after tile
template <typename T>
struct ChexStage {
  const T *p;
  int row0;
};
// w (tile row I, stored row r at w + I e + r) over the rows k0..n-1 <- job 2: the moved variable's old column in the
// new row order, chud's vector; job 1: what a row carries into its rotations (row k0 is left to launch_chex_coef)
template <typename T>
void launch_chex_vec(hipStream_t s, const ChexMat<T> &M, int k0, int l0, int job, T *w);
// A(i, l0) <- w_i for i >= l0
template <typename T>
void launch_chex_setcol(hipStream_t s, const ChexMat<T> &M, int l0, const T *w);
// the columns c < c1 of tile column J, tile rows [I0, I1), from the copies S0 (of tile column J) and S1 (of J + 1): in
// a column before k0 the rows k0..l0 permuted; job 2: a column j of k0..l0-1 <- the old column j + 1, its rows above
// l0 moved up by one, a zero in row l0 (the other columns and rows are left alone)
template <typename T>
void launch_chex_move(hipStream_t s, const ChexMat<T> &M, int J, int c1, int I0, int I1, int k0, int l0, int job,
                      const ChexStage<T> &S0, const ChexStage<T> &S1);
// job 1: tab[2 (i - k0) ..] <- (cc_i, ss_i) of column i, i = l0-1 down to k0 (chex_rot.h), from row l0 of A; w_k0 <- the
// last pivot; info[0] <- the 1-based new column of the first rotation whose rho^2 is not positive (else untouched)
template <typename T>
void launch_chex_coef(hipStream_t s, const ChexMat<T> &M, int k0, int l0, T *tab, T *w, int *info);
// job 1: the new columns jlo..jhi (inside tile column J and k0..l0) of every row from tile row J down (nt tile rows),
// right to left, read from S0 (the copy of tile column J) and S1 (of J - 1, its last column), written to A
template <typename T>
void launch_chex_apply(hipStream_t s, const ChexMat<T> &M, int nt, int J, int jlo, int jhi, int k0, int l0,
                       const ChexStage<T> &S0, const ChexStage<T> &S1, const T *tab, T *w);

// ---- launchers (sytrf.hip): chol_sytrf_nopiv_tile / chol_sytrs_nopiv_tile (A = L D L^T, Lower) on a single-process image ----
// one diagonal tile (e x e, ld e, e % 128 == 0) <- its factor in place, by 128-block steps: D on the diagonal, the unit
// lower triangular L below it, the strict upper triangle not touched.  Wt: one tile of scratch; Lc, winv: e / 128 blocks
// of 128 x 128 each (afterwards: the unit lower triangular diagonal blocks of L and their inverses, what
// launch_trsm_panel takes with the tile itself as lkk); dv, rv (e each) <- d_j and 1 / d_j; *info <- info_base + j
// (1-based) at the first pivot that is zero or not finite (the first one wins); pm: ldl_partials() doubles, zeroed once
// per factorisation, that collect the partial maxima of |L|
int ldl_partials();
template <typename T>
void launch_ldl_tile(hipStream_t s, T *tile, int e, T *Wt, T *Lc, T *winv, T *dv, T *rv, int *info, int info_base,
                     double *pm);
// the solved panel W (`total` elements in whole tiles of bs, ld e) copied to Wscr and scaled in place to L = W diag(rv),
// rv = 1 / d: one multiplication by the reciprocal per entry (LAPACK DSYTF2's r1 = 1 / d)
template <typename T>
void launch_ldl_scale(hipStream_t s, T *W, T *Wscr, long total, long bs, int e, const T *rv, double *pm);
// out[0..4] <- the number of positive and of negative pivots, min |d|, max |d| over rows 0 .. n-1 (the padding is not
// counted), max |L| from the partials
template <typename T>
void launch_ldl_stats(hipStream_t s, const T *dv, long n, int mb, int e, const double *pm, double *out);
// U (nt tiles of bs) <- the diagonal tiles of the factor (tile t at A + t dstride) with unit diagonals and zeros above,
// rv (nt e) <- 1 / d
template <typename T>
void launch_ldl_stage(hipStream_t s, const T *A, long dstride, long bs, int e, int nt, T *U, T *rv);
// potrs's transposed image Z of the right-hand sides (tile row r of tile column i at (r + i nr) bs) <- Z diag(rv)
template <typename T>
void launch_ldl_zscale(hipStream_t s, T *Z, long total, long bs, int e, int nr, const T *rv);

// ---- launchers (rbt.hip): the symmetric random butterfly transformation of chol_sytrf_rbt_tile and its solves ----
// W: an n x depth (or wider) image with A's row tiling whose column k holds the diagonal entries of level k in row
// order (level k: 2^k butterflies of order n / 2^k; n a multiple of 2^(k+1)).
// one level of A <- W^T A W on the stored Lower triangle, in place: A <- D_k^T A D_k
template <typename T>
void launch_rbt_sym(hipStream_t s, const TileGeo &ga, T *A, const TileGeo &gw, const T *W, int level);
// one level on the rows of an n x ncols image: X <- D_k^T X (trans) or D_k X
template <typename T>
void launch_rbt_vec(hipStream_t s, const TileGeo &gx, T *X, const TileGeo &gw, const T *W, int level, bool trans);
// W(r, k) <- src[r + k n], k < depth (src: device)
template <typename T>
void launch_rbt_put(hipStream_t s, const TileGeo &gw, T *W, const T *src, long n, int depth);

// out-of-place transposes of `count` mb x mb tiles (mb % 64 == 0)
template <typename T>
void launch_tiles_transpose(hipStream_t s, const T *in, long istride, T *out, long ostride, int mb, int count);

// register-only MFMA stream (blocks x 256 threads, 16 MFMA per wave per iteration)
template <typename T>
void launch_mfma_probe(hipStream_t s, T *out, int blocks, int iters);

}  // namespace cholmi
