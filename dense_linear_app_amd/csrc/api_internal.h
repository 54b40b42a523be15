// What api.hip shares with the other host translation units of the ABI (spd.hip, the routines that work from a factor;
// batched.hip, the batched small-matrix routines, which use the context, the errors and the scratch pools alone):
// the context's state, the error reporting, the dispatch on the element type, the scratch pools, the view refresh, the
// descriptor rules, running an Upper call through the Lower path, and a whole-matrix descriptor's trailing update.  Host only: the kernel translation
// units see cholmi_internal.h alone.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <functional>
#include <initializer_list>
#include <mutex>

#include "../../include/cholmi.h"
#include "cholmi_internal.h"

namespace cholmi {

// (api.hip and spd.hip are compiled with default visibility for the C ABI; CHOL_LOCAL keeps a helper out of the
// library's dynamic symbols)
#define CHOL_LOCAL __attribute__((visibility("hidden")))

bool ctx_inited();
std::recursive_mutex &ctx_mutex();  // one ABI call at a time on the context
bool is_device_ptr(const void *p);  // device or managed memory (plain host memory: false)

// record msg as chol_last_error's text and return code; failf: the text formatted as printf does
int fail(int code, const char *msg);
CHOL_LOCAL int failf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char *what, const char *file, int line);
#define HIPCHECK(call)                                                           \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) return cholmi::fail_hip(e_, #call, __FILE__, __LINE__); \
  } while (0)
// CHOL_ERR_OUT_OF_MEMORY with "<what>: scratch allocation failed" (the HIP error cleared)
int scratch_failed(const char *what);

inline int roundup(int x, int m) { return (x + m - 1) / m * m; }

// f(T{}) for the element type T of `dtype` (CHOL_REAL_DOUBLE, else float): the call site is a generic lambda that
// names the type as decltype of its parameter
template <typename F>
auto by_dtype(int dtype, F &&f) {
  return dtype == CHOL_REAL_DOUBLE ? f(double{}) : f(float{});
}

// N device buffers, each grown on demand (in whole MiB) and kept until release(); Zero: a buffer is cleared when it
// grows.  One pool per set of buffers that are live together: two pools never share memory.
template <int N, bool Zero = false>
struct ScratchPool {
  void *p[N] = {};
  size_t bytes[N] = {};
  // buffer i holds at least `need` bytes afterwards, or CHOL_ERR_OUT_OF_MEMORY (scratch_failed(what))
  int ensure_bytes(int i, size_t need, const char *what) {
    if (bytes[i] >= need) return 0;
    if (p[i] && hipFree(p[i]) != hipSuccess) return scratch_failed(what);
    p[i] = nullptr;
    bytes[i] = 0;
    need = (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    // (the clearing runs on the null stream, which the library's non-blocking streams do not wait for, and hipMemset
    // of device memory may return before it is done: without the synchronisation it can overtake and wipe what the
    // caller's first kernels write into the new buffer)
    if (hipMalloc(&p[i], need) != hipSuccess ||
        (Zero && (hipMemset(p[i], 0, need) != hipSuccess || hipDeviceSynchronize() != hipSuccess)))
      return scratch_failed(what);
    bytes[i] = need;
    return 0;
  }
  template <typename T>
  T *as(int i) const {
    return reinterpret_cast<T *>(p[i]);
  }
  void release() {
    for (int i = 0; i < N; ++i) {
      if (p[i]) (void)hipFree(p[i]);
      p[i] = nullptr;
      bytes[i] = 0;
    }
  }
};

// One entry point's body between the refresh of its views' images and their write-back; a failed refresh returns
// before the body runs, a failed write-back is reported unless the body already failed.  The write-back also follows
// a body that returned info > 0 (a partly factored matrix, as LAPACK leaves it).  The body runs under the context
// lock, so bodies, and what only they call, do not take it again.
struct ViewArg {
  chol_desc *d;
  bool write_back;
};
int with_views(std::initializer_list<ViewArg> views, const std::function<int()> &body);

// the descriptor rules of the whole-matrix routines
int resident_whole(const char *what, const chol_desc *d);
bool same_geometry(const chol_desc *a, const chol_desc *b);
// b has a's rows: its order, tile size, stored tile edge and dtype (a right-hand side of a, or a vector over its rows)
CHOL_LOCAL bool same_rows(const chol_desc *a, const chol_desc *b);
TileGeo geo_of(const chol_desc *d);

// the context holds the inverses of at most 32 diagonal 128-blocks (tiles up to 4096): every entry
// that factors, inverts or solves with a tile checks this before any launch writes winv
bool winv_fits(const chol_desc *d);
#define CHECK_WINV(d, what) \
  if (!winv_fits(d)) return failf(CHOL_ERR_NOT_SUPPORTED, "%s: tile size above 4096", what)
void forget_winv(const void *ptr);  // (a tile that is overwritten: its cached block inverses are stale)

// chol_potrf_tile after its argument checks, on the descriptor's image as it stands
int potrf_run(int uplo, chol_desc *A);
// the stored tiles of a square matrix transposed in place on ST_MAIN, by its dtype
void transpose_storage(chol_desc *A);
// body() on the Lower orientation of the square matrices `ds`.  Lower: the body and nothing else.  Upper (A = U^T U
// with U = L^T): every storage flipped, in the order given, before the body and again after it -- also after a body
// that failed: the other triangle comes back as it was -- then ST_MAIN synchronised.  wait = false leaves that
// synchronisation out, for a caller whose next work on the stream follows.  -> the body's status
CHOL_LOCAL int through_lower(bool upper, std::initializer_list<chol_desc *> ds, const std::function<int()> &body,
                        bool wait = true, void (*flip)(chol_desc *) = transpose_storage);

// a whole-matrix descriptor's trailing update: its local tile matrix (the segments of its work list that hold the
// tiles of columns [jlo, jhi): cholmi_internal.h, col_range), and a panel whose tiles lie one after another from
// `base` (tile `first` at base)
LocalMat whole_local_mat(const chol_desc *d);
inline PanelRef one_panel(const void *base, int first = 0) {
  PanelRef pan = {};
  pan.P = 1;
  pan.base[0] = base;
  pan.first[0] = first;
  return pan;
}

// spd.hip, batched.hip: their scratch, freed by chol_finalize
void spd_release();
void batched_release();

}  // namespace cholmi
