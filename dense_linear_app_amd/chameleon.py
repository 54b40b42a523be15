"""Chameleon-shaped Python surface over libcholmi.so.

Names follow the Chameleon C API the reference calls (chameleon.h is not in the
reference tree; call sites: worker_distrib.cpp:78, 238, 256, 323, 416, 511, 589 and
v6_test.c:41-56, 90-93), so reference-side code reads the same:

    CHAMELEON_Init(ncpu, ngpu)
    desc = CHAMELEON_Desc_Create(mat, ChamRealDouble, mb, nb, bsiz, lm, ln, i, j, m, n, p, q)
    info = CHAMELEON_dpotrf_Tile(ChamLower, desc)

`mat` may be None (library-owned HBM tile storage), a numpy array (host buffer, staged
around every call like the worker's blobs) or an int / torch tensor (device pointer,
tiles stay resident).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CholmiError, check, lib

ChamRealFloat, ChamRealDouble = 2, 3
ChamNoTrans, ChamTrans = 111, 112
ChamUpper, ChamLower, ChamUpperLower = 121, 122, 123
ChamOneNorm, ChamFrobeniusNorm, ChamInfNorm, ChamMaxNorm = 171, 174, 175, 177
ChamNonUnit, ChamUnit = 131, 132
ChamLeft, ChamRight = 141, 142

_NP_OF = {ChamRealDouble: np.float64, ChamRealFloat: np.float32}


def CHAMELEON_Init(ncpu: int, ngpu: int) -> None:
    """W2:589 / V6:41.  Raises CholmiError(CHOL_ERR_NO_GPU) when no GPU is usable."""
    check("chol_init", lib().chol_init(int(ncpu), int(ngpu)))


def CHAMELEON_Finalize() -> None:
    """V6:93."""
    check("chol_finalize", lib().chol_finalize())


def set_device(device: int) -> None:
    check("chol_set_device", lib().chol_set_device(int(device)))


def set_rank(rank: int, nranks: int) -> None:
    check("chol_set_rank", lib().chol_set_rank(int(rank), int(nranks)))


def _ptr_of(mat):
    """-> (address or None, keepalive object)"""
    if mat is None:
        return None, None
    if isinstance(mat, np.ndarray):
        if not (mat.flags.f_contiguous or mat.flags.c_contiguous):
            raise ValueError("descriptor buffers must be contiguous")
        return mat.ctypes.data, mat
    if isinstance(mat, int):
        return mat, None
    if hasattr(mat, "data_ptr"):  # torch tensor
        return mat.data_ptr(), mat
    if isinstance(mat, (bytearray, memoryview)):
        buf = (C.c_char * len(mat)).from_buffer(mat)
        return C.addressof(buf), (mat, buf)
    raise TypeError(f"unsupported descriptor buffer type {type(mat)!r}")


class Desc:
    """CHAM_desc_t handle.  Destroyed explicitly (CHAMELEON_Desc_Destroy) or on GC."""

    def __init__(self, mat, dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q):
        addr, self._keep = _ptr_of(mat)
        h = C.c_void_p()
        check("chol_desc_create",
              lib().chol_desc_create(C.byref(h), addr, dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q))
        self._h = h
        self.dtype, self.mb, self.nb, self.bsiz = dtype, mb, nb, bsiz
        if (i, j, m, n) != (0, 0, lm, ln):
            # a sub-matrix view (library-owned storage): everything below works in view coordinates
            lm, ln = m, n
        self.lm, self.ln, self.m, self.n, self.p, self.q = lm, ln, m, n, p, q
        self.mt, self.nt = (lm + mb - 1) // mb, (ln + nb - 1) // nb

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("descriptor already destroyed")
        return self._h

    @property
    def np_dtype(self):
        return _NP_OF[self.dtype]

    def destroy(self):
        if self._h is not None:
            h, self._h = self._h, None
            lib().chol_desc_destroy(C.byref(h))
            self._keep = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- resident-matrix helpers (extensions; Chameleon's Lapack_to_Tile / Tile_to_Lapack)
    def local_ptr(self) -> tuple[int, int]:
        n = C.c_size_t()
        p = lib().chol_desc_local_ptr(self.handle, C.byref(n))
        return int(p or 0), int(n.value)

    def set_version(self, version: int) -> None:
        """Name the content behind this 1-tile descriptor's device buffer (chol_desc_set_version)."""
        check("chol_desc_set_version", lib().chol_desc_set_version(self._h, C.c_ulonglong(int(version) & (2 ** 64 - 1))))

    def local_tiles(self) -> tuple[int, int]:
        a, b = C.c_int(), C.c_int()
        check("chol_desc_local_tiles", lib().chol_desc_local_tiles(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def from_lapack(self, A: np.ndarray) -> None:
        A = np.asfortranarray(A, dtype=self.np_dtype)
        check("chol_lapack_to_tile", lib().chol_lapack_to_tile(A.ctypes.data, A.shape[0], self.handle))

    def to_lapack(self) -> np.ndarray:
        A = np.zeros((self.lm, self.ln), dtype=self.np_dtype, order="F")
        check("chol_tile_to_lapack", lib().chol_tile_to_lapack(self.handle, A.ctypes.data, A.shape[0]))
        return A

    def upload_tile(self, I: int, J: int, tile: np.ndarray) -> None:
        t = np.asfortranarray(tile, dtype=self.np_dtype)
        assert t.size == self.bsiz
        check("chol_tile_upload", lib().chol_tile_upload(self.handle, I, J, t.ctypes.data))

    def download_tile(self, I: int, J: int) -> np.ndarray:
        t = np.empty((self.mb, self.nb), dtype=self.np_dtype, order="F")
        check("chol_tile_download", lib().chol_tile_download(self.handle, I, J, t.ctypes.data))
        return t


def CHAMELEON_Desc_Create(mat, dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q) -> Desc:
    """W2:78, V6:44."""
    return Desc(mat, dtype, mb, nb, bsiz, lm, ln, i, j, m, n, p, q)


def CHAMELEON_Desc_Destroy(desc: Desc) -> None:
    """W2:256, V6:90."""
    desc.destroy()


def CHAMELEON_dpotrf_Tile(uplo: int, A: Desc) -> int:
    """W2:238, V6:56.  Returns info (0, or 1-based index of the first bad pivot)."""
    return check("chol_potrf_tile", lib().chol_potrf_tile(uplo, A.handle))


def CHAMELEON_dtrsm_Tile(side, uplo, trans, diag, alpha: float, A: Desc, B: Desc) -> int:
    """W2:323."""
    return check("chol_trsm_tile", lib().chol_trsm_tile(side, uplo, trans, diag, alpha, A.handle, B.handle))


def CHAMELEON_dsyrk_Tile(uplo, trans, alpha: float, A: Desc, beta: float, Cd: Desc) -> int:
    """W2:416."""
    return check("chol_syrk_tile", lib().chol_syrk_tile(uplo, trans, alpha, A.handle, beta, Cd.handle))


def CHAMELEON_dgemm_Tile(transA, transB, alpha: float, A: Desc, B: Desc, beta: float, Cd: Desc) -> int:
    """W2:511."""
    return check("chol_gemm_tile",
                 lib().chol_gemm_tile(transA, transB, alpha, A.handle, B.handle, beta, Cd.handle))


# single-precision names map to the same entry points (type comes from the descriptor)
CHAMELEON_spotrf_Tile = CHAMELEON_dpotrf_Tile
CHAMELEON_strsm_Tile = CHAMELEON_dtrsm_Tile
CHAMELEON_ssyrk_Tile = CHAMELEON_dsyrk_Tile
CHAMELEON_sgemm_Tile = CHAMELEON_dgemm_Tile


def CHAMELEON_dplgsy_Tile(bump: float, uplo: int, A: Desc, seed: int) -> int:
    """V6:46."""
    return check("chol_plgsy_tile", lib().chol_plgsy_tile(float(bump), uplo, A.handle, int(seed)))


CHAMELEON_splgsy_Tile = CHAMELEON_dplgsy_Tile


# -- the validation block of the reference driver (V6:51, 72-86)
def CHAMELEON_dlacpy_Tile(uplo: int, A: Desc, B: Desc) -> int:
    """V6:51, 79: B <- A on the `uplo` part (ChamUpperLower: everything)."""
    return check("chol_lacpy_tile", lib().chol_lacpy_tile(uplo, A.handle, B.handle))


def CHAMELEON_dlange_Tile(norm: int, A: Desc) -> float:
    """V6:74, 85.  Returns the norm, as Chameleon does."""
    r = C.c_double()
    check("chol_lange_tile", lib().chol_lange_tile(norm, A.handle, C.byref(r)))
    return r.value


def CHAMELEON_dlauum_Tile(uplo: int, A: Desc) -> int:
    """V6:80: tril(A) <- tril(L^T L) with L = tril(A)  (ChamLower)."""
    return check("chol_lauum_tile", lib().chol_lauum_tile(uplo, A.handle))


def CHAMELEON_dgeadd_Tile(trans: int, alpha: float, A: Desc, beta: float, B: Desc) -> int:
    """V6:83: B <- alpha A + beta B."""
    return check("chol_geadd_tile", lib().chol_geadd_tile(trans, float(alpha), A.handle, float(beta), B.handle))


def CHAMELEON_dpotrs_Tile(uplo: int, A: Desc, B: Desc) -> int:
    """B <- A^{-1} B with A = L L^T already factored by CHAMELEON_dpotrf_Tile (ChamLower)."""
    return check("chol_potrs_tile", lib().chol_potrs_tile(uplo, A.handle, B.handle))


def CHAMELEON_dposv_Tile(uplo: int, A: Desc, B: Desc) -> int:
    """Factor A and solve A X = B in place of B.  Returns info (> 0: A is not positive definite)."""
    return check("chol_posv_tile", lib().chol_posv_tile(uplo, A.handle, B.handle))


def CHAMELEON_dsposv_Tile(uplo: int, A: Desc, B: Desc, X: Desc) -> tuple[int, int]:
    """Mixed-precision solve (LAPACK DSPOSV): fp32 factor of A, fp64 iterative refinement of X; only the `uplo`
    triangle of A is read and B is never written.  Returns (info, iter): iter >= 0 is the number of refinement
    steps (A unchanged); iter < 0 (-2 fp32 overflow, -3 fp32 factor not SPD, -31 no convergence) means X was
    solved by dposv in fp64, A then holds the fp64 factor and info > 0 says A is not positive definite."""
    it = C.c_int()
    info = check("chol_dsposv_tile", lib().chol_dsposv_tile(uplo, A.handle, B.handle, X.handle, C.byref(it)))
    return info, it.value


def last_dsposv_stats() -> dict:
    """Phases of the last CHAMELEON_dsposv_Tile [ms] (chol_last_dsposv_stats)."""
    v = (C.c_double * 8)()
    check("chol_last_dsposv_stats", lib().chol_last_dsposv_stats(v))
    return {"total_ms": v[0], "convert_ms": v[1], "factor_ms": v[2], "solve_ms": v[3], "residual_ms": v[4],
            "solves": int(v[5]), "residuals": int(v[6])}


def CHAMELEON_dtrtri_Tile(uplo: int, diag: int, A: Desc) -> int:
    """LAPACK DTRTRI: the `uplo` triangle of A <- its inverse, in place (diag must be ChamNonUnit).  Returns info
    (> 0: A(info, info) is exactly zero, A unchanged)."""
    return check("chol_trtri_tile", lib().chol_trtri_tile(uplo, diag, A.handle))


def CHAMELEON_dpotri_Tile(uplo: int, A: Desc) -> int:
    """LAPACK DPOTRI: A holds the Cholesky factor of CHAMELEON_dpotrf_Tile; its `uplo` triangle <- that of inv(A).
    Returns info (> 0: a zero on the factor's diagonal, A unchanged)."""
    return check("chol_potri_tile", lib().chol_potri_tile(uplo, A.handle))


def CHAMELEON_dpoinv_Tile(uplo: int, A: Desc) -> int:
    """Chameleon poinv: the `uplo` triangle of A <- that of inv(A) (potrf, then potri).  Returns potrf's info
    (> 0: A is not positive definite)."""
    return check("chol_poinv_tile", lib().chol_poinv_tile(uplo, A.handle))


def CHAMELEON_dlansy_Tile(norm: int, uplo: int, A: Desc) -> float:
    """LAPACK DLANSY: the norm of the symmetric matrix whose `uplo` triangle A stores (ChamMaxNorm, ChamOneNorm,
    ChamInfNorm, ChamFrobeniusNorm).  Returns the norm, as CHAMELEON_dlange_Tile does."""
    r = C.c_double()
    check("chol_lansy_tile", lib().chol_lansy_tile(norm, uplo, A.handle, C.byref(r)))
    return r.value


def CHAMELEON_dpocon_Tile(uplo: int, A: Desc, anorm: float) -> float:
    """LAPACK DPOCON: A holds the factor of CHAMELEON_dpotrf_Tile(uplo, .), anorm = ||A||_1 of the original matrix
    (CHAMELEON_dlansy_Tile).  Returns rcond, the reciprocal 1-norm condition estimate (0: a zero on the factor's
    diagonal, anorm = 0 or +Inf, or a sweep that overflowed)."""
    r = C.c_double()
    check("chol_pocon_tile", lib().chol_pocon_tile(uplo, A.handle, float(anorm), C.byref(r)))
    return r.value


def last_pocon_stats() -> dict:
    """The last CHAMELEON_dpocon_Tile (chol_last_pocon_stats): total and sweep time [ms], applications of A^{-1}."""
    v = (C.c_double * 4)()
    check("chol_last_pocon_stats", lib().chol_last_pocon_stats(v))
    return {"total_ms": v[0], "sweep_ms": v[1], "applications": int(v[2])}


# LAPACK's FACT / EQUED characters <-> the C ABI's codes (CHOL_FACT_*, *equed 0 / 1)
FACT_CODES = {"N": 0, "E": 1, "F": 2}
EQUED_CODES = {"N": 0, "Y": 1}


def fact_code(fact: str) -> int:
    """'N' / 'E' / 'F' (any case) -> CHOL_FACT_NONE / _EQUILIBRATE / _FACTORED."""
    try:
        return FACT_CODES[str(fact).upper()]
    except KeyError:
        raise ValueError(f"fact must be 'N', 'E' or 'F', not {fact!r}") from None


def equed_code(equed: str) -> int:
    """'N' / 'Y' (any case) -> 0 / 1."""
    try:
        return EQUED_CODES[str(equed).upper()]
    except KeyError:
        raise ValueError(f"equed must be 'N' or 'Y', not {equed!r}") from None


def equed_char(code: int) -> str:
    """0 / 1 -> 'N' / 'Y'."""
    return {0: "N", 1: "Y"}[int(code)]


def CHAMELEON_dpoequ_Tile(A: Desc, S: Desc) -> tuple[int, float, float]:
    """LAPACK DPOEQU: S (n x 1) <- 1/sqrt(A(i,i)).  Returns (info, scond, amax); info = i > 0 for the first
    A(i,i) <= 0 (S then unspecified)."""
    sc, am = C.c_double(), C.c_double()
    info = check("chol_poequ_tile", lib().chol_poequ_tile(A.handle, S.handle, C.byref(sc), C.byref(am)))
    return info, sc.value, am.value


def CHAMELEON_dlaqsy_Tile(uplo: int, A: Desc, S: Desc, scond: float, amax: float) -> str:
    """LAPACK DLAQSY: scale the `uplo` triangle of A by S when scond < 0.1 or amax is out of range.  Returns equed,
    'Y' (A scaled) or 'N' (A untouched)."""
    e = C.c_int()
    check("chol_laqsy_tile", lib().chol_laqsy_tile(uplo, A.handle, S.handle, float(scond), float(amax), C.byref(e)))
    return equed_char(e.value)


def CHAMELEON_dporfs_Tile(uplo: int, A: Desc, AF: Desc, B: Desc, X: Desc) -> tuple[int, np.ndarray, np.ndarray]:
    """LAPACK DPORFS: refine X in place (AF the factor of A).  Returns (info, ferr, berr), one bound per column."""
    nrhs = B.ln
    ferr, berr = np.zeros(nrhs), np.zeros(nrhs)
    dp = C.POINTER(C.c_double)
    info = check("chol_porfs_tile", lib().chol_porfs_tile(uplo, A.handle, AF.handle, B.handle, X.handle,
                                                         ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp)))
    return info, ferr, berr


def CHAMELEON_dposvx_Tile(fact: str, uplo: int, A: Desc, AF: Desc, equed: str, S, B: Desc,
                          X: Desc) -> tuple[int, str, float, np.ndarray, np.ndarray]:
    """LAPACK DPOSVX with fact / equed as LAPACK's characters ('N', 'E', 'F' / 'N', 'Y'; equed is an input for 'F').
    S may be None when it is not used.  Returns (info, equed, rcond, ferr, berr); info = n + 1: rcond < eps."""
    nrhs = B.ln
    ferr, berr = np.zeros(nrhs), np.zeros(nrhs)
    e = C.c_int(equed_code(equed))
    rc = C.c_double()
    dp = C.POINTER(C.c_double)
    info = check("chol_posvx_tile", lib().chol_posvx_tile(fact_code(fact), uplo, A.handle, AF.handle, C.byref(e),
                                                         S.handle if S is not None else None, B.handle, X.handle,
                                                         C.byref(rc), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp)))
    return info, equed_char(e.value), rc.value, ferr, berr


def last_posvx_stats() -> dict:
    """The last CHAMELEON_dposvx_Tile / dporfs_Tile (chol_last_posvx_stats): phases [ms] and the columns to which
    A^{-1} was applied by the multi-vector sweeps and by potrs."""
    v = (C.c_double * 8)()
    check("chol_last_posvx_stats", lib().chol_last_posvx_stats(v))
    return {"total_ms": v[0], "equilibrate_ms": v[1], "factor_ms": v[2], "rcond_ms": v[3], "solve_ms": v[4],
            "porfs_ms": v[5], "sweep_columns": int(v[6]), "potrs_columns": int(v[7])}


def bench_refine(uplo: int, A: Desc, AF: Desc, X: Desc, path: int, reps: int = 3) -> float:
    """The parts of CHAMELEON_dporfs_Tile alone on X's columns [ms, fastest of reps]: path 0 the residual pass, 1 one
    application of A^{-1} by the multi-vector sweeps, 2 the same by potrs (chol_bench_refine)."""
    r = C.c_double()
    check("chol_bench_refine", lib().chol_bench_refine(uplo, A.handle, AF.handle, X.handle, path, reps, C.byref(r)))
    return r.value


def CHAMELEON_dpstrf_Tile(uplo: int, A: Desc, tol: float = -1.0) -> tuple[int, np.ndarray, int]:
    """LAPACK DPSTRF: P^T A P = L L^T (ChamLower) or U^T U (ChamUpper) with complete pivoting, in the `uplo` triangle
    of A.  tol < 0: n * eps * max(diag(A)).  Returns (info, piv, rank): info 0 (rank = n) or 1 (rank < n), piv the
    1-based np.int32 pivot vector (as scipy.linalg.lapack.dpstrf), rank the number of pivots taken."""
    n = int(A.lm)
    piv = np.zeros(max(n, 1), dtype=np.int32)
    r = C.c_int()
    info = check("chol_pstrf_tile", lib().chol_pstrf_tile(uplo, A.handle, piv.ctypes.data_as(C.POINTER(C.c_int)),
                                                          C.byref(r), float(tol)))
    return info, piv[:n], r.value


def last_pstrf_stats() -> dict:
    """The last CHAMELEON_dpstrf_Tile (chol_last_pstrf_stats): total, pivot-step, row-interchange and trailing-update
    time [ms], and the number of pivot steps."""
    v = (C.c_double * 8)()
    check("chol_last_pstrf_stats", lib().chol_last_pstrf_stats(v))
    return {"total_ms": v[0], "steps_ms": v[1], "laswp_ms": v[2], "update_ms": v[3], "steps": int(v[4])}


def CHAMELEON_dsygst_Tile(itype: int, uplo: int, A: Desc, B: Desc) -> int:
    """LAPACK DSYGST with itype 1: the `uplo` triangle of A <- that of inv(L) A inv(L)^T (ChamLower, B = L L^T) or
    inv(U^T) A inv(U) (ChamUpper, B = U^T U), B the factor chol_potrf_tile returned.  Returns 0, or info > 0: the
    1-based index of a zero on B's diagonal (A unchanged).  itype 2 and 3 raise (CHOL_ERR_NOT_SUPPORTED)."""
    return check("chol_sygst_tile", lib().chol_sygst_tile(itype, uplo, A.handle, B.handle))


def last_sygst_stats() -> dict:
    """The last CHAMELEON_dsygst_Tile (chol_last_sygst_stats): total, diagonal-tile inverses, chain (diagonal tiles,
    panel TRSM, the two SYMMs), rank-2k updates and deferred-solve time [ms], and the number of steps."""
    v = (C.c_double * 8)()
    check("chol_last_sygst_stats", lib().chol_last_sygst_stats(v))
    return {"total_ms": v[0], "diag_inv_ms": v[1], "chain_ms": v[2], "syr2k_ms": v[3], "solve_ms": v[4],
            "steps": int(v[5])}


def CHAMELEON_dchud_Tile(uplo: int, A: Desc, V: Desc) -> int:
    """LINPACK DCHUD for r vectors (MATLAB cholupdate): A, the factor chol_potrf_tile(uplo, .) returned, <- the factor
    of L L^T + V V^T in O(n^2 r) operations; V (n x r) is workspace and is overwritten.  Returns 0, or info > 0: the
    1-based index of a zero on the factor's diagonal (A and V unchanged)."""
    return check("chol_chud_tile", lib().chol_chud_tile(uplo, A.handle, V.handle))


def CHAMELEON_dchdd_Tile(uplo: int, A: Desc, V: Desc) -> int:
    """LINPACK DCHDD for r vectors: A <- the factor of L L^T - V V^T; V (n x r) is workspace.  Returns 0, or info > 0:
    a zero at L(info, info) (A and V unchanged), or the leading minor of order info of L L^T - V V^T is not positive
    definite (A and V unspecified: keep a copy of the factor if it is needed)."""
    return check("chol_chdd_tile", lib().chol_chdd_tile(uplo, A.handle, V.handle))


def last_chud_stats() -> dict:
    """The last CHAMELEON_dchud_Tile / dchdd_Tile (chol_last_chud_stats): total, chain (generators and in-tile
    appliers) and bulk applier time [ms], r, the passes over the matrix, and the vector at which a downdate stopped
    (-1: none)."""
    v = (C.c_double * 8)()
    check("chol_last_chud_stats", lib().chol_last_chud_stats(v))
    return {"total_ms": v[0], "chain_ms": v[1], "bulk_ms": v[2], "r": int(v[3]), "passes": int(v[4]),
            "stop_vector": int(v[5])}


def CHAMELEON_dchex_Tile(uplo: int, A: Desc, k: int, l: int, job: int) -> int:
    """LINPACK DCHEX without Z: A, the factor chol_potrf_tile(uplo, .) returned of a matrix M, <- the factor of
    P^T M P, P the circular shift of the variables k..l (1-based): job 1 moves variable l up to position k, job 2 moves
    variable k down to position l, in O(n (l - k)) operations.  To delete variable k: job 2 with l = n, then the
    leading (n-1) x (n-1) view holds the factor without it.  Returns 0, or info > 0: the 1-based index of a zero on the
    factor's diagonal (A unchanged), or the column at which non-finite data stopped a rotation (A unspecified)."""
    return check("chol_chex_tile", lib().chol_chex_tile(uplo, A.handle, k, l, job))


def last_chex_stats() -> dict:
    """The last CHAMELEON_dchex_Tile (chol_last_chex_stats): total, data movement, chain (job 2: generators and
    in-tile appliers; job 1: the coefficient chain) and bulk applier time [ms], the job and l - k."""
    v = (C.c_double * 8)()
    check("chol_last_chex_stats", lib().chol_last_chex_stats(v))
    return {"total_ms": v[0], "move_ms": v[1], "chain_ms": v[2], "bulk_ms": v[3], "job": int(v[4]), "l_minus_k": int(v[5])}


def CHAMELEON_dtrtrs_Tile(uplo: int, trans: int, diag: int, A: Desc, B: Desc) -> int:
    """LAPACK DTRTRS: B <- inv(op(T)) B, T the `uplo` triangle of A (the factor chol_potrf_tile(uplo, .) returned), op
    the transpose for ChamTrans; A is only read.  Returns 0, or info > 0: the 1-based index of a zero on the diagonal
    (B unchanged).  ChamUnit raises (CHOL_ERR_NOT_SUPPORTED)."""
    return check("chol_trtrs_tile", lib().chol_trtrs_tile(uplo, trans, diag, A.handle, B.handle))


def CHAMELEON_dtrmm_Tile(side: int, uplo: int, trans: int, diag: int, alpha: float, A: Desc, B: Desc) -> int:
    """BLAS DTRMM, side ChamLeft: B <- alpha op(T) B in place, T the `uplo` triangle of A; A is only read.  ChamRight
    and ChamUnit raise (CHOL_ERR_NOT_SUPPORTED)."""
    return check("chol_trmm_tile", lib().chol_trmm_tile(side, uplo, trans, diag, float(alpha), A.handle, B.handle))


def CHAMELEON_dlogdet_Tile(A: Desc) -> tuple[int, float]:
    """(info, 2 sum_j log A(j,j)): log det(L L^T) from the diagonal of the factor A, summed in fp64 in a fixed order.
    info > 0: the 1-based index of the first diagonal entry that is <= 0 or NaN (the value is then unspecified)."""
    v = C.c_double(0.0)
    info = check("chol_logdet_tile", lib().chol_logdet_tile(A.handle, C.byref(v)))
    return info, v.value


def last_trtrs_stats() -> dict:
    """The last CHAMELEON_dtrtrs_Tile / dtrmm_Tile (chol_last_trtrs_stats): total, diagonal-tile staging and sweep or
    product time [ms], and the columns that took the narrow and the wide path."""
    v = (C.c_double * 8)()
    check("chol_last_trtrs_stats", lib().chol_last_trtrs_stats(v))
    return {"total_ms": v[0], "stage_ms": v[1], "work_ms": v[2], "narrow_cols": int(v[3]), "wide_cols": int(v[4])}


def half_limits(trtrs_cols: int = -1, trmm_cols: int = -1) -> None:
    """Diagnostic: the widest trtrs / trmm call that takes the narrow path (negative: the built-in limit)."""
    check("chol_debug_half_limits", lib().chol_debug_half_limits(trtrs_cols, trmm_cols))


def CHAMELEON_dsymm_Tile(side: int, uplo: int, alpha: float, A: Desc, B: Desc, beta: float, C: Desc) -> int:
    """BLAS DSYMM, side ChamLeft: C <- alpha A B + beta C for the symmetric A of which only the `uplo` triangle is read
    (the other strict triangle may hold anything); B and C n x nrhs, any nrhs.  A and B are only read, B may be A, C
    must not alias either.  beta == 0: C is not read; alpha == 0: A and B are not read.  ChamRight raises
    (CHOL_ERR_NOT_SUPPORTED)."""
    return check("chol_symm_tile", lib().chol_symm_tile(side, uplo, float(alpha), A.handle, B.handle, float(beta), C.handle))


def last_symm_stats() -> dict:
    """The last CHAMELEON_dsymm_Tile (chol_last_symm_stats): total and kernel time [ms], nrhs, the column width of a
    workgroup's block of C (0: alpha == 0), the number of workgroups and the flop count 2 n^2 nrhs."""
    v = (C.c_double * 8)()
    check("chol_last_symm_stats", lib().chol_last_symm_stats(v))
    return {"total_ms": v[0], "kernel_ms": v[1], "nrhs": int(v[2]), "block_cols": int(v[3]), "workgroups": int(v[4]),
            "flops": v[5]}


def CHAMELEON_dsytrf_nopiv_Tile(uplo: int, A: Desc) -> int:
    """A = L D L^T (ChamLower) or U^T D U (ChamUpper) without pivoting, for symmetric matrices whose factorisation
    needs none (quasi-definite, diagonally dominant): on return D on the diagonal of A and the unit triangular factor
    in the strict `uplo` triangle.  Returns 0, or info > 0: the 1-based index of the first pivot that is exactly zero
    or not finite.  A negative pivot is not an error; last_sytrf_stats() reports the inertia and the growth."""
    return check("chol_sytrf_nopiv_tile", lib().chol_sytrf_nopiv_tile(uplo, A.handle))


def CHAMELEON_dsytrs_nopiv_Tile(uplo: int, A: Desc, B: Desc) -> int:
    """B <- inv(A) B from the factor CHAMELEON_dsytrf_nopiv_Tile(uplo, A) returned; A is only read.  Returns 0, or
    info > 0: the 1-based index of a zero on the stored diagonal (B unchanged)."""
    return check("chol_sytrs_nopiv_tile", lib().chol_sytrs_nopiv_tile(uplo, A.handle, B.handle))


def CHAMELEON_dsysv_nopiv_Tile(uplo: int, A: Desc, B: Desc) -> int:
    """Factor A = L D L^T without pivoting and solve A X = B in place of B.  Returns info (> 0: a zero or non-finite
    pivot, B untouched)."""
    return check("chol_sysv_nopiv_tile", lib().chol_sysv_nopiv_tile(uplo, A.handle, B.handle))


def last_sytrf_stats() -> dict:
    """The last CHAMELEON_dsytrf_nopiv_Tile (chol_last_sytrf_stats): total, chain (diagonal tiles, panel TRSM, scaling)
    and trailing-update time [ms]; the inertia (number of positive, of negative pivots; the padding of a ragged order
    is not counted); min |d|, max |d| and max |L| over the strict triangle -- what shows an unstable run."""
    v = (C.c_double * 8)()
    check("chol_last_sytrf_stats", lib().chol_last_sytrf_stats(v))
    return {"total_ms": v[0], "chain_ms": v[1], "update_ms": v[2], "inertia": (int(v[3]), int(v[4])),
            "min_abs_d": v[5], "max_abs_d": v[6], "max_abs_l": v[7]}


def CHAMELEON_drbt_apply_Tile(uplo: int, A: Desc, W: Desc, depth: int) -> int:
    """A <- W^T A W on the `uplo` triangle, W the recursive butterfly of `depth` (1 or 2) levels whose diagonal
    entries are the columns of the n x depth descriptor W; n a multiple of 2^depth."""
    return check("chol_rbt_apply_tile", lib().chol_rbt_apply_tile(uplo, A.handle, W.handle, depth))


def CHAMELEON_dsytrf_rbt_Tile(uplo: int, A: Desc, W: Desc, depth: int = 2, seed: int = 1) -> int:
    """The factorisation for general symmetric indefinite matrices: W filled from `seed` (seed = 0: W as given),
    A <- W^T A W, then A = L D L^T without pivoting.  Returns info as CHAMELEON_dsytrf_nopiv_Tile does (of the
    transformed matrix); last_sytrf_stats() reports the inertia and the growth, last_rbt_stats() the phases."""
    return check("chol_sytrf_rbt_tile", lib().chol_sytrf_rbt_tile(uplo, A.handle, W.handle, depth, seed))


def CHAMELEON_dsytrs_rbt_Tile(uplo: int, A: Desc, W: Desc, depth: int, B: Desc) -> int:
    """B <- W inv(L D L^T) W^T B from what CHAMELEON_dsytrf_rbt_Tile left in A and W; both are only read."""
    return check("chol_sytrs_rbt_tile", lib().chol_sytrs_rbt_tile(uplo, A.handle, W.handle, depth, B.handle))


def CHAMELEON_dsysv_rbt_Tile(uplo: int, A: Desc, AF: Desc, W: Desc, depth: int, seed: int, B: Desc, X: Desc):
    """A X = B for a general symmetric indefinite A (fp64): the butterfly-randomised factorisation of a copy AF, the
    solve, and refinement against the untouched A.  Returns (info, iter, berr): info 0, the factorisation's info
    (iter = -3) or n + 1 (iter = -31: no convergence in 10 steps); iter the refinement steps; berr the final
    max |R(:,j)| / (||A||_inf max |X(:,j)|) of every column."""
    it = C.c_int(0)
    berr = (C.c_double * max(1, B.n))()
    info = check("chol_sysv_rbt_tile", lib().chol_sysv_rbt_tile(uplo, A.handle, AF.handle, W.handle, depth, seed, B.handle,
                                                                X.handle, C.byref(it), berr))
    return info, it.value, [berr[j] for j in range(B.n)]


def last_rbt_stats() -> dict:
    """The last butterfly routine (chol_last_rbt_stats) [ms]: total, generation of W, the transformation of A, the
    factorisation, the solves, the residual passes, the vector butterflies; then the refinement steps."""
    v = (C.c_double * 8)()
    check("chol_last_rbt_stats", lib().chol_last_rbt_stats(v))
    return {"total_ms": v[0], "gen_ms": v[1], "transform_ms": v[2], "factor_ms": v[3], "solve_ms": v[4],
            "resid_ms": v[5], "vec_ms": v[6], "steps": int(v[7])}


CHAMELEON_spotrs_Tile = CHAMELEON_dpotrs_Tile
CHAMELEON_sposv_Tile = CHAMELEON_dposv_Tile
CHAMELEON_slacpy_Tile = CHAMELEON_dlacpy_Tile
CHAMELEON_slange_Tile = CHAMELEON_dlange_Tile
CHAMELEON_slauum_Tile = CHAMELEON_dlauum_Tile
CHAMELEON_sgeadd_Tile = CHAMELEON_dgeadd_Tile
CHAMELEON_strtri_Tile = CHAMELEON_dtrtri_Tile
CHAMELEON_spotri_Tile = CHAMELEON_dpotri_Tile
CHAMELEON_spoinv_Tile = CHAMELEON_dpoinv_Tile
CHAMELEON_slansy_Tile = CHAMELEON_dlansy_Tile
CHAMELEON_spocon_Tile = CHAMELEON_dpocon_Tile
CHAMELEON_spoequ_Tile = CHAMELEON_dpoequ_Tile
CHAMELEON_slaqsy_Tile = CHAMELEON_dlaqsy_Tile
CHAMELEON_sporfs_Tile = CHAMELEON_dporfs_Tile
CHAMELEON_sposvx_Tile = CHAMELEON_dposvx_Tile
CHAMELEON_spstrf_Tile = CHAMELEON_dpstrf_Tile
CHAMELEON_ssygst_Tile = CHAMELEON_dsygst_Tile
CHAMELEON_schud_Tile = CHAMELEON_dchud_Tile
CHAMELEON_schdd_Tile = CHAMELEON_dchdd_Tile
CHAMELEON_schex_Tile = CHAMELEON_dchex_Tile
CHAMELEON_strtrs_Tile = CHAMELEON_dtrtrs_Tile
CHAMELEON_strmm_Tile = CHAMELEON_dtrmm_Tile
CHAMELEON_slogdet_Tile = CHAMELEON_dlogdet_Tile
CHAMELEON_ssymm_Tile = CHAMELEON_dsymm_Tile
CHAMELEON_ssytrf_nopiv_Tile = CHAMELEON_dsytrf_nopiv_Tile
CHAMELEON_ssytrs_nopiv_Tile = CHAMELEON_dsytrs_nopiv_Tile
CHAMELEON_ssysv_nopiv_Tile = CHAMELEON_dsysv_nopiv_Tile
CHAMELEON_srbt_apply_Tile = CHAMELEON_drbt_apply_Tile
CHAMELEON_ssytrf_rbt_Tile = CHAMELEON_dsytrf_rbt_Tile
CHAMELEON_ssytrs_rbt_Tile = CHAMELEON_dsytrs_rbt_Tile
CHAMELEON_ssysv_rbt_Tile = CHAMELEON_dsysv_rbt_Tile


def residual_plgsy(L: Desc, bump: float, seed: int) -> float:
    """||tril(L)tril(L)^T - A||_F/||A||_F with A regenerated on the device (what V6:72-87 meant)."""
    r = C.c_double()
    check("chol_residual_plgsy", lib().chol_residual_plgsy(L.handle, float(bump), int(seed), C.byref(r)))
    return r.value


def residual_plgsy_inf(L: Desc, bump: float, seed: int) -> float:
    """||A - L L^T||_inf / ||A||_inf: the number V6:86 prints, computed correctly on the device."""
    r = C.c_double()
    check("chol_residual_plgsy_inf", lib().chol_residual_plgsy_inf(L.handle, float(bump), int(seed), C.byref(r)))
    return r.value


def last_potrf_stats() -> dict:
    t, u, f = C.c_double(), C.c_double(), C.c_double()
    n = C.c_int()
    lib().chol_last_potrf_stats(C.byref(t), C.byref(u), C.byref(n), C.byref(f))
    return {"total_ms": t.value, "update_ms": u.value, "update_launches": n.value, "update_flops": f.value}


REGIME_NAMES = ("paired", "plain", "halves", "counter_linked", "near_column", "flow", "yielding", "column_latency_form")


def last_potrf_regimes() -> dict:
    """How many waves of the last whole-matrix factorisation ran in which regime of the walker (chol_last_potrf_regimes):
    paired / plain / halves / near_column partition the waves that have an update; the others are attributes."""
    v, nt = (C.c_int * 8)(), C.c_int()
    lib().chol_last_potrf_regimes(v, C.byref(nt))
    d = {k: int(v[i]) for i, k in enumerate(REGIME_NAMES)}
    d["waves"] = int(nt.value)
    return d


def mfma_probe(dtype: int = ChamRealDouble, waves_per_simd: int = 1) -> float:
    """TFLOP/s of a register-only MFMA stream on every CU (sustained matrix-core ceiling)."""
    r = C.c_double()
    check("chol_mfma_probe", lib().chol_mfma_probe(dtype, waves_per_simd, C.byref(r)))
    return r.value


def bench_update(desc: Desc, k: int = 0, ablate: int = 0, reps: int = 3) -> tuple[float, float]:
    """(ms, TFLOP/s) of wave k's trailing-update launch alone (diagnostic; modifies the matrix)."""
    ms, fl = C.c_double(), C.c_double()
    check("chol_bench_update", lib().chol_bench_update(desc.handle, k, ablate, reps, C.byref(ms), C.byref(fl)))
    return ms.value, fl.value / (ms.value * 1e-3) / 1e12


def calibration() -> list:
    """[fp64 MFMA probe TFLOP/s, fp64 diagonal-block step us, fp32 ..., fp32 ...] + the four derived figures the
    walker's regime switches use (chol_debug_calibration)."""
    out = (C.c_double * 8)()
    check("chol_debug_calibration", lib().chol_debug_calibration(out))
    return list(out)


def update_kernel_name(dtype: int = ChamRealDouble) -> str:
    """Name (as rocprofv3 prints it) of the trailing-update kernel the library launches for `dtype` right now."""
    buf = C.create_string_buffer(96)
    check("chol_debug_update_kernel", lib().chol_debug_update_kernel(dtype, buf, len(buf)))
    return buf.value.decode()


def set_profiling(on: bool) -> None:
    lib().chol_set_profiling(1 if on else 0)


__all__ = [n for n in dir() if n.startswith(("CHAMELEON_", "Cham"))] + [
    "Desc", "CholmiError", "residual_plgsy", "residual_plgsy_inf", "last_potrf_stats", "last_dsposv_stats", "set_profiling", "set_device", "set_rank"]
