"""Batched Cholesky of small matrices on torch device tensors, in place (include/cholmi.h: chol_potrf_batched,
chol_potrs_batched, chol_posv_batched, chol_chud_batched, chol_chdd_batched, chol_trtrs_batched, chol_trmm_batched,
chol_logdet_batched, chol_trtri_batched, chol_potri_batched, chol_poinv_batched, chol_invdiag_batched): 10^3 .. 10^6
independent SPD matrices of order n <= 64.

    info = potrf_batched(A)            A: (batch, n, n) or (n, n), float64 or float32
    info = potrs_batched(A, B)         B: (batch, n) or (batch, n, nrhs)   [(n,) or (n, nrhs) with a 2-d A]
    info = posv_batched(A, B)
    info = chud_batched(A, V)          V: (batch, n) or (batch, n, r), only read: the factors of L L^T + V V^T
    info = chdd_batched(A, V)                                                     the factors of L L^T - V V^T
    info = trtrs_batched(A, B, uplo, trans)     B <- inv(op(T)) B, T the `uplo` triangle of A (a factor), only read
    trmm_batched(A, B, uplo, trans, alpha)      B <- alpha op(T) B
    logdet, info = logdet_batched(A)            log det(L L^T) from the diagonal: a float64 tensor on A's device
    info = trtri_batched(A, uplo)               the stored triangle T <- inv(T)
    info = potri_batched(A, uplo)               the factor's triangle <- that of inv(L L^T)
    info = poinv_batched(A, uplo)               potrf_batched then potri_batched in one pass
    D, info = invdiag_batched(A, uplo)          diag(inv(L L^T)): a new (batch, n) tensor of A's dtype; A only read

Each info is LAPACK's info of every matrix as a numpy int32 array.  The matrices of A are column-major
(stride(-2) == 1, lda = stride(-1)) or row-major (stride(-1) == 1, lda = stride(-2)); `uplo` always speaks of the
mathematical matrix, so for a row-major tensor the other code goes to the library (and the other `trans` as well: a
row-major tensor is the column-major image of the transpose).  The matrices of a 3-d B or V are
column-major (what torch.empty(batch, nrhs, n).mT gives); a row-major one is refused: nothing is copied or transposed
behind the caller's back.  Negative statuses raise CholmiError."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib
from .chameleon import ChamLower, ChamNoTrans, ChamRealDouble, ChamRealFloat, ChamTrans, ChamUpper


def _dtype_code(t, what):
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor")
    if t.dtype == torch.float64:
        return ChamRealDouble
    if t.dtype == torch.float32:
        return ChamRealFloat
    raise ValueError(f"{what} must be float64 or float32, not {t.dtype}")


def _require_device(*tensors):
    """(after the layout rules, which need no device)  The library runs on a stream of its own and is synchronous at
    the boundary: what torch has queued on these tensors finishes first"""
    import torch

    for t in tensors:
        if t.device.type != "cuda" or t.device != tensors[0].device:
            raise ValueError(f"A and B must be device tensors on one device, not on {t.device}")
    torch.cuda.current_stream(tensors[0].device).synchronize()


def _images_of_A(A, uplo):
    """-> (dtype code, uplo for the library, n, lda, strideA, batch)"""
    if uplo not in (ChamLower, ChamUpper):
        raise ValueError("uplo must be ChamLower or ChamUpper")
    dt = _dtype_code(A, "A")
    if A.dim() not in (2, 3) or A.shape[-1] != A.shape[-2]:
        raise ValueError(f"A must be (batch, n, n) or (n, n), not {tuple(A.shape)}")
    n = A.shape[-1]
    batch = A.shape[0] if A.dim() == 3 else 1
    if n <= 1 or A.stride(-2) == 1:  # column-major
        lda, code = (A.stride(-1) if n > 1 else 1), uplo
    elif A.stride(-1) == 1:  # row-major: the transposed images, so the other triangle
        lda, code = A.stride(-2), (ChamUpper if uplo == ChamLower else ChamLower)
    else:
        raise ValueError("the matrices of A must be column-major (stride(-2) == 1) or row-major (stride(-1) == 1)")
    stride = A.stride(0) if A.dim() == 3 and batch > 1 else lda * n
    if lda < max(1, n) or stride < lda * n:
        raise ValueError(f"the matrices of A overlap: strides {tuple(A.stride())} for shape {tuple(A.shape)}")
    return dt, code, n, lda, stride, batch


def _images_of_B(A, B, dt, n, batch, name="B"):
    """-> (nrhs, ldb, strideB); name: what the messages call it (the vectors V of chud_batched follow B's rules)"""
    if _dtype_code(B, name) != dt:
        raise ValueError(f"{name} must have A's dtype")
    lead = tuple(A.shape[:-2])
    if B.dim() == A.dim() - 1 and tuple(B.shape) == lead + (n,):
        nrhs, ldb = 1, max(1, n)
        if n > 1 and B.stride(-1) != 1:
            raise ValueError(f"the vectors of a (batch, n) {name} must be contiguous (stride(-1) == 1)")
    elif B.dim() == A.dim() and tuple(B.shape[:-1]) == lead + (n,):
        nrhs = B.shape[-1]
        if n > 1 and B.stride(-2) != 1:
            if B.stride(-1) == 1:
                raise ValueError(f"{name} is row-major: its matrices must be column-major (stride(-2) == 1), which is "
                                 "what torch.empty(batch, nrhs, n).mT gives; nothing is transposed here")
            raise ValueError(f"the matrices of {name} must be column-major (stride(-2) == 1)")
        ldb = B.stride(-1) if nrhs > 1 else max(1, n)
    else:
        raise ValueError(f"{name} must be {lead + (n,)} or {lead + (n, 'nrhs')}, not {tuple(B.shape)}")
    stride = B.stride(0) if A.dim() == 3 and batch > 1 else ldb * nrhs
    if ldb < max(1, n) or stride < ldb * nrhs:
        raise ValueError(f"the matrices of {name} overlap: strides {tuple(B.stride())} for shape {tuple(B.shape)}")
    return nrhs, ldb, stride


def _info(batch):
    info = np.zeros(batch, dtype=np.int32)
    return info, info.ctypes.data_as(C.POINTER(C.c_int))


def potrf_batched(A, uplo: int = ChamLower) -> np.ndarray:
    """Every matrix of A <- its Cholesky factor in the `uplo` triangle.  -> info (numpy int32, one per matrix)"""
    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    _require_device(A)
    info, pinfo = _info(batch)
    check("chol_potrf_batched", lib().chol_potrf_batched(code, dt, n, A.data_ptr(), lda, sa, batch, pinfo))
    return info


def _solve(name, A, B, uplo):
    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    nrhs, ldb, sb = _images_of_B(A, B, dt, n, batch)
    _require_device(A, B)
    info, pinfo = _info(batch)
    check(name, getattr(lib(), name)(code, dt, n, nrhs, A.data_ptr(), lda, sa, B.data_ptr(), ldb, sb, batch, pinfo))
    return info


def potrs_batched(A, B, uplo: int = ChamLower) -> np.ndarray:
    """B <- inv(A) B from the factors potrf_batched left in A.  info[b] = j: an exact zero at L_jj of matrix b, its B
    untouched"""
    return _solve("chol_potrs_batched", A, B, uplo)


def posv_batched(A, B, uplo: int = ChamLower) -> np.ndarray:
    """potrf_batched and potrs_batched in one pass, the same bits.  info[b] > 0: B of that matrix untouched"""
    return _solve("chol_posv_batched", A, B, uplo)


def _update(name, A, V, uplo):
    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    r, ldv, sv = _images_of_B(A, V, dt, n, batch, "V")
    _require_device(A, V)
    info, pinfo = _info(batch)
    check(name, getattr(lib(), name)(code, dt, n, r, A.data_ptr(), lda, sa, V.data_ptr(), ldv, sv, batch, pinfo))
    return info


def chud_batched(A, V, uplo: int = ChamLower) -> np.ndarray:
    """The factors potrf_batched left in A <- the factors of L L^T + V V^T (LINPACK DCHUD, MATLAB cholupdate, for the
    r columns of V at once; the bits of r calls with one column each).  V is only read.  -> info; info[b] = j > 0: an
    exact zero at L_jj, or a NaN / Inf reached column j; that matrix's A is untouched.

    LINPACK's Z and RHO (a recursive least-squares step: the row x with the observation y joins) need no argument of
    their own: border the matrix with the right-hand side, M = [[A, b], [b^T, c]] of order n + 1 <= 64, factor it,
    and update with the vector (x, y).  The last row of the bordered factor is (z^T, rho): L z = b solves the
    triangular half of the normal equations and rho^2 is the residual sum of squares."""
    return _update("chol_chud_batched", A, V, uplo)


def chdd_batched(A, V, uplo: int = ChamLower) -> np.ndarray:
    """The factors of L L^T - V V^T (LINPACK DCHDD).  info[b] = j > 0: the leading minor of order j of matrix b's
    L L^T - V V^T is not positive definite (or an exact zero at L_jj): that matrix's A is untouched, bit for bit, and
    the others are updated as if it were not there.  The bordered form of chud_batched gives Z and RHO here too."""
    return _update("chol_chdd_batched", A, V, uplo)


def _half_of_A(A, uplo, trans):
    """-> (dtype code, uplo and trans for the library, n, lda, strideA, batch).  `uplo` and `trans` speak of the
    mathematical matrix; a row-major tensor is the column-major image of its transpose, so there BOTH codes flip"""
    if trans not in (ChamNoTrans, ChamTrans):
        raise ValueError("trans must be ChamNoTrans or ChamTrans")
    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    if code != uplo:
        trans = ChamTrans if trans == ChamNoTrans else ChamNoTrans
    return dt, code, trans, n, lda, sa, batch


def trtrs_batched(A, B, uplo: int = ChamLower, trans: int = ChamNoTrans) -> np.ndarray:
    """B <- inv(op(T)) B, T the `uplo` triangle of every matrix of A (what potrf_batched left), op(T) = T or T^T; A is
    only read.  (Lower, NoTrans) then (Lower, Trans) on the same B returns the bits of potrs_batched.  -> info;
    info[b] = j: an exact zero at T_jj of matrix b, its B untouched"""
    dt, code, tr, n, lda, sa, batch = _half_of_A(A, uplo, trans)
    nrhs, ldb, sb = _images_of_B(A, B, dt, n, batch)
    _require_device(A, B)
    info, pinfo = _info(batch)
    check("chol_trtrs_batched", lib().chol_trtrs_batched(code, tr, dt, n, nrhs, A.data_ptr(), lda, sa, B.data_ptr(),
                                                         ldb, sb, batch, pinfo))
    return info


def trmm_batched(A, B, uplo: int = ChamLower, trans: int = ChamNoTrans, alpha: float = 1.0) -> None:
    """B <- alpha op(T) B (a sample x = L z, or L^T z); A is only read.  alpha == 0: B <- +0 with neither A nor B
    read.  A zero on the diagonal is no failure: there is no info"""
    dt, code, tr, n, lda, sa, batch = _half_of_A(A, uplo, trans)
    nrhs, ldb, sb = _images_of_B(A, B, dt, n, batch)
    _require_device(A, B)
    check("chol_trmm_batched", lib().chol_trmm_batched(code, tr, dt, n, nrhs, float(alpha), A.data_ptr(), lda, sa,
                                                       B.data_ptr(), ldb, sb, batch))


def logdet_batched(A):
    """-> (logdet, info): log det(L L^T) = 2 sum log L_jj of every factor in A as a float64 tensor on A's device
    (for both dtypes), and info (numpy int32); info[b] = j: the first L_jj <= 0 or NaN, logdet[b] is NaN then.  Only
    the diagonal is read"""
    import torch

    dt, _, n, lda, sa, batch = _images_of_A(A, ChamLower)
    _require_device(A)
    out = torch.empty(batch, dtype=torch.float64, device=A.device)
    info, pinfo = _info(batch)
    check("chol_logdet_batched", lib().chol_logdet_batched(dt, n, A.data_ptr(), lda, sa, batch, out.data_ptr(), pinfo))
    return out, info


def _inverse(name, A, uplo):
    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    _require_device(A)
    info, pinfo = _info(batch)
    check(name, getattr(lib(), name)(code, dt, n, A.data_ptr(), lda, sa, batch, pinfo))
    return info


def trtri_batched(A, uplo: int = ChamLower) -> np.ndarray:
    """The `uplo` triangle T of every matrix of A (what potrf_batched left) <- inv(T), in place: Lower gives
    W = inv(L), Upper inv(U) = W^T.  For a finite factor the bits of the lower triangle of trtrs_batched(A, I).
    -> info; info[b] = j: an exact zero at T_jj of matrix b, its A untouched"""
    return _inverse("chol_trtri_batched", A, uplo)


def potri_batched(A, uplo: int = ChamLower) -> np.ndarray:
    """The factor in the `uplo` triangle of every matrix of A <- the `uplo` triangle of inv(L L^T) (the covariance of
    a normal-equations estimate, a block-Jacobi block).  -> info; info[b] = j: an exact zero at L_jj of matrix b, its
    A untouched"""
    return _inverse("chol_potri_batched", A, uplo)


def poinv_batched(A, uplo: int = ChamLower) -> np.ndarray:
    """The `uplo` triangle of every SPD matrix of A <- that of its inverse: potrf_batched and potri_batched in one
    pass, the same bits.  -> potrf_batched's info; a failing matrix is left as potrf_batched leaves it"""
    return _inverse("chol_poinv_batched", A, uplo)


def invdiag_batched(A, uplo: int = ChamLower):
    """-> (D, info): the diagonal of inv(L L^T) of every factor in A (the marginal variances of a local Gaussian
    process) as a new contiguous (batch, n) tensor of A's dtype on A's device, the bits of the diagonal potri_batched
    would write; A is only read.  info[b] = j: an exact zero at L_jj of matrix b, D[b] is then not written"""
    import torch

    dt, code, n, lda, sa, batch = _images_of_A(A, uplo)
    _require_device(A)
    D = torch.empty((batch, n), dtype=A.dtype, device=A.device)
    info, pinfo = _info(batch)
    check("chol_invdiag_batched", lib().chol_invdiag_batched(code, dt, n, A.data_ptr(), lda, sa, D.data_ptr(), n,
                                                             batch, pinfo))
    return D, info


def last_batched_stats() -> dict:
    """The last batched call (chol_last_batched_stats)"""
    v = (C.c_double * 8)()
    check("chol_last_batched_stats", lib().chol_last_batched_stats(v))
    return {"total_ms": v[0], "kernel_ms": v[1], "batch": int(v[2]), "n": int(v[3]), "per_wavefront": int(v[4]),
            "workgroups": int(v[5]), "bytes": v[6]}


__all__ = ["potrf_batched", "potrs_batched", "posv_batched", "chud_batched", "chdd_batched", "trtrs_batched",
           "trmm_batched", "logdet_batched", "trtri_batched", "potri_batched", "poinv_batched", "invdiag_batched",
           "last_batched_stats"]
