"""The arithmetic of the batched small-matrix routines (chol_potrf_batched, chol_potrs_batched, chol_posv_batched:
include/cholmi.h) in numpy, and the inputs that test_potrf_batched_host.py and test_gpu_potrf_batched.py share.

potrf_model is the header's left-looking chain, every operation in the dtype; numpy has no fused multiply-add, so the
product is rounded before it is subtracted -- the one difference from the device.  solve_model is the library's solve
order: forward by columns, y_j = b_j r_j with r_j = 1 / L(j,j), b_i <- b_i - L(i,j) y_j (i > j); backward, j
descending, x_j = (y_j - S_j) r_j where S_j sums t_i = L(i,j) x_i (j < i < n; +0 at every other i below the padded
order P = 8, 16, 32 or 64) by the butterfly t <- t + t[i xor off], off = P/2 .. 1.  One column of B at a time.

On the dyadic family (dyadic_model.cholesky_case with smax = 4) every partial sum is a small integer, so the model, the
device and any other correct order return the known factor and solution bit for bit.

The bounds are theorems (Higham, Accuracy and Stability, Thms 10.3 and 10.4, with one more rounding for the
reciprocal), componentwise and evaluated in fp64:
    |A - L L^T| <= gamma(n+2) |L| |L^T|            |B - A X| <= gamma(3n+3) |L| |L^T| |X|
factor_ratio and solve_ratio return the largest left side over its right side (<= 1 is the assertion)."""
import functools

import numpy as np

import dyadic_model as dy
from chol_testkit import gamma, npdt, spd_spectral

ORDERS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)  # both sides of every packing boundary
HOST_ORDERS = ORDERS[:12] + (48,) + ORDERS[12:]
FAMILIES = ("parity", "mirror", "mod3")
NRHS = (1, 3, 8, 9, 17)
SEEDS = (0, 1, 2, 3)


def padded_order(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


# ---------------------------------------------------------------- the arithmetic
def potrf_model(A, dt):
    """-> (F, info): the lower triangle of A (dtype dt) factored; on info = j+1 the columns before j+1 hold the
    factor's and the rest is as it was given.  The strict upper triangle of F is A's."""
    F = np.array(A, dtype=npdt(dt))
    n = F.shape[0]
    one = F.dtype.type(1)
    for j in range(n):
        s = F[j:, j].copy()
        for k in range(j):
            s = s - F[j:, k] * F[j, k]
        if not s[0] > 0:
            return F, j + 1
        p = np.sqrt(s[0])
        r = one / p
        F[j, j] = p
        F[j + 1:, j] = s[1:] * r
    return F, 0


def solve_model(L, B, dt):
    """-> (X, info): inv(L L^T) B from the lower triangle of L, B n x nrhs; info = j (1-based): the first exact zero on
    the diagonal, X = B"""
    L = np.tril(np.asarray(L, dtype=npdt(dt)))
    X = np.array(B, dtype=npdt(dt)).reshape(L.shape[0], -1)
    n, P = L.shape[0], padded_order(L.shape[0])
    d = np.diag(L)
    if np.any(d == 0):
        return X.reshape(np.shape(B)), int(np.argmax(d == 0)) + 1
    with np.errstate(all="ignore"):
        r = X.dtype.type(1) / d
        b = X.copy()
        for j in range(n):
            yj = b[j] * r[j]
            b[j + 1:] = b[j + 1:] - L[j + 1:, j, None] * yj[None, :]
        y = b * r[:, None]
        x = np.zeros_like(y)
        lane = np.arange(P)
        for j in range(n - 1, -1, -1):
            t = np.zeros((P, x.shape[1]), dtype=x.dtype)
            t[j + 1:n] = L[j + 1:, j, None] * x[j + 1:]
            off = P // 2
            while off:
                t = t + t[lane ^ off]
                off //= 2
            x[j] = (y[j] - t[j]) * r[j]
    return x.reshape(np.shape(B)), 0


# ---------------------------------------------------------------- the bounds
def _ratio(lhs, rhs):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lhs == 0, 0.0, lhs / rhs)  # (0 <= 0 holds; anything positive over 0 is inf)
    return float(q.max()) if q.size else 0.0


def factor_ratio(A, L, dt):
    """max of |A - L L^T| / (gamma(n+2) |L| |L^T|) over the lower triangle, in fp64"""
    n = A.shape[0]
    A, L = np.tril(np.asarray(A, dtype=np.float64)), np.tril(np.asarray(L, dtype=np.float64))
    return _ratio(np.tril(np.abs(A - L @ L.T)), gamma(n + 2, dt) * np.tril(np.abs(L) @ np.abs(L).T))


def solve_ratio(A, L, X, B, dt):
    """max of |B - A X| / (gamma(3n+3) |L| |L^T| |X|), in fp64; A symmetric (both triangles)"""
    n = A.shape[0]
    A, L = np.asarray(A, dtype=np.float64), np.tril(np.asarray(L, dtype=np.float64))
    X, B = np.asarray(X, dtype=np.float64).reshape(n, -1), np.asarray(B, dtype=np.float64).reshape(n, -1)
    return _ratio(np.abs(B - A @ X), gamma(3 * n + 3, dt) * (np.abs(L) @ np.abs(L).T @ np.abs(X)))


# ---------------------------------------------------------------- the shared inputs (read-only, cached)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def spectral_case(n, seed, dt, nrhs=3):
    """-> (A, B): spd_spectral(n, 1e3, 100 n + seed) and a standard normal n x nrhs right-hand side, rounded to dt"""
    A = spd_spectral(n, 1e3, 100 * n + seed).astype(npdt(dt))
    B = np.random.default_rng(7000003 + 100 * n + seed).standard_normal((n, nrhs)).astype(npdt(dt))
    return _frozen(np.asfortranarray(A), np.asfortranarray(B))


@functools.lru_cache(maxsize=None)
def dyadic_case(n, seed, family, dt):
    """-> (A, L, s) of dyadic_model.cholesky_case(n, seed, 4, family) in dt (exact: max |A| = 121 at n = 64)"""
    A, L, s = dy.cholesky_case(n, seed, 4, family)
    assert np.abs(A).max() < 2 ** 20
    return _frozen(A.astype(npdt(dt)), L.astype(npdt(dt)), s.astype(npdt(dt)))


@functools.lru_cache(maxsize=None)
def dyadic_rhs(n, nrhs, seed, family, dt):
    """-> (X, B): X = dyadic_model.solution(n, nrhs, seed), B = A X (exact)"""
    A = dy.cholesky_case(n, seed, 4, family)[0]
    X = dy.solution(n, nrhs, seed)
    return _frozen(X.astype(npdt(dt)), (A @ X).astype(npdt(dt)))


def failing_case(n, seed, family, dt, j, nan=False):
    """the dyadic A with A(j,j) -= s_j^2 (0-based j): pivot j is exactly 0, info = j + 1; nan: a NaN there instead"""
    A, _, s = dyadic_case(n, seed, family, dt)
    A = A.copy()
    A[j, j] = np.nan if nan else A[j, j] - s[j] * s[j]
    return A
