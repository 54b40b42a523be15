"""The arithmetic of the batched half routines (chol_trtrs_batched, chol_trmm_batched, chol_logdet_batched:
include/cholmi.h) in numpy, and the inputs that test_trtrs_batched_host.py and test_gpu_trtrs_batched.py share.

L is the lower factor.  Every operation is in the dtype; numpy has no fused multiply-add, so each product is rounded
before it is added -- the one difference from the device, as in potrf_batched_model.py.  r_j = 1 / L(j,j), P = 8, 16,
32 or 64 the padded order, one column of B at a time:
    solve_forward    y_j = b_j r_j, b_i <- b_i - L(i,j) y_j (i > j), j ascending
    solve_backward   j descending: t_i = L(i,j) x_i (j < i < n, +0 at the other i < P), the butterfly
                     t <- t + t[i xor off], off = P/2 .. 1, x_j = (b_j - t_j) r_j
    mul_forward      s_i = +0, s_i <- s_i + L(i,k) z_k for k = 0 .. i ascending, alpha s_i
    mul_backward     j descending: t_i = L(i,j) z_i (j <= i < n, else +0), the same butterfly, alpha t_j
    logdet           2 (((log d_0 + log d_1) + log d_2) + ..) in fp64, d_j = L(j,j); info = j (1-based) at the first
                     d_j <= 0 or NaN, the value NaN then
solve_forward then solve_backward is potrf_batched_model.solve_model, bit for bit.

On the dyadic family (potrf_batched_model.dyadic_case, s_j <= 4) with the integer X of dyadic_model.solution the
products L X and L^T X are exact (|entries| <= 104, diagonals in {1, 2, 4}), so the models, the device and any other
correct order return X from them, and them from X, bit for bit.

The bounds are theorems, componentwise and evaluated in fp64 (Higham, Accuracy and Stability, Thm 8.5: substitution in
any order, one more rounding for the reciprocal; Sec. 3.1 for the inner products, one more rounding for alpha and one
spare):
    |B - op(T) X| <= gamma(n+1) |op(T)| |X|            |C - alpha op(T) B| <= gamma(n+2) |alpha| |op(T)| |B|
    |logdet - ref| <= gamma(n+4) 2 sum |log L_jj|      (fp64 u; ref in np.longdouble from the stored diagonal)
The *_ratio functions return the largest left side over its right side (<= 1 is the assertion)."""
import functools

import numpy as np

from chol_testkit import gamma, npdt
from dyadic_model import solution
from potrf_batched_model import (FAMILIES, HOST_ORDERS, ORDERS, SEEDS, dyadic_case, padded_order, potrf_model,
                                 spectral_case)

__all__ = ["FAMILIES", "HOST_ORDERS", "ORDERS", "SEEDS", "dyadic_case", "padded_order", "spectral_case", "solution"]


# ---------------------------------------------------------------- the arithmetic
def _factor(L, B, dt):
    L = np.tril(np.asarray(L, dtype=npdt(dt)))
    return L, np.array(B, dtype=npdt(dt)).reshape(L.shape[0], -1)


def _first_zero(L):
    d = np.diag(L)
    return int(np.argmax(d == 0)) + 1 if np.any(d == 0) else 0


def _butterfly(t):
    lane, off = np.arange(t.shape[0]), t.shape[0] // 2
    while off:
        t = t + t[lane ^ off]
        off //= 2
    return t


def solve_forward(L, B, dt):
    """-> (Y, info): inv(L) B; info = j (1-based): the first exact zero on the diagonal, Y = B"""
    L, b = _factor(L, B, dt)
    info = _first_zero(L)
    if info:
        return b.reshape(np.shape(B)), info
    with np.errstate(all="ignore"):
        r = b.dtype.type(1) / np.diag(L)
        for j in range(L.shape[0]):
            yj = b[j] * r[j]
            b[j + 1:] = b[j + 1:] - L[j + 1:, j, None] * yj[None, :]
        return (b * r[:, None]).reshape(np.shape(B)), 0


def solve_backward(L, B, dt):
    """-> (X, info): inv(L^T) B"""
    L, y = _factor(L, B, dt)
    info = _first_zero(L)
    if info:
        return y.reshape(np.shape(B)), info
    n, P = L.shape[0], padded_order(L.shape[0])
    with np.errstate(all="ignore"):
        r = y.dtype.type(1) / np.diag(L)
        x = np.zeros_like(y)
        for j in range(n - 1, -1, -1):
            t = np.zeros((P, x.shape[1]), dtype=x.dtype)
            t[j + 1:n] = L[j + 1:, j, None] * x[j + 1:]
            x[j] = (y[j] - _butterfly(t)[j]) * r[j]
    return x.reshape(np.shape(B)), 0


def mul_forward(L, Z, alpha, dt):
    """-> alpha L Z"""
    L, z = _factor(L, Z, dt)
    n = L.shape[0]
    with np.errstate(all="ignore"):
        s = np.zeros_like(z)
        for k in range(n):
            s[k:] = s[k:] + L[k:, k, None] * z[k][None, :]
        return (z.dtype.type(alpha) * s).reshape(np.shape(Z))


def mul_backward(L, Z, alpha, dt):
    """-> alpha L^T Z"""
    L, z = _factor(L, Z, dt)
    n, P = L.shape[0], padded_order(L.shape[0])
    with np.errstate(all="ignore"):
        x = np.zeros_like(z)
        for j in range(n - 1, -1, -1):
            t = np.zeros((P, z.shape[1]), dtype=z.dtype)
            t[j:n] = L[j:, j, None] * z[j:]
            x[j] = z.dtype.type(alpha) * _butterfly(t)[j]
    return x.reshape(np.shape(Z))


def logdet(d):
    """-> (value, info) from the diagonal d (any dtype; converted to fp64)"""
    d = np.asarray(d, dtype=np.float64)
    failing = ~(d > 0)
    if failing.any():
        return np.nan, int(np.argmax(failing)) + 1
    s = np.float64(0)
    for lg in np.log(d):
        s = s + lg
    return 2 * s, 0


# ---------------------------------------------------------------- the bounds
def _ratio(lhs, rhs):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lhs == 0, 0.0, lhs / rhs)  # (0 <= 0 holds; anything positive over 0 is inf)
    return float(q.max()) if q.size else 0.0


def _f64(n, *arrays):
    return [np.asarray(a, dtype=np.float64).reshape(n, -1) for a in arrays]


def trtrs_ratio(T, X, B, dt):
    """max of |B - T X| / (gamma(n+1) |T| |X|), in fp64; T = op(T), the whole triangular matrix"""
    n = T.shape[0]
    T, X, B = _f64(n, T, X, B)
    return _ratio(np.abs(B - T @ X), gamma(n + 1, dt) * (np.abs(T) @ np.abs(X)))


def trmm_ratio(T, C, B, alpha, dt):
    """max of |C - alpha T B| / (gamma(n+2) |alpha| |T| |B|), in fp64"""
    n = T.shape[0]
    T, C, B = _f64(n, T, C, B)
    return _ratio(np.abs(C - alpha * (T @ B)), gamma(n + 2, dt) * abs(alpha) * (np.abs(T) @ np.abs(B)))


def logdet_ratio(value, d):
    """|value - ref| / (gamma(n+4) 2 sum |log d_j|) with fp64's u, ref in np.longdouble from the stored diagonal d"""
    logs = np.log(np.asarray(d).astype(np.longdouble))
    ref, scale = 2 * logs.sum(), 2 * np.abs(logs).sum()
    err = abs(np.longdouble(value) - ref)
    return 0.0 if err == 0 else float(err / (gamma(len(logs) + 4, "d") * scale))


# ---------------------------------------------------------------- the shared inputs (read-only, cached)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def spectral_factor(n, seed, dt, nrhs=3):
    """-> (L, B): the model's factor of spectral_case(n, seed, dt, nrhs)'s matrix (lower, zeros above) and its
    standard normal right-hand side, both in dt"""
    A, B = spectral_case(n, seed, dt, nrhs)
    F, info = potrf_model(A, dt)
    assert info == 0
    return _frozen(np.tril(F))[0], B


@functools.lru_cache(maxsize=None)
def dyadic_products(n, nrhs, seed, family, dt):
    """-> (L, X, L X, L^T X), all exact in dt"""
    L = dyadic_case(n, seed, family, dt)[1]
    X = solution(n, nrhs, seed)
    Ld = L.astype(np.float64)
    return (L,) + _frozen(X.astype(npdt(dt)), (Ld @ X).astype(npdt(dt)), (Ld.T @ X).astype(npdt(dt)))
