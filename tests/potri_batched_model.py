"""The arithmetic of the batched inverses (chol_trtri_batched, chol_potri_batched, chol_poinv_batched,
chol_invdiag_batched: include/cholmi.h) in numpy, and the inputs that test_potri_batched_host.py and
test_gpu_potri_batched.py share.

L is the lower factor, W = inv(L), X = W^T W = inv(L L^T).  Every operation is in the dtype; numpy has no fused
multiply-add, so each product is rounded before it is added -- the one difference from the device, as in
potrf_batched_model.py.  r_j = 1 / L(j,j):
    trtri_model   column c of W on its own: b_c = 1, b_i = +0 (i > c); for j = c .. n-1 ascending:
                  W(j,c) = b_j r_j, b_i <- b_i - L(i,j) W(j,c) (i > j)
    lauum_model   X(i,m), i >= m: s = +0; for k = i .. n-1 ascending: s <- s + W(k,i) W(k,m)
Both select the terms of an entry; nothing is multiplied by a stored zero, so a NaN at L(p,q) reaches W(k,c) for
c <= q, k >= p and X(i,m) for m <= q, and no other entry.  trtri_model is trtrs_batched_model.solve_forward(L, I),
bit for bit.

On the dyadic families (potrf_batched_model.dyadic_case, s_j <= 4) inv(L) is dyadic with at most 3 significant bits
and every partial sum of W^T W has at most 10, so the models, the device and any other correct order return the exact
W and X bit for bit, in fp32 and fp64.

The bounds are theorems, componentwise and evaluated in fp64 (Higham, Accuracy and Stability, Thm 8.5: substitution in
any order, one more rounding for the reciprocal; Sec. 3.1 for the inner products):
    |L W - I| <= gamma(n+1) |L| |W|            |X - W^T W| <= gamma(n+1) |W^T| |W|   (the lower triangle)
The *_ratio functions return the largest left side over its right side (<= 1 is the assertion)."""
import functools

import numpy as np

from chol_testkit import gamma, npdt
from potrf_batched_model import (FAMILIES, HOST_ORDERS, ORDERS, SEEDS, dyadic_case, failing_case, padded_order,
                                 potrf_model, spectral_case)

__all__ = ["FAMILIES", "HOST_ORDERS", "ORDERS", "SEEDS", "dyadic_case", "failing_case", "padded_order", "potrf_model",
           "spectral_case"]


# ---------------------------------------------------------------- the arithmetic
def trtri_model(L, dt):
    """-> (W, info): inv(L) from the lower triangle of L, zeros above; info = j (1-based): the first exact zero on
    the diagonal, W = tril(L) then"""
    L = np.tril(np.asarray(L, dtype=npdt(dt)))
    n = L.shape[0]
    d = np.diag(L)
    if np.any(d == 0):
        return L, int(np.argmax(d == 0)) + 1
    with np.errstate(all="ignore"):
        r = L.dtype.type(1) / d
        B = np.eye(n, dtype=L.dtype)  # column c: the running b of e_c
        W = np.zeros_like(L)
        for j in range(n):
            W[j, :j + 1] = B[j, :j + 1] * r[j]
            B[j + 1:, :j + 1] = B[j + 1:, :j + 1] - L[j + 1:, j, None] * W[j, None, :j + 1]
    return W, 0


def lauum_model(W, dt):
    """-> the lower triangle of W^T W from the lower triangle of W, zeros above"""
    W = np.tril(np.asarray(W, dtype=npdt(dt)))
    n = W.shape[0]
    X = np.zeros_like(W)
    with np.errstate(all="ignore"):
        for k in range(n):
            X[:k + 1, :k + 1] = X[:k + 1, :k + 1] + W[k, :k + 1, None] * W[k, None, :k + 1]
    return np.tril(X)


def potri_model(L, dt):
    """-> (X, info): the lower triangle of inv(L L^T); on info > 0: tril(L)"""
    W, info = trtri_model(L, dt)
    return (W, info) if info else (lauum_model(W, dt), 0)


# ---------------------------------------------------------------- the bounds
def _ratio(lhs, rhs):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lhs == 0, 0.0, lhs / rhs)  # (0 <= 0 holds; anything positive over 0 is inf)
    return float(q.max()) if q.size else 0.0


def trtri_ratio(L, W, dt):
    """max of |L W - I| / (gamma(n+1) |L| |W|), in fp64, from the lower triangles"""
    n = L.shape[0]
    L, W = np.tril(np.asarray(L, dtype=np.float64)), np.tril(np.asarray(W, dtype=np.float64))
    return _ratio(np.abs(L @ W - np.eye(n)), gamma(n + 1, dt) * (np.abs(L) @ np.abs(W)))


def lauum_ratio(W, X, dt):
    """max over the lower triangle of |X - W^T W| / (gamma(n+1) |W^T| |W|), in fp64"""
    n = W.shape[0]
    W, X = np.tril(np.asarray(W, dtype=np.float64)), np.tril(np.asarray(X, dtype=np.float64))
    return _ratio(np.tril(np.abs(X - W.T @ W)), gamma(n + 1, dt) * np.tril(np.abs(W).T @ np.abs(W)))


# ---------------------------------------------------------------- the shared inputs (read-only, cached)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def spectral_inverse(n, seed, dt):
    """-> (A, L, W, X): spectral_case(n, seed, dt)'s matrix, the model's factor of it (lower, zeros above), and the
    models' inv(L) and lower triangle of inv(L L^T), all in dt"""
    A = spectral_case(n, seed, dt)[0]
    F, info = potrf_model(A, dt)
    assert info == 0
    L = np.tril(F)
    W, info = trtri_model(L, dt)
    assert info == 0
    return (A,) + _frozen(L, W, lauum_model(W, dt))


@functools.lru_cache(maxsize=None)
def dyadic_inverse(n, seed, family, dt):
    """-> (A, L, W, X) of dyadic_case(n, seed, family, dt): W = inv(L) and X = tril(inv(A)), exact in dt (the models in
    fp64, which are exact there; test_potri_batched_host.py holds them to L W = I and X = W^T W in exact arithmetic)"""
    A, L, _ = dyadic_case(n, seed, family, dt)
    W, info = trtri_model(L, "d")
    assert info == 0
    X = lauum_model(W, "d")
    Wt, Xt = W.astype(npdt(dt)), X.astype(npdt(dt))
    assert np.array_equal(Wt.astype(np.float64), W) and np.array_equal(Xt.astype(np.float64), X)
    return (A, L) + _frozen(Wt, Xt)
