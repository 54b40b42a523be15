"""A numpy model of chol_sytrf_nopiv_tile's algorithm (A = L D L^T without pivoting, Lower; L unit lower triangular, D
diagonal), step for step as the library runs it: right-looking with the tile as the block.  Tile column k (T: the tile
rows after k):
    1. A(k,k) = L_kk D_k L_kk^T, unblocked: d_j = a(j,j); r_j = 1 / d_j; l(i,j) = w(i,j) r_j with w the column as the
       earlier pivots left it; a(i,c) -= w(i,j) l(c,j) for j < c <= i
    2. W(T) = A(T,k) L_kk^-T                        (L_kk with its unit diagonal)
    3. A(T,k) <- L(T,k) = W(T) diag(r)              (a multiplication by the reciprocal formed once per pivot, as LAPACK
                                                     DSYTF2's r1 = 1 / d; not a division per entry)
    4. A(T,T) -= W(T) L(T,k)^T                      (lower tiles)
The info rule: the 1-based index of the first pivot that is exactly zero or not finite; the walk stops after the
tile column that holds it (the tile columns before it are final).  A negative pivot is not an error.  The matrix sits
in an image of whole tiles with the identity outside it (the library's padded image); the padding is not part of the
result or of the inertia.  Arithmetic in A's dtype throughout.  The solve: L y = b, z = y r, L^T x = z."""
import numpy as np
from scipy.linalg import solve_triangular


def ldl_unblocked(T, base=0):
    """T (lower triangle read) <- D on the diagonal, L below it, in place -> the first bad pivot (1-based, + base) or 0"""
    n = T.shape[0]
    one = T.dtype.type(1)
    info = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            d = T[j, j]
            if info == 0 and (d == 0 or not np.isfinite(d)):
                info = base + j + 1
            r = one / d
            w = T[j + 1:, j].copy()
            l = w * r
            T[j + 1:, j] = l
            T[j + 1:, j + 1:] -= np.tril(np.outer(w, l))
    return info


def sytrf_model(A, B):
    """-> (F, info): the lower triangle of F holds D (diagonal) and L (below); A symmetric, only its lower triangle
    read; B the tile edge"""
    A = np.asarray(A)
    dt = A.dtype
    n = A.shape[0]
    nt = -(-n // B)
    N = nt * B
    M = np.eye(N, dtype=dt)
    M[:n, :n] = np.tril(A)
    info = 0
    with np.errstate(all="ignore"):
        for k in range(nt):
            d = slice(k * B, (k + 1) * B)
            t = slice((k + 1) * B, N)
            Tk = np.tril(M[d, d])
            info = ldl_unblocked(Tk, k * B)
            M[d, d] = Tk + np.triu(M[d, d], 1)
            if k < nt - 1:
                r = dt.type(1) / np.diag(Tk)
                if info == 0:
                    W = solve_triangular(Tk, M[t, d].T, lower=True, unit_diagonal=True, check_finite=False).T.astype(dt)
                else:
                    W = M[t, d].copy()  # (unspecified from here on)
                M[t, d] = W * r[None, :]
                M[t, t] -= np.tril(W @ M[t, d].T)
            if info:
                break
    return np.tril(M[:n, :n]), info


def split(F):
    """-> (L with its unit diagonal, d) of a factor as stored"""
    return np.tril(F, -1) + np.eye(F.shape[0], dtype=F.dtype), np.diag(F).copy()


def sytrs_model(F, b):
    """x = inv(L D L^T) b from the stored factor, in F's dtype"""
    L, d = split(F)
    r = F.dtype.type(1) / d
    y = solve_triangular(L, b.astype(F.dtype), lower=True, unit_diagonal=True).astype(F.dtype)
    z = y * (r[:, None] if y.ndim == 2 else r)
    return solve_triangular(L.T, z, lower=False, unit_diagonal=True).astype(F.dtype)


def residual(F, K):
    """max |L D L^T - K| / max (|L| |D| |L|^T), in fp64"""
    L, d = split(np.asarray(F, dtype=np.float64))
    R = (L * d) @ L.T - np.asarray(K, dtype=np.float64)
    return np.abs(R).max() / growth_scale(F)


def growth_scale(F):
    L, d = split(np.asarray(F, dtype=np.float64))
    return ((np.abs(L) * np.abs(d)) @ np.abs(L).T).max()


def inertia(F):
    d = np.diag(F)
    return int((d > 0).sum()), int((d < 0).sum())


def quasi_definite(n, m, seed, perm=False):
    """[[H, J^T], [J, -C]], H = G G^T / 2n with G n x 2n standard normal, C likewise of order m, J = randn / sqrt(n):
    what test_sytrf_host.py and test_gpu_sytrf.py factor (a fresh array per call)"""
    r = np.random.default_rng(seed)
    G = r.standard_normal((n, 2 * n))
    H = G @ G.T / (2 * n)
    G = r.standard_normal((m, 2 * m))
    C = G @ G.T / (2 * m)
    J = r.standard_normal((m, n)) / np.sqrt(n)
    K = np.block([[H, J.T], [J, -C]])
    if perm:
        p = r.permutation(n + m)
        K = K[np.ix_(p, p)]
    return K
