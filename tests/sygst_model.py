"""A numpy model of chol_sygst_tile's algorithm (the reduction of the symmetric-definite generalized eigenproblem
A x = lambda B x to standard form, LAPACK DSYGST with itype 1, Lower), step for step as the library runs it: LAPACK's
blocked DSYGST with the tile as the block, except that the left solve of every tile column, A(T,k) <- inv(L(T,T))
A(T,k), is deferred into one pass over the tile rows after the walk.  Step k (T: the tile rows and columns after k):
    1. A(k,k) <- X A(k,k) X^T, X = inv(L(k,k)), computed as X (S X^T) on the symmetric expansion S of A(k,k)'s lower
       triangle; only the lower triangle is kept, and its symmetric expansion serves steps 3 and 5
    2. A(T,k) <- A(T,k) L(k,k)^-T
    3. A(T,k) -= 1/2 L(T,k) A(k,k)
    4. A(T,T) -= A(T,k) L(T,k)^T + L(T,k) A(T,k)^T          (lower tiles)
    5. step 3 again
then, for every tile row m = 1 .. nt-1 in order and every k < m,
    X(m,k) = inv(L(m,m)) (P(m,k) - sum_{k<j<m} L(m,j) X(j,k))
where P is column k as step k left it.  The matrix sits in an image of whole tiles with the identity outside it (the
library's padded image).  Arithmetic in A's dtype throughout."""
import numpy as np
from scipy.linalg import solve_triangular


def sygst_model(A, L, B):
    """-> the lower triangle of inv(L) A inv(L)^T (A symmetric, only its lower triangle read; L lower triangular, only
    its lower triangle read), B the tile edge"""
    A = np.asarray(A)
    dt = A.dtype
    n = A.shape[0]
    nt = -(-n // B)
    N = nt * B
    M = np.eye(N, dtype=dt)
    M[:n, :n] = np.tril(A)
    F = np.eye(N, dtype=dt)
    F[:n, :n] = np.tril(L)
    half = dt.type(0.5)
    # the inverted diagonal tiles of the factor
    Xd = [np.tril(np.linalg.inv(F[k * B:(k + 1) * B, k * B:(k + 1) * B])) for k in range(nt)]
    for k in range(nt):
        d = slice(k * B, (k + 1) * B)
        t = slice((k + 1) * B, N)
        Lkk = F[d, d]
        lo = np.tril(M[d, d])
        S = lo + np.tril(lo, -1).T
        C = Xd[k] @ (S @ Xd[k].T)
        lo = np.tril(C)
        M[d, d] = lo + np.triu(M[d, d], 1)
        if k == nt - 1:
            break
        S = lo + np.tril(lo, -1).T
        # A(T,k) <- A(T,k) L(k,k)^-T
        M[t, d] = solve_triangular(Lkk, M[t, d].T, lower=True).T
        M[t, d] -= half * (F[t, d] @ S)
        Ptk, Ltk = M[t, d].copy(), F[t, d]
        upd = Ptk @ Ltk.T + Ltk @ Ptk.T
        M[t, t] -= np.tril(upd)
        M[t, d] -= half * (F[t, d] @ S)
    # the deferred left solves
    for m in range(1, nt):
        r = slice(m * B, (m + 1) * B)
        for k in range(m):
            c = slice(k * B, (k + 1) * B)
            Y = M[r, c].copy()
            for j in range(k + 1, m):
                Y -= F[r, j * B:(j + 1) * B] @ M[j * B:(j + 1) * B, c]
            M[r, c] = Xd[m] @ Y
    return np.tril(M[:n, :n])

