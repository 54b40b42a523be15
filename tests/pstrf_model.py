"""A numpy model of chol_pstrf_tile's algorithm (the pivoted Cholesky factorisation, LAPACK DPSTRF, Lower), step for
step as the library runs it: tile columns of B, right-looking between them and left-looking inside one, the
candidates d = dg - w reset at each tile column, the symmetric interchange of the trailing matrix, the rows of the
tile column's finished columns swapped at each step and those of the earlier tile columns once at its end.  The
matrix sits in an image of whole tiles with the identity outside it (the library's padded image); the padded rows
are candidates only when exclude_padding is False (what the library must not do)."""
import numpy as np


def best(v):
    """LAPACK's MAXLOC with the library's NaN rule: the first NaN, else the first largest entry"""
    nan = np.isnan(v)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(v))


def pstrf_model(A, B, tol=-1.0, exclude_padding=True):
    """-> (piv 1-based, rank, info, L): A symmetric (n x n), B the tile edge"""
    A = np.asarray(A)
    dt = A.dtype.type
    n = A.shape[0]
    nt = -(-n // B)
    N = nt * B
    M = np.eye(N, dtype=A.dtype)
    M[:n, :n] = A
    real = n if exclude_padding else N
    piv = np.arange(N)
    amax = M[best(np.diag(M)[:real]), best(np.diag(M)[:real])]
    if not amax > 0:
        return piv[:n] + 1, 0, 1, np.zeros_like(A)
    dstop = dt(tol) if tol >= 0 else dt(n) * dt(np.finfo(A.dtype).eps / 2) * amax
    stop = None
    for k in range(nt):
        k0, k1 = k * B, min(k * B + B, real)
        dg = np.diag(M).copy()
        w = np.zeros(N, dtype=A.dtype)
        swaps = []
        for j in range(k0, k1):
            cand = dg[j:real] - w[j:real]
            p = j + best(cand)
            ajj = cand[p - j]
            if j > 0 and not ajj > dstop:
                stop = j
                break
            swaps.append((j, p))
            if p != j:
                for x in (M[j:, j:],):  # the trailing matrix, symmetric at update level k-1
                    x[[0, p - j], :] = x[[p - j, 0], :]
                    x[:, [0, p - j]] = x[:, [p - j, 0]]
                M[[j, p], k0:j] = M[[p, j], k0:j]
                dg[[j, p]] = dg[[p, j]]
                w[[j, p]] = w[[p, j]]
                piv[[j, p]] = piv[[p, j]]
            ljj = np.sqrt(ajj)
            M[j, j] = ljj
            col = M[j + 1:, j] - M[j + 1:, k0:j] @ M[j, k0:j]
            M[j + 1:, j] = col * (dt(1) / ljj)
            M[j, j + 1:] = 0
            w[j + 1:] = w[j + 1:] + M[j + 1:, j] * M[j + 1:, j]
        for j, p in swaps:  # the deferred interchanges of the earlier tile columns, in order
            M[[j, p], :k0] = M[[p, j], :k0]
        if stop is not None:
            break
        Lk = M[k1:, k0:k1]
        M[k1:, k1:] -= Lk @ Lk.T
    rank = stop if stop is not None else min(n, real)
    L = np.tril(M)[:n, :n]
    return piv[:n] + 1, rank, int(rank < n), L


def gram(n, r, seed, dtype=np.float64):
    """G G^T, G n x r standard normal: rank min(n, r); what test_pstrf_host.py and test_gpu_pstrf.py factor"""
    G = np.random.default_rng(seed).standard_normal((n, r))
    return np.asfortranarray((G @ G.T).astype(dtype))
