"""A numpy model of chol_pstrf_tile's algorithm (the pivoted Cholesky factorisation, LAPACK DPSTRF, Lower), step for
step as the library runs it: tile columns of B, right-looking between them and left-looking inside one, the
candidates d = dg - w reset at each tile column, the symmetric interchange of the trailing matrix, the rows of the
tile column's finished columns swapped at each step and those of the earlier tile columns once at its end.  The
matrix sits in an image of whole tiles with the identity outside it (the library's padded image); the padded rows
are candidates only when exclude_padding is False (what the library must not do).

level_case is the family on which the pivoted factorisation is exact and its elimination order forced up to ties:
levels of m indices, the diagonal of the factor 2^g falling by one power of two per level, the entries under it
-1, 0 or 1 times 2^(g - t), nothing off the diagonal within a level.  While a level is being eliminated each of its
remaining rows has the candidate 4^g exactly and every later row at most 4^g ((4/3) m 4^-t + 1/4), so with
m 4^-t < 9/16 the level is finished before any later row is taken; the rows of one level tie, the smallest current
position wins, and because the factor is diagonal within a level that choice permutes the factor and changes no value:
expected_factor is the result in closed form.  Pivots are powers of 4, 1 / L(j,j) a power of 2, w and dg - w exact sums
of squares.  CASES lists (n, tile, m, t, r, the dtypes in which all of this is exact); tests/test_pstrf_host.py proves
the list, against LAPACK and against this model."""
import functools

import numpy as np


def best(v, tie="first"):
    """LAPACK's MAXLOC with the library's NaN rule: the first NaN, else the first largest entry.  tie = "last" is the
    wrong rule (the last of the equals) that the exact cases must tell apart"""
    nan = np.isnan(v)
    if nan.any():
        return int(np.argmax(nan))
    if tie == "last":
        return len(v) - 1 - int(np.argmax(v[::-1]))
    return int(np.argmax(v))


def pstrf_model(A, B, tol=-1.0, exclude_padding=True, tie="first", stop_at_equal=True):
    """-> (piv 1-based, rank, info, L): A symmetric (n x n), B the tile edge.  The wrong variants, beside
    exclude_padding=False: tie="last" takes the last of equal candidates, stop_at_equal=False goes on at a pivot equal
    to the stopping value (LAPACK stops unless the pivot is greater)"""
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
            p = j + best(cand, tie)
            ajj = cand[p - j]
            if j > 0 and not (ajj > dstop if stop_at_equal else ajj >= dstop):
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


# ------------------------------------------------------------------------------------------- the exact family
# (n, tile, m, t, r, dtypes): r = None is full rank.  The level structure per case (G = the last level):
#   (1024, 256): 8 levels, 4 tile columns; in fp32 the default stopping value 1024 2^-24 4^7 = 1 equals the pivots of
#                the last level
#   (1000, 192): ragged, a tile that is no multiple of 128, n % 64 != 0; r = 700 stops inside the fourth tile column
#   (1536, 512): three tiles of 512
#   (1100, 128): nine tile columns, long composed interchange lists for the earlier ones
#   (700, 320):  levels and tiles misaligned
#   (2048, 512): stops inside the first tile column of four
#   (300, 512):  a tile larger than the matrix
#   (100, 100):  a single tile whose edge is no multiple of 64
CASES = [(1024, 256, 128, 4, None, ("d", "s")),
         (1000, 192, 128, 4, None, ("d", "s")), (1000, 192, 128, 4, 700, ("d", "s")),
         (1536, 512, 256, 5, None, ("d", "s")), (1536, 512, 256, 5, 1100, ("d", "s")),
         (1100, 128, 160, 5, None, ("d", "s")),
         (700, 320, 100, 4, None, ("d", "s")),
         (2048, 512, 512, 5, 300, ("d", "s")),
         (300, 512, 64, 4, None, ("d", "s")),
         (100, 100, 16, 3, 60, ("d", "s"))]
VIEW_CASE = (768, 256, 96, 4, 500, ("d",))  # chol_testkit.UserView's order and tile
EXACT = [(*c[:5], dt) for c in CASES for dt in c[5]]
EXACT_IDS = ["-".join(str(x) for x in c) for c in EXACT]
STOP_CASE = CASES[0]
RAGGED_CASE, RAGGED_DEFICIENT_CASE = CASES[1], CASES[2]


def case_seed(n, B):
    return 1000 * n + B


@functools.lru_cache(maxsize=None)
def level_case(n, m, t, seed, r=None):
    """-> (A, L0, sigma), fp64 and read-only: L0 (n x r) the factor by levels, A = (L0 L0^T)[sigma][:, sigma]"""
    r = n if r is None else r
    rng = np.random.default_rng(seed)
    lev = np.arange(n) // m
    g = (lev[-1] - lev).astype(np.float64)
    N = rng.integers(-1, 2, size=(n, r)) * (rng.random((n, r)) < 0.75)  # -1, 0, 1 at density 1/2
    L0 = np.where(lev[:, None] > lev[None, :r], N * 2.0 ** (g[None, :r] - t), 0.0)
    L0[np.arange(r), np.arange(r)] = 2.0 ** g[:r]
    A0 = L0 @ L0.T + 0.0
    sigma = rng.permutation(n)
    A = np.asfortranarray(A0[np.ix_(sigma, sigma)])
    for x in (A, L0, sigma):
        x.setflags(write=False)
    return A, L0, sigma


def case_of(c):
    """level_case of an entry of CASES (or its first five fields)"""
    n, B, m, t, r = c[:5]
    return level_case(n, m, t, case_seed(n, B), r)


def level_bits(L0, t):
    """log2 of (the largest partial sum of any summation order) / (the unit of the data, 4^-t)"""
    a = np.abs(L0)
    return float(np.log2((a @ a.T).max() * 4.0 ** t))


def expected_factor(L0, sigma, piv, rank):
    """the first rank columns of the factor, given the pivots: row a of the pivoted matrix is row e(a) = sigma[piv(a)
    - 1] of A0, so L(:, :rank) = tril(L0[e][:, e[:rank]]) (fp64; every entry is representable in fp32 too)"""
    e = np.asarray(sigma)[np.asarray(piv, dtype=np.int64) - 1]
    return np.tril(L0[e][:, e[:rank]])


@functools.lru_cache(maxsize=None)
def lapack_level(n, B, m, t, r, dt, tol=-1.0):
    """LAPACK's dpstrf / spstrf (Lower) on that case -> (piv, rank, info, tril of what it returned), read-only"""
    import scipy.linalg.lapack as lapack

    A = case_of((n, B, m, t, r))[0]
    fn, dtype = (lapack.dpstrf, np.float64) if dt == "d" else (lapack.spstrf, np.float32)
    c, piv, rank, info = fn(np.asfortranarray(A.astype(dtype)), tol=tol, lower=1)
    L = np.tril(c)
    for x in (piv, L):
        x.setflags(write=False)
    return piv, int(rank), int(info), L


NAN_PLANTS = [(900, 300), (500, 191), (999, 0)]  # (i, k) in A0's numbering on RAGGED_CASE, level(i) > level(k)


def nan_planted(case, i, k):
    """the case's matrix with a NaN at (i, k) and (k, i) of A0 (a fresh, writable copy)"""
    A, _, sigma = case_of(case)
    inv = np.argsort(sigma)
    A = A.copy(order="F")
    A[inv[i], inv[k]] = A[inv[k], inv[i]] = np.nan
    return A


def nan_expected_factor(case, i, k, piv, rank):
    """expected_factor with the NaN where it must be: at row i's position in the column of k"""
    _, L0, sigma = case_of(case)
    L0 = L0.copy()
    L0[i, k] = np.nan
    return expected_factor(L0, sigma, piv, rank)


def chunk_factor():
    """the case with more than 256 chunks of 64 rows: n = 16640, rank 5, G = 2, t = 3 (5 4^(G - t) < 16: the five
    rows of the first level are taken first), the five tied rows at positions that straddle chunks 255, 256 (the
    second pass of thread 0 over the partial maxima) and 257 -> (L0 float32, sigma, the first five pivots expected)"""
    n, r, where = 16640, 5, [16484, 100, 16383, 16384, 8000]
    rng = np.random.default_rng(16640)
    L0 = (rng.integers(-1, 2, size=(n, r)) * (rng.random((n, r)) < 0.75) * 0.5).astype(np.float32)
    L0[:r] = 4.0 * np.eye(r, dtype=np.float32)
    sigma = np.full(n, -1, dtype=np.int64)
    sigma[where] = np.arange(r)
    sigma[sigma < 0] = r + rng.permutation(n - r)
    return L0, sigma, np.sort(where) + 1


def chunk_matrix(L0, sigma):
    """(L0 L0^T)[sigma][:, sigma] formed in float32, about 1 GiB (every product and sum is a multiple of 1/4 below
    2^5: exact), Fortran order"""
    Lp = L0[sigma]
    return (Lp @ Lp.T).T  # (symmetric: the transposed view is the same matrix in Fortran order)
