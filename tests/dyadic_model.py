"""An input family on which every blocked algorithm of the library is exact, and numpy emulations that prove it.

Nn is strictly lower triangular with an entry only where the (global) row index is odd and the column index even, drawn
from {-1, 0, 1} at density 1/2.  A product Nn Nn pairs a column index that must be even with a row index that must be
odd, so Nn Nn = 0 and inv(I + Nn) = I - Nn -- for the matrix and for every principal sub-block, so the inverse of
every 128-, 64- and 16-block of a factor is dense and has entries of magnitude <= 1 (times a scaling).  The members:
    Cholesky   L = (I + Nn) diag(s), s_j in {1, 2};  A = L L^T;  pivots s_j^2 in {1, 4};  inv(L) = diag(1/s) (I - Nn)
    LDL^T      A = (I + Nn) diag(d) (I + Nn)^T, d_j = +-{1, 2, 4}
    sygst      B = L L^T as above, A = L M L^T with M symmetric, entries in [-3, 3]:  inv(L) A inv(L)^T = M
    solves     X integer in [-3, 3], the right-hand side A X formed in fp64 (exact)
Every Schur complement of these matrices is a short dyadic number (an integer, or a multiple of 1/16 at the worst where
inv(L) enters), so a blocked algorithm in fp32 or fp64 -- whatever its block size, schedule or summation order -- returns
the known answer bit for bit as long as no partial sum leaves the range in which such numbers are exact.  The
emulations below run the right-looking algorithms in 128-blocks (explicit recursive inverse of every diagonal block,
the panel times that inverse, the trailing update; sygst with its two half updates and the deferred solve) in a given
dtype and record, for every product they form, the largest entry of |X| |Y|: a bound on every partial sum of every
summation order.  tests/test_dyadic_host.py asserts that 16 times that peak (four fractional bits) is below 2^24.

That family ("parity") is thin: half the rows and half the columns of the factor carry nothing below the diagonal, and
every product of two off-diagonal pieces of it is zero.  Three more families take the same draws through another mask
(FAMILIES, family_mask):
    mirror   row even, column odd: Nn Nn = 0 again, the other half of the rows and columns carries the entries
    mod3     row % 3 > column % 3: Nn^3 = 0, inv(I + Nn) = I - Nn + Nn^2 -- a second-order term in every inverse
    panel    (of a tile size B, a multiple of 128) the mod3 rule inside the diagonal 128-blocks of the tiles, no mask
             outside them: every panel tile and every trailing update dense
For A = L L^T with L an integer lower triangle whose diagonal is a power of two, unblocked Cholesky is exact whatever the
sparsity of L; only the inverses a blocked algorithm forms constrain the family.  The factorisations (potrf, sytrf) and
the forward sweep of the solves invert nothing larger than a 128-block, as potrf_blocked and ldl_blocked do.  sygst and
the backward sweep of the solves multiply by the inverse of a whole diagonal tile (inv_tile; sygst_blocked with nb = the
tile size follows the library): on a panel member that inverse has magnitude 5e2 for a tile of 256 and 2e6 for one of
512, which is where the host proofs send some of its cases to fp64 alone.  The global inverse of a panel member is huge
(1e13 at n = 1024), so inv_factor and inv_spd refuse that family."""
import functools

import numpy as np

NB = 128


FAMILIES = ("parity", "mirror", "mod3", "panel")


def family_mask(n, family="parity", B=None):
    """where a member of the family may have an entry of Nn (boolean n x n, strictly lower)"""
    i = np.arange(n)
    r, c = i[:, None], i[None, :]
    if family == "parity":
        extra = (r % 2 == 1) & (c % 2 == 0)
    elif family == "mirror":
        extra = (r % 2 == 0) & (c % 2 == 1)
    elif family == "mod3":
        extra = r % 3 > c % 3
    elif family == "panel":
        if B is None or B <= 0 or B % NB:
            raise ValueError(f"the panel family needs a tile size that is a multiple of {NB}, not {B}")
        same_block = (r // B == c // B) & (r % B // NB == c % B // NB)  # a diagonal 128-block of a tile
        extra = ~same_block | (r % 3 > c % 3)
    else:
        raise ValueError(f"unknown family {family!r}")
    return extra & (r > c)


@functools.lru_cache(maxsize=None)
def nn(n, seed, family="parity", B=None):
    """Nn of order n (read-only); B: the tile size, for the panel family only"""
    r = np.random.default_rng(seed)
    N = r.integers(-1, 2, (n, n)).astype(np.float64) * (r.random((n, n)) < 0.75)  # P(nonzero) = 2/3 * 3/4 = 1/2
    N *= family_mask(n, family, B)
    N.setflags(write=False)
    return N


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def cholesky_case(n, seed, smax=2, family="parity", B=None):
    """-> (A, L, s): A = L L^T, L = (I + Nn) diag(s), s_j a power of two <= smax (smax = 1: s = 1)"""
    r = np.random.default_rng(seed + 1000003)
    s = r.choice([1.0, 2.0, 4.0][:int(np.log2(smax)) + 1], n)
    L = (np.eye(n) + nn(n, seed, family, B)) * s[None, :]
    return _frozen(L @ L.T, L, s)


@functools.lru_cache(maxsize=None)
def ldl_case(n, seed, family="parity", B=None):
    """-> (A, L, d): A = L diag(d) L^T, L = I + Nn, d_j = +-{1, 2, 4}"""
    r = np.random.default_rng(seed + 2000003)
    d = r.choice([1.0, 2.0, 4.0], n) * r.choice([-1.0, 1.0], n)
    L = np.eye(n) + nn(n, seed, family, B)
    return _frozen((L * d) @ L.T, L, d)


@functools.lru_cache(maxsize=None)
def sygst_case(n, seed, family="parity", B=None):
    """-> (A, L, M): A = L M L^T, L the Cholesky member's factor, M symmetric with integer entries in [-3, 3]"""
    r = np.random.default_rng(seed + 3000003)
    _, L, _ = cholesky_case(n, seed, 2, family, B)
    M = r.integers(-3, 4, (n, n)).astype(np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    return _frozen(L @ M @ L.T, L, M)


@functools.lru_cache(maxsize=None)
def solution(n, nrhs, seed):
    """an integer X (n x nrhs) with entries in [-3, 3]"""
    X = np.random.default_rng(seed + 4000003).integers(-3, 4, (n, nrhs)).astype(np.float64)
    return _frozen(X)[0]


def inv_factor(n, seed, smax=2, family="parity"):
    """inv(L) of the Cholesky member, from the closed form diag(1/s) (I - Nn) -- mod3: diag(1/s) (I - Nn + Nn Nn), the
    product in fp64 (integers far below 2^53): multiples of 1/smax.  Not for the panel family, whose inverse is huge"""
    if family == "panel":
        raise ValueError("the global inverse of a panel member is not a short dyadic number")
    _, _, s = cholesky_case(n, seed, smax, family)
    N = nn(n, seed, family)
    X = np.eye(n) - N
    if family == "mod3":
        X += N @ N
    return X / s[:, None]


def inv_spd(n, seed, smax=2, family="parity"):
    """inv(A) = inv(L)^T inv(L) of the Cholesky member in fp64 (exact: multiples of 1/smax^2, far below 2^53)"""
    X = inv_factor(n, seed, smax, family)
    return X.T @ X


# ---- the emulations ---------------------------------------------------------------------------------------------------
class Peak:
    """the largest magnitude any stored value or any partial sum of a product can have reached"""

    def __init__(self):
        self.value = 0.0

    def see(self, *arrays):
        for a in arrays:
            if a.size:
                self.value = max(self.value, float(np.abs(a).max()))

    def mm(self, X, Y, C=None):
        """X @ Y in the operands' dtype (C - X @ Y when C is given); |C| + |X| |Y| bounds every partial sum"""
        if X.size == 0 or Y.size == 0:
            return (np.zeros((X.shape[0], Y.shape[1]), dtype=X.dtype) if C is None else C.copy())
        bound = np.abs(X).astype(np.float64) @ np.abs(Y).astype(np.float64)
        if C is not None:
            bound += np.abs(C)
        self.value = max(self.value, float(bound.max()))
        P = X @ Y
        return P if C is None else C - P


def inv_lower(T, peak, unit=False):
    """the inverse of the lower triangular T by halving, as the library's invert_level does: W11 = inv(T11), W22 =
    inv(T22), W21 = -W22 (T21 W11); blocks of 16 by substitution"""
    n = T.shape[0]
    dt = T.dtype
    if n <= 16:
        W = np.zeros((n, n), dtype=dt)
        for j in range(n):
            W[j, j] = dt.type(1) if unit else dt.type(1) / T[j, j]
            for i in range(j + 1, n):
                acc = -(T[i, j:i] @ W[j:i, j])
                peak.value = max(peak.value, float(np.abs(T[i, j:i]).astype(np.float64) @ np.abs(W[j:i, j])))
                W[i, j] = acc if unit else acc / T[i, i]
        return W
    h = n // 2
    W = np.zeros((n, n), dtype=dt)
    W[:h, :h] = inv_lower(T[:h, :h], peak, unit)
    W[h:, h:] = inv_lower(T[h:, h:], peak, unit)
    W[h:, :h] = -peak.mm(W[h:, h:], peak.mm(T[h:, :h], W[:h, :h]))
    peak.see(W)
    return W


def inv_tile(T, peak):
    """the inverse of a lower triangular tile as the library forms it for sygst, pocon and the tile level of trtri
    (stage_factor_diag_into): the tile in an image of whole 128-blocks, the identity beyond it; the diagonal 128-blocks
    by inv_lower; then block column c = n - 2 .. 0 of the inverse from the columns to its right, Y(m) = L(m,c) Xd(c) and
    X(i,c) = - sum_{c < m <= i} X(i,m) Y(m) (each X(i,c) one sum in one accumulator: one product here).  One 128-block:
    inv_lower itself"""
    n = T.shape[0]
    if n <= NB:
        return inv_lower(T, peak)
    P = padded(T, T.dtype)
    nbk = P.shape[0] // NB
    blk = lambda i: slice(i * NB, (i + 1) * NB)
    for i in range(nbk):
        P[blk(i), blk(i)] = inv_lower(P[blk(i), blk(i)], peak)
    for c in range(nbk - 2, -1, -1):
        below = slice((c + 1) * NB, nbk * NB)
        Y = peak.mm(P[below, blk(c)], P[blk(c), blk(c)])
        for i in range(c + 1, nbk):
            P[blk(i), blk(c)] = -peak.mm(P[blk(i), (c + 1) * NB:(i + 1) * NB], Y[:(i - c) * NB])
    peak.see(P)
    return np.tril(P[:n, :n])


def padded(A, dtype, nb=NB):
    """the lower triangle of A in an image of whole nb-blocks, the identity outside it"""
    n = A.shape[0]
    N = -(-n // nb) * nb
    M = np.eye(N, dtype=dtype)
    M[:n, :n] = np.tril(A)
    return M


def chol_unblocked(T, peak):
    """column Cholesky of the lower triangle of T in place, T's dtype; -> info"""
    n = T.shape[0]
    for j in range(n):
        d = T[j, j]
        if not d > 0:
            return j + 1
        p = np.sqrt(d)
        T[j, j] = p
        c = T[j + 1:, j] / p
        T[j + 1:, j] = c
        T[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
        peak.see(T[j:, j:])
    return 0


def potrf_blocked_info(A, dtype, nb=NB):
    """-> (info, M, peak): right-looking Cholesky of the lower triangle of A in nb-blocks, stopped at the first pivot that
    is not > 0 (info = its column + 1, LAPACK's).  M: the working image as it then stands -- the factor's columns before
    that pivot, the pivot itself at M[info - 1, info - 1], the Schur complement behind it; info = 0: the factor"""
    dtype = np.dtype(dtype)
    n = A.shape[0]
    M = padded(A, dtype, nb)
    N = M.shape[0]
    peak = Peak()
    peak.see(M)
    for k in range(0, N, nb):
        d, t = slice(k, k + nb), slice(k + nb, N)
        Tk = np.tril(M[d, d])
        info = chol_unblocked(Tk, peak)
        M[d, d] = Tk
        if info:
            return k + info, np.tril(M[:n, :n]), peak.value
        if k + nb < N:
            W = inv_lower(Tk, peak)
            M[t, d] = peak.mm(M[t, d], W.T)
            M[t, t] = np.tril(peak.mm(M[t, d], M[t, d].T, M[t, t]))
            peak.see(M[t, :])
    return 0, np.tril(M[:n, :n]), peak.value


def potrf_blocked(A, dtype, nb=NB):
    """-> (L, peak): right-looking Cholesky of the lower triangle of A in nb-blocks"""
    info, L, peak = potrf_blocked_info(A, dtype, nb)
    assert info == 0
    return L, peak


def ldl_blocked(A, dtype, nb=NB):
    """-> (F, peak): L D L^T without pivoting of the lower triangle of A in nb-blocks, D on the diagonal of F, L below"""
    dtype = np.dtype(dtype)
    n = A.shape[0]
    M = padded(A, dtype, nb)
    N = M.shape[0]
    one = dtype.type(1)
    peak = Peak()
    peak.see(M)
    for k in range(0, N, nb):
        d, t = slice(k, k + nb), slice(k + nb, N)
        Tk = np.tril(M[d, d])
        for j in range(nb):
            r = one / Tk[j, j]
            w = Tk[j + 1:, j].copy()
            Tk[j + 1:, j] = w * r
            Tk[j + 1:, j + 1:] -= np.tril(np.outer(w, Tk[j + 1:, j]))
            peak.see(Tk[j:, j:])
        M[d, d] = Tk
        if k + nb < N:
            X = inv_lower(np.tril(Tk, -1) + np.eye(nb, dtype=dtype), peak, unit=True)
            W = peak.mm(M[t, d], X.T)
            M[t, d] = W * (one / np.diag(Tk))[None, :]
            M[t, t] = np.tril(peak.mm(W, M[t, d].T, M[t, t]))
            peak.see(M[t, :], W)
    return np.tril(M[:n, :n]), peak.value


def sygst_blocked(A, L, dtype, nb=NB):
    """-> (C, peak): the lower triangle of inv(L) A inv(L)^T by LAPACK's blocked DSYGST (itype 1, Lower) in nb-blocks
    with the left solve of every block column deferred into one pass over the block rows (sygst_model.py).  The
    library's block is the tile, and it inverts the whole diagonal tile of L (inv_tile): nb = the tile size follows it"""
    dtype = np.dtype(dtype)
    n = A.shape[0]
    M = padded(A, dtype, nb)
    F = padded(L, dtype, nb)
    N = M.shape[0]
    half = dtype.type(0.5)
    peak = Peak()
    peak.see(M, F)
    Xd = [inv_tile(F[k:k + nb, k:k + nb], peak) for k in range(0, N, nb)]
    for b, k in enumerate(range(0, N, nb)):
        d, t = slice(k, k + nb), slice(k + nb, N)
        lo = np.tril(M[d, d])
        S = lo + np.tril(lo, -1).T
        lo = np.tril(peak.mm(Xd[b], peak.mm(S, Xd[b].T)))
        M[d, d] = lo
        if k + nb >= N:
            break
        S = lo + np.tril(lo, -1).T
        M[t, d] = peak.mm(M[t, d], Xd[b].T)
        M[t, d] = peak.mm(half * F[t, d], S, M[t, d])
        P, Lt = M[t, d].copy(), F[t, d]
        M[t, t] = np.tril(peak.mm(Lt, P.T, peak.mm(P, Lt.T, M[t, t])))
        M[t, d] = peak.mm(half * F[t, d], S, M[t, d])
        peak.see(M[t, :])
    for b, m in enumerate(range(0, N, nb)):
        r = slice(m, m + nb)
        for c0 in range(0, m, nb):
            c = slice(c0, c0 + nb)
            Y = peak.mm(F[r, c0 + nb:m], M[c0 + nb:m, c], M[r, c])
            M[r, c] = peak.mm(Xd[b], Y)
    peak.see(M)
    return np.tril(M[:n, :n]), peak.value
