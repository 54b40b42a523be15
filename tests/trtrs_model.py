"""The half solve and the half product with a Cholesky factor (chol_trtrs_tile, chol_trmm_tile) in numpy, what the
tests of both share, and the cases on which they are exact.

half_solve is the narrow path's arithmetic per tile column: the inverse of the whole diagonal tile (dyadic_model.inv_tile,
what stage_factor_diag forms), the product of that inverse with the tile's part of the right-hand side, and the update
of the rows to come; forward it walks the tile columns down (L y = b), backward it walks them up (L^T x = y).  With a
dyadic_model.Peak every product records the largest |X| |Y|, a bound on every partial sum of every summation order.

The cases: the families of dyadic_model (smax = 2), X = dyadic_model.solution, integers in [-3, 3], B = op(L) X formed
in fp64.  CASES lists (family, n, tile, the dtypes in which the emulation is exact); tests/test_trtrs_host.py proves the
list."""
import functools

import numpy as np

import dyadic_model as dm

SHAPES = [(1000, 128), (1100, 192), (1536, 256), (2100, 512), (300, 512), (192, 192)]
NARROW = 40  # the widest call of the narrow paths (TRTRS_KX, TRMM_KX)
NRHS = [1, 3, 8, 9, NARROW + 1]

# the peaks the emulation reaches over both halves with this X: parity, mirror, mod3 <= 3.8e3 on all six shapes; panel
# 5.9e2 at (1000, 128), 4.9e4 at (1536, 256), 6.4e5 at (300, 512), and 1.28e8 at (2100, 512): exact in fp64, too large
# for fp32 (16 x 1.28e8 > 2^24)
CASES = [(fam, n, B, ("d", "s")) for fam in ("parity", "mirror", "mod3") for n, B in SHAPES]
CASES += [("panel", 1000, 128, ("d", "s")), ("panel", 1536, 256, ("d", "s")), ("panel", 300, 512, ("d", "s")),
          ("panel", 2100, 512, ("d",))]
EXACT = [(fam, n, B, dt) for fam, n, B, dts in CASES for dt in dts]
EXACT_IDS = ["-".join(str(x) for x in c) for c in EXACT]


def limit(dt):
    """16 x peak (four fractional bits) must stay below this"""
    return 2.0 ** 53 if dt == "d" else 2.0 ** 24


def fam_kw(fam, B):
    return {} if fam == "parity" else {"family": fam, "B": B} if fam == "panel" else {"family": fam}


def factor(fam, n, B):
    """the exact factor L of the family's member (fp64, read-only)"""
    return dm.cholesky_case(n, n, 2, **fam_kw(fam, B))[1]


def solution(n, nrhs=NARROW + 1):
    """the leading nrhs columns of ONE integer matrix per order: what is proven for all of them holds for each"""
    return dm.solution(n, NARROW + 1, n)[:, :nrhs]


def is_forward(u, t):
    """(Lower, NoTrans) and (Upper, Trans): L y = b; the other two: L^T x = y (L the factor as Lower)"""
    return (u == "L") == (t == "N")


def half_solve(L, B, tile, forward, dtype, peak=None):
    """-> inv(L) B (forward) or inv(L^T) B in dtype, tile column by tile column through the whole-tile inverses"""
    peak = dm.Peak() if peak is None else peak
    n = L.shape[0]
    Lt = np.tril(L).astype(dtype)
    R = np.array(B, dtype=dtype)
    X = np.zeros_like(R)
    starts = list(range(0, n, tile))
    for k in (starts if forward else starts[::-1]):
        d = slice(k, min(k + tile, n))
        W = dm.inv_tile(np.array(Lt[d, d]), peak)
        if forward:
            X[d] = peak.mm(W, R[d])
            rest = slice(d.stop, n)
            R[rest] = peak.mm(Lt[rest, d], X[d], R[rest])
        else:
            X[d] = peak.mm(np.ascontiguousarray(W.T), R[d])
            rest = slice(0, k)
            R[rest] = peak.mm(np.ascontiguousarray(Lt[d, rest].T), X[d], R[rest])
    return X


def half_product(L, X, forward):
    """-> (L X or L^T X in fp64, the largest |L| |X|: the bound on every partial sum of the product)"""
    M = np.tril(L) if forward else np.tril(L).T
    return M @ X, float((np.abs(M) @ np.abs(X)).max())


def solve_backward_error(M, X, B):
    """the componentwise backward error of M X = B per column, in fp64: max_i |B - M X|_i / (|M| |X| + |B|)_i"""
    M, X, B = (np.asarray(a, dtype=np.float64) for a in (M, X, B))
    num, den = np.abs(B - M @ X), np.abs(M) @ np.abs(X) + np.abs(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(den > 0, num / den, 0.0)
    return q.max(axis=0)


@functools.lru_cache(maxsize=None)
def random_problem(n):
    """as test_gpu_chud.py: problem -- A = G G^T with G n x 2n standard normal, -> (its LAPACK factor, B n x 41
    standard normal), fp64, read-only"""
    g = np.random.default_rng(n)
    G = g.standard_normal((n, 2 * n))
    L = np.linalg.cholesky(G @ G.T)
    B = g.standard_normal((n, NARROW + 1))
    L.setflags(write=False)
    B.setflags(write=False)
    return L, B
