"""The numpy model of chol_symm_tile (BLAS DSYMM, side Left): C <- alpha A B + beta C with A read from one stored
triangle, and the cases that test_symm_host.py proves and test_gpu_symm.py runs.

Exact family: A symmetric with integer entries in [-4, 4], B integer in [-4, 4], C integer in [-8, 8], the scalars of
SCALARS.  Every partial sum of alpha A B + beta C is then a multiple of 1/2 whose magnitude is at most
|alpha| (|A| |B|) + |beta| |C|; where that is below 2^23 (test_symm_host.py asserts it for every case) every such sum is
a number of fp32, so any summation order, with or without fma, returns the integer result bit for bit.

Random family: A symmetric standard normal, B and C standard normal, alpha = -1.5, beta = 0.75."""
import functools

import numpy as np

# (n, tile): three block rows (a stored block, the diagonal, a mirrored block); two 128-blocks inside a tile; a ragged
# order with the tile edge padded to 256; one tile larger than the matrix; five block rows
SHAPES = [(384, 128), (512, 256), (333, 192), (100, 128), (640, 128)]
# 129: one column past a 128-wide block; 300: three tile columns of B and C at tile 128
NRHS = (1, 8, 129, 300)
SCALARS = ((1.0, 0.0), (-2.0, 1.0), (0.5, -1.0))
RANDOM_SCALARS = (-1.5, 0.75)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def exact_problem(n):
    """-> integer (A symmetric n x n, B, C n x max(NRHS)) in fp64 (read-only)"""
    r = np.random.default_rng(7000 + n)
    G = r.integers(-4, 5, size=(n, n))
    A = np.tril(G) + np.tril(G, -1).T
    B = r.integers(-4, 5, size=(n, max(NRHS)))
    C = r.integers(-8, 9, size=(n, max(NRHS)))
    return _frozen(A.astype(np.float64), B.astype(np.float64), C.astype(np.float64))


@functools.lru_cache(maxsize=None)
def random_problem(n):
    """-> (A symmetric, B, C) standard normal in fp64 (read-only)"""
    r = np.random.default_rng(9000 + n)
    G = r.standard_normal((n, n))
    A = np.tril(G) + np.tril(G, -1).T
    return _frozen(A, r.standard_normal((n, max(NRHS))), r.standard_normal((n, max(NRHS))))


def symm(S, u, alpha, B, beta, C):
    """the routine on the stored triangle S alone (BLAS's rules for the scalars), in the dtype of B"""
    T = np.tril(S) if u == "L" else np.triu(S)
    A = T + (np.tril(S, -1).T if u == "L" else np.triu(S, 1).T)
    dt = B.dtype.type
    if alpha == 0:
        return np.zeros_like(C) if beta == 0 else dt(beta) * C
    P = dt(alpha) * (A.astype(dt) @ B)
    return P if beta == 0 else P + dt(beta) * C


def magnitude(A, B, C, alpha, beta):
    """max over the entries of |alpha| (|A| |B|) + |beta| |C|: what bounds every partial sum of the result"""
    return float((abs(alpha) * (np.abs(A) @ np.abs(B)) + abs(beta) * np.abs(C)).max())
