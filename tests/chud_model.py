"""The numpy model of chol_chud_tile / chol_chdd_tile (LINPACK DCHUD / DCHDD for r vectors): the specification of
the library's arithmetic.  Columns outer, vectors inner; column j, vector t, sigma = +1 (update) or -1 (downdate):

    d2 = L_jj L_jj + sigma v_j v_j;   if not d2 > 0: stop, info = j + 1
    rr = sqrt(d2);  c = rr / L_jj;  s = v_j / L_jj;  ci = L_jj / rr;  L_jj = rr
    i > j:   L_ij = (L_ij + sigma s v_i) ci;   v_i = c v_i - s L_ij   (the new L_ij)

vectorised over the rows i.  Every operation is rounded to `dtype`.  The device forms each `a + b c` with one fused
multiply-add; `fused=True` imitates that for float32 (the product and the sum in float64, rounded once), which is how
the tests measure what the contraction can change.

problem: the inputs that test_chud_host.py and test_gpu_chud.py share."""
import functools

import numpy as np


def chud_model(L, V, sigma, dtype=np.float64, fused=False):
    """L: a Lower Cholesky factor (n x n, its lower triangle is used), V: n x r.  -> (info, L', stop_vector): info 0
    and the factor of L L^T + sigma V V^T (stop_vector -1), or info = j + 1 and the vector at which column j stopped
    (L' is then the partly rotated factor)."""
    dt = np.dtype(dtype).type
    L = np.tril(np.asarray(L)).astype(dt)
    V = np.array(np.asarray(V).reshape(L.shape[0], -1), dtype=dt)
    n, r = V.shape
    sg = dt(sigma)
    wide = np.float64 if fused and dt is np.float32 else None

    def muladd(a, b, c):  # a * b + c
        if wide is None:
            return a * b + c
        return (wide(a) * np.asarray(b, dtype=wide) + np.asarray(c, dtype=wide)).astype(dt)

    for j in range(n):
        for t in range(r):
            ljj, vj = L[j, j], V[j, t]
            d2 = dt(muladd(sg * vj, vj, ljj * ljj))
            if not d2 > 0:
                return j + 1, L, t
            rr = np.sqrt(d2)
            c, s, ci = rr / ljj, vj / ljj, ljj / rr
            L[j, j] = rr
            col, v = L[j + 1:, j], V[j + 1:, t]
            col[:] = muladd(sg * s, v, col) * ci
            v[:] = muladd(-s, col, c * v)
    return 0, L, -1


@functools.lru_cache(maxsize=None)
def problem(n, r, seed):
    """A, V, the factor of A, the factor of A + V V^T"""
    g = np.random.default_rng(seed)
    G = g.standard_normal((n, 2 * n))
    A = G @ G.T
    V = g.standard_normal((n, r)) * np.sqrt(n)
    return A, V, np.linalg.cholesky(A), np.linalg.cholesky(A + V @ V.T)
