"""A numpy model of the symmetric random butterfly transformation behind chol_sytrf_rbt_tile / chol_sytrs_rbt_tile /
chol_sysv_rbt_tile / chol_rbt_apply_tile, in the dtype's arithmetic and in the kernels' order of operations.

A butterfly of order 2h over the rows o .. o+2h-1 is B = 2^(-1/2) [[R0, R1], [R0, -R1]], R0 = diag(w[o : o+h]),
R1 = diag(w[o+h : o+2h]).  The recursive butterfly of depth d is W = D_(d-1) ... D_0: D_0 one butterfly of order n, D_k
block diagonal with 2^k butterflies of order n / 2^k; column k of the n x d array Wcols is the w of level k.  So
W^T A W applies the level of the smallest butterflies first.

The four-number map (rbt.hip).  For the row butterfly p and the column butterfly q of a level, with
A(p,q) = [[a11, a12], [a21, a22]] in h x h quarters, entry (i,j) of every quarter:
    s1 = a11 + a21   d1 = a11 - a21   s2 = a12 + a22   d2 = a12 - a22
    c11 = (r0p_i r0q_j) ((s1 + s2) / 2)      c12 = (r0p_i r1q_j) ((s1 - s2) / 2)
    c21 = (r1p_i r0q_j) ((d1 + d2) / 2)      c22 = (r1p_i r1q_j) ((d1 - d2) / 2)
On a diagonal block (p == q) only the lower triangle is stored: a12(i,j) is a21(j,i), the groups i >= j cover it, the
group (i,j), i > j, writes c12 to the place of a21(j,i), and a group (i,i) writes c21 there.  Vectors: B^T x is
y1 = r0 ((x1 + x2) c), y2 = r1 ((x1 - x2) c); B x is t1 = r0 x1, t2 = r1 x2, y1 = (t1 + t2) c, y2 = (t1 - t2) c;
c = 2^(-1/2) rounded to the dtype."""
import numpy as np

from sytrf_model import sytrf_model, sytrs_model


def butterfly_dense(Wcols, depth):
    """the dense W = D_(depth-1) ... D_0 in fp64 (exact 2^(-1/2) up to fp64 rounding), for checking"""
    Wcols = np.asarray(Wcols, dtype=np.float64)
    n = Wcols.shape[0]
    assert n % (1 << depth) == 0
    W = np.eye(n)
    for k in range(depth):  # W = D_(d-1) ... D_1 D_0: D_0 rightmost
        m = n >> k
        h = m // 2
        D = np.zeros((n, n))
        for b in range(1 << k):
            o = b * m
            r0, r1 = Wcols[o:o + h, k], Wcols[o + h:o + m, k]
            D[o:o + h, o:o + h] = np.diag(r0)
            D[o:o + h, o + h:o + m] = np.diag(r1)
            D[o + h:o + m, o:o + h] = np.diag(r0)
            D[o + h:o + m, o + h:o + m] = -np.diag(r1)
        W = (D / np.sqrt(2.0)) @ W
    return W


def _four(a11, a21, a12, a22, r0p, r1p, r0q, r1q):
    half = a11.dtype.type(0.5)
    s1, d1, s2, d2 = a11 + a21, a11 - a21, a12 + a22, a12 - a22
    c11 = np.outer(r0p, r0q) * ((s1 + s2) * half)
    c21 = np.outer(r1p, r0q) * ((d1 + d2) * half)
    c12 = np.outer(r0p, r1q) * ((s1 - s2) * half)
    c22 = np.outer(r1p, r1q) * ((d1 - d2) * half)
    return c11, c21, c12, c22


def rbt_level(L, w, level):
    """one level D^T A D on the lower triangle L of A (the strict upper triangle of L is not read) -> the new lower
    triangle"""
    dt = L.dtype
    n = L.shape[0]
    m = n >> level
    h = m // 2
    w = np.asarray(w, dtype=dt)
    M = np.tril(L) + np.tril(L, -1).T
    N = np.zeros_like(M)
    for p in range(1 << level):
        op = p * m
        rp = slice(op, op + h), slice(op + h, op + m)
        for q in range(p + 1):
            oq = q * m
            cq = slice(oq, oq + h), slice(oq + h, oq + m)
            a11, a21, a22 = M[rp[0], cq[0]], M[rp[1], cq[0]], M[rp[1], cq[1]]
            a12 = a21.T if p == q else M[rp[0], cq[1]]
            c11, c21, c12, c22 = _four(a11, a21, a12, a22, w[rp[0]], w[rp[1]], w[cq[0]], w[cq[1]])
            if p == q:
                N[rp[0], cq[0]] = np.tril(c11)
                N[rp[1], cq[1]] = np.tril(c22)
                N[rp[1], cq[0]] = np.tril(c21) + np.triu(c12.T, 1)
            else:
                N[rp[0], cq[0]], N[rp[1], cq[0]], N[rp[0], cq[1]], N[rp[1], cq[1]] = c11, c21, c12, c22
    return np.tril(N)


def rbt_sym(A, Wcols, depth):
    """the lower triangle of W^T A W from the lower triangle of A, in A's dtype: level depth-1 first, level 0 last"""
    L = np.tril(np.asarray(A))
    for k in range(depth - 1, -1, -1):
        L = rbt_level(L, Wcols[:, k], k)
    return L


def rbt_vec(X, Wcols, depth, trans):
    """W^T X (trans: level depth-1 first) or W X (level 0 first), in X's dtype"""
    X = np.array(X, copy=True)
    dt = X.dtype
    n = X.shape[0]
    c = dt.type(np.sqrt(0.5))
    for x in range(depth):
        k = depth - 1 - x if trans else x
        m = n >> k
        h = m // 2
        w = np.asarray(Wcols[:, k], dtype=dt)
        for b in range(1 << k):
            o = b * m
            r0 = w[o:o + h].reshape((h,) + (1,) * (X.ndim - 1))
            r1 = w[o + h:o + m].reshape((h,) + (1,) * (X.ndim - 1))
            x1, x2 = X[o:o + h].copy(), X[o + h:o + m].copy()
            if trans:
                X[o:o + h] = r0 * ((x1 + x2) * c)
                X[o + h:o + m] = r1 * ((x1 - x2) * c)
            else:
                t1, t2 = r0 * x1, r1 * x2
                X[o:o + h] = (t1 + t2) * c
                X[o + h:o + m] = (t1 - t2) * c
    return X


def backward_error(A, x, b):
    """per column: max |b - A x| / (||A||_inf max |x|), in fp64"""
    A = np.asarray(A, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(A.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(A.shape[0], -1)
    return np.abs(b - A @ x).max(0) / (np.abs(A).sum(1).max() * np.abs(x).max(0))


def sysv_rbt_model(A, Wcols, depth, B, b, itmax=10):
    """chol_sysv_rbt_tile: the blocked L D L^T (tile B) of W^T A W, the solve, and refinement with DSPOSV's stopping
    rule -> dict(info, x, iter, berr (final, per column), berr0 (unrefined), max_l, F)"""
    A = np.asarray(A)
    dt = A.dtype
    n = A.shape[0]
    b = np.asarray(b, dtype=dt).reshape(n, -1)
    F, info = sytrf_model(rbt_sym(A, Wcols, depth), B)
    out = dict(info=info, F=F, x=None, iter=-3, berr=None, berr0=None, max_l=np.abs(np.tril(F, -1)).max())
    if info:
        return out

    def solve(r):
        return rbt_vec(sytrs_model(F, rbt_vec(r, Wcols, depth, True)), Wcols, depth, False)

    Ad = A.astype(np.float64)
    anrm = np.abs(Ad).sum(1).max()
    eps = 2.0 ** -53 if dt == np.float64 else 2.0 ** -24
    cte = anrm * eps * np.sqrt(n)
    x = solve(b)
    for it in range(itmax + 1):
        r = (b.astype(np.float64) - Ad @ x.astype(np.float64)).astype(dt)
        rn, xn = np.abs(r).max(0), np.abs(x).max(0)
        berr = rn / (anrm * xn)
        if it == 0:
            out["berr0"] = berr
        out["berr"], out["x"] = berr, x
        if np.all(rn <= xn * cte):
            out["iter"] = it
            return out
        if it == itmax:
            out["iter"] = -31
            return out
        x = x + solve(r)
    return out


def family(name, n, seed):
    """the test matrices (fp64, symmetric, indefinite): "zero_diag" random symmetric with a zero diagonal; "saddle"
    [[0, J], [J^T, H]] with a zero (1,1) block of order n / 4, H = G G^T / (n - m), J = randn / sqrt(n); "randsym"
    random symmetric"""
    r = np.random.default_rng(seed)
    if name == "zero_diag":
        A = r.standard_normal((n, n))
        A = (A + A.T) / 2
        np.fill_diagonal(A, 0.0)
    elif name == "saddle":
        m = n // 4
        G = r.standard_normal((n - m, n - m))
        J = r.standard_normal((m, n - m)) / np.sqrt(n)
        A = np.block([[np.zeros((m, m)), J], [J.T, G @ G.T / (n - m)]])
    elif name == "randsym":
        A = r.standard_normal((n, n))
        A = (A + A.T) / 2
    else:
        raise KeyError(name)
    return A


def random_w(n, depth, seed, dtype=np.float64):
    """entries exp(r / 10), r uniform in [-1/2, 1/2] (numpy's generator: for the host tests; the library's own W is
    read back from its descriptor)"""
    r = np.random.default_rng(seed)
    return np.exp(r.uniform(-0.5, 0.5, (n, depth)) / 10).astype(dtype)
