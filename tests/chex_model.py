"""The numpy model of chol_chex_tile (LINPACK DCHEX without Z): the specification of the library's arithmetic.  L is
the Lower factor of M; the result is the factor of P^T M P, P the circular shift of the variables k..l (1-based).

job 2 (left shift, variable k moves down to l): the chud of one vector, sigma = +1, on the columns k..l-1 alone
(chud_model.py spells a rotation).  The vector is the moved variable's old column, the columns are their right
neighbours moved up by one row, with a zero in the moved variable's new row:

    v_i = L(i+1,k) (k <= i < l),  v_l = L(k,k),  v_i = L(i,k) (i > l)
    W(i,j) = L(i+1,j+1) (j <= i < l),  W(l,j) = 0,  W(i,j) = L(i,j+1) (i > l)          for j = k..l-1
    j = k..l-1 in order: column j of W rotated against v -> L'(.,j);   then L'(i,l) = v_i, i >= l

job 1 (right shift, variable l moves up to k): the rotations come from the moved row alone,

    y = L(l,l);  i = l-1 down to k:  x = L(l,i);  rho_i = sqrt(x x + y y);  cc_i = y / rho_i;  ss_i = x / rho_i;  y = rho_i

and every other old row r >= k, whose new row is r' = r + 1 (r < l) or r (r > l), takes them from right to left:

    b = L(r,l) (r > l) or +0 (r < l);  i = min(r, l-1) down to k:  a = L(r,i);
        L'(r',i+1) = cc_i a - (ss_i b);   b = ss_i a + cc_i b;           finally L'(r',k) = b
    L'(k,k) = rho_k

In both jobs the columns before k have their rows k..l permuted and nothing else, and the rows before k and the
columns after l are not touched.  A rotation whose squared pivot is not > 0 (or is NaN) stops: info = the 1-based new
column it would have written (job 2: j; job 1: i + 1).

Every operation is rounded to `dtype`.  The device forms each `a b + c` with one fused multiply-add; `fused=True`
imitates that for float32 (the product and the sum in float64, rounded once).

decoupled_case: factors on which every rotation is the identity, so that the result is the permuted factor bit for
bit; permutation: the new order of the variables."""
import numpy as np


def permutation(n, k, l, job):
    """p (0-based): new variable i is old variable p[i]"""
    p = list(range(n))
    w = p[k - 1:l]
    p[k - 1:l] = ([w[-1]] + w[:-1]) if job == 1 else (w[1:] + [w[0]])
    return np.array(p)


def chex_model(L, k, l, job, dtype=np.float64, fused=False):
    """L: a Lower Cholesky factor (its lower triangle is used); 1 <= k <= l <= n, job 1 or 2.  -> (info, L'): info 0
    and the shifted factor, or the column at which a rotation stopped (L' is then partly made)."""
    dt = np.dtype(dtype).type
    Lo = np.tril(np.asarray(L)).astype(dt)
    n = Lo.shape[0]
    assert 1 <= k <= l <= n and job in (1, 2)
    N = Lo.copy()
    if k == l:
        return 0, N
    k0, l0 = k - 1, l - 1
    wide = np.float64 if fused and dt is np.float32 else None

    def muladd(a, b, c):  # a * b + c
        if wide is None:
            return a * b + c
        return (wide(a) * np.asarray(b, dtype=wide) + np.asarray(c, dtype=wide)).astype(dt)

    N[k0:l + 0, :k0] = Lo[permutation(n, k, l, job)[k0:l], :k0]
    N[k0:, k0:l] = 0
    if job == 2:
        v = np.zeros(n, dtype=dt)
        v[k0:l0] = Lo[k0 + 1:l, k0]
        v[l0] = Lo[k0, k0]
        v[l:] = Lo[l:, k0]
        for j in range(k0, l0):
            col = np.zeros(n, dtype=dt)
            col[j:l0] = Lo[j + 1:l, j + 1]
            col[l:] = Lo[l:, j + 1]
            ljj, vj = col[j], v[j]
            d2 = dt(muladd(vj, vj, ljj * ljj))
            if not d2 > 0:
                return j + 1, N
            rr = np.sqrt(d2)
            c, s, ci = rr / ljj, vj / ljj, ljj / rr
            col[j] = rr
            col[j + 1:] = muladd(s, v[j + 1:], col[j + 1:]) * ci
            v[j + 1:] = muladd(-s, col[j + 1:], c * v[j + 1:])
            N[j:, j] = col[j:]
        N[l0:, l0] = v[l0:]
        return 0, N
    # job 1
    y = Lo[l0, l0]
    cc, ss = np.ones(n, dtype=dt), np.zeros(n, dtype=dt)
    for i in range(l0 - 1, k0 - 1, -1):
        x = Lo[l0, i]
        d2 = dt(muladd(x, x, y * y))
        if not d2 > 0:
            return i + 2, N
        rho = np.sqrt(d2)
        cc[i], ss[i] = y / rho, x / rho
        y = rho
    b = np.zeros(n, dtype=dt)  # by old row
    b[l:] = Lo[l:, l0]
    new = np.arange(n)
    new[k0:l0] += 1
    for i in range(l0 - 1, k0 - 1, -1):
        r = np.r_[i:l0, l:n]
        a = Lo[r, i]
        N[new[r], i + 1] = muladd(cc[i], a, -(ss[i] * b[r]))
        b[r] = muladd(ss[i], a, cc[i] * b[r])
    r = np.r_[k0:l0, l:n]
    N[new[r], k0] = b[r]
    N[k0, k0] = y
    return 0, N


def decoupled_case(n, k, l, job, seed):
    """a lower-triangular L with a positive diagonal and no -0, on which the shift needs no rotation: job 2: L(k+1..l, k)
    = 0; job 1: L(l, k..l-1) = 0"""
    g = np.random.default_rng(seed)
    L = g.standard_normal((n, n))
    L[L == 0] = 1.0
    L = np.tril(L)
    L[np.arange(n), np.arange(n)] = 1.0 + g.random(n)
    if job == 2:
        L[k:l, k - 1] = 0.0
    else:
        L[l - 1, k - 1:l - 1] = 0.0
    return L
