"""What test_gpu_conditioning.py, test_gpu_pivot_info.py and test_conditioning_host.py share: the parameter rows of either
dtype, the inputs built from them, the bounds, and the assertion helpers that take the factorisation under test as a
callable -- the GPU tests hand them the library, the host test the oracle, a numpy Cholesky and that Cholesky with one
fault.  A plain module like chol_testkit.py: numpy alone to import, no fixtures, no hooks.

fp32 rows: the fp64 construction rounded to fp32 first; every reference quantity (kappa, the high-precision factor and
solve) is computed in fp64 from that rounded input; info and special values follow the oracle's scalar fp32 code.  The
fp32 parameters keep B eps cond where the fp64 rows have it (a few 1e-3 to a few 1e-2)."""
import numpy as np

import dyadic_model as dm
from chol_testkit import bits, lower_of, npdt, other_triangle_kept, spd_spectral, stored_sym

DTYPES = ("d", "s")


def eps_of(dt):
    return float(np.finfo(npdt(dt)).eps)


def rounded(A, dt):
    """A in the dtype of dt, Fortran order (fp64: A itself, copied)"""
    return np.array(A, dtype=npdt(dt), order="F")


def wide(A):
    """the entries as they are, in fp64, Fortran order"""
    return np.array(A, dtype=np.float64, order="F")


def has_subnormal(A):
    a = np.abs(A[np.isfinite(A)])
    return bool(((a > 0) & (a < np.finfo(A.dtype).tiny)).any())


def oracle_potrf(orc, dt):
    return orc.dpotrf if dt == "d" else orc.spotrf


def rows(table, fmt=lambda r: "-".join(str(x) for x in r)):
    """(dt, *row) for every row of table[dt], and the ids: the fp64 rows keep the ids they had before the file ran in two
    dtypes, the fp32 rows carry an s in front"""
    params = [(dt,) + tuple(r) for dt in DTYPES for r in table[dt]]
    return params, [fmt(p[1:]) if p[0] == "d" else "s-" + fmt(p[1:]) for p in params]


# ---------------------------------------------------------------- the parameter rows
TILE_KAPPA = {"d": [(B, k) for k in (1e2, 1e6, 1e10, 1e13) for B in (128, 256, 512)],
              "s": [(B, k) for k in (1e1, 1e2, 1e3, 1e4) for B in (128, 256, 512)] + [(128, 1e5)]}
GRADED = {"d": [(B, k) for k in (6, 13, 20) for B in (128, 512)], "s": [(B, k) for k in (3, 6, 9) for B in (128, 512)]}
TRIANGULAR = {"d": [(1e3,), (1e8,), (1e12,)], "s": [(1e1,), (1e3,), (1e5,)]}
FULL_KAPPA = {"d": [(1024, 256, 1e2), (1024, 256, 1e6), (1024, 256, 1e10), (2048, 512, 1e8), (1536, 128, 1e9)],
              "s": [(1024, 256, 1e1), (1024, 256, 1e2), (1024, 256, 1e3), (2048, 512, 1e2), (1536, 128, 1e3)]}
FULL_GRADED = {"d": [(1024, 256, 13), (2048, 512, 24)], "s": [(1024, 256, 6), (2048, 512, 12)]}
RANGE = {"d": [(B, e) for e in (-1010, -960, 960, 1010) for B in (64, 128, 384)],
         "s": [(B, e) for e in (-105, -90, 100, 114) for B in (64, 128, 384)]}
RANGE_ID = lambda r: f"{r[1]}-{r[0]}"  # noqa: E731  (these rows have always had the exponent in front)
NAN_TILE = {"d": [(64,), (256,), (512,)], "s": [(64,), (256,), (512,)]}
# subnormal pivots at column 0, B // 2 and B - 1, and the subnormal pivot / the column below it of the last case
SPECIAL_PIVOTS = {"d": (1e-310, 4e-320, 1e-315), "s": (1e-40, 3e-45, 1e-42)}
SPECIAL_COLUMN = {"d": (3e-312, 1e-157), "s": (3e-41, 1e-20)}
NAN_WHOLE = ((700, 100), (300, 299), (1023, 0), (600, 520))
RESIDUAL_F = {"d": 1e-13, "s": 5e-5}  # the stated normwise residual of a whole factorisation


def substitution_floor(dt):
    """the floor under "as good as substitution": 1e-15 in fp64, the same multiple of eps in fp32"""
    return 1e-15 / eps_of("d") * eps_of(dt)


# ---------------------------------------------------------------- inputs
def spd_graded(n, decades, seed):
    """D A0 D with A0 well conditioned and D = powers of two falling over `decades` decades: the
    leading blocks of L = D L0 have kappa up to 10^decades while the problem stays well posed.
    Returns (A, A0, d)."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    A0 = M @ M.T / n + np.eye(n)
    d = 2.0 ** (-np.round(np.linspace(0, decades * np.log2(10.0), n)))
    return np.asfortranarray(d[:, None] * A0 * d[None, :]), A0, d


def tile_kappa_input(dt, B, kappa):
    """-> (Akk, A10, A11) of Q diag(logspace) Q^T of order 2 B"""
    A = rounded(spd_spectral(2 * B, kappa, seed=int(np.log10(kappa)) * 1000 + B), dt)
    return np.asfortranarray(A[:B, :B]), np.asfortranarray(A[B:, :B]), np.asfortranarray(A[B:, B:])


def graded_input(dt, n, decades, seed):
    """-> (A, A0, d): A in dt; A0 the equilibrated matrix A stands for (fp32: of the rounded A, the scaling being exact)"""
    A, A0, d = spd_graded(n, decades, seed)
    A = rounded(A, dt)
    if dt != "d":
        A0 = wide(A) / d[:, None] / d[None, :]
    return A, A0, d


def triangular_input(dt, kl, B=256):
    """-> (Lm, A): the triangular factor of U diag(logspace(0, -log10 kl)) V^T with a NaN strict upper triangle, and a
    right-hand side"""
    rng = np.random.default_rng(int(np.log10(kl)))
    U, _ = np.linalg.qr(rng.standard_normal((B, B)))
    V, _ = np.linalg.qr(rng.standard_normal((B, B)))
    _, R = np.linalg.qr(((U * np.logspace(0, -np.log10(kl), B)) @ V.T).T)
    Lm = rounded(R.T + np.triu(np.full((B, B), np.nan), 1), dt)  # strict upper: stale, must not be read
    return Lm, rounded(rng.uniform(-1, 1, (B, B)), dt)


def range_input(orc, dt, B, scale_exp):
    """-> (A, X): the reference input's leading tile and the tile below it, scaled by 2^scale_exp"""
    A = rounded(np.ldexp(orc.extract_block(orc.reference_input(B), B, 0, 0), scale_exp), dt)
    X = rounded(np.ldexp(orc.extract_block(orc.reference_input(2 * B), B, 1, 0), scale_exp), dt)
    return A, X


def special_pivot_cases(dt, B):
    """diag(linspace(1, 2)) with one pivot subnormal or +Inf"""
    p0, p1, p2 = SPECIAL_PIVOTS[dt]
    for j, v in ((0, p0), (B // 2, p1), (B - 1, p2), (1, np.inf), (B - 1, np.inf)):
        A = np.asfortranarray(np.diag(np.linspace(1.0, 2.0, B)))
        A[j, j] = v
        if j + 1 < B:
            A[j + 1, j] = A[j, j + 1] = 0.0
        yield j, v, rounded(A, dt)


def special_column_input(orc, dt, B=64):
    """a subnormal pivot with a non-trivial column below it: L(i,j) = a(i,j) / sqrt(tiny) is large but finite"""
    pivot, scale = SPECIAL_COLUMN[dt]
    A = np.asfortranarray(orc.extract_block(orc.reference_input(B), B, 0, 0))
    A[0, 0] = pivot
    A[1:, 0] = A[0, 1:] = np.linspace(-1.0, 1.0, B - 1) * scale  # |a(i,0)| < sqrt(a(0,0) a(i,i))
    return rounded(A, dt)


def nan_tile_positions(B):
    return [(5, 3), (B - 1, 0), (B // 2, B // 2), (B - 1, B - 2), (0, 0), (B // 2 + 3, B // 2 - 5)]


# ---------------------------------------------------------------- bounds
def potrf_backward_ok(L, A, B, eps=eps_of("d")):
    L = np.tril(wide(L))
    E = np.abs(np.tril(L @ L.T - wide(A)))
    bound = 8 * B * eps * (np.abs(L) @ np.abs(L).T)
    return bool((E <= bound + 1e-300).all()), float((E / (bound + 1e-300)).max())


def trsm_backward_ok(X, L, A, B, eps=eps_of("d")):
    X, L, A = wide(X), np.tril(wide(L)), wide(A)
    E = np.abs(X @ L.T - A)
    bound = 8 * B * eps * (np.abs(X) @ np.abs(L).T + np.abs(A))
    return bool((E <= bound + 1e-300).all()), float((E / (bound + 1e-300)).max())


def forward_active(dt, what, factor):
    """is a forward-error assertion with the bound `factor` x max|ref| worth making?  fp64: always, as before.  fp32: where
    16 B eps kappa <= 1/8; beyond that the bound allows an error of the size of the result, and a line says so"""
    if dt == "d" or factor <= 0.125:
        return True
    print(f"{what}: forward bound vacuous (16 B eps kappa = {factor:.3g} > 1/8), not asserted")
    return False


# ---------------------------------------------------------------- helpers on a factorisation handed in as a callable
# potrf(A) -> (info, F): the lower Cholesky factorisation of one tile in A's dtype, A left alone, the strict upper
# triangle of F as A had it
def check_special_pivots(potrf, orc, dt, sizes=(4, 64, 128)):
    """A subnormal pivot is a positive pivot (LAPACK: sqrt, divide); +Inf passes `ajj > 0` too.
    Whatever the oracle's scalar code makes of them, the factorisation under test must make the same."""
    EPS = eps_of(dt)
    for B in sizes:
        for j, v, A in special_pivot_cases(dt, B):
            info, L = potrf(A)
            Lref, iref = oracle_potrf(orc, dt)(A)
            assert info == iref, (B, j, v, info, iref)
            a, b = np.tril(L), np.tril(Lref)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (B, j, v)
            m = np.isfinite(b)
            assert np.allclose(a[m], b[m], rtol=8 * EPS, atol=0.0), (B, j, v)


def check_special_column(potrf, orc, dt, B=64):
    EPS = eps_of(dt)
    A = special_column_input(orc, dt, B)
    info, L = potrf(A)
    Lref, iref = oracle_potrf(orc, dt)(A)
    assert info == iref == 0
    assert np.abs(np.tril(wide(L)) - np.tril(wide(Lref))).max() <= 16 * B * EPS * np.abs(Lref).max()
    assert abs(float(L[0, 0]) - float(Lref[0, 0])) <= 4 * EPS * float(Lref[0, 0])


def check_nan_info(potrf, orc, dt, B):
    """a NaN anywhere in the lower triangle: the oracle's info, and it is positive"""
    base = rounded(orc.extract_block(orc.reference_input(B), B, 0, 0), dt)
    for (i, j) in nan_tile_positions(B):
        A = base.copy(order="F")
        A[i, j] = np.nan
        info, _ = potrf(A)
        _, iref = oracle_potrf(orc, dt)(A)
        assert info == iref and info > 0, (B, i, j, info, iref)
    return base


# ---------------------------------------------------------------- the failing pivot's position, on exact data
# factor(S, u) -> (info, F): the `u` factorisation of the symmetric matrix stored in the `u` triangle of S (the other
# strict triangle NaN), in S's dtype, S left alone
ONE_TILE = (128, 256, 200)  # (200: the staged, padded path)
WHOLE = [("mirror", 1024, 256), ("mirror", 1000, 192), ("mod3", 1024, 256), ("mod3", 1000, 192), ("panel", 1024, 256)]
PIVOT_SHAPES = [(fam, B, B) for fam in ("mirror", "mod3") for B in ONE_TILE] + WHOLE
# the tiny pivot is 2^-20 in the last diagonal entry, beside the integer sum of squares of the factor's last row: fp32
# holds that only where the row is empty -- the odd last rows of mirror, the last rows = 0 (mod 3) of mod3
TINY_SHAPES = [(fam, n, B) for fam, n, B in PIVOT_SHAPES
               if fam == "mirror" and n % 2 == 0 or fam == "mod3" and (n - 1) % 3 == 0]
FORCED = ("mirror", 1024, 256, 700)  # the case of the forced chain forms: (family, n, B, column)


def pivot_member(fam, n, B):
    """(A, L, s) of dyadic_model.cholesky_case(n, seed n, 2, family, B)"""
    return dm.cholesky_case(n, n, 2, fam, B if fam == "panel" else None)


def pivot_columns(n, B):
    """the 16-panel and 128-block boundaries of the pivot chain, the tile boundary, one column in a middle tile, the first
    column of the (ragged) last tile, the last column"""
    nt = -(-n // B)
    cols = {0, 15, 16, 127, 128, B - 1, B, (nt // 2) * B + B // 2 + 5, (nt - 1) * B, n - 1}
    return sorted(c for c in cols if 0 <= c < n)


def perturbed(A, s, j, kind):
    """A with its pivot j made exactly 0 ("zero"), exactly -1 ("minus") or 2^-20 ("tiny"); fp64, every entry still a
    short dyadic number"""
    P = np.array(A, dtype=np.float64, order="F")
    P[j, j] -= {"zero": s[j] ** 2, "minus": s[j] ** 2 + 1, "tiny": s[j] ** 2 - 2.0 ** -20}[kind]
    return P


def stored_exactly(P, dt, u):
    """P's `u` triangle in dt with a NaN other triangle, having checked that dt holds every entry exactly"""
    S = stored_sym(P.astype(npdt(dt)), u)
    keep = ~np.isnan(S)
    assert np.array_equal(S[keep].astype(np.float64), P[keep]), "the dtype does not hold the perturbed member"
    return S


def failing_block_start(j, B):
    """the first column of the 128-block (of its tile) that holds column j"""
    return j // B * B + j % B // dm.NB * dm.NB


def check_pivot_positions(factor, fam, n, B, dt, u, cols=None, kinds=("zero", "minus")):
    """pivot j exactly 0 / exactly -1 with exact arithmetic before it: info == j + 1 whatever the summation order, the
    other triangle bit for bit; printed, not asserted: whether the columns before the failing 128-block are L's"""
    A, L, s = pivot_member(fam, n, B)
    Ld = L.astype(npdt(dt))
    for j in (pivot_columns(n, B) if cols is None else cols):
        for kind in kinds:
            S = stored_exactly(perturbed(A, s, j, kind), dt, u)
            info, F = factor(S, u)
            assert info == j + 1, (fam, n, B, dt, u, kind, j, info)
            assert other_triangle_kept(F, S, u), (fam, n, B, dt, u, kind, j)
            j0 = failing_block_start(j, B)
            print(f"{fam} n={n} B={B} {dt} {u} {kind} j={j}: info {info}, columns before {j0} equal L: "
                  f"{np.array_equal(lower_of(F, u)[:, :j0], Ld[:, :j0])}")


def check_tiny_last_pivot(factor, fam, n, B, dt, u):
    """the last pivot exactly 2^-20 and nothing scaled by it: info == 0, L[n-1, n-1] == 2^-10 and the rest of L, bit for
    bit"""
    A, L, s = pivot_member(fam, n, B)
    S = stored_exactly(perturbed(A, s, n - 1, "tiny"), dt, u)
    want = L.astype(npdt(dt))
    want[n - 1, n - 1] = 2.0 ** -10
    info, F = factor(S, u)
    assert info == 0, (fam, n, B, dt, u, info)
    got = lower_of(F, u)
    assert bits(got[n - 1:, n - 1])[0] == bits(want[n - 1:, n - 1])[0], (fam, n, B, dt, u, float(got[n - 1, n - 1]))
    assert np.array_equal(got, want), (fam, n, B, dt, u, int((got != want).sum()))  # (by value: the family's zeros are signed)
    assert other_triangle_kept(F, S, u), (fam, n, B, dt, u)
