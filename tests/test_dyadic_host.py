"""The dyadic input families (dyadic_model.py) are exact for the blocked algorithms in fp32 and fp64: the numpy
emulations return the known answers bit for bit at every order the GPU tests (test_gpu_chain_exact.py,
test_gpu_factor_exact.py) use, and 16 times the largest partial sum any summation order can reach (four fractional bits
of headroom) stays below 2^24, the range in which fp32 holds such numbers exactly.  No GPU.

The rule: a (routine, family, order, dtype) may appear in a GPU test only if a test here proves it.  The lists of the new
families below are therefore taken from the GPU tests' own parameters (the modules import without a GPU)."""
import numpy as np
import pytest

import dyadic_model as dm
import test_gpu_chain_exact as chain
import test_gpu_factor_exact as factor

POTRF_ORDERS = [128, 200, 256, 512, 700, 1000, 1024, 1100, 1536, 2048, 4096]
LDL_ORDERS = [700, 1000, 1024, 1536]
SYGST_ORDERS = [1000, 1024, 1100, 1536]
LIMIT = 2.0 ** 24 / 16

DTYPES = [np.float32, np.float64]


def fam_kw(fam):
    """(the panel mask is the same for every tile size of whole 128-blocks -- test_the_family_is_what_it_says --
    so a proof at B = 128 covers them all)"""
    return {} if fam == "parity" else {"family": fam, "B": 128} if fam == "panel" else {"family": fam}


def new_family_orders(*lists):
    """the distinct (family, order) of the GPU tests' parameters (family, ..., N, B) outside the parity family"""
    seen = sorted({(p[0], p[-2]) for ps in lists for p in ps if p[0] != "parity"})
    assert all(p[-1] % 128 == 0 for ps in lists for p in ps if p[0] == "panel")
    return seen


NEW_POTRF = new_family_orders(chain.CASES, chain.UPPER[0], chain.WAVE[0], [(f, b, b) for f, b in chain.ONE_TILE[0]],
                              [(f, b, b) for f, b in chain.FILL_CASES], factor.SOLVES["argvalues"],
                              factor.SOLVES_FP64_ONLY["argvalues"], factor.INVERSES["argvalues"])
NEW_LDL = new_family_orders(factor.LDL["argvalues"], factor.LDL_FP64_ONLY["argvalues"])
# (family, order, tile size), every family: sygst and the backward sweep of the solves invert whole tiles
SYGST_TILES = factor.SYGST["argvalues"]
SOLVE_TILES = factor.SOLVES["argvalues"]
LDL_TILES = factor.LDL["argvalues"]
NEW_SOLVES = new_family_orders(factor.SOLVES["argvalues"])
NEW_INVERSES = new_family_orders(factor.INVERSES["argvalues"])
NEW_ONE_TILE = new_family_orders([(f, b, b) for f, b in chain.ONE_TILE[0]])


def test_the_family_is_what_it_says():
    n = 777
    N = dm.nn(n, n)
    i, j = np.nonzero(N)
    assert (i % 2 == 1).all() and (j % 2 == 0).all() and (i > j).all()
    assert set(np.unique(N)) == {-1.0, 0.0, 1.0}
    dens = len(i) / (((np.arange(n)[:, None] % 2 == 1) & (np.arange(n)[None, :] % 2 == 0) & (np.arange(n)[:, None] > np.arange(n)[None, :])).sum())
    assert 0.45 < dens < 0.55
    assert not np.any(N @ N)
    A, L, s = dm.cholesky_case(n, n)
    assert set(np.unique(s)) == {1.0, 2.0} and np.array_equal(A, A.T)
    assert np.array_equal(dm.inv_factor(n, n) @ L, np.eye(n))
    assert np.array_equal(dm.inv_spd(n, n) @ A, np.eye(n))
    assert np.array_equal(dm.inv_spd(n, n) * 4, np.round(dm.inv_spd(n, n) * 4))
    # every aligned 16-, 64- and 128-block of the factor has a dense inverse of magnitude <= 1 (times 1 / s)
    for nb in (16, 64, 128):
        W = np.linalg.inv(L[256:256 + nb, 256:256 + nb])
        assert np.abs(W).max() <= 1 and np.count_nonzero(np.tril(W, -1)) >= nb * nb // 24
    A, L, d = dm.ldl_case(n, n)
    assert set(np.unique(np.abs(d))) == {1.0, 2.0, 4.0} and (d < 0).any() and (d > 0).any()
    A, L, M = dm.sygst_case(n, n)
    X = dm.inv_factor(n, n)
    assert np.array_equal(X @ A @ X.T, M) and np.abs(M).max() == 3
    assert np.abs(dm.solution(n, 5, n)).max() == 3
    the_new_families_are_what_they_say()


def the_new_families_are_what_they_say():
    n = 777
    i = np.arange(n)
    r, c = i[:, None], i[None, :]
    draws = dm.nn(n, n) + dm.nn(n, n, "mirror")  # (disjoint masks of the same draws)
    for fam, want, fill in (("mirror", (r % 2 == 0) & (c % 2 == 1) & (r > c), 0.125),
                            ("mod3", (r % 3 > c % 3) & (r > c), 1 / 6),
                            ("panel", ((r // 128 != c // 128) | (r % 3 > c % 3)) & (r > c), 0.46)):
        kw = fam_kw(fam)
        N = dm.nn(n, n, **kw)
        assert np.array_equal(dm.family_mask(n, fam, kw.get("B")), want)
        assert not np.any(N[~want]) and set(np.unique(N)) == {-1.0, 0.0, 1.0}
        assert 0.45 < np.count_nonzero(N) / want.sum() < 0.55
        assert abs(np.count_nonzero(N) / (n * (n - 1) / 2) - fill) < 0.02
        both = want & ((r % 2) != (c % 2))
        assert np.array_equal(N[both], draws[both])  # the same draws as the parity family's, through another mask
        A, L, s = dm.cholesky_case(n, n, **kw)
        assert set(np.unique(s)) == {1.0, 2.0} and np.array_equal(A, A.T) and np.array_equal(L, (np.eye(n) + N) * s)
        assert np.abs(A).max() * 16 < 2.0 ** 24
        _, Lu, d = dm.ldl_case(n, n, **kw)
        assert np.array_equal(Lu, np.eye(n) + N) and set(np.unique(np.abs(d))) == {1.0, 2.0, 4.0}
        A, Ls, M = dm.sygst_case(n, n, **kw)
        assert np.array_equal(Ls, L) and np.array_equal(A, L @ M @ L.T) and np.array_equal(M, M.T)
    # mirror: Nn Nn = 0 again, and the rows and columns the parity family leaves empty carry the entries
    N = dm.nn(n, n, "mirror")
    assert not np.any(N @ N)
    assert N[32::2].any(1).all() and N[:, 1:n - 32:2].any(0).all() and not N[1::2].any() and not N[:, 0::2].any()
    # mod3: Nn^3 = 0 and Nn^2 != 0, for the matrix and inside the aligned 128-blocks; the closed forms
    N = dm.nn(n, n, "mod3")
    assert np.any(N @ N) and not np.any(N @ N @ N)
    for k in range(0, n - 127, 128):
        Nk = N[k:k + 128, k:k + 128]
        assert np.count_nonzero(Nk @ Nk) >= 128 * 128 // 32 and not np.any(Nk @ Nk @ Nk)
    for fam in ("mirror", "mod3"):
        A, L, s = dm.cholesky_case(n, n, family=fam)
        X, Ai = dm.inv_factor(n, n, family=fam), dm.inv_spd(n, n, family=fam)
        assert np.array_equal(X @ L, np.eye(n)) and np.array_equal(L @ X, np.eye(n))
        assert np.array_equal(Ai @ A, np.eye(n)) and np.array_equal(Ai * 4, np.round(Ai * 4))
        _, _, M = dm.sygst_case(n, n, family=fam)
        assert np.array_equal(X @ dm.sygst_case(n, n, family=fam)[0] @ X.T, M)
    assert np.abs(dm.inv_factor(n, n, family="mirror")).max() == 1
    assert 8 <= np.abs(dm.inv_factor(n, n, family="mod3")).max() <= 64  # a second-order term: sums of products
    # panel: the mask does not depend on the tile size; outside the diagonal 128-blocks no mask, inside them mod3 with
    # its second-order inverse; no panel tile has an empty row or column; the global inverse is out of reach
    n = 1024
    N = dm.nn(n, n, "panel", 256)
    for B in (128, 384, 512, 1024):
        assert np.array_equal(dm.family_mask(n, "panel", B), dm.family_mask(n, "panel", 256))
    for B in (None, 0, 192, 200):
        with pytest.raises(ValueError):
            dm.family_mask(n, "panel", B)
    with pytest.raises(ValueError):
        dm.inv_factor(n, n, family="panel")
    for k in range(0, n, 128):
        Nk = N[k:k + 128, k:k + 128]
        assert np.array_equal(Nk != 0, (Nk != 0) & dm.family_mask(n, "mod3")[k:k + 128, k:k + 128])
        assert np.count_nonzero(Nk @ Nk) >= 128 * 128 // 32 and not np.any(Nk @ Nk @ Nk)
        W = np.linalg.inv(np.eye(128) + Nk)
        assert np.array_equal(W, np.eye(128) - Nk + Nk @ Nk) and np.abs(W).max() <= 16
        below = N[k + 128:, k:k + 128]
        assert not below.size or 0.45 < np.count_nonzero(below) / below.size < 0.55
    for B in (128, 256, 512):  # every panel tile (tile row > tile column): no empty row, no empty column
        for a in range(B, n, B):
            for b in range(0, a, B):
                assert N[a:a + B, b:b + B].any(0).all() and N[a:a + B, b:b + B].any(1).all()
    assert np.abs(np.linalg.inv(np.eye(n) + N)).max() > 2.0 ** 30


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", POTRF_ORDERS)
def test_potrf_emulation_is_exact(n, dtype):
    A, L, _ = dm.cholesky_case(n, n)
    assert np.abs(A).max() * 16 < 2.0 ** 24
    Lg, peak = dm.potrf_blocked(A.astype(dtype), dtype)
    assert Lg.dtype == dtype and np.array_equal(Lg, L.astype(dtype))
    assert peak < LIMIT, peak


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam,n", NEW_POTRF)
def test_potrf_emulation_is_exact_on_the_new_families(fam, n, dtype):
    A, L, _ = dm.cholesky_case(n, n, **fam_kw(fam))
    assert np.abs(A).max() * 16 < 2.0 ** 24
    Lg, peak = dm.potrf_blocked(A.astype(dtype), dtype)
    assert Lg.dtype == dtype and np.array_equal(Lg, L.astype(dtype))
    print(fam, n, np.dtype(dtype).name, "potrf peak", peak)
    assert peak < LIMIT, peak


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1024, 1000])
def test_potrf_emulation_is_exact_with_unit_scaling(n, dtype):
    """s = 1: the fall-back of the fp64 cases should the hardware's reciprocal square root be inexact at 4"""
    A, L, s = dm.cholesky_case(n, n, 1)
    assert (s == 1).all()
    Lg, peak = dm.potrf_blocked(A.astype(dtype), dtype)
    assert np.array_equal(Lg, L.astype(dtype)) and peak < LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LDL_ORDERS)
def test_ldl_emulation_is_exact(n, dtype):
    A, L, d = dm.ldl_case(n, n)
    F, peak = dm.ldl_blocked(A.astype(dtype), dtype)
    assert F.dtype == dtype
    assert np.array_equal(np.tril(F, -1), np.tril(L, -1).astype(dtype)) and np.array_equal(np.diag(F), d.astype(dtype))
    assert peak < LIMIT, peak


def sytrs_bound(A, L, d, X):
    """every partial sum of A X and of the sweeps that undo it: L Z = B with Z = D L^T X, then L^T X = inv(D) Z"""
    return max((np.abs(A) @ np.abs(X)).max(), (np.abs(L) @ (np.abs(d)[:, None] * np.abs(L.T @ X))).max(),
               (np.abs(L.T) @ np.abs(X)).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam,n", [("parity", n) for n in LDL_ORDERS] + NEW_LDL)
def test_ldl_emulation_and_its_solves_are_exact_on_every_family(fam, n, dtype):
    A, L, d = dm.ldl_case(n, n, **fam_kw(fam))
    assert np.array_equal(A.astype(dtype).astype(np.float64), A)
    F, peak = dm.ldl_blocked(A.astype(dtype), dtype)
    assert F.dtype == dtype
    assert np.array_equal(np.tril(F, -1), np.tril(L, -1).astype(dtype)) and np.array_equal(np.diag(F), d.astype(dtype))
    X = dm.solution(n, 5, n)
    bound = sytrs_bound(A, L, d, X)
    print(fam, n, np.dtype(dtype).name, "ldl peak", peak, "sytrs bound", bound)
    assert peak < LIMIT, peak
    assert bound < LIMIT and np.array_equal((A @ X).astype(dtype).astype(np.float64), A @ X)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fam,n,B", SYGST_TILES)
def test_sygst_emulation_is_exact_with_the_tile_as_the_block(fam, n, B, dtype):
    """as the library runs it: the block is the tile, and the inverse of the whole diagonal tile of L enters (inv_tile)"""
    A, L, M = dm.sygst_case(n, n, **fam_kw(fam))
    assert np.abs(A).max() * 16 < 2.0 ** 24
    C, peak = dm.sygst_blocked(A.astype(dtype), L.astype(dtype), dtype, nb=B)
    assert C.dtype == dtype and np.array_equal(C, np.tril(M).astype(dtype))
    print(fam, n, B, np.dtype(dtype).name, "sygst peak", peak)
    assert peak < LIMIT, peak


@pytest.mark.parametrize("fam,n,B", factor.SYGST_FP64_ONLY["argvalues"])
def test_sygst_on_wide_panel_tiles_is_exact_in_fp64_only(fam, n, B):
    """the inverse of a panel member's diagonal tile of 256 or 512 is large: the emulation with the tile as the block
    stays exact in fp64 (every partial sum 16 times below 2^53) and leaves the range of fp32, so the GPU test runs these
    in fp64 alone"""
    A, L, M = dm.sygst_case(n, n, **fam_kw(fam))
    C, peak = dm.sygst_blocked(A, L, np.float64, nb=B)
    assert np.array_equal(C, np.tril(M))
    tile = dm.inv_tile(L[:B, :B].copy(), dm.Peak())
    print(fam, n, B, "sygst peak", peak, "max |inv(tile)|", np.abs(tile).max())
    assert LIMIT <= peak < 2.0 ** 53 / 16, peak


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SYGST_ORDERS)
def test_sygst_emulation_is_exact(n, dtype):
    A, L, M = dm.sygst_case(n, n)
    assert np.abs(A).max() * 16 < 2.0 ** 24
    C, peak = dm.sygst_blocked(A.astype(dtype), L.astype(dtype), dtype)
    assert C.dtype == dtype and np.array_equal(C, np.tril(M).astype(dtype))
    assert peak < LIMIT, peak


@pytest.mark.parametrize("n", [1000, 1024, 1536])
def test_inverses_and_right_hand_sides_are_exact_in_fp32(n):
    A, L, _ = dm.cholesky_case(n, n)
    Ai = dm.inv_spd(n, n)
    X = dm.solution(n, 300, n)
    for M in (A, dm.inv_factor(n, n), Ai, A @ X):
        assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    assert np.abs(Ai).max() * 16 < 2.0 ** 24
    # the partial sums of A X and of the two triangular sweeps that undo it
    assert (np.abs(A) @ np.abs(X)).max() * 16 < 2.0 ** 24
    assert (np.abs(L) @ np.abs(L.T @ X)).max() * 16 < 2.0 ** 24
    assert (np.abs(dm.inv_factor(n, n)) @ np.abs(A @ X)).max() * 16 < 2.0 ** 24


@pytest.mark.parametrize("fam,n", NEW_SOLVES)
def test_right_hand_sides_are_exact_in_fp32_on_the_new_families(fam, n):
    """potrs / posv / dsposv (every family): A X and the two triangular sweeps that undo it, at the widest nrhs"""
    A, L, _ = dm.cholesky_case(n, n, **fam_kw(fam))
    X = dm.solution(n, 300, n)
    for M in (A, L, A @ X):
        assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    ax, sweep = (np.abs(A) @ np.abs(X)).max(), (np.abs(L) @ np.abs(L.T @ X)).max()
    print(fam, n, "|A||X|", ax, "|L||L^T X|", sweep, "|L^T||X|", (np.abs(L.T) @ np.abs(X)).max())
    assert ax < LIMIT and sweep < LIMIT and (np.abs(L.T) @ np.abs(X)).max() < LIMIT
    # the sweeps go through the inverses of the diagonal 128-blocks: |inv(Lkk)| |Lkk Y| bounds that product
    Y = L.T @ X
    for k in range(0, n, 128):
        d = slice(k, k + 128)
        W = np.linalg.inv(L[d, d])
        assert np.array_equal(W @ L[d, d], np.eye(W.shape[0])) and np.array_equal(W * 2, np.round(W * 2))
        assert (np.abs(W) @ np.abs(L[d, d] @ Y[d])).max() < LIMIT and (np.abs(W.T) @ np.abs(L[d, d].T @ X[d])).max() < LIMIT


@pytest.mark.parametrize("fam,n", NEW_INVERSES)
def test_inverses_are_exact_in_fp32_on_the_new_families(fam, n):
    """trtri, potri / poinv, porfs / posvx (mirror and mod3): the closed forms fit fp32, and so do the partial sums of
    W21 = -W22 L21 W11, of inv(L)^T inv(L), and of a sweep with inv(L) over A X (the solve through the inverse, which
    bounds every sweep of the refinement on an exact solution: its residual is zero)"""
    assert fam != "panel"
    A, L, _ = dm.cholesky_case(n, n, family=fam)
    Li, Ai = dm.inv_factor(n, n, family=fam), dm.inv_spd(n, n, family=fam)
    X = dm.solution(n, 300, n)
    for M in (Li, Ai):
        assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    assert np.array_equal(Li @ L, np.eye(n)) and np.array_equal(Ai @ A, np.eye(n))
    a, b, c = (np.abs(Li) @ np.abs(A @ X)).max(), (np.abs(Li.T) @ np.abs(Li)).max(), (np.abs(Li) @ np.abs(L) @ np.abs(Li)).max()
    print(fam, n, "max|inv(L)|", np.abs(Li).max(), "|inv(L)||AX|", a, "|inv(L)^T||inv(L)|", b, "|W||L||W|", c)
    assert np.abs(Ai).max() < LIMIT and a < LIMIT and b < LIMIT and c < LIMIT
    # porfs chooses X without zeros
    X5 = dm.solution(n, 5, n)
    X5 = np.where(X5 == 0, 1.0, X5)
    assert (np.abs(A @ X5) + np.abs(A) @ np.abs(X5)).min() >= 1


@pytest.mark.parametrize("fam,n", NEW_ONE_TILE)
def test_single_tile_trsm_is_exact_in_fp32_on_the_new_families(fam, n):
    """X L^T and the solve that returns X, in 128-blocks through the inverses of the diagonal blocks"""
    _, L, _ = dm.cholesky_case(n, n, **fam_kw(fam))
    X = dm.solution(n, n, n)
    P = X @ L.T
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    assert 2 * (np.abs(X) @ np.abs(L.T)).max() < LIMIT  # (|alpha| <= 2)
    for k in range(0, n, 128):
        d = slice(k, k + 128)
        W = np.linalg.inv(L[d, d])
        assert np.array_equal(W @ L[d, d], np.eye(W.shape[0]))
        assert 2 * (np.abs(X[:, d] @ L[d, d].T) @ np.abs(W.T)).max() < LIMIT


def backward_sweep_bound(L, X, B, dtype):
    """the backward sweep of potrs as the library runs it: Z(k) <- Z(k) inv(L(k,k)) with the transposed inverse of the
    WHOLE diagonal tile, itself from a TRSM of the identity.  -> (the largest partial sum of inv(Lkk)^T (Lkk^T Xk) and
    of the inversion of a tile, whether the tile inverses come out exactly in dtype)"""
    n = L.shape[0]
    worst, exact, peak = 0.0, True, dm.Peak()
    for k in range(0, n, B):
        d = slice(k, min(k + B, n))
        W = dm.inv_tile(np.array(L[d, d]), dm.Peak())  # fp64
        assert np.array_equal(W @ L[d, d], np.eye(W.shape[0]))
        exact = exact and np.array_equal(dm.inv_tile(L[d, d].astype(dtype), peak), W.astype(dtype))
        worst = max(worst, float((np.abs(W.T) @ np.abs(L[d, d].T @ X[d])).max()))
    return max(worst, peak.value), exact


@pytest.mark.parametrize("fam,n,B", SOLVE_TILES)
def test_backward_sweep_through_the_tile_inverse_is_exact_in_fp32(fam, n, B):
    """potrs / posv / dsposv at every (family, order, tile size) that runs in fp32, every nrhs of the GPU test"""
    _, L, _ = dm.cholesky_case(n, n, **fam_kw(fam))
    for nrhs in (1, 5, 300):
        bound, exact = backward_sweep_bound(L, dm.solution(n, nrhs, n), B, np.float32)
        print(fam, n, B, nrhs, "backward sweep bound", bound)
        assert exact and bound < LIMIT, bound


@pytest.mark.parametrize("fam,n,B", LDL_TILES)
def test_sytrs_backward_sweep_through_the_tile_inverse_is_exact_in_fp32(fam, n, B):
    _, L, _ = dm.ldl_case(n, n, **fam_kw(fam))
    bound, exact = backward_sweep_bound(L, dm.solution(n, 5, n), B, np.float32)
    print(fam, n, B, "backward sweep bound", bound)
    assert exact and bound < LIMIT, bound


@pytest.mark.parametrize("fam,n,B", factor.SOLVES_FP64_ONLY["argvalues"])
def test_solves_on_wide_panel_tiles_are_exact_in_fp64_only(fam, n, B):
    """a panel member's diagonal tile of 512 has an inverse of magnitude 2e6: the backward sweep of potrs and of sytrs
    leaves the range of fp32 and stays far inside that of fp64, so the GPU tests solve there in fp64 alone (and dsposv,
    whose solves are fp32, not at all); the right-hand sides and the forward sweep fit as everywhere"""
    assert factor.LDL_FP64_ONLY["argvalues"] == factor.SOLVES_FP64_ONLY["argvalues"]
    for L in (dm.cholesky_case(n, n, **fam_kw(fam))[1], dm.ldl_case(n, n, **fam_kw(fam))[1]):
        for nrhs in (1, 5, 300):
            bound, exact = backward_sweep_bound(L, dm.solution(n, nrhs, n), B, np.float64)
            print(fam, n, B, nrhs, "backward sweep bound", bound)
            assert exact and LIMIT <= bound < 2.0 ** 53 / 16, bound
