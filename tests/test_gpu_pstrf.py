"""The pivoted Cholesky factorisation CHAMELEON_dpstrf_Tile / CHAMELEON_spstrf_Tile (LAPACK DPSTRF / SPSTRF) against
scipy's dpstrf / spstrf: pivots, rank, info, the residual of P^T A P = L L^T and the factor itself, full rank and rank
deficient, Lower and Upper, fp64 and fp32, ragged orders and tiles that are not multiples of 128 -- with the other
triangle NaN-filled and returned bit for bit, and repeated calls bit-identical.

The random Gram matrices never tie, never sit on the stopping value and hide a wrong entry in a norm, so the exact tests
at the end run pstrf_model.level_case, on which the elimination order is forced up to ties, the ties are many, and
pivots, rank, info and the factor are known in closed form and compared bit for bit with LAPACK's
(tests/test_pstrf_host.py proves the family without a GPU)."""
import functools
import time

import numpy as np
import pytest
import scipy.linalg.lapack as lapack

import pstrf_model as pm
from chol_testkit import UserView, bits, desc, npdt, other_triangle_kept, pxq_refused, stored_lower, uplo_code
from pstrf_model import gram

pytestmark = pytest.mark.gpu

EPS = {"d": 2.0 ** -53, "s": 2.0 ** -24}
# The residual ||(P^T A P - L L^T)(:, 1:rank)||_F / ||A||_F of the random families is held to RES_MARGIN x LAPACK's own
# on the same input, pivots and all.  LAPACK reaches 0.1 eps (rank 1) to 3.6 eps (N = 8192) there, nearly flat in N, so
# the former 30 N eps left four orders of magnitude; the library's ratio to LAPACK's is printed per case.
RES_MARGIN = 4


@functools.lru_cache(maxsize=None)
def full_rank(n, seed):
    """a well-conditioned SPD Gram matrix (n x 2n factor) and its 2-norm condition number"""
    A = gram(n, 2 * n, seed)
    ev = np.linalg.eigvalsh(A)
    return A, float(ev[-1] / ev[0])


def pstrf(ch, A, B, u="L", dt="d", tol=-1.0):
    """-> (info, piv, rank, L as Lower, the stored matrix after the call, what was stored)"""
    S = stored_lower(A.astype(npdt(dt)), u)
    d = desc(ch, A.shape[0], B, dt)
    d.from_lapack(S)
    info, piv, rank = ch.CHAMELEON_dpstrf_Tile(uplo_code(ch, u), d, tol)
    F = d.to_lapack()
    ch.CHAMELEON_Desc_Destroy(d)
    L = np.tril(F) if u == "L" else np.triu(F).T
    return info, piv, rank, L, F, S


def scipy_pstrf(A, dt="d", tol=-1.0):
    fn = lapack.dpstrf if dt == "d" else lapack.spstrf
    c, piv, rank, info = fn(np.asfortranarray(A.astype(npdt(dt))), tol=tol, lower=1)
    return np.tril(c), piv, rank, info


def residual(A, piv, L, rank):
    """||(P^T A P - L L^T)(:, 1:rank)||_F / ||A||_F on the first rank columns"""
    A = A.astype(np.float64)
    P = A[np.ix_(piv - 1, piv - 1)]
    Lr = L.astype(np.float64)[:, :rank]
    return np.linalg.norm(P[:, :rank] - Lr @ Lr[:rank].T) / np.linalg.norm(A)


def residual_like_lapack(what, A, piv, L, rank, ref, dt="d"):
    """the library's residual against LAPACK's own on the same input, printed (pytest -s shows it) -> the two.  ref =
    scipy_pstrf's result"""
    A = A.astype(npdt(dt))
    res, ref_res = residual(A, piv, L, rank), residual(A, ref[1], ref[0], ref[2])
    print(f"pstrf residual {what}: library {res / EPS[dt]:.3f} eps, scipy {ref_res / EPS[dt]:.3f} eps, "
          f"ratio {res / ref_res:.3f}")
    return res, ref_res


# ------------------------------------------------------------------------------------------------------- full rank
@pytest.mark.parametrize("N,B", [(1024, 256), (1000, 192), (2048, 512), (4096, 1024)])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_full_rank(cham, N, B, u, dt):
    """the residual bound, here and in the other random-family tests: RES_MARGIN = 4 times LAPACK's own residual on
    the same input (1.3 to 2.5 eps on these matrices); the library measured 0.63 to 1.26 times LAPACK's"""
    ch = cham
    A, kappa = full_rank(N, N + B)
    info, piv, rank, L, F, S = pstrf(ch, A, B, u, dt)
    assert info == 0 and rank == N
    assert sorted(piv) == list(range(1, N + 1))
    Lref, ref_piv, ref_rank, ref_info = scipy_pstrf(A, dt)
    assert ref_info == 0 and ref_rank == N
    if dt == "d":
        assert np.array_equal(piv, ref_piv)
    res, ref_res = residual_like_lapack(f"full {N} {B} {u} {dt}", A, piv, L, rank, (Lref, ref_piv, ref_rank), dt)
    assert res <= RES_MARGIN * ref_res, (res, ref_res)
    if np.array_equal(piv, ref_piv):
        err = np.abs(L.astype(np.float64) - Lref).max() / np.abs(Lref).max()
        assert err <= 10 * kappa * np.sqrt(N) * EPS[dt], (err, kappa)
    assert other_triangle_kept(F, S, u)
    st = ch.last_pstrf_stats()
    assert st["steps"] == N and st["total_ms"] > 0 and st["steps_ms"] > 0


# ------------------------------------------------------------------------------------------------- rank deficient
@pytest.mark.parametrize("r", [1, 37, 256, 261, 512, 1023])
@pytest.mark.parametrize("u", ["L", "U"])
def test_rank_deficient(cham, r, u):
    ch = cham
    N, B = 1024, 256
    A = gram(N, r, r)
    info, piv, rank, L, F, S = pstrf(ch, A, B, u)
    Lref, ref_piv, ref_rank, ref_info = scipy_pstrf(A)
    assert rank == r == ref_rank and info == 1 == ref_info
    assert sorted(piv) == list(range(1, N + 1))
    assert np.array_equal(piv[:rank], ref_piv[:rank])
    res, ref_res = residual_like_lapack(f"rank {r} {u}", A, piv, L, rank, (Lref, ref_piv, ref_rank))
    assert res <= RES_MARGIN * ref_res, (res, ref_res)  # (the rows of L match piv)
    assert other_triangle_kept(F, S, u)
    assert ch.last_pstrf_stats()["steps"] == r


@pytest.mark.parametrize("r", [5, 300])
def test_rank_deficient_fp32(cham, r):
    ch = cham
    N, B = 1000, 192
    A = gram(N, r, 3 * r)
    info, piv, rank, L, F, S = pstrf(ch, A, B, "L", "s")
    Lref, ref_piv, ref_rank, _ = scipy_pstrf(A, "s")
    assert info == 1 and rank == ref_rank
    res, ref_res = residual_like_lapack(f"rank {r} fp32", A, piv, L, rank, (Lref, ref_piv, ref_rank), "s")
    assert res <= RES_MARGIN * ref_res, (res, ref_res)


@pytest.mark.parametrize("tol", [1e-2, 1e-6, 1e-10])
def test_explicit_tol(cham, tol):
    ch = cham
    N, B = 1024, 256
    s = np.logspace(0, -6, N)
    A = np.asfortranarray(gram(N, N, 9) * np.outer(s, s))
    info, piv, rank, L, _, _ = pstrf(ch, A, B, tol=tol)
    _, ref_piv, ref_rank, ref_info = scipy_pstrf(A, tol=tol)
    assert rank == ref_rank and info == ref_info
    assert np.array_equal(piv[:rank], ref_piv[:rank])


def test_pivots_from_the_last_tile_column(cham):
    """an increasing diagonal: every pivot comes from far below, the first from the last tile column"""
    ch = cham
    N, B = 1024, 256
    G = gram(N, 2 * N, 10)
    s = np.linspace(1.0, 4.0, N) / np.sqrt(np.diag(G))
    A = np.asfortranarray(G * np.outer(s, s))
    info, piv, rank, L, _, _ = pstrf(ch, A, B)
    Lref, ref_piv, ref_rank, _ = scipy_pstrf(A)
    assert info == 0 and piv[0] == N
    assert np.array_equal(piv, ref_piv)
    res, ref_res = residual_like_lapack("increasing diagonal", A, piv, L, rank, (Lref, ref_piv, ref_rank))
    assert res <= RES_MARGIN * ref_res, (res, ref_res)


@pytest.mark.parametrize("N,B", [(1000, 192), (700, 320)])
def test_padding_is_never_chosen(cham, N, B):
    """a ragged order in tiles that are not multiples of 128: the padded image's identity entries would outrank a
    diagonal scaled by 1e-3"""
    ch = cham
    A = np.asfortranarray(full_rank(N, 11)[0] * 1e-3 / (2 * N))
    assert np.diag(A).max() < 1
    info, piv, rank, L, _, _ = pstrf(ch, A, B)
    Lref, ref_piv, ref_rank, _ = scipy_pstrf(A)
    assert info == 0 and rank == N
    assert np.array_equal(piv, ref_piv)
    res, ref_res = residual_like_lapack(f"padding {N} {B}", A, piv, L, rank, (Lref, ref_piv, ref_rank))
    assert res <= RES_MARGIN * ref_res, (res, ref_res)


@pytest.mark.parametrize("u", ["L", "U"])
def test_deterministic(cham, u):
    ch = cham
    N, B = 2048, 256
    A = gram(N, 700, 12)
    a = pstrf(ch, A, B, u)
    b = pstrf(ch, A, B, u)
    assert np.array_equal(bits(a[4]), bits(b[4]))
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] == 700


# ------------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("u", ["L", "U"])
def test_early_exit(cham, u):
    ch = cham
    N, B = 512, 128
    for A in (np.zeros((N, N)), -np.eye(N) + 0.01 * np.ones((N, N))):
        info, piv, rank, _, F, S = pstrf(ch, A, B, u)
        assert info == 1 and rank == 0
        assert np.array_equal(piv, np.arange(1, N + 1))
        assert np.array_equal(bits(F), bits(S))  # A unchanged


def test_nan_stops(cham):
    ch = cham
    N, B = 512, 128
    A = full_rank(N, 13)[0].copy()
    A[300, 300] = np.nan
    # a NaN on the diagonal is the largest diagonal entry: rank 0 before anything is written
    for u in ("L", "U"):
        info, piv, rank, _, F, S = pstrf(ch, A, B, u)
        assert info == 1 and rank == 0
        assert np.array_equal(piv, np.arange(1, N + 1))
        assert np.array_equal(bits(F), bits(S))  # A unchanged
        assert ch.last_pstrf_stats()["steps"] == 0
    # a NaN that appears during the factorisation: an entry off the diagonal
    A = full_rank(N, 13)[0].copy()
    # enters a candidate when the first of its row and column is eliminated, and that candidate stops the next step
    _, ref_piv, _, _ = scipy_pstrf(A)
    A[400, 200] = A[200, 400] = np.nan
    info, piv, rank, _, _, _ = pstrf(ch, A, B)
    first = int(np.flatnonzero((ref_piv == 401) | (ref_piv == 201))[0])
    assert info == 1 and rank == first + 1 < N
    assert np.array_equal(piv[:rank], ref_piv[:rank])


@pytest.mark.parametrize("B", [1, 64, 128])
def test_order_one(cham, B):
    ch = cham
    info, piv, rank, L, _, _ = pstrf(ch, np.array([[4.0]]), B)
    assert (info, list(piv), rank, L[0, 0]) == (0, [1], 1, 2.0)
    info, piv, rank, _, _, _ = pstrf(ch, np.array([[0.0]]), B)
    assert (info, list(piv), rank) == (1, [1], 0)


def test_single_tile_not_a_multiple_of_64(cham):
    ch = cham
    N = 100
    A = gram(N, 60, 14)
    for u in ("L", "U"):
        info, piv, rank, L, F, S = pstrf(ch, A, N, u)
        Lref, ref_piv, ref_rank, _ = scipy_pstrf(A)
        assert info == 1 and rank == ref_rank == 60
        assert np.array_equal(piv[:rank], ref_piv[:rank])
        res, ref_res = residual_like_lapack(f"single tile {u}", A, piv, L, rank, (Lref, ref_piv, ref_rank))
        assert res <= RES_MARGIN * ref_res, (res, ref_res)
        assert other_triangle_kept(F, S, u)


def test_argument_errors(cham):
    from dense_linear_app_amd._lib import lib
    import ctypes as C

    ch = cham
    N, B = 256, 128
    d = desc(ch, N, B, "d")
    d.from_lapack(full_rank(N, 15)[0])
    piv = (C.c_int * N)()
    r = C.c_int()
    assert lib().chol_pstrf_tile(7, d.handle, piv, C.byref(r), -1.0) == -1
    assert lib().chol_pstrf_tile(ch.ChamLower, None, piv, C.byref(r), -1.0) == -2
    assert lib().chol_pstrf_tile(ch.ChamLower, d.handle, None, C.byref(r), -1.0) == -3
    assert lib().chol_pstrf_tile(ch.ChamLower, d.handle, piv, None, -1.0) == -4
    assert lib().chol_pstrf_tile(ch.ChamLower, d.handle, piv, C.byref(r), float("nan")) == -5
    assert lib().chol_last_pstrf_stats(None) == -1
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dpstrf_Tile(7, d)
    assert e.value.code == -1
    rect = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, 2 * N, 0, 0, N, 2 * N, 1, 1)
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, rect)
    assert e.value.code == -2


def test_pxq_descriptor_is_not_supported(cham):
    ch = cham
    pxq_refused(ch, 1, lambda d: ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, d))


def test_sub_matrix_view(cham):
    """a tile-aligned view of a device user buffer gives the factor of the whole-matrix descriptor; the user's tiles
    outside the view stay as they were"""
    ch = cham
    uv = UserView(ch)
    mb, m = uv.mb, uv.m
    A = gram(m, 500, 16)
    v = uv.view_desc()
    v.from_lapack(A)
    info, piv, rank = ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, v)
    Lv = np.tril(v.to_lapack())
    ch.CHAMELEON_Desc_Destroy(v)
    info2, piv2, rank2, L2, _, _ = pstrf(ch, A, mb)
    assert (info, rank) == (info2, rank2) == (1, 500)
    assert np.array_equal(piv, piv2)
    assert np.array_equal(bits(Lv[:, :rank]), bits(L2[:, :rank]))
    uv.outside_unchanged()


def test_large(cham):
    ch = cham
    N, B = 8192, 512
    A = gram(N, N + 512, 17)
    info, piv, rank, L, _, _ = pstrf(ch, A, B)
    Lref, ref_piv, ref_rank, _ = scipy_pstrf(A)
    assert info == 0 and rank == ref_rank == N
    assert np.array_equal(piv, ref_piv)
    res, ref_res = residual_like_lapack(f"large {N}", A, piv, L, rank, (Lref, ref_piv, ref_rank))
    assert res <= RES_MARGIN * ref_res, (res, ref_res)


# ----------------------------------------------------------------------------------------------- the exact family
def check_exact(ch, case, dt, u, A, out, want_piv, want_rank, want_info, E=None):
    """out = pstrf()'s result on A: pivots, rank and info as given, the first rank columns of the factor equal to the
    closed form (E, or expected_factor at the library's own pivots) bit for bit -- NaN where E has one --, the other
    triangle kept, piv a permutation, one pivot step per column taken"""
    _, L0, sigma = pm.case_of(case)
    info, piv, rank, L, F, S = out
    n = A.shape[0]
    assert (rank, info) == (want_rank, want_info)
    assert np.array_equal(piv[:rank], want_piv[:rank])
    assert sorted(piv) == list(range(1, n + 1))
    E = (pm.expected_factor(L0, sigma, piv, rank) if E is None else E).astype(npdt(dt))
    got = L[:, :rank]
    bad = np.argwhere((bits(got) != bits(E)) & ~(np.isnan(got) & np.isnan(E)))
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], E[tuple(bad[0])])
    assert other_triangle_kept(F, S, u)
    assert ch.last_pstrf_stats()["steps"] == rank


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("n,B,m,t,r,dt", pm.EXACT, ids=pm.EXACT_IDS)
def test_exact(cham, n, B, m, t, r, dt, u):
    """pivots, rank and info are LAPACK's in the same dtype and the factor is the closed form, bit for bit: the rows of
    a level tie exactly at every step (lanes, waves and chunks of the arg-max must all take the smallest index), the
    finished block is dense (all three segments of the interchange, the dg / w swap, the composed interchanges of the
    earlier tile columns), and one wrong entry is one wrong bit pattern.  Nothing is asserted beyond column rank"""
    ch = cham
    case = (n, B, m, t, r)
    A = pm.case_of(case)[0]
    ref_piv, ref_rank, ref_info, _ = pm.lapack_level(*case, dt)
    a = pstrf(ch, A, B, u, dt)
    check_exact(ch, case, dt, u, A, a, ref_piv, ref_rank, ref_info)
    b = pstrf(ch, A, B, u, dt)
    assert np.array_equal(bits(a[4]), bits(b[4])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt,tol,want", [("s", -1.0, (896, 1)), ("d", -1.0, (1024, 0)), ("d", 16.0, (640, 1)),
                                         ("d", 15.0, (768, 1)), ("s", 16.0, (640, 1)), ("s", 15.0, (768, 1))])
def test_exact_stop_rules(cham, dt, tol, want, u):
    """(1024, 256): the largest diagonal entry is 4^7, so the default stopping value in fp32, 1024 2^-24 2^14, is 1
    exactly -- the pivots of the last level: fp32 stops at rank 896 (a pivot equal to the stopping value stops) and
    fp64 finishes; tol = 16 equals the pivots of the sixth level (rank 640), tol = 15 lets them through (rank 768)"""
    ch = cham
    case = pm.STOP_CASE[:5]
    A = pm.case_of(case)[0]
    ref_piv, ref_rank, ref_info, _ = pm.lapack_level(*case, dt, tol)
    assert (ref_rank, ref_info) == want
    check_exact(ch, case, dt, u, A, pstrf(ch, A, case[1], u, dt, tol), ref_piv, *want)


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("i,k", pm.NAN_PLANTS)
def test_exact_nan_off_the_diagonal(cham, i, k, u):
    """a NaN at (i, k) of A0, level(i) > level(k), enters row i's candidate when column k is eliminated; a NaN
    candidate ranks first and stops: rank = (the place of k in the elimination order without the NaN) + 1, the pivots
    up to there are that run's, and the factor's columns are the closed form with the NaN at row i's place in the
    column of k.  (LAPACK's MAXLOC skips a NaN, so the reference is the library's documented rule evaluated on the
    LAPACK run of the matrix without the NaN.)"""
    ch = cham
    case = pm.RAGGED_CASE[:5]
    sigma = pm.case_of(case)[2]
    ref_piv = pm.lapack_level(*case, "d")[0]
    want_rank = int(np.flatnonzero(sigma[ref_piv - 1] == k)[0]) + 1
    A = pm.nan_planted(case, i, k)
    out = pstrf(ch, A, case[1], u)
    E = pm.nan_expected_factor(case, i, k, out[1], want_rank)
    assert np.isnan(E).sum() == 1 and np.isnan(E[:, want_rank - 1]).sum() == 1
    check_exact(ch, case, "d", u, A, out, ref_piv, want_rank, 1, E)


def test_exact_sub_matrix_view(cham):
    """an exact case through a tile-aligned view of a device user buffer: bit-identical to the whole-matrix descriptor,
    LAPACK's pivots, the closed form; the user's tiles outside the view stay as they were"""
    ch = cham
    uv = UserView(ch)
    case = pm.VIEW_CASE[:5]
    assert case[:2] == (uv.m, uv.mb)
    A, L0, sigma = pm.case_of(case)
    v = uv.view_desc()
    v.from_lapack(A)
    info, piv, rank = ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, v)
    Lv = np.tril(v.to_lapack())
    ch.CHAMELEON_Desc_Destroy(v)
    ref_piv, ref_rank, ref_info, _ = pm.lapack_level(*case, "d")
    assert (rank, info) == (ref_rank, ref_info) == (case[4], 1)
    assert np.array_equal(piv[:rank], ref_piv[:rank]) and sorted(piv) == list(range(1, uv.m + 1))
    assert np.array_equal(bits(Lv[:, :rank]), bits(pm.expected_factor(L0, sigma, piv, rank)))
    info2, piv2, rank2, L2, _, _ = pstrf(ch, A, uv.mb)
    assert (info2, rank2) == (info, rank) and np.array_equal(piv, piv2)
    assert np.array_equal(bits(Lv[:, :rank]), bits(L2[:, :rank]))
    uv.outside_unchanged()


def test_more_than_256_chunks(cham):
    """n = 16640 in fp32: 260 chunks of 64 rows, so the 256 threads that reduce the partial maxima go round their
    strided loop a second time.  Rank 5; the five tied rows of the first level sit at rows 100, 8000, 16383 (chunk
    255), 16384 (chunk 256: thread 0 on its second pass) and 16484 (chunk 257), and the smallest current position must
    win each time.  tests/test_pstrf_host.py: test_chunk_case derives the expected pivots and factor without the
    matrix; the times of the 1 GiB round trip are printed"""
    ch = cham
    L0, sigma, want = pm.chunk_factor()
    n, B = L0.shape[0], 512
    t0 = time.perf_counter()
    A = pm.chunk_matrix(L0, sigma)
    d = desc(ch, n, B, "s")
    t1 = time.perf_counter()
    d.from_lapack(A)
    del A
    t2 = time.perf_counter()
    info, piv, rank = ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, d)
    t3 = time.perf_counter()
    L = d.to_lapack()[:, :5]
    ch.CHAMELEON_Desc_Destroy(d)
    t4 = time.perf_counter()
    print(f"pstrf n = {n}: forming the matrix {t1 - t0:.2f} s, upload {t2 - t1:.2f} s, factorisation {t3 - t2:.2f} s, "
          f"download {t4 - t3:.2f} s")
    assert (rank, info) == (5, 1)
    assert np.array_equal(piv[:5], want) and np.array_equal(want, [101, 8001, 16384, 16385, 16485])
    assert sorted(piv) == list(range(1, n + 1))
    assert np.array_equal(bits(np.tril(L)), bits(pm.expected_factor(L0, sigma, piv, 5).astype(np.float32)))
    assert ch.last_pstrf_stats()["steps"] == 5
