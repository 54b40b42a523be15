"""The mixed-precision SPD solve CHAMELEON_dsposv_Tile (LAPACK DSPOSV): an fp32 factor of A, fp64 iterative refinement
of X from residuals read off one stored triangle of A, and the fp64 dposv fallback -- checked against numpy on plgsy
and spectrally constructed matrices."""
import ctypes as C
import functools

import numpy as np
import pytest

from chol_testkit import bits, desc, other, spd_spectral, uplo_code

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SHAPES = [(1024, 256, 1), (1000, 192, 7), (2048, 128, 128), (1536, 512, 1024), (16384, 512, 16)]
CASES = [(N, B, r, u) for N, B, r in SHAPES for u in "LU" if u == "L" or N % B == 0]  # Upper as the potrs test


@functools.lru_cache(maxsize=2)
def plgsy_problem(N, nrhs):
    from oracle import oracle as orc

    A = orc.plgsy_matrix(N, float(N), 42)
    Bm = np.asfortranarray(np.random.default_rng(11).standard_normal((N, nrhs)))
    return A, Bm, np.linalg.solve(A, Bm)


def solve(ch, A, Bm, B, uplo):
    """-> (info, iter, X, A after, B after)"""
    N, nrhs = Bm.shape
    dA, dB, dX = desc(ch, N, B), desc(ch, N, B, cols=nrhs), desc(ch, N, B, cols=nrhs)
    dA.from_lapack(A)
    dB.from_lapack(Bm)
    info, it = ch.CHAMELEON_dsposv_Tile(uplo, dA, dB, dX)
    return info, it, dX.to_lapack(), dA.to_lapack(), dB.to_lapack()


def residual_ld(A, Bm, X):
    """B - A X in np.longdouble, by row blocks"""
    Xl = X.astype(np.longdouble)
    R = np.empty(Bm.shape, dtype=np.longdouble)
    for i in range(0, A.shape[0], 1024):
        R[i:i + 1024] = Bm[i:i + 1024].astype(np.longdouble) - A[i:i + 1024].astype(np.longdouble) @ Xl
    return R


def stopping_test_holds(A, Bm, X):
    """LAPACK dsposv's test, every column: max|R(:,j)| <= max|X(:,j)| ||A||_inf eps sqrt(n)"""
    cte = np.abs(A).sum(axis=1).max() * EPS * np.sqrt(A.shape[0])
    R = residual_ld(A, Bm, X)
    return bool(np.all(np.abs(R).max(axis=0) <= np.abs(X).max(axis=0) * cte)), R


@pytest.mark.parametrize("N,B,nrhs,u", CASES)
def test_dsposv_against_numpy(cham, N, B, nrhs, u):
    ch = cham
    A, Bm, Xref = plgsy_problem(N, nrhs)
    info, it, X, Aafter, Bafter = solve(ch, A, Bm, B, uplo_code(ch, u))
    assert info == 0 and 0 <= it <= 30, (info, it)
    ok, _ = stopping_test_holds(A, Bm, X)
    assert ok
    assert np.abs(X - Xref).max() / np.abs(Xref).max() <= 1e-12
    assert np.array_equal(bits(Aafter), bits(A)) and np.array_equal(bits(Bafter), bits(Bm))
    st = ch.last_dsposv_stats()
    assert st["residuals"] == it + 1 and st["solves"] == it + 1
    # deterministic: a second call gives the same X and iter, bit for bit
    info2, it2, X2, _, _ = solve(ch, A, Bm, B, uplo_code(ch, u))
    assert (info2, it2) == (info, it) and np.array_equal(bits(X2), bits(X))


@pytest.mark.parametrize("N,B,nrhs,u", [(1000, 192, 7, "L"), (1024, 256, 1, "U"), (1024, 256, 5, "L")])
def test_only_the_uplo_triangle_is_read(cham, N, B, nrhs, u):
    """The other triangle -- the other halves of the diagonal tiles included -- full of NaN: same X and iter."""
    ch = cham
    A, Bm, _ = plgsy_problem(N, nrhs)
    info, it, X, _, _ = solve(ch, A, Bm, B, uplo_code(ch, u))
    M = A.copy(order="F")
    M[other(N, u)] = np.nan
    info2, it2, X2, Mafter, _ = solve(ch, M, Bm, B, uplo_code(ch, u))
    assert info == info2 == 0 and it2 == it >= 0
    assert np.array_equal(bits(X2), bits(X))
    assert np.array_equal(bits(Mafter), bits(M))


def test_harder_conditioning_still_converges(cham):
    ch = cham
    N, B, nrhs = 1024, 256, 4
    A = spd_spectral(N, 1e5, 3)
    Bm = np.asfortranarray(np.random.default_rng(5).standard_normal((N, nrhs)))
    info, it, X, Aafter, _ = solve(ch, A, Bm, B, ch.ChamLower)
    Ap, Bp, _ = plgsy_problem(N, nrhs)
    _, it_plgsy, _, _, _ = solve(ch, Ap, Bp, B, ch.ChamLower)
    assert info == 0 and 0 <= it_plgsy <= it <= 30, (it, it_plgsy)
    assert np.array_equal(bits(Aafter), bits(A))
    ok, R = stopping_test_holds(A, Bm, X)
    assert ok
    berr = float(np.abs(R).max() / (np.abs(A).sum(axis=1).max() * np.abs(X).max()))
    assert berr <= 1e-14, berr


def fallback_matches_dposv(ch, A, Bm, B, uplo, want_iter):
    """dsposv falls back (iter in want_iter) and leaves X and A bit-identical to lacpy(B -> X) + posv(A, X) on copies."""
    N, nrhs = Bm.shape
    dA, dB, dX = desc(ch, N, B), desc(ch, N, B, cols=nrhs), desc(ch, N, B, cols=nrhs)
    dA.from_lapack(A)
    dB.from_lapack(Bm)
    info, it = ch.CHAMELEON_dsposv_Tile(uplo, dA, dB, dX)
    assert it in want_iter, it
    assert np.array_equal(bits(dB.to_lapack()), bits(Bm))
    cA, cB, cX = desc(ch, N, B), desc(ch, N, B, cols=nrhs), desc(ch, N, B, cols=nrhs)
    cA.from_lapack(A)
    cB.from_lapack(Bm)
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, cB, cX)
    info_ref = ch.CHAMELEON_dposv_Tile(uplo, cA, cX)
    assert info == info_ref
    assert np.array_equal(bits(dA.to_lapack()), bits(cA.to_lapack()))
    if info == 0:
        assert np.array_equal(bits(dX.to_lapack()), bits(cX.to_lapack()))
    return info, it


@pytest.mark.parametrize("u", ["L", "U"])
def test_fallback_ill_conditioned(cham, u):
    ch = cham
    N, B = 1024, 256
    A = spd_spectral(N, 1e10, 7)
    Bm = np.asfortranarray(np.random.default_rng(9).standard_normal((N, 3)))
    info, _ = fallback_matches_dposv(ch, A, Bm, B, uplo_code(ch, u), (-3, -31))
    assert info == 0


@pytest.mark.parametrize("what", ["A", "B"])
def test_fallback_fp32_overflow(cham, what):
    ch = cham
    N, B, nrhs = 1024, 256, 3
    A, Bm, _ = plgsy_problem(N, nrhs)
    if what == "A":
        A = np.asfortranarray(A * 2.0 ** 200)
    else:
        Bm = Bm.copy(order="F")
        Bm[N // 3, 1] = 1e300
    info, _ = fallback_matches_dposv(ch, A, Bm, B, ch.ChamLower, (-2,))
    assert info == 0


def test_not_spd(cham):
    ch = cham
    N, B, nrhs = 1000, 192, 3
    A, Bm, _ = plgsy_problem(N, nrhs)
    M = A.copy(order="F")
    M[N // 2, N // 2] = -1.0
    info, it = fallback_matches_dposv(ch, M, Bm, B, ch.ChamLower, (-3,))
    assert info == N // 2 + 1


def test_argument_errors(cham):
    ch = cham
    N, B = 512, 128
    A, Bm, _ = plgsy_problem(N, 2)
    dA, dB, dX = desc(ch, N, B), desc(ch, N, B, cols=2), desc(ch, N, B, cols=2)
    dA.from_lapack(A)
    dB.from_lapack(Bm)
    fA = desc(ch, N, B, "s")
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dsposv_Tile(ch.ChamLower, fA, dB, dX)  # fp32 A
    assert e.value.code == -2
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dsposv_Tile(ch.ChamLower, dA, dB, dB)  # X aliases B
    assert e.value.code == -4
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dsposv_Tile(ch.ChamLower, dA, desc(ch, N, 256, cols=2), dX)  # tile size differs
    assert e.value.code == -3
    assert ch.lib().chol_dsposv_tile(ch.ChamLower, dA.handle, dB.handle, dX.handle, None) == -5  # iter NULL
    it = C.c_int()
    assert ch.lib().chol_dsposv_tile(7, dA.handle, dB.handle, dX.handle, C.byref(it)) == -1
    # nothing was touched by the refused calls
    assert np.array_equal(bits(dA.to_lapack()), bits(A)) and np.array_equal(bits(dB.to_lapack()), bits(Bm))
