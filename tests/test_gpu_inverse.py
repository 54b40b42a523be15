"""The inverse from the Cholesky factor: CHAMELEON_dtrtri_Tile (LAPACK DTRTRI), CHAMELEON_dpotri_Tile (DPOTRI) and
CHAMELEON_dpoinv_Tile (potrf + potri) -- checked against LAPACK's error bounds in long double, against numpy's inverse,
and for the triangle they must leave alone."""
import functools

import numpy as np
import pytest

from chol_testkit import bits, desc, other, spd_spectral, stored_lower, uplo_code

pytestmark = pytest.mark.gpu

EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24


@functools.lru_cache(maxsize=4)
def plgsy_problem(N):
    """(A, L): the plgsy matrix of order N and its Cholesky factor (numpy)"""
    from oracle import oracle as orc

    A = orc.plgsy_matrix(N, float(N), 42)
    return A, np.asfortranarray(np.linalg.cholesky(A))


def run(ch, fn, M, B, u, dt="d", extra=()):
    """-> (info, the stored matrix after fn(uplo, *extra, A))"""
    d = desc(ch, M.shape[0], B, dt)
    d.from_lapack(M)
    info = fn(uplo_code(ch, u), *extra, d)
    return info, d.to_lapack()


def trtri(ch, M, B, u, dt="d"):
    return run(ch, ch.CHAMELEON_dtrtri_Tile, M, B, u, dt, (ch.ChamNonUnit,))


def potri(ch, M, B, u):
    return run(ch, ch.CHAMELEON_dpotri_Tile, M, B, u)


def lower_of_rowmajor(X, u):
    """chol_testkit.lower_of in C order for Upper too (tril of the transposed view, not the transposed triu): the
    residual checks below multiply by it, and a BLAS may sum another layout in another order"""
    return np.tril(X) if u == "L" else np.tril(X.T)


def check_trtri_bound(L, X, eps, c=4.0, max_rows=128):
    """|L X - I| <= c n eps |L| |X| componentwise: in long double up to n = 2048 (on a sample of rows above 1024),
    in double above (all rows; c + 2 for the rounding of the check itself)"""
    n = L.shape[0]
    if n > 2048:
        R = np.abs(L @ X - np.eye(n))
        worst = float(np.max(R - (c + 2.0) * n * eps * (np.abs(L) @ np.abs(X))))
        assert worst <= 0.0, worst
        return
    rows = np.arange(n) if n <= 1024 else np.unique(np.r_[np.random.default_rng(1).choice(n, max_rows, replace=False), n - 1])
    Lr, Xl = L[rows].astype(np.longdouble), X.astype(np.longdouble)
    R = np.abs(Lr @ Xl - np.eye(n, dtype=np.longdouble)[rows])
    bound = c * n * eps * (np.abs(Lr) @ np.abs(Xl))
    worst = float(np.max(R - bound))
    assert worst <= 0.0, worst


TRTRI = [(512, 128, "L"), (512, 128, "U"), (1000, 192, "L"), (2048, 256, "L"), (2048, 256, "U"), (4096, 1024, "L"),
         (4096, 1024, "U"), (192, 192, "L")]


@pytest.mark.parametrize("N,B,u", TRTRI)
def test_trtri_fp64(cham, N, B, u):
    ch = cham
    A, L = plgsy_problem(N)
    M = stored_lower(L, u, A)
    info, Xs = trtri(ch, M, B, u)
    assert info == 0
    assert np.array_equal(bits(Xs[other(N, u)]), bits(M[other(N, u)]))
    check_trtri_bound(L, lower_of_rowmajor(Xs, u), EPS64)


@pytest.mark.parametrize("u", ["L", "U"])
def test_trtri_fp32(cham, u):
    ch = cham
    N, B = 2048, 256
    _, L = plgsy_problem(N)
    L32 = np.asfortranarray(L.astype(np.float32))
    M = stored_lower(L32, u, np.float32(0.5))
    info, Xs = trtri(ch, M, B, u, "s")
    assert info == 0 and Xs.dtype == np.float32
    assert np.array_equal(bits(Xs[other(N, u)]), bits(M[other(N, u)]))
    check_trtri_bound(L32.astype(np.float64), lower_of_rowmajor(Xs, u).astype(np.float64), EPS32)


@pytest.mark.parametrize("N,B,u", [(1000, 192, "L"), (1024, 256, "U")])
def test_other_triangle_nan(cham, N, B, u):
    """NaN in the other strict triangle (the other halves of the diagonal tiles included): same inverse, NaN kept"""
    ch = cham
    A, L = plgsy_problem(N)
    info, X0 = trtri(ch, stored_lower(L, u, A), B, u)
    M = stored_lower(L, u, np.nan)
    info2, X1 = trtri(ch, M, B, u)
    assert info == info2 == 0
    assert np.array_equal(bits(lower_of_rowmajor(X1, u)), bits(lower_of_rowmajor(X0, u)))
    assert np.array_equal(bits(X1[other(N, u)]), bits(M[other(N, u)]))
    # potri on the same storage
    info3, P = potri(ch, M, B, u)
    assert info3 == 0 and np.array_equal(bits(P[other(N, u)]), bits(M[other(N, u)]))
    assert not np.isnan(lower_of_rowmajor(P, u)).any()


def check_potri(A, P, u, kappa, c=10.0):
    n = A.shape[0]
    Xl = lower_of_rowmajor(P, u)
    X = Xl + np.tril(Xl, -1).T
    r = np.linalg.norm(A @ X - np.eye(n)) / (np.linalg.norm(A) * np.linalg.norm(X))
    assert r <= c * n * EPS64, r
    Xref = np.linalg.inv(A)
    err = np.abs(X - Xref).max() / np.abs(Xref).max()
    assert err <= max(1e-13, 10.0 * n * kappa * EPS64), (err, kappa)


@pytest.mark.parametrize("N,B,u", [(1000, 192, "L"), (1024, 256, "U"), (1024, 256, "L")])
def test_potri_plgsy(cham, N, B, u):
    ch = cham
    A, L = plgsy_problem(N)
    M = stored_lower(L, u, A)
    info, P = potri(ch, M, B, u)
    assert info == 0
    assert np.array_equal(bits(P[other(N, u)]), bits(M[other(N, u)]))
    check_potri(A, P, u, np.linalg.cond(A))


@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10])
@pytest.mark.parametrize("u", ["L", "U"])
def test_potri_conditioning(cham, kappa, u):
    """the factor from the library's own potrf, then potri"""
    ch = cham
    N, B = 1024, 256
    A = spd_spectral(N, kappa, 5)
    d = desc(ch, N, B)
    d.from_lapack(A)
    assert ch.CHAMELEON_dpotrf_Tile(uplo_code(ch, u), d) == 0
    assert ch.CHAMELEON_dpotri_Tile(uplo_code(ch, u), d) == 0
    P = d.to_lapack()
    assert np.array_equal(bits(P[other(N, u)]), bits(A[other(N, u)]))
    check_potri(A, P, u, kappa)


def sym_matvec_ld(Xl, V, blk=1024):
    """(tril(Xl) + tril(Xl, -1)^T) V in long double, by row blocks"""
    n = Xl.shape[0]
    V = V.astype(np.longdouble)
    Y = np.zeros(V.shape, dtype=np.longdouble)
    for i0 in range(0, n, blk):
        i1 = min(n, i0 + blk)
        R = Xl[i0:i1, :i1].astype(np.longdouble)
        R[:, i0:i1] = np.tril(R[:, i0:i1])
        Y[i0:i1] += R @ V[:i1]
        R[:, i0:i1] = np.tril(R[:, i0:i1], -1)
        Y[:i1] += R.T @ V[i0:i1]
    return Y


def test_poinv_large_probed(cham):
    """N = 16384 / 512: |A (X v) - v| / (|A| |X| |v|) for random v, in long double -- O(N^2) on the host"""
    ch = cham
    from oracle import oracle as orc

    N, B = 16384, 512
    A = orc.plgsy_matrix(N, float(N), 42)
    d = desc(ch, N, B)
    d.from_lapack(A)
    assert ch.CHAMELEON_dpoinv_Tile(ch.ChamLower, d) == 0
    Xl = np.tril(d.to_lapack())
    del d
    V = np.random.default_rng(3).standard_normal((N, 2))
    XV = sym_matvec_ld(Xl, V)
    AXV = sym_matvec_ld(np.tril(A), XV)
    nX = np.sqrt(2.0 * np.sum(Xl * Xl) - np.sum(np.diag(Xl) ** 2))
    for j in range(V.shape[1]):
        r = float(np.linalg.norm((AXV[:, j] - V[:, j]).astype(np.float64)))
        rel = r / (np.linalg.norm(A) * nX * np.linalg.norm(V[:, j]))
        assert rel <= 10.0 * N * EPS64, rel


@pytest.mark.parametrize("N,B,u", [(1000, 192, "L"), (1024, 256, "U")])
def test_poinv_is_potrf_then_potri(cham, N, B, u):
    ch = cham
    A = spd_spectral(N, 1e4, 9)
    d1, d2 = desc(ch, N, B), desc(ch, N, B)
    d1.from_lapack(A)
    d2.from_lapack(A)
    assert ch.CHAMELEON_dpoinv_Tile(uplo_code(ch, u), d1) == 0
    assert ch.CHAMELEON_dpotrf_Tile(uplo_code(ch, u), d2) == 0
    assert ch.CHAMELEON_dpotri_Tile(uplo_code(ch, u), d2) == 0
    assert np.array_equal(bits(d1.to_lapack()), bits(d2.to_lapack()))


def test_poinv_not_spd(cham):
    ch = cham
    N, B = 1000, 192
    A, _ = plgsy_problem(N)
    M = A.copy(order="F")
    M[N // 2, N // 2] = -1.0
    d1, d2 = desc(ch, N, B), desc(ch, N, B)
    d1.from_lapack(M)
    d2.from_lapack(M)
    assert ch.CHAMELEON_dpoinv_Tile(ch.ChamLower, d1) == N // 2 + 1
    assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d2) == N // 2 + 1
    assert np.array_equal(bits(d1.to_lapack()), bits(d2.to_lapack()))


@pytest.mark.parametrize("which", ["trtri", "potri"])
@pytest.mark.parametrize("N,B,u,j", [(1000, 192, "L", 700), (1024, 256, "U", 5), (1024, 256, "L", 1023)])
def test_zero_on_the_diagonal(cham, which, N, B, u, j):
    ch = cham
    A, L = plgsy_problem(N)
    L0 = L.copy(order="F")
    L0[j, j] = 0.0
    M = stored_lower(L0, u, A)
    info, after = (trtri if which == "trtri" else potri)(ch, M, B, u)
    assert info == j + 1
    assert np.array_equal(bits(after), bits(M))


def test_argument_errors(cham):
    ch = cham
    N, B = 512, 128
    A, L = plgsy_problem(N)
    d = desc(ch, N, B)
    d.from_lapack(L)
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dtrtri_Tile(ch.ChamLower, ch.ChamUnit, d)
    assert e.value.code == -104  # CHOL_ERR_NOT_SUPPORTED
    for call in (lambda x: ch.CHAMELEON_dtrtri_Tile(7, ch.ChamNonUnit, x), lambda x: ch.CHAMELEON_dpotri_Tile(7, x),
                 lambda x: ch.CHAMELEON_dpoinv_Tile(7, x)):
        with pytest.raises(ch.CholmiError) as e:
            call(d)
        assert e.value.code == -1
    rect = desc(ch, N, B, cols=N + B)
    with pytest.raises(ch.CholmiError) as e:
        ch.CHAMELEON_dtrtri_Tile(ch.ChamLower, ch.ChamNonUnit, rect)
    assert e.value.code == -3
    for fn in (ch.CHAMELEON_dpotri_Tile, ch.CHAMELEON_dpoinv_Tile):
        with pytest.raises(ch.CholmiError) as e:
            fn(ch.ChamLower, rect)
        assert e.value.code == -2
    odd = desc(ch, 100, 100)  # one 100 x 100 tile: a stored edge that is not a multiple of 64
    odd.from_lapack(np.eye(100))
    for call in (lambda: ch.CHAMELEON_dtrtri_Tile(ch.ChamLower, ch.ChamNonUnit, odd),
                 lambda: ch.CHAMELEON_dpotri_Tile(ch.ChamLower, odd), lambda: ch.CHAMELEON_dpoinv_Tile(ch.ChamLower, odd)):
        with pytest.raises(ch.CholmiError) as e:
            call()
        assert e.value.code == -104
    assert np.array_equal(bits(d.to_lapack()), bits(L))  # nothing was touched by the refused calls
    assert np.array_equal(bits(odd.to_lapack()), bits(np.eye(100)))


def test_deterministic(cham):
    ch = cham
    N, B = 2048, 256
    A, L = plgsy_problem(N)
    M = stored_lower(L, "L", A)
    _, X1 = trtri(ch, M, B, "L")
    _, X2 = trtri(ch, M, B, "L")
    assert np.array_equal(bits(X1), bits(X2))
    _, P1 = potri(ch, M, B, "L")
    _, P2 = potri(ch, M, B, "L")
    assert np.array_equal(bits(P1), bits(P2))
