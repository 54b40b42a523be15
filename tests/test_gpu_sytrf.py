"""The L D L^T factorisation without pivoting CHAMELEON_{d,s}sytrf_nopiv_Tile with its solves sytrs_nopiv / sysv_nopiv
against the numpy model of the algorithm (sytrf_model.py) and by reconstruction, on symmetric quasi-definite matrices
K = [[H, J^T], [J, -C]] as built and under a random symmetric permutation: Lower and Upper, fp64 and fp32, tiles from
64 to 1024, ragged orders, a single tile and a sub-matrix view; the inertia; an integer case whose factor is exact; the
stops at a zero or non-finite pivot; the other triangle and the padding returned bit for bit; repeated calls
bit-identical; the argument errors.

The bounds.  u = 2^-53 (fp64) or 2^-24 (fp32).  Measured on the CPU with the committed model on the cases of
test_factor below (and (1000+536)/384), as built and permuted, fp64 and fp32:
    residual max |L D L^T - K| / max (|L| |D| |L|^T)     3.1 - 16.0 u   (largest: (1024+1024)/1024 fp32)
    max (|L| |D| |L|^T) / max |K|                         3.4 - 5.5
    max |L|                                               0.16 - 0.58
    kappa_2(K)                                            10.4 - 19.8
    inertia                                               exactly (n, m), info = 0, every case
    solve, max |K x - b| / (||K||_inf max |x|)            0.29 - 1.46 u
The device sums in another order than the model, so it gets 10 x the largest of what the model itself leaves (the
margin test_gpu_sygst.py uses): RESID_U = 160, SOLVE_U = 14.6."""
import functools

import numpy as np
import pytest

from chol_testkit import (U, UserView, bits, desc, image_matrix, npdt, other_triangle_kept, pxq_refused,
                          ragged_padding_mask, stored_lower, uplo_code)
from sytrf_model import growth_scale, inertia, quasi_definite, residual, split, sytrf_model, sytrs_model

pytestmark = pytest.mark.gpu

RESID_U = 160.0  # 10 x 16.0 u, the model's largest residual (above)
SOLVE_U = 14.6   # 10 x 1.46 u, the model's largest backward error (above)

quasi_definite = functools.lru_cache(maxsize=None)(quasi_definite)  # (one array per case here: copy before writing)


@functools.lru_cache(maxsize=None)
def model(n, m, seed, perm, B, dt):
    return sytrf_model(quasi_definite(n, m, seed, perm).astype(npdt(dt)), B)


def sytrf(ch, K, B, u="L", dt="d", fill=np.nan):
    """-> (info, the factor as Lower storage (D on the diagonal, L below), A after the call, A as stored, stats)"""
    S = stored_lower(K.astype(npdt(dt)), u, fill)
    d = desc(ch, K.shape[0], B, dt)
    d.from_lapack(S)
    info = ch.CHAMELEON_dsytrf_nopiv_Tile(uplo_code(ch, u), d)
    F = d.to_lapack()
    ch.CHAMELEON_Desc_Destroy(d)
    return info, (np.tril(F) if u == "L" else np.triu(F).T), F, S, ch.last_sytrf_stats()


def check_factor(Fg, K, Fm, dt, what=""):
    """the reconstruction and the distance to the model's factor, both over max (|L| |D| |L|^T)"""
    Kd = K.astype(npdt(dt)).astype(np.float64)
    res = residual(Fg, Kd)
    dist = np.abs(Fg.astype(np.float64) - Fm.astype(np.float64)).max() / growth_scale(Fm)
    print(f"sytrf {what} {dt}: residual {res / U[dt]:.1f} u (model {residual(Fm, Kd) / U[dt]:.1f} u), "
          f"|F - F_model| {dist / U[dt]:.1f} u")
    assert res <= RESID_U * U[dt], res / U[dt]
    assert dist <= RESID_U * U[dt], dist / U[dt]


CASES = [(600, 424, 128), (1500, 548, 512), (700, 300, 64), (800, 337, 256), (1024, 1024, 1024), (300, 212, 512)]


@pytest.mark.parametrize("n,m,B", CASES)
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_factor(cham, n, m, B, perm, u, dt):
    """quasi-definite, against the model and by reconstruction; the inertia (the padding of a ragged order is not
    counted); the magnitudes of the stats"""
    ch = cham
    K = quasi_definite(n, m, n + m + B, perm)
    Fm, minfo = model(n, m, n + m + B, perm, B, dt)
    assert minfo == 0
    info, Fg, F, S, st = sytrf(ch, K, B, u, dt)
    assert info == 0
    check_factor(Fg, K, Fm, dt, f"({n}+{m})/{B} perm={perm} {u}")
    assert other_triangle_kept(F, S, u)
    assert st["inertia"] == (n, m) == inertia(Fg)
    d = np.abs(np.diag(Fg).astype(np.float64))
    assert st["min_abs_d"] == d.min() and st["max_abs_d"] == d.max()
    assert st["max_abs_l"] == np.abs(np.tril(Fg, -1)).max()
    assert st["total_ms"] > 0 and st["chain_ms"] > 0 and (n + m <= B or st["update_ms"] > 0)


@pytest.mark.parametrize("dt", ["d", "s"])
def test_inertia_diagonally_dominant(cham, dt):
    """symmetric strictly diagonally dominant with random diagonal signs: the pivot signs are the eigenvalue signs"""
    ch = cham
    n, B = 900, 128
    r = np.random.default_rng(9)
    A = r.standard_normal((n, n))
    A = np.tril(A, -1) + np.tril(A, -1).T
    A[np.diag_indices(n)] = 1.5 * np.abs(A).sum(1) * r.choice([-1.0, 1.0], n)
    A = A.astype(npdt(dt)).astype(np.float64)
    ev = np.linalg.eigvalsh(A)
    info, Fg, _, _, st = sytrf(ch, A, B, "L", dt)
    assert info == 0
    assert st["inertia"] == (int((ev > 0).sum()), int((ev < 0).sum()))
    assert residual(Fg, A) <= RESID_U * U[dt]
    assert st["max_abs_l"] < 0.05


def exact_case(n, seed):
    """L = I + E (E nonzero only in rows >= n/2 and columns < n/2, {-1, 0, 1} at density 1/16: inv(L) = I - E),
    d_j = +-{1, 2, 4}, A = L D L^T: every intermediate is a small integer"""
    r = np.random.default_rng(seed)
    h = n // 2
    E = np.zeros((n, n))
    E[h:, :h] = r.integers(-1, 2, (n - h, h)) * (r.random((n - h, h)) < 1 / 16)
    L = np.eye(n) + E
    d = r.choice([1.0, 2.0, 4.0], n) * r.choice([-1.0, 1.0], n)
    return (L * d) @ L.T, L, d


@pytest.mark.parametrize("n,B", [(1000, 256), (700, 128), (1536, 512)])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_exact_integer(cham, n, B, u, dt):
    """a sparse exact case: every diagonal tile of L but the one that straddles n / 2 is the identity.  The dense exact
    family, with its solves: test_gpu_factor_exact.py::test_sytrf_sytrs_sysv_nopiv"""
    ch = cham
    A, L, d = exact_case(n, n + B)
    info, Fg, _, _, st = sytrf(ch, A, B, u, dt)
    assert info == 0
    Lg, dg = split(Fg)
    assert np.array_equal(Lg, L.astype(npdt(dt))) and np.array_equal(dg, d.astype(npdt(dt)))
    assert st["inertia"] == (int((d > 0).sum()), int((d < 0).sum()))
    assert (st["min_abs_d"], st["max_abs_d"], st["max_abs_l"]) == (1.0, 4.0, 1.0)


def backward_error(K, x, b):
    K = K.astype(np.float64)
    return np.abs(K @ x.astype(np.float64) - b).max() / (np.abs(K).sum(1).max() * np.abs(x).max())


@pytest.mark.parametrize("nrhs", [1, 5, 300])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_solve(cham, nrhs, u, dt):
    """sytrs_nopiv from the factor (A bit-identical afterwards) and sysv_nopiv; one, a ragged few, more than a tile of
    right-hand sides"""
    ch = cham
    n, m, B = 800, 337, 256
    N = n + m
    K = quasi_definite(n, m, 77, True).astype(npdt(dt))
    b = np.random.default_rng(3).standard_normal((N, nrhs)).astype(npdt(dt))
    Fm, _ = model(n, m, 77, True, B, dt)
    bem = backward_error(K, sytrs_model(Fm, b), b.astype(np.float64))
    for call in ("sytrs", "sysv"):
        da, db = desc(ch, N, B, dt), desc(ch, N, B, dt, nrhs)
        S = stored_lower(K, u)
        da.from_lapack(S)
        db.from_lapack(np.asfortranarray(b))
        if call == "sytrs":
            assert ch.CHAMELEON_dsytrf_nopiv_Tile(uplo_code(ch, u), da) == 0
            F0 = da.to_lapack()
            assert ch.CHAMELEON_dsytrs_nopiv_Tile(uplo_code(ch, u), da, db) == 0
            assert np.array_equal(bits(da.to_lapack()), bits(F0))  # A only read
        else:
            assert ch.CHAMELEON_dsysv_nopiv_Tile(uplo_code(ch, u), da, db) == 0
        x = db.to_lapack()
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(db)
        be = backward_error(K, x, b.astype(np.float64))
        print(f"{call} nrhs={nrhs} {u} {dt}: backward error {be / U[dt]:.2f} u (model {bem / U[dt]:.2f} u)")
        assert be <= SOLVE_U * U[dt], be / U[dt]


SING = np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 1]])  # d_1 = 1, d_2 = 0


def embedded_singular(at):
    K = quasi_definite(300, 212, 12).copy()
    K[at:at + 3, :] = 0
    K[:, at:at + 3] = 0
    K[at:at + 3, at:at + 3] = SING
    return K


@pytest.mark.parametrize("at", [40, 200, 500])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_zero_pivot(cham, at, u, dt):
    """a zero pivot in the first, a middle and the LAST tile column (512 = 4 x 128); sysv leaves B untouched"""
    ch = cham
    K = embedded_singular(at)
    assert sytrf_model(K.astype(npdt(dt)), 128)[1] == at + 2
    info, *_ = sytrf(ch, K, 128, u, dt)
    assert info == at + 2
    N = K.shape[0]
    da, db = desc(ch, N, 128, dt), desc(ch, N, 128, dt, 3)
    da.from_lapack(stored_lower(K.astype(npdt(dt)), u))
    b = np.asfortranarray(np.random.default_rng(4).standard_normal((N, 3)).astype(npdt(dt)))
    db.from_lapack(b)
    assert ch.CHAMELEON_dsysv_nopiv_Tile(uplo_code(ch, u), da, db) == at + 2
    assert np.array_equal(bits(db.to_lapack()), bits(b))
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)


@pytest.mark.parametrize("dt", ["d", "s"])
def test_non_finite_and_order_one(cham, dt):
    """a NaN on the diagonal and one below it return an index (ordinary data for the kernels); order 1, negative"""
    ch = cham
    K = quasi_definite(300, 212, 12).copy()
    K[150, 150] = np.nan
    assert sytrf(ch, K, 128, "L", dt)[0] == 151 == sytrf_model(K.astype(npdt(dt)), 128)[1]
    K = quasi_definite(300, 212, 12).copy()
    K[400, 20] = K[20, 400] = np.nan  # reaches the diagonal at row 400
    info = sytrf(ch, K, 128, "L", dt)[0]
    assert info == 401 == sytrf_model(K.astype(npdt(dt)), 128)[1]
    K = quasi_definite(300, 212, 12).copy()
    K[30, 30] = np.inf
    assert sytrf(ch, K, 128, "U", dt)[0] == 31
    info, Fg, _, _, st = sytrf(ch, np.array([[-3.0]]), 64, "L", dt)
    assert info == 0 and Fg[0, 0] == -3.0 and st["inertia"] == (0, 1)
    # a zero on the stored diagonal of a factor: sytrs returns its index, B unchanged
    N = 512
    da, db = desc(ch, N, 128, dt), desc(ch, N, 128, dt, 2)
    F = np.asfortranarray(np.eye(N, dtype=npdt(dt)))
    F[200, 200] = 0
    da.from_lapack(F)
    b = np.asfortranarray(np.ones((N, 2), dtype=npdt(dt)))
    db.from_lapack(b)
    assert ch.CHAMELEON_dsytrs_nopiv_Tile(ch.ChamLower, da, db) == 201
    assert np.array_equal(bits(db.to_lapack()), bits(b))
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)


def test_repeatable_and_padding(cham):
    """two calls give the same bits; a ragged order keeps the padding of the image (the identity on the diagonal,
    zeros elsewhere) bit for bit"""
    ch = cham
    n, B, nt = 1000, 256, 4
    pad = ragged_padding_mask(n, B, nt)
    K = quasi_definite(600, 400, 21, True)
    outs = []
    for _ in range(2):
        da = desc(ch, n, B, "d")
        da.from_lapack(stored_lower(K, "L"))
        before = image_matrix(da, nt, B, np.float64)
        assert ch.CHAMELEON_dsytrf_nopiv_Tile(ch.ChamLower, da) == 0
        outs.append(da.to_lapack())
        after = image_matrix(da, nt, B, np.float64)
        ch.CHAMELEON_Desc_Destroy(da)
        assert np.array_equal(bits(after[pad]), bits(before[pad]))
        assert np.array_equal(after[n:, n:], np.eye(nt * B - n)) and not np.any(after[n:, :n])
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    assert other_triangle_kept(outs[0], stored_lower(K, "L"), "L")


def test_sub_matrix_view(cham):
    """a tile-aligned view of a device user buffer gives the whole-matrix descriptor's result; the user's tiles
    outside the view stay as they were"""
    ch = cham
    uv = UserView(ch)
    mb = uv.mb
    K = quasi_definite(500, 268, 6, True)
    v = uv.view_desc()
    v.from_lapack(stored_lower(K, "L"))
    assert ch.CHAMELEON_dsytrf_nopiv_Tile(ch.ChamLower, v) == 0
    Fv = np.tril(v.to_lapack())
    ch.CHAMELEON_Desc_Destroy(v)
    _, Fg, *_ = sytrf(ch, K, mb)
    assert np.array_equal(bits(Fv), bits(Fg))
    check_factor(Fv, K, sytrf_model(K, mb)[0], "d", "view")
    uv.outside_unchanged()


def test_potrf_still_stops_at_the_first_negative_pivot(cham):
    """existing behaviour: potrf on the unpermuted quasi-definite matrix returns info = n + 1"""
    ch = cham
    n, m, B = 600, 424, 128
    d = desc(ch, n + m, B, "d")
    d.from_lapack(stored_lower(quasi_definite(n, m, n + m + B), "L", 0.0))
    assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d) == n + 1
    ch.CHAMELEON_Desc_Destroy(d)
    assert sytrf(ch, quasi_definite(n, m, n + m + B), B)[0] == 0  # ... where sytrf_nopiv goes through


@pytest.mark.parametrize("dt", ["d", "s"])
def test_spd_matches_potrf(cham, dt):
    """an SPD matrix: D > 0 and L D^(1/2) is potrf's factor"""
    ch = cham
    n, B = 1000, 256
    H = quasi_definite(n, 1, 31)[:n, :n]
    info, Fg, _, _, st = sytrf(ch, H, B, "L", dt)
    assert info == 0 and st["inertia"] == (n, 0)
    d = desc(ch, n, B, dt)
    d.from_lapack(stored_lower(H.astype(npdt(dt)), "L", 0.0))
    assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d) == 0
    Lc = np.tril(d.to_lapack()).astype(np.float64)
    ch.CHAMELEON_Desc_Destroy(d)
    L, dd = split(Fg.astype(np.float64))
    err = np.abs(L * np.sqrt(dd) - Lc).max() / growth_scale(Fg)
    assert err <= RESID_U * U[dt], err / U[dt]


def test_argument_errors(cham):
    from dense_linear_app_amd._lib import lib

    ch = cham
    n, B = 512, 128
    da, db = desc(ch, n, B, "d"), desc(ch, n, B, "d", 3)
    L = lib()
    assert L.chol_sytrf_nopiv_tile(7, da.handle) == -1
    assert L.chol_sytrf_nopiv_tile(ch.ChamLower, None) == -2
    for fn in (L.chol_sytrs_nopiv_tile, L.chol_sysv_nopiv_tile):
        assert fn(7, da.handle, db.handle) == -1
        assert fn(ch.ChamLower, None, db.handle) == -2
        assert fn(ch.ChamLower, da.handle, None) == -3
    assert L.chol_sytrs_nopiv_tile(ch.ChamLower, da.handle, da.handle) == -3  # B aliasing A
    for other in (desc(ch, n, B, "s", 3), desc(ch, n, 256, "d", 3), desc(ch, 640, B, "d", 3)):
        assert L.chol_sytrs_nopiv_tile(ch.ChamLower, da.handle, other.handle) == -3
        ch.CHAMELEON_Desc_Destroy(other)
    rect = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, n, 2 * n, 0, 0, n, 2 * n, 1, 1)
    assert L.chol_sytrf_nopiv_tile(ch.ChamLower, rect.handle) == -2
    assert L.chol_sytrs_nopiv_tile(ch.ChamLower, rect.handle, db.handle) == -2
    ch.CHAMELEON_Desc_Destroy(rect)
    assert L.chol_last_sytrf_stats(None) == -1
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)


def test_pxq_descriptor_is_not_supported(cham):
    ch = cham
    pxq_refused(ch, 1, lambda da: ch.CHAMELEON_dsytrf_nopiv_Tile(ch.ChamLower, da))


def test_large(cham):
    """N = 8192, tile 512, host-built: the residual of the solution through sysv_nopiv"""
    ch = cham
    n, m, B = 5000, 3192, 512
    N = n + m
    r = np.random.default_rng(8)
    G = r.standard_normal((n, 2 * n))
    H = G @ G.T / (2 * n)
    G = r.standard_normal((m, 2 * m))
    C = G @ G.T / (2 * m)
    J = r.standard_normal((m, n)) / np.sqrt(n)
    K = np.block([[H, J.T], [J, -C]])
    b = r.standard_normal((N, 2))
    da, db = desc(ch, N, B, "d"), desc(ch, N, B, "d", 2)
    da.from_lapack(np.asfortranarray(K))
    db.from_lapack(np.asfortranarray(b))
    assert ch.CHAMELEON_dsysv_nopiv_Tile(ch.ChamLower, da, db) == 0
    x = db.to_lapack()
    st = ch.last_sytrf_stats()
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)
    be = backward_error(K, x, b)
    print(f"large: backward error {be / U['d']:.2f} u, stats {st}")
    assert st["inertia"] == (n, m)
    assert be <= SOLVE_U * U["d"], be / U["d"]
