"""The generalized eigenproblem reduction CHAMELEON_dsygst_Tile / CHAMELEON_ssygst_Tile (LAPACK DSYGST / SSYGST, itype
1) against scipy's dsygst / ssygst and scipy.linalg.eigh(A, B): Lower and Upper, fp64 and fp32, tiles from 128 to
1024, ragged orders, a single tile and a sub-matrix view; an integer case whose result is exact; the other triangle of
A, all of B and the padding of A's image returned bit for bit; repeated calls bit-identical; the argument errors."""
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.linalg.lapack as lapack

from chol_testkit import (UserView, bits, desc, image_matrix, npdt, other_triangle_kept, pxq_refused,
                          ragged_padding_mask, stored_lower, uplo_code)

pytestmark = pytest.mark.gpu

# max |C - ref| / (max |A| ||inv(L)||_2^2): about 10 x what was measured (the CPU model against scipy: 2-4e-16 in
# fp64, 1-2e-7 in fp32)
BOUND = {"d": 4e-15, "s": 2e-6}


@functools.lru_cache(maxsize=None)
def problem(n, seed):
    """A symmetric; B a Gram matrix with an n x 2n factor (kappa ~ 34), L its Cholesky factor, lambda_min(B)"""
    r = np.random.default_rng(seed)
    G = r.standard_normal((n, 2 * n))
    Bm = G @ G.T
    H = r.standard_normal((n, n))
    return H + H.T, Bm, np.linalg.cholesky(Bm), float(np.linalg.eigvalsh(Bm)[0])


def sygst(ch, A, L, B, u="L", dt="d", fill=np.nan, bfill=-7.0):
    """-> (info, C as Lower, A after the call, A as stored, B after the call, B as stored)"""
    SA = stored_lower(A.astype(npdt(dt)), u, fill)
    SB = stored_lower(L.astype(npdt(dt)), u, bfill)
    n = A.shape[0]
    da, db = desc(ch, n, B, dt), desc(ch, n, B, dt)
    da.from_lapack(SA)
    db.from_lapack(SB)
    info = ch.CHAMELEON_dsygst_Tile(1, uplo_code(ch, u), da, db)
    F, FB = da.to_lapack(), db.to_lapack()
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)
    C = np.tril(F) if u == "L" else np.triu(F).T
    return info, C, F, SA, FB, SB


def reference(A, L, dt):
    fn = lapack.dsygst if dt == "d" else lapack.ssygst
    c, info = fn(A.astype(npdt(dt)), L.astype(npdt(dt)), itype=1, lower=1)
    assert info == 0
    return np.tril(c)


@pytest.mark.parametrize("n,B", [(1000, 128), (1100, 192), (1536, 256), (2100, 512), (2048, 1024), (300, 512),
                                 (192, 192)])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_against_lapack(cham, n, B, u, dt):
    ch = cham
    A, _, L, lmin = problem(n, n + B)
    info, C, F, SA, FB, SB = sygst(ch, A, L, B, u, dt)
    assert info == 0
    err = np.abs(C.astype(np.float64) - reference(A, L, dt)).max() / (np.abs(A).max() / lmin)
    assert err <= BOUND[dt], err
    assert other_triangle_kept(F, SA, u)
    assert np.array_equal(bits(FB), bits(SB))  # all of B, the other triangle included
    st = ch.last_sygst_stats()
    assert st["steps"] == -(-n // B) and st["total_ms"] > 0 and st["diag_inv_ms"] > 0
    if n > B:
        assert st["syr2k_ms"] > 0 and st["solve_ms"] > 0 and st["chain_ms"] > 0


@pytest.mark.parametrize("dt", ["d", "s"])
def test_eigenvalues(cham, dt):
    ch = cham
    n, B = 1000, 256
    A, Bm, L, _ = problem(n, 3)
    info, C, *_ = sygst(ch, A, L, B, "L", dt)
    assert info == 0
    C = C.astype(np.float64)
    ev = np.linalg.eigvalsh(C + np.tril(C, -1).T)
    ref = scipy.linalg.eigh(A, Bm, eigvals_only=True)
    err = np.abs(ev - ref).max() / np.abs(ref).max()
    assert err <= (1e-13 if dt == "d" else 1e-5), err


def exact_case(n, seed):
    """L = I + E (E strictly lower, {-1, 0, 1} at density 1/16, rows >= n/2 and columns < n/2: E^2 = 0, inv(L) =
    I - E) and A = L M L^T, M symmetric with entries in [-3, 3]: inv(L) A inv(L)^T = M exactly"""
    r = np.random.default_rng(seed)
    h = n // 2
    E = np.zeros((n, n))
    E[h:, :h] = r.integers(-1, 2, (n - h, h)) * (r.random((n - h, h)) < 1 / 16)
    L = np.eye(n) + E
    M = r.integers(-3, 4, (n, n)).astype(np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    return L @ M @ L.T, L, M


@pytest.mark.parametrize("n,B", [(1000, 256), (1100, 128), (1000, 192)])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_exact_integer(cham, n, B, u, dt):
    """a sparse exact case: n / 2 is not tile-aligned, so E reaches into the one diagonal tile that straddles it; every
    other diagonal tile of L is the identity and most panel tiles are zero.  The dense exact family, in which every
    diagonal block, block inverse and panel tile is non-trivial: test_gpu_factor_exact.py::test_sygst"""
    ch = cham
    A, L, M = exact_case(n, n + B)
    info, C, *_ = sygst(ch, A, L, B, u, dt)
    assert info == 0
    assert np.array_equal(C, np.tril(M).astype(npdt(dt)))


def test_repeatable_and_padding(cham):
    """two calls give the same bits; a ragged order keeps the padding of A's image (the identity on the diagonal,
    zeros elsewhere) bit for bit"""
    ch = cham
    n, B, nt = 1000, 256, 4
    pad = ragged_padding_mask(n, B, nt)
    A, _, L, _ = problem(n, 5)
    outs = []
    for _ in range(2):
        da, db = desc(ch, n, B, "d"), desc(ch, n, B, "d")
        da.from_lapack(stored_lower(A, "L"))
        db.from_lapack(stored_lower(L, "L"))
        before = image_matrix(da, nt, B, np.float64)
        assert ch.CHAMELEON_dsygst_Tile(1, ch.ChamLower, da, db) == 0
        outs.append(da.to_lapack())
        after = image_matrix(da, nt, B, np.float64)
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(db)
        assert np.array_equal(bits(after[pad]), bits(before[pad]))
        assert np.array_equal(after[n:, n:], np.eye(nt * B - n)) and not np.any(after[n:, :n])
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


def test_sub_matrix_view(cham):
    """a tile-aligned view of a device user buffer gives the whole-matrix descriptor's result; the user's tiles
    outside the view stay as they were"""
    ch = cham
    uv = UserView(ch)
    mb, m = uv.mb, uv.m
    A, _, L, _ = problem(m, 6)
    v = uv.view_desc()
    v.from_lapack(stored_lower(A, "L"))
    db = desc(ch, m, mb, "d")
    db.from_lapack(stored_lower(L, "L"))
    assert ch.CHAMELEON_dsygst_Tile(1, ch.ChamLower, v, db) == 0
    Cv = np.tril(v.to_lapack())
    ch.CHAMELEON_Desc_Destroy(v)
    ch.CHAMELEON_Desc_Destroy(db)
    _, C, *_ = sygst(ch, A, L, mb)
    assert np.array_equal(bits(Cv), bits(C))
    uv.outside_unchanged()


@pytest.mark.parametrize("u", ["L", "U"])
def test_zero_on_the_diagonal_of_b(cham, u):
    ch = cham
    n, B = 600, 128
    A, _, L, _ = problem(n, 8)
    L = L.copy()
    L[300, 300] = 0.0
    info, _, F, SA, FB, SB = sygst(ch, A, L, B, u)
    assert info == 301
    assert np.array_equal(bits(F), bits(SA))  # A unchanged
    assert np.array_equal(bits(FB), bits(SB))


def test_argument_errors(cham):
    from dense_linear_app_amd._lib import lib

    ch = cham
    n, B = 512, 128
    da, db = desc(ch, n, B, "d"), desc(ch, n, B, "d")
    L = lib()
    assert L.chol_sygst_tile(0, ch.ChamLower, da.handle, db.handle) == -1
    assert L.chol_sygst_tile(4, ch.ChamLower, da.handle, db.handle) == -1
    assert L.chol_sygst_tile(1, 7, da.handle, db.handle) == -2
    assert L.chol_sygst_tile(1, ch.ChamLower, None, db.handle) == -3
    assert L.chol_sygst_tile(1, ch.ChamLower, da.handle, None) == -4
    assert L.chol_sygst_tile(1, ch.ChamLower, da.handle, da.handle) == -4  # B aliasing A
    for other in (desc(ch, n, B, "s"), desc(ch, n, 256, "d"), desc(ch, 640, B, "d")):
        assert L.chol_sygst_tile(1, ch.ChamLower, da.handle, other.handle) == -4
        ch.CHAMELEON_Desc_Destroy(other)
    rect = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, n, 2 * n, 0, 0, n, 2 * n, 1, 1)
    assert L.chol_sygst_tile(1, ch.ChamLower, rect.handle, db.handle) == -3
    ch.CHAMELEON_Desc_Destroy(rect)
    for itype in (2, 3):
        with pytest.raises(ch.CholmiError) as e:
            ch.CHAMELEON_dsygst_Tile(itype, ch.ChamLower, da, db)
        assert e.value.code == -104  # CHOL_ERR_NOT_SUPPORTED
    assert L.chol_last_sygst_stats(None) == -1
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)


def test_pxq_descriptor_is_not_supported(cham):
    ch = cham
    pxq_refused(ch, 2, lambda da, db: ch.CHAMELEON_dsygst_Tile(1, ch.ChamLower, da, db))
