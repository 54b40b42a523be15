"""What consumes the factor, bit for bit, on the dyadic families of dyadic_model.py (dense diagonal blocks and panels,
every intermediate a short dyadic number; test_dyadic_host.py proves the reference alone exact in fp32 and fp64 at every
(routine, family, order) used here): potrs / posv, trtri, potri / poinv, lansy, porfs / posvx on the exact solution,
dsposv, the L D L^T
factorisation and its solves, and sygst -- fp64 and fp32, Lower and Upper, a tile-multiple order, a ragged one with an
odd tile, and three tiles of 512.  The factor-consuming routines are fed the exact L directly, so they do not depend on
potrf; posv, poinv, posvx and dsposv run the factorisation themselves.

The families: "parity" (half the rows and columns of the factor empty, every product of two off-diagonal pieces zero),
"mirror" (the other half), "mod3" (Nn^3 = 0: a second-order term in every inverse) and "panel" (dense outside the
diagonal 128-blocks, on tiles of whole 128-blocks only).  The global inverse of a panel member reaches 1e13 at order
1024 and 5e19 at 1536 -- no short dyadic number -- so whatever forms inv(L) or inv(A), or measures them, runs on mirror
and mod3 only: trtri, potri / poinv and porfs / posvx (whose rcond is an estimate of |inv(A)|)."""
import numpy as np
import pytest

import dyadic_model as dm
from chol_testkit import bits, desc, lower_of, npdt, other_triangle_kept, stored_lower, uplo_code

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 256), (1000, 192), (1536, 512)]


def cases(shapes, families):
    """-> (parameters (family, N, B), ids): parity under the ids the shapes alone had, the family in front for the
    others; panel on tiles of whole 128-blocks only"""
    ps = [(fam, N, B) for fam in ("parity",) + families for N, B in shapes if fam != "panel" or B % 128 == 0]
    return {"argvalues": ps, "ids": ["-".join(str(x) for x in (p[1:] if p[0] == "parity" else p)) for p in ps]}


SOLVES = cases(SHAPES, ("mirror", "mod3", "panel"))
INVERSES = cases(SHAPES, ("mirror", "mod3"))
LDL = cases(SHAPES + [(700, 128)], ("mirror", "mod3", "panel"))
SYGST = cases(SHAPES + [(1100, 128)], ("mirror", "mod3", "panel"))


def split(cs, fp64_only):
    """-> (the cases that run in both types, those of fp64_only with their ids)"""
    keep = [(p, i) for p, i in zip(cs["argvalues"], cs["ids"]) if p not in fp64_only]
    assert all(p in cs["argvalues"] for p in fp64_only)
    return ({"argvalues": [p for p, _ in keep], "ids": [i for _, i in keep]},
            {"argvalues": fp64_only, "ids": ["-".join(str(x) for x in p) for p in fp64_only]})


# Not everything the library inverts is a 128-block: sygst multiplies by the inverse of the whole diagonal tile of L, and
# the backward sweep of potrs (so posv, dsposv, sytrs, sysv) by the transposed inverse of the whole diagonal tile.  On
# the panel family such an inverse is large -- magnitude 5e2 for a tile of 256, 2e6 for one of 512 -- and the host
# proofs (test_dyadic_host.py, which follow the library there) leave the range of fp32: for sygst on both tile sizes,
# for the solves on 512.  Those shapes run in fp64 only; dsposv, whose solves are fp32, does not run there at all.
SYGST, SYGST_FP64_ONLY = split(SYGST, [("panel", 1024, 256), ("panel", 1536, 512)])
SOLVES, SOLVES_FP64_ONLY = split(SOLVES, [("panel", 1536, 512)])
LDL, LDL_FP64_ONLY = split(LDL, [("panel", 1536, 512)])


def fam_kw(fam, B):
    return {} if fam == "parity" else {"family": fam, "B": B} if fam == "panel" else {"family": fam}


def stored_as(M, u, dt, fill=np.nan):
    """stored_lower of M rounded to dt"""
    return stored_lower(M.astype(npdt(dt)), u, fill)


def same(got, want, dt):
    want = np.asarray(want).astype(npdt(dt))
    assert got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:6].tolist())


def rhs(fam, N, B, nrhs):
    """(X, A X): integers, exact in fp64 and in fp32"""
    A, _, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    X = dm.solution(N, nrhs, N)
    return X, A @ X


@pytest.mark.parametrize("fam,N,B", **SOLVES)
@pytest.mark.parametrize("nrhs", [1, 5, 300])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_potrs_and_posv(cham, fam, N, B, nrhs, u, dt):
    """the solution is the integer X; after posv A holds L"""
    potrs_and_posv_are_exact(cham, fam, N, B, nrhs, u, dt)


@pytest.mark.parametrize("fam,N,B", **SOLVES_FP64_ONLY)
@pytest.mark.parametrize("nrhs", [1, 5, 300])
@pytest.mark.parametrize("u", ["L", "U"])
def test_potrs_and_posv_on_wide_panel_tiles_in_fp64(cham, fam, N, B, nrhs, u):
    """the panel family on tiles of 512: the backward sweep multiplies by the inverse of a whole diagonal tile, of
    magnitude 2e6 there -- exact in fp64, out of the range of fp32 (the host proof says so; no fp32 case)"""
    potrs_and_posv_are_exact(cham, fam, N, B, nrhs, u, "d")


def potrs_and_posv_are_exact(ch, fam, N, B, nrhs, u, dt):
    A, L, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    X, Bm = rhs(fam, N, B, nrhs)
    SL = stored_as(L, u, dt)
    dA, dB = desc(ch, N, B, dt, content=SL), desc(ch, N, B, dt, nrhs, Bm)
    assert ch.CHAMELEON_dpotrs_Tile(uplo_code(ch, u), dA, dB) == 0
    same(dB.to_lapack(), X, dt)
    assert np.array_equal(bits(dA.to_lapack()), bits(SL))  # the factor is only read
    SA = stored_as(A, u, dt)
    dA.from_lapack(SA)
    dB.from_lapack(Bm.astype(npdt(dt)))
    assert ch.CHAMELEON_dposv_Tile(uplo_code(ch, u), dA, dB) == 0
    same(dB.to_lapack(), X, dt)
    F = dA.to_lapack()
    same(lower_of(F, u), L, dt)
    assert other_triangle_kept(F, SA, u)
    ch.CHAMELEON_Desc_Destroy(dA)
    ch.CHAMELEON_Desc_Destroy(dB)


@pytest.mark.parametrize("fam,N,B", **INVERSES)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_trtri(cham, fam, N, B, u, dt):
    """inv(L) = diag(1/s) (I - Nn), mod3: diag(1/s) (I - Nn + Nn Nn); the other triangle untouched.  (Not panel: its
    inverse is no short dyadic number)"""
    ch = cham
    _, L, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    S = stored_as(L, u, dt)
    d = desc(ch, N, B, dt, content=S)
    assert ch.CHAMELEON_dtrtri_Tile(uplo_code(ch, u), ch.ChamNonUnit, d) == 0
    F = d.to_lapack()
    ch.CHAMELEON_Desc_Destroy(d)
    same(lower_of(F, u), dm.inv_factor(N, N, family=fam), dt)
    assert other_triangle_kept(F, S, u)


@pytest.mark.parametrize("fam,N,B", **INVERSES)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_potri_and_poinv(cham, fam, N, B, u, dt):
    """inv(A) = inv(L)^T inv(L) from the closed form (multiples of 1/4): potri from the exact factor, poinv from A.
    (Not panel: its inverse is no short dyadic number)"""
    ch = cham
    A, L, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    want = np.tril(dm.inv_spd(N, N, family=fam))
    for call, M in ((ch.CHAMELEON_dpotri_Tile, L), (ch.CHAMELEON_dpoinv_Tile, A)):
        S = stored_as(M, u, dt)
        d = desc(ch, N, B, dt, content=S)
        assert call(uplo_code(ch, u), d) == 0
        F = d.to_lapack()
        ch.CHAMELEON_Desc_Destroy(d)
        same(lower_of(F, u), want, dt)
        assert other_triangle_kept(F, S, u)


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_lansy(cham, N, B, u, dt):
    """sums of integers: the one, infinity and max norms equal numpy's; Frobenius on its tolerance"""
    ch = cham
    A, _, _ = dm.cholesky_case(N, N)
    d = desc(ch, N, B, dt, content=stored_as(A, u, dt))
    one = np.abs(A).sum(0).max()
    assert ch.CHAMELEON_dlansy_Tile(ch.ChamOneNorm, uplo_code(ch, u), d) == one
    assert ch.CHAMELEON_dlansy_Tile(ch.ChamInfNorm, uplo_code(ch, u), d) == one
    assert ch.CHAMELEON_dlansy_Tile(ch.ChamMaxNorm, uplo_code(ch, u), d) == np.abs(A).max()
    fro = np.linalg.norm(A)
    assert abs(ch.CHAMELEON_dlansy_Tile(ch.ChamFrobeniusNorm, uplo_code(ch, u), d) - fro) <= (1e-12 if dt == "d" else 1e-5) * fro
    ch.CHAMELEON_Desc_Destroy(d)


@pytest.mark.parametrize("fam,N,B", **INVERSES)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_porfs_and_posvx_on_the_exact_solution(cham, fam, N, B, u, dt):
    """porfs on the exact X: the residual is exactly zero, so berr == 0 and X comes back bit for bit; posvx with
    fact = N (A needs no equilibration) returns X.  (X without zeros: a row of A with two entries -- the last even row
    has no more -- times a zero in both places has the weight |b| + |A| |x| = 0, for which LAPACK's rule, and the
    library's, gives berr = (0 + safe1) / (0 + safe1) = 1.)  Not panel: the error bound and the condition estimate
    sweep with inv(A), which is no short dyadic number there"""
    ch = cham
    A, L, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    nrhs = 5
    X = dm.solution(N, nrhs, N)
    X = np.where(X == 0, 1.0, X)
    Bm = A @ X
    assert (np.abs(Bm) + np.abs(A) @ np.abs(X)).min() >= 1
    SA = stored_as(A, u, dt)
    dA, dAF = desc(ch, N, B, dt, content=SA), desc(ch, N, B, dt, content=stored_as(L, u, dt))
    dB, dX = desc(ch, N, B, dt, nrhs, Bm), desc(ch, N, B, dt, nrhs, X)
    info, ferr, berr = ch.CHAMELEON_dporfs_Tile(uplo_code(ch, u), dA, dAF, dB, dX)
    assert info == 0 and np.array_equal(berr, np.zeros(nrhs)), berr
    same(dX.to_lapack(), X, dt)
    dAF.from_lapack(np.full((N, N), np.nan, dtype=npdt(dt)))
    dX.from_lapack(np.zeros((N, nrhs), dtype=npdt(dt)))
    info, equed, rcond, ferr, berr = ch.CHAMELEON_dposvx_Tile("N", uplo_code(ch, u), dA, dAF, "N", None, dB, dX)
    # (LAPACK's info = n + 1, "rcond below eps", comes with the solution computed; fp32 reaches it at these orders)
    assert info == (N + 1 if rcond < (2.0 ** -53 if dt == "d" else 2.0 ** -24) else 0) and equed == "N" and rcond > 0
    same(dX.to_lapack(), X, dt)
    assert np.array_equal(berr, np.zeros(nrhs)), berr
    same(lower_of(dAF.to_lapack(), u), L, dt)
    assert np.array_equal(bits(dA.to_lapack()), bits(SA))
    for d in (dA, dAF, dB, dX):
        ch.CHAMELEON_Desc_Destroy(d)


@pytest.mark.parametrize("fam,N,B", **SOLVES)
@pytest.mark.parametrize("u", ["L", "U"])
def test_dsposv(cham, fam, N, B, u):
    """the fp32 factor is exact, so the first solve is: the residual is zero, iter = 0 (the loop of dsposv_mixed leaves
    at its first convergence test, after one solve and one residual pass), X bit for bit"""
    ch = cham
    A, _, _ = dm.cholesky_case(N, N, **fam_kw(fam, B))
    nrhs = 5
    X, Bm = rhs(fam, N, B, nrhs)
    SA = stored_as(A, u, "d")
    dA, dB, dX = desc(ch, N, B, "d", content=SA), desc(ch, N, B, "d", nrhs, Bm), desc(ch, N, B, "d", nrhs)
    info, it = ch.CHAMELEON_dsposv_Tile(uplo_code(ch, u), dA, dB, dX)
    st = ch.last_dsposv_stats()
    assert (info, it) == (0, 0) and st["solves"] == 1 and st["residuals"] == 1
    same(dX.to_lapack(), X, "d")
    assert np.array_equal(bits(dA.to_lapack()), bits(SA))
    for d in (dA, dB, dX):
        ch.CHAMELEON_Desc_Destroy(d)


@pytest.mark.parametrize("fam,N,B", **LDL)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_sytrf_sytrs_sysv_nopiv(cham, fam, N, B, u, dt):
    """the L D L^T member: (L, d), the inertia and the stats exact; both solves return the integer X"""
    ldl_is_exact(cham, fam, N, B, u, dt)


@pytest.mark.parametrize("fam,N,B", **LDL_FP64_ONLY)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_sytrf_sytrs_sysv_nopiv_on_wide_panel_tiles(cham, fam, N, B, u, dt):
    """the panel family on tiles of 512: the factorisation in both types (it inverts 128-blocks only); the solves, whose
    backward sweep multiplies by the inverse of a whole diagonal tile, in fp64 alone"""
    ldl_is_exact(cham, fam, N, B, u, dt, solves=dt == "d")


def ldl_is_exact(ch, fam, N, B, u, dt, solves=True):
    A, L, dd = dm.ldl_case(N, N, **fam_kw(fam, B))
    nrhs = 5
    X = dm.solution(N, nrhs, N)
    Bm = A @ X
    SA = stored_as(A, u, dt)
    dA, dB = desc(ch, N, B, dt, content=SA), desc(ch, N, B, dt, nrhs, Bm)

    def check_factor():
        F = dA.to_lapack()
        Fl = lower_of(F, u)
        same(np.tril(Fl, -1), np.tril(L, -1), dt)
        same(np.diag(Fl).copy(), dd, dt)
        assert other_triangle_kept(F, SA, u)
        st = ch.last_sytrf_stats()
        assert st["inertia"] == (int((dd > 0).sum()), int((dd < 0).sum()))
        assert (st["min_abs_d"], st["max_abs_d"], st["max_abs_l"]) == (1.0, 4.0, 1.0)

    assert ch.CHAMELEON_dsytrf_nopiv_Tile(uplo_code(ch, u), dA) == 0
    check_factor()
    assert ch.CHAMELEON_dsytrs_nopiv_Tile(uplo_code(ch, u), dA, dB) == 0
    if solves:
        same(dB.to_lapack(), X, dt)
    dA.from_lapack(SA)
    dB.from_lapack(Bm.astype(npdt(dt)))
    assert ch.CHAMELEON_dsysv_nopiv_Tile(uplo_code(ch, u), dA, dB) == 0
    check_factor()
    if solves:
        same(dB.to_lapack(), X, dt)
    ch.CHAMELEON_Desc_Destroy(dA)
    ch.CHAMELEON_Desc_Destroy(dB)


@pytest.mark.parametrize("fam,N,B", **SYGST)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_sygst(cham, fam, N, B, u, dt):
    """inv(L) (L M L^T) inv(L)^T = M, every tile of L and of the panels dense"""
    sygst_is_exact(cham, fam, N, B, u, dt)


@pytest.mark.parametrize("fam,N,B", **SYGST_FP64_ONLY)
@pytest.mark.parametrize("u", ["L", "U"])
def test_sygst_on_wide_panel_tiles_in_fp64(cham, fam, N, B, u):
    """the panel family on tiles of 256 and 512: the inverse of a whole diagonal tile (second- to sixth-order terms)
    enters every product.  fp64 only: the host emulation proves these two exact there and not in fp32"""
    sygst_is_exact(cham, fam, N, B, u, "d")


def sygst_is_exact(ch, fam, N, B, u, dt):
    A, L, M = dm.sygst_case(N, N, **fam_kw(fam, B))
    SA, SB = stored_as(A, u, dt), stored_as(L, u, dt, fill=-7.0)
    dA, dB = desc(ch, N, B, dt, content=SA), desc(ch, N, B, dt, content=SB)
    assert ch.CHAMELEON_dsygst_Tile(1, uplo_code(ch, u), dA, dB) == 0
    F = dA.to_lapack()
    same(lower_of(F, u), np.tril(M), dt)
    assert other_triangle_kept(F, SA, u)
    assert np.array_equal(bits(dB.to_lapack()), bits(SB))
    ch.CHAMELEON_Desc_Destroy(dA)
    ch.CHAMELEON_Desc_Destroy(dB)
