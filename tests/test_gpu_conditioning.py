"""Parity where it is hard: ill-conditioned and badly scaled inputs, extreme pivots, NaN / Inf -- in fp64 and in fp32.

The reference's arithmetic is LAPACK dpotrf + BLAS dtrsm (W2:238, 323): a backward-stable
factorisation and a backward-stable substitution.  The GPU path solves with explicitly inverted
128 x 128 diagonal blocks, which alone is NOT backward stable (its residual grows with the
condition number of the block) -- so blocks whose inverse says kappa_inf(L11) is above a small
threshold get one step of iterative refinement inside the solve kernels.  These tests pin what
that buys, as a function of kappa (DESIGN.md section 6 carries the same table):

  * componentwise backward error, independent of kappa -- the bounds of Higham, Accuracy and
    Stability of Numerical Algorithms, Th. 10.3 (Cholesky) and Th. 8.5 (substitution), with the
    constant 8 B eps:   |L L^T - A| <= 8 B eps |L||L^T|,   |X L^T - A| <= 8 B eps (|X||L^T| + |A|);
  * forward error against the oracle (substitution TRSM, scalar-pivot POTRF) proportional to kappa:
    max|L - Lref| <= 16 B eps kappa_2(A) max|Lref|,  max|X - Xref| <= 16 B eps kappa_inf(L) max|Xref|
    (for graded matrices D A0 D, kappa of the equilibrated A0 and errors measured after unscaling:
    Cholesky and substitution are invariant under power-of-two diagonal scaling);
  * info identical to the oracle's for NaN / Inf / non-positive pivots; subnormal and huge pivots
    give the oracle's factor.

Every test runs in both dtypes through the d / s entry points (the rows, inputs and helpers: cond_cases.py; what admits
the fp32 rows is checked without a GPU in test_conditioning_host.py).  The fp64 rows are what they were.  An fp32 row is
the fp64 construction rounded to fp32 first, at parameters that keep B eps cond where the fp64 row has it; eps is the
dtype's; the high-precision reference is numpy / the oracle in fp64 on the rounded input, kappa is computed in fp64 from
it, info and the special values follow the oracle's scalar fp32 code (orc.spotrf).  The bounds are the ones above with
that eps.  An fp32 forward assertion is made where 16 B eps kappa <= 1/8 (beyond that it would allow an error as large
as the result; a printed line says so); the backward assertions always run.

Measured on the MI355X, fp32, the worst error over its asserted bound per test (the bound is 1; the oracle's own fp32
routines come to 0.0058 / 0.0035 on the same tile rows, so the inverse-based solve costs nothing visible in fp32):
    test_tile_ops_prescribed_kappa       POTRF backward 0.0051, TRSM backward 0.0038, SYRK / GEMM 0.0015
    test_tile_ops_graded                 POTRF backward 0.0058, TRSM backward 0.0012
    test_trsm_general_triangular_factor  TRSM backward 0.0006 (kappa_inf(L) 4e2 ... 2e6)
    test_full_potrf_prescribed_kappa     componentwise backward 0.0008; residual 0.14 of 4 x the oracle's
    test_full_potrf_graded               componentwise backward 0.0008
    test_pivots_near_the_ends_...        POTRF forward 0.0013, TRSM forward 0.0008 (of 16 B eps max|ref|)
info, the subnormal, +Inf and NaN cases: the oracle's in every case.
"""
import numpy as np
import pytest

import cond_cases as cc
from chol_testkit import chdt, spd_spectral  # noqa: F401  (scripts/cond_table.py takes spd_spectral from here)
from cond_cases import eps_of, potrf_backward_ok, rounded, spd_graded, trsm_backward_ok, wide  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def desc1(ch, a):
    B = a.shape[0]
    return ch.CHAMELEON_Desc_Create(a, ch.ChamRealDouble if a.dtype == np.float64 else ch.ChamRealFloat, B, B, B * B, B,
                                    B, 0, 0, B, B, 1, 1)


def op(ch, dt, name):
    """the d / s entry point of a tile operation"""
    return getattr(ch, f"CHAMELEON_{dt}{name}_Tile")


def tile_potrf(ch, dt):
    """potrf(A) -> (info, F) on one tile, as the helpers of cond_cases.py take it"""
    def potrf(A):
        F = A.copy(order="F")
        return op(ch, dt, "potrf")(ch.ChamLower, desc1(ch, F)), F
    return potrf


def potrf_refs(orc, dt, A):
    """-> (Lref, iref): fp64 the oracle's factor and info; fp32 the fp64 factor of the (rounded) input and the info of the
    oracle's scalar fp32 code"""
    if dt == "d":
        return orc.dpotrf(A)
    _, iref = orc.spotrf(A)
    return (np.linalg.cholesky(wide(A)) if iref == 0 else None), iref


def trsm(ch, dt, L, X):
    return op(ch, dt, "trsm")(ch.ChamRight, ch.ChamLower, ch.ChamTrans, ch.ChamNonUnit, 1.0, desc1(ch, L), desc1(ch, X))


def whole_potrf(ch, dt, A, B):
    """-> (info, tril(L) in fp64) of the whole-matrix factorisation"""
    N = A.shape[0]
    d = ch.CHAMELEON_Desc_Create(None, chdt(ch, dt), B, B, B * B, N, N, 0, 0, N, N, 1, 1)
    d.from_lapack(A)
    info = op(ch, dt, "potrf")(ch.ChamLower, d)
    return info, np.tril(wide(d.to_lapack()))


def whole_refs(orc, dt, A, B):
    """-> (oracle's factor in its dtype, oracle's info, the high-precision factor): fp64 the tile DAG for all three; fp32
    orc.spotrf on the whole matrix and the fp64 factor of the rounded input"""
    if dt == "d":
        Lref, iref = orc.cholesky_lower(A, B)
        return Lref, iref, Lref
    Lo, iref = orc.spotrf(A)
    return np.tril(wide(Lo)), iref, (np.linalg.cholesky(wide(A)) if iref == 0 else None)


TILE_KAPPA = cc.rows(cc.TILE_KAPPA)


@pytest.mark.parametrize("dt,B,kappa", TILE_KAPPA[0], ids=TILE_KAPPA[1])
def test_tile_ops_prescribed_kappa(cham, orc, dt, B, kappa):
    """POTRF -> TRSM -> SYRK/GEMM on Q diag(logspace) Q^T, against the oracle."""
    if kappa > 1e12 and B > 128:
        pytest.skip("kappa 1e13 is within n*eps of singular beyond one 128-block")
    ch, EPS = cham, eps_of(dt)
    Akk, A10, A11 = cc.tile_kappa_input(dt, B, kappa)
    kap = np.linalg.cond(wide(Akk))
    L = Akk.copy(order="F")
    info = op(ch, dt, "potrf")(ch.ChamLower, desc1(ch, L))
    Lref, iref = potrf_refs(orc, dt, Akk)
    assert info == iref == 0
    ok, worst = potrf_backward_ok(L, Akk, B, EPS)
    print(f"ratio {dt} tile_kappa potrf_bw {worst:.4f}")
    assert ok, f"POTRF componentwise backward error {worst:.2f} x bound"
    if cc.forward_active(dt, "POTRF", 16 * B * EPS * kap):
        assert np.abs(np.tril(wide(L)) - np.tril(Lref)).max() <= 16 * B * EPS * kap * np.abs(Lref).max()
    assert np.array_equal(np.triu(L, 1), np.triu(Akk, 1))
    # TRSM against the factor the GPU itself produced (what the DAG does) and against the oracle's
    X = A10.copy(order="F")
    assert trsm(ch, dt, L, X) == 0
    ok, worst = trsm_backward_ok(X, L, A10, B, EPS)
    print(f"ratio {dt} tile_kappa trsm_bw {worst:.4f}")
    assert ok, f"TRSM componentwise backward error {worst:.2f} x bound"
    Xref = orc.dtrsm(np.tril(wide(L)), wide(A10))
    kl = np.linalg.cond(np.tril(wide(L)), np.inf)
    if cc.forward_active(dt, "TRSM", 16 * B * EPS * kl):
        assert np.abs(X - Xref).max() <= 16 * B * EPS * kl * np.abs(Xref).max()
    # SYRK / GEMM with these operands: plain contractions, kappa does not enter
    C = A11.copy(order="F")
    assert op(ch, dt, "syrk")(ch.ChamLower, ch.ChamNoTrans, -1.0, desc1(ch, X), 1.0, desc1(ch, C)) == 0
    Cref = orc.dsyrk(wide(X), wide(A11))
    scale = np.abs(wide(X)) @ np.abs(wide(X)).T + np.abs(wide(A11))
    print(f"ratio {dt} tile_kappa syrk {(np.abs(np.tril(C - Cref)) / (16 * B * EPS * scale)).max():.4f}")
    assert (np.abs(np.tril(C - Cref)) <= 16 * B * EPS * np.tril(scale)).all()
    G = A11.copy(order="F")
    assert op(ch, dt, "gemm")(ch.ChamNoTrans, ch.ChamTrans, -1.0, desc1(ch, X), desc1(ch, X), 1.0, desc1(ch, G)) == 0
    Gref = orc.dgemm(wide(X), wide(X), wide(A11))
    print(f"ratio {dt} tile_kappa gemm {(np.abs(G - Gref) / (16 * B * EPS * scale)).max():.4f}")
    assert (np.abs(G - Gref) <= 16 * B * EPS * scale).all()


GRADED = cc.rows(cc.GRADED)


@pytest.mark.parametrize("dt,B,decades", GRADED[0], ids=GRADED[1])
def test_tile_ops_graded(cham, orc, dt, B, decades):
    """Graded D A0 D: kappa_inf of every leading 128-block of L is ~10^decades, the equilibrated
    problem is benign.  Errors are measured after unscaling."""
    ch, EPS = cham, eps_of(dt)
    A, A0, d = cc.graded_input(dt, 2 * B, decades, seed=decades * 10 + B)
    Akk, A10 = np.asfortranarray(A[:B, :B]), np.asfortranarray(A[B:, :B])
    L = Akk.copy(order="F")
    info = op(ch, dt, "potrf")(ch.ChamLower, desc1(ch, L))
    Lref, iref = potrf_refs(orc, dt, Akk)
    assert info == iref == 0
    assert np.linalg.cond(np.tril(wide(L))[:128, :128], np.inf) > 10.0 ** (decades * 127 / (2 * B) - 1)
    ok, worst = potrf_backward_ok(L, Akk, B, EPS)
    print(f"ratio {dt} tile_graded potrf_bw {worst:.4f}")
    assert ok, f"POTRF componentwise backward error {worst:.2f} x bound"
    k0 = np.linalg.cond(A0[:B, :B])
    dk = d[:B]
    if cc.forward_active(dt, "POTRF", 16 * B * EPS * k0):
        assert np.abs((np.tril(wide(L)) - np.tril(Lref)) / dk[:, None]).max() <= 16 * B * EPS * k0 * np.abs(Lref / dk[:, None]).max()
    X = A10.copy(order="F")
    assert trsm(ch, dt, L, X) == 0
    ok, worst = trsm_backward_ok(X, L, A10, B, EPS)
    print(f"ratio {dt} tile_graded trsm_bw {worst:.4f}")
    assert ok, f"TRSM componentwise backward error {worst:.2f} x bound"
    Xref = orc.dtrsm(np.tril(wide(L)), wide(A10))
    k0l = np.linalg.cond(np.tril(wide(L)) / dk[:, None], np.inf)
    rs = d[B:, None]
    if cc.forward_active(dt, "TRSM", 16 * B * EPS * k0l):
        assert np.abs((X - Xref) / rs).max() <= 16 * B * EPS * k0l * np.abs(Xref / rs).max()


TRIANGULAR = cc.rows(cc.TRIANGULAR)


@pytest.mark.parametrize("dt,kl", TRIANGULAR[0], ids=TRIANGULAR[1])
def test_trsm_general_triangular_factor(cham, orc, dt, kl):
    """TRSM is an ABI operation of its own (W2:323): L need not be a Cholesky factor.  The
    triangular factor of U diag(logspace(0, -log10 kl)) V^T: kappa_2(L) = kl, not graded."""
    ch, EPS = cham, eps_of(dt)
    B = 256
    Lm, A = cc.triangular_input(dt, kl, B)
    X = A.copy(order="F")
    assert trsm(ch, dt, Lm, X) == 0
    Lt = np.tril(np.nan_to_num(wide(Lm)))
    assert np.isfinite(X).all()
    ok, worst = trsm_backward_ok(X, Lt, A, B, EPS)
    print(f"ratio {dt} triangular trsm_bw {worst:.4f}")
    assert ok, f"TRSM componentwise backward error {worst:.2f} x bound"
    Xref = orc.dtrsm(np.asfortranarray(Lt), wide(A))
    kinf = np.linalg.cond(Lt, np.inf)
    if cc.forward_active(dt, "TRSM", 16 * B * EPS * kinf):
        assert np.abs(X - Xref).max() <= 16 * B * EPS * kinf * np.abs(Xref).max()


FULL_KAPPA = cc.rows(cc.FULL_KAPPA)


@pytest.mark.parametrize("dt,N,B,kappa", FULL_KAPPA[0], ids=FULL_KAPPA[1])
def test_full_potrf_prescribed_kappa(cham, orc, dt, N, B, kappa):
    """The whole wave DAG on an ill-conditioned matrix: residual independent of kappa, factor
    within 16 N eps kappa of the oracle's, same info."""
    ch, EPS = cham, eps_of(dt)
    A = rounded(spd_spectral(N, kappa, seed=N + B), dt)
    info, L = whole_potrf(ch, dt, A, B)
    Lorc, iref, Lref = whole_refs(orc, dt, A, B)
    assert info == iref == 0
    A = wide(A)
    assert np.linalg.norm(L @ L.T - A) / np.linalg.norm(A) <= cc.RESIDUAL_F[dt]
    ok, worst = potrf_backward_ok(L, A, N, EPS)
    print(f"ratio {dt} full_kappa potrf_bw {worst:.4f}")
    assert ok
    kap = kappa if dt == "d" else np.linalg.cond(A)  # (fp32: of the rounded input)
    if cc.forward_active(dt, "POTRF", 16 * N * EPS * kap):
        assert np.abs(L - Lref).max() <= 16 * N * EPS * kap * np.abs(Lref).max()
    ores = np.linalg.norm(Lorc @ Lorc.T - A) / np.linalg.norm(A)
    print(f"ratio {dt} full_kappa residual_over_4x_oracle {np.linalg.norm(L @ L.T - A) / np.linalg.norm(A) / (4 * ores):.4f}")
    assert np.linalg.norm(L @ L.T - A) / np.linalg.norm(A) <= max(4 * ores, cc.substitution_floor(dt))  # as good as substitution


FULL_GRADED = cc.rows(cc.FULL_GRADED)


@pytest.mark.parametrize("dt,N,B,decades", FULL_GRADED[0], ids=FULL_GRADED[1])
def test_full_potrf_graded(cham, orc, dt, N, B, decades):
    ch, EPS = cham, eps_of(dt)
    A, A0, dd = cc.graded_input(dt, N, decades, seed=N)
    info, L = whole_potrf(ch, dt, A, B)
    _, iref, Lref = whole_refs(orc, dt, A, B)
    assert info == iref == 0
    ok, worst = potrf_backward_ok(L, A, N, EPS)
    print(f"ratio {dt} full_graded potrf_bw {worst:.4f}")
    assert ok, f"componentwise backward error {worst:.2f} x bound"
    k0 = np.linalg.cond(A0)
    if cc.forward_active(dt, "POTRF", 16 * N * EPS * k0):
        assert np.abs((L - Lref) / dd[:, None]).max() <= 16 * N * EPS * k0 * np.abs(Lref / dd[:, None]).max()


RANGE = cc.rows(cc.RANGE, cc.RANGE_ID)


@pytest.mark.parametrize("dt,B,scale_exp", RANGE[0], ids=RANGE[1])
def test_pivots_near_the_ends_of_the_exponent_range(cham, orc, dt, B, scale_exp):
    """The reference input scaled by 2^+-1010: pivots ~1e-302 / ~1e306 (DBL_MIN 2.2e-308, DBL_MAX
    1.8e308); fp32 by 2^-105 ... 2^114 (FLT_MIN 1.2e-38, FLT_MAX 3.4e38), no entry of the rounded input subnormal.  The
    scaling is exact, so the factor is the oracle's within the usual tolerance."""
    ch, EPS = cham, eps_of(dt)
    A, X = cc.range_input(orc, dt, B, scale_exp)
    assert np.isfinite(A).all() and (np.diag(A) > 0).all()
    assert dt == "d" or not (cc.has_subnormal(A) or cc.has_subnormal(X))
    L = A.copy(order="F")
    info = op(ch, dt, "potrf")(ch.ChamLower, desc1(ch, L))
    Lref, iref = potrf_refs(orc, dt, A)
    assert info == iref == 0
    assert np.isfinite(np.tril(L)).all()
    print(f"ratio {dt} range potrf_fw {np.abs(np.tril(wide(L)) - np.tril(Lref)).max() / (16 * B * EPS * np.abs(Lref).max()):.4f}")
    assert np.abs(np.tril(wide(L)) - np.tril(Lref)).max() <= 16 * B * EPS * np.abs(Lref).max()
    X0 = X.copy(order="F")
    assert trsm(ch, dt, L, X) == 0
    Xref = orc.dtrsm(np.tril(wide(L)), wide(X0))
    print(f"ratio {dt} range trsm_fw {np.abs(X - Xref).max() / (16 * B * EPS * np.abs(Xref).max()):.4f}")
    assert np.abs(X - Xref).max() <= 16 * B * EPS * np.abs(Xref).max()


@pytest.mark.parametrize("dt", cc.DTYPES)
def test_subnormal_and_infinite_pivots_follow_the_oracle(cham, orc, dt):
    """A subnormal pivot is a positive pivot (LAPACK: sqrt, divide); +Inf passes `ajj > 0` too.
    Whatever the oracle's scalar code makes of them, the GPU must make the same."""
    cc.check_special_pivots(tile_potrf(cham, dt), orc, dt)
    # a subnormal pivot with a non-trivial column below it: L(i,j) = a(i,j) / sqrt(tiny) is large but finite
    cc.check_special_column(tile_potrf(cham, dt), orc, dt)


NAN_TILE = cc.rows(cc.NAN_TILE)


@pytest.mark.parametrize("dt,B", NAN_TILE[0], ids=NAN_TILE[1])
def test_nan_input_gives_the_oracles_info(cham, orc, dt, B):
    ch, EPS = cham, eps_of(dt)
    base = cc.check_nan_info(tile_potrf(ch, dt), orc, dt, B)
    # a NaN in the strict upper triangle is never read: info 0, same factor
    A = base.copy(order="F")
    A[3, 7] = np.nan
    got = A.copy(order="F")
    assert op(ch, dt, "potrf")(ch.ChamLower, desc1(ch, got)) == 0
    Lref, _ = potrf_refs(orc, dt, base)
    assert np.abs(np.tril(wide(got)) - np.tril(Lref)).max() <= 16 * B * EPS * np.abs(Lref).max()
    assert np.isnan(got[3, 7])


@pytest.mark.parametrize("dt", cc.DTYPES)
def test_nan_in_a_panel_tile_whole_matrix(cham, orc, dt):
    """NaN below the diagonal tile: the TRSM spreads it over its row, the SYRK onto the diagonal of a
    later tile; info is the oracle's (first NaN pivot, global index)."""
    ch = cham
    N, B = 1024, 256
    base = rounded(orc.reference_input(N), dt)
    for (i, j) in cc.NAN_WHOLE:
        A = base.copy(order="F")
        A[i, j] = A[j, i] = np.nan
        info, _ = whole_potrf(ch, dt, A, B)
        _, iref, _ = whole_refs(orc, dt, A, B)
        assert info == iref and info > 0, (i, j, info, iref)
