"""What the fp32 rows of test_gpu_conditioning.py and the cases of test_gpu_pivot_info.py rest on, checked without a GPU.

Part 1, per fp32 row (cond_cases.py): the rounded input is finite (and free of subnormal entries where that admits the
row), the oracle's scalar fp32 code returns info = 0 on it, the oracle's own fp32 factor and solve meet the backward
bounds the GPU is held to, and the forward assertion is active (16 B eps kappa <= 1/8) on at least half of the kappa rows
of the tile test -- so that a GPU row cannot quietly test nothing, and a device info > 0 is a bug and not bad luck.

Part 2: the blocked emulation of dyadic_model.py in fp32 and fp64 on every perturbed member meets a pivot of exactly 0
(exactly -1) at column j, is exact up to there and stays in the range where the dtype is exact; the tiny last pivot is held
exactly and gives 2^-10.

Sharpness: a small unblocked fp32 Cholesky in numpy passes the assertion helpers the GPU tests use; with one fault --
subnormal pivots flushed to zero, `d <= 0` in place of `!(d > 0)`, a zero pivot replaced by the smallest subnormal, the
last rank-1 term of a pivot dropped -- it fails the matching one."""
import numpy as np
import pytest

import cond_cases as cc
import dyadic_model as dm
from chol_testkit import lower_of, npdt, stored_lower
from cond_cases import eps_of, potrf_backward_ok, rounded, trsm_backward_ok, wide

EPS32 = eps_of("s")
S_ROWS = {name: [r for r in getattr(cc, name)["s"]] for name in ("TILE_KAPPA", "GRADED", "TRIANGULAR", "FULL_KAPPA",
                                                                  "FULL_GRADED", "RANGE", "NAN_TILE")}


def admitted(A):
    assert A.dtype == np.float32 and np.isfinite(A).all()


# ---------------------------------------------------------------- part 1
def test_the_fp64_rows_are_the_ones_the_file_always_had():
    assert cc.rows(cc.TILE_KAPPA)[1][:3] == ["128-100.0", "256-100.0", "512-100.0"]
    assert cc.rows(cc.TILE_KAPPA)[1][11] == "512-10000000000000.0" and cc.rows(cc.TILE_KAPPA)[1][12] == "s-128-10.0"
    assert cc.rows(cc.FULL_KAPPA)[1][3] == "2048-512-100000000.0" and cc.rows(cc.TRIANGULAR)[1][0] == "1000.0"
    assert cc.rows(cc.RANGE, cc.RANGE_ID)[1][0] == "-1010-64" and cc.rows(cc.NAN_TILE)[1][:4] == ["64", "256", "512", "s-64"]
    assert cc.substitution_floor("d") == 1e-15 and abs(cc.substitution_floor("s") / (4.5 * EPS32) - 1) < 0.01


@pytest.mark.parametrize("B,kappa", S_ROWS["TILE_KAPPA"])
def test_tile_kappa_row_is_admitted(orc, B, kappa):
    Akk, A10, A11 = cc.tile_kappa_input("s", B, kappa)
    for M in (Akk, A10, A11):
        admitted(M)
    L, info = orc.spotrf(Akk)
    assert info == 0
    ok, worst = potrf_backward_ok(L, Akk, B, EPS32)
    assert ok, worst
    X = orc.strsm(np.tril(L), A10)
    ok, worst_t = trsm_backward_ok(X, L, A10, B, EPS32)
    assert ok, worst_t
    scale = np.abs(wide(X)) @ np.abs(wide(X)).T + np.abs(wide(A11))
    assert (np.abs(np.tril(orc.ssyrk(X, A11) - orc.dsyrk(wide(X), wide(A11)))) <= 16 * B * EPS32 * np.tril(scale)).all()
    assert (np.abs(orc.sgemm(X, X, A11) - orc.dgemm(wide(X), wide(X), wide(A11))) <= 16 * B * EPS32 * scale).all()
    print(f"B={B} kappa={kappa:.0e}: cond2(Akk) {np.linalg.cond(wide(Akk)):.3g}, oracle backward error / bound: potrf "
          f"{worst:.4f}, trsm {worst_t:.4f}")


def test_forward_assertion_is_active_on_half_the_kappa_rows():
    """POTRF's forward assertion of test_tile_ops_prescribed_kappa, per fp32 row; and the conditions the issue quotes for
    the leading blocks at B = 128"""
    active = []
    for B, kappa in S_ROWS["TILE_KAPPA"]:
        Akk, _, _ = cc.tile_kappa_input("s", B, kappa)
        active.append(bool(16 * B * EPS32 * np.linalg.cond(wide(Akk)) <= 0.125))
    print(list(zip(S_ROWS["TILE_KAPPA"], active)))
    assert 2 * sum(active) >= len(active), active
    assert cc.forward_active("s", "row", 0.125) and not cc.forward_active("s", "row", 0.126)
    assert cc.forward_active("d", "row", 4.5)  # (the fp64 rows assert whatever the factor, as they always have)


@pytest.mark.parametrize("B,decades", S_ROWS["GRADED"])
def test_graded_row_is_admitted(orc, B, decades):
    A, A0, d = cc.graded_input("s", 2 * B, decades, seed=decades * 10 + B)
    admitted(A)
    assert not cc.has_subnormal(A) and np.array_equal(wide(A), d[:, None] * A0 * d[None, :])  # (the unscaling is exact)
    Akk, A10 = np.asfortranarray(A[:B, :B]), np.asfortranarray(A[B:, :B])
    L, info = orc.spotrf(Akk)
    assert info == 0
    # the condition the GPU's factor is asked to show
    kinf = np.linalg.cond(np.tril(wide(L))[:128, :128], np.inf)
    assert kinf > 10.0 ** (decades * 127 / (2 * B) - 1)
    ok, worst = potrf_backward_ok(L, Akk, B, EPS32)
    assert ok, worst
    X = orc.strsm(np.tril(L), A10)
    ok, worst_t = trsm_backward_ok(X, L, A10, B, EPS32)
    assert ok, worst_t
    print(f"B={B} decades={decades}: kappa_inf(L11) {kinf:.3g}, min|a| {np.abs(A[A != 0]).min():.2g}, oracle backward "
          f"error / bound: potrf {worst:.4f}, trsm {worst_t:.4f}")


@pytest.mark.parametrize("kl", [r[0] for r in S_ROWS["TRIANGULAR"]])
def test_triangular_row_is_admitted(orc, kl):
    Lm, A = cc.triangular_input("s", kl)
    admitted(A)
    admitted(np.tril(Lm))
    assert np.isnan(Lm[np.triu_indices(256, 1)]).all()
    Lt = np.tril(np.nan_to_num(Lm))
    X = orc.strsm(Lt, A)
    ok, worst = trsm_backward_ok(X, Lt, A, 256, EPS32)
    assert np.isfinite(X).all() and ok, worst
    print(f"kl={kl:.0e}: kappa_inf(L) {np.linalg.cond(wide(Lt), np.inf):.3g}, oracle backward error / bound {worst:.4f}")


@pytest.mark.parametrize("N,B,kappa", S_ROWS["FULL_KAPPA"])
def test_full_kappa_row_is_admitted(orc, N, B, kappa):
    from chol_testkit import spd_spectral

    A = rounded(spd_spectral(N, kappa, seed=N + B), "s")
    admitted(A)
    L, info = orc.spotrf(A)
    assert info == 0
    L, A = np.tril(wide(L)), wide(A)
    ok, worst = potrf_backward_ok(L, A, N, EPS32)
    assert ok, worst
    assert np.linalg.norm(L @ L.T - A) / np.linalg.norm(A) <= cc.RESIDUAL_F["s"]


@pytest.mark.parametrize("N,B,decades", S_ROWS["FULL_GRADED"])
def test_full_graded_row_is_admitted(orc, N, B, decades):
    A, A0, d = cc.graded_input("s", N, decades, seed=N)
    admitted(A)
    assert not cc.has_subnormal(A) and np.array_equal(wide(A), d[:, None] * A0 * d[None, :])
    L, info = orc.spotrf(A)
    assert info == 0
    ok, worst = potrf_backward_ok(L, A, N, EPS32)
    assert ok, worst


@pytest.mark.parametrize("B,scale_exp", S_ROWS["RANGE"])
def test_exponent_range_row_is_admitted(orc, B, scale_exp):
    A, X = cc.range_input(orc, "s", B, scale_exp)
    admitted(A)
    admitted(X)
    assert (np.diag(A) > 0).all() and not cc.has_subnormal(A) and not cc.has_subnormal(X)
    L, info = orc.spotrf(A)
    assert info == 0 and np.isfinite(np.tril(L)).all() and not cc.has_subnormal(np.tril(L))
    Lref = np.linalg.cholesky(wide(A))
    assert np.abs(np.tril(wide(L)) - Lref).max() <= 16 * B * EPS32 * np.abs(Lref).max()
    Xo = orc.strsm(np.tril(L), X)
    Xref = orc.dtrsm(np.tril(wide(L)), wide(X))
    assert np.isfinite(Xo).all() and np.abs(Xo - Xref).max() <= 16 * B * EPS32 * np.abs(Xref).max()


def test_the_admission_check_sees_a_subnormal_entry(orc):
    """at 2^-110 the reference input already has subnormal off-diagonal entries at B = 384: not a row"""
    A, X = cc.range_input(orc, "s", 384, -110)
    assert cc.has_subnormal(A) or cc.has_subnormal(X)
    assert not cc.has_subnormal(np.array([0.0, 1.2e-38, -1.0, np.inf], dtype=np.float32))
    assert cc.has_subnormal(np.array([1.0, -1.1e-38], dtype=np.float32))


def test_special_pivot_cases_are_what_they_claim(orc):
    """subnormal in fp32, a positive pivot to the oracle: info = 0 and the root of the subnormal on the diagonal"""
    for B in (4, 64, 128):
        for j, v, A in cc.special_pivot_cases("s", B):
            admitted(np.where(np.isinf(A), np.float32(1), A))
            assert np.isinf(v) or 0 < A[j, j] < np.finfo(np.float32).tiny
            L, info = orc.spotrf(A)
            assert info == 0 and L[j, j] == np.sqrt(A[j, j]) and L[j, j] > 0
    A = cc.special_column_input(orc, "s")
    admitted(A)
    assert 0 < A[0, 0] < np.finfo(np.float32).tiny and not cc.has_subnormal(A[1:, :])
    assert (np.abs(wide(A[1:, 0])) < np.sqrt(wide(A[0, 0]) * np.diag(wide(A))[1:])).all()
    L, info = orc.spotrf(A)
    assert info == 0 and np.isfinite(np.tril(L)).all() and np.abs(L[1:, 0]).max() > 0.1


@pytest.mark.parametrize("B", [r[0] for r in S_ROWS["NAN_TILE"]])
def test_nan_rows_have_a_positive_oracle_info(orc, B):
    base = rounded(orc.extract_block(orc.reference_input(B), B, 0, 0), "s")
    admitted(base)
    assert orc.spotrf(base)[1] == 0
    for (i, j) in cc.nan_tile_positions(B):
        A = base.copy(order="F")
        A[i, j] = np.nan
        assert orc.spotrf(A)[1] == i + 1  # (a NaN in row i >= j reaches pivot i first)


def test_nan_whole_matrix_rows_have_a_positive_oracle_info(orc):
    base = rounded(orc.reference_input(1024), "s")
    admitted(base)
    for (i, j) in cc.NAN_WHOLE:
        A = base.copy(order="F")
        A[i, j] = A[j, i] = np.nan
        i32, i64 = orc.spotrf(A)[1], orc.cholesky_lower(wide(A), 256)[1]
        assert i32 == i64 == i + 1, (i, j, i32, i64)  # (structural: either reference will do)


# ---------------------------------------------------------------- part 2
@pytest.mark.parametrize("dt", cc.DTYPES)
@pytest.mark.parametrize("fam,n,B", cc.PIVOT_SHAPES)
def test_emulation_meets_the_pivot_exactly(fam, n, B, dt):
    A, L, s = cc.pivot_member(fam, n, B)
    cols = cc.pivot_columns(n, B)
    assert {0, n - 1} <= set(cols) and (n == B or {B - 1, B, (-(-n // B) - 1) * B} <= set(cols))
    for j in cols:
        for kind, pivot in (("zero", 0.0), ("minus", -1.0)):
            S = cc.stored_exactly(cc.perturbed(A, s, j, kind), dt, "L")
            info, M, peak = dm.potrf_blocked_info(np.tril(S), npdt(dt))
            assert info == j + 1 and M[j, j] == pivot, (fam, n, j, kind, info, M[j, j])
            k, Ld = j // dm.NB * dm.NB, L.astype(npdt(dt))  # exact up to there: the finished blocks, and the failing one's
            assert np.array_equal(M[:, :k], Ld[:, :k]) and np.array_equal(M[k:k + dm.NB, k:j], Ld[k:k + dm.NB, k:j])
            assert 16 * peak < 2.0 ** 24, peak


@pytest.mark.parametrize("dt", cc.DTYPES)
@pytest.mark.parametrize("fam,n,B", cc.TINY_SHAPES)
def test_emulation_keeps_the_tiny_last_pivot(fam, n, B, dt):
    A, L, s = cc.pivot_member(fam, n, B)
    assert not L[n - 1, :n - 1].any()  # (what lets fp32 hold 2^-20 there)
    S = cc.stored_exactly(cc.perturbed(A, s, n - 1, "tiny"), dt, "L")
    assert S[n - 1, n - 1] == 2.0 ** -20
    info, M, peak = dm.potrf_blocked_info(np.tril(S), npdt(dt))
    want = L.astype(npdt(dt))
    want[n - 1, n - 1] = 2.0 ** -10
    assert info == 0 and np.array_equal(M, want) and 16 * peak < 2.0 ** 24


def test_the_tiny_cases_cover_both_families_and_every_shape_of_mirror():
    assert [c for c in cc.PIVOT_SHAPES if c[0] == "mirror"] == [c for c in cc.TINY_SHAPES if c[0] == "mirror"]
    assert {c[0] for c in cc.TINY_SHAPES} == {"mirror", "mod3"}
    assert cc.FORCED[:3] in cc.PIVOT_SHAPES and 2 * 256 <= cc.FORCED[3] < 3 * 256


# ---------------------------------------------------------------- sharpness
FAULTS = ("flush", "le", "zero_to_subnormal", "drop_last")


def chol32(A, fault=None):
    """unblocked (left-looking) fp32 Cholesky of the lower triangle of A -> (info, F), LAPACK's rule for info; one fault:
    flush              a subnormal pivot is taken for zero
    le                 `d <= 0` in place of `!(d > 0)`: a NaN pivot passes
    zero_to_subnormal  a pivot of exactly zero comes out as the smallest subnormal (an update that does not round as an fma)
    drop_last          the last rank-1 term of every pivot is missing"""
    F = np.array(A, dtype=np.float32, order="F")
    n = F.shape[0]
    f32 = np.float32
    with np.errstate(all="ignore"):
        for j in range(n):
            row = F[j, :j]
            terms = row * row
            if fault == "drop_last":
                terms = terms[:-1]
            d = f32(F[j, j] - terms.sum(dtype=f32))
            if fault == "flush" and 0 < abs(d) < np.finfo(f32).tiny:
                d = f32(0)
            if fault == "zero_to_subnormal" and d == 0:
                d = f32(1e-45)
            if (d <= 0) if fault == "le" else not (d > 0):
                F[j, j] = d
                return j + 1, F
            p = np.sqrt(d)
            F[j, j] = p
            F[j + 1:, j] = (F[j + 1:, j] - F[j + 1:, :j] @ row) * (f32(1) / p)
    return 0, F


def potrf_with(fault):
    return lambda A: chol32(A, fault)


def factor_with(fault):
    """factor(S, u) of cond_cases.py on chol32"""
    def factor(S, u):
        info, F = chol32(np.tril(lower_of(np.nan_to_num(S), u)), fault)
        out = stored_lower(F, u, fill=S)
        return info, out
    return factor


PIVOT_SHARP = ("mirror", 200, 200)


def run_helpers(fault, orc):
    """-> the names of the helpers the faulted Cholesky fails"""
    helpers = {
        "special_pivots": lambda: cc.check_special_pivots(potrf_with(fault), orc, "s"),
        "special_column": lambda: cc.check_special_column(potrf_with(fault), orc, "s"),
        "nan_info": lambda: cc.check_nan_info(potrf_with(fault), orc, "s", 64),
        "pivot_zero": lambda: cc.check_pivot_positions(factor_with(fault), *PIVOT_SHARP, "s", "L", kinds=("zero",)),
        "pivot_minus": lambda: cc.check_pivot_positions(factor_with(fault), *PIVOT_SHARP, "s", "U", kinds=("minus",)),
        "tiny": lambda: cc.check_tiny_last_pivot(factor_with(fault), *PIVOT_SHARP, "s", "L"),
    }
    failed = set()
    for name, run in helpers.items():
        try:
            run()
        except AssertionError:
            failed.add(name)
    return failed


def test_the_plain_cholesky_passes_every_helper(orc):
    assert run_helpers(None, orc) == set()


@pytest.mark.parametrize("fault,must_fail", [("flush", {"special_pivots", "special_column"}), ("le", {"nan_info"}),
                                             ("zero_to_subnormal", {"pivot_zero"}),
                                             ("drop_last", {"pivot_zero"})], ids=FAULTS)
def test_one_fault_fails_the_matching_helper(orc, fault, must_fail):
    failed = run_helpers(fault, orc)
    print(fault, sorted(failed))
    assert must_fail <= failed, (fault, failed)
