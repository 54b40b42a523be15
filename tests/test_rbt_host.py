"""CPU-side checks of the butterfly-randomised symmetric indefinite solve (chol_sytrf_rbt_tile / chol_sytrs_rbt_tile /
chol_sysv_rbt_tile / chol_rbt_apply_tile / chol_last_rbt_stats): the Python wrappers and ABI symbols exist, every entry
point refuses to run before chol_init, and the numpy model (rbt_model.py) of the four-number map equals W^T A W with
the dense W, is exact on an integer case, and solves the families on which L D L^T without pivoting stops or loses
accuracy.  The device numerics are in test_gpu_rbt.py."""
import numpy as np
import pytest

from chol_testkit import assert_before_init_refused, assert_symbols_exported
from dense_linear_app_amd import _lib, chameleon as ch
from rbt_model import (backward_error, butterfly_dense, family, random_w, rbt_sym, rbt_vec, sysv_rbt_model)
from sytrf_model import sytrf_model, sytrs_model

SYMBOLS = ["chol_sytrf_rbt_tile", "chol_sytrs_rbt_tile", "chol_sysv_rbt_tile", "chol_rbt_apply_tile",
           "chol_last_rbt_stats"]
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}


def test_wrappers_exist():
    for p in "ds":
        for r in ("sytrf_rbt", "sytrs_rbt", "sysv_rbt", "rbt_apply"):
            assert callable(getattr(ch, f"CHAMELEON_{p}{r}_Tile"))
    assert callable(ch.last_rbt_stats)
    assert_symbols_exported(SYMBOLS)
    for s in SYMBOLS:
        assert getattr(_lib.lib(), s).argtypes is not None


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = {"chol_sytrf_rbt_tile": (ch.ChamLower, None, None, 2, 1), "chol_sytrs_rbt_tile": (ch.ChamLower, None, None, 2, None),
            "chol_sysv_rbt_tile": (ch.ChamLower, None, None, None, 2, 1, None, None, None, None),
            "chol_rbt_apply_tile": (ch.ChamLower, None, None, 2), "chol_last_rbt_stats": (None,)}[sym]
    assert_before_init_refused(sym, args)


@pytest.mark.parametrize("n", [8, 60, 256])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_map_equals_dense_product(n, depth, dt):
    """the four-number map on the stored triangle is W^T A W: each entry is a sum of at most 4^depth products, so a
    few u of the largest entry (16 u allows 2 u per level and term)"""
    Wc = random_w(n, depth, n + depth, dt)
    A = family("randsym", n, 3).astype(dt)
    W = butterfly_dense(Wc, depth)
    ref = W.T @ A.astype(np.float64) @ W
    got = rbt_sym(A, Wc, depth)
    assert got.dtype == dt and not np.any(np.triu(got, 1))
    assert np.abs(got - np.tril(ref)).max() <= 16 * U[dt] * np.abs(ref).max()
    x = np.random.default_rng(5).standard_normal((n, 3)).astype(dt)
    for trans, M in ((True, W.T), (False, W)):
        y = rbt_vec(x, Wc, depth, trans)
        assert y.dtype == dt
        assert np.abs(y - M @ x.astype(np.float64)).max() <= 16 * U[dt] * np.abs(x).max()
    assert np.array_equal(rbt_vec(x[:, 0], Wc, depth, True), rbt_vec(x, Wc, depth, True)[:, 0])


@pytest.mark.parametrize("depth", [1, 2])
def test_orthogonal_with_unit_entries(depth):
    n = 64
    W = butterfly_dense(np.ones((n, depth)), depth)
    assert np.abs(W.T @ W - np.eye(n)).max() <= 4 * U[np.float64]
    # level 0 is the full-order butterfly: the first row of D_0 pairs column 0 with column n/2
    D0 = butterfly_dense(np.ones((n, 1)), 1)
    assert D0[0, 0] > 0 and D0[0, n // 2] > 0 and D0[n // 2, n // 2] < 0


@pytest.mark.parametrize("n,depth", [(64, 1), (96, 2), (200, 2)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_integer_case_is_exact(n, depth, dt):
    """entries of W equal to 1 and A = 4 x small integers: every halving is exact, so the model equals the integer
    arithmetic of 2^depth W^T A W / 2^depth"""
    r = np.random.default_rng(n)
    A = r.integers(-8, 9, (n, n))
    A = 4 * (np.tril(A) + np.tril(A, -1).T)
    Wc = np.ones((n, depth), dtype=dt)
    S = np.rint(butterfly_dense(Wc, depth) * np.sqrt(2.0) ** depth).astype(np.int64)  # entries 0, +-1
    ref = (S.T @ A @ S) // (2 ** depth)
    assert np.array_equal((S.T @ A @ S) % (2 ** depth), np.zeros_like(A))
    got = rbt_sym(A.astype(dt), Wc, depth)
    assert np.array_equal(got, np.tril(ref).astype(dt))


@pytest.mark.parametrize("name", ["zero_diag", "saddle", "randsym"])
@pytest.mark.parametrize("n,B,depth", [(256, 64, 2), (384, 128, 1)])
def test_model_solves_what_nopiv_does_not(name, n, B, depth):
    """without the butterflies the factorisation stops at a zero pivot or leaves a backward error of hundreds of u;
    with them one or two refinement steps reach DSPOSV's criterion (sqrt(n) u)"""
    A = family(name, n, 11)
    b = np.random.default_rng(12).standard_normal((n, 2))
    F, info = sytrf_model(A, B)
    if info == 0:
        assert backward_error(A, sytrs_model(F, b), b).max() > 50 * U[np.float64]
    m = sysv_rbt_model(A, random_w(n, depth, 13), depth, B, b)
    assert m["info"] == 0 and 0 <= m["iter"] <= 3
    assert m["berr"].max() <= np.sqrt(n) * U[np.float64]
    assert backward_error(A, m["x"], b).max() <= 2 * np.sqrt(n) * U[np.float64]


def test_model_reports_a_singular_matrix():
    m = sysv_rbt_model(np.zeros((64, 64)), random_w(64, 2, 1), 2, 32, np.ones(64))
    assert m["info"] == 1 and m["iter"] == -3 and m["x"] is None
