"""chol_symm_tile without a GPU: the symbols and wrappers, the refusal before chol_init, the numpy model
(symm_model.py) against a dense product, and the proof that the exact family of test_gpu_symm.py is exact for any
summation order: for every case max |alpha| (|A| |B|) + |beta| |C| is below 2^24 -- here even below 2^23, so that the
multiples of 1/2 which alpha = 0.5 produces are numbers of fp32 too.  The largest case (n = 640, nrhs = 300) reaches a
few thousand."""
import numpy as np
import pytest

import symm_model as sm
from chol_testkit import assert_before_init_refused, assert_symbols_exported, npdt, stored_sym
from dense_linear_app_amd import chameleon as ch

SYMBOLS = ["chol_symm_tile", "chol_last_symm_stats"]


def test_wrappers_exist():
    for p in "ds":
        assert callable(getattr(ch, f"CHAMELEON_{p}symm_Tile"))
    assert callable(ch.last_symm_stats)
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = {"chol_symm_tile": (ch.ChamLeft, ch.ChamLower, 1.0, None, None, 0.0, None),
            "chol_last_symm_stats": (None,)}[sym]
    assert_before_init_refused(sym, args)


@pytest.mark.parametrize("n,tile", sm.SHAPES)
def test_the_exact_family_is_exact_in_any_order(n, tile):
    A, B, C = sm.exact_problem(n)
    assert np.array_equal(A, A.T) and np.abs(A).max() <= 4 and np.abs(B).max() <= 4 and np.abs(C).max() <= 8
    worst = 0.0
    for nrhs in sm.NRHS:
        for alpha, beta in sm.SCALARS:
            worst = max(worst, sm.magnitude(A, B[:, :nrhs], C[:, :nrhs], alpha, beta))
    print(f"n={n}: max |alpha| (|A| |B|) + |beta| |C| = {worst:g}")
    assert worst < 2.0 ** 24
    assert 2 * worst < 2.0 ** 24  # (multiples of 1/2)
    # the results are numbers of fp32
    for alpha, beta in sm.SCALARS:
        R = alpha * (A @ B) + beta * C
        assert np.array_equal(R.astype(np.float32).astype(np.float64), R)


@pytest.mark.parametrize("dt", ["d", "s"])
@pytest.mark.parametrize("u", ["L", "U"])
def test_model_reads_one_triangle(u, dt):
    """the model on the stored triangle (NaN in the other) is the dense product, and follows BLAS's rules for the scalars"""
    n, nrhs = 100, 8
    A, B, C = (a.astype(npdt(dt)) for a in sm.exact_problem(n))
    B, C = B[:, :nrhs], C[:, :nrhs]
    S = stored_sym(A, u).astype(npdt(dt))
    for alpha, beta in sm.SCALARS:
        want = alpha * (A.astype(np.float64) @ B) + beta * C
        got = sm.symm(S, u, alpha, B, beta, np.full_like(C, np.nan) if beta == 0 else C)
        assert got.dtype == npdt(dt) and np.array_equal(got, want)
    nan = np.full_like(B, np.nan)
    assert np.array_equal(sm.symm(np.full_like(S, np.nan), u, 0.0, nan, -1.0, C), -C)
    assert np.array_equal(sm.symm(np.full_like(S, np.nan), u, 0.0, nan, 0.0, nan), np.zeros_like(C))
