"""The dyadic input family (dyadic_model.py) is exact for the blocked algorithms in fp32 and fp64: the numpy emulations
return the known answers bit for bit at every order the GPU tests (test_gpu_chain_exact.py, test_gpu_factor_exact.py)
use, and 16 times the largest partial sum any summation order can reach (four fractional bits of headroom) stays below
2^24, the range in which fp32 holds such numbers exactly.  No GPU."""
import numpy as np
import pytest

import dyadic_model as dm

POTRF_ORDERS = [128, 200, 256, 512, 700, 1000, 1024, 1100, 1536, 2048, 4096]
LDL_ORDERS = [700, 1000, 1024, 1536]
SYGST_ORDERS = [1000, 1024, 1100, 1536]
LIMIT = 2.0 ** 24 / 16

DTYPES = [np.float32, np.float64]


def test_the_family_is_what_it_says():
    n = 777
    N = dm.nn(n, n)
    i, j = np.nonzero(N)
    assert (i % 2 == 1).all() and (j % 2 == 0).all() and (i > j).all()
    assert set(np.unique(N)) == {-1.0, 0.0, 1.0}
    dens = len(i) / (((np.arange(n)[:, None] % 2 == 1) & (np.arange(n)[None, :] % 2 == 0) & (np.arange(n)[:, None] > np.arange(n)[None, :])).sum())
    assert 0.45 < dens < 0.55
    assert not np.any(N @ N)
    A, L, s = dm.cholesky_case(n, n)
    assert set(np.unique(s)) == {1.0, 2.0} and np.array_equal(A, A.T)
    assert np.array_equal(dm.inv_factor(n, n) @ L, np.eye(n))
    assert np.array_equal(dm.inv_spd(n, n) @ A, np.eye(n))
    assert np.array_equal(dm.inv_spd(n, n) * 4, np.round(dm.inv_spd(n, n) * 4))
    # every aligned 16-, 64- and 128-block of the factor has a dense inverse of magnitude <= 1 (times 1 / s)
    for nb in (16, 64, 128):
        W = np.linalg.inv(L[256:256 + nb, 256:256 + nb])
        assert np.abs(W).max() <= 1 and np.count_nonzero(np.tril(W, -1)) >= nb * nb // 24
    A, L, d = dm.ldl_case(n, n)
    assert set(np.unique(np.abs(d))) == {1.0, 2.0, 4.0} and (d < 0).any() and (d > 0).any()
    A, L, M = dm.sygst_case(n, n)
    X = dm.inv_factor(n, n)
    assert np.array_equal(X @ A @ X.T, M) and np.abs(M).max() == 3
    assert np.abs(dm.solution(n, 5, n)).max() == 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", POTRF_ORDERS)
def test_potrf_emulation_is_exact(n, dtype):
    A, L, _ = dm.cholesky_case(n, n)
    assert np.abs(A).max() * 16 < 2.0 ** 24
    Lg, peak = dm.potrf_blocked(A.astype(dtype), dtype)
    assert Lg.dtype == dtype and np.array_equal(Lg, L.astype(dtype))
    assert peak < LIMIT, peak


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1024, 1000])
def test_potrf_emulation_is_exact_with_unit_scaling(n, dtype):
    """s = 1: the fall-back of the fp64 cases should the hardware's reciprocal square root be inexact at 4"""
    A, L, s = dm.cholesky_case(n, n, 1)
    assert (s == 1).all()
    Lg, peak = dm.potrf_blocked(A.astype(dtype), dtype)
    assert np.array_equal(Lg, L.astype(dtype)) and peak < LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LDL_ORDERS)
def test_ldl_emulation_is_exact(n, dtype):
    A, L, d = dm.ldl_case(n, n)
    F, peak = dm.ldl_blocked(A.astype(dtype), dtype)
    assert F.dtype == dtype
    assert np.array_equal(np.tril(F, -1), np.tril(L, -1).astype(dtype)) and np.array_equal(np.diag(F), d.astype(dtype))
    assert peak < LIMIT, peak


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SYGST_ORDERS)
def test_sygst_emulation_is_exact(n, dtype):
    A, L, M = dm.sygst_case(n, n)
    assert np.abs(A).max() * 16 < 2.0 ** 24
    C, peak = dm.sygst_blocked(A.astype(dtype), L.astype(dtype), dtype)
    assert C.dtype == dtype and np.array_equal(C, np.tril(M).astype(dtype))
    assert peak < LIMIT, peak


@pytest.mark.parametrize("n", [1000, 1024, 1536])
def test_inverses_and_right_hand_sides_are_exact_in_fp32(n):
    A, L, _ = dm.cholesky_case(n, n)
    Ai = dm.inv_spd(n, n)
    X = dm.solution(n, 300, n)
    for M in (A, dm.inv_factor(n, n), Ai, A @ X):
        assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    assert np.abs(Ai).max() * 16 < 2.0 ** 24
    # the partial sums of A X and of the two triangular sweeps that undo it
    assert (np.abs(A) @ np.abs(X)).max() * 16 < 2.0 ** 24
    assert (np.abs(L) @ np.abs(L.T @ X)).max() * 16 < 2.0 ** 24
    assert (np.abs(dm.inv_factor(n, n)) @ np.abs(A @ X)).max() * 16 < 2.0 ** 24
