"""CPU-side checks of the generalized eigenproblem reduction (chol_sygst_tile / chol_last_sygst_stats): the Python
wrappers and ABI symbols exist, both entry points refuse to run before chol_init, and the numpy model of the library's
algorithm (sygst_model.py: LAPACK's blocked DSYGST with the tile as the block and the left solves deferred into one
pass over the tile rows) agrees with scipy's dsygst / ssygst, and is exact on the integer case the GPU test uses.
The device numerics are in test_gpu_sygst.py."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

from chol_testkit import assert_before_init_refused, assert_symbols_exported
from dense_linear_app_amd import chameleon as ch
from sygst_model import sygst_model

SYMBOLS = ["chol_sygst_tile", "chol_last_sygst_stats"]


def test_wrappers_exist():
    for p in "ds":
        assert callable(getattr(ch, f"CHAMELEON_{p}sygst_Tile"))
    assert callable(ch.last_sygst_stats)
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = {"chol_sygst_tile": (1, ch.ChamLower, None, None), "chol_last_sygst_stats": (None,)}[sym]
    assert_before_init_refused(sym, args)


def problem(n, seed, dtype=np.float64):
    """A symmetric, B a Gram matrix with an n x 2n factor (kappa ~ 34), L its Cholesky factor"""
    r = np.random.default_rng(seed)
    G = r.standard_normal((n, 2 * n))
    L = np.linalg.cholesky(G @ G.T / (2 * n))
    H = r.standard_normal((n, n))
    return (H + H.T).astype(dtype), L.astype(dtype)


def rel_err(C, ref, A, L):
    Li = np.linalg.inv(L.astype(np.float64))
    return np.abs(C - ref).max() / (np.abs(A).max() * np.abs(Li).max() ** 2 * A.shape[0])


@pytest.mark.parametrize("n,B", [(700, 128), (1000, 256), (512, 512), (300, 64), (130, 128), (1, 64)])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_model_lower(n, B, dt):
    A, L = problem(n, n + B, np.float64 if dt == "d" else np.float32)
    C = sygst_model(A, L, B)
    fn = lapack.dsygst if dt == "d" else lapack.ssygst
    ref, info = fn(A, L, itype=1, lower=1)
    assert info == 0
    eps = 2.0 ** -53 if dt == "d" else 2.0 ** -24
    assert rel_err(C, np.tril(ref), A, L) <= 4 * eps, rel_err(C, np.tril(ref), A, L)


@pytest.mark.parametrize("n,B", [(700, 128), (333, 64)])
def test_model_upper(n, B):
    """Upper: inv(U^T) A inv(U) with U = L^T is the transposed Lower result (what the library runs)"""
    A, L = problem(n, 7)
    U = L.T.copy()
    ref, info = lapack.dsygst(A, U, itype=1, lower=0)
    assert info == 0
    C = sygst_model(A, L, B)
    assert rel_err(C.T, np.triu(ref), A, L) <= 4 * 2.0 ** -53


def exact_case(n, seed, dtype=np.float64):
    """L = I + E (E strictly lower, {-1, 0, 1} at density 1/16, rows >= n/2 and columns < n/2: E^2 = 0, inv(L) =
    I - E) and A = L M L^T, M symmetric with entries in [-3, 3]: inv(L) A inv(L)^T = M exactly"""
    r = np.random.default_rng(seed)
    h = n // 2
    E = np.zeros((n, n))
    E[h:, :h] = r.integers(-1, 2, (n - h, h)) * (r.random((n - h, h)) < 1 / 16)
    L = np.eye(n) + E
    M = r.integers(-3, 4, (n, n)).astype(np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    A = L @ M @ L.T
    return A.astype(dtype), L.astype(dtype), M.astype(dtype)


@pytest.mark.parametrize("n,B", [(1000, 256), (1100, 128), (1000, 192), (300, 64)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_exact_integer(n, B, dt):
    A, L, M = exact_case(n, n + B, dt)
    assert np.abs(A).max() < 2 ** 20  # (every partial sum an integer below 2^24: exact in fp32 too)
    C = sygst_model(A, L, B)
    assert np.array_equal(C, np.tril(M))
