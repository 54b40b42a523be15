"""CPU-side checks of the L D L^T factorisation without pivoting (chol_sytrf_nopiv_tile / chol_sytrs_nopiv_tile /
chol_sysv_nopiv_tile / chol_last_sytrf_stats): the Python wrappers and ABI symbols exist, every entry point refuses to
run before chol_init, and the numpy model of the library's algorithm (sytrf_model.py: right-looking with the tile as
the block, the reciprocal scaling, the info rule) agrees with an unblocked L D L^T, reconstructs the matrix, and is
exact on the integer case the GPU test uses.  The device numerics are in test_gpu_sytrf.py."""
import numpy as np
import pytest

from chol_testkit import assert_before_init_refused, assert_symbols_exported
from dense_linear_app_amd import chameleon as ch
from sytrf_model import inertia, ldl_unblocked, quasi_definite, residual, split, sytrf_model, sytrs_model

SYMBOLS = ["chol_sytrf_nopiv_tile", "chol_sytrs_nopiv_tile", "chol_sysv_nopiv_tile", "chol_last_sytrf_stats"]


def test_wrappers_exist():
    for p in "ds":
        for r in ("sytrf", "sytrs", "sysv"):
            assert callable(getattr(ch, f"CHAMELEON_{p}{r}_nopiv_Tile"))
    assert callable(ch.last_sytrf_stats)
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = {"chol_sytrf_nopiv_tile": (ch.ChamLower, None), "chol_sytrs_nopiv_tile": (ch.ChamLower, None, None),
            "chol_sysv_nopiv_tile": (ch.ChamLower, None, None), "chol_last_sytrf_stats": (None,)}[sym]
    assert_before_init_refused(sym, args)


U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}


@pytest.mark.parametrize("n,m,B", [(300, 212, 128), (350, 150, 64), (260, 124, 512), (1, 0, 64)])
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_against_unblocked_and_reconstruction(n, m, B, perm, dt):
    K = quasi_definite(n, m, n + m + B, perm).astype(dt)
    F, info = sytrf_model(K, B)
    assert info == 0 and inertia(F) == (n, m)
    ref = np.tril(K).copy()
    assert ldl_unblocked(ref) == 0
    # (two stable orders of the same sums on a matrix with kappa_2 < 20: 100 u is a few kappa u; the model's residual
    # was measured at 3 - 16 u on the GPU test's cases)
    assert np.abs(F.astype(np.float64) - ref).max() <= 100 * U[dt] * np.abs(K).max()
    assert residual(F, K) <= 50 * U[dt]
    if n + m > 1:
        b = np.random.default_rng(2).standard_normal((n + m, 3)).astype(dt)
        x = sytrs_model(F, b).astype(np.float64)
        Kd = K.astype(np.float64)
        assert np.abs(Kd @ x - b).max() / (np.abs(Kd).sum(1).max() * np.abs(x).max()) <= 10 * U[dt]


def exact_case(n, seed, dtype=np.float64):
    """L = I + E (E nonzero only in rows >= n/2 and columns < n/2, {-1, 0, 1} at density 1/16: inv(L) = I - E),
    d_j = +-{1, 2, 4}, A = L D L^T: every intermediate is a small integer"""
    r = np.random.default_rng(seed)
    h = n // 2
    E = np.zeros((n, n))
    E[h:, :h] = r.integers(-1, 2, (n - h, h)) * (r.random((n - h, h)) < 1 / 16)
    L = np.eye(n) + E
    d = r.choice([1.0, 2.0, 4.0], n) * r.choice([-1.0, 1.0], n)
    A = (L * d) @ L.T
    return A.astype(dtype), L.astype(dtype), d.astype(dtype)


@pytest.mark.parametrize("n,B", [(1000, 256), (700, 128), (1536, 512)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_exact_integer(n, B, dt):
    A, L, d = exact_case(n, n + B, dt)
    assert np.abs(A).max() < 2 ** 10
    F, info = sytrf_model(A, B)
    assert info == 0
    Lm, dm = split(F)
    assert np.array_equal(Lm, L) and np.array_equal(dm, d)


def test_model_stops():
    """the first zero pivot's index; a NaN; order 1 with a negative entry"""
    S = np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 1]])
    assert sytrf_model(S, 2)[1] == 2
    K = quasi_definite(100, 60, 5)
    K[40:43, 40:43] = S
    K[40:43, :40] = K[:40, 40:43] = 0
    assert sytrf_model(K, 32)[1] == 42
    K = quasi_definite(100, 60, 5)
    K[70, 70] = np.nan
    assert sytrf_model(K, 64)[1] == 71
    F, info = sytrf_model(np.array([[-3.0]]), 64)
    assert info == 0 and F[0, 0] == -3.0 and inertia(F) == (0, 1)
