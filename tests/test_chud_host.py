"""CPU-side checks of the rank-r update / downdate of a Cholesky factor (chol_chud_tile / chol_chdd_tile /
chol_last_chud_stats): the Python wrappers and ABI symbols exist, every entry point refuses to run before chol_init,
and the numpy model of the library's arithmetic (chud_model.py) agrees with numpy.linalg.cholesky(A +- V V^T) and
follows the info rule.  The device numerics are in test_gpu_chud.py.

A is a Gram matrix with an n x 2n standard-normal factor (kappa ~ 33, test_gpu_sygst.py's recipe) and V is standard
normal times sqrt(n), so that the update is not negligible; the downdate starts from the factor of A + V V^T (kappa up
to about 6800) and is compared with the factor of A.  Errors are max |dL| / max |L| in units of eps (2^-52, 2^-23).
Measured with this model on this file's inputs, (n, r) = (600, 1), (600, 5), (1000, 16):

    update    fp64 <= 36 eps     fp32 <= 3.1 eps
    downdate  fp64 <= 140 eps    fp32 <= 56 eps

The bounds below are about 10 x that."""
import numpy as np
import pytest

from dense_linear_app_amd import chameleon as ch
from chol_testkit import assert_before_init_refused, assert_symbols_exported
from chud_model import chud_model, problem

SYMBOLS = ["chol_chud_tile", "chol_chdd_tile", "chol_last_chud_stats"]
# [update, downdate] in eps
BOUND = {np.float64: (360.0, 1400.0), np.float32: (31.0, 560.0)}
CASES = [(600, 1), (600, 5), (1000, 16)]


def test_wrappers_exist():
    for p in "ds":
        assert callable(getattr(ch, f"CHAMELEON_{p}chud_Tile"))
        assert callable(getattr(ch, f"CHAMELEON_{p}chdd_Tile"))
    assert callable(ch.last_chud_stats)
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    assert_before_init_refused(sym, (None,) if sym == "chol_last_chud_stats" else (ch.ChamLower, None, None))


def err_eps(L, ref, dt):
    return np.abs(L.astype(np.float64) - ref).max() / np.abs(ref).max() / np.finfo(dt).eps


@pytest.mark.parametrize("n,r", CASES)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_update(n, r, dt):
    _, V, L0, L1 = problem(n, r, n + r)
    info, L, stop = chud_model(L0, V, +1, dt)
    assert (info, stop) == (0, -1) and L.dtype == dt
    e = err_eps(L, L1, dt)
    print(f"update n={n} r={r} {np.dtype(dt).name}: {e:.1f} eps")
    assert e <= BOUND[dt][0], e
    assert not np.any(np.triu(L, 1))


@pytest.mark.parametrize("n,r", CASES)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_downdate(n, r, dt):
    _, V, L0, L1 = problem(n, r, n + r)
    info, L, stop = chud_model(L1, V, -1, dt)
    assert (info, stop) == (0, -1)
    e = err_eps(L, L0, dt)
    print(f"downdate n={n} r={r} {np.dtype(dt).name}: {e:.1f} eps")
    assert e <= BOUND[dt][1], e


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_model_info_rule(dt):
    """v = 1.001 L[:, 137] makes the leading minor of order 138 of L L^T - v v^T indefinite (the first 137 rotations
    have nothing to do: v is zero above row 137); 0.999 leaves it definite"""
    _, _, L, _ = problem(600, 1, 77)
    info, _, stop = chud_model(L, 1.001 * L[:, 137], -1, dt)
    assert (info, stop) == (138, 0)
    info, _, stop = chud_model(L, 0.999 * L[:, 137], -1, dt)
    assert (info, stop) == (0, -1)
    # the update never stops on finite data
    assert chud_model(L, 1.001 * L[:, 137], +1, dt)[0] == 0


def test_model_info_is_column_outer():
    """the second vector fails at column 137, the first one only at column 300: the columns come first"""
    _, _, L, _ = problem(600, 1, 77)
    V = np.stack([1.001 * L[:, 300], 1.001 * L[:, 137]], axis=1)
    info, _, stop = chud_model(L, V, -1)
    assert (info, stop) == (138, 1)
    info, _, stop = chud_model(L, V[:, ::-1], -1)
    assert (info, stop) == (138, 0)


def test_model_nan_stops_at_its_row():
    _, V, L, _ = problem(600, 5, 605)
    V = V.copy()
    V[211, 3] = np.nan
    # (the NaN spreads along row 211 of L and to the later vectors' entries of that row, nowhere else)
    info, _, stop = chud_model(L, V, +1)
    assert (info, stop) == (212, 3)
