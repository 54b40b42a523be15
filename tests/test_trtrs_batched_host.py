"""CPU-side checks of the batched half routines (chol_trtrs_batched, chol_trmm_batched, chol_logdet_batched): the ABI
symbols and the Python functions exist, every entry point refuses to run before chol_init, the wrapper's layout rules
raise ValueError on CPU tensors before any library call and send a row-major tensor to the library with uplo AND trans
flipped, the numpy models of the arithmetic (trtrs_batched_model.py) return the dyadic solutions and products bit for
bit, forward then backward is potrf_batched_model.solve_model bit for bit, the models meet the componentwise bounds on
the shared inputs, and no new kernel uses scratch.  The device numerics are in test_gpu_trtrs_batched.py.

The bounds are theorems (trtrs_batched_model.py).  Measured with the models on spectral_case's factors (seeds 0..3,
the orders of HOST_ORDERS, both dtypes, the right-hand sides spectral_case's three standard normal columns): at worst
0.51 of the forward solve's bound, 0.47 of the backward solve's, 0.55 of the forward product's and 0.36 of the
backward product's (alpha = -1.5, which adds a rounding; every worst case at n = 2) and 0.19 of logdet's."""
import os

import numpy as np
import pytest

from dense_linear_app_amd import batched
from dense_linear_app_amd import chameleon as ch
from chol_testkit import assert_before_init_refused, assert_symbols_exported, bits
from potrf_batched_model import solve_model
from trtrs_batched_model import (FAMILIES, HOST_ORDERS, SEEDS, dyadic_products, logdet, logdet_ratio, mul_backward,
                                 mul_forward, solve_backward, solve_forward, spectral_factor, trmm_ratio, trtrs_ratio)

SYMBOLS = ["chol_trtrs_batched", "chol_trmm_batched", "chol_logdet_batched"]
ARGS = {"chol_trtrs_batched": (ch.ChamLower, ch.ChamNoTrans, ch.ChamRealDouble, 4, 1, None, 4, 16, None, 4, 4, 1, None),
        "chol_trmm_batched": (ch.ChamLower, ch.ChamNoTrans, ch.ChamRealDouble, 4, 1, 1.0, None, 4, 16, None, 4, 4, 1),
        "chol_logdet_batched": (ch.ChamRealDouble, 4, None, 4, 16, 1, None, None)}


def test_symbols_and_functions_exist():
    assert_symbols_exported(SYMBOLS)
    for name in ("trtrs_batched", "trmm_batched", "logdet_batched"):
        assert callable(getattr(batched, name)) and name in batched.__all__


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    assert_before_init_refused(sym, ARGS[sym])


def test_wrapper_layout_rules_on_cpu_tensors():
    """uplo and trans speak of the mathematical matrix: a row-major tensor is the column-major image of the transpose,
    so both codes flip on the way to the library; a good layout on the CPU is refused as such and every bad one
    before that -- all before any library call"""
    import torch

    L, U, N, T, f64 = ch.ChamLower, ch.ChamUpper, ch.ChamNoTrans, ch.ChamTrans, torch.float64
    cm = torch.empty(3, 4, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 4), strides (20, 1, 5)
    rm = torch.empty(3, 4, 6, dtype=torch.float32)[:, :, :4]  # strides (24, 6, 1)
    for u, t in ((L, N), (L, T), (U, N), (U, T)):
        assert batched._half_of_A(cm, u, t) == (ch.ChamRealDouble, u, t, 4, 5, 20, 3)
        assert batched._half_of_A(rm, u, t) == (ch.ChamRealFloat, U if u == L else L, T if t == N else N, 4, 6, 24, 3)
    B1 = torch.empty(3, 4, dtype=f64)
    for call in (lambda: batched.trtrs_batched(cm, B1), lambda: batched.trmm_batched(cm, B1, L, T, 2.0),
                 lambda: batched.logdet_batched(cm), lambda: batched.logdet_batched(rm)):
        with pytest.raises(ValueError, match="device tensors"):
            call()
    for fn in (batched.trtrs_batched, batched.trmm_batched):
        with pytest.raises(ValueError, match="trans"):
            fn(cm, B1, L, 0)
        with pytest.raises(ValueError, match="uplo"):
            fn(cm, B1, 0, N)
        with pytest.raises(ValueError, match="row-major"):
            fn(cm, torch.empty(3, 4, 7, dtype=f64))
        with pytest.raises(ValueError, match="torch tensor"):
            fn(cm, np.zeros((3, 4)))
        for bad in (torch.empty(3, 5, dtype=f64), torch.empty(2, 4, dtype=f64), torch.empty(3, 4, dtype=torch.float32),
                    torch.empty(3, 8, dtype=f64)[:, ::2]):
            with pytest.raises(ValueError) as e:
                fn(cm, bad)
            assert "device" not in str(e.value)
    for bad in (torch.empty(3, 4, 5, dtype=f64), torch.empty(3, 4, 4, dtype=torch.float16), np.eye(4)):
        with pytest.raises(ValueError) as e:
            batched.logdet_batched(bad)
        assert "device" not in str(e.value)


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_models_are_exact_on_the_dyadic_family(n, dt):
    """L X and L^T X are exactly representable, and the models return X from them and them from X, bit for bit"""
    for family in FAMILIES:
        for seed in SEEDS:
            L, X, LX, LtX = dyadic_products(n, 3, seed, family, dt)
            exact_f = L.astype(np.longdouble) @ X.astype(np.longdouble)
            exact_b = L.astype(np.longdouble).T @ X.astype(np.longdouble)
            assert np.array_equal(LX.astype(np.longdouble), exact_f) and np.abs(LX).max() <= 104
            assert np.array_equal(LtX.astype(np.longdouble), exact_b) and np.abs(LtX).max() <= 104
            assert set(np.diag(L)) <= {1.0, 2.0, 4.0}
            key = (family, seed)
            Y, info = solve_forward(L, LX, dt)
            assert info == 0 and np.array_equal(bits(Y), bits(X)), key
            Y, info = solve_backward(L, LtX, dt)
            assert info == 0 and np.array_equal(bits(Y), bits(X)), key
            for alpha in (1.0, -2.0):
                assert np.array_equal(bits(mul_forward(L, X, alpha, dt)), bits(X.dtype.type(alpha) * LX)), key
                assert np.array_equal(bits(mul_backward(L, X, alpha, dt)), bits(X.dtype.type(alpha) * LtX)), key
            value, info = logdet(np.diag(L))
            assert info == 0 and logdet_ratio(value, np.diag(L)) <= 1.0


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_forward_then_backward_is_the_solve_model(n, dt):
    cases = [spectral_factor(n, seed, dt) for seed in SEEDS]
    cases += [dyadic_products(n, 3, n, family, dt)[::2] for family in FAMILIES]  # (L, L X)
    for L, B in cases:
        Y, info = solve_forward(L, B, dt)
        assert info == 0
        X, info = solve_backward(L, Y, dt)
        assert info == 0
        assert np.array_equal(bits(X), bits(solve_model(L, B, dt)[0]))
    Z = np.array(cases[0][0])
    Z[n // 2, n // 2] = 0
    for model in (solve_forward, solve_backward):
        X, info = model(Z, cases[0][1], dt)
        assert info == n // 2 + 1 and np.array_equal(bits(X), bits(cases[0][1]))


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_models_meet_the_bounds(n, dt):
    worst = np.zeros(5)
    for seed in SEEDS:
        L, B = spectral_factor(n, seed, dt)
        assert L.dtype == B.dtype
        Y, info = solve_forward(L, B, dt)
        X, info2 = solve_backward(L, B, dt)
        assert info == 0 and info2 == 0 and Y.dtype == L.dtype and X.dtype == L.dtype
        Cf, Cb = mul_forward(L, B, -1.5, dt), mul_backward(L, B, -1.5, dt)
        value, info = logdet(np.diag(L))
        assert info == 0
        worst = np.maximum(worst, [trtrs_ratio(L, Y, B, dt), trtrs_ratio(L.T, X, B, dt),
                                   trmm_ratio(L, Cf, B, -1.5, dt), trmm_ratio(L.T, Cb, B, -1.5, dt),
                                   logdet_ratio(value, np.diag(L))])
    print(f"n={n} {dt}: of the bounds, solve {worst[0]:.2f} / {worst[1]:.2f}, product {worst[2]:.2f} / {worst[3]:.2f} "
          f"(forward / backward), logdet {worst[4]:.2f}")
    assert (worst <= 1.0).all()


def test_logdet_model_info():
    d = np.array([2.0, 0.5, 4.0, 1.0])
    assert logdet(d) == (2 * ((np.log(2.0) + np.log(0.5)) + np.log(4.0)), 0)
    assert logdet(np.zeros(0)) == (0.0, 0)
    for planted, want in (([(2, 0.0)], 3), ([(1, -1.0)], 2), ([(3, np.nan)], 4), ([(3, 0.0), (0, np.nan)], 1)):
        e = d.copy()
        for j, v in planted:
            e[j] = v
        value, info = logdet(e)
        assert info == want and np.isnan(value)


def test_kernels_use_no_scratch():
    import codeobj

    so = os.path.join(os.path.dirname(os.path.abspath(ch.__file__)), "libcholmi.so")
    seen = {"k_half_rows": 0, "k_zero_rows": 0, "k_diag_logdet": 0}
    for elf in codeobj.device_elfs(so):
        for name, res in codeobj.kernel_resources(so, elf).items():
            for k in seen:
                if k in name:
                    seen[k] += 1
                    assert res["scratch"] == 0, (name, res)
                    assert "k_batched" not in name and "k_chud_rows" not in name
    # two precisions, four padded orders, two triangles, four sweeps; two precisions each for the small ones
    assert seen == {"k_half_rows": 64, "k_zero_rows": 2, "k_diag_logdet": 2}
