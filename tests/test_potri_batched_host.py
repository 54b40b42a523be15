"""CPU-side checks of the batched inverses (chol_trtri_batched, chol_potri_batched, chol_poinv_batched,
chol_invdiag_batched): the ABI symbols and the Python functions exist, every entry point refuses to run before
chol_init, the wrapper's layout rules raise ValueError on CPU tensors before any library call and send a row-major
tensor to the library with the other uplo, the numpy models of the arithmetic (potri_batched_model.py) return the exact
inverses of the dyadic families bit for bit, trtri_model is solve_forward(L, I) bit for bit, the models meet the
componentwise bounds on the shared inputs and confine a planted NaN to the entries that depend on it, and no new
kernel uses scratch.  The device numerics are in test_gpu_potri_batched.py.

The bounds are theorems (potri_batched_model.py).  Measured with the models on spectral_case's factors (seeds 0..3,
the orders of HOST_ORDERS, both dtypes): at worst 0.33 of trtri's bound and 0.47 of the product's."""
import os
from fractions import Fraction

import numpy as np
import pytest

from dense_linear_app_amd import batched
from dense_linear_app_amd import chameleon as ch
from chol_testkit import assert_before_init_refused, assert_symbols_exported, bits
from potri_batched_model import (FAMILIES, HOST_ORDERS, SEEDS, dyadic_inverse, lauum_model, lauum_ratio, potri_model,
                                 spectral_inverse, trtri_model, trtri_ratio)
from trtrs_batched_model import solve_forward

SYMBOLS = ["chol_trtri_batched", "chol_potri_batched", "chol_poinv_batched", "chol_invdiag_batched"]
_IN_PLACE = (ch.ChamLower, ch.ChamRealDouble, 4, None, 4, 16, 1, None)
ARGS = {"chol_trtri_batched": _IN_PLACE, "chol_potri_batched": _IN_PLACE, "chol_poinv_batched": _IN_PLACE,
        "chol_invdiag_batched": (ch.ChamLower, ch.ChamRealDouble, 4, None, 4, 16, None, 4, 1, None)}


def test_symbols_and_functions_exist():
    assert_symbols_exported(SYMBOLS)
    for name in ("trtri_batched", "potri_batched", "poinv_batched", "invdiag_batched"):
        assert callable(getattr(batched, name)) and name in batched.__all__ and name in batched.__doc__


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    assert_before_init_refused(sym, ARGS[sym])


def test_wrapper_layout_rules_on_cpu_tensors():
    """uplo speaks of the mathematical matrix: a row-major tensor is the column-major image of the transpose, whose
    inverse is the transposed inverse, so the other code goes to the library and nothing else changes; a good layout
    on the CPU is refused as such and every bad one before that -- all before any library call"""
    import torch

    L, U, f64 = ch.ChamLower, ch.ChamUpper, torch.float64
    cm = torch.empty(3, 4, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 4), strides (20, 1, 5)
    rm = torch.empty(3, 4, 6, dtype=torch.float32)[:, :, :4]  # strides (24, 6, 1)
    for u in (L, U):
        assert batched._images_of_A(cm, u) == (ch.ChamRealDouble, u, 4, 5, 20, 3)
        assert batched._images_of_A(rm, u) == (ch.ChamRealFloat, U if u == L else L, 4, 6, 24, 3)
    fns = (batched.trtri_batched, batched.potri_batched, batched.poinv_batched, batched.invdiag_batched)
    for fn in fns:
        for good in (cm, rm, torch.empty(4, 4, dtype=f64)):
            with pytest.raises(ValueError, match="device tensors"):
                fn(good, U)
        with pytest.raises(ValueError, match="uplo"):
            fn(cm, 0)
        for bad in (torch.empty(3, 4, 5, dtype=f64), torch.empty(3, 4, 4, dtype=torch.float16), np.eye(4),
                    torch.empty(3, 8, 8, dtype=f64)[:, ::2, ::2], torch.empty(4, dtype=f64)):
            with pytest.raises(ValueError) as e:
                fn(bad)
            assert "device" not in str(e.value)


def _exact(M):
    return [[Fraction(float(x)) for x in row] for row in M]


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_models_are_exact_on_the_dyadic_families(n, dt):
    """L W == I and X == W^T W in exact arithmetic, W with at most 3 significant bits, and the models in the dtype
    return that W and X bit for bit"""
    for family in FAMILIES:
        seeds = SEEDS if n <= 17 else SEEDS[:1]  # (the rational products are cubic in n)
        for seed in seeds:
            A, L, W, X = dyadic_inverse(n, seed, family, dt)
            key = (family, seed)
            assert W.dtype == L.dtype == X.dtype and not np.triu(W, 1).any() and not np.triu(X, 1).any()
            Lq, Wq, Xq = _exact(L), _exact(W), _exact(X)
            for i in range(n):
                for c in range(i + 1):
                    assert sum(Lq[i][k] * Wq[k][c] for k in range(c, i + 1)) == (1 if i == c else 0), key
                    assert sum(Wq[k][i] * Wq[k][c] for k in range(i, n)) == Xq[i][c], key
            m, _ = np.frexp(np.abs(W[W != 0]).astype(np.float64))
            assert np.array_equal(m * 8, np.round(m * 8)), key  # at most 3 significant bits
            Wm, info = trtri_model(L, dt)
            assert info == 0 and np.array_equal(bits(Wm), bits(W)), key
            assert np.array_equal(bits(lauum_model(Wm, dt)), bits(X)), key
            Xm, info = potri_model(L, dt)
            assert info == 0 and np.array_equal(bits(Xm), bits(X)), key


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_trtri_model_is_the_forward_solve_of_the_identity(n, dt):
    cases = [spectral_inverse(n, seed, dt)[1] for seed in SEEDS]
    cases += [dyadic_inverse(n, n, family, dt)[1] for family in FAMILIES]
    for L in cases:
        W, info = trtri_model(L, dt)
        Y, info2 = solve_forward(L, np.eye(n, dtype=L.dtype), dt)
        assert info == 0 and info2 == 0 and W.dtype == L.dtype
        assert np.array_equal(bits(W), bits(Y))
    Z = np.array(cases[0])
    Z[n // 2, n // 2] = 0
    W, info = trtri_model(Z, dt)
    assert info == n // 2 + 1 and np.array_equal(bits(W), bits(Z))
    X, info = potri_model(Z, dt)
    assert info == n // 2 + 1 and np.array_equal(bits(X), bits(Z))


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_models_meet_the_bounds(n, dt):
    worst = np.zeros(2)
    for seed in SEEDS:
        A, L, W, X = spectral_inverse(n, seed, dt)
        assert W.dtype == L.dtype == X.dtype == A.dtype
        worst = np.maximum(worst, [trtri_ratio(L, W, dt), lauum_ratio(W, X, dt)])
    print(f"n={n} {dt}: of the bounds, trtri {worst[0]:.2f}, the product {worst[1]:.2f}")
    assert (worst <= 1.0).all()


@pytest.mark.parametrize("n", [3, 9, 17])
def test_models_confine_a_nan(n):
    L = spectral_inverse(n, 0, "d")[1]
    W, _ = trtri_model(L, "d")
    X = lauum_model(W, "d")
    k, c = np.indices((n, n))
    for p, q in {(n - 1, 0), (n // 2, n // 2), (n - 1, n // 2), (n - 1, n - 1), (0, 0)}:
        M = L.copy()
        M[p, q] = np.nan
        Wn, info = trtri_model(M, "d")
        Xn = lauum_model(Wn, "d")
        hit_w = (c <= q) & (k >= p)
        hit_x = (c <= q) & (k >= c)
        assert info == 0 and np.isnan(Wn[hit_w]).all() and np.isnan(Xn[hit_x]).all()
        assert np.array_equal(bits(Wn[~hit_w]), bits(W[~hit_w])) and np.array_equal(bits(Xn[~hit_x]), bits(X[~hit_x]))


def test_kernels_use_no_scratch():
    import codeobj

    so = os.path.join(os.path.dirname(os.path.abspath(ch.__file__)), "libcholmi.so")
    seen = 0
    for elf in codeobj.device_elfs(so):
        for name, res in codeobj.kernel_resources(so, elf).items():
            if "k_inv_rows" in name:
                seen += 1
                assert res["scratch"] == 0, (name, res)
    assert seen == 64  # two precisions, four padded orders, two triangles, four routines
