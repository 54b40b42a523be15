"""CPU-side checks of the batched small-matrix routines (chol_potrf_batched, chol_potrs_batched, chol_posv_batched,
chol_last_batched_stats): the ABI symbols and the Python functions exist, every entry point refuses to run before
chol_init, the wrapper's stride rules raise ValueError on CPU tensors before any library call, the numpy model of the
arithmetic (potrf_batched_model.py) meets the componentwise bounds on the shared inputs and returns the dyadic factor
and solution bit for bit, and no batched kernel uses scratch.  The device numerics are in test_gpu_potrf_batched.py.

The bounds are theorems (potrf_batched_model.py).  Measured with the model on the shared inputs
(spd_spectral(n, 1e3, 100 n + seed), seeds 0..3, the orders of HOST_ORDERS): at worst 0.47 of the factor bound and
0.21 of the solve bound (right-hand sides: spectral_case's, three standard normal columns)."""
import os

import numpy as np
import pytest

from dense_linear_app_amd import batched
from dense_linear_app_amd import chameleon as ch
from chol_testkit import assert_before_init_refused, assert_symbols_exported, bits
from potrf_batched_model import (FAMILIES, HOST_ORDERS, NRHS, SEEDS, dyadic_case, dyadic_rhs, factor_ratio,
                                 failing_case, padded_order, potrf_model, solve_model, solve_ratio, spectral_case)

SYMBOLS = ["chol_potrf_batched", "chol_potrs_batched", "chol_posv_batched", "chol_last_batched_stats"]
SOLVE_ARGS = (ch.ChamLower, ch.ChamRealDouble, 4, 1, None, 4, 16, None, 4, 4, 1, None)
ARGS = {"chol_potrf_batched": (ch.ChamLower, ch.ChamRealDouble, 4, None, 4, 16, 1, None),
        "chol_potrs_batched": SOLVE_ARGS, "chol_posv_batched": SOLVE_ARGS, "chol_last_batched_stats": (None,)}


def test_symbols_and_functions_exist():
    assert_symbols_exported(SYMBOLS)
    for name in ("potrf_batched", "potrs_batched", "posv_batched", "last_batched_stats"):
        assert callable(getattr(batched, name))


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    assert_before_init_refused(sym, ARGS[sym])


def test_wrapper_layout_rules_on_cpu_tensors():
    """the layout rules need no device: on CPU tensors they give the library's arguments or raise ValueError, and a
    CPU tensor with a good layout is refused as such -- all before any library call"""
    import torch

    L, U, f64 = ch.ChamLower, ch.ChamUpper, torch.float64
    # column-major and row-major images, and which triangle goes to the library
    cm = torch.empty(3, 4, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 4), strides (20, 1, 5)
    assert batched._images_of_A(cm, L) == (ch.ChamRealDouble, L, 4, 5, 20, 3)
    rm = torch.empty(3, 4, 6, dtype=torch.float32)[:, :, :4]  # strides (24, 6, 1)
    assert batched._images_of_A(rm, L) == (ch.ChamRealFloat, U, 4, 6, 24, 3)
    assert batched._images_of_A(rm, U)[1] == L
    one = torch.empty(4, 4, dtype=f64)
    assert batched._images_of_A(one, U) == (ch.ChamRealDouble, L, 4, 4, 16, 1)
    B1 = torch.empty(3, 4, dtype=f64)
    assert batched._images_of_B(cm, B1, ch.ChamRealDouble, 4, 3) == (1, 4, 4)
    Bc = torch.empty(3, 7, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 7), strides (35, 1, 5)
    assert batched._images_of_B(cm, Bc, ch.ChamRealDouble, 4, 3) == (7, 5, 35)

    for call in (lambda: batched.potrf_batched(cm), lambda: batched.potrs_batched(cm, B1),
                 lambda: batched.posv_batched(rm.double(), Bc, U)):
        with pytest.raises(ValueError, match="device tensors"):
            call()
    with pytest.raises(ValueError, match="torch tensor"):
        batched.potrf_batched(np.eye(4))
    with pytest.raises(ValueError, match="uplo"):
        batched.potrf_batched(one, 0)
    for bad in (torch.empty(3, 4, 8, dtype=f64)[:, :, ::2],  # neither stride is 1
                torch.empty(3, 4, 5, dtype=f64),  # not square
                torch.empty(4, dtype=f64),
                torch.empty(1, 4, 4, dtype=f64).expand(3, 4, 4),  # the matrices overlap
                torch.empty(3, 4, 4, dtype=torch.float16), torch.empty(3, 4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError) as e:
            batched.potrf_batched(bad)
        assert "device" not in str(e.value)
    with pytest.raises(ValueError, match="row-major"):
        batched.posv_batched(cm, torch.empty(3, 4, 7, dtype=f64))
    for bad in (torch.empty(3, 5, dtype=f64), torch.empty(2, 4, dtype=f64), torch.empty(3, 4, dtype=torch.float32),
                torch.empty(3, 8, dtype=f64)[:, ::2], torch.empty(3, 4, 2, 2, dtype=f64)):
        with pytest.raises(ValueError) as e:
            batched.potrs_batched(cm, bad)
        assert "device" not in str(e.value)


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_model_meets_the_bounds(n, dt):
    worst_f = worst_s = 0.0
    for seed in SEEDS:
        A, B = spectral_case(n, seed, dt)
        F, info = potrf_model(A, dt)
        assert info == 0 and F.dtype == A.dtype
        X, info = solve_model(F, B, dt)
        assert info == 0 and X.dtype == A.dtype
        worst_f = max(worst_f, factor_ratio(A, F, dt))
        worst_s = max(worst_s, solve_ratio(A, F, X, B, dt))
    print(f"n={n} {dt}: {worst_f:.2f} of the factor bound, {worst_s:.2f} of the solve bound")
    assert worst_f <= 1.0 and worst_s <= 1.0


@pytest.mark.parametrize("n", HOST_ORDERS)
@pytest.mark.parametrize("dt", ["d", "s"])
def test_model_is_exact_on_the_dyadic_family(n, dt):
    for family in FAMILIES:
        A, L, _ = dyadic_case(n, n, family, dt)
        F, info = potrf_model(A, dt)
        assert info == 0
        assert np.array_equal(bits(np.tril(F)), bits(L))
        for nrhs in NRHS:
            X, B = dyadic_rhs(n, nrhs, n, family, dt)
            Xm, info = solve_model(F, B, dt)
            assert info == 0
            assert np.array_equal(bits(Xm), bits(X)), (family, nrhs)


@pytest.mark.parametrize("dt", ["d", "s"])
def test_model_info_rules(dt):
    for n, j in ((1, 0), (9, 0), (9, 4), (33, 32), (64, 17)):
        for nan in (False, True):
            A, L, _ = dyadic_case(n, 5, "mod3", dt)
            F, info = potrf_model(failing_case(n, 5, "mod3", dt, j, nan), dt)
            assert info == j + 1
            assert np.array_equal(bits(np.tril(F)[:, :j]), bits(L[:, :j]))
        Z = np.array(L)
        Z[j, j] = 0
        B = dyadic_rhs(n, 3, 5, "mod3", dt)[1]
        X, info = solve_model(Z, B, dt)
        assert info == j + 1 and np.array_equal(bits(X), bits(B))
    assert [padded_order(n) for n in (1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]


def test_kernels_use_no_scratch():
    import codeobj

    so = os.path.join(os.path.dirname(os.path.abspath(ch.__file__)), "libcholmi.so")
    seen = 0
    for elf in codeobj.device_elfs(so):
        for name, res in codeobj.kernel_resources(so, elf).items():
            if "k_batched" in name:
                seen += 1
                assert res["scratch"] == 0, (name, res)
    assert seen == 48  # two precisions, four padded orders, two triangles, three modes
