"""CPU-side checks of the batched rank-r update and downdate of small factors (chol_chud_batched, chol_chdd_batched):
the ABI symbols and the Python functions exist, both entry points refuse to run before chol_init, the wrapper's layout
rules for V raise ValueError on CPU tensors before any library call, the numpy model of the arithmetic (chud_model.py)
meets the bounds of chud_batched_model.py on the shared inputs, running the vectors outside the columns gives the
model's bits and info, and the sixteen k_chud_rows kernels use no scratch.  The device numerics are in
test_gpu_chud_batched.py.

Measured with the model on the shared batches (chud_batched_model.py, r = 3, every order of ORDERS), in eps: fused
against plain fp32 2.42 (update) and 39.9 (downdate); against numpy's fp64 Cholesky 4.75 / 88.6 in fp64 and
2.25 / 47.2 in fp32.  The bounds are 10 x that."""
import os

import numpy as np
import pytest

from dense_linear_app_amd import batched
from dense_linear_app_amd import chameleon as ch
from chol_testkit import assert_before_init_refused, assert_symbols_exported, bits, npdt
from chud_batched_model import (LAPACK_BOUND, MODEL_BOUND, ORDERS, R, batch, batch_size, chud_model, err_eps,
                                fused_batch, problem)

SYMBOLS = ["chol_chud_batched", "chol_chdd_batched"]
ARGS = (ch.ChamLower, ch.ChamRealDouble, 4, 1, None, 4, 16, None, 4, 4, 1, None)


def test_symbols_and_functions_exist():
    assert_symbols_exported(SYMBOLS)
    for name in ("chud_batched", "chdd_batched"):
        assert callable(getattr(batched, name)) and name in batched.__all__


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    assert_before_init_refused(sym, ARGS)


def test_wrapper_layout_rules_for_v_on_cpu_tensors():
    """V follows B's rules: (batch, n) contiguous vectors or column-major (batch, n, r) images; a good layout on the
    CPU is refused as such, every bad one before that -- all before any library call"""
    import torch

    f64 = torch.float64
    A = torch.empty(3, 4, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 4), strides (20, 1, 5)
    v1 = torch.empty(3, 4, dtype=f64)
    assert batched._images_of_B(A, v1, ch.ChamRealDouble, 4, 3, "V") == (1, 4, 4)
    vc = torch.empty(3, 7, 5, dtype=f64).mT[:, :4, :]  # (3, 4, 7), strides (35, 1, 5)
    assert batched._images_of_B(A, vc, ch.ChamRealDouble, 4, 3, "V") == (7, 5, 35)
    for fn in (batched.chud_batched, batched.chdd_batched):
        for good in (v1, vc):
            with pytest.raises(ValueError, match="device tensors"):
                fn(A, good)
        with pytest.raises(ValueError, match="V is row-major"):
            fn(A, torch.empty(3, 4, 7, dtype=f64))
        with pytest.raises(ValueError, match="uplo"):
            fn(A, v1, 0)
        with pytest.raises(ValueError, match="torch tensor"):
            fn(A, np.zeros((3, 4)))
        for bad in (torch.empty(3, 5, dtype=f64), torch.empty(2, 4, dtype=f64), torch.empty(3, 4, dtype=torch.float32),
                    torch.empty(3, 8, dtype=f64)[:, ::2], torch.empty(3, 4, 2, 2, dtype=f64),
                    torch.empty(1, 4, 2, dtype=f64).mT.expand(3, 2, 4).mT):  # the images overlap
            with pytest.raises(ValueError) as e:
                fn(A, bad)
            assert "device" not in str(e.value) and "V" in str(e.value)
        with pytest.raises(ValueError):  # A's own rules come first
            fn(torch.empty(3, 4, 5, dtype=f64), v1)


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("sigma", [1, -1])
def test_model_meets_the_bounds(n, sigma):
    k = 0 if sigma > 0 else 1
    Lm = batch(n, sigma, "s")[2]
    ef = err_eps(fused_batch(n, sigma), Lm, "s")
    print(f"n={n} sigma={sigma}: fused against plain fp32 {ef:.2f} eps")
    assert ef <= MODEL_BOUND[k]
    for dt in "ds":
        start, V, Lm, ref = batch(n, sigma, dt)
        assert start.shape == (batch_size(n), n, n) and V.shape == (batch_size(n), n, R) and Lm.dtype == npdt(dt)
        el = err_eps(Lm, ref, dt)
        print(f"n={n} sigma={sigma} {dt}: the model against LAPACK {el:.2f} eps")
        assert el <= LAPACK_BOUND[dt][k]


def vectors_outer(L, V, sigma, dt):
    """the kernel's loop order with the model's operations: vectors outside, columns inside; a rotation that cannot be
    made is skipped (the identity); -> (info, L'), info the least first failing column over the vectors"""
    t = npdt(dt)
    L, V = np.tril(L).astype(t), np.array(V, dtype=t)
    n, r = V.shape
    sg, stop = t(sigma), 0
    for k in range(r):
        v = V[:, k]
        for j in range(n):
            ljj, vj = L[j, j], v[j]
            d2 = (sg * vj) * vj + ljj * ljj
            if not d2 > 0:
                stop = min(stop or j + 1, j + 1)
                continue
            rr = np.sqrt(d2)
            c, s, ci = rr / ljj, vj / ljj, ljj / rr
            L[j, j] = rr
            L[j + 1:, j] = ((sg * s) * v[j + 1:] + L[j + 1:, j]) * ci
            v[j + 1:] = c * v[j + 1:] - s * L[j + 1:, j]
    return stop, L


@pytest.mark.parametrize("dt", ["d", "s"])
def test_vectors_outer_gives_the_models_bits_and_info(dt):
    for n in (3, 9, 33):
        for sigma in (1, -1):
            start, V, Lm, _ = batch(n, sigma, dt, 5, 2)
            for b in range(2):
                info, L = vectors_outer(start[b], V[b], sigma, dt)
                assert info == 0 and np.array_equal(bits(L), bits(Lm[b])), (n, sigma, b)
    L = problem(33, 1, 77)[2].astype(npdt(dt))
    for cols, want in (((20, 4, 2), 3), ((2, 4, 20), 3), ((20, 4), 5), ((20,), 21)):
        scale = [0.999 if (len(cols) == 3 and c == 20) else 1.001 for c in cols]
        V = np.stack([f * L[:, c].astype(np.float64) for f, c in zip(scale, cols)], axis=1)
        with np.errstate(all="ignore"):
            assert chud_model(L, V, -1, npdt(dt))[0] == want
            assert vectors_outer(L, V, -1, dt)[0] == want, cols


def test_kernels_use_no_scratch():
    import codeobj

    so = os.path.join(os.path.dirname(os.path.abspath(ch.__file__)), "libcholmi.so")
    seen = 0
    for elf in codeobj.device_elfs(so):
        for name, res in codeobj.kernel_resources(so, elf).items():
            if "k_chud_rows" in name:
                seen += 1
                assert res["scratch"] == 0, (name, res)
                assert "k_batched" not in name
    assert seen == 16  # two precisions, four padded orders, two triangles
