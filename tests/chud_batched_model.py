"""The inputs that test_chud_batched_host.py and test_gpu_chud_batched.py share, for the batched rank-r update and
downdate of small factors (chol_chud_batched / chol_chdd_batched: include/cholmi.h).  The arithmetic is that of the
tile routine, so the model is chud_model.py's and the matrices are its problem(n, r, seed): A a Gram matrix with an
n x 2n standard normal factor, V standard normal times sqrt(n); the downdate starts from the factor of A + V V^T and
is compared with the factor of A.  The orders are potrf_batched_model.ORDERS (both sides of every packing boundary).

A batch holds 2 (64 / P) + 1 distinct matrices, P the padded order: several sub-groups of a wavefront, two full
wavefronts and a partly filled one.  Matrix b of the batch of order n is problem(n, r, 1000 n + b).

Errors are max |dL| / max |L| in eps (2^-52, 2^-23).  The bounds are 10 x what the model itself measures on exactly
these batches (r = 3, both signs; test_chud_batched_host.py prints the figures and holds the model to the bounds):

    against the model   what one fused multiply-add per a b + c can change: fp32 chud_model(fused=True) against plain
                        fp32: 2.42 eps (update), 39.9 eps (downdate, the 1 x 1 matrices, where the
                        difference of two squares cancels most); the same bounds in eps for both precisions
    against LAPACK      the plain model against numpy's fp64 Cholesky of A +- V V^T:
                        fp64 4.75 / 88.6 eps, fp32 2.25 / 47.2 eps (update / downdate)"""
import functools

import numpy as np

from chol_testkit import npdt
from chud_model import chud_model, problem
from potrf_batched_model import ORDERS, padded_order

R = 3
MODEL_BOUND = (24.2, 399.0)  # [update, downdate], eps of the dtype
LAPACK_BOUND = {"d": (47.5, 886.0), "s": (22.5, 472.0)}


def batch_size(n):
    return 2 * (64 // padded_order(n)) + 1


def err_eps(L, ref, dt):
    """max |L - ref| / max |ref| in eps of dt; stacks of matrices: the worst of them"""
    L, ref = np.asarray(L, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    L, ref = L.reshape((-1,) + L.shape[-2:]), ref.reshape((-1,) + ref.shape[-2:])
    return max(np.abs(l - f).max() / np.abs(f).max() for l, f in zip(L, ref)) / np.finfo(npdt(dt)).eps


@functools.lru_cache(maxsize=None)
def case(n, r, seed, sigma, dt):
    """-> (the Lower factor to start from and V, both rounded to dt; the model's result in dt; LAPACK's fp64 factor),
    read-only"""
    _, V, L0, L1 = problem(n, r, seed)
    start, ref = (L0, L1) if sigma > 0 else (L1, L0)
    start, V = start.astype(npdt(dt)), V.astype(npdt(dt))
    info, Lm, _ = chud_model(start, V, sigma, npdt(dt))
    assert info == 0
    out = (np.tril(start), V, Lm, np.array(ref))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch(n, sigma, dt, r=R, count=None):
    """-> (start, V, model, LAPACK) stacked over the batch_size(n) (or count) matrices of that order"""
    cases = [case(n, r, 1000 * n + b, sigma, dt) for b in range(count or batch_size(n))]
    out = tuple(np.stack([c[k] for c in cases]) for k in range(4))
    for a in out:
        a.setflags(write=False)
    return out


def fused_batch(n, sigma, r=R):
    """the fp32 model with every a b + c rounded once, on batch(n, sigma, "s")"""
    start, V, _, _ = batch(n, sigma, "s", r)
    return np.stack([chud_model(l, v, sigma, np.float32, fused=True)[1] for l, v in zip(start, V)])


__all__ = ["ORDERS", "R", "MODEL_BOUND", "LAPACK_BOUND", "batch_size", "err_eps", "case", "batch", "fused_batch",
           "chud_model", "problem", "padded_order"]
