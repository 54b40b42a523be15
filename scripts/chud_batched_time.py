#!/usr/bin/env python3
"""Timing of the batched rank-r update and downdate of small factors against the memory floor and against what a
caller had to do without them, in one process:
python scripts/chud_batched_time.py [GiB [out]]   (default 1.0 profiles/chud_batched_time.txt)

n in {4, 8, 16, 32, 48, 64} x {fp64, fp32} x {Lower, Upper} x r in {1, 4, 16}; `batch` such that the n x n images total
GiB (far beyond the caches).  The matrices are G G^T + n I, G uniform in (-1/2, 1/2), stored whole (lda = n, stride =
n n) and factored in place by potrf_batched; V is uniform in (-1/2, 1/2), column-major with ldv = n and stride 16 n,
its first r columns taken.  Every shape is warmed up, then each figure is the median of REPS calls, alternated:
  chud, chdd  the update and then the downdate with the same V, which returns the factor (up to rounding), so nothing
              has to be restored between the repetitions: kernel time from the library's own events
              (chol_last_batched_stats), GB/s of the bytes that must move (the stored triangles read and written, V
              read) and the ratio to the copy
  copy        the device-to-device copy_ of the same images (torch events): the memory floor of n n elements read and
              written per matrix
  refact      what a caller must do today: K.baddbmm_(V, V^T) into a kept copy K of the matrices, a copy_ of K into
              the work images (both by torch events) and potrf_batched of those (kernel time): the sum, and chud's
              time over it (< 1: chud is faster)
Every line goes to stdout and to `out`."""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import torch
from dense_linear_app_amd import batched as bt
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
GIB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "chud_batched_time.txt")
REPS = 5
RMAX = 16
out = open(OUT, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def median(xs):
    return sorted(xs)[len(xs) // 2]


def torch_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms(fn):
    info = fn()
    assert not info.any()
    return bt.last_batched_stats()["kernel_ms"], bt.last_batched_stats()["bytes"]


say(f"images of {GIB} GiB per shape, median of {REPS}; times in ms, chud / chdd / potrf: kernel time from the "
    "library's events; refact = baddbmm_ + copy_ + potrf_batched")
say(f"{'n':>3} {'type':>4} {'uplo':>5} {'r':>2} {'batch':>9} | {'copy':>8} | {'chud':>8} {'GB/s':>7} {'x copy':>7} | "
    f"{'chdd':>8} {'GB/s':>7} {'x copy':>7} | {'baddbmm':>8} {'potrf':>8} {'refact':>8} {'chud/ref':>8}")
for n in (4, 8, 16, 32, 48, 64):
    for dtype, name in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        es = 8 if dtype == torch.float64 else 4
        batch = int(GIB * 2 ** 30 / (n * n * es))
        G = torch.rand(batch, n, n, dtype=dtype, device="cuda") - 0.5
        A = torch.bmm(G, G.mT)
        del G
        A.diagonal(dim1=-2, dim2=-1).add_(float(n))
        W, K, W2 = torch.empty_like(A), torch.empty_like(A), torch.empty_like(A)
        Vall = (torch.rand(batch, RMAX, n, dtype=dtype, device="cuda") - 0.5).mT  # (batch, n, 16), column-major
        torch.cuda.synchronize()
        for uplo, uname in ((ch.ChamLower, "Lower"), (ch.ChamUpper, "Upper")):
            for r in (1, 4, 16):
                V = Vall[:, :, :r]
                W.copy_(A), K.copy_(A)
                assert not bt.potrf_batched(W, uplo).any()
                # warm-up of every path of this shape
                bt.chud_batched(W, V, uplo), bt.chdd_batched(W, V, uplo)
                K.baddbmm_(V, V.mT), W2.copy_(K), bt.potrf_batched(W2, uplo)
                t_copy, t_u, t_d, t_b, t_f = [], [], [], [], []
                for _ in range(REPS):
                    ms, by = kernel_ms(lambda: bt.chud_batched(W, V, uplo))
                    t_u.append(ms)
                    t_b.append(torch_ms(lambda: K.baddbmm_(V, V.mT)))
                    t_copy.append(torch_ms(lambda: W2.copy_(K)))
                    ms, _ = kernel_ms(lambda: bt.potrf_batched(W2, uplo))
                    t_f.append(ms)
                    ms, _ = kernel_ms(lambda: bt.chdd_batched(W, V, uplo))
                    t_d.append(ms)
                c, u, d, b, f = median(t_copy), median(t_u), median(t_d), median(t_b), median(t_f)
                ref = b + c + f
                say(f"{n:3d} {name:>4} {uname:>5} {r:2d} {batch:9d} | {c:8.3f} | {u:8.3f} {by / u / 1e6:7.0f} "
                    f"{u / c:7.2f} | {d:8.3f} {by / d / 1e6:7.0f} {d / c:7.2f} | {b:8.3f} {f:8.3f} {ref:8.3f} "
                    f"{u / ref:8.2f}")
        del A, W, K, W2, Vall
        torch.cuda.empty_cache()
out.close()
