#!/usr/bin/env python3
"""Timing of the batched small-matrix Cholesky routines against the memory floor and against torch, in one process:
python scripts/potrf_batched_time.py [GiB [out]]   (default 1.0 profiles/potrf_batched_time.txt)

n in {4, 8, 16, 32, 48, 64} x {fp64, fp32} x {Lower, Upper}; `batch` such that the n x n images total GiB (far beyond
the caches); nrhs = 1 for the solves.  The matrices are G G^T + n I, G uniform in (-1/2, 1/2), stored whole (lda = n,
stride = n n), so Lower and Upper work on the same images.  Every shape is warmed up, then each figure is the median of
REPS calls, alternated with the two comparisons:
  copy    the device-to-device copy_ of the same images (torch events) -- it also restores the matrices before each
          factorisation: the memory floor (n n elements read and written per matrix)
  torch   torch.linalg.cholesky_ex on the same batch (torch events), where it runs; a call that takes seconds is
          timed once
potrf / potrs / posv: kernel time from the library's own events (chol_last_batched_stats), GB/s of the bytes the
algorithm must move (the stored triangles read and written, plus B), the ratio to the copy and, for potrf, to torch
(> 1: torch is faster).  Every line goes to stdout and to `out`."""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import torch
from dense_linear_app_amd import batched as bt
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
GIB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "potrf_batched_time.txt")
REPS = 5
TORCH_REPS = 3
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


say(f"images of {GIB} GiB per shape, nrhs = 1, median of {REPS} (torch: {TORCH_REPS}); times in ms, kernel time from "
    "the library's events")
say(f"{'n':>3} {'type':>4} {'uplo':>5} {'batch':>9} | {'copy':>8} | {'potrf':>8} {'GB/s':>7} {'x copy':>7} "
    f"{'torch':>9} {'x torch':>8} | {'potrs':>8} {'GB/s':>7} {'x copy':>7} | {'posv':>8} {'GB/s':>7} {'x copy':>7}")
for n in (4, 8, 16, 32, 48, 64):
    for dtype, name in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        es = 8 if dtype == torch.float64 else 4
        batch = int(GIB * 2 ** 30 / (n * n * es))
        G = torch.rand(batch, n, n, dtype=dtype, device="cuda") - 0.5
        A = torch.bmm(G, G.mT)
        del G
        A.diagonal(dim1=-2, dim2=-1).add_(float(n))
        W = torch.empty_like(A)
        B = torch.rand(batch, n, dtype=dtype, device="cuda")
        Bw = torch.empty_like(B)
        torch.cuda.synchronize()
        for uplo, uname in ((ch.ChamLower, "Lower"), (ch.ChamUpper, "Upper")):
            # warm-up of every path of this shape
            W.copy_(A), Bw.copy_(B)
            bt.potrf_batched(W, uplo), bt.potrs_batched(W, Bw, uplo)
            W.copy_(A), Bw.copy_(B)
            bt.posv_batched(W, Bw, uplo)
            t_copy, t_f, t_s, t_v = [], [], [], []
            for _ in range(REPS):
                t_copy.append(torch_ms(lambda: W.copy_(A)))
                Bw.copy_(B)
                ms, by_f = kernel_ms(lambda: bt.potrf_batched(W, uplo))
                t_f.append(ms)
                ms, by_s = kernel_ms(lambda: bt.potrs_batched(W, Bw, uplo))
                t_s.append(ms)
                t_copy.append(torch_ms(lambda: W.copy_(A)))
                Bw.copy_(B)
                ms, by_v = kernel_ms(lambda: bt.posv_batched(W, Bw, uplo))
                t_v.append(ms)
            try:
                upper = uplo == ch.ChamUpper
                t_t = torch_ms(lambda: torch.linalg.cholesky_ex(A, upper=upper))  # warm-up
                if t_t < 2000.0:  # (a call of seconds is timed once: its first call)
                    t_t = median([torch_ms(lambda: torch.linalg.cholesky_ex(A, upper=upper))
                                  for _ in range(TORCH_REPS)])
                torch_cols = f"{t_t:9.2f} {median(t_f) / t_t:8.2f}"
            except Exception as e:  # (it does not run there: say so and go on)
                torch.cuda.synchronize()
                torch_cols = f"{'n/a':>9} {'n/a':>8}"
                say(f"# torch.linalg.cholesky_ex n={n} {name} {uname}: {type(e).__name__}: {str(e)[:120]}")
            c, f, s, v = median(t_copy), median(t_f), median(t_s), median(t_v)
            say(f"{n:3d} {name:>4} {uname:>5} {batch:9d} | {c:8.3f} | {f:8.3f} {by_f / f / 1e6:7.0f} {f / c:7.2f} "
                f"{torch_cols} | {s:8.3f} {by_s / s / 1e6:7.0f} {s / c:7.2f} | {v:8.3f} {by_v / v / 1e6:7.0f} "
                f"{v / c:7.2f}")
        del A, W, B, Bw
        torch.cuda.empty_cache()
out.close()
