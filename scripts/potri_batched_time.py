#!/usr/bin/env python3
"""Timing of the batched inverses (trtri_batched, potri_batched, poinv_batched, invdiag_batched) against the memory
floor, against potrf_batched, against what a caller had before them (potrs_batched on an identity block) and against
torch, in one process:
python scripts/potri_batched_time.py [GiB [out]]   (default 1.0 profiles/potri_batched_time.txt)

n in {4, 8, 16, 32, 48, 64} x {fp64, fp32} x {Lower, Upper}; `batch` such that the n x n images total GiB (far beyond
the caches).  The matrices are G G^T + n I, G uniform in (-1/2, 1/2), stored whole (lda = n, stride = n n); S keeps
them, F their factors in both triangles (potrf_batched), so Lower and Upper work on the same images.  The tensors are
row-major, so `uplo` is the caller's and the library gets the other code: the Lower rows run the kernels that read
rows (the library's Upper), the Upper rows those that read columns.  Every call works on the image W, restored from F
or S before it.  Every shape is warmed up, then each figure is the median of REPS calls, alternated with the
comparisons, the order of the calls rotated from one repetition to the next:
  copy    the device-to-device copy_ of the same images (torch events): n n elements read and written per matrix
  potrf   potrf_batched at the same shape
  solveI  potrs_batched with the identity as its n right-hand columns: the inverse a caller could have before, with a
          second operand of the images' size
  torch   torch.cholesky_inverse on the same factors (torch events).  It is first run on batch / 64 matrices; where that
          projects to more than 5 s for the whole batch the projection is printed, marked `~`, and the whole batch is
          not run
trtri, potri, poinv, invdiag, potrf and solveI: kernel time from the library's own events (chol_last_batched_stats).
/potrf: potri and poinv over potrf; /solveI and /torch: potri over them (< 1: potri is faster); /copy: potri over the
copy.  Every line goes to stdout and to `out`."""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import torch
from dense_linear_app_amd import batched as bt
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
GIB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "potri_batched_time.txt")
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
    fn()
    return bt.last_batched_stats()["kernel_ms"]


def torch_inverse_ms(Tm, upper):
    """-> (ms, mark): torch.cholesky_inverse of the whole batch, or `~` and the projection from batch / 64 matrices"""
    part = Tm[:max(1, Tm.shape[0] // 64)]
    torch_ms(lambda: torch.cholesky_inverse(part, upper=upper))  # warm-up
    t = torch_ms(lambda: torch.cholesky_inverse(part, upper=upper)) * Tm.shape[0] / part.shape[0]
    if t > 5000.0:
        return t, "~"
    torch_ms(lambda: torch.cholesky_inverse(Tm, upper=upper))
    return median([torch_ms(lambda: torch.cholesky_inverse(Tm, upper=upper)) for _ in range(TORCH_REPS)]), " "


say(f"images of {GIB} GiB per shape, median of {REPS} (torch: {TORCH_REPS}); times in ms, kernel time from the "
    "library's events; row-major tensors: uplo is the caller's, the library gets the other code")
say(f"{'n':>3} {'type':>4} {'uplo':>5} {'batch':>9} | {'copy':>7} {'potrf':>7} | {'trtri':>7} {'potri':>8} {'poinv':>8} "
    f"{'invdiag':>7} | {'potri':>6} {'poinv':>6} {'potri':>6} | {'solveI':>9} {'potri':>7} | {'torch':>10} {'potri':>7}")
say(f"{'':>3} {'':>4} {'':>5} {'':>9} | {'':>7} {'':>7} | {'':>7} {'':>8} {'':>8} {'':>7} | {'/potrf':>6} {'/potrf':>6} "
    f"{'/copy':>6} | {'':>9} {'/solveI':>7} | {'':>10} {'/torch':>7}")
for n in (4, 8, 16, 32, 48, 64):
    for dtype, name in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        es = 8 if dtype == torch.float64 else 4
        batch = int(GIB * 2 ** 30 / (n * n * es))
        G = torch.rand(batch, n, n, dtype=dtype, device="cuda") - 0.5
        S = torch.bmm(G, G.mT)
        del G
        S.diagonal(dim1=-2, dim2=-1).add_(float(n))
        F = S.clone()
        # F is row-major: Lower for the caller is the library's Upper.  Either way both triangles hold the factor
        assert not bt.potrf_batched(F, ch.ChamLower).any() and not bt.potrf_batched(F, ch.ChamUpper).any()
        W = torch.empty_like(F)
        E = torch.empty(batch, n, n, dtype=dtype, device="cuda").mT  # (column-major, as potrs_batched takes B)

        def identity():
            E.zero_()
            E.diagonal(dim1=-2, dim2=-1).fill_(1.0)

        torch.cuda.synchronize()
        for uplo, uname in ((ch.ChamLower, "Lower"), (ch.ChamUpper, "Upper")):
            calls = {"potrf": (S, lambda: bt.potrf_batched(W, uplo)),
                     "trtri": (F, lambda: bt.trtri_batched(W, uplo)),
                     "potri": (F, lambda: bt.potri_batched(W, uplo)),
                     "poinv": (S, lambda: bt.poinv_batched(W, uplo)),
                     "invdiag": (F, lambda: bt.invdiag_batched(W, uplo)),
                     "solveI": (F, lambda: bt.potrs_batched(W, E, uplo))}
            for src, fn in calls.values():  # warm-up of every path of this shape
                W.copy_(src)
                identity()
                info = fn()
                assert not (info[1] if isinstance(info, tuple) else info).any()
            t = {k: [] for k in calls}
            t_copy = []
            keys = list(calls)
            for rep in range(REPS):
                t_copy.append(torch_ms(lambda: W.copy_(F)))
                for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:  # (no call always follows the same one)
                    W.copy_(calls[k][0])
                    if k == "solveI":
                        identity()
                    torch.cuda.synchronize()
                    t[k].append(kernel_ms(calls[k][1]))
            m = {k: median(v) for k, v in t.items()}
            c = median(t_copy)
            try:
                t_t, mark = torch_inverse_ms(F, uplo == ch.ChamUpper)
                torch_cols = f"{t_t:9.2f}{mark} {m['potri'] / t_t:7.3f}"
            except Exception as e:  # (it does not run there: say so and go on)
                torch.cuda.synchronize()
                torch_cols = f"{'n/a':>10} {'n/a':>7}"
                say(f"# torch.cholesky_inverse n={n} {name} {uname}: {type(e).__name__}: {str(e)[:120]}")
            say(f"{n:3d} {name:>4} {uname:>5} {batch:9d} | {c:7.3f} {m['potrf']:7.3f} | {m['trtri']:7.3f} "
                f"{m['potri']:8.3f} {m['poinv']:8.3f} {m['invdiag']:7.3f} | {m['potri'] / m['potrf']:6.2f} "
                f"{m['poinv'] / m['potrf']:6.2f} {m['potri'] / c:6.2f} | {m['solveI']:9.3f} "
                f"{m['potri'] / m['solveI']:7.3f} | {torch_cols}")
            torch.cuda.empty_cache()
        del S, F, W, E
        torch.cuda.empty_cache()
out.close()
