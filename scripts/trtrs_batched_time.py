#!/usr/bin/env python3
"""Timing of the batched half routines (trtrs_batched, trmm_batched, logdet_batched) against the memory floor, against
potrs_batched and against torch, in one process:
python scripts/trtrs_batched_time.py [GiB [out]]   (default 1.0 profiles/trtrs_batched_time.txt)

n in {4, 8, 16, 32, 48, 64} x {fp64, fp32} x {Lower, Upper} x nrhs in {1, 8}; `batch` such that the n x n images total
GiB (far beyond the caches).  The matrices are G G^T + n I, G uniform in (-1/2, 1/2), stored whole (lda = n, stride =
n n) and factored once in both triangles by potrf_batched, so Lower and Upper work on the same images; B is uniform in
(0, 1) and restored before every call.  The tensors are row-major, so `uplo` is the caller's and the library gets the
other code: the Lower rows run the kernels that read rows (the library's Upper), the Upper rows those that read
columns.  Every shape is warmed up, then each figure is the median of REPS calls, alternated with the comparisons, the
order of the calls rotated from one repetition to the next:
  copy    the device-to-device copy_ of the same images (torch events): n n elements read and written per matrix
  potrs   potrs_batched at the same shape (kernel time from the library's events); `spread` is max - min of its REPS
          calls, the run-to-run spread a half solve may exceed it by
  torch   torch.linalg.solve_triangular with the forward half on the same factors (torch events), where it runs; a
          call that takes seconds is timed once.  logdet: torch.diagonal(F).log().sum(-1) (float64 for both dtypes)
fwd / bwd: the forward (op(T) = L) and backward (L^T) trtrs, mfwd / mbwd the two trmm: kernel time from the library's
own events (chol_last_batched_stats).  x potrs: the slower half solve over potrs (a `!` where it exceeds potrs by more
than the spread); x copy and x torch: the forward solve over the copy and over torch (< 1: faster than torch).  logdet
has no nrhs; it is printed with the nrhs = 1 rows.  Every line goes to stdout and to `out`."""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import torch
from dense_linear_app_amd import batched as bt
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
GIB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "trtrs_batched_time.txt")
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


def torch_median(fn):
    t = torch_ms(fn)  # warm-up
    if t < 2000.0:  # (a call of seconds is timed once: its first call)
        t = median([torch_ms(fn) for _ in range(TORCH_REPS)])
    return t


say(f"images of {GIB} GiB per shape, median of {REPS} (torch: {TORCH_REPS}); times in ms, kernel time from the "
    "library's events; row-major tensors: uplo is the caller's, the library gets the other code")
say(f"{'n':>3} {'type':>4} {'uplo':>5} {'nrhs':>4} {'batch':>9} | {'copy':>7} | {'potrs':>7} {'spread':>6} | "
    f"{'fwd':>7} {'bwd':>7} {'x potrs':>8} {'x copy':>6} {'torch':>9} {'x torch':>7} | {'mfwd':>7} {'mbwd':>7} | "
    f"{'logdet':>7} {'torch':>7} {'x torch':>7}")
N, T = ch.ChamNoTrans, ch.ChamTrans
for n in (4, 8, 16, 32, 48, 64):
    for dtype, name in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        es = 8 if dtype == torch.float64 else 4
        batch = int(GIB * 2 ** 30 / (n * n * es))
        G = torch.rand(batch, n, n, dtype=dtype, device="cuda") - 0.5
        F = torch.bmm(G, G.mT)
        del G
        F.diagonal(dim1=-2, dim2=-1).add_(float(n))
        # F is row-major: Lower for the caller is the library's Upper.  Either way both triangles hold the factor
        assert not bt.potrf_batched(F, ch.ChamLower).any() and not bt.potrf_batched(F, ch.ChamUpper).any()
        W = torch.empty_like(F)
        torch.cuda.synchronize()
        for uplo, uname in ((ch.ChamLower, "Lower"), (ch.ChamUpper, "Upper")):
            fwd, bwd = (N, T) if uplo == ch.ChamLower else (T, N)
            for nrhs in (1, 8):
                B = (torch.rand(batch, n, dtype=dtype, device="cuda") if nrhs == 1 else
                     torch.rand(batch, nrhs, n, dtype=dtype, device="cuda").mT)
                Bw = torch.empty_like(B) if nrhs == 1 else torch.empty(batch, nrhs, n, dtype=dtype, device="cuda").mT
                calls = {"potrs": lambda: bt.potrs_batched(F, Bw, uplo),
                         "fwd": lambda: bt.trtrs_batched(F, Bw, uplo, fwd),
                         "bwd": lambda: bt.trtrs_batched(F, Bw, uplo, bwd),
                         "mfwd": lambda: bt.trmm_batched(F, Bw, uplo, fwd),
                         "mbwd": lambda: bt.trmm_batched(F, Bw, uplo, bwd),
                         "logdet": lambda: bt.logdet_batched(F)}
                for fn in calls.values():  # warm-up of every path of this shape
                    Bw.copy_(B)
                    fn()
                t = {k: [] for k in calls}
                t_copy = []
                keys = list(calls)
                for rep in range(REPS):
                    t_copy.append(torch_ms(lambda: W.copy_(F)))
                    for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:  # (no call always follows the same one)
                        Bw.copy_(B)
                        torch.cuda.synchronize()
                        t[k].append(kernel_ms(calls[k]))
                m = {k: median(v) for k, v in t.items()}
                spread = max(t["potrs"]) - min(t["potrs"])
                try:
                    # the mathematical matrix's `uplo` triangle; the forward half is T itself (Lower) or T^T (Upper)
                    Tm = F if uplo == ch.ChamLower else F.mT
                    Bt = B if nrhs > 1 else B.unsqueeze(-1)
                    t_t = torch_median(lambda: torch.linalg.solve_triangular(Tm, Bt, upper=False))
                    torch_cols = f"{t_t:9.2f} {m['fwd'] / t_t:7.2f}"
                except Exception as e:  # (it does not run there: say so and go on)
                    torch.cuda.synchronize()
                    torch_cols = f"{'n/a':>9} {'n/a':>7}"
                    say(f"# torch.linalg.solve_triangular n={n} {name} {uname} nrhs={nrhs}: {type(e).__name__}: "
                        f"{str(e)[:120]}")
                if nrhs == 1:
                    t_l = torch_median(lambda: torch.diagonal(F, dim1=-2, dim2=-1).double().log().sum(-1).mul_(2.0))
                    logdet_cols = f"{m['logdet']:7.3f} {t_l:7.3f} {m['logdet'] / t_l:7.2f}"
                else:
                    logdet_cols = f"{'':>7} {'':>7} {'':>7}"
                half = max(m["fwd"], m["bwd"])
                mark = "!" if half > m["potrs"] + spread else " "
                c = median(t_copy)
                say(f"{n:3d} {name:>4} {uname:>5} {nrhs:4d} {batch:9d} | {c:7.3f} | {m['potrs']:7.3f} {spread:6.3f} | "
                    f"{m['fwd']:7.3f} {m['bwd']:7.3f} {half / m['potrs']:7.2f}{mark} {m['fwd'] / c:6.2f} {torch_cols} "
                    f"| {m['mfwd']:7.3f} {m['mbwd']:7.3f} | {logdet_cols}")
                del B, Bw
        del F, W
        torch.cuda.empty_cache()
out.close()
