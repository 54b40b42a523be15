#!/usr/bin/env python3
"""Timing of the inverse from the factor on one plgsy matrix, in one process:
python scripts/potri_time.py [N tile dtype]   (dtype: d or s; default 32768 1024 d)

potrf, trtri (Lower, on the factor), lauum (Lower, on the factor: the kernel potri's second half runs) and potri
(trtri + lauum), each a warm-up call and then the median of REPS calls.  The input of every call is restored outside
the timed region (plgsy for potrf, a lacpy of the factor for the others).  TFLOP/s count N^3/3 for potrf, trtri and
lauum each and 2 N^3/3 for potri."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (32768, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat


def desc():
    return ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, N, 0, 0, N, N, 1, 1)


A, F = desc(), desc()


def timed(prep, fn):
    prep()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(name, prep, fn, flops):
    timed(prep, fn)  # warm-up (scratch allocation, first launches)
    runs = [timed(prep, fn) for _ in range(REPS)]
    assert all(o == 0 for _, o in runs), [o for _, o in runs]
    ts = sorted(t for t, _ in runs)
    med = ts[REPS // 2]
    print(f"{name:6s}: median {med * 1e3:9.1f} ms  (min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f})  "
          f"{flops / med / 1e12:6.2f} TFLOP/s", flush=True)
    return med


def plgsy():
    ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)


def factor():
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, F, A)


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}", flush=True)
n3 = float(N) ** 3 / 3.0
run("potrf", plgsy, lambda: ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, A), n3)
st = ch.last_potrf_stats()
if st["update_ms"] > 0:
    print(f"        (its trailing updates: {st['update_flops'] / (st['update_ms'] * 1e-3) / 1e12:.2f} TFLOP/s over "
          f"{st['update_ms']:.1f} ms)", flush=True)
plgsy()
assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, A) == 0
ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, A, F)
run("trtri", factor, lambda: ch.CHAMELEON_dtrtri_Tile(ch.ChamLower, ch.ChamNonUnit, A), n3)
run("lauum", factor, lambda: ch.CHAMELEON_dlauum_Tile(ch.ChamLower, A), n3)
run("potri", factor, lambda: ch.CHAMELEON_dpotri_Tile(ch.ChamLower, A), 2 * n3)
