#!/usr/bin/env python3
"""Timing of the symmetric product from one stored triangle beside the residual pass it may replace, in one process:
python scripts/symm_time.py [N tile [out]]   (default 65536 1024 profiles/symm_time_N<N>_B<tile>.txt)

fp64, Lower.  A is a plgsy matrix (bump N), B standard normal, C <- -A B + C (the residual's scalars).  symm: the median
of REPS calls after a warm-up, from the device events that the library records on its own stream
(chol_last_symm_stats).  The yardsticks, from the same process:
  lacpy (Lower)     the stored triangle read once and written once: the copy floor (wall time of the synchronous call)
  residual pass     chol_bench_refine path 0 at the same nrhs: the vector kernel of chol_porfs_tile, 8 columns per
                    launch, the stored triangle read once per launch (the fastest of REPS, its own events)
  crossover         the same pair at nrhs = 16, 24, 32, 48
  update kernel     chol_bench_update at wave 0: the TFLOP/s of the trailing update on this box
Every line goes to stdout and to `out`."""
import os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"symm_time_N{N}_B{B}.txt")
REPS = 3
NRHS = (1, 8, 64, 128, 1024)
CROSS = (16, 24, 32, 48)  # between 8 and 64: where symm overtakes the residual pass
L = ch.ChamLower
out = open(OUT, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def desc(cols):
    return ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, cols, 0, 0, N, cols, 1, 1)


def median(fn):
    """fn() -> ms (or None: the wall time of the call)"""
    ts = []
    for r in range(REPS + 1):
        t0 = time.perf_counter()
        v = fn()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3 if v is None else v)
    return sorted(ts)[REPS // 2]


A = desc(N)
say(f"N={N} tile={B} dtype=fp64 Lower  (median of {REPS})")
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
W = desc(N)
def copy_once():
    ch.CHAMELEON_dlacpy_Tile(L, A, W)  # (-> None: timed by the wall clock)


t_cp = median(copy_once)
ch.CHAMELEON_Desc_Destroy(W)
tri_bytes = 8.0 * N * (N + B) / 2  # the stored triangle: whole diagonal tiles
say(f"{'lacpy (Lower): floor':26s}: {t_cp:10.2f} ms  {2 * tri_bytes / t_cp / 1e9:6.2f} TB/s (2 x {tri_bytes / 1e9:.2f} GB)")

rng = np.random.default_rng(1)
rows = {}
for k in sorted(set(NRHS) | set(CROSS)):
    Bd, Cd = desc(k), desc(k)
    Bd.from_lapack(np.asfortranarray(rng.standard_normal((N, k))))
    Cd.from_lapack(np.asfortranarray(rng.standard_normal((N, k))))
    keep = {}

    def one():
        assert ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, L, -1.0, A, Bd, 1.0, Cd) == 0
        keep["st"] = ch.last_symm_stats()
        return keep["st"]["kernel_ms"]

    t = median(one)
    st = keep["st"]
    t_res = ch.bench_refine(L, A, A, Bd, 0, REPS)
    rows[k] = (t, t_res, st["flops"] / t / 1e9)
    say(f"{'symm nrhs=' + str(k):26s}: {t:10.2f} ms  {st['flops'] / t / 1e9:6.2f} TFLOP/s  ({st['workgroups']} workgroups of "
        f"128 x {st['block_cols']}; {t / t_cp:.2f} x the floor)   residual pass {t_res:10.2f} ms = {t_res / t:.2f} x symm")
    ch.CHAMELEON_Desc_Destroy(Bd)
    ch.CHAMELEON_Desc_Destroy(Cd)

ms, tf = ch.bench_update(A, 0, 0, REPS)  # (modifies A: last)
say(f"{'update kernel, wave 0':26s}: {ms:10.2f} ms  {tf:6.2f} TFLOP/s   symm at nrhs={NRHS[-1]} reaches {rows[NRHS[-1]][2] / tf:.2f} of it")
ks = sorted(rows)
lost = [k for k in ks if rows[k][0] >= rows[k][1]]
first = next((k for k in ks if not lost or k > lost[-1]), None)
say(f"symm is faster than the residual pass from nrhs = {first} on (of {ks}); slower or equal at {lost}")
out.close()
