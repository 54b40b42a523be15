#!/usr/bin/env python3
"""Timing of the rank-r update / downdate of a Cholesky factor against a new factorisation, in one process:
python scripts/chud_time.py [N tile [out]]   (default 65536 1024 profiles/chud_time_N<N>_B<tile>.txt)

fp64, Lower.  A is a plgsy matrix (bump N), F its factor.  Each figure is the median of REPS calls after a warm-up,
with the inputs restored on the device outside the timed region:
  lacpy + potrf   W <- A (everything), potrf(W): what a caller without chud does when A changes
  lacpy (Lower)   the stored triangle read once and written once: its time is the floor of one pass of chud, and
                  2 x bytes of the triangle over it the bandwidth that floor stands for
  chud / chdd     W <- F, V <- 0.1 x uniform(-1/2, 1/2) (so that A - V V^T stays positive definite), r = 1, 8, 32, with
                  the phases of chol_last_chud_stats
Every line goes to stdout and to `out`."""
import os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"chud_time_N{N}_B{B}.txt")
REPS = 3
RANKS = (1, 8, 32)
out = open(OUT, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def desc(cols):
    return ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, cols, 0, 0, N, cols, 1, 1)


def timed(fn, regen):
    regen()
    fn()  # warm-up (scratch allocation, first launches)
    ts = []
    for _ in range(REPS):
        regen()
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0, res))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


A, F, W = desc(N), desc(N), desc(N)
say(f"N={N} tile={B} dtype=fp64  (median of {REPS})")
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, A, F)
assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, F) == 0


def refactor():
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, A, W)
    return ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, W)


t_ref, info = timed(refactor, lambda: None)
assert info == 0
say(f"{'lacpy + potrf':24s}: {t_ref * 1e3:10.2f} ms")
t_cp, _ = timed(lambda: ch.CHAMELEON_dlacpy_Tile(ch.ChamLower, F, W), lambda: None)
tri_bytes = 8.0 * N * (N + B) / 2  # the stored triangle: whole diagonal tiles
say(f"{'lacpy (Lower): floor':24s}: {t_cp * 1e3:10.2f} ms  {2 * tri_bytes / t_cp / 1e12:6.2f} TB/s "
    f"(2 x {tri_bytes / 1e9:.2f} GB)")
rng = np.random.default_rng(7)
for name, fn in (("chud", ch.CHAMELEON_dchud_Tile), ("chdd", ch.CHAMELEON_dchdd_Tile)):
    for r in RANKS:
        Vh = np.asfortranarray(0.1 * (rng.random((N, r)) - 0.5))
        V = desc(r)

        def regen():
            ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, F, W)
            V.from_lapack(Vh)

        t, info = timed(lambda: fn(ch.ChamLower, W, V), regen)
        assert info == 0
        st = ch.last_chud_stats()
        say(f"{name + ' r=' + str(r):24s}: {t * 1e3:10.2f} ms  ({t_ref / t:7.1f} x faster than lacpy + potrf, "
            f"{t / (st['passes'] * t_cp):5.2f} x the floor of {st['passes']} pass{'es' if st['passes'] > 1 else ''})")
        say(f"{'  device total':24s}: {st['total_ms']:10.2f} ms")
        say(f"{'  chain':24s}: {st['chain_ms']:10.2f} ms  (generators, in-tile appliers)")
        say(f"{'  bulk appliers':24s}: {st['bulk_ms']:10.2f} ms")
        ch.CHAMELEON_Desc_Destroy(V)
out.close()
