#!/usr/bin/env python3
"""Timing of the butterfly-randomised factorisation and solve against sytrf_nopiv, in one process:
timeout -k 10 900 python scripts/rbt_time.py [N tile dtype]   (dtype: d or s; default 65536 1024 d)

The yardstick is chol_sytrf_nopiv_tile in the SAME process (its kernels are untouched by the butterfly routines).
sytrf_nopiv and sytrf_rbt (depth 2, W from a seed) of the same plgsy matrix, Lower, each the median of REPS calls after a
warm-up, the input regenerated on the device outside the timed region; the transformation alone (rbt_apply with depth
1: level 0; depth 2 minus depth 1: level 1) with the rate at which each level moves the stored triangle (read once and
written once: 2 x n (n + 1) / 2 elements); and, fp64, sysv_rbt with one right-hand side with its phases
(chol_last_rbt_stats).  The matrix is the library's device-generated SPD matrix: without pivoting no launch depends on
the data, and W^T A W of an SPD matrix is SPD, so the time is that of an indefinite matrix of the same order while the
refinement stops after the first residual.  One process, no retries: run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
esize = 8 if DT == "d" else 4


def desc(ncols):
    return ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, ncols, 0, 0, N, ncols, 1, 1)


A, W = desc(N), desc(2)


def timed(fn, regen):
    regen()
    fn()  # warm-up (scratch allocation, first launches)
    ts = []
    for _ in range(REPS):
        regen()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0, out, ch.last_rbt_stats()))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


def regen():
    ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}", flush=True)
t_nopiv, info, _ = timed(lambda: ch.CHAMELEON_dsytrf_nopiv_Tile(ch.ChamLower, A), regen)
assert info == 0
print(f"{'sytrf_nopiv':24s}: {t_nopiv * 1e3:10.1f} ms  {N ** 3 / 3 / t_nopiv / 1e12:6.1f} TFLOP/s", flush=True)
t_rbt, info, rs = timed(lambda: ch.CHAMELEON_dsytrf_rbt_Tile(ch.ChamLower, A, W, 2, 7), regen)
assert info == 0
st = ch.last_sytrf_stats()
ratio = t_rbt / t_nopiv
print(f"{'sytrf_rbt depth 2':24s}: {t_rbt * 1e3:10.1f} ms  ({ratio:.3f} x sytrf_nopiv; goal <= 1.05 at 65536 / 1024 "
      f"fp64: {'met' if ratio <= 1.05 else 'NOT met'})", flush=True)
print(f"{'  W from the seed':24s}: {rs['gen_ms']:10.1f} ms", flush=True)
print(f"{'  transformation':24s}: {rs['transform_ms']:10.1f} ms", flush=True)
print(f"{'  factorisation':24s}: {rs['factor_ms']:10.1f} ms", flush=True)
print(f"{'  inertia':24s}: {st['inertia']}  max|L| {st['max_abs_l']:.3g}", flush=True)
tri = 2.0 * N * (N + 1) / 2 * esize
t1, _, _ = timed(lambda: ch.CHAMELEON_drbt_apply_Tile(ch.ChamLower, A, W, 1), regen)
t2, _, _ = timed(lambda: ch.CHAMELEON_drbt_apply_Tile(ch.ChamLower, A, W, 2), regen)
print(f"{'rbt_apply level 0':24s}: {t1 * 1e3:10.2f} ms  {tri / t1 / 1e12:6.2f} TB/s", flush=True)
print(f"{'rbt_apply level 1':24s}: {(t2 - t1) * 1e3:10.2f} ms  {tri / max(t2 - t1, 1e-9) / 1e12:6.2f} TB/s  (depth 2 minus "
      f"depth 1; depth 2: {t2 * 1e3:.2f} ms)", flush=True)
if DT == "d":
    AF, Bd, X = desc(N), desc(1), desc(1)
    import numpy as np

    Bd.from_lapack(np.asfortranarray(np.random.default_rng(1).standard_normal((N, 1))))
    regen()
    t, (info, it, berr), rs = timed(lambda: ch.CHAMELEON_dsysv_rbt_Tile(ch.ChamLower, A, AF, W, 2, 7, Bd, X), lambda: None)
    assert info == 0
    print(f"{'sysv_rbt nrhs=1':24s}: {t * 1e3:10.1f} ms  steps {it}  berr {berr[0] / 2.0 ** -53:.3g} u", flush=True)
    tot = rs["total_ms"]
    for k, what in (("gen_ms", "W from the seed"), ("transform_ms", "transformation"), ("factor_ms", "factorisation"),
                    ("solve_ms", "solves"), ("resid_ms", "residual passes + norm"), ("vec_ms", "vector butterflies")):
        print(f"{'  ' + what:24s}: {rs[k]:10.1f} ms  {100 * rs[k] / tot:5.1f} %", flush=True)
