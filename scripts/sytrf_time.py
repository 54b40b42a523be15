#!/usr/bin/env python3
"""Timing of the L D L^T factorisation without pivoting against potrf, in one process:
python scripts/sytrf_time.py [N tile dtype [nrhs]]   (dtype: d or s; default 65536 1024 d)

potrf (Lower) and sytrf_nopiv (Lower) of the same plgsy matrix, each the median of REPS calls after a warm-up, with the
input regenerated on the device outside the timed region, and the phases and magnitudes of the last sytrf_nopiv
(chol_last_sytrf_stats).  The matrix is the library's device-generated SPD matrix: without pivoting no launch depends
on the data, so the time is that of a quasi-definite matrix of the same order.  Both count N^3 / 3 flops; the updates
tile m^2 for a step whose trailing order is m.  With nrhs values: potrs and sytrs_nopiv on that many columns (the
right-hand sides are whatever the image holds: only the time is read)."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
NRHS = [int(a) for a in sys.argv[4:]]
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
A = ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, N, 0, 0, N, N, 1, 1)


def timed(fn, regen):
    regen()
    fn()  # warm-up (scratch allocation, first launches)
    ts = []
    for _ in range(REPS):
        regen()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0, out))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


def regen():
    ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}", flush=True)
t_potrf, info = timed(lambda: ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, A), regen)
assert info == 0
print(f"{'potrf':24s}: {t_potrf * 1e3:10.1f} ms  {N ** 3 / 3 / t_potrf / 1e12:6.1f} TFLOP/s", flush=True)
rhs = {}
for nrhs in NRHS:
    X = ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, nrhs, 0, 0, N, nrhs, 1, 1)
    rhs[nrhs] = X
    t, info = timed(lambda: ch.CHAMELEON_dpotrs_Tile(ch.ChamLower, A, X),
                    lambda: None)
    print(f"{'potrs nrhs=' + str(nrhs):24s}: {t * 1e3:10.1f} ms", flush=True)
t_sytrf, info = timed(lambda: ch.CHAMELEON_dsytrf_nopiv_Tile(ch.ChamLower, A), regen)
assert info == 0
st = ch.last_sytrf_stats()
print(f"{'sytrf_nopiv':24s}: {t_sytrf * 1e3:10.1f} ms  {N ** 3 / 3 / t_sytrf / 1e12:6.1f} TFLOP/s  "
      f"({t_sytrf / t_potrf:.2f} x potrf)", flush=True)
nt = -(-N // B)
upd = sum(1.0 * B * (N - (k + 1) * B) ** 2 for k in range(nt - 1))
print(f"{'  device total':24s}: {st['total_ms']:10.1f} ms", flush=True)
print(f"{'  chain':24s}: {st['chain_ms']:10.1f} ms  (diagonal tiles, panel TRSM, scaling)", flush=True)
print(f"{'  trailing updates':24s}: {st['update_ms']:10.1f} ms  {upd / (st['update_ms'] * 1e-3) / 1e12:6.1f} TFLOP/s",
      flush=True)
print(f"{'  inertia':24s}: {st['inertia']}  min|d| {st['min_abs_d']:.3g}  max|d| {st['max_abs_d']:.3g}  "
      f"max|L| {st['max_abs_l']:.3g}", flush=True)
for nrhs, X in rhs.items():
    t, info = timed(lambda: ch.CHAMELEON_dsytrs_nopiv_Tile(ch.ChamLower, A, X), lambda: None)
    assert info == 0
    print(f"{'sytrs_nopiv nrhs=' + str(nrhs):24s}: {t * 1e3:10.1f} ms", flush=True)
