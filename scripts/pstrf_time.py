#!/usr/bin/env python3
"""Timing of the pivoted Cholesky factorisation against potrf on one plgsy matrix, in one process:
python scripts/pstrf_time.py [N tile dtype]   (dtype: d or s; default 65536 1024 d)

potrf (Lower) and pstrf (Lower, default tol) on the same full-rank matrix, each the median of REPS calls with the input
regenerated on the device outside the timed region, and the phases of the last pstrf (chol_last_pstrf_stats): the pivot
steps (two launches per column: the choice and interchange, then the left-looking column), the deferred row
interchanges of the finished tile columns, the trailing updates.  The pivot steps' GB/s count the bytes of the
left-looking products, sum over columns j of (n - j) (j - k0) elements."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
ES = 8 if DT == "d" else 4
A = ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, N, 0, 0, N, N, 1, 1)


def timed(fn):
    fn()  # warm-up (scratch allocation, first launches)
    ts = []
    for _ in range(REPS):
        ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0, out))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


def gemv_bytes():
    tot = 0
    for k0 in range(0, N, B):
        m = min(B, N - k0)  # sum over t < m of (N - k0 - t) t
        tot += (N - k0) * m * (m - 1) // 2 - (m - 1) * m * (2 * m - 1) // 6
    return tot * ES


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}", flush=True)
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
t_potrf, info = timed(lambda: ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, A))
assert info == 0
print(f"{'potrf':24s}: {t_potrf * 1e3:10.1f} ms  {N ** 3 / 3 / t_potrf / 1e12:6.1f} TFLOP/s", flush=True)
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
t_pstrf, (info, piv, rank) = timed(lambda: ch.CHAMELEON_dpstrf_Tile(ch.ChamLower, A))
st = ch.last_pstrf_stats()
print(f"{'pstrf':24s}: {t_pstrf * 1e3:10.1f} ms  info={info} rank={rank}  ({t_pstrf / t_potrf:.2f} x potrf)", flush=True)
gb = gemv_bytes()
print(f"{'  device total':24s}: {st['total_ms']:10.1f} ms", flush=True)
print(f"{'  pivot steps':24s}: {st['steps_ms']:10.1f} ms  {st['steps']} steps, {st['steps_ms'] * 1e3 / max(st['steps'], 1):.2f} us "
      f"per step; products {gb / 1e12:.2f} TB -> {gb / (st['steps_ms'] * 1e-3) / 1e12:.2f} TB/s", flush=True)
print(f"{'  row interchanges':24s}: {st['laswp_ms']:10.1f} ms", flush=True)
print(f"{'  trailing updates':24s}: {st['update_ms']:10.1f} ms", flush=True)
