#!/usr/bin/env python3
"""Timing of the generalized eigenproblem reduction against potrf, in one process:
python scripts/sygst_time.py [N tile dtype]   (dtype: d or s; default 65536 1024 d)

potrf (Lower) of a plgsy matrix B, then sygst (itype 1, Lower) of a second plgsy matrix A with that factor, each the
median of REPS calls after a warm-up, with the input regenerated on the device outside the timed region, and the
phases of the last sygst (chol_last_sygst_stats).  Rates: sygst counts N^3 flops; the rank-2k updates 2 tile m^2 for a
step whose trailing order is m; the deferred solve the tile products of its NN sums, sum over rows m of m (m - 1) / 2
products of 2 tile^3, plus its (triangular) diagonal-tile products, m tile^3 per row."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
A = ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, N, 0, 0, N, N, 1, 1)
F = ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, N, 0, 0, N, N, 1, 1)


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


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}", flush=True)
t_potrf, info = timed(lambda: ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, F),
                      lambda: ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, F, 42))
assert info == 0  # F holds the factor of the last call
print(f"{'potrf':24s}: {t_potrf * 1e3:10.1f} ms  {N ** 3 / 3 / t_potrf / 1e12:6.1f} TFLOP/s", flush=True)
t_sygst, info = timed(lambda: ch.CHAMELEON_dsygst_Tile(1, ch.ChamLower, A, F),
                      lambda: ch.CHAMELEON_dplgsy_Tile(0.0, ch.ChamUpperLower, A, 7))
assert info == 0
st = ch.last_sygst_stats()
print(f"{'sygst':24s}: {t_sygst * 1e3:10.1f} ms  {N ** 3 / t_sygst / 1e12:6.1f} TFLOP/s  ({t_sygst / t_potrf:.2f} x potrf)",
      flush=True)
nt = -(-N // B)
syr2k = sum(2.0 * B * (N - (k + 1) * B) ** 2 for k in range(nt - 1))
solve = sum(m * (m - 1) / 2 * 2.0 * B ** 3 + m * B ** 3 for m in range(1, nt))
print(f"{'  device total':24s}: {st['total_ms']:10.1f} ms  {st['steps']} steps", flush=True)
print(f"{'  diagonal-tile inverses':24s}: {st['diag_inv_ms']:10.1f} ms", flush=True)
print(f"{'  chain':24s}: {st['chain_ms']:10.1f} ms  (diagonal tiles, panel TRSM, two SYMMs)", flush=True)
print(f"{'  rank-2k updates':24s}: {st['syr2k_ms']:10.1f} ms  {syr2k / (st['syr2k_ms'] * 1e-3) / 1e12:6.1f} TFLOP/s",
      flush=True)
print(f"{'  deferred solve':24s}: {st['solve_ms']:10.1f} ms  {solve / (st['solve_ms'] * 1e-3) / 1e12:6.1f} TFLOP/s",
      flush=True)
