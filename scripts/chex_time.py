#!/usr/bin/env python3
"""Timing of the circular shift of a Cholesky factor's variables against a new factorisation, in one process:
python scripts/chex_time.py [N tile [out]]   (default 65536 1024 profiles/chex_time_N<N>_B<tile>.txt)

fp64, Lower.  A is a plgsy matrix (bump N), F its factor.  Each figure is the median of REPS calls after a warm-up,
with the factor restored on the device outside the timed region:
  lacpy + potrf   W <- A (everything), potrf(W): what a caller without chex does when the order changes (the
                  permutation of A itself not counted)
  lacpy (Lower)   the stored triangle read once and written once: the copy floor
  chud r=1        W <- F, one vector 0.1 x uniform(-1/2, 1/2): job 2 is this on a window, plus the data movement
  chex            W <- F, jobs 1 and 2 on the windows (1, N), (N/2, N) and one tile column (N/2+1, N/2+tile), with the
                  phases of chol_last_chex_stats; `window floor`: the copy floor scaled to the window's share of the
                  stored triangle (the columns k..l of the rows >= k)
Every line goes to stdout and to `out`."""
import os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"chex_time_N{N}_B{B}.txt")
REPS = 3
WINDOWS = ((1, N), (N // 2, N), (N // 2 + 1, N // 2 + B))
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


def restore():
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, F, W)


t_ref, info = timed(refactor, lambda: None)
assert info == 0
say(f"{'lacpy + potrf':24s}: {t_ref * 1e3:10.2f} ms")
t_cp, _ = timed(lambda: ch.CHAMELEON_dlacpy_Tile(ch.ChamLower, F, W), lambda: None)
tri_bytes = 8.0 * N * (N + B) / 2  # the stored triangle: whole diagonal tiles
say(f"{'lacpy (Lower): floor':24s}: {t_cp * 1e3:10.2f} ms  {2 * tri_bytes / t_cp / 1e12:6.2f} TB/s "
    f"(2 x {tri_bytes / 1e9:.2f} GB)")
V = desc(1)
Vh = np.asfortranarray(0.1 * (np.random.default_rng(7).random((N, 1)) - 0.5))


def regen_chud():
    restore()
    V.from_lapack(Vh)


t_ud, info = timed(lambda: ch.CHAMELEON_dchud_Tile(ch.ChamLower, W, V), regen_chud)
assert info == 0
say(f"{'chud r=1':24s}: {t_ud * 1e3:10.2f} ms  ({t_ref / t_ud:7.1f} x faster than lacpy + potrf)")
for k, l in WINDOWS:
    share = ((N - k + 1.0) ** 2 - (N - l) ** 2) / (float(N) * N)  # of the triangle's entries
    for job in (1, 2):
        t, info = timed(lambda: ch.CHAMELEON_dchex_Tile(ch.ChamLower, W, k, l, job), restore)
        assert info == 0
        st = ch.last_chex_stats()
        assert st["job"] == job and st["l_minus_k"] == l - k
        say(f"{f'chex job {job} ({k}, {l})':24s}: {t * 1e3:10.2f} ms  ({t_ref / t:7.1f} x faster than lacpy + potrf, "
            f"{t / (share * t_cp):5.2f} x the window floor of {share * t_cp * 1e3:.2f} ms)")
        say(f"{'  device total':24s}: {st['total_ms']:10.2f} ms")
        say(f"{'  data movement':24s}: {st['move_ms']:10.2f} ms  (staging copies, plain moves)")
        say(f"{'  chain':24s}: {st['chain_ms']:10.2f} ms  "
            f"({'the coefficient chain' if job == 1 else 'generators, in-tile appliers'})")
        say(f"{'  bulk appliers':24s}: {st['bulk_ms']:10.2f} ms")
out.close()
