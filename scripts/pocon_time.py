#!/usr/bin/env python3
"""Timing of the condition estimate on one plgsy matrix, in one process:
python scripts/pocon_time.py [N tile dtype]   (dtype: d or s; default 65536 1024 d)

lansy (One norm, Lower), pocon on the Lower factor (with its number of applications of A^{-1}), one application
(pocon's sweep time over its applications: a forward and a backward sweep), the same application through potrs at
nrhs = 1, and potrf for scale.  Each a warm-up call and then the median of REPS calls.  TB/s count the bytes of the
stored triangle, 8 n (n + 1) / 2 (fp32: 4 n (n + 1) / 2), once for lansy and per sweep (twice per application)."""
import os, sys, time
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
TRI = (8 if DT == "d" else 4) * N * (N + 1) / 2


def desc(ncols=N):
    return ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, ncols, 0, 0, N, ncols, 1, 1)


A = desc()


def median(fn):
    fn()  # warm-up (scratch allocation, first launches)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0, out))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


def line(name, sec, nbytes, extra=""):
    print(f"{name:22s}: {sec * 1e3:9.3f} ms  {nbytes / sec / 1e12:6.2f} TB/s  {extra}", flush=True)


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}  stored triangle {TRI / 1e9:.2f} GB", flush=True)
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
t, anorm = median(lambda: ch.CHAMELEON_dlansy_Tile(ch.ChamOneNorm, ch.ChamLower, A))
line("lansy(One)", t, TRI, f"anorm = {anorm:.6e}")
pts = []
for _ in range(REPS):  # (the input restored outside the timed region; the last call leaves the factor)
    ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A, 42)
    t0 = time.perf_counter()
    assert ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, A) == 0
    pts.append(time.perf_counter() - t0)
t_potrf = sorted(pts)[REPS // 2]
t, rcond = median(lambda: ch.CHAMELEON_dpocon_Tile(ch.ChamLower, A, anorm))
st = ch.last_pocon_stats()
napp = st["applications"]
line("pocon", t, 2 * napp * TRI, f"rcond = {rcond:.6e}, {napp} applications, device total {st['total_ms']:.3f} ms")
one = st["sweep_ms"] * 1e-3 / napp
line("one application", one, 2 * TRI, f"({one / 2 * 1e3:.3f} ms per sweep)")
Bv = desc(1)
t, _ = median(lambda: ch.CHAMELEON_dpotrs_Tile(ch.ChamLower, A, Bv))
line("potrs nrhs=1", t, 2 * TRI, f"({t / one:.1f} x one application)")
print(f"{'potrf':22s}: {t_potrf * 1e3:9.1f} ms  (pocon = {st['total_ms'] / (t_potrf * 1e3) * 100:.2f} % of it)", flush=True)
