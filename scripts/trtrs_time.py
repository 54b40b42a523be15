#!/usr/bin/env python3
"""Timing of the half solve, the half product and the log-determinant with a Cholesky factor, in one process:
python scripts/trtrs_time.py [N tile [out]]   (default 65536 1024 profiles/trtrs_time_N<N>_B<tile>.txt)

fp64, Lower.  A is a plgsy matrix (bump N), F its factor, B standard normal.  Each figure is the median of REPS calls
after a warm-up, from the device events that the library records on its own stream (chol_last_trtrs_stats; for the
yardsticks chol_bench_refine's events, or the wall time of the synchronous call), with B restored on the device
outside the timed region:
  lacpy (Lower)    the stored triangle read once and written once: the read-and-write floor
  application      chol_bench_refine path 1: one full application of inv(A) by the narrow sweeps, both halves
  trtrs / trmm     forward (Lower, NoTrans) and backward (Lower, Trans) at nrhs = 1, 8, 40, 41, 64, 1024 by the path rule,
                   beside chol_potrs_tile at the same nrhs
  crossovers       both paths forced (chol_debug_half_limits) at nrhs = 1 ... 128
  logdet
Every line goes to stdout and to `out`."""
import os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"trtrs_time_N{N}_B{B}.txt")
REPS = 3
NRHS = (1, 8, 40, 41, 64, 1024)
CROSS = (1, 8, 16, 24, 32, 40, 48, 64, 96, 128)
L, NT, TR, NU = ch.ChamLower, ch.ChamNoTrans, ch.ChamTrans, ch.ChamNonUnit
out = open(OUT, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def desc(cols):
    return ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, cols, 0, 0, N, cols, 1, 1)


def median(fn, prep=lambda: None):
    """fn() -> ms (or None: the wall time of the call)"""
    ts = []
    for r in range(REPS + 1):
        prep()
        t0 = time.perf_counter()
        v = fn()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3 if v is None else v)
    return sorted(ts)[REPS // 2]


def wall(f):
    """f timed by the wall clock (a synchronous call)"""
    def run():
        f()
        return None
    return run


def half(kind, trans, X):
    """one call -> its phases (total, staging, sweeps or products [ms]) and the path it took"""
    if kind == "trtrs":
        assert ch.CHAMELEON_dtrtrs_Tile(L, trans, NU, F, X) == 0
    else:
        assert ch.CHAMELEON_dtrmm_Tile(ch.ChamLeft, L, trans, NU, 1.0, F, X) == 0
    return ch.last_trtrs_stats()


F = desc(N)
say(f"N={N} tile={B} dtype=fp64  (median of {REPS})")
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, F, 42)
assert ch.CHAMELEON_dpotrf_Tile(L, F) == 0
W = desc(N)
t_cp = median(wall(lambda: ch.CHAMELEON_dlacpy_Tile(L, F, W)))
ch.CHAMELEON_Desc_Destroy(W)
tri_bytes = 8.0 * N * (N + B) / 2  # the stored triangle: whole diagonal tiles
say(f"{'lacpy (Lower): floor':30s}: {t_cp:10.2f} ms  {2 * tri_bytes / t_cp / 1e9:6.2f} TB/s (2 x {tri_bytes / 1e9:.2f} GB)")
info, ld = ch.CHAMELEON_dlogdet_Tile(F)
t_ld = median(wall(lambda: ch.CHAMELEON_dlogdet_Tile(F)))
say(f"{'logdet':30s}: {t_ld:10.3f} ms  (info {info}, value {ld:.6f})")

rng = np.random.default_rng(1)
Bh = np.asfortranarray(rng.standard_normal((N, max(NRHS))))
app = {}
for k in sorted(set(NRHS) | set(CROSS)):
    B0, X = desc(k), desc(k)
    B0.from_lapack(Bh[:, :k])
    restore = lambda: ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, B0, X)
    restore()
    if k <= 8:
        app[k] = ch.bench_refine(L, F, F, X, 1, REPS)
        say(f"{'application nrhs=' + str(k):30s}: {app[k]:10.2f} ms  (chol_bench_refine path 1: both halves, staging excluded)")
    if k in NRHS:
        t_potrs = median(wall(lambda: ch.CHAMELEON_dpotrs_Tile(L, F, X)), restore)
        say(f"{'potrs nrhs=' + str(k):30s}: {t_potrs:10.2f} ms")
        for kind in ("trtrs", "trmm"):
            for name, trans in (("forward", NT), ("backward", TR)):
                keep = {}

                def one():
                    keep["st"] = half(kind, trans, X)
                    return keep["st"]["total_ms"]

                t = median(one, restore)
                st = keep["st"]
                path = "narrow" if st["narrow_cols"] else "wide"
                extra = ""
                if kind == "trtrs" and k in app:
                    extra = f"  sweeps {st['work_ms'] / app[k]:.2f} x the full application"
                if kind == "trmm" and path == "narrow":
                    extra = f"  {st['work_ms'] / (-(-k // 8) * t_cp):.2f} x the lacpy floor of {-(-k // 8)} pass(es)"
                say(f"{kind + ' ' + name + ' nrhs=' + str(k):30s}: {t:10.2f} ms  ({path}: staging {st['stage_ms']:.2f}, "
                    f"sweeps or products {st['work_ms']:.2f}){extra}")
    if k in CROSS:
        for kind in ("trtrs", "trmm"):
            res = []
            for limit in (1 << 20, 0):  # narrow forced, then wide forced
                ch.half_limits(limit, limit)
                res.append(median(lambda: half(kind, NT, X)["total_ms"], restore))
            ch.half_limits()
            say(f"{'crossover ' + kind + ' nrhs=' + str(k):30s}: narrow {res[0]:10.2f} ms  wide {res[1]:10.2f} ms  "
                f"({'narrow' if res[0] <= res[1] else 'wide'} faster)")
    ch.CHAMELEON_Desc_Destroy(B0)
    ch.CHAMELEON_Desc_Destroy(X)
out.close()
