#!/usr/bin/env python3
"""Timing of CHAMELEON_dsposv_Tile (fp32 factor + fp64 refinement) against CHAMELEON_dposv_Tile on the same plgsy
matrix, in one process: python scripts/dsposv_time.py [N tile nrhs]

A warm-up call, then the median of 5 of each; A is restored from a pristine copy before every call (dposv overwrites
it with the factor) and X from B, outside the timed region.  The residual pass R = B - A X reads the stored triangle,
8 n (n + 1) / 2 bytes: its effective bandwidth is printed over that count."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B, nrhs = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (65536, 1024, 1)
REPS = 5


def desc(ncols):
    return ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, ncols, 0, 0, N, ncols, 1, 1)


A0, A, dB, X = desc(N), desc(N), desc(nrhs), desc(nrhs)
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A0, 42)
dB.from_lapack(np.asfortranarray(np.random.default_rng(11).standard_normal((N, nrhs))))


def timed(fn):
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, A0, A)
    ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, dB, X)
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(name, fn):
    timed(fn)  # warm-up (scratch allocation, first launches)
    runs = [timed(fn) for _ in range(REPS)]
    ts = sorted(t for t, _ in runs)
    print(f"{name}: median {ts[REPS // 2] * 1e3:.1f} ms  (min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f})", flush=True)
    return ts[REPS // 2], runs[-1][1]


print(f"N={N} tile={B} nrhs={nrhs}", flush=True)
t_d, info = run("dposv ", lambda: ch.CHAMELEON_dposv_Tile(ch.ChamLower, A, X))
assert info == 0
t_m, (info, it) = run("dsposv", lambda: ch.CHAMELEON_dsposv_Tile(ch.ChamLower, A, dB, X))
assert info == 0
st = ch.last_dsposv_stats()
tr = st["residual_ms"] / st["residuals"]
ts = st["solve_ms"] / st["solves"]
print(f"iter = {it}   dsposv / dposv = {t_m / t_d:.3f}")
print(f"last dsposv call: total {st['total_ms']:.1f} ms = fp64->fp32 conversions + ||A||_inf {st['convert_ms']:.1f}"
      f" + fp32 factor {st['factor_ms']:.1f} + {st['solves']} fp32 solves {st['solve_ms']:.1f}"
      f" + {st['residuals']} residual passes {st['residual_ms']:.1f} (+ updates / host {st['total_ms'] - st['convert_ms'] - st['factor_ms'] - st['solve_ms'] - st['residual_ms']:.1f})")
print(f"per refinement step: {ts + tr:.2f} ms (fp32 solve {ts:.2f} + residual {tr:.2f})")
print(f"residual pass: {tr:.3f} ms, {8.0 * N * (N + 1) / 2 / (tr * 1e-3) / 1e12:.2f} TB/s effective over 8 n(n+1)/2 bytes",
      flush=True)
