#!/usr/bin/env python3
"""Timing of the SPD expert solve on one plgsy matrix, in one process:
python scripts/posvx_time.py [N tile dtype [nrhs,...]]   (dtype: d or s; default 65536 1024 d 1,8,64)

For each nrhs: posv (potrf + potrs) against posvx ('E': poequ finds the plgsy matrix well scaled, so no scaling),
posvx split by phase from its device events (chol_last_posvx_stats), the residual pass of porfs alone (TB/s count
the stored triangle once per group of up to 8 columns), and the path porfs took.  Then one application of A^{-1}
at NV = 1, 2, 4, 8 vectors (the multi-vector sweeps) and the crossover against potrs on k columns (K_X).  Each
number: a warm-up call and then the median (host wall time) or the fastest (device events, chol_bench_refine) of
REPS calls.  The input is restored outside the timed region."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from dense_linear_app_amd import chameleon as ch
ch.CHAMELEON_Init(1, 1)
N, B = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (65536, 1024)
DT = sys.argv[3] if len(sys.argv) > 3 else "d"
NRHS = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 8, 64]
REPS = 3
dtype = ch.ChamRealDouble if DT == "d" else ch.ChamRealFloat
npt = np.float64 if DT == "d" else np.float32
TRI = (8 if DT == "d" else 4) * N * (N + 1) / 2
L = ch.ChamLower


def desc(ncols=N):
    return ch.CHAMELEON_Desc_Create(None, dtype, B, B, B * B, N, ncols, 0, 0, N, ncols, 1, 1)


A0, A, AF, S = desc(), desc(), desc(), desc(1)
ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, A0, 42)
rng = np.random.default_rng(1)


def median(fn, prep):
    ts = []
    for r in range(REPS + 1):
        prep()
        t0 = time.perf_counter()
        out = fn()
        if r:
            ts.append((time.perf_counter() - t0, out))
    ts.sort(key=lambda x: x[0])
    return ts[REPS // 2]


print(f"N={N} tile={B} dtype={'fp64' if DT == 'd' else 'fp32'}  stored triangle {TRI / 1e9:.2f} GB", flush=True)
for nrhs in NRHS:
    Bh = np.asfortranarray(rng.standard_normal((N, nrhs)).astype(npt))
    B0, Bd, X = desc(nrhs), desc(nrhs), desc(nrhs)
    B0.from_lapack(Bh)

    def prep():
        ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, A0, A)
        ch.CHAMELEON_dlacpy_Tile(ch.ChamUpperLower, B0, Bd)

    def posv():
        assert ch.CHAMELEON_dpotrf_Tile(L, A) == 0
        ch.CHAMELEON_dpotrs_Tile(L, A, Bd)

    t_posv, _ = median(posv, prep)
    t_potrf, _ = median(lambda: ch.CHAMELEON_dpotrf_Tile(L, A), prep)
    t_posvx, out = median(lambda: ch.CHAMELEON_dposvx_Tile("E", L, A, AF, "N", S, Bd, X), prep)
    st = ch.last_posvx_stats()
    info, equed, rcond, ferr, berr = out
    path = f"{st['sweep_columns']} columns by sweeps, {st['potrs_columns']} by potrs"
    print(f"nrhs={nrhs:<4d} posv {t_posv * 1e3:9.1f} ms  posvx {t_posvx * 1e3:9.1f} ms  ({t_posvx / t_posv:.3f} x posv)"
          f"  potrf {t_potrf * 1e3:9.1f} ms", flush=True)
    print(f"          posvx phases [ms, device]: total {st['total_ms']:.1f}  equilibrate {st['equilibrate_ms']:.2f}"
          f"  factor {st['factor_ms']:.1f}  rcond {st['rcond_ms']:.2f}  solve {st['solve_ms']:.2f}"
          f"  porfs {st['porfs_ms']:.2f} ({st['porfs_ms'] / (t_potrf * 1e3) * 100:.2f} % of potrf)", flush=True)
    print(f"          info={info} equed={equed} rcond={rcond:.3e} max ferr={ferr.max():.2e} max berr={berr.max():.2e}"
          f"  ({path})", flush=True)
    t = ch.bench_refine(L, A, AF, X, 0, REPS) * 1e-3
    passes = (nrhs + 7) // 8
    print(f"          residual pass: {t * 1e3:.3f} ms  {passes * TRI / t / 1e12:.2f} TB/s  ({passes} pass(es) over the"
          f" triangle)", flush=True)

# one application at NV = 1, 2, 4, 8 on the factor of the last posvx, then the sweeps against potrs on k columns
Xh = np.asfortranarray(rng.standard_normal((N, 256)).astype(npt))
one = None
for nv in (1, 2, 4, 8):
    Xv = desc(nv)
    Xv.from_lapack(Xh[:, :nv])
    t = ch.bench_refine(L, A, AF, Xv, 1, REPS)
    one = one or t
    print(f"application NV={nv}: {t:8.3f} ms  ({t / one:.2f} x NV=1, {2 * TRI / (t * 1e-3) / 1e12:.2f} TB/s per"
          f" application)", flush=True)
for k in (8, 16, 24, 32, 40, 48, 56, 64, 96, 128):
    Xk = desc(k)
    Xk.from_lapack(Xh[:, :k])
    ts = ch.bench_refine(L, A, AF, Xk, 1, 1)
    tp = ch.bench_refine(L, A, AF, Xk, 2, 1)
    print(f"k={k:<4d} sweeps {ts:9.2f} ms  potrs {tp:9.2f} ms  ({'sweeps' if ts <= tp else 'potrs'} faster)", flush=True)
