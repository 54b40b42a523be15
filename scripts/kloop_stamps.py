#!/usr/bin/env python3
"""In-kernel stamps of the fp64 update's K-loop (diagnostic build only: kernels.hip built with
-DCHOLMI_KLOOP_STAMPS, loaded through LIBCHOLMI_PATH).  Runs the update of tile column 0 back to back for
about 2 s, then reads the stamps of the last launch (workgroups 0-15, every wave, the first 64 stages):
  clock   = d(s_memtime) / d(s_memrealtime) x 100 MHz over the whole K-loop
  stage   = cycles from one stage's start to the next one's (1024 MFMA cycles of a wave per 8-deep stage)
  wait    = cycles from just before the counted vmcnt wait to the first fragment wait behind the barrier
            (vmcnt wait + barrier + LDS round trip), less the cost of the two stamps in it
usage: LIBCHOLMI_PATH=<diag .so> python scripts/kloop_stamps.py 32768x1024 32768x512"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import numpy as np

from dense_linear_app_amd import chameleon as ch
from dense_linear_app_amd._lib import lib

WGS, STAGES = 16, 64
REC = 4 + 5 * STAGES

ch.CHAMELEON_Init(1, 1)
L = lib()
cfgs = [tuple(map(int, a.split("x"))) for a in sys.argv[1:]] or [(32768, 1024)]
for N, B in cfgs:
    d = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, N, 0, 0, N, N, 1, 1)
    ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamLower, d, 42)
    t0 = time.time()
    while time.time() - t0 < 2.0:
        ms, tf = ch.bench_update(d, 0, 0, 3)
    buf = (C.c_ulonglong * (WGS * 8 * REC))()
    n = L.chol_debug_kloop_stamps(buf, len(buf))
    assert n == len(buf), n
    a = np.array(buf, dtype=np.uint64).astype(np.int64).reshape(WGS * 8, REC)
    clock = (a[:, 2] - a[:, 0]) / ((a[:, 3] - a[:, 1]) / 100e6) / 1e9
    st = a[:, 4:].reshape(-1, STAGES, 5)  # per stage: start, after DMA, before wait, after barrier, after fragment wait
    stage = np.diff(st[:, :, 0], axis=1)
    pair = st[:, :, 4] - st[:, :, 3]  # two stamps back to back in the ring (the old loop: the LDS round trip too)
    wait = st[:, :, 4] - st[:, :, 2]
    print(f"N={N} B={B}: {tf:6.2f} TF/s (stamped build)  clock median {np.median(clock):.3f} GHz "
          f"(min {clock.min():.3f}, max {clock.max():.3f})")
    print(f"  per stage (cycles, median over waves and stages 1..{STAGES - 2}): stage {np.median(stage[:, 1:]):.0f}  "
          f"wait+barrier+fragment {np.median(wait[:, 1:-1]):.0f}  back-to-back stamps/after-barrier pair "
          f"{np.median(pair[:, 1:-1]):.0f}  p90 wait {np.percentile(wait[:, 1:-1], 90):.0f}")
    ch.CHAMELEON_Desc_Destroy(d)
