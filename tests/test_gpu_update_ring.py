"""The fp64 trailing update (k_trail_update_w8<double, 3>) fed from the four-stage LDS ring.

On the GPU: the update alone on integer data, where every product and partial sum is exact in fp64, must match
the host reference bit for bit (off-diagonal tiles, and diagonal tiles whose 128-blocks above the diagonal are
masked in the epilogue), at tiles 512 and 1024 and on ragged lists of tiles; the paired (two-panel) launches of the
factorisation must match the oracle.  Without a GPU: the built code object keeps the update's register and LDS
budget, which the co-residency of the panel chain's kernels rests on.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
@pytest.mark.parametrize("B,nt,k", [(512, 5, 0), (512, 5, 2), (1024, 4, 0), (1024, 4, 1)])
def test_update_alone_is_exact_on_integers(cham, B, nt, k):
    """bench_update(k, reps=1) applies C(i, j) -= L(i, k) L(j, k)^T twice to every tile below column k (lower
    triangle of the diagonal tiles only).  k > 0 leaves a ragged number of tiles (not a multiple of the XCD count)."""
    ch = cham
    N = nt * B
    rng = np.random.default_rng(1000 * B + k)
    A = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    d = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, N, N, 0, 0, N, N, 1, 1)
    try:
        d.from_lapack(A)
        ch.bench_update(d, k, 0, 1)
        got = d.to_lapack()
    finally:
        ch.CHAMELEON_Desc_Destroy(d)
    want = A.copy()
    P = A[:, k * B:(k + 1) * B]
    for j in range(k + 1, nt):
        for i in range(j, nt):
            upd = 2.0 * (P[i * B:(i + 1) * B] @ P[j * B:(j + 1) * B].T)
            if i == j:
                upd = np.tril(upd)
            want[i * B:(i + 1) * B, j * B:(j + 1) * B] -= upd
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("N,B", [(4096, 512), (6144, 1024)])
def test_paired_launches_match_the_oracle(orc, N, B):
    """CHOLMI_PAIR_FACTOR=0: every wave that may go in pairs does, so the update's launches carry two panels (two
    K-loops back to back through the same ring).  Fresh process: the switches are read once."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        code = (
            "import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from dense_linear_app_amd import chameleon as ch\n"
            "ch.CHAMELEON_Init(1, 1)\n"
            "d = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, %d, %d, %d, %d, %d, 0, 0, %d, %d, 1, 1)\n"
            "ch.CHAMELEON_dplgsy_Tile(float(%d), ch.ChamLower, d, 42)\n"
            "info = ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d)\n"
            "np.save(%r + '/L.npy', d.to_lapack()); print('info', info)\n"
        ) % (ROOT, B, B, B * B, N, N, N, N, N, tmp)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CHOLMI_PAIR_FACTOR="0"),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "info 0" in r.stdout, (r.stdout, r.stderr[-2000:])
        L = np.tril(np.load(tmp + "/L.npy"))
    T = orc.plgsy_tiles(N // B, B, float(N), 42)
    assert orc.tiled_potrf(T, N // B, B) == 0
    Lref = np.tril(orc.tile_to_lapack(T, N, B))
    assert np.abs(L - Lref).max() / np.abs(Lref).max() <= 1e-12


def test_fp64_update_kernels_keep_their_register_and_lds_budget():
    """The ring lives in the 64 KiB the double buffer had, and the update stays within 120 VGPRs: beside two
    update workgroups per CU, the diagonal-block kernel (about 257 VGPRs, 93 KiB of LDS) must still fit."""
    sys.path.insert(0, os.path.dirname(__file__))
    import codeobj
    from dense_linear_app_amd._lib import LIB_PATH

    res = codeobj.kernel_resources(LIB_PATH)
    for part in ("k_trail_update_w8IdLi3E", "k_update_ptrs_w8IdLi3E"):
        hits = [v for name, v in res.items() if part in name]
        assert len(hits) == 1, (part, hits)
        assert hits[0]["vgprs"] <= 120 and hits[0]["lds"] <= 64 * 1024, (part, hits[0])
