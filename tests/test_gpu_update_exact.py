"""Every update kernel, exact on integer data, fp64 and fp32.

Entries are integers in [-3, 3], so every product and every partial sum of a K-loop is an integer of magnitude at most
2 * 9 * mb + 3 < 2^24 (mb <= 4096): the fp32 and the fp64 MFMAs give the exact result in any order of summation, and
so does the host's fp64 BLAS.  A kernel that drops a K-slice, writes a wrong row block, updates an entry above the
diagonal or maps a workgroup to the wrong block is caught bit for bit, whatever the rounding model.

  * the whole-matrix trailing update (k_trail_update_w8<double, 3> / k_trail_update_w8f) through bench_update, at
    tile sizes of 1, 2, 3, 5 and 8 128-blocks: the single-diagonal-tile launch (k = nt - 2), segments whose block
    counts are not a multiple of the unit, and the units of 64 and of 8 forced in a fresh process (CHOLMI_MIN_UNITS);
  * the task path's out-of-place updates (k_update_ptrs_w8 / k_update_ptrs_w8f) through chol_tile_batch SYRK / GEMM /
    UPDATE, against numpy and against chol_syrk_tile / chol_gemm_tile on the same tile;
  * the single-tile GEMM / SYRK (k_gemm_nt_tile) with power-of-two scalars, on tile edges that are and are not
    multiples of 128.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DTYPES = ["f64", "f32"]


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float64)


def _cdt(ch, dtype):
    return ch.ChamRealDouble if dtype == "f64" else ch.ChamRealFloat


# --------------------------------------------------------------------------------------------------------------------
# 1. the whole-matrix trailing update
#
# (mb, nt, k); nbm = mb / 128, na = off-diagonal tiles of the launch, nb = diagonal tiles.  At the library's default
# (CHOLMI_MIN_UNITS = 128) every launch below is dealt in units of 8 blocks.
#   (128, 6, 0)   nbm 1: na = 10 blocks, segment B starts on XCD 2
#   (128, 6, 4)   k = nt - 2: one diagonal tile of one block (map_update_block's na == 0 && nb == 1 branch)
#   (256, 5, 1)   nbm 2: na * 4 = 12 blocks, segment B on XCD 2
#   (384, 5, 0)   nbm 3: 54 blocks, a tile straddles two units; segment B on XCD 7 (on XCD 1 with units of 64)
#   (384, 4, 2)   k = nt - 2 at nbm 3
#   (640, 4, 0)   nbm 5: 75 blocks, segment B on XCD 2 (units of 8 and of 64)
#   (640, 3, 1)   k = nt - 2 at nbm 5
#   (1024, 3, 0)  nbm 8: one off-diagonal tile of 64 blocks (one unit of 64 when forced, segment B on XCD 1)
#   (1024, 3, 1)  k = nt - 2 at nbm 8
# --------------------------------------------------------------------------------------------------------------------
UPDATE_CASES = [(128, 6, 0), (128, 6, 4), (256, 5, 1), (384, 5, 0), (384, 4, 2), (640, 4, 0), (640, 3, 1),
                (1024, 3, 0), (1024, 3, 1)]


def _update_input(mb, nt, k):
    return _ints(np.random.default_rng(7000 + 10 * mb + k), (nt * mb, nt * mb))


def _run_update(ch, dtype, A, mb, k):
    N = A.shape[0]
    d = ch.CHAMELEON_Desc_Create(None, _cdt(ch, dtype), mb, mb, mb * mb, N, N, 0, 0, N, N, 1, 1)
    try:
        d.from_lapack(A)
        ch.bench_update(d, k, 0, 1)  # the update twice: one warm-up, one timed rep
        return d.to_lapack().astype(np.float64)
    finally:
        ch.CHAMELEON_Desc_Destroy(d)


def _check_update(got, A, mb, nt, k, what):
    """got = A with C(i, j) -= 2 L(i, k) L(j, k)^T on every tile i >= j > k, lower triangle of the diagonal tiles
    only; everything else bit for bit as it was."""
    t = lambda i: slice(i * mb, (i + 1) * mb)
    # panel column k and every tile column left of it
    assert np.array_equal(got[:, :(k + 1) * mb], A[:, :(k + 1) * mb]), (what, "columns <= k changed")
    for j in range(k + 1, nt):
        assert np.array_equal(got[:j * mb, t(j)], A[:j * mb, t(j)]), (what, "tiles above the diagonal changed", j)
        assert np.array_equal(np.triu(got[t(j), t(j)], 1), np.triu(A[t(j), t(j)], 1)), (what, "strict upper of tile", j)
    want = A.copy()
    P = A[:, t(k)]
    for j in range(k + 1, nt):
        for i in range(j, nt):
            upd = 2.0 * (P[t(i)] @ P[t(j)].T)
            want[t(i), t(j)] -= np.tril(upd) if i == j else upd
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:8], [(i // 128, j // 128) for i, j in bad[:8]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mb,nt,k", UPDATE_CASES)
def test_whole_matrix_update_is_exact_on_integers(cham, dtype, mb, nt, k):
    A = _update_input(mb, nt, k)
    _check_update(_run_update(cham, dtype, A, mb, k), A, mb, nt, k, (dtype, mb, nt, k))


# the forced units: 64 (CHOLMI_MIN_UNITS=1: (384, 5, 0), (640, 4, 0) and (1024, 3, 0) then leave their segment A
# partly empty and start segment B on XCD 1, 2 and 1) and 8 (CHOLMI_MIN_UNITS=100000)
FORCED_CASES = [(384, 5, 0), (640, 4, 0), (1024, 3, 0), (384, 4, 2), (256, 5, 1)]


@pytest.mark.parametrize("min_units", ["1", "100000"])
def test_whole_matrix_update_with_forced_units_is_exact(min_units):
    """CHOLMI_MIN_UNITS is read once, so each setting runs in a fresh process; both precisions there."""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "from dense_linear_app_amd import chameleon as ch\n"
        "ch.CHAMELEON_Init(1, 1)\n"
        "for name in sys.argv[1:]:\n"
        "    mb, nt, k, dt = name.split('_')\n"
        "    mb, k = int(mb), int(k)\n"
        "    A = np.load(sys.argv[0].rsplit('/', 1)[0] + '/' + name + '_in.npy')\n"
        "    N = A.shape[0]\n"
        "    d = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble if dt == 'f64' else ch.ChamRealFloat, mb, mb, mb * mb,"
        " N, N, 0, 0, N, N, 1, 1)\n"
        "    d.from_lapack(A)\n"
        "    ch.bench_update(d, k, 0, 1)\n"
        "    np.save(sys.argv[0].rsplit('/', 1)[0] + '/' + name + '_out.npy', d.to_lapack().astype(np.float64))\n"
        "    ch.CHAMELEON_Desc_Destroy(d)\n"
        "print('done')\n"
    ) % ROOT
    with tempfile.TemporaryDirectory() as tmp:
        script = os.path.join(tmp, "child.py")
        with open(script, "w") as f:
            f.write(code)
        names = []
        for mb, nt, k in FORCED_CASES:
            A = _update_input(mb, nt, k)
            for dt in DTYPES:
                name = "%d_%d_%d_%s" % (mb, nt, k, dt)
                np.save(os.path.join(tmp, name + "_in.npy"), A)
                names.append(name)
        r = subprocess.run([sys.executable, script] + names, env=dict(os.environ, CHOLMI_MIN_UNITS=min_units),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "done" in r.stdout, (r.stdout, r.stderr[-2000:])
        for name in names:
            mb, nt, k, dt = name.split("_")
            mb, nt, k = int(mb), int(nt), int(k)
            _check_update(np.load(os.path.join(tmp, name + "_out.npy")), _update_input(mb, nt, k), mb, nt, k,
                          (min_units, name))


# --------------------------------------------------------------------------------------------------------------------
# 2. the task path: chol_tile_batch SYRK / GEMM / UPDATE (k_update_ptrs_w8 / k_update_ptrs_w8f)
#
# (mb, n, operands): "wave" -- the tasks are the first n tiles (i, j), i >= j, of a wave's trailing matrix, column by
# column, with a = L(i, k) and b = L(j, k): operands shared across tasks, SYRK tasks on the diagonal; "distinct" --
# every task has operands of its own.  n * nbm^2 = 33, 81, 112, 576, 256, 2112 (units of 16 at the default) and 1
# block.  The SYRK and GEMM batches go out on the bulk stream and are short against a panel step, so their
# workgroups poll the yield table (the K-loop's yield branch); the UPDATE batches go out URGENT, which never yields.
# --------------------------------------------------------------------------------------------------------------------
BATCH_CASES = [(128, 33, "wave"), (384, 9, "wave"), (512, 7, "distinct"), (1024, 9, "distinct"),
               (2048, 1, "distinct"), (1024, 33, "wave"), (128, 1, "distinct")]
SYRK, GEMM, UPDATE, URGENT = 2, 3, 4, 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mb,n,operands", BATCH_CASES)
def test_tile_batch_updates_are_exact_on_integers(cham, dtype, mb, n, operands):
    import torch

    from dense_linear_app_amd._lib import lib

    ch, L = cham, lib()
    cdt = _cdt(ch, dtype)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(100 * mb + n)

    def dev(a):
        return torch.from_numpy(a.ravel(order="F").copy()).to(tdt).cuda()

    def host(t):
        return t.cpu().numpy().astype(np.float64).reshape((mb, mb), order="F")

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[None if x is None else x.data_ptr() for x in ts])

    if operands == "wave":
        p = 1
        while p * (p + 1) // 2 < n:
            p += 1
        pairs = [(i, j) for j in range(p) for i in range(j, p)][:n]
        panel = [_ints(rng, (mb, mb)) for _ in range(p)]
        dpanel = [dev(x) for x in panel]
        a_h = [panel[i] for i, j in pairs]
        b_h = [panel[j] for i, j in pairs]
        a_d = [dpanel[i] for i, j in pairs]
        b_d = [dpanel[j] for i, j in pairs]
        diag = [i == j for i, j in pairs]
    else:
        a_h = [_ints(rng, (mb, mb)) for _ in range(n)]
        b_h = [_ints(rng, (mb, mb)) for _ in range(n)]
        a_d, b_d = [dev(x) for x in a_h], [dev(x) for x in b_h]
        diag = [t % 3 == 1 for t in range(n)]
    c_h = [_ints(rng, (mb, mb)) for _ in range(n)]
    c_d = [dev(x) for x in c_h]
    out = [torch.full((mb * mb,), float("nan"), dtype=tdt, device="cuda") for _ in range(n)]
    up = np.triu_indices(mb, 1)

    def single_tile(t, syrk):
        """The same task through chol_syrk_tile / chol_gemm_tile (k_gemm_nt_tile) on a copy of c_in."""
        ct = c_d[t].clone()
        torch.cuda.synchronize()  # (the library's streams are not ordered behind torch's)
        mk = lambda x: ch.CHAMELEON_Desc_Create(x, cdt, mb, mb, mb * mb, mb, mb, 0, 0, mb, mb, 1, 1)
        dc, da = mk(ct), mk(a_d[t])
        if syrk:
            assert ch.CHAMELEON_dsyrk_Tile(ch.ChamLower, ch.ChamNoTrans, -1.0, da, 1.0, dc) == 0
        else:
            db = mk(b_d[t])
            assert ch.CHAMELEON_dgemm_Tile(ch.ChamNoTrans, ch.ChamTrans, -1.0, da, db, 1.0, dc) == 0
            ch.CHAMELEON_Desc_Destroy(db)
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(dc)
        return ct

    for op in (SYRK, GEMM, UPDATE):
        syrk = [True] * n if op == SYRK else [False] * n if op == GEMM else diag
        blist = None if op == SYRK else ptrs([None if s else b for s, b in zip(syrk, b_d)])
        for o in out:
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        flags = URGENT if op == UPDATE else 0
        rc = L.chol_tile_batch(op, cdt, mb, n, ptrs(c_d), ptrs(a_d), blist, ptrs(out), None, flags)
        assert rc == 0, L.chol_last_error()
        for t in range(n):
            got = host(out[t])
            ref = c_h[t] - a_h[t] @ (a_h[t] if syrk[t] else b_h[t]).T
            if syrk[t]:
                ref[up] = c_h[t][up]
                assert np.array_equal(got[up], c_h[t][up]), (op, t, "strict upper not copied")
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (op, t, len(bad), bad[:8])
            assert torch.equal(out[t], single_tile(t, syrk[t])), (op, t, "differs from the single-tile kernel")
    for t in range(n):  # the inputs are read only
        assert np.array_equal(host(c_d[t]), c_h[t]) and np.array_equal(host(a_d[t]), a_h[t])
        assert np.array_equal(host(b_d[t]), b_h[t])


# --------------------------------------------------------------------------------------------------------------------
# 3. single-tile GEMM / SYRK (k_gemm_nt_tile): C := alpha A B^T + beta C; 200 and 300 go through the staged, padded path
# --------------------------------------------------------------------------------------------------------------------
SCALARS = [1.0, -1.0, 2.0, 0.5, 0.0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [128, 256, 1024, 200, 300])
def test_single_tile_gemm_syrk_are_exact_on_integers(cham, dtype, B):
    ch = cham
    cdt, npdt = _cdt(ch, dtype), (np.float64 if dtype == "f64" else np.float32)
    rng = np.random.default_rng(B)
    A, Bm, C0 = _ints(rng, (B, B)), _ints(rng, (B, B)), _ints(rng, (B, B))
    AB, AA = A @ Bm.T, A @ A.T
    mk = lambda a: ch.CHAMELEON_Desc_Create(a, cdt, B, B, B * B, B, B, 0, 0, B, B, 1, 1)
    dA, dB = mk(np.asfortranarray(A, dtype=npdt)), mk(np.asfortranarray(Bm, dtype=npdt))
    low, up = np.tril_indices(B), np.triu_indices(B, 1)
    for alpha in SCALARS:
        for beta in SCALARS:
            Cg = np.asfortranarray(C0, dtype=npdt)
            assert ch.CHAMELEON_dgemm_Tile(ch.ChamNoTrans, ch.ChamTrans, alpha, dA, dB, beta, mk(Cg)) == 0
            assert np.array_equal(Cg.astype(np.float64), alpha * AB + beta * C0), ("gemm", alpha, beta)
            Cs = np.asfortranarray(C0, dtype=npdt)
            assert ch.CHAMELEON_dsyrk_Tile(ch.ChamLower, ch.ChamNoTrans, alpha, dA, beta, mk(Cs)) == 0
            assert np.array_equal(Cs.astype(np.float64)[low], (alpha * AA + beta * C0)[low]), ("syrk", alpha, beta)
            assert np.array_equal(Cs[up], np.asarray(C0, dtype=npdt)[up]), ("syrk upper", alpha, beta)
    # beta = 0: C is not read, NaN in it does not reach the result (and the strict upper triangle of SYRK keeps it)
    for alpha in (1.0, -1.0):
        Cg = np.full((B, B), np.nan, dtype=npdt, order="F")
        assert ch.CHAMELEON_dgemm_Tile(ch.ChamNoTrans, ch.ChamTrans, alpha, dA, dB, 0.0, mk(Cg)) == 0
        assert np.array_equal(Cg.astype(np.float64), alpha * AB), ("gemm beta 0", alpha)
        Cs = np.full((B, B), np.nan, dtype=npdt, order="F")
        assert ch.CHAMELEON_dsyrk_Tile(ch.ChamLower, ch.ChamNoTrans, alpha, dA, 0.0, mk(Cs)) == 0
        assert np.array_equal(Cs.astype(np.float64)[low], (alpha * AA)[low]), ("syrk beta 0", alpha)
        assert np.isnan(Cs[up]).all()
