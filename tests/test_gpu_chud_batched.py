"""The batched rank-r update and downdate of small factors on the device (dense_linear_app_amd.batched: chud_batched,
chdd_batched over chol_chud_batched, chol_chdd_batched), at the orders on both sides of every packing boundary
(potrf_batched_model.ORDERS), fp64 and fp32, Lower and Upper.  Batches hold 2 (64 / P) + 1 distinct matrices (several
sub-groups, two wavefronts and a partly filled one) unless stated; the inputs are chud_batched_model.py's.

  numerics    max |dL| / max |L| in eps against chud_model in the dtype (only the fused multiply-add differs) and
              against numpy's fp64 Cholesky of A +- V V^T; the bounds are 10 x what the model itself measures on
              these batches (chud_batched_model.py): 2.42 / 39.9 eps fused against plain, 4.75 / 88.6 eps (fp64) and
              2.25 / 47.2 eps (fp32) against LAPACK, update / downdate
  tile        bit for bit what CHAMELEON_dchud_Tile / dchdd_Tile return for the same L and V (n = 7, 33, 64 as ragged
              orders in one tile of 128, r = 1 and 5)
  invariance  bit for bit: Upper and row-major tensors = Lower, r vectors at once = r calls with one, the position in
              the batch with failing neighbours, a repeated call
  round trip  chud then chdd with the same V returns L within the downdate bound
  failure     downdates that leave a minor indefinite (info exact, columns before vectors), an exact zero on the
              diagonal ahead of everything else, a NaN in V: the matrix's A and all of V unchanged, the neighbours'
              bits what they get alone, the return value the first failing b + 1
  footprint   NaN-filled buffers, odd lda / ldv, gaps, the base one element off: everything outside the triangles and
              all of V comes back bit for bit
  and the batch of 70001, the argument errors with their positions, the zero sizes and the statistics.

Images, raw and the small helpers are test_gpu_potrf_batched.py's, the tile call is test_gpu_chud.py's run."""
import ctypes as C

import numpy as np
import pytest

from chol_testkit import npdt, stored_lower, uplo_code
from chud_batched_model import LAPACK_BOUND, MODEL_BOUND, ORDERS, R, batch, batch_size, err_eps, padded_order, problem
from test_gpu_chud import run as tile_run
from test_gpu_potrf_batched import Images, lowers, raw, same_bits, triangle

pytestmark = pytest.mark.gpu

DT = ["d", "s"]
UPLO = ["L", "U"]
SIGMA = [1, -1]
NAME = {1: "chol_chud_batched", -1: "chol_chdd_batched"}


@pytest.fixture(scope="module")
def bt(cham):
    from dense_linear_app_amd import batched

    return batched


def fn_of(bt, sigma):
    return bt.chud_batched if sigma > 0 else bt.chdd_batched


def factor_images(L, u, dt, **kw):
    """the Lower factors L stored in the `u` triangle, NaN in the other"""
    return Images([stored_lower(l, u) for l in L], dt, **kw)


def updated(cham, bt, sigma, L, V, dt, u="L"):
    """-> the Lower factors after the call on plain images; every info must be 0"""
    ia, iv = factor_images(L, u, dt), Images(V, dt)
    assert not fn_of(bt, sigma)(ia.view, iv.view, uplo_code(cham, u)).any()
    return lowers(ia.read(), u)


# ---------------------------------------------------------------- numerics
@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_against_model_and_lapack(cham, bt, n, dt, u, sigma):
    start, V, Lm, ref = batch(n, sigma, dt)
    ia, iv = factor_images(start, u, dt), Images(V, dt)
    assert not fn_of(bt, sigma)(ia.view, iv.view, uplo_code(cham, u)).any()
    L = lowers(ia.read(), u)
    k = 0 if sigma > 0 else 1
    em, el = err_eps(L, Lm, dt), err_eps(L, ref, dt)
    print(f"n={n} {dt} {u} sigma={sigma}: {em:.2f} eps from the model, {el:.2f} eps from LAPACK")
    assert em <= MODEL_BOUND[k], em
    assert el <= LAPACK_BOUND[dt][k], el
    assert ia.kept_outside(triangle(n, u))  # (NaN there: nothing of it was read either)
    assert same_bits(iv.flat(), iv.host)  # V is only read


@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("n", [7, 33, 64])
def test_bits_of_the_tile_routine(cham, bt, n, r, dt, sigma):
    start, V, _, _ = batch(n, sigma, dt, r, 2)
    L = updated(cham, bt, sigma, start, V, dt)
    for b in range(2):
        info, T, *_ = tile_run(cham, sigma, start[b], V[b], 128, "L", dt)
        assert info == 0
        assert same_bits(L[b], T), b


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_upper_and_row_major_return_lowers_bits(cham, bt, n, dt, sigma):
    start, V, _, _ = batch(n, sigma, dt)
    F = updated(cham, bt, sigma, start, V, dt)
    assert same_bits(updated(cham, bt, sigma, start, V, dt, "U"), F)
    for u in UPLO:  # a row-major tensor: the column-major image of the transpose, seen through .mT
        ra, iv = Images([stored_lower(l, u).T for l in start], dt), Images(V, dt)
        T = ra.view.mT
        assert n == 1 or T.stride(-1) == 1
        assert not fn_of(bt, sigma)(T, iv.view, uplo_code(cham, u)).any()
        assert same_bits(lowers(ra.read().transpose(0, 2, 1), u), F), u


@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_vectors_at_once_and_one_by_one(cham, bt, n, dt, sigma):
    start, V, _, _ = batch(n, sigma, dt)
    F = updated(cham, bt, sigma, start, V, dt)
    ia = factor_images(start, "L", dt)
    for t in range(R):
        one = Images(V[:, :, t:t + 1], dt)
        assert not fn_of(bt, sigma)(ia.view, one.view[:, :, 0]).any()  # (batch, n): contiguous vectors
    assert same_bits(lowers(ia.read(), "L"), F)


@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_position_in_the_batch_and_repeated_calls(cham, bt, n, dt, sigma):
    """the probe first, in the middle and last of batches that are no multiple of a packing factor, the other
    matrices different and (from 5 on) one next to the first and one next to the last probe failing"""
    start, V, _, _ = batch(n, sigma, dt, R, 4)
    ref = [updated(cham, bt, sigma, start[:1], V[:1], dt)[0] for _ in range(2)]
    assert same_bits(ref[0], ref[1])
    bad = np.array(start[1])
    bad[n - 1, n - 1] = 0.0  # info = n
    for size in (2, 5, 67):
        probes = sorted({0, size // 2, size - 1})
        fails = [] if size < 5 else [1, size - 2]
        Ls = [start[1 + b % 3] for b in range(size)]
        Vs = [V[1 + b % 3] for b in range(size)]
        for p in probes:
            Ls[p], Vs[p] = start[0], V[0]
        for f in fails:
            Ls[f] = bad
        ia, iv = factor_images(Ls, "L", dt), Images(Vs, dt)
        info = fn_of(bt, sigma)(ia.view, iv.view)
        want = np.zeros(size, dtype=np.int32)
        want[fails] = n
        assert np.array_equal(info, want), size
        F = lowers(ia.read(), "L")
        for p in probes:
            assert same_bits(F[p], ref[0]), (size, p)
        for f in fails:
            assert same_bits(F[f], bad), (size, f)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_round_trip(cham, bt, n, dt):
    """chud then chdd with the same V returns L within the downdate bound"""
    start, V, _, _ = batch(n, 1, dt)
    ia, iv = factor_images(start, "L", dt), Images(V, dt)
    assert not bt.chud_batched(ia.view, iv.view).any()
    assert not bt.chdd_batched(ia.view, iv.view).any()
    e = err_eps(lowers(ia.read(), "L"), start, dt)
    print(f"round trip n={n} {dt}: {e:.2f} eps")
    assert e <= LAPACK_BOUND[dt][1], e


# ---------------------------------------------------------------- failure
def check_plan(cham, bt, n, dt, u, sigma, Ls, Vs, want):
    """the entry point itself on the matrices Ls with the vectors Vs (n x r each): info is `want` exactly, the return
    value the first failing b + 1; a failing matrix's A and all of V are unchanged; every other matrix has the bits it
    gets alone"""
    r = np.shape(Vs[0])[1]
    ia, iv = factor_images(Ls, u, dt), Images(Vs, dt)
    rc, info = raw(cham, NAME[sigma], u, dt, n, ia, iv, r)
    assert list(info) == list(want), (info, want)
    fails = [b for b, w in enumerate(want) if w]
    assert rc == (fails[0] + 1 if fails else 0)
    assert same_bits(iv.flat(), iv.host)
    assert ia.kept_outside(triangle(n, u))
    got, before = ia.read(), ia.host[ia.idx]
    for b in range(len(Ls)):
        if want[b]:
            assert same_bits(got[b], before[b]), b
        else:
            alone = updated(cham, bt, sigma, [Ls[b]], [Vs[b]], dt, u)[0]
            assert same_bits(lowers(got[b:b + 1], u)[0], alone), b


def factor(n, dt, seed=77):
    return problem(n, 1, seed + n)[2].astype(npdt(dt))


def scaled_column(L, f, j):
    return (f * L[:, j:j + 1].astype(np.float64)).astype(L.dtype)


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_failing_downdates(cham, bt, n, dt, u):
    """v = 1.001 L[:, j]: the rotations before column j are identities and d2 < 0 at column j: info j + 1 exactly;
    0.999: the downdate succeeds.  A good matrix on either side of every failing one."""
    L = factor(n, dt)
    cols = sorted({0, n // 2, n - 1})
    Ls, Vs, want = [], [], []
    for j in cols:
        Ls += [L, L]
        Vs += [scaled_column(L, 0.999, j), scaled_column(L, 1.001, j)]
        want += [0, j + 1]
    Ls.append(L), Vs.append(scaled_column(L, 0.999, cols[-1])), want.append(0)
    check_plan(cham, bt, n, dt, u, -1, Ls, Vs, want)


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
def test_failing_downdates_are_column_outer(cham, bt, dt, u):
    n = 33
    L = factor(n, dt)
    A = np.hstack([scaled_column(L, 0.999, 20), scaled_column(L, 1.001, 4), scaled_column(L, 1.001, 2)])
    check_plan(cham, bt, n, dt, u, -1, [L, L, L], [A, A[:, ::-1], A[:, [1, 2, 0]]], [3, 3, 3])
    B = np.hstack([scaled_column(L, 1.001, 20), scaled_column(L, 1.001, 4)])
    G = np.hstack([scaled_column(L, 0.999, 20), scaled_column(L, 0.999, 4)])
    check_plan(cham, bt, n, dt, u, -1, [L, L, L], [G, B, B[:, ::-1]], [0, 5, 5])


@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_zero_diagonal_and_nan(cham, bt, n, dt, u, sigma):
    """an exact zero at L_jj: info j (1-based), also when a rotation fails at an earlier column; a NaN in row i of V:
    info i + 1"""
    start, V, _, _ = batch(n, sigma, dt, R, 4)
    L = factor(n, dt)
    j, i = n // 2, (2 * n) // 3
    Z = np.array(L)
    Z[j, j] = 0.0
    early = np.hstack([scaled_column(L, 1.001, 0)] * R)  # (fails at column 1 where the diagonal has no zero)
    Zs = np.array(start[1])
    Zs[n - 1, n - 1] = 0.0
    Vn = np.array(V[2])
    Vn[i, 1] = np.nan
    Ls = [start[0], Z, start[1], Zs, start[2], start[3]]
    Vs = [V[0], early, V[1], V[1], Vn, V[3]]
    check_plan(cham, bt, n, dt, u, sigma, Ls, Vs, [0, j + 1, 0, n, i + 1, 0])


# ---------------------------------------------------------------- footprint
# (pad, gap, offset): lda and ldv odd for even and for odd n, gaps, the base one element off; and rows of a whole
# number of 16 bytes with a ragged order (n = 7, 15, 31, 63)
LAYOUTS = [(1, 5, 1), (2, 3, 1), (1, 0, 0)]


@pytest.mark.parametrize("sigma", SIGMA)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_footprint(cham, bt, n, dt, u, sigma):
    start, V, _, _ = batch(n, sigma, dt)
    F = updated(cham, bt, sigma, start, V, dt)
    tri = triangle(n, u)
    for pad, gap, offset in LAYOUTS:
        kw = dict(pad=pad, gap=gap, offset=offset)
        ia, iv = factor_images(start, u, dt, **kw), Images(V, dt, **kw)
        assert not fn_of(bt, sigma)(ia.view, iv.view, uplo_code(cham, u)).any()
        assert same_bits(lowers(ia.read(), u), F), kw
        assert ia.kept_outside(tri) and same_bits(iv.flat(), iv.host), kw


# ---------------------------------------------------------------- large batch
def test_batch_beyond_a_16_bit_grid(cham, bt):
    n, dt, size = 3, "s", 70001
    start, V, _, _ = batch(n, 1, dt, R, 8)
    F = updated(cham, bt, 1, start, V, dt)
    pick = np.arange(size) % 8
    big_a, big_v = Images(start[pick], dt), Images(V[pick], dt)
    assert not bt.chud_batched(big_a.view, big_v.view).any()
    assert same_bits(np.tril(big_a.read()), F[pick])
    st = bt.last_batched_stats()
    assert st["batch"] == size and st["per_wavefront"] == 8 and st["workgroups"] == -(-size // 32)
    assert not bt.chdd_batched(big_a.view, big_v.view).any()
    back = np.tril(big_a.read())
    assert same_bits(back, back[:8][pick])


# ---------------------------------------------------------------- arguments
def test_argument_errors_by_position(cham):
    import torch

    from dense_linear_app_amd._lib import lib

    L = lib()
    A = torch.zeros(64, dtype=torch.float64).cuda()
    V = torch.zeros(16, dtype=torch.float64).cuda()
    host = np.zeros(64)
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    good = [lo, f64, 4, 1, A.data_ptr(), 4, 16, V.data_ptr(), 4, 4, 2, None]
    for name in NAME.values():
        fn = getattr(L, name)
        assert fn(*good) == 1  # (zeros: an exact zero at L_11 of matrix 0, nothing is written)
        for pos, value, want in ((0, 0, -1), (1, 7, -2), (2, -1, -3), (3, -1, -4), (4, host.ctypes.data, -5),
                                 (4, None, -5), (5, 3, -6), (6, 15, -7), (7, host.ctypes.data, -8), (7, None, -8),
                                 (8, 3, -9), (9, 3, -10), (10, -1, -11), (7, A.data_ptr() + 8, -8),
                                 (7, A.data_ptr() + 8 * 31, -8), (2, 65, -104)):
            args = list(good)
            args[pos] = value
            assert fn(*args) == want, (name, pos, value)
        assert b"chol_chud_tile" in L.chol_last_error()
        args = list(good)
        args[3], args[9] = 3, 11  # strideV < ldv r
        assert fn(*args) == -10
    assert not A.cpu().numpy().any() and not V.cpu().numpy().any()


def test_zero_sizes_write_nothing(cham, bt):
    import torch

    from dense_linear_app_amd._lib import lib

    L = lib()
    A = torch.full((64,), float("nan"), dtype=torch.float64).cuda()
    V = torch.full((16,), float("nan"), dtype=torch.float64).cuda()
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    for name in NAME.values():
        fn = getattr(L, name)
        info = np.full(2, -7, dtype=np.int32)
        pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
        assert fn(lo, f64, 0, 1, A.data_ptr(), 1, 0, V.data_ptr(), 1, 1, 2, pinfo) == 0 and not info.any()
        info[:] = -7
        assert fn(lo, f64, 4, 0, A.data_ptr(), 4, 16, V.data_ptr(), 4, 0, 2, pinfo) == 0 and not info.any()
        assert fn(lo, f64, 4, 0, A.data_ptr(), 4, 16, None, 4, 0, 2, None) == 0
        assert fn(lo, f64, 4, 1, A.data_ptr(), 4, 16, V.data_ptr(), 4, 4, 0, None) == 0
        assert fn(lo, f64, 0, 0, None, 1, 0, None, 1, 0, 0, None) == 0
    assert np.isnan(A.cpu().numpy()).all() and np.isnan(V.cpu().numpy()).all()
    # the wrapper on empty tensors
    for fn in (bt.chud_batched, bt.chdd_batched):
        f64t = torch.float64
        assert fn(torch.empty(0, 4, 4, dtype=f64t).cuda(), torch.empty(0, 4, dtype=f64t).cuda()).shape == (0,)
        assert not fn(torch.empty(3, 0, 0, dtype=f64t).cuda(), torch.empty(3, 0, 2, dtype=f64t).cuda()).any()
        E = torch.full((3, 4, 4), float("nan"), dtype=f64t).cuda()
        assert not fn(E, torch.empty(3, 0, 4, dtype=f64t).cuda().mT).any()  # r = 0
        assert np.isnan(E.cpu().numpy()).all()


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_statistics(cham, bt, n, dt):
    size, es, tri = batch_size(n), 8 if dt == "d" else 4, n * (n + 1) // 2
    per = 64 // padded_order(n)
    for sigma in SIGMA:
        start, V, _, _ = batch(n, sigma, dt)
        updated(cham, bt, sigma, start, V, dt)
        st = bt.last_batched_stats()
        assert (st["batch"], st["n"], st["per_wavefront"]) == (size, n, per)
        assert st["workgroups"] == -(-(-(-size // per)) // 4)
        assert st["bytes"] == (2 * tri + n * R) * es * size
        assert 0 < st["kernel_ms"] <= st["total_ms"]
