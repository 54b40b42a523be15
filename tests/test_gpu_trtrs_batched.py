"""The batched half routines on the device (dense_linear_app_amd.batched: trtrs_batched, trmm_batched, logdet_batched
over chol_trtrs_batched, chol_trmm_batched, chol_logdet_batched), at the orders on both sides of every packing boundary
(potrf_batched_model.ORDERS), fp64 and fp32, all four (uplo, trans), nrhs in {1, 3, 9}.  L is the lower factor however
it is stored; (Lower, NoTrans) and (Upper, Trans) are the forward half op(T) = L, the other two the backward half L^T.

  exact       the dyadic families with the integer X of dyadic_model.solution: trtrs returns X from op(T) X and trmm
              alpha op(T) X from X (alpha = 1, -2), bit for bit
  bounds      the model's factors of spd_spectral(n, 1e3, .) and standard normal B against the componentwise theorems
              of trtrs_batched_model.py: |B - op(T) X| <= gamma(n+1) |op(T)||X|, |C - alpha op(T) B| <=
              gamma(n+2) |alpha||op(T)||B|, |logdet - ref| <= gamma(n+4) 2 sum |log L_jj|
  invariance  bit for bit: forward then backward = potrs_batched, Upper = Lower transposed with trans flipped, a
              row-major tensor = a column-major one, a column alone = inside nrhs = 9, the position in a batch of 1, 2,
              3, 5, 67 or 1000 matrices with a failing neighbour, a repeated call; logdet of fp32 values = of the same
              values stored as fp64
  dependence  a NaN planted at b_k or z_k reaches the rows i >= k (forward) or i <= k (backward), the others keep
              their bits: a mask that multiplies by a stored zero instead of selecting fails here
  failure     exact zeros on the diagonal at several columns and batch positions in trtrs (info, the return value,
              B untouched, the neighbours' bits), the same factors in trmm (no failure), a zero, a negative and a NaN
              diagonal entry in logdet (info and a NaN value)
  footprint   NaN-filled buffers, lda = n + 1 and n + 3, a gap of 5 between the images, the base one element off: all
              of A and everything of B outside its entries comes back bit for bit, and no NaN reaches the result
  scalars     alpha == 0 with a NaN-filled B and an all-NaN A: +0 everywhere inside
  and the batch of 70001, the argument errors with their positions, the zero sizes and the statistics.

Images and same_bits are test_gpu_potrf_batched.py's."""
import ctypes as C

import numpy as np
import pytest

from chol_testkit import npdt, stored_lower, uplo_code
from test_gpu_potrf_batched import Images, same_bits
from trtrs_batched_model import (FAMILIES, ORDERS, SEEDS, dyadic_products, logdet_ratio, padded_order, spectral_factor,
                                 trmm_ratio, trtrs_ratio)

pytestmark = pytest.mark.gpu

DT = ["d", "s"]
UPLO = ["L", "U"]
TRANS = ["N", "T"]
NRHS = (1, 3, 9)


@pytest.fixture(scope="module")
def bt(cham):
    from dense_linear_app_amd import batched

    return batched


def trans_code(ch, t):
    return ch.ChamNoTrans if t == "N" else ch.ChamTrans


def forward(u, t):
    return (u == "L") == (t == "N")


def op_of(L, u, t):
    """op(T) as a whole matrix, T the `u` triangle in which the lower factor L is stored"""
    return L if forward(u, t) else L.T


def factor_images(L, u, dt, **kw):
    """the Lower factors L stored in the `u` triangle (transposed for Upper), NaN in the other"""
    return Images([stored_lower(l, u) for l in L], dt, **kw)


def trtrs(cham, bt, ia, ib, u="L", t="N"):
    return bt.trtrs_batched(ia.view, ib.view, uplo_code(cham, u), trans_code(cham, t))


def trmm(cham, bt, ia, ib, u="L", t="N", alpha=1.0):
    bt.trmm_batched(ia.view, ib.view, uplo_code(cham, u), trans_code(cham, t), alpha)


def solved(cham, bt, L, B, dt, u="L", t="N"):
    ia, ib = factor_images(L, u, dt), Images(B, dt)
    assert not trtrs(cham, bt, ia, ib, u, t).any()
    return ib.read()


def multiplied(cham, bt, L, B, dt, u="L", t="N", alpha=1.0):
    ia, ib = factor_images(L, u, dt), Images(B, dt)
    trmm(cham, bt, ia, ib, u, t, alpha)
    return ib.read()


def dyadic_batch(n, nrhs, dt, per_family=2):
    """-> (L, X, L X, L^T X): per_family members of each family, seeds n, n + 1, .."""
    cases = [dyadic_products(n, nrhs, n + s, fam, dt) for fam in FAMILIES for s in range(per_family)]
    return [np.stack([c[k] for c in cases]) for k in range(4)]


def spectral_batch(n, dt, nrhs=3):
    cases = [spectral_factor(n, seed, dt, nrhs) for seed in SEEDS]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_dyadic_families_bit_for_bit(cham, bt, n, dt, u, t):
    for nrhs in NRHS:
        L, X, LX, LtX = dyadic_batch(n, nrhs, dt)
        P = LX if forward(u, t) else LtX  # op(T) X
        ia = factor_images(L, u, dt)
        ib = Images(P, dt)
        assert not trtrs(cham, bt, ia, ib, u, t).any()
        assert same_bits(ib.read(), X), nrhs
        for alpha in (1.0, -2.0):
            ib = Images(X, dt)
            trmm(cham, bt, ia, ib, u, t, alpha)
            assert same_bits(ib.read(), npdt(dt)(alpha) * P), (nrhs, alpha)
        assert same_bits(ia.flat(), ia.host)  # A is only read


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_componentwise_bounds(cham, bt, n, dt, u, t):
    L, B = spectral_batch(n, dt)
    X = solved(cham, bt, L, B, dt, u, t)
    Cm = multiplied(cham, bt, L, B, dt, u, t, -1.5)
    worst_s = max(trtrs_ratio(op_of(L[b], u, t), X[b], B[b], dt) for b in range(len(L)))
    worst_m = max(trmm_ratio(op_of(L[b], u, t), Cm[b], B[b], -1.5, dt) for b in range(len(L)))
    print(f"n={n} {dt} {u} {t}: {worst_s:.2f} of the solve bound, {worst_m:.2f} of the product bound")
    assert worst_s <= 1.0 and worst_m <= 1.0


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_logdet_bound_and_fp32_values_as_fp64(cham, bt, n, dt):
    L, _ = spectral_batch(n, dt)
    vals = []
    for u in UPLO:
        ia = factor_images(L, u, dt, pad=1, gap=5, offset=1)
        value, info = bt.logdet_batched(ia.view)
        again, _ = bt.logdet_batched(ia.view)
        assert not info.any() and value.dtype.is_floating_point and value.element_size() == 8 and value.is_cuda
        assert same_bits(value.cpu().numpy(), again.cpu().numpy()) and same_bits(ia.flat(), ia.host)
        vals.append(value.cpu().numpy())
    assert same_bits(vals[0], vals[1])
    worst = max(logdet_ratio(vals[0][b], np.diag(L[b])) for b in range(len(L)))
    print(f"n={n} {dt}: {worst:.2f} of the logdet bound")
    assert worst <= 1.0
    wide, _ = bt.logdet_batched(factor_images(L.astype(np.float64), "L", "d").view)  # the same values as fp64
    assert same_bits(wide.cpu().numpy(), vals[0])
    rm = Images([stored_lower(l, "L").T for l in L], dt)  # row-major: only the diagonal counts
    assert same_bits(bt.logdet_batched(rm.view.mT)[0].cpu().numpy(), vals[0])


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_forward_then_backward_is_potrs(cham, bt, n, dt, u):
    L, B = spectral_batch(n, dt)
    ia, ref = factor_images(L, u, dt), Images(B, dt)
    assert not bt.potrs_batched(ia.view, ref.view, uplo_code(cham, u)).any()
    ib = Images(B, dt)
    first, second = ("N", "T") if u == "L" else ("T", "N")
    assert forward(u, first) and not forward(u, second)
    assert not trtrs(cham, bt, ia, ib, u, first).any()
    assert not trtrs(cham, bt, ia, ib, u, second).any()
    assert same_bits(ib.read(), ref.read())


@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_upper_and_row_major_return_lowers_bits(cham, bt, n, dt, t):
    L, B = spectral_batch(n, dt)
    flip = "T" if t == "N" else "N"
    X = solved(cham, bt, L, B, dt, "L", t)
    Cm = multiplied(cham, bt, L, B, dt, "L", t, -1.5)
    # Upper holds the transposed triangle: the same op(T) with trans flipped
    assert same_bits(solved(cham, bt, L, B, dt, "U", flip), X)
    assert same_bits(multiplied(cham, bt, L, B, dt, "U", flip, -1.5), Cm)
    # a row-major tensor of the same mathematical matrix, seen through .mT: the same codes from the caller
    for u, tt in (("L", t), ("U", flip)):
        ra = Images([stored_lower(l, u).T for l in L], dt)
        T = ra.view.mT
        assert n == 1 or T.stride(-1) == 1
        rb = Images(B, dt)
        assert not bt.trtrs_batched(T, rb.view, uplo_code(cham, u), trans_code(cham, tt)).any()
        assert same_bits(rb.read(), X), u
        rb = Images(B, dt)
        bt.trmm_batched(T, rb.view, uplo_code(cham, u), trans_code(cham, tt), -1.5)
        assert same_bits(rb.read(), Cm), u


@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_a_column_alone_and_inside_nine(cham, bt, n, dt, t):
    L, B = spectral_batch(n, dt, nrhs=9)
    ia = factor_images(L, "L", dt)
    X = solved(cham, bt, L, B, dt, "L", t)
    Cm = multiplied(cham, bt, L, B, dt, "L", t, -1.5)
    for c in (0, 4, 8):
        one = Images(B[:, :, c:c + 1], dt)
        assert not bt.trtrs_batched(ia.view, one.view[:, :, 0], cham.ChamLower, trans_code(cham, t)).any()
        assert same_bits(one.read()[:, :, 0], X[:, :, c]), c
        one = Images(B[:, :, c:c + 1], dt)
        bt.trmm_batched(ia.view, one.view[:, :, 0], cham.ChamLower, trans_code(cham, t), -1.5)
        assert same_bits(one.read()[:, :, 0], Cm[:, :, c]), c


@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_position_in_the_batch_and_repeated_calls(cham, bt, n, dt, t):
    """the probe at positions 0, the middle and last of batches that are no multiple of a packing factor, the other
    matrices different and (from 5 on) one next to the first and one next to the last probe failing: a zero on the
    diagonal (trtrs, logdet: also negative) and, for trmm, a NaN-filled B"""
    cases = [spectral_factor(n, seed, dt) for seed in SEEDS]
    L0, B0 = cases[0]
    bad = np.array(cases[1][0])
    bad[n - 1, n - 1] = 0.0  # info = n
    ref = []
    for _ in range(2):
        ld, _ = bt.logdet_batched(factor_images([L0], "L", dt).view)
        ref.append((solved(cham, bt, [L0], [B0], dt, "L", t)[0], multiplied(cham, bt, [L0], [B0], dt, "L", t, -1.5)[0],
                    ld.cpu().numpy()[0]))
    assert all(same_bits(x, y) for x, y in zip(ref[0], ref[1]))
    X0, C0, D0 = ref[0]
    for batch in (2, 3, 5, 67, 1000):
        probes = sorted({0, batch // 2, batch - 1})
        fails = [] if batch < 5 else [1, batch - 2]
        Ls = [cases[1 + b % 3][0] for b in range(batch)]
        Bs = [cases[1 + b % 3][1] for b in range(batch)]
        for p in probes:
            Ls[p], Bs[p] = L0, B0
        for f in fails:
            Ls[f] = bad
        want = np.zeros(batch, dtype=np.int32)
        want[fails] = n
        ia, ib = factor_images(Ls, "L", dt), Images(Bs, dt)
        assert np.array_equal(trtrs(cham, bt, ia, ib, "L", t), want), batch
        X = ib.read()
        Bn = np.array(Bs)
        Bn[fails] = np.nan
        ib = Images(Bn, dt)
        trmm(cham, bt, ia, ib, "L", t, -1.5)
        Cm = ib.read()
        ld, info = bt.logdet_batched(ia.view)
        ld = ld.cpu().numpy()
        assert np.array_equal(info, want) and np.isnan(ld[fails]).all() and not np.isnan(np.delete(ld, fails)).any()
        for p in probes:
            assert same_bits(X[p], X0) and same_bits(Cm[p], C0) and same_bits(ld[p], D0), (batch, p)
        for f in fails:
            assert same_bits(X[f], Bs[f]), (batch, f)


# ---------------------------------------------------------------- dependence
@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_a_nan_reaches_only_the_rows_that_depend_on_it(cham, bt, n, dt, u, t):
    L, B = spectral_batch(n, dt)
    X = solved(cham, bt, L, B, dt, u, t)
    Cm = multiplied(cham, bt, L, B, dt, u, t, -1.5)
    for k in sorted({0, n - 1, min(n - 1, padded_order(n) // 2), n // 2}):
        Bk = B.copy()
        Bk[1:, k, 0] = np.nan  # (matrix 0 stays clean, next to them in the wavefront)
        clean = np.arange(n) < k if forward(u, t) else np.arange(n) > k
        for got, ref in ((solved(cham, bt, L, Bk, dt, u, t), X), (multiplied(cham, bt, L, Bk, dt, u, t, -1.5), Cm)):
            assert same_bits(got[0], ref[0]) and same_bits(got[:, :, 1:], ref[:, :, 1:]), k
            assert same_bits(got[1:, clean, 0], ref[1:, clean, 0]), k
            assert np.isnan(got[1:, k, 0]).all(), k


# ---------------------------------------------------------------- failure
def raw_half(cham, name, u, t, dt, n, ia, ib, nrhs, alpha=None):
    """the C entry point itself -> (return value, info)"""
    from dense_linear_app_amd._lib import lib

    batch = ia.idx.shape[0]
    info = np.full(batch, -7, dtype=np.int32)
    code = cham.ChamRealDouble if dt == "d" else cham.ChamRealFloat
    head = (uplo_code(cham, u), trans_code(cham, t), code, n, nrhs)
    tail = (ia.ptr, ia.lda, ia.stride, ib.ptr, ib.lda, ib.stride, batch)
    if name == "chol_trmm_batched":
        return lib().chol_trmm_batched(*head, alpha, *tail), None
    return lib().chol_trtrs_batched(*head, *tail, info.ctypes.data_as(C.POINTER(C.c_int))), info


@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_zeros_on_the_diagonal(cham, bt, n, dt, u, t):
    nrhs = 3
    L, X, LX, LtX = dyadic_batch(n, nrhs, dt, per_family=4)  # 12 matrices
    P = LX if forward(u, t) else LtX
    cols = sorted({0, n // 2, n - 1})
    plan = {2: cols[-1], 3: cols[0], 7: cols[len(cols) // 2], 11: cols[-1]}  # position -> 0-based column
    Lz = L.copy()
    want = np.zeros(len(L), dtype=np.int32)
    for b, j in plan.items():
        Lz[b][j, j] = 0
        want[b] = j + 1
    good = [b for b in range(len(L)) if b not in plan]
    ia, ib = factor_images(Lz, u, dt), Images(P, dt)
    rc, info = raw_half(cham, "chol_trtrs_batched", u, t, dt, n, ia, ib, nrhs)
    assert rc == 3 and np.array_equal(info, want), (rc, info)
    got = ib.read()
    assert same_bits(got[good], X[good]) and same_bits(got[list(plan)], P[list(plan)])
    assert same_bits(ia.flat(), ia.host)
    # trmm: a zero on the diagonal is a factor like any other (still exact: an entry less in each sum)
    ib = Images(X, dt)
    rc, _ = raw_half(cham, "chol_trmm_batched", u, t, dt, n, ia, ib, nrhs, alpha=-2.0)
    assert rc == 0
    exact = np.stack([op_of(l, u, t).astype(np.float64) @ x.astype(np.float64) for l, x in zip(Lz, X)])
    assert same_bits(ib.read(), (-2.0 * exact).astype(npdt(dt)))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_logdet_failures(cham, bt, n, dt):
    L = np.stack([spectral_factor(n, seed % 4, dt)[0] for seed in range(12)])
    cols = sorted({0, n // 2, n - 1})
    plan = {1: [(cols[-1], 0.0)], 4: [(cols[0], -1.0)], 6: [(cols[len(cols) // 2], np.nan)],
            10: [(cols[-1], np.nan), (cols[0], -2.0)]}
    M = L.copy()
    want = np.zeros(len(L), dtype=np.int32)
    for b, planted in plan.items():
        for j, v in planted:
            M[b][j, j] = v
        want[b] = min(j for j, _ in planted) + 1
    ref, _ = bt.logdet_batched(factor_images(L, "L", dt).view)
    value, info = bt.logdet_batched(factor_images(M, "L", dt).view)
    ref, value = ref.cpu().numpy(), value.cpu().numpy()
    assert np.array_equal(info, want)
    good = [b for b in range(len(L)) if b not in plan]
    assert np.isnan(value[list(plan)]).all() and same_bits(value[good], ref[good])
    from dense_linear_app_amd._lib import lib
    import torch

    ia = factor_images(M, "L", dt)
    out = torch.zeros(len(M), dtype=torch.float64).cuda()
    code = cham.ChamRealDouble if dt == "d" else cham.ChamRealFloat
    assert lib().chol_logdet_batched(code, n, ia.ptr, ia.lda, ia.stride, len(M), out.data_ptr(), None) == 2


# ---------------------------------------------------------------- footprint and scalars
LAYOUTS = [(1, 5, 1), (3, 5, 1), (1, 0, 0)]  # (pad, gap, offset); the last: rows of whole 16 bytes at n = 7, 15, ..


@pytest.mark.parametrize("t", TRANS)
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_footprint_and_alpha_zero(cham, bt, n, dt, u, t):
    nrhs = 3
    L, X, LX, LtX = dyadic_batch(n, nrhs, dt, per_family=1)
    P = LX if forward(u, t) else LtX
    allb = np.ones((n, nrhs), dtype=bool)
    for pad, gap, offset in LAYOUTS:
        kw = dict(pad=pad, gap=gap, offset=offset)
        ia, ib = factor_images(L, u, dt, **kw), Images(P, dt, **kw)
        assert not trtrs(cham, bt, ia, ib, u, t).any()
        assert same_bits(ib.read(), X) and ib.kept_outside(allb) and same_bits(ia.flat(), ia.host), kw
        ib = Images(X, dt, **kw)
        trmm(cham, bt, ia, ib, u, t, -2.0)
        assert same_bits(ib.read(), npdt(dt)(-2.0) * P) and ib.kept_outside(allb), kw
        assert same_bits(ia.flat(), ia.host), kw
        value, info = bt.logdet_batched(ia.view)
        assert not info.any() and not np.isnan(value.cpu().numpy()).any() and same_bits(ia.flat(), ia.host), kw
        # alpha == 0: neither A (all NaN) nor B (all NaN) is read
        na, nb = Images(np.full_like(L, np.nan), dt, **kw), Images(np.full_like(X, np.nan), dt, **kw)
        trmm(cham, bt, na, nb, u, t, 0.0)
        assert same_bits(nb.read(), np.zeros_like(X)) and nb.kept_outside(allb) and same_bits(na.flat(), na.host), kw


# ---------------------------------------------------------------- large batch
def test_batch_beyond_a_16_bit_grid(cham, bt):
    n, dt, batch = 8, "s", 70001
    cases = [dyadic_products(n, 1, seed, "mod3", dt) for seed in range(8)]
    pick = np.arange(batch) % 8
    L, X, LX, LtX = [np.stack([c[k] for c in cases])[pick] for k in range(4)]
    ia = Images(np.stack([stored_lower(c[0], "L") for c in cases])[pick], dt)
    ib = Images(LX, dt)
    assert not bt.trtrs_batched(ia.view, ib.view[:, :, 0]).any()
    assert same_bits(ib.read(), X)
    st = bt.last_batched_stats()
    assert st["batch"] == batch and st["per_wavefront"] == 8 and st["workgroups"] == -(-batch // 32)
    bt.trmm_batched(ia.view, ib.view[:, :, 0], cham.ChamLower, cham.ChamTrans)
    assert same_bits(ib.read(), LtX)
    value, info = bt.logdet_batched(ia.view)
    assert not info.any()
    value = value.cpu().numpy()
    assert same_bits(value, value[:8][pick])
    assert max(logdet_ratio(value[b], np.diag(L[b])) for b in range(8)) <= 1.0


# ---------------------------------------------------------------- arguments
def test_argument_errors_by_position(cham):
    import torch

    from dense_linear_app_amd._lib import lib

    R = lib()
    A = torch.zeros(64, dtype=torch.float64).cuda()
    B = torch.zeros(16, dtype=torch.float64).cuda()
    D = torch.zeros(2, dtype=torch.float64).cuda()
    host = np.zeros(64)
    lo, nt, f64 = cham.ChamLower, cham.ChamNoTrans, cham.ChamRealDouble
    good = [lo, nt, f64, 4, 1, A.data_ptr(), 4, 16, B.data_ptr(), 4, 4, 2, None]
    assert R.chol_trtrs_batched(*good) == 1  # (zeros: the diagonal of matrix 0 is zero, nothing is written)
    table = ((0, 0, -1), (1, 0, -2), (1, 113, -2), (2, 7, -3), (3, -1, -4), (4, -1, -5), (5, host.ctypes.data, -6),
             (5, None, -6), (6, 3, -7), (7, 15, -8), (8, host.ctypes.data, -9), (8, None, -9), (9, 3, -10),
             (10, 3, -11), (11, -1, -12), (8, A.data_ptr() + 8, -9), (8, A.data_ptr() + 8 * 31, -9), (3, 65, -104))
    for pos, value, want in table:
        args = list(good)
        args[pos] = value
        assert R.chol_trtrs_batched(*args) == want, (pos, value)
    assert b"chol_trtrs_tile" in R.chol_last_error() and b"chol_logdet_tile" in R.chol_last_error()
    good = good[:5] + [1.0] + good[5:12]
    assert R.chol_trmm_batched(*good) == 0
    for pos, value, want in table:
        args = list(good)
        args[pos + (pos >= 5)] = value
        assert R.chol_trmm_batched(*args) == (want - (pos >= 5) if want > -100 else want), (pos, value)
    assert b"chol_trmm_tile" in R.chol_last_error()
    good = [f64, 4, A.data_ptr(), 4, 16, 2, D.data_ptr(), None]
    assert R.chol_logdet_batched(*good) == 1  # (a zero diagonal: info 1 in matrix 0)
    assert np.isnan(D.cpu().numpy()).all()
    for pos, value, want in ((0, 7, -1), (1, -1, -2), (2, host.ctypes.data, -3), (2, None, -3), (3, 3, -4), (4, 15, -5),
                             (5, -1, -6), (6, host.ctypes.data, -7), (6, None, -7), (1, 65, -104)):
        args = list(good)
        args[pos] = value
        assert R.chol_logdet_batched(*args) == want, (pos, value)
    assert b"chol_logdet_tile" in R.chol_last_error()
    assert not A.cpu().numpy().any() and not B.cpu().numpy().any()


def test_zero_sizes_write_nothing(cham, bt):
    import torch

    from dense_linear_app_amd._lib import lib

    R = lib()
    A = torch.full((64,), float("nan"), dtype=torch.float64).cuda()
    B = torch.full((16,), float("nan"), dtype=torch.float64).cuda()
    D = torch.full((2,), float("nan"), dtype=torch.float64).cuda()
    lo, nt, f64 = cham.ChamLower, cham.ChamNoTrans, cham.ChamRealDouble
    info = np.full(2, -7, dtype=np.int32)
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
    assert R.chol_trtrs_batched(lo, nt, f64, 0, 1, A.data_ptr(), 1, 0, B.data_ptr(), 1, 1, 2, pinfo) == 0
    assert not info.any()
    assert R.chol_trtrs_batched(lo, nt, f64, 4, 0, A.data_ptr(), 4, 16, B.data_ptr(), 4, 0, 2, None) == 0
    assert R.chol_trtrs_batched(lo, nt, f64, 4, 1, A.data_ptr(), 4, 16, B.data_ptr(), 4, 4, 0, None) == 0
    assert R.chol_trmm_batched(lo, nt, f64, 0, 1, 2.0, A.data_ptr(), 1, 0, B.data_ptr(), 1, 1, 2) == 0
    assert R.chol_trmm_batched(lo, nt, f64, 4, 0, 2.0, A.data_ptr(), 4, 16, B.data_ptr(), 4, 0, 2) == 0
    assert R.chol_trmm_batched(lo, nt, f64, 4, 1, 0.0, A.data_ptr(), 4, 16, B.data_ptr(), 4, 4, 0) == 0
    assert R.chol_logdet_batched(f64, 4, A.data_ptr(), 4, 16, 0, D.data_ptr(), None) == 0
    assert R.chol_logdet_batched(f64, 4, None, 4, 16, 0, None, None) == 0
    assert np.isnan(A.cpu().numpy()).all() and np.isnan(B.cpu().numpy()).all() and np.isnan(D.cpu().numpy()).all()
    # the determinant of the empty matrix is 1: the one write of a zero size
    info[:] = -7
    assert R.chol_logdet_batched(f64, 0, A.data_ptr(), 1, 0, 2, D.data_ptr(), pinfo) == 0
    assert not info.any() and same_bits(D.cpu().numpy(), np.zeros(2)) and np.isnan(A.cpu().numpy()).all()
    # the wrappers on empty tensors
    E = torch.empty(3, 0, 0, dtype=torch.float32).cuda()
    value, info = bt.logdet_batched(E)
    assert value.shape == (3,) and not value.cpu().numpy().any() and not info.any()
    assert bt.trtrs_batched(torch.empty(0, 4, 4, dtype=torch.float64).cuda(),
                            torch.empty(0, 4, dtype=torch.float64).cuda()).shape == (0,)


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_statistics(cham, bt, n, dt):
    L, B = spectral_batch(n, dt)
    batch, nrhs, es = len(L), B.shape[2], 8 if dt == "d" else 4
    tri = n * (n + 1) // 2
    ia, ib = factor_images(L, "L", dt), Images(B, dt)
    per = 64 // padded_order(n)
    for fn, nbytes in ((lambda: trtrs(cham, bt, ia, ib, "L", "T"), (tri + 2 * n * nrhs) * es),
                       (lambda: trmm(cham, bt, ia, ib, "L", "N", 0.5), (tri + 2 * n * nrhs) * es),
                       (lambda: trmm(cham, bt, ia, ib, "L", "N", 0.0), n * nrhs * es),
                       (lambda: bt.logdet_batched(ia.view), n * es + 8)):
        fn()
        st = bt.last_batched_stats()
        assert (st["batch"], st["n"], st["per_wavefront"]) == (batch, n, per)
        assert st["workgroups"] == -(-(-(-batch // per)) // 4)
        assert st["bytes"] == nbytes * batch
        assert 0 < st["kernel_ms"] <= st["total_ms"]
