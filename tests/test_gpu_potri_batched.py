"""The batched inverses on the device (dense_linear_app_amd.batched: trtri_batched, potri_batched, poinv_batched,
invdiag_batched over chol_trtri_batched, chol_potri_batched, chol_poinv_batched, chol_invdiag_batched), at the orders on
both sides of every packing boundary (potrf_batched_model.ORDERS), fp64 and fp32, Lower and Upper, mostly in batches of
nine to twelve matrices (partial sub-groups and more than one wavefront at every padded order; the bounds on four).
L is the lower factor however it is stored, W = inv(L), X = W^T W.

  exact       the dyadic families: trtri, potri, poinv from A and invdiag against the exact W and X, bit for bit, and
              potri = the model's product order applied to the device's W
  bounds      the model's factors of spd_spectral(n, 1e3, .) against the componentwise theorems of
              potri_batched_model.py: |L W - I| <= gamma(n+1) |L||W|, and |X - W^T W| <= gamma(n+1) |W^T||W| with W
              from a trtri_batched call on a copy
  identities  bit for bit: trtri(F) = the lower triangle of trtrs_batched(F, I), poinv(A) = potrf then potri,
              invdiag(F) = the diagonal of potri(F)
  invariance  bit for bit: Upper and row-major tensors = Lower, the position in a batch of 2, 3, 5, 67 or 259 matrices
              with failing neighbours, a repeated call
  failure     exact zeros on the diagonal at several columns and batch positions (info, the return value, that matrix
              untouched, the neighbours' bits); poinv on potrf_batched_model.failing_case: potrf's info and state
  dependence  a NaN planted at L(p,q) reaches W(k,c) for c <= q, k >= p and X(i,m) for m <= q; every other entry keeps
              its bits: a mask that multiplies by a stored zero instead of selecting fails here
  footprint   NaN-filled buffers, lda = n + 1 and n + 3, a gap of 5 between the images, the base one element off: only
              the `uplo` triangle changes; invdiag writes n elements per matrix and leaves A bit for bit
  and the batch of 70001, the argument errors with their positions, the zero sizes and the statistics.

Images and same_bits are test_gpu_potrf_batched.py's."""
import ctypes as C

import numpy as np
import pytest

from chol_testkit import chdt, npdt, stored_lower, stored_sym, uplo_code
from potri_batched_model import (FAMILIES, ORDERS, SEEDS, dyadic_inverse, failing_case, lauum_model, lauum_ratio,
                                 padded_order, spectral_inverse, trtri_ratio)
from test_gpu_potrf_batched import Images, lowers, same_bits, triangle

pytestmark = pytest.mark.gpu

DT = ["d", "s"]
UPLO = ["L", "U"]
IN_PLACE = ("trtri_batched", "potri_batched", "poinv_batched")


@pytest.fixture(scope="module")
def bt(cham):
    from dense_linear_app_amd import batched

    return batched


def factor_images(L, u, dt, **kw):
    """the Lower factors L stored in the `u` triangle (transposed for Upper), NaN in the other"""
    return Images([stored_lower(l, u) for l in L], dt, **kw)


def sym_images(A, u, dt, **kw):
    return Images([stored_sym(a, u) for a in A], dt, **kw)


def dyadic_batch(n, dt, per_family=3):
    """-> (A, L, W, X, keys): per_family members of each family, seeds n, n + 1, .."""
    keys = [(n + s, fam) for fam in FAMILIES for s in range(per_family)]
    cases = [dyadic_inverse(n, seed, fam, dt) for seed, fam in keys]
    return [np.stack([c[k] for c in cases]) for k in range(4)] + [keys]


def spectral_batch(n, dt, count=9):
    """-> (A, L): count matrices, the seeds of SEEDS in turn"""
    cases = [spectral_inverse(n, SEEDS[b % len(SEEDS)], dt) for b in range(count)]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])


def inverted(cham, bt, name, M, dt, u="L"):
    """the lower-stored results of the in-place routine `name` on the factors (poinv: the matrices) M"""
    ia = (sym_images if name == "poinv_batched" else factor_images)(M, u, dt)
    assert not getattr(bt, name)(ia.view, uplo_code(cham, u)).any()
    return lowers(ia.read(), u)


def diagonals(cham, bt, L, dt, u="L"):
    ia = factor_images(L, u, dt)
    D, info = bt.invdiag_batched(ia.view, uplo_code(cham, u))
    assert not info.any() and same_bits(ia.flat(), ia.host)  # A is only read
    assert D.shape == (len(L), L[0].shape[0]) and D.is_contiguous() and D.device == ia.view.device
    return D.cpu().numpy()


def diag_of(X):
    return np.stack([np.diag(x) for x in X])


def raw(cham, name, u, dt, n, ia, idm=None, stride_d=0):
    """the C entry point itself -> (return value, info)"""
    from dense_linear_app_amd._lib import lib

    batch = ia.idx.shape[0]
    info = np.full(batch, -7, dtype=np.int32)
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
    head = (uplo_code(cham, u), chdt(cham, dt), n, ia.ptr, ia.lda, ia.stride)
    if name == "chol_invdiag_batched":
        return lib().chol_invdiag_batched(*head, idm.ptr, stride_d, batch, pinfo), info
    return getattr(lib(), name)(*head, batch, pinfo), info


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_dyadic_families_bit_for_bit(cham, bt, n, dt, u):
    A, L, W, X, _ = dyadic_batch(n, dt)
    Wd = inverted(cham, bt, "trtri_batched", L, dt, u)
    assert same_bits(Wd, W)
    Xd = inverted(cham, bt, "potri_batched", L, dt, u)
    assert same_bits(Xd, X)
    assert same_bits(Xd, np.stack([lauum_model(w, dt) for w in Wd]))  # the model's order on the device's W
    assert same_bits(inverted(cham, bt, "poinv_batched", A, dt, u), X)
    assert same_bits(diagonals(cham, bt, L, dt, u), diag_of(X))


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_componentwise_bounds(cham, bt, n, dt, u):
    _, L = spectral_batch(n, dt, len(SEEDS))
    W = inverted(cham, bt, "trtri_batched", L, dt, u)  # (on a copy)
    X = inverted(cham, bt, "potri_batched", L, dt, u)
    worst_w = max(trtri_ratio(L[b], W[b], dt) for b in range(len(L)))
    worst_x = max(lauum_ratio(W[b], X[b], dt) for b in range(len(L)))
    print(f"n={n} {dt} {u}: {worst_w:.2f} of trtri's bound, {worst_x:.2f} of the product's")
    assert worst_w <= 1.0 and worst_x <= 1.0


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_identities_bit_for_bit(cham, bt, n, dt, u):
    A, L = spectral_batch(n, dt)
    uc = uplo_code(cham, u)
    # trtri = the forward half solve of the identity
    ia = factor_images(L, u, dt)
    ib = Images(np.stack([np.eye(n)] * len(L)), dt)
    assert not bt.trtrs_batched(ia.view, ib.view, uc, cham.ChamNoTrans if u == "L" else cham.ChamTrans).any()
    assert same_bits(inverted(cham, bt, "trtri_batched", L, dt, u), np.tril(ib.read()))
    # poinv = potrf then potri
    two = sym_images(A, u, dt)
    assert not bt.potrf_batched(two.view, uc).any()
    F = lowers(two.read(), u)
    assert not bt.potri_batched(two.view, uc).any()
    one = sym_images(A, u, dt)
    assert not bt.poinv_batched(one.view, uc).any()
    assert same_bits(one.flat(), two.flat())
    # invdiag = the diagonal of potri
    assert same_bits(diagonals(cham, bt, F, dt, u), diag_of(lowers(two.read(), u)))


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_upper_and_row_major_return_lowers_bits(cham, bt, n, dt):
    A, L = spectral_batch(n, dt)
    ref = {name: inverted(cham, bt, name, A if name == "poinv_batched" else L, dt, "L") for name in IN_PLACE}
    Dref = diagonals(cham, bt, L, dt, "L")
    assert same_bits(Dref, diag_of(ref["potri_batched"]))
    for name in IN_PLACE:
        assert same_bits(inverted(cham, bt, name, A if name == "poinv_batched" else L, dt, "U"), ref[name]), name
    assert same_bits(diagonals(cham, bt, L, dt, "U"), Dref)
    # a row-major tensor of the same mathematical matrix, seen through .mT: the same code from the caller
    for u in UPLO:
        for name in IN_PLACE:
            M = [stored_sym(a, u).T for a in A] if name == "poinv_batched" else [stored_lower(l, u).T for l in L]
            ra = Images(M, dt)
            T = ra.view.mT
            assert n == 1 or T.stride(-1) == 1
            assert not getattr(bt, name)(T, uplo_code(cham, u)).any()
            assert same_bits(lowers(ra.read().transpose(0, 2, 1), u), ref[name]), (name, u)
        ra = Images([stored_lower(l, u).T for l in L], dt)
        D, info = bt.invdiag_batched(ra.view.mT, uplo_code(cham, u))
        assert not info.any() and same_bits(D.cpu().numpy(), Dref) and same_bits(ra.flat(), ra.host), u


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_position_in_the_batch_and_repeated_calls(cham, bt, n, dt):
    """the probe at positions 0, the middle and last of batches that are no multiple of a packing factor, the other
    matrices different and (from 5 on) one next to the first and one next to the last probe failing: a zero on the
    factor's diagonal, a negative last pivot for poinv"""
    cases = [spectral_inverse(n, seed, dt) for seed in SEEDS]
    A0, L0 = cases[0][:2]
    bad_l, bad_a = np.array(cases[1][1]), np.array(cases[1][0])
    bad_l[n - 1, n - 1] = 0.0  # info = n
    bad_a[n - 1, n - 1] = -1.0  # info = n
    ref = []
    for _ in range(2):
        ref.append([inverted(cham, bt, name, [A0] if name == "poinv_batched" else [L0], dt)[0] for name in IN_PLACE]
                   + [diagonals(cham, bt, [L0], dt)[0]])
    assert all(same_bits(x, y) for x, y in zip(ref[0], ref[1]))
    for batch in (2, 3, 5, 67, 259):
        probes = sorted({0, batch // 2, batch - 1})
        fails = [] if batch < 5 else [1, batch - 2]
        As = [cases[1 + b % 3][0] for b in range(batch)]
        Ls = [cases[1 + b % 3][1] for b in range(batch)]
        for p in probes:
            As[p], Ls[p] = A0, L0
        for f in fails:
            As[f], Ls[f] = bad_a, bad_l
        want = np.zeros(batch, dtype=np.int32)
        want[fails] = n
        for name, r0 in zip(IN_PLACE, ref[0]):
            ia = sym_images(As, "L", dt) if name == "poinv_batched" else factor_images(Ls, "L", dt)
            assert np.array_equal(getattr(bt, name)(ia.view), want), (name, batch)
            got = lowers(ia.read(), "L")
            for p in probes:
                assert same_bits(got[p], r0), (name, batch, p)
        D, info = bt.invdiag_batched(factor_images(Ls, "L", dt).view)
        assert np.array_equal(info, want)
        for p in probes:
            assert same_bits(D.cpu().numpy()[p], ref[0][3]), (batch, p)


# ---------------------------------------------------------------- failure
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_zeros_on_the_diagonal(cham, bt, n, dt, u):
    A, L, W, X, _ = dyadic_batch(n, dt, per_family=4)  # 12 matrices
    cols = sorted({0, n // 2, n - 1})
    plan = {2: cols[-1], 3: cols[0], 7: cols[len(cols) // 2], 11: cols[-1]}  # position -> 0-based column
    Lz = L.copy()
    want = np.zeros(len(L), dtype=np.int32)
    for b, j in plan.items():
        Lz[b][j, j] = 0
        want[b] = j + 1
    good, failed = [b for b in range(len(L)) if b not in plan], list(plan)
    for name, ref in (("chol_trtri_batched", W), ("chol_potri_batched", X)):
        ia = factor_images(Lz, u, dt)
        rc, info = raw(cham, name, u, dt, n, ia)
        assert rc == 3 and np.array_equal(info, want), (name, rc, info)
        assert same_bits(lowers(ia.read(), u)[good], ref[good]), name
        assert same_bits(ia.read()[failed], ia.host[ia.idx][failed]) and ia.kept_outside(triangle(n, u)), name
    ia = factor_images(Lz, u, dt)
    idm = Images(np.full((len(L), n, 1), 7.0), dt)
    rc, info = raw(cham, "chol_invdiag_batched", u, dt, n, ia, idm, n)
    assert rc == 3 and np.array_equal(info, want)
    D = idm.read()[:, :, 0]
    assert same_bits(D[good], diag_of(X)[good]) and same_bits(D[failed], np.full((len(failed), n), 7.0, npdt(dt)))
    assert same_bits(ia.flat(), ia.host)


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_poinv_fails_as_potrf_does(cham, bt, n, dt, u):
    A, L, W, X, keys = dyadic_batch(n, dt, per_family=4)
    cols = sorted({0, n // 2, n - 1})
    # position -> (0-based column, NaN instead of the exact zero)
    plan = {2: (cols[-1], False), 3: (cols[0], True), 7: (cols[len(cols) // 2], False), 11: (cols[-1], True)}
    Af = A.copy()
    want = np.zeros(len(A), dtype=np.int32)
    for b, (j, nan) in plan.items():
        Af[b] = failing_case(n, keys[b][0], keys[b][1], dt, j, nan)
        want[b] = j + 1
    good, failed = [b for b in range(len(A)) if b not in plan], list(plan)
    fa, pa = sym_images(Af, u, dt), sym_images(Af, u, dt)
    rc, info = raw(cham, "chol_potrf_batched", u, dt, n, fa)
    assert rc == 3 and np.array_equal(info, want)
    rc, info = raw(cham, "chol_poinv_batched", u, dt, n, pa)
    assert rc == 3 and np.array_equal(info, want), (rc, info)
    assert same_bits(pa.read()[failed], fa.read()[failed])  # potrf's state
    assert same_bits(lowers(pa.read(), u)[good], X[good]) and pa.kept_outside(triangle(n, u))


# ---------------------------------------------------------------- dependence
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_a_nan_reaches_only_the_entries_that_depend_on_it(cham, bt, n, dt, u):
    _, L = spectral_batch(n, dt)
    W = inverted(cham, bt, "trtri_batched", L, dt, u)
    X = inverted(cham, bt, "potri_batched", L, dt, u)
    k, c = np.indices((n, n))
    low = k >= c
    h = min(n - 1, padded_order(n) // 2)
    for p, q in sorted({(0, 0), (n - 1, 0), (n // 2, n // 2), (n - 1, n // 2), (h, h // 2), (n - 1, n - 1)}):
        Ln = L.copy()
        Ln[1:, p, q] = np.nan  # (matrix 0 stays clean, next to them in the wavefront)
        for name, ref, hit in (("trtri_batched", W, low & (c <= q) & (k >= p)), ("potri_batched", X, low & (c <= q))):
            ia = factor_images(Ln, u, dt)
            assert not getattr(bt, name)(ia.view, uplo_code(cham, u)).any()
            got = lowers(ia.read(), u)
            assert same_bits(got[0], ref[0]), (name, p, q)
            assert np.isnan(got[1:, hit]).all(), (name, p, q)
            assert same_bits(got[1:, low & ~hit], ref[1:, low & ~hit]), (name, p, q)


# ---------------------------------------------------------------- footprint
LAYOUTS = [(1, 5, 1), (3, 5, 1), (1, 0, 0)]  # (pad, gap, offset); the last: rows of whole 16 bytes at n = 7, 15, ..


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_footprint(cham, bt, n, dt, u):
    A, L, W, X, _ = dyadic_batch(n, dt, per_family=1)
    tri = triangle(n, u)
    for pad, gap, offset in LAYOUTS:
        kw = dict(pad=pad, gap=gap, offset=offset)
        for name, M, ref in (("trtri_batched", L, W), ("potri_batched", L, X), ("poinv_batched", A, X)):
            ia = (sym_images if name == "poinv_batched" else factor_images)(M, u, dt, **kw)
            assert not getattr(bt, name)(ia.view, uplo_code(cham, u)).any()
            assert same_bits(lowers(ia.read(), u), ref) and ia.kept_outside(tri), (name, kw)
        # invdiag: n elements per matrix at a stride of its own, in a NaN-filled buffer; A bit for bit
        ia = factor_images(L, u, dt, **kw)
        idm = Images(np.zeros((len(L), n, 1)), dt, pad=0, gap=3, offset=offset)
        rc, info = raw(cham, "chol_invdiag_batched", u, dt, n, ia, idm, idm.stride)
        assert rc == 0 and not info.any()
        assert same_bits(idm.read()[:, :, 0], diag_of(X)) and idm.kept_outside(np.ones((n, 1), dtype=bool)), kw
        assert same_bits(ia.flat(), ia.host), kw


# ---------------------------------------------------------------- large batch
def test_batch_beyond_a_16_bit_grid(cham, bt):
    n, dt, batch = 3, "s", 70001
    cases = [dyadic_inverse(n, seed, "mod3", dt) for seed in range(8)]
    pick = np.arange(batch) % 8
    A, L, W, X = [np.stack([c[k] for c in cases])[pick] for k in range(4)]
    ia = Images(np.stack([stored_lower(c[1], "L") for c in cases])[pick], dt)
    assert not bt.trtri_batched(ia.view).any()
    assert same_bits(np.tril(ia.read()), W)
    st = bt.last_batched_stats()
    assert st["batch"] == batch and st["per_wavefront"] == 8 and st["workgroups"] == -(-batch // 32)
    ia = Images(np.stack([stored_sym(c[0], "L") for c in cases])[pick], dt)
    assert not bt.poinv_batched(ia.view).any()
    assert same_bits(np.tril(ia.read()), X)
    ia = Images(np.stack([stored_lower(c[1], "L") for c in cases])[pick], dt)
    D, info = bt.invdiag_batched(ia.view)
    assert not info.any() and same_bits(D.cpu().numpy(), diag_of(X))
    assert not bt.potri_batched(ia.view).any()
    assert same_bits(np.tril(ia.read()), X)


# ---------------------------------------------------------------- arguments
def test_argument_errors_by_position(cham):
    import torch

    from dense_linear_app_amd._lib import lib

    R = lib()
    A = torch.zeros(64, dtype=torch.float64).cuda()
    D = torch.zeros(16, dtype=torch.float64).cuda()
    host = np.zeros(64)
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    good = [lo, f64, 4, A.data_ptr(), 4, 16, 2, None]
    for name, tile in (("chol_trtri_batched", b"chol_trtri_tile"), ("chol_potri_batched", b"chol_potri_tile"),
                       ("chol_poinv_batched", b"chol_poinv_tile")):
        fn = getattr(R, name)
        assert fn(*good) == 1  # (zeros: the diagonal, or the first pivot, of matrix 0 fails; nothing is written)
        for pos, value, want in ((0, 0, -1), (1, 7, -2), (2, -1, -3), (3, host.ctypes.data, -4), (3, None, -4),
                                 (4, 3, -5), (5, 15, -6), (6, -1, -7), (2, 65, -104)):
            args = list(good)
            args[pos] = value
            assert fn(*args) == want, (name, pos, value)
        assert tile in R.chol_last_error() and b"n > 64" in R.chol_last_error()
    good = [lo, f64, 4, A.data_ptr(), 4, 16, D.data_ptr(), 4, 2, None]
    assert R.chol_invdiag_batched(*good) == 1
    for pos, value, want in ((0, 0, -1), (1, 7, -2), (2, -1, -3), (3, host.ctypes.data, -4), (3, None, -4), (4, 3, -5),
                             (5, 15, -6), (6, host.ctypes.data, -7), (6, None, -7), (7, 3, -8), (8, -1, -9),
                             (6, A.data_ptr() + 8, -7), (6, A.data_ptr() + 8 * 31, -7), (2, 65, -104)):
        args = list(good)
        args[pos] = value
        assert R.chol_invdiag_batched(*args) == want, (pos, value)
    assert b"chol_potri_tile" in R.chol_last_error()
    assert not A.cpu().numpy().any() and not D.cpu().numpy().any()


def test_zero_sizes_write_nothing(cham, bt):
    import torch

    from dense_linear_app_amd._lib import lib

    R = lib()
    A = torch.full((64,), float("nan"), dtype=torch.float64).cuda()
    D = torch.full((16,), float("nan"), dtype=torch.float64).cuda()
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    info = np.full(2, -7, dtype=np.int32)
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
    for name in ("chol_trtri_batched", "chol_potri_batched", "chol_poinv_batched"):
        fn = getattr(R, name)
        info[:] = -7
        assert fn(lo, f64, 0, A.data_ptr(), 1, 0, 2, pinfo) == 0 and not info.any()
        assert fn(lo, f64, 4, A.data_ptr(), 4, 16, 0, None) == 0
        assert fn(lo, f64, 0, None, 1, 0, 0, None) == 0
    info[:] = -7
    assert R.chol_invdiag_batched(lo, f64, 0, A.data_ptr(), 1, 0, D.data_ptr(), 0, 2, pinfo) == 0 and not info.any()
    assert R.chol_invdiag_batched(lo, f64, 4, A.data_ptr(), 4, 16, D.data_ptr(), 4, 0, None) == 0
    assert R.chol_invdiag_batched(lo, f64, 0, None, 1, 0, None, 0, 0, None) == 0
    assert np.isnan(A.cpu().numpy()).all() and np.isnan(D.cpu().numpy()).all()
    # the wrappers on empty tensors
    for name in IN_PLACE:
        assert getattr(bt, name)(torch.empty(0, 4, 4, dtype=torch.float64).cuda()).shape == (0,)
        assert not getattr(bt, name)(torch.empty(3, 0, 0, dtype=torch.float32).cuda()).any()
    Dd, info = bt.invdiag_batched(torch.empty(3, 0, 0, dtype=torch.float32).cuda())
    assert Dd.shape == (3, 0) and Dd.dtype == torch.float32 and not info.any()
    Dd, info = bt.invdiag_batched(torch.empty(0, 4, 4, dtype=torch.float64).cuda())
    assert Dd.shape == (0, 4) and info.shape == (0,)


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_statistics(cham, bt, n, dt):
    A, L = spectral_batch(n, dt)
    batch, es = len(L), 8 if dt == "d" else 4
    tri = n * (n + 1) // 2
    per = 64 // padded_order(n)
    for name, elements in (("trtri_batched", 2 * tri), ("potri_batched", 2 * tri), ("poinv_batched", 2 * tri),
                           ("invdiag_batched", tri + n)):
        ia = sym_images(A, "L", dt) if name == "poinv_batched" else factor_images(L, "L", dt)
        getattr(bt, name)(ia.view)
        st = bt.last_batched_stats()
        assert (st["batch"], st["n"], st["per_wavefront"]) == (batch, n, per), name
        assert st["workgroups"] == -(-(-(-batch // per)) // 4)
        assert st["bytes"] == elements * es * batch, name
        assert 0 < st["kernel_ms"] <= st["total_ms"]
