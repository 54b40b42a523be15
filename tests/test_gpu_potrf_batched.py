"""The batched small-matrix Cholesky routines on the device (dense_linear_app_amd.batched: potrf_batched,
potrs_batched, posv_batched over chol_potrf_batched, chol_potrs_batched, chol_posv_batched), at the orders on both
sides of every packing boundary (potrf_batched_model.ORDERS), fp64 and fp32, Lower and Upper:

  exact       the dyadic families (parity, mirror, mod3; s_j <= 4): L and X bit for bit, nrhs in {1, 3, 8, 9, 17}
  bounds      spd_spectral(n, 1e3, .) rounded to the dtype against the componentwise theorems of
              potrf_batched_model.py: |A - L L^T| <= gamma(n+2) |L||L^T|, |B - A X| <= gamma(3n+3) |L||L^T||X|
  invariance  bit for bit: Upper = Lower transposed, row-major = column-major, the position in a batch of 1, 2, 3, 5,
              67 or 1000 matrices with a failing neighbour, a repeated call, posv = potrf then potrs, a column of X
              alone and inside nrhs = 9
  failure     exact zero pivots and NaNs at several columns and batch positions: info, the return value, the
              neighbours' bits, B untouched; the zero on a factor's diagonal in potrs
  footprint   NaN-filled buffers, lda = n + 1 and n + 3, a gap of 5 between the images, the base one element off:
              everything outside the triangles and B's entries comes back bit for bit
  and the batch of 70001, the argument errors with their positions, the zero sizes and the statistics."""
import ctypes as C

import numpy as np
import pytest

from chol_testkit import bits, lower_of, npdt, stored_lower, stored_sym, uplo_code
from potrf_batched_model import (FAMILIES, NRHS, ORDERS, SEEDS, dyadic_case, dyadic_rhs, factor_ratio, failing_case,
                                 padded_order, solve_ratio, spectral_case)

pytestmark = pytest.mark.gpu

DT = ["d", "s"]
UPLO = ["L", "U"]


@pytest.fixture(scope="module")
def bt(cham):
    from dense_linear_app_amd import batched

    return batched


class Images:
    """`batch` column-major n x m images (mats: batch x n x m) in a NaN-filled buffer on the device: lda = max(1, n) +
    pad, gap elements between the images, the first one `offset` elements into the buffer.  view: the torch tensor
    (batch, n, m) over them, strides (stride, 1, lda)"""

    def __init__(self, mats, dt, pad=0, gap=0, offset=0):
        import torch

        mats = np.asarray(mats, dtype=npdt(dt))
        batch, n, m = mats.shape
        self.lda = max(1, n) + pad
        self.stride = self.lda * m + gap
        self.offset = offset
        b, i, j = np.ogrid[:batch, :n, :m]
        self.idx = offset + b * self.stride + i + j * self.lda
        self.host = np.full(offset + batch * self.stride + 3, np.nan, dtype=npdt(dt))
        self.host[self.idx] = mats
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.view = torch.as_strided(self.dev, (batch, n, m), (self.stride, 1, self.lda), offset)
        self.ptr = self.dev.data_ptr() + offset * self.host.itemsize

    def read(self):
        return self.flat()[self.idx]

    def flat(self):
        return self.dev.cpu().numpy()

    def kept_outside(self, written):
        """the buffer outside the entries written[n x m] (True: the routine may write there) is what it was"""
        keep = np.ones(self.host.size, dtype=bool)
        keep[self.idx[:, written]] = False
        return np.array_equal(bits(self.flat()[keep]), bits(self.host[keep]))


def triangle(n, u):
    return np.tril(np.ones((n, n), dtype=bool)) if u == "L" else np.triu(np.ones((n, n), dtype=bool))


def same_bits(x, y):
    return np.array_equal(bits(np.asarray(x)), bits(np.asarray(y)))


def lowers(F, u):
    return np.stack([lower_of(f, u) for f in F])


def dyadic_batch(n, dt, per_family=2):
    """-> (A, L, seeds and families): per_family members of each family, seeds n, n + 1, .."""
    keys = [(n + s, fam) for fam in FAMILIES for s in range(per_family)]
    cases = [dyadic_case(n, seed, fam, dt) for seed, fam in keys]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), keys


def spectral_batch(n, dt, nrhs=3):
    cases = [spectral_case(n, seed, dt, nrhs) for seed in SEEDS]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])


def sym_images(A, u, dt, **kw):
    return Images([stored_sym(a, u) for a in A], dt, **kw)


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_dyadic_families_bit_for_bit(cham, bt, n, dt, u):
    A, L, keys = dyadic_batch(n, dt)
    uc = uplo_code(cham, u)
    fa = sym_images(A, u, dt)
    assert not bt.potrf_batched(fa.view, uc).any()
    assert same_bits(lowers(fa.read(), u), L)
    for nrhs in NRHS:
        XB = [dyadic_rhs(n, nrhs, seed, fam, dt) for seed, fam in keys]
        X, B = np.stack([x for x, _ in XB]), np.stack([b for _, b in XB])
        ib = Images(B, dt)
        assert not bt.potrs_batched(fa.view, ib.view, uc).any()
        assert same_bits(ib.read(), X), nrhs
        ia, ib = sym_images(A, u, dt), Images(B, dt)
        assert not bt.posv_batched(ia.view, ib.view if nrhs > 1 else ib.view[:, :, 0], uc).any()
        assert same_bits(lowers(ia.read(), u), L) and same_bits(ib.read(), X), nrhs


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_componentwise_bounds_and_posv_is_potrf_then_potrs(cham, bt, n, dt, u):
    A, B = spectral_batch(n, dt)
    uc = uplo_code(cham, u)
    fa = sym_images(A, u, dt)
    assert not bt.potrf_batched(fa.view, uc).any()
    F = lowers(fa.read(), u)
    ib = Images(B, dt)
    assert not bt.potrs_batched(fa.view, ib.view, uc).any()
    X = ib.read()
    worst_f = max(factor_ratio(A[b], F[b], dt) for b in range(len(A)))
    worst_s = max(solve_ratio(A[b], F[b], X[b], B[b], dt) for b in range(len(A)))
    print(f"n={n} {dt} {u}: {worst_f:.2f} of the factor bound, {worst_s:.2f} of the solve bound")
    assert worst_f <= 1.0 and worst_s <= 1.0
    pa, pb = sym_images(A, u, dt), Images(B, dt)
    assert not bt.posv_batched(pa.view, pb.view, uc).any()
    assert same_bits(pa.read(), fa.read()) and same_bits(pb.read(), X)


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_upper_and_row_major_return_lowers_bits(cham, bt, n, dt):
    A, B = spectral_batch(n, dt)
    ref_a, ref_b = sym_images(A, "L", dt), Images(B, dt)
    assert not bt.posv_batched(ref_a.view, ref_b.view, cham.ChamLower).any()
    F, X = lowers(ref_a.read(), "L"), ref_b.read()
    ua, ub = sym_images(A, "U", dt), Images(B, dt)
    assert not bt.posv_batched(ua.view, ub.view, cham.ChamUpper).any()
    assert same_bits(lowers(ua.read(), "U"), F) and same_bits(ub.read(), X)
    for u in UPLO:  # a row-major tensor: the column-major image of the transpose, seen through .mT
        ra, rb = Images([stored_sym(a, u).T for a in A], dt), Images(B, dt)
        T = ra.view.mT
        assert n == 1 or T.stride(-1) == 1
        assert not bt.posv_batched(T, rb.view, uplo_code(cham, u)).any()
        assert same_bits(lowers(ra.read().transpose(0, 2, 1), u), F) and same_bits(rb.read(), X), u


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_position_in_the_batch_and_repeated_calls(cham, bt, n, dt):
    """the probe at positions 0, the middle and last of batches that are no multiple of a packing factor, the other
    matrices different and (from 5 on) one next to the first and one next to the last probe failing"""
    cases = [spectral_case(n, seed, dt) for seed in SEEDS]
    A0, B0 = cases[0]
    bad = np.array(cases[1][0])
    bad[n - 1, n - 1] = -1.0  # info = n
    ref = []
    for _ in range(2):
        ia, ib = sym_images([A0], "L", dt), Images([B0], dt)
        assert not bt.posv_batched(ia.view, ib.view).any()
        ref.append((ia.read()[0], ib.read()[0]))
    assert same_bits(ref[0][0], ref[1][0]) and same_bits(ref[0][1], ref[1][1])
    F0, X0 = ref[0]
    for batch in (2, 3, 5, 67, 1000):
        probes = sorted({0, batch // 2, batch - 1})
        fails = [] if batch < 5 else [1, batch - 2]
        As = [cases[1 + b % 3][0] for b in range(batch)]
        Bs = [cases[1 + b % 3][1] for b in range(batch)]
        for p in probes:
            As[p], Bs[p] = A0, B0
        for f in fails:
            As[f] = bad
        ia, ib = sym_images(As, "L", dt), Images(Bs, dt)
        info = bt.posv_batched(ia.view, ib.view)
        want = np.zeros(batch, dtype=np.int32)
        want[fails] = n
        assert np.array_equal(info, want), batch
        F, X = ia.read(), ib.read()
        for p in probes:
            assert same_bits(F[p], F0) and same_bits(X[p], X0), (batch, p)
        for f in fails:
            assert same_bits(X[f], Bs[f]), (batch, f)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_a_column_of_x_alone_and_inside_nine(cham, bt, n, dt):
    A, B = spectral_batch(n, dt, nrhs=9)
    fa = sym_images(A, "L", dt)
    assert not bt.potrf_batched(fa.view).any()
    ib = Images(B, dt)
    assert not bt.potrs_batched(fa.view, ib.view).any()
    X = ib.read()
    for c in (0, 4, 8):
        one = Images(B[:, :, c:c + 1], dt)
        assert not bt.potrs_batched(fa.view, one.view[:, :, 0]).any()
        assert same_bits(one.read()[:, :, 0], X[:, :, c]), c


# ---------------------------------------------------------------- failure
def raw(cham, name, u, dt, n, ia, ib=None, nrhs=0, batch=None):
    """the C entry point itself -> (return value, info)"""
    from dense_linear_app_amd._lib import lib

    batch = ia.idx.shape[0] if batch is None else batch
    info = np.full(batch, -7, dtype=np.int32)
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
    code = cham.ChamRealDouble if dt == "d" else cham.ChamRealFloat
    if name == "chol_potrf_batched":
        rc = lib().chol_potrf_batched(uplo_code(cham, u), code, n, ia.ptr, ia.lda, ia.stride, batch, pinfo)
    else:
        rc = getattr(lib(), name)(uplo_code(cham, u), code, n, nrhs, ia.ptr, ia.lda, ia.stride, ib.ptr, ib.lda,
                                  ib.stride, batch, pinfo)
    return rc, info


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_failing_matrices(cham, bt, n, dt, u):
    A, L, keys = dyadic_batch(n, dt, per_family=4)  # 12 matrices
    nrhs = 3
    XB = [dyadic_rhs(n, nrhs, seed, fam, dt) for seed, fam in keys]
    X, B = np.stack([x for x, _ in XB]), np.stack([b for _, b in XB])
    cols = sorted({0, n // 2, n - 1})
    # position -> (0-based column, NaN instead of the exact zero)
    plan = {2: (cols[-1], False), 3: (cols[0], True), 7: (cols[len(cols) // 2], False), 11: (cols[-1], True)}
    Af = A.copy()
    for b, (j, nan) in plan.items():
        Af[b] = failing_case(n, keys[b][0], keys[b][1], dt, j, nan)
    want = np.zeros(len(A), dtype=np.int32)
    for b, (j, _) in plan.items():
        want[b] = j + 1
    good = [b for b in range(len(A)) if b not in plan]
    for name in ("chol_potrf_batched", "chol_posv_batched"):
        ia, ib = sym_images(Af, u, dt), Images(B, dt)
        rc, info = raw(cham, name, u, dt, n, ia, ib, nrhs)
        assert rc == 3 and np.array_equal(info, want), (name, rc, info)
        F = lowers(ia.read(), u)
        assert same_bits(F[good], L[good])
        for b, (j, _) in plan.items():
            assert same_bits(F[b][:, :j], L[b][:, :j]), (name, b)
        Xd = ib.read()
        if name == "chol_posv_batched":
            assert same_bits(Xd[good], X[good])
            assert same_bits(Xd[list(plan)], B[list(plan)])
        else:
            assert same_bits(Xd, B)
    # potrs: an exact zero on the stored diagonal
    Lz = L.copy()
    for b, (j, _) in plan.items():
        Lz[b][j, j] = 0
    ia, ib = Images([stored_lower(l, u) for l in Lz], dt), Images(B, dt)
    rc, info = raw(cham, "chol_potrs_batched", u, dt, n, ia, ib, nrhs)
    assert rc == 3 and np.array_equal(info, want)
    Xd = ib.read()
    assert same_bits(Xd[good], X[good]) and same_bits(Xd[list(plan)], B[list(plan)])
    assert same_bits(ia.flat(), ia.host)  # (the factor is only read)


# ---------------------------------------------------------------- footprint
# (pad, gap, offset): the issue's two, and rows of a whole number of 16 bytes with a ragged order (n = 7, 15, 31, 63)
LAYOUTS = [(1, 5, 1), (3, 5, 1), (1, 0, 0)]


@pytest.mark.parametrize("u", UPLO)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_footprint(cham, bt, n, dt, u):
    A, L, keys = dyadic_batch(n, dt, per_family=1)
    nrhs = 3
    XB = [dyadic_rhs(n, nrhs, seed, fam, dt) for seed, fam in keys]
    X, B = np.stack([x for x, _ in XB]), np.stack([b for _, b in XB])
    uc = uplo_code(cham, u)
    tri, allb = triangle(n, u), np.ones((n, nrhs), dtype=bool)
    for pad, gap, offset in LAYOUTS:
        kw = dict(pad=pad, gap=gap, offset=offset)
        fa = sym_images(A, u, dt, **kw)
        assert not bt.potrf_batched(fa.view, uc).any()
        assert same_bits(lowers(fa.read(), u), L) and fa.kept_outside(tri), kw
        before = fa.flat()
        ib = Images(B, dt, **kw)
        assert not bt.potrs_batched(fa.view, ib.view, uc).any()
        assert same_bits(ib.read(), X) and ib.kept_outside(allb) and same_bits(fa.flat(), before), kw
        pa, pb = sym_images(A, u, dt, **kw), Images(B, dt, **kw)
        assert not bt.posv_batched(pa.view, pb.view, uc).any()
        assert same_bits(lowers(pa.read(), u), L) and same_bits(pb.read(), X), kw
        assert pa.kept_outside(tri) and pb.kept_outside(allb), kw
        # a failing matrix writes the columns before the failing one at most, and nothing of B
        Af = A.copy()
        Af[1] = failing_case(n, keys[1][0], keys[1][1], dt, n - 1)
        qa, qb = sym_images(Af, u, dt, **kw), Images(B, dt, **kw)
        assert list(bt.posv_batched(qa.view, qb.view, uc)) == [0, n, 0]
        assert qa.kept_outside(tri) and qb.kept_outside(allb) and same_bits(qb.read()[1], B[1]), kw


# ---------------------------------------------------------------- large batch
def test_batch_beyond_a_16_bit_grid(cham, bt):
    n, dt, batch = 4, "s", 70001
    cases = [dyadic_case(n, seed, "mod3", dt) for seed in range(8)]
    rhs = [dyadic_rhs(n, 1, seed, "mod3", dt) for seed in range(8)]
    pick = np.arange(batch) % 8
    A = np.stack([stored_sym(c[0], "L") for c in cases])[pick]
    L = np.stack([c[1] for c in cases])[pick]
    X, B = np.stack([x for x, _ in rhs])[pick], np.stack([b for _, b in rhs])[pick]
    ia = Images(A, dt)
    assert not bt.potrf_batched(ia.view).any()
    assert same_bits(np.tril(ia.read()), L)
    pa, pb = Images(A, dt), Images(B, dt)
    assert not bt.posv_batched(pa.view, pb.view[:, :, 0]).any()
    assert same_bits(np.tril(pa.read()), L) and same_bits(pb.read(), X)
    st = bt.last_batched_stats()
    assert st["batch"] == batch and st["per_wavefront"] == 8 and st["workgroups"] == -(-batch // 32)


# ---------------------------------------------------------------- arguments
def test_argument_errors_by_position(cham):
    import torch

    from dense_linear_app_amd._lib import lib

    L = lib()
    A = torch.zeros(64, dtype=torch.float64).cuda()
    B = torch.zeros(16, dtype=torch.float64).cuda()
    host = np.zeros(64)
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    good = [lo, f64, 4, A.data_ptr(), 4, 16, 2, None]
    assert L.chol_potrf_batched(*good) == 1  # (zeros: the first pivot of matrix 0 fails, nothing is written)
    for pos, value, want in ((0, 0, -1), (1, 7, -2), (2, -1, -3), (3, host.ctypes.data, -4), (3, None, -4),
                             (4, 3, -5), (5, 15, -6), (6, -1, -7), (2, 65, -104)):
        args = list(good)
        args[pos] = value
        assert L.chol_potrf_batched(*args) == want, (pos, value)
    assert b"chol_potrf_batch " in L.chol_last_error() and b"descriptor" in L.chol_last_error()
    good = [lo, f64, 4, 1, A.data_ptr(), 4, 16, B.data_ptr(), 4, 4, 2, None]
    for name in ("chol_potrs_batched", "chol_posv_batched"):
        fn = getattr(L, name)
        for pos, value, want in ((0, 0, -1), (1, 7, -2), (2, -1, -3), (3, -1, -4), (4, host.ctypes.data, -5),
                                 (4, None, -5), (5, 3, -6), (6, 15, -7), (7, host.ctypes.data, -8), (7, None, -8),
                                 (8, 3, -9), (9, 3, -10), (10, -1, -11), (7, A.data_ptr() + 8, -8),
                                 (7, A.data_ptr() + 8 * 31, -8), (2, 65, -104)):
            args = list(good)
            args[pos] = value
            assert fn(*args) == want, (name, pos, value)
    assert not A.cpu().numpy().any() and not B.cpu().numpy().any()


def test_zero_sizes_write_nothing(cham, bt):
    import torch

    from dense_linear_app_amd._lib import lib

    L = lib()
    A = torch.full((64,), float("nan"), dtype=torch.float64).cuda()
    B = torch.full((16,), float("nan"), dtype=torch.float64).cuda()
    lo, f64 = cham.ChamLower, cham.ChamRealDouble
    info = np.full(2, -7, dtype=np.int32)
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int))
    assert L.chol_potrf_batched(lo, f64, 0, A.data_ptr(), 1, 0, 2, pinfo) == 0 and not info.any()
    assert L.chol_potrf_batched(lo, f64, 4, A.data_ptr(), 4, 16, 0, None) == 0
    assert L.chol_potrf_batched(lo, f64, 0, None, 1, 0, 0, None) == 0
    for name in ("chol_potrs_batched", "chol_posv_batched"):
        fn = getattr(L, name)
        assert fn(lo, f64, 0, 1, A.data_ptr(), 1, 0, B.data_ptr(), 1, 1, 2, None) == 0
        assert fn(lo, f64, 4, 1, A.data_ptr(), 4, 16, B.data_ptr(), 4, 4, 0, None) == 0
    assert L.chol_potrs_batched(lo, f64, 4, 0, A.data_ptr(), 4, 16, B.data_ptr(), 4, 0, 2, None) == 0
    assert np.isnan(A.cpu().numpy()).all() and np.isnan(B.cpu().numpy()).all()
    # the wrapper on empty tensors
    assert bt.potrf_batched(torch.empty(0, 4, 4, dtype=torch.float64).cuda()).shape == (0,)
    assert not bt.potrf_batched(torch.empty(3, 0, 0, dtype=torch.float32).cuda()).any()
    # posv with no right-hand side still factors
    Ad, Ld, _ = dyadic_case(4, 1, "mod3", "d")
    ia = Images([stored_sym(Ad, "L")], "d")
    assert L.chol_posv_batched(lo, f64, 4, 0, ia.ptr, 4, 16, None, 4, 0, 1, None) == 0
    assert same_bits(np.tril(ia.read()[0]), Ld)


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", ORDERS)
def test_statistics(cham, bt, n, dt):
    A, B = spectral_batch(n, dt)
    batch, nrhs, es = len(A), B.shape[2], 8 if dt == "d" else 4
    tri = n * (n + 1) // 2
    ia, ib = sym_images(A, "L", dt), Images(B, dt)
    per = 64 // padded_order(n)
    for fn, elements in ((lambda: bt.potrf_batched(ia.view), 2 * tri),
                         (lambda: bt.potrs_batched(ia.view, ib.view), tri + 2 * n * nrhs),
                         (lambda: bt.posv_batched(ia.view, ib.view), 2 * tri + 2 * n * nrhs)):
        fn()
        st = bt.last_batched_stats()
        assert (st["batch"], st["n"], st["per_wavefront"]) == (batch, n, per)
        assert st["workgroups"] == -(-(-(-batch // per)) // 4)
        assert st["bytes"] == elements * es * batch
        assert 0 < st["kernel_ms"] <= st["total_ms"]
