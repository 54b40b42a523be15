"""The symmetric matrix product from one stored triangle on the device: CHAMELEON_dsymm_Tile / ssymm (chol_symm_tile),
C <- alpha A B + beta C.  Both dtypes and both uplo on the shapes of symm_model.SHAPES (three and five block rows, two
128-blocks inside a tile, a ragged order with the tile edge padded to 256, one tile larger than the matrix) at
nrhs = 1, 8, 129 and 300.

A is stored as test_gpu_trtrs.py stores its factor: the other strict triangle is NaN.  On top of that the PADDING of
the stored images of A, B and C (stored rows beyond n, stored columns beyond n or nrhs) is overwritten with NaN before
every call: nothing of it may reach C.  After every call the raw stored images of A and B are bit for bit what they were
(the NaN triangle and the padding included), and so is the padding of C.

Exact: on the integer family that test_symm_host.py proves, the result is the integer result bit for bit for the
scalar pairs (1, 0), (-2, 1), (0.5, -1); with beta = 0 C holds NaN on entry; with alpha = 0 A and B hold NaN everywhere
and C comes back as beta C0 bit for bit (zeros for beta = 0).

Random family (A symmetric standard normal rounded to the dtype, B and C standard normal, alpha = -1.5, beta = 0.75),
with u = 2^-53 / 2^-24 and gamma_k = k u / (1 - k u): entry by entry
    |got - ref| <= gamma_{n+2} (|alpha| |A| |B| + |beta| |C0|),
ref formed from the rounded inputs in np.longdouble: the product bound for any summation order, with or without fma
(n products and n - 1 additions, the scaling by alpha, the product beta C0, the last addition), derived, not measured.
numpy's own product in the dtype sits at 0.003-0.016 of it on these inputs and the device at 0.004 (n = 640) to 0.041
(n = 100), so a failure is a bug.  Columns 0, 7 and 128
of an nrhs = 300 call equal the same columns of calls with nrhs = 1, 8 and 129 bit for bit, and a repeated call returns
the same bits."""
import functools

import numpy as np
import pytest

import symm_model as sm
from chol_testkit import bits, desc, gamma, npdt, put_image, pxq_refused, raw_image, stored_sym

pytestmark = pytest.mark.gpu

NS = -104  # CHOL_ERR_NOT_SUPPORTED

_PAD = {}


def padding_of(ch, n, tile, dt, cols):
    """-> bool per stored element of an n x cols image: True where it is padding (found once per geometry: the positions
    that the upload of two matrices without a common entry leaves equal)"""
    key = (n, tile, dt, cols)
    if key not in _PAD:
        d = desc(ch, n, tile, dt, cols)
        d.from_lapack(np.full((n, cols), 1.0, order="F"))
        one = raw_image(d).view(npdt(dt))
        d.from_lapack(np.full((n, cols), 2.0, order="F"))
        two = raw_image(d).view(npdt(dt))
        ch.CHAMELEON_Desc_Destroy(d)
        pad = one == two
        assert (~pad).sum() == n * cols
        _PAD[key] = pad
    return _PAD[key]


class Image:
    """an n x cols matrix on the device with NaN in all its padding; `before` is the raw stored image"""

    def __init__(self, ch, M, tile, dt):
        self.ch, self.dt = ch, dt
        n, cols = M.shape
        self.pad = padding_of(ch, n, tile, dt, cols)
        self.d = desc(ch, n, tile, dt, cols)
        self.d.from_lapack(np.asfortranarray(M, dtype=npdt(dt)))
        img = raw_image(self.d).view(npdt(dt)).copy()
        img[self.pad] = np.nan
        put_image(self.d, img.view(np.uint8))
        self.before = raw_image(self.d)

    def unchanged(self):
        return np.array_equal(raw_image(self.d), self.before)

    def padding_unchanged(self):
        w = np.uint64 if self.dt == "d" else np.uint32
        return np.array_equal(raw_image(self.d).view(w)[self.pad], self.before.view(w)[self.pad])

    def destroy(self):
        self.ch.CHAMELEON_Desc_Destroy(self.d)


class Sym:
    """A (rounded to dt) on the device in the `u` triangle, NaN in the other and in the padding; every product checks
    the images of A, B and C as the module's docstring says"""

    def __init__(self, ch, S, tile, u, dt):
        self.ch, self.u, self.dt, self.tile = ch, u, dt, tile
        self.a = Image(ch, S, tile, dt)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.a.destroy()

    def symm(self, alpha, B, beta, C0):
        ch = self.ch
        b, c = Image(ch, B, self.tile, self.dt), Image(ch, C0, self.tile, self.dt)
        uc = ch.ChamLower if self.u == "L" else ch.ChamUpper
        info = ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, uc, alpha, self.a.d, b.d, beta, c.d)
        out = c.d.to_lapack()
        same = self.a.unchanged(), b.unchanged(), c.padding_unchanged()
        b.destroy()
        c.destroy()
        assert info == 0
        assert same == (True, True, True), f"stored image changed (A, B, padding of C unchanged: {same})"
        return out


def same_bits(got, want, dt, what):
    want = np.asarray(want).astype(npdt(dt))
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), what


CASES = [pytest.param(n, tile, dt, u, id=f"{n}-{tile}-{dt}-{u}") for n, tile in sm.SHAPES for dt in "ds" for u in "LU"]


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("n,tile,dt,u", CASES)
def test_exact(cham, n, tile, dt, u):
    A, B, C = sm.exact_problem(n)
    AB = A @ B
    nan = np.full_like(C, np.nan)
    with Sym(cham, stored_sym(A, u), tile, u, dt) as S:
        for nrhs in sm.NRHS:
            for alpha, beta in sm.SCALARS:
                got = S.symm(alpha, B[:, :nrhs], beta, (nan if beta == 0 else C)[:, :nrhs])
                same_bits(got, alpha * AB[:, :nrhs] + beta * C[:, :nrhs], dt, (nrhs, alpha, beta))
    # alpha = 0: A and B are not read
    with Sym(cham, np.full((n, n), np.nan), tile, u, dt) as S:
        for nrhs in sm.NRHS:
            same_bits(S.symm(0.0, nan[:, :nrhs], -1.0, C[:, :nrhs]), -C[:, :nrhs], dt, (nrhs, "alpha = 0"))
            same_bits(S.symm(0.0, nan[:, :nrhs], 0.0, nan[:, :nrhs]), np.zeros((n, nrhs)), dt, (nrhs, "alpha = beta = 0"))


# ---------------------------------------------------------------- the random family, the columns
@functools.lru_cache(maxsize=None)
def random_reference(n, dt):
    """-> the inputs rounded to dt, alpha A B + beta C0 in np.longdouble and |alpha| |A| |B| + |beta| |C0| (read-only)"""
    alpha, beta = sm.RANDOM_SCALARS
    A, B, C = (a.astype(npdt(dt)) for a in sm.random_problem(n))
    hi = [a.astype(np.longdouble) for a in (A, B, C)]
    ref = np.longdouble(alpha) * (hi[0] @ hi[1]) + np.longdouble(beta) * hi[2]
    scale = abs(alpha) * (np.abs(hi[0]) @ np.abs(hi[1])) + abs(beta) * np.abs(hi[2])
    for a in (A, B, C, ref, scale):
        a.setflags(write=False)
    return A, B, C, ref, scale


@pytest.mark.parametrize("n,tile,dt,u", CASES)
def test_random_family_and_columns(cham, n, tile, dt, u):
    alpha, beta = sm.RANDOM_SCALARS
    A, B, C, ref, scale = random_reference(n, dt)
    got = {}
    with Sym(cham, stored_sym(A, u), tile, u, dt) as S:
        for nrhs in sm.NRHS:
            got[nrhs] = S.symm(alpha, B[:, :nrhs], beta, C[:, :nrhs])
            err = np.abs(got[nrhs].astype(np.longdouble) - ref[:, :nrhs])
            bound = gamma(n + 2, dt) * scale[:, :nrhs]
            print(f"n={n} tile={tile} {dt} {u} nrhs={nrhs}: worst error / bound {float((err / bound).max()):.4f}")
            assert np.all(err <= bound), (nrhs, float((err / bound).max()))
        again = S.symm(alpha, B, beta, C)
    wide = got[300]
    assert np.array_equal(bits(again), bits(wide))
    for col, nrhs in ((0, 1), (7, 8), (128, 129)):
        assert np.array_equal(bits(wide[:, col]), bits(got[nrhs][:, col])), (col, nrhs)


# ---------------------------------------------------------------- views, B = A
def test_c_as_a_sub_matrix_view(cham):
    """C a view over a user buffer: the product lands in the view's tiles, every other entry of the buffer is untouched"""
    import torch

    ch = cham
    mb, lt, oi, oj, vt = 128, 4, 1, 2, 2
    n = vt * mb
    A, B, C = (a[:, :n] for a in sm.exact_problem(n))
    user = np.random.default_rng(5).integers(-8, 9, size=lt * lt * mb * mb).astype(np.float64)
    buf = torch.from_numpy(user.copy()).cuda()
    lm = lt * mb
    v = ch.CHAMELEON_Desc_Create(buf, ch.ChamRealDouble, mb, mb, mb * mb, lm, lm, oi * mb, oj * mb, n, n, 1, 1)
    v.from_lapack(np.asfortranarray(C))
    held = buf.cpu().numpy().copy()
    with Sym(ch, stored_sym(A, "L"), mb, "L", "d") as S:
        plain = S.symm(-2.0, B, 1.0, C)
        b = Image(ch, B, mb, "d")
        assert ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, ch.ChamLower, -2.0, S.a.d, b.d, 1.0, v) == 0
        assert S.a.unchanged() and b.unchanged()
        b.destroy()
    same_bits(v.to_lapack(), plain, "d", "view")
    same_bits(plain, -2.0 * (A @ B) + C, "d", "plain")
    ch.CHAMELEON_Desc_Destroy(v)
    after = buf.cpu().numpy().reshape(lt, lt, mb * mb)  # [tile column][tile row]
    before = held.reshape(lt, lt, mb * mb)
    inside = np.zeros((lt, lt), dtype=bool)
    inside[oj:oj + vt, oi:oi + vt] = True
    assert np.array_equal(bits(after[~inside]), bits(before[~inside]))
    assert not np.array_equal(after[inside], before[inside])


@pytest.mark.parametrize("dt", ["d", "s"])
def test_b_may_be_a(cham, dt):
    """B = A itself (a full symmetric matrix in storage): C <- A A"""
    ch = cham
    n, tile = 384, 128
    A = sm.exact_problem(n)[0]
    a, c = Image(ch, A, tile, dt), Image(ch, np.full((n, n), np.nan), tile, dt)
    for uc in (ch.ChamLower, ch.ChamUpper):
        assert ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, uc, 1.0, a.d, a.d, 0.0, c.d) == 0
        same_bits(c.d.to_lapack(), A @ A, dt, "A A")
        assert a.unchanged() and c.padding_unchanged()
    a.destroy()
    c.destroy()


# ---------------------------------------------------------------- arguments, stats
def test_argument_errors(cham):
    ch = cham
    from dense_linear_app_amd._lib import CholmiError, lib

    n, tile, k = 512, 256, 4
    L_, LE, RI = ch.ChamLower, ch.ChamLeft, ch.ChamRight
    a, b, c = desc(ch, n, tile, "d"), desc(ch, n, tile, "d", k), desc(ch, n, tile, "d", k)
    a.from_lapack(np.asfortranarray(np.eye(n)))
    b.from_lapack(np.asfortranarray(np.ones((n, k))))
    c.from_lapack(np.asfortranarray(np.full((n, k), 3.0)))
    others = {"dtype": desc(ch, n, tile, "s", k), "order": desc(ch, n - tile, tile, "d", k),
              "tile": desc(ch, n, 128, "d", k)}
    rect, wider = desc(ch, n, tile, "d", 2 * n), desc(ch, n, tile, "d", k + 1)
    raw = lib()

    def code(*args):
        with pytest.raises(CholmiError) as e:
            ch.CHAMELEON_dsymm_Tile(*args)
        return e.value.code

    assert code(7, L_, 1.0, a, b, 0.0, c) == -1
    assert code(RI, L_, 1.0, a, b, 0.0, c) == NS
    assert code(LE, 7, 1.0, a, b, 0.0, c) == -2
    assert raw.chol_symm_tile(LE, L_, 1.0, None, b.handle, 0.0, c.handle) == -4
    assert raw.chol_symm_tile(LE, L_, 1.0, a.handle, None, 0.0, c.handle) == -5
    assert raw.chol_symm_tile(LE, L_, 1.0, a.handle, b.handle, 0.0, None) == -7
    assert code(LE, L_, 1.0, rect, b, 0.0, c) == -4  # (A is not square)
    for key, d in others.items():
        assert code(LE, L_, 1.0, a, d, 0.0, c) == -5, key
        assert code(LE, L_, 1.0, a, b, 0.0, d) == -7, key
    assert code(LE, L_, 1.0, a, b, 0.0, wider) == -7  # (another width than B's)
    assert code(LE, L_, 1.0, a, b, 0.0, b) == -7  # (C aliases B)
    assert code(LE, L_, 1.0, a, a, 0.0, a) == -7  # (C aliases A)
    assert raw.chol_last_symm_stats(None) == -1
    # nothing above touched C; the good call still works: C <- 2 I B - C
    assert np.array_equal(c.to_lapack(), np.full((n, k), 3.0))
    assert ch.CHAMELEON_dsymm_Tile(LE, L_, 2.0, a, b, -1.0, c) == 0
    assert np.array_equal(c.to_lapack(), np.full((n, k), -1.0))
    for d in [a, b, c, rect, wider] + list(others.values()):
        ch.CHAMELEON_Desc_Destroy(d)


def test_pxq_descriptor_is_not_supported(cham):
    ch = cham
    pxq_refused(ch, 3, lambda da, db, dc: ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, ch.ChamLower, 1.0, da, db, 0.0, dc))


def test_stats_return_what_the_call_did(cham):
    ch = cham
    n, tile = 384, 128
    A, B, C = sm.exact_problem(n)
    with Sym(ch, stored_sym(A, "L"), tile, "L", "d") as S:
        for nrhs, width in ((1, 16), (8, 16), (129, 128), (300, 128)):
            S.symm(1.0, B[:, :nrhs], 0.0, C[:, :nrhs])
            st = ch.last_symm_stats()
            assert (st["nrhs"], st["block_cols"]) == (nrhs, width)
            assert st["workgroups"] == -(-nrhs // width) * (n // 128)
            assert st["flops"] == 2.0 * n * n * nrhs
            assert 0 < st["kernel_ms"] <= st["total_ms"]
        S.symm(0.0, B[:, :8], 2.0, C[:, :8])
        st = ch.last_symm_stats()
        assert (st["nrhs"], st["block_cols"]) == (8, 0) and st["workgroups"] > 0
