"""The butterfly-randomised symmetric indefinite solve on the device: CHAMELEON_{d,s}rbt_apply_Tile against the numpy
model of the four-number map (rbt_model.py) BIT FOR BIT (rbt.hip is built with floating-point contraction off and the
model mirrors its operation order, so no FMA stands between them), Lower and Upper, fp64 and fp32, depth 1 and 2, tiles
128 ... 1024, orders whose half is not a multiple of the tile, a single tile, a sub-matrix view; the other triangle and
the padding bit for bit; repeated calls bit-identical; W from a seed bit-identical and W with seed = 0 taken as given;
sytrf_rbt = rbt_apply + sytrf_nopiv; sytrs_rbt; and sysv_rbt on the matrices that sysv_nopiv cannot solve.

The bounds.  u = 2^-53.  Measured on the CPU with the committed model (sysv_rbt_model on sytrf_model, same tile size,
same W: the tests pin W with seed = 0) on exactly the 18 cases of test_sysv_families (three families x SOLVE_CASES x
nrhs 1 and 5; Upper and Lower share a model run):
    final berr = max |R(:,j)| / (||A||_inf max |X(:,j)|)     0.221 - 0.623 u
    refinement steps                                          1, every case
    unrefined backward error                                  422 - 35 100 u
    max |L| of the factor of W^T A W                          600 - 22 800
    kappa_2(A)                                                113 - 32 500
    sysv_nopiv's model on the same matrices                   info = 1 (zero_diag, saddle), 616 - 2 540 u (randsym)
The device sums in another order than the model, so it gets 10 x the model's largest final berr and the model's largest
step count + 2: BERR_U = 6.23, MAX_STEPS = 3.  The unrefined error and max |L| are printed, not bounded: they are what
refinement is for.  The device on the 36 cases: berr 0.066 - 0.335 u, 1 step each, max |L| as the model's to three
digits; sysv_nopiv on the random symmetric cases 5 880 - 468 000 u.  The model's own final berr is the rounding noise
of its residual and moves with the BLAS under numpy (up to 0.77 u), so the test holds the model to the device's bounds,
not to the range above.
The forward error: max |x - x_numpy| / max |x_numpy| per column against kappa_inf(A) x BERR_U u (the device: 0.005 - 0.15 u x kappa_inf).
sytrs_rbt alone is measured on SPD matrices (W^T A W stays SPD, so nothing grows): the model leaves 0.86 - 0.96 u
(fp64) and 0.50 - 0.58 u (fp32) on the two cases of test_sytrs_spd; 10 x the largest: SPD_SOLVE_U = 9.63 (the device:
1.02 - 1.04 u in fp64, 0.49 - 0.70 u in fp32)."""
import functools

import numpy as np
import pytest

from chol_testkit import (U, UserView, bits, desc, image_matrix, lower_of, npdt, other, other_triangle_kept,
                          ragged_padding_mask, stored_lower, uplo_code)
from rbt_model import backward_error, family, random_w, rbt_sym, sysv_rbt_model

pytestmark = pytest.mark.gpu

BERR_U = 6.23       # 10 x 0.623 u, the model's largest final berr (above)
MAX_STEPS = 3       # the model's largest step count (1) + 2
SPD_SOLVE_U = 9.63  # 10 x 0.963 u, the model's largest backward error of sytrs_rbt on the SPD cases (above)


def wdesc(ch, Wc, B, dt):
    d = desc(ch, Wc.shape[0], B, dt, Wc.shape[1])
    d.from_lapack(np.asfortranarray(Wc.astype(npdt(dt))))
    return d


def apply(ch, A, Wc, B, depth, u="L", dt="d"):
    """-> (the lower triangle of W^T A W from the device, A after the call, A as stored)"""
    S = stored_lower(A.astype(npdt(dt)), u)
    da, dw = desc(ch, A.shape[0], B, dt), wdesc(ch, Wc, B, dt)
    da.from_lapack(S)
    assert ch.CHAMELEON_drbt_apply_Tile(uplo_code(ch, u), da, dw, depth) == 0
    F, W = da.to_lapack(), dw.to_lapack()
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(dw)
    assert np.array_equal(bits(W), bits(Wc.astype(npdt(dt))))  # W only read
    return lower_of(F, u), F, S


APPLY_CASES = [(512, 128, 2), (1024, 256, 2), (1000, 256, 2), (1000, 256, 1), (1536, 1024, 2), (2048, 1024, 1),
               (512, 512, 2), (768, 384, 2), (520, 128, 1), (128, 64, 2)]


@pytest.mark.parametrize("n,B,depth", APPLY_CASES)
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_apply_bit_for_bit(cham, n, B, depth, u, dt):
    """1000 / 256 and 1536 / 1024: the half order is not a multiple of the tile; 512 / 512: a single tile; 520 / 128:
    a half order that is not a multiple of the workgroup's 64 x 64 block; 128 / 64: stored tiles larger than the
    caller's"""
    ch = cham
    A = family("randsym", n, n + B)
    Wc = random_w(n, depth, n + depth, npdt(dt))
    Lg, F, S = apply(ch, A, Wc, B, depth, u, dt)
    Lm = rbt_sym(A.astype(npdt(dt)), Wc, depth)
    diff = np.abs(Lg.astype(np.float64) - Lm.astype(np.float64)).max()
    print(f"rbt_apply {n}/{B} depth {depth} {u} {dt}: max |device - model| = {diff:.3g}")
    assert np.array_equal(bits(Lg), bits(Lm))
    assert other_triangle_kept(F, S, u)


@pytest.mark.parametrize("dt", ["d", "s"])
def test_apply_integer_exact(cham, dt):
    """entries of W equal to 1, A = 4 x small integers: both halvings are exact"""
    ch = cham
    n, B, depth = 768, 256, 2
    r = np.random.default_rng(4)
    A = r.integers(-8, 9, (n, n))
    A = 4.0 * (np.tril(A) + np.tril(A, -1).T)
    Wc = np.ones((n, depth))
    Lg, _, _ = apply(ch, A, Wc, B, depth, "L", dt)
    assert np.array_equal(Lg, rbt_sym(A.astype(npdt(dt)), Wc.astype(npdt(dt)), depth))
    assert np.array_equal(Lg, np.rint(Lg))


def test_repeatable_and_padding(cham):
    """two calls give the same bits; a ragged order keeps the padding of the image bit for bit"""
    ch = cham
    n, B, nt, depth = 1000, 256, 4, 2
    pad = ragged_padding_mask(n, B, nt)
    A = family("zero_diag", n, 2)
    Wc = random_w(n, depth, 3)
    outs = []
    for _ in range(2):
        da, dw = desc(ch, n, B, "d"), wdesc(ch, Wc, B, "d")
        da.from_lapack(stored_lower(A, "L"))
        before = image_matrix(da, nt, B, np.float64)
        assert ch.CHAMELEON_drbt_apply_Tile(ch.ChamLower, da, dw, depth) == 0
        outs.append(da.to_lapack())
        after = image_matrix(da, nt, B, np.float64)
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(dw)
        assert np.array_equal(bits(after[pad]), bits(before[pad]))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


def test_sub_matrix_view(cham):
    """a tile-aligned view of a device user buffer gives the whole-matrix descriptor's result; the user's tiles outside
    the view stay as they were"""
    ch = cham
    uv, depth = UserView(ch), 2
    mb, m = uv.mb, uv.m
    A = family("saddle", m, 6)
    Wc = random_w(m, depth, 7)
    v = uv.view_desc()
    v.from_lapack(stored_lower(A, "L"))
    dw = wdesc(ch, Wc, mb, "d")
    assert ch.CHAMELEON_drbt_apply_Tile(ch.ChamLower, v, dw, depth) == 0
    Lv = np.tril(v.to_lapack())
    ch.CHAMELEON_Desc_Destroy(v)
    ch.CHAMELEON_Desc_Destroy(dw)
    assert np.array_equal(bits(Lv), bits(rbt_sym(A, Wc, depth)))
    uv.outside_unchanged()


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_sytrf_rbt_seed_and_composition(cham, u, dt):
    """W from a seed: the same bits on a second call, entries exp(r / 10) with |r| <= 1/2, another seed another W; and
    sytrf_rbt with seed = 0 takes W as given: with the W read back from the seeded run it returns the seeded run's
    factor, which is rbt_apply followed by sytrf_nopiv, bit for bit"""
    ch = cham
    n, B, depth = 1024, 256, 2
    A = family("saddle", n, 31).astype(npdt(dt))
    S = stored_lower(A, u)

    def run(seed, Win=None):
        da, dw = desc(ch, n, B, dt), desc(ch, n, B, dt, depth)
        da.from_lapack(S)
        dw.from_lapack(np.asfortranarray(np.full((n, depth), 7.0) if Win is None else Win))
        info = ch.CHAMELEON_dsytrf_rbt_Tile(uplo_code(ch, u), da, dw, depth, seed)
        F, W, st = da.to_lapack(), dw.to_lapack(), ch.last_sytrf_stats()
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(dw)
        return info, F, W, st

    info, F, W, st = run(5)
    info2, F2, W2, _ = run(5)
    assert info == 0 == info2
    assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(F), bits(F2))
    lo, hi = np.exp(-0.05), np.exp(0.05)
    assert W.min() >= npdt(dt)(lo) * (1 - 2 * U[dt]) and W.max() <= npdt(dt)(hi) * (1 + 2 * U[dt])
    assert W.std() > 0.02 and not np.array_equal(W[:, 0], W[:, 1])
    assert not np.array_equal(run(6)[2], W)
    info3, F3, W3, _ = run(0, W)
    assert info3 == 0 and np.array_equal(bits(W3), bits(W)) and np.array_equal(bits(F3), bits(F))
    assert other_triangle_kept(F, S, u)
    # the composition
    da, dw = desc(ch, n, B, dt), wdesc(ch, W, B, dt)
    da.from_lapack(S)
    assert ch.CHAMELEON_drbt_apply_Tile(uplo_code(ch, u), da, dw, depth) == 0
    assert np.array_equal(bits(lower_of(da.to_lapack(), u)), bits(rbt_sym(A, W, depth)))
    assert ch.CHAMELEON_dsytrf_nopiv_Tile(uplo_code(ch, u), da) == 0
    assert np.array_equal(bits(da.to_lapack()), bits(F))
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(dw)
    if dt == "d":  # (fp32 with max |L| in the thousands does not pin the signs of the smallest pivots)
        ev = np.linalg.eigvalsh(A.astype(np.float64))
        assert st["inertia"] == (int((ev > 0).sum()), int((ev < 0).sum()))
    rs = ch.last_rbt_stats()
    assert rs["steps"] == 0 and rs["solve_ms"] == 0


@pytest.mark.parametrize("n,B,depth", [(1024, 256, 2), (1000, 128, 1)])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_sytrs_spd(cham, n, B, depth, u, dt):
    """sytrf_rbt + sytrs_rbt on an SPD matrix (W^T A W is SPD: no growth), three right-hand sides; A and W only read by
    the solve"""
    ch = cham
    r = np.random.default_rng(n)
    G = r.standard_normal((n, n))
    A = (G @ G.T / n + np.eye(n)).astype(npdt(dt))
    b = r.standard_normal((n, 3)).astype(npdt(dt))
    Wc = random_w(n, depth, n + depth, npdt(dt))
    da, dw, db = desc(ch, n, B, dt), wdesc(ch, Wc, B, dt), desc(ch, n, B, dt, 3)
    da.from_lapack(stored_lower(A, u))
    db.from_lapack(np.asfortranarray(b))
    assert ch.CHAMELEON_dsytrf_rbt_Tile(uplo_code(ch, u), da, dw, depth, 0) == 0
    assert ch.last_sytrf_stats()["inertia"] == (n, 0)
    F0 = da.to_lapack()
    assert ch.CHAMELEON_dsytrs_rbt_Tile(uplo_code(ch, u), da, dw, depth, db) == 0
    assert np.array_equal(bits(da.to_lapack()), bits(F0))
    assert np.array_equal(bits(dw.to_lapack()), bits(Wc))
    x = db.to_lapack()
    for d in (da, dw, db):
        ch.CHAMELEON_Desc_Destroy(d)
    be = backward_error(A, x, b).max()
    print(f"sytrs_rbt SPD {n}/{B} depth {depth} {u} {dt}: backward error {be / U[dt]:.2f} u")
    assert be <= SPD_SOLVE_U * U[dt], be / U[dt]


SOLVE_CASES = [(1024, 256, 2), (1536, 512, 2), (1000, 128, 1)]


@functools.lru_cache(maxsize=None)
def solve_case(name, n, B, depth, nrhs):
    A = family(name, n, n + nrhs)
    b = np.random.default_rng(n + 100 + nrhs).standard_normal((n, nrhs))
    Wc = random_w(n, depth, n + depth)
    return A, b, Wc, sysv_rbt_model(A, Wc, depth, B, b)


@pytest.mark.parametrize("name", ["zero_diag", "saddle", "randsym"])
@pytest.mark.parametrize("n,B,depth", SOLVE_CASES)
@pytest.mark.parametrize("nrhs", [1, 5])
@pytest.mark.parametrize("u", ["L", "U"])
def test_sysv_families(cham, name, n, B, depth, nrhs, u):
    """side by side: sysv_nopiv stops (info > 0) or leaves a backward error above the bound; sysv_rbt returns 0 with
    berr within the bound, X within cond x bound of numpy's solve, and the inertia of A"""
    ch = cham
    A, b, Wc, m = solve_case(name, n, B, depth, nrhs)
    # (the model itself stays inside the device's bounds on every case; its final berr is rounding noise of the
    # residual and moves with the BLAS that numpy runs on)
    assert m["info"] == 0 and 0 <= m["iter"] <= MAX_STEPS and m["berr"].max() <= BERR_U * U["d"]
    S = stored_lower(A, u)
    # without the butterflies
    da, db = desc(ch, n, B, "d"), desc(ch, n, B, "d", nrhs)
    da.from_lapack(S)
    db.from_lapack(np.asfortranarray(b))
    info0 = ch.CHAMELEON_dsysv_nopiv_Tile(uplo_code(ch, u), da, db)
    be_nopiv = np.inf if info0 else backward_error(A, db.to_lapack(), b).max()
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(db)
    assert info0 > 0 or be_nopiv > BERR_U * U["d"], (info0, be_nopiv / U["d"])
    # with them
    da, daf, dw = desc(ch, n, B, "d"), desc(ch, n, B, "d"), wdesc(ch, Wc, B, "d")
    db, dx = desc(ch, n, B, "d", nrhs), desc(ch, n, B, "d", nrhs)
    da.from_lapack(S)
    daf.from_lapack(np.asfortranarray(np.full((n, n), -7.0)))
    db.from_lapack(np.asfortranarray(b))
    info, it, berr = ch.CHAMELEON_dsysv_rbt_Tile(uplo_code(ch, u), da, daf, dw, depth, 0, db, dx)
    x, AF = dx.to_lapack(), daf.to_lapack()
    st, rs = ch.last_sytrf_stats(), ch.last_rbt_stats()
    assert np.array_equal(bits(da.to_lapack()), bits(S)) and np.array_equal(bits(db.to_lapack()), bits(b))
    assert np.array_equal(bits(dw.to_lapack()), bits(Wc))
    for d in (da, daf, dw, db, dx):
        ch.CHAMELEON_Desc_Destroy(d)
    be = backward_error(A, x, b)
    print(f"sysv_rbt {name} {n}/{B} depth {depth} nrhs {nrhs} {u}: nopiv "
          f"{'info %d' % info0 if np.isinf(be_nopiv) else '%.3g u' % (be_nopiv / U['d'])}; rbt iter {it}, berr "
          f"{max(berr) / U['d']:.3g} u (model {m['berr'].max() / U['d']:.3g} u, iter {m['iter']}, unrefined "
          f"{m['berr0'].max() / U['d']:.3g} u), max |L| {st['max_abs_l']:.3g} (model {m['max_l']:.3g}), stats {rs}")
    assert info == 0 and 0 <= it <= MAX_STEPS and it == rs["steps"]
    assert max(berr) <= BERR_U * U["d"], max(berr) / U["d"]
    # what numpy measures (the two residuals differ by their own rounding, of the order of u, so both get the bound)
    assert be.max() <= BERR_U * U["d"], be.max() / U["d"]
    assert np.all(AF[other(n, u)] == -7.0)  # the other triangle of AF
    xr = np.linalg.solve(A, b)
    cond = np.linalg.cond(A, np.inf)
    ferr = (np.abs(x - xr).max(0) / np.abs(xr).max(0)).max()
    print(f"  forward error {ferr / U['d']:.3g} u, kappa_inf {cond:.3g}: {ferr / (cond * U['d']):.3g} u of cond")
    assert ferr <= cond * BERR_U * U["d"], (ferr, cond)
    ev = np.linalg.eigvalsh(A)
    assert st["inertia"] == (int((ev > 0).sum()), int((ev < 0).sum()))
    assert rs["total_ms"] > 0 and rs["transform_ms"] > 0 and rs["factor_ms"] > 0 and rs["resid_ms"] > 0


def test_matrix_of_zeros(cham):
    """the factorisation stops at the first pivot: iter = -3, the return value its info, X untouched"""
    ch = cham
    n, B, depth = 512, 128, 2
    da, daf, dw = desc(ch, n, B, "d"), desc(ch, n, B, "d"), wdesc(ch, random_w(n, depth, 1), B, "d")
    db, dx = desc(ch, n, B, "d", 2), desc(ch, n, B, "d", 2)
    da.from_lapack(np.zeros((n, n), order="F"))
    db.from_lapack(np.asfortranarray(np.ones((n, 2))))
    x0 = np.asfortranarray(np.full((n, 2), 3.0))
    dx.from_lapack(x0)
    info, it, _ = ch.CHAMELEON_dsysv_rbt_Tile(ch.ChamLower, da, daf, dw, depth, 0, db, dx)
    assert (info, it) == (1, -3)
    assert np.array_equal(bits(dx.to_lapack()), bits(x0))
    assert ch.CHAMELEON_dsytrf_rbt_Tile(ch.ChamLower, da, dw, depth, 9) == 1
    for d in (da, daf, dw, db, dx):
        ch.CHAMELEON_Desc_Destroy(d)


def test_argument_errors(cham):
    import ctypes as C

    from dense_linear_app_amd._lib import lib

    ch = cham
    n, B = 512, 128
    da, daf, dw = desc(ch, n, B, "d"), desc(ch, n, B, "d"), desc(ch, n, B, "d", 2)
    db, dx = desc(ch, n, B, "d", 3), desc(ch, n, B, "d", 3)
    L = lib()
    LO = ch.ChamLower
    it = C.c_int(0)
    assert L.chol_rbt_apply_tile(7, da.handle, dw.handle, 2) == -1
    assert L.chol_rbt_apply_tile(LO, None, dw.handle, 2) == -2
    assert L.chol_rbt_apply_tile(LO, da.handle, None, 2) == -3
    assert L.chol_rbt_apply_tile(LO, da.handle, da.handle, 2) == -3  # W aliasing A
    assert L.chol_rbt_apply_tile(LO, da.handle, dw.handle, 0) == -4
    assert L.chol_rbt_apply_tile(LO, da.handle, dw.handle, 3) == -4
    assert L.chol_sytrf_rbt_tile(7, da.handle, dw.handle, 2, 1) == -1
    assert L.chol_sytrf_rbt_tile(LO, None, dw.handle, 2, 1) == -2
    assert L.chol_sytrf_rbt_tile(LO, da.handle, None, 2, 1) == -3
    assert L.chol_sytrf_rbt_tile(LO, da.handle, dw.handle, 5, 1) == -4
    assert L.chol_sytrs_rbt_tile(7, da.handle, dw.handle, 2, db.handle) == -1
    assert L.chol_sytrs_rbt_tile(LO, None, dw.handle, 2, db.handle) == -2
    assert L.chol_sytrs_rbt_tile(LO, da.handle, None, 2, db.handle) == -3
    assert L.chol_sytrs_rbt_tile(LO, da.handle, dw.handle, 4, db.handle) == -4
    assert L.chol_sytrs_rbt_tile(LO, da.handle, dw.handle, 2, None) == -5
    assert L.chol_sytrs_rbt_tile(LO, da.handle, dw.handle, 2, dw.handle) == -5  # B aliasing W
    sysv = L.chol_sysv_rbt_tile
    ok = [LO, da.handle, daf.handle, dw.handle, 2, 0, db.handle, dx.handle, C.byref(it), None]
    for pos, bad in ((1, 7), (2, None), (3, None), (3, da.handle), (4, None), (5, 0), (7, None), (8, None),
                     (8, db.handle), (9, None)):
        args = list(ok)
        args[pos - 1] = bad
        assert sysv(*args) == -pos, (pos, bad)
    # a W of one column does not serve depth 2; another dtype, tile size or order
    for other in (desc(ch, n, B, "d", 1), desc(ch, n, B, "s", 2), desc(ch, n, 256, "d", 2), desc(ch, 640, B, "d", 2)):
        assert L.chol_rbt_apply_tile(LO, da.handle, other.handle, 2) == -3
        ch.CHAMELEON_Desc_Destroy(other)
    rect = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, B, B, B * B, n, 2 * n, 0, 0, n, 2 * n, 1, 1)
    assert L.chol_rbt_apply_tile(LO, rect.handle, dw.handle, 2) == -2
    ch.CHAMELEON_Desc_Destroy(rect)
    assert L.chol_last_rbt_stats(None) == -1
    for d in (da, daf, dw, db, dx):
        ch.CHAMELEON_Desc_Destroy(d)


@pytest.mark.parametrize("n,depth", [(514, 2), (513, 1), (1001, 2)])
def test_order_not_a_multiple_is_refused(cham, n, depth):
    ch = cham
    B = 128
    da, dw = desc(ch, n, B, "d"), desc(ch, n, B, "d", 2)
    A = stored_lower(family("randsym", n, 1), "L", 0.0)
    da.from_lapack(A)
    for call in (lambda: ch.CHAMELEON_drbt_apply_Tile(ch.ChamLower, da, dw, depth),
                 lambda: ch.CHAMELEON_dsytrf_rbt_Tile(ch.ChamLower, da, dw, depth, 1)):
        with pytest.raises(ch.CholmiError) as e:
            call()
        assert e.value.code == -104  # CHOL_ERR_NOT_SUPPORTED
    assert np.array_equal(bits(da.to_lapack()), bits(A))  # nothing written
    ch.CHAMELEON_Desc_Destroy(da)
    ch.CHAMELEON_Desc_Destroy(dw)


def test_fp32_sysv_and_pxq_are_not_supported(cham):
    import ctypes as C

    from dense_linear_app_amd._lib import lib

    ch = cham
    n, B = 512, 128
    da, daf, dw = desc(ch, n, B, "s"), desc(ch, n, B, "s"), desc(ch, n, B, "s", 2)
    db, dx = desc(ch, n, B, "s", 1), desc(ch, n, B, "s", 1)
    it = C.c_int(0)
    assert lib().chol_sysv_rbt_tile(ch.ChamLower, da.handle, daf.handle, dw.handle, 2, 1, db.handle, dx.handle,
                                    C.byref(it), None) == -104
    for d in (da, daf, dw, db, dx):
        ch.CHAMELEON_Desc_Destroy(d)
    lib().chol_set_transport(None)
    ch.set_rank(0, 2)
    try:
        da = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, 256, 256, 256 * 256, 1024, 1024, 0, 0, 1024, 1024, 1, 2)
        dw = ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, 256, 256, 256 * 256, 1024, 2, 0, 0, 1024, 2, 1, 2)
        with pytest.raises(ch.CholmiError) as e:
            ch.CHAMELEON_dsytrf_rbt_Tile(ch.ChamLower, da, dw, 2, 1)
        assert e.value.code == -104
        ch.CHAMELEON_Desc_Destroy(da)
        ch.CHAMELEON_Desc_Destroy(dw)
    finally:
        ch.set_rank(0, 1)
