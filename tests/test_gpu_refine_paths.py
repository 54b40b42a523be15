"""The refinement loop of porfs / posvx (spd.hip: porfs_impl, groups_of, apply_inv; refine.hip: k_porfs_resid,
k_porfs_reduce, k_gather, k_scatter, k_vec_weight, k_msweep_*) on a factor that is wrong on purpose, against scipy's
dposvx / sposvx given the same bits and against the long-double model of refine_model.py.

With AF the factor of another matrix the columns leave the loop one by one and by all three exits (refine_model.py):
|rho| = 0.7 stagnates after one correction, |rho| in {0.3, 0.4} is stopped by the iteration limit after five, the
generic columns converge, a zero right-hand side gives berr = 1.  After the second pass the active set is a scattered
third of the columns, so count[j], lstres[j], the shrinking `active` list and the VecCols slot / column mapping all
matter: a wrong index gives another column's berr, a correction added to another column or one correction too many,
each 30 % or more away in berr and 1e-5 or more in X.  nrhs = 1, 3, 19 run the NR = 1, 4 and 8 kernels on such sets;
nrhs = 57 starts on the potrs path (more than POSVX_KX = 40 active columns) and is handed to the sweeps by pass 2.

Tolerances.  X and berr against the model: ten times LAPACK's own distance from the model on the same A, AF and
triangle (the largest over the 57 columns of the family, recomputed here; test_refine_model_host.py bounds it).  Both
are roundings of the same exact trajectory, summed in different orders.  ferr against LAPACK's: 1e-6 (fp64) / 1e-4
(fp32), the project's figures for estimator comparisons (test_gpu_posvx.py), unless LAPACK's Lower and Upper runs on
these bits already differ by more for that kind of column: then ten times that difference.  It does for the columns
whose final residual is rounding noise (fp64, generic: 1.5e-4; fp32, generic and iteration limit: about 1e-4), where
ferr = || |A^-1| (|R| + (n + 1) eps W) || / max |x| inherits the noise of R.

Measured on an MI355X, the largest over all cases (`pytest -s` prints every case):
                                     fp64                       fp32
    LAPACK against the model         X 1.2e-14  berr 9.6e-12    X 6.5e-6  berr 5.1e-3    (refine_model.X_DEV, BERR_DEV)
    device against the model         X 1.1e-14  berr 9.5e-12    X 2.4e-6  berr 3.8e-3    (at most 0.30 of the tolerance)
    device ferr against LAPACK's
      stagnating                     9.6e-15                    4.5e-6
      iteration limit                2.5e-12                    7.2e-5    (LAPACK Lower against Upper: up to 4.6e-5)
      generic                        1.2e-4                     1.2e-4    (LAPACK Lower against Upper: 1.5e-4, 8.7e-5)
    device ferr / true error         62 or more                 85 or more
The generic columns are the only ones whose ferr misses 1e-6 / 1e-4, by as much as LAPACK's own two triangles differ:
their R is nothing but rounding noise, and the estimator's weight |R| + (n + 1) eps W carries a thousandth of it.
"""
import functools

import numpy as np
import pytest
import scipy.linalg.lapack as lapack

import refine_model as rm
from chol_testkit import bits, desc, stored_lower, uplo_code

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 192), (1024, 256)]
NMAX = 57
FERR_TOL = {"d": 1e-6, "s": 1e-4}
RCOND_TOL = {"d": 1e-6, "s": 1e-4}


def scaling(n, dt):
    """S for equed = 'Y': powers of two 2^-3 .. 2^3 in a cycle, so that every scaling is exact"""
    return (2.0 ** ((np.arange(n) % 7) - 3)).astype(rm.NPT[dt])


@functools.lru_cache(maxsize=None)
def model(n, dt):
    """the trajectory of the 57-column problem from the fp64 first solve; fewer columns are a prefix"""
    A, AF, B, Xt, kinds = rm.problem(n, NMAX, dt)
    return rm.trajectory(A, AF, B, rm.first_solve(AF, B))


@functools.lru_cache(maxsize=None)
def lapack_run(n, dt, u, equed="N"):
    """scipy's xPOSVX, fact = 'F', on the 57-column problem: dict of X, rcond, ferr, berr, info and, from the model,
    its distances dx (relative to max |x| of the column) and db (relative, the columns that do not simply converge)"""
    A, AF, B, Xt, kinds = rm.problem(n, NMAX, dt)
    fn = lapack.dposvx if dt == "d" else lapack.sposvx
    af = AF if u == "L" else np.asfortranarray(AF.T)
    if equed == "Y":
        S = scaling(n, dt)
        out = fn(A, np.asfortranarray(B / S[:, None]), fact="F", af=af, equed="Y", s=S, lower=int(u == "L"))
        assert np.array_equal(bits(out[4]), bits(B))
    else:
        out = fn(A, B, fact="F", af=af, equed="N", lower=int(u == "L"))
    r = dict(zip(("X", "rcond", "ferr", "berr", "info"), out[5:10]))
    r.update(distances(r["X"] / scaling(n, dt)[:, None] if equed == "Y" else r["X"], r["berr"], model(n, dt), kinds))
    # (the tolerances are multiples of these: a model that LAPACK itself does not follow must not widen them)
    assert r["info"] == 0 and r["dx"].max() <= rm.X_DEV[dt] and r["db"].max() <= rm.BERR_DEV[dt], (r["dx"], r["db"])
    return r


def distances(X, berr, tr, kinds):
    kinds = np.array(kinds)
    hard = (kinds != "zero") & (kinds != "generic")
    xm = np.where(kinds == "zero", 1, np.abs(tr.X).max(axis=0))
    dx = np.abs(X - tr.X).max(axis=0) / xm
    db = np.where(hard, np.abs(berr - tr.final_berr) / tr.final_berr, 0)
    return dict(dx=dx, db=db)


def ferr_tolerance(n, dt, kinds):
    """per column: FERR_TOL, or ten times the relative difference of LAPACK's own Lower and Upper ferr over the
    columns of the same kind, where that is more"""
    allk = np.array(rm.problem(n, NMAX, dt)[4])
    fl, fu = lapack_run(n, dt, "L")["ferr"], lapack_run(n, dt, "U")["ferr"]
    tol = {}
    for k in ("stagnating", "itmax", "generic"):
        m = allk == k
        tol[k] = max(FERR_TOL[dt], 10 * (np.abs(fl - fu)[m] / fl[m]).max())
    return np.array([tol.get(k, 0.0) for k in kinds])


class Device:
    """the descriptors of one problem on the device: A and AF with the other strict triangle NaN"""

    def __init__(self, ch, N, T, u, dt, A, AF, B, X0=None, S=None):
        self.ch, self.u = ch, uplo_code(ch, u)
        nrhs = B.shape[1]
        self.dA, self.dAF, self.dS, self.dB, self.dX = (desc(ch, N, T, dt, nc) for nc in (N, N, 1, nrhs, nrhs))
        self.A0, self.AF0, self.B0 = stored_lower(A, u), stored_lower(AF, u), np.asfortranarray(B)
        self.dA.from_lapack(self.A0)
        self.dAF.from_lapack(self.AF0)
        self.dB.from_lapack(self.B0)
        self.dX.from_lapack(np.asfortranarray(X0) if X0 is not None else np.full(B.shape, 7.0, dtype=B.dtype))
        if S is not None:
            self.dS.from_lapack(S.reshape(N, 1))

    def result(self, **kw):
        kw.update(A=self.dA.to_lapack(), AF=self.dAF.to_lapack(), B=self.dB.to_lapack(), X=self.dX.to_lapack(),
                  stats=self.ch.last_posvx_stats())
        return kw

    def posvx(self, equed="N"):
        info, eq, rcond, ferr, berr = self.ch.CHAMELEON_dposvx_Tile("F", self.u, self.dA, self.dAF, equed, self.dS,
                                                                    self.dB, self.dX)
        return self.result(info=info, equed=eq, rcond=rcond, ferr=ferr, berr=berr)

    def porfs(self):
        info, ferr, berr = self.ch.CHAMELEON_dporfs_Tile(self.u, self.dA, self.dAF, self.dB, self.dX)
        return self.result(info=info, ferr=ferr, berr=berr)

    def destroy(self):
        for d in (self.dA, self.dAF, self.dS, self.dB, self.dX):
            self.ch.CHAMELEON_Desc_Destroy(d)


def check_columns(tag, r, X, tr, ref, kinds, Xt, n, dt, tolx, tolb, only=None):
    """the per-column expectations: X (the device's solution of the unscaled system) and r's berr against the model's
    trajectory tr, r's ferr against ref (LAPACK's result for these columns, or None) and the true error.  only: the
    columns that are compared with the model (default: every one that does not simply converge)."""
    nrhs = len(kinds)
    kinds = np.array(kinds)
    zero, generic = kinds == "zero", kinds == "generic"
    hard = ~zero & ~generic if only is None else only
    d = distances(X, r["berr"], tr, kinds)
    xm = np.where(zero, 1, np.abs(X).max(axis=0))
    err = np.abs(X - Xt).max(axis=0) / xm
    fdev = np.zeros(nrhs)
    if ref is not None:
        fdev[~zero] = np.abs(r["ferr"] - ref["ferr"])[~zero] / ref["ferr"][~zero]
    ftol = ferr_tolerance(n, dt, kinds)
    print("refine_paths %s: X %.2e (tol %.2e)  berr %.2e (tol %.2e)  ferr against LAPACK: stagnating %.2e itmax %.2e "
          "generic %.2e (tol %.2e %.2e %.2e)  min ferr / err %.1f  generic berr / LAPACK's %.2f" % (
              tag, d["dx"][hard].max(initial=0), tolx, (d["db"] / tolb)[hard].max(initial=0) * np.min(tolb),
              np.min(tolb),
              fdev[kinds == "stagnating"].max(initial=0), fdev[kinds == "itmax"].max(initial=0),
              fdev[generic].max(initial=0), ftol[kinds == "stagnating"].max(initial=0),
              ftol[kinds == "itmax"].max(initial=0), ftol[generic].max(initial=0),
              (r["ferr"][~zero] / np.maximum(err[~zero], 1e-300)).min(initial=np.inf),
              (r["berr"] / ref["berr"])[generic].max(initial=0) if ref is not None else 0))
    assert r["info"] == 0
    # the predicted iterate, and not one of its neighbours
    assert np.all(d["dx"][hard] <= tolx), (np.nonzero(hard & (d["dx"] > tolx))[0], d["dx"])
    assert np.all((d["db"] <= tolb)[hard]), (np.nonzero(hard & (d["db"] > tolb))[0], d["db"])
    for j in np.nonzero(hard)[0]:
        mine = np.abs(X[:, j] - tr.X[:, j]).max()
        assert all(mine < np.abs(X[:, j] - v).max() for v in tr.neighbours(j)), j
    # zero right-hand sides: LAPACK's safe1 rule
    assert np.all(r["berr"][zero] == 1.0), r["berr"]
    assert not bits(r["X"][:, zero]).any()
    assert np.all(np.isfinite(r["ferr"][zero])) and np.all(r["ferr"][zero] < 1e-30), r["ferr"]
    # ferr: a bound of the true error, and LAPACK's figure
    assert np.all(r["ferr"][~zero] >= err[~zero]), (r["ferr"], err)
    if ref is not None:
        assert np.all(fdev <= ftol), (np.nonzero(fdev > ftol)[0], fdev, ftol)
        # the columns that converge: as good as LAPACK's, and the same solution within its bound
        assert np.all(r["berr"][generic] <= 4 * ref["berr"][generic]), (r["berr"], ref["berr"])
        assert np.all((np.abs(r["X"] - ref["X"]).max(axis=0) <= ref["ferr"] * np.abs(ref["X"]).max(axis=0))[generic])
    return d


def check_images(dev, r, B=None):
    """A, AF and B come back bit for bit, NaN halves included (B: the image expected instead of the one given)"""
    assert np.array_equal(bits(r["A"]), bits(dev.A0))
    assert np.array_equal(bits(r["AF"]), bits(dev.AF0))
    assert np.array_equal(bits(r["B"]), bits(dev.B0 if B is None else B))
    assert np.isnan(r["A"]).sum() == np.isnan(r["AF"]).sum() == dev.A0.shape[0] * (dev.A0.shape[0] - 1) // 2


def cut(ref, nrhs):
    return {k: (v[..., :nrhs] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


@pytest.mark.parametrize("nrhs", [1, 3, 19, 57])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_posvx_on_a_wrong_factor(cham, N, T, dt, u, nrhs):
    A, AF, B, Xt, kinds = rm.problem(N, nrhs, dt)
    tr, full = model(N, dt).prefix(nrhs), lapack_run(N, dt, u)
    ref = cut(full, nrhs)
    dev = Device(cham, N, T, u, dt, A, AF, B)
    r = dev.posvx()
    dev.destroy()
    assert r["equed"] == "N" and full["info"] == 0
    check_columns("posvx N %d/%d %s %s nrhs %d" % (N, T, dt, u, nrhs), r, r["X"], tr, ref, kinds, Xt, N, dt,
                  10 * full["dx"].max(), 10 * full["db"].max())
    assert abs(r["rcond"] - ref["rcond"]) <= RCOND_TOL[dt] * ref["rcond"], (r["rcond"], ref["rcond"])
    check_images(dev, r)
    st = r["stats"]
    if nrhs == NMAX:
        # the solve and the first correction run through potrs, the corrections of the columns that run into the
        # iteration limit, from the second on, through the sweeps
        n_itmax = kinds.count("itmax")
        assert tr.survivors[0] > rm.KX >= tr.survivors[1] and tr.survivors[1:5] == [n_itmax] * 4
        assert st["potrs_columns"] >= nrhs + tr.survivors[0], (st, tr.survivors)
        assert st["sweep_columns"] >= 4 * n_itmax, (st, tr.survivors)
    else:
        # the solve, and the corrections of the columns that do not simply converge
        hard = np.array(kinds) != "generic"
        assert st["potrs_columns"] == 0 and st["sweep_columns"] >= nrhs + tr.steps[hard].sum(), (st, tr.steps)


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_posvx_on_a_wrong_factor_equilibrated(cham, N, T, dt, u):
    """equed = 'Y' with S powers of two: A is taken as the scaled matrix, B comes back as diag(S) B, X = diag(S) times
    the solution of the scaled system, ferr is divided by scond = 2^-6"""
    nrhs = 19
    A, AF, B, Xt, kinds = rm.problem(N, nrhs, dt)
    S = scaling(N, dt)
    tr, full, plain = model(N, dt).prefix(nrhs), lapack_run(N, dt, u, "Y"), lapack_run(N, dt, u)
    ref = cut(full, nrhs)
    dev = Device(cham, N, T, u, dt, A, AF, B / S[:, None], S=S)
    r = dev.posvx("Y")
    dev.destroy()
    assert r["equed"] == "Y" and full["info"] == 0
    # (X / S and S Xtrue are exact: check_columns sees the scaled system's solution, ferr the returned one)
    Xs = r["X"] / S[:, None]
    assert np.array_equal(bits(Xs * S[:, None]), bits(r["X"]))
    check_columns("posvx Y %d/%d %s %s" % (N, T, dt, u), dict(r, ferr=r["ferr"] / 64, X=Xs), Xs, tr,
                  dict(ref, ferr=ref["ferr"] / 64, X=ref["X"] / S[:, None]), kinds, Xt, N, dt,
                  10 * plain["dx"].max(), 10 * plain["db"].max())
    nz = np.array(kinds) != "zero"
    err = np.abs(r["X"] - S[:, None] * Xt).max(axis=0)[nz] / np.abs(r["X"]).max(axis=0)[nz]
    assert np.all(r["ferr"][nz] >= err)
    assert abs(r["rcond"] - ref["rcond"]) <= RCOND_TOL[dt] * ref["rcond"], (r["rcond"], ref["rcond"])
    check_images(dev, r, B=B)


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", ["d", "s"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_porfs_on_a_wrong_factor_twice(cham, N, T, dt, u):
    """porfs on the host's first solve, then again on what it returned: count and lstres start afresh in every call"""
    nrhs = 19
    A, AF, B, Xt, kinds = rm.problem(N, nrhs, dt)
    full = lapack_run(N, dt, u)
    tolx, tolb = 10 * full["dx"].max(), 10 * full["db"].max()
    X0 = rm.first_solve(AF, B).astype(rm.NPT[dt])
    tr = rm.trajectory(A, AF, B, X0)
    dev = Device(cham, N, T, u, dt, A, AF, B, X0=X0)
    r1 = dev.porfs()
    # (the first iterate differs from LAPACK's by roundings, far below the margins: its ferr is still the reference)
    check_columns("porfs 1st %d/%d %s %s" % (N, T, dt, u), r1, r1["X"], tr, cut(full, nrhs), kinds, Xt, N, dt, tolx,
                  tolb)
    check_images(dev, r1)
    hard = np.array(kinds) != "generic"
    assert np.array_equal(tr.steps[hard], model(N, dt).prefix(nrhs).steps[hard])
    tr2 = rm.trajectory(A, AF, B, r1["X"])
    r2 = dev.porfs()
    dev.destroy()
    # the model's second call: one more correction where the first stagnated, five more where it was stopped
    decided = np.array([k not in ("zero", "generic") and tr2.decided(j, dt) for j, k in enumerate(kinds)])
    for j, k in enumerate(kinds):
        if decided[j]:
            assert (tr2.steps[j], tr2.exit[j]) == ((1, "stagnation") if k == "stagnating" else (5, "itmax")), (j, k)
    assert all(decided[j] for j, k in enumerate(kinds) if k == "stagnating" or (k == "itmax" and dt == "d"))
    # (the rounding noise of berr is absolute, a rounding of R against W: the relative tolerance grows as berr falls)
    check_columns("porfs 2nd %d/%d %s %s" % (N, T, dt, u), r2, r2["X"], tr2, None, kinds, Xt, N, dt, tolx,
                  tolb * np.maximum(1, tr.final_berr / tr2.final_berr), only=decided)
    # (fp32: five more corrections take a column stopped by the limit down to rounding level, where no model decides)
    rest = ~decided & (np.array(kinds) == "itmax")
    assert np.all(r2["berr"][rest] < r1["berr"][rest])
    check_images(dev, r2)


def test_posvx_on_a_wrong_factor_is_deterministic(cham):
    N, T, dt, u = 1000, 192, "d", "U"
    A, AF, B, Xt, kinds = rm.problem(N, NMAX, dt)
    out = []
    for _ in range(2):
        dev = Device(cham, N, T, u, dt, A, AF, B)
        out.append(dev.posvx())
        dev.destroy()
    for k in ("X", "ferr", "berr"):
        assert np.array_equal(bits(out[0][k]), bits(out[1][k])), k
    assert out[0]["rcond"] == out[1]["rcond"] and out[0]["stats"]["potrs_columns"] == out[1]["stats"]["potrs_columns"]
