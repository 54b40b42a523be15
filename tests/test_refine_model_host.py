"""The reference of test_gpu_refine_paths.py on its own (refine_model.py against scipy's dposvx / sposvx, no GPU): the
decisions of every column that does not simply converge are far from their thresholds, LAPACK given the same wrong
factor returns the iterate the model predicts, with berr = 1 and X = 0 for a zero right-hand side and ferr above the
true error, and LAPACK's distance from the model is what the GPU tolerances (ten times it, recomputed there) assume.

Measured on two machines, the largest over n in {1000, 1024}, both triangles and the 57 columns the GPU test uses:
                        X (relative to max |x| of the column)     berr (relative, non-generic columns)
    fp64                1.2e-14  (Lower, n = 1000: 3.2e-15)       9.6e-12  (Lower, n = 1000: 3.3e-12)
    fp32                6.5e-6   (Lower, n = 1000: 3.2e-6)        5.1e-3   (Lower, n = 1000: 1.1e-3)
LAPACK's Upper solve sums in another order than the model's fp64 Lower one and lies two to three times as far from it,
and the distance in berr is a rounding of the residual, absolute, so relative to a berr of 5e-6 it is the largest.
refine_model.X_DEV and BERR_DEV, asserted here on the first 19 columns, are twice the larger figure.

The margins: consecutive backward errors have the ratio |rho| = 0.7, 0.3 or 0.4 to two digits, and rho = 0.4 puts
|2 b[k+1] - b[k]| at 0.2 b[k] by construction (measured: 0.196 .. 0.198), so refine_model.MARGIN is 0.19: more than
thirty times LAPACK's fp32 distance in berr and 1e10 times its fp64 one.  The smallest backward error of a column that
runs into the iteration limit is 0.3^5 of its first, about 5e-6: 5e10 eps in fp64, and 86 eps .. 98 eps in fp32, so
refine_model.FLOOR, the distance from the berr <= eps exit, is 1e3 eps in fp64 and 50 eps in fp32."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.linalg.lapack as lapack

import refine_model as rm

WANT = {"stagnating": (1, "stagnation"), "itmax": (5, "itmax"), "zero": (1, "stagnation")}


@pytest.fixture(scope="module", params=[(n, dt) for n in (1000, 1024) for dt in "ds"], ids=lambda p: "%d-%s" % p)
def case(request):
    n, dt = request.param
    A, AF, B, Xt, kinds = rm.problem(n, 19, dt)
    return n, dt, A, AF, B, Xt, kinds, rm.trajectory(A, AF, B, rm.first_solve(AF, B))


def test_the_problem_is_what_it_says(case):
    n, dt, A, AF, B, Xt, kinds, tr = case
    assert kinds == [rm.kind_of(p) for p in rm.PATTERN]
    assert A.dtype == AF.dtype == B.dtype == rm.NPT[dt] and np.array_equal(A, A.T) and not np.triu(AF, 1).any()
    # a smaller nrhs is a prefix
    assert np.array_equal(rm.problem(n, 3, dt)[2], B[:, :3]) and rm.problem(n, 3, dt)[4] == kinds[:3]
    # I - M^{-1} A has the eigenvalues rho
    L = AF.astype(np.float64)
    ev = np.sort(1 - sla.eigvalsh(A.astype(np.float64), L @ L.T))
    assert np.allclose(ev[:3], [-0.7, -0.4, -0.3], atol=1e-3) and np.allclose(ev[-3:], [0.3, 0.4, 0.7], atol=1e-3)
    assert np.abs(ev[3:-3]).max() < 1e-3
    for j, k in enumerate(kinds):
        assert (not B[:, j].any()) == (k == "zero")


def test_every_decision_has_margin(case):
    n, dt, A, AF, B, Xt, kinds, tr = case
    for j, k in enumerate(kinds):
        b = np.array(tr.berr[j])
        if k == "generic":
            assert tr.exit[j] == "eps" and tr.steps[j] <= 1
            continue
        assert (tr.steps[j], tr.exit[j]) == WANT[k], (j, k, tr.steps[j], tr.exit[j])
        assert len(b) == tr.steps[j] + 1
        assert np.all(np.abs(2 * b[1:] - b[:-1]) >= rm.MARGIN * b[:-1]), (j, b)
        assert np.all(b >= rm.FLOOR[dt] * rm.EPS[dt]), (j, b)
        assert tr.decided(j, dt)
        if k != "zero":
            rho = abs(rm.PATTERN[j])
            assert np.allclose(b[1:] / b[:-1], rho, atol=1e-2), (j, b[1:] / b[:-1])
    # after the second pass: the nine scattered columns that run into the iteration limit
    assert tr.sizes[2:] == [9, 9, 9, 9] and tr.survivors[1:] == [9, 9, 9, 9, 0]
    assert [j for j, k in enumerate(kinds) if k == "itmax"] == [2, 3, 5, 7, 10, 13, 14, 15, 18]
    assert tr.potrs_columns == 0 and tr.sweep_columns == sum(tr.survivors)
    cut = tr.prefix(3)
    assert cut.sizes[2:] == [1, 1, 1, 1] and cut.steps.tolist() == [1, tr.steps[1], 5] and cut.X.shape == (n, 3)


@pytest.mark.parametrize("lower", [1, 0])
def test_lapack_returns_the_predicted_iterate(case, lower):
    n, dt, A, AF, B, Xt, kinds, tr = case
    fn = lapack.dposvx if dt == "d" else lapack.sposvx
    af = AF if lower else np.asfortranarray(AF.T)
    x, rcond, ferr, berr, info = fn(A, B, fact="F", af=af, equed="N", lower=lower)[5:10]
    assert info == 0 and 1e-4 < rcond < 1e-3
    kinds = np.array(kinds)
    zero, hard = kinds == "zero", (kinds != "zero") & (kinds != "generic")
    assert np.all(berr[zero] == 1.0) and not x[:, zero].any()
    assert np.all(ferr[zero] < 1e-30)
    xm = np.where(zero, 1, np.abs(x).max(axis=0))
    dx = np.abs(x - tr.X).max(axis=0) / xm
    db = np.abs(berr - tr.final_berr)[hard] / tr.final_berr[hard]
    print("lapack against the model: n %d %s lower %d  X %.2e  berr %.2e" % (n, dt, lower, dx.max(), db.max()))
    assert dx.max() <= rm.X_DEV[dt], dx
    assert db.max() <= rm.BERR_DEV[dt], db
    for j in np.nonzero(hard)[0]:
        assert all(np.abs(x[:, j] - tr.X[:, j]).max() < np.abs(x[:, j] - v).max() for v in tr.neighbours(j)), j
    err = np.abs(x - Xt).max(axis=0) / xm
    assert np.all(ferr[~zero] >= err[~zero]), (ferr, err)
