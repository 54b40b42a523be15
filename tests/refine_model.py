"""A reference for the refinement loop of porfs / posvx on a factor that is wrong on purpose (numpy and scipy only).

problem(): A = Q diag(lam) Q^T and AF = chol(M), M = Q diag(lam_i / (1 - rho_i)) Q^T, so that I - M^{-1} A =
Q diag(rho) Q^T: one correction with AF multiplies the error of an iterate along q_i by rho_i.  rho is zero except on
six eigen-directions; column j of the true solution is a generic vector of the rho = 0 subspace (max 1) plus
S_SPECIAL sqrt(n) q_k for the direction k that the column pattern gives it.  The special part is small against the
column, so the denominator of the backward error stays put and consecutive backward errors have the ratio |rho_k| from
the first pass on: |rho| = 0.7 stagnates after one correction (2 berr > lstres), |rho| in {0.3, 0.4} runs into the
iteration limit after five, rho = 0 converges at once, and a zero right-hand side gives berr = 1 by LAPACK's safe1 rule.

trajectory(): DPORFS's rule column by column on residuals formed in long double and corrections solved in fp64, with
every iterate kept, and the schedule of active-set sizes that the lockstep loop of porfs_impl goes through."""
import functools

import numpy as np
import scipy.linalg as sla

NPT = {"d": np.float64, "s": np.float32}
EPS = {"d": 2.0 ** -53, "s": 2.0 ** -24}  # xLAMCH('Epsilon')
SAFMIN = {"d": 2.0 ** -1022, "s": 2.0 ** -126}
ITMAX = 5
KX = 40  # spd.hip: POSVX_KX, the widest application of A^{-1} that runs as multi-vector sweeps
S_SPECIAL = 1e-2
# what a column's decisions must keep clear of for rounding not to change them (test_refine_model_host.py): the
# relative distance of 2 berr from lstres, and the smallest berr in units of eps
MARGIN = 0.19
FLOOR = {"d": 1e3, "s": 50.0}
# how far LAPACK's xPOSVX may lie from trajectory(): X relative to max |x| of the column, berr relative (the columns
# that do not simply converge); twice the largest distance measured (test_refine_model_host.py)
X_DEV = {"d": 2 * 1.2e-14, "s": 2 * 6.5e-6}
BERR_DEV = {"d": 2 * 9.6e-12, "s": 2 * 5.1e-3}
# the eigen-direction that contracts by rho
SPECIAL = {0.7: 5, 0.3: 17, -0.4: 40, 0.4: 77, -0.7: 123, -0.3: 200}
G, Z = "g", "0"
PATTERN = [0.7, G, 0.3, -0.4, Z, 0.4, -0.7, -0.3, G, 0.7, 0.3, -0.7, Z, -0.4, 0.4, -0.3, G, 0.7, 0.3]


def kind_of(p):
    return "zero" if p == Z else "generic" if p == G else "stagnating" if abs(p) == 0.7 else "itmax"


def pattern(nrhs):
    return [PATTERN[j % len(PATTERN)] for j in range(nrhs)]


@functools.lru_cache(maxsize=None)
def _matrices(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0, -2, n)
    rho = np.zeros(n)
    for r, i in SPECIAL.items():
        rho[i] = r
    A = (Q * lam) @ Q.T
    M = (Q * (lam / (1 - rho))) @ Q.T
    return Q, (A + A.T) / 2, np.linalg.cholesky((M + M.T) / 2), rng.bit_generator.state


@functools.lru_cache(maxsize=None)
def problem(n, nrhs, dt, seed=3):
    """(A, AF, B, Xtrue, kinds): A symmetric and AF = chol(M) (Lower, zero above) in the working type, B = fl(A Xtrue),
    Xtrue in fp64, kinds[j] in {stagnating, itmax, generic, zero}.  The columns are drawn in order from one generator,
    so a smaller nrhs is a prefix of a larger one.  The arrays are shared: read-only."""
    Q, A0, L0, state = _matrices(n, seed)
    rng = np.random.default_rng()
    rng.bit_generator.state = state
    mask = np.ones(n)
    mask[list(SPECIAL.values())] = 0
    pat = pattern(nrhs)
    Xt = np.zeros((n, nrhs), order="F")
    for j, p in enumerate(pat):
        if p == Z:
            continue
        z = Q @ (mask * rng.standard_normal(n))
        Xt[:, j] = z / np.abs(z).max()
        if p != G:
            Xt[:, j] += S_SPECIAL * np.sqrt(n) * Q[:, SPECIAL[p]]
    A = np.asfortranarray(A0.astype(NPT[dt]))
    AF = np.asfortranarray(L0.astype(NPT[dt]))
    B = np.asfortranarray((A.astype(np.float64) @ Xt).astype(NPT[dt]))
    for a in (A, AF, B, Xt):
        a.setflags(write=False)
    return A, AF, B, Xt, [kind_of(p) for p in pat]


def first_solve(AF, B):
    """AF^{-1} B in fp64 (AF Lower)"""
    return sla.cho_solve((AF.astype(np.float64), True), B.astype(np.float64))


class Trajectory:
    """berr[j]: the backward error of every pass of column j; steps[j]: its corrections; exit[j]: the rule that ended
    it (eps, stagnation, itmax); X: the returned iterates; iterates[j][k]: iterate k of column j, k = 0 .. steps[j] + 1
    (one past the returned one); sizes[p]: the columns whose residual pass p forms; survivors[p]: those it corrects;
    potrs_columns / sweep_columns: the corrections that are wider than KX columns / that are not."""

    def neighbours(self, j):
        """the iterates next to the returned one"""
        k = self.steps[j]
        return [self.iterates[j][i] for i in (k - 1, k + 1) if i >= 0]

    def decided(self, j, dt):
        """every decision of column j is MARGIN away from the stagnation threshold and FLOOR eps above the eps exit"""
        b = np.array(self.berr[j])
        return bool(np.all(np.abs(2 * b[1:] - b[:-1]) >= MARGIN * b[:-1]) and np.all(b >= FLOOR[dt] * EPS[dt]))

    def prefix(self, nrhs):
        """the trajectory of the first nrhs columns alone"""
        t = Trajectory()
        t.berr, t.iterates, t.exit = self.berr[:nrhs], self.iterates[:nrhs], self.exit[:nrhs]
        t.steps, t.X = self.steps[:nrhs], self.X[:, :nrhs]
        return t._schedule()

    def _schedule(self):
        passes = max(len(b) for b in self.berr)
        self.sizes = [sum(len(b) > p for b in self.berr) for p in range(passes)]
        self.survivors = [int((self.steps > p).sum()) for p in range(passes)]
        self.final_berr = np.array([b[-1] for b in self.berr])
        self.potrs_columns = sum(k for k in self.survivors if k > KX)
        self.sweep_columns = sum(k for k in self.survivors if k <= KX)
        return self


def trajectory(A, AF, B, X0):
    """DPORFS's loop on A (symmetric), AF (Lower), B and the first iterate X0, in the working type of A"""
    dt = "d" if A.dtype == np.float64 else "s"
    n, nrhs = B.shape
    eps, safe1 = EPS[dt], (n + 1) * SAFMIN[dt]
    safe2 = safe1 / eps
    # (row-major operands: numpy's long-double product is a plain loop)
    Al = np.ascontiguousarray(A, dtype=np.longdouble)
    aAl = np.abs(Al)
    Bl = B.astype(np.longdouble)
    cf = (AF.astype(np.float64), True)
    X = np.array(X0, dtype=np.float64, order="F")
    t = Trajectory()
    t.berr = [[] for _ in range(nrhs)]
    t.iterates = [[X[:, j].copy()] for j in range(nrhs)]
    t.steps, t.exit = np.zeros(nrhs, dtype=int), [None] * nrhs
    lstres, count = np.full(nrhs, 3.0), np.ones(nrhs, dtype=int)
    active = list(range(nrhs))
    while active:
        Xl = np.ascontiguousarray(X[:, active], dtype=np.longdouble)
        R = Bl[:, active] - np.dot(Al, Xl)
        W = np.abs(Bl[:, active]) + np.dot(aAl, np.abs(Xl))
        ratio = np.where(W > safe2, np.abs(R) / np.where(W > safe2, W, 1), (np.abs(R) + safe1) / (W + safe1))
        b = ratio.max(axis=0).astype(np.float64)
        D = sla.cho_solve(cf, R.astype(np.float64))
        nxt = []
        for i, j in enumerate(active):
            t.berr[j].append(b[i])
            t.iterates[j].append(X[:, j] + D[:, i])
            if b[i] > eps and 2 * b[i] <= lstres[j] and count[j] <= ITMAX:
                lstres[j] = b[i]
                count[j] += 1
                X[:, j] = t.iterates[j][-1]
                nxt.append(j)
            else:
                t.exit[j] = "eps" if not b[i] > eps else "stagnation" if not 2 * b[i] <= lstres[j] else "itmax"
                t.steps[j] = count[j] - 1
        active = nxt
    t.X = X
    return t._schedule()
