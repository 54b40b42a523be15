"""The position of a failing pivot, exact, in fp64 and fp32, Lower and Upper.

The members of dyadic_model.cholesky_case (A = L L^T, L = (I + Nn) diag(s)) have short dyadic Schur complements, so the
blocked factorisation is exact on them in either dtype whatever its summation order (test_dyadic_host.py).  One diagonal
entry is perturbed (cond_cases.py):
    A[j,j] -= s_j^2            pivot j is exactly 0     info == j + 1
    A[j,j] -= s_j^2 + 1        pivot j is exactly -1    info == j + 1
    A[n-1,n-1] -= s^2 - 2^-20  the last pivot is 2^-20  info == 0, L[n-1,n-1] == 2^-10 bit for bit, the rest of L as it was
All arithmetic before pivot j is exact, so rounding excuses nothing: a zero pivot that the fp32 MFMA's rounding left at
+tiny, a pivot read from the wrong register or lane of the chain, an info counted from the wrong base or reported a
column late all change the integer.  The columns are the 16-panel and 128-block boundaries of the pivot chain (0, 15, 16,
127, 128), the tile boundary (B - 1, B), a column in a middle tile, the first column of the (ragged) last tile and n - 1; the
shapes one tile of 128, 256 and 200 (the staged, padded path) and whole matrices (1024, 256) and (1000, 192) on mirror
and mod3, (1024, 256) on panel.  The other triangle comes back bit for bit.  Printed, not asserted (the header does not
promise it): whether the columns before the failing 128-block are L's.  test_conditioning_host.py shows without a GPU
that the emulation meets these pivots exactly and that the helpers fail a Cholesky with one fault.

The zero pivot at column 700 of (1024, 256) once more under the forced counter-linked form and the forced flow form, each
in a fresh child process: either reports a failed pivot through a path of its own (the abort word, the raised counters)."""
import json
import os
import sys

import numpy as np
import pytest

import cond_cases as cc
from chol_testkit import chdt, desc, other_triangle_kept, run_child, uplo_code

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PIPE_ALL = {"CHOLMI_PIPE_FACTOR": "100", "CHOLMI_PAIR_FACTOR": "1000"}
FLOW_ALL = {"CHOLMI_FLOW_FACTOR": "100", "CHOLMI_PIPE_FACTOR": "100", "CHOLMI_PAIR_FACTOR": "1000"}
SHAPE_IDS = [f"{fam}-{n}-{B}" for fam, n, B in cc.PIVOT_SHAPES]


def gpu_factor(ch, B):
    """factor(S, u) of cond_cases.py on the library: one tile on the caller's buffer, a whole matrix in the library's own
    storage"""
    def factor(S, u):
        n, dt = S.shape[0], ("d" if S.dtype == np.float64 else "s")
        potrf = getattr(ch, f"CHAMELEON_{dt}potrf_Tile")
        if n == B:
            F = S.copy(order="F")
            d = ch.CHAMELEON_Desc_Create(F, chdt(ch, dt), B, B, B * B, B, B, 0, 0, B, B, 1, 1)
            info = potrf(uplo_code(ch, u), d)
        else:
            d = desc(ch, n, B, dt)
            d.from_lapack(S)
            info = potrf(uplo_code(ch, u), d)
            F = d.to_lapack()
        ch.CHAMELEON_Desc_Destroy(d)
        return info, F
    return factor


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", cc.DTYPES)
@pytest.mark.parametrize("fam,n,B", cc.PIVOT_SHAPES, ids=SHAPE_IDS)
def test_zero_and_negative_pivots_are_reported_at_their_column(cham, fam, n, B, dt, u):
    cc.check_pivot_positions(gpu_factor(cham, B), fam, n, B, dt, u)


@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dt", cc.DTYPES)
@pytest.mark.parametrize("fam,n,B", cc.TINY_SHAPES, ids=[f"{fam}-{n}-{B}" for fam, n, B in cc.TINY_SHAPES])
def test_tiny_positive_last_pivot_is_a_pivot(cham, fam, n, B, dt, u):
    cc.check_tiny_last_pivot(gpu_factor(cham, B), fam, n, B, dt, u)


def child_main():
    """the zero pivot of cc.FORCED in fp64 and fp32 under the switches of this process's environment"""
    sys.path.insert(0, ROOT)
    from dense_linear_app_amd import chameleon as ch

    ch.CHAMELEON_Init(1, 1)
    fam, n, B, j = cc.FORCED
    A, _, s = cc.pivot_member(fam, n, B)
    for dt in cc.DTYPES:
        S = cc.stored_exactly(cc.perturbed(A, s, j, "zero"), dt, "L")
        info, F = gpu_factor(ch, B)(S, "L")
        rec = {"dt": dt, "info": int(info), "other_kept": bool(other_triangle_kept(F, S, "L")),
               "regimes": ch.last_potrf_regimes()}
        print("CASE " + json.dumps(rec), flush=True)


@pytest.mark.parametrize("name,env,regime", [("counters", PIPE_ALL, "counter_linked"),
                                             ("flow", dict(FLOW_ALL, CHOLMI_FLOW_NBM="2:8"), "flow")],
                         ids=["counters", "flow"])
def test_forced_chain_forms_report_the_zero_pivot(name, env, regime):
    """the counter-linked form raises the counters its waiters poll, the flow form its abort word: info == 701 from
    both, in both dtypes, and the library's count says that the form ran"""
    cases = run_child(__file__, ["forced"], env, 120, f"the forced {name} form")
    assert [c["dt"] for c in cases] == list(cc.DTYPES)
    for c in cases:
        assert c["info"] == cc.FORCED[3] + 1 and c["other_kept"], c
        assert c["regimes"][regime] >= 1, c


if __name__ == "__main__":
    assert sys.argv[1:] == ["forced"]
    child_main()
