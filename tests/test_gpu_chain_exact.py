"""The panel chain, bit for bit: CHAMELEON_{d,s}potrf_Tile on the dyadic families of dyadic_model.py, whose factor every
blocked algorithm must return exactly (test_dyadic_host.py proves that for the reference alone, at every (family, order)
of CASES and of the in-process tests), in every form of the chain -- event-linked, counter-linked and flow;
small-block and throughput TRSM steps; fused and split in-tile steps;
paired panels; gates and self-polling grids -- each forced through its environment switch in one fresh child process
(the switches are read once, at chol_init).  Dense diagonal blocks, block inverses, in-tile solves and panel tiles
throughout: a wrong hand-off, a skipped block column or a sign in the recursive inverse changes integers.

Four families.  "parity" (entries at odd row, even column only) leaves half the rows and columns of the factor empty and
makes every product of two off-diagonal pieces zero: the rank-1 update of every odd column of a diagonal block adds
zeros, and the recursive inverse is right with or without the strictly lower part of W11.  "mirror" fills the other
half; "mod3" (Nn^3 = 0) gives every inverse a second-order term; "panel" (tiles of whole 128-blocks only) is dense
everywhere outside the diagonal 128-blocks, which follow mod3: every row and column of every panel tile and of every
trailing update carries entries, and every K-loop of 128 sums dozens of non-zero products.

In-process: the probe of the fp64 pivot chain (rsq + two Goldschmidt steps, no sqrt) at powers of four, ChamUpper, the
single-tile POTRF and TRSM (alpha != 1 takes the throughput form on one tile; B = 200 the staged, padded path) and the
wave-level task path."""
import json
import os
import sys

import numpy as np
import pytest

import dyadic_model as dm
from chol_testkit import bits, chdt, desc, npdt, run_child, stored_lower

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(512, 128), (1024, 256), (1536, 384), (2048, 512), (4096, 1024), (1000, 192), (1100, 320)]
PANEL_SHAPES = [(N, B) for N, B in SHAPES if B % 128 == 0] + [(1000, 256), (1100, 384)]  # (two ragged orders on such tiles)
THIN_SHAPES = [(1024, 256), (2048, 512), (1000, 192), (1100, 320)]
CASES = ([("parity", N, B) for N, B in SHAPES] + [("panel", N, B) for N, B in PANEL_SHAPES]
         + [(fam, N, B) for fam in ("mirror", "mod3") for N, B in THIN_SHAPES])
FILL_CASES = [(fam, B) for fam in ("parity", "panel") for B in (256, 512)]
NEW_FAMILIES = ("mirror", "mod3", "panel")
PIPE_ALL = {"CHOLMI_PIPE_FACTOR": "100", "CHOLMI_PAIR_FACTOR": "1000"}
FLOW_ALL = {"CHOLMI_FLOW_FACTOR": "100", "CHOLMI_PIPE_FACTOR": "100", "CHOLMI_PAIR_FACTOR": "1000"}


def member(fam, N, B):
    """(A, L, s) of the Cholesky member of a family at order N (seed N); B, the tile size, shapes the panel family only"""
    if fam == "parity":
        return dm.cholesky_case(N, N)
    return dm.cholesky_case(N, N, 2, fam, B if fam == "panel" else None)


def with_families(shapes, one=lambda s: s):
    """the (family, shape) parameters of an in-process test and their ids: today's ids for parity, the family in front
    for the others, panel on tiles of whole 128-blocks only (one(shape): its tile size)"""
    params = [("parity", s) for s in shapes] + [(fam, s) for fam in NEW_FAMILIES for s in shapes
                                                 if fam != "panel" or one(s) % 128 == 0]
    flat = [(fam,) + (s if isinstance(s, tuple) else (s,)) for fam, s in params]
    return flat, ["-".join(str(x) for x in (f[1:] if f[0] == "parity" else f)) for f in flat]


def lower_as(A, dt, fill=np.nan):
    """the lower triangle of A in dtype dt, the strict upper triangle = fill"""
    return stored_lower(A.astype(npdt(dt)), "L", fill)


def mismatches(got, want, B):
    """-> (count, the first few as (tile row, tile column, 128-block row, 128-block column) of the tile)"""
    i, j = np.nonzero(got != want)
    where = sorted({(int(a // B), int(b // B), int(a % B // 128), int(b % B // 128)) for a, b in zip(i[:4096], j[:4096])})
    return int(len(i)), where[:6]


def factor_case(ch, fam, N, B, dt, S, L):
    """one whole-matrix factorisation of S (the Cholesky member as lower_as leaves it) -> the record the child
    prints"""
    d = desc(ch, N, B, dt)
    d.from_lapack(S)
    info = ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d)
    F = d.to_lapack()
    ch.CHAMELEON_Desc_Destroy(d)
    low = np.tri(N, dtype=bool)
    count, where = mismatches(np.where(low, F, 0), L, B)
    return {"family": fam, "N": N, "B": B, "dt": dt, "info": int(info), "mismatches": count, "first": where,
            "upper_touched": int(((bits(F) != bits(S)) & ~low).sum()), "regimes": ch.last_potrf_regimes()}


def chain_inputs(fam, N, B):
    """-> (S, L) in fp32: A as lower_as leaves it and the factor (integers far below 2^24: the fp32 image holds them
    exactly, and the fp64 inputs are its widening)"""
    A, L, _ = member(fam, N, B)
    return lower_as(A, "s"), L.astype(np.float32)


_inputs_file = None


def inputs_file():
    """the inputs of every case, built once per session and handed to the children: each of the fifteen would
    otherwise spend its first seconds on the same random draws and L L^T products"""
    global _inputs_file
    if _inputs_file is None:
        import atexit
        import tempfile

        fd, path = tempfile.mkstemp(prefix="chain_exact_", suffix=".npz")
        os.close(fd)
        atexit.register(lambda: os.path.exists(path) and os.remove(path))
        arrays = {}
        for fam, N, B in CASES:  # (small integers: A as int16 and L as int8 keep the file at a tenth of the fp32 images)
            A, L, _ = member(fam, N, B)
            assert np.abs(A).max() < 2 ** 15 and np.abs(L).max() < 2 ** 7
            arrays[f"A_{fam}_{N}_{B}"], arrays[f"L_{fam}_{N}_{B}"] = np.tril(A).astype(np.int16), L.astype(np.int8)
        np.savez(path, **arrays)
        _inputs_file = path
    return _inputs_file


def child_main(inputs=None):
    """every case in fp64 and fp32 under the switches of this process's environment, one record per case; inputs: the
    parent's file of inputs (without one the child builds them itself)"""
    import time

    t0 = time.perf_counter()
    sys.path.insert(0, ROOT)
    from dense_linear_app_amd import chameleon as ch

    ch.CHAMELEON_Init(1, 1)
    t1 = time.perf_counter()
    held = np.load(inputs) if inputs else None
    for fam, N, B in CASES:
        if held is not None:
            S, Ls = lower_as(held[f"A_{fam}_{N}_{B}"], "s"), held[f"L_{fam}_{N}_{B}"].astype(np.float32)
        else:
            S, Ls = chain_inputs(fam, N, B)
        for dt in ("d", "s"):
            rec = factor_case(ch, fam, N, B, dt, S.astype(npdt(dt)), Ls.astype(npdt(dt)))
            print("CASE " + json.dumps(rec), flush=True)
    print(f"TIME start-up {t1 - t0:.2f} s, cases {time.perf_counter() - t1:.2f} s", flush=True)


def nbm_of(c):
    return -(-c["B"] // 128)


def four_tiles(cases):
    """the cases with at least four tiles per side: a head tile, a far column, room for a pair from wave 1 (every shape
    but the ragged (1100, 384) of the panel family, which has three)"""
    return [c for c in cases if -(-c["N"] // c["B"]) >= 4]


def counter_linked(cases):
    assert all(c["regimes"]["counter_linked"] >= 1 for c in cases), cases


def event_linked(cases):
    assert all(c["regimes"]["counter_linked"] == 0 and c["regimes"]["flow"] == 0 for c in cases), cases


def paired(cases):
    assert all(c["regimes"]["paired"] >= 1 for c in four_tiles(cases)), cases


def near_off(cases):
    counter_linked(cases)
    assert all(c["regimes"]["near_column"] == 0 and c["regimes"]["column_latency_form"] == 0 for c in cases), cases


def near_on(cases):
    counter_linked(cases)
    assert all(c["regimes"]["near_column"] >= 1 for c in four_tiles(cases)), cases
    assert all(c["regimes"]["column_latency_form"] >= 1 for c in cases if nbm_of(c) <= 4), cases


def flow(cases):
    assert all(c["regimes"]["flow"] >= 1 for c in cases if nbm_of(c) >= 2), cases


SETTINGS = [
    ("default", {}, None),
    ("trsm-throughput", {"CHOLMI_TRSM_SMALL_MAX": "0"}, None),
    ("trsm-throughput-counters", dict(PIPE_ALL, CHOLMI_TRSM_SMALL_MAX="0"), counter_linked),
    ("trsm-small", {"CHOLMI_TRSM_SMALL_MAX": "100000"}, None),
    ("intile-split", {"CHOLMI_INTILE_FUSED": "0"}, None),
    ("intile-split-counters", dict(PIPE_ALL, CHOLMI_INTILE_FUSED="0"), counter_linked),
    ("events-only", {"CHOLMI_DEVICE_FLAGS": "0"}, event_linked),
    ("counters", PIPE_ALL, counter_linked),
    ("counters-no-near", dict(PIPE_ALL, CHOLMI_NEAR_FACTOR="0", CHOLMI_U1_SMALL="0"), near_off),
    ("counters-near", dict(PIPE_ALL, CHOLMI_NEAR_FACTOR="100", CHOLMI_U1_SMALL="64"), near_on),
    ("paired", {"CHOLMI_PAIR_FACTOR": "0"}, paired),
    ("gates", {"CHOLMI_POLL_MAX_WGS": "0"}, None),
    ("self-polling", {"CHOLMI_POLL_MAX_WGS": "100000"}, None),
    ("flow", dict(FLOW_ALL, CHOLMI_FLOW_NBM="2:8"), flow),
    ("flow-fences", dict(FLOW_ALL, CHOLMI_FLOW_NBM="2:8", CHOLMI_FLOW_FENCES="1"), flow),
]


@pytest.mark.parametrize("name,env,regime", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_potrf_is_exact_in_every_form_of_the_chain(name, env, regime):
    """every shape (nbm = 1, 2, 3, 4, 8 with four tiles per side: a head tile, a far column, room for a pair from wave 1;
    two ragged orders with odd tiles and identity padding) on the parity family, the panel family on the tiles of whole
    128-blocks (and two ragged orders on such tiles), mirror and mod3 on nbm = 2, 4 and the two ragged orders (CASES),
    fp64 and fp32, in one child per setting: info = 0, tril(F) == L with zero mismatches, the NaN-filled strict upper
    triangle untouched, and -- where the setting forces a regime -- the library's count says that it ran"""
    cases = run_child(__file__, ["cases", inputs_file()], env, 300, f"setting {name}")
    assert [(c["family"], c["N"], c["B"], c["dt"]) for c in cases] == [(fam, N, B, dt) for fam, N, B in CASES for dt in "ds"]
    bad = [c for c in cases if c["info"] != 0 or c["mismatches"] or c["upper_touched"]]
    assert not bad, bad
    if regime:
        regime(cases)


def fill_child_main():
    """single-tile POTRF with a FINITE strict upper triangle, under this process's in-tile switch"""
    sys.path.insert(0, ROOT)
    from dense_linear_app_amd import chameleon as ch

    ch.CHAMELEON_Init(1, 1)
    for fam, B in FILL_CASES:
        A, L, _ = member(fam, B, B)
        for dt in ("d", "s"):
            info, T, S = potrf_tile(ch, A, dt, fill=-7.0)
            iu = np.triu_indices(B, 1)
            rec = {"family": fam, "B": B, "dt": dt, "info": int(info),
                   "mismatches": mismatches(np.tril(T), L.astype(npdt(dt)), B)[0],
                   "upper_touched": int((bits(T[iu]) != bits(S[iu])).sum())}
            print("CASE " + json.dumps(rec), flush=True)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "split"])
def test_intile_update_leaves_a_finite_upper_triangle_alone(fused):
    """the diagonal 64 x 64 blocks of the in-tile update write i >= j only.  Above the diagonal the other cases hold NaN,
    and NaN - x stores the same NaN back: an update that lost its mask would pass them.  Here the strict upper triangle
    is -7, one tile of 2 and of 4 blocks (one and three in-tile steps), the parity and the panel family (whose in-tile
    update touches every entry of the diagonal blocks' lower triangles), fp64 and fp32, the solve and the update of a step
    in one launch and in two: L exact, and not one bit above the diagonal changed"""
    cases = run_child(__file__, ["finite-fill"], {"CHOLMI_INTILE_FUSED": fused}, 120, "the finite fill")
    assert [(c["family"], c["B"], c["dt"]) for c in cases] == [(fam, B, dt) for fam, B in FILL_CASES for dt in "ds"]
    bad = [c for c in cases if c["info"] != 0 or c["mismatches"] or c["upper_touched"]]
    assert not bad, bad


# ---- in-process ---------------------------------------------------------------------------------------------------------
def potrf_tile(ch, A, dt, fill=np.nan):
    """single-tile POTRF on a host buffer -> (info, the tile afterwards, the tile as stored)"""
    S = lower_as(A, dt, fill)
    T = S.copy(order="F")
    B = A.shape[0]
    d = ch.CHAMELEON_Desc_Create(T, chdt(ch, dt), B, B, B * B, B, B, 0, 0, B, B, 1, 1)
    info = ch.CHAMELEON_dpotrf_Tile(ch.ChamLower, d)
    ch.CHAMELEON_Desc_Destroy(d)
    return info, T, S


@pytest.mark.parametrize("dt", ["d", "s"])
def test_pivot_chain_is_exact_at_powers_of_four(cham, dt):
    """the fp64 pivot chain takes no square root: v_rsq_f64 and two Goldschmidt steps, rinv = h + h uncorrected.  At
    d = 4^k the second step lands on 2^k and 2^-k exactly as long as the instruction's result is within about 2^-26 of
    2^-k -- the fact every fp64 case of this file and of test_gpu_factor_exact.py rests on"""
    ch = cham
    d = np.array([1.0, 4.0, 16.0])[np.arange(128) % 3]
    info, T, _ = potrf_tile(ch, np.diag(d), dt, fill=0.0)
    got, want = np.diag(T), np.sqrt(d).astype(npdt(dt))
    print("pivots", dt, [(float(a), hex(int(b))) for a, b in zip(d[:3], bits(got[:3]))])
    assert info == 0 and np.array_equal(bits(got), bits(want)), [hex(int(b)) for b in bits(got[:3])]
    assert not np.any(np.tril(T, -1))
    A, L, _ = dm.cholesky_case(128, 128)
    info, T, S = potrf_tile(ch, A, dt)
    assert info == 0
    assert mismatches(np.tril(T), L.astype(npdt(dt)), 128)[0] == 0


UPPER = with_families([(1024, 256), (1000, 192)], lambda s: s[1])
ONE_TILE = with_families([128, 256, 512, 1024, 200])
WAVE = with_families([(1024, 256), (1536, 512)], lambda s: s[1])


@pytest.mark.parametrize("fam,N,B", UPPER[0], ids=UPPER[1])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_potrf_upper_is_exact(cham, fam, N, B, dt):
    ch = cham
    A, L, _ = member(fam, N, B)
    S = np.array(lower_as(A, dt).T, order="F")
    d = desc(ch, N, B, dt)
    d.from_lapack(S)
    assert ch.CHAMELEON_dpotrf_Tile(ch.ChamUpper, d) == 0
    F = d.to_lapack()
    ch.CHAMELEON_Desc_Destroy(d)
    assert mismatches(np.triu(F).T, L.astype(npdt(dt)), B) == (0, [])
    il = np.tril_indices(N, -1)
    assert np.array_equal(bits(F[il]), bits(S[il]))


@pytest.mark.parametrize("fam,B", ONE_TILE[0], ids=ONE_TILE[1])
@pytest.mark.parametrize("dt", ["d", "s"])
def test_single_tile_potrf_and_trsm_are_exact(cham, fam, B, dt):
    """one tile: POTRF returns L; TRSM (Right, Lower, Trans, NonUnit, alpha) on X L^T returns alpha X -- alpha = 1 in the
    small-block form, alpha = -2 and 1/2 through k_panel_solve / k_panel_update"""
    ch = cham
    A, L, _ = member(fam, B, B)
    info, T, S = potrf_tile(ch, A, dt)
    assert info == 0
    assert mismatches(np.tril(T), L.astype(npdt(dt)), B) == (0, [])
    iu = np.triu_indices(B, 1)
    assert np.array_equal(bits(T[iu]), bits(S[iu]))
    X = dm.solution(B, B, B)
    P = X @ L.T
    assert np.abs(P).max() * 16 < 2.0 ** 24
    Lt = np.array(lower_as(L, dt), order="F")  # (TRSM reads the lower triangle only)
    dl = ch.CHAMELEON_Desc_Create(Lt, chdt(ch, dt), B, B, B * B, B, B, 0, 0, B, B, 1, 1)
    for alpha in (1.0, -2.0, 0.5):
        Pt = np.array(P, dtype=npdt(dt), order="F")
        dp = ch.CHAMELEON_Desc_Create(Pt, chdt(ch, dt), B, B, B * B, B, B, 0, 0, B, B, 1, 1)
        assert ch.CHAMELEON_dtrsm_Tile(ch.ChamRight, ch.ChamLower, ch.ChamTrans, ch.ChamNonUnit, alpha, dl, dp) == 0
        ch.CHAMELEON_Desc_Destroy(dp)
        assert mismatches(Pt, (alpha * X).astype(npdt(dt)), B) == (0, []), alpha
    ch.CHAMELEON_Desc_Destroy(dl)


@pytest.mark.parametrize("fam,N,B", WAVE[0], ids=WAVE[1])
def test_wave_level_task_path_is_exact(cham, fam, N, B):
    """the worker / client route (every ready task of a wave in one ExecuteBatch) and the per-task route: exactly L"""
    from dense_linear_app_amd import client
    from dense_linear_app_amd.worker import DagCholeskyWorker

    A, L, _ = member(fam, N, B)
    Af = np.array(A, order="F")
    wave = client.run_cholesky_dag(N, B, A=Af, device_results=True, batched=True, worker=DagCholeskyWorker())
    assert mismatches(wave.lower_factor(), L, B) == (0, [])
    per_task = client.run_cholesky_dag(N, B, A=np.array(A, order="F"), device_results=True)
    assert mismatches(per_task.lower_factor(), L, B) == (0, [])


if __name__ == "__main__":
    fill_child_main() if sys.argv[1:] == ["finite-fill"] else child_main(sys.argv[2] if sys.argv[1:2] == ["cases"] else None)
