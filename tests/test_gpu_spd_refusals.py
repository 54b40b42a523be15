"""What the entry points of spd.hip refuse, with which code and text, and in which order.

Every case is refused before a launch.  A table per entry point lists its refusals in source order: the arguments
that differ from a valid call, the return code and the full text of chol_last_error().  test_single_faults makes each
wrong argument alone; test_order makes two neighbouring rows wrong in one call, and the earlier row's code and text
must win (rows that change the same argument cannot be combined and are left out; the rows tagged ORDER are such pairs
written out by hand).  test_valid_after_refusal makes a valid call after a refused one: it returns 0, and the refusal
left every descriptor's stored image as it was.

The codes and texts were read from the entry points and confirmed by running this file against a build of the commit
before the prologue fold; some are unexpected but are the behaviour (a NULL descriptor that resident_whole meets
answers -2 whatever its position; porfs says "A is not square" of AF).  Not covered here: the P x Q and the
before-init refusals (the scaffolds of each family's own tests), a descriptor in host memory or with rectangular
tiles, a view over a user buffer, and "tile size above 4096", which needs a descriptor of 140 MB."""
import ctypes as C

import numpy as np
import pytest

from chol_testkit import desc, put_image, raw_image

pytestmark = pytest.mark.gpu

LO, UP, NOTR, TR, NONU, UNIT, LEFT, RIGHT, MAXN = 122, 121, 111, 112, 131, 132, 141, 142, 177
BAD = 7  # no enum has it
NAN = float("nan")
ORDER = "order"  # a row for test_order alone: two wrong arguments, the earlier check's refusal expected


def same(i):
    """the descriptor that argument i is in this call: an alias"""
    return ("same", i)


# out arguments (a valid call may write them)
D1, D2, F8, G8 = C.c_double(), C.c_double(), (C.c_double * 8)(), (C.c_double * 8)()
I1, PIV = C.c_int(), (C.c_int * 256)()
P1, P2, PF, PG, PI = C.byref(D1), C.byref(D2), F8, G8, C.byref(I1)
EQ5 = C.c_int(5)

# name -> (order, tile, dtype, columns); the stored tile edge is 128 except T96 (96) and T64* (64)
DESCS = {
    "A": (256, 128, "d", None), "A2": (256, 128, "d", None), "A3": (256, 128, "d", None),
    "Af": (256, 128, "s", None), "Af2": (256, 128, "s", None),
    "R": (256, 128, "d", 512),
    "b1": (256, 128, "d", 1), "b1b": (256, 128, "d", 1), "b1f": (256, 128, "s", 1),
    "b3": (256, 128, "d", 3), "b3b": (256, 128, "d", 3), "b3c": (256, 128, "d", 3),
    "b3f": (256, 128, "s", 3), "b3fb": (256, 128, "s", 3), "b3fc": (256, 128, "s", 3),
    "A64": (256, 64, "d", None), "b64": (256, 64, "d", 3), "b64b": (256, 64, "d", 3),  # a tile size that is not A's
    "T64": (64, 64, "d", None), "T64b": (64, 64, "d", None), "T64c": (64, 64, "d", None),
    "T96": (96, 96, "d", None),
    "A130": (130, 128, "d", None), "A130b": (130, 128, "d", None), "W130": (130, 128, "d", 3),
}

M64 = "stored tile edge must be a multiple of 64"
M128 = "stored tile edge must be a multiple of 128"
NOUNIT = "ChamUnit (a Cholesky factor has no unit diagonal)"
ROWS = "must have A's dtype, order and tile size"
OWN_ROWS = "must be a descriptor of its own with A's order, tile size and type"
WRULE = "W must be an n x depth descriptor of its own with A's order, tile size and type"
POW2 = "the order must be a multiple of 2^depth (border A with an identity row)"


def rbt_rows(w, a, wi, di):
    """rbt_args' refusals for `w`_tile: A at argument a (position a + 1), W at wi, depth at di"""
    return [
        ({0: BAD}, -1, f"{w}: uplo"),
        ({a: None}, -(a + 1), f"{w}: NULL A"),
        ({a: "R"}, -(a + 1), f"{w}: A is not square"),
        ({a: "T96"}, -104, f"{w}: {M64}"),
        ({a: "T64"}, -104, f"{w}: {M128}"),
        ({wi: None}, -(wi + 1), f"{w}: NULL W"),
        ({di: 3}, -(di + 1), f"{w}: depth must be 1 or 2"),
        ({wi: "b1", di: 2}, -(wi + 1), f"{w}: {WRULE}"),
        ({wi: "b3f"}, -(wi + 1), f"{w}: {WRULE}"),
        ({wi: same(a)}, -(wi + 1), f"{w}: {WRULE}"),
        ({wi: "b64"}, -(wi + 1), f"{w}: {WRULE}"),
        ({a: "A130", wi: "b64", di: 2}, -(wi + 1), f"{w}: {WRULE}", ORDER),
        ({a: "A130", wi: "W130", di: 2}, -104, f"{w}: {POW2}"),
    ]


def chud_rows(w):
    return [
        ({0: BAD}, -1, f"{w}: uplo"),
        ({1: None}, -2, f"{w}: NULL A"),
        ({2: None}, -3, f"{w}: NULL V"),
        ({2: same(1)}, -3, f"{w}: V aliases A"),
        ({1: "R"}, -2, f"{w}: A is not square"),
        ({1: "T96"}, -104, f"{w}: {M64}"),
        ({2: "b1f"}, -3, f"{w}: V {ROWS}"),
        ({2: "b64"}, -3, f"{w}: V {ROWS}"),
    ]


def stats_rows(name):
    return [({0: None}, -1, f"last_{name}_stats: NULL")]


# (entry point, a valid call, its refusals in source order)
ENTRIES = [
    ("chol_potrs_tile", (LO, "A", "b3"), [
        ({0: BAD}, -1, "potrs_tile: uplo"),
        ({1: None}, -2, "potrs_tile: NULL descriptor"),
        ({2: None}, -2, "potrs_tile: NULL descriptor"),
        ({1: "R"}, -2, "potrs_tile: A is not square"),
        ({2: "b3f"}, -3, "potrs_tile: B must have A's order, tile size and type"),
        ({2: "b64"}, -3, "potrs_tile: B must have A's order, tile size and type"),
        ({1: "T96", 2: "T96"}, -104, "potrs_tile: " + M64),
    ]),
    ("chol_posv_tile", (LO, "A", "b3"), [
        ({0: BAD}, -1, "posv_tile: uplo"),
        ({1: None}, -2, "potrf_tile: NULL descriptor"),
        ({2: None}, -2, "potrs_tile: NULL descriptor"),  # (A is factored by then)
        ({2: "b64"}, -3, "potrs_tile: B must have A's order, tile size and type"),
    ]),
    ("chol_dsposv_tile", (LO, "A", "b3", "b3b", PI), [
        ({0: BAD}, -1, "dsposv_tile: uplo"),
        ({1: None}, -2, "dsposv_tile: NULL descriptor"),
        ({1: "Af"}, -2, "dsposv_tile: A must be fp64"),
        ({1: "R"}, -2, "dsposv_tile: A is not square"),
        ({2: None}, -3, "dsposv_tile: B is NULL"),
        ({2: same(1)}, -3, "dsposv_tile: B must be fp64 with A's order and tile size"),
        ({2: "b3f"}, -3, "dsposv_tile: B must be fp64 with A's order and tile size"),
        ({2: "b64"}, -3, "dsposv_tile: B must be fp64 with A's order and tile size"),
        ({3: None}, -4, "dsposv_tile: X is NULL"),
        ({3: "b1"}, -4, "dsposv_tile: X must have B's shape, tile size and type"),
        ({2: "A2", 3: same(1)}, -4, "dsposv_tile: X aliases A or B"),
        ({3: same(2)}, -4, "dsposv_tile: X aliases A or B"),
        ({4: None}, -5, "dsposv_tile: iter is NULL"),
        ({1: "T64", 2: "T64b", 3: "T64c"}, -104, "dsposv_tile: " + M128),
    ]),
    ("chol_last_dsposv_stats", (PF,), stats_rows("dsposv")),
    ("chol_trtri_tile", (LO, NONU, "A"), [
        ({0: BAD}, -1, "trtri_tile: uplo"),
        ({1: BAD}, -2, "trtri_tile: diag"),
        ({1: UNIT}, -104, "trtri_tile: " + NOUNIT),
        ({2: None}, -2, "trtri_tile: NULL descriptor"),
        ({2: "R"}, -3, "trtri_tile: A is not square"),
        ({2: "T96"}, -104, "trtri_tile: " + M64),
    ]),
    ("chol_potri_tile", (LO, "A"), [
        ({0: BAD}, -1, "potri_tile: uplo"),
        ({1: None}, -2, "potri_tile: NULL descriptor"),
        ({1: "R"}, -2, "potri_tile: A is not square"),
        ({1: "T96"}, -104, "potri_tile: " + M64),
    ]),
    ("chol_poinv_tile", (LO, "A"), [
        ({0: BAD}, -1, "poinv_tile: uplo"),
        ({1: None}, -2, "poinv_tile: NULL descriptor"),
        ({1: "R"}, -2, "poinv_tile: A is not square"),
        ({1: "T96"}, -104, "poinv_tile: " + M64),
    ]),
    ("chol_lansy_tile", (MAXN, LO, "A", P1), [
        ({0: BAD}, -1, "lansy_tile: norm"),
        ({1: BAD}, -2, "lansy_tile: uplo"),
        ({2: None}, -2, "lansy_tile: NULL descriptor"),
        ({2: "R"}, -3, "lansy_tile: A is not square"),
        ({2: "T96"}, -104, "lansy_tile: " + M64),
        ({3: None}, -4, "lansy_tile: NULL value"),
    ]),
    ("chol_pocon_tile", (LO, "A", 1.0, P1), [
        ({0: BAD}, -1, "pocon_tile: uplo"),
        ({1: None}, -2, "pocon_tile: NULL descriptor"),
        ({1: "R"}, -2, "pocon_tile: A is not square"),
        ({1: "T96"}, -104, "pocon_tile: " + M64),
        ({2: NAN}, -3, "pocon_tile: anorm is negative or NaN"),
        ({2: -1.0}, -3, "pocon_tile: anorm is negative or NaN"),
        ({3: None}, -4, "pocon_tile: NULL rcond"),
    ]),
    ("chol_last_pocon_stats", (PF,), stats_rows("pocon")),
    ("chol_poequ_tile", ("A", "b1", P1, P2), [
        ({0: None}, -1, "poequ_tile: NULL descriptor"),
        ({0: "R"}, -1, "poequ_tile: A is not square"),
        ({0: "T96"}, -104, "poequ_tile: " + M64),
        ({1: None}, -2, "poequ_tile: S is NULL"),
        ({1: "b1f"}, -2, "poequ_tile: S " + ROWS),
        ({1: "b64"}, -2, "poequ_tile: S " + ROWS),
        ({1: same(0)}, -2, "poequ_tile: S must be an n x 1 descriptor of its own"),
        ({1: "b3"}, -2, "poequ_tile: S must be an n x 1 descriptor of its own"),
        ({2: None}, -3, "poequ_tile: NULL scond"),
        ({3: None}, -4, "poequ_tile: NULL amax"),
    ]),
    ("chol_laqsy_tile", (LO, "A", "b1", 1.0, 1.0, PI), [
        ({0: BAD}, -1, "laqsy_tile: uplo"),
        ({1: None}, -2, "laqsy_tile: NULL descriptor"),
        ({1: "R"}, -2, "laqsy_tile: A is not square"),
        ({1: "T96"}, -104, "laqsy_tile: " + M64),
        ({2: None}, -3, "laqsy_tile: S is NULL"),
        ({2: "b64"}, -3, "laqsy_tile: S " + ROWS),
        ({2: "b3"}, -3, "laqsy_tile: S must be an n x 1 descriptor of its own"),
        ({3: NAN}, -4, "laqsy_tile: scond is negative or NaN"),
        ({3: -1.0}, -4, "laqsy_tile: scond is negative or NaN"),
        ({4: NAN}, -5, "laqsy_tile: amax is negative or NaN"),
        ({4: -1.0}, -5, "laqsy_tile: amax is negative or NaN"),
        ({5: None}, -6, "laqsy_tile: NULL equed"),
    ]),
    ("chol_porfs_tile", (LO, "A", "A2", "b3", "b3b", PF, PG), [
        ({0: BAD}, -1, "porfs_tile: uplo"),
        ({1: None}, -2, "porfs_tile: NULL descriptor"),
        ({1: "R"}, -2, "porfs_tile: A is not square"),
        ({1: "T96"}, -104, "porfs_tile: " + M64),
        ({2: None}, -3, "porfs_tile: NULL descriptor"),
        ({2: "R"}, -3, "porfs_tile: A is not square"),
        ({2: "Af"}, -3, "porfs_tile: AF must have A's shape, tile size and type, in storage of its own"),
        ({2: "A64"}, -3, "porfs_tile: AF must have A's shape, tile size and type, in storage of its own"),
        ({2: same(1)}, -3, "porfs_tile: AF must have A's shape, tile size and type, in storage of its own"),
        ({3: None}, -4, "porfs_tile: B is NULL"),
        ({3: "b64"}, -4, "porfs_tile: B " + ROWS),
        ({4: None}, -5, "porfs_tile: X is NULL"),
        ({4: "b64"}, -5, "porfs_tile: X " + ROWS),
        ({4: "b1"}, -5, "porfs_tile: X must have B's shape, tile size and type"),
        ({3: same(1), 4: "A3"}, -5, "porfs_tile: X aliases A, AF or B"),
        ({4: same(3)}, -5, "porfs_tile: X aliases A, AF or B"),
        ({5: None}, -6, "porfs_tile: NULL ferr"),
        ({6: None}, -7, "porfs_tile: NULL berr"),
    ]),
    ("chol_posvx_tile", (0, LO, "A", "A2", PI, None, "b3", "b3b", P1, PF, PG), [
        ({0: BAD}, -1, "posvx_tile: fact"),
        ({1: BAD}, -2, "posvx_tile: uplo"),
        ({2: None}, -3, "posvx_tile: NULL descriptor"),
        ({2: "R"}, -3, "posvx_tile: A is not square"),
        ({2: "T96"}, -104, "posvx_tile: " + M64),
        ({3: None}, -4, "posvx_tile: NULL descriptor"),
        ({3: "A64"}, -4, "posvx_tile: AF must have A's shape, tile size and type, in storage of its own"),
        ({3: same(2)}, -4, "posvx_tile: AF must have A's shape, tile size and type, in storage of its own"),
        ({6: None}, -7, "posvx_tile: B is NULL"),
        ({6: "b64"}, -7, "posvx_tile: B " + ROWS),
        ({7: None}, -8, "posvx_tile: X is NULL"),
        ({7: "b1"}, -8, "posvx_tile: X must have B's shape, tile size and type"),
        ({7: same(6)}, -8, "posvx_tile: X aliases A, AF or B"),
        ({4: None}, -5, "posvx_tile: NULL equed"),
        ({0: 2, 4: EQ5}, -5, "posvx_tile: equed must be 0 or 1"),
        ({0: 2, 4: EQ5, 5: "b3"}, -5, "posvx_tile: equed must be 0 or 1", ORDER),
        ({0: 1, 5: None}, -6, "posvx_tile: S is NULL"),
        ({5: "b64"}, -6, "posvx_tile: S " + ROWS),
        ({5: "b3"}, -6, "posvx_tile: S must be an n x 1 descriptor of its own"),
        ({5: "b1", 6: "b1", 7: "b1b"}, -6, "posvx_tile: S must be an n x 1 descriptor of its own"),
        ({5: "b3", 8: None}, -6, "posvx_tile: S must be an n x 1 descriptor of its own", ORDER),
        ({8: None}, -9, "posvx_tile: NULL rcond"),
        ({9: None}, -10, "posvx_tile: NULL ferr"),
        ({10: None}, -11, "posvx_tile: NULL berr"),
    ]),
    ("chol_bench_refine", (LO, "A", "A2", "b3", 0, 1, P1), [
        ({0: BAD}, -1, "bench_refine: uplo"),
        ({1: None}, -2, "bench_refine: NULL descriptor"),
        ({1: "R"}, -2, "bench_refine: A is not square"),
        ({2: None}, -3, "bench_refine: NULL descriptor"),
        ({2: "R"}, -3, "bench_refine: A is not square"),
        ({3: None}, -4, "bench_refine: X is NULL"),
        ({3: "b64"}, -4, "bench_refine: X " + ROWS),
        ({4: -1}, -5, "bench_refine: path, reps or ms"),
        ({4: 3}, -5, "bench_refine: path, reps or ms"),
        ({5: 0}, -5, "bench_refine: path, reps or ms"),
        ({6: None}, -5, "bench_refine: path, reps or ms"),
    ]),
    ("chol_last_posvx_stats", (PF,), stats_rows("posvx")),
    ("chol_pstrf_tile", (LO, "A", PIV, PI, -1.0), [
        ({0: BAD}, -1, "pstrf_tile: uplo"),
        ({1: None}, -2, "pstrf_tile: NULL descriptor"),
        ({1: "R"}, -2, "pstrf_tile: A is not square"),
        ({2: None}, -3, "pstrf_tile: NULL piv"),
        ({3: None}, -4, "pstrf_tile: NULL rank"),
        ({4: NAN}, -5, "pstrf_tile: tol is NaN"),
    ]),
    ("chol_last_pstrf_stats", (PF,), stats_rows("pstrf")),
    ("chol_sygst_tile", (1, LO, "A", "A2"), [
        ({0: 0}, -1, "sygst_tile: itype"),
        ({0: 4}, -1, "sygst_tile: itype"),
        ({1: BAD}, -2, "sygst_tile: uplo"),
        ({2: None}, -3, "sygst_tile: NULL A"),
        ({3: None}, -4, "sygst_tile: NULL B"),
        ({3: same(2)}, -4, "sygst_tile: B aliases A"),
        ({2: "R"}, -3, "sygst_tile: A is not square"),
        ({2: "T96"}, -104, "sygst_tile: " + M64),
        ({3: "R"}, -4, "sygst_tile: A is not square"),
        ({3: "Af"}, -4, "sygst_tile: B's dtype or geometry differs from A's"),
        ({3: "A64"}, -4, "sygst_tile: B's dtype or geometry differs from A's"),
        ({0: 2}, -104, "sygst_tile: itype 2 and 3 (C = L^T A L)"),
        ({0: 3}, -104, "sygst_tile: itype 2 and 3 (C = L^T A L)"),
        ({0: 2, 3: same(2)}, -4, "sygst_tile: B aliases A", ORDER),  # (the alias is looked for before the view refresh)
    ]),
    ("chol_last_sygst_stats", (PF,), stats_rows("sygst")),
    ("chol_chud_tile", (LO, "A", "b1"), chud_rows("chud_tile")),
    ("chol_chdd_tile", (LO, "A", "b1"), chud_rows("chdd_tile")),
    ("chol_last_chud_stats", (PF,), stats_rows("chud")),
    ("chol_chex_tile", (LO, "A", 1, 5, 1), [
        ({0: BAD}, -1, "chex_tile: uplo"),
        ({1: None}, -2, "chex_tile: NULL A"),
        ({1: "R"}, -2, "chex_tile: A is not square"),
        ({1: "T96"}, -104, "chex_tile: " + M64),
        ({2: 257}, -3, "chex_tile: k outside 1..n"),
        ({2: 0}, -3, "chex_tile: k outside 1..n"),
        ({3: 0}, -4, "chex_tile: l outside k..n"),
        ({3: 257}, -4, "chex_tile: l outside k..n"),
        ({4: 0}, -5, "chex_tile: job must be 1 (right shift) or 2 (left shift)"),
        ({4: 3}, -5, "chex_tile: job must be 1 (right shift) or 2 (left shift)"),
    ]),
    ("chol_last_chex_stats", (PF,), stats_rows("chex")),
    ("chol_trtrs_tile", (LO, NOTR, NONU, "A", "b3"), [
        ({0: BAD}, -1, "trtrs_tile: uplo"),
        ({1: BAD}, -2, "trtrs_tile: trans"),
        ({2: BAD}, -3, "trtrs_tile: diag"),
        ({3: None}, -4, "trtrs_tile: NULL A"),
        ({4: None}, -5, "trtrs_tile: NULL B"),
        ({4: same(3)}, -5, "trtrs_tile: B aliases A"),
        ({3: "R"}, -4, "trtrs_tile: A is not square"),
        ({3: "T96"}, -104, "trtrs_tile: " + M64),
        ({4: "b3f"}, -5, "trtrs_tile: B " + ROWS),
        ({4: "b64"}, -5, "trtrs_tile: B " + ROWS),
        ({2: UNIT}, -104, "trtrs_tile: " + NOUNIT),
        ({2: UNIT, 4: same(3)}, -5, "trtrs_tile: B aliases A", ORDER),
    ]),
    ("chol_trmm_tile", (LEFT, LO, NOTR, NONU, 1.0, "A", "b3"), [
        ({0: BAD}, -1, "trmm_tile: side"),
        ({1: BAD}, -2, "trmm_tile: uplo"),
        ({2: BAD}, -3, "trmm_tile: trans"),
        ({3: BAD}, -4, "trmm_tile: diag"),
        ({5: None}, -6, "trmm_tile: NULL A"),
        ({6: None}, -7, "trmm_tile: NULL B"),
        ({6: same(5)}, -7, "trmm_tile: B aliases A"),
        ({5: "R"}, -6, "trmm_tile: A is not square"),
        ({5: "T96"}, -104, "trmm_tile: " + M64),
        ({6: "b3f"}, -7, "trmm_tile: B " + ROWS),
        ({6: "b64"}, -7, "trmm_tile: B " + ROWS),
        ({0: RIGHT}, -104, "trmm_tile: ChamRight"),
        ({3: UNIT}, -104, "trmm_tile: " + NOUNIT),
        ({0: RIGHT, 6: same(5)}, -7, "trmm_tile: B aliases A", ORDER),
    ]),
    ("chol_symm_tile", (LEFT, LO, 1.0, "A", "b3", 0.0, "b3b"), [
        ({0: BAD}, -1, "symm_tile: side"),
        ({1: BAD}, -2, "symm_tile: uplo"),
        ({3: None}, -4, "symm_tile: NULL A"),
        ({4: None}, -5, "symm_tile: NULL B"),
        ({6: None}, -7, "symm_tile: NULL C"),
        ({6: same(3)}, -7, "symm_tile: C aliases A or B"),
        ({6: same(4)}, -7, "symm_tile: C aliases A or B"),
        ({3: "R"}, -4, "symm_tile: A is not square"),
        ({3: "T96"}, -104, "symm_tile: " + M64),
        ({4: "b3f"}, -5, "symm_tile: B " + ROWS),
        ({4: "b64"}, -5, "symm_tile: B " + ROWS),
        ({6: "b64b"}, -7, "symm_tile: C " + ROWS),
        ({6: "b1"}, -7, "symm_tile: C must have B's width"),
        ({0: RIGHT}, -104, "symm_tile: ChamRight"),
        ({0: RIGHT, 6: same(4)}, -7, "symm_tile: C aliases A or B", ORDER),
    ]),
    ("chol_last_symm_stats", (PF,), stats_rows("symm")),
    ("chol_logdet_tile", ("A", P1), [
        ({0: None}, -1, "logdet_tile: NULL A"),
        ({0: "R"}, -1, "logdet_tile: A is not square"),
        ({0: "T96"}, -104, "logdet_tile: " + M64),
        ({1: None}, -2, "logdet_tile: NULL logdet"),
    ]),
    ("chol_last_trtrs_stats", (PF,), stats_rows("trtrs")),
    ("chol_debug_half_limits", (-1, -1), []),  # (refuses nothing)
    ("chol_sytrf_nopiv_tile", (LO, "A"), [
        ({0: BAD}, -1, "sytrf_nopiv_tile: uplo"),
        ({1: None}, -2, "sytrf_nopiv_tile: NULL A"),
        ({1: "R"}, -2, "sytrf_nopiv_tile: A is not square"),
        ({1: "T96"}, -104, "sytrf_nopiv_tile: " + M64),
        ({1: "T64"}, -104, "sytrf_nopiv_tile: " + M128),
    ]),
    ("chol_sytrs_nopiv_tile", (LO, "A", "b3"), [
        ({0: BAD}, -1, "sytrs_nopiv_tile: uplo"),
        ({1: None}, -2, "sytrs_nopiv_tile: NULL A"),
        ({2: None}, -3, "sytrs_nopiv_tile: NULL B"),
        ({2: same(1)}, -3, "sytrs_nopiv_tile: B aliases A"),
        ({1: "R"}, -2, "sytrs_nopiv_tile: A is not square"),
        ({1: "T96"}, -104, "sytrs_nopiv_tile: " + M64),
        ({2: "b3f"}, -3, "sytrs_nopiv_tile: B must have A's order, tile size and type"),
        ({2: "b64"}, -3, "sytrs_nopiv_tile: B must have A's order, tile size and type"),
    ]),
    ("chol_sysv_nopiv_tile", (LO, "A", "b3"), [
        ({0: BAD}, -1, "sysv_nopiv_tile: uplo"),
        ({1: None}, -2, "sysv_nopiv_tile: NULL A"),
        ({2: None}, -3, "sysv_nopiv_tile: NULL B"),
        ({1: "R"}, -2, "sytrf_nopiv_tile: A is not square"),
        ({1: "T96"}, -104, "sytrf_nopiv_tile: " + M64),
        ({1: "T64"}, -104, "sytrf_nopiv_tile: " + M128),
        ({2: same(1)}, -3, "sytrs_nopiv_tile: B aliases A"),  # (A is factored by then, here and below)
        ({2: "b64"}, -3, "sytrs_nopiv_tile: B must have A's order, tile size and type"),
    ]),
    ("chol_last_sytrf_stats", (PF,), stats_rows("sytrf")),
    ("chol_rbt_apply_tile", (LO, "A", "b3", 1), rbt_rows("rbt_apply_tile", 1, 2, 3)),
    ("chol_sytrf_rbt_tile", (LO, "A", "b3", 1, 1), rbt_rows("sytrf_rbt_tile", 1, 2, 3)),
    ("chol_sytrs_rbt_tile", (LO, "A", "b3", 1, "b3b"), rbt_rows("sytrs_rbt_tile", 1, 2, 3) + [
        ({4: None}, -5, "sytrs_rbt_tile: NULL B"),
        ({4: "b64"}, -5, "sytrs_rbt_tile: B " + OWN_ROWS),
        ({4: same(1)}, -5, "sytrs_rbt_tile: B " + OWN_ROWS),
        ({4: same(2)}, -5, "sytrs_rbt_tile: B " + OWN_ROWS),
    ]),
    ("chol_sysv_rbt_tile", (LO, "A", "A2", "b3", 1, 1, "b3b", "b3c", PI, PG), [
        ({0: BAD}, -1, "sysv_rbt_tile: uplo"),
        ({1: None}, -2, "sysv_rbt_tile: NULL A"),
        ({1: "R"}, -2, "sysv_rbt_tile: A is not square"),
        ({1: "T96"}, -104, "sysv_rbt_tile: " + M64),
        ({2: None}, -3, "sysv_rbt_tile: NULL AF"),
        ({2: "A64"}, -3, "sysv_rbt_tile: AF must be a descriptor of its own with A's geometry and type"),
        ({2: same(1)}, -3, "sysv_rbt_tile: AF must be a descriptor of its own with A's geometry and type"),
        ({1: "T64", 2: "T64b"}, -104, "sysv_rbt_tile: " + M128),
        ({3: None}, -4, "sysv_rbt_tile: NULL W"),
        ({4: 3}, -5, "sysv_rbt_tile: depth must be 1 or 2"),
        ({3: "b1", 4: 2}, -4, "sysv_rbt_tile: " + WRULE),
        ({3: same(2)}, -4, "sysv_rbt_tile: " + WRULE),
        ({3: "b64"}, -4, "sysv_rbt_tile: " + WRULE),
        ({1: "A130", 2: "A130b", 3: "b64", 4: 2}, -4, "sysv_rbt_tile: " + WRULE, ORDER),
        ({1: "A130", 2: "A130b", 3: "W130", 4: 2}, -104, "sysv_rbt_tile: " + POW2),
        ({3: same(1)}, -4, "sysv_rbt_tile: W aliases A"),
        ({6: None}, -7, "sysv_rbt_tile: NULL B"),
        ({6: "b64"}, -7, "sysv_rbt_tile: B " + OWN_ROWS),
        ({6: same(3)}, -7, "sysv_rbt_tile: B " + OWN_ROWS),
        ({7: None}, -8, "sysv_rbt_tile: NULL X"),
        ({7: "b1"}, -8, "sysv_rbt_tile: X must be a descriptor of its own with B's shape, tile size and type"),
        ({7: same(6)}, -8, "sysv_rbt_tile: X must be a descriptor of its own with B's shape, tile size and type"),
        ({8: None}, -9, "sysv_rbt_tile: NULL iter"),
        ({1: "Af", 2: "Af2", 3: "b3f", 6: "b3fb", 7: "b3fc"}, -104,
         "sysv_rbt_tile: fp32 (the residual pass is fp64: use sytrf_rbt / sytrs_rbt)"),
    ]),
    ("chol_last_rbt_stats", (PF,), stats_rows("rbt")),
]
IDS = [e[0] for e in ENTRIES]


class World:
    """the descriptors, filled once: the squares with one well-conditioned SPD matrix (A2 with its Cholesky factor, so
    that (A, A2) is a matrix with its factor), the others with random numbers; and their images to put back"""

    def __init__(self, ch):
        from dense_linear_app_amd._lib import lib

        self.ch, self.lib = ch, lib()
        rng = np.random.default_rng(54)
        self.d, self.img = {}, {}
        for name, (n, tile, dt, cols) in DESCS.items():
            if cols is None:
                G = rng.standard_normal((n, n))
                X = (G + G.T) / 8 + n * np.eye(n)
                if name == "A2":
                    X = np.linalg.cholesky(self.spd)
                elif name == "A":
                    self.spd = X
                else:
                    X = self.spd if n == 256 else X
            else:
                X = rng.standard_normal((n, cols))
            self.d[name] = desc(ch, n, tile, dt, cols, content=X)
            self.img[name] = raw_image(self.d[name])

    def restore(self):
        for name, d in self.d.items():
            put_image(d, self.img[name])

    def call(self, fn, valid, mut=None):
        """-> (return code, chol_last_error()) of fn on the valid arguments changed by mut"""
        args = list(valid)
        mut = mut or {}
        for i, v in mut.items():
            if not (isinstance(v, tuple) and v[0] == "same"):
                args[i] = v
        for i, v in mut.items():
            if isinstance(v, tuple) and v[0] == "same":
                args[i] = args[v[1]]
        args = [self.d[a].handle if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, fn)(*args)
        return rc, self.lib.chol_last_error().decode()

    def close(self):
        for d in self.d.values():
            self.ch.CHAMELEON_Desc_Destroy(d)


@pytest.fixture(scope="module")
def world(cham):
    w = World(cham)
    yield w
    w.close()


def check(world, fn, valid, cases):
    """every case's call gives its code and text (all are made; the ones that differ are listed)"""
    got = [(mut, world.call(fn, valid, mut)) for mut, _, _ in cases]
    wrong = [(mut, g, (code, text)) for (mut, g), (_, code, text) in zip(got, cases) if g != (code, text)]
    assert not wrong, (fn, wrong)


@pytest.mark.parametrize("fn,valid,rows", ENTRIES, ids=IDS)
def test_single_faults(world, fn, valid, rows):
    world.restore()
    check(world, fn, valid, [r for r in rows if len(r) == 3])


@pytest.mark.parametrize("fn,valid,rows", ENTRIES, ids=IDS)
def test_order(world, fn, valid, rows):
    world.restore()
    plain = [r for r in rows if len(r) == 3]
    cases = [({**later[0], **first[0]}, first[1], first[2])
             for first, later in zip(plain, plain[1:]) if not set(first[0]) & set(later[0])]
    cases += [r[:3] for r in rows if len(r) == 4]
    check(world, fn, valid, cases)


@pytest.mark.parametrize("fn,valid,rows", ENTRIES, ids=IDS)
def test_valid_after_refusal(world, fn, valid, rows):
    """the entry point's first refusal (or none, where it refuses nothing), then the valid call"""
    world.restore()
    for mut, code, text, *_ in rows[:1]:
        assert world.call(fn, valid, mut) == (code, text)
    for name, d in world.d.items():
        assert np.array_equal(raw_image(d), world.img[name]), (fn, name)
    rc, text = world.call(fn, valid)
    assert rc == 0, (fn, rc, text)
