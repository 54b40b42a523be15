"""CPU-side checks of the inverse from the factor (chol_trtri_tile / chol_potri_tile / chol_poinv_tile): the Python
wrappers exist and every entry point refuses to run before chol_init.  The numerics are in test_gpu_inverse.py."""
import pytest

from chol_testkit import assert_before_init_refused, assert_symbols_exported
from dense_linear_app_amd import chameleon as ch

SYMBOLS = ["chol_trtri_tile", "chol_potri_tile", "chol_poinv_tile"]


def test_wrappers_exist():
    for name in ("trtri", "potri", "poinv"):
        for p in "ds":
            assert callable(getattr(ch, f"CHAMELEON_{p}{name}_Tile"))
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = (ch.ChamLower, ch.ChamNonUnit, None) if sym == "chol_trtri_tile" else (ch.ChamLower, None)
    assert_before_init_refused(sym, args)
