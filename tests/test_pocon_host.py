"""CPU-side checks of the condition estimate (chol_lansy_tile / chol_pocon_tile / chol_last_pocon_stats): the Python
wrappers and ABI symbols exist and every entry point refuses to run before chol_init.  The numerics are in
test_gpu_pocon.py."""
import pytest

from chol_testkit import assert_before_init_refused, assert_symbols_exported
from dense_linear_app_amd import chameleon as ch

SYMBOLS = ["chol_lansy_tile", "chol_pocon_tile", "chol_last_pocon_stats"]


def test_wrappers_exist():
    for name in ("lansy", "pocon"):
        for p in "ds":
            assert callable(getattr(ch, f"CHAMELEON_{p}{name}_Tile"))
    assert callable(ch.last_pocon_stats)
    assert_symbols_exported(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    args = {"chol_lansy_tile": (ch.ChamOneNorm, ch.ChamLower, None, None),
            "chol_pocon_tile": (ch.ChamLower, None, 1.0, None),
            "chol_last_pocon_stats": (None,)}[sym]
    assert_before_init_refused(sym, args)
