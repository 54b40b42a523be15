"""CPU-side checks of the condition estimate (chol_lansy_tile / chol_pocon_tile / chol_last_pocon_stats): the Python
wrappers and ABI symbols exist and every entry point refuses to run before chol_init.  The numerics are in
test_gpu_pocon.py."""
import pytest

from dense_linear_app_amd import _lib, chameleon as ch

SYMBOLS = ["chol_lansy_tile", "chol_pocon_tile", "chol_last_pocon_stats"]


def test_wrappers_exist():
    for name in ("lansy", "pocon"):
        for p in "ds":
            assert callable(getattr(ch, f"CHAMELEON_{p}{name}_Tile"))
    assert callable(ch.last_pocon_stats)
    for s in SYMBOLS:
        assert s in _lib.abi_symbols()


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    L = _lib.lib()
    args = {"chol_lansy_tile": (ch.ChamOneNorm, ch.ChamLower, None, None),
            "chol_pocon_tile": (ch.ChamLower, None, 1.0, None),
            "chol_last_pocon_stats": (None,)}[sym]
    assert getattr(L, sym)(*args) == -101  # CHOL_ERR_NOT_INITIALIZED
    assert b"before chol_init" in L.chol_last_error()
