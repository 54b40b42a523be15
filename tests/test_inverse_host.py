"""CPU-side checks of the inverse from the factor (chol_trtri_tile / chol_potri_tile / chol_poinv_tile): the Python
wrappers exist and every entry point refuses to run before chol_init.  The numerics are in test_gpu_inverse.py."""
import pytest

from dense_linear_app_amd import _lib, chameleon as ch

SYMBOLS = ["chol_trtri_tile", "chol_potri_tile", "chol_poinv_tile"]


def test_wrappers_exist():
    for name in ("trtri", "potri", "poinv"):
        for p in "ds":
            assert callable(getattr(ch, f"CHAMELEON_{p}{name}_Tile"))
    for s in SYMBOLS:
        assert s in _lib.abi_symbols()


@pytest.mark.parametrize("sym", SYMBOLS)
def test_before_init_is_refused(sym):
    L = _lib.lib()
    args = (ch.ChamLower, ch.ChamNonUnit, None) if sym == "chol_trtri_tile" else (ch.ChamLower, None)
    assert getattr(L, sym)(*args) == -101  # CHOL_ERR_NOT_INITIALIZED
    assert b"before chol_init" in L.chol_last_error()
