"""CPU-side checks of the mixed-precision solve's boundary (chol_dsposv_tile / chol_last_dsposv_stats): the Python
wrapper exists and both entry points refuse to run before chol_init.  The numerics are in test_gpu_dsposv.py."""
import ctypes as C

from dense_linear_app_amd import _lib, chameleon as ch


def test_wrapper_exists():
    assert callable(ch.CHAMELEON_dsposv_Tile)
    assert callable(ch.last_dsposv_stats)
    assert "chol_dsposv_tile" in _lib.abi_symbols()


def test_dsposv_before_init_is_refused():
    L = _lib.lib()
    it = C.c_int(7)
    assert L.chol_dsposv_tile(ch.ChamLower, None, None, None, C.byref(it)) == -101  # CHOL_ERR_NOT_INITIALIZED
    assert b"before chol_init" in L.chol_last_error()
    assert it.value == 7


def test_last_dsposv_stats_before_init_is_refused():
    L = _lib.lib()
    assert L.chol_last_dsposv_stats(None) == -101  # CHOL_ERR_NOT_INITIALIZED
    assert b"before chol_init" in L.chol_last_error()
