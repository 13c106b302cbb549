"""The denoiser's options and the symbols behind them (CPU only: loading
libigx.so needs no GPU, like igx_version)."""
import ctypes as C

import ignis_amd
from ignis_amd import _native


def test_denoiser_defaults():
    """RuntimeOptions::Denoiser (src/runtime/RuntimeSettings.h:8-9)."""
    d = ignis_amd.RuntimeOptions().Denoiser
    assert d.Enabled is False and d.FollowSpecular is False and d.OnlyFirstIteration is True
    assert ignis_amd.RuntimeOptions.makeDefault().Denoiser.Enabled is False
    # every RuntimeOptions has its own
    a, b = ignis_amd.RuntimeOptions(), ignis_amd.RuntimeOptions()
    a.Denoiser.Enabled = True
    assert b.Denoiser.Enabled is False


def test_new_symbols_resolve():
    lib = _native.lib()
    for name in ("igx_clear_aov", "igx_aov_iteration_count", "igx_write_exr_layers"):
        assert name in _native.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes
    assert lib.igx_clear_aov.argtypes == [C.c_void_p, C.c_char_p]
    assert lib.igx_aov_iteration_count.argtypes == [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]


def test_null_handles_are_refused():
    """No device, no GPU call: both entry points refuse a null handle."""
    lib = _native.lib()
    n = C.c_uint64(7)
    assert lib.igx_clear_aov(None, b"Depth") == 1  # IGX_ERR_INVALID_ARGUMENT
    assert lib.igx_aov_iteration_count(None, b"Depth", C.byref(n)) == 1
    assert n.value == 7
