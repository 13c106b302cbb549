"""The C-ABI of the film post-processing entry points (igx_tonemap,
igx_imageinfo, igx_tonemap_film, igx_imageinfo_film): exported, bound with the
header's struct layouts, and bad arguments refused before anything touches the
GPU.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np

from ignis_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["igx_tonemap", "igx_imageinfo", "igx_tonemap_film", "igx_imageinfo_film"]
IGX_ERR_INVALID_ARGUMENT = 1


def test_symbols_exported_and_bound():
    L = _native.lib()
    vp = C.c_void_p
    for name in SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert L.igx_tonemap.argtypes == [vp, C.c_char_p, C.POINTER(_native.TonemapSettings), C.POINTER(C.c_uint32), C.c_size_t]
    assert L.igx_imageinfo.argtypes == [vp, C.c_char_p, C.POINTER(_native.ImageInfoSettings), C.POINTER(_native.ImageInfoOutput)]
    assert L.igx_tonemap_film.argtypes == [vp, vp, C.c_int32, C.c_int32, C.POINTER(_native.TonemapSettings), vp, C.c_int32]
    assert L.igx_imageinfo_film.argtypes == [vp, vp, C.c_int32, C.c_int32, C.POINTER(_native.ImageInfoSettings),
                                             C.POINTER(_native.ImageInfoOutput)]


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include "igx.h"\n#include <stdio.h>\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(igx_tonemap_settings), sizeof(igx_imageinfo_settings), '
                   'sizeof(igx_imageinfo_output)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_native.TonemapSettings), C.sizeof(_native.ImageInfoSettings), C.sizeof(_native.ImageInfoOutput)]
    assert sizes[0] == 20 and sizes[2] == 36


def test_null_arguments_are_refused_untouched():
    """A null handle, null settings and a null output give IGX_ERR_INVALID_ARGUMENT
    and leave the output memory alone.  The non-null "handle" is never
    dereferenced: the argument checks come first."""
    L = _native.lib()
    ts = _native.TonemapSettings(1, 0, 1.0, 1.0, 0.0)
    st = _native.ImageInfoSettings(1.0, 0, None, None, None, None, 1, 0)
    px = np.full(16, 0xDEADBEEF, dtype=np.uint32)
    pxp = px.ctypes.data_as(C.POINTER(C.c_uint32))
    out = _native.ImageInfoOutput(7, 7, 7, 7, 7, 7, 7, 7, 7)
    film = C.c_void_p(64)  # never read
    handle = C.c_void_p(C.addressof(C.create_string_buffer(8)))  # never read either
    # null handle
    assert L.igx_tonemap(None, b"", C.byref(ts), pxp, 16) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo(None, b"", C.byref(st), C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(None, film, 4, 4, C.byref(ts), C.c_void_p(px.ctypes.data), 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo_film(None, film, 4, 4, C.byref(st), C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    # null settings / null output / bad sizes, with a handle that would crash if it were used
    assert L.igx_tonemap(handle, b"", None, pxp, 16) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap(handle, b"", C.byref(ts), None, 16) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap(handle, b"", C.byref(ts), pxp, 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo(handle, b"", None, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo(handle, b"", C.byref(st), None) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(handle, film, 4, 4, None, C.c_void_p(px.ctypes.data), 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(handle, film, 4, 4, C.byref(ts), None, 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(handle, None, 4, 4, C.byref(ts), C.c_void_p(px.ctypes.data), 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(handle, film, 0, 4, C.byref(ts), C.c_void_p(px.ctypes.data), 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_tonemap_film(handle, film, 4, -1, C.byref(ts), C.c_void_p(px.ctypes.data), 0) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo_film(handle, film, 4, 4, None, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo_film(handle, film, 4, 4, C.byref(st), None) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo_film(handle, film, 4, 0, C.byref(st), C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    neg = _native.ImageInfoSettings(1.0, -1, None, None, None, None, 1, 1)
    assert L.igx_imageinfo(handle, b"", C.byref(neg), C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_imageinfo_film(handle, film, 4, 4, C.byref(neg), C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert (px == 0xDEADBEEF).all()
    assert [getattr(out, k) for k, _ in _native.ImageInfoOutput._fields_] == [7] * 9
