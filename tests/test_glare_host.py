"""host/glare_model.h (the arithmetic of the daylight glare kernel k_glare_scan
and of its host restatement glare_host) against closed forms and float64:
tests/native/glare_check.cpp, compiled here with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own.  And the C-ABI
of igx_evaluate_glare / igx_evaluate_glare_film: exported, bound with the
header's struct layouts, bad arguments refused before anything touches the GPU.
CPU only."""
import ctypes as C
import os
import subprocess

from ignis_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")
IGX_ERR_INVALID_ARGUMENT = 1


def test_glare_model_against_closed_forms_and_float64(tmp_path):
    exe = str(tmp_path / "glare_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "native", "glare_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr[-4000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr[-4000:]


def test_symbols_exported_and_bound():
    L = _native.lib()
    vp = C.c_void_p
    for name in ("igx_evaluate_glare", "igx_evaluate_glare_film"):
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert L.igx_evaluate_glare.argtypes == [vp, C.c_char_p, C.POINTER(_native.GlareSettings), vp, C.c_size_t,
                                             C.POINTER(_native.GlareOutput)]
    assert L.igx_evaluate_glare_film.argtypes == [vp, vp, C.c_int32, C.c_int32, C.POINTER(_native.GlareSettings), vp, C.c_int32,
                                                  C.POINTER(_native.GlareOutput)]


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include "igx.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(igx_glare_settings), sizeof(igx_glare_output), '
                   'offsetof(igx_glare_settings, vertical_illuminance), offsetof(igx_glare_output, num_pixels)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_native.GlareSettings), C.sizeof(_native.GlareOutput),
                     _native.GlareSettings.vertical_illuminance.offset, _native.GlareOutput.num_pixels.offset]
    assert sizes == [20, 20, 16, 16]


def test_null_arguments_are_refused_untouched():
    """A null handle, null settings, a null output and a bad film size give
    IGX_ERR_INVALID_ARGUMENT and leave the output alone; the non-null "handle"
    is never dereferenced, the argument checks come first."""
    L = _native.lib()
    gs = _native.GlareSettings(1.0, 8.0, 0.25, 5.0, -1.0)
    out = _native.GlareOutput(7, 7, 7, 7, 7)
    film = C.c_void_p(64)  # never read
    handle = C.c_void_p(C.addressof(C.create_string_buffer(8)))  # never read either
    assert L.igx_evaluate_glare(None, b"", C.byref(gs), None, 16, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare(handle, b"", None, None, 16, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare(handle, b"", C.byref(gs), None, 16, None) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(None, film, 4, 4, C.byref(gs), None, 0, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(handle, None, 4, 4, C.byref(gs), None, 0, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(handle, film, 4, 4, None, None, 0, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(handle, film, 4, 4, C.byref(gs), None, 0, None) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(handle, film, 0, 4, C.byref(gs), None, 0, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert L.igx_evaluate_glare_film(handle, film, 4, -1, C.byref(gs), None, 0, C.byref(out)) == IGX_ERR_INVALID_ARGUMENT
    assert [getattr(out, k) for k, _ in _native.GlareOutput._fields_] == [7] * 5
