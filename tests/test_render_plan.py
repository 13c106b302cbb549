"""The chunk plan of a render call (CPU only): host/render_plan.h works out a
call's local pixels, the automatic chunk size, capacity, iterations per chunk
and slot capacity, enumerates the chunks for both render schedules, and holds
the tail threshold and the count of a chunk's film pixels.
tests/native/render_plan_check.cpp checks valid_pixels_in_chunk against a
per-pixel count, the enumeration's invariants, the automatic chunk against the
memory budget, the tail threshold's regimes, the four refusals with their
messages, and sixteen full plans against literals worked out from the
expressions the render driver held before.  Compiled here with g++, once
optimised and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["O2", "sanitized"])
def test_render_plan(tmp_path, flags):
    exe = str(tmp_path / "render_plan_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "host"), "-I", os.path.join(PKG, "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "render_plan_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
