"""The scene-table builder (CPU only): host/scene_tables.cpp turns an
igx_scene_desc into the device's flat tables.  tests/native/scene_tables_check.cpp
builds its scenes in memory and checks node references, BLAS leaves, Tri1
records, instance flags, entity records, light order and remap, stack depth,
node width, the hot order, enclosing entities, every refusal's status and
message, and the full-shading decision.  Compiled here with g++ against
scene_tables.cpp, bvh_build.cpp and light_select.cpp, once optimised and once
with the address and undefined-behaviour sanitizers (the refusals index
caller-supplied arrays)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")
HOST = os.path.join(PKG, "host")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["O2", "sanitized"])
def test_scene_tables(tmp_path, flags):
    exe = str(tmp_path / "scene_tables_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-I", HOST, "-I", os.path.join(PKG, "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "scene_tables_check.cpp"),
                    os.path.join(HOST, "scene_tables.cpp"), os.path.join(HOST, "bvh_build.cpp"),
                    os.path.join(HOST, "light_select.cpp"), "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
