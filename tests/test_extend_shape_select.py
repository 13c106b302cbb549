"""k_extend's launch-shape rule (CPU only): pick_extend_shape of
host/extend_shape.h gives a launch the generate or the bounce shape exactly
when it runs the default fused mode and option "extend_shapes" allows it, and
the generate shape only to a launch that builds its camera paths
(tests/native/extend_shape_check.cpp, compiled here with g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")


def test_extend_shape_grid(tmp_path):
    exe = str(tmp_path / "extend_shape_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", HOST, os.path.join(ROOT, "tests", "native", "extend_shape_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
