"""host/film_tools.h (the host restatement of the reference's tonemap and
imageinfo shaders, and the yardstick of the device kernels) against values
worked out by hand: tests/native/film_tools_check.cpp, compiled here with g++.
CPU only: no libigx, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")


def test_film_tools_against_hand_values(tmp_path):
    exe = str(tmp_path / "film_tools_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", HOST,
                    os.path.join(ROOT, "tests", "native", "film_tools_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
