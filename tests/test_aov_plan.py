"""The AOV name table and the schedule of the denoiser's info-buffer pass
(CPU only): info_pass_due / info_passes_in / aov_lookup of host/aov_plan.h,
which the driver uses (tests/native/aov_plan_check.cpp, compiled here with g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")


def test_aov_plan_edges(tmp_path):
    exe = str(tmp_path / "aov_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", HOST, os.path.join(ROOT, "tests", "native", "aov_plan_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
