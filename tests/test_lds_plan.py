"""k_extend's LDS layout rule (CPU only): plan_lds of host/lds_plan.h picks the
wide layout exactly when everything fits the device's LDS per workgroup
(tests/native/lds_plan_check.cpp, compiled here with g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")


def test_lds_plan_edges(tmp_path):
    exe = str(tmp_path / "lds_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", HOST, os.path.join(ROOT, "tests", "native", "lds_plan_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
