"""The stream layout k_extend's shapes address by scalar bases (CPU only):
stream_layout and streams_offsets_32bit of host/extend_shape.h against real
pointers into packed blocks, the 4-GiB rule at, below and above the largest
chunk, and pick_extend_shape falling back to the generic kernel past it
(tests/native/stream_layout_check.cpp, compiled here with g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")


def test_stream_layout(tmp_path):
    exe = str(tmp_path / "stream_layout_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", HOST, os.path.join(ROOT, "tests", "native", "stream_layout_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
