"""The sampling table of an image environment map (host/env_cdf.h, run by
tests/native/env_cdf_check.cpp) against a numpy float32 restatement of
CDF::computeForImage (CDF.cpp:42-133), bit for bit; and the table's sampling
(host/image_texture.h, core/cdf.art) against its own pdf and the image.  CPU only."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import image_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cdf") / "env_cdf_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", HOST, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "env_cdf_check.cpp"), "-o", path], check=True)
    return path


def run(exe, tmp_path, mode, payload):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(payload)
    out = subprocess.run([exe, mode, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.frombuffer(dst.read_bytes(), np.float32)


def native_table(exe, tmp_path, rgb, compensate):
    h, w = rgb.shape[:2]
    return run(exe, tmp_path, "build", struct.pack("<3i", w, h, int(compensate)) + np.ascontiguousarray(rgb, np.float32).tobytes())


def numpy_table(rgb, compensate):
    """CDF::computeForImage with premultiplySin, every operation in float32 and every sum sequential."""
    h, w = rgb.shape[:2]
    rgb = rgb.astype(F)
    defect = np.zeros(3, F)
    if compensate:
        terms = np.maximum(rgb.reshape(-1, 3), F(0)) / F(w)
        for c in range(3):
            defect[c] = np.cumsum(np.concatenate([[F(0)], terms[:, c]]), dtype=F)[-1]
        defect = defect / F(h)
    func = np.maximum(rgb - defect, F(0))
    cell = ((func[..., 0] + func[..., 1]) + func[..., 2]) / F(3)
    cond = np.cumsum(cell, axis=1, dtype=F)
    sums = cond[:, -1].copy()
    sin = np.array([F(math.sin(float(F(F(math.pi) * F(y + 0.5)) / F(h)))) for y in range(h)], F)
    marginal = sums * sin
    rows = np.empty_like(cond)
    for y in range(h):
        if sums[y] > F(1e-5):
            rows[y] = cond[y] * (F(1) / sums[y])
        else:
            rows[y] = np.arange(w, dtype=F) * (F(1) / F(w - 1))
    rows[:, -1] = 1
    marginal = np.cumsum(marginal, dtype=F)
    if marginal[-1] > F(1e-5):
        marginal = marginal * (F(1) / marginal[-1])
    else:
        marginal = np.arange(h, dtype=F) * (F(1) / F(h - 1))
    marginal[-1] = 1
    return np.concatenate([marginal, rows.ravel()]).astype(F)


def images():
    bright = IR.texels_float64(IR.packed_expected(np.load(os.path.join(IR.TEXTURES, "single_bright_pixel.npy")), False))[..., :3]
    constant = np.full((8, 16, 3), 0.75, F)  # sums exact in float32: compensation leaves nothing, every row takes the fallback
    ys, xs = np.mgrid[0:12, 0:20]
    gradient = np.stack([xs / 19, ys / 11, (xs + ys) / 30], axis=2)
    return {"bright_pixel": bright.astype(F), "constant": constant, "gradient": gradient.astype(F)}


@pytest.mark.parametrize("compensate", [True, False])
@pytest.mark.parametrize("name", ["bright_pixel", "constant", "gradient"])
def test_table_equals_the_float32_restatement(exe, tmp_path, name, compensate):
    rgb = images()[name]
    h, w = rgb.shape[:2]
    got = native_table(exe, tmp_path, rgb, compensate)
    assert got.size == h + w * h
    marginal, rows = got[:h], got[h:].reshape(h, w)
    assert marginal[-1] == 1 and (rows[:, -1] == 1).all()
    assert (np.diff(marginal) >= 0).all() and (np.diff(rows, axis=1) >= 0).all() and marginal[0] >= 0 and (rows[:, 0] >= 0).all()
    if name == "constant" and compensate:
        np.testing.assert_array_equal(rows[:, :-1], np.broadcast_to(np.arange(w - 1, dtype=F) * (F(1) / F(w - 1)), (h, w - 1)))
    want = numpy_table(rgb, compensate)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_sampling_follows_the_image(exe, tmp_path):
    """Samples land in cells in proportion to (image - defect)+ * sin, the sample's pdf is the pdf
    looked up at its position, and u = 1 is pulled into the last cell."""
    rgb = images()["gradient"]
    h, w = rgb.shape[:2]
    table = native_table(exe, tmp_path, rgb, False)
    rng = np.random.default_rng(2)
    n = 200000
    u = rng.random((n, 2), dtype=F)
    u[:4] = [[0, 0], [1, 1], [0, 1], [1, 0]]
    out = run(exe, tmp_path, "sample", struct.pack("<3i", w, h, n) + table.tobytes() + u.tobytes()).reshape(n, 4)
    x, y, pdf, pdf_at = out.T
    assert (x >= 0).all() and (x <= 1).all() and (y >= 0).all() and (y <= 1).all()
    inside = (x < 1) & (y < 1) & (np.abs(x * w - np.round(x * w)) > 1e-3) & (np.abs(y * h - np.round(y * h)) > 1e-3)
    np.testing.assert_array_equal(pdf[inside], pdf_at[inside])
    cell = rgb.astype(np.float64).mean(axis=2) * np.sin(np.pi * (np.arange(h) + 0.5) / h)[:, None]
    want = cell / cell.sum()
    counts = np.zeros((h, w))
    np.add.at(counts, (np.minimum((y * h).astype(int), h - 1), np.minimum((x * w).astype(int), w - 1)), 1)
    sigma = np.sqrt(want * (1 - want) / n)
    assert (np.abs(counts / n - want) <= 5 * sigma + 1e-6).all()
    # the pdf integrates to one over the unit square
    marginal, rows = np.concatenate([[0], table[:h]]), np.concatenate([np.zeros((h, 1), F), table[h:].reshape(h, w)], axis=1)
    mass = (np.diff(marginal)[:, None] * np.diff(rows, axis=1)).sum()
    assert abs(mass - 1) < 1e-5
