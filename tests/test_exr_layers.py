"""igx_write_exr_layers (CPU only): one EXR with the channels <layer>.R/.G/.B of
the film ("Default") and the AOVs, the reference's layout of a render with
AOVs (frontend/common/IO.cpp:105-129); igx_write_exr keeps writing what it wrote."""
import numpy as np
import pytest

import ignis_amd
from exr_read import read_exr

W, H = 7, 5


def layers():
    rng = np.random.default_rng(7)
    base = rng.random((H, W, 3)).astype(np.float32)
    return {"Default": base, "Normals": base * 2 - 1, "Albedo": base[::-1].copy() + 3, "Depth": base[:, ::-1].copy() * 10}


def test_layered_file_roundtrip(tmp_path):
    path = str(tmp_path / "layers.exr")
    ls = layers()
    scales = {"Default": 0.125, "Normals": 1.0, "Albedo": 0.5, "Depth": 0.25}
    ignis_amd.write_exr_layers(path, ls, scales)
    chans, attrs = read_exr(path)
    assert set(chans) == {f"{n}.{c}" for n in ls for c in "RGB"}
    for n, img in ls.items():
        for k, c in enumerate("RGB"):
            assert chans[f"{n}.{c}"].shape == (H, W)
            np.testing.assert_array_equal(chans[f"{n}.{c}"], img[..., k] * np.float32(scales[n]))
    # distinct layers stayed distinct
    assert not np.array_equal(chans["Normals.R"], chans["Albedo.R"])
    assert not np.array_equal(chans["Depth.G"], chans["Default.G"])


def test_layer_order_does_not_matter(tmp_path):
    ls = layers()
    a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
    ignis_amd.write_exr_layers(a, ls)
    ignis_amd.write_exr_layers(b, dict(reversed(list(ls.items()))))
    assert open(a, "rb").read() == open(b, "rb").read()


def test_bad_arguments(tmp_path):
    with pytest.raises(ignis_amd.IgxError):
        ignis_amd.write_exr_layers(str(tmp_path / "x.exr"), {"A": np.zeros((H, W, 3)), "B": np.zeros((H, W + 1, 3))})
    with pytest.raises(ignis_amd.IgxError):
        ignis_amd.write_exr_layers(str(tmp_path / "x.exr"), {"": np.zeros((H, W, 3))})


def test_single_layer_writer_unchanged(tmp_path):
    """igx_write_exr still writes the plain B, G, R file: byte for byte the same
    before and after the layered writer ran, and with the values it was given."""
    path = str(tmp_path / "film.exr")
    film = layers()["Default"]
    ignis_amd.write_exr(path, film, scale=0.5)
    before = open(path, "rb").read()
    ignis_amd.write_exr_layers(str(tmp_path / "layers.exr"), layers())
    assert open(path, "rb").read() == before
    ignis_amd.write_exr(path, film, scale=0.5)
    assert open(path, "rb").read() == before
    chans, _ = read_exr(path)
    assert set(chans) == {"R", "G", "B"}
    for k, c in enumerate("RGB"):
        np.testing.assert_array_equal(chans[c], film[..., k] * np.float32(0.5))
    # header + line table + 5 scanlines of 3 channels x 7 floats, as before
    hdr = before.index(b"screenWindowWidth\x00float\x00") + len(b"screenWindowWidth\x00float\x00") + 4 + 4 + 1
    assert len(before) == hdr + H * 8 + H * (8 + 3 * W * 4)
