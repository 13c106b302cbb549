"""Film post-processing on the device: the tonemap / imageinfo kernels against
the host loops of host/film_tools.h (tests/native/film_post_check.cpp), and a
known answer through the Python Runtime and igcli: a camera that sees only a
constant environment, so every pixel of the film is the same radiance E."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

import ignis_amd
from conftest import ENV_LIGHT, flat_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")

# binary fractions: spi samples of E times 1 / spi, added over two iterations, are exact
E = [0.5, 0.25, 0.125]
Y_E = 0.2126729 * E[0] + 0.7151522 * E[1] + 0.0721750 * E[2]
W, H = 48, 32


def test_kernels_against_host_loops(tmp_path):
    exe = str(tmp_path / "film_post_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"), "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "film_post_check.cpp"), "-o", exe, "-L", PKG, "-ligx",
                    f"-Wl,-rpath,{PKG}", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-6000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-6000:] + out.stderr[-2000:]


def env_only_scene():
    """flat_scene with the environment as the only light and the camera turned
    away from the ground plane (half a turn about y)."""
    sc = flat_scene([dict(ENV_LIGHT, radiance=E)])
    sc = copy.deepcopy(sc)
    sc["film"] = {"size": [W, H]}
    sc["camera"]["transform"] = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, -1]
    return sc


@pytest.fixture(scope="module")
def runtime():
    opts = ignis_amd.RuntimeOptions.makeDefault()
    opts.SPI = 4
    rt = ignis_amd.Runtime(ignis_amd.Scene.from_string(env_only_scene()), opts)
    rt.step()
    rt.step()
    yield rt
    rt.close()


def test_film_is_the_environment(runtime):
    fb = runtime.getFramebufferForHost()
    assert runtime.IterationCount == 2
    np.testing.assert_array_equal(fb, np.broadcast_to(np.float32(2) * np.array(E, np.float32), (H, W, 3)))


def test_runtime_tonemap_reinhard_closed_form(runtime):
    img = runtime.tonemap(method=1)
    assert img.shape == (H, W) and img.dtype == np.uint32
    assert (img == img[0, 0]).all()
    t = Y_E / (1 + Y_E)  # Reinhard on the luminance; the chromaticity is kept, so sRGB = E * t / Y
    p = int(img[0, 0])
    assert p >> 24 == 255
    for k, shift in enumerate((16, 8, 0)):
        assert abs(((p >> shift) & 255) - int(E[k] * t / Y_E * 255)) <= 1, hex(p)
    # an explicit film pointer with the same scale gives the same image
    ptr, count = runtime.device.framebuffer_device_ptr()
    assert count == W * H * 3
    np.testing.assert_array_equal(runtime.device.tonemap_film(ptr, W, H, method=1, scale=1 / 2), img)
    # gamma: the sRGB curve on each channel
    g = int(runtime.tonemap(method=1, use_gamma=True)[H - 1, W - 1])
    for k, shift in enumerate((16, 8, 0)):
        assert abs(((g >> shift) & 255) - int((1.055 * (E[k] * t / Y_E) ** (1 / 2.4) - 0.055) * 255)) <= 1, hex(g)


def test_runtime_imageinfo_constant_film(runtime):
    info = runtime.imageinfo(bins=8)
    assert info["min"] == info["max"]
    assert abs(info["avg"] - Y_E) <= 1e-5 * Y_E and abs(info["min"] - Y_E) <= 1e-6 * Y_E
    assert info["soft_min"] == info["min"] and info["soft_max"] == info["max"]
    assert abs(info["median"] - Y_E) <= 1e-5 * Y_E
    assert (info["inf_count"], info["nan_count"], info["neg_count"]) == (0, 0, 0)
    # min == max: the histograms span [0, 1] (start = 0, end = start + 1), so bin = int(v * 8)
    for key, v in (("histogram_r", E[0]), ("histogram_g", E[1]), ("histogram_b", E[2]), ("histogram_l", Y_E)):
        want = np.zeros(8, np.int32)
        want[int(v * 8)] = W * H
        np.testing.assert_array_equal(info[key], want, err_msg=key)
    ptr, _ = runtime.device.framebuffer_device_ptr()
    again = runtime.device.imageinfo_film(ptr, W, H, scale=1 / 2, bins=8)
    assert {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in again.items()} == \
           {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items()}
    assert "histogram_l" not in runtime.imageinfo()


def test_unknown_aov_is_an_error(runtime):
    with pytest.raises(ignis_amd.IgxError, match="unknown aov"):
        runtime.tonemap("Bogus")
    with pytest.raises(ignis_amd.IgxError, match="unknown aov"):
        runtime.imageinfo("Bogus")


def test_igcli_imageinfo_and_ppm(runtime, tmp_path):
    scene = tmp_path / "env.json"
    scene.write_text(json.dumps(env_only_scene()))
    ppm = tmp_path / "out.ppm"
    out = subprocess.run([os.path.join(PKG, "igcli"), str(scene), "--spp", "8", "--spi", "4", "--imageinfo", "8",
                          "--ppm", str(ppm), "--tonemap", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("imageinfo ")]
    assert len(lines) == 1, out.stdout
    cli = json.loads(lines[0][len("imageinfo "):])
    info = runtime.imageinfo(bins=8)
    for k in ("min", "max", "avg"):  # igcli prints %.9g, which names one float32
        assert np.float32(cli[k]) == np.float32(info[k]), (k, cli[k], info[k])
    assert cli["histogram_l"] == info["histogram_l"].tolist()
    data = ppm.read_bytes()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    img = runtime.tonemap(method=1)
    p = int(img[0, 0])
    assert data[len(head):len(head) + 3] == bytes([(p >> 16) & 255, (p >> 8) & 255, p & 255])
