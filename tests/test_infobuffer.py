"""The denoiser's feature buffers on the device (runs on the MI355X box):
option "denoise_aovs" adds the info-buffer pass (technique/infobuffer.art,
InfoBufferTechnique.cpp) that fills the AOVs "Normals", "Albedo" and "Depth"
with one sample per pixel and leaves the film alone.  The oracle has no
info-buffer, so the checks are analytic or go against oracle.trace_hits.
"""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import ignis_amd
from oracle import oracle_py as O
from conftest import flat_scene
from exr_read import read_exr

pytestmark = pytest.mark.gpu
AOVS = ("Normals", "Albedo", "Depth")


@pytest.fixture()
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def params(w=0, h=0, spi=1, iteration=0, rays=None, tile=None):
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration = w, h, spi, iteration
    if rays is not None:
        p.num_rays = rays.shape[0]
        p.rays = rays.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    return p


def read_aovs(device, count):
    """{name: (data, iteration count)} of the three AOVs."""
    return {n: device.framebuffer(count, n) for n in AOVS}


def images(device, w, h):
    """The three AOVs over their own counts, (h, w, 3) each."""
    out = {}
    for n, (a, it) in read_aovs(device, w * h * 3).items():
        assert it >= 1, (n, it)
        out[n] = a.reshape(h, w, 3) / it
    return out


def test_off_by_default_then_on(device):
    sc = ignis_amd.Scene.from_string(flat_scene(size=16))
    device.upload(sc)
    device.render(params(16, 16))
    with pytest.raises(ignis_amd.IgxError):
        device.framebuffer(16 * 16 * 3, "Normals")
    device.set_option("denoise_aovs", 1)
    device.clear()
    device.render(params(16, 16))
    a, it = device.framebuffer(16 * 16 * 3, "Normals")
    assert it == 1 and device.aov_iteration_count("Normals") == 1
    assert np.abs(a).sum() > 0
    device.set_option("denoise_aovs", 0)
    with pytest.raises(ignis_amd.IgxError):
        device.framebuffer(16 * 16 * 3, "Normals")


W, H = 50, 37  # a partial wave at the end of the film


def footprint_depth_bounds(w, h):
    """Smallest and largest distance to the plane z = 0 from the eye (0, 0, -1)
    over each pixel's footprint: sqrt(1 + (sx nx)^2 + (sy ny)^2), fov 90."""
    sx = math.tan(math.radians(90) / 2)
    sy = sx / (w / h)
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    nx0, nx1 = 2 * xs / w - 1, 2 * (xs + 1) / w - 1
    ny0, ny1 = 1 - 2 * ys / h, 1 - 2 * (ys + 1) / h

    def absrange(a, b):
        lo = np.where((a <= 0) & (b >= 0) | (b <= 0) & (a >= 0), 0.0, np.minimum(np.abs(a), np.abs(b)))
        return lo, np.maximum(np.abs(a), np.abs(b))

    xlo, xhi = absrange(nx0, nx1)
    ylo, yhi = absrange(ny0, ny1)
    dmin = np.sqrt(1 + (sx * xlo[None, :]) ** 2 + (sy * ylo[:, None]) ** 2)
    dmax = np.sqrt(1 + (sx * xhi[None, :]) ** 2 + (sy * yhi[:, None]) ** 2)
    return dmin, dmax


def test_flat_plane_analytic(device):
    """Every camera ray hits the white Lambert plane z = 0 facing the eye:
    Normals (0, 0, -1), Albedo 1/pi (every Lambert sample contributes
    kd / (16 pi)), Depth inside the pixel footprint's range; the film is that
    of the same render without the pass."""
    sc = ignis_amd.Scene.from_string(flat_scene(size=50))
    device.upload(sc)
    device.render(params(W, H, spi=4))
    film_off, it_off = device.framebuffer(W * H * 3)
    device.set_option("denoise_aovs", 1)
    device.clear()
    device.render(params(W, H, spi=4))
    film_on, it_on = device.framebuffer(W * H * 3)
    assert it_off == 1 and it_on == 1
    np.testing.assert_array_equal(film_on, film_off)
    img = images(device, W, H)
    inner = (slice(1, H - 1), slice(1, W - 1))  # the jittered edge rays are tie cases
    nrm = img["Normals"][inner]
    print("normals max err", np.abs(nrm - np.array([0, 0, -1], np.float32)).max())
    np.testing.assert_allclose(nrm, np.broadcast_to(np.array([0, 0, -1], np.float32), nrm.shape), rtol=0, atol=1e-6)
    alb = img["Albedo"][inner]
    print("albedo max err", np.abs(alb - 1 / math.pi).max())
    np.testing.assert_allclose(alb, 1 / math.pi, rtol=0, atol=1e-5)
    dep = img["Depth"][inner]
    dmin, dmax = footprint_depth_bounds(W, H)
    assert (dep[..., 0] == dep[..., 1]).all() and (dep[..., 0] == dep[..., 2]).all()
    print("depth slack", (dep[..., 0] - dmin[inner]).min(), (dmax[inner] - dep[..., 0]).min())
    assert (dep[..., 0] >= dmin[inner] - 1e-5).all() and (dep[..., 0] <= dmax[inner] + 1e-5).all()


def test_checker_texture(device):
    """The albedo sees the texture the path tracer sees: pi * Albedo is one of
    the checker's two colours at every pixel, and both occur."""
    a, b = np.array([0.8, 0.2, 0.1], np.float32), np.array([0.1, 0.3, 0.9], np.float32)
    sd = flat_scene(size=50)
    sd["bsdfs"][0]["reflectance"] = "select(checkerboard(uvw * 4) == 1, color(0.8, 0.2, 0.1), color(0.1, 0.3, 0.9))"
    sc = ignis_amd.Scene.from_string(sd)
    device.upload(sc)
    device.set_option("denoise_aovs", 1)
    device.render(params(W, H, spi=4))
    alb = images(device, W, H)["Albedo"][1:H - 1, 1:W - 1].reshape(-1, 3) * math.pi
    da, db = np.abs(alb - a).max(axis=1), np.abs(alb - b).max(axis=1)
    print("checker max err", np.minimum(da, db).max(), "pixels of a / b", (da <= 1e-5).sum(), (db <= 1e-5).sum())
    assert (np.minimum(da, db) <= 1e-5).all()
    assert (da <= 1e-5).any() and (db <= 1e-5).any()


def grid_rays(eye, half, n, tmin=0.0, tmax=100.0):
    """n x n rays from `eye` through a grid on the plane z = eye.z + 1, |x|, |y| <= half."""
    t = (np.arange(n) + 0.5) / n * 2 * half - half
    xs, ys = np.meshgrid(t, t)
    d = np.stack([xs.ravel(), ys.ravel(), np.ones(n * n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n * n, 8), np.float32)
    rays[:, 0:3] = eye
    rays[:, 3:6] = d
    rays[:, 6], rays[:, 7] = tmin, tmax
    return rays


def camera_rays(scene, w, h):
    """Pixel-centre camera rays of the scene camera (camera/perspective.art:29-42)."""
    c = scene.desc.camera
    eye, dr, up = np.array(c.eye[:]), np.array(c.dir[:]), np.array(c.up[:])
    right = np.cross(dr, up)
    right /= np.linalg.norm(right)
    sx = math.tan(c.fov / 2)
    sy = sx / (w / h)
    ys, xs = np.mgrid[0:h, 0:w]
    v = sx * (2 * (xs + 0.5) / w - 1)[..., None] * right + sy * (1 - 2 * (ys + 0.5) / h)[..., None] * up + dr
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3] = eye
    rays[:, 3:6] = v.reshape(-1, 3)
    rays[:, 6], rays[:, 7] = c.near_clip, c.far_clip
    return rays


def assert_depth_matches_hits(depth, ep_o, tuv_o):
    """The project's hit contract (test_gpu.assert_hit_parity) for Depth against
    the oracle's t: >= 99.9 % of rays with the same hit / miss status, relative
    error <= 1e-5 at the 99.9th percentile and <= 1e-4 at worst."""
    hit_o = ep_o[:, 0] >= 0
    hit_g = depth > 0
    same = hit_o == hit_g
    print("hit status agreement", same.mean())
    assert same.mean() >= 0.999, same.mean()
    both = hit_o & hit_g
    assert both.sum() > 0
    rel = np.abs(depth[both] - tuv_o[both, 0]) / np.maximum(np.abs(tuv_o[both, 0]), 1e-6)
    print("depth rel err p99.9 / max", np.percentile(rel, 99.9), rel.max())
    assert np.percentile(rel, 99.9) <= 1e-5, np.percentile(rel, 99.9)
    assert rel.max() <= 1e-4, rel.max()
    return both


def test_sphere_ray_list(device):
    c, r = np.array([0.2, -0.1, 0.5]), 0.75
    sd = {
        "technique": {"type": "path", "max_depth": 2},
        "camera": {"type": "perspective", "fov": 60, "near_clip": 0.01, "far_clip": 100,
                   "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2]},
        "film": {"size": [64, 64]},
        "bsdfs": [{"type": "diffuse", "name": "d", "reflectance": [0.5, 0.6, 0.7]}],
        "shapes": [{"type": "sphere", "name": "S", "center": [float(v) for v in c], "radius": r}],
        "entities": [{"name": "S", "shape": "S", "bsdf": "d"}],
        "lights": [],
    }
    sc = ignis_amd.Scene.from_string(sd)
    rays = grid_rays(np.array([0, 0, -2.0]), 0.5, 64)
    device.upload(sc)
    device.set_option("denoise_aovs", 1)
    device.render(params(rays=rays))
    n = rays.shape[0]
    got = {k: (a.reshape(n, 3), it) for k, (a, it) in read_aovs(device, n * 3).items()}
    assert all(it == 1 for _, it in got.values())
    ep_o, tuv_o = O.OracleScene(sc).trace_hits(rays, 0)
    assert (ep_o[:, 0] >= 0).any() and (ep_o[:, 0] < 0).any()
    depth = got["Depth"][0]
    both = assert_depth_matches_hits(depth[:, 0], ep_o, tuv_o)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    nrm = (o + tuv_o[:, 0:1].astype(np.float64) * d - c) / r
    err = np.abs(got["Normals"][0][both] - nrm[both]).max()
    print("normal max abs err", err)
    assert err <= 1e-4
    np.testing.assert_allclose(got["Albedo"][0][both], np.broadcast_to(np.array([0.5, 0.6, 0.7]) / math.pi, (both.sum(), 3)),
                               rtol=0, atol=1e-5)
    # a missing ray writes nothing (the few silhouette rays the contract lets differ aside)
    miss = (ep_o[:, 0] < 0) & (depth[:, 0] == 0)
    assert miss.sum() >= 0.999 * (ep_o[:, 0] < 0).sum()
    for k in AOVS:
        assert (got[k][0][miss] == 0).all()


KD_BACK = [0.2, 0.5, 0.8]


def mirror_scene():
    """A delta conductor plane at z = 0 and a diffuse plane at z = -3, behind
    an eye at (0, 0, -1) that looks at the mirror."""
    return {
        "technique": {"type": "path", "max_depth": 4},
        "camera": {"type": "perspective", "fov": 60, "near_clip": 0.01, "far_clip": 100,
                   "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1]},
        "film": {"size": [32, 32]},
        "bsdfs": [{"type": "conductor", "name": "mirror", "specular_reflectance": [1, 1, 1]},
                  {"type": "diffuse", "name": "back", "reflectance": KD_BACK}],
        "shapes": [{"type": "rectangle", "name": "M", "width": 4, "height": 4, "flip_normals": True},
                   {"type": "rectangle", "name": "B", "width": 16, "height": 16}],
        "entities": [{"name": "M", "shape": "M", "bsdf": "mirror"},
                     {"name": "B", "shape": "B", "bsdf": "back", "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -3]}],
        "lights": [],
    }


def test_mirror_follow_specular(device):
    sc = ignis_amd.Scene.from_string(mirror_scene())
    rays = grid_rays(np.array([0, 0, -1.0]), 0.3, 32)
    n = rays.shape[0]
    dz = rays[:, 5].astype(np.float64)
    device.upload(sc)
    device.set_option("denoise_aovs", 2)

    def run():
        device.clear()
        device.render(params(rays=rays))
        return {k: a.reshape(n, 3) for k, (a, it) in read_aovs(device, n * 3).items()}

    got = run()  # stops at the mirror
    np.testing.assert_allclose(got["Normals"], np.broadcast_to(np.array([0, 0, -1.0]), (n, 3)), rtol=0, atol=1e-6)
    rel = np.abs(got["Depth"][:, 0] - 1 / dz) * dz
    print("mirror depth rel err", rel.max())
    assert rel.max() <= 1e-5
    assert np.isfinite(got["Albedo"]).all() and (got["Albedo"] >= 0).all() and (got["Albedo"] <= 1).all()

    device.set_option("denoise_follow_specular", 1)
    got = run()  # follows the reflection to the diffuse plane
    np.testing.assert_allclose(got["Normals"], np.broadcast_to(np.array([0, 0, 1.0]), (n, 3)), rtol=0, atol=1e-6)
    rel = np.abs(got["Depth"][:, 0] - 4 / dz) * dz / 4
    print("followed depth rel err", rel.max())
    assert rel.max() <= 1e-5
    print("followed albedo err", np.abs(got["Albedo"] - np.array(KD_BACK) / math.pi).max())
    np.testing.assert_allclose(got["Albedo"], np.broadcast_to(np.array(KD_BACK) / math.pi, (n, 3)), rtol=0, atol=1e-5)

    device.set_option("denoise_max_depth", 0)
    got = run()  # the specular hit is neither recorded nor followed
    for k in AOVS:
        assert (got[k] == 0).all()


def test_counts_and_modes(device, primitives_path):
    sc = ignis_amd.Scene.from_file(primitives_path)
    w = h = 48
    n = w * h * 3
    device.upload(sc)
    device.set_option("denoise_aovs", 1)
    device.render_iterations(params(w, h, spi=2), 3)
    first = read_aovs(device, n)
    assert all(it == 1 for _, it in first.values())
    assert device.framebuffer(n)[1] == 3
    device.render_iterations(params(w, h, spi=2, iteration=3), 3)
    again = read_aovs(device, n)
    assert device.framebuffer(n)[1] == 6
    for k in AOVS:
        assert again[k][1] == 1
        np.testing.assert_array_equal(again[k][0], first[k][0])

    device.set_option("denoise_aovs", 2)
    device.clear()
    device.render_iterations(params(w, h, spi=2), 3)
    batch = read_aovs(device, n)
    assert all(it == 3 for _, it in batch.values())
    device.clear()
    for i in range(3):
        device.render(params(w, h, spi=2, iteration=i))
    single = read_aovs(device, n)
    for k in AOVS:
        assert single[k][1] == 3
        assert np.abs(batch[k][0]).sum() > 0
        np.testing.assert_array_equal(batch[k][0], single[k][0])


@pytest.mark.parametrize("name", ["primitives.json", "diamond_scene.json"])
def test_schedule_invariance(device, root, name):
    """The AOVs do not depend on how the film's work is scheduled, nor on the
    BVH's width (closest hits are independent of the tree), nor on the run."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    w = h = 64
    n = w * h * 3
    device.set_option("denoise_aovs", 2)
    device.set_option("denoise_follow_specular", 1)

    def run(**opts):
        for k, v in opts.items():
            device.set_option(k, v)
        device.upload(sc)
        device.clear()
        device.render_iterations(params(w, h, spi=2), 2)
        out = read_aovs(device, n)
        assert all(it == 2 for _, it in out.values())
        return out

    base = run()
    assert all(np.abs(base[k][0]).sum() > 0 for k in AOVS)
    for opts in ({}, {"async_render": 0}, {"async_render": 1, "capacity": 4096}, {"capacity": 0, "bvh_width": 2}, {"bvh_width": 4}):
        other = run(**opts)
        for k in AOVS:
            np.testing.assert_array_equal(other[k][0], base[k][0], err_msg=f"{k} {opts}")
    # ray-list mode: Depth against the oracle's hits (camera rays through the pixel centres)
    device.set_option("bvh_width", 0)
    device.set_option("denoise_follow_specular", 0)
    device.upload(sc)
    rays = camera_rays(sc, w, h)
    device.render(params(rays=rays))
    depth, it = device.framebuffer(rays.shape[0] * 3, "Depth")
    assert it == 1
    ep_o, tuv_o = O.OracleScene(sc).trace_hits(rays, 0)
    assert_depth_matches_hits(depth.reshape(-1, 3)[:, 0], ep_o, tuv_o)


def test_tiles(device, primitives_path):
    """Two ranks' tile shards (tile 16, stride 2) add up to the whole AOVs bit
    for bit, and a rank leaves the other's tiles alone."""
    sc = ignis_amd.Scene.from_file(primitives_path)
    w = h = 64
    n = w * h * 3
    device.upload(sc)
    device.set_option("denoise_aovs", 1)
    device.render(params(w, h, spi=2))
    whole = {k: a.reshape(h, w, 3) for k, (a, it) in read_aovs(device, n).items()}
    ty, tx = np.mgrid[0:h, 0:w] // 16
    tile_id = ty * (w // 16) + tx
    parts = []
    for off in (0, 1):
        device.clear()
        device.render(params(w, h, spi=2, tile=(16, off, 2)))
        part = {k: a.reshape(h, w, 3) for k, (a, it) in read_aovs(device, n).items()}
        for k in AOVS:
            assert (part[k][tile_id % 2 != off] == 0).all()
        parts.append(part)
    for k in AOVS:
        assert np.abs(whole[k]).sum() > 0
        np.testing.assert_array_equal(parts[0][k] + parts[1][k], whole[k])


def test_clear_by_name(device, root):
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "primitives_aov.json"))
    assert sc.desc.technique.aov_mis == 1
    w = h = 32
    n = w * h * 3
    device.upload(sc)
    device.set_option("denoise_aovs", 2)

    def state():
        names = (None, "Direct Weights", "NEE Weights") + AOVS
        return {k: device.framebuffer(n, k) for k in names}

    device.render(params(w, h, spi=2))
    s0 = state()
    assert all(np.abs(a).sum() > 0 and it == 1 for a, it in s0.values())

    device.clear("Color")
    s1 = state()
    assert (s1[None][0] == 0).all() and s1[None][1] == 0
    for k in ("Direct Weights", "NEE Weights") + AOVS:
        np.testing.assert_array_equal(s1[k][0], s0[k][0])
    for k in AOVS:
        assert s1[k][1] == 1

    device.clear("Depth")
    s2 = state()
    assert (s2["Depth"][0] == 0).all() and s2["Depth"][1] == 0
    for k in ("Direct Weights", "NEE Weights", "Normals", "Albedo"):
        np.testing.assert_array_equal(s2[k][0], s0[k][0])
    assert s2["Normals"][1] == 1 and s2["Albedo"][1] == 1

    device.clear("NEE Weights")
    s3 = state()
    assert (s3["NEE Weights"][0] == 0).all()
    np.testing.assert_array_equal(s3["Direct Weights"][0], s0["Direct Weights"][0])

    device.render(params(w, h, spi=2, iteration=1))
    device.clear()
    s4 = state()
    assert all((a == 0).all() and it == 0 for a, it in s4.values())

    with pytest.raises(ignis_amd.IgxError):
        device.clear("Position")


def test_igcli_layers(root, tmp_path):
    scene = tmp_path / "flat.json"
    scene.write_text(json.dumps(flat_scene(size=50)))
    out = tmp_path / "out.exr"
    exe = os.path.join(root, "ignis-masterthesis_amd", "igcli")
    res = subprocess.run([exe, str(scene), "--spp", "8", "--spi", "4", "--width", str(W), "--height", str(H), "--denoise-aovs",
                          "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    chans, _ = read_exr(str(out))
    assert set(chans) == {f"{layer}.{c}" for layer in ("Default",) + AOVS for c in "RGB"}
    np.testing.assert_allclose(chans["Albedo.R"][1:H - 1, 1:W - 1], 1 / math.pi, rtol=0, atol=1e-5)
    np.testing.assert_allclose(chans["Normals.B"][1:H - 1, 1:W - 1], -1.0, rtol=0, atol=1e-6)
