"""Image environment maps on the GPU: the map seen directly by camera rays
against the float64 restatement of map_env_uv and the texture filters
(tests/image_ref.py), and the map lighting a diffuse plane against float64
quadrature, sampled through its CDF, uniformly, and rotated."""
import math
import os

import numpy as np
import pytest

import daylight_ref as R
import ignis_amd
import image_ref as IR
from image_ref import env_radiance, env_uv
from ignis_amd import _native as N

pytestmark = pytest.mark.gpu

ROT = {"rotate": [40, 0, 25]}
SCALE = [2, 1, 0.5]
# The largest deviation of the film from scale * tex(map_env_uv(d)) in float64 at the
# device's own camera rays d, measured on an MI355X over the eight cases of
# test_map_seen_directly ("Image textures"): acos and atan2 are
# approximate under -fapprox-func, and a bilinear lookup turns a coordinate error
# into a colour error at 16 texels per unit.  The test allows 4x.
MEASURED = 1.4e-5


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def params(w, h, spi=1, iteration=0):
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration = w, h, spi, iteration
    return p


def rotation(t):
    """transform.linear().transpose().inverse() of a rotate op (Rx * Ry * Rz, degrees), at the six printed digits."""
    ax, ay, az = (math.radians(v) for v in t["rotate"])
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return np.vectorize(R.printed)(np.linalg.inv((rx @ ry @ rz).T))


@pytest.fixture(scope="module")
def distinct_map(tmp_path_factory):
    """16 x 8 float texels, all distinct, in [0, 1]."""
    rng = np.random.default_rng(41)
    path = tmp_path_factory.mktemp("env") / "distinct16x8.exr"
    ignis_amd.write_exr(path, rng.random((8, 16, 3), dtype=np.float32))
    return str(path)


CAMERAS = {"perspective": {"type": "perspective", "fov": 70, "near_clip": 0.1, "far_clip": 100,
                           "transform": {"lookat": {"origin": [0, 0, 0], "direction": [0.3, 0.5, -0.8], "up": [0, 1, 0]}}},
           "fishlens": {"type": "fishlens", "near_clip": 0.1, "far_clip": 100,
                        "transform": {"lookat": {"origin": [0, 0, 0], "direction": [0, 1, 0], "up": [0, 0, 1]}}}}


@pytest.mark.parametrize("rotated", [False, True], ids=["upright", "rotated"])
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_map_seen_directly(device, distinct_map, camera, filt, rotated):
    w, h = 64, 48
    light = {"type": "env", "name": "sky", "radiance": "map", "scale": SCALE}
    if rotated:
        light["transform"] = ROT
    sc = ignis_amd.Scene.from_string({"camera": CAMERAS[camera], "film": {"size": [w, h]},
                                      "textures": [{"type": "image", "name": "map", "filename": distinct_map, "filter_type": filt}],
                                      "lights": [light]})
    L = sc.desc.lights[0]
    assert L.type == N.LIGHT_ENVMAP and L.env_cdf == 1 and L.env_compensate == 1 and list(L.env_scale) == SCALE
    np.testing.assert_allclose(np.array(L.sky_transform[:]).reshape(3, 3), rotation(ROT) if rotated else np.eye(3), atol=1e-6)
    device.upload(sc)
    device.clear()
    device.render(params(w, h))
    film, it = device.framebuffer(w * h * 3)
    assert it == 1
    rays = device.camera_rays(0, 0).reshape(-1, 8)
    d = rays[:, 3:6].astype(np.float64)
    live = np.linalg.norm(d, axis=1) > 0.5  # the fishlens leaves the corners of the film without a ray
    want, (tex, tx, tu, tv) = env_radiance(sc.desc, d[live])
    stable = IR.choice_is_stable(tex, tx.filter, tx.wrap_u, tx.wrap_v, tu, tv, eps=1e-5)
    assert stable.mean() >= 0.98
    got = film.reshape(-1, 3).astype(np.float64)[live]
    dev = float(np.abs(got - want)[stable].max())
    print(f"{camera} {filt} rotated={rotated}: max deviation {dev:.3e}, {int((~stable).sum())} of {int(live.sum())} pixels left out")
    assert 4 * MEASURED < 1 / 510 and want.max() - want.min() > 0.5
    assert dev <= 4 * MEASURED
    if not live.all():
        assert (film.reshape(-1, 3)[~live] == 0).all()


# ---- the map as a light -------------------------------------------------------------------
@pytest.fixture(scope="module")
def patch_map(tmp_path_factory):
    """32 x 16: a smooth gradient plus a 2 x 2 patch 50 times brighter, above the horizon
    (the file's upper rows are the map's upper half)."""
    ys, xs = np.mgrid[0:16, 0:32]
    img = np.stack([0.2 + 0.3 * xs / 31, 0.3 + 0.2 * ys / 15, 0.25 + 0.1 * (xs + ys) / 46], axis=2).astype(np.float32)
    img[3:5, 20:22] *= 50
    path = tmp_path_factory.mktemp("env") / "patch32x16.exr"
    ignis_amd.write_exr(path, img)
    return str(path)


def plane_under_map(filename, nee, cdf, rotated):
    light = {"type": "env", "name": "sky", "radiance": "map", "scale": SCALE, "cdf": cdf}
    if rotated:
        light["transform"] = ROT
    return {"technique": {"type": "path", "max_depth": 2, "nee": nee},
            "camera": {"type": "orthogonal", "scale": 0.5, "near_clip": 0.01, "far_clip": 100,
                       "transform": {"lookat": {"origin": [0, 2, 0], "direction": [0, -1, 0], "up": [0, 0, 1]}}},
            "film": {"size": [32, 32]},
            "textures": [{"type": "image", "name": "map", "filename": filename, "filter_type": "bilinear"}],
            "bsdfs": [{"type": "diffuse", "name": "m", "reflectance": [0.5, 0.5, 0.5]}],
            "shapes": [{"type": "rectangle", "name": "r", "width": 2, "height": 2}],
            "entities": [{"name": "e", "shape": "r", "bsdf": "m", "transform": {"rotate": [-90, 0, 0]}}],
            "lights": [light]}


def nee_reach(desc):
    """Where the compensated CDF can sample at all, as a (512, 1024) mask over the baked map: MIS
    compensation (CDF.cpp:57-66) subtracts the map's mean from every pixel, so NEE never takes a
    direction darker than the mean -- those are left to BSDF sampling, which on the two-sided
    plane reaches the upper side only."""
    light = desc.lights[0]
    tx = desc.textures[light.env_texture]
    tex = IR.texels_float64(IR.desc_image(desc, tx.image))
    w, h = 1024, 512
    u, v = np.meshgrid(np.arange(w) / (w - 1), np.arange(h) / (h - 1))
    baked = IR.sample(tex, tx.filter, tx.wrap_u, tx.wrap_v, *IR.transform_uv(tx.transform[:], u, v))[..., :3]
    defect = np.maximum(baked, 0).mean(axis=(0, 1))
    return np.maximum(baked - defect, 0).sum(axis=2) > 0


def quadrature(desc, below, n=1024):
    """kd / pi * integral of L(d) |cos| over the upper hemisphere about +Y, plus the lower one
    (`below` "all"), or its part NEE can reach (`below` a nee_reach mask), or nothing (None);
    kd = 0.5, midpoint rule in (cos theta, phi); per channel."""
    mu = (np.arange(n) + 0.5) / n
    phi = (np.arange(2 * n) + 0.5) * (math.pi / n)
    m, p = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - m * m)
    total = np.zeros(3)
    for sign in ((1,) if below is None else (1, -1)):
        d = np.stack([s * np.cos(p), sign * m, s * np.sin(p)], axis=-1).reshape(-1, 3)
        rad = env_radiance(desc, d)[0]
        if sign < 0 and not isinstance(below, str):
            u, v = env_uv(desc.lights[0].sky_transform[:], d)
            hh, ww = below.shape
            rad = rad * below[np.minimum((v * hh).astype(int), hh - 1), np.minimum((u * ww).astype(int), ww - 1)][:, None]
        total += (rad * m.reshape(-1, 1)).sum(axis=0) * (1.0 / n) * (math.pi / n)
    return 0.5 / math.pi * total


@pytest.fixture(scope="module")
def expected(patch_map):
    """The quadrature of every case, computed once: (rotated, what NEE reaches below the plane)."""
    out = {}
    for rotated in (False, True):
        sc = ignis_amd.Scene.from_string(plane_under_map(patch_map, True, True, rotated))
        out[rotated, "none"] = quadrature(sc.desc, None)
        out[rotated, "cdf"] = quadrature(sc.desc, nee_reach(sc.desc))
        if not rotated:
            out[rotated, "uniform"] = quadrature(sc.desc, "all")
    return out


def test_map_lights_a_plane(device, patch_map, expected):
    se_nee = {}
    for case, cdf, rotated in (("cdf", True, False), ("uniform", False, False), ("cdf-rotated", True, True)):
        for nee in (True, False):
            sc = ignis_amd.Scene.from_string(plane_under_map(patch_map, nee, cdf, rotated))
            assert sc.desc.lights[0].env_cdf == int(cdf)
            device.upload(sc)
            device.clear()
            device.render_iterations(params(32, 32, spi=8), 8)
            film, it = device.framebuffer(32 * 32 * 3)
            assert it == 8 and np.isfinite(film).all()
            pix = film.reshape(-1, 3).astype(np.float64) / it
            # NEE also samples the map below the two-sided Lambert plane, where its density is not
            # zero; BSDF sampling alone does not
            want = expected[rotated, ("cdf" if cdf else "uniform") if nee else "none"]
            mean, se = pix.mean(axis=0), pix.std(axis=0) / math.sqrt(pix.shape[0])
            print(f"{case} nee={nee}: mean {mean} expected {want} se {se}")
            assert (np.abs(mean - want) <= 5 * se + 1e-6).all(), (case, nee, mean, want, se)
            if nee:
                se_nee[case] = se
    # the CDF finds the bright patch: less noise than uniform sampling of the sphere
    assert (se_nee["cdf"] < se_nee["uniform"]).all(), se_nee


# ---- a single bright texel over the Cornell box floor ------------------------------------
FLOOR_KD = [0.885809, 0.698859, 0.666422]


def bright_pixel_scene(nee, size=64):
    """The reference's evaluation scene env.json at 64 x 64: single_bright_pixel.png (nearest,
    scale 100) as the only light over cbox_floor.obj."""
    return {"technique": {"type": "path", "max_depth": 6, "nee": nee},
            "camera": {"type": "perspective", "transform": [1, 0, 0, 278, 0, 1, 0, 273, 0, 0, 1, -800, 0, 0, 0, 1],
                       "fov": 39.3077, "far_clip": 2800, "near_clip": 10},
            "film": {"size": [size, size]},
            "textures": [{"type": "image", "name": "env", "filter_type": "nearest",
                          "filename": os.path.join(IR.TEXTURES, "single_bright_pixel.png")}],
            "bsdfs": [{"name": "bsdf", "type": "diffuse", "reflectance": FLOOR_KD}],
            "shapes": [{"name": "shape", "type": "obj", "filename": os.path.join(IR.TEXTURES, "cbox_floor.obj")}],
            "entities": [{"name": "entity", "shape": "shape", "bsdf": "bsdf"}],
            "lights": [{"name": "env", "type": "env", "radiance": "env", "scale": 100}]}


def floor_radiance(desc, below):
    """kd / pi * integral of L cos over the hemisphere above the floor (normal +Y, the map's own
    up), exactly: with the nearest filter and the identity transforms, texel (i, j) covers
    u in [i / w, (i + 1) / w), theta = (1 - v) pi in [theta0, theta1], and
    integral cos sin dtheta dphi = (2 pi / w) (sin^2 theta1 - sin^2 theta0) / 2.  `below` adds the
    texels under the horizon that NEE can reach (brighter than the map's mean, nee_reach)."""
    light = desc.lights[0]
    tx = desc.textures[light.env_texture]
    assert tx.filter == N.FILTER_NEAREST and list(tx.transform) == [1, 0, 0, 0, 1, 0] and list(light.sky_transform) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    tex = IR.texels_float64(IR.desc_image(desc, tx.image))[..., :3] * np.asarray(light.env_scale[:], np.float64)
    h, w = tex.shape[:2]
    assert h % 2 == 0  # the horizon is a texel border
    v0, v1 = np.arange(h) / h, (np.arange(h) + 1) / h
    weight = np.abs(np.sin((1 - v0) * math.pi) ** 2 - np.sin((1 - v1) * math.pi) ** 2) / 2 * (2 * math.pi / w)
    upper = np.arange(h) >= h // 2  # v > 1 / 2 is above the horizon
    total = (tex[upper] * weight[upper, None, None]).sum(axis=(0, 1))
    if below:
        reach = tex.sum(axis=2) > tex.mean(axis=(0, 1)).sum()
        total = total + (tex * (reach & ~upper[:, None])[..., None] * weight[:, None, None]).sum(axis=(0, 1))
    return np.asarray(FLOOR_KD) / math.pi * total


def test_bright_pixel_over_the_floor(device):
    size = 64
    expected = None
    for nee in (True, False):
        sc = ignis_amd.Scene.from_string(bright_pixel_scene(nee, size))
        assert sc.desc.images[0].format == N.IMAGE_RGBA8 and (sc.desc.images[0].width, sc.desc.images[0].height) == (100, 50)
        if expected is None:
            expected = {True: floor_radiance(sc.desc, True), False: floor_radiance(sc.desc, False)}
            print("floor radiance by the rendering equation:", expected[False])
        device.upload(sc)
        # floor pixels: the camera ray and those of its eight neighbours meet the floor
        rays = device.camera_rays(0, 0).reshape(-1, 8)
        ep, _ = device.trace_hits(rays)
        hit = (ep[:, 0] == 0).reshape(size, size)
        inner = hit.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inner &= np.roll(np.roll(hit, dy, axis=0), dx, axis=1)
        inner[[0, -1], :] = False
        inner[:, [0, -1]] = False
        assert inner.sum() > 300  # the floor fills a trapezoid of the lower half of the film
        device.clear()
        device.render_iterations(params(size, size, spi=16), 16)
        film, it = device.framebuffer(size * size * 3)
        assert it == 16 and np.isfinite(film).all()
        pix = film.reshape(size, size, 3)[inner].astype(np.float64) / it
        mean, se = pix.mean(axis=0), pix.std(axis=0) / math.sqrt(pix.shape[0])
        print(f"bright pixel nee={nee}: floor mean {mean} expected {expected[nee]} se {se} over {int(inner.sum())} pixels")
        assert (np.abs(mean - expected[nee]) <= 5 * se + 1e-6).all(), (nee, mean, expected[nee], se)
