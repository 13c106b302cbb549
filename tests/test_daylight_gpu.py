"""Daylight scenes on the GPU: the four CIE sky fixture scenes against the
reference's converged Radiance images, the camera rays of the fishlens,
orthogonal and depth-of-field cameras against a float64 restatement
(Device.camera_rays: the rays the renderer traces), every schedule rendering
the same film, and a CIE sky lighting a diffuse plane against float64
quadrature of the sky function (tests/daylight_ref.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import daylight_ref as R
import evalref
import ignis_amd
from exr_read import read_rgb
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def params(w, h, spi=1, iteration=0, tile=None, seed=0):
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration, p.seed = w, h, spi, iteration, seed
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    return p


# ---- the sky scenes against Radiance ---------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_sky_scene_against_radiance(device, kind):
    """RunEvaluations' own condition at 64 spp (8 iterations of spi 8)."""
    sc = ignis_amd.Scene.from_file(os.path.join(R.DAYLIGHT, f"sky-{kind}.json"))
    device.upload(sc)
    device.clear()
    device.render_iterations(params(256, 256, spi=8), 8)
    film, it = device.framebuffer(256 * 256 * 3)
    assert it == 8 and np.isfinite(film).all()
    ref = read_rgb(os.path.join(R.DAYLIGHT, f"ref-sky-{kind}-rad.exr")).astype(np.float32)
    err, _ = evalref.error_image(film.reshape(256, 256, 3) / it, ref)
    print(f"sky-{kind}: error_image {err:.3e}")
    assert err < 1e-3


# ---- camera rays ---------------------------------------------------------------------
LOOK = {"lookat": {"origin": [0.5, -1.0, 2.0], "direction": [0.48, -0.6, 0.64], "up": [0.8, 0.0, -0.6]}}
CAMERAS = {
    "fishlens": {"type": "fishlens", "near_clip": 0.1, "far_clip": 100, "transform": LOOK},
    "orthogonal": {"type": "orthogonal", "scale": 1.75, "near_clip": 0.1, "far_clip": 100, "transform": LOOK},
    "dof": {"type": "perspective", "fov": 50, "aperture_radius": 0.05, "focal_length": 3, "near_clip": 0.1, "far_clip": 100,
            "transform": LOOK},
}
# The largest deviation of the device's rays (-fapprox-func: a / b as a * rcp(b),
# approximate sin / cos / sqrt) from the float64 restatement, measured on an
# MI355X over the nine cases below ("Daylight"): direction components
# and origins (world units, a few units from the origin).  The test allows 4x.
MEASURED_DIR, MEASURED_ORG = 6.7e-7, 6.5e-7


def jitter_and_lens(w, h, iteration, sample, frame, seed, draws):
    """The path's first `draws` random numbers per pixel, (draws, h, w) float32."""
    lib = O.lib()
    out = np.zeros((draws, h, w), np.float32)
    for y in range(h):
        for x in range(w):
            s = lib.oracle_random_seed(sample, iteration, frame, x, y, seed)
            c = C.c_uint32(1)
            for k in range(draws):
                out[k, y, x] = lib.oracle_next_f32(s, C.byref(c))
    return out


def reference_rays(cam_desc, w, h, rnd):
    """Float64 rays for the desc's camera and the device's jitter."""
    kind = {0: "perspective", 1: "orthogonal", 2: "fishlens"}[cam_desc.type]
    cam = R.Camera(kind, cam_desc.eye[:], cam_desc.dir[:], cam_desc.up[:], w, h, fov=cam_desc.fov,
                   vertical_fov=bool(cam_desc.vertical_fov), scale=cam_desc.ortho_scale, aperture=cam_desc.aperture_radius,
                   focal=cam_desc.focal_length)
    ys, xs = np.mgrid[0:h, 0:w]
    nx = 2 * (xs + rnd[0].astype(np.float64)) / w - 1
    ny = 1 - 2 * (ys + rnd[1].astype(np.float64)) / h
    lens = (rnd[2].ravel(), rnd[3].ravel()) if rnd.shape[0] > 2 else (None, None)
    org, d = cam.rays(nx, ny, *lens)
    return cam, org.reshape(h, w, 3), d.reshape(h, w, 3)


@pytest.mark.parametrize("model", list(CAMERAS))
@pytest.mark.parametrize("size", [(64, 48), (48, 64), (37, 23)])
def test_camera_rays_against_float64(device, model, size):
    w, h = size
    sc = ignis_amd.Scene.from_string({"camera": CAMERAS[model], "film": {"size": [w, h]},
                                      "lights": [{"type": "cieuniform", "name": "sky"}]})
    device.upload(sc)
    iteration, sample = 3, 5
    rays = device.camera_rays(iteration, sample)
    assert rays.shape == (h, w, 8)
    assert (rays[..., 6] == np.float32(0.1)).all() and (rays[..., 7] == 100).all()
    rnd = jitter_and_lens(w, h, iteration, sample, 0, 0, 4 if model == "dof" else 2)
    cam, org, d = reference_rays(sc.desc.camera, w, h, rnd)
    dev_d, dev_o = float(np.abs(rays[..., 3:6] - d).max()), float(np.abs(rays[..., 0:3] - org).max())
    print(f"{model} {w}x{h}: max deviation dir {dev_d:.3e} org {dev_o:.3e}")
    # the allowed deviation stays below 1/100 of a pixel's footprint: the angle
    # between neighbouring fishlens / perspective rays, the orthogonal pixel pitch
    if model == "orthogonal":
        foot = min(2 * cam.sx / w, 2 * cam.sy / h)
        assert 4 * MEASURED_ORG < foot / 100
    else:
        foot = (math.pi / 2) * min(2 * cam.xasp / w, 2 * cam.yasp / h) if model == "fishlens" else \
            min(2 * cam.sx / w, 2 * cam.sy / h) / (1 + cam.sx ** 2 + cam.sy ** 2)
        assert 4 * MEASURED_DIR < foot / 100
    assert dev_d <= 4 * MEASURED_DIR and dev_o <= 4 * MEASURED_ORG
    if model == "dof":
        # every ray passes through eye + dir0 * focal (dir0: the pinhole ray of the
        # same jitter) and starts on the aperture disk in the camera plane
        pin = R.Camera("perspective", cam.eye, cam.dir, cam.up, w, h, fov=sc.desc.camera.fov)
        ys, xs = np.mgrid[0:h, 0:w]
        _, d0 = pin.rays(2 * (xs + rnd[0].astype(np.float64)) / w - 1, 1 - 2 * (ys + rnd[1].astype(np.float64)) / h)
        focus = cam.eye[None] + d0 * cam.focal
        o, dd = rays[..., 0:3].reshape(-1, 3).astype(np.float64), rays[..., 3:6].reshape(-1, 3).astype(np.float64)
        t = np.einsum("ij,ij->i", focus - o, dd)
        miss = np.linalg.norm(o + t[:, None] * dd - focus, axis=1)
        print(f"dof: largest distance from the focus point {miss.max():.3e}")
        assert miss.max() <= 4 * (MEASURED_ORG + cam.focal * MEASURED_DIR * math.sqrt(3))
        off = o - cam.eye[None]
        assert np.abs(off @ cam.dir).max() <= 4 * MEASURED_ORG
        assert np.linalg.norm(off, axis=1).max() <= cam.aperture + 4 * MEASURED_ORG
        assert np.linalg.norm(off, axis=1).max() > 0.5 * cam.aperture


def test_zero_aperture_is_the_pinhole_camera(device):
    """A perspective camera with aperture 0 is the pinhole camera whatever the
    scene's shading variant: the same rays bit for bit and no lens draws; an
    aperture set through igx_set_camera moves the origins, and taking it away
    gives the pinhole rays back.  (That the basic variant's own camera code and
    camera_ray agree is test_gpu.py's test_shading_variant_invariance.)"""
    w, h = 37, 23
    cam = dict(CAMERAS["dof"], aperture_radius=0.0)
    sc = ignis_amd.Scene.from_string({"camera": cam, "film": {"size": [w, h]}})
    device.upload(sc)
    basic = device.camera_rays(2, 1)
    try:
        device.set_option("full_shading", 1)
        device.upload(sc)
        np.testing.assert_array_equal(device.camera_rays(2, 1), basic)
        rnd = jitter_and_lens(w, h, 2, 1, 0, 0, 2)
        _, org, d = reference_rays(sc.desc.camera, w, h, rnd)
        assert np.abs(basic[..., 3:6] - d).max() <= 4 * MEASURED_DIR and np.abs(basic[..., 0:3] - org).max() == 0
        lens = ignis_amd._native.Camera.from_buffer_copy(sc.desc.camera)
        lens.aperture_radius, lens.focal_length = 0.05, 3.0
        device.set_camera(lens)
        moved = device.camera_rays(2, 1)
        assert (moved[..., 0:3] != basic[..., 0:3]).any()
        lens.aperture_radius = 0.0
        device.set_camera(lens)
        np.testing.assert_array_equal(device.camera_rays(2, 1), basic)
    finally:
        device.set_option("full_shading", 0)
    # the basic variant refuses a camera it has not compiled
    device.upload(sc)
    lens.aperture_radius = 0.05
    with pytest.raises(ignis_amd.IgxError, match="full shading"):
        device.set_camera(lens)


# ---- the rays are the renderer's ---------------------------------------------------
def test_rays_trace_to_the_depth_aov(device):
    """Orthogonal camera over a tilted plane: trace_hits on the dumped rays of
    sample 0 gives the info-buffer pass's Depth (spi 1), and both the plane's
    analytic depth at the jittered pixel position."""
    w, h = 37, 23
    tilt = math.radians(25)
    scene = {"technique": {"type": "path", "max_depth": 2},
             "camera": {"type": "orthogonal", "scale": 0.8, "near_clip": 0.01, "far_clip": 100,
                        "transform": {"lookat": {"origin": [0, 0, -3], "direction": [0, 0, 1], "up": [0, 1, 0]}}},
             "film": {"size": [w, h]},
             "bsdfs": [{"type": "diffuse", "name": "m", "reflectance": [0.5, 0.5, 0.5]}],
             "shapes": [{"type": "rectangle", "name": "r", "width": 6, "height": 6, "flip_normals": True}],
             "entities": [{"name": "e", "shape": "r", "bsdf": "m", "transform": {"rotate": [25, 0, 0]}}],
             "lights": [{"type": "cieuniform", "name": "sky"}]}
    sc = ignis_amd.Scene.from_string(scene)
    device.upload(sc)
    try:
        device.set_option("denoise_aovs", 1)
        device.clear()
        device.render(params(w, h, spi=1))
        depth, it = device.framebuffer(w * h * 3, "Depth")
    finally:
        device.set_option("denoise_aovs", 0)
    assert it == 1
    depth = depth.reshape(h, w, 3)[..., 0].astype(np.float64)
    rays = device.camera_rays(0, 0)
    ep, tuv = device.trace_hits(rays.reshape(-1, 8))
    assert (ep[:, 0] == 0).all()
    t = tuv[:, 0].reshape(h, w).astype(np.float64)
    # the plane through the origin with normal (0, -sin, cos) (rotate x by 25 degrees): a
    # ray from (px, py, -3) along +z meets it at z = py * tan(tilt)
    rnd = jitter_and_lens(w, h, 0, 0, 0, 0, 2)
    ys, xs = np.mgrid[0:h, 0:w]
    ny = 1 - 2 * (ys + rnd[1].astype(np.float64)) / h
    py = (0.8 / (w / h)) * ny
    want = 3 + py * math.tan(tilt)
    assert np.abs(t - want).max() <= 1e-5 * want.max()
    assert np.abs(depth - want).max() <= 1e-5 * want.max()
    assert np.abs(depth - t).max() <= 1e-5 * want.max()


# ---- schedule invariance ---------------------------------------------------------------
DEFAULTS = {"extend_shapes": -1, "tail_threshold": -1, "fuse_generate": 1, "split": -1}


def daylight_room():
    return {"technique": {"type": "path", "max_depth": 8},
            "camera": {"type": "fishlens", "near_clip": 0.01, "far_clip": 100,
                       "transform": {"lookat": {"origin": [0, 1.5, 0], "direction": [0.3, -1, 0.2], "up": [0, 0, 1]}}},
            "film": {"size": [64, 64]},
            "bsdfs": [{"type": "diffuse", "name": "floor", "reflectance": [0.6, 0.5, 0.4]},
                      {"type": "dielectric", "name": "glass", "int_ior": 1.5}],
            "shapes": [{"type": "rectangle", "name": "floor", "width": 8, "height": 8},
                       {"type": "icosphere", "name": "ball", "radius": 0.5, "subdivisions": 2}],
            "entities": [{"name": "floor", "shape": "floor", "bsdf": "floor", "transform": {"rotate": [-90, 0, 0]}},
                         {"name": "ball", "shape": "ball", "bsdf": "glass", "transform": {"translate": [0.2, 0.5, 0.1]}}],
            "lights": [dict(R.FIXTURE_SUN, type="cieclear", name="sky")]}


def test_every_schedule_renders_the_same_film(device):
    """Reaches every gen_path call site (k_generate, bounce 0 of the generic and
    of the generate-shape k_extend, the tail kernel's input) and the tile path."""
    sc = ignis_amd.Scene.from_string(daylight_room())
    w = h = 64

    def film(opts, plist=None):
        device.upload(sc)
        for k, v in {**DEFAULTS, **opts}.items():
            device.set_option(k, v)
        device.clear()
        for p in plist or [params(w, h, spi=8)]:
            device.render_iterations(p, 2)
        return device.framebuffer(w * h * 3)[0].copy()

    try:
        base = film({})
        assert np.isfinite(base).all() and base.sum() > 0
        for opts in ({}, {"fuse_generate": 0}, {"extend_shapes": 0}, {"extend_shapes": 0, "fuse_generate": 0}, {"split": 1},
                     {"tail_threshold": 1 << 30}, {"tail_threshold": 0}):
            np.testing.assert_array_equal(film(opts), base, err_msg=str(opts))
        shards = [params(w, h, spi=8, tile=(8, off, 3)) for off in range(3)]
        np.testing.assert_array_equal(film({}, shards), base, err_msg="tile shards")
    finally:
        for k, v in DEFAULTS.items():
            device.set_option(k, v)


# ---- the sky as a light -----------------------------------------------------------------
def plane_under_sky(sky, nee):
    return {"technique": {"type": "path", "max_depth": 2, "nee": nee},
            "camera": {"type": "orthogonal", "scale": 0.5, "near_clip": 0.01, "far_clip": 100,
                       "transform": {"lookat": {"origin": [0, 2, 0], "direction": [0, -1, 0], "up": [0, 0, 1]}}},
            "film": {"size": [32, 32]},
            "bsdfs": [{"type": "diffuse", "name": "m", "reflectance": [0.5, 0.5, 0.5]}],
            "shapes": [{"type": "rectangle", "name": "r", "width": 2, "height": 2}],
            "entities": [{"name": "e", "shape": "r", "bsdf": "m", "transform": {"rotate": [-90, 0, 0]}}],
            "lights": [dict(sky, name="sky")]}


def quadrature(sky, both_sides, n=1024):
    """kd / pi * integral of L(d) |cos| over the upper hemisphere about +Y (or the
    whole sphere), kd = 0.5, midpoint rule in (cos theta, phi); per channel."""
    mu = (np.arange(n) + 0.5) / n
    phi = (np.arange(2 * n) + 0.5) * (math.pi / n)
    m, p = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - m * m)
    total = np.zeros(3)
    for sign in ((1, -1) if both_sides else (1,)):
        d = np.stack([s * np.cos(p), sign * m, s * np.sin(p)], axis=-1).reshape(-1, 3)
        total += (sky.world_radiance(d) * m.reshape(-1, 1)).sum(axis=0) * (1.0 / n) * (math.pi / n)
    return 0.5 / math.pi * total


ROT = {"rotate": [40, 0, 25]}
SKY_CASES = {
    # name: (light, reference sky, whether the sky reaches below the plane: NEE then lights the
    # two-sided Lambert plane from both sides -- a sky with a ground, or a tilted hemisphere)
    "cloudy-hemi": ({"type": "ciecloudy", "has_ground": False, "zenith": [1.0, 0.9, 0.8]},
                    lambda: R.Sky("cloudy", has_ground=False, zenith=[1.0, 0.9, 0.8]), False),
    "clear-ground": (dict(R.FIXTURE_SUN, type="cieclear", ground=[0.5, 0.6, 0.7]),
                     lambda: R.Sky.for_sun("clear", *R.sun_ea(**R.FIXTURE_SUN), ground=[0.5, 0.6, 0.7]), True),
    "clear-hemi-rotated": (dict(R.FIXTURE_SUN, type="cieclear", has_ground=False, transform=ROT),
                           lambda: R.Sky.for_sun("clear", *R.sun_ea(**R.FIXTURE_SUN), has_ground=False,
                                                 transform=rotation(ROT)), True),
    "intermediate-ground-rotated": (dict(R.FIXTURE_SUN, type="cieintermediate", transform=ROT),
                                    lambda: R.Sky.for_sun("intermediate", *R.sun_ea(**R.FIXTURE_SUN), transform=rotation(ROT)), True),
}


def rotation(t):
    """transform.linear().transpose().inverse() of a rotate op (Parser.cpp:177-181:
    Rx * Ry * Rz, degrees), at the shader's six printed digits."""
    ax, ay, az = (math.radians(v) for v in t["rotate"])
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    m = np.linalg.inv((rx @ ry @ rz).T)
    return np.vectorize(R.printed)(m)


@pytest.mark.parametrize("name", list(SKY_CASES))
def test_sky_lights_a_plane(device, name):
    light, make_sky, two_sided = SKY_CASES[name]
    sky = make_sky()
    means = {}
    for nee in (True, False):
        sc = ignis_amd.Scene.from_string(plane_under_sky(light, nee))
        device.upload(sc)
        device.clear()
        device.render_iterations(params(32, 32, spi=8), 8)
        film, it = device.framebuffer(32 * 32 * 3)
        assert it == 8 and np.isfinite(film).all()
        pix = film.reshape(-1, 3).astype(np.float64) / it
        # NEE also samples the sky below the two-sided Lambert plane; BSDF sampling alone does not
        want = quadrature(sky, two_sided and nee)
        mean, se = pix.mean(axis=0), pix.std(axis=0) / math.sqrt(pix.shape[0])
        print(f"{name} nee={nee}: mean {mean} expected {want} se {se}")
        assert (np.abs(mean - want) <= 5 * se + 1e-6).all(), (name, nee, mean, want, se)
        means[nee] = (mean, se)
    if not two_sided:  # both estimators integrate the same hemisphere
        (a, sa), (b, sb) = means[True], means[False]
        assert (np.abs(a - b) <= 5 * np.sqrt(sa * sa + sb * sb) + 1e-6).all()
