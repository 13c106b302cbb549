"""Daylight scenes on the CPU: the loader (fishlens / orthogonal / depth-of-field
cameras, CIE skies, the sun from date and place), the shared camera and sky
arithmetic (host/camera_model.h, host/cie_sky.h, compiled here with g++ as
tests/native/daylight_check.cpp) against the float64 restatement of
tests/daylight_ref.py, and that restatement against the reference's converged
Radiance images (tests/golden/daylight/ref-sky-*-rad.exr)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import daylight_ref as R
import evalref
import ignis_amd
from exr_read import read_rgb
from ignis_amd import _native
from test_db_adapter import assert_desc_equal
from test_inmem import objects_of_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")
SKY_KIND = {"uniform": _native.SKY_UNIFORM, "cloudy": _native.SKY_CLOUDY, "clear": _native.SKY_CLEAR,
            "intermediate": _native.SKY_INTERMEDIATE}


_SCENES = []  # a desc lives as long as its scene


def desc_of(scene):
    """The desc of a scene given as a file name or as a dict."""
    sc = ignis_amd.Scene.from_file(scene) if isinstance(scene, str) else ignis_amd.Scene.from_string(scene)
    _SCENES.append(sc)
    return sc.desc


def scene_file(kind):
    return os.path.join(R.DAYLIGHT, f"sky-{kind}.json")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- loader --------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_fixture_scene_loads(kind):
    d = desc_of(scene_file(kind))
    assert (d.film_width, d.film_height) == (256, 256)
    cam = d.camera
    assert cam.type == _native.CAMERA_FISHLENS
    assert list(cam.eye) == [0, 0, 0] and list(cam.dir) == [0, 1, 0] and list(cam.up) == [0, 0, 1]
    assert cam.near_clip == np.float32(0.1) and cam.far_clip == 100
    assert d.num_lights == 1
    L = d.lights[0]
    assert L.type == _native.LIGHT_CIE and L.sky_kind == SKY_KIND[kind] and L.has_ground == 1
    assert list(L.sky_zenith) == [1, 1, 1] and list(L.sky_ground) == [1, 1, 1] and list(L.sky_scale) == [1, 1, 1]
    assert L.ground_brightness == np.float32(0.2)
    assert list(L.sky_transform) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    ref = R.fixture_sky(kind)
    if kind in ("clear", "intermediate"):
        # float32 rounding of a few dozen operations plus six-digit printing
        assert rel(L.sun_direction[:], ref.sun_dir) <= 1e-5
        assert rel(L.zenith_ratio, ref.zenith_ratio) <= 1e-5
        assert rel(L.sky_c2, ref.c2) <= 1e-5


def test_sun_position_known_answer():
    el, az = R.sun_ea(**R.FIXTURE_SUN)
    assert abs(math.degrees(el) - 20.82) <= 0.01 and abs(math.degrees(az) - 10.82) <= 0.01
    # and the loader's direction is that sun's
    L = desc_of(scene_file("clear")).lights[0]
    s = np.array(L.sun_direction[:], dtype=np.float64)
    assert abs(math.degrees(math.asin(s[1])) - 20.82) <= 0.01
    assert abs(math.degrees(math.atan2(s[0], -s[2])) - 10.82) <= 0.01


def test_sun_light_by_date_and_place():
    sun = dict(R.FIXTURE_SUN, type="sun", name="Sun", irradiance=[1, 1, 1])
    d = desc_of({"lights": [sun, dict(sun, type="directional", name="Dir")]})
    want = R.ea_direction(*R.sun_ea(**R.FIXTURE_SUN))
    for i in range(2):
        assert d.lights[i].type in (_native.LIGHT_SUN, _native.LIGHT_DIRECTIONAL)
        assert rel(d.lights[i].normal[:], want) <= 1e-5
    # the three ways to give a sun agree (getEA, LoaderUtils.cpp:140-151)
    el, az = R.sun_ea(**R.FIXTURE_SUN)
    by_ea = desc_of({"lights": [{"type": "sun", "name": "s", "elevation": el, "azimuth": az}]}).lights[0]
    by_dir = desc_of({"lights": [{"type": "sun", "name": "s", "direction": list(want)}]}).lights[0]
    assert rel(by_ea.normal[:], want) <= 1e-5 and rel(by_dir.normal[:], want) <= 1e-5


def test_sky_properties_and_type_names():
    for name, kind in [("cie_uniform", 0), ("cieuniform", 0), ("cie_cloudy", 1), ("ciecloudy", 1), ("cie_clear", 2),
                       ("cieclear", 2), ("cie_intermediate", 3), ("cieintermediate", 3)]:
        L = desc_of({"lights": [{"type": name, "name": "s", "elevation": 0.5}]}).lights[0]
        assert L.type == _native.LIGHT_CIE and L.sky_kind == kind
    sky = {"type": "cieclear", "name": "s", "zenith": [0.2, 0.4, 0.8], "ground": [0.3, 0.2, 0.1], "scale": [2, 3, 4],
           "ground_brightness": 0.4, "has_ground": False, "turbidity": 3.0, "elevation": 1.0, "azimuth": 2.0,
           "transform": {"rotate": [30, 0, 0]}}
    L = desc_of({"lights": [sky]}).lights[0]
    assert L.has_ground == 0 and L.ground_brightness == np.float32(0.4)
    np.testing.assert_array_equal(np.array(L.sky_zenith[:]), np.float32([0.2, 0.4, 0.8]))
    np.testing.assert_array_equal(np.array(L.sky_ground[:]), np.float32([0.3, 0.2, 0.1]))
    np.testing.assert_array_equal(np.array(L.sky_scale[:]), np.float32([2, 3, 4]))
    ref = R.Sky.for_sun("clear", 1.0, 2.0, turbidity=3.0)
    assert rel(L.zenith_ratio, ref.zenith_ratio) <= 1e-5 and rel(L.sky_c2, ref.c2) <= 1e-5
    # transform.linear().transpose().inverse() of a rotation is the rotation itself
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    np.testing.assert_allclose(np.array(L.sky_transform[:]).reshape(3, 3), [[1, 0, 0], [0, c, -s], [0, s, c]], atol=2e-6)
    # the elevation clamps to 87 degrees (CIELight.cpp:66-69)
    hi = desc_of({"lights": [dict(sky, elevation=math.radians(89.5))]}).lights[0]
    sun_y = math.sin(math.radians(89.5))
    zr, c2 = R.sunny_constants(True, math.radians(87), sun_y, 3.0)
    assert rel(hi.zenith_ratio, R.printed(zr)) <= 1e-5 and rel(hi.sky_c2, R.printed(c2)) <= 1e-5
    with pytest.raises(ignis_amd.IgxError, match="shading"):
        ignis_amd.Scene.from_string({"lights": [dict(sky, zenith="checkerboard(uv)")]})


def test_orthogonal_and_dof_cameras_carry_their_fields():
    t = {"lookat": {"origin": [1, 2, 3], "direction": [0, -1, 0], "up": [0, 0, 1]}}
    cam = desc_of({"camera": {"type": "orthogonal", "scale": 2.5, "aspect_ratio": 2, "near_clip": 0.5,
                                                  "far_clip": 50, "transform": t}}).camera
    assert cam.type == _native.CAMERA_ORTHOGONAL and cam.ortho_scale == 2.5 and cam.aspect == 2
    assert (cam.near_clip, cam.far_clip) == (0.5, 50)
    assert list(cam.eye) == [1, 2, 3] and list(cam.dir) == [0, -1, 0]
    assert (cam.aperture_radius, cam.focal_length) == (0, 0)
    # orientation from the transform only: identity without one (OrthogonalCamera.cpp:58-66)
    cam = desc_of({"camera": {"type": "orthogonal"},
                                       "shapes": [{"type": "cube", "name": "c"}], "bsdfs": [{"type": "diffuse", "name": "b"}],
                                       "entities": [{"name": "e", "shape": "c", "bsdf": "b"}]}).camera
    assert cam.ortho_scale == 1 and list(cam.eye) == [0, 0, 0] and list(cam.dir) == [0, 0, 1] and list(cam.up) == [0, 1, 0]
    cam = desc_of({"camera": {"type": "perspective", "fov": 40, "aperture_radius": 0.05,
                                                  "focal_length": 3, "transform": t}}).camera
    assert cam.type == _native.CAMERA_PERSPECTIVE and cam.ortho_scale == 0
    assert cam.aperture_radius == np.float32(0.05) and cam.focal_length == 3
    # no aperture: today's pinhole camera, all new fields zero
    cam = desc_of({"camera": {"type": "perspective", "fov": 40, "focal_length": 3, "transform": t}}).camera
    assert (cam.type, cam.ortho_scale, cam.aperture_radius, cam.focal_length) == (0, 0, 0, 0)
    assert desc_of({"camera": {"type": "fisheye"}}).camera.type == _native.CAMERA_FISHLENS
    with pytest.raises(ignis_amd.IgxError, match="unsupported camera type"):
        ignis_amd.Scene.from_string({"camera": {"type": "pinhole360"}})


@pytest.mark.parametrize("kind", ["clear", "cloudy"])
def test_in_memory_scene_equals_json(kind):
    a = ignis_amd.Scene.from_file(scene_file(kind))
    b = ignis_amd.Scene.from_objects(objects_of_file(scene_file(kind)))
    assert b.desc.camera.type == _native.CAMERA_FISHLENS and b.desc.lights[0].type == _native.LIGHT_CIE
    assert_desc_equal(a.desc, b.desc)  # every field of the ctypes mirror, the new ones included, bit for bit


def test_database_adapter_carries_camera_and_sky():
    """igcli / igtrace path: tables + shading view -> igx_scene_from_database."""
    from refdb import RefDatabase
    sc = ignis_amd.Scene.from_file(scene_file("clear"))
    ref = RefDatabase(sc)
    db, sv, keep = ref.views()
    back = ignis_amd.Scene.from_database(db, sv)
    assert back.desc.camera.type == _native.CAMERA_FISHLENS and back.desc.lights[0].type == _native.LIGHT_CIE
    assert_desc_equal(sc.desc, back.desc)


# ---- the shared arithmetic, compiled for the host -------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("daylight") / "daylight_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", HOST, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "daylight_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, mode, numbers, data, out_cols, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.asarray(data, dtype=np.float32).tofile(fin)
    out = subprocess.run([exe, mode] + ["%.9g" % float(np.float32(v)) for v in numbers] + [fin, fout], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return np.fromfile(fout, dtype=np.float32).reshape(-1, out_cols).astype(np.float64)


def pixel_grid(w, h):
    """nx, ny over the film: pixel corners and centres, so the centre (r = 0),
    the image circle's rim and the film's corners are all in it."""
    xs = np.unique(np.concatenate([np.linspace(-1, 1, 2 * w + 1), [0.0, 1e-9, -1e-9]]))
    ys = np.unique(np.concatenate([np.linspace(-1, 1, 2 * h + 1), [0.0, 1e-9, -1e-9]]))
    nx, ny = np.meshgrid(xs, ys)
    return nx.ravel().astype(np.float32), ny.ravel().astype(np.float32)


EYE, DIR, UP = [0.5, -1.0, 2.0], [0.48, -0.6, 0.64], [0.8, 0.0, -0.6]  # orthonormal: dir . up = 0


@pytest.mark.parametrize("model", ["perspective", "dof", "orthogonal", "fishlens"])
@pytest.mark.parametrize("size", [(64, 48), (48, 64), (37, 23)])
def test_camera_ray_against_float64(check_exe, tmp_path, model, size):
    w, h = size
    nx, ny = pixel_grid(w, h)
    rng = np.random.default_rng(7)
    u, v = rng.random(nx.size, dtype=np.float32), rng.random(nx.size, dtype=np.float32)
    u[:4], v[:4] = [0.5, 0.0, 1.0, 0.25], [0.5, 0.0, 1.0, 0.75]  # the disk's centre and corners of the square
    typ = {"perspective": 0, "dof": 0, "orthogonal": 1, "fishlens": 2}[model]
    fov, scale = math.radians(50), 1.75
    aperture, focal = (0.05, 3.0) if model == "dof" else (0.0, 0.0)
    f32 = lambda a: [float(np.float32(x)) for x in a]
    numbers = [typ, w, h] + EYE + DIR + UP + [fov, 1, -1, 0.1, 100, scale, aperture, focal]
    got = run_check(check_exe, "camera", numbers, np.stack([nx, ny, u, v], axis=1), 6, tmp_path)
    cam = R.Camera("orthogonal" if typ == 1 else "fishlens" if typ == 2 else "perspective", f32(EYE), f32(DIR), f32(UP), w, h,
                   fov=float(np.float32(fov)), vertical_fov=True, scale=float(np.float32(scale)),
                   aperture=float(np.float32(aperture)), focal=focal)
    org, d = cam.rays(nx, ny, u, v)
    # unit-vector components to 1e-6 (about 8 float ulps); origins are a few units from the world origin
    assert np.max(np.abs(got[:, 3:] - d)) <= 1e-6
    assert np.max(np.abs(got[:, :3] - org)) <= 1e-6 * 4
    assert np.max(np.abs(np.linalg.norm(got[:, 3:], axis=1) - 1)) <= 1e-6


@pytest.mark.parametrize("has_ground", [True, False])
@pytest.mark.parametrize("kind", R.KINDS)
def test_sky_function_against_float64(check_exe, tmp_path, kind, has_ground):
    rng = np.random.default_rng(11)
    d = rng.normal(size=(10000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:3] = [[0, 1, 0], [0, -1, 0], [1, 0, 0]]
    el, az = R.sun_ea(**R.FIXTURE_SUN)
    sky = R.Sky.for_sun(kind, el, az, has_ground=has_ground, zenith=[0.9, 1.0, 1.1], ground=[0.5, 0.4, 0.3], scale=[1.0, 0.9, 0.8],
                        ground_brightness=0.25)
    numbers = ([SKY_KIND[kind], int(has_ground)] + list(sky.zenith) + list(sky.ground) + list(sky.scale) + [sky.ground_brightness]
               + list(sky.sun_dir) + [sky.zenith_ratio, sky.c2] + [1, 0, 0, 0, 1, 0, 0, 0, 1])
    got = run_check(check_exe, "sky", numbers, d, 3, tmp_path)
    # the restatement sees the same float32 constants
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    sky.zenith, sky.ground, sky.scale, sky.sun_dir = f(sky.zenith), f(sky.ground), f(sky.scale), f(sky.sun_dir)
    sky.zenith_ratio, sky.c2 = float(np.float32(sky.zenith_ratio)), float(np.float32(sky.c2))
    want = sky.radiance(d.astype(np.float64))
    zen = sky.radiance(np.array([[0.0, 1.0, 0.0]]))[0]
    big = want > 1e-3 * zen[None, :]
    assert big.sum() > 10000
    assert np.max(np.abs(got[big] - want[big]) / want[big]) <= 1e-5
    if not has_ground:
        assert np.all(got[d[:, 1] < 0] == 0)


# ---- the restatement against Radiance --------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_matches_radiance(kind):
    ref = read_rgb(os.path.join(R.DAYLIGHT, f"ref-sky-{kind}-rad.exr")).astype(np.float32)
    assert ref.shape == (256, 256, 3)
    img = R.fishlens_sky_image(R.fixture_sky(kind), 256, 4).astype(np.float32)
    err, _ = evalref.error_image(img, ref)
    print(f"sky-{kind}: error_image {err:.3e}")
    assert err < 1e-3
