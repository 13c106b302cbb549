"""Image textures on the GPU: the texel fetch through the renderer against the
float64 restatement of texture/image.art (tests/image_ref.py), a constant image
against the constant colour, every schedule rendering the same film, and the
refusal of a textured analytic sphere."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import daylight_ref as R
import ignis_amd
import image_ref as IR
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

W, H = 37, 23
# A transform that takes the rectangle's [0, 1]^2 out of [0, 1] on every side
# (so every wrap rule is used): u' in [-0.27, 1.83], v' in [-0.71, 1.79]
TRANSFORM = [1.7, -0.4, 0, 0.13, 0.3, 2.2, 0, -0.71, 0, 0, 1, 0, 0, 0, 0, 1]
# The largest deviation of pi * Albedo from the float64 restatement, measured on
# an MI355X over the 18 cases below ("Image textures"): the device
# interpolates uv, transforms it and filters in float32 with -fapprox-func
# (a / b as a * rcp(b)), and the albedo is a float32 sum of 16 BSDF samples.
# The test allows 4x, which must stay below half an 8-bit step (1 / 510).
MEASURED = 1.4e-6


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def params(w, h, spi=1, iteration=0, tile=None):
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration = w, h, spi, iteration
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    return p


@pytest.fixture(scope="module")
def jitter():
    """The first two random numbers of every pixel's path (iteration 0, sample 0), (2, H, W)."""
    lib = O.lib()
    out = np.zeros((2, H, W), np.float32)
    for y in range(H):
        for x in range(W):
            s = lib.oracle_random_seed(0, 0, 0, x, y, 0)
            c = C.c_uint32(1)
            for k in range(2):
                out[k, y, x] = lib.oracle_next_f32(s, C.byref(c))
    return out


@pytest.fixture(scope="module")
def float_texture(tmp_path_factory):
    """An 8 x 8 float EXR with distinct texels in [0, 1], written with the project's writer."""
    rng = np.random.default_rng(23)
    img = rng.random((8, 8, 3), dtype=np.float32)
    path = tmp_path_factory.mktemp("tex") / "float8x8.exr"
    ignis_amd.write_exr(path, img)
    return str(path)


def rectangle_scene(filename, filt, wrap):
    return {"technique": {"type": "path", "max_depth": 2},
            "camera": {"type": "orthogonal", "scale": 0.5, "near_clip": 0.01, "far_clip": 100,
                       "transform": {"lookat": {"origin": [0, 0, -1], "direction": [0, 0, 1], "up": [0, 1, 0]}}},
            "film": {"size": [W, H]},
            "textures": [{"type": "image", "name": "tex", "filename": filename, "filter_type": IR.FILTER_NAMES[filt],
                          "wrap_mode": IR.WRAP_NAMES[wrap], "transform": TRANSFORM}],
            "bsdfs": [{"type": "diffuse", "name": "m", "reflectance": "tex"}],
            "shapes": [{"type": "rectangle", "name": "r", "width": 1, "height": 1, "flip_normals": True}],
            "entities": [{"name": "e", "shape": "r", "bsdf": "m"}],
            "lights": [{"type": "env", "name": "sky", "radiance": [1, 1, 1]}]}


def pixel_uv(desc, rnd):
    """Float64 texture coordinates of every pixel's hit: the orthogonal camera's
    ray for the pixel's jitter meets the rectangle z = 0 at its own (x, y); the
    rectangle's texture coordinates are affine in the position."""
    cam = desc.camera
    model = R.Camera("orthogonal", cam.eye[:], cam.dir[:], cam.up[:], W, H, scale=cam.ortho_scale)
    ys, xs = np.mgrid[0:H, 0:W]
    nx = 2 * (xs + rnd[0].astype(np.float64)) / W - 1
    ny = 1 - 2 * (ys + rnd[1].astype(np.float64)) / H
    org, d = model.rays(nx, ny)
    assert np.allclose(d, [0, 0, 1])
    m = desc.meshes[0]
    v = np.ctypeslib.as_array(m.vertices, (m.num_vertices, 3)).astype(np.float64)
    t = np.ctypeslib.as_array(m.texcoords, (m.num_vertices, 2)).astype(np.float64)
    assert np.abs(v[:, 2]).max() == 0 and np.abs(v[:, :2]).max() == 0.5
    A, res, *_ = np.linalg.lstsq(np.c_[v[:, :2], np.ones(len(v))], t, rcond=None)
    assert np.allclose(np.c_[v[:, :2], np.ones(len(v))] @ A, t, atol=1e-12)  # affine indeed
    uv = np.c_[org[:, :2], np.ones(len(org))] @ A
    assert uv.min() > 0 and uv.max() < 1  # every ray meets the rectangle
    return uv[:, 0].reshape(H, W), uv[:, 1].reshape(H, W)


@pytest.mark.parametrize("wrap", [IR.REPEAT, IR.CLAMP, IR.MIRROR], ids=["repeat", "clamp", "mirror"])
@pytest.mark.parametrize("filt", [IR.NEAREST, IR.BILINEAR, IR.BICUBIC], ids=["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("image", ["bitmap.png", "float.exr"])
def test_texel_fetch_through_the_renderer(device, jitter, float_texture, image, filt, wrap):
    filename = os.path.join(IR.TEXTURES, "bitmap.png") if image == "bitmap.png" else float_texture
    sc = ignis_amd.Scene.from_string(rectangle_scene(filename, filt, wrap))
    device.upload(sc)
    device.set_option("denoise_aovs", 1)
    try:
        device.clear()
        device.render(params(W, H))
        albedo, it = device.framebuffer(W * H * 3, "Albedo")
    finally:
        device.set_option("denoise_aovs", 0)
    assert it == 1
    got = albedo.reshape(H, W, 3).astype(np.float64) * math.pi
    tex = IR.texels_float64(IR.desc_image(sc.desc, 0))
    u, v = pixel_uv(sc.desc, jitter)
    tu, tv = IR.transform_uv(sc.desc.textures[0].transform[:], u, v)
    assert tu.min() < 0 and tu.max() > 1 and tv.min() < 0 and tv.max() > 1
    want = IR.sample(tex, filt, wrap, wrap, tu, tv)[..., :3]
    # nearest and bicubic choose texels with floor: pixels whose choice changes within 1e-5 of uv are left out
    stable = IR.choice_is_stable(tex, filt, wrap, wrap, tu, tv, eps=1e-5)
    assert stable.mean() >= 0.98, stable.mean()
    dev = float(np.abs(got - want)[stable].max())
    print(f"{image} {IR.FILTER_NAMES[filt]} {IR.WRAP_NAMES[wrap]}: max deviation {dev:.3e}, {int((~stable).sum())} pixels left out")
    assert 4 * MEASURED < 1 / 510  # a wrong texel cannot pass
    assert want[stable].max() - want[stable].min() > 0.3  # the film sees many texels
    assert dev <= 4 * MEASURED


@pytest.mark.parametrize("bsdf", ["diffuse", "principled"])
def test_constant_image_equals_constant_colour(device, tmp_path, bsdf):
    """An image of one colour: with the nearest filter the textured
    material is that colour exactly, so the film of the path tracer (k_extend's
    shade_step, three bounces under a constant sky) equals the film of the same
    scene with the colour written out, bit for bit."""
    path = str(tmp_path / "one_colour.exr")
    ignis_amd.write_exr(path, np.broadcast_to(np.array([0.7, 0.4, 0.2], np.float32), (3, 5, 3)).copy())
    key = "reflectance" if bsdf == "diffuse" else "base_color"

    def scene(colour):
        sd = rectangle_scene(path, IR.NEAREST, IR.REPEAT)
        sd["technique"]["max_depth"] = 4
        sd["bsdfs"] = [{"type": bsdf, "name": "m", key: colour}]
        sd["shapes"].append({"type": "rectangle", "name": "wall", "width": 1, "height": 1})
        sd["entities"].append({"name": "w", "shape": "wall", "bsdf": "m",
                               "transform": [{"translate": [0.3, 0, -0.4]}, {"rotate": [0, 70, 0]}]})
        return ignis_amd.Scene.from_string(sd)

    textured = scene("tex")
    texels = IR.desc_image(textured.desc, 0)
    colour = texels[0, 0, :3]
    assert (texels[..., :3] == colour).all() and 0 < colour.min() and len(set(colour)) > 1
    plain = scene([float(c) for c in colour])
    films = []
    for sc in (textured, plain):
        device.upload(sc)
        device.clear()
        device.render_iterations(params(W, H, spi=4), 2)
        films.append(device.framebuffer(W * H * 3)[0].copy())
    assert np.isfinite(films[0]).all() and films[0].sum() > 0
    np.testing.assert_array_equal(films[0], films[1])


DEFAULTS = {"extend_shapes": -1, "tail_threshold": -1, "fuse_generate": 1, "split": -1, "async_render": 1}


def textured_room(float_texture):
    """The daylight room of tests/test_daylight_gpu.py with image-textured surfaces -- a bicubic
    PNG on the floor, a bilinear mirrored float image on a principled wall, a glass ball -- under
    an image environment map sampled through its CDF."""
    return {"technique": {"type": "path", "max_depth": 8},
            "camera": {"type": "fishlens", "near_clip": 0.01, "far_clip": 100,
                       "transform": {"lookat": {"origin": [0, 1.5, 0], "direction": [0.3, -1, 0.2], "up": [0, 0, 1]}}},
            "film": {"size": [64, 64]},
            "textures": [{"type": "image", "name": "tiles", "filename": os.path.join(IR.TEXTURES, "bitmap.png"),
                          "transform": [{"scale": [4, 4, 1]}]},
                         {"type": "image", "name": "paint", "filename": float_texture, "filter_type": "bilinear",
                          "wrap_mode": "mirror", "transform": [{"translate": [0.3, 0.1, 0]}, {"scale": [2.5, 1.5, 1]}]}],
            "bsdfs": [{"type": "diffuse", "name": "floor", "reflectance": "tiles"},
                      {"type": "principled", "name": "wall", "base_color": "paint", "roughness": 0.4},
                      {"type": "dielectric", "name": "glass", "int_ior": 1.5}],
            "shapes": [{"type": "rectangle", "name": "floor", "width": 8, "height": 8},
                       {"type": "rectangle", "name": "wall", "width": 4, "height": 2},
                       {"type": "icosphere", "name": "ball", "radius": 0.5, "subdivisions": 2}],
            "entities": [{"name": "floor", "shape": "floor", "bsdf": "floor", "transform": {"rotate": [-90, 0, 0]}},
                         {"name": "wall", "shape": "wall", "bsdf": "wall", "transform": {"translate": [0.5, 1, 1.5]}},
                         {"name": "ball", "shape": "ball", "bsdf": "glass", "transform": {"translate": [0.2, 0.5, 0.1]}}],
            "lights": [{"type": "env", "name": "sky", "radiance": "paint", "scale": [3, 3, 4], "transform": {"rotate": [10, 20, 0]}}]}


def test_every_schedule_renders_the_same_film(device, float_texture):
    sc = ignis_amd.Scene.from_string(textured_room(float_texture))
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
        # the textures are seen: the floor's film is not that of a constant floor
        assert len(np.unique(np.round(base.reshape(-1, 3), 3), axis=0)) > 500
        for opts in ({}, {"fuse_generate": 0}, {"extend_shapes": 0}, {"extend_shapes": 0, "fuse_generate": 0}, {"split": 1},
                     {"tail_threshold": 1 << 30}, {"tail_threshold": 0}, {"async_render": 0}):
            np.testing.assert_array_equal(film(opts), base, err_msg=str(opts))
        shards = [params(w, h, spi=8, tile=(8, off, 3)) for off in range(3)]
        np.testing.assert_array_equal(film({}, shards), base, err_msg="tile shards")
    finally:
        for k, v in DEFAULTS.items():
            device.set_option(k, v)


def test_textured_analytic_sphere_is_refused(device):
    sd = rectangle_scene(os.path.join(IR.TEXTURES, "bitmap.png"), IR.NEAREST, IR.REPEAT)
    sd["shapes"].append({"type": "sphere", "name": "s", "radius": 0.2})
    sd["entities"].append({"name": "ball", "shape": "s", "bsdf": "m"})
    with pytest.raises(ignis_amd.IgxError, match="textured material on an analytic sphere"):
        device.upload(ignis_amd.Scene.from_string(sd))
