"""numpy restatements for the image texture tests (no GPU, no project code):
the packed-image byte mapping and row flip of the reference's Image.cpp, the
image texture arithmetic of texture/image.art and the environment map lookup of
light/env.art in float64."""
import ctypes as C
import math
import os

import numpy as np

TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textures")

NEAREST, BILINEAR, BICUBIC = range(3)
REPEAT, CLAMP, MIRROR = range(3)
FILTER_NAMES = {NEAREST: "nearest", BILINEAR: "bilinear", BICUBIC: "bicubic"}
WRAP_NAMES = {REPEAT: "repeat", CLAMP: "clamp", MIRROR: "mirror"}


def byte_color_to_linear(c):
    """floor(srgb_invgamma(c / 255) * 255) in float32 (Image.cpp:31-41)."""
    v = np.asarray(c, np.uint8).astype(np.float32) / np.float32(255)
    lo = v / np.float32(12.92)
    hi = np.power((v + np.float32(0.055)) / np.float32(1.055), np.float32(2.4), dtype=np.float32)
    lin = np.where(v <= np.float32(0.04045), lo, hi).astype(np.float32)
    return np.minimum(255, np.floor(lin * np.float32(255))).astype(np.uint8)


def packed_expected(decoded, linear):
    """What the reader stores for an 8-bit file whose decoded pixels (top row
    first, (h, w) or (h, w, c)) are `decoded`: rows flipped, colour bytes mapped
    unless `linear`, alpha as is; (h, w) for mono, (h, w, 4) otherwise."""
    a = np.asarray(decoded, np.uint8)[::-1]
    if a.ndim == 2:
        return a if linear else byte_color_to_linear(a)
    rgb = a[..., :3] if linear else byte_color_to_linear(a[..., :3])
    alpha = a[..., 3:4] if a.shape[2] == 4 else np.full(a.shape[:2] + (1,), 255, np.uint8)
    return np.concatenate([rgb, alpha], axis=2)


def desc_image(desc, i):
    """Image i of a scene desc as a numpy array: (h, w, 4) uint8, (h, w) uint8 or (h, w, 4) float32."""
    im = desc.images[i]
    w, h = im.width, im.height
    if im.format == 2:
        return np.ctypeslib.as_array(C.cast(im.pixels, C.POINTER(C.c_float)), (h, w, 4)).copy()
    n = w * h * (4 if im.format == 0 else 1)
    a = np.ctypeslib.as_array(C.cast(im.pixels, C.POINTER(C.c_uint8)), (n,)).copy()
    return a.reshape(h, w, 4) if im.format == 0 else a.reshape(h, w)


def texels_float64(img):
    """(h, w, 4) float64 texels of a desc image as the device unpacks them."""
    if img.dtype == np.uint8:
        f = img.astype(np.float64) / 255
        if f.ndim == 2:
            f = np.stack([f, f, f, np.ones_like(f)], axis=2)
        return f
    return img.astype(np.float64)


def border(wrap, x, w):
    x = np.asarray(x, np.int64)
    if wrap == CLAMP:
        return np.clip(x, 0, w - 1)
    if wrap == MIRROR:  # as written in texture/image.art:29-34: the even periods are the reversed ones
        t = np.where(x < 0, -1 - x, x)
        i = t // w
        k = t - i * w
        return np.where((i & 1) == 0, w - 1 - k, k)
    return np.mod(x, w)


def _w0(a): return (a * (a * (-a + 3) - 3) + 1) / 6
def _w1(a): return (a * a * (3 * a - 6) + 4) / 6
def _w2(a): return (a * (a * (-3 * a + 3) + 3) + 1) / 6
def _w3(a): return (a * a * a) / 6


def texel_point(tex, filt, u, v, dtype=np.float64):
    """map_uv_to_image_pixel(_nearest): integer texel and fraction, the
    coordinate arithmetic carried out in `dtype` (the header's is float32)."""
    h, w = tex.shape[:2]
    u, v = np.asarray(u, dtype), np.asarray(v, dtype)
    half = dtype(0.0 if filt == NEAREST else 0.5)
    fu, fv = u * dtype(w) - half, v * dtype(h) - half
    ix, iy = np.floor(fu), np.floor(fv)
    return ix.astype(np.float64), iy.astype(np.float64), (fu - ix).astype(np.float64), (fv - iy).astype(np.float64)


def texel_choice(tex, filt, wrap_u, wrap_v, u, v, dtype=np.float64):
    """The integer texel coordinates a lookup at the transformed (u, v) reads."""
    h, w = tex.shape[:2]
    ix, iy, fx, fy = texel_point(tex, filt, u, v, dtype)
    if filt != BICUBIC:
        return [border(wrap_u, ix, w), border(wrap_v, iy, h)]
    g0x, g1x, g0y, g1y = _w0(fx) + _w1(fx), _w2(fx) + _w3(fx), _w0(fy) + _w1(fy), _w2(fy) + _w3(fy)
    return [border(wrap_u, np.floor(ix + _w1(fx) / g0x - 1 + 0.5), w), border(wrap_u, np.floor(ix + _w3(fx) / g1x + 1 + 0.5), w),
            border(wrap_v, np.floor(iy + _w1(fy) / g0y - 1 + 0.5), h), border(wrap_v, np.floor(iy + _w3(fy) / g1y + 1 + 0.5), h)]


def transform_uv(m, u, v):
    m = np.asarray(m, np.float64)
    return m[0] * u + m[1] * v + m[2], m[3] * u + m[4] * v + m[5]


def sample(tex, filt, wrap_u, wrap_v, u, v, dtype=np.float64):
    """tex: (h, w, 4) float64; u, v: transformed coordinates; returns (..., 4)
    float64.  `dtype` is that of the coordinate arithmetic (texel_point); the
    weights and the blend are float64 either way."""
    h, w = tex.shape[:2]
    if filt == NEAREST:
        x, y = texel_choice(tex, filt, wrap_u, wrap_v, u, v, dtype)
        return tex[y, x]
    ix, iy, fx, fy = texel_point(tex, filt, u, v, dtype)
    fx, fy = fx[..., None], fy[..., None]
    if filt == BILINEAR:
        x0, y0 = border(wrap_u, ix, w), border(wrap_v, iy, h)
        x1, y1 = border(wrap_u, ix + 1, w), border(wrap_v, iy + 1, h)
        top = (1 - fx) * tex[y0, x0] + fx * tex[y0, x1]
        bot = (1 - fx) * tex[y1, x0] + fx * tex[y1, x1]
        return (1 - fy) * top + fy * bot
    x0, x1, y0, y1 = texel_choice(tex, filt, wrap_u, wrap_v, u, v, dtype)
    g0x, g1x, g0y, g1y = _w0(fx) + _w1(fx), _w2(fx) + _w3(fx), _w0(fy) + _w1(fy), _w2(fy) + _w3(fy)
    return (tex[y0, x0] * (g0x * g0y) + tex[y0, x1] * (g1x * g0y)) + (tex[y1, x0] * (g0x * g1y) + tex[y1, x1] * (g1x * g1y))


def choice_is_stable(tex, filt, wrap_u, wrap_v, u, v, eps=1e-5):
    """Whether the floor-chosen texels stay the same when (u, v) moves by +-eps
    (nearest and bicubic choose texels with floor; a bilinear lookup is continuous)."""
    if filt == BILINEAR:
        return np.ones(np.shape(u), bool)
    base = texel_choice(tex, filt, wrap_u, wrap_v, u, v)
    ok = np.ones(np.shape(u), bool)
    for du in (-eps, eps):
        for dv in (-eps, eps):
            other = texel_choice(tex, filt, wrap_u, wrap_v, u + du, v + dv)
            for a, b in zip(base, other):
                ok &= a == b
    return ok


LIGHT_ENVMAP = 10  # igx_light.type of an image environment map (include/igx_scene.h)


def env_uv(m, d):
    """map_env_uv(switch_env_up(m d)) in float64 (light/env.art:13-21)."""
    l = d @ np.asarray(m, np.float64).reshape(3, 3).T
    x, y, z = l[:, 0], l[:, 2], l[:, 1]
    theta = np.arccos(np.clip(z, -1, 1))
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, phi + 2 * math.pi, phi)
    t = phi / (2 * math.pi) + 0.25
    return t - np.floor(t), 1 - theta / math.pi


def env_radiance(desc, d, scale=None):
    """scale * tex(map_env_uv(...)) of the scene's environment map in float64, (n, 3);
    `scale` None is the light's own env_scale."""
    light = [desc.lights[i] for i in range(desc.num_lights) if desc.lights[i].type == LIGHT_ENVMAP][0]
    tx = desc.textures[light.env_texture]
    tex = texels_float64(desc_image(desc, tx.image))
    u, v = env_uv(light.sky_transform[:], d)
    tu, tv = transform_uv(tx.transform[:], u, v)
    scale = light.env_scale[:] if scale is None else scale
    return sample(tex, tx.filter, tx.wrap_u, tx.wrap_v, tu, tv)[..., :3] * np.asarray(scale, np.float64), (tex, tx, tu, tv)
