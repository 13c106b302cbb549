"""ignis_amd — Python face of the MI355X wavefront path-tracing device.

Mirrors the reference's Python module surface used by its integration tests
(src/frontend/python/runtime.cpp:178-260; src/tests/integrator/common/__init__.py:68-90):

    opts = ignis_amd.RuntimeOptions.makeDefault()
    with ignis_amd.loadFromString(json_text, opts) as runtime:
        runtime.step()
        img = runtime.getFramebufferForHost() / runtime.IterationCount

Semantics follow IG::Runtime (src/runtime/Runtime.cpp): SPI defaults to the
reference's GPU recommendation (8 for a 1000^2 film, Runtime.cpp:61-69), each
step() renders one iteration (Runtime::step, Runtime.cpp:292-319) and the
framebuffer holds sum(colour)/spi per pixel until cleared.
"""
import ctypes as C
import json
import math
import os

import numpy as np

from . import _native
from ._native import (EXPORTED_SYMBOLS, LIB_PATH, GlareOutput, GlareSettings, ImageInfoOutput, ImageInfoSettings,
                      RenderParams, Stats, TonemapSettings, lib)

__all__ = ["RuntimeOptions", "DenoiserSettings", "Scene", "Runtime", "loadFromFile", "loadFromString", "version",
           "EXPORTED_SYMBOLS", "LIB_PATH", "IgxError"]


class IgxError(RuntimeError):
    pass


def version():
    return lib().igx_version().decode()


def write_exr(path, rgb, scale=1.0, alpha=False):
    """Write a (H, W, 3) float image as an uncompressed float OpenEXR file
    (Image::save, src/runtime/Image.h:92-101)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[0], rgb.shape[1]
    rc = _native.lib().igx_write_exr(os.fsencode(path), rgb.ctypes.data_as(C.POINTER(C.c_float)), w, h, 4 if alpha else 3,
                                      float(scale))
    if rc != 0:
        raise IgxError(f"cannot write EXR {path} (code {rc})")


def write_exr_layers(path, layers, scales=None):
    """One EXR with the channels <name>.R / .G / .B of every layer, the
    reference's layout of a render with AOVs (frontend/common/IO.cpp:105-129;
    the film is the layer "Default").  `layers`: {name: (H, W, 3) image},
    `scales`: {name: factor} (e.g. 1 / the layer's own iteration count)."""
    names = list(layers)
    imgs = [np.ascontiguousarray(layers[n], dtype=np.float32) for n in names]
    h, w = imgs[0].shape[0], imgs[0].shape[1]
    if any(i.shape != (h, w, 3) for i in imgs):
        raise IgxError("write_exr_layers: every layer must be (H, W, 3) of one size")
    n = len(names)
    c_names = (C.c_char_p * n)(*[s.encode() for s in names])
    c_planes = (C.POINTER(C.c_float) * n)(*[i.ctypes.data_as(C.POINTER(C.c_float)) for i in imgs])
    c_scales = (C.c_float * n)(*[float((scales or {}).get(s, 1.0)) for s in names])
    rc = _native.lib().igx_write_exr_layers(os.fsencode(path), c_names, c_planes, n, w, h, c_scales)
    if rc != 0:
        raise IgxError(f"cannot write EXR {path} (code {rc})")


def recommend_spi(width, height, interactive=False):
    """Runtime.cpp:61-69 for a GPU target."""
    spi_f = 8
    if interactive:
        spi_f //= 2
    spi = math.ceil(spi_f / ((width / 1000.0) * (height / 1000.0)))
    return max(1, min(64, spi))


class DenoiserSettings:
    """RuntimeOptions::Denoiser (src/runtime/RuntimeSettings.h:8-9): Enabled adds
    the info-buffer pass (technique/infobuffer.art) that fills the AOVs
    "Normals", "Albedo" and "Depth", in the first iteration only or in every one."""

    def __init__(self):
        self.Enabled = False
        self.FollowSpecular = False
        self.OnlyFirstIteration = True


class RuntimeOptions:
    """Subset of IG::RuntimeOptions (src/runtime/RuntimeSettings.h:16-62)."""

    def __init__(self):
        self.Denoiser = DenoiserSettings()
        self.Device = 0          # HIP device ordinal (--gpu-device)
        self.SPI = 0             # 0 = recommended
        self.Seed = 0
        self.AcquireStats = False
        self.OverrideFilmSize = (0, 0)
        self.Capacity = 0        # paths in flight; 0 = whole iteration (<= 16M)

    @staticmethod
    def makeDefault():
        return RuntimeOptions()


class Scene:
    """A loaded scene (owner of the igx_scene handle)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def from_file(path):
        err = C.create_string_buffer(2048)
        h = lib().igx_scene_load_file(os.fsencode(path), err, len(err))
        if not h:
            raise IgxError(err.value.decode())
        return Scene(h)

    @staticmethod
    def from_string(text, base_dir=None):
        if isinstance(text, dict):
            text = json.dumps(text)
        err = C.create_string_buffer(2048)
        h = lib().igx_scene_load_string(text.encode(), os.fsencode(base_dir) if base_dir else None, err, len(err))
        if not h:
            raise IgxError(err.value.decode())
        return Scene(h)

    @staticmethod
    def from_objects(objects):
        """igx_scene_from_objects: a scene built object by object
        (`ObjectScene`, the reference's in-memory IG::Scene)."""
        err = C.create_string_buffer(2048)
        h = lib().igx_scene_from_objects(objects._h, err, len(err))
        if not h:
            raise IgxError(err.value.decode())
        return Scene(h)

    @staticmethod
    def from_database(db, shading):
        """igx_scene_from_database: the reference's SceneDatabase tables
        (`_native.DatabaseView`) plus the shading tables (`_native.ShadingView`);
        the caller keeps the viewed buffers alive for the call."""
        err = C.create_string_buffer(2048)
        h = lib().igx_scene_from_database(C.byref(db), C.byref(shading), err, len(err))
        if not h:
            raise IgxError(err.value.decode())
        return Scene(h)

    @property
    def desc_ptr(self):
        """Raw `const igx_scene_desc*` (for C consumers such as the oracle)."""
        return C.cast(lib().igx_scene_get_desc(self._h), C.c_void_p)

    @property
    def desc(self):
        return lib().igx_scene_get_desc(self._h).contents

    @property
    def film_size(self):
        d = self.desc
        return d.film_width, d.film_height

    def close(self):
        if self._h:
            lib().igx_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObjectScene:
    """The reference's in-memory scene (IG::Scene: technique, camera, film and
    named bsdfs / shapes / lights / entities / textures / media, each a
    SceneObject of SceneProperty values) built through the igx_objscene_* C-ABI,
    the way a binding forwards the `const Scene*` that Runtime::loadFromScene
    receives (Runtime.cpp:183-199)."""

    OBJ = {"bsdfs": 0, "camera": 1, "entities": 2, "film": 3, "lights": 4, "media": 5, "shapes": 6, "technique": 7,
           "textures": 8, "parameters": 9}
    BOOL, INTEGER, NUMBER, STRING, TRANSFORM, VECTOR2, VECTOR3, INTEGER_ARRAY, NUMBER_ARRAY = range(1, 10)

    def __init__(self, base_dir=None):
        self._h = lib().igx_objscene_create(os.fsencode(base_dir) if base_dir else None)

    def add(self, category, plugin_type, name=None, base_dir=None):
        h = lib().igx_objscene_add(self._h, self.OBJ[category], plugin_type.encode(), name.encode() if name else None,
                                   os.fsencode(base_dir) if base_dir else None)
        if h < 0:
            raise IgxError(f"igx_objscene_add({category}, {plugin_type}, {name}) refused")
        return h

    def set(self, obj, key, ptype, value):
        if ptype == self.STRING:
            buf = C.create_string_buffer(value.encode())
            data, n = C.cast(buf, C.c_void_p), 1
        elif ptype in (self.BOOL, self.INTEGER, self.INTEGER_ARRAY):
            vals = [int(v) for v in (value if isinstance(value, (list, tuple)) else [value])]
            buf = (C.c_int32 * max(1, len(vals)))(*vals)
            data, n = C.cast(buf, C.c_void_p), len(vals)
        else:
            vals = [float(v) for v in (value if isinstance(value, (list, tuple)) else [value])]
            buf = (C.c_float * max(1, len(vals)))(*vals)
            data, n = C.cast(buf, C.c_void_p), len(vals)
        if lib().igx_objscene_set_property(self._h, obj, key.encode(), ptype, data, n) != 0:
            raise IgxError(f"igx_objscene_set_property({key}) refused")

    def set_value(self, obj, key, v):
        """A JSON value typed as the reference parser types it (getProperty, Parser.cpp:281-318)."""
        if isinstance(v, bool):
            self.set(obj, key, self.BOOL, int(v))
        elif isinstance(v, str):
            self.set(obj, key, self.STRING, v)
        elif isinstance(v, int):
            self.set(obj, key, self.INTEGER, v)
        elif isinstance(v, float):
            self.set(obj, key, self.NUMBER, v)
        elif isinstance(v, list):
            if len(v) == 2:
                self.set(obj, key, self.VECTOR2, v)
            elif len(v) == 3:
                self.set(obj, key, self.VECTOR3, v)
            elif len(v) in (9, 12, 16):
                m = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
                for i in range(3 if len(v) != 16 else 4):
                    for j in range(3 if len(v) == 9 else 4):
                        m[i][j] = float(v[i * (3 if len(v) == 9 else 4) + j])
                self.set(obj, key, self.TRANSFORM, [x for row in m for x in row])
            else:
                raise IgxError(f"property '{key}': an array of {len(v)} is not a scene property")
        elif isinstance(v, dict) and "values" in v:
            ints = str(v.get("type", "")) in ("int", "integer")
            self.set(obj, key, self.INTEGER_ARRAY if ints else self.NUMBER_ARRAY, v["values"])
        else:
            raise IgxError(f"property '{key}': unsupported value {v!r}")

    @staticmethod
    def from_dict(scene, base_dir=None):
        """Every object of a scene dict (the JSON schema), as a binding would
        forward the parsed IG::Scene's objects."""
        o = ObjectScene(base_dir)
        for cat in ("technique", "camera", "film"):
            if cat in scene:
                d = scene[cat]
                h = o.add(cat, d.get("type", ""))
                for k, v in d.items():
                    if k != "type":
                        o.set_value(h, k, v)
        for cat in ("textures", "bsdfs", "shapes", "lights", "media", "entities"):
            for d in scene.get(cat, []):
                h = o.add(cat, d.get("type", ""), d["name"])
                for k, v in d.items():
                    if k not in ("type", "name"):
                        o.set_value(h, k, v)
        return o

    def close(self):
        if self._h:
            lib().igx_objscene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Device:
    """Thin owner of an igx_device handle (IG::Device, src/runtime/device/Device.h:14-74)."""

    def __init__(self, hip_device=0):
        self._lib = lib()
        h = C.c_void_p()
        st = self._lib.igx_create(int(hip_device), C.byref(h))
        if st != 0 or not h:
            raise IgxError(f"igx_create({hip_device}) failed with status {st}")
        self._h = h
        self._film = None  # (width, height) of the last render: the shape of tonemap()
        self._rays_film = None  # (width, height) of camera_rays(): the scene's film, then the last render's

    def _check(self, st):
        if st != 0:
            raise IgxError(self._lib.igx_last_error(self._h).decode())

    def set_option(self, key, value):
        self._check(self._lib.igx_set_option(self._h, key.encode(), int(value)))

    def upload(self, scene):
        self._check(self._lib.igx_upload_scene(self._h, scene.desc_ptr))
        d = scene.desc
        self._rays_film = (d.film_width, d.film_height)

    def _rendered(self, params):
        self._film = (params.num_rays, 1) if params.num_rays > 0 else (params.width, params.height)
        if params.num_rays <= 0:
            self._rays_film = (params.width, params.height)

    def render(self, params):
        self._check(self._lib.igx_render(self._h, C.byref(params)))
        self._rendered(params)

    def set_camera(self, camera):
        """Replace the uploaded scene's camera (an N.Camera; igx_set_camera, as
        Runtime::setCameraOrientationParameter reaches the device through
        render's ParameterSet, Runtime.cpp:703-708)."""
        self._check(self._lib.igx_set_camera(self._h, C.byref(camera)))

    def render_iterations(self, params, count):
        """`count` consecutive iterations from params.iteration (igx_render_iterations)."""
        self._check(self._lib.igx_render_iterations(self._h, C.byref(params), int(count)))
        self._rendered(params)

    def framebuffer(self, count, name=None):
        """The film, or a named AOV (igx_get_aov: "Color", with the
        technique's aov_mis "Direct Weights" / "NEE Weights", with option
        "denoise_aovs" "Normals" / "Albedo" / "Depth"), and its iteration
        count (the denoiser's AOVs count their own passes)."""
        out = np.zeros(count, dtype=np.float32)
        it = C.c_uint64()
        if name is None:
            self._check(self._lib.igx_get_framebuffer(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), count, C.byref(it)))
        else:
            self._check(self._lib.igx_get_aov(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), count,
                                              C.byref(it)))
        return out, int(it.value)

    def framebuffer_device_ptr(self):
        p = C.c_void_p()
        n = C.c_size_t()
        self._check(self._lib.igx_framebuffer_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pack_tiles(self, params, dst_ptr, count):
        self._check(self._lib.igx_pack_tiles(self._h, C.byref(params), C.c_void_p(dst_ptr), count))

    def aov_iteration_count(self, name=None):
        """igx_aov_iteration_count: the count `framebuffer(count, name)` returns, without the copy."""
        it = C.c_uint64()
        self._check(self._lib.igx_aov_iteration_count(self._h, name.encode() if name else None, C.byref(it)))
        return int(it.value)

    def clear(self, name=None):
        """Everything (igx_clear), or with a name that film and its iteration
        count only (igx_clear_aov; "Color" is the film)."""
        if name is None:
            self._check(self._lib.igx_clear(self._h))
        else:
            self._check(self._lib.igx_clear_aov(self._h, name.encode()))

    # ---- film post-processing on the device (igx_tonemap / igx_imageinfo) ----
    @staticmethod
    def _tonemap_settings(method, use_gamma, scale, exposure_factor, exposure_offset):
        return TonemapSettings(int(method), int(bool(use_gamma)), float(scale), float(exposure_factor), float(exposure_offset))

    def tonemap(self, name=None, method=0, use_gamma=False, scale=1.0, exposure_factor=1.0, exposure_offset=0.0):
        """Device::tonemap of the film or a named AOV, scaled by scale / its
        iteration count: an (h, w) uint32 array of (a << 24) | (r << 16) |
        (g << 8) | b words (method: 0 none, 1 Reinhard, 2 modified Reinhard,
        3 ACES, else Uncharted 2).  None before the first render."""
        if self._film is None:
            return None
        w, h = self._film
        out = np.zeros((h, w), dtype=np.uint32)
        ts = self._tonemap_settings(method, use_gamma, scale, exposure_factor, exposure_offset)
        self._check(self._lib.igx_tonemap(self._h, name.encode() if name else None, C.byref(ts),
                                          out.ctypes.data_as(C.POINTER(C.c_uint32)), w * h))
        return out

    def tonemap_film(self, ptr, w, h, method=0, use_gamma=False, scale=1.0, exposure_factor=1.0, exposure_offset=0.0,
                     out_ptr=None):
        """igx_tonemap_film over w * h * 3 floats at the device pointer `ptr`
        (e.g. tensor.data_ptr()), `scale` as given.  Returns the (h, w) uint32
        image, or with `out_ptr` (device memory for w * h words) writes there
        and returns None."""
        ts = self._tonemap_settings(method, use_gamma, scale, exposure_factor, exposure_offset)
        if out_ptr is not None:
            self._check(self._lib.igx_tonemap_film(self._h, C.c_void_p(ptr), int(w), int(h), C.byref(ts), C.c_void_p(out_ptr), 1))
            return None
        out = np.zeros((h, w), dtype=np.uint32)
        self._check(self._lib.igx_tonemap_film(self._h, C.c_void_p(ptr), int(w), int(h), C.byref(ts), C.c_void_p(out.ctypes.data), 0))
        return out

    def _imageinfo(self, call, scale, bins, error_stats):
        bins = int(bins)
        hist = np.zeros((4, max(bins, 1)), dtype=np.int32)
        ptrs = [hist[c].ctypes.data_as(C.POINTER(C.c_int32)) if bins > 0 else None for c in range(4)]
        st = ImageInfoSettings(float(scale), bins, *ptrs, int(bool(error_stats)), int(bins > 0))
        out = ImageInfoOutput()
        self._check(call(C.byref(st), C.byref(out)))
        res = {k: getattr(out, k) for k, _ in ImageInfoOutput._fields_}
        if bins > 0:
            for c, k in enumerate("rgbl"):
                res["histogram_" + k] = hist[c].copy()
        return res

    def imageinfo(self, name=None, scale=1.0, bins=0, error_stats=True):
        """Device::imageinfo of the film or a named AOV (scaled by scale / its
        iteration count): a dict of min, max, avg, soft_min, soft_max, median,
        inf_count, nan_count, neg_count and, with bins > 0, histogram_r / _g /
        _b / _l (int32 arrays of `bins`)."""
        aov = name.encode() if name else None
        return self._imageinfo(lambda st, out: self._lib.igx_imageinfo(self._h, aov, st, out), scale, bins, error_stats)

    def imageinfo_film(self, ptr, w, h, scale=1.0, bins=0, error_stats=True):
        """igx_imageinfo_film over w * h * 3 floats at the device pointer `ptr`, `scale` as given."""
        return self._imageinfo(lambda st, out: self._lib.igx_imageinfo_film(self._h, C.c_void_p(ptr), int(w), int(h), st, out),
                               scale, bins, error_stats)

    # ---- daylight glare probability on the device (igx_evaluate_glare) ----
    def _evaluate_glare(self, call, shape, lum_max, lum_avg, lum_mul, vertical_illuminance, scale, overlay):
        gs = GlareSettings(float(scale), float(lum_max), float(lum_avg), float(lum_mul), float(vertical_illuminance))
        out = GlareOutput()
        if overlay is not None:
            overlay = np.ascontiguousarray(overlay, dtype=np.uint32).copy()
            if overlay.shape != shape:
                raise ValueError(f"overlay must have shape {shape}, not {overlay.shape}")
        self._check(call(C.byref(gs), C.c_void_p(overlay.ctypes.data) if overlay is not None else None, C.byref(out)))
        res = {k: getattr(out, k) for k, _ in GlareOutput._fields_}
        return res if overlay is None else (res, overlay)

    def evaluate_glare(self, name=None, lum_max=0.0, lum_avg=0.0, lum_mul=5.0, vertical_illuminance=-1.0, scale=1.0,
                       overlay=None):
        """Device::evaluateGlare of the film or a named AOV (scaled by scale /
        its iteration count) through the current camera: a dict of dgp,
        vertical_illuminance, avg_lum, avg_omega (the source's summed solid
        angle) and num_pixels.  lum_max and lum_avg are imageinfo's soft_max
        and avg; a vertical_illuminance >= 0 is used as given.  With `overlay`
        (an (h, w) uint32 image, e.g. tonemap()'s) also a copy of it with the
        heat-map words of the pixels above the threshold laid over.  None
        before the first render."""
        if self._film is None:
            return None
        w, h = self._film
        aov = name.encode() if name else None
        return self._evaluate_glare(lambda gs, ov, out: self._lib.igx_evaluate_glare(self._h, aov, gs, ov, w * h, out), (h, w),
                                    lum_max, lum_avg, lum_mul, vertical_illuminance, scale, overlay)

    def evaluate_glare_film(self, ptr, w, h, lum_max=0.0, lum_avg=0.0, lum_mul=5.0, vertical_illuminance=-1.0, scale=1.0,
                            overlay=None, overlay_ptr=None):
        """igx_evaluate_glare_film over w * h * 3 floats at the device pointer
        `ptr`, `scale` as given, the current camera on w x h.  `overlay` as for
        evaluate_glare; with `overlay_ptr` (device memory for w * h words) the
        words of the pixels above the threshold are stored there instead."""
        if overlay_ptr is not None:
            return self._evaluate_glare(
                lambda gs, ov, out: self._lib.igx_evaluate_glare_film(self._h, C.c_void_p(ptr), int(w), int(h), gs,
                                                                      C.c_void_p(overlay_ptr), 1, out),
                (h, w), lum_max, lum_avg, lum_mul, vertical_illuminance, scale, None)
        return self._evaluate_glare(
            lambda gs, ov, out: self._lib.igx_evaluate_glare_film(self._h, C.c_void_p(ptr), int(w), int(h), gs, ov, 0, out),
            (h, w), lum_max, lum_avg, lum_mul, vertical_illuminance, scale, overlay)

    def synchronize(self):
        self._check(self._lib.igx_synchronize(self._h))

    def wait_ready(self):
        """igx_wait_ready: the handle's queued chunks are in their late bounces."""
        self._check(self._lib.igx_wait_ready(self._h))

    def stats(self):
        s = Stats()
        self._check(self._lib.igx_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def store_split(self):
        """igx_get_store_split: the instrumented k_extend's store-phase wave
        cycles by part (group take, class tests, append, stores)."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.igx_get_store_split(self._h, out))
        return list(out)

    def reset_stats(self):
        self._check(self._lib.igx_reset_stats(self._h))

    def trace_hits(self, rays, flags=0x1):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        ep = np.zeros((n, 2), dtype=np.int32)
        tuv = np.zeros((n, 3), dtype=np.float32)
        self._check(self._lib.igx_trace_hits(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n, flags,
                                             ep.ctypes.data_as(C.POINTER(C.c_int32)),
                                             tuv.ctypes.data_as(C.POINTER(C.c_float))))
        return ep, tuv

    def camera_rays(self, iteration=0, sample=0):
        """The camera rays the renderer traces for sample `sample` of iteration
        `iteration` (igx_camera_rays): an (height, width, 8) array of org, dir,
        tmin, tmax, for the film, frame and seed of the last render call (the
        uploaded scene's film, frame 0 and seed 0 before the first) and the
        current camera.  Feed it to trace_hits or to ray-list mode."""
        if self._rays_film is None:
            raise IgxError("camera_rays: no scene uploaded")
        w, h = self._rays_film
        out = np.zeros((h, w, 8), dtype=np.float32)
        self._check(self._lib.igx_camera_rays(self._h, int(iteration), int(sample),
                                              out.ctypes.data_as(C.POINTER(C.c_float)), 0))
        return out

    def trace_occlusion(self, rays, flags=0x8):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        occ = np.zeros(n, dtype=np.int32)
        self._check(self._lib.igx_trace_occlusion(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n, flags,
                                                  occ.ctypes.data_as(C.POINTER(C.c_int32))))
        return occ

    def close(self):
        if getattr(self, "_h", None):
            self._lib.igx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Runtime:
    """IG::Runtime restricted to the hot path (src/runtime/Runtime.h:19-198)."""

    def __init__(self, scene, opts=None):
        opts = opts or RuntimeOptions.makeDefault()
        self.scene = scene
        self.options = opts
        w, h = scene.film_size
        if opts.OverrideFilmSize[0] > 0:
            w, h = opts.OverrideFilmSize
        self.FilmWidth, self.FilmHeight = int(w), int(h)
        self.SamplesPerIteration = opts.SPI if opts.SPI > 0 else recommend_spi(self.FilmWidth, self.FilmHeight)
        self.Seed = opts.Seed
        self.device = Device(opts.Device)
        if opts.AcquireStats:
            self.device.set_option("timing", 1)
        if opts.Capacity:
            self.device.set_option("capacity", opts.Capacity)
        dn = opts.Denoiser
        if dn.Enabled:
            self.device.set_option("denoise_aovs", 1 if dn.OnlyFirstIteration else 2)
            self.device.set_option("denoise_follow_specular", int(bool(dn.FollowSpecular)))
        self.device.upload(scene)
        self._iteration = 0
        self._frame = 0
        self._fb_count = self.FilmWidth * self.FilmHeight * 3

    @property
    def IterationCount(self):
        return self._iters

    def _params(self, tile=None):
        p = RenderParams()
        p.width, p.height = self.FilmWidth, self.FilmHeight
        p.spi = self.SamplesPerIteration
        p.iteration = self._iteration
        p.frame = self._frame
        p.seed = self.Seed
        if tile is not None:
            p.tile_size, p.tile_offset, p.tile_stride = tile
        return p

    _iters = 0

    def step(self, tile=None):
        """Runtime::step: one iteration of SamplesPerIteration samples."""
        self.device.render(self._params(tile))
        self._iteration += 1
        self._iters += 1

    def getFramebufferForHost(self, name=""):
        """Runtime::getFramebufferForHost(name) (Runtime.cpp:417-435): the
        film ("" / "Color") or a named AOV of the technique."""
        fb, it = self.device.framebuffer(self._fb_count, name or None)
        if name in ("", "Color"):
            self._iters = it
        return fb.reshape(self.FilmHeight, self.FilmWidth, 3)

    def getFramebufferIterationCount(self, name=""):
        """The iteration count of the film or of a named AOV (an AOV of the
        denoiser counts its own passes, Device.cpp:1390-1403)."""
        return self.device.aov_iteration_count(name or None)

    def aovs(self):
        """Names of the enabled AOVs (TechniqueInfo::EnabledAOVs)."""
        names = []
        if self.scene.desc.technique.aov_mis:
            names += ["Direct Weights", "NEE Weights"]
        if self.options.Denoiser.Enabled:
            names += ["Normals", "Albedo", "Depth"]
        return names

    def clearFramebuffer(self, name=None):
        """Runtime::clearFramebuffer() (Runtime.cpp:427-430): everything; with a
        name, Runtime::clearFramebuffer(name) (:432-435, Device.cpp:1415-1443):
        the film ("" / "Color") or one AOV, and its iteration count, only."""
        self.device.clear(None if name is None else (name or "Color"))
        if name in (None, "", "Color"):
            self._iters = 0

    def reset(self):
        self.clearFramebuffer()
        self._iteration = 0

    def trace(self, rays):
        """Runtime::trace (Runtime.cpp:385-407): radiance per ray, one iteration."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        p = self._params()
        p.num_rays = rays.shape[0]
        p.rays = rays.ctypes.data_as(C.POINTER(C.c_float))
        self.device.clear()
        self.device.render(p)
        fb, it = self.device.framebuffer(rays.shape[0] * 3)
        self.device.clear()
        return fb.reshape(-1, 3) / max(it, 1)

    def tonemap(self, name="", **settings):
        """Runtime::tonemap (Runtime.cpp:637): Device.tonemap of the runtime's film or AOV."""
        return self.device.tonemap(name or None, **settings)

    def imageinfo(self, name="", **settings):
        """Runtime::imageinfo (Runtime.cpp:663): Device.imageinfo of the runtime's film or AOV."""
        return self.device.imageinfo(name or None, **settings)

    def evaluateGlare(self, name="", **settings):
        """Runtime::evaluateGlare (Runtime.cpp:640): Device.evaluate_glare of the runtime's film or AOV."""
        return self.device.evaluate_glare(name or None, **settings)

    def getStatistics(self):
        return self.device.stats()

    def close(self):
        self.device.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def loadFromFile(path, opts=None):
    return Runtime(Scene.from_file(path), opts)


def loadFromString(text, opts=None, base_dir=None):
    return Runtime(Scene.from_string(text, base_dir), opts)
