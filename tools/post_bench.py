#!/usr/bin/env python3
"""Times the film post-processing calls on the GPU next to the host path they
replace.

After one iteration of the diamond scene at 1000 x 1000, and one of S-deep at
4096 x 4096, 20 calls each (after 3 warm-up calls) of
  * Device.tonemap          device kernel, packed image copied to the host
  * Device.tonemap_film     device kernel, device output (no copy)
  * Device.imageinfo        bins = 256
  * the host path           Device.framebuffer (the whole film to the host) plus
                            the loops of host/film_tools.h (tools/post_bench_host.cpp),
                            which is what IG::Device::tonemap / imageinfo did
                            before the kernels.
And on a random film of each size seen through a fishlens camera, 5 bright
4 x 4 patches as the glare source:
  * Device.evaluate_glare_film   one k_glare_scan, the slab back, the tail on the host
  * the same with a device overlay
  * glare_host                   the film to the host plus host/glare_model.h's loop
and 64 single-pixel sources across the 1000 x 1000 film, whose avg_omega is that
pixel's solid angle as the device computes it, against float64.
Every call returns after a stream synchronise, so a host clock around it is the
call's time.  Prints one JSON object (median and minimum per call in ms, the
bytes k_tonemap moves and the rate that implies) and writes it with --out.

    python tools/post_bench.py --out profiles/post_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")
sys.path.insert(0, PKG)


def build_host_helper():
    out = os.path.join(tempfile.mkdtemp(prefix="post_bench_"), "libpost_bench_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(PKG, "host"),
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "post_bench_host.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.post_host_tonemap.argtypes = [fp, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_uint32)]
    lib.post_host_tonemap.restype = None
    lib.post_host_imageinfo.argtypes = [fp, C.c_size_t, C.c_size_t, C.c_float, C.c_size_t, ip, ip, ip, ip]
    lib.post_host_imageinfo.restype = C.c_float
    lib.post_host_glare.argtypes = [fp, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.post_host_glare.restype = None
    return lib


def fish_omega64(size, x, y):
    """float64 solid angle of pixel (x, y) of a size x size fishlens film (glare.art's calc_omega)"""
    def d(px, py):
        fx, fy = 2.0 * px / size - 1, 1 - 2.0 * py / size
        r = np.hypot(fx, fy)
        th = r * np.pi / 2
        v = np.array([np.sin(th) * fx / r, np.sin(th) * fy / r, -np.cos(th)]) if r else np.array([0, 0, -1.0])
        return v / np.linalg.norm(v)
    r = [d(x, y), d(x, y + 1), d(x + 1, y + 1), d(x + 1, y)]
    n = [np.cross(r[i], r[(i + 1) % 4] - r[i]) for i in range(4)]
    n = [v / np.linalg.norm(v) for v in n]
    return sum(np.pi - np.arccos(n[i] @ n[(i + 1) % 4]) for i in range(4)) - 2 * np.pi


def measure_glare(ignis_amd, torch, host, size, calls, warmup):
    from ignis_amd import _native
    dev = ignis_amd.Device(0)
    cam = _native.Camera()
    cam.dir[:], cam.up[:] = [0, 0, -1], [0, 1, 0]
    cam.near_clip, cam.far_clip, cam.type = 0.01, 100, 2  # fishlens
    dev.set_camera(cam)
    rng = np.random.default_rng(1)
    film = (rng.random((size, size, 3), dtype=np.float32) * 0.5).astype(np.float32)
    for k in range(5):
        x0, y0 = (k + 1) * size // 7, (k + 2) * size // 9
        film[y0:y0 + 4, x0:x0 + 4] = 64.0
    t = torch.from_numpy(film).to("cuda")
    d_overlay = torch.zeros(size * size, dtype=torch.int32, device="cuda")
    settings = dict(lum_max=64.0, lum_avg=0.25, lum_mul=5.0)
    gs = _native.GlareSettings(1.0, 64.0, 0.25, 5.0, -1.0)
    out = _native.GlareOutput()
    back = np.empty_like(film)

    def host_glare():
        back[...] = t.cpu().numpy()  # the film to the host, as Device.framebuffer does
        host.post_host_glare(back.ctypes.data_as(C.POINTER(C.c_float)), size, size, C.addressof(cam), C.addressof(gs), None,
                             C.addressof(out))

    res = {"width": size, "height": size, "camera": "fishlens"}
    res["device_glare"] = timed(lambda: dev.evaluate_glare_film(t.data_ptr(), size, size, **settings), calls, warmup)
    res["device_glare_device_overlay"] = timed(
        lambda: dev.evaluate_glare_film(t.data_ptr(), size, size, overlay_ptr=d_overlay.data_ptr(), **settings), calls, warmup)
    res["host_glare"] = timed(host_glare, 3, 1)
    res["device"] = dev.evaluate_glare_film(t.data_ptr(), size, size, **settings)
    res["host"] = {k: getattr(out, k) for k, _ in _native.GlareOutput._fields_}
    if size <= 1000:
        # one-pixel sources: avg_omega is the pixel's solid angle as the device computes it
        worst, worst_rel, lo, hi = 0.0, 0.0, 1e30, 0.0
        for k in range(64):
            x, y = int(rng.integers(size // 8, 7 * size // 8)), int(rng.integers(size // 8, 7 * size // 8))
            one = torch.zeros((size, size, 3), dtype=torch.float32, device="cuda")
            one[y, x] = 64.0
            got = dev.evaluate_glare_film(one.data_ptr(), size, size, **settings)
            want = fish_omega64(size, x, y)
            assert got["num_pixels"] == 1
            worst, worst_rel = max(worst, abs(got["avg_omega"] - want)), max(worst_rel, abs(got["avg_omega"] - want) / want)
            lo, hi = min(lo, want), max(hi, want)
        res["single_pixel_omega"] = {"pixels": 64, "omega_min": lo, "omega_max": hi, "worst_abs_error": worst, "worst_rel_error": worst_rel}
    dev.close()
    return res


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "calls": calls}


def measure(ignis_amd, torch, host, scene_file, size, spi, calls, warmup, method, gamma):
    scene = ignis_amd.Scene.from_file(os.path.join(ROOT, "scenes", scene_file))
    dev = ignis_amd.Device(0)
    dev.upload(scene)
    p = ignis_amd.RenderParams()
    p.width = p.height = size
    p.spi = spi
    dev.render(p)
    dev.synchronize()
    n = size * size
    ptr, count = dev.framebuffer_device_ptr()
    assert count == 3 * n
    d_out = torch.empty(n, dtype=torch.int32, device="cuda")
    px = np.zeros(n, np.uint32)
    hist = np.zeros((4, 256), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)

    def host_tonemap():
        fb, it = dev.framebuffer(3 * n)
        host.post_host_tonemap(fb.ctypes.data_as(fp), n, 1.0 / max(it, 1), method, int(gamma), 1.0, 0.0,
                               px.ctypes.data_as(C.POINTER(C.c_uint32)))

    def host_imageinfo():
        fb, it = dev.framebuffer(3 * n)
        host.post_host_imageinfo(fb.ctypes.data_as(fp), size, size, 1.0 / max(it, 1), 256, *[hist[c].ctypes.data_as(ip) for c in range(4)])

    res = {"scene": scene_file, "width": size, "height": size, "spi": spi, "method": method, "use_gamma": bool(gamma)}
    res["device_tonemap"] = timed(lambda: dev.tonemap(method=method, use_gamma=gamma), calls, warmup)
    res["device_tonemap_film_device_output"] = timed(
        lambda: dev.tonemap_film(ptr, size, size, method=method, use_gamma=gamma, out_ptr=d_out.data_ptr()), calls, warmup)
    res["device_imageinfo_bins256"] = timed(lambda: dev.imageinfo(bins=256), calls, warmup)
    res["host_tonemap"] = timed(host_tonemap, max(3, calls // 4), 1)
    res["host_imageinfo_bins256"] = timed(host_imageinfo, max(3, calls // 4), 1)
    # k_tonemap reads 12 B and writes 4 B per pixel; the device-output call is the kernel plus launch and wait
    moved = 16 * n
    res["tonemap_bytes_moved"] = moved
    res["tonemap_film_implied_GBps"] = round(moved / (res["device_tonemap_film_device_output"]["min_ms"] * 1e-3) / 1e9, 1)
    # the same image and statistics both ways (device pow differs from the host's by a byte at most)
    img = dev.tonemap(method=method, use_gamma=gamma).reshape(-1)
    host_tonemap()
    diff = np.abs(((img[:, None] >> np.array([16, 8, 0], np.uint32)) & 255).astype(np.int32) -
                  ((px[:, None] >> np.array([16, 8, 0], np.uint32)) & 255).astype(np.int32))
    res["tonemap_max_channel_difference_to_host"] = int(diff.max())
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--method", type=int, default=3, help="tone curve (3 = ACES)")
    ap.add_argument("--no-gamma", action="store_true")
    ap.add_argument("--skip-4096", action="store_true")
    ap.add_argument("--glare-only", action="store_true", help="only the glare measurements")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("post_bench.py needs the GPU: a timing taken elsewhere says nothing about it")
    torch.zeros(1, device="cuda")
    import ignis_amd

    host = build_host_helper()
    cases = [("diamond_scene.json", 1000, 8)] + ([] if args.skip_4096 else [("s_deep.json", 4096, 8)])
    out = {"tool": "tools/post_bench.py", "device": torch.cuda.get_device_name(0), "results": [
        measure(ignis_amd, torch, host, f, size, spi, args.calls, args.warmup, args.method, not args.no_gamma)
        for f, size, spi in ([] if args.glare_only else cases)],
        "glare": [measure_glare(ignis_amd, torch, host, size, args.calls, args.warmup) for size in [1000] + ([] if args.skip_4096 else [4096])]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
