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
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(PKG, "host"),
                    os.path.join(ROOT, "tools", "post_bench_host.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.post_host_tonemap.argtypes = [fp, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_uint32)]
    lib.post_host_tonemap.restype = None
    lib.post_host_imageinfo.argtypes = [fp, C.c_size_t, C.c_size_t, C.c_float, C.c_size_t, ip, ip, ip, ip]
    lib.post_host_imageinfo.restype = C.c_float
    return lib


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
        measure(ignis_amd, torch, host, f, size, spi, args.calls, args.warmup, args.method, not args.no_gamma) for f, size, spi in cases]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
