"""Daylight glare probability on the device (igx_evaluate_glare, k_glare_scan)
against a float64 restatement of entrypoints/glare.art written here, and word
for word against the host restatement glare_host (host/glare_model.h, compiled
into a small shared library with g++): synthetic films handed to
evaluate_glare_film, a rendered constant environment through the Runtime, the
IG::Device facade and igcli.

Bounds.  B = 6.5e-6 is the per-pixel bound on a float32 solid angle, derived in
tests/native/glare_check.cpp by counting rounded operations (the float64
restatement computes its own corners; a corner off by 1e-7 moves a pixel's
solid angle by 1e-7 times its edge, below 1e-8).  With K source pixels of N:
  avg_omega            K * B
  vertical_illuminance B * sum(lum_i * |cos_i|) (every pixel's own weight, which
                       is at most N * B * the largest weight) and a relative
                       1e-5 for the rounding of the products and of the at most
                       50 additions in a row of the tree
  avg_lum              numerator and denominator each off by at most K * B
                       (times the luminance): 2 * K * B * L / omega, and 1e-5 L
  dgp                  through glare_finish: c1 * d_ev + c2 / ln 10 * acc / (1 +
                       acc) * (2 d_lum / L + d_omega / omega + 1.87 d_ev / ev +
                       2e-5 for the position index, which glare_check.cpp holds
                       to 1e-5), and 1e-6 for its own roundings
A corner taken for a centre, or the corners in another order, moves omega by
about 1 / w: ten times these bounds and more."""
import copy
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ignis_amd
from ignis_amd import _native
from conftest import ENV_LIGHT, flat_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")
B = 6.5e-6
MARK = 0x01234567  # what the overlay buffers hold before a call
BG, SRC = 0.25, 8.0  # binary fractions; luminances 44.75 and 1432 against a threshold of 223.75
SETTINGS = dict(lum_max=8.0, lum_avg=0.25, lum_mul=5.0)
PERSPECTIVE, FISHLENS = 0, 2


def camera(kind):
    c = _native.Camera()
    c.eye[:] = [0, 0, 0]
    c.dir[:] = [0, 0, -1]
    c.up[:] = [0, 1, 0]
    c.fov = math.radians(60)
    c.near_clip, c.far_clip = 0.01, 100
    c.type = kind
    return c


# ---- float64 restatement of glare.art ---------------------------------------
def dirs64(kind, w, h, xs, ys):
    """camera directions at the lattice points (xs, ys); right = +x, up = +y, dir = -z"""
    nx, ny, aspect = 2.0 * xs / w - 1, 1 - 2.0 * ys / h, w / h
    if kind == FISHLENS:
        fx, fy = nx * max(aspect, 1.0), ny * (1.0 if aspect > 1 else aspect)
        r = np.sqrt(fx * fx + fy * fy)
        th = r * np.pi / 2
        safe = np.where(r == 0, 1, r)
        d = np.stack([np.sin(th) * fx / safe, np.sin(th) * fy / safe, -np.cos(th)], -1)
    else:
        tx = math.tan(math.radians(30))
        d = np.stack([tx * nx, tx / aspect * ny, -np.ones_like(nx)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def omega64(kind, w, h):
    ys, xs = np.mgrid[0:h + 1, 0:w + 1].astype(np.float64)
    D = dirs64(kind, w, h, xs, ys)
    r1, r2, r3, r4 = D[:-1, :-1], D[1:, :-1], D[1:, 1:], D[:-1, 1:]  # (x, y), (x, y + 1), (x + 1, y + 1), (x + 1, y)

    def splane(a, b):
        n = np.cross(a, b - a)
        ln = np.linalg.norm(n, axis=-1, keepdims=True)
        return np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0)

    n = [splane(r1, r2), splane(r2, r3), splane(r3, r4), splane(r4, r1)]
    ang = sum(np.pi - np.arccos(np.clip(np.einsum("...k,...k", n[i], n[(i + 1) % 4]), -1, 1)) for i in range(4))
    return ang - 2 * np.pi, np.abs(r1[..., 2])  # |dot(dir, r1)| with dir = -z


def posindex64(kind, w, h, px, py):
    d = dirs64(kind, w, h, np.float64(px), np.float64(py))
    up, view, right = np.array([0, 1.0, 0]), np.array([0, 0, -1.0]), np.array([1.0, 0, 0])
    phi = math.acos(up @ d) - math.pi / 2
    theta = math.pi / 2 - math.acos(right @ d)
    sigma = math.acos(min(1.0, view @ d))
    hv = d / math.cos(sigma) - d
    if not hv @ hv > 0:
        return 1.0  # difference 2
    tau = math.degrees(math.acos(up @ (hv / np.linalg.norm(hv))))
    phi = phi or 0.00001
    theta = theta or 0.0001
    sigma = math.degrees(abs(sigma))
    p = math.exp((35.2 - 0.31889 * tau - 1.22 * math.exp(-2 * tau / 9)) / 1000 * sigma
                 + (21 + 0.26667 * tau - 0.002963 * tau * tau) / 100000 * sigma * sigma)
    if phi < 0:
        dd, s = 1 / math.tan(phi), math.tan(theta) / math.tan(phi)
        r = math.sqrt(1 / dd / dd + s * s / dd / dd)
        p = 1 + (1.2 if r > 0.6 else 0.8) * min(r, 3.0)
    return min(p, 16.0)


def glare64(kind, film, lum_avg, lum_mul, scale=1.0, ev_given=-1.0):
    """-> the outputs and their bounds (module docstring)"""
    h, w, _ = film.shape
    omega, cos = omega64(kind, w, h)
    lum = 179 * (film.astype(np.float64) * scale @ np.array([0.2126729, 0.7151522, 0.0721750]))
    src = lum > 179 * lum_avg * lum_mul
    K = int(src.sum())
    ev = float((lum * cos * omega).sum()) if ev_given < 0 else ev_given
    d_ev = (B * float((lum * cos).sum()) + 1e-5 * ev) if ev_given < 0 else 0.0
    out = dict(num_pixels=K, vertical_illuminance=ev, avg_lum=0.0, avg_omega=0.0, dgp=5.87e-5 * ev + 0.16)
    tol = dict(vertical_illuminance=d_ev, avg_lum=0.0, avg_omega=0.0, dgp=5.87e-5 * d_ev + 1e-6)
    if K:
        ys, xs = np.mgrid[0:h, 0:w]
        om = float(omega[src].sum())
        L = float((lum * omega)[src].sum()) / om
        gx, gy = float((xs * omega)[src].sum()) / om, float((ys * omega)[src].sum()) / om
        # the centroid is not within rounding of a lattice line, so (int) cannot flip
        assert min(gx % 1, 1 - gx % 1, gy % 1, 1 - gy % 1) > 0.05 or (w, h) == (1, 1), (gx, gy)
        posi = posindex64(kind, w, h, int(gx), int(gy))
        acc = L ** 2 / posi ** 2 * om / ev ** 1.87
        d_om, d_lum = K * B, 2 * K * B * float(lum[src].max()) / om + 1e-5 * L
        out.update(avg_lum=L, avg_omega=om, dgp=5.87e-5 * ev + 0.0981 * math.log10(1 + acc) + 0.16)
        tol.update(avg_lum=d_lum, avg_omega=d_om,
                   dgp=5.87e-5 * d_ev + 0.0981 / math.log(10) * acc / (1 + acc) * (2 * d_lum / L + d_om / om + 1.87 * d_ev / ev + 2e-5)
                   + 1e-6)
        out["posindex"] = posi
    return out, tol


# ---- the host restatement glare_host through ctypes --------------------------
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("glare") / "libglare_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG, "host"), os.path.join(ROOT, "tests", "native", "glare_host_lib.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.glare_host_c.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_native.Camera), C.POINTER(_native.GlareSettings), C.c_void_p,
                               C.POINTER(_native.GlareOutput)]
    L.glare_host_c.restype = None
    return L


def glare_host(L, kind, film, vertical_illuminance=-1.0, scale=1.0):
    h, w, _ = film.shape
    film = np.ascontiguousarray(film, np.float32)
    overlay = np.full((h, w), MARK, np.uint32)
    gs = _native.GlareSettings(scale, SETTINGS["lum_max"], SETTINGS["lum_avg"], SETTINGS["lum_mul"], vertical_illuminance)
    out = _native.GlareOutput()
    cam = camera(kind)
    L.glare_host_c(film.ctypes.data, w, h, C.byref(cam), C.byref(gs), overlay.ctypes.data, C.byref(out))
    return {k: getattr(out, k) for k, _ in _native.GlareOutput._fields_}, overlay


@pytest.fixture(scope="module")
def device():
    dev = ignis_amd.Device(0)
    yield dev
    dev.close()


def make_film(w, h, patches):
    """grey background, (x0, y0, width, height) patches of the source colour"""
    film = np.full((h, w, 3), BG, np.float32)
    for x0, y0, pw, ph in patches:
        film[y0:y0 + ph, x0:x0 + pw] = SRC
    return film


def bits(res):
    return {k: np.float32(v).tobytes() if isinstance(v, float) else v for k, v in res.items()}


# kind, w, h, source patches.  Even-sized patches, so the omega-weighted centre
# sits near a half pixel.  67 x 45: odd, a thread's 4 pixels wrap rows; 131 x 97
# spans two blocks of 8192 pixels (the second starts in row 62) with a source on each side; 64 x 64: the patch
# whose centre (32.5, 32.5) picks the lattice point (w / 2, h / 2), the view
# direction itself (difference 2); 96 x 64: one source in the upper half
# (glare.art's Iwata branch), and in the 67 x 45 and 300 x 5 films in the lower
# half (its Guth branch).
CASES = {
    "1x1": (PERSPECTIVE, 1, 1, [(0, 0, 1, 1)]),
    "3x2": (PERSPECTIVE, 3, 2, [(1, 0, 2, 2)]),
    "67x45": (PERSPECTIVE, 67, 45, [(40, 30, 4, 2)]),
    "300x5": (PERSPECTIVE, 300, 5, [(200, 3, 6, 2)]),
    "131x97": (PERSPECTIVE, 131, 97, [(40, 58, 4, 4), (40, 64, 4, 4)]),
    "fish64x64-centre": (FISHLENS, 64, 64, [(31, 31, 4, 4)]),
    "fish96x64-upper": (FISHLENS, 96, 64, [(60, 12, 6, 4)]),
    "fish64x64-lower": (FISHLENS, 64, 64, [(20, 44, 4, 2)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_synthetic_film(device, host_lib, case):
    kind, w, h, patches = CASES[case]
    film = make_film(w, h, patches)
    K = sum(pw * ph for _, _, pw, ph in patches)
    device.set_camera(camera(kind))
    t = torch.from_numpy(film).to("cuda:0")
    res, overlay = device.evaluate_glare_film(t.data_ptr(), w, h, overlay=np.full((h, w), MARK, np.uint32), **SETTINGS)
    want, tol = glare64(kind, film, SETTINGS["lum_avg"], SETTINGS["lum_mul"])
    host, host_overlay = glare_host(host_lib, kind, film)
    print(case, "device", res, "\n  host", host, "\n  float64", want, "\n  bounds", tol)
    # exact outputs
    assert res["num_pixels"] == K == want["num_pixels"] == host["num_pixels"]
    np.testing.assert_array_equal(overlay, host_overlay)
    assert int((overlay != MARK).sum()) == K and (overlay[film[..., 0] == BG] == MARK).all()
    assert ((overlay[film[..., 0] == SRC] >> 24) == 255).all()
    # sums against float64
    for key in ("vertical_illuminance", "avg_omega", "avg_lum", "dgp"):
        assert abs(res[key] - want[key]) <= tol[key], (key, res[key], want[key], tol[key])
    if case == "fish64x64-centre":
        assert want["posindex"] == 1.0
    # the same bits on every call, with and without an overlay, to host or device memory
    assert bits(device.evaluate_glare_film(t.data_ptr(), w, h, **SETTINGS)) == bits(res)
    dev_overlay = torch.full((h, w), MARK, dtype=torch.int32, device="cuda:0")
    assert bits(device.evaluate_glare_film(t.data_ptr(), w, h, overlay_ptr=dev_overlay.data_ptr(), **SETTINGS)) == bits(res)
    np.testing.assert_array_equal(dev_overlay.cpu().numpy().view(np.uint32), overlay)


def test_unaligned_film_takes_the_scalar_path(device):
    kind, w, h, patches = CASES["67x45"]
    film = make_film(w, h, patches)
    device.set_camera(camera(kind))
    t = torch.from_numpy(film).to("cuda:0")
    shifted = torch.empty(w * h * 3 + 1, dtype=torch.float32, device="cuda:0")[1:]
    shifted.copy_(t.reshape(-1))
    assert t.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    mark = np.full((h, w), MARK, np.uint32)
    a, oa = device.evaluate_glare_film(t.data_ptr(), w, h, overlay=mark, **SETTINGS)
    b, ob = device.evaluate_glare_film(shifted.data_ptr(), w, h, overlay=mark, **SETTINGS)
    assert bits(a) == bits(b) and a["num_pixels"] == 8
    np.testing.assert_array_equal(oa, ob)


def test_no_source_and_given_illuminance(device):
    kind, w, h, patches = CASES["fish96x64-upper"]
    device.set_camera(camera(kind))
    grey = make_film(w, h, [])
    t = torch.from_numpy(grey).to("cuda:0")
    res, overlay = device.evaluate_glare_film(t.data_ptr(), w, h, overlay=np.full((h, w), MARK, np.uint32), **SETTINGS)
    want, tol = glare64(kind, grey, SETTINGS["lum_avg"], SETTINGS["lum_mul"])
    assert (res["num_pixels"], res["avg_lum"], res["avg_omega"]) == (0, 0.0, 0.0) and (overlay == MARK).all()
    assert abs(res["vertical_illuminance"] - want["vertical_illuminance"]) <= tol["vertical_illuminance"]
    assert abs(res["dgp"] - (5.87e-5 * want["vertical_illuminance"] + 0.16)) <= tol["dgp"]
    # a given vertical illuminance is returned as it is, and the DGP uses it
    film = make_film(w, h, patches)
    t = torch.from_numpy(film).to("cuda:0")
    res = device.evaluate_glare_film(t.data_ptr(), w, h, vertical_illuminance=1234.5, **SETTINGS)
    want, tol = glare64(kind, film, SETTINGS["lum_avg"], SETTINGS["lum_mul"], ev_given=1234.5)
    assert res["vertical_illuminance"] == 1234.5 and res["num_pixels"] == 24
    assert abs(res["dgp"] - want["dgp"]) <= tol["dgp"], (res, want, tol)


def test_before_the_first_render_and_bad_arguments():
    dev = ignis_amd.Device(0)
    try:
        L = _native.lib()
        gs = _native.GlareSettings(1.0, 8.0, 0.25, 5.0, -1.0)
        out = _native.GlareOutput(7, 7, 7, 7, 7)
        px = np.full(16, MARK, np.uint32)
        assert L.igx_evaluate_glare(dev._h, None, C.byref(gs), C.c_void_p(px.ctypes.data), 16, C.byref(out)) == 0
        assert [getattr(out, k) for k, _ in _native.GlareOutput._fields_] == [0] * 5 and (px == MARK).all()
        assert dev.evaluate_glare() is None
        assert L.igx_evaluate_glare(dev._h, b"Bogus", C.byref(gs), None, 16, C.byref(out)) == 1
        assert b"unknown aov" in L.igx_last_error(dev._h)
    finally:
        dev.close()


# ---- through the renderer: a fishlens camera that sees only a constant environment
E = [0.5, 0.25, 0.125]
Y_E = 0.2126729 * E[0] + 0.7151522 * E[1] + 0.0721750 * E[2]
W, H = 64, 64


def env_only_scene():
    """flat_scene with the environment as the only light, seen through a
    fishlens camera turned away from the ground plane (half a turn about y) and
    far enough from it that no direction of the film, the corners at 127
    degrees off the axis included, reaches the plane."""
    sc = copy.deepcopy(flat_scene([dict(ENV_LIGHT, radiance=E)]))
    sc["film"] = {"size": [W, H]}
    sc["camera"] = {"type": "fishlens", "near_clip": 0.01, "far_clip": 100, "transform": [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, -3]}
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


def test_rendered_constant_environment(runtime):
    fb = runtime.getFramebufferForHost()
    np.testing.assert_array_equal(fb, np.broadcast_to(np.float32(2) * np.array(E, np.float32), (H, W, 3)))
    info = runtime.imageinfo()
    res = runtime.evaluateGlare(lum_max=info["soft_max"], lum_avg=info["avg"], lum_mul=5.0)
    # known answer: E_v = 179 Y_E sum |cos| omega, no source
    omega, cos = omega64(FISHLENS, W, H)
    ev = 179 * Y_E * float((cos * omega).sum())
    bound = B * 179 * Y_E * float(cos.sum()) + 1e-5 * ev
    print("E_v", res["vertical_illuminance"], "float64", ev, "bound", bound)
    assert abs(res["vertical_illuminance"] - ev) <= bound
    assert res["num_pixels"] == 0 and abs(res["dgp"] - (5.87e-5 * ev + 0.16)) <= 5.87e-5 * bound + 1e-6
    # the AOV route is the film route with the handle's film and scale / iterations, bit for bit
    settings = dict(lum_max=info["soft_max"], lum_avg=info["avg"], lum_mul=0.5)  # threshold below the film: all source
    mark = np.full((H, W), MARK, np.uint32)
    a, oa = runtime.evaluateGlare(overlay=mark, **settings)
    ptr, count = runtime.device.framebuffer_device_ptr()
    assert count == W * H * 3
    b, ob = runtime.device.evaluate_glare_film(ptr, W, H, scale=1 / 2, overlay=mark, **settings)
    assert bits(a) == bits(b) and a["num_pixels"] == W * H
    np.testing.assert_array_equal(oa, ob)
    assert (oa != MARK).all()
    with pytest.raises(ignis_amd.IgxError, match="unknown aov"):
        runtime.evaluateGlare("Bogus")
    with pytest.raises(ignis_amd.IgxError, match="size mismatch"):
        gs = _native.GlareSettings(1.0, 1.0, 1.0, 5.0, -1.0)
        out = _native.GlareOutput()
        runtime.device._check(_native.lib().igx_evaluate_glare(runtime.device._h, None, C.byref(gs), None, W * H - 1, C.byref(out)))


def test_igcli_glare_line(runtime, tmp_path):
    scene = tmp_path / "env.json"
    scene.write_text(json.dumps(env_only_scene()))
    ppm = tmp_path / "out.ppm"
    out = subprocess.run([os.path.join(PKG, "igcli"), str(scene), "--spp", "8", "--spi", "4", "--glare", "--glare-mul", "0.5",
                          "--ppm", str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("glare: ")]
    assert len(lines) == 1, out.stdout
    words = lines[0].split()
    assert words[1::2] == ["dgp", "ev", "avg_lum", "omega", "pixels"]
    cli = dict(zip(words[1::2], words[2::2]))
    info = runtime.imageinfo()
    res, overlay = runtime.evaluateGlare(lum_max=info["soft_max"], lum_avg=info["avg"], lum_mul=0.5, overlay=runtime.tonemap())
    for key, name in (("dgp", "dgp"), ("ev", "vertical_illuminance"), ("avg_lum", "avg_lum"), ("omega", "avg_omega")):
        assert np.float32(cli[key]) == np.float32(res[name]), (key, cli[key], res[name])  # %.9g names one float32
    assert int(cli["pixels"]) == res["num_pixels"] == W * H
    # the heat map lies over the tonemapped image
    data = ppm.read_bytes()
    head = b"P6\n%d %d\n255\n" % (W, H)
    p = int(overlay[0, 0])
    assert data.startswith(head) and data[len(head):len(head) + 3] == bytes([(p >> 16) & 255, (p >> 8) & 255, p & 255])


def test_facade_evaluates_glare(tmp_path):
    exe = str(tmp_path / "glare_facade")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "host"),
                    os.path.join(ROOT, "tests", "native", "glare_facade.cpp"), "-o", exe, "-L", PKG, "-ligx", f"-Wl,-rpath,{PKG}",
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
