"""The cases of the per-ray BSDF tests (tests/test_bsdf_ref.py on the oracle,
tests/test_bsdf_gpu.py on the device): one rotated rectangle, one material, a
list of rays that hit it from both sides, and the three observables of each
material as tests/bsdf_ref.py expects them."""
import ctypes as C
import json
import math
import os

import numpy as np

import bsdf_ref as B
import daylight_ref as R
import ignis_amd
import image_ref as IR
from oracle import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 2048
N_DRAWS = 12  # the longest path: lobe choice, two samples of a failed lobe, two of the other, roulette; NEE adds two
ROTATE = [25, -40, 10]  # the normal lies on no axis
# the point light of observable (a): (along the normal, along the rectangle's x), twice above the face and once below
LIGHT_PLACES = {"near": (0.7, 0.4), "far": (3.0, -1.1), "below": (-1.2, 0.6)}
LIGHT_INTENSITY = [3.0, 2.0, 1.5]
CAMERA_FILM, CAMERA_HEIGHT = 32, 0.25  # observable (b) on the device: two films of 32 x 32 rays


def _named(path):
    with open(os.path.join(ROOT, "scenes", path)) as f:
        return {b["name"]: b for b in json.load(f)["bsdfs"]}


_MATERIALS, _PRINCIPLED = _named("materials.json"), _named("principled.json")
BSDFS = {"lambert": {"type": "diffuse", "reflectance": [0.6, 0.4, 0.2]}}
BSDFS.update({k: _MATERIALS[k] for k in ("rough_copper", "aniso_alu", "beckmann_silver", "plastic", "rough_plastic", "oren_nayar")})
BSDFS.update({k: v for k, v in _PRINCIPLED.items() if v["type"] == "principled"})
BSDFS["p_rough0"] = {"type": "principled", "base_color": [0.8, 0.5, 0.3], "roughness": 0}  # reaches max(1e-3, .)
NON_DELTA = list(BSDFS)
assert len(NON_DELTA) == 1 + 6 + 9 + 1
BSDFS.update({k: _MATERIALS[k] for k in ("mirror", "gold", "glass")})
BSDFS["thin_glass"] = {"type": "dielectric", "int_ior": 1.5, "thin": True}
DELTA = ["mirror", "gold", "glass", "thin_glass"]


def write_gradient_map(path):
    """16 x 8 float texels; the three channels are different smooth gradients."""
    ys, xs = np.mgrid[0:8, 0:16]
    img = np.stack([0.2 + 0.8 * xs / 15, 0.3 + 0.7 * ys / 7, 1.0 - 0.6 * (xs + 2 * ys) / 29], axis=2).astype(np.float32)
    ignis_amd.write_exr(path, img)
    return str(path)


def scene(name, observable, env_map=None, light="near", camera_side=0):
    sd = {"technique": {"type": "path", "max_depth": 2, "min_depth": 2, "light_selector": "uniform"},
          "camera": {"type": "perspective", "fov": 40, "near_clip": 0.01, "far_clip": 100,
                     "transform": {"lookat": {"origin": [0, 0, 5], "direction": [0, 0, -1], "up": [0, 1, 0]}}},
          "film": {"size": [8, 8]},
          "bsdfs": [{**BSDFS[name], "name": "m"}],
          "shapes": [{"type": "rectangle", "name": "r", "width": 4, "height": 4}],
          "entities": [{"name": "e", "shape": "r", "bsdf": "m", "transform": {"rotate": ROTATE}}]}
    if observable == "eval":
        # placed from the entity's own matrix, so build the scene once without a light to read it
        probe = ignis_amd.Scene.from_string({**sd, "lights": [{"type": "env", "name": "l", "radiance": [1, 1, 1]}]})
        m = np.array(probe.desc.entities[0].to_global[:], np.float64).reshape(3, 4)
        h, x = LIGHT_PLACES[light]
        pos = m[:, 3] + h * face_normal(probe.desc) + x * m[:, 0]
        sd["lights"] = [{"type": "point", "name": "l", "position": [float(v) for v in pos], "intensity": LIGHT_INTENSITY}]
    elif observable == "mis":
        sd["technique"]["aov_mis"] = True
        sd["lights"] = [{"type": "env", "name": "l", "radiance": [1, 1, 1]}]
        if camera_side:
            # a wide camera close over the face's centre (under it: the back side), for the
            # device, whose ray-list mode writes no AOVs: |cos| to the normal from 1 down to 0.19
            probe = ignis_amd.Scene.from_string(sd)
            m = np.array(probe.desc.entities[0].to_global[:], np.float64).reshape(3, 4)
            n = face_normal(probe.desc) * camera_side
            sd["camera"] = {"type": "perspective", "fov": 150, "near_clip": 0.01, "far_clip": 100,
                            "transform": {"lookat": {"origin": [float(v) for v in m[:, 3] + CAMERA_HEIGHT * n],
                                                     "direction": [float(-v) for v in n], "up": [float(v) for v in m[:, 0]]}}}
            sd["film"] = {"size": [CAMERA_FILM, CAMERA_FILM]}
    else:
        sd["technique"]["nee"] = False
        sd["textures"] = [{"type": "image", "name": "map", "filename": env_map, "filter_type": "bilinear"}]
        sd["lights"] = [{"type": "env", "name": "l", "radiance": "map"}]
    return ignis_amd.Scene.from_string(sd)


def face_normal(desc):
    """The rectangle's world normal in float64: the entity's normal matrix on the mesh's normal."""
    e, m = desc.entities[0], desc.meshes[0]
    n = np.ctypeslib.as_array(m.normals, (m.num_vertices, 3)).astype(np.float64)
    assert (n == n[0]).all()
    w = np.array(e.normal[:], np.float64).reshape(3, 3) @ n[0]
    return w / np.linalg.norm(w)


def make_rays(desc, seed=7, n=N_RAYS):
    """(n, 8) float32 rays: hit points uniform over the inner 3 x 3 of the 4 x 4
    face, |cos| to the normal stratified over [0.02, 1], any azimuth, every other
    one from the back; origins one unit from the hit point."""
    rng = np.random.default_rng(seed)
    m = np.array(desc.entities[0].to_global[:], np.float64).reshape(3, 4)
    nrm = face_normal(desc)
    local = np.c_[rng.uniform(-1.5, 1.5, (n, 2)), np.zeros(n), np.ones(n)]
    p = local @ m.T
    cos = 0.02 + 0.98 * (rng.permutation(n) + rng.random(n)) / n
    sin, phi = np.sqrt(1 - cos * cos), rng.uniform(0, 2 * math.pi, n)
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    out = B.Frame(nrm).to_world(B.vec(sin * np.cos(phi), sin * np.sin(phi), side * cos))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = p + out, -out, 0, 100
    return rays


_draws = {}


def draws(n=N_RAYS):
    """The random numbers of ray i's path: seeded create_random_seed(sample 0,
    iteration 0, frame 0, i, 0, seed 0), counter 1 (ray-list mode draws none for the ray itself)."""
    if n not in _draws:
        lib = O.lib()
        t = np.zeros((n, N_DRAWS), np.float32)
        for i in range(n):
            s, c = lib.oracle_random_seed(0, 0, 0, i, 0, 0), C.c_uint32(1)
            for k in range(N_DRAWS):
                t[i, k] = lib.oracle_next_f32(s, C.byref(c))
        _draws[n] = t
    return _draws[n]


def replay(sc, rays, mutant=None, table=None):
    d = sc.desc
    m = np.array(d.entities[0].to_global[:], np.float64).reshape(3, 4)
    table = draws(len(rays)) if table is None else table
    return B.Replay(d.materials[d.entities[0].material], face_normal(d), m[:, 3], rays, table, mutant)


_camera_draws = {}


def camera_rays(desc):
    """The camera paths of a film rendered with one sample: float64 rays of the
    camera model (tests/daylight_ref.py) at every pixel's replayed jitter, the
    random numbers that follow the jitter, and which pixels belong to the case:
    their ray meets the face well inside its border."""
    w = h = CAMERA_FILM
    if not _camera_draws:
        lib = O.lib()
        t = np.zeros((h * w, 2 + N_DRAWS), np.float32)
        for i in range(h * w):
            s, c = lib.oracle_random_seed(0, 0, 0, i % w, i // w, 0), C.c_uint32(1)
            for k in range(2 + N_DRAWS):
                t[i, k] = lib.oracle_next_f32(s, C.byref(c))
        _camera_draws[0] = t.astype(np.float64)
    t = _camera_draws[0]
    cam = desc.camera
    assert cam.type == 0 and cam.aperture_radius == 0  # a pinhole
    model = R.Camera("perspective", cam.eye[:], cam.dir[:], cam.up[:], w, h, fov=cam.fov, vertical_fov=bool(cam.vertical_fov))
    ys, xs = np.mgrid[0:h, 0:w]
    nx = 2 * (xs.ravel() + t[:, 0]) / w - 1
    ny = 1 - 2 * (ys.ravel() + t[:, 1]) / h
    org, d = model.rays(nx, ny)
    rays = np.c_[org, d, np.full(len(d), cam.near_clip), np.full(len(d), cam.far_clip)]
    e = desc.entities[0]
    m = np.array(e.to_global[:], np.float64).reshape(3, 4)
    n = face_normal(desc)
    dist = ((m[:, 3] - org) @ n) / (d @ n)
    local = np.c_[org + d * dist[:, None], np.ones(len(d))] @ np.array(e.to_local[:], np.float64).reshape(3, 4).T
    keep = (dist > 0) & (np.abs(local[:, :2]).max(axis=1) < 1.9)
    return rays, t[:, 2:], keep


def expected(sc, observable, rays, mutant=None, table=None):
    """{observable name: (want (n, 3), stable (n,), ill (n,))} of one scene in float64
    (bsdf_ref.Trace: rays left out, rays with an allowance of their own)."""
    r = replay(sc, rays, mutant, table)
    d = sc.desc
    if observable == "eval":
        L = d.lights[0]
        want = {"eval": r.eval_point_light(L.origin[:], L.radiance[:])}
    elif observable == "mis":
        nee, direct = r.env_nee(min_depth=d.technique.min_depth)
        want = {"nee_weight": nee, "direct_weight": direct}
    else:
        direction, weight, valid, _, _ = r.sampled(min_depth=d.technique.min_depth)
        safe = np.where(valid[:, None], direction, [0.0, 0.0, 1.0])
        want = {"sampled": np.where(valid[:, None], weight * IR.env_radiance(d, safe)[0], 0.0)}
    return {k: (v, r.stable, r.ill & (k in ("direct_weight", "sampled"))) for k, v in want.items()}


def list_params(rays):
    p = ignis_amd.RenderParams()
    p.spi, p.num_rays = 1, rays.shape[0]
    p.rays = rays.ctypes.data_as(C.POINTER(C.c_float))
    return p


def render_oracle(sc, observable, rays):
    n = len(rays)
    orc = O.OracleScene(sc)
    aov = {"Direct Weights": np.zeros(n * 3, np.float32), "NEE Weights": np.zeros(n * 3, np.float32)} if observable == "mis" else None
    fb, _ = orc.render(n, 1, 1, threads=4, rays=rays, aov=aov)
    orc.close()
    return _films(observable, fb, aov, n)


def render_device(device, sc, observable, rays, options=None):
    n = len(rays)
    device.upload(sc)
    for k, v in (options or {}).items():
        device.set_option(k, v)
    device.clear()
    device.render(list_params(rays))
    fb = device.framebuffer(n * 3)[0].copy()
    aov = {k: device.framebuffer(n * 3, k)[0].copy() for k in ("Direct Weights", "NEE Weights")} if observable == "mis" else None
    return _films(observable, fb, aov, n)


def camera_mis(render, name):
    """Observable (b) through the two cameras: (got, want) over the rays of both
    that belong to the case; render(scene) -> (film, {AOV name: film}) of one
    sample per pixel."""
    got, want = {}, {}
    for side in (1, -1):
        sc = scene(name, "mis", camera_side=side)
        rays, table, keep = camera_rays(sc.desc)
        fb, aov = render(sc)
        g = _films("mis", fb, aov, len(rays))
        w = expected(sc, "mis", rays[keep], table=table[keep])
        for k in w:
            got[k] = np.concatenate([got[k], g[k][keep]]) if k in got else g[k][keep]
            want[k] = tuple(np.concatenate([a, b]) for a, b in zip(want[k], w[k])) if k in want else w[k]
    return got, want


def camera_render_oracle(sc):
    n = CAMERA_FILM * CAMERA_FILM
    orc = O.OracleScene(sc)
    aov = {"Direct Weights": np.zeros(n * 3, np.float32), "NEE Weights": np.zeros(n * 3, np.float32)}
    fb, _ = orc.render(CAMERA_FILM, CAMERA_FILM, 1, threads=4, aov=aov)
    orc.close()
    return fb, aov


def camera_render_device(device):
    def render(sc):
        n = CAMERA_FILM * CAMERA_FILM
        device.upload(sc)
        device.clear()
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi = CAMERA_FILM, CAMERA_FILM, 1
        device.render(p)
        return device.framebuffer(n * 3)[0].copy(), {k: device.framebuffer(n * 3, k)[0].copy() for k in ("Direct Weights", "NEE Weights")}
    return render


def _films(observable, fb, aov, n):
    fb = fb.reshape(n, 3).astype(np.float64)
    if observable == "eval":
        return {"eval": fb}
    if observable == "mis":
        out = {"nee_weight": aov["NEE Weights"].reshape(n, 3).astype(np.float64),
               "direct_weight": aov["Direct Weights"].reshape(n, 3).astype(np.float64)}
        # the film is the sum of its two parts
        np.testing.assert_allclose(fb, out["nee_weight"] + out["direct_weight"], rtol=1e-6, atol=1e-7)
        return out
    return {"sampled": fb}


def runs(name):
    """The (observable, light) renders of a material."""
    if name in DELTA:
        return [("sampled", None)]
    return [("eval", k) for k in LIGHT_PLACES] + [("mis", None), ("sampled", None)]


_cache = {}


def case(name, observable, light, env_map, mutant=None):
    """(scene, rays, {observable name: (want, stable)}) of one render, computed once."""
    key = (name, observable, light, mutant)
    if key not in _cache:
        sc = scene(name, observable, env_map, light or "near")
        rays = make_rays(sc.desc)
        _cache[key] = (sc, rays, expected(sc, observable, rays, mutant))
    return _cache[key]


def judge(name, got, want, measured):
    """[(observable and ray class, deviation, passes)] of one render: bsdf_ref.check on
    the stable rays, the ill-conditioned ones (bsdf_ref.Microfacet.sample) apart, each
    against 4x what was measured for that observable (or for that material's, where
    `measured` has an entry of its own)."""
    out = []
    for key, (w, stable, ill) in want.items():
        for cls, mask in ((key, stable & ~ill), (key + "_ill", stable & ill)):
            if mask.any():
                ok, dev = B.check(got[key], w, mask, 4 * measured.get((name, cls), measured[cls]))
                out.append((cls, dev, ok))
    return out


# The largest deviation (bsdf_ref.deviation: relative to max(|want|, 1e-3 of the case's 90th
# percentile)) of each observable from tests/bsdf_ref.py over all materials, measured on an
# MI355X (float32 with -fapprox-func) and, for the oracle twin, on the CPU (float32, libm);
# DESIGN.md section 5, "Per-ray BSDF reference".  The tests allow 4x.  "_ill" is the class of
# ill-conditioned rays (bsdf_ref.Microfacet.sample).  A material whose own largest deviation
# is several times that of all others has an entry of its own, so that it does not widen the
# allowance of the rest:
#   p_glass (a): the light's direction is far off the narrow refraction lobe, the film is 1e-6;
#   p_sheen, p_tint (c): a sample grazing the face (|cos| 5e-5) and one of alpha_v 0.0025;
#   p_aniso (b, oracle's rays): a grazing sample; p_rough0 (alpha 1e-3): D changes by its own
#   size over 1e-3 rad, so where the sampler is ill-conditioned the weight is not observable.
MEASURED_DEVICE = {"eval": 9.3e-5, ("p_glass", "eval"): 2.4e-3,
                   "nee_weight": 7.7e-5, ("p_glass", "nee_weight"): 1.2e-3,
                   "direct_weight": 5.7e-3,
                   "direct_weight_ill": 1.7e-3, ("p_rough0", "direct_weight_ill"): 1.6e-2,
                   "sampled": 3.2e-3, ("p_sheen", "sampled"): 1.6e-2, ("p_tint", "sampled"): 9.7e-3,
                   "sampled_ill": 1.92e-2, ("p_rough0", "sampled_ill"): 0.60}
MEASURED_ORACLE = {"eval": 9.2e-5, ("p_glass", "eval"): 2.4e-3,
                   "nee_weight": 3.2e-4, ("p_glass", "nee_weight"): 2.5e-3,
                   "direct_weight": 6.1e-3, ("p_aniso", "direct_weight"): 1.8e-2,
                   "direct_weight_ill": 9.5e-2, ("p_rough0", "direct_weight_ill"): 0.23,
                   "sampled": 3.2e-3, ("p_sheen", "sampled"): 1.6e-2, ("p_tint", "sampled"): 9.7e-3,
                   "sampled_ill": 1.92e-2, ("p_rough0", "sampled_ill"): 0.60}
