"""HIP device vs. the oracle (runs on the MI355X box).

Parity contract: hit level -- (entity, primitive) identical on
>= 99.99 % of rays (edge/coplanar ties recognised by equal t) and t within
1e-5 relative on 99.9 % of rays, 1e-4 at worst; image level -- relMSE
(RunEvaluations RelSE, 99th-percentile clamp) <= 1e-3 for primitives and
<= 5e-3 for diamond, >= 99 % of pixels within 1e-3 (1e-2 for diamond) relative;
analytic known answers within 5 standard errors.  The GPU and the oracle agree
per path up to float rounding (FMA contraction, libm vs ocml transcendentals),
which flips rare discrete decisions (Russian roulette, Fresnel choice) and so
gives sparse per-pixel outliers -- hence statistical image tolerances.
"""
import json
import math
import os

import numpy as np
import pytest

import ignis_amd
from oracle import oracle_py as O
from conftest import DIRECTIONAL_LIGHT, ENV_LIGHT, POINT_LIGHT, SPOT_LIGHT, SUN_LIGHT, emitter_scene, flat_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def rel_mse(img, ref):
    """RunEvaluations' error_image (scripts/RunEvaluations.py:80-87, tests/evalref.py):
    RelSE where ref != 0, AbsSE where ref == 0, mean clamped at the 99th percentile."""
    import evalref

    return evalref.error_image(np.asarray(img, np.float32), np.asarray(ref, np.float32))[0]


def render_gpu(device, scene, w, h, spi, iteration=0, seed=0, tile=None, capacity=0):
    device.upload(scene)
    device.set_option("capacity", capacity)
    device.clear()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration, p.seed = w, h, spi, iteration, seed
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    device.render(p)
    fb, it = device.framebuffer(w * h * 3)
    return fb


def camera_rays(scene, w, h, jitter=0.5):
    """Pixel-centre camera rays of the scene camera (camera/perspective.art:29-42)."""
    d = scene.desc
    c = d.camera
    eye, dr, up = np.array(c.eye[:]), np.array(c.dir[:]), np.array(c.up[:])
    right = np.cross(dr, up)
    right /= np.linalg.norm(right)
    sx = math.tan(c.fov / 2)
    sy = sx / (w / h)
    ys, xs = np.mgrid[0:h, 0:w]
    nx = 2 * (xs + jitter) / w - 1
    ny = 1 - 2 * (ys + jitter) / h
    v = sx * nx[..., None] * right + sy * ny[..., None] * up + dr
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    n = w * h
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = eye
    rays[:, 3:6] = v.reshape(-1, 3)
    rays[:, 6] = c.near_clip
    rays[:, 7] = c.far_clip
    return rays


def random_rays(scene, n, seed=1):
    d = scene.desc
    lo = np.array(d.scene_bbox_min[:]) - 0.1
    hi = np.array(d.scene_bbox_max[:]) + 0.1
    rng = np.random.default_rng(seed)
    org = rng.uniform(lo, hi, size=(n, 3))
    dr = rng.normal(size=(n, 3))
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = org
    rays[:, 3:6] = dr
    rays[:, 6] = 1e-3
    rays[:, 7] = 3.4e38
    return rays


def assert_hit_parity(gpu, orc, rays, flags):
    ep_g, tuv_g = gpu
    ep_o, tuv_o = orc
    same = np.all(ep_g == ep_o, axis=1)
    # A ray through a shared edge or onto coincident surfaces is accepted by
    # both primitives (MT uses a -eps barycentric tolerance); the reference
    # then keeps the one its BVH visits last, so the
    # ids of such ties depend on BVH topology.  Ties are recognised by equal t.
    both = (ep_g[:, 0] >= 0) & (ep_o[:, 0] >= 0)
    tie = ~same & both & (np.abs(tuv_g[:, 0] - tuv_o[:, 0]) <= 1e-5 * np.abs(tuv_o[:, 0]))
    assert same.mean() >= 0.999, same.mean()
    assert (same | tie).mean() >= 0.9999, ((same | tie).mean(), np.flatnonzero(~(same | tie))[:10])
    hit = same & (ep_o[:, 0] >= 0)
    assert hit.sum() > 0
    rel = np.abs(tuv_g[hit, 0] - tuv_o[hit, 0]) / np.maximum(np.abs(tuv_o[hit, 0]), 1e-6)
    # FMA contraction on the GPU vs separate mul/add in the oracle: grazing
    # rays (small MT determinant) amplify the last-bit differences
    assert np.percentile(rel, 99.9) <= 1e-5, np.percentile(rel, 99.9)
    assert rel.max() <= 1e-4, rel.max()
    np.testing.assert_allclose(tuv_g[hit, 1:], tuv_o[hit, 1:], atol=1e-3)


@pytest.mark.parametrize("name", ["diamond_scene.json", "primitives.json", "s_deep.json", "s_soup_1m.json"])
def test_hit_parity_camera_and_random(device, root, name):
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    device.upload(sc)
    orc = O.OracleScene(sc)
    for rays, flags in [(camera_rays(sc, 320, 320, jitter=0.37), 0x1), (random_rays(sc, 100000), 0x4)]:
        assert_hit_parity(device.trace_hits(rays, flags), orc.trace_hits(rays, flags), rays, flags)


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
def test_bvh_width_invariance(device, root, name):
    """BVH2 and the collapsed 4-wide BVH (each with and without stack spill:
    diamond's BVH2 fits the LDS stack, S-deep's does not) return the same closest
    hits and images bit for bit: the tie rule makes hits independent of topology
    and traversal order."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    rays = np.concatenate([camera_rays(sc, 200, 200, jitter=0.41), random_rays(sc, 50000, seed=5)])
    res, imgs = [], []
    try:
        for width in (2, 4):
            device.set_option("bvh_width", width)
            device.upload(sc)
            assert device.stats()["bvh_width"] == width
            res.append(device.trace_hits(rays, 0x1))
            imgs.append(render_gpu(device, sc, 96, 96, 4))
    finally:
        device.set_option("bvh_width", 0)
    (ep2, tuv2), (ep4, tuv4) = res
    np.testing.assert_array_equal(ep2, ep4)
    np.testing.assert_array_equal(tuv2, tuv4)
    np.testing.assert_array_equal(imgs[0], imgs[1])


def test_quantised_nodes_match(device, root):
    """Quantised 4-wide nodes (the soups' default, bvh_quantize) against the
    128-B nodes on soup-1M: conservative boxes visit a superset of the
    triangles, so closest hits agree (tie rule); a triangle hit inside the
    Moeller-Trumbore tolerance but outside an exact padded box can appear in
    rare rays, as with any change of the tree (padded boxes)."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "s_soup_1m.json"))
    rays = np.concatenate([camera_rays(sc, 200, 200, jitter=0.29), random_rays(sc, 100000, seed=9)])
    res, imgs = [], []
    try:
        for q in (0, 1):
            device.set_option("bvh_quantize", q)
            device.upload(sc)
            st = device.stats()
            assert st["node_bytes"] == (64 if q else 128)  # quantised or float 4-wide nodes
            res.append(device.trace_hits(rays, 0x1))
            imgs.append(render_gpu(device, sc, 128, 128, 4))
    finally:
        device.set_option("bvh_quantize", -1)
    (e0, t0), (e1, t1) = res
    same = np.all(e0 == e1, axis=1) & (t0[:, 0] == t1[:, 0])
    assert same.mean() >= 0.99999, same.mean()
    assert rel_mse(imgs[1], imgs[0]) <= 1e-6


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
def test_spatial_split_invariance(device, root, name):
    """BLAS built with spatial splits (SBVH: triangles referenced from several
    leaves) and without return the same closest hits and images bit for bit."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    rays = np.concatenate([camera_rays(sc, 200, 200, jitter=0.29), random_rays(sc, 50000, seed=11)])
    res, imgs = [], []
    try:
        for split in (0, 1):
            device.set_option("spatial_splits", split)
            device.upload(sc)
            res.append(device.trace_hits(rays, 0x1))
            imgs.append(render_gpu(device, sc, 96, 96, 4))
    finally:
        device.set_option("spatial_splits", 0)
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
def test_tail_threshold_invariance(device, root, name):
    """Paths finished by the tail kernel and by the wavefront kernels are
    bit-identical: no tail, the whole chunk in the tail from the first bounce,
    and the automatic threshold render the same image with the same ray counts."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        for tail in (0, 1 << 30, 3000, -1):
            device.set_option("tail_threshold", tail)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, 120, 90, 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("tail_threshold", -1)
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
@pytest.mark.parametrize("tile", [None, (64, 1, 3)])
def test_fused_generate_invariance(device, root, name, tile):
    """Camera paths built by bounce 0 of k_extend (fuse_generate, default) and
    by the separate k_generate pass give the same image and ray counts, bit
    for bit, also with tile padding (dead slots) in the chunk."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        device.set_option("tail_threshold", 0)  # force the wavefront path, where the fusion applies
        device.set_option("split", 0)  # and the fused schedule (S-deep's tables are global)
        for fuse in (0, 1):
            device.set_option("fuse_generate", fuse)
            device.reset_stats()
            device.clear()
            device.upload(sc)
            p = ignis_amd.RenderParams()
            p.width, p.height, p.spi = 150, 100, 4
            if tile:
                p.tile_size, p.tile_offset, p.tile_stride = tile
            device.render_iterations(p, 2)
            imgs.append(device.framebuffer(150 * 100 * 3)[0])
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("fuse_generate", 1)
        device.set_option("split", -1)
        device.set_option("tail_threshold", -1)
    np.testing.assert_array_equal(imgs[0], imgs[1])
    assert counts[0] == counts[1]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("tile,capacity", [(None, 0), ((64, 1, 3), 0), (None, 20000)])
def test_render_iterations_equals_single_calls(device, diamond_path, tile, capacity):
    """igx_render_iterations (iterations batched into one wavefront when they fit the
    capacity; pixel chunks otherwise) == the same iterations one igx_render call each,
    bit for bit, with and without tile sharding."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, spi, n = 160, 120, 2, 5
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.iteration = w, h, spi, 3
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    device.upload(sc)
    device.set_option("capacity", capacity)
    try:
        device.clear()
        device.reset_stats()
        for it in range(n):
            p.iteration = 3 + it
            device.render(p)
        a, ia = device.framebuffer(w * h * 3)
        sa = device.stats()
        device.clear()
        device.reset_stats()
        p.iteration = 3
        device.render_iterations(p, n)
        b, ib = device.framebuffer(w * h * 3)
        sb = device.stats()
    finally:
        device.set_option("capacity", 0)
    assert ia == ib == n
    np.testing.assert_array_equal(a, b)
    assert a.sum() > 0
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "iterations"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


@pytest.mark.parametrize("split", [0, 1])
def test_one_stream_slot_matches_two(diamond_path, split):
    """stream_slots 1 (every chunk in the same slot: each waits for the one
    before, bench.py's setting at N > 1) renders the frame of stream_slots 2
    bit for bit over many chunks, gives the second slot's memory back, and the
    per-path hit record is only allocated for the split schedule (a fresh
    handle, so no slot is left over from a larger earlier render)."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = 160, 120, 2
    d = ignis_amd.Device(0)
    try:
        d.upload(sc)
        d.set_option("split", split)
        d.set_option("capacity", 20000)  # 10000 pixels x spi 2 per chunk: 4 chunks per iteration
        imgs, mem = [], []
        for slots in (2, 1, 2):
            d.set_option("stream_slots", slots)
            d.clear()
            d.render_iterations(p, 3)
            imgs.append(d.framebuffer(160 * 120 * 3)[0])
            mem.append(d.stats()["slot_bytes"])
    finally:
        d.close()
    np.testing.assert_array_equal(imgs[0], imgs[1])
    np.testing.assert_array_equal(imgs[0], imgs[2])
    assert imgs[0].sum() > 0
    assert mem[1] * 2 == mem[0] == mem[2], mem
    cap = 20000
    # two path buffers (with the class-C region of path_classes 4 on the fused
    # schedule: twice the records), shadow ray, hit record (split schedule)
    per_rec = 2 * 56 * (1 if split else 2) + 48 + (20 if split else 0)
    shard_cap = -(-cap // (64 * 64)) * 64
    assert mem[1] == shard_cap * 64 * per_rec + cap * 16, (mem[1], split)


def test_bench_frame_equals_single_iterations(device, diamond_path):
    """At the bench's full size (diamond 1000x1000, 32 iterations of spi 8 =
    256 spp) the batched frame -- 128 M-path chunks, 16 iterations each -- is
    bit for bit the frame of 32 single-iteration renders, with the same ray
    counts: chunking, sharded streams and the tail are exact at scale."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h = sc.film_size
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, 8
    device.upload(sc)
    device.clear()
    device.reset_stats()
    p.iteration = 0
    device.render_iterations(p, 32)
    a, ia = device.framebuffer(w * h * 3)
    sa = device.stats()
    device.clear()
    device.reset_stats()
    for it in range(32):
        p.iteration = it
        device.render(p)
    b, ib = device.framebuffer(w * h * 3)
    sb = device.stats()
    assert ia == ib == 32
    np.testing.assert_array_equal(a, b)
    for k in ("camera_rays", "bounce_rays", "shadow_rays"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert sa["camera_rays"] == w * h * 8 * 32


def test_shading_variant_invariance(device, diamond_path):
    """The basic-shading kernel variant (Lambert + dielectric only, chosen for the
    diamond) and the full one render the diamond bit for bit alike."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    imgs = []
    try:
        for full in (0, 1):
            device.set_option("full_shading", full)
            imgs.append(render_gpu(device, sc, 128, 128, 4))
    finally:
        device.set_option("full_shading", 0)
    np.testing.assert_array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("name", ["s_deep.json", "s_soup_1m.json"])
def test_treelet_invariance(device, root, name):
    """The LDS treelet of the hottest BVH nodes (global-table scenes: k_extend
    and the shadow kernels read nodes below tree_n from LDS) changes where a
    node is read from, never what is traced: images bit for bit equal and
    ray counts equal with the treelet off, automatic and at 32 nodes."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts, staged = [], [], []
    try:
        device.upload(sc)
        for treelet in (0, -1, 32):
            device.set_option("treelet", treelet)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, 112, 80, 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
            staged.append(list(st["treelet_nodes"]))
    finally:
        device.set_option("treelet", -1)
    assert staged[0] == [0, 0, 0, 0] and max(staged[1]) > 0 and max(staged[2]) <= 32, staged
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
def test_split_and_refill_invariance(device, root, name):
    """Fused k_extend, split k_trace + k_shade, and the persistent-lane (refill)
    trace and shadow kernels render the same image bit for bit, with the same ray
    counts, with global and (diamond) LDS-staged traversal tables."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        device.upload(sc)
        # global tables, then (diamond) LDS-staged tables with explicit split / refill
        # (lds_scene_max, split, refill, shadow_ifif): if-if stepping of the persistent-lane shadow kernel too
        runs = [(0, 0, 0, -1), (0, 1, 0, -1), (0, 1, 16, 0), (0, 1, 16, 1), (0, 0, 8, 1), (0, -1, -1, -1),
                (48 * 1024, 1, 16, -1), (48 * 1024, 0, 32, -1)]
        for lds, split, refill, ifif in runs:
            device.set_option("lds_scene_max", lds)
            device.set_option("split", split)
            device.set_option("refill", refill)
            device.set_option("shadow_ifif", ifif)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, 112, 80, 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("split", -1)
        device.set_option("refill", -1)
        device.set_option("shadow_ifif", -1)
        device.set_option("lds_scene_max", 48 * 1024)
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "s_deep.json"])
def test_path_class_invariance(device, root, name):
    """Surviving paths split into two stream classes (inside a dielectric or
    not, or after a specular event: front / back of each shard) or three
    (inside / heading for an enclosing entity's box / the rest: class C in its
    own region) render the same image bit for bit with the same ray counts as
    one class, on the fused and the split schedule (three classes fall back
    to two there), and through the tail kernel (tail threshold 0 / all)."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        device.upload(sc)
        for classes, split, tail in [(0, -1, -1), (1, -1, -1), (2, -1, -1), (1, 1, -1), (1, 0, 0), (1, -1, 1 << 30),
                                     (3, -1, -1), (4, 0, -1), (4, 0, 0), (4, 1, -1)]:
            device.set_option("path_classes", classes)
            device.set_option("split", split)
            device.set_option("tail_threshold", tail)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, 112, 80, 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("path_classes", 3)
        device.set_option("split", -1)
        device.set_option("tail_threshold", -1)
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "materials.json", "s_deep.json"])
def test_enclosing_shortcut_invariance(device, root, name):
    """Paths inside a closed convex dielectric apart from every other entity
    trace only its BLAS (trace_enclosed): the image and ray counts equal the
    full traversal's bit for bit, through the wavefront and the tail kernel."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        for enclosing, tail in [(0, -1), (1, -1), (1, 0), (1, 1 << 30)]:
            device.set_option("enclosing", enclosing)
            device.set_option("tail_threshold", tail)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, 112, 80, 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("enclosing", 1)
        device.set_option("tail_threshold", -1)
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "materials.json"])
def test_face_normal_table_invariance(device, root, name):
    """World-space face normals precomputed at upload (the host restates
    make_triangle in float with the device's operation order) and the per-face
    shading records (vertex normals and indices in one record, option
    face_shade) render the same image bit for bit as normals computed per hit
    from the index and normal tables."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs = []
    try:
        for fnt, fsh in ((0, 0), (1, 0), (0, 1), (1, 1)):
            device.set_option("face_normals", fnt)
            device.set_option("face_shade", fsh)
            device.upload(sc)
            imgs.append(render_gpu(device, sc, 160, 120, 4))
    finally:
        device.set_option("face_normals", 1)
        device.set_option("face_shade", 1)
        device.upload(sc)
    for img in imgs[1:]:
        np.testing.assert_array_equal(imgs[0], img)
    assert imgs[0].sum() > 0


AOV_CONFIGS = [{}, {"fuse_generate": 0}, {"concurrent_chunks": 0}, {"tail_threshold": 0}, {"tail_threshold": 1 << 30},
               {"split": 1}, {"lds_scene_max": 0, "split": 1, "refill": 1, "tail_pairs": 1, "tail_threshold": 0},
               {"lds_scene_max": 0, "split": 1, "refill": 1, "tail_pairs": 1}]


@pytest.mark.parametrize("name,plain", [("primitives_aov.json", "primitives.json"), ("diamond_scene_uniform.json", None)])
def test_mis_aovs(device, root, name, plain):
    """The path tracer's MIS AOVs (technique aov_mis, PathTechnique.cpp:16-27;
    the reference's own AOV scenes): "Direct Weights" collects emission hits
    and misses (pathtracer.art:128,158), "NEE Weights" the unoccluded shadow
    rays (:206).  The film is bit-identical to the same scene without the
    AOVs; the two AOVs sum to the film up to float rounding; every schedule
    (fused / generate pass / sequential chunks / tail kernels / split /
    persistent-lane global-table kernels with lane-pair tails) gives the same
    AOVs bit for bit; and they match the oracle's per-path split (RelSE as the
    film's parity bound).  An unknown AOV name is an error."""
    w, h, spi = 160, 120, 4
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    assert sc.desc.technique.aov_mis == 1
    films, aovs = [], []
    try:
        for cfg in AOV_CONFIGS:
            for k, v in cfg.items():
                device.set_option(k, v)
            films.append(render_gpu(device, sc, w, h, spi))
            aovs.append([device.framebuffer(w * h * 3, n)[0] for n in ("Direct Weights", "NEE Weights")])
            for k in cfg:
                device.set_option(k, {"fuse_generate": 1, "concurrent_chunks": 1, "tail_threshold": -1, "split": -1,
                                      "lds_scene_max": 48 * 1024, "refill": -1, "tail_pairs": -1}[k])
        with pytest.raises(RuntimeError):
            device.framebuffer(w * h * 3, "Normals")
    finally:
        for k, v in (("fuse_generate", 1), ("concurrent_chunks", 1), ("tail_threshold", -1), ("split", -1),
                     ("lds_scene_max", 48 * 1024), ("refill", -1), ("tail_pairs", -1)):
            device.set_option(k, v)
    for f, a in zip(films[1:], aovs[1:]):
        np.testing.assert_array_equal(films[0], f)
        np.testing.assert_array_equal(aovs[0][0], a[0])
        np.testing.assert_array_equal(aovs[0][1], a[1])
    di, nee = aovs[0]
    assert di.sum() > 0 and nee.sum() > 0
    np.testing.assert_allclose(di + nee, films[0], rtol=1e-5, atol=1e-6)
    if plain:
        ref = render_gpu(device, ignis_amd.Scene.from_file(os.path.join(root, "scenes", plain)), w, h, spi)
        np.testing.assert_array_equal(films[0], ref)
    orc = O.OracleScene(sc)
    od, on = np.zeros(w * h * 3, np.float32), np.zeros(w * h * 3, np.float32)
    o, _ = orc.render(w, h, spi, threads=16, aov={"Direct Weights": od, "NEE Weights": on})
    assert rel_mse(films[0], o) <= 5e-3
    assert rel_mse(di, od) <= 5e-3
    assert rel_mse(nee, on) <= 5e-3


@pytest.mark.parametrize("name", ["diamond_scene.json", "primitives.json", "s_deep.json"])
@pytest.mark.parametrize("film", [(112, 80), (640, 400)])
def test_dynamic_groups_invariance(device, root, name, film):
    """k_extend handing out groups of 64 paths through per-shard counters
    (waves move on to the next open shard once their own is exhausted)
    renders the same image bit for bit, with the same ray counts, as the
    static grid-stride distribution: survivors stay in the shard they came
    from and every path is taken exactly once; likewise with a shard's groups
    taken from its end (group_order 1: classes C, B, A)."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    imgs, counts = [], []
    try:
        device.upload(sc)
        for dynamic, tail, order in [(0, -1, 0), (1, -1, 0), (15, -1, 0), (2, 0, 0), (15, 0, 0), (13, -1, 1), (13, -1, 0)]:
            device.set_option("dynamic", dynamic)
            device.set_option("tail_threshold", tail)
            device.set_option("group_order", order)
            device.reset_stats()
            imgs.append(render_gpu(device, sc, film[0], film[1], 4))
            st = device.stats()
            counts.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
    finally:
        device.set_option("dynamic", 13)
        device.set_option("tail_threshold", -1)
        device.set_option("group_order", -1)
    for im, c in zip(imgs[1:], counts[1:]):
        np.testing.assert_array_equal(imgs[0], im)
        assert c == counts[0]
    assert imgs[0].sum() > 0


@pytest.mark.parametrize("name", ["diamond_scene.json", "primitives.json", "s_deep.json", "s_soup_1m.json"])
def test_occlusion_parity(device, root, name):
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    device.upload(sc)
    orc = O.OracleScene(sc)
    rays = random_rays(sc, 100000, seed=7)
    rays[:, 7] = np.random.default_rng(3).uniform(0.01, 3.0, size=rays.shape[0])
    g = device.trace_occlusion(rays, 0x8)
    o = orc.trace_occlusion(rays, 0x8)
    assert (g == o).mean() >= 0.9999
    assert 0.01 < o.mean() < 0.99  # both outcomes exercised


def test_image_parity_diamond(device, diamond_path):
    sc = ignis_amd.Scene.from_file(diamond_path)
    w = h = 256
    g = render_gpu(device, sc, w, h, 8)
    o, _ = O.OracleScene(sc).render(w, h, 8)
    assert abs(g.mean() - o.mean()) / o.mean() < 0.01
    assert rel_mse(g, o) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()


def test_image_parity_primitives(device, primitives_path):
    sc = ignis_amd.Scene.from_file(primitives_path)
    w = h = 256
    g = render_gpu(device, sc, w, h, 8)
    o, _ = O.OracleScene(sc).render(w, h, 8)
    assert rel_mse(g, o) <= 1e-3
    close = np.abs(g - o) <= 1e-3 * np.maximum(np.abs(o), 1e-3)
    assert close.mean() >= 0.99, close.mean()


@pytest.mark.parametrize("name,size,spi", [("s_deep.json", 160, 4), ("s_soup_1m.json", 96, 2)])
def test_image_parity_synthetic(device, root, name, size, spi):
    """SURVEY.md §8d stand-in scenes (many instances / 1M-triangle soup) vs the oracle."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    g = render_gpu(device, sc, size, size, spi)
    o, _ = O.OracleScene(sc).render(size, size, spi)
    assert abs(g.mean() - o.mean()) / o.mean() < 0.01
    assert rel_mse(g, o) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()


def test_full_size_window_parity(device, diamond_path):
    """BASELINE size (1000^2, spi 8) on the GPU; the oracle re-renders a 1000x48 band."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    g = render_gpu(device, sc, 1000, 1000, 8, iteration=3).reshape(1000, 1000, 3)
    o, _ = O.OracleScene(sc).render(1000, 1000, 8, iteration=3, window=(0, 500, 1000, 548))
    o = o.reshape(1000, 1000, 3)[500:548]
    gb = g[500:548]
    assert rel_mse(gb, o) <= 5e-3
    close = np.abs(gb - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99
    assert np.isfinite(g).all() and (g >= 0).all()


def test_config2_diamond_256spp_matches_cpu_device(device, diamond_path):
    """BASELINE config 2 at its stated size: diamond 1000x1000, 256 spp = 32
    iterations x spi 8 (the bench's frame), rendered whole on the GPU in one
    render_iterations call (the bench's chunking); the oracle (the restated
    reference CPU device) accumulates the same 32 iterations over the WHOLE
    frame (~1.24 G rays, ~20 s on 16 threads).  Diamond contract of
    SURVEY.md §8c, and the ray counts."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    W = H = 1000
    device.upload(sc)
    device.set_option("capacity", 0)
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, 8
    device.render_iterations(p, 32)
    g, it = device.framebuffer(W * H * 3)
    assert it == 32
    st = device.stats()
    orc = O.OracleScene(sc)
    o = np.zeros(W * H * 3, np.float32)
    rays = 0
    for k in range(32):
        _, ost = orc.render(W, H, 8, iteration=k, threads=16, fb=o)
        rays += ost["camera_rays"] + ost["bounce_rays"] + ost["shadow_rays"]
    gi, oi = g.reshape(H, W, 3) / 32, o.reshape(H, W, 3) / 32
    assert rel_mse(gi, oi) <= 5e-3
    close = np.abs(gi - oi) <= 1e-2 * np.maximum(np.abs(oi), 1e-2)
    assert close.mean() >= 0.99, close.mean()
    assert np.isfinite(g).all() and (g >= 0).all()
    gpu_rays = st["camera_rays"] + st["bounce_rays"] + st["shadow_rays"]
    assert abs(gpu_rays - rays) / rays < 1e-3, (gpu_rays, rays)


def test_config3_primitives_256spp_matches_cpu_device(device, primitives_path):
    """BASELINE config 3 at its stated size: primitives.json (mixed BSDFs),
    1000x1000, 256 spp = 32 iterations x spi 8, whole frame on the GPU and on
    the oracle (max_depth 2 keeps the oracle cheap); primitives contract
    (RelSE <= 1e-3, >= 99 % of pixels within 1e-3 relative) and ray counts."""
    sc = ignis_amd.Scene.from_file(primitives_path)
    W = H = 1000
    device.upload(sc)
    device.set_option("capacity", 0)
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, 8
    device.render_iterations(p, 32)
    g, it = device.framebuffer(W * H * 3)
    assert it == 32
    st = device.stats()
    orc = O.OracleScene(sc)
    o = np.zeros(W * H * 3, np.float32)
    rays = 0
    for k in range(32):
        _, ost = orc.render(W, H, 8, iteration=k, threads=16, fb=o)
        rays += ost["camera_rays"] + ost["bounce_rays"] + ost["shadow_rays"]
    assert rel_mse(g / 32, o / 32) <= 1e-3
    close = np.abs(g - o) <= 1e-3 * np.maximum(np.abs(o), 1e-3)
    assert close.mean() >= 0.99, close.mean()
    gpu_rays = st["camera_rays"] + st["bounce_rays"] + st["shadow_rays"]
    assert abs(gpu_rays - rays) / rays < 1e-3, (gpu_rays, rays)


def test_config1_diamond_64spp_matches_cpu_device(device, diamond_path):
    """BASELINE config 1 (diamond, 1000x1000, 64 spp = 8 iterations x spi 8,
    seed 0) rendered whole by the HIP device and by the oracle (the restated
    reference CPU device): the accumulated framebuffers agree within the
    diamond contract of SURVEY.md §8c (RunEvaluations RelSE <= 5e-3, >= 99 %
    of pixels within 1e-2 relative), and so do the ray counts."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    W = H = 1000
    device.upload(sc)
    device.set_option("capacity", 0)
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, 8
    device.render_iterations(p, 8)
    g, it = device.framebuffer(W * H * 3)
    assert it == 8
    st = device.stats()
    orc = O.OracleScene(sc)
    o = np.zeros(W * H * 3, np.float32)
    rays = 0
    for k in range(8):
        _, ost = orc.render(W, H, 8, iteration=k, threads=16, fb=o)
        rays += ost["camera_rays"] + ost["bounce_rays"] + ost["shadow_rays"]
    assert rel_mse(g / 8, o / 8) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()
    gpu_rays = st["camera_rays"] + st["bounce_rays"] + st["shadow_rays"]
    assert abs(gpu_rays - rays) / rays < 1e-3, (gpu_rays, rays)


ANALYTIC = json.load(open(os.path.join(GOLDEN, "analytic_kats.json")))["cases"]


@pytest.mark.parametrize("name,light", [("no_light", None), ("point", POINT_LIGHT), ("spot", SPOT_LIGHT), ("env", ENV_LIGHT),
                                        ("directional", DIRECTIONAL_LIGHT), ("sun", SUN_LIGHT)])
def test_analytic_known_answers(device, name, light):
    """test_lights.py / test_init.py at the reference's 1000^2 film, values re-derived (tests/golden)."""
    sc = ignis_amd.Scene.from_string(flat_scene([light] if light else []))
    fb = render_gpu(device, sc, 1000, 1000, 8)
    pix = fb.reshape(-1, 3).mean(axis=1)
    mean, se = float(pix.mean()), float(pix.std() / math.sqrt(pix.size))
    assert abs(mean - ANALYTIC[name]["value"]) <= 5 * se + 1e-6, (mean, ANALYTIC[name]["value"], se)


def test_empty_scene(device):
    sc = ignis_amd.Scene.from_string({})
    fb = render_gpu(device, sc, 64, 48, 4)
    assert np.all(fb == 0)


def test_bitwise_reproducible_and_spi_dependent(device):
    """test_reproducibility.py:5-20 -- and the GPU result is bitwise deterministic (no float atomics)."""
    sc = ignis_amd.Scene.from_string(flat_scene([POINT_LIGHT], size=128))
    a = render_gpu(device, sc, 128, 128, 1, seed=42)
    b = render_gpu(device, sc, 128, 128, 1, seed=42)
    np.testing.assert_array_equal(a, b)
    c = render_gpu(device, sc, 128, 128, 4, seed=42)
    assert not np.allclose(a, c)


@pytest.mark.parametrize("start_pct", [10, 100])
def test_concurrent_chunks_bit_identical(root, diamond_path, start_pct):
    """Concurrent chunks (render_chunks_concurrent: the two stream slots' chunks
    run their bounces at once, resolves in chunk order) give the sequential
    schedule's film bit for bit; small chunks (option capacity) force many
    chunks per call, over iterations and over pixel ranges of one iteration,
    with and without tiles."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, spi, iters = 160, 120, 4, 6
    films = []
    for conc, asy in ((0, 0), (1, 0), (1, 1)):
        for tile in (None, (40, 1, 3)):
            d = ignis_amd.Device(0)
            d.upload(sc)
            d.set_option("async_render", asy)
            # chunks of at most 65536 paths: a tile share's two iterations, or part
            # of one iteration of the whole film; a low tail threshold keeps each
            # chunk in its wavefront bounce loop for several bounces
            d.set_option("capacity", 65536)
            d.set_option("tail_threshold", 4096)
            d.set_option("concurrent_chunks", conc)
            d.set_option("concurrent_start_pct", start_pct)
            p = ignis_amd.RenderParams()
            p.width, p.height, p.spi = w, h, spi
            if tile:
                p.tile_size, p.tile_offset, p.tile_stride = tile
            d.render_iterations(p, iters)
            fb, n = d.framebuffer(w * h * 3)
            assert n == iters
            films.append(fb)
            d.close()
    for k in (2, 4):
        np.testing.assert_array_equal(films[0], films[k])
        np.testing.assert_array_equal(films[1], films[k + 1])
    assert films[0].sum() > 0


def test_async_render_queue_matches_synchronous(diamond_path):
    """async_render: clear / render calls only queue work for the handle's
    worker thread, which overlaps consecutive frames; the frame left in the
    framebuffer after several queued clear + render pairs, and the statistics,
    equal a synchronous render of that frame."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, spi = 200, 150, 8
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, spi
    films, rays = [], []
    for asy in (0, 1):
        d = ignis_amd.Device(0)
        d.upload(sc)
        d.set_option("async_render", asy)
        d.set_option("capacity", 65536)
        d.set_option("tail_threshold", 4096)
        for it in range(3):  # three frames back to back; the last one stays
            d.clear()
            p.iteration = it * 4
            d.render_iterations(p, 4)
        d.reset_stats()
        d.clear()
        p.iteration = 12
        d.render_iterations(p, 4)
        fb, n = d.framebuffer(w * h * 3)
        st = d.stats()
        assert n == 4
        films.append(fb)
        rays.append((st["camera_rays"], st["bounce_rays"], st["shadow_rays"]))
        d.close()
    np.testing.assert_array_equal(films[0], films[1])
    assert rays[0] == rays[1]


@pytest.mark.parametrize("tail", [0, 1 << 30])
def test_schedules_share_chunk_steps(diamond_path, tail):
    """The sequential schedule, the concurrent one and the concurrent one on
    the async worker run the same chunk steps: three iterations in one call,
    cut into chunks of one iteration's paths, with every path in the wavefront
    bounces (tail_threshold 0) or every chunk one tail pass (1 << 30), leave
    bit-identical films and equal ray, iteration and tail-launch counts."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, spi, iters = 100, 100, 2, 3
    films, counts = [], []
    for conc, asy in ((0, 0), (1, 0), (1, 1)):
        d = ignis_amd.Device(0)
        d.upload(sc)
        d.set_option("concurrent_chunks", conc)
        d.set_option("async_render", asy)
        d.set_option("capacity", 20000)
        d.set_option("tail_threshold", tail)
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi = w, h, spi
        d.render_iterations(p, iters)
        fb, n = d.framebuffer(w * h * 3)
        st = d.stats()
        assert n == iters
        films.append(fb)
        counts.append((st["camera_rays"], st["bounce_rays"] + st["tail_bounce_rays"], st["shadow_rays"] + st["tail_shadow_rays"],
                       st["iterations"], st["launches_finish"]))
        d.close()
    np.testing.assert_array_equal(films[0], films[1])
    np.testing.assert_array_equal(films[0], films[2])
    assert films[0].sum() > 0
    assert counts[0] == counts[1] == counts[2]
    assert counts[0][0] == w * h * spi * iters and counts[0][3] == iters


def test_async_worker_failure_is_sticky_until_clear(diamond_path):
    """A chunk that fails on the async worker (test hook "fail_chunk") drops the
    queue, so film and iteration count no longer agree: every later call that
    waits for the queue reports the failure (with its message) until igx_clear,
    after which the handle renders the synchronous frame again."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, spi = 160, 120, 4
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, spi
    ref = ignis_amd.Device(0)
    ref.upload(sc)
    ref.set_option("async_render", 0)
    ref.set_option("capacity", 32768)
    ref.render_iterations(p, 4)
    want, _ = ref.framebuffer(w * h * 3)
    ref.close()
    d = ignis_amd.Device(0)
    d.upload(sc)
    d.set_option("async_render", 1)
    d.set_option("capacity", 32768)  # several chunks per call
    d.set_option("fail_chunk", 3)
    d.render_iterations(p, 4)  # queued; the third chunk fails on the worker
    for call in (lambda: d.framebuffer(w * h * 3), d.stats, lambda: d.set_option("timing", 0),
                 lambda: d.render_iterations(p, 1)):
        with pytest.raises(ignis_amd.IgxError, match="injected failure"):
            call()
    d.clear()  # lifts the failure
    d.render_iterations(p, 4)
    got, n = d.framebuffer(w * h * 3)
    assert n == 4
    np.testing.assert_array_equal(got, want)
    d.close()


def test_signed_zero_directions_hit_alike(device, root):
    """Axis-aligned rays through the diamond scene (identity and translated
    instances, whose BLAS entry skips the transform): +0 and -0 direction
    components give bit-identical closest hits, and the hits agree with the
    oracle's general transform_ray (ray.art:53-59).  A -0 component would give
    safe_rcp's -FLT_MAX where the transform gives +FLT_MAX; such rays take the
    general transform."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "diamond_scene.json"))
    device.upload(sc)
    lo = np.array(sc.desc.scene_bbox_min[:]) - 0.05
    hi = np.array(sc.desc.scene_bbox_max[:]) + 0.05
    rng = np.random.default_rng(5)
    n = 6 * 4096
    org = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    axes = np.repeat(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32), n // 6, 0)
    pos = np.zeros((n, 8), np.float32)
    pos[:, 0:3], pos[:, 3:6], pos[:, 6], pos[:, 7] = org, axes, 1e-3, 3.4e38
    neg = pos.copy()
    neg[:, 3:6] = np.where(axes == 0, np.float32(-0.0), axes)  # the zero components negative
    assert np.signbit(neg[:, 3:6]).sum() > n
    hp, hn = device.trace_hits(pos, 0x4), device.trace_hits(neg, 0x4)
    np.testing.assert_array_equal(hp[0], hn[0])
    np.testing.assert_array_equal(hp[1].view(np.uint32), hn[1].view(np.uint32))
    assert (hp[0][:, 0] >= 0).mean() > 0.2
    orc = O.OracleScene(sc)
    assert_hit_parity(hn, orc.trace_hits(neg, 0x4), neg, 0x4)


def test_tile_sharding_equals_full_render(device, diamond_path):
    """Multi-GPU decomposition: tiles rendered by 3 shards sum to the full render bit for bit."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h = 200, 150
    full = render_gpu(device, sc, w, h, 4)
    acc = np.zeros_like(full)
    for r in range(3):
        acc += render_gpu(device, sc, w, h, 4, tile=(64, r, 3))
    np.testing.assert_array_equal(acc, full)


def test_pack_tiles_and_assemble(device, diamond_path):
    """The bench's multi-GPU gather: every shard packs its tiles on the device
    (igx_pack_tiles), the packed buffers are concatenated as all_gather would,
    and shard.assemble rebuilds the full render bit for bit."""
    import torch
    from ignis_amd import shard

    sc = ignis_amd.Scene.from_file(diamond_path)
    w, h, T, N = 200, 150, 64, 3
    full = render_gpu(device, sc, w, h, 4)
    per = shard.max_tiles_per_rank(w, h, T, N) * T * T * 3
    packs = []
    for r in range(N):
        render_gpu(device, sc, w, h, 4, tile=(T, r, N))
        buf = torch.zeros(per, dtype=torch.float32, device="cuda")
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi, p.tile_size, p.tile_offset, p.tile_stride = w, h, 4, T, r, N
        device.pack_tiles(p, buf.data_ptr(), buf.numel())
        packs.append(buf.cpu().numpy())
    dst = shard.packed_destinations(w, h, T, N)
    frame = shard.assemble(np.concatenate(packs).reshape(-1, 3), dst, np.zeros((w * h, 3), np.float32))
    np.testing.assert_array_equal(frame.reshape(-1), full)


def test_capacity_chunking_is_exact(device, diamond_path):
    sc = ignis_amd.Scene.from_file(diamond_path)
    a = render_gpu(device, sc, 160, 120, 8)
    b = render_gpu(device, sc, 160, 120, 8, capacity=8 * 1000 + 3)
    np.testing.assert_array_equal(a, b)


def test_ray_list_mode(device, diamond_path):
    """igtrace mode (trace/main.cpp:16-67, emitter.art:18-30) vs the oracle's list emitter."""
    sc = ignis_amd.Scene.from_file(diamond_path)
    rays = camera_rays(sc, 64, 64, jitter=0.3)
    device.upload(sc)
    device.clear()
    p = ignis_amd.RenderParams()
    import ctypes as C
    p.spi, p.num_rays = 4, rays.shape[0]
    p.rays = rays.ctypes.data_as(C.POINTER(C.c_float))
    device.render(p)
    g, _ = device.framebuffer(rays.shape[0] * 3)
    o, _ = O.OracleScene(sc).render(rays.shape[0], 1, 4, rays=rays)
    assert rel_mse(g, o) <= 5e-3


def test_ray_counters_match_oracle(device, diamond_path):
    sc = ignis_amd.Scene.from_file(diamond_path)
    device.reset_stats()
    render_gpu(device, sc, 128, 128, 8)
    s = device.stats()
    _, os_ = O.OracleScene(sc).render(128, 128, 8)
    assert s["camera_rays"] == os_["camera_rays"]
    for k in ("bounce_rays", "shadow_rays"):
        assert abs(s[k] - os_[k]) <= 1e-3 * os_[k] + 5, (k, s[k], os_[k])


def test_runtime_api(diamond_path):
    """Python surface mirroring ignis.Runtime (src/tests/integrator/common/__init__.py:68-90)."""
    opts = ignis_amd.RuntimeOptions.makeDefault()
    opts.SPI = 2
    opts.OverrideFilmSize = (96, 64)
    with ignis_amd.loadFromFile(diamond_path, opts) as rt:
        for _ in range(3):
            rt.step()
        assert rt.IterationCount == 3
        img = rt.getFramebufferForHost() / rt.IterationCount
        assert img.shape == (64, 96, 3)
        assert img.mean() > 0
        out = rt.trace(np.array([[0, 0, 3.85, 0, 0, -1, 0, 100]], np.float32))
        assert out.shape == (1, 3)


def test_igtrace_cli(tmp_path, diamond_path, root):
    """igtrace frontend (trace/main.cpp:16-170): ray file in, mean radiance per ray out,
    against the oracle's ray-list emitter at the same seed and spp."""
    import subprocess
    sc = ignis_amd.Scene.from_file(diamond_path)
    rays = camera_rays(sc, 32, 32, jitter=0.3)
    rf = tmp_path / "rays.txt"
    with open(rf, "w") as f:
        for r in rays:
            f.write(" ".join(f"{v:.9g}" for v in r[:6]) + f" {r[6]:.9g} {r[7]:.9g}\n")
    out = tmp_path / "out.txt"
    exe = os.path.join(root, "ignis-masterthesis_amd", "igtrace")
    subprocess.run([exe, diamond_path, "--input", str(rf), "--spp", "4", "-o", str(out)], check=True, timeout=120)
    g = np.loadtxt(out).reshape(-1)
    assert g.shape[0] == rays.shape[0] * 3
    orc = O.OracleScene(sc)
    acc = None
    for it in range(4):
        o, _ = orc.render(rays.shape[0], 1, 1, iteration=it, rays=rays)
        acc = o if acc is None else acc + o
    o = acc / 4
    assert rel_mse(g, o) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()


def test_igcli_writes_exr(tmp_path, diamond_path, root):
    """igcli frontend: one iteration of the full 1000x1000 frame to EXR equals the API render."""
    import subprocess
    from exr_read import read_exr
    out = tmp_path / "img.exr"
    exe = os.path.join(root, "ignis-masterthesis_amd", "igcli")
    r = subprocess.run([exe, diamond_path, "--spp", "8", "--spi", "8", "-o", str(out)], check=True, timeout=120,
                       capture_output=True, text=True)
    assert "Msamples/s" in r.stdout and "Mrays/s" in r.stdout
    ch, _ = read_exr(out)
    img = np.stack([ch["R"], ch["G"], ch["B"]], axis=-1).reshape(-1)
    sc = ignis_amd.Scene.from_file(diamond_path)
    ref = render_gpu(device=ignis_amd.Device(0), scene=sc, w=1000, h=1000, spi=8)
    np.testing.assert_array_equal(img, ref)


def test_igcli_camera_orientation_matches_api(tmp_path, diamond_path, root):
    """igcli --eye / --dir / --up (cli/main.cpp:103-107 -> the runtime's
    __camera_* parameters -> IG::Device::render's ParameterSet) and --width /
    --height render the same image, bit for bit, as the API with the scene
    camera replaced by that orientation; --stats dumps the ray quantities."""
    import subprocess
    from exr_read import read_exr
    from ignis_amd import _native as N
    out = tmp_path / "img.exr"
    exe = os.path.join(root, "ignis-masterthesis_amd", "igcli")
    eye, dr, up = (0.4, -0.3, 3.2), (-0.1, 0.08, -1.0), (0.05, 1.0, 0.0)
    r = subprocess.run([exe, diamond_path, "--spp", "8", "--spi", "4", "--width", "320", "--height", "240",
                        "--eye", *map(str, eye), "--dir", *map(str, dr), "--up", *map(str, up), "--stats",
                        "-o", str(out)], check=True, timeout=120, capture_output=True, text=True)
    for key in ("CameraRays", "BounceRays", "ShadowRays", "PrimaryRays", "TotalRays", "Iterations: 2"):
        assert key in r.stdout, r.stdout
    ch, _ = read_exr(out)
    img = np.stack([ch["R"], ch["G"], ch["B"]], axis=-1).reshape(-1)
    sc = ignis_amd.Scene.from_file(diamond_path)
    cam = N.Camera.from_buffer_copy(sc.desc.camera)
    cam.eye[:], cam.dir[:], cam.up[:] = eye, dr, up
    dev = ignis_amd.Device(0)
    dev.upload(sc)
    dev.set_camera(cam)
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = 320, 240, 4
    dev.render_iterations(p, 2)
    ref, it = dev.framebuffer(320 * 240 * 3)
    dev.close()
    assert it == 2
    np.testing.assert_array_equal(img, ref / np.float32(2))
    # and the orientation did change the image
    plain = render_gpu(device=ignis_amd.Device(0), scene=sc, w=320, h=240, spi=4)
    assert not np.array_equal(plain, ref)


def test_bench_plain_run_dumps_last_frame(tmp_path, diamond_path, root):
    """A plain `bench.py --gpus 1 --steps N --warmup W` times N steps and prints
    the headline line without any of the --full measurements; --dump-outputs
    writes the last timed frame, which equals the API render of the same frame
    bit for bit (same arguments, same inputs, same outputs)."""
    import subprocess
    import sys
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--size", "96", "--spp", "8", "--spi", "4", "--dump-outputs", str(out)],
                       check=True, timeout=120, capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # N steps were timed: the rays of the line are two frames' worth of camera rays
    assert line["rays"]["camera"] == 2 * 96 * 96 * 8
    total = sum(line["rays"].values())
    # ms_per_step is printed to 1e-3 ms and a step of this frame takes well over 0.1 ms
    assert line["value"] == pytest.approx(total / (2 * line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for key in ("roofline", "roofline_shadow", "cpu_baseline", "parity", "suite"):
        assert line[key] is None, key
    assert "config5" not in line
    fb = np.load(out / "framebuffer.npy")
    assert fb.dtype == np.float32 and fb.shape == (96, 96, 3)
    assert np.load(out / "iterations.npy").tolist() == [2.0]
    dev = ignis_amd.Device(0)
    dev.upload(ignis_amd.Scene.from_file(diamond_path))
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = 96, 96, 4
    dev.render_iterations(p, 2)
    ref, it = dev.framebuffer(96 * 96 * 3)
    dev.close()
    assert it == 2
    np.testing.assert_array_equal(fb.reshape(-1), ref)


def test_image_parity_materials(device, root):
    """§8f wider materials: mirror, smooth / rough conductors (VNDF-GGX, GGX, Beckmann,
    anisotropic), smooth / rough plastic, Oren-Nayar, glass -- GPU vs oracle."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "materials.json"))
    g = render_gpu(device, sc, 192, 192, 8)
    o, _ = O.OracleScene(sc).render(192, 192, 8)
    assert abs(g.mean() - o.mean()) / o.mean() < 0.01
    assert rel_mse(g, o) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()


@pytest.mark.parametrize("name", ["sphere_area", "mesh_area"])
def test_area_emitters_known_answers(device, name):
    """Sphere and triangle-shape emitters (light/area.art:45-105, 240-293) against closed forms."""
    sc = ignis_amd.Scene.from_string(emitter_scene(name))
    fb = render_gpu(device, sc, 1000, 1000, 8)
    pix = fb.reshape(-1, 3).mean(axis=1)
    mean, se = float(pix.mean()), float(pix.std() / math.sqrt(pix.size))
    assert abs(mean - ANALYTIC[name]["value"]) <= 5 * se + 1e-6, (mean, ANALYTIC[name]["value"], se)


LIGHTS_SCENE = {
    "technique": {"type": "path", "max_depth": 8},
    "camera": {"type": "perspective", "fov": 55, "near_clip": 0.01, "far_clip": 100,
               "transform": [{"lookat": {"origin": [0, -4.5, 1.6], "target": [0, 0, 0.9], "up": [0, 0, 1]}}]},
    "bsdfs": [{"type": "diffuse", "name": "white", "reflectance": [0.75, 0.75, 0.75]},
              {"type": "diffuse", "name": "red", "reflectance": [0.7, 0.15, 0.1]},
              {"type": "roughconductor", "name": "metal", "material": "gold", "roughness": 0.2},
              {"type": "diffuse", "name": "black", "reflectance": [0, 0, 0]}],
    "shapes": [{"type": "rectangle", "name": "floor", "width": 6, "height": 6},
               {"type": "rectangle", "name": "wall", "width": 6, "height": 3,
                "transform": [{"translate": [0, 2.5, 1.5]}, {"rotate": [90, 0, 0]}]},
               {"type": "cube", "name": "block", "width": 0.8, "height": 0.8, "depth": 1.2,
                "transform": [{"rotate": [0, 0, 25]}, {"translate": [-0.9, 0.6, 0.6]}]},
               {"type": "sphere", "name": "ball", "center": [0.9, 0.3, 0.5], "radius": 0.5},
               {"type": "sphere", "name": "lamp", "center": [0.2, -0.6, 2.1], "radius": 0.25},
               {"type": "cylinder", "name": "tube", "radius": 0.06, "p0": [-1.8, 1.8, 0.2], "p1": [-1.8, 1.8, 2.4]},
               {"type": "icosphere", "name": "bulb", "center": [1.6, 1.6, 1.8], "radius": 0.2, "subdivisions": 3}],
    "entities": [{"name": "floor", "shape": "floor", "bsdf": "white"},
                 {"name": "wall", "shape": "wall", "bsdf": "red"},
                 {"name": "block", "shape": "block", "bsdf": "white"},
                 {"name": "ball", "shape": "ball", "bsdf": "metal"},
                 {"name": "lamp", "shape": "lamp", "bsdf": "black"},
                 {"name": "tube", "shape": "tube", "bsdf": "black"},
                 {"name": "bulb", "shape": "bulb", "bsdf": "black"}],
    "lights": [{"type": "area", "name": "L_lamp", "entity": "lamp", "radiance": [6, 5, 4]},
               {"type": "area", "name": "L_tube", "entity": "tube", "radiance": [2, 3, 6]},
               {"type": "area", "name": "L_bulb", "entity": "bulb", "radiance": [5, 5, 5]},
               {"type": "env", "name": "sky", "radiance": [0.05, 0.05, 0.06]}],
}


def test_image_parity_area_emitters(device):
    """§8f wider lights: analytic sphere, mesh-detected sphere and triangle-mesh emitters
    next to an environment, GPU vs oracle."""
    sc = ignis_amd.Scene.from_string(LIGHTS_SCENE)
    types = sorted(sc.desc.lights[i].type for i in range(sc.desc.num_lights))
    assert types == [2, 7, 7, 8]
    g = render_gpu(device, sc, 192, 192, 8)
    o, _ = O.OracleScene(sc).render(192, 192, 8)
    assert abs(g.mean() - o.mean()) / o.mean() < 0.01
    assert rel_mse(g, o) <= 5e-3
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()


def test_image_parity_principled(device, root):
    """§8f principled BSDF (bsdf/principled.art): nine lobe configurations, GPU vs oracle."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "principled.json"))
    g = render_gpu(device, sc, 192, 192, 8)
    o, _ = O.OracleScene(sc).render(192, 192, 8)
    assert np.isfinite(g).all()
    close = np.abs(g - o) <= 1e-2 * np.maximum(np.abs(o), 1e-2)
    assert close.mean() >= 0.99, close.mean()
    # fireflies of the thin / transmissive spheres dominate a plain mean: compare clamped
    gc, oc = np.minimum(g, 10), np.minimum(o, 10)
    assert abs(gc.mean() - oc.mean()) / oc.mean() < 0.01
    assert rel_mse(g, o) <= 5e-3


def test_gpu_furnace_mirror_exact(device):
    """make_mirror_bsdf (ks 1) in a white environment renders exactly 1 on the device too."""
    scene = {
        "technique": {"type": "path", "max_depth": 64},
        "camera": {"type": "perspective", "fov": 30, "near_clip": 0.1, "far_clip": 100,
                   "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -4, 0, 0, 0, 1]},
        "bsdfs": [{"type": "conductor", "name": "m", "specular_reflectance": [1, 1, 1]}],
        "shapes": [{"type": "sphere", "name": "S"}],
        "entities": [{"name": "S", "shape": "S", "bsdf": "m"}],
        "lights": [{"type": "env", "name": "E", "radiance": [1, 1, 1]}],
    }
    fb = render_gpu(device, ignis_amd.Scene.from_string(scene), 64, 64, 2)
    np.testing.assert_allclose(fb, 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("n_shards", [8, 3])
def test_config5_tile_shard_gather_equals_single_device(root, n_shards):
    """BASELINE config 5 stand-in: S-deep at 4096x4096, 64 spp
    (8 iterations of spi 8), tile-sharded over N shards exactly as bench.py
    shards it (shard.balanced_tile, round-robin tiles, igx_pack_tiles, gather
    of equal-size packed buffers, assembly on rank 0): the assembled frame
    equals the single-device frame bit for bit."""
    import torch
    from ignis_amd import shard

    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "s_deep.json"))
    W = H = 4096
    spi, iters = 8, 8
    dev = ignis_amd.Device(0)
    try:
        dev.upload(sc)
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi = W, H, spi
        dev.render_iterations(p, iters)
        full, it = dev.framebuffer(W * H * 3)
        assert it == iters and np.isfinite(full).all() and full.mean() > 0
        T = shard.balanced_tile(W, n_shards)
        per = shard.max_tiles_per_rank(W, H, T, n_shards) * T * T * 3
        packs = []
        for r in range(n_shards):
            dev.clear()
            q = ignis_amd.RenderParams()
            q.width, q.height, q.spi = W, H, spi
            q.tile_size, q.tile_offset, q.tile_stride = T, r, n_shards
            dev.render_iterations(q, iters)
            buf = torch.zeros(per, dtype=torch.float32, device="cuda")
            dev.pack_tiles(q, buf.data_ptr(), buf.numel())
            packs.append(buf.cpu().numpy())
        dst = shard.packed_destinations(W, H, T, n_shards)
        frame = shard.assemble(np.concatenate(packs).reshape(-1, 3), dst, np.zeros((W * H, 3), np.float32))
        np.testing.assert_array_equal(frame.reshape(-1), full)
    finally:
        dev.close()


def probe_diverted_paths(device, orc, w, h, y, x, iters, spi=8):
    """The paths of pixel (x, y) over `iters` iterations that carry its
    device-vs-oracle difference: per sample (test hook probe_sample: the film
    receives one sample of each pixel; the pixel alone as a 1-pixel tile
    shard), then by halving the iteration range of a sample wherever a half
    holds at least 5 % of the pixel's difference, down to single paths.
    Returns [(iteration, sample, relative difference of the path)] for the
    paths found and the share of the pixel's difference they carry."""
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, spi
    p.tile_size, p.tile_offset, p.tile_stride = 1, y * w + x, w * h
    o = 3 * (y * w + x)

    def gpu(s, a, b):
        device.set_option("probe_sample", s + 1)
        device.clear()
        p.iteration = a
        device.render_iterations(p, b - a)
        fb, _ = device.framebuffer(3 * w * h)
        return fb[o:o + 3].astype(np.float64)

    def cpu(s, a, b):
        acc = np.zeros(3 * w * h, np.float32)
        for k in range(a, b):
            orc.render(w, h, spi, iteration=k, threads=1, window=(x, y, x + 1, y + 1), fb=acc, probe_sample=s)
        return acc[o:o + 3].astype(np.float64)

    found = []
    try:
        sums = [(s, gpu(s, 0, iters), cpu(s, 0, iters)) for s in range(spi)]
        total = sum(np.abs(g - c).sum() for _, g, c in sums)
        stack = [(s, 0, iters, g, c) for s, g, c in sums if np.abs(g - c).sum() >= 0.05 * total]
        while stack:
            s, a, b, g, c = stack.pop()
            if b - a == 1:
                rel = np.abs(g - c).max() / max(np.abs(c).max(), np.abs(g).max(), 1e-30)
                found.append((a, s, float(rel), float(np.abs(g - c).sum())))
                continue
            m = (a + b) // 2
            for lo, hi in ((a, m), (m, b)):
                gg, cc = gpu(s, lo, hi), cpu(s, lo, hi)
                if np.abs(gg - cc).sum() >= 0.05 * total:
                    stack.append((s, lo, hi, gg, cc))
    finally:
        device.set_option("probe_sample", 0)
    share = sum(f[3] for f in found) / max(total, 1e-30)
    return sorted((k, s, round(r, 4)) for k, s, r, _ in found), share


def test_config4_s_deep_1024spp_full_size(device, root):
    """BASELINE config 4 stand-in at its stated sample count:
    S-deep (4096 instances) at 1000x1000, 1024 spp = 128 iterations of spi 8.
    Size-independent properties at full size: the one-call frame equals the
    frame of two 64-iteration calls bit for bit (iteration offsets, chunking
    and the tail are exact over 128 M-path wavefronts), and the two
    independent 512-spp halves agree in RunEvaluations' metric (the estimator
    is converging, no NaN/inf, no biased half)."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "s_deep.json"))
    w, h = sc.film_size
    assert (w, h) == (1000, 1000)
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, 8
    device.upload(sc)
    device.set_option("capacity", 0)
    device.clear()
    device.reset_stats()
    p.iteration = 0
    device.render_iterations(p, 128)
    full, it = device.framebuffer(w * h * 3)
    assert it == 128
    assert device.stats()["camera_rays"] == w * h * 1024
    halves = []
    device.clear()
    for k in range(2):
        p.iteration = 64 * k
        device.render_iterations(p, 64)
        acc, _ = device.framebuffer(w * h * 3)
        halves.append(acc.copy())
    np.testing.assert_array_equal(full, halves[1])
    first = halves[0] / 64
    second = (halves[1] - halves[0]) / 64
    assert np.isfinite(full).all() and full.mean() > 0
    # two independent 512-spp estimates: their RunEvaluations distance is
    # about twice the per-estimate RelSE (the noise, no bias): measured 3.06e-3,
    # means 0.341778 / 0.341796
    halves_err = rel_mse(second.reshape(h, w, 3), first.reshape(h, w, 3))
    print(f"config 4 halves RelSE {halves_err:.3e}, means {first.mean():.6f} / {second.mean():.6f}")
    assert halves_err < 6e-3, halves_err
    assert abs(first.mean() - second.mean()) <= 1e-3 * first.mean()
    # and against the restated reference CPU device: the same 128 iterations
    # of a 100-row band at the diamond contract of SURVEY.md §8c
    y0, y1 = 450, 550
    orc = O.OracleScene(sc)
    o = np.zeros(w * h * 3, np.float32)
    for k in range(128):
        orc.render(w, h, 8, iteration=k, threads=16, window=(0, y0, w, y1), fb=o)
    gb = full.reshape(h, w, 3)[y0:y1] / 128
    ob = o.reshape(h, w, 3)[y0:y1] / 128
    err = rel_mse(gb, ob)
    close = np.abs(gb - ob) <= 1e-2 * np.maximum(np.abs(ob), 1e-2)
    print(f"config 4 band vs oracle: RelSE {err:.3e}, within 1e-2 {close.mean():.5f}, means {gb.mean():.6f} / {ob.mean():.6f}")
    assert err <= 5e-3
    assert abs(gb.mean() - ob.mean()) <= 1e-3 * ob.mean()  # no bias
    # the same paths on both sides, up to float rounding (fast-math light
    # sampling on the device), which diverts rare paths at a grazing edge or a
    # Russian-roulette / Fresnel threshold.  A pixel averages 1024 paths here,
    # so more pixels hold one diverted path than at the diamond contract's
    # 8-64 spp (measured 98.3 % within 1e-2 where 64 spp gives >= 99 %)
    assert close.mean() >= 0.975, close.mean()
    # ... and that is what the pixels outside 1e-2 hold: probed path by path,
    # each has one to three paths (of 1024) that differ between the device and
    # the oracle, the rest agree to float rounding, and the diverted paths make
    # up the pixel's difference
    off = np.argwhere(~close.all(axis=-1))
    pick = off[np.random.default_rng(3).choice(len(off), size=min(8, len(off)), replace=False)]
    diverted = [probe_diverted_paths(device, orc, w, h, y0 + int(r), int(x), 128) for r, x in pick]
    for (r, x), (paths, share) in zip(pick, diverted):
        print(f"config 4 pixel ({x}, {y0 + r}): paths carrying the difference (iteration, sample, relative "
              f"difference) {paths}, share {share:.3f}")
        # one to three whole paths (a diverted path differs by O(1), not by rounding) carry >= 90 %
        assert 1 <= len(paths) <= 3, paths
        assert all(rel > 1e-2 for _, _, rel in paths), paths
        assert share >= 0.9, share


def test_config5_s_deep_4096_band_matches_cpu_device(device, root):
    """BASELINE config 5 stand-in at its stated size: S-deep at 4096x4096,
    64 spp = 8 iterations of spi 8, rendered whole on the GPU in one call (a
    134 M-path iteration: two chunks per iteration); the oracle accumulates the
    same 8 iterations over a 64-row band, diamond contract of SURVEY.md §8c."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "s_deep.json"))
    W = H = 4096
    device.upload(sc)
    device.set_option("capacity", 0)
    device.clear()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, 8
    device.render_iterations(p, 8)
    g, it = device.framebuffer(W * H * 3)
    assert it == 8 and np.isfinite(g).all()
    y0, y1 = 2016, 2080
    orc = O.OracleScene(sc)
    o = np.zeros(W * H * 3, np.float32)
    for k in range(8):
        orc.render(W, H, 8, iteration=k, threads=16, window=(0, y0, W, y1), fb=o)
    gb = g.reshape(H, W, 3)[y0:y1] / 8
    ob = o.reshape(H, W, 3)[y0:y1] / 8
    assert rel_mse(gb, ob) <= 5e-3
    close = np.abs(gb - ob) <= 1e-2 * np.maximum(np.abs(ob), 1e-2)
    assert close.mean() >= 0.99, close.mean()


def test_pack_tiles_rejects_a_film_that_is_not_the_framebuffer(device, diamond_path):
    """igx_pack_tiles reads dev->fb through the tile table: a film larger than
    the allocated framebuffer must be refused, not read out of bounds."""
    import torch

    sc = ignis_amd.Scene.from_file(diamond_path)
    render_gpu(device, sc, 200, 150, 4, tile=(64, 0, 3))
    buf = torch.zeros(64 * 64 * 3 * 64, dtype=torch.float32, device="cuda")
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi, p.tile_size, p.tile_offset, p.tile_stride = 400, 300, 4, 64, 0, 3
    with pytest.raises(ignis_amd.IgxError, match="does not match the framebuffer"):
        device.pack_tiles(p, buf.data_ptr(), buf.numel())


@pytest.mark.parametrize("name,max_leaf", [("diamond_scene.json", 4), ("primitives.json", 4), ("materials.json", 40)])
def test_database_adapter_renders_bit_identically(device, root, name, max_leaf):
    """The reference's SceneDatabase tables (tests/refdb.py) through
    igx_scene_from_database, traced over the reference-layout BLAS they carry
    (Node2 + Tri1, leaves up to max_leaf triangles), render the same image bit
    for bit as the JSON loader's scene over igx's own BVH (closest hits do not
    depend on BVH topology: order-independent ties), and so do the same tables
    with the BLAS rebuilt (option rebuild_bvh)."""
    from refdb import RefDatabase

    scene = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    db, sv, keep = RefDatabase(scene, max_leaf=max_leaf).views()
    adapted = ignis_amd.Scene.from_database(db, sv)
    w, h, spi = 160, 120, 4
    a = render_gpu(device, scene, w, h, spi)
    b = render_gpu(device, adapted, w, h, spi)
    ra = device.stats()
    device.set_option("rebuild_bvh", 1)
    try:
        c = render_gpu(device, adapted, w, h, spi)
    finally:
        device.set_option("rebuild_bvh", 0)
    assert np.isfinite(a).all() and a.mean() > 0
    assert np.array_equal(a, b), f"max |diff| {np.abs(a - b).max()}"
    assert np.array_equal(a, c)
    assert ra["bvh_depth"] > 0


def test_imported_one_leaf_blas_with_infinite_tmax(device):
    """A reference BLAS whose root wraps ONE leaf of more than 16 triangles
    (BvhNAdapter.h:94-98) is imported with the duplicated sibling absent
    (kEmptyRef, +inf bounds).  Rays with tmax = +inf and an all-positive
    direction (the case where an +inf box passes a slab test against an
    infinite tmax) must not enter it: closest hits equal those over igx's own
    BVH of the same scene (trav_init keeps tmax finite)."""
    from refdb import RefDatabase

    doc = {
        "technique": {"type": "path", "max_depth": 2},
        "camera": {"type": "perspective", "fov": 60, "near_clip": 0.01, "far_clip": 100,
                   "transform": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -4]},
        "film": {"size": [64, 64]},
        "bsdfs": [{"type": "diffuse", "name": "grey", "reflectance": [0.5, 0.5, 0.5]}],
        "shapes": [{"type": "icosphere", "name": "Ball", "radius": 1.0, "subdivisions": 1}],
        "entities": [{"name": "Ball", "shape": "Ball", "bsdf": "grey"}],
        "lights": [{"type": "env", "name": "sky", "radiance": [1, 1, 1]}],
    }
    scene = ignis_amd.Scene.from_string(json.dumps(doc))
    assert scene.desc.meshes[0].num_faces == 80
    db, sv, keep = RefDatabase(scene, max_leaf=100).views()  # one leaf of 80 triangles under the root
    adapted = ignis_amd.Scene.from_database(db, sv)
    rng = np.random.default_rng(3)
    n = 20000
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-3.0, -1.2, size=(n, 3))
    d = rng.uniform(0.05, 1.0, size=(n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6], rays[:, 7] = 0.0, np.inf
    device.upload(scene)
    own = device.trace_hits(rays, 0x4)
    device.upload(adapted)
    imp = device.trace_hits(rays, 0x4)
    assert (own[0][:, 0] >= 0).mean() > 0.05  # some rays hit the ball, the rest miss
    np.testing.assert_array_equal(own[0], imp[0])
    np.testing.assert_array_equal(own[1], imp[1])
    del keep
