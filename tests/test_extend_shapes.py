"""Option "extend_shapes": launches of the default fused mode run k_extend
compiled for that mode (one shape for bounce 0 building its camera paths, one
for the launches that read the path stream) instead of the generic kernel that
decides everything from run-time flags.  The shapes fold flags to constants and
drop dead branches; a path's arithmetic is the generic kernel's, so films and
ray counts must be the same bit for bit under every schedule, and every
combination of options outside the default mode must keep the generic kernel.
"""
import ctypes as C
import os

import numpy as np
import pytest

import ignis_amd

pytestmark = pytest.mark.gpu

W, H, SPI, ITERS = 64, 64, 8, 3
DEFAULTS = {"extend_shapes": -1, "tail_threshold": -1, "fuse_generate": 1, "concurrent_chunks": 1, "capacity": 0,
            "lds_shading": -1, "path_classes": 4, "shadow_classes": 1, "group_order": -1, "instrument": 0}
# scene, options: the wide LDS layout (1024 threads), the 256-thread LDS
# layout, global tables with 4-wide nodes
LAYOUTS = {"wide": ("diamond_scene.json", {}, 1024), "lds256": ("diamond_scene.json", {"lds_shading": 0}, 256),
           "global": ("primitives.json", {}, 256)}


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def load(root, name):
    return ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))


def render(device, scene, opts, params=None, aovs=(), count=None):
    """(film, AOV films, (camera, bounce, shadow) rays, (extend launches, [generate, bounce] shaped launches), stats)."""
    device.upload(scene)
    for k, v in {**DEFAULTS, **opts}.items():
        device.set_option(k, v)
    device.clear()
    device.reset_stats()
    plist = params
    if plist is None:
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi = W, H, SPI
        plist = [p]
    for p in plist:
        device.render_iterations(p, ITERS)
    n = count if count is not None else W * H * 3
    fb = device.framebuffer(n)[0].copy()
    extra = [device.framebuffer(n, a)[0].copy() for a in aovs]
    st = device.stats()
    return fb, extra, (st["camera_rays"], st["bounce_rays"], st["shadow_rays"]), (st["launches_extend"], list(st["launches_extend_shaped"])), st


def restore(device):
    for k, v in DEFAULTS.items():
        device.set_option(k, v)


def assert_shaped_equals_generic(device, scene, opts, eligible, **kw):
    """Option 1 against 0; with 1 every k_extend launch of an eligible
    combination ran a shape (and none of an ineligible one), with 0 none did."""
    off, a_off, c_off, (n_off, s_off), _ = render(device, scene, {**opts, "extend_shapes": 0}, **kw)
    on, a_on, c_on, (n_on, s_on), st = render(device, scene, {**opts, "extend_shapes": 1}, **kw)
    np.testing.assert_array_equal(off, on, err_msg=str(opts))
    for x, y in zip(a_off, a_on):
        np.testing.assert_array_equal(x, y, err_msg=str(opts))
    assert c_on == c_off, opts
    assert off.sum() > 0
    assert s_off == [0, 0], (opts, s_off)
    assert n_on == n_off, opts
    assert sum(s_on) == (n_on if eligible else 0), (opts, n_on, s_on)
    return off, (n_on, s_on), st


@pytest.mark.parametrize("tail", [-1, 0, 1 << 30])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_shaped_equals_generic(device, root, layout, tail):
    """The three LDS layouts of k_extend; the automatic tail threshold, the
    wavefront to the last path, the tail kernel only; generation fused into
    bounce 0 or by k_generate; concurrent or sequential chunks; one chunk for
    all three iterations or chunks of 8192 paths (four per iteration: slots
    are reused, chunks overlap, and under the automatic threshold every such
    chunk goes straight to the tail kernel)."""
    name, lopts, threads = LAYOUTS[layout]
    sc = load(root, name)
    films = []
    try:
        for cap in (0, 8192):
            for fuse in (1, 0):
                for conc in (1, 0):
                    opts = {**lopts, "tail_threshold": tail, "fuse_generate": fuse, "concurrent_chunks": conc, "capacity": cap}
                    film, (n, shaped), st = assert_shaped_equals_generic(device, sc, opts, eligible=True)
                    assert st["extend_block_threads"] == threads, (layout, st["extend_block_threads"])
                    wavefront = tail == 0 or (tail < 0 and cap == 0)
                    assert (n > 0) == wavefront, (opts, n)
                    # the generate shape runs exactly where bounce 0 builds its camera paths
                    assert (shaped[0] > 0) == (wavefront and fuse == 1), (opts, shaped)
                    assert (shaped[1] > 0) == wavefront, (opts, shaped)
                    films.append(film)
    finally:
        restore(device)
    for f in films[1:]:
        np.testing.assert_array_equal(films[0], f)


@pytest.mark.parametrize("layout", ["wide", "global"])
def test_tiles_equal_whole_film(device, root, layout):
    """Two tile shards (tile_size 8, offsets 0 and 1 of stride 2) rendered with
    the shapes fill the film of the whole-film render: the generate shape keeps
    the tile fields as run-time values."""
    name, lopts, _ = LAYOUTS[layout]
    sc = load(root, name)
    shards = []
    for off in (0, 1):
        p = ignis_amd.RenderParams()
        p.width, p.height, p.spi, p.tile_size, p.tile_offset, p.tile_stride = W, H, SPI, 8, off, 2
        shards.append(p)
    try:
        opts = {**lopts, "tail_threshold": 0}
        whole, _, c_whole, _, _ = render(device, sc, {**opts, "extend_shapes": 0})
        tiled, (n, shaped), _ = assert_shaped_equals_generic(device, sc, opts, eligible=True, params=shards)
        assert shaped[0] > 0 and shaped[1] > 0, shaped
    finally:
        restore(device)
    np.testing.assert_array_equal(whole, tiled)


@pytest.mark.parametrize("opts", [{"path_classes": 3}, {"path_classes": 1}, {"path_classes": 0}, {"shadow_classes": 0},
                                  {"group_order": 1}, {"instrument": 1}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("layout", ["wide", "global"])
def test_other_modes_keep_the_generic_kernel(device, root, layout, opts):
    """Outside the default fused mode option 1 launches the generic kernel
    only, and renders what option 0 renders."""
    name, lopts, _ = LAYOUTS[layout]
    sc = load(root, name)
    try:
        _, (n, _), _ = assert_shaped_equals_generic(device, sc, {**lopts, **opts, "tail_threshold": 0}, eligible=False)
        assert n > 0
    finally:
        restore(device)


def test_ray_list_keeps_the_generic_kernel(device, root):
    """Ray-list mode (a 4096-ray list of camera-like rays)."""
    sc = load(root, "diamond_scene.json")
    rng = np.random.default_rng(7)
    n = 4096
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 2] = -np.abs(d[:, 2]) - 2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 2] = 3.85
    rays[:, 3:6] = d
    rays[:, 6], rays[:, 7] = 0.1, 100
    p = ignis_amd.RenderParams()
    p.spi, p.num_rays = SPI, n
    p.rays = rays.ctypes.data_as(C.POINTER(C.c_float))
    try:
        _, (launches, _), _ = assert_shaped_equals_generic(device, sc, {"tail_threshold": 0}, eligible=False, params=[p], count=n * 3)
        assert launches > 0
    finally:
        restore(device)


def test_mis_aovs_keep_the_generic_kernel(device, root):
    """An aov_mis scene: the film and both AOVs."""
    sc = load(root, "primitives_aov.json")
    assert sc.desc.technique.aov_mis == 1
    try:
        _, (launches, _), _ = assert_shaped_equals_generic(device, sc, {"tail_threshold": 0}, eligible=False,
                                                          aovs=("Direct Weights", "NEE Weights"))
        assert launches > 0
    finally:
        restore(device)
