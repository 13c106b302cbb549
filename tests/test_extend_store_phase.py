"""The store phase of k_extend's generate and bounce shapes (one class pass
for the bounced ray and the shadow ray, the append's atomics issued ahead of
the record arithmetic, records addressed by scalar array bases and 32-bit
offsets) against the generic kernel, which keeps the two early-exit class
loops and the per-lane 64-bit addresses: every ray must get the class it gets
there and every record the place it gets there, so option "extend_shapes" 1
renders the film of option 0 bit for bit, with the same ray counts and the same
number of surviving paths, on small frames that reach every branch of the
phase: partial groups, the wavefront to the last path, several chunks, both
chunk schedules, both shadow modes, a tile shard, scenes without and with the
largest number of enclosing entities, and the three LDS layouts.
"""
import json
import os

import numpy as np
import pytest

import ignis_amd

pytestmark = pytest.mark.gpu

SPI, ITERS = 8, 3
DEFAULTS = {"extend_shapes": -1, "tail_threshold": -1, "concurrent_chunks": 1, "capacity": 0, "slot_budget_mb": 0,
            "lds_shading": -1, "shadow_optimistic": -1}
COUNTS = ("camera_rays", "bounce_rays", "shadow_rays", "extend_paths_out")
MAX_ENCLOSING = 31  # csrc/device_scene.h: the enclosing entities a scene's tables hold (MAX_ENC_BOXES - 1)
BSDF_DIELECTRIC = 1  # include/igx_scene.h: IGX_BSDF_DIELECTRIC


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def render(device, scene, opts, params):
    device.upload(scene)
    for k, v in {**DEFAULTS, **opts}.items():
        device.set_option(k, v)
    device.clear()
    device.reset_stats()
    for p in params:
        device.render_iterations(p, ITERS)
    fb = device.framebuffer(params[0].width * params[0].height * 3)[0].copy()
    return fb, device.stats()


def frame(w=64, h=64, tile=None):
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = w, h, SPI
    if tile:
        p.tile_size, p.tile_offset, p.tile_stride = tile
    return p


def assert_store_phase_equal(device, scene, opts, params=None):
    """Option 0 against 1: film, ray counts, surviving paths; with 1 every
    k_extend launch ran a shape, with 0 none."""
    params = params or [frame()]
    try:
        off, s_off = render(device, scene, {**opts, "extend_shapes": 0}, params)
        on, s_on = render(device, scene, {**opts, "extend_shapes": 1}, params)
    finally:
        for k, v in DEFAULTS.items():
            device.set_option(k, v)
    np.testing.assert_array_equal(off, on, err_msg=str(opts))
    assert off.sum() > 0 and np.isfinite(off).all()
    for k in COUNTS:
        assert s_on[k] == s_off[k], (opts, k, s_on[k], s_off[k])
    assert list(s_off["launches_extend_shaped"]) == [0, 0], opts
    assert s_on["launches_extend"] == s_off["launches_extend"] > 0, opts
    assert sum(s_on["launches_extend_shaped"]) == s_on["launches_extend"], (opts, list(s_on["launches_extend_shaped"]))
    return s_on


@pytest.fixture(scope="module")
def diamond(root):
    return ignis_amd.Scene.from_file(os.path.join(root, "scenes", "diamond_scene.json"))


def test_diamond(device, diamond):
    st = assert_store_phase_equal(device, diamond, {})
    assert st["extend_block_threads"] == 1024
    assert st["extend_paths_out"] > 0 and st["shadow_rays"] > 0


def test_partial_groups(device, diamond):
    """50 x 38 pixels x spi 8 x 3 iterations = 45600 paths: no multiple of 64
    per shard, so the last group of a shard has idle lanes."""
    assert (50 * 38 * SPI * ITERS) % (64 * 64) != 0 and (50 * 38 * SPI) % 64 != 0
    assert_store_phase_equal(device, diamond, {}, [frame(50, 38)])


def test_wavefront_to_the_last_path(device, diamond):
    assert_store_phase_equal(device, diamond, {"tail_threshold": 0})


def test_lds256_layout(device, diamond):
    st = assert_store_phase_equal(device, diamond, {"lds_shading": 0, "tail_threshold": 0})
    assert st["extend_block_threads"] == 256


@pytest.mark.parametrize("concurrent", [0, 1])
@pytest.mark.parametrize("budget", ["capacity", "slot_budget_mb"])
def test_several_chunks(device, diamond, budget, concurrent):
    """Slots too small for the frame, so it runs as several chunks, in sequence
    or overlapped.  An explicit slot budget never cuts a chunk below 2^20 paths
    (host/render_plan.h), so 1 MB splits the 3.5 M paths of a 384 x 384 film
    (two pixel runs per iteration); on the 64 x 64 film the slot's path
    capacity does (8192 paths: four chunks per iteration)."""
    params = [frame(384, 384)] if budget == "slot_budget_mb" else None
    small = {"slot_budget_mb": 1} if budget == "slot_budget_mb" else {"capacity": 8192}
    whole = assert_store_phase_equal(device, diamond, {"tail_threshold": 0, "concurrent_chunks": concurrent}, params)
    st = assert_store_phase_equal(device, diamond, {"tail_threshold": 0, "concurrent_chunks": concurrent, **small}, params)
    assert st["launches_extend"] > whole["launches_extend"], (st["launches_extend"], whole["launches_extend"])
    for k in COUNTS:
        assert st[k] == whole[k], k


@pytest.mark.parametrize("optimistic", [0, 1])
def test_shadow_modes(device, diamond, optimistic):
    assert_store_phase_equal(device, diamond, {"shadow_optimistic": optimistic, "tail_threshold": 0})


def test_tile_shard(device, diamond):
    assert_store_phase_equal(device, diamond, {"tail_threshold": 0}, [frame(tile=(8, off, 2)) for off in (0, 1)])


@pytest.mark.parametrize("name", ["primitives.json", "s_deep.json"])
def test_global_tables(device, root, name):
    """Scenes whose tables stay in global memory (the third layout);
    primitives.json has no enclosing entity: the class pass has no box."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    st = assert_store_phase_equal(device, sc, {"tail_threshold": 0})
    assert st["lds_scene_bytes"] == 0 and st["extend_block_threads"] == 256


def many_diamonds(root, n):
    """The diamond scene with n small diamonds on a grid in front of the back
    wall instead of its three: closed dielectric meshes whose boxes keep apart
    from each other and from the walls, so the first MAX_ENCLOSING of them
    become enclosing entities."""
    with open(os.path.join(root, "scenes", "diamond_scene.json")) as f:
        sc = json.load(f)
    sc["entities"] = [e for e in sc["entities"] if e["shape"] != "Diamond"]
    side = int(np.ceil(np.sqrt(n)))
    s = 0.2
    for k in range(n):
        x, y = (k % side - (side - 1) / 2) * 0.2, (k // side - (side - 1) / 2) * 0.2
        sc["entities"].append({"bsdf": "mat-Diamond", "name": f"D{k}", "shape": "Diamond",
                               "transform": [s, 0, 0, x, 0, s, 0, y, 0, 0, s, 0, 0, 0, 0, 1]})
    return ignis_amd.Scene.from_string(json.dumps(sc), os.path.join(root, "scenes"))


def enclosing_count(scene):
    """scene_tables' rule for enclosing entities, on the scene's entity boxes."""
    d = scene.desc
    lo = np.array([list(d.entities[e].bbox_min) for e in range(d.num_entities)])
    hi = np.array([list(d.entities[e].bbox_max) for e in range(d.num_entities)])
    margin = 1e-4 * max(float(np.max(np.array(list(d.scene_bbox_max)) - np.array(list(d.scene_bbox_min)))), 1e-6)
    n = 0
    for e in range(d.num_entities):
        if d.materials[d.entities[e].material].bsdf_type != BSDF_DIELECTRIC:
            continue
        others = [o for o in range(d.num_entities) if o != e]
        apart = all(not all(lo[o][a] <= hi[e][a] + margin and lo[e][a] <= hi[o][a] + margin for a in range(3)) for o in others)
        n += apart
    return n


def test_most_enclosing_entities(device, root):
    """36 diamonds apart: the tables take the first MAX_ENCLOSING, so the class
    pass runs over the largest box count a scene can have."""
    sc = many_diamonds(root, 36)
    assert enclosing_count(sc) == 36 > MAX_ENCLOSING
    assert_store_phase_equal(device, sc, {"tail_threshold": 0})
