"""Every kernel the schedule options can choose, plain and instrumented.

The options below pick the k_extend layout and shape, the split schedule's
k_trace or k_trace_refill, the shadow kernel (grid-stride, persistent lanes,
if-if) and the tail kernel (k_finish, k_finish_pairs), each on LDS-staged and
on global tables; option "instrument" picks the counting instantiation of
each.  Which kernel runs never changes what is traced: within one upload all
films are bit-identical and the ray counts equal, and with "instrument" 1 the
counters show that the counting kernels ran."""
import os

import numpy as np
import pytest

import ignis_amd

pytestmark = pytest.mark.gpu

W, H, SPI = 112, 80, 4
ALL = 1 << 30  # tail threshold: the whole chunk goes to the tail kernel

# (row, options, needs LDS-staged tables); every row runs with tail_threshold 0 unless it says otherwise
ROWS = [
    ("wide shaped", {}, True),
    ("wide generic", {"extend_shapes": 0}, True),
    ("256-thread LDS shaped", {"lds_shading": 0}, True),
    ("256-thread LDS generic", {"lds_shading": 0, "extend_shapes": 0}, True),
    ("global fused shaped", {"lds_scene_max": 0}, False),
    ("global fused generic", {"lds_scene_max": 0, "extend_shapes": 0}, False),
    ("k_trace LDS", {"split": 1, "refill": 0}, True),
    ("k_trace global", {"lds_scene_max": 0, "split": 1, "refill": 0}, False),
    ("refill LDS", {"split": 1, "refill": 16}, True),
    ("refill global while-while", {"lds_scene_max": 0, "split": 1, "refill": 16, "shadow_ifif": 0}, False),
    ("refill global if-if", {"lds_scene_max": 0, "split": 1, "refill": 16, "shadow_ifif": 1}, False),
    ("LDS tail", {"tail_threshold": ALL}, True),
    ("global tail", {"lds_scene_max": 0, "tail_threshold": ALL, "tail_pairs": 0}, False),
    ("global tail pairs", {"lds_scene_max": 0, "tail_threshold": ALL, "tail_pairs": 1}, False),
]
ROW_DEFAULTS = {"lds_scene_max": 48 * 1024, "lds_shading": -1, "extend_shapes": -1, "split": -1, "refill": -1, "shadow_ifif": -1,
                "tail_threshold": 0, "tail_pairs": -1}

# (scene, options that apply at upload, node bytes to expect or None)
GROUPS = {
    "diamond": ("diamond_scene.json", {"full_shading": 0}, None),
    "diamond-full": ("diamond_scene.json", {"full_shading": 1}, None),
    "s_deep": ("s_deep.json", {"lds_scene_max": 0, "bvh_quantize": 0}, 128),
    "s_deep-q4": ("s_deep.json", {"lds_scene_max": 0, "bvh_quantize": 1}, 64),
}


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def render(device):
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, SPI
    device.render(p)
    return device.framebuffer(W * H * 3)[0].copy(), device.stats()


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_choice_renders_the_same(device, root, group):
    """One upload (films of different uploads are not compared: quantised
    nodes may differ in rare rays, test_quantised_nodes_match), every row
    with instrument 0 and 1: all films equal the first bit for bit, all ray
    counts are equal, and the instrumented runs counted node visits, launched
    no shape, and launched k_trace / the tail kernel where the row asks for them."""
    name, upload_opts, node_bytes = GROUPS[group]
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    global_only = name == "s_deep.json"  # its tables stay in global memory
    films = []
    try:
        device.set_option("concurrent_chunks", 0)
        for k, v in upload_opts.items():
            device.set_option(k, v)
        device.upload(sc)
        if node_bytes is not None:
            assert device.stats()["node_bytes"] == node_bytes
        for row, opts, needs_lds in ROWS:
            if needs_lds and global_only:
                continue
            for k, v in {**ROW_DEFAULTS, **opts}.items():
                device.set_option(k, 0 if global_only and k == "lds_scene_max" else v)
            for inst in (0, 1):
                device.set_option("instrument", inst)
                fb, st = render(device)
                films.append((f"{row}, instrument {inst}", fb, (st["camera_rays"], st["bounce_rays"], st["shadow_rays"])))
                if inst:
                    assert st["node_visits"] > 0 and st["shadow_node_visits"] > 0, row
                    assert list(st["launches_extend_shaped"]) == [0, 0], row
                    if opts.get("split") == 1:
                        assert st["launches_trace"] > 0, row
                    if opts.get("tail_threshold") == ALL:
                        assert st["launches_finish"] > 0, row
    finally:
        device.set_option("instrument", 0)
        device.set_option("concurrent_chunks", 1)
        device.set_option("full_shading", 0)
        device.set_option("bvh_quantize", -1)
        for k, v in ROW_DEFAULTS.items():
            device.set_option(k, -1 if k == "tail_threshold" else v)
    _, fb0, counts0 = films[0]
    assert fb0.sum() > 0
    for what, fb, counts in films[1:]:
        assert np.array_equal(fb0, fb), what
        assert counts == counts0, what
