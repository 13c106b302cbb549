"""Option "shadow_optimistic": the fused k_extend adds the colour of a class-A
shadow ray (one whose segment crosses no enclosing entity's box) to the
radiance slot itself and leaves the slot's previous value in the shadow
record; the shadow kernel stores that value back for the occluded rays and
touches nothing for the others.  Every slot sees the same float additions in
the same order, so the film must be bit-identical to the plain path (the
shadow kernel adds the colour of every unoccluded ray) under every schedule.
"""
import os

import numpy as np
import pytest

import ignis_amd

pytestmark = pytest.mark.gpu

W, H, SPI = 112, 80, 4
DEFAULTS = {"shadow_optimistic": -1, "tail_threshold": -1, "fuse_generate": 1, "concurrent_chunks": 1, "capacity": 0,
            "instrument": 0}


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def render(device, scene, opts, iterations=1, aovs=()):
    """(film, named AOV films, (camera, bounce, shadow) ray counts) of the scene under the options."""
    device.upload(scene)
    for k, v in {**DEFAULTS, **opts}.items():
        device.set_option(k, v)
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, SPI
    if iterations == 1:
        device.render(p)
    else:
        device.render_iterations(p, iterations)
    fb, it = device.framebuffer(W * H * 3)
    assert it == iterations
    extra = [device.framebuffer(W * H * 3, n)[0] for n in aovs]
    st = device.stats()
    return fb, extra, (st["camera_rays"], st["bounce_rays"], st["shadow_rays"])


def restore(device):
    for k, v in DEFAULTS.items():
        device.set_option(k, v)


def assert_on_equals_off(device, scene, opts, iterations=1):
    off, _, c_off = render(device, scene, {**opts, "shadow_optimistic": 0}, iterations)
    on, _, c_on = render(device, scene, {**opts, "shadow_optimistic": 1}, iterations)
    np.testing.assert_array_equal(off, on, err_msg=str(opts))
    assert c_on == c_off, opts
    assert off.sum() > 0 and c_off[2] > 0
    return off


@pytest.mark.parametrize("tail", [-1, 0, 1 << 30])
@pytest.mark.parametrize("name", ["diamond_scene.json", "materials.json"])
def test_on_equals_off(device, root, name, tail):
    """Bit identity and equal ray counts, option 1 against 0: wavefront with the
    automatic tail, wavefront to the last path, tail kernel only; generation
    fused into bounce 0 or by k_generate; concurrent or sequential chunks."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    try:
        films = [assert_on_equals_off(device, sc, {"tail_threshold": tail, "fuse_generate": fuse, "concurrent_chunks": conc})
                 for fuse in (1, 0) for conc in (1, 0)]
    finally:
        restore(device)
    for f in films[1:]:
        np.testing.assert_array_equal(films[0], f)


@pytest.mark.parametrize("conc", [1, 0])
@pytest.mark.parametrize("name", ["diamond_scene.json", "materials.json"])
def test_on_equals_off_chunked(device, root, name, conc):
    """Three iterations in chunks of 8192 paths (five chunks per iteration,
    the last one short): slots are reused by later chunks, chunks overlap."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))
    try:
        assert_on_equals_off(device, sc, {"capacity": 8192, "concurrent_chunks": conc, "tail_threshold": 0}, iterations=3)
        assert_on_equals_off(device, sc, {"capacity": 8192, "concurrent_chunks": conc}, iterations=3)
    finally:
        restore(device)


def test_undo_path_runs(device, root):
    """The instrumented kernels follow the option, and occluded class-A rays
    (whose slots the shadow kernel has to put back) are no accident of the
    case: with the wavefront running every bounce the instrumented k_shadow
    counts them per class.  The diamond scene, three iterations: its tables are
    LDS-staged, so it runs k_shadow (the persistent-lane kernel of
    materials.json keeps no per-class counters), and about 2 % of its class-A
    rays at this film are occluded."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "diamond_scene.json"))
    opts = {"tail_threshold": 0, "instrument": 1}
    try:
        off, _, c_off = render(device, sc, {**opts, "shadow_optimistic": 0}, iterations=3)
        occ_off = list(device.stats()["shadow_class_occluded"])
        on, _, c_on = render(device, sc, {**opts, "shadow_optimistic": 1}, iterations=3)
        st = device.stats()
    finally:
        restore(device)
    occ_on, rays = list(st["shadow_class_occluded"]), list(st["shadow_class_rays"])
    print("class-A/B shadow rays", rays, "occluded", occ_on)
    np.testing.assert_array_equal(off, on)
    assert c_on == c_off
    # the counters go by the class of a wave's group: a shard's one group with
    # both classes counts as A, and which rays it holds depends on the order of
    # the appends, so only the sum is the same from run to run
    assert sum(occ_on) == sum(occ_off)
    assert occ_on[0] >= 100, (occ_on, rays)  # measured: about 4000 of 172181 rays in class-A groups (2500 of 6012 in class B)


@pytest.mark.parametrize("tail", [-1, 0])
def test_forced_on_without_enclosing_entity(device, root, tail):
    """s_deep.json has no enclosing entity: every shadow ray is class A, many
    are occluded, and the persistent-lane k_shadow_refill's finish step does the
    undo.  Auto leaves the option off there; 1 forces it."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "s_deep.json"))
    try:
        off = assert_on_equals_off(device, sc, {"tail_threshold": tail})
        auto, _, _ = render(device, sc, {"tail_threshold": tail, "shadow_optimistic": -1})
    finally:
        restore(device)
    np.testing.assert_array_equal(off, auto)


def test_auto_is_off_with_mis_aovs(device, root):
    """With the MIS AOVs "NEE Weights" needs the colour in the shadow record:
    auto (-1) renders the film and both AOVs as 0 does."""
    sc = ignis_amd.Scene.from_file(os.path.join(root, "scenes", "primitives_aov.json"))
    assert sc.desc.technique.aov_mis == 1
    names = ("Direct Weights", "NEE Weights")
    try:
        off, a_off, c_off = render(device, sc, {"shadow_optimistic": 0}, aovs=names)
        auto, a_auto, c_auto = render(device, sc, {"shadow_optimistic": -1}, aovs=names)
    finally:
        restore(device)
    np.testing.assert_array_equal(off, auto)
    for x, y in zip(a_off, a_auto):
        np.testing.assert_array_equal(x, y)
        assert x.sum() > 0
    assert c_off == c_auto
