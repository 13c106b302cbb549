"""k_extend's wide LDS layout (option lds_shading): one 1024-thread block per
CU with the shading tables (entity records, per-face shading records, face
normals, materials, lights, enclosing indices) staged in LDS behind the
traversal tables, against today's 256-thread kernel that reads them from
global memory.  The staged tables hold the same values, so every image, AOV
and ray count is the same bit for bit, under every schedule; a scene whose
tables do not fit (or lack the per-face tables) keeps today's layout."""
import os

import numpy as np
import pytest

import ignis_amd

pytestmark = pytest.mark.gpu

W, H, SPI, ITERS = 112, 80, 4, 3


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


def load(root, name):
    return ignis_amd.Scene.from_file(os.path.join(root, "scenes", name))


def render(device, scene, upload=True):
    """3 iterations in one call; the film, the ray counts and the layout in effect."""
    if upload:
        device.upload(scene)
    device.clear()
    device.reset_stats()
    p = ignis_amd.RenderParams()
    p.width, p.height, p.spi = W, H, SPI
    device.render_iterations(p, ITERS)
    fb = device.framebuffer(W * H * 3)[0].copy()
    st = device.stats()
    return fb, (st["camera_rays"], st["bounce_rays"], st["shadow_rays"]), (st["lds_shading_bytes"], st["extend_block_threads"])


@pytest.mark.parametrize("name", ["diamond_scene.json", "primitives.json", "materials.json"])
@pytest.mark.parametrize("tail", [-1, 0, 1 << 30])
@pytest.mark.parametrize("fuse", [0, 1])
def test_on_equals_off(device, root, name, tail, fuse):
    """lds_shading 0 and 1 render the same framebuffer with the same ray
    counts: BVH2 with path classes A/B/C and basic shading (diamond, which
    runs the wide kernel), and two scenes whose traversal tables exceed
    lds_scene_max and so keep today's layout whatever the option says
    (primitives: 4-wide nodes, spheres; materials: the full shading variant;
    test_full_shading_variant_runs_wide and test_aovs run that variant wide);
    with no tail kernel, the whole chunk in the tail kernel and the
    automatic threshold; with and without fused generation."""
    sc = load(root, name)
    res = []
    try:
        device.set_option("tail_threshold", tail)
        device.set_option("fuse_generate", fuse)
        for on in (0, 1):
            device.set_option("lds_shading", on)
            res.append(render(device, sc))
    finally:
        device.set_option("lds_shading", -1)
        device.set_option("fuse_generate", 1)
        device.set_option("tail_threshold", -1)
    (img0, cnt0, lay0), (img1, cnt1, lay1) = res
    assert lay0 == (0, 256), lay0
    if name == "diamond_scene.json":  # not vacuous: the wide layout is in effect
        assert lay1[0] > 0 and lay1[1] == 1024, lay1
    assert np.array_equal(img0, img1), f"{name}: layout with lds_shading 1 = {lay1}"
    assert cnt0 == cnt1, f"{name}: layout with lds_shading 1 = {lay1}"
    assert img0.sum() > 0


def test_full_shading_variant_runs_wide(device, root):
    """The full-shading instantiation of the wide kernel: the diamond uploaded
    with option full_shading 1 fits like the plain diamond, so lds_shading 1
    runs the 1024-thread kernel of variant bit 2, and renders what the
    256-thread one renders (primitives.json and materials.json keep their
    tables in global memory, so they check the fallback only)."""
    sc = load(root, "diamond_scene.json")
    res = []
    try:
        device.set_option("full_shading", 1)
        for on in (0, 1):
            device.set_option("lds_shading", on)
            res.append(render(device, sc))
    finally:
        device.set_option("lds_shading", -1)
        device.set_option("full_shading", 0)
        device.upload(sc)
    assert res[0][2] == (0, 256), res[0][2]
    assert res[1][2][0] > 0 and res[1][2][1] == 1024, res[1][2]
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    assert res[0][0].sum() > 0


def test_auto_layout_is_reported(device, root):
    """Whichever layout auto chooses, the statistics report a consistent one."""
    device.set_option("lds_shading", -1)
    _, _, (sh_bytes, threads) = render(device, load(root, "diamond_scene.json"))
    assert (sh_bytes > 0 and threads == 1024) or (sh_bytes == 0 and threads == 256), (sh_bytes, threads)


def test_byte_cap_falls_back(device, root):
    """lds_shading_max below the tables' size keeps today's layout, same image."""
    sc = load(root, "diamond_scene.json")
    try:
        device.set_option("lds_shading", 1)
        ref, cnt, lay = render(device, sc)
        assert lay[0] > 1024 and lay[1] == 1024, lay
        device.set_option("lds_shading_max", 1024)
        img, cnt2, lay2 = render(device, sc, upload=False)
        assert lay2 == (0, 256), lay2
        # lifting the cap restores the wide layout without an upload
        device.set_option("lds_shading_max", 48 * 1024)
        img3, cnt3, lay3 = render(device, sc, upload=False)
        assert lay3 == lay
    finally:
        device.set_option("lds_shading_max", 48 * 1024)
        device.set_option("lds_shading", -1)
    assert np.array_equal(ref, img) and np.array_equal(ref, img3)
    assert cnt == cnt2 == cnt3


@pytest.mark.parametrize("name", ["diamond_scene.json", "materials.json"])
def test_missing_face_tables_fall_back(device, root, name):
    """Without the face-normal table or the per-face shading records (options
    face_normals / face_shade 0, next upload) the scene keeps today's layout
    and renders the image the wide layout renders with both."""
    sc = load(root, name)
    imgs, lays = [], []
    try:
        device.set_option("lds_shading", 1)
        for fnt, fsh in ((1, 1), (0, 0), (1, 0), (0, 1)):
            device.set_option("face_normals", fnt)
            device.set_option("face_shade", fsh)
            img, _, lay = render(device, sc)
            imgs.append(img)
            lays.append(lay)
    finally:
        device.set_option("face_normals", 1)
        device.set_option("face_shade", 1)
        device.set_option("lds_shading", -1)
        device.upload(sc)
    if name == "diamond_scene.json":  # with both tables the diamond runs the wide layout
        assert lays[0][0] > 0 and lays[0][1] == 1024, lays
    else:  # materials.json: 108 KB of traversal tables, global under the default lds_scene_max
        assert (lays[0][0] > 0) == (lays[0][1] == 1024), lays
    for lay in lays[1:]:
        assert lay == (0, 256), lays
    for img in imgs[1:]:
        assert np.array_equal(imgs[0], img), lays
    assert imgs[0].sum() > 0


def test_instrumented_variant(device, root):
    """The instrumented (STATS) instantiation of the wide kernel renders the
    framebuffer of the plain one."""
    sc = load(root, "diamond_scene.json")
    res = []
    try:
        device.set_option("lds_shading", 1)
        for inst in (0, 1):
            device.set_option("instrument", inst)
            res.append(render(device, sc))
    finally:
        device.set_option("instrument", 0)
        device.set_option("lds_shading", -1)
    assert res[1][2][1] == 1024, res[1][2]
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]


def test_aovs(device, root):
    """The film and both MIS AOVs of an aov_mis scene, staging on and off."""
    sc = load(root, "diamond_scene_uniform.json")
    assert sc.desc.technique.aov_mis == 1
    out = []
    try:
        for on in (0, 1):
            device.set_option("lds_shading", on)
            film, cnt, lay = render(device, sc)
            aovs = [device.framebuffer(W * H * 3, n)[0].copy() for n in ("Direct Weights", "NEE Weights")]
            out.append((film, aovs, cnt, lay))
    finally:
        device.set_option("lds_shading", -1)
    # the diamond's tables with the AOVs on: the full-shading wide kernel
    assert out[0][3] == (0, 256), out[0][3]
    assert out[1][3][0] > 0 and out[1][3][1] == 1024, out[1][3]
    msg = f"layout with lds_shading 1 = {out[1][3]}"
    assert np.array_equal(out[0][0], out[1][0]), msg
    assert np.array_equal(out[0][1][0], out[1][1][0]), msg
    assert np.array_equal(out[0][1][1], out[1][1][1]), msg
    assert out[0][2] == out[1][2], msg
    assert out[0][1][0].sum() > 0 and out[0][1][1].sum() > 0
