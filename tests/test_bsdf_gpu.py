"""bsdf_eval, bsdf_pdf and bsdf_sample of the shipped shade_step against the
float64 restatement of the reference's shading models (tests/bsdf_ref.py), per
ray: renders of depth 2 on one rotated rectangle (tests/bsdf_cases.py), whose
film is one NEE term plus one bounce that leaves the scene.  The rays come as a
list, except for the MIS AOVs, which ray-list mode does not write: those are
rendered through a camera whose jitter is replayed."""
import numpy as np
import pytest

import bsdf_cases as K
import bsdf_ref as B
import ignis_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def env_map(tmp_path_factory):
    return K.write_gradient_map(tmp_path_factory.mktemp("bsdf") / "gradient16x8.exr")


@pytest.mark.parametrize("name", K.NON_DELTA + K.DELTA)
def test_device_matches_the_reference(device, env_map, name):
    """Observable (a) eval under a point light at three places, (b) the MIS
    AOVs under a constant sky (bsdf_pdf in "NEE Weights", the sample's pdf and
    weight in "Direct Weights"), (c) the sampled direction and weight seen in a
    gradient environment map; the delta models through (c) only."""
    failed = []
    for obs, light in K.runs(name):
        if obs == "mis":  # ray-list mode writes no AOVs: two small films through a camera instead
            got, want = K.camera_mis(K.camera_render_device(device), name)
        else:
            sc, rays, want = K.case(name, obs, light, env_map)
            got = K.render_device(device, sc, obs, rays)
        assert all(stable.mean() >= 0.98 for _, stable, _ in want.values())
        for cls, dev, ok in K.judge(name, got, want, K.MEASURED_DEVICE):
            print(f"{name} {cls} {light or ''}: deviation {dev:.3e}")
            if not ok:
                failed.append((cls, light, dev))
    assert not failed, (name, failed)


@pytest.mark.parametrize("name", ["aniso_alu", "p_glass"])
def test_generic_kernel_renders_the_same_film(device, env_map, name):
    """Observable (a) once more with extend_shapes 0: bit for bit the default schedule's film."""
    sc, rays, _ = K.case(name, "eval", "near", env_map)
    try:
        base = K.render_device(device, sc, "eval", rays)["eval"]
        other = K.render_device(device, sc, "eval", rays, {"extend_shapes": 0})["eval"]
    finally:
        device.set_option("extend_shapes", -1)
    assert base.sum() > 0
    np.testing.assert_array_equal(base, other)
