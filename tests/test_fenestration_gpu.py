"""tensortree_eval, klems_eval and their pdf and sample in the shipped shade_step
against the float64 restatement of the reference (tests/fenestration_ref.py),
per ray, with the machinery of tests/test_bsdf_gpu.py: one rotated rectangle,
2048 listed rays from both sides; (a) eval under a point light at three places,
(b) the MIS AOVs through the replayed cameras, (c) the sampled direction and
weight seen in a gradient environment map."""
import numpy as np
import pytest

import bsdf_cases as K
import bsdf_ref as B
import fenestration_cases as FC
import ignis_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    d = ignis_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fenestration")


@pytest.fixture(scope="module")
def env_map(tmp):
    return K.write_gradient_map(tmp / "gradient16x8.exr")


@pytest.mark.parametrize("name", list(FC.CASES))
def test_device_matches_the_reference(device, tmp, env_map, name):
    failed = []
    for obs, light in FC.RUNS:
        if obs == "mis":
            got, want = FC.camera_mis(K.camera_render_device(device), name, tmp)
        else:
            sc, rays, want = FC.case(name, obs, light, tmp, env_map)
            got = K.render_device(device, sc, obs, rays)
        for key, (w, stable) in want.items():
            assert stable.mean() >= 0.98, (name, key, stable.mean())
            assert np.abs(w[stable]).max() > 0, (name, key)
            ok, dev = B.check(got[key], w, stable, FC.ALLOWED[key])
            print(f"{name} {key} {light or ''}: deviation {dev:.3e}")
            if not ok:
                failed.append((key, light, dev))
    assert not failed, (name, failed)


def test_generic_kernel_renders_the_same_film(device, tmp, env_map):
    """Observable (a) once more with extend_shapes 0: bit for bit the default schedule's film."""
    sc, rays, _ = FC.case("mixed_t4", "eval", "near", tmp, env_map)
    try:
        base = K.render_device(device, sc, "eval", rays)["eval"]
        other = K.render_device(device, sc, "eval", rays, {"extend_shapes": 0})["eval"]
    finally:
        device.set_option("extend_shapes", -1)
    assert base.sum() > 0
    np.testing.assert_array_equal(base, other)
