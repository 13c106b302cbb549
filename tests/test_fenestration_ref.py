"""The float64 restatement of the measured BSDFs (tests/fenestration_ref.py) on
the CPU: enough stable rays in every per-ray case, every mutant of its own
displaces some observable by far more than the device tests allow, known
answers by quadrature, and the expected images of the four tensor tree
evaluation scenes against Radiance's."""
import os

import numpy as np
import pytest

import bsdf_cases as K
import bsdf_ref as B
import evalref as E
import fenestration_cases as FC
import fenestration_ref as F
import ignis_amd


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fenestration_ref")


@pytest.fixture(scope="module")
def env_map(tmp):
    return K.write_gradient_map(tmp / "gradient16x8.exr")


@pytest.mark.parametrize("name", list(FC.CASES))
def test_cases_are_stable_and_alive(tmp, env_map, name):
    """At least 98 % of the 2048 rays of every case keep 1e-5 away from every cell boundary
    and threshold, and every observable is non-zero on at least 20 of them."""
    for obs, light in FC.RUNS:
        sc, rays, want = FC.case(name, obs, light, tmp, env_map)
        for key, (w, stable) in want.items():
            assert stable.mean() >= 0.98, (name, key, stable.mean())
            assert np.isfinite(w).all()
            assert (np.abs(w[stable]).max(axis=1) > 0).sum() >= 20, (name, key)


# mutant -> the case and observable that show it
SHOWN_BY = {
    "in_out_exchanged": [("mixed_t4", "eval", "near"), ("klems_full", "eval", "near")],
    "transmission_exchanged": [("mixed_t3", "eval", "below"), ("klems_small", "eval", "below")],
    "leaf_bits_reversed": [("mixed_t4", "eval", "near"), ("d3_t3_refl", "eval", "near")],
    "klems_row_col_exchanged": [("klems_small", "eval", "near")],
    "k_fi_without_flip": [("klems_full", "eval", "near")],
    "third_draw_unconditional": [("d2_trans", "sampled", None), ("d2_trans", "mis", None)],
}


def test_every_mutant_is_listed():
    assert set(SHOWN_BY) == set(F.MUTANTS) and len(F.MUTANTS) >= 6


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_mutants_move_an_observable(tmp, env_map, mutant):
    """Each slip displaces an observable of each listed case by more than SMALLEST_MUTANT, which
    is far above the largest deviation the device tests allow: no tolerance there can hide one."""
    assert max(FC.ALLOWED.values()) < FC.SMALLEST_MUTANT / 100
    for name, obs, light in SHOWN_BY[mutant]:
        sc, rays, want = FC.case(name, obs, light, tmp, env_map)
        _, _, moved = FC.case(name, obs, light, tmp, env_map, mutant=mutant)
        shown = 0.0
        for key, (w, stable) in want.items():
            m, mstable = moved[key]
            shown = max(shown, B.deviation(m, w, stable & mstable))
        print(f"{mutant}: {name} {obs} {light or ''} displaced by {shown:.3g}")
        assert shown > FC.SMALLEST_MUTANT, (mutant, name, obs, shown)


# ---- known answers -----------------------------------------------------------------------------
def _integral(path, kind, out_side, in_side):
    """The integral of eval (f times |cos|) over the incoming hemisphere `in_side` for a fixed outgoing
    direction on `out_side` of a window in the z = 0 plane, up = +z (the identity frame)."""
    doc = {"bsdfs": [{"type": kind, "name": "w", "filename": str(path)}], "shapes": [{"type": "rectangle", "name": "r"}],
           "entities": [{"name": "e", "shape": "r", "bsdf": "w"}]}
    sc = ignis_amd.Scene.from_string(doc)
    d, w = F.hemisphere_grid()
    wi = d * [1, 1, in_side]
    wo = np.tile(B.normalize(np.array([0.3, -0.2, 0.9 * out_side])), (len(wi), 1))
    surf = B.Surface([0.0, 0.0, 1.0], -wo, None)
    bsdf = F.Measured(surf, sc.desc.materials[0], sc.desc.measured[0])
    assert bsdf.identity.all()
    return float((bsdf.eval(wi, wo)[:, 0] / np.abs(wi[:, 2]) * w).sum())


@pytest.mark.parametrize("out_side", [1, -1])
def test_constant_transmission_and_reflection_integrate_to_0_8(tmp, out_side):
    trans = os.path.join(FC.GOLDEN, "simple_tensor_trans.xml")
    refl = os.path.join(FC.GOLDEN, "simple_tensor_refl.xml")
    klems = tmp / "constant_klems.xml"
    klems.write_text(FC.constant_klems_xml(0.8 / np.pi))
    for path, kind, through in ((trans, "tensortree", True), (refl, "tensortree", False), (klems, "klems", True)):
        lit = _integral(path, kind, out_side, -out_side if through else out_side)
        dark = _integral(path, kind, out_side, out_side if through else -out_side)
        assert lit == pytest.approx(0.8, abs=1e-4), (path, lit)
        assert dark == 0.0, (path, dark)


# ---- expected images -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.EVAL_SCENES)
def test_expected_image_against_radiance(name):
    assert FC.BOUND["plane-array-tensortree-front"] == FC.BOUND["plane-array-tensortree-back"] == 2e-2
    q, masks = FC.expected_image(name)
    err, _ = E.error_image(q.astype(np.float32), FC.radiance_image(name))
    print(f"{name}: error_image(Q, Radiance) = {err:.4e}")
    assert np.isfinite(q).all() and all(m.sum() > 1000 for m in masks)
    assert err <= FC.BOUND[name]
    assert err == pytest.approx(FC.MEASURED_Q[name], rel=0.02)
