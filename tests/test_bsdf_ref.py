"""The float64 restatement of the shading models (tests/bsdf_ref.py) on the CPU:
its Lambert against closed forms, the share of rays it can replay, the mutants
its tolerance must catch, and the CPU oracle against it per ray."""
import math

import numpy as np
import pytest

import bsdf_cases as K
import bsdf_ref as B
import image_ref as IR


@pytest.fixture(scope="module")
def env_map(tmp_path_factory):
    return K.write_gradient_map(tmp_path_factory.mktemp("bsdf") / "gradient16x8.exr")


def all_runs():
    return [(name, obs, light) for name in K.NON_DELTA + K.DELTA for obs, light in K.runs(name)]


def test_lambert_closed_forms(env_map):
    """kd |cos| / pi under the point light, its MIS weights under the constant
    sky, and kd L(d) at the cosine-sampled direction d, written out by hand."""
    kd = np.array(K.BSDFS["lambert"]["reflectance"], np.float32).astype(np.float64)  # the record is float32
    t = K.draws().astype(np.float64)
    for light in K.LIGHT_PLACES:
        sc, rays, want = K.case("lambert", "eval", light, env_map)
        r = K.replay(sc, rays)
        n = K.face_normal(sc.desc)
        # the hit point lies on the face, one unit along the ray (the float32 origin is off the
        # float64 one by 2^-24 of its size, and a ray at |cos| 0.02 turns that into 50 times as much)
        np.testing.assert_allclose(np.linalg.norm(r.point - r.org, axis=1), 1, atol=1e-5)
        to_light = np.array(sc.desc.lights[0].origin[:], np.float64) - r.point
        d2 = (to_light ** 2).sum(axis=1)
        cos = np.abs(to_light @ n) / np.sqrt(d2)
        assert ((to_light @ n > 0).all() if light != "below" else (to_light @ n < 0).all())
        closed = kd * (cos / math.pi / d2)[:, None] * np.array(K.LIGHT_INTENSITY)
        np.testing.assert_allclose(want["eval"][0], closed, rtol=1e-6)  # the light's position is float32
    sc, rays, want = K.case("lambert", "mis", None, env_map)
    r = K.replay(sc, rays)
    side = np.where(r.surf.entering, 1.0, -1.0)[:, None] * K.face_normal(sc.desc)
    wi = B.equal_area_square_to_sphere(t[:, 0], t[:, 1])
    np.testing.assert_allclose(np.linalg.norm(wi, axis=1), 1, atol=1e-12)
    c = (wi * side).sum(axis=1)
    nee = kd * (np.abs(c) / math.pi * 4 * math.pi / (1 + 4 * np.maximum(c, 0)))[:, None]
    np.testing.assert_allclose(want["nee_weight"][0], nee, rtol=1e-12)
    cz = np.sqrt(t[:, 3])  # the bounce draws after NEE's two: u = t[2], v = t[3]
    np.testing.assert_allclose(want["direct_weight"][0], kd * (1 / (1 + 1 / (4 * cz)))[:, None], rtol=1e-12)
    sc, rays, want = K.case("lambert", "sampled", None, env_map)
    r = K.replay(sc, rays)
    f = B.Frame(np.where(r.surf.entering[:, None], 1.0, -1.0) * K.face_normal(sc.desc))
    s, phi = np.sqrt(1 - t[:, 1]), 2 * math.pi * t[:, 0]
    d = f.to_world(B.vec(s * np.cos(phi), s * np.sin(phi), np.sqrt(t[:, 1])))
    np.testing.assert_allclose(want["sampled"][0], kd * IR.env_radiance(sc.desc, d)[0], rtol=1e-12)
    assert r.surf.entering.mean() == 0.5


@pytest.mark.parametrize("name", K.NON_DELTA + K.DELTA)
def test_replay_keeps_98_percent_of_the_rays(env_map, name):
    for obs, light in K.runs(name):
        for key, (want, stable, _) in K.case(name, obs, light, env_map)[2].items():
            assert np.isfinite(want).all(), (name, key, light)
            assert stable.mean() >= 0.98, (name, key, light, stable.mean())
            assert np.abs(want[stable]).max() > 0, (name, key, light)


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_tolerance_catches_the_mutant(env_map, mutant):
    """check(mutant's output, reference's output) fails on some case of some
    observable, with the device's allowance and with the oracle's."""
    for measured in (K.MEASURED_DEVICE, K.MEASURED_ORACLE):
        caught = []
        for name, obs, light in all_runs():
            ref = K.case(name, obs, light, env_map)[2]
            mut = K.case(name, obs, light, env_map, mutant)[2]
            # the reference's own stable rays and classes judge the mutant's output
            want = {k: (w, st & mut[k][1], ill) for k, (w, st, ill) in ref.items()}
            caught += [(name, light, cls, dev) for cls, dev, ok in K.judge(name, {k: v[0] for k, v in mut.items()}, want, measured) if not ok]
        print(mutant, "caught by", len(caught), "comparisons; largest", max(caught, key=lambda c: c[3], default=None))
        assert caught, mutant


@pytest.mark.parametrize("name", K.NON_DELTA + K.DELTA)
def test_oracle_matches_the_reference(env_map, name):
    failed = []
    for obs, light in K.runs(name):
        sc, rays, want = K.case(name, obs, light, env_map)
        for cls, dev, ok in K.judge(name, K.render_oracle(sc, obs, rays), want, K.MEASURED_ORACLE):
            print(f"{name} {cls} {light or ''}: deviation {dev:.3e}")
            if not ok:
                failed.append((cls, light, dev))
    assert not failed, (name, failed)
