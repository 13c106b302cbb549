"""host/image_texture.h (the texture arithmetic the device runs, compiled here
for the host by tests/native/image_texture_check.cpp) against the float64
restatement of texture/image.art in tests/image_ref.py: three filters x three
wraps (and a split wrap) under a non-identity transform, on a 5 x 3 and an
8 x 8 image, at uv inside and outside [0, 1] and negative.  Two comparisons: one
whose restatement takes the header's float32 coordinate steps and holds the
weights and the blend to 4 ulps, and one in float64 throughout with the
coordinate rounding allowed for, which holds the coordinate steps.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import image_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ignis-masterthesis_amd", "host")
TRANSFORM = [1.7, -0.4, 0.13, 0.3, 2.2, -0.71]  # rotates, scales and shifts: leaves [0, 1] on every side
IDENTITY = [1, 0, 0, 0, 1, 0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tex") / "image_texture_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", HOST,
                    os.path.join(ROOT, "tests", "native", "image_texture_check.cpp"), "-o", path], check=True)
    return path


def run(exe, tmp_path, texels, fmt, filt, wrap_u, wrap_v, m, uv):
    h, w = texels.shape[:2]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<7i", w, h, fmt, filt, wrap_u, wrap_v, len(uv)) + np.asarray(m, np.float32).tobytes() +
                    np.ascontiguousarray(texels).tobytes() + np.ascontiguousarray(uv, np.float32).tobytes())
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.frombuffer(dst.read_bytes(), np.float32).reshape(-1, 4)


def uv_samples(rng):
    """A grid over about [-2.3, 3.1]^2 plus random points, float32."""
    g = np.linspace(-2.3017, 3.1049, 41)  # off the texel borders of both image sizes
    uv = np.stack(np.meshgrid(g, g), axis=2).reshape(-1, 2)
    return np.concatenate([uv, rng.uniform(-4, 4, (600, 2)), rng.uniform(0, 1, (300, 2))]).astype(np.float32)


def images(rng):
    f53 = rng.random((3, 5, 4), dtype=np.float32) * 10  # 5 wide, 3 high
    f88 = rng.random((8, 8, 4), dtype=np.float32)
    b88 = rng.integers(0, 256, (8, 8, 4)).astype(np.uint8)
    m53 = rng.integers(0, 256, (3, 5)).astype(np.uint8)
    return {"float5x3": (f53, 2), "float8x8": (f88, 2), "rgba8x8": (b88, 0), "mono5x3": (m53, 1)}


@pytest.mark.parametrize("wraps", [(IR.REPEAT, IR.REPEAT), (IR.CLAMP, IR.CLAMP), (IR.MIRROR, IR.MIRROR), (IR.MIRROR, IR.CLAMP)],
                         ids=["repeat", "clamp", "mirror", "mirror_clamp"])
@pytest.mark.parametrize("filt", [IR.NEAREST, IR.BILINEAR, IR.BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_header_against_float64(exe, tmp_path, filt, wraps):
    rng = np.random.default_rng(17)
    uv = uv_samples(rng)
    for name, (texels, fmt) in images(rng).items():
        tex = IR.texels_float64(texels)
        for m in (TRANSFORM, IDENTITY):
            got = run(exe, tmp_path, texels, fmt, filt, wraps[0], wraps[1], m, uv)
            # the header transforms in float32; the restatement takes the float32 result, so that
            # both choose texels from the same coordinates
            m32 = np.asarray(m, np.float32)
            tu = (m32[0] * uv[:, 0] + m32[1] * uv[:, 1]) + m32[2] * np.float32(1)
            tv = (m32[3] * uv[:, 0] + m32[4] * uv[:, 1]) + m32[5] * np.float32(1)
            assert tu.dtype == np.float32
            # ... and finds the texel and the fraction in float32 (u * width - 0.5), as written: the
            # restatement takes those two steps in float32 too and everything after them in float64
            stable = IR.choice_is_stable(tex, filt, wraps[0], wraps[1], tu.astype(np.float64), tv.astype(np.float64), eps=1e-5)
            want = IR.sample(tex, filt, wraps[0], wraps[1], tu, tv, dtype=np.float32)
            assert stable.mean() > 0.97, (name, stable.mean())
            err = np.abs(got[stable] - want[stable]).max()
            ulp = float(np.spacing(np.float32(tex.max())))
            print(f"{name} transform {m is TRANSFORM}: max err {err:.3e} ({err / ulp:.2f} ulp of the largest texel)")
            if filt == IR.NEAREST:
                np.testing.assert_array_equal(got[stable], want[stable].astype(np.float32))
            else:
                assert err <= 4 * ulp, (name, err, ulp)
            # The comparison above shares the float32 coordinate steps with the header, so it does not
            # hold them to anything.  This one does: the restatement in float64 from the float32 uv
            # on.  The header rounds the transform's two products and two sums and then u * w and
            # - 0.5, six roundings of at most half a spacing of the largest coordinate (in texels);
            # a lookup moves by at most the texel range per texel of coordinate error, on two axes.
            exact_u, exact_v = IR.transform_uv(np.asarray(m, np.float32).astype(np.float64), uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64))
            pure = IR.sample(tex, filt, wraps[0], wraps[1], exact_u, exact_v)
            h, w = tex.shape[:2]
            reach = max(np.abs(exact_u).max() * w, np.abs(exact_v).max() * h) + 1
            delta = 3 * float(np.spacing(np.float32(reach)))
            steady = IR.choice_is_stable(tex, filt, wraps[0], wraps[1], exact_u, exact_v, eps=2e-5)
            assert delta / min(w, h) < 2e-5 and steady.mean() > 0.95
            pure_err = np.abs(got[steady] - pure[steady]).max()
            print(f"{name} pure float64: max err {pure_err:.3e}, allowed {2 * delta * tex.max() + 4 * ulp:.3e}")
            if filt == IR.NEAREST:
                np.testing.assert_array_equal(got[steady], pure[steady].astype(np.float32))
            else:
                assert pure_err <= 2 * delta * tex.max() + 4 * ulp, (name, pure_err)
