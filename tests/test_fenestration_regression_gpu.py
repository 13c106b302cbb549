"""Regression guard of the measured BSDFs: they are compiled into the full
shading variant only, so the diamond (basic variant) and scenes/principled.json
(full variant, no measured material) must render the film they rendered before.
tests/golden/fenestration/parent_films.npz holds both films, 64 x 64, two
iterations of 4 samples, as the library of the commit before this feature
rendered them on an MI355X (recorded with `IGX_LIB_PATH=<that library> python
tests/test_fenestration_regression_gpu.py <file.npz>`); the comparison is bit
for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fenestration", "parent_films.npz")
SCENES = {"diamond": "diamond_scene.json", "principled": "principled.json"}
SIZE, SPI, ITERATIONS = 64, 4, 2


def render_films():
    import ignis_amd

    out = {}
    dev = ignis_amd.Device(0)
    try:
        for name, file in SCENES.items():
            sc = ignis_amd.Scene.from_file(os.path.join(ROOT, "scenes", file))
            dev.upload(sc)
            dev.clear()
            for k in range(ITERATIONS):
                p = ignis_amd.RenderParams()
                p.width, p.height, p.spi, p.iteration = SIZE, SIZE, SPI, k
                dev.render(p)
            fb, it = dev.framebuffer(SIZE * SIZE * 3)
            assert it == ITERATIONS
            out[name] = fb.reshape(SIZE, SIZE, 3).copy()
    finally:
        dev.close()
    return out


@pytest.mark.gpu
def test_films_without_measured_bsdfs_are_unchanged():
    want = np.load(GOLDEN)
    got = render_films()
    for name in SCENES:
        assert np.isfinite(got[name]).all() and got[name].mean() > 0
        differ = int((got[name].view(np.uint32) != want[name].view(np.uint32)).sum())
        print(f"{name}: {differ} of {got[name].size} film values differ from the recorded film")
        np.testing.assert_array_equal(got[name], want[name])


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "ignis-masterthesis_amd"), ROOT]
    np.savez_compressed(sys.argv[1], **render_films())
