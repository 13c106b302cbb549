"""Copy the reference's tensor tree test data into tests/golden/fenestration/
(data fixtures only: BSDF XML files, one mesh, scene descriptions, Radiance's
reference images).

The 13 `scenes/radiance/simple_tensor_*.xml` files, `scenes/meshes/RoomWindow.obj`,
`plane-array-base.json` with the four `plane-array-tensortree*-{front,back}.json`
and their `ref-plane-array-tensortree*-rad.exr` images.  Everything lands in one
directory, so the paths inside the scene files are rewritten to bare file names;
nothing else changes.  The Klems files of the reference (0.2-0.85 MB each) are
not copied: the tests generate their Klems inputs (tests/fenestration_cases.py).
"""
import glob
import os
import re
import shutil
import sys

from make_eval_fixtures import REF, ROOT

OUT = os.path.join(ROOT, "tests", "golden", "fenestration")
SCENES = ["plane-array-base"] + [f"plane-array-tensortree{t}-{side}" for t in ("", "-t3") for side in ("front", "back")]


def main():
    if not os.path.isdir(REF):
        print("reference scenes not available; nothing to do", file=sys.stderr)
        return 1
    os.makedirs(OUT, exist_ok=True)
    copied = 0
    for src in sorted(glob.glob(os.path.join(REF, "radiance", "simple_tensor_*.xml"))) + [os.path.join(REF, "meshes", "RoomWindow.obj")]:
        shutil.copyfile(src, os.path.join(OUT, os.path.basename(src)))
        copied += 1
    for stem in SCENES:
        with open(os.path.join(REF, "evaluation", stem + ".json")) as f:
            text = f.read()
        text = re.sub(r'"\.\./(?:meshes|radiance)/([^"]+)"', r'"\1"', text)
        with open(os.path.join(OUT, stem + ".json"), "w") as f:
            f.write(text)
        copied += 1
        if stem != "plane-array-base":
            img = f"ref-{stem}-rad.exr"
            shutil.copyfile(os.path.join(REF, "evaluation", "references", img), os.path.join(OUT, img))
            copied += 1
    print(f"copied {copied} files into {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
