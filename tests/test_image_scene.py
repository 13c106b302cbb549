"""Image textures in the scene description: the loader reads `textures` of
type "image", a colour property may name one (diffuse `reflectance`, principled
`base_color`), the desc carries the image and texture tables with the
reference's defaults (pattern/ImagePattern.cpp:19-52), an in-memory object scene
gives the same desc as the JSON scene, the SceneDatabase seam carries the
tables, and everything else keeps its refusal.  CPU only."""
import os

import numpy as np
import pytest

import ignis_amd
import image_ref as IR
from ignis_amd import _native as N
from refdb import RefDatabase
from test_db_adapter import assert_desc_equal

BITMAP = os.path.join(IR.TEXTURES, "bitmap.png")
CONSTANT = os.path.join(IR.TEXTURES, "constant.exr")


def scene(textures, bsdfs):
    return {"textures": textures, "bsdfs": bsdfs, "shapes": [{"type": "rectangle", "name": "r"}],
            "entities": [{"name": "e%d" % i, "shape": "r", "bsdf": b["name"]} for i, b in enumerate(bsdfs)]}


def material_of(desc, entity):
    return desc.materials[desc.entities[entity].material]


def test_defaults_and_indices():
    doc = scene([{"type": "image", "name": "a", "filename": BITMAP},
                 {"type": "image", "name": "unused", "filename": "/nonexistent/never_read.png"},
                 {"type": "image", "name": "b", "filename": CONSTANT, "filter_type": "nearest", "wrap_mode": "clamp"}],
                [{"type": "diffuse", "name": "plain", "reflectance": [0.1, 0.2, 0.3]},
                 {"type": "diffuse", "name": "db", "reflectance": "b"},
                 {"type": "principled", "name": "pa", "base_color": "a"},
                 {"type": "diffuse", "name": "da", "reflectance": "a"}])
    sc = ignis_amd.Scene.from_string(doc)  # owns the desc
    d = sc.desc
    # textures and images appear in the order they are first used; an unused one is never read
    assert d.num_textures == 2 and d.num_images == 2
    plain, db, pa, da = (material_of(d, i) for i in range(4))
    assert plain.texture == N.TEXTURE_NONE
    assert (db.texture, db.tex_index, db.bsdf_type) == (N.TEXTURE_IMAGE, 0, 0)
    assert (pa.texture, pa.tex_index, pa.bsdf_type) == (N.TEXTURE_IMAGE, 1, 4)
    assert (da.texture, da.tex_index) == (N.TEXTURE_IMAGE, 1)
    tb, ta = d.textures[0], d.textures[1]
    assert (tb.image, tb.filter, tb.wrap_u, tb.wrap_v) == (0, N.FILTER_NEAREST, N.WRAP_CLAMP, N.WRAP_CLAMP)
    assert (ta.image, ta.filter, ta.wrap_u, ta.wrap_v) == (1, N.FILTER_BICUBIC, N.WRAP_REPEAT, N.WRAP_REPEAT)
    assert list(ta.transform) == [1, 0, 0, 0, 1, 0]
    assert (d.images[0].width, d.images[0].height, d.images[0].format) == (60, 40, N.IMAGE_FLOAT4)
    assert (d.images[1].width, d.images[1].height, d.images[1].format) == (8, 8, N.IMAGE_RGBA8)


def test_properties_are_honoured():
    doc = scene([{"type": "image", "name": "split", "filename": BITMAP, "filter_type": "bilinear", "wrap_mode_u": "mirror",
                  "wrap_mode_v": "clamp", "wrap_mode": "repeat",
                  "transform": [{"translate": [0.25, -0.5, 9]}, {"rotate": [0, 0, 90]}, {"scale": [2, 3, 1]}]},
                 {"type": "image", "name": "only_u", "filename": BITMAP, "wrap_mode_u": "clamp"},
                 {"type": "image", "name": "lin", "filename": BITMAP, "linear": True},
                 {"type": "image", "name": "matrix", "filename": BITMAP, "transform": [1, 2, 3, 4, 5, 6, 7, 8, 0, 0, 1, 0, 0, 0, 0, 1]}],
                [{"type": "diffuse", "name": n, "reflectance": n} for n in ("split", "only_u", "lin", "matrix")])
    sc = ignis_amd.Scene.from_string(doc)  # owns the desc
    d = sc.desc
    split, only_u, lin, matrix = (d.textures[i] for i in range(4))
    assert (split.filter, split.wrap_u, split.wrap_v) == (N.FILTER_BILINEAR, N.WRAP_MIRROR, N.WRAP_CLAMP)
    # T(0.25, -0.5) * Rz(90 deg) * S(2, 3): the 2x2 block and the x, y translation (inlineTransformAs2d)
    np.testing.assert_allclose(list(split.transform), [0, -3, 0.25, 2, 0, -0.5], atol=1e-6)
    # wrap_mode_u alone: v takes its own default, not wrap_mode (ImagePattern.cpp:43-45)
    assert (only_u.wrap_u, only_u.wrap_v) == (N.WRAP_CLAMP, N.WRAP_REPEAT)
    assert list(matrix.transform) == [1, 2, 4, 5, 6, 8]
    # the same file with and without `linear` is two images; the same file twice is one
    assert d.num_images == 2 and split.image == only_u.image == matrix.image != lin.image
    decoded = np.load(os.path.join(IR.TEXTURES, "bitmap.npy"))
    np.testing.assert_array_equal(IR.desc_image(d, split.image), IR.packed_expected(decoded, False))
    np.testing.assert_array_equal(IR.desc_image(d, lin.image), IR.packed_expected(decoded, True))


def test_relative_filenames_resolve_against_the_scene(tmp_path):
    doc = scene([{"type": "image", "name": "a", "filename": "golden/textures/bitmap.png"}], [{"type": "diffuse", "name": "d", "reflectance": "a"}])
    sc = ignis_amd.Scene.from_string(doc, base_dir=os.path.dirname(os.path.abspath(__file__)))
    d = sc.desc
    assert d.num_images == 1 and d.images[0].width == 8


def test_object_scene_equals_json_scene():
    doc = scene([{"type": "image", "name": "a", "filename": BITMAP, "filter_type": "bilinear", "wrap_mode_u": "mirror",
                  "wrap_mode_v": "repeat", "linear": True, "transform": [2.0, 0.5, 0, 0.25, -0.5, 3.0, 0, 0.75, 0, 0, 1, 0, 0, 0, 0, 1]},
                 {"type": "image", "name": "b", "filename": CONSTANT}],
                [{"type": "diffuse", "name": "da", "reflectance": "a"}, {"type": "principled", "name": "pb", "base_color": "b"}])
    js = ignis_amd.Scene.from_string(doc)
    ob = ignis_amd.Scene.from_objects(ignis_amd.ObjectScene.from_dict(doc))
    assert_desc_equal(js.desc, ob.desc)
    d1, d2 = js.desc, ob.desc
    assert d1.num_textures == d2.num_textures == 2 and d1.num_images == d2.num_images == 2
    for i in range(2):
        t1, t2 = d1.textures[i], d2.textures[i]
        assert (t1.image, t1.filter, t1.wrap_u, t1.wrap_v, list(t1.transform)) == (t2.image, t2.filter, t2.wrap_u, t2.wrap_v, list(t2.transform))
        np.testing.assert_array_equal(IR.desc_image(d1, i), IR.desc_image(d2, i))
    assert list(d1.textures[0].transform) == [2.0, 0.5, 0.25, -0.5, 3.0, 0.75]


def test_database_seam_carries_the_tables():
    doc = scene([{"type": "image", "name": "a", "filename": BITMAP}], [{"type": "diffuse", "name": "da", "reflectance": "a"}])
    sc = ignis_amd.Scene.from_string(doc)
    db = RefDatabase(sc)
    view, shading, _keep = db.views()
    assert shading.num_images == 0  # the test database predates the tables: hand them over as a binding would
    shading.num_images, shading.images = sc.desc.num_images, sc.desc.images
    shading.num_textures, shading.textures = sc.desc.num_textures, sc.desc.textures
    back = ignis_amd.Scene.from_database(view, shading)
    assert_desc_equal(sc.desc, back.desc)
    assert back.desc.num_images == 1 and back.desc.num_textures == 1
    np.testing.assert_array_equal(IR.desc_image(back.desc, 0), IR.desc_image(sc.desc, 0))
    # the texels are copied, the indices checked
    assert back.desc.images[0].pixels != sc.desc.images[0].pixels
    shading.num_textures = 0
    with pytest.raises(ignis_amd.IgxError, match="texture index beyond the texture table"):
        ignis_amd.Scene.from_database(view, shading)


def test_refusals():
    tex = [{"type": "image", "name": "a", "filename": BITMAP}, {"type": "checkerboard", "name": "c"}]
    refused = "is not a constant colour \\(shading networks are not supported\\)"
    for bsdf in ({"type": "diffuse", "name": "d", "reflectance": "a * 2"},          # an expression around the name
                 {"type": "diffuse", "name": "d", "reflectance": "a.r"},
                 {"type": "diffuse", "name": "d", "reflectance": " a"},              # not exactly the name
                 {"type": "diffuse", "name": "d", "reflectance": "c"},               # a texture that is no image
                 {"type": "diffuse", "name": "d", "reflectance": "nope"},            # no texture at all
                 {"type": "plastic", "name": "d", "diffuse_reflectance": "a"},       # a property that takes no texture
                 {"type": "conductor", "name": "d", "specular_reflectance": "a"}):
        with pytest.raises(ignis_amd.IgxError, match=refused):
            ignis_amd.Scene.from_string(scene(tex, [bsdf]))
    with pytest.raises(ignis_amd.IgxError, match=refused):
        ignis_amd.Scene.from_string({"textures": tex, "lights": [{"type": "env", "name": "l", "radiance": "c"}]})
    with pytest.raises(ignis_amd.IgxError, match=refused):
        ignis_amd.Scene.from_string({"textures": tex, "lights": [{"type": "env", "name": "l", "radiance": "a * 2"}]})
    with pytest.raises(ignis_amd.IgxError, match=refused):  # a sky's colours take no texture
        ignis_amd.Scene.from_string({"textures": tex, "lights": [{"type": "ciecloudy", "name": "l", "zenith": "a"}]})
    with pytest.raises(ignis_amd.IgxError, match="texture 'a': no filename"):
        ignis_amd.Scene.from_string(scene([{"type": "image", "name": "a"}], [{"type": "diffuse", "name": "d", "reflectance": "a"}]))
    with pytest.raises(ignis_amd.IgxError, match="cannot open the file"):
        ignis_amd.Scene.from_string(scene([{"type": "image", "name": "a", "filename": "/nonexistent/x.png"}],
                                          [{"type": "diffuse", "name": "d", "reflectance": "a"}]))


def test_image_environment_light():
    tex = [{"type": "image", "name": "sky", "filename": CONSTANT, "filter_type": "bilinear"}]
    base = {"type": "env", "name": "l", "radiance": "sky"}
    sc = ignis_amd.Scene.from_string({"textures": tex, "lights": [base]})
    L = sc.desc.lights[0]
    assert L.type == N.LIGHT_ENVMAP and (L.env_texture, L.env_cdf, L.env_compensate) == (0, 1, 1)
    assert list(L.env_scale) == [1, 1, 1] and list(L.sky_transform) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert sc.desc.num_textures == 1 and sc.desc.textures[0].filter == N.FILTER_BILINEAR
    sc2 = ignis_amd.Scene.from_string({"textures": tex, "lights": [dict(base, cdf=False, compensate=False, scale=[2, 1, 0.5],
                                                                        transform={"rotate": [0, 90, 0]})],
                                       "shapes": [{"type": "rectangle", "name": "r"}], "bsdfs": [{"type": "diffuse", "name": "d"}],
                                       "entities": [{"name": "e", "shape": "r", "bsdf": "d"}]})
    L = sc2.desc.lights[0]
    assert (L.env_cdf, L.env_compensate) == (0, 0) and list(L.env_scale) == [2, 1, 0.5]
    np.testing.assert_allclose(np.array(L.sky_transform[:]).reshape(3, 3), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-6)
    # EnvironmentLight::computeFlux: scale * 1 * pi * r^2 with r half the scene's diagonal (2 sqrt 2 / 2)
    assert L.select_flux == pytest.approx((3.5 / 3) * np.pi * 2, rel=1e-4)
    # a constant environment is what it was
    sc3 = ignis_amd.Scene.from_string({"textures": tex, "lights": [{"type": "env", "name": "l", "radiance": [1, 2, 3], "scale": 2}]})
    assert sc3.desc.lights[0].type == N.LIGHT_ENV and list(sc3.desc.lights[0].radiance) == [2, 4, 6]
    with pytest.raises(ignis_amd.IgxError, match="cdf_method 'sat' is not supported"):
        ignis_amd.Scene.from_string({"textures": tex, "lights": [dict(base, cdf_method="SAT")]})
    # an in-memory object scene reads the same light
    doc = {"textures": tex, "lights": [dict(base, scale=[2.0, 1.0, 0.5], cdf=False)]}
    ob = ignis_amd.Scene.from_objects(ignis_amd.ObjectScene.from_dict(doc))
    js = ignis_amd.Scene.from_string(doc)
    assert_desc_equal(js.desc, ob.desc)
    assert ob.desc.lights[0].type == N.LIGHT_ENVMAP and ob.desc.lights[0].env_cdf == 0
