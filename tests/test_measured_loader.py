"""The measured-BSDF loaders (host/measured_bsdf.cpp) through the scene loader,
CPU only: every tensor tree fixture against tables derived by hand from the
file's few numbers, a generated tree of depth 3 against a flattening written
here, a generated Klems file on an unsorted basis in both matrix orders,
malformed files, the three ways into the loader, and the stand-alone check of
tests/native/measured_check.cpp (damaged files, build_scene_tables' refusals),
built optimised and with the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fenestration_cases as FC
import ignis_amd
from ignis_amd import _native as N

ROOT = FC.ROOT
PKG = os.path.join(ROOT, "ignis-masterthesis_amd")
HOST = os.path.join(PKG, "host")
FR, FT, BR, BT = range(4)
V = np.float32(0.254647909)  # 0.8 / pi, the value of the constant and the spot files
PI = math.pi


def load(path, kind="tensortree", **props):
    doc = {"bsdfs": [dict({"type": kind, "name": "w", "filename": str(path)}, **props)],
           "shapes": [{"type": "rectangle", "name": "r"}],
           "entities": [{"name": "e", "shape": "r", "bsdf": "w"}]}
    return ignis_amd.Scene.from_string(doc)


def component(measured, k):
    """(spec, nodes int32, values float32) of component k."""
    c = measured.component[k]
    w = np.ctypeslib.as_array(measured.words, (measured.num_words,))
    return c, w[c.offset:c.offset + c.node_count].view(np.int32), w[c.offset + c.node_count:c.offset + c.node_count + c.value_count].view(np.float32)


# ---- the fixtures, by hand -----------------------------------------------------------------
# A component is (nodes, values, total, max depth).  "Transmission Back" is the front
# transmission, "Reflection Back" the front reflection, "Reflection Front" the back
# reflection (TensorTreeLoader.cpp:292-300); a file without "Transmission Front" has the
# same tree on both sides; a missing reflection is black.
BLACK = ([], [-0.0], 0.0, 0)


def singles(*v):
    """One inner node whose children are all leaves of one value: node k names value k;
    every value has its sign bit set.  Each counts pi * v / (2 * 1) (depth 2, one value)."""
    return list(range(-1, -len(v) - 1, -1)), [-x for x in v], PI * sum(v) / 2, 1


def root_leaf(*v):
    """The root is a leaf: pi * sum / (1 * count)."""
    return [], ([-v[0]] if len(v) == 1 else list(v)), PI * sum(v) / len(v), 0


def spot(n, *at):
    return [float(V) if i in at else 0.0 for i in range(n)]


HUNDREDTHS = [k / 100 for k in range(1, 17)]
# { .01 } { .02 } { .03 } { .04 } { sixteen or eight values } { .06 } ...: the full leaf sits at value 4
D3_16 = (list(range(-1, -5, -1)) + [-5] + list(range(-21, -32, -1)),
         [-x for x in HUNDREDTHS[:4]] + HUNDREDTHS + [-x for x in HUNDREDTHS[5:]],
         PI * (sum(HUNDREDTHS) - 0.05) / 2 + PI * sum(HUNDREDTHS) / (2 * 16), 1)


def d3_8(last):
    full = HUNDREDTHS[:7] + [last]
    return (list(range(-1, -5, -1)) + [-5] + list(range(-13, -16, -1)),
            [-x for x in HUNDREDTHS[:4]] + full + [-x for x in HUNDREDTHS[5:8]],
            PI * (sum(HUNDREDTHS[:8]) - 0.05) / 2 + PI * sum(full) / (2 * 8), 1)


LINE = [0.0] + HUNDREDTHS[1:]
ZERO = root_leaf(0.0)
#                 ndim, front reflection, front transmission, back reflection, back transmission
EXPECTED = {
    "trans": (4, BLACK, root_leaf(V), BLACK, root_leaf(V)),
    "refl": (4, root_leaf(V), ZERO, root_leaf(V), ZERO),
    "front_refl": (4, ZERO, ZERO, root_leaf(V), ZERO),
    "spot_trans": (4, BLACK, root_leaf(*spot(16, 7)), BLACK, root_leaf(*spot(16, 7))),
    "spot_t3_trans": (3, BLACK, root_leaf(*spot(8, 7)), BLACK, root_leaf(*spot(8, 7))),
    "spot_refl": (4, root_leaf(*spot(16, 7, 12)), ZERO, root_leaf(*spot(16, 7, 12)), ZERO),
    "d2_trans": (4, BLACK, singles(*spot(16, 7, 12)), BLACK, singles(*spot(16, 7, 12))),
    "d2_t3_trans": (3, BLACK, singles(*spot(8, 7)), BLACK, singles(*spot(8, 7))),
    "d2_refl": (4, singles(*HUNDREDTHS), ZERO, singles(*HUNDREDTHS), ZERO),
    "d2_t3_refl": (3, singles(*HUNDREDTHS[:8]), ZERO, singles(*HUNDREDTHS[:8]), ZERO),
    "d2_line_refl": (4, root_leaf(*LINE), ZERO, root_leaf(*LINE), ZERO),
    "d3_refl": (4, D3_16, ZERO, D3_16, ZERO),
    "d3_t3_refl": (3, d3_8(0.08), ZERO, d3_8(0.0), ZERO),  # the "Reflection Front" block ends in 0.0
}


def test_every_fixture_is_listed():
    files = sorted(f for f in os.listdir(FC.GOLDEN) if f.startswith("simple_tensor_"))
    assert files == sorted("simple_tensor_%s.xml" % k for k in EXPECTED) and len(files) == 13


@pytest.mark.parametrize("name", list(EXPECTED))
def test_fixture_tables(name):
    sc = load(os.path.join(FC.GOLDEN, "simple_tensor_%s.xml" % name))
    d = sc.desc
    assert d.num_measured == 1 and d.materials[0].bsdf_type == N.BSDF_TENSORTREE and d.materials[0].measured == 0
    assert d.materials[0].kd[:] == [1, 1, 1] and d.materials[0].up[:] == [0, 0, 1]
    m = d.measured[0]
    assert m.kind == N.MEASURED_TENSORTREE
    ndim, *comps = EXPECTED[name]
    for k, (nodes, values, total, depth) in enumerate(comps):
        c, got_nodes, got_values = component(m, k)
        assert c.ndim == ndim
        assert list(got_nodes) == nodes, (name, k)
        want = np.array(values, np.float32)
        np.testing.assert_array_equal(got_values, want)
        np.testing.assert_array_equal(np.signbit(got_values), np.signbit(want))
        assert bool(c.root_is_leaf) == (not nodes) and c.max_depth == depth
        assert c.total == pytest.approx(total, rel=1e-5, abs=1e-12), (name, k)
    # one tree on both sides is stored once
    if comps[FT] == comps[BT]:
        assert m.component[FT].offset == m.component[BT].offset


# ---- a generated tree, flattened here ----------------------------------------------------------
def parse_braces(text):
    """Nested lists of a brace text: a leaf is a list of floats."""
    tokens = re.findall(r"[{}]|[^\s{},]+", text)
    pos = [0]

    def node():
        assert tokens[pos[0]] == "{"
        pos[0] += 1
        out = []
        while tokens[pos[0]] != "}":
            out.append(node() if tokens[pos[0]] == "{" else float(tokens[pos[0]]))
            if not isinstance(out[-1], list):
                pos[0] += 1
        pos[0] += 1
        return out

    return node()


def flatten(tree):
    """TensorTreeComponent::addNode: child slots first, then the children in order."""
    nodes, values, depth = [], [], [0]

    def total(n, d):  # TensorTreeNode::computeTotal, as written
        if isinstance(n[0], list):
            return sum(total(c, d + 1) for c in n)
        return sum(PI * v / (d * len(n)) for v in n)

    def add(n, parent, level):
        if not isinstance(n[0], list):
            if parent is not None:
                nodes[parent] = -(len(values) + 1)
            values.extend([-n[0]] if len(n) == 1 else n)
            return
        off = len(nodes)
        if parent is not None:
            nodes[parent] = off
        depth[0] = max(depth[0], level)
        nodes.extend([0] * len(n))
        for i, c in enumerate(n):
            add(c, off + i, level + 1)

    add(tree, None, 1)
    return nodes, values, total(tree, 1), depth[0]


@pytest.mark.parametrize("ndim", [3, 4])
def test_generated_tree_of_depth_3(tmp_path, ndim):
    trees = {d: FC.tree_text(ndim, 10 * ndim + k) for k, d in enumerate(FC.DIRECTIONS)}
    p = tmp_path / "mixed.xml"
    p.write_text(FC.tensortree_xml(ndim, trees))
    sc = load(p)  # owns the tables
    m = sc.desc.measured[0]
    place = {"Transmission Front": BT, "Transmission Back": FT, "Reflection Front": BR, "Reflection Back": FR}
    offsets = set()
    for d, k in place.items():
        nodes, values, total, depth = flatten(parse_braces(trees[d]))
        c, got_nodes, got_values = component(m, k)
        assert depth == 3 and c.max_depth == 3 and not c.root_is_leaf and c.ndim == ndim
        assert any(v < 0 for v in values) and any(v > 0 for v in values)  # single and full leaves
        assert list(got_nodes) == nodes
        np.testing.assert_array_equal(got_values, np.array(values, np.float32))
        assert c.total == pytest.approx(total, rel=1e-5)
        offsets.add(c.offset)
    assert len(offsets) == 4


def test_only_visible_blocks_count(tmp_path):
    p = tmp_path / "solar.xml"
    p.write_text(FC.tensortree_xml(4, {"Transmission Back": "{ 0.5 }"}, visible=False))
    with pytest.raises(ignis_amd.IgxError, match="no transmission data"):
        load(p)


# ---- Klems -------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["Columns", "Rows"])
def test_klems_on_an_unsorted_basis(tmp_path, structure):
    """Bands listed as 0-30 (1 patch), 60-90 (4), 30-60 (4): the loader sorts them by upper
    theta, so the file's patches 1..4 become patches 5..8 and 5..8 become 1..4, in rows and columns."""
    p = tmp_path / "small.xml"
    p.write_text(FC.small_klems_xml(structure))
    sc = load(p, "klems", base_color=[0.5, 0.25, 1.0], up=[0, 3, 4])
    d = sc.desc
    mat = d.materials[0]
    assert mat.bsdf_type == N.BSDF_KLEMS and mat.kd[:] == [0.5, 0.25, 1.0]
    np.testing.assert_allclose(mat.up[:], [0, 0.6, 0.8], rtol=1e-6)
    m = d.measured[0]
    assert m.kind == N.MEASURED_KLEMS
    to_sorted = np.array([0, 5, 6, 7, 8, 1, 2, 3, 4])
    # projected solid angle of a patch: pi (cos^2 lower - cos^2 upper) / phi count
    psa = np.array([PI / 4] + [PI * 0.5 / 4] * 4 + [PI * 0.25 / 4] * 4)
    place = {"Transmission Front": BT, "Transmission Back": FT, "Reflection Front": BR, "Reflection Back": FR}
    w = np.ctypeslib.as_array(m.words, (m.num_words,))
    for k, direction in enumerate(FC.DIRECTIONS):
        c = m.component[place[direction]]
        assert c.theta_count[:] == [3, 3] and c.entry_count[:] == [9, 9]
        at = c.offset
        for axis in range(2):
            rec = w[at:at + 12].reshape(3, 4)
            np.testing.assert_allclose(rec[:, 1].copy().view(np.float32), np.radians([0, 30, 60]), rtol=1e-6)
            np.testing.assert_allclose(rec[:, 2].copy().view(np.float32), np.radians([30, 60, 90]), rtol=1e-6)
            np.testing.assert_allclose(rec[:, 0].copy().view(np.float32), np.radians([0, 45, 75]), rtol=1e-6)
            assert list(rec[:, 3]) == [1, 4, 4] and list(w[at + 12:at + 15]) == [0, 1, 5]
            at += 15
        got = w[at:at + 81].view(np.float32).reshape(9, 9)
        file_matrix = FC.small_matrix(100 + k)
        want = np.zeros((9, 9))
        want[np.ix_(to_sorted, to_sorted)] = file_matrix
        np.testing.assert_array_equal(got, want.astype(np.float32))
        assert c.total == pytest.approx(float(psa @ want @ psa), rel=1e-5)


def test_klems_without_theta_and_with_two_bases(tmp_path):
    p = tmp_path / "full.xml"
    p.write_text(FC.full_klems_xml())
    sc = load(p, "klems")  # owns the tables
    m = sc.desc.measured[0]
    assert m.component[FT].theta_count[:] == [7, 9] and m.component[FT].entry_count[:] == [73, 145]
    assert m.component[BT].theta_count[:] == [9, 9] and m.component[BT].entry_count[:] == [145, 145]
    w = np.ctypeslib.as_array(m.words, (m.num_words,))
    centre = w[m.component[FT].offset:][:28].reshape(7, 4)[:, 0].copy().view(np.float32)
    np.testing.assert_allclose(centre, np.radians([3.25, 13, 26, 39.5, 54, 69, 83.25]), rtol=1e-6)  # no <Theta>: the band's middle


def test_klems_negative_and_non_finite_entries_are_zero(tmp_path):
    m9 = FC.small_matrix(5)
    text = FC.klems_xml("Columns", [FC.basis_xml("small", *FC.SMALL_BASIS)], {"Transmission Back": ("small", "small", m9)})
    first = "%.6f" % m9[0, 0]
    second = "%.6f" % m9[0, 1]
    text = text.replace(first + ", " + second, "-1.5, nan", 1)
    p = tmp_path / "neg.xml"
    p.write_text(text)
    sc = load(p, "klems")  # owns the tables
    m = sc.desc.measured[0]
    c = m.component[FT]
    got = np.ctypeslib.as_array(m.words, (m.num_words,))[c.offset + 30:c.offset + 111].view(np.float32).reshape(9, 9)
    want = m9.copy()
    want[0, 0] = want[0, 1] = 0
    np.testing.assert_array_equal(got, want.astype(np.float32))
    assert m.component[FR].total == 0 and m.component[FR].entry_count[:] == [0, 0]  # black by default
    assert m.component[BT].offset == c.offset


# ---- refusals ----------------------------------------------------------------------------------
def _tree(data, ndim=4):
    return FC.tensortree_xml(ndim, {"Transmission Back": data})


def _deep(levels):
    s = "{ " * levels + " ".join(["{1}"] * 8) + " }" + (" " + " ".join(["{2}"] * 7) + " }") * (levels - 1)
    return _tree(s, 3)


MALFORMED = {
    "unbalanced braces": ("tensortree", _tree("{ { 1 } { 2 }"), "unbalanced braces"),
    "leaf of 3 values": ("tensortree", _tree("{ 1 2 3 }"), "bad amount of values"),
    "missing basis": ("tensortree", _tree("{ 1 }").replace("<AngleBasis>LBNL/Shirley-Chiu</AngleBasis>", ""), "no angle basis"),
    "another basis": ("tensortree", _tree("{ 1 }").replace("Shirley-Chiu", "Klems Full"), "Shirley-Chiu"),
    "depth 17": ("tensortree", _deep(17), "deeper than 16"),
    "klems without a basis": ("klems", FC.klems_xml("Columns", [], {"Transmission Back": ("b", "b", np.ones((9, 9)))}), "no basis given"),
    "klems with an unknown basis": ("klems", FC.klems_xml("Columns", [FC.basis_xml("small", *FC.SMALL_BASIS)],
                                                          {"Transmission Back": ("small", "other", np.ones((9, 9)))}), "no known column or row basis"),
    "short matrix": ("klems", FC.klems_xml("Columns", [FC.basis_xml("small", *FC.SMALL_BASIS)],
                                           {"Transmission Back": ("small", "small", np.ones((8, 9)))}), "not of length 81"),
    "truncated file": ("tensortree", _tree("{ 1 }")[:400], "xml:"),
    "klems file as a tree": ("tensortree", FC.small_klems_xml(), "IncidentDataStructure"),
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_malformed_files_are_refused(tmp_path, what):
    kind, text, message = MALFORMED[what]
    p = tmp_path / "bad.xml"
    p.write_text(text)
    with pytest.raises(ignis_amd.IgxError, match=message):
        load(p, kind)


def test_depth_16_loads(tmp_path):
    p = tmp_path / "deep.xml"
    p.write_text(_deep(16))
    sc = load(p)
    assert sc.desc.measured[0].component[FT].max_depth == 16


def test_missing_file_is_reported():
    with pytest.raises(ignis_amd.IgxError, match="cannot open"):
        load("/nonexistent/window.xml")


# ---- the three ways into the loader ----------------------------------------------------------------
def test_evaluation_scenes_load_and_share_files():
    """Before these BSDFs existed, every one of these scenes failed with "unsupported bsdf type"."""
    for name in FC.EVAL_SCENES:
        sc = FC.load_eval_scene(name)
        d = sc.desc
        assert d.num_materials == 4 and d.num_measured == 4 and d.num_entities == 4
        assert sorted(d.materials[i].measured for i in range(4)) == [0, 1, 2, 3]
        assert all(d.materials[i].up[:] == [0, 1, 0] for i in range(4))


def test_two_bsdfs_of_one_file_share_the_table(tmp_path):
    f = os.path.join(FC.GOLDEN, "simple_tensor_d3_refl.xml")
    doc = {"bsdfs": [{"type": "tensortree", "name": "a", "filename": f}, {"type": "tensortree", "name": "b", "filename": f, "up": [0, 1, 0]},
                     {"type": "tensortree", "name": "c", "filename": os.path.join(FC.GOLDEN, "simple_tensor_trans.xml")}],
           "shapes": [{"type": "rectangle", "name": "r"}],
           "entities": [{"name": n, "shape": "r", "bsdf": n} for n in "abc"]}
    sc = ignis_amd.Scene.from_string(doc)
    d = sc.desc
    assert d.num_measured == 2
    by_name = {n: d.materials[sc.find_material(n)].measured for n in "abc"} if hasattr(sc, "find_material") else None
    used = sorted(d.materials[i].measured for i in range(d.num_materials))
    assert used == [0, 0, 1]
    if by_name:
        assert by_name["a"] == by_name["b"] != by_name["c"]


def test_file_names_resolve_against_the_base_directory():
    doc = {"bsdfs": [{"type": "tensortree", "name": "w", "filename": "simple_tensor_trans.xml"}],
           "shapes": [{"type": "rectangle", "name": "r"}], "entities": [{"name": "e", "shape": "r", "bsdf": "w"}]}
    import json
    L = N.lib()
    err = C.create_string_buffer(512)
    h = L.igx_scene_load_string(json.dumps(doc).encode(), FC.GOLDEN.encode(), err, 512)
    assert h, err.value
    assert L.igx_scene_get_desc(h).contents.num_measured == 1
    L.igx_scene_free(h)
    assert not L.igx_scene_load_string(json.dumps(doc).encode(), b"/nonexistent", err, 512)
    assert b"cannot open" in err.value


def test_object_scene_loads_a_measured_bsdf():
    """igx_scene_from_objects: the same loader, the file resolved against the object's directory."""
    L = N.lib()
    os_ = L.igx_objscene_create(b"/nonexistent")
    b = L.igx_objscene_add(os_, 0, b"klems", b"w", FC.GOLDEN.encode())  # IGX_OBJ_BSDF
    assert L.igx_objscene_set_property(os_, b, b"filename", 4, C.c_char_p(b"simple_tensor_trans.xml"), 1) == 0
    L.igx_objscene_add(os_, 6, b"rectangle", b"r", None)
    e = L.igx_objscene_add(os_, 2, b"entity", b"e", None)
    for key, val in ((b"shape", b"r"), (b"bsdf", b"w")):
        assert L.igx_objscene_set_property(os_, e, key, 4, C.c_char_p(val), 1) == 0
    err = C.create_string_buffer(512)
    assert not L.igx_scene_from_objects(os_, err, 512)  # a tensor tree file named by a klems bsdf
    assert b"IncidentDataStructure" in err.value
    L.igx_objscene_free(os_)
    os_ = L.igx_objscene_create(b"/nonexistent")
    b = L.igx_objscene_add(os_, 0, b"tensortree", b"w", FC.GOLDEN.encode())
    assert L.igx_objscene_set_property(os_, b, b"filename", 4, C.c_char_p(b"simple_tensor_trans.xml"), 1) == 0
    up = (C.c_float * 3)(0, 2, 0)
    assert L.igx_objscene_set_property(os_, b, b"up", 7, up, 3) == 0
    L.igx_objscene_add(os_, 6, b"rectangle", b"r", None)
    e = L.igx_objscene_add(os_, 2, b"entity", b"e", None)
    for key, val in ((b"shape", b"r"), (b"bsdf", b"w")):
        assert L.igx_objscene_set_property(os_, e, key, 4, C.c_char_p(val), 1) == 0
    h = L.igx_scene_from_objects(os_, err, 512)
    assert h, err.value
    d = L.igx_scene_get_desc(h).contents
    assert d.num_measured == 1 and d.materials[0].bsdf_type == N.BSDF_TENSORTREE and d.materials[0].up[:] == [0, 1, 0]
    L.igx_scene_free(h)
    L.igx_objscene_free(os_)


# ---- the stand-alone check ---------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["O2", "sanitized"])
def test_damaged_files_and_table_refusals(tmp_path, flags):
    exe = str(tmp_path / "measured_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-I", HOST, "-I", os.path.join(PKG, "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "measured_check.cpp"),
                    os.path.join(HOST, "measured_bsdf.cpp"), os.path.join(HOST, "scene_tables.cpp"), os.path.join(HOST, "bvh_build.cpp"),
                    os.path.join(HOST, "light_select.cpp"), "-pthread", "-o", exe], check=True)
    files = [os.path.join(FC.GOLDEN, "simple_tensor_%s.xml" % k) for k in EXPECTED]
    for name, text in (("mixed3", FC.mixed_tree_xml(3)), ("mixed4", FC.mixed_tree_xml(4)), ("small", FC.small_klems_xml()),
                       ("rows", FC.small_klems_xml("Rows")), ("full", FC.full_klems_xml())):
        p = tmp_path / (name + ".xml")
        p.write_text(text)
        files.append(str(p))
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
