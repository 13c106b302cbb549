// CPU check of the measured-BSDF host code (host/measured_bsdf.cpp and the
// measured part of host/scene_tables.cpp), a stand-alone program that
// tests/test_measured_loader.py builds with g++, once optimised and once with
// -fsanitize=address,undefined.  The XML reader and both loaders read files a
// user hands in, so every input here is run for its memory behaviour first:
//   * each file named on the command line (tensor tree fixtures, generated
//     Klems files) loads, and its table passes validate_measured;
//   * each of them cut short at every 37th byte, and with bytes overwritten by
//     braces, angle brackets, quotes, digits and NULs from a fixed generator,
//     either loads into a table that validates or is refused with a message;
//   * hand-written malformed documents are refused;
//   * build_scene_tables accepts a scene with a measured material and refuses
//     it once a node reference, a leaf offset, the depth, the ndim or a Klems
//     count is wrong, with IGX_ERR_INVALID_ARGUMENT and a message, before
//     anything could reach the device.
#include "measured_bsdf.h"
#include "scene_tables.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace igx;

static int g_bad = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_bad;                                                    \
        }                                                               \
    } while (0)

static bool is_klems(const std::string& text) { return text.find("TensorTree") == std::string::npos; }

// load as its own kind and as the other one; a loaded table must validate
static int load_both(const std::string& text, bool must_load) {
    int loaded = 0;
    for (int kind = 0; kind < 2; ++kind) {
        MeasuredData md;
        std::string err;
        const bool ok = kind == IGX_MEASURED_KLEMS ? load_klems_xml(text, md, err) : load_tensortree_xml(text, md, err);
        if (ok) {
            ++loaded;
            std::string verr;
            if (!validate_measured(md.m, verr)) {
                std::printf("FAIL: a loaded table does not validate: %s\n", verr.c_str());
                ++g_bad;
            }
        } else if (err.empty()) {
            std::printf("FAIL: refused without a message\n");
            ++g_bad;
        }
    }
    if (must_load) CHECK(loaded == 1);
    return loaded;
}

static void refused(const char* what, const std::string& text, bool klems, const char* needle) {
    MeasuredData md;
    std::string err;
    const bool ok = klems ? load_klems_xml(text, md, err) : load_tensortree_xml(text, md, err);
    if (ok || err.find(needle) == std::string::npos) {
        std::printf("FAIL %s: %s '%s' (expected '%s')\n", what, ok ? "loaded" : "refused with", err.c_str(), needle);
        ++g_bad;
    }
}

static std::string tree_doc(const std::string& data, const char* type = "TensorTree4") {
    return std::string("<?xml version=\"1.0\"?><WindowElement><Optical><Layer><DataDefinition><IncidentDataStructure>") + type +
           "</IncidentDataStructure></DataDefinition><WavelengthData><Wavelength unit=\"Integral\">Visible</Wavelength>"
           "<WavelengthDataBlock><WavelengthDataDirection>Transmission Back</WavelengthDataDirection>"
           "<AngleBasis>LBNL/Shirley-Chiu</AngleBasis><ScatteringData>" + data +
           "</ScatteringData></WavelengthDataBlock></WavelengthData></Layer></Optical></WindowElement>";
}

// ---- a one-quad scene with one measured material --------------------------------
struct QuadScene {
    std::vector<float> v{-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0}, n{0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    std::vector<uint32_t> ix{0, 1, 2, 0, 2, 3};
    igx_mesh mesh{};
    igx_shape shape{};
    igx_entity ent{};
    igx_material mat{};
    igx_measured meas{};
    std::vector<uint32_t> words;
    igx_scene_desc d{};
    explicit QuadScene(const MeasuredData& md) {
        mesh = igx_mesh{4, 2, v.data(), n.data(), nullptr, ix.data()};
        shape.type = IGX_SHAPE_TRIMESH;
        shape.mesh = 0;
        const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, N[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(ent.to_global, I, sizeof(I));
        std::memcpy(ent.to_local, I, sizeof(I));
        std::memcpy(ent.normal, N, sizeof(N));
        ent.flags = 0xf;
        for (int a = 0; a < 3; ++a) {
            ent.bbox_min[a] = shape.bbox_min[a] = -1;
            ent.bbox_max[a] = shape.bbox_max[a] = 1;
            d.scene_bbox_min[a] = -1;
            d.scene_bbox_max[a] = 1;
        }
        mat.bsdf_type = md.m.kind == IGX_MEASURED_KLEMS ? IGX_BSDF_KLEMS : IGX_BSDF_TENSORTREE;
        mat.light = -1;
        mat.tex_index = -1;
        mat.measured = 0;
        mat.kd[0] = mat.kd[1] = mat.kd[2] = 1;
        mat.up[2] = 1;
        meas = md.m;
        words = md.words;
        d.film_width = d.film_height = 8;
        d.technique.max_depth = 2;
    }
    const igx_scene_desc& desc() {
        meas.num_words = (uint32_t)words.size();
        meas.words = words.data();
        d.num_meshes = d.num_shapes = d.num_entities = d.num_materials = d.num_measured = 1;
        d.meshes = &mesh;
        d.shapes = &shape;
        d.entities = &ent;
        d.materials = &mat;
        d.measured = &meas;
        return d;
    }
};

static void expect_refusal(QuadScene& s, const char* what, const char* needle) {
    SceneTables t;
    std::string err;
    const igx_status st = build_scene_tables(s.desc(), SceneBuildOptions{}, t, err);
    if (st != IGX_ERR_INVALID_ARGUMENT || err.find(needle) == std::string::npos) {
        std::printf("FAIL %s: status %d '%s' (expected '%s')\n", what, (int)st, err.c_str(), needle);
        ++g_bad;
    }
}

int main(int argc, char** argv) {
    std::vector<std::string> docs;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        std::stringstream ss;
        ss << f.rdbuf();
        CHECK(!ss.str().empty());
        docs.push_back(ss.str());
        load_both(docs.back(), true);
    }
    // cut short and garbled
    uint32_t lcg = 12345;
    auto next = [&]() { return (lcg = lcg * 1664525u + 1013904223u) >> 8; };
    long variants = 0, survived = 0;
    for (const std::string& doc : docs) {
        const size_t stride = doc.size() > 20000 ? doc.size() / 200 : 37;
        for (size_t cut = 0; cut < doc.size(); cut += stride, ++variants) survived += load_both(doc.substr(0, cut), false);
        static const char junk[] = "{}<>/\"' 09-.e,\0!?[";
        for (int k = 0; k < 150; ++k, ++variants) {
            std::string g = doc;
            const int hits = 1 + next() % 4;
            for (int h = 0; h < hits; ++h) g[next() % g.size()] = junk[next() % (sizeof(junk) - 1)];
            survived += load_both(g, false);
        }
    }
    std::printf("%ld damaged variants, %ld of them still load\n", variants, survived);

    // hand-written malformed documents
    refused("unbalanced braces", tree_doc("{ { 1 } { 2 }"), false, "unbalanced braces");
    refused("closing brace first", tree_doc("} { 1 }"), false, "unbalanced braces");
    refused("leaf of 3 values", tree_doc("{ 1 2 3 }"), false, "bad amount of values");
    refused("leaf of 17 values", tree_doc("{ 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 }"), false, "bad amount of values");
    refused("seven children", tree_doc("{ {1} {1} {1} {1} {1} {1} {1} }", "TensorTree3"), false, "bad amount of children");
    refused("wrong structure", tree_doc("{ 1 }", "TensorTree5"), false, "IncidentDataStructure");
    refused("not xml", "{ 1 }", false, "xml:");
    refused("unclosed element", "<WindowElement><Optical>", false, "unexpected end of input");
    refused("mismatched end tag", "<a><b></a></b>", false, "does not match");
    {
        std::string deep17, deep16; // a chain of first children, the other 7 leaves
        for (int depth : {16, 17}) {
            std::string s;
            for (int k = 0; k < depth; ++k) s += "{ ";
            s += "{1} {1} {1} {1} {1} {1} {1} {1} }";
            for (int k = 1; k < depth; ++k) s += " {2} {2} {2} {2} {2} {2} {2} }";
            (depth == 16 ? deep16 : deep17) = tree_doc(s, "TensorTree3");
        }
        refused("depth 17", deep17, false, "deeper than 16");
        MeasuredData md;
        std::string err;
        CHECK(load_tensortree_xml(deep16, md, err));
        CHECK(md.m.component[IGX_MEASURED_FRONT_TRANSMISSION].max_depth == 16);
        CHECK(validate_measured(md.m, err));
    }

    // build_scene_tables: accepted, then refused for every kind of damage
    if (!docs.empty()) {
        for (const std::string& doc : docs) {
            MeasuredData md;
            std::string err;
            const bool klems = is_klems(doc);
            if (!(klems ? load_klems_xml(doc, md, err) : load_tensortree_xml(doc, md, err))) continue;
            QuadScene s(md);
            SceneTables t;
            CHECK(build_scene_tables(s.desc(), SceneBuildOptions{}, t, err) == IGX_OK);
            CHECK(t.full_shading);
            CHECK(t.measured_bytes == 4 * md.words.size());
            CHECK(t.mats.size() == 1 && t.mats[0].type == (klems ? igxd::MAT_KLEMS : igxd::MAT_TENSORTREE));
            CHECK(t.uvs.size() * 2 >= md.words.size());
            CHECK(md.words.empty() || std::memcmp(t.uvs.data(), md.words.data(), 4 * md.words.size()) == 0);
            {
                QuadScene b(md);
                b.mat.measured = 1;
                expect_refusal(b, "material index", "beyond the measured bsdf table");
            }
            {
                QuadScene b(md);
                b.mat.bsdf_type = klems ? IGX_BSDF_TENSORTREE : IGX_BSDF_KLEMS;
                expect_refusal(b, "kind", "other kind");
            }
            {
                QuadScene b(md);
                b.meas.component[1].offset = (uint32_t)md.words.size() + 1;
                expect_refusal(b, "offset", "offset beyond the word array");
            }
            if (klems) {
                QuadScene b(md);
                b.meas.component[1].entry_count[1] += 1;
                expect_refusal(b, "klems entry count", "measured bsdf component 1");
                QuadScene c(md);
                c.meas.component[1].theta_count[0] = 0;
                expect_refusal(c, "klems theta count", "invalid theta count");
                QuadScene e(md);
                e.words[e.meas.component[1].offset + 3] = 0; // the first band's phi count
                expect_refusal(e, "klems phi count", "invalid theta band");
                continue;
            }
            for (int k = 0; k < 4; ++k) {
                const igx_measured_component& c = md.m.component[k];
                if (c.root_is_leaf || c.node_count == 0) continue;
                {
                    QuadScene b(md);
                    b.words[c.offset] = c.node_count; // a node reference one group past the component's nodes
                    expect_refusal(b, "node reference", "node reference outside the component");
                }
                {
                    QuadScene b(md);
                    b.words[c.offset + 1] = (uint32_t)(-(int32_t)c.value_count - 1); // a leaf one past the values
                    expect_refusal(b, "leaf offset", "leaf offset outside the component");
                }
                {
                    QuadScene b(md);
                    b.words[c.offset] = 0; // the root's first child is the root again
                    expect_refusal(b, "cycle", "node reference outside the component");
                }
                {
                    QuadScene b(md);
                    for (int j = 0; j < 4; ++j)
                        if (b.meas.component[j].offset == c.offset) b.meas.component[j].max_depth = 0;
                    expect_refusal(b, "depth", "deeper than its stated max depth");
                }
                {
                    QuadScene b(md);
                    for (int j = 0; j < 4; ++j) b.meas.component[j].max_depth = 17;
                    expect_refusal(b, "depth 17", "deeper than 16");
                }
                {
                    QuadScene b(md);
                    for (int j = 0; j < 4; ++j) b.meas.component[j].ndim = 5;
                    expect_refusal(b, "ndim", "ndim is neither 3 nor 4");
                }
                break;
            }
        }
    }
    std::printf(g_bad ? "%d checks failed\n" : "ok\n", g_bad);
    return g_bad ? 1 : 0;
}
