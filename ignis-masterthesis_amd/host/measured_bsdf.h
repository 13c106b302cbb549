// Measured fenestration BSDFs as Radiance exports them (no HIP): the XML subset
// both formats use, the tensor tree (measured/TensorTreeLoader.cpp) and the
// Klems matrix (measured/KlemsLoader.cpp) of the reference, restated into the
// word layout of igx_measured (include/igx_scene.h), and the check of such a
// table that build_scene_tables runs before anything reaches the device.
#pragma once

#include "igx_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace igx {

// ---- XML -------------------------------------------------------------------
// Elements, text, comments, the prolog and <!...> declarations; attributes are
// skipped.  Text of an element is the concatenation of its character data.
struct XmlNode {
    std::string name, text;
    std::vector<XmlNode> children;
    const XmlNode* child(const char* n) const;
    // text of the first child `n` without surrounding white space, "" if absent
    std::string child_value(const char* n) const;
};
constexpr int XML_MAX_DEPTH = 64;
// false and `error` on malformed input (never throws on bad text)
bool parse_xml(const std::string& text, XmlNode& root, std::string& error);

// ---- loaders ----------------------------------------------------------------
constexpr int MEASURED_MAX_DEPTH = 16;    // tensor tree levels the device climbs at most
constexpr uint32_t KLEMS_MAX_THETAS = 256; // theta bands of one Klems basis

// One loaded file: `m.words` points into `words`.  Components in the order
// front reflection, front transmission, back reflection, back transmission,
// after the reference's front / back renaming.
struct MeasuredData {
    igx_measured m{};
    std::vector<uint32_t> words;
};
bool load_tensortree_xml(const std::string& xml_text, MeasuredData& out, std::string& error);
bool load_klems_xml(const std::string& xml_text, MeasuredData& out, std::string& error);
// kind: IGX_MEASURED_TENSORTREE or IGX_MEASURED_KLEMS
bool load_measured_file(const std::string& path, int kind, MeasuredData& out, std::string& error);

// Every node reference, leaf offset, count and offset of `m` lies inside its
// component and inside `words` (a caller of the C ABI need not have used the
// loaders above).  Also recomputes the tensor tree depth: it must not exceed
// what the component states, nor MEASURED_MAX_DEPTH.  Defined here, so that the table
// builder (scene_tables.cpp) needs no further object file.
inline bool validate_measured(const igx_measured& m, std::string& error);

// ---------------------------------------------------------------------------
// validation
// ---------------------------------------------------------------------------
inline bool validate_measured(const igx_measured& m, std::string& error) {
    auto fail = [&](int k, const std::string& msg) {
        error = "measured bsdf component " + std::to_string(k) + ": " + msg;
        return false;
    };
    if (m.kind != IGX_MEASURED_TENSORTREE && m.kind != IGX_MEASURED_KLEMS) {
        error = "measured bsdf: unknown kind " + std::to_string(m.kind);
        return false;
    }
    if (m.num_words && !m.words) {
        error = "measured bsdf: null word array";
        return false;
    }
    for (int k = 0; k < 4; ++k) {
        const igx_measured_component& c = m.component[k];
        if (!std::isfinite(c.total)) return fail(k, "total is not finite");
        if (c.offset > m.num_words) return fail(k, "offset beyond the word array");
        const uint64_t room = m.num_words - c.offset;
        const uint32_t* w = m.words + c.offset;
        if (m.kind == IGX_MEASURED_TENSORTREE) {
            if (c.ndim != 3 && c.ndim != 4) return fail(k, "ndim is neither 3 nor 4");
            if (c.ndim != m.component[0].ndim) return fail(k, "ndim differs between the components");
            const uint32_t per = 1u << c.ndim;
            if ((uint64_t)c.node_count + c.value_count > room) return fail(k, "nodes and values beyond the word array");
            if (c.value_count == 0) return fail(k, "no values");
            if (c.max_depth < 0 || c.max_depth > MEASURED_MAX_DEPTH)
                return fail(k, "tree deeper than " + std::to_string(MEASURED_MAX_DEPTH) + " levels");
            const uint32_t* vals = w + c.node_count;
            auto leaf_ok = [&](uint32_t off) { // one value with the sign bit set, or 2^ndim values
                if (off >= c.value_count) return false;
                return (vals[off] >> 31) != 0 || (uint64_t)off + per <= c.value_count;
            };
            if (c.root_is_leaf) {
                if (!leaf_ok(0)) return fail(k, "root leaf has neither 1 nor 2^ndim values");
                continue;
            }
            if (c.node_count == 0 || c.node_count % per) return fail(k, "node count is no multiple of 2^ndim");
            // groups of 2^ndim child slots; a child group lies behind its parent, so one forward pass gives every depth
            std::vector<int> level(c.node_count / per, 0);
            level[0] = 1;
            int deepest = 1;
            for (uint32_t i = 0; i < c.node_count; ++i) {
                const int lv = level[i / per];
                if (lv == 0) return fail(k, "unreachable node group");
                const int32_t v = (int32_t)w[i];
                if (v < 0) {
                    const int64_t off = -(int64_t)v - 1;
                    if (off >= c.value_count || !leaf_ok((uint32_t)off)) return fail(k, "leaf offset outside the component");
                } else {
                    if ((uint32_t)v % per || (uint64_t)v + per > c.node_count || (uint32_t)v / per <= i / per)
                        return fail(k, "node reference outside the component");
                    if (level[(uint32_t)v / per] != 0) return fail(k, "node group referenced twice");
                    level[(uint32_t)v / per] = lv + 1;
                    deepest = std::max(deepest, lv + 1);
                }
            }
            if (deepest > c.max_depth) return fail(k, "tree deeper than its stated max depth");
        } else {
            const uint64_t rt = c.theta_count[0], ct = c.theta_count[1], re = c.entry_count[0], ce = c.entry_count[1];
            if (rt == 0 && ct == 0 && re == 0 && ce == 0) {
                if (c.total != 0) return fail(k, "component without data has a total");
                continue;
            }
            if (rt == 0 || ct == 0 || rt > KLEMS_MAX_THETAS || ct > KLEMS_MAX_THETAS) return fail(k, "invalid theta count");
            if (re > (1u << 16) || ce > (1u << 16)) return fail(k, "too many patches");
            if (5 * rt + 5 * ct + re * ce > room) return fail(k, "bases and matrix beyond the word array");
            const uint32_t* b = w;
            for (int axis = 0; axis < 2; ++axis) {
                const uint64_t tc = c.theta_count[axis];
                uint64_t off = 0;
                for (uint64_t i = 0; i < tc; ++i) {
                    float lo, up;
                    std::memcpy(&lo, &b[4 * i + 1], 4);
                    std::memcpy(&up, &b[4 * i + 2], 4);
                    const uint32_t phis = b[4 * i + 3];
                    if (!std::isfinite(lo) || !std::isfinite(up) || phis == 0 || phis > 4096) return fail(k, "invalid theta band");
                    if (b[4 * tc + i] != off) return fail(k, "linear offsets do not match the phi counts");
                    off += phis;
                }
                if (off != c.entry_count[axis]) return fail(k, "entry count does not match the phi counts");
                b += 5 * tc;
            }
        }
    }
    return true;
}

} // namespace igx
