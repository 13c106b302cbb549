// Measured fenestration BSDFs: XML reader, tensor tree and Klems loaders, table check (measured_bsdf.h).
#include "measured_bsdf.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <numeric>
#include <sstream>

namespace igx {

// ---------------------------------------------------------------------------
// XML
// ---------------------------------------------------------------------------
const XmlNode* XmlNode::child(const char* n) const {
    for (const auto& c : children)
        if (c.name == n) return &c;
    return nullptr;
}
static std::string trimmed(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && std::isspace((unsigned char)s[a])) ++a;
    while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}
std::string XmlNode::child_value(const char* n) const {
    const XmlNode* c = child(n);
    return c ? trimmed(c->text) : std::string();
}

bool parse_xml(const std::string& t, XmlNode& root, std::string& error) {
    root = XmlNode{};
    auto fail = [&](const std::string& msg, size_t at) {
        error = "xml: " + msg + " at byte " + std::to_string(at);
        return false;
    };
    // the open elements, as child indices from the root (pointers would move as vectors grow)
    std::vector<size_t> path;
    auto current = [&]() -> XmlNode& {
        XmlNode* n = &root;
        for (size_t i : path) n = &n->children[i];
        return *n;
    };
    bool have_root = false, root_closed = false;
    const size_t n = t.size();
    size_t i = 0;
    while (i < n) {
        if (t[i] != '<') {
            const size_t e = std::min(t.find('<', i), n);
            if (have_root && !root_closed) current().text.append(t, i, e - i);
            else
                for (size_t k = i; k < e; ++k)
                    if (!std::isspace((unsigned char)t[k]) && !(k < 3 && (unsigned char)t[k] >= 0x80)) // a byte order mark
                        return fail("text outside the root element", k);
            i = e;
            continue;
        }
        if (t.compare(i, 4, "<!--") == 0) {
            const size_t e = t.find("-->", i + 4);
            if (e == std::string::npos) return fail("unterminated comment", i);
            i = e + 3;
        } else if (t.compare(i, 2, "<?") == 0) {
            const size_t e = t.find("?>", i + 2);
            if (e == std::string::npos) return fail("unterminated processing instruction", i);
            i = e + 2;
        } else if (t.compare(i, 9, "<![CDATA[") == 0) {
            const size_t e = t.find("]]>", i + 9);
            if (e == std::string::npos) return fail("unterminated CDATA section", i);
            if (!have_root || root_closed) return fail("CDATA outside the root element", i);
            current().text.append(t, i + 9, e - (i + 9));
            i = e + 3;
        } else if (t.compare(i, 2, "<!") == 0) {
            const size_t e = t.find('>', i + 2);
            if (e == std::string::npos) return fail("unterminated declaration", i);
            i = e + 1;
        } else if (t.compare(i, 2, "</") == 0) {
            const size_t e = t.find('>', i + 2);
            if (e == std::string::npos) return fail("unterminated end tag", i);
            const std::string name = trimmed(t.substr(i + 2, e - (i + 2)));
            if (!have_root || root_closed) return fail("end tag without an open element", i);
            if (current().name != name) return fail("end tag </" + name + "> does not match <" + current().name + ">", i);
            if (path.empty()) root_closed = true;
            else path.pop_back();
            i = e + 1;
        } else {
            size_t k = i + 1;
            while (k < n && !std::isspace((unsigned char)t[k]) && t[k] != '>' && t[k] != '/') ++k;
            const std::string name = t.substr(i + 1, k - (i + 1));
            if (name.empty()) return fail("empty element name", i);
            // attributes: skipped, quoted values may hold '>' and '/'
            bool self_closing = false;
            for (;;) {
                if (k >= n) return fail("unterminated start tag", i);
                const char c = t[k];
                if (c == '"' || c == '\'') {
                    const size_t q = t.find(c, k + 1);
                    if (q == std::string::npos) return fail("unterminated attribute value", k);
                    k = q + 1;
                } else if (c == '/' && k + 1 < n && t[k + 1] == '>') {
                    self_closing = true;
                    k += 2;
                    break;
                } else if (c == '>') {
                    ++k;
                    break;
                } else if (c == '<') {
                    return fail("'<' inside a start tag", k);
                } else {
                    ++k;
                }
            }
            if (root_closed) return fail("second root element", i);
            if (!have_root) {
                have_root = true;
                root.name = name;
                if (self_closing) root_closed = true;
            } else {
                if ((int)path.size() + 1 >= XML_MAX_DEPTH) return fail("elements nested too deeply", i);
                XmlNode& cur = current();
                cur.children.emplace_back();
                cur.children.back().name = name;
                if (!self_closing) path.push_back(cur.children.size() - 1);
            }
            i = k;
        }
    }
    if (!have_root) return fail("no root element", n);
    if (!root_closed) return fail("unexpected end of input inside <" + current().name + ">", n);
    return true;
}

// ---------------------------------------------------------------------------
// shared: the layer of a WindowElement, the front / back renaming
// ---------------------------------------------------------------------------
namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kDeg2Rad = kPi / 180.0f;
constexpr float kFltEps = 1.1920928955e-07f;

enum { FR = IGX_MEASURED_FRONT_REFLECTION, FT = IGX_MEASURED_FRONT_TRANSMISSION, BR = IGX_MEASURED_BACK_REFLECTION,
       BT = IGX_MEASURED_BACK_TRANSMISSION };

const XmlNode* find_layer(const XmlNode& doc, std::string& error) {
    const XmlNode* layer = nullptr;
    if (doc.name == "WindowElement")
        if (const XmlNode* opt = doc.child("Optical")) layer = opt->child("Layer");
    if (!layer) error = "no WindowElement/Optical/Layer element";
    return layer;
}

// The window definition flips front and back (TensorTreeLoader.cpp:290-300, KlemsLoader.cpp:459-469)
int component_of(const std::string& direction) {
    if (direction == "Transmission Front") return BT;
    if (direction == "Scattering Back" || direction == "Reflection Back") return FR;
    if (direction == "Transmission Back") return FT;
    return BR;
}

// ---------------------------------------------------------------------------
// tensor tree
// ---------------------------------------------------------------------------
struct TreeNode {
    std::vector<std::unique_ptr<TreeNode>> children;
    std::vector<float> values;
};

// TensorTreeNode::computeTotal, as written: `area` is no solid angle; the
// totals only steer the choice between reflection and transmission
float tree_total(const TreeNode& n, size_t depth) {
    const float area = 1.0f / (depth * (n.values.size() + n.children.size()));
    float total = 0;
    for (const auto& c : n.children) total += tree_total(*c, depth + 1);
    for (float v : n.values) total += kPi * v * area;
    return total;
}

struct TreeComponent {
    std::vector<int32_t> nodes;
    std::vector<float> values;
    float total = 0;
    bool root_is_leaf = false;
    int max_depth = 0;
    uint32_t per_node = 16;

    // TensorTreeComponent::addNode: child slots first, then the children in order
    void add(const TreeNode& n, long parent, int level) {
        if (n.children.empty()) {
            const size_t off = values.size();
            if (parent >= 0) nodes[parent] = -((int32_t)off + 1);
            else root_is_leaf = true;
            if (n.values.size() == 1) values.push_back(std::copysign(n.values.front(), -1.0f));
            else values.insert(values.end(), n.values.begin(), n.values.end());
        } else {
            const size_t off = nodes.size();
            if (parent >= 0) nodes[parent] = (int32_t)off;
            max_depth = std::max(max_depth, level);
            nodes.resize(off + n.children.size(), 0);
            for (size_t i = 0; i < n.children.size(); ++i) add(*n.children[i], (long)(off + i), level + 1);
        }
    }
    void make_black() {
        // never evaluated (total 0): one single-value leaf of -0 as the root
        nodes.clear();
        values.assign(1, -0.0f);
        total = 0;
        root_is_leaf = true;
        max_depth = 0;
    }
};

bool parse_tree(const std::string& s, uint32_t per_node, TreeNode& root, std::string& error) {
    std::vector<TreeNode*> stack{&root};
    const char* p = s.c_str();
    while (*p) {
        const char c = *p;
        if (c == '{') {
            // root + the eaten level + MEASURED_MAX_DEPTH inner levels + the leaf
            if (stack.size() > (size_t)MEASURED_MAX_DEPTH + 2) {
                error = "tensor tree deeper than " + std::to_string(MEASURED_MAX_DEPTH) + " levels";
                return false;
            }
            ++p;
            stack.back()->children.emplace_back(new TreeNode());
            stack.push_back(stack.back()->children.back().get());
        } else if (c == '}') {
            if (stack.size() <= 1) {
                error = "misformed scatter data: unbalanced braces";
                return false;
            }
            ++p;
            stack.pop_back();
        } else if (c == ',' || std::isspace((unsigned char)c)) {
            ++p;
        } else {
            TreeNode* node = stack.back();
            if (stack.size() <= 1 || !node->children.empty() || !node->values.empty()) {
                error = "misformed scatter data: values outside a leaf";
                return false;
            }
            while (*p && *p != '}') {
                if (*p == ',' || std::isspace((unsigned char)*p)) {
                    ++p;
                    continue;
                }
                char* end = nullptr;
                const float v = std::strtof(p, &end);
                if (end == p || !std::isfinite(v)) {
                    error = "misformed scatter data: not a finite number";
                    return false;
                }
                p = end;
                if (node->values.size() >= per_node) {
                    error = "misformed scatter data: bad amount of values per node";
                    return false;
                }
                node->values.push_back(std::fabs(v)); // absolute values, as the reference
            }
            if (node->values.size() != 1 && node->values.size() != per_node) {
                error = "misformed scatter data: bad amount of values per node";
                return false;
            }
        }
    }
    if (stack.size() != 1) {
        error = "misformed scatter data: unbalanced braces";
        return false;
    }
    return true;
}

bool check_tree(const TreeNode& n, uint32_t per_node, std::string& error) {
    if (n.children.empty()) return true;
    if (!n.values.empty() || n.children.size() != per_node) {
        error = "misformed scatter data: bad amount of children per node";
        return false;
    }
    for (const auto& c : n.children) {
        if (c->children.empty() && c->values.empty()) {
            error = "misformed scatter data: empty node";
            return false;
        }
        if (!check_tree(*c, per_node, error)) return false;
    }
    return true;
}

} // namespace

bool load_tensortree_xml(const std::string& xml_text, MeasuredData& out, std::string& error) {
    out = MeasuredData{};
    XmlNode doc;
    if (!parse_xml(xml_text, doc, error)) return false;
    const XmlNode* layer = find_layer(doc, error);
    if (!layer) return false;
    const XmlNode* dd = layer->child("DataDefinition");
    if (!dd) {
        error = "no DataDefinition element";
        return false;
    }
    const std::string type = dd->child_value("IncidentDataStructure");
    const bool dim4 = type == "TensorTree4";
    if (!dim4 && type != "TensorTree3") {
        error = "expected IncidentDataStructure 'TensorTree4' or 'TensorTree3' but got '" + type + "'";
        return false;
    }
    const int ndim = dim4 ? 4 : 3;
    const uint32_t per_node = 1u << ndim;
    std::shared_ptr<TreeComponent> comp[4];
    for (const XmlNode& data : layer->children) {
        if (data.name != "WavelengthData") continue;
        if (data.child_value("Wavelength") != "Visible") continue; // other wavelength ranges are skipped
        const XmlNode* block = data.child("WavelengthDataBlock");
        if (!block) {
            error = "no WavelengthDataBlock given";
            return false;
        }
        const std::string basis = block->child_value("AngleBasis");
        if (basis.empty()) {
            error = "WavelengthDataBlock has no angle basis given";
            return false;
        }
        if (basis != "LBNL/Shirley-Chiu") {
            error = "AngleBasis is not 'LBNL/Shirley-Chiu'";
            return false;
        }
        const XmlNode* sd = block->child("ScatteringData");
        TreeNode root;
        if (!parse_tree(sd ? sd->text : std::string(), per_node, root, error)) return false;
        if (root.children.empty()) {
            error = "root of scatter data has no data";
            return false;
        }
        if (root.children.size() != 1) {
            error = "root of scatter data has invalid data";
            return false;
        }
        { // the root eats its only child
            std::unique_ptr<TreeNode> only = std::move(root.children[0]);
            root.children = std::move(only->children);
            root.values = std::move(only->values);
        }
        if (root.children.empty() && root.values.empty()) {
            error = "no data given";
            return false;
        }
        if (!check_tree(root, per_node, error)) return false;
        auto c = std::make_shared<TreeComponent>();
        c->per_node = per_node;
        c->add(root, -1, 1);
        if (c->max_depth > MEASURED_MAX_DEPTH) {
            error = "tensor tree deeper than " + std::to_string(MEASURED_MAX_DEPTH) + " levels";
            return false;
        }
        c->total = tree_total(root, 1);
        if (!std::isfinite(c->total)) {
            error = "scatter data sums to no finite total";
            return false;
        }
        comp[component_of(block->child_value("WavelengthDataDirection"))] = c;
    }
    // missing reflection components are black (Radiance doc/notes/BSDFdirections.txt)
    for (int k : {BR, FR})
        if (!comp[k]) {
            comp[k] = std::make_shared<TreeComponent>();
            comp[k]->make_black();
        }
    // both transmission parts are equal unless given otherwise
    if (!comp[BT] || (comp[FT] && comp[BT]->total <= kFltEps)) comp[BT] = comp[FT];
    if (!comp[FT] || (comp[BT] && comp[FT]->total <= kFltEps)) comp[FT] = comp[BT];
    if (!comp[FT] && !comp[BT]) {
        error = "no transmission data found";
        return false;
    }
    out.m.kind = IGX_MEASURED_TENSORTREE;
    std::map<const TreeComponent*, uint32_t> placed; // a shared transmission tree is stored once
    for (int k = 0; k < 4; ++k) {
        const TreeComponent& c = *comp[k];
        igx_measured_component& s = out.m.component[k];
        auto at = placed.find(&c);
        if (at == placed.end()) {
            at = placed.emplace(&c, (uint32_t)out.words.size()).first;
            const size_t o = out.words.size();
            out.words.resize(o + c.nodes.size() + c.values.size());
            if (!c.nodes.empty()) std::memcpy(&out.words[o], c.nodes.data(), 4 * c.nodes.size());
            std::memcpy(&out.words[o + c.nodes.size()], c.values.data(), 4 * c.values.size());
        }
        s.total = c.total;
        s.offset = at->second;
        s.ndim = ndim;
        s.node_count = (uint32_t)c.nodes.size();
        s.value_count = (uint32_t)c.values.size();
        s.root_is_leaf = c.root_is_leaf ? 1 : 0;
        s.max_depth = c.max_depth;
    }
    out.m.num_words = (uint32_t)out.words.size();
    out.m.words = out.words.data();
    return true;
}

// ---------------------------------------------------------------------------
// Klems
// ---------------------------------------------------------------------------
namespace {

struct ThetaBasis {
    float center, lower, upper;
    uint32_t phi_count;
    float phi_solid_angle; // projected, per phi patch
};

struct KlemsBasis {
    std::vector<ThetaBasis> thetas;   // sorted by upper theta
    std::vector<uint32_t> lin_offset; // first patch of each band
    std::vector<uint32_t> permutation; // file patch -> sorted patch
    uint32_t entries = 0;

    // KlemsBasis::setup, as written: the enlarged permutation reads the band
    // sizes and offsets of the *sorted* basis at the band's file index.  For a
    // basis in ascending order (every file Radiance writes) and for any two
    // bands exchanged that is the inverse permutation; it is kept for others too.
    void setup() {
        std::vector<size_t> perm(thetas.size());
        std::iota(perm.begin(), perm.end(), 0);
        std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return thetas[a].upper < thetas[b].upper; });
        std::sort(thetas.begin(), thetas.end(), [](const ThetaBasis& a, const ThetaBasis& b) { return a.upper < b.upper; });
        lin_offset.resize(thetas.size());
        uint32_t off = 0;
        for (size_t i = 0; i < thetas.size(); ++i) {
            lin_offset[i] = off;
            off += thetas[i].phi_count;
        }
        entries = off;
        permutation.clear();
        for (size_t i = 0; i < thetas.size(); ++i) {
            const size_t ri = perm[i];
            for (uint32_t j = 0; j < thetas[ri].phi_count; ++j) permutation.push_back(lin_offset[ri] + j);
        }
    }
};

struct KlemsComponent {
    std::shared_ptr<KlemsBasis> row, col;
    std::vector<float> matrix; // row-major, row->entries x col->entries

    // KlemsComponent::computeTotal with the projected solid angles
    float total() const {
        float sum = 0;
        size_t r = 0;
        for (const ThetaBasis& rt : row->thetas)
            for (uint32_t ip = 0; ip < rt.phi_count; ++ip, ++r) {
                size_t c = 0;
                for (const ThetaBasis& ct : col->thetas)
                    for (uint32_t jp = 0; jp < ct.phi_count; ++jp, ++c)
                        sum += matrix[r * col->entries + c] * rt.phi_solid_angle * ct.phi_solid_angle;
            }
        return sum;
    }
};

float number_of(const XmlNode* n) { return n ? std::strtof(n->text.c_str(), nullptr) : 0.0f; }

} // namespace

bool load_klems_xml(const std::string& xml_text, MeasuredData& out, std::string& error) {
    out = MeasuredData{};
    XmlNode doc;
    if (!parse_xml(xml_text, doc, error)) return false;
    const XmlNode* layer = find_layer(doc, error);
    if (!layer) return false;
    const XmlNode* dd = layer->child("DataDefinition");
    if (!dd) {
        error = "no DataDefinition element";
        return false;
    }
    const std::string type = dd->child_value("IncidentDataStructure");
    const bool row_based = type == "Rows";
    if (!row_based && type != "Columns") {
        error = "expected IncidentDataStructure 'Columns' or 'Rows' but got '" + type + "'";
        return false;
    }
    std::map<std::string, std::shared_ptr<KlemsBasis>> all_basis;
    for (const XmlNode& ab : dd->children) {
        if (ab.name != "AngleBasis") continue;
        if (!ab.child("AngleBasisName")) {
            error = "AngleBasis has no name";
            return false;
        }
        auto full = std::make_shared<KlemsBasis>();
        for (const XmlNode& blk : ab.children) {
            if (blk.name != "AngleBasisBlock") continue;
            ThetaBasis b{};
            const XmlNode* bounds = blk.child("ThetaBounds");
            b.lower = kDeg2Rad * number_of(bounds ? bounds->child("LowerTheta") : nullptr);
            b.upper = kDeg2Rad * number_of(bounds ? bounds->child("UpperTheta") : nullptr);
            const XmlNode* nphis = blk.child("nPhis");
            const long np = nphis ? std::strtol(nphis->text.c_str(), nullptr, 10) : 0;
            b.phi_count = np > 0 && np <= 4096 ? (uint32_t)np : 0;
            const float sa = std::cos(b.lower), sb = std::cos(b.upper);
            b.phi_solid_angle = b.phi_count > 0 ? (kPi * (sa * sa - sb * sb) / b.phi_count) : 0.0f;
            const XmlNode* theta = blk.child("Theta");
            b.center = theta ? kDeg2Rad * number_of(theta) : (b.upper + b.lower) / 2;
            if (!(b.phi_count > 0 && b.lower < b.upper) || !std::isfinite(b.center)) {
                error = "invalid AngleBasisBlock given";
                return false;
            }
            if (full->thetas.size() >= KLEMS_MAX_THETAS) {
                error = "more than " + std::to_string(KLEMS_MAX_THETAS) + " theta bands in an angle basis";
                return false;
            }
            full->thetas.push_back(b);
        }
        if (full->thetas.empty()) {
            error = "AngleBasis without an AngleBasisBlock";
            return false;
        }
        full->setup();
        all_basis[ab.child_value("AngleBasisName")] = full;
    }
    if (all_basis.empty()) {
        error = "no basis given";
        return false;
    }
    std::shared_ptr<KlemsComponent> comp[4];
    for (const XmlNode& data : layer->children) {
        if (data.name != "WavelengthData") continue;
        if (data.child_value("Wavelength") != "Visible") continue;
        const XmlNode* block = data.child("WavelengthDataBlock");
        if (!block) {
            error = "no WavelengthDataBlock given";
            return false;
        }
        if (!block->child("ColumnAngleBasis") || !block->child("RowAngleBasis")) {
            error = "WavelengthDataBlock has no column or row basis given";
            return false;
        }
        auto cb = all_basis.find(block->child_value("ColumnAngleBasis")); // incoming direction
        auto rb = all_basis.find(block->child_value("RowAngleBasis"));    // outgoing direction
        if (cb == all_basis.end() || rb == all_basis.end()) {
            error = "WavelengthDataBlock has no known column or row basis given";
            return false;
        }
        auto c = std::make_shared<KlemsComponent>();
        c->row = rb->second;
        c->col = cb->second;
        const size_t rows = c->row->entries, cols = c->col->entries, size = rows * cols;
        c->matrix.assign(size, 0.0f);
        const XmlNode* sd = block->child("ScatteringData");
        const std::string text = sd ? sd->text : std::string();
        const char* s = text.c_str();
        size_t ind = 0;
        while (ind < size && *s) {
            char* end = nullptr;
            float value = std::strtof(s, &end);
            if (s == end) { // no number here: skip the character
                ++s;
                continue;
            }
            if (std::signbit(value) || !std::isfinite(value)) value = 0; // negative and non-finite entries are 0
            size_t row, col;
            if (row_based) {
                row = ind % cols;
                col = ind / cols;
            } else {
                row = ind / cols;
                col = ind % cols;
            }
            if (row >= rows || col >= cols) {
                error = "'Rows' order needs as many row as column patches";
                return false;
            }
            c->matrix[(size_t)c->row->permutation[row] * cols + c->col->permutation[col]] = value;
            ++ind;
            s = end;
        }
        if (ind != size) {
            error = "given scattered data is not of length " + std::to_string(size);
            return false;
        }
        comp[component_of(block->child_value("WavelengthDataDirection"))] = c;
    }
    // both transmission parts are equal unless given otherwise
    if (!comp[BT] || (comp[FT] && comp[BT]->total() <= kFltEps)) comp[BT] = comp[FT];
    if (!comp[FT] || (comp[BT] && comp[FT]->total() <= kFltEps)) comp[FT] = comp[BT];
    if (!comp[FT] && !comp[BT]) {
        error = "no transmission data found";
        return false;
    }
    out.m.kind = IGX_MEASURED_KLEMS;
    std::map<const KlemsComponent*, uint32_t> placed;
    for (int k = 0; k < 4; ++k) {
        igx_measured_component& s = out.m.component[k];
        s.offset = (uint32_t)out.words.size();
        if (!comp[k]) continue; // a missing reflection component is black: total 0, no words
        const KlemsComponent& c = *comp[k];
        auto at = placed.find(&c);
        if (at == placed.end()) {
            at = placed.emplace(&c, (uint32_t)out.words.size()).first;
            auto put = [&](const void* w) {
                uint32_t u;
                std::memcpy(&u, w, 4);
                out.words.push_back(u);
            };
            for (const KlemsBasis* b : {c.row.get(), c.col.get()}) {
                for (const ThetaBasis& t : b->thetas) {
                    put(&t.center);
                    put(&t.lower);
                    put(&t.upper);
                    put(&t.phi_count);
                }
                for (uint32_t o : b->lin_offset) put(&o);
            }
            const size_t o = out.words.size();
            out.words.resize(o + c.matrix.size());
            std::memcpy(&out.words[o], c.matrix.data(), 4 * c.matrix.size());
        }
        s.offset = at->second;
        s.total = c.total();
        if (!std::isfinite(s.total)) {
            error = "scatter data sums to no finite total";
            return false;
        }
        s.theta_count[0] = (uint32_t)c.row->thetas.size();
        s.theta_count[1] = (uint32_t)c.col->thetas.size();
        s.entry_count[0] = c.row->entries;
        s.entry_count[1] = c.col->entries;
    }
    out.m.num_words = (uint32_t)out.words.size();
    out.m.words = out.words.data();
    return true;
}

bool load_measured_file(const std::string& path, int kind, MeasuredData& out, std::string& error) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        error = "cannot open '" + path + "'";
        return false;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    const bool ok = kind == IGX_MEASURED_KLEMS ? load_klems_xml(ss.str(), out, error) : load_tensortree_xml(ss.str(), out, error);
    if (!ok) error = "'" + path + "': " + error;
    return ok;
}

} // namespace igx
