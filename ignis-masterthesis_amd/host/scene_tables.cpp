// build_scene_tables: an igx_scene_desc as the device's flat tables (scene_tables.h).
#include "scene_tables.h"

#include "env_cdf.h"

#include "cie_sky.h"
#include "measured_bsdf.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <exception>
#include <map>

using namespace igxd;

namespace igx {

void order_hot_nodes(std::vector<Float4>& nodes, int format, std::vector<Float4>& inst, int& tlas_root, size_t front) {
    const int nf4 = format == 4 ? 8 : 4;
    const size_t nn = nodes.size() / nf4;
    if (nn == 0 || front == 0) return;
    const int width = format == 2 ? 2 : 4;
    auto ref = [&](size_t n, int k) -> int32_t& {
        return reinterpret_cast<int32_t*>(&nodes[n * nf4])[format == 4 ? 24 + k : 12 + k];
    };
    auto box = [&](size_t n, int k, float lo[3], float hi[3]) {
        const float* f = reinterpret_cast<const float*>(&nodes[n * nf4]);
        if (format == 5) { // origin + code * scale (Bvh4QNode)
            const uint32_t* u = reinterpret_cast<const uint32_t*>(f);
            const float sc[3] = {f[3], f[4], f[5]};
            for (int a = 0; a < 3; ++a) {
                lo[a] = f[a] + (float)((u[6 + 2 * a] >> (8 * k)) & 255u) * sc[a];
                hi[a] = f[a] + (float)((u[7 + 2 * a] >> (8 * k)) & 255u) * sc[a];
            }
            if (ref(n, k) == kEmptyRef) lo[0] = INFINITY;
            return;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = width == 4 ? f[8 * a + k] : f[6 * k + 2 * a];
            hi[a] = width == 4 ? f[8 * a + 4 + k] : f[6 * k + 2 * a + 1];
        }
    };
    auto half_area = [](const float lo[3], const float hi[3]) -> double {
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || lo[a] > hi[a]) return 0.0;
        const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    // children of node n with the node's likelihood pn: f(child ref, child likelihood)
    auto children = [&](size_t n, double pn, auto&& f) {
        float ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double ak[4] = {0, 0, 0, 0};
        for (int k = 0; k < width; ++k) {
            float lo[3], hi[3];
            box(n, k, lo, hi);
            ak[k] = half_area(lo, hi);
            if (ak[k] <= 0) continue;
            for (int a = 0; a < 3; ++a) {
                ulo[a] = std::min(ulo[a], lo[a]);
                uhi[a] = std::max(uhi[a], hi[a]);
            }
        }
        const double ua = half_area(ulo, uhi);
        for (int k = 0; k < width; ++k) {
            const int32_t r = ref(n, k);
            if (r == kEmptyRef || ak[k] <= 0) continue;
            f(r, ua > 0 ? pn * std::min(1.0, ak[k] / ua) : pn);
        }
    };
    std::vector<double> p(nn, 0.0), pblas(nn, 0.0);
    auto instances = [&](int32_t leaf, double pl) { // TLAS leaf: its instances' BLAS roots
        const int code = ~leaf;
        const int first = code >> kLeafCountBits, count = (code & ((1 << kLeafCountBits) - 1)) + 1;
        for (int k = 0; k < count; ++k) {
            Int4 info;
            std::memcpy(&info, &inst[4 * (size_t)(first + k) + 3], 16);
            if (info.y == 0 && info.z >= 0 && (size_t)info.z < nn) pblas[info.z] += pl;
        }
    };
    std::vector<std::pair<int32_t, double>> todo;
    if (tlas_root >= 0) todo.push_back({tlas_root, 1.0});
    else if (!inst.empty()) instances(tlas_root, 1.0); // one entity: the root is its leaf
    while (!todo.empty()) { // TLAS (a tree)
        const auto [n, pn] = todo.back();
        todo.pop_back();
        p[n] += pn;
        children((size_t)n, pn, [&](int32_t r, double pc) {
            if (r >= 0) todo.push_back({r, pc});
            else instances(r, pc);
        });
    }
    for (size_t r = 0; r < nn; ++r) { // every BLAS from its root (a BLAS is a tree; shared BLAS summed at the root)
        if (pblas[r] <= 0) continue;
        todo.push_back({(int32_t)r, pblas[r]});
        while (!todo.empty()) {
            const auto [n, pn] = todo.back();
            todo.pop_back();
            p[n] += pn;
            children((size_t)n, pn, [&](int32_t c, double pc) {
                if (c >= 0) todo.push_back({c, pc});
            });
        }
    }
    std::vector<int32_t> order(nn);
    for (size_t i = 0; i < nn; ++i) order[i] = (int32_t)i;
    front = std::min(front, nn);
    std::partial_sort(order.begin(), order.begin() + front, order.end(), [&](int32_t a, int32_t b) {
        return p[a] != p[b] ? p[a] > p[b] : a < b;
    });
    std::vector<int32_t> newidx(nn, -1);
    for (size_t i = 0; i < front; ++i) newidx[order[i]] = (int32_t)i;
    int32_t next = (int32_t)front;
    for (size_t i = 0; i < nn; ++i)
        if (newidx[i] < 0) newidx[i] = next++;
    std::vector<Float4> out(nodes.size());
    for (size_t i = 0; i < nn; ++i) std::copy(&nodes[i * nf4], &nodes[i * nf4] + nf4, &out[(size_t)newidx[i] * nf4]);
    nodes.swap(out);
    for (size_t i = 0; i < nn; ++i)
        for (int k = 0; k < width; ++k)
            if (ref(i, k) >= 0) ref(i, k) = newidx[ref(i, k)];
    for (size_t slot = 0; slot < inst.size() / 4; ++slot) {
        Int4 info;
        std::memcpy(&info, &inst[4 * slot + 3], 16);
        if (info.y == 0 && info.z >= 0) {
            info.z = newidx[info.z];
            std::memcpy(&inst[4 * slot + 3], &info, 16);
        }
    }
    if (tlas_root >= 0) tlas_root = newidx[tlas_root];
}

bool closed_mesh(const igx_mesh& m) {
    if (m.num_faces < 4 || m.num_faces > (1u << 20)) return false;
    std::map<std::array<float, 3>, uint32_t> weld;
    std::vector<uint32_t> id(m.num_vertices);
    for (uint32_t v = 0; v < m.num_vertices; ++v)
        id[v] = weld.emplace(std::array<float, 3>{m.vertices[3 * v], m.vertices[3 * v + 1], m.vertices[3 * v + 2]}, (uint32_t)weld.size()).first->second;
    std::map<std::pair<uint32_t, uint32_t>, int> edges;
    for (uint32_t f = 0; f < m.num_faces; ++f)
        for (int k = 0; k < 3; ++k) {
            uint32_t a = id[m.indices[3 * f + k]], b = id[m.indices[3 * f + (k + 1) % 3]];
            if (a == b) return false;
            ++edges[{std::min(a, b), std::max(a, b)}];
        }
    for (const auto& e : edges)
        if (e.second != 2) return false;
    return true;
}

namespace {

Float4 bits4(const Int4& i) {
    Float4 f;
    std::memcpy(&f, &i, 16);
    return f;
}

} // namespace

igx_status build_scene_tables(const igx_scene_desc& desc, const SceneBuildOptions& opt, SceneTables& out, std::string& error) {
    auto fail = [&](igx_status s, const std::string& msg) {
        error = msg;
        return s;
    };
    out = SceneTables{};

    // ---- phase 1: BVH2 of every trimesh shape and of the entity TLAS ------
    std::vector<BvhBuildResult> brs(desc.num_shapes);
    int blas_depth2 = 0;
    for (uint32_t s = 0; s < desc.num_shapes; ++s) {
        const igx_shape& sh = desc.shapes[s];
        if (sh.type == IGX_SHAPE_SPHERE) continue;
        if (sh.mesh < 0 || (uint32_t)sh.mesh >= desc.num_meshes)
            return fail(IGX_ERR_INVALID_ARGUMENT, "shape references an invalid mesh");
        const igx_mesh& m = desc.meshes[sh.mesh];
        BvhBuildInput bi;
        bi.bmin.resize(3 * m.num_faces);
        bi.bmax.resize(3 * m.num_faces);
        bi.centroid.resize(3 * m.num_faces);
        for (uint32_t f = 0; f < m.num_faces; ++f) {
            for (int a = 0; a < 3; ++a) {
                float lo = 3.4e38f, hi = -3.4e38f;
                for (int k = 0; k < 3; ++k) {
                    uint32_t vi = m.indices[3 * f + k];
                    if (vi >= m.num_vertices) return fail(IGX_ERR_INVALID_ARGUMENT, "mesh index out of range");
                    float v = m.vertices[3 * vi + a];
                    lo = std::min(lo, v);
                    hi = std::max(hi, v);
                }
                bi.bmin[3 * f + a] = lo;
                bi.bmax[3 * f + a] = hi;
                bi.centroid[3 * f + a] = 0.5f * (lo + hi);
            }
        }
        if (sh.ref_bvh && !opt.rebuild_bvh) {
            // the reference loader's BLAS (Node2 + Tri1, TriMeshProvider.cpp:553-554)
            std::string err;
            if (!bvh2_from_reference(sh.ref_bvh, sh.ref_bvh_bytes, m.num_faces, brs[s], err))
                return fail(IGX_ERR_INVALID_ARGUMENT, "shape " + std::to_string(s) + ": " + err);
            blas_depth2 = std::max(blas_depth2, brs[s].depth);
            continue;
        }
        try {
            if (opt.spatial_splits && m.num_faces <= SPATIAL_SPLIT_MAX_FACES) {
                std::vector<float> tv(9 * (size_t)m.num_faces);
                for (uint32_t f = 0; f < m.num_faces; ++f)
                    for (int k = 0; k < 3; ++k)
                        for (int a = 0; a < 3; ++a) tv[9 * (size_t)f + 3 * k + a] = m.vertices[3 * m.indices[3 * f + k] + a];
                brs[s] = build_sbvh2(bi, tv, opt.leaf_size);
            } else {
                brs[s] = build_bvh2(bi, opt.leaf_size, opt.bvh_bins, opt.sah_node_cost);
            }
        } catch (const std::exception& ex) {
            return fail(IGX_ERR_INVALID_ARGUMENT, ex.what());
        }
        blas_depth2 = std::max(blas_depth2, brs[s].depth);
    }
    BvhBuildResult tlas_br;
    if (desc.num_entities > 0) {
        BvhBuildInput bi;
        for (uint32_t e = 0; e < desc.num_entities; ++e) {
            const igx_entity& en = desc.entities[e];
            if (en.shape < 0 || (uint32_t)en.shape >= desc.num_shapes)
                return fail(IGX_ERR_INVALID_ARGUMENT, "entity references an invalid shape");
            if (en.material < 0 || (uint32_t)en.material >= desc.num_materials)
                return fail(IGX_ERR_INVALID_ARGUMENT, "entity references an invalid material");
            for (int a = 0; a < 3; ++a) {
                bi.bmin.push_back(en.bbox_min[a]);
                bi.bmax.push_back(en.bbox_max[a]);
                bi.centroid.push_back(0.5f * (en.bbox_min[a] + en.bbox_max[a]));
            }
        }
        tlas_br = build_bvh2(bi, 1, opt.bvh_bins_tlas);
    }
    // Node width: BVH2 while its whole stack fits the LDS column (fewer,
    // cheaper node steps on small scenes), else 4-wide nodes (half the node
    // iterations on deep trees; the deepest entries spill).  Option
    // "bvh_width" forces either.
    const int width = opt.bvh_width_opt == 2 || opt.bvh_width_opt == 4
                          ? opt.bvh_width_opt
                          : (tlas_br.depth + blas_depth2 + 3 <= LDS_STACK ? 2 : 4);
    // 4-wide nodes quantised to 64 B (Bvh4QNode) on the split schedule's
    // scenes, whose node fetches go to the Infinity Cache / HBM (soup-16M frame
    // 74.7 -> 70.0, soup-1M 98.2 -> 92.8 ms); where the tables stay on chip the
    // decode only costs instructions (primitives 8.6 -> 9.4, S-deep 46.7 -> 49.5)
    size_t est_tri = 0;
    for (const auto& b : brs) est_tri += b.prim_order.size();
    const size_t est_bytes = est_tri * 48 + (size_t)desc.num_entities * 64 + (est_tri / 2 + desc.num_entities) * 128;
    const bool quantize = width == 4 && (opt.quantize_opt == 1 || (opt.quantize_opt < 0 && est_bytes > SPLIT_TABLE_BYTES));
    const int nf4 = quantize ? 4 : node_f4(width);

    // ---- phase 2: node, triangle and instance tables ----------------------
    auto& nodes = out.nodes; // nf4 Float4s per node
    auto &tris = out.tris, &vtx = out.vtx, &nrm = out.nrm, &spheres = out.spheres;
    auto& uvs = out.uvs;
    bool textured = false;
    for (uint32_t i = 0; i < desc.num_materials; ++i) textured = textured || desc.materials[i].texture != IGX_TEXTURE_NONE;
    auto& idx = out.idx;
    // per face: vertex normals and indices in one record (SceneView::fsh),
    // for scenes with at most FACE_SHADE_MAX faces over all meshes (48 B each)
    auto& fsh = out.fsh;
    size_t total_faces = 0;
    for (uint32_t i = 0; i < desc.num_shapes; ++i)
        if (desc.shapes[i].type != IGX_SHAPE_SPHERE && desc.shapes[i].mesh >= 0) total_faces += desc.meshes[desc.shapes[i].mesh].num_faces;
    const bool with_fsh = opt.face_shade_opt && total_faces <= FACE_SHADE_MAX;
    // Append a built BVH2 (as Node2, or collapsed to 4-wide nodes) to the
    // unified node array: inner refs move by the array offset, leaf codes by
    // `leaf_off` slots.  Returns the node offset; `need` = stack entries the
    // tree can occupy.
    auto append_nodes = [&](const BvhBuildResult& br, int leaf_off, int& need) -> int {
        const int node_off = (int)(nodes.size() / nf4);
        auto move_leaf = [&](int32_t ref) {
            int code = ~ref;
            return encode_leaf((code >> kLeafCountBits) + leaf_off, (code & ((1 << kLeafCountBits) - 1)) + 1);
        };
        if (width == 2) {
            for (auto nd : br.nodes) {
                for (int k = 0; k < 2; ++k) {
                    if (nd.ref[k] >= 0) nd.ref[k] += node_off;
                    else if (nd.ref[k] != kEmptyRef && nd.b[k * 6] <= nd.b[k * 6 + 1])
                        nd.ref[k] = move_leaf(nd.ref[k]); // empty and absent children keep their code
                }
                Float4 f[4];
                std::memcpy(f, &nd, 64);
                nodes.insert(nodes.end(), f, f + 4);
            }
            need = br.depth;
        } else {
            Bvh4Result b4 = collapse_bvh4(br);
            for (auto nd : b4.nodes) {
                for (int k = 0; k < 4; ++k) {
                    if (nd.ref[k] >= 0) nd.ref[k] += node_off;
                    else if (nd.ref[k] != kEmptyRef) nd.ref[k] = move_leaf(nd.ref[k]);
                }
                if (quantize) {
                    const Bvh4QNode qn = quantize_bvh4(nd);
                    Float4 f[4];
                    std::memcpy(f, &qn, 64);
                    nodes.insert(nodes.end(), f, f + 4);
                } else {
                    Float4 f[8];
                    std::memcpy(f, &nd, 128);
                    nodes.insert(nodes.end(), f, f + 8);
                }
            }
            need = b4.stack_need;
        }
        return node_off;
    };
    struct ShapeDev { int type, root, vtx_off, idx_off_or_sphere; };
    std::vector<ShapeDev> sdev(desc.num_shapes);
    int blas_depth = 0;
    for (uint32_t s = 0; s < desc.num_shapes; ++s) {
        const igx_shape& sh = desc.shapes[s];
        if (sh.type == IGX_SHAPE_SPHERE) {
            sdev[s] = {1, -1, 0, (int)spheres.size()};
            spheres.push_back(Float4{sh.sphere[0], sh.sphere[1], sh.sphere[2], sh.sphere[3]});
            continue;
        }
        const igx_mesh& m = desc.meshes[sh.mesh];
        const BvhBuildResult& br = brs[s];
        int tri_off = (int)(tris.size() / 3);
        if (tri_off + br.prim_order.size() >= (size_t)(1 << 26))
            return fail(IGX_ERR_UNSUPPORTED, "too many triangles for the leaf encoding");
        int need = 0;
        int node_off = append_nodes(br, tri_off, need);
        blas_depth = std::max(blas_depth, need);
        for (uint32_t slot = 0; slot < br.prim_order.size(); ++slot) {
            uint32_t f = br.prim_order[slot];
            const uint32_t* ix = m.indices + 3 * f;
            const float* v0 = m.vertices + 3 * ix[0];
            const float* v1 = m.vertices + 3 * ix[1];
            const float* v2 = m.vertices + 3 * ix[2];
            // Tri1 (shapes/trimesh.art:107-114; TriBVHAdapter.h:148-158): e1 = v0 - v1, e2 = v2 - v0
            Float4 q0{v0[0], v0[1], v0[2], 0};
            int32_t pid = (int32_t)f;
            std::memcpy(&q0.w, &pid, 4);
            tris.push_back(q0);
            tris.push_back(Float4{v0[0] - v1[0], v0[1] - v1[1], v0[2] - v1[2], 0});
            tris.push_back(Float4{v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2], 0});
        }
        // a BLAS that is a single leaf is entered at the leaf itself
        int root_ref = node_off;
        if (br.root_is_leaf) {
            int code = ~br.root_leaf_ref;
            root_ref = encode_leaf((code >> kLeafCountBits) + tri_off, (code & ((1 << kLeafCountBits) - 1)) + 1);
        }
        sdev[s] = {0, root_ref, (int)vtx.size(), (int)idx.size()};
        for (uint32_t v = 0; v < m.num_vertices; ++v) {
            vtx.push_back(Float4{m.vertices[3 * v], m.vertices[3 * v + 1], m.vertices[3 * v + 2], 0});
            nrm.push_back(Float4{m.normals[3 * v], m.normals[3 * v + 1], m.normals[3 * v + 2], 0});
            if (textured) uvs.push_back(m.texcoords ? Float2{m.texcoords[2 * v], m.texcoords[2 * v + 1]} : Float2{0, 0});
        }
        for (uint32_t f = 0; f < m.num_faces; ++f)
            idx.push_back(Int4{(int)m.indices[3 * f], (int)m.indices[3 * f + 1], (int)m.indices[3 * f + 2], 0});
        if (with_fsh)
            for (uint32_t f = 0; f < m.num_faces; ++f)
                for (int k = 0; k < 3; ++k) {
                    const uint32_t v = m.indices[3 * f + k];
                    Float4 r{m.normals[3 * v], m.normals[3 * v + 1], m.normals[3 * v + 2], 0};
                    const int vi = (int)v;
                    std::memcpy(&r.w, &vi, 4);
                    fsh.push_back(r);
                }
        brs[s] = BvhBuildResult{}; // release the host copy
    }

    // ---- TLAS over entities (leaf size 1), instance records ---------------
    auto &inst = out.inst, &ent = out.ent;
    auto& ent_fn = out.ent_fn;
    auto& fn_tab = out.fn_tab;
    auto& ent_enc = out.ent_enc;
    auto& enc_tab = out.enc_tab;
    auto& enc_box = out.enc_box;
    int tlas_root = -1;
    int tlas_depth = 0;
    if (desc.num_entities > 0) {
        const BvhBuildResult& br = tlas_br;
        int node_off = append_nodes(br, 0, tlas_depth);
        tlas_root = br.root_is_leaf ? br.root_leaf_ref : node_off; // single entity: start at its leaf
        for (uint32_t slot = 0; slot < br.prim_order.size(); ++slot) {
            uint32_t e = br.prim_order[slot];
            const igx_entity& en = desc.entities[e];
            const ShapeDev& sd = sdev[en.shape];
            for (int r = 0; r < 3; ++r)
                inst.push_back(Float4{en.to_local[r * 4 + 0], en.to_local[r * 4 + 1], en.to_local[r * 4 + 2], en.to_local[r * 4 + 3]});
            static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            const float* m = en.to_local;
            const bool linear_identity = m[0] == 1 && m[1] == 0 && m[2] == 0 && m[4] == 0 && m[5] == 1 && m[6] == 0 &&
                                         m[8] == 0 && m[9] == 0 && m[10] == 1 && std::isfinite(m[3]) &&
                                         std::isfinite(m[7]) && std::isfinite(m[11]);
            const bool identity = sd.type == 0 && std::equal(m, m + 12, kIdentity);
            const bool translate = sd.type == 0 && !identity && linear_identity;
            const uint32_t iflags = (en.flags & ~(INST_IDENTITY | INST_TRANSLATE)) | (identity ? INST_IDENTITY : 0u) |
                                    (translate ? INST_TRANSLATE : 0u);
            inst.push_back(bits4(Int4{(int)e, sd.type, sd.type == 1 ? sd.idx_off_or_sphere : sd.root, (int)iflags}));
        }
        // enclosing entities (trace_enclosed): a closed mesh of a non-thin
        // dielectric whose world box keeps a margin from every other entity's
        // box, at most MAX_ENCLOSING of them (ent_enc: index, enc_tab: entity and TLAS leaf slot)
        ent_enc.assign(desc.num_entities, -1);
        if (opt.enclosing_opt && desc.num_entities <= 4096) {
            float slo[3], shi[3];
            for (int a = 0; a < 3; ++a) { slo[a] = desc.scene_bbox_min[a]; shi[a] = desc.scene_bbox_max[a]; }
            const float margin = 1e-4f * std::max({shi[0] - slo[0], shi[1] - slo[1], shi[2] - slo[2], 1e-6f});
            std::vector<int> closed(desc.num_shapes, -1);
            for (uint32_t slot = 0; slot < br.prim_order.size(); ++slot) {
                const uint32_t e = br.prim_order[slot];
                const igx_entity& en = desc.entities[e];
                const igx_shape& sh = desc.shapes[en.shape];
                const igx_material& mat = desc.materials[en.material];
                if (sh.type != IGX_SHAPE_TRIMESH || mat.bsdf_type != IGX_BSDF_DIELECTRIC || mat.thin) continue;
                if (closed[en.shape] < 0) closed[en.shape] = closed_mesh(desc.meshes[sh.mesh]) ? 1 : 0;
                if (!closed[en.shape]) continue;
                bool apart = true;
                for (uint32_t o = 0; o < desc.num_entities && apart; ++o) {
                    if (o == e) continue;
                    const igx_entity& q = desc.entities[o];
                    bool overlap = true;
                    for (int a = 0; a < 3; ++a)
                        overlap = overlap && q.bbox_min[a] <= en.bbox_max[a] + margin && en.bbox_min[a] <= q.bbox_max[a] + margin;
                    apart = !overlap;
                }
                if (apart && (int)enc_tab.size() < MAX_ENCLOSING) {
                    ent_enc[e] = (int)enc_tab.size();
                    enc_tab.push_back(Int2{(int)e, (int)slot});
                    enc_box.push_back(Float4{en.bbox_min[0], en.bbox_min[1], en.bbox_min[2], 0});
                    enc_box.push_back(Float4{en.bbox_max[0], en.bbox_max[1], en.bbox_max[2], 0});
                }
            }
        }
        for (uint32_t e = 0; e < desc.num_entities; ++e) {
            const igx_entity& en = desc.entities[e];
            const ShapeDev& sd = sdev[en.shape];
            for (int r = 0; r < 3; ++r)
                ent.push_back(Float4{en.to_global[r * 4 + 0], en.to_global[r * 4 + 1], en.to_global[r * 4 + 2], en.to_global[r * 4 + 3]});
            for (int r = 0; r < 3; ++r) ent.push_back(Float4{en.normal[r * 3 + 0], en.normal[r * 3 + 1], en.normal[r * 3 + 2], 0});
            ent.push_back(bits4(Int4{sd.type, en.material, sd.vtx_off, sd.idx_off_or_sphere}));
        }
        // world-space unit face normals of every (mesh entity, face) when the
        // scene has few face instances: surface_element then skips three vertex
        // loads and transforms per hit.  make_triangle (core/triangle.art:11-26)
        // on the entity's to_global rows, in float, same operation order.
        size_t face_instances = 0;
        for (uint32_t e = 0; e < desc.num_entities; ++e) {
            const igx_shape& sh = desc.shapes[desc.entities[e].shape];
            if (sh.type == IGX_SHAPE_TRIMESH && sh.mesh >= 0) face_instances += desc.meshes[sh.mesh].num_faces;
        }
        if (opt.face_normals_opt && face_instances > 0 && face_instances <= FACE_NORMAL_TABLE_MAX) {
            ent_fn.assign(desc.num_entities, -1);
            fn_tab.reserve(face_instances);
            for (uint32_t e = 0; e < desc.num_entities; ++e) {
                const igx_entity& en = desc.entities[e];
                const igx_shape& sh = desc.shapes[en.shape];
                if (sh.type != IGX_SHAPE_TRIMESH || sh.mesh < 0) continue;
                const igx_mesh& m = desc.meshes[sh.mesh];
                ent_fn[e] = (int)fn_tab.size();
                const float* T = en.to_global;
                auto xf = [&](uint32_t v, float o[3]) {
                    const float* p = m.vertices + 3 * v;
                    for (int r = 0; r < 3; ++r) {
                        float acc = T[r * 4 + 0] * p[0];
                        acc = acc + T[r * 4 + 1] * p[1];
                        acc = acc + T[r * 4 + 2] * p[2];
                        o[r] = acc + T[r * 4 + 3];
                    }
                };
                for (uint32_t f = 0; f < m.num_faces; ++f) {
                    float v0[3], v1[3], v2[3];
                    xf(m.indices[3 * f], v0);
                    xf(m.indices[3 * f + 1], v1);
                    xf(m.indices[3 * f + 2], v2);
                    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
                    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
                    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                    float nn2 = n[0] * n[0];
                    nn2 = nn2 + n[1] * n[1];
                    nn2 = nn2 + n[2] * n[2];
                    const float inv = 1 / std::sqrt(nn2);
                    fn_tab.push_back(Float4{n[0] * inv, n[1] * inv, n[2] * inv, 0});
                }
            }
        }
        // the entity's face-normal offset in row 3 .w of its record, read
        // with the normal matrix by surface_element's fsh path (-1: none)
        for (uint32_t e = 0; e < desc.num_entities; ++e) {
            const int off = ent_fn.empty() ? -1 : ent_fn[e];
            std::memcpy(&ent[ENT_STRIDE * e + 3].w, &off, 4);
        }
    }

    // ---- materials and lights (infinite lights first) --------------------
    std::vector<int> light_remap(desc.num_lights, -1);
    bool env_mapped = false; // an image environment map: the texture table is needed without a textured material, too
    auto& lights = out.lights;
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t l = 0; l < desc.num_lights; ++l) {
            const igx_light& L = desc.lights[l];
            bool infinite = L.type == IGX_LIGHT_ENV || L.type == IGX_LIGHT_DIRECTIONAL || L.type == IGX_LIGHT_SUN ||
                            L.type == IGX_LIGHT_CIE || L.type == IGX_LIGHT_ENVMAP; // a sky is infinite and not delta
            if ((pass == 0) != infinite) continue;
            DevLight d{};
            d.type = L.type;
            d.infinite = infinite ? 1 : 0;
            d.delta = (L.type == IGX_LIGHT_POINT || L.type == IGX_LIGHT_SPOT || L.type == IGX_LIGHT_DIRECTIONAL ||
                       L.type == IGX_LIGHT_SUN) ? 1 : 0;
            for (int i = 0; i < 3; ++i) d.radiance[i] = L.radiance[i];
            if (L.type == IGX_LIGHT_PLANE) {
                // make_plane_area_emitter constants (light/area.art:107-115)
                float xa[3] = {L.x_axis[0], L.x_axis[1], L.x_axis[2]};
                float ya[3] = {L.y_axis[0], L.y_axis[1], L.y_axis[2]};
                float width = std::sqrt(xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2]);
                float height = std::sqrt(ya[0] * ya[0] + ya[1] * ya[1] + ya[2] * ya[2]);
                float iw = 1 / width, ih = 1 / height;
                for (int i = 0; i < 3; ++i) {
                    d.origin[i] = L.origin[i];
                    d.ex[i] = xa[i] * iw;
                    d.ey[i] = ya[i] * ih;
                    d.normal[i] = L.normal[i];
                }
                d.origin[3] = width;
                d.ex[3] = height;
                d.ey[3] = 1 / L.area;
                d.normal[3] = L.area;
            } else if (L.type == IGX_LIGHT_POINT) {
                for (int i = 0; i < 3; ++i) d.origin[i] = L.origin[i];
            } else if (L.type == IGX_LIGHT_SPOT) {
                for (int i = 0; i < 3; ++i) { d.origin[i] = L.origin[i]; d.normal[i] = L.normal[i]; }
                float cc = std::cos(L.cutoff), cf = std::cos(L.falloff);
                d.spot[0] = cc;
                d.spot[1] = cf;
                d.spot[2] = cf - cc;
            } else if (L.type == IGX_LIGHT_DIRECTIONAL) {
                for (int i = 0; i < 3; ++i) d.normal[i] = L.normal[i];
            } else if (L.type == IGX_LIGHT_SUN) {
                // make_sun_light constants (light/sun.art:4-8)
                for (int i = 0; i < 3; ++i) d.normal[i] = L.normal[i];
                float c = L.cutoff;
                float r = std::sqrt(1 - c * c) / c; // sun_radius_from_cos_angle
                d.spot[0] = c;
                d.spot[1] = 3.14159265359f * r * r;
            } else if (L.type == IGX_LIGHT_SPHERE || L.type == IGX_LIGHT_MESH) {
                if (L.entity < 0 || (uint32_t)L.entity >= desc.num_entities)
                    return fail(IGX_ERR_INVALID_ARGUMENT, "area light references an invalid entity");
                d.entity = L.entity;
                if (L.type == IGX_LIGHT_SPHERE) {
                    if (!(L.area > 0) || !(L.radius > 0))
                        return fail(IGX_ERR_INVALID_ARGUMENT, "sphere light needs a positive radius and area");
                    for (int i = 0; i < 3; ++i) d.origin[i] = L.origin[i];
                    d.origin[3] = L.radius;
                    d.spot[0] = L.area;
                } else {
                    const igx_shape& sh = desc.shapes[desc.entities[L.entity].shape];
                    if (sh.type != IGX_SHAPE_TRIMESH || sh.mesh < 0 || desc.meshes[sh.mesh].num_faces == 0)
                        return fail(IGX_ERR_INVALID_ARGUMENT, "mesh light needs a non-empty triangle entity");
                    d.spot[0] = (float)desc.meshes[sh.mesh].num_faces;
                }
            } else if (L.type == IGX_LIGHT_CIE) {
                if (L.sky_kind < IGX_SKY_UNIFORM || L.sky_kind > IGX_SKY_INTERMEDIATE)
                    return fail(IGX_ERR_INVALID_ARGUMENT, "invalid CIE sky kind");
                static_assert(offsetof(DevLight, radiance) == 16 && sizeof(DevLight) == 16 + sizeof(CieSky), "CieSky lives behind the DevLight header");
                const CieSky sky = make_cie_sky(L);
                std::memcpy(d.radiance, &sky, sizeof(sky));
            } else if (L.type == IGX_LIGHT_ENVMAP) {
                // its EnvMap record follows once the texture table stands (below)
                if (L.env_texture < 0 || (uint32_t)L.env_texture >= desc.num_textures)
                    return fail(IGX_ERR_INVALID_ARGUMENT, "environment map: texture index beyond the texture table");
                env_mapped = true;
            } else if (L.type != IGX_LIGHT_ENV) {
                return fail(IGX_ERR_UNSUPPORTED, "unsupported light type");
            }
            light_remap[l] = (int)lights.size();
            lights.push_back(d);
        }
    int num_infinite = 0;
    for (auto& l : lights) num_infinite += l.infinite;
    // NEE selector tables over the finite lights, in device order (light_select.h)
    std::vector<igx_light> finite_lights;
    for (uint32_t l = 0; l < desc.num_lights; ++l)
        if (light_remap[l] >= num_infinite) finite_lights.push_back(desc.lights[l]);
    // (pass 1 above numbers the finite lights in desc order, so this is device order)
    out.lsel = build_light_select(desc.technique.light_selector, (int)lights.size(), finite_lights);
    // Image textures: behind the texture coordinates, the uv table carries one
    // TexRecord per texture (32-B aligned) and then the texels of every image
    // (16-B aligned), so a lookup needs no further table pointer: the material
    // names its record, the record its texels, both as offsets into the table.
    std::vector<uint32_t> tex_record_at(desc.num_textures, 0); // in Float2 units
    if ((textured || env_mapped) && desc.num_textures) {
        if (!desc.textures || !desc.images) return fail(IGX_ERR_INVALID_ARGUMENT, "null texture or image table");
        auto pad_to = [&](size_t unit) { uvs.resize((uvs.size() + unit - 1) / unit * unit, Float2{0, 0}); };
        std::vector<uint32_t> image_at(desc.num_images, 0);
        size_t total = (uvs.size() + 3) / 4 * 4 + 4 * (size_t)desc.num_textures;
        for (uint32_t i = 0; i < desc.num_images; ++i) {
            const igx_image& im = desc.images[i];
            if (im.width < 1 || im.height < 1 || im.width > 16384 || im.height > 16384 || !im.pixels || im.format < IGX_IMAGE_RGBA8 ||
                im.format > IGX_IMAGE_FLOAT4)
                return fail(IGX_ERR_INVALID_ARGUMENT, "invalid image " + std::to_string(i));
            const size_t bytes = (size_t)im.width * im.height * (im.format == IGX_IMAGE_FLOAT4 ? 16 : im.format == IGX_IMAGE_MONO8 ? 1 : 4);
            total = (total + 1) / 2 * 2 + (bytes + 7) / 8;
        }
        if (total > 0x7fffffffu) return fail(IGX_ERR_UNSUPPORTED, "texture coordinates and images exceed 16 GB");
        pad_to(4);
        const size_t records = uvs.size();
        uvs.resize(records + 4 * (size_t)desc.num_textures, Float2{0, 0});
        for (uint32_t i = 0; i < desc.num_images; ++i) {
            const igx_image& im = desc.images[i];
            const size_t bytes = (size_t)im.width * im.height * (im.format == IGX_IMAGE_FLOAT4 ? 16 : im.format == IGX_IMAGE_MONO8 ? 1 : 4);
            pad_to(2);
            image_at[i] = (uint32_t)uvs.size();
            uvs.resize(uvs.size() + (bytes + 7) / 8, Float2{0, 0});
            std::memcpy(reinterpret_cast<uint8_t*>(uvs.data() + image_at[i]), im.pixels, bytes);
            out.image_bytes += bytes;
        }
        for (uint32_t t = 0; t < desc.num_textures; ++t) {
            const igx_texture& tx = desc.textures[t];
            if (tx.image < 0 || (uint32_t)tx.image >= desc.num_images || tx.filter < IGX_FILTER_NEAREST || tx.filter > IGX_FILTER_BICUBIC ||
                tx.wrap_u < IGX_WRAP_REPEAT || tx.wrap_u > IGX_WRAP_MIRROR || tx.wrap_v < IGX_WRAP_REPEAT || tx.wrap_v > IGX_WRAP_MIRROR)
                return fail(IGX_ERR_INVALID_ARGUMENT, "invalid texture " + std::to_string(t));
            const igx_image& im = desc.images[tx.image];
            const TexRecord r{im.width, im.height, im.format, tx.filter, tx.wrap_u, tx.wrap_v, image_at[tx.image], 0};
            tex_record_at[t] = (uint32_t)(records + 4 * (size_t)t);
            std::memcpy(reinterpret_cast<uint8_t*>(uvs.data() + tex_record_at[t]), &r, sizeof(r));
        }
        // Image environment maps: the CDF of each (host/env_cdf.h) goes behind the texels
        for (uint32_t l = 0; l < desc.num_lights; ++l) {
            const igx_light& L = desc.lights[l];
            if (L.type != IGX_LIGHT_ENVMAP) continue;
            const igx_texture& tx = desc.textures[L.env_texture];
            const igx_image& im = desc.images[tx.image];
            EnvMap e{};
            static_assert(offsetof(DevLight, radiance) == 16 && sizeof(DevLight) == 16 + sizeof(EnvMap), "EnvMap lives behind the DevLight header");
            for (int i = 0; i < 3; ++i) e.scale[i] = L.env_scale[i];
            for (int i = 0; i < 9; ++i) e.m[i] = L.sky_transform[i];
            for (int i = 0; i < 6; ++i) e.uv_transform[i] = tx.transform[i];
            e.texture = tex_record_at[L.env_texture];
            if (L.env_cdf && (im.width > 1 || im.height > 1)) {
                int bw = 0, bh = 0;
                std::vector<float> baked, table;
                bake_env_image(tx, im, bw, bh, baked);
                build_env_cdf(baked.data(), bw, bh, true, L.env_compensate != 0, table);
                pad_to(2);
                if (uvs.size() + (table.size() + 1) / 2 > 0x7fffffffu) return fail(IGX_ERR_UNSUPPORTED, "texture coordinates and images exceed 16 GB");
                e.cdf = (uint32_t)uvs.size();
                e.cdf_w = bw;
                e.cdf_h = bh;
                uvs.resize(uvs.size() + (table.size() + 1) / 2, Float2{0, 0});
                std::memcpy(reinterpret_cast<uint8_t*>(uvs.data() + e.cdf), table.data(), table.size() * sizeof(float));
                out.cdf_bytes += table.size() * sizeof(float);
            }
            std::memcpy(lights[light_remap[l]].radiance, &e, sizeof(e));
        }
    }
    // Measured BSDFs: every table is checked, then its words go behind whatever the
    // uv table holds so far; a material names its components by word offsets
    std::vector<uint32_t> measured_at(desc.num_measured, 0); // in 32-bit words from the start of uvs
    if (desc.num_measured) {
        if (!desc.measured) return fail(IGX_ERR_INVALID_ARGUMENT, "null measured bsdf table");
        for (uint32_t i = 0; i < desc.num_measured; ++i) {
            std::string err;
            if (!validate_measured(desc.measured[i], err)) return fail(IGX_ERR_INVALID_ARGUMENT, err);
        }
        for (uint32_t i = 0; i < desc.num_measured; ++i) {
            const igx_measured& md = desc.measured[i];
            if (uvs.size() + (md.num_words + 1) / 2 > 0x3fffffffu) return fail(IGX_ERR_UNSUPPORTED, "uv table and measured bsdfs exceed 8 GB");
            measured_at[i] = (uint32_t)(2 * uvs.size());
            uvs.resize(uvs.size() + ((size_t)md.num_words + 1) / 2, Float2{0, 0});
            if (md.num_words) std::memcpy(reinterpret_cast<uint8_t*>(uvs.data()) + 4 * (size_t)measured_at[i], md.words, 4 * (size_t)md.num_words);
            out.measured_bytes += 4 * (size_t)md.num_words;
        }
    }
    auto& mats = out.mats;
    mats.resize(desc.num_materials);
    for (uint32_t i = 0; i < desc.num_materials; ++i) {
        const igx_material& m = desc.materials[i];
        DevMaterial d{};
        switch (m.bsdf_type) {
        case IGX_BSDF_DIFFUSE: d.type = MAT_DIFFUSE; break;
        case IGX_BSDF_DIELECTRIC: d.type = MAT_DIELECTRIC; break;
        case IGX_BSDF_CONDUCTOR: d.type = MAT_CONDUCTOR; break;
        case IGX_BSDF_PLASTIC: d.type = MAT_PLASTIC; break;
        case IGX_BSDF_PRINCIPLED: d.type = MAT_PRINCIPLED; break;
        case IGX_BSDF_TENSORTREE: d.type = MAT_TENSORTREE; break;
        case IGX_BSDF_KLEMS: d.type = MAT_KLEMS; break;
        default: return fail(IGX_ERR_UNSUPPORTED, "unsupported bsdf type " + std::to_string(m.bsdf_type));
        }
        if (m.distribution < IGX_MICROFACET_DELTA || m.distribution > IGX_MICROFACET_BECKMANN)
            return fail(IGX_ERR_INVALID_ARGUMENT, "invalid microfacet distribution");
        d.light = m.light >= 0 && (uint32_t)m.light < desc.num_lights ? light_remap[m.light] : -1;
        // check_if_delta_distribution (core/microfacet.art:272): alpha <= 1e-4 is a delta lobe
        const bool rough = m.distribution != IGX_MICROFACET_DELTA && m.alpha_u > 1e-4f && m.alpha_v > 1e-4f;
        d.dist = rough ? m.distribution : MF_DELTA;
        bool mirror = true; // make_conductor_bsdf: eta ~ black and k ~ white (bsdf/conductor.art:111-121)
        for (int c = 0; c < 3; ++c) {
            d.kd[c] = m.kd[c];
            d.ks[c] = m.ks[c];
            d.kt[c] = m.kt[c];
            d.eta[c] = m.eta[c];
            d.kappa[c] = m.kappa[c];
            mirror = mirror && std::fabs(m.eta[c]) <= 1e-4f && std::fabs(m.kappa[c] - 1.0f) <= 1e-4f;
        }
        d.mirror = mirror ? 1 : 0;
        if (m.bsdf_type == IGX_BSDF_DIELECTRIC) d.mirror = m.thin ? 1 : 0; // dielectric: thin flag
        d.kd[3] = m.bsdf_type == IGX_BSDF_DIFFUSE ? m.diffuse_alpha : 0.0f;
        d.ks[3] = m.ext_ior;
        d.kt[3] = m.int_ior;
        d.eta[3] = m.alpha_u;
        d.kappa[3] = m.alpha_v;
        if (m.texture == IGX_TEXTURE_CHECKER && m.bsdf_type == IGX_BSDF_DIFFUSE) {
            const int32_t kind = IGX_TEXTURE_CHECKER;
            std::memcpy(&d.pad[0], &kind, 4);
            d.pad[1] = m.tex_scale;
            for (int c = 0; c < 3; ++c) d.pad[2 + c] = m.tex_kd1[c];
        } else if (m.texture == IGX_TEXTURE_IMAGE && (m.bsdf_type == IGX_BSDF_DIFFUSE || m.bsdf_type == IGX_BSDF_PRINCIPLED)) {
            if (m.tex_index < 0 || (uint32_t)m.tex_index >= desc.num_textures)
                return fail(IGX_ERR_INVALID_ARGUMENT, "material " + std::to_string(i) + ": texture index beyond the texture table");
            const int32_t kind = IGX_TEXTURE_IMAGE;
            std::memcpy(&d.pad[0], &kind, 4);
            for (int k = 0; k < 6; ++k) d.pad[1 + k] = desc.textures[m.tex_index].transform[k];
            std::memcpy(&d.pad[7], &tex_record_at[m.tex_index], 4);
        } else if (m.texture != IGX_TEXTURE_NONE) {
            return fail(IGX_ERR_UNSUPPORTED, "texture " + std::to_string(m.texture) + " on this bsdf type");
        }
        if (m.bsdf_type == IGX_BSDF_TENSORTREE || m.bsdf_type == IGX_BSDF_KLEMS) {
            // packing of a measured BSDF (device_scene.h, DevMaterial)
            if (m.measured < 0 || (uint32_t)m.measured >= desc.num_measured)
                return fail(IGX_ERR_INVALID_ARGUMENT, "material " + std::to_string(i) + ": index beyond the measured bsdf table");
            const igx_measured& md = desc.measured[m.measured];
            const bool tree = m.bsdf_type == IGX_BSDF_TENSORTREE;
            if (md.kind != (tree ? IGX_MEASURED_TENSORTREE : IGX_MEASURED_KLEMS))
                return fail(IGX_ERR_INVALID_ARGUMENT, "material " + std::to_string(i) + ": measured bsdf of the other kind");
            if (m.texture != IGX_TEXTURE_NONE) return fail(IGX_ERR_UNSUPPORTED, "texture on a measured bsdf");
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(m.up[c])) return fail(IGX_ERR_INVALID_ARGUMENT, "material " + std::to_string(i) + ": up is not finite");
            DevMaterial q{};
            q.type = d.type;
            q.light = d.light;
            q.dist = tree ? md.component[0].ndim : 0;
            const float fr = md.component[IGX_MEASURED_FRONT_REFLECTION].total, ft = md.component[IGX_MEASURED_FRONT_TRANSMISSION].total;
            const float br = md.component[IGX_MEASURED_BACK_REFLECTION].total, bt = md.component[IGX_MEASURED_BACK_TRANSMISSION].total;
            auto sdiv = [](float a, float b) { return std::fabs(b) <= 1.1920928955e-07f ? 0.0f : a / b; }; // safe_div
            for (int c = 0; c < 3; ++c) {
                q.kd[c] = m.kd[c];
                q.ks[c] = m.up[c];
            }
            q.kd[3] = sdiv(fr, fr + bt); // front_refl_prob (bsdf/tensortree.art:187-188)
            q.ks[3] = sdiv(br, br + ft); // back_refl_prob
            for (int k = 0; k < 4; ++k) {
                const igx_measured_component& mc = md.component[k];
                if (mc.total > 0) q.mirror |= 1 << k;
                if (tree && mc.root_is_leaf) q.mirror |= 16 << k;
                const uint32_t at = measured_at[m.measured] + mc.offset;
                const uint32_t a = tree ? mc.node_count : (mc.theta_count[0] | (mc.theta_count[1] << 16));
                const uint32_t b = tree ? (uint32_t)mc.max_depth : mc.entry_count[1];
                std::memcpy(&q.kt[k], &at, 4);
                std::memcpy(&q.eta[k], &a, 4);
                std::memcpy(&q.kappa[k], &b, 4);
            }
            d = q;
        }
        if (m.bsdf_type == IGX_BSDF_PRINCIPLED) {
            // packing of the principled closure (igx_kernels.h, principled_of)
            DevMaterial q{};
            q.type = MAT_PRINCIPLED;
            q.light = d.light;
            q.dist = MF_VNDF_GGX;
            q.mirror = (m.thin ? 1 : 0) | (m.clearcoat_top_only ? 2 : 0);
            for (int c = 0; c < 3; ++c) q.kd[c] = m.kd[c];
            q.kd[3] = m.ior;
            q.ks[0] = m.diffuse_transmission;
            q.ks[1] = m.specular_transmission;
            q.ks[2] = m.specular_tint;
            q.ks[3] = m.alpha_u;
            q.kt[0] = m.alpha_v;
            q.kt[1] = m.flatness;
            q.kt[2] = m.metallic;
            q.kt[3] = m.sheen;
            q.eta[0] = m.sheen_tint;
            q.eta[1] = m.clearcoat;
            q.eta[2] = m.clearcoat_gloss;
            q.eta[3] = m.clearcoat_roughness;
            std::memcpy(q.pad, d.pad, sizeof(q.pad)); // an image texture on base_color
            d = q;
        }
        mats[i] = d;
    }

    // hot nodes first: any prefix of the node array is a treelet (stage_treelet)
    order_hot_nodes(nodes, quantize ? 5 : width, inst, tlas_root, opt.treelet_front);

    out.tlas_root = tlas_root;
    out.width = width;
    out.quantized = quantize;
    out.nf4 = nf4;
    out.num_infinite = num_infinite;
    out.textured = textured;
    // bbox_radius(scene_bbox) * 1.01 (light/env.art:75; core/bbox.art:24)
    float dx = desc.scene_bbox_max[0] - desc.scene_bbox_min[0];
    float dy = desc.scene_bbox_max[1] - desc.scene_bbox_min[1];
    float dz = desc.scene_bbox_max[2] - desc.scene_bbox_min[2];
    out.scene_radius = std::sqrt(dx * dx + dy * dy + dz * dz) / 2 * 1.01f;
    if (desc.technique.max_depth > 255)
        return fail(IGX_ERR_UNSUPPORTED, "max_depth above 255 is not supported (8-bit path depth)");
    out.aov_on = desc.technique.aov_mis != 0;
    // stack: TLAS pushes + BLAS pushes (the depth for BVH2) + marker + resume entry + exit sentinel
#ifndef IGX_STACK_SLACK
#define IGX_STACK_SLACK 0
#endif
    out.tlas_depth = tlas_depth;
    out.blas_depth = blas_depth;
    out.scene_depth = tlas_depth + blas_depth + 3 + IGX_STACK_SLACK;
    if (out.scene_depth > MAX_STACK)
        return fail(IGX_ERR_UNSUPPORTED, "BVH too deep for the traversal stack (" + std::to_string(out.scene_depth) + " entries)");
    // shading feature set (variant bit 2): beyond Lambert + dielectric and the
    // plane/env/point/spot/directional/sun lights
    out.full_shading = opt.full_shading_opt;
    for (uint32_t i = 0; i < desc.num_materials; ++i) {
        const igx_material& m = desc.materials[i];
        if (m.bsdf_type == IGX_BSDF_CONDUCTOR || m.bsdf_type == IGX_BSDF_PLASTIC || m.bsdf_type == IGX_BSDF_PRINCIPLED ||
            m.bsdf_type == IGX_BSDF_TENSORTREE || m.bsdf_type == IGX_BSDF_KLEMS ||
            (m.bsdf_type == IGX_BSDF_DIFFUSE && m.diffuse_alpha > 1.1920929e-7f))
            out.full_shading = true;
    }
    for (uint32_t l = 0; l < desc.num_lights; ++l)
        if (desc.lights[l].type == IGX_LIGHT_SPHERE || desc.lights[l].type == IGX_LIGHT_MESH) out.full_shading = true;
    if (textured) out.full_shading = true; // textures are looked up by the full shading variant only
    if (out.aov_on) out.full_shading = true; // so are the MIS AOVs (add_aov)
    // and every camera but the pinhole perspective one (gen_pixel), and the CIE skies
    if (camera_needs_full(desc.camera)) out.full_shading = true;
    for (uint32_t l = 0; l < desc.num_lights; ++l)
        if (desc.lights[l].type == IGX_LIGHT_CIE || desc.lights[l].type == IGX_LIGHT_ENVMAP) out.full_shading = true;
    for (uint32_t e = 0; textured && e < desc.num_entities; ++e) {
        const igx_entity& en = desc.entities[e];
        if (desc.materials[en.material].texture != IGX_TEXTURE_NONE && desc.shapes[en.shape].type == IGX_SHAPE_SPHERE)
            return fail(IGX_ERR_UNSUPPORTED, "textured material on an analytic sphere (texture coordinates of spheres are not supported)");
    }
    return IGX_OK;
}

} // namespace igx
