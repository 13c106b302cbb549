// CPU check of the scene-table builder (host/scene_tables.cpp, compiled here
// with g++ together with bvh_build.cpp and light_select.cpp; also built with
// -fsanitize=address,undefined by tests/test_scene_tables.py).  Every scene is
// made in memory:
//   * a small scene (two meshes, two spheres, four entities, three materials,
//     three lights) at BVH2, 4-wide and quantised 4-wide nodes, each in hot
//     order with the default front and with a front of 3 nodes: node
//     references, BLAS leaves, Tri1 records, instance flags, entity records,
//     light order and remap, stack depth, auto width, the reorder as a
//     permutation;
//   * enclosing entities: a closed dielectric cube and the four ways to lose it;
//   * one scene per refusal, with the status and the message text;
//   * the full-shading decision, trigger by trigger.
#include "scene_tables.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace igx;
using namespace igxd;

static int g_bad = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_bad;                                                       \
        }                                                                  \
    } while (0)

// ---- scenes in memory ------------------------------------------------------
struct Mesh {
    std::vector<float> v, n, uv;
    std::vector<uint32_t> ix;
};
struct Scene {
    std::vector<Mesh> mesh_data;
    std::vector<igx_mesh> meshes;
    std::vector<igx_shape> shapes;
    std::vector<igx_entity> entities;
    std::vector<igx_material> materials;
    std::vector<igx_light> lights;
    igx_scene_desc d{};
    // call after every change
    const igx_scene_desc& desc() {
        meshes.resize(mesh_data.size());
        for (size_t i = 0; i < mesh_data.size(); ++i) {
            const Mesh& m = mesh_data[i];
            meshes[i] = igx_mesh{(uint32_t)(m.v.size() / 3), (uint32_t)(m.ix.size() / 3), m.v.data(), m.n.data(),
                                 m.uv.empty() ? nullptr : m.uv.data(), m.ix.data()};
        }
        d.num_meshes = (uint32_t)meshes.size();
        d.meshes = meshes.data();
        d.num_shapes = (uint32_t)shapes.size();
        d.shapes = shapes.data();
        d.num_entities = (uint32_t)entities.size();
        d.entities = entities.data();
        d.num_materials = (uint32_t)materials.size();
        d.materials = materials.data();
        d.num_lights = (uint32_t)lights.size();
        d.lights = lights.data();
        for (int a = 0; a < 3; ++a) {
            d.scene_bbox_min[a] = 3.4e38f;
            d.scene_bbox_max[a] = -3.4e38f;
            for (const auto& e : entities) {
                d.scene_bbox_min[a] = std::min(d.scene_bbox_min[a], e.bbox_min[a]);
                d.scene_bbox_max[a] = std::max(d.scene_bbox_max[a], e.bbox_max[a]);
            }
        }
        return d;
    }
};

// nx x ny quads on z = a gentle bump, two triangles each
static Mesh grid_mesh(int nx, int ny) {
    Mesh m;
    for (int j = 0; j <= ny; ++j)
        for (int i = 0; i <= nx; ++i) {
            const float x = (float)i / nx * 2 - 1, y = (float)j / ny * 2 - 1;
            m.v.insert(m.v.end(), {x, y, 0.1f * x * y});
            m.n.insert(m.n.end(), {0, 0, 1});
            m.uv.insert(m.uv.end(), {(float)i / nx, (float)j / ny});
        }
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const uint32_t a = j * (nx + 1) + i, b = a + 1, c = a + nx + 1, e = c + 1;
            m.ix.insert(m.ix.end(), {a, b, e, a, e, c});
        }
    return m;
}
static Mesh quad_mesh() { return grid_mesh(1, 1); }
// closed cube [-1, 1]^3: 8 vertices, 12 triangles
static Mesh cube_mesh() {
    Mesh m;
    for (int k = 0; k < 8; ++k) {
        m.v.insert(m.v.end(), {k & 1 ? 1.f : -1.f, k & 2 ? 1.f : -1.f, k & 4 ? 1.f : -1.f});
        m.n.insert(m.n.end(), {0, 0, 1});
    }
    m.ix = {0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
    return m;
}

static igx_shape mesh_shape(int mesh) {
    igx_shape s{};
    s.type = IGX_SHAPE_TRIMESH;
    s.mesh = mesh;
    return s;
}
static igx_shape sphere_shape(float x, float y, float z, float r) {
    igx_shape s{};
    s.type = IGX_SHAPE_SPHERE;
    s.mesh = -1;
    s.sphere[0] = x, s.sphere[1] = y, s.sphere[2] = z, s.sphere[3] = r;
    return s;
}
// an entity of `shape` under the rigid transform x -> R x + t (R row-major 3x3),
// its world box from the local box [lo, hi]
static igx_entity entity(int shape, int material, const float R[9], const float t[3], const float lo[3], const float hi[3]) {
    igx_entity e{};
    e.shape = shape;
    e.material = material;
    e.flags = 0xF;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            e.to_global[r * 4 + c] = R[r * 3 + c];
            e.to_local[r * 4 + c] = R[c * 3 + r]; // rotation: the inverse is the transpose
            e.normal[r * 3 + c] = R[r * 3 + c];
        }
        e.to_global[r * 4 + 3] = t[r];
    }
    for (int r = 0; r < 3; ++r) {
        float s = 0;
        for (int c = 0; c < 3; ++c) s += e.to_local[r * 4 + c] * t[c];
        e.to_local[r * 4 + 3] = s == 0 ? 0.0f : -s;
    }
    for (int a = 0; a < 3; ++a) {
        e.bbox_min[a] = 3.4e38f;
        e.bbox_max[a] = -3.4e38f;
    }
    for (int k = 0; k < 8; ++k) {
        const float p[3] = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
        for (int r = 0; r < 3; ++r) {
            const float w = R[r * 3] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + t[r];
            e.bbox_min[r] = std::min(e.bbox_min[r], w);
            e.bbox_max[r] = std::max(e.bbox_max[r], w);
        }
    }
    return e;
}
static const float kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
static const float kRotZ[9] = {0.6f, -0.8f, 0, 0.8f, 0.6f, 0, 0, 0, 1};
static const float kRotX[9] = {1, 0, 0, 0, 0.6f, -0.8f, 0, 0.8f, 0.6f};

static igx_material material(int bsdf) {
    igx_material m{};
    m.bsdf_type = bsdf;
    m.light = -1;
    for (int c = 0; c < 3; ++c) m.kd[c] = 0.5f, m.ks[c] = 1, m.kt[c] = 1, m.eta[c] = 0.2f, m.kappa[c] = 3;
    m.ext_ior = 1;
    m.int_ior = 1.5f;
    return m;
}
static igx_light light(int type) {
    igx_light l{};
    l.type = type;
    l.entity = -1;
    for (int c = 0; c < 3; ++c) l.radiance[c] = 1;
    l.select_flux = 1;
    return l;
}

enum { E_GRID = 0, E_GRID_MOVED = 1, E_SPHERE = 2, E_QUAD = 3 };
enum { M_DIFFUSE = 0, M_GLASS = 1, M_CHECKER = 2 };
enum { L_POINT = 0, L_PLANE = 1, L_ENV = 2 };
constexpr int GRID_FACES = 64;

// meshes: 0 quad, 1 grid; shapes: 0 quad, 1 sphere, 2 grid, 3 sphere
static Scene small_scene(int grid_nx = 8, int grid_ny = 4) {
    Scene s;
    s.mesh_data = {quad_mesh(), grid_mesh(grid_nx, grid_ny)};
    s.shapes = {mesh_shape(0), sphere_shape(5, 5, 5, 1), mesh_shape(1), sphere_shape(0, 0, 0, 0.5f)};
    const float lo[3] = {-1, -1, -0.1f}, hi[3] = {1, 1, 0.1f};
    const float slo[3] = {-0.5f, -0.5f, -0.5f}, shi[3] = {0.5f, 0.5f, 0.5f};
    const float t0[3] = {0, 0, 0}, t1[3] = {3, 0, 0}, t2[3] = {0, 3, 0}, t3[3] = {0, 0, 4};
    s.entities = {entity(2, M_DIFFUSE, kI, t0, lo, hi), entity(2, M_CHECKER, kI, t1, lo, hi),
                  entity(3, M_GLASS, kRotZ, t2, slo, shi), entity(0, M_DIFFUSE, kRotX, t3, lo, hi)};
    s.entities[E_GRID_MOVED].flags = 0x7;
    s.materials = {material(IGX_BSDF_DIFFUSE), material(IGX_BSDF_DIELECTRIC), material(IGX_BSDF_DIFFUSE)};
    s.materials[M_DIFFUSE].light = L_PLANE;
    s.materials[M_GLASS].light = 7; // no such light
    s.materials[M_CHECKER].light = L_POINT;
    s.materials[M_CHECKER].texture = IGX_TEXTURE_CHECKER;
    s.materials[M_CHECKER].tex_scale = 4;
    s.lights = {light(IGX_LIGHT_POINT), light(IGX_LIGHT_PLANE), light(IGX_LIGHT_ENV)};
    s.lights[L_POINT].origin[2] = 2;
    igx_light& pl = s.lights[L_PLANE];
    pl.entity = E_QUAD;
    pl.x_axis[0] = 2;
    pl.y_axis[1] = 3;
    pl.normal[2] = -1;
    pl.area = 6;
    s.d.film_width = s.d.film_height = 16;
    s.d.camera.dir[2] = -1;
    s.d.camera.up[1] = 1;
    s.d.camera.fov = 1;
    s.d.technique.max_depth = 8;
    s.d.technique.min_depth = 2;
    s.d.technique.nee = 1;
    return s;
}

// ---- reading the tables back -----------------------------------------------
static Int4 as_int4(const Float4& f) {
    Int4 i;
    std::memcpy(&i, &f, 16);
    return i;
}
static int32_t as_int(float f) {
    int32_t i;
    std::memcpy(&i, &f, 4);
    return i;
}
struct NodeView {
    const SceneTables& t;
    int width() const { return t.width; }
    size_t count() const { return t.nodes.size() / t.nf4; }
    const float* rec(size_t n) const { return reinterpret_cast<const float*>(&t.nodes[n * t.nf4]); }
    int32_t ref(size_t n, int k) const {
        return reinterpret_cast<const int32_t*>(rec(n))[t.width == 4 && !t.quantized ? 24 + k : 12 + k];
    }
    bool present(size_t n, int k) const { // an absent BVH2 child has an inverted or infinite box
        if (ref(n, k) == kEmptyRef) return false;
        return t.width == 4 || rec(n)[6 * k] <= rec(n)[6 * k + 1];
    }
};
// the instance slot of entity e, -1 if none
static int slot_of(const SceneTables& t, int e) {
    for (size_t s = 0; s < t.inst.size() / 4; ++s)
        if (as_int4(t.inst[4 * s + 3]).x == e) return (int)s;
    return -1;
}
// node records with their inner references masked, sorted
static std::vector<std::string> masked_nodes(const SceneTables& t) {
    const NodeView nv{t};
    std::vector<std::string> out;
    for (size_t n = 0; n < nv.count(); ++n) {
        std::string r(reinterpret_cast<const char*>(nv.rec(n)), (size_t)t.nf4 * 16);
        for (int k = 0; k < t.width; ++k)
            if (nv.ref(n, k) >= 0) std::memset(&r[4 * (t.width == 4 && !t.quantized ? 24 + k : 12 + k)], 0, 4);
        out.push_back(r);
    }
    std::sort(out.begin(), out.end());
    return out;
}

static igx_status build(Scene& s, const SceneBuildOptions& o, SceneTables& t, std::string* msg = nullptr) {
    std::string err;
    const igx_status st = build_scene_tables(s.desc(), o, t, err);
    if (msg) *msg = err;
    else if (st != IGX_OK) std::printf("build failed: %s\n", err.c_str());
    return st;
}

// ---- the small scene -------------------------------------------------------
static void check_small(int width_opt, int quantize_opt, size_t front, bool default_front) {
    Scene s = small_scene();
    SceneBuildOptions o;
    o.bvh_width_opt = width_opt;
    o.quantize_opt = quantize_opt;
    if (!default_front) o.treelet_front = front;
    SceneTables t;
    CHECK(build(s, o, t) == IGX_OK);
    if (t.nodes.empty()) return;
    std::printf("small: width %d quantized %d front %zu: %zu nodes, %zu tris, depth %d\n", t.width, (int)t.quantized,
                o.treelet_front, t.nodes.size() / t.nf4, t.tris.size() / 3, t.scene_depth);
    CHECK(t.width == width_opt && t.quantized == (quantize_opt == 1) && t.nf4 == (width_opt == 4 && quantize_opt != 1 ? 8 : 4));
    const NodeView nv{t};
    const int nn = (int)nv.count();
    const Mesh& grid = s.mesh_data[1];

    // every inner reference is below the node count
    for (int n = 0; n < nn; ++n)
        for (int k = 0; k < t.width; ++k) CHECK(nv.ref(n, k) < nn);
    CHECK(t.tlas_root >= 0 && t.tlas_root < nn);
    CHECK(t.inst.size() == 4 * s.entities.size());
    for (size_t sl = 0; sl < t.inst.size() / 4; ++sl) {
        const Int4 info = as_int4(t.inst[4 * sl + 3]);
        if (info.y == 0) CHECK(info.z < nn);
    }

    // the leaves under each BLAS root name every face of the mesh exactly once
    for (int e : {E_GRID, E_GRID_MOVED, E_QUAD}) {
        const int sl = slot_of(t, e);
        CHECK(sl >= 0);
        if (sl < 0) continue;
        const uint32_t faces = e == E_QUAD ? 2 : GRID_FACES;
        std::vector<int> seen(faces, 0);
        std::vector<int32_t> todo{as_int4(t.inst[4 * sl + 3]).z};
        size_t steps = 0;
        while (!todo.empty() && ++steps < 10000) {
            const int32_t r = todo.back();
            todo.pop_back();
            if (r >= 0) {
                if (r >= nn) continue;
                for (int k = 0; k < t.width; ++k)
                    if (nv.present(r, k)) todo.push_back(nv.ref(r, k));
                continue;
            }
            const int code = ~r, first = code >> kLeafCountBits, count = (code & ((1 << kLeafCountBits) - 1)) + 1;
            for (int q = first; q < first + count; ++q) {
                CHECK((size_t)q < t.tris.size() / 3);
                if ((size_t)q >= t.tris.size() / 3) continue;
                const int32_t f = as_int(t.tris[3 * q].w);
                CHECK(f >= 0 && (uint32_t)f < faces);
                if (f >= 0 && (uint32_t)f < faces) ++seen[f];
            }
        }
        CHECK(steps < 10000);
        CHECK(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }));
    }
    if (slot_of(t, E_GRID) >= 0 && slot_of(t, E_GRID_MOVED) >= 0) // two instances of one BLAS
        CHECK(as_int4(t.inst[4 * slot_of(t, E_GRID) + 3]).z == as_int4(t.inst[4 * slot_of(t, E_GRID_MOVED) + 3]).z);

    // Tri1: v0 and the face id, e1 = v0 - v1, e2 = v2 - v0 (the quad's two slots come first)
    CHECK(t.tris.size() == 3 * (2 + (size_t)GRID_FACES));
    for (size_t q = 2; q < t.tris.size() / 3; ++q) {
        const int32_t f = as_int(t.tris[3 * q].w);
        if (f < 0 || f >= GRID_FACES) continue;
        const float* v0 = &grid.v[3 * grid.ix[3 * f]];
        const float* v1 = &grid.v[3 * grid.ix[3 * f + 1]];
        const float* v2 = &grid.v[3 * grid.ix[3 * f + 2]];
        const Float4 &a = t.tris[3 * q], &b = t.tris[3 * q + 1], &c = t.tris[3 * q + 2];
        CHECK(a.x == v0[0] && a.y == v0[1] && a.z == v0[2]);
        CHECK(b.x == v0[0] - v1[0] && b.y == v0[1] - v1[1] && b.z == v0[2] - v1[2]);
        CHECK(c.x == v2[0] - v0[0] && c.y == v2[1] - v0[1] && c.z == v2[2] - v0[2]);
    }

    // instance records: to_local rows, flags, sphere index
    for (int e = 0; e < 4; ++e) {
        const int sl = slot_of(t, e);
        if (sl < 0) continue;
        const Int4 info = as_int4(t.inst[4 * sl + 3]);
        const uint32_t fl = (uint32_t)info.w;
        CHECK(((fl & INST_IDENTITY) != 0) == (e == E_GRID));
        CHECK(((fl & INST_TRANSLATE) != 0) == (e == E_GRID_MOVED));
        CHECK((fl & ~(INST_IDENTITY | INST_TRANSLATE)) == s.entities[e].flags);
        CHECK(info.y == (e == E_SPHERE ? 1 : 0));
        if (e == E_SPHERE) CHECK(info.z == 1); // the second sphere shape
        CHECK(std::memcmp(&t.inst[4 * sl], s.entities[e].to_local, 48) == 0);
    }
    CHECK(t.spheres.size() == 2 && t.spheres[1].w == 0.5f && t.spheres[0].x == 5);

    // entity records: to_global, normal matrix, info; the face-normal offset in row 3 .w
    CHECK(t.ent.size() == (size_t)ENT_STRIDE * 4);
    const int want_info[4][4] = {{0, M_DIFFUSE, 4, 2}, {0, M_CHECKER, 4, 2}, {1, M_GLASS, 0, 1}, {0, M_DIFFUSE, 0, 0}};
    const int want_fn[4] = {0, GRID_FACES, -1, 2 * GRID_FACES};
    for (int e = 0; e < 4 && t.ent.size() == (size_t)ENT_STRIDE * 4; ++e) {
        const Float4* r = &t.ent[ENT_STRIDE * e];
        const Int4 info = as_int4(r[6]);
        CHECK(info.x == want_info[e][0] && info.y == want_info[e][1] && info.z == want_info[e][2] && info.w == want_info[e][3]);
        CHECK(std::memcmp(r, s.entities[e].to_global, 48) == 0);
        for (int k = 0; k < 3; ++k) CHECK(std::memcmp(&r[3 + k], &s.entities[e].normal[3 * k], 12) == 0);
        CHECK(as_int(r[3].w) == want_fn[e]);
    }
    CHECK(t.ent_fn == std::vector<int32_t>({want_fn[0], want_fn[1], want_fn[2], want_fn[3]}));
    CHECK(t.fn_tab.size() == 2 * (size_t)GRID_FACES + 2);
    for (const Float4& n : t.fn_tab) CHECK(std::fabs(n.x * n.x + n.y * n.y + n.z * n.z - 1) < 1e-5f);
    CHECK(t.vtx.size() == 4 + 45 && t.nrm.size() == t.vtx.size() && t.uvs.size() == t.vtx.size() && t.idx.size() == 2 + (size_t)GRID_FACES);
    CHECK(t.fsh.size() == 3 * t.idx.size() && as_int(t.fsh[3 * 2 + 1].w) == (int)grid.ix[1]);
    CHECK(t.ent_enc == std::vector<int32_t>(4, -1) && t.enc_tab.empty()); // the glass is a sphere

    // lights: infinite first, then desc order; the materials' lights follow
    CHECK(t.lights.size() == 3 && t.num_infinite == 1);
    if (t.lights.size() == 3) {
        CHECK(t.lights[0].type == IGX_LIGHT_ENV && t.lights[1].type == IGX_LIGHT_POINT && t.lights[2].type == IGX_LIGHT_PLANE);
        CHECK(t.lights[0].infinite == 1 && t.lights[1].infinite == 0 && t.lights[2].infinite == 0);
        CHECK(t.lights[1].delta == 1 && t.lights[0].delta == 0 && t.lights[2].delta == 0);
        CHECK(t.lights[1].origin[2] == 2);
        CHECK(t.lights[2].origin[3] == 2 && t.lights[2].ex[3] == 3 && t.lights[2].ex[0] == 1 && t.lights[2].ey[1] == 1 &&
              t.lights[2].normal[3] == 6 && t.lights[2].ey[3] == 1 / 6.0f);
    }
    CHECK(t.mats.size() == 3);
    if (t.mats.size() == 3) {
        CHECK(t.mats[M_DIFFUSE].light == 2 && t.mats[M_GLASS].light == -1 && t.mats[M_CHECKER].light == 1);
        CHECK(t.mats[M_DIFFUSE].type == MAT_DIFFUSE && t.mats[M_GLASS].type == MAT_DIELECTRIC);
        CHECK(as_int(t.mats[M_CHECKER].pad[0]) == IGX_TEXTURE_CHECKER && t.mats[M_CHECKER].pad[1] == 4);
    }
    CHECK(t.lsel.selector == IGX_SELECT_UNIFORM);

    CHECK(t.scene_depth == t.tlas_depth + t.blas_depth + 3);
    CHECK(t.tlas_depth >= 1 && t.blas_depth >= 1);
    CHECK(t.textured && t.full_shading && !t.aov_on);
    const float ext[3] = {s.d.scene_bbox_max[0] - s.d.scene_bbox_min[0], s.d.scene_bbox_max[1] - s.d.scene_bbox_min[1],
                          s.d.scene_bbox_max[2] - s.d.scene_bbox_min[2]};
    CHECK(std::fabs(t.scene_radius - 0.505f * std::sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2])) < 1e-4f);

    // the hot order is a permutation of the nodes in build order (front 0)
    SceneBuildOptions o0 = o;
    o0.treelet_front = 0;
    SceneTables t0;
    CHECK(build(s, o0, t0) == IGX_OK);
    CHECK(t0.nodes.size() == t.nodes.size() && masked_nodes(t0) == masked_nodes(t));
    // the TLAS is appended last, and its root is among the hottest nodes: it moves to the front
    CHECK(t0.tlas_root >= 3 && t.tlas_root < 3);
    CHECK(std::memcmp(t0.nodes.data(), t.nodes.data(), t.nodes.size() * sizeof(Float4)) != 0);
    CHECK(t0.tris.size() == t.tris.size() && std::memcmp(t0.tris.data(), t.tris.data(), t.tris.size() * sizeof(Float4)) == 0);
}

// auto width: BVH2 while tlas.depth + blas_depth2 + 3 fits the LDS stack
static void check_auto_width() {
    for (int big = 0; big < 2; ++big) {
        Scene s = big ? small_scene(128, 128) : small_scene();
        SceneBuildOptions o;
        o.leaf_size = big ? 1 : 4;
        SceneTables t2, ta;
        o.bvh_width_opt = 2; // its depths are the BVH2 depths
        CHECK(build(s, o, t2) == IGX_OK);
        o.bvh_width_opt = 0;
        CHECK(build(s, o, ta) == IGX_OK);
        const int want = t2.tlas_depth + t2.blas_depth + 3 <= LDS_STACK ? 2 : 4;
        std::printf("auto width: BVH2 depths %d + %d: width %d\n", t2.tlas_depth, t2.blas_depth, ta.width);
        CHECK(ta.width == want && want == (big ? 4 : 2));
        CHECK(!ta.quantized); // far below SPLIT_TABLE_BYTES
        CHECK(ta.scene_depth == ta.tlas_depth + ta.blas_depth + 3);
    }
}

// ---- enclosing entities ----------------------------------------------------
enum { ENC_OK, ENC_OPEN, ENC_THIN, ENC_NEAR, ENC_OFF };
static void check_enclosing(int variant) {
    Scene s;
    s.mesh_data = {quad_mesh(), cube_mesh()};
    if (variant == ENC_OPEN) s.mesh_data[1].ix.resize(3 * 11);
    s.shapes = {mesh_shape(0), mesh_shape(1)};
    const float qlo[3] = {-1, -1, -0.1f}, qhi[3] = {1, 1, 0.1f}, clo[3] = {-1, -1, -1}, chi[3] = {1, 1, 1};
    const float tq[3] = {0, 0, -5}, tc[3] = {0, 0, 0};
    s.entities = {entity(0, 0, kI, tq, qlo, qhi), entity(1, 1, kI, tc, clo, chi)};
    s.materials = {material(IGX_BSDF_DIFFUSE), material(IGX_BSDF_DIELECTRIC)};
    if (variant == ENC_THIN) s.materials[1].thin = 1;
    s.lights = {light(IGX_LIGHT_ENV)};
    s.d.technique.max_depth = 8;
    if (variant == ENC_NEAR) {
        // the margin is 1e-4 of the scene's longest side (z: -5.1 to 1): the other box ends half a margin below the cube
        s.entities[0].bbox_max[2] = -1 - 0.5f * 1e-4f * 6.1f;
    }
    SceneBuildOptions o;
    o.enclosing_opt = variant != ENC_OFF;
    SceneTables t;
    CHECK(build(s, o, t) == IGX_OK);
    CHECK(t.ent_enc.size() == 2);
    if (t.ent_enc.size() != 2) return;
    if (variant != ENC_OK) {
        CHECK(t.ent_enc[0] == -1 && t.ent_enc[1] == -1 && t.enc_tab.empty() && t.enc_box.empty());
        return;
    }
    CHECK(t.ent_enc[0] == -1 && t.ent_enc[1] == 0);
    CHECK(t.enc_tab.size() == 1 && t.enc_box.size() == 2);
    if (t.enc_tab.size() != 1 || t.enc_box.size() != 2) return;
    CHECK(t.enc_tab[0].x == 1 && t.enc_tab[0].y == slot_of(t, 1));
    const igx_entity& c = s.entities[1];
    CHECK(t.enc_box[0].x == c.bbox_min[0] && t.enc_box[0].y == c.bbox_min[1] && t.enc_box[0].z == c.bbox_min[2]);
    CHECK(t.enc_box[1].x == c.bbox_max[0] && t.enc_box[1].y == c.bbox_max[1] && t.enc_box[1].z == c.bbox_max[2]);
    CHECK(closed_mesh(s.desc().meshes[1]) && !closed_mesh(s.desc().meshes[0]));
}

// ---- refusals --------------------------------------------------------------
template <typename F>
static void check_error(const char* what, igx_status want, const std::string& text, F&& change) {
    Scene s = small_scene();
    change(s);
    SceneTables t;
    std::string msg;
    const igx_status st = build(s, SceneBuildOptions{}, t, &msg);
    if (st != want || msg != text) {
        std::printf("FAIL %s: status %d '%s', want %d '%s'\n", what, (int)st, msg.c_str(), (int)want, text.c_str());
        ++g_bad;
    }
}
static void check_errors() {
    const igx_status INV = IGX_ERR_INVALID_ARGUMENT, UNS = IGX_ERR_UNSUPPORTED;
    check_error("mesh reference", INV, "shape references an invalid mesh", [](Scene& s) { s.shapes[2].mesh = 5; });
    check_error("negative mesh reference", INV, "shape references an invalid mesh", [](Scene& s) { s.shapes[0].mesh = -1; });
    check_error("vertex index", INV, "mesh index out of range", [](Scene& s) { s.mesh_data[1].ix[5] = 1000000; });
    check_error("vertex index = count", INV, "mesh index out of range", [](Scene& s) { s.mesh_data[0].ix[0] = 4; });
    check_error("entity shape", INV, "entity references an invalid shape", [](Scene& s) { s.entities[E_GRID].shape = 99; });
    check_error("entity shape < 0", INV, "entity references an invalid shape", [](Scene& s) { s.entities[E_QUAD].shape = -3; });
    check_error("entity material", INV, "entity references an invalid material", [](Scene& s) { s.entities[E_GRID].material = 3; });
    check_error("entity material < 0", INV, "entity references an invalid material", [](Scene& s) { s.entities[E_SPHERE].material = -1; });
    check_error("area light entity", INV, "area light references an invalid entity", [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_MESH));
        s.lights.back().entity = 100;
    });
    check_error("area light entity < 0", INV, "area light references an invalid entity", [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_SPHERE));
    });
    check_error("sphere light radius", INV, "sphere light needs a positive radius and area", [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_SPHERE));
        s.lights.back().entity = E_SPHERE;
        s.lights.back().area = 1;
        s.lights.back().radius = 0;
    });
    check_error("mesh light on a sphere", INV, "mesh light needs a non-empty triangle entity", [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_MESH));
        s.lights.back().entity = E_SPHERE;
    });
    check_error("CIE sky kind", INV, "invalid CIE sky kind", [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_CIE));
        s.lights.back().sky_kind = 9;
    });
    check_error("light type", UNS, "unsupported light type", [](Scene& s) { s.lights.push_back(light(42)); });
    check_error("bsdf", UNS, "unsupported bsdf type 17", [](Scene& s) { s.materials[M_DIFFUSE].bsdf_type = 17; });
    check_error("microfacet distribution", INV, "invalid microfacet distribution", [](Scene& s) { s.materials[M_GLASS].distribution = 9; });
    check_error("texture on a dielectric", UNS, "texture 1 on this bsdf type", [](Scene& s) { s.materials[M_GLASS].texture = IGX_TEXTURE_CHECKER; });
    check_error("max_depth", UNS, "max_depth above 255 is not supported (8-bit path depth)", [](Scene& s) { s.d.technique.max_depth = 256; });
    check_error("textured sphere", UNS, "textured material on an analytic sphere (texture coordinates of spheres are not supported)",
                [](Scene& s) { s.entities[E_SPHERE].material = M_CHECKER; });
}

// ---- the shading variant ---------------------------------------------------
template <typename F>
static void check_full(const char* what, bool want, F&& change, bool option = false) {
    Scene s = small_scene();
    s.materials[M_CHECKER].texture = IGX_TEXTURE_NONE; // the basic scene
    change(s);
    SceneBuildOptions o;
    o.full_shading_opt = option;
    SceneTables t;
    const igx_status st = build(s, o, t);
    if (st != IGX_OK || t.full_shading != want) {
        std::printf("FAIL full shading, %s: status %d, full %d, want %d\n", what, (int)st, (int)t.full_shading, (int)want);
        ++g_bad;
    }
}
static void check_full_shading() {
    check_full("basic scene", false, [](Scene&) {});
    check_full("conductor", true, [](Scene& s) { s.materials.push_back(material(IGX_BSDF_CONDUCTOR)); });
    check_full("plastic", true, [](Scene& s) { s.materials.push_back(material(IGX_BSDF_PLASTIC)); });
    check_full("principled", true, [](Scene& s) { s.materials.push_back(material(IGX_BSDF_PRINCIPLED)); });
    check_full("Oren-Nayar", true, [](Scene& s) { s.materials[M_DIFFUSE].diffuse_alpha = 0.5f; });
    check_full("Oren-Nayar alpha on a dielectric", false, [](Scene& s) { s.materials[M_GLASS].diffuse_alpha = 0.5f; });
    check_full("sphere light", true, [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_SPHERE));
        s.lights.back().entity = E_SPHERE;
        s.lights.back().area = 3;
        s.lights.back().radius = 0.5f;
    });
    check_full("mesh light", true, [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_MESH));
        s.lights.back().entity = E_GRID;
    });
    check_full("CIE sky", true, [](Scene& s) {
        s.lights.push_back(light(IGX_LIGHT_CIE));
        s.lights.back().sky_kind = IGX_SKY_CLEAR;
    });
    check_full("texture", true, [](Scene& s) { s.materials[M_CHECKER].texture = IGX_TEXTURE_CHECKER; });
    check_full("aov_mis", true, [](Scene& s) { s.d.technique.aov_mis = 1; });
    check_full("orthogonal camera", true, [](Scene& s) { s.d.camera.type = IGX_CAMERA_ORTHOGONAL; });
    check_full("fishlens camera", true, [](Scene& s) { s.d.camera.type = IGX_CAMERA_FISHLENS; });
    check_full("depth of field", true, [](Scene& s) { s.d.camera.aperture_radius = 0.1f; });
    check_full("option", true, [](Scene&) {}, true);
}

int main() {
    for (int cfg = 0; cfg < 3; ++cfg) {
        check_small(cfg == 0 ? 2 : 4, cfg == 2 ? 1 : 0, TREELET_FRONT, true);
        check_small(cfg == 0 ? 2 : 4, cfg == 2 ? 1 : 0, 3, false);
    }
    check_auto_width();
    for (int v : {ENC_OK, ENC_OPEN, ENC_THIN, ENC_NEAR, ENC_OFF}) check_enclosing(v);
    check_errors();
    check_full_shading();
    std::printf(g_bad ? "failed\n" : "ok\n");
    return g_bad ? 1 : 0;
}
