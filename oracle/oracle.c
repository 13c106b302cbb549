/*
 * oracle.c — CPU restatement of the reference path (TEST INFRASTRUCTURE).
 * See oracle.h for scope and citations.  Plain C11 + pthreads; no code from
 * the product library (ignis-masterthesis_amd/) is used here.
 */
#include "oracle.h"

#include <math.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#define FLT_EPS_ 1.1920928955e-07f   /* core/common.art:3 */
#define FLT_MAX_ 3.4028234664e+38f   /* core/common.art:4 */
#define PI_ 3.14159265359f           /* core/common.art:7 */
#define INV_PI_ 0.31830988618379067154f

#define RAY_CAMERA 0x1u
#define RAY_BOUNCE 0x4u
#define RAY_SHADOW 0x8u
#define RAY_TYPE_MASK 0xFu

/* ------------------------------------------------------------------------ */
typedef struct { float x, y, z; } v3;
static inline v3 V(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static inline v3 vadd(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 vsub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 vneg(v3 a) { return V(-a.x, -a.y, -a.z); }
static inline v3 vmulf(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static inline v3 vmul(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline float vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline v3 vcross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static inline float vlen(v3 a) { return sqrtf(vdot(a, a)); }
static inline v3 vnormalize(v3 a) { return vmulf(a, 1.0f / vlen(a)); }

/* core/common.art:95-98, 167-171 */
static inline float safe_rcp(float x) {
    float ax = x > 0 ? x : -x;
    if (ax < 1e-8f) return copysignf(FLT_MAX_, x);
    return 1.0f / x;
}
static inline float safe_div(float a, float b) { return fabsf(b) <= FLT_EPS_ ? 0.0f : a / b; }
static inline float safe_sqrt(float a) { return sqrtf(fmaxf(0.0f, a)); }
static inline float clampf_(float v, float l, float u) { return fminf(u, fmaxf(l, v)); }
static inline float sum_of_prod(float a, float b, float c, float d) {
    float cd = c * d;
    float s = fmaf(a, b, cd);
    float err = fmaf(c, d, -cd);
    return s + err;
}
static inline float lerp2(float a, float b, float c, float k1, float k2) { return (1 - k1 - k2) * a + k1 * b + k2 * c; }

/* make_orthonormal_mat3x3 (core/matrix.art:20-28) */
typedef struct { v3 t, b, n; } frame_t;
static frame_t make_frame(v3 n) {
    float sign = copysignf(1.0f, n.z);
    float a = -1.0f / (sign + n.z);
    float b = n.x * n.y * a;
    frame_t f;
    f.t = V(1 + sign * n.x * n.x * a, sign * b, -sign * n.x);
    f.b = V(b, sign + n.y * n.y * a, -n.y);
    f.n = n;
    return f;
}
static inline v3 frame_to_world(const frame_t* f, v3 v) {
    return V(f->t.x * v.x + f->b.x * v.y + f->n.x * v.z, f->t.y * v.x + f->b.y * v.y + f->n.y * v.z,
             f->t.z * v.x + f->b.z * v.y + f->n.z * v.z);
}

/* ---- RNG (core/random.art) --------------------------------------------- */
static inline uint32_t hash_combine(uint32_t h, uint32_t d) {
    h = (h * 16777619u) ^ (d & 0xFFu);
    h = (h * 16777619u) ^ ((d >> 8) & 0xFFu);
    h = (h * 16777619u) ^ ((d >> 16) & 0xFFu);
    h = (h * 16777619u) ^ ((d >> 24) & 0xFFu);
    return h;
}
uint32_t oracle_random_seed(int32_t sample, int32_t iter, int32_t frame, int32_t x, int32_t y, int32_t user) {
    uint32_t h = 0x811C9DC5u;
    h = hash_combine(h, (uint32_t)sample);
    h = hash_combine(h, (uint32_t)iter);
    h = hash_combine(h, (uint32_t)frame);
    h = hash_combine(h, (uint32_t)x);
    h = hash_combine(h, (uint32_t)y);
    h = hash_combine(h, (uint32_t)user);
    return h;
}
static inline uint32_t tea(uint32_t v0, uint32_t v1) {
    uint32_t sum = 0;
    for (int i = 0; i < 4; ++i) {
        sum += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v1;
}
typedef struct { uint32_t seed, counter; } rng_t;
static inline uint32_t rng_u32(rng_t* r) { return tea(r->seed, r->counter++); }
static inline float rng_f32(rng_t* r) {
    uint32_t x = rng_u32(r);
    uint32_t b = (x & 0x7FFFFFu) | 0x3F800000u;
    float f;
    memcpy(&f, &b, 4);
    return f - 1.0f;
}
static inline int rng_i32(rng_t* r, int s, int e) {
    uint32_t range = (uint32_t)(e - s);
    if (range == 0xFFFFFFFFu) return (int)rng_u32(r) + s;
    uint32_t erange = range + 1;
    uint32_t scaling = 0xFFFFFFFFu / erange;
    uint32_t past = erange * scaling;
    uint32_t ret = rng_u32(r);
    while (ret >= past) ret = rng_u32(r);
    return (int)(ret / scaling) + s;
}
float oracle_next_f32(uint32_t seed, uint32_t* counter) {
    rng_t r = {seed, *counter};
    float f = rng_f32(&r);
    *counter = r.counter;
    return f;
}

/* ------------------------------------------------------------------------ */
/* Scene                                                                     */
/* ------------------------------------------------------------------------ */
typedef struct {
    float lo[3], hi[3];
    int32_t ref; /* >= 0 inner node, < 0 leaf: ~(first << 4 | (count-1)) */
} ochild;
typedef struct { ochild c[2]; } onode;

/* 4-wide node of the CPU traversal (the reference CPU device's Node4,
 * traversal/mapping_cpu.art:3-13: four child boxes SoA, child refs) */
typedef struct {
    float lo[3][4], hi[3][4];
    int32_t ref[4]; /* >= 0 inner node, < 0 leaf: ~(first << 4 | (count-1)) */
    int32_t n;      /* valid children */
} onode4;

typedef struct {
    onode4* nodes;
    int num_nodes;
    int32_t* order; /* leaf slot -> primitive */
} obvh;

typedef struct {
    int type; /* 0 mesh, 1 sphere */
    int mesh;
    float sphere[4];
    obvh bvh;
    /* Tri with e1 = v0 - v1, e2 = v2 - v0, n = cross(e1, e2) per slot (shapes/trimesh.art:116-122) */
    float* tri; /* 12 floats per slot */
} oshape;

typedef struct {
    int type, infinite, delta;
    float rad[3];
    float origin[3], ex[3], ey[3], normal[3];
    float width, height, area;
    float cos_cut, blend;
    float sun_cos, sun_area; /* make_sun_light (light/sun.art:4-8) */
    int entity;              /* sphere / mesh area lights: emitting entity */
    float sph[4];            /* sphere emitter: object-space centre, radius */
    float sph_area;          /* compute_ellipsoid_area (shapes/sphere.art:21-27) */
    int faces;               /* shape emitter: primitive_count */
    float sel_pos[3], sel_dir[3], sel_flux; /* Light::position / direction / computeFlux */
    int sel_has_dir;
    int desc_light;          /* image environment map: its igx_light (texture, scale, transform) */
} olight;

struct oracle_scene {
    igx_scene_desc desc;        /* borrowed pointers for meshes/entities/materials */
    oshape* shapes;
    obvh tlas;
    olight* lights;
    int num_lights, num_infinite;
    int* mat_light;             /* remapped light index per material */
    float scene_radius;
    int selector;               /* light selector in effect (IGX_SELECT_*) */
    float* sel_cdf;             /* simple: CDF over the finite lights */
    int* lh_codes;              /* hierarchy: per finite light, bit d = right at depth d */
    float* lh_nodes;            /* hierarchy: 8 floats per node (pos, signed flux, dir, index bits) */
};

/* ---- NEE light selection (light/light_selector.art) ----------------------
 * Finite light f is s->lights[num_infinite + f].  "simple": flux CDF
 * (CDF::computeForArray, CDF.cpp:11-40; make_cdf_1d, core/cdf.art:40-45);
 * "hierarchy": PointBvh (container/PointBvh.inl) turned into a light tree by
 * LightHierarchy::setup (LightHierarchy.cpp:46-118), walked as in
 * light/light_hierarchy.art.  One light or none, or no finite light: uniform
 * (LoaderLight.cpp:423-453). */
typedef struct { float lo[3], hi[3]; int axis; int index; } opnode; /* axis < 0: leaf of light `index` */

static void pbox_extend(opnode* n, const float* p) {
    for (int i = 0; i < 3; ++i) {
        if (p[i] < n->lo[i]) n->lo[i] = p[i];
        if (p[i] > n->hi[i]) n->hi[i] = p[i];
    }
}

/* PointBvh::store: descend by the (grown) node's mid plane, split the leaf reached */
static int pbvh_store(opnode* nodes, int count, int light, const float* p) {
    if (count == 0) {
        opnode n;
        for (int i = 0; i < 3; ++i) n.lo[i] = n.hi[i] = p[i];
        n.axis = -1;
        n.index = 0;
        nodes[0] = n;
        return 1;
    }
    int at = 0;
    for (;;) {
        pbox_extend(&nodes[at], p);
        if (nodes[at].axis < 0) break;
        int ax = nodes[at].axis;
        float mid = (nodes[at].hi[ax] + nodes[at].lo[ax]) / 2;
        at = p[ax] < mid ? nodes[at].index : nodes[at].index + 1;
    }
    opnode box = nodes[at];
    float d0 = box.hi[0] - box.lo[0], d1 = box.hi[1] - box.lo[1], d2 = box.hi[2] - box.lo[2];
    int ax = 0;
    float dm = d0;
    if (d1 > dm) { ax = 1; dm = d1; }
    if (d2 > dm) { ax = 2; dm = d2; }
    float mid = dm / 2; /* PointBvh.inl: half the extent, compared with the coordinate */
    int old_leaf = box.index;
    nodes[at].index = count;
    nodes[at].axis = ax;
    opnode l = box, r = box;
    float off = (box.hi[ax] - box.lo[ax]) * 0.5f;
    l.hi[ax] -= off;
    r.lo[ax] += off;
    l.axis = r.axis = -1;
    int new_left = p[ax] < mid;
    l.index = new_left ? light : old_leaf;
    r.index = new_left ? old_leaf : light;
    nodes[count] = l;
    nodes[count + 1] = r;
    return count + 2;
}

/* populateInnerNodes: fills node entry `id` (8 floats), returns it in out[8] */
static void lh_populate(const oracle_scene* s, const opnode* nodes, int id, uint32_t code, uint32_t depth, float* ent,
                        int* codes, float* out) {
    const opnode* n = &nodes[id];
    float* e = ent + 8 * id;
    if (n->axis < 0) {
        const olight* L = &s->lights[s->num_infinite + n->index];
        e[0] = L->sel_pos[0]; e[1] = L->sel_pos[1]; e[2] = L->sel_pos[2];
        e[3] = L->sel_has_dir ? L->sel_flux : -L->sel_flux;
        if (L->sel_has_dir) { e[4] = L->sel_dir[0]; e[5] = L->sel_dir[1]; e[6] = L->sel_dir[2]; }
        else { e[4] = 0; e[5] = 0; e[6] = 1; }
        int32_t lid = n->index;
        memcpy(&e[7], &lid, 4);
        codes[n->index] = (int)code;
        memcpy(out, e, 32);
        return;
    }
    float l[8], r[8];
    lh_populate(s, nodes, n->index, code, depth + 1, ent, codes, l);
    lh_populate(s, nodes, n->index + 1, code | (1u << depth), depth + 1, ent, codes, r);
    e[0] = (n->hi[0] + n->lo[0]) / 2; e[1] = (n->hi[1] + n->lo[1]) / 2; e[2] = (n->hi[2] + n->lo[2]) / 2;
    int32_t idx = -(n->index + 1);
    memcpy(&e[7], &idx, 4);
    if (l[3] < 0 && r[3] < 0) { e[4] = 0; e[5] = 0; e[6] = 1; e[3] = l[3] + r[3]; }
    else if (l[3] < 0) { e[4] = 0; e[5] = 0; e[6] = 1; e[3] = -(-l[3] + r[3]); }
    else if (r[3] < 0) { e[4] = 0; e[5] = 0; e[6] = 1; e[3] = -(l[3] - r[3]); }
    else {
        float d[3] = {l[4] + r[4], l[5] + r[5], l[6] + r[6]};
        float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        e[4] = d[0] / len; e[5] = d[1] / len; e[6] = d[2] / len;
        e[3] = l[3] + r[3];
    }
    memcpy(out, e, 32);
}

static void build_selector(oracle_scene* s, int selector) {
    int nf = s->num_lights - s->num_infinite;
    s->selector = IGX_SELECT_UNIFORM;
    if (s->num_lights <= 1 || nf == 0) return;
    if (selector == IGX_SELECT_SIMPLE) {
        float* c = (float*)malloc(sizeof(float) * nf);
        c[0] = s->lights[s->num_infinite].sel_flux;
        for (int x = 1; x < nf; ++x) c[x] = c[x - 1] + s->lights[s->num_infinite + x].sel_flux;
        float sum = c[nf - 1];
        if (sum > 1e-5f) {
            float inv = 1.0f / sum;
            for (int x = 0; x < nf; ++x) c[x] *= inv;
        } else {
            float inv = 1.0f / (float)nf;
            for (int x = 0; x < nf; ++x) c[x] = (float)x * inv;
        }
        c[nf - 1] = 1;
        s->sel_cdf = c;
        s->selector = IGX_SELECT_SIMPLE;
    } else if (selector == IGX_SELECT_HIERARCHY) {
        opnode* nodes = (opnode*)malloc(sizeof(opnode) * (2 * nf));
        int count = 0;
        for (int f = 0; f < nf; ++f) count = pbvh_store(nodes, count, f, s->lights[s->num_infinite + f].sel_pos);
        s->lh_nodes = (float*)calloc((size_t)count * 8, sizeof(float));
        s->lh_codes = (int*)calloc((size_t)nf, sizeof(int));
        float root[8];
        lh_populate(s, nodes, 0, 0, 0, s->lh_nodes, s->lh_codes, root);
        free(nodes);
        s->selector = IGX_SELECT_HIERARCHY;
    }
}

static float cdf_at(const float* c, int i) { return i == 0 ? 0.0f : c[i - 1]; }

typedef struct { v3 pos, dir; float flux; int id, has_dir, is_leaf; } olh_entry;
static olh_entry lh_entry(const oracle_scene* s, int id) {
    const float* e = s->lh_nodes + 8 * id;
    int32_t index;
    memcpy(&index, &e[7], 4);
    olh_entry r = {V(e[0], e[1], e[2]), V(e[4], e[5], e[6]), fabsf(e[3]), index < 0 ? -index - 1 : index, !signbit(e[3]),
                   index >= 0};
    return r;
}
static float lh_cost(const olh_entry* e, v3 pos) {
    v3 cdir = vsub(e->pos, pos);
    float dist2 = vdot(cdir, cdir);
    float cos_d = e->has_dir ? fabsf(vdot(e->dir, vnormalize(cdir))) : 1.0f;
    return safe_div(e->flux * cos_d, dist2);
}
static float lh_prop(const olh_entry* l, const olh_entry* r, v3 pos) {
    float cl = lh_cost(l, pos), cr = lh_cost(r, pos);
    return 1 / (1 + cr / cl);
}

static int finite_select(const oracle_scene* s, rng_t* rnd, v3 from, float* pdf) {
    int nf = s->num_lights - s->num_infinite;
    if (s->selector == IGX_SELECT_SIMPLE) {
        float u = rng_f32(rnd);
        int first = 0, len = nf + 1; /* interval::binary_search */
        while (len > 0) {
            int half = len / 2, middle = first + half;
            if (cdf_at(s->sel_cdf, middle) <= u) { first = middle + 1; len -= half + 1; }
            else len = half;
        }
        int off = first - 1 < 0 ? 0 : (first - 1 > nf ? nf : first - 1);
        if (off > nf - 1) off = nf - 1;
        *pdf = cdf_at(s->sel_cdf, off + 1) - cdf_at(s->sel_cdf, off);
        return off;
    }
    if (nf == 1) { *pdf = 1.0f; return 0; }
    float p = 1.0f;
    olh_entry e = lh_entry(s, 0);
    while (!e.is_leaf) {
        olh_entry l = lh_entry(s, e.id), r = lh_entry(s, e.id + 1);
        float prop = lh_prop(&l, &r, from);
        int left = rng_f32(rnd) < prop;
        e = left ? l : r;
        p *= left ? prop : 1 - prop;
    }
    *pdf = p;
    return e.id;
}
static float finite_pdf(const oracle_scene* s, int f, v3 from) {
    int nf = s->num_lights - s->num_infinite;
    if (s->selector == IGX_SELECT_SIMPLE) return cdf_at(s->sel_cdf, f + 1) - cdf_at(s->sel_cdf, f);
    if (nf == 1) return 1.0f;
    uint32_t code = (uint32_t)s->lh_codes[f];
    float p = 1.0f;
    olh_entry e = lh_entry(s, 0);
    while (!e.is_leaf) {
        olh_entry l = lh_entry(s, e.id), r = lh_entry(s, e.id + 1);
        float prop = lh_prop(&l, &r, from);
        int left = (code & 1u) == 0;
        e = left ? l : r;
        p *= left ? prop : 1 - prop;
        code >>= 1;
    }
    return p;
}
/* LightSelector::sample / pdf */
static int select_light(const oracle_scene* s, rng_t* rnd, v3 from, float* pdf) {
    int n = s->num_lights, ninf = s->num_infinite;
    if (s->selector == IGX_SELECT_UNIFORM) {
        *pdf = 1.0f / (float)n;
        return n <= 1 ? 0 : rng_i32(rnd, 0, n - 1);
    }
    if (ninf == 0) return finite_select(s, rnd, from, pdf);
    float q = rng_f32(rnd);
    if (q < 0.5f) {
        *pdf = (1 / (float)ninf) * 0.5f;
        return ninf <= 1 ? 0 : rng_i32(rnd, 0, ninf - 1);
    }
    float p;
    int f = finite_select(s, rnd, from, &p);
    *pdf = p * (1 - 0.5f);
    return ninf + f;
}
static float select_pdf(const oracle_scene* s, int lid, v3 from) {
    int n = s->num_lights, ninf = s->num_infinite;
    if (s->selector == IGX_SELECT_UNIFORM) return n == 0 ? 1.0f : 1.0f / (float)n;
    if (ninf == 0) return finite_pdf(s, lid, from);
    if (lid < ninf) return (1 / (float)ninf) * 0.5f;
    return finite_pdf(s, lid - ninf, from) * (1 - 0.5f);
}


/* ---- binned-SAH BVH2, collapsed to 4-wide nodes --------------------------
 * The reference CPU device traverses BVH4 trees with Tri4 leaves built by
 * madmann91/bvh's SAH builders (TriMeshProvider.cpp:551-559, TriBVHAdapter.h,
 * BvhNAdapter.h).  This is an independent, simple equivalent: 16-bin SAH over
 * the three axes (leaf when no split beats the leaf cost), then each 4-wide
 * node absorbs the largest-area inner children of its binary subtree.
 * Closest hits do not depend on the tree (the equal-distance rule below is
 * order-independent), so the tree only sets the speed of the CPU baseline. */
typedef struct {
    const float* bmin;
    const float* bmax;
    int32_t* idx;
    onode* nodes;
    int num_nodes, cap;
    int max_leaf;
} obuild;

#define SAH_BINS 16
static float box_half_area(const float* lo, const float* hi) {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (dx < 0 || dy < 0 || dz < 0) return 0;
    return dx * dy + dy * dz + dz * dx;
}
static void box_empty(float* lo, float* hi) {
    for (int k = 0; k < 3; ++k) { lo[k] = FLT_MAX_; hi[k] = -FLT_MAX_; }
}
static void box_grow(float* lo, float* hi, const float* plo, const float* phi) {
    for (int k = 0; k < 3; ++k) {
        if (plo[k] < lo[k]) lo[k] = plo[k];
        if (phi[k] > hi[k]) hi[k] = phi[k];
    }
}
static void range_box(obuild* b, int first, int count, float* lo, float* hi) {
    box_empty(lo, hi);
    for (int i = first; i < first + count; ++i) box_grow(lo, hi, b->bmin + 3 * b->idx[i], b->bmax + 3 * b->idx[i]);
}
static int32_t new_node(obuild* b) {
    if (b->num_nodes == b->cap) {
        b->cap = b->cap * 2 + 16;
        b->nodes = (onode*)realloc(b->nodes, sizeof(onode) * (size_t)b->cap);
    }
    return b->num_nodes++;
}
/* returns the child ref of the range [first, first + count) */
static int32_t build_range(obuild* b, int first, int count) {
    float clo[3], chi[3];
    box_empty(clo, chi);
    for (int i = first; i < first + count; ++i) {
        int p = b->idx[i];
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = 0.5f * (b->bmin[3 * p + k] + b->bmax[3 * p + k]);
        box_grow(clo, chi, c, c);
    }
    float plo[3], phi[3];
    range_box(b, first, count, plo, phi);
    const float leaf_cost = (float)count * box_half_area(plo, phi); /* intersection cost 1, traversal 1 */
    float best_cost = FLT_MAX_;
    int best_axis = -1, best_bin = 0;
    for (int ax = 0; ax < 3; ++ax) {
        float ext = chi[ax] - clo[ax];
        if (!(ext > 0)) continue;
        int cnt[SAH_BINS] = {0};
        float blo[SAH_BINS][3], bhi[SAH_BINS][3];
        for (int i = 0; i < SAH_BINS; ++i) box_empty(blo[i], bhi[i]);
        for (int i = first; i < first + count; ++i) {
            int p = b->idx[i];
            float c = 0.5f * (b->bmin[3 * p + ax] + b->bmax[3 * p + ax]);
            int bin = (int)((c - clo[ax]) / ext * SAH_BINS);
            bin = bin < 0 ? 0 : (bin >= SAH_BINS ? SAH_BINS - 1 : bin);
            cnt[bin]++;
            box_grow(blo[bin], bhi[bin], b->bmin + 3 * p, b->bmax + 3 * p);
        }
        float rarea[SAH_BINS];
        int rcnt[SAH_BINS];
        float lo[3], hi[3];
        box_empty(lo, hi);
        int n = 0;
        for (int i = SAH_BINS - 1; i > 0; --i) {
            box_grow(lo, hi, blo[i], bhi[i]);
            n += cnt[i];
            rarea[i] = box_half_area(lo, hi);
            rcnt[i] = n;
        }
        box_empty(lo, hi);
        n = 0;
        for (int i = 0; i < SAH_BINS - 1; ++i) {
            box_grow(lo, hi, blo[i], bhi[i]);
            n += cnt[i];
            if (n == 0 || rcnt[i + 1] == 0) continue;
            float cost = box_half_area(plo, phi) + (float)n * box_half_area(lo, hi) + (float)rcnt[i + 1] * rarea[i + 1];
            if (cost < best_cost) { best_cost = cost; best_axis = ax; best_bin = i; }
        }
    }
    if (count <= b->max_leaf && (best_axis < 0 || leaf_cost <= best_cost)) return ~((first << 4) | (count - 1));
    int mid;
    if (best_axis >= 0) {
        float ext = chi[best_axis] - clo[best_axis];
        int i = first, j = first + count - 1;
        while (i <= j) { /* partition by bin */
            int p = b->idx[i];
            float c = 0.5f * (b->bmin[3 * p + best_axis] + b->bmax[3 * p + best_axis]);
            int bin = (int)((c - clo[best_axis]) / ext * SAH_BINS);
            bin = bin < 0 ? 0 : (bin >= SAH_BINS ? SAH_BINS - 1 : bin);
            if (bin <= best_bin) ++i;
            else { int t = b->idx[i]; b->idx[i] = b->idx[j]; b->idx[j] = t; --j; }
        }
        mid = i - first;
    } else {
        mid = count / 2; /* all centroids equal: halve */
    }
    int32_t me = new_node(b);
    int32_t l = build_range(b, first, mid);
    int32_t r = build_range(b, first + mid, count - mid);
    onode* nd = &b->nodes[me];
    range_box(b, first, mid, nd->c[0].lo, nd->c[0].hi);
    range_box(b, first + mid, count - mid, nd->c[1].lo, nd->c[1].hi);
    nd->c[0].ref = l;
    nd->c[1].ref = r;
    return me;
}
/* collapse the binary subtree under node2 `i` into 4-wide nodes; returns the new node index */
static int32_t collapse(const obuild* b, int32_t i, onode4** out, int* n_out, int* cap) {
    ochild kids[4];
    int nk = 2;
    kids[0] = b->nodes[i].c[0];
    kids[1] = b->nodes[i].c[1];
    while (nk < 4) {
        int pick = -1;
        float area = -1;
        for (int k = 0; k < nk; ++k)
            if (kids[k].ref >= 0 && box_half_area(kids[k].lo, kids[k].hi) > area) {
                area = box_half_area(kids[k].lo, kids[k].hi);
                pick = k;
            }
        if (pick < 0) break;
        const onode* g = &b->nodes[kids[pick].ref];
        kids[pick] = g->c[0];
        kids[nk++] = g->c[1];
    }
    if (*n_out == *cap) {
        *cap = *cap * 2 + 16;
        *out = (onode4*)realloc(*out, sizeof(onode4) * (size_t)*cap);
    }
    int32_t me = (*n_out)++;
    onode4 nd;
    memset(&nd, 0, sizeof(nd));
    nd.n = nk;
    for (int k = 0; k < nk; ++k) {
        for (int a = 0; a < 3; ++a) { nd.lo[a][k] = kids[k].lo[a]; nd.hi[a][k] = kids[k].hi[a]; }
        nd.ref[k] = kids[k].ref >= 0 ? collapse(b, kids[k].ref, out, n_out, cap) : kids[k].ref;
    }
    (*out)[me] = nd;
    return me;
}
static obvh build_bvh(const float* bmin, const float* bmax, int n, int max_leaf) {
    obuild b;
    memset(&b, 0, sizeof(b));
    b.bmin = bmin;
    b.bmax = bmax;
    b.max_leaf = max_leaf;
    b.idx = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) b.idx[i] = i;
    obvh out;
    out.nodes = NULL;
    out.num_nodes = 0;
    int cap = 0;
    int32_t root = n > 0 ? build_range(&b, 0, n) : -1;
    if (root >= 0) {
        collapse(&b, root, &out.nodes, &out.num_nodes, &cap);
    } else {
        /* a single leaf: a root node holding just that leaf */
        out.nodes = (onode4*)calloc(1, sizeof(onode4));
        out.num_nodes = 1;
        out.nodes[0].n = n > 0 ? 1 : 0;
        out.nodes[0].ref[0] = root;
        float lo[3], hi[3];
        range_box(&b, 0, n, lo, hi);
        for (int a = 0; a < 3; ++a) { out.nodes[0].lo[a][0] = lo[a]; out.nodes[0].hi[a][0] = hi[a]; }
    }
    free(b.nodes);
    out.order = b.idx;
    return out;
}

oracle_scene* oracle_scene_create(const igx_scene_desc* desc) {
    if (!desc) return NULL;
    oracle_scene* s = (oracle_scene*)calloc(1, sizeof(oracle_scene));
    s->desc = *desc;
    s->shapes = (oshape*)calloc(desc->num_shapes ? desc->num_shapes : 1, sizeof(oshape));
    for (uint32_t i = 0; i < desc->num_shapes; ++i) {
        const igx_shape* sh = &desc->shapes[i];
        oshape* o = &s->shapes[i];
        o->type = sh->type;
        o->mesh = sh->mesh;
        memcpy(o->sphere, sh->sphere, sizeof(o->sphere));
        if (sh->type != IGX_SHAPE_TRIMESH) continue;
        const igx_mesh* m = &desc->meshes[sh->mesh];
        int nf = (int)m->num_faces;
        float* bmin = (float*)malloc(sizeof(float) * 3 * (size_t)nf);
        float* bmax = (float*)malloc(sizeof(float) * 3 * (size_t)nf);
        for (int f = 0; f < nf; ++f)
            for (int k = 0; k < 3; ++k) {
                float lo = FLT_MAX_, hi = -FLT_MAX_;
                for (int j = 0; j < 3; ++j) {
                    float v = m->vertices[3 * m->indices[3 * f + j] + k];
                    lo = fminf(lo, v);
                    hi = fmaxf(hi, v);
                }
                bmin[3 * f + k] = lo;
                bmax[3 * f + k] = hi;
            }
        o->bvh = build_bvh(bmin, bmax, nf, 4);
        free(bmin);
        free(bmax);
        o->tri = (float*)malloc(sizeof(float) * 12 * (size_t)nf);
        for (int slot = 0; slot < nf; ++slot) {
            int f = o->bvh.order[slot];
            const float* v0 = m->vertices + 3 * m->indices[3 * f];
            const float* v1 = m->vertices + 3 * m->indices[3 * f + 1];
            const float* v2 = m->vertices + 3 * m->indices[3 * f + 2];
            v3 a = V(v0[0], v0[1], v0[2]);
            v3 e1 = V(v0[0] - v1[0], v0[1] - v1[1], v0[2] - v1[2]);
            v3 e2 = V(v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]);
            v3 n = vcross(e1, e2);
            float* t = o->tri + 12 * slot;
            t[0] = a.x; t[1] = a.y; t[2] = a.z;
            t[3] = e1.x; t[4] = e1.y; t[5] = e1.z;
            t[6] = e2.x; t[7] = e2.y; t[8] = e2.z;
            t[9] = n.x; t[10] = n.y; t[11] = n.z;
        }
    }
    int ne = (int)desc->num_entities;
    if (ne > 0) {
        float* bmin = (float*)malloc(sizeof(float) * 3 * (size_t)ne);
        float* bmax = (float*)malloc(sizeof(float) * 3 * (size_t)ne);
        for (int e = 0; e < ne; ++e)
            for (int k = 0; k < 3; ++k) {
                bmin[3 * e + k] = desc->entities[e].bbox_min[k];
                bmax[3 * e + k] = desc->entities[e].bbox_max[k];
            }
        s->tlas = build_bvh(bmin, bmax, ne, 1);
        free(bmin);
        free(bmax);
    }
    /* lights: infinite first (light/light_selector.art:26-44) */
    s->lights = (olight*)calloc(desc->num_lights ? desc->num_lights : 1, sizeof(olight));
    int* remap = (int*)malloc(sizeof(int) * (desc->num_lights ? desc->num_lights : 1));
    int k = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t l = 0; l < desc->num_lights; ++l) {
            const igx_light* L = &desc->lights[l];
            int inf = L->type == IGX_LIGHT_ENV || L->type == IGX_LIGHT_DIRECTIONAL || L->type == IGX_LIGHT_SUN ||
                      L->type == IGX_LIGHT_ENVMAP;
            if ((pass == 0) != inf) continue;
            olight* o = &s->lights[k];
            o->type = L->type;
            o->infinite = inf;
            o->desc_light = (int)l;
            o->delta = L->type == IGX_LIGHT_POINT || L->type == IGX_LIGHT_SPOT || L->type == IGX_LIGHT_DIRECTIONAL ||
                       L->type == IGX_LIGHT_SUN;
            memcpy(o->rad, L->radiance, sizeof(o->rad));
            memcpy(o->sel_pos, L->select_position, sizeof(o->sel_pos));
            memcpy(o->sel_dir, L->select_direction, sizeof(o->sel_dir));
            o->sel_flux = L->select_flux;
            o->sel_has_dir = L->select_has_direction;
            memcpy(o->origin, L->origin, sizeof(o->origin));
            memcpy(o->normal, L->normal, sizeof(o->normal));
            if (L->type == IGX_LIGHT_PLANE) {
                /* make_plane_area_emitter (light/area.art:107-115) */
                v3 xa = V(L->x_axis[0], L->x_axis[1], L->x_axis[2]);
                v3 ya = V(L->y_axis[0], L->y_axis[1], L->y_axis[2]);
                o->width = vlen(xa);
                o->height = vlen(ya);
                v3 ex = vmulf(xa, 1 / o->width), ey = vmulf(ya, 1 / o->height);
                o->ex[0] = ex.x; o->ex[1] = ex.y; o->ex[2] = ex.z;
                o->ey[0] = ey.x; o->ey[1] = ey.y; o->ey[2] = ey.z;
                o->area = L->area;
            } else if (L->type == IGX_LIGHT_SUN) {
                float c = L->cutoff, r = sqrtf(1 - c * c) / c;
                o->sun_cos = c;
                o->sun_area = PI_ * r * r;
            } else if (L->type == IGX_LIGHT_SPHERE) {
                /* make_sphere_area_emitter (light/area.art:240-246): the area is
                 * recomputed here from the entity transform, not taken from the desc */
                const float* g = desc->entities[L->entity].to_global;
                float r = L->radius;
                float l1 = vlen(V(g[0] * r, g[4] * r, g[8] * r));
                float l2 = vlen(V(g[1] * r, g[5] * r, g[9] * r));
                float l3 = vlen(V(g[2] * r, g[6] * r, g[10] * r));
                const float P = 1.6f;
                o->entity = L->entity;
                o->sph[0] = L->origin[0]; o->sph[1] = L->origin[1]; o->sph[2] = L->origin[2]; o->sph[3] = r;
                o->sph_area = 4 * PI_ * powf((powf(l1 * l2, P) + powf(l1 * l3, P) + powf(l2 * l3, P)) / 3, 1 / P);
            } else if (L->type == IGX_LIGHT_MESH) {
                o->entity = L->entity;
                o->faces = (int)desc->meshes[desc->shapes[desc->entities[L->entity].shape].mesh].num_faces;
            } else if (L->type == IGX_LIGHT_SPOT) {
                float cc = cosf(L->cutoff), cf = cosf(L->falloff);
                o->cos_cut = cc;
                o->blend = cf - cc;
            }
            remap[l] = k++;
        }
    s->num_lights = k;
    s->num_infinite = 0;
    for (int i = 0; i < k; ++i) s->num_infinite += s->lights[i].infinite;
    build_selector(s, desc->technique.light_selector);
    s->mat_light = (int*)malloc(sizeof(int) * (desc->num_materials ? desc->num_materials : 1));
    for (uint32_t m = 0; m < desc->num_materials; ++m) {
        int l = desc->materials[m].light;
        s->mat_light[m] = (l >= 0 && (uint32_t)l < desc->num_lights) ? remap[l] : -1;
    }
    free(remap);
    float dx = desc->scene_bbox_max[0] - desc->scene_bbox_min[0];
    float dy = desc->scene_bbox_max[1] - desc->scene_bbox_min[1];
    float dz = desc->scene_bbox_max[2] - desc->scene_bbox_min[2];
    s->scene_radius = sqrtf(dx * dx + dy * dy + dz * dz) / 2 * 1.01f;
    return s;
}

void oracle_scene_free(oracle_scene* s) {
    if (!s) return;
    for (uint32_t i = 0; i < s->desc.num_shapes; ++i) {
        free(s->shapes[i].bvh.nodes);
        free(s->shapes[i].bvh.order);
        free(s->shapes[i].tri);
    }
    free(s->shapes);
    free(s->tlas.nodes);
    free(s->tlas.order);
    free(s->lights);
    free(s->sel_cdf);
    free(s->lh_codes);
    free(s->lh_nodes);
    free(s->mat_light);
    free(s);
}

/* ------------------------------------------------------------------------ */
/* Traversal (traversal/mapping_cpu.art:398-495 semantics, scalar)          */
/* ------------------------------------------------------------------------ */
typedef struct {
    v3 org, dir, inv_dir, inv_org;
    float tmin, tmax;
    uint32_t flags;
} oray;
typedef struct {
    float t, u, v;
    int prim, ent;
} ohit;
typedef struct {
    uint64_t nodes, leaves, tris;
} otstats;

/* make_ray (traversal/ray.art:27-39) */
static oray make_ray(v3 org, v3 dir, float tmin, float tmax, uint32_t flags) {
    oray r;
    r.org = org;
    r.dir = dir;
    r.inv_dir = V(safe_rcp(dir.x), safe_rcp(dir.y), safe_rcp(dir.z));
    r.inv_org = vneg(vmul(org, r.inv_dir));
    r.tmin = tmin;
    r.tmax = tmax;
    r.flags = flags;
    return r;
}

/* intersect_ray_box, unordered, make_default_min_max (intersection.art:46-50, 170-181) */
static inline float dmin(float x, float y) { return x < y ? x : y; }
static inline float dmax(float x, float y) { return x > y ? x : y; }
static inline void ray_box(const oray* r, const float* lo, const float* hi, float* entry, float* exit) {
    float t0x = lo[0] * r->inv_dir.x + r->inv_org.x, t1x = hi[0] * r->inv_dir.x + r->inv_org.x;
    float t0y = lo[1] * r->inv_dir.y + r->inv_org.y, t1y = hi[1] * r->inv_dir.y + r->inv_org.y;
    float t0z = lo[2] * r->inv_dir.z + r->inv_org.z, t1z = hi[2] * r->inv_dir.z + r->inv_org.z;
    *entry = dmax(dmax(dmin(t0x, t1x), dmin(t0y, t1y)), dmax(dmin(t0z, t1z), r->tmin));
    *exit = dmin(dmin(dmax(t0x, t1x), dmax(t0y, t1y)), dmin(dmax(t0z, t1z), r->tmax));
}

/* Moeller-Trumbore (intersection.art:71-101) */
static int tri_test(const oray* r, const float* t, float* tt, float* uu, float* vv) {
    v3 v0 = V(t[0], t[1], t[2]), e1 = V(t[3], t[4], t[5]), e2 = V(t[6], t[7], t[8]), n = V(t[9], t[10], t[11]);
    v3 c = vsub(v0, r->org);
    v3 rr = vcross(r->dir, c);
    float det = vdot(n, r->dir);
    float inv_det = 1 / det;
    float u = vdot(rr, e2) * inv_det;
    float v = vdot(rr, e1) * inv_det;
    float w = 1 - u - v;
    int mask = u >= -FLT_EPS_ && v >= -FLT_EPS_ && w >= -FLT_EPS_;
    if (!mask) return 0;
    float tv = vdot(c, n) * inv_det;
    if (!(tv >= r->tmin && tv <= r->tmax)) return 0;
    *tt = tv;
    *uu = u > 0 ? u : 0;
    *vv = v > 0 ? v : 0;
    return 1;
}

/* intersect_sphere (shapes/sphere.art:104-130) */
static int sphere_test(const oray* r, const float* sph, float* tt) {
    v3 L = vsub(r->org, V(sph[0], sph[1], sph[2]));
    float S = -vdot(L, r->dir);
    float D2 = vdot(r->dir, r->dir);
    float L2 = vdot(L, L);
    float R2 = sph[3] * sph[3] * D2;
    float M2 = L2 * D2 - S * S;
    if (S < 0 || M2 > R2) return 0;
    float Q = sqrtf(R2 - M2);
    float ta = (S - Q) / D2, tb = (S + Q) / D2;
    float t0 = ta > tb ? tb : ta, t1 = ta > tb ? ta : tb;
    float th = t0 < r->tmin ? t1 : t0;
    if (th >= r->tmin && th <= r->tmax) { *tt = th; return 1; }
    return 0;
}

#define OSTACK 256
typedef struct { int32_t ref; float tmin; } sentry;

/* One 4-wide node: slab-test the valid children and push the hit ones, the
 * nearest on top (cpu_traverse_helper, traversal/mapping_cpu.art:398-495). */
static inline void push_children(const onode4* n, const oray* r, sentry* stack, int* sp) {
    float en[4];
    int32_t ref[4];
    int m = 0;
    for (int k = 0; k < n->n; ++k) {
        float e, x;
        float lo[3] = {n->lo[0][k], n->lo[1][k], n->lo[2][k]}, hi[3] = {n->hi[0][k], n->hi[1][k], n->hi[2][k]};
        ray_box(r, lo, hi, &e, &x);
        if (x < e) continue;
        int j = m++; /* insertion by entry distance, farthest first */
        while (j > 0 && en[j - 1] < e) { en[j] = en[j - 1]; ref[j] = ref[j - 1]; --j; }
        en[j] = e;
        ref[j] = n->ref[k];
    }
    for (int j = 0; j < m; ++j) stack[(*sp)++] = (sentry){ref[j], en[j]};
}

/* Tie rule at equal distance: 0 the larger (entity, primitive) wins, as on
 * the device (order-independent); 1 the later-visited hit wins, the
 * reference's rule (intersection.art:97, traversal/mapping_gpu.art:208:
 * distance <= hit.distance), which depends on BVH topology and visiting
 * order.  Test hook: tests/test_oracle.py measures what the rule changes. */
static int tie_rule_reference = 0;
void oracle_set_tie_rule(int reference) { tie_rule_reference = reference != 0; }

/* BLAS traversal in entity space (cpu_traverse_helper_prim) */
static int traverse_blas(const oshape* sh, oray* r, int any, ohit* h, otstats* st) {
    sentry stack[OSTACK];
    int sp = 0;
    int found = 0;
    stack[sp++] = (sentry){0, r->tmin};
    while (sp > 0) {
        sentry e = stack[--sp];
        if (e.tmin > r->tmax) continue; /* cull */
        if (e.ref >= 0) {
            st->nodes++;
            push_children(&sh->bvh.nodes[e.ref], r, stack, &sp);
        } else {
            int code = ~e.ref;
            int first = code >> 4, count = (code & 15) + 1;
            for (int k = 0; k < count; ++k) {
                st->tris++;
                float t, u, v;
                if (tri_test(r, sh->tri + 12 * (first + k), &t, &u, &v)) {
                    /* ties at equal distance: the larger primitive id wins (order-independent
                       rule shared with the device; the reference keeps the later-visited
                       triangle, intersection.art:97, which depends on BVH topology) */
                    if (!tie_rule_reference && t == r->tmax && !((int)sh->bvh.order[first + k] > h->prim)) continue;
                    r->tmax = t;
                    h->t = t;
                    h->u = u;
                    h->v = v;
                    h->prim = sh->bvh.order[first + k];
                    found = 1;
                    if (any) return 1;
                }
            }
        }
    }
    return found;
}

static int trace_scene(const oracle_scene* s, const oray* ray_in, int any, ohit* hit, otstats* st) {
    hit->ent = -1;
    hit->prim = -1;
    hit->t = ray_in->tmax;
    hit->u = hit->v = 0;
    if (s->desc.num_entities == 0) return 0;
    oray ray = *ray_in;
    sentry stack[OSTACK];
    int sp = 0;
    stack[sp++] = (sentry){0, ray.tmin};
    while (sp > 0) {
        sentry e = stack[--sp];
        if (e.tmin > ray.tmax) continue;
        if (e.ref >= 0) {
            st->nodes++;
            push_children(&s->tlas.nodes[e.ref], &ray, stack, &sp);
            continue;
        }
        int code = ~e.ref;
        int first = code >> 4, count = (code & 15) + 1;
        for (int k = 0; k < count; ++k) {
            st->leaves++;
            int eid = s->tlas.order[first + k];
            const igx_entity* ent = &s->desc.entities[eid];
            /* check_ray_visibility (ray.art:51) */
            if ((ray.flags & RAY_TYPE_MASK) != ((ray.flags & ent->flags) & RAY_TYPE_MASK)) continue;
            /* intersect_ray_box_single_section on the entity box + tmin <= hit.distance */
            float en, ex;
            ray_box(&ray, ent->bbox_min, ent->bbox_max, &en, &ex);
            if (!((en <= ex) && (ex >= 0))) continue;
            if (!(en <= hit->t)) continue;
            /* transform_ray (ray.art:53-59): no renormalisation */
            const float* m = ent->to_local;
            v3 lo = V(m[0] * ray.org.x + m[1] * ray.org.y + m[2] * ray.org.z + m[3],
                      m[4] * ray.org.x + m[5] * ray.org.y + m[6] * ray.org.z + m[7],
                      m[8] * ray.org.x + m[9] * ray.org.y + m[10] * ray.org.z + m[11]);
            v3 ld = V(m[0] * ray.dir.x + m[1] * ray.dir.y + m[2] * ray.dir.z,
                      m[4] * ray.dir.x + m[5] * ray.dir.y + m[6] * ray.dir.z,
                      m[8] * ray.dir.x + m[9] * ray.dir.y + m[10] * ray.dir.z);
            oray lr = make_ray(lo, ld, ray.tmin, ray.tmax, ray.flags);
            const oshape* sh = &s->shapes[ent->shape];
            ohit lh = {lr.tmax, 0, 0, -1, -1};
            int got;
            if (sh->type == IGX_SHAPE_SPHERE) {
                float t;
                got = sphere_test(&lr, sh->sphere, &t);
                if (got) { lh.t = t; lh.prim = 0; }
            } else {
                got = traverse_blas(sh, &lr, any, &lh, st);
            }
            if (got && lh.prim != -1 && (lh.t < hit->t || (lh.t == hit->t && (tie_rule_reference || eid > hit->ent)))) {
                hit->ent = eid;
                hit->prim = lh.prim;
                hit->t = lh.t;
                hit->u = lh.u;
                hit->v = lh.v;
                ray.tmax = lh.t;
                if (any) return 1;
            }
        }
    }
    return hit->ent >= 0;
}

/* ------------------------------------------------------------------------ */
/* Shading                                                                   */
/* ------------------------------------------------------------------------ */
typedef struct {
    v3 point, face_normal;
    frame_t local;
    int entering;
    float tu, tv; /* texture coordinates (vec2_lerp2 of the mesh's, shapes/trimesh.art:25) */
} osurf;

static inline v3 xf_point(const float* m, v3 p) {
    return V(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
             m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
static inline v3 xf_normal(const float* n, v3 p) {
    return V(n[0] * p.x + n[1] * p.y + n[2] * p.z, n[3] * p.x + n[4] * p.y + n[5] * p.z, n[6] * p.x + n[7] * p.y + n[8] * p.z);
}

/* make_trimesh_shape.surface_element (shapes/trimesh.art:14-39); sphere (shapes/sphere.art:50-64) */
static osurf surface_element(const oracle_scene* s, const ohit* h, const oray* r) {
    const igx_entity* ent = &s->desc.entities[h->ent];
    const oshape* sh = &s->shapes[ent->shape];
    osurf out;
    out.point = vadd(r->org, vmulf(r->dir, h->t));
    if (sh->type == IGX_SHAPE_SPHERE) {
        v3 dir = vsub(out.point, xf_point(ent->to_global, V(sh->sphere[0], sh->sphere[1], sh->sphere[2])));
        float l = vlen(dir);
        v3 n = vmulf(dir, 1 / l);
        out.entering = 1;
        out.face_normal = n;
        out.local = make_frame(n);
        out.tu = out.tv = 0;
        return out;
    }
    const igx_mesh* m = &s->desc.meshes[sh->mesh];
    const uint32_t* f = m->indices + 3 * h->prim;
    v3 p0 = V(m->vertices[3 * f[0]], m->vertices[3 * f[0] + 1], m->vertices[3 * f[0] + 2]);
    v3 p1 = V(m->vertices[3 * f[1]], m->vertices[3 * f[1] + 1], m->vertices[3 * f[1] + 2]);
    v3 p2 = V(m->vertices[3 * f[2]], m->vertices[3 * f[2] + 1], m->vertices[3 * f[2] + 2]);
    v3 v0 = xf_point(ent->to_global, p0), v1 = xf_point(ent->to_global, p1), v2 = xf_point(ent->to_global, p2);
    v3 e1 = vsub(v1, v0), e2 = vsub(v2, v0);
    v3 n = vcross(e1, e2);
    float nn = vlen(n);
    v3 fn = vmulf(n, 1 / nn);
    v3 n0 = V(m->normals[3 * f[0]], m->normals[3 * f[0] + 1], m->normals[3 * f[0] + 2]);
    v3 n1 = V(m->normals[3 * f[1]], m->normals[3 * f[1] + 1], m->normals[3 * f[1] + 2]);
    v3 n2 = V(m->normals[3 * f[2]], m->normals[3 * f[2] + 1], m->normals[3 * f[2] + 2]);
    v3 ln = V(lerp2(n0.x, n1.x, n2.x, h->u, h->v), lerp2(n0.y, n1.y, n2.y, h->u, h->v), lerp2(n0.z, n1.z, n2.z, h->u, h->v));
    v3 normal = vnormalize(xf_normal(ent->normal, ln));
    out.entering = vdot(r->dir, fn) <= 0;
    out.face_normal = out.entering ? fn : vneg(fn);
    out.local = make_frame(out.entering ? normal : vneg(normal));
    out.tu = out.tv = 0;
    if (m->texcoords) {
        const float* t = m->texcoords;
        out.tu = lerp2(t[2 * f[0]], t[2 * f[1]], t[2 * f[2]], h->u, h->v);
        out.tv = lerp2(t[2 * f[0] + 1], t[2 * f[1] + 1], t[2 * f[2] + 1], h->u, h->v);
    }
    return out;
}

/* node_checkerboard3 (texture/checkerboard.art:2) on uvw * scale with
 * math::wrap(x, 0, 2) as i32 % 2 per axis (core/math.art:88-91); uvw =
 * (u, v, 0) (driver/shading_context.art:38) */
static int checker_bit(float x) { return ((int)(x - 2.0f * floorf(x / 2.0f))) % 2; }
static int checkerboard3(float u, float v, float scale) {
    const int a = checker_bit(u * scale), b = checker_bit(v * scale), c = checker_bit(0.0f * scale);
    return (a == b) == (c == 1) ? 1 : 0;
}

/* compute_sq (light/area.art:127-176) */
typedef struct { v3 o, n; float x0, y0, z0, x1, y1, b0, b1, k, s; } sq_t;
static inline float safe_acos(float a) { return acosf(clampf_(a, -1, 1)); }
static sq_t compute_sq(const olight* L, v3 from) {
    v3 origin = V(L->origin[0], L->origin[1], L->origin[2]);
    v3 ex = V(L->ex[0], L->ex[1], L->ex[2]), ey = V(L->ey[0], L->ey[1], L->ey[2]);
    v3 normal = V(L->normal[0], L->normal[1], L->normal[2]);
    v3 dir = vsub(origin, from);
    sq_t q;
    q.x0 = vdot(dir, ex);
    q.y0 = vdot(dir, ey);
    float z0_ = vdot(dir, normal);
    q.x1 = q.x0 + L->width;
    q.y1 = q.y0 + L->height;
    int nsb = !signbit(z0_);
    q.z0 = nsb ? -z0_ : z0_;
    q.n = nsb ? vneg(normal) : normal;
    float dx = q.x0 - q.x1, dy = q.y1 - q.y0, dz = q.x1 - q.x0, dw = q.y0 - q.y1;
    float zx = q.y0 * dx, zy = q.x1 * dy, zz = q.y1 * dz, zw = q.x0 * dw;
    float z02 = q.z0 * q.z0;
    float nzx = zx / sqrtf((dx * dx) * z02 + zx * zx);
    float nzy = zy / sqrtf((dy * dy) * z02 + zy * zy);
    float nzz = zz / sqrtf((dz * dz) * z02 + zz * zz);
    float nzw = zw / sqrtf((dw * dw) * z02 + zw * zw);
    float g0 = safe_acos(-nzx * nzy);
    float g1 = safe_acos(-nzy * nzz);
    float g2 = safe_acos(-nzz * nzw);
    float g3 = safe_acos(-nzw * nzx);
    q.b0 = nzx;
    q.b1 = nzz;
    q.k = 2 * PI_ - g2 - g3;
    q.s = g0 + g1 - q.k;
    q.o = from;
    return q;
}

typedef struct {
    v3 pos, dir, intensity;
    float pdf_value;
    int pdf_solid;
    float cos, dist;
} odirect;

/* equal_area_square_to_sphere (core/warp.art:63-91) */
static v3 eq_area_sphere(float ux, float uy) {
    float u = 2 * ux - 1, v = 2 * uy - 1;
    float au = fabsf(u), av = fabsf(v);
    float sd = 1 - (au + av);
    float dd = fabsf(sd);
    float r = 1 - dd;
    float phi = (r == 0 ? 1.0f : (av - au) / r + 1) * PI_ / 4;
    float ct = copysignf(1 - r * r, sd);
    float st = safe_sqrt(2 - r * r) * r;
    float cp = copysignf(cosf(phi), u);
    float sp = copysignf(sinf(phi), v);
    return V(cp * st, sp * st, ct);
}

/* world-space triangle `f` of a mesh entity (make_triangle, core/triangle.art:11-26) */
static void emitter_triangle(const oracle_scene* s, int entity, int f, v3* v0, v3* v1, v3* v2, v3* n, float* area) {
    const igx_entity* ent = &s->desc.entities[entity];
    const igx_mesh* m = &s->desc.meshes[s->desc.shapes[ent->shape].mesh];
    const uint32_t* ix = m->indices + 3 * (size_t)f;
    *v0 = xf_point(ent->to_global, V(m->vertices[3 * ix[0]], m->vertices[3 * ix[0] + 1], m->vertices[3 * ix[0] + 2]));
    *v1 = xf_point(ent->to_global, V(m->vertices[3 * ix[1]], m->vertices[3 * ix[1] + 1], m->vertices[3 * ix[1] + 2]));
    *v2 = xf_point(ent->to_global, V(m->vertices[3 * ix[2]], m->vertices[3 * ix[2] + 1], m->vertices[3 * ix[2] + 2]));
    v3 c = vcross(vsub(*v1, *v0), vsub(*v2, *v0));
    float nn = vlen(c);
    *n = vmulf(c, 1 / nn);
    *area = nn / 2;
}

/* face picked by the shape emitter for sample coordinates u (light/area.art:49-50) */
static int emitter_face(const olight* L, float u) {
    float ux = u * (float)L->faces;
    int f = (int)ux;
    return f < L->faces - 1 ? f : L->faces - 1;
}

/* sphere emitter point for a local normal (sphere_compute_surface_element_for_normal, shapes/sphere.art:29-42) */
static void sphere_point(const oracle_scene* s, const olight* L, v3 nrm, v3* p, v3* fn) {
    const igx_entity* ent = &s->desc.entities[L->entity];
    v3 o = V(L->sph[0], L->sph[1], L->sph[2]);
    *p = xf_point(ent->to_global, vadd(o, vmulf(nrm, L->sph[3])));
    *fn = vnormalize(xf_normal(ent->normal, nrm));
}

/* Light::pdf_direct of an area light, solid-angle measure (make_area_light, light/area.art:41) */
static float area_pdf_direct_solid(const oracle_scene* s, const olight* L, v3 org, float cos, float dist2, float u) {
    if (L->type == IGX_LIGHT_PLANE) { sq_t q = compute_sq(L, org); return safe_div(1, q.s); }
    if (L->type == IGX_LIGHT_SPHERE) return (2 / L->sph_area) * dist2 / cos;
    if (L->type == IGX_LIGHT_MESH) {
        v3 a, b, c, n;
        float area;
        emitter_triangle(s, L->entity, emitter_face(L, u), &a, &b, &c, &n, &area);
        return ((1 / area) / (float)L->faces) * dist2 / cos;
    }
    return 1 / (4 * PI_);
}

static odirect light_sample_direct(const oracle_scene* s, const olight* L, rng_t* rnd, const osurf* from) {
    odirect d;
    v3 rad = V(L->rad[0], L->rad[1], L->rad[2]);
    if (L->type == IGX_LIGHT_PLANE) {
        float ux = rng_f32(rnd);
        float uy = rng_f32(rnd);
        sq_t q = compute_sq(L, from->point);
        v3 ex = V(L->ex[0], L->ex[1], L->ex[2]), ey = V(L->ey[0], L->ey[1], L->ey[2]);
        float au = fmaf(ux, q.s, q.k);
        float fu = fmaf(cosf(au), q.b0, -q.b1) / sinf(au);
        float cu = clampf_(copysignf(1.0f, fu) / sqrtf(sum_of_prod(fu, fu, q.b0, q.b0)), -1, 1);
        float xu = clampf_(-(cu * q.z0) / sqrtf(fmaf(-cu, cu, 1.0f)), q.x0, q.x1);
        float dd = sqrtf(sum_of_prod(xu, xu, q.z0, q.z0));
        float h0 = q.y0 / sqrtf(sum_of_prod(dd, dd, q.y0, q.y0));
        float h1 = q.y1 / sqrtf(sum_of_prod(dd, dd, q.y1, q.y1));
        float hv = fmaf(uy, h1 - h0, h0);
        float hv2 = hv * hv;
        float yv = hv2 < 1 - 1e-6f ? (hv * dd) / sqrtf(1 - hv2) : q.y1;
        v3 p = vadd(q.o, vadd(vmulf(ex, xu), vadd(vmulf(ey, yv), vmulf(q.n, q.z0))));
        v3 dir_ = vsub(p, from->point);
        float dist = vlen(dir_);
        v3 dir = vmulf(dir_, safe_div(1, dist));
        v3 normal = V(L->normal[0], L->normal[1], L->normal[2]);
        d.pos = p;
        d.dir = dir;
        d.intensity = vmulf(rad, q.s);
        d.pdf_value = safe_div(1, q.s);
        d.pdf_solid = 1;
        d.cos = vdot(dir, normal) * (from->entering ? -1.0f : 1.0f);
        d.dist = dist;
    } else if (L->type == IGX_LIGHT_ENV) {
        float ux = rng_f32(rnd);
        float uy = rng_f32(rnd);
        v3 dir = eq_area_sphere(ux, uy);
        float pdf = 1 / (4 * PI_);
        d.intensity = vmulf(rad, 1 / pdf);
        d.pos = vadd(from->point, vmulf(dir, s->scene_radius));
        d.dir = dir;
        d.pdf_value = pdf;
        d.pdf_solid = 1;
        d.cos = 1.0f;
        d.dist = s->scene_radius;
    } else if (L->type == IGX_LIGHT_DIRECTIONAL) {
        /* light/directional.art:6 */
        v3 dir = V(L->normal[0], L->normal[1], L->normal[2]);
        d.pos = vadd(from->point, vmulf(dir, -s->scene_radius));
        d.dir = vneg(dir);
        d.intensity = rad;
        d.pdf_value = 1;
        d.pdf_solid = 1; /* delta pdf: as_solid = 1 */
        d.cos = 1;
        d.dist = s->scene_radius;
    } else if (L->type == IGX_LIGHT_SUN) {
        /* light/sun.art:10-14, sample_uniform_cone (core/sampling.art:106-116) */
        float u = rng_f32(rnd), v = rng_f32(rnd);
        float c1 = 1 - L->sun_cos;
        float a = 2 * u - 1, b = 2 * v - 1, px, py;
        if (a == 0 && b == 0) { px = 0; py = 0; }
        else if (a * a > b * b) { float phi = (PI_ / 4) * safe_div(b, a); px = cosf(phi) * a; py = sinf(phi) * a; }
        else { float phi = (PI_ / 2) - (PI_ / 4) * safe_div(a, b); px = cosf(phi) * b; py = sinf(phi) * b; }
        float n2 = px * px + py * py;
        float z = L->sun_cos + c1 * (1 - n2);
        float sc = safe_sqrt(c1 * (2 - c1 * n2));
        float den = 2 * PI_ * (1 - L->sun_cos);
        float pdf = fabsf(den) <= FLT_EPS_ ? 1.0f : 1 / den;
        frame_t fr = make_frame(V(L->normal[0], L->normal[1], L->normal[2]));
        v3 nd = frame_to_world(&fr, V(px * sc, py * sc, z));
        d.pos = V(0, 0, 0);
        d.dir = vneg(nd);
        d.intensity = vmulf(rad, 1 / (L->sun_area * pdf));
        d.pdf_value = 1;
        d.pdf_solid = 1;
        d.cos = z;
        d.dist = INFINITY;
    } else if (L->type == IGX_LIGHT_SPHERE || L->type == IGX_LIGHT_MESH) {
        float ux = rng_f32(rnd);
        float uy = rng_f32(rnd);
        v3 p, fn;
        float pdf_a, weight;
        if (L->type == IGX_LIGHT_SPHERE) {
            /* make_sphere_area_emitter.sample_direct (light/area.art:248-274) */
            v3 glb = xf_point(s->desc.entities[L->entity].to_global, V(L->sph[0], L->sph[1], L->sph[2]));
            sphere_point(s, L, eq_area_sphere(ux, uy), &p, &fn);
            v3 os = vsub(from->point, glb), pq = vsub(from->point, p);
            if (!(vdot(pq, pq) <= vdot(os, os))) {
                v3 np = vsub(p, vmulf(vsub(p, glb), 2));
                sphere_point(s, L, vnormalize(vsub(np, glb)), &p, &fn);
            }
            float inv_area = 1 / L->sph_area;
            pdf_a = 2 * inv_area;
            weight = 1 / (2 * inv_area);
        } else {
            /* make_shape_area_emitter.sample (light/area.art:48-57) */
            int f = emitter_face(L, ux);
            float su = ux * (float)L->faces - (float)f, sw = uy;
            if (su + sw > 1) { su = 1 - su; sw = 1 - sw; }
            v3 a, b, c;
            float area;
            emitter_triangle(s, L->entity, f, &a, &b, &c, &fn, &area);
            float inv_area = 1 / area;
            p = V(lerp2(a.x, b.x, c.x, su, sw), lerp2(a.y, b.y, c.y, su, sw), lerp2(a.z, b.z, c.z, su, sw));
            pdf_a = inv_area / (float)L->faces;
            weight = (float)L->faces / inv_area;
        }
        /* make_area_light.sample_direct (light/area.art:12-27) */
        v3 dir_ = vsub(p, from->point);
        float dist = vlen(dir_);
        v3 dir = vmulf(dir_, safe_div(1, dist));
        d.pos = p;
        d.dir = dir;
        d.intensity = vmulf(rad, weight);
        d.pdf_value = pdf_a;
        d.pdf_solid = 0;
        d.cos = vdot(dir, fn) * (from->entering ? -1.0f : 1.0f);
        d.dist = dist;
    } else if (L->type == IGX_LIGHT_POINT) {
        v3 pos = V(L->origin[0], L->origin[1], L->origin[2]);
        v3 dir_ = vsub(pos, from->point);
        float dist = vlen(dir_);
        d.dir = vmulf(dir_, safe_div(1, dist));
        d.pos = pos;
        d.intensity = rad;
        d.pdf_value = 1;
        d.pdf_solid = 0;
        d.cos = 1;
        d.dist = dist;
    } else {
        v3 pos = V(L->origin[0], L->origin[1], L->origin[2]);
        v3 sdir = V(L->normal[0], L->normal[1], L->normal[2]);
        v3 od_ = vsub(pos, from->point);
        float dist = vlen(od_);
        v3 od = vmulf(od_, safe_div(1, dist));
        float cos_angle = vdot(vneg(od), sdir);
        float factor;
        if (L->blend <= FLT_EPS_) factor = cos_angle <= L->cos_cut ? 0.0f : 1.0f;
        else {
            float x = clampf_((cos_angle - L->cos_cut) / L->blend, 0, 1);
            factor = x * x * (3 - 2 * x);
        }
        d.intensity = vmulf(rad, factor);
        d.pos = pos;
        d.dir = od;
        d.cos = -vdot(od, sdir);
        d.pdf_value = vdot(vneg(od), sdir) > L->cos_cut ? 1.0f : 0.0f;
        d.pdf_solid = 0;
        d.dist = dist;
    }
    return d;
}

static inline float fresnel_factor(float eta, float cos_i, float cos_t) {
    float rs = safe_div(eta * cos_i - cos_t, eta * cos_i + cos_t);
    float rp = safe_div(cos_i - eta * cos_t, cos_i + eta * cos_t);
    return clampf_((rs * rs + rp * rp) * 0.5f, 0, 1);
}

/* ------------------------------------------------------------------------ */
/* BSDFs: the Artic Bsdf records {eval, pdf, sample, is_specular} built per  */
/* hit (bsdf/diffuse.art, dielectric.art, conductor.art, plastic.art, mix.art */
/* and core/microfacet.art), restated as one record + lobe functions.        */
/* ------------------------------------------------------------------------ */
enum { LOBE_LAMBERT, LOBE_OREN_NAYAR, LOBE_DIELECTRIC, LOBE_MIRROR, LOBE_PURE_CONDUCTOR, LOBE_ROUGH_CONDUCTOR, LOBE_THIN_DIELECTRIC };

typedef struct {
    int lobe;          /* primary lobe; plastic = mix(LAMBERT+scatter, spec) */
    int plastic;
    int spec;          /* plastic specular lobe: LOBE_MIRROR or LOBE_ROUGH_CONDUCTOR */
    int model;         /* IGX_MICROFACET_* for rough lobes */
    float au, av, on_alpha;
    v3 kd, ks, kt, eta, kap;
    float n1, n2;
    const osurf* surf;
    int principled;    /* make_principled_bsdf (bsdf/principled.art:238-481) */
    const igx_material* mat;
} obsdf;

typedef struct { v3 dir; float pdf; v3 color; float eta; int ok; } osample;

static inline osample osample_make(v3 d, float pdf, v3 c, float eta) { osample r = {d, pdf, c, eta, 1}; return r; }
static inline osample osample_reject(void) { osample r = {V(0, 0, 0), 0, V(0, 0, 0), 1, 0}; return r; }
static inline float pos_cos(v3 a, v3 b) { float c = vdot(a, b); return c >= 0 ? c : 0; }
static inline float abs_cos(v3 a, v3 b) { return fabsf(vdot(a, b)); }
static inline v3 vreflect(v3 v, v3 n) { return vsub(vmulf(n, 2 * vdot(n, v)), v); }
static inline v3 vhalf(v3 a, v3 b) { return vnormalize(vadd(a, b)); }
static inline float lerp1(float a, float b, float k) { return (1 - k) * a + k * b; }
static inline v3 clerp(v3 a, v3 b, float t) { return V((1 - t) * a.x + t * b.x, (1 - t) * a.y + t * b.y, (1 - t) * a.z + t * b.z); }
static inline float diff_of_prod(float a, float b, float c, float d) {
    float cd = c * d;
    return fmaf(a, b, -cd) + fmaf(-c, d, cd);
}
/* core/fresnel.art */
static float fresnel_dielectric_f(float eta, float cos_i) {
    float eta2 = cos_i < 0 ? 1 / eta : eta;
    float c2 = 1 - (1 - cos_i * cos_i) * eta2 * eta2;
    return c2 <= 0.0f ? 1.0f : fresnel_factor(eta2, fabsf(cos_i), sqrtf(c2));
}
static float conductor_f(float n, float k, float ci) {
    float f = n * n + k * k, d1 = f * ci * ci, d2 = 2.0f * n * ci;
    float rs = safe_div(d1 - d2, d1 + d2), rp = safe_div(f - d2 + ci * ci, f + d2 + ci * ci);
    return clampf_((rs * rs + rp * rp) * 0.5f, 0, 1);
}
static float diffuse_fresnel(float eta) {
    if (eta < 1) return -1.4399f * (eta * eta) + 0.7099f * eta + 0.6681f + 0.0636f / eta;
    float a = 1 / eta, b = a * a, c = b * a, d = c * a, e = d * a;
    return 0.919317f - 3.4793f * a + 6.75335f * b - 7.80989f * c + 4.98554f * d - 1.36881f * e;
}
/* core/microfacet.art */
static float d_ggx(const frame_t* l, v3 m, float au, float av) {
    float z = vdot(l->n, m), x = vdot(l->t, m), y = vdot(l->b, m);
    float kx = x / au, ky = y / av, k = kx * kx + ky * ky + z * z;
    return safe_div(1, PI_ * au * av * k * k);
}
static float d_beckmann(const frame_t* l, v3 m, float au, float av) {
    float z = vdot(l->n, m), x = vdot(l->t, m), y = vdot(l->b, m);
    float kx = x / au, ky = y / av;
    float k2 = safe_div(kx * kx + ky * ky, z * z);
    return safe_div(expf(-k2), PI_ * au * av * z * z * z * z);
}
static float g1_smith_f(const frame_t* l, v3 w, float au, float av) {
    float z = vdot(l->n, w);
    if (fabsf(z) <= FLT_EPS_) return 0;
    float kx = au * vdot(l->t, w), ky = av * vdot(l->b, w), a2 = kx * kx + ky * ky;
    if (a2 <= FLT_EPS_) return 1;
    return 2 / (1 + sqrtf(1 + a2 / (z * z)));
}
static float g1_walter_f(const frame_t* l, v3 w, float au, float av) {
    float z = vdot(l->n, w);
    if (fabsf(z) <= FLT_EPS_) return 0;
    float kx = au * vdot(l->t, w), ky = av * vdot(l->b, w);
    float k2 = (kx * kx + ky * ky) / (z * z);
    if (k2 <= FLT_EPS_) return 1;
    float a = 1 / sqrtf(k2), a2 = 1 / k2;
    if (a >= 1.6f) return 1.0f;
    return (3.535f * a + 2.181f * a2) / (1.0f + 2.276f * a + 2.577f * a2);
}
static float mf_d(const obsdf* b, v3 h) {
    return b->model == IGX_MICROFACET_BECKMANN ? d_beckmann(&b->surf->local, h, b->au, b->av) : d_ggx(&b->surf->local, h, b->au, b->av);
}
static float mf_g(const obsdf* b, v3 wi, v3 wo) {
    const frame_t* l = &b->surf->local;
    if (b->model == IGX_MICROFACET_BECKMANN) return g1_walter_f(l, wi, b->au, b->av) * g1_walter_f(l, wo, b->au, b->av);
    return g1_smith_f(l, wi, b->au, b->av) * g1_smith_f(l, wo, b->au, b->av);
}
static float vndf_pdf(const frame_t* l, v3 w, v3 h, float au, float av) {
    return safe_div(g1_smith_f(l, w, au, av) * abs_cos(w, h) * d_ggx(l, h, au, av), abs_cos(l->n, w));
}
static float mf_pdf(const obsdf* b, v3 wo, v3 h) {
    if (b->model == IGX_MICROFACET_VNDF_GGX) return vndf_pdf(&b->surf->local, wo, h, b->au, b->av);
    return mf_d(b, h) * abs_cos(b->surf->local.n, h);
}
static v3 mf_sample(const obsdf* b, rng_t* r, v3 wo, float* pdf) {
    const frame_t* l = &b->surf->local;
    const float au = b->au, av = b->av;
    if (b->model == IGX_MICROFACET_VNDF_GGX) {
        /* Heitz 2018 (sample_vndf_ggx / sample_vndf_ggx_11) */
        v3 vl = V(vdot(l->t, wo), vdot(l->b, wo), vdot(l->n, wo));
        v3 sl = vnormalize(V(au * vl.x, av * vl.y, vl.z));
        float st = safe_sqrt(1 - sl.z * sl.z);
        float sphi = 0, cphi = 1;
        if (fabsf(st) > FLT_EPS_) { sphi = sl.y / st; cphi = sl.x / st; }
        float ct = fabsf(sl.z);
        float u0 = rng_f32(r), u1 = rng_f32(r);
        float a = 2 * u0 - 1, c = 2 * u1 - 1, px, py;
        if (a == 0 && c == 0) { px = 0; py = 0; }
        else if (a * a > c * c) { float phi = (PI_ / 4) * safe_div(c, a); px = cosf(phi) * a; py = sinf(phi) * a; }
        else { float phi = (PI_ / 2) - (PI_ / 4) * safe_div(a, c); px = cosf(phi) * c; py = sinf(phi) * c; }
        float sv = 0.5f * (1 + ct);
        float y = (1 - sv) * safe_sqrt(1 - px * px) + sv * py;
        float z = safe_sqrt(1 - y * y - px * px);
        float sin_t = safe_sqrt(1 - ct * ct);
        float norm = safe_div(1, sum_of_prod(sin_t, y, ct, z));
        float sx = diff_of_prod(ct, y, sin_t, z) * norm, sy = px * norm;
        float tx = (cphi * sx - sphi * sy) * au, ty = (sphi * sx + cphi * sy) * av;
        v3 nh = isfinite(tx) ? vnormalize(V(-tx, -ty, 1)) : V(0, 0, 0);
        v3 h = frame_to_world(l, nh);
        *pdf = vndf_pdf(l, wo, h, au, av);
        return h;
    }
    float u0 = rng_f32(r), u1 = rng_f32(r), ar = av / au;
    if (b->model == IGX_MICROFACET_BECKMANN) {
        float phi = atanf(ar * tanf(2 * PI_ * u1));
        float cp = cosf(phi), sp = sqrtf(1 - cp * cp);
        float kx = cp / au, ky = sp / av, k2 = 1 / (kx * kx + ky * ky);
        float cth = 1 / sqrtf(1 - k2 * logf(1.0f - u0)), c2 = cth * cth, sth = sqrtf(1 - c2);
        *pdf = (1 - u0) / (PI_ * au * av * c2 * cth);
        return frame_to_world(l, V(sth * cp, sth * sp, cth));
    }
    float phi = au == av ? 2 * PI_ * u1 : atanf(ar * tanf(2 * PI_ * u1));
    float cp = cosf(phi), sp = sqrtf(1 - cp * cp);
    float kx = cp / au, ky = sp / av, d2 = kx * kx + ky * ky;
    float t2 = safe_div(1, d2) * u0 / (1 - u0);
    float cth = 1 / sqrtf(1 + t2), c2 = cth * cth, sth = sqrtf(1 - c2);
    float k2 = d2 * (sth * sth) / c2;
    *pdf = safe_div(1, PI_ * au * av * c2 * cth * (1 + k2) * (1 + k2));
    return frame_to_world(l, V(sth * cp, sth * sp, cth));
}

static obsdf obsdf_make(const igx_material* m, const osurf* surf) {
    obsdf b;
    memset(&b, 0, sizeof(b));
    b.surf = surf;
    b.kd = V(m->kd[0], m->kd[1], m->kd[2]);
    b.ks = V(m->ks[0], m->ks[1], m->ks[2]);
    b.kt = V(m->kt[0], m->kt[1], m->kt[2]);
    b.eta = V(m->eta[0], m->eta[1], m->eta[2]);
    b.kap = V(m->kappa[0], m->kappa[1], m->kappa[2]);
    b.n1 = m->ext_ior;
    b.n2 = m->int_ior;
    b.au = m->alpha_u;
    b.av = m->alpha_v;
    b.on_alpha = m->diffuse_alpha;
    /* check_if_delta_distribution: alpha <= 1e-4 */
    int rough = m->distribution != IGX_MICROFACET_DELTA && m->alpha_u > 1e-4f && m->alpha_v > 1e-4f;
    b.model = rough ? m->distribution : IGX_MICROFACET_DELTA;
    switch (m->bsdf_type) {
    case IGX_BSDF_DIELECTRIC: b.lobe = m->thin ? LOBE_THIN_DIELECTRIC : LOBE_DIELECTRIC; break;
    case IGX_BSDF_CONDUCTOR:
        if (rough) b.lobe = LOBE_ROUGH_CONDUCTOR;
        else {
            int mirror = fabsf(b.eta.x) <= 1e-4f && fabsf(b.eta.y) <= 1e-4f && fabsf(b.eta.z) <= 1e-4f &&
                         fabsf(b.kap.x - 1) <= 1e-4f && fabsf(b.kap.y - 1) <= 1e-4f && fabsf(b.kap.z - 1) <= 1e-4f;
            b.lobe = mirror ? LOBE_MIRROR : LOBE_PURE_CONDUCTOR;
        }
        break;
    case IGX_BSDF_PRINCIPLED:
        b.principled = 1;
        b.mat = m;
        break;
    case IGX_BSDF_PLASTIC:
        b.plastic = 1;
        b.lobe = LOBE_LAMBERT;
        b.spec = rough ? LOBE_ROUGH_CONDUCTOR : LOBE_MIRROR;
        b.eta = V(0, 0, 0);
        b.kap = V(1, 1, 1);
        break;
    default: b.lobe = m->diffuse_alpha <= FLT_EPS_ ? LOBE_LAMBERT : LOBE_OREN_NAYAR; break;
    }
    return b;
}
static int obsdf_specular(const obsdf* b) {
    return !b->plastic && !b->principled && (b->lobe == LOBE_DIELECTRIC || b->lobe == LOBE_THIN_DIELECTRIC || b->lobe == LOBE_MIRROR || b->lobe == LOBE_PURE_CONDUCTOR);
}
static int lobe_specular(int lobe) {
    return lobe == LOBE_DIELECTRIC || lobe == LOBE_THIN_DIELECTRIC || lobe == LOBE_MIRROR || lobe == LOBE_PURE_CONDUCTOR;
}

static v3 rough_eval(const obsdf* b, v3 in, v3 out) {
    v3 N = b->surf->local.n;
    float co = abs_cos(out, N), ci = abs_cos(in, N);
    if (co <= FLT_EPS_ || ci <= FLT_EPS_) return V(0, 0, 0);
    v3 h = vhalf(in, out);
    float D = mf_d(b, h), G = mf_g(b, in, out), ch = abs_cos(out, h);
    v3 F = V(conductor_f(b->eta.x, b->kap.x, ch), conductor_f(b->eta.y, b->kap.y, ch), conductor_f(b->eta.z, b->kap.z, ch));
    return vmulf(vmul(b->ks, F), D * G / (4 * co));
}
static float rough_pdf(const obsdf* b, v3 in, v3 out) {
    v3 h = vhalf(in, out);
    return mf_pdf(b, out, h) * safe_div(1, 4 * abs_cos(out, h));
}
/* eval / pdf / sample of one lobe (plastic's diffuse lobe carries the inner scattering term) */
static float plastic_scatter_f(const obsdf* b, float ci) {
    float eta = b->n1 / b->n2;
    return (1 - fresnel_dielectric_f(eta, ci)) * eta * eta / (1 - diffuse_fresnel(eta));
}
static v3 lobe_eval(const obsdf* b, int lobe, v3 in, v3 out) {
    v3 N = b->surf->local.n;
    switch (lobe) {
    case LOBE_LAMBERT: {
        v3 e = vmulf(b->kd, abs_cos(in, N) * INV_PI_);
        return b->plastic ? vmulf(e, plastic_scatter_f(b, abs_cos(in, N))) : e;
    }
    case LOBE_OREN_NAYAR: {
        float a2 = b->on_alpha * b->on_alpha;
        float p1 = abs_cos(in, N), p2 = abs_cos(out, N);
        float sv = -p1 * p2 + pos_cos(out, in);
        float t = sv <= FLT_EPS_ ? 1.0f : fmaxf(FLT_EPS_, fmaxf(p1, p2));
        float A = 1 - 0.5f * a2 / (a2 + 0.33f), B = 0.45f * a2 / (a2 + 0.09f), C = 0.17f * a2 / (a2 + 0.13f);
        return vmulf(vadd(vmulf(b->kd, (A + (B * sv / t)) / PI_), vmul(b->kd, vmulf(b->kd, C / PI_))), p1);
    }
    case LOBE_ROUGH_CONDUCTOR: return rough_eval(b, in, out);
    default: return V(0, 0, 0);
    }
}
static float lobe_pdf(const obsdf* b, int lobe, v3 in, v3 out) {
    if (lobe == LOBE_LAMBERT || lobe == LOBE_OREN_NAYAR) return pos_cos(in, b->surf->local.n) / PI_;
    if (lobe == LOBE_ROUGH_CONDUCTOR) return rough_pdf(b, in, out);
    return 0;
}
static osample lobe_sample(const obsdf* b, int lobe, rng_t* r, v3 out) {
    const osurf* sf = b->surf;
    v3 N = sf->local.n;
    switch (lobe) {
    case LOBE_LAMBERT:
    case LOBE_OREN_NAYAR: {
        float u = rng_f32(r), v = rng_f32(r);
        float c = safe_sqrt(v), sn = safe_sqrt(1 - v), phi = 2 * PI_ * u;
        float pdf = c / PI_;
        v3 d = frame_to_world(&sf->local, V(sn * cosf(phi), sn * sinf(phi), c));
        if (lobe == LOBE_OREN_NAYAR) return osample_make(d, pdf, vmulf(lobe_eval(b, lobe, d, out), 1 / pdf), 1);
        v3 col = b->plastic ? vmulf(b->kd, plastic_scatter_f(b, abs_cos(d, N))) : b->kd;
        return osample_make(d, pdf, col, 1);
    }
    case LOBE_DIELECTRIC: {
        float k = sf->entering ? b->n1 / b->n2 : b->n2 / b->n1;
        float co = vdot(out, N);
        float ft_cos_t = 0, ft_factor = 1;
        float eta2 = co < 0 ? 1 / k : k;
        float c2 = 1 - (1 - co * co) * eta2 * eta2;
        if (!(c2 <= 0.0f)) {
            float ct = sqrtf(c2);
            ft_cos_t = co < 0 ? -ct : ct;
            ft_factor = fresnel_factor(eta2, fabsf(co), ct);
        }
        if (rng_f32(r) > ft_factor) return osample_make(vsub(vmulf(N, k * co - ft_cos_t), vmulf(out, k)), 1, b->kt, k);
        return osample_make(vreflect(out, N), 1, b->ks, 1);
    }
    case LOBE_THIN_DIELECTRIC: {
        /* make_thin_dielectric_bsdf (bsdf/dielectric.art:26-47): always outside -> inside,
         * F = f + (1 - f) f / (f + 1) (the inter-reflection sum of a thin slab), straight
         * transmission with eta 1 */
        float k = b->n1 / b->n2;
        float f = fresnel_dielectric_f(k, abs_cos(out, N));
        float F = f + (1 - f) * f / (f + 1);
        if (rng_f32(r) > F) return osample_make(vmulf(out, -1), 1, b->kt, 1);
        return osample_make(vnormalize(vreflect(out, N)), 1, b->ks, 1);
    }
    case LOBE_MIRROR: return osample_make(vreflect(out, N), 1, b->ks, 1);
    case LOBE_PURE_CONDUCTOR: {
        float ci = vdot(out, N);
        v3 F = V(conductor_f(b->eta.x, b->kap.x, ci), conductor_f(b->eta.y, b->kap.y, ci), conductor_f(b->eta.z, b->kap.z, ci));
        return osample_make(vreflect(out, N), 1, vmul(b->ks, F), 1);
    }
    default: { /* rough conductor */
        if (abs_cos(out, N) <= FLT_EPS_) return osample_reject();
        float mpdf;
        v3 mn = mf_sample(b, r, out, &mpdf);
        if (vdot(mn, mn) <= FLT_EPS_) return osample_reject();
        v3 oh = vnormalize(mn);
        v3 h = signbit(vdot(oh, out)) ? vneg(oh) : oh;
        v3 in = vreflect(out, h);
        if (abs_cos(in, N) <= FLT_EPS_) return osample_reject();
        float pdf = mpdf * (1 / (4 * abs_cos(out, h)));
        return osample_make(in, pdf, vmulf(rough_eval(b, in, out), safe_div(1, pdf)), 1);
    }
    }
}

/* ---- principled BSDF (bsdf/principled.art), restated in the local shading
 * frame: w.z is the cosine to the shading normal, microfacet lobes use the
 * identity frame. -------------------------------------------------------- */
typedef struct {
    v3 base;
    float eta, ior, ru, rv, dtr, str, stint, flat, metal, sheen, sheen_tint, cc, ccg, ccr;
    int thin, cc_top, entering;
} oprin;

static const frame_t PRIN_IDENTITY = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};

static oprin oprin_make(const igx_material* m, const osurf* sf) {
    oprin p;
    p.base = V(m->kd[0], m->kd[1], m->kd[2]);
    p.ru = fmaxf(1e-3f, m->alpha_u);
    p.rv = fmaxf(1e-3f, m->alpha_v);
    p.dtr = m->diffuse_transmission;
    p.str = m->specular_transmission;
    p.stint = m->specular_tint;
    p.flat = m->flatness;
    p.metal = m->metallic;
    p.sheen = m->sheen;
    p.sheen_tint = m->sheen_tint;
    p.cc = m->clearcoat;
    p.ccg = m->clearcoat_gloss;
    p.ccr = m->clearcoat_roughness;
    p.thin = m->thin != 0;
    p.cc_top = m->clearcoat_top_only != 0;
    p.entering = sf->entering;
    p.ior = m->ior;
    p.eta = (sf->entering || p.thin) ? 1 / m->ior : m->ior;
    return p;
}
static float lum_of(v3 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }
static v3 tint_of(v3 c) {
    float l = lum_of(c);
    if (l <= FLT_EPS_) return V(1, 1, 1);
    return V(c.x / l, c.y / l, c.z / l);
}
static float schlick_w(float f) {
    float s = clampf_(1 - f, 0, 1);
    return (s * s) * (s * s) * s;
}
static int hemi_same(v3 a, v3 b) { return (a.z >= 0) == (b.z >= 0); }
static v3 hemi_like(v3 a, v3 b) { return hemi_same(a, b) ? b : vneg(b); }
static v3 hemi_pos(v3 v) { return v.z >= 0 ? v : vneg(v); }
static float jac_refr(float eta, float ci, float co) {
    float d = ci + co * eta;
    return safe_div(eta * eta * ci, d * d);
}
static float prin_g(const oprin* p, v3 wi, v3 wo) {
    return g1_smith_f(&PRIN_IDENTITY, wi, p->ru, p->rv) * g1_smith_f(&PRIN_IDENTITY, wo, p->ru, p->rv);
}
/* diffuse lobe of prin_eval_local: 0 the reference's (evalDiffuseTerm,
 * bsdf/principled.art:117-129); 1 and 2 are what-if models of another
 * renderer, used ONLY by oracle_principled_eval (tests/golden/cycles_box_model.py) */
static int prin_diffuse_model = 0;
static v3 prin_eval_local(const oprin* p, v3 wo, v3 wi) {
    int trans = !hemi_same(wi, wo);
    v3 h = hemi_like(wo, trans ? vnormalize(vadd(wi, vmulf(wo, p->eta))) : vnormalize(vadd(wi, wo)));
    int in_front = p->entering == (wi.z >= 0), out_front = p->entering == (wo.z >= 0);
    float cl = fabsf(wi.z), cv = fabsf(wo.z);
    if (cl <= 1e-5f) return V(0, 0, 0);
    v3 c = V(0, 0, 0);
    float m01 = clampf_(p->metal, 0, 1), s01 = clampf_(p->str, 0, 1);
    float w_diff = (p->thin ? 1.0f : 1 - m01) * (1 - s01);
    float w_trans = (1 - m01) * s01;
    float lk = schlick_w(cl), vk = schlick_w(cv);
    if (!trans) {
        if (w_diff > 0) {
            float base_d = (1 - 0.5f * lk) * (1 - 0.5f * vk);
            float rr = (fabsf(vdot(wi, wo)) + 1) * (p->ru + p->rv) / 2;
            float retro = rr * (lk + vk + lk * vk * (rr - 1));
            if (prin_diffuse_model == 1) {
                /* Disney 2015's split with R = roughness * (1 + L.V) on the
                 * roughness input itself (alpha = roughness^2 here) */
                float rg = sqrtf(0.5f * (p->ru + p->rv));
                rr = rg * (1 + vdot(wi, wo));
                retro = rr * (lk + vk + lk * vk * (rr - 1));
            } else if (prin_diffuse_model == 2) {
                /* Burley 2012: (1 + (F_D90 - 1) F_L)(1 + (F_D90 - 1) F_V), F_D90 = 0.5 + 2 r cos^2(theta_d) */
                float rg = sqrtf(0.5f * (p->ru + p->rv));
                v3 hh = vnormalize(vadd(wi, wo));
                float cd = vdot(wi, hh);
                float fd90 = 0.5f + 2 * rg * cd * cd;
                base_d = (1 + (fd90 - 1) * lk) * (1 + (fd90 - 1) * vk);
                retro = 0;
            }
            float ss = 1;
            if (p->thin) {
                float hl = vdot(wi, h);
                float f90 = hl * hl * (p->ru * p->rv);
                float fss = (1 - lk + f90 * lk) * (1 - vk + f90 * vk);
                float subs = 1.25f * (fss * (1 / (cl + cv + 1e-5f) - 0.5f) + 0.5f);
                ss = 1 - p->flat + subs * p->flat;
            }
            c = vadd(c, vmulf(p->base, INV_PI_ * (base_d + retro) * ss * cl * w_diff));
        }
        if (p->sheen > 0) {
            v3 tint = clerp(V(1, 1, 1), tint_of(p->base), p->sheen_tint);
            c = vadd(c, vmulf(vmulf(tint, p->sheen * lk * cl), w_diff));
        }
        {   /* specular reflection with the Disney Fresnel term */
            float hv = fabsf(vdot(wo, h)), hl = fabsf(vdot(wi, h));
            v3 F = V(0, 0, 0);
            if (!(hv * hl <= FLT_EPS_)) {
                float f1 = fresnel_dielectric_f(p->eta, hv);
                v3 a = clerp(V(1, 1, 1), tint_of(p->base), p->stint);
                float r0f = clampf_((p->eta - 1) / (p->eta + 1), -1, 1);
                v3 r0 = clerp(vmulf(a, r0f * r0f), p->base, p->metal);
                float sw = schlick_w(hl);
                v3 f2 = vadd(r0, vmulf(vsub(V(1, 1, 1), r0), sw));
                F = clerp(V(f1, f1, f1), f2, p->metal);
            }
            float D = d_ggx(&PRIN_IDENTITY, h, p->ru, p->rv);
            float G = prin_g(p, wi, wo);
            c = vadd(c, vmulf(F, fabsf(D * G * safe_div(1, 4 * wo.z))));
        }
        if ((!p->cc_top || (in_front && out_front)) && p->cc > 0) {
            const float R = 0.25f;
            float r2 = fmaxf(0.001f, p->ccr * (1 - p->ccg) + 0.01f * p->ccg);
            float d = d_ggx(&PRIN_IDENTITY, h, r2, r2);
            float f = 0.04f + (1 - 0.04f) * schlick_w(fabsf(vdot(wi, h)));
            float g = g1_smith_f(&PRIN_IDENTITY, wi, R, R) * g1_smith_f(&PRIN_IDENTITY, wo, R, R);
            float v = fabsf(R * d * f * g * safe_div(1, 4 * wo.z) * wi.z);
            c = vadd(c, vmulf(V(v, v, v), p->cc));
        }
    } else {
        if (p->thin && p->dtr > 0) {
            float base_d = (1 - 0.5f * lk) * (1 - 0.5f * vk);
            c = vadd(c, vmulf(p->base, INV_PI_ * base_d * cl * p->dtr));
        }
        if (p->str > 0) {
            float t;
            if (p->thin) {
                float ft = fresnel_dielectric_f(p->eta, cv);
                t = 1 - (ft + (1 - ft) * ft / (ft + 1));
            } else {
                float hi = vdot(wi, h), ho = vdot(wo, h);
                float F = fresnel_dielectric_f(p->eta, fabsf(ho));
                float D = d_ggx(&PRIN_IDENTITY, h, p->ru, p->rv);
                float G = prin_g(p, wi, wo);
                float nrm = fabsf(safe_div(ho * jac_refr(p->eta, hi, ho), wo.z));
                t = (1 - F) * D * G * nrm;
            }
            v3 col = p->thin ? V(sqrtf(p->base.x), sqrtf(p->base.y), sqrtf(p->base.z)) : p->base;
            c = vadd(c, vmulf(vmulf(col, t), w_trans));
        }
    }
    return c;
}
static void prin_lobes(const oprin* p, v3 wo, float* dr, float* dt, float* sr, float* st) {
    float m01 = clampf_(p->metal, 0, 1), d01 = clampf_(p->dtr, 0, 1), s01 = clampf_(p->str, 0, 1);
    float gen = lum_of(p->base);
    float spec = lerp1(1.0f, lum_of(tint_of(p->base)), p->stint);
    float a = clampf_(gen * (1 - m01) * (1 - s01), 0, 1);
    float F = fresnel_dielectric_f(p->eta, fabsf(wo.z));
    float b = clampf_(spec * (1 - F) + F, 0, 1);
    float c = 0, d = 0;
    if (d01 > 0 || s01 > 0) {
        c = clampf_(gen * d01 * a, 0, 1);
        d = clampf_((1 - F) * gen * (1 - m01) * s01, 0, 1);
    }
    float n = a + b + c + d;
    if (n <= FLT_EPS_) { *dr = 1; *dt = 0; *sr = 0; *st = 0; return; }
    *dr = a / n; *dt = c / n; *sr = b / n; *st = d / n;
}
static float prin_bound(float v) { return v <= 1e-5f ? 0.0f : v; }
static float prin_refl_pdf(const oprin* p, v3 wo, v3 wi) {
    v3 a = hemi_pos(wo), b = hemi_pos(wi);
    v3 H = vnormalize(vadd(a, b));
    return fabsf(prin_bound(vndf_pdf(&PRIN_IDENTITY, a, H, p->ru, p->rv)) * safe_div(1, 4 * vdot(a, H)));
}
static float prin_trans_pdf(const oprin* p, v3 wo, v3 wi) {
    v3 a = hemi_pos(wo), b = vneg(hemi_pos(wi));
    v3 H = vnormalize(vadd(b, vmulf(a, p->eta)));
    /* getRefractionMicro (bsdf/principled.art:73-80): a thin surface refracts
     * through a lobe of its own roughness; one at or below 1e-4 is the delta
     * distribution (core/microfacet.art:298), whose pdf is 0 */
    float ru = p->ru, rv = p->rv;
    if (p->thin) {
        const float f = 0.65f * p->ior - 0.35f;
        ru = clampf_(f * ru, 0, 1);
        rv = clampf_(f * rv, 0, 1);
        if (ru <= 1e-4f || rv <= 1e-4f) return 0.0f;
    }
    return fabsf(prin_bound(vndf_pdf(&PRIN_IDENTITY, a, H, ru, rv)) * jac_refr(p->eta, vdot(b, H), vdot(a, H)));
}
static float prin_pdf_local(const oprin* p, v3 wo, v3 wi) {
    if (fabsf(wo.z) <= 1e-5f || fabsf(wi.z) <= 1e-5f) return 0;
    float dr, dt, sr, st;
    prin_lobes(p, wo, &dr, &dt, &sr, &st);
    float cp = fabsf(wi.z) / PI_;
    if (hemi_same(wo, wi)) return dr * cp + sr * prin_refl_pdf(p, wo, wi);
    if (p->thin) return dt * cp + st;
    return dt * cp + st * prin_trans_pdf(p, wo, wi);
}
static v3 local_of(const frame_t* f, v3 v) { return V(vdot(f->t, v), vdot(f->b, v), vdot(f->n, v)); }
static v3 prin_eval(const obsdf* b, v3 in, v3 out) {
    oprin p = oprin_make(b->mat, b->surf);
    return prin_eval_local(&p, local_of(&b->surf->local, out), local_of(&b->surf->local, in));
}
static float prin_pdf(const obsdf* b, v3 in, v3 out) {
    oprin p = oprin_make(b->mat, b->surf);
    return prin_pdf_local(&p, local_of(&b->surf->local, out), local_of(&b->surf->local, in));
}
/* VNDF GGX normal for local pwo (sample_vndf_ggx with the identity frame) */
static v3 prin_vndf(const oprin* p, rng_t* r, v3 pwo, float* pdf) {
    obsdf tmp;
    osurf sf;
    memset(&tmp, 0, sizeof(tmp));
    memset(&sf, 0, sizeof(sf));
    sf.local = PRIN_IDENTITY;
    tmp.surf = &sf;
    tmp.model = IGX_MICROFACET_VNDF_GGX;
    tmp.au = p->ru;
    tmp.av = p->rv;
    return mf_sample(&tmp, r, pwo, pdf);
}
static osample prin_sample(const obsdf* b, rng_t* r, v3 out) {
    const oprin p = oprin_make(b->mat, b->surf);
    const frame_t* L = &b->surf->local;
    v3 wo = local_of(L, out);
    if (fabsf(wo.z) <= 1e-5f) return osample_reject();
    float dr, dt, sr, st;
    prin_lobes(&p, wo, &dr, &dt, &sr, &st);
    float pick = rng_f32(r);
    v3 wi;
    float pdf;
    if (pick < dr || pick < dr + dt) {
        int refl = pick < dr;
        float u = rng_f32(r), v = rng_f32(r);
        float c = safe_sqrt(v), sn = safe_sqrt(1 - v), phi = 2 * PI_ * u;
        v3 d = hemi_like(wo, V(sn * cosf(phi), sn * sinf(phi), c));
        if (refl) {
            wi = d;
            pdf = (c / PI_) * dr + prin_refl_pdf(&p, wo, wi) * sr;
        } else {
            wi = vneg(d);
            pdf = (c / PI_) * dt + prin_trans_pdf(&p, wo, wi) * st;
        }
    } else if (pick < dr + dt + st) {
        if (p.thin) {
            wi = vneg(wo);
            pdf = st;
        } else {
            v3 a = hemi_pos(wo);
            float mp;
            v3 m = prin_vndf(&p, r, a, &mp);
            if (mp <= 1e-5f || vdot(m, m) <= FLT_EPS_) return osample_reject();
            v3 om = vnormalize(m);
            v3 H = signbit(vdot(om, a)) ? vneg(om) : om;
            float ch = vdot(a, H);
            float e2 = ch < 0 ? 1 / p.eta : p.eta;
            float c2 = 1 - (1 - ch * ch) * e2 * e2;
            if (c2 <= 0.0f) { /* total internal reflection */
                v3 bw = vnormalize(vreflect(a, H));
                if (!(hemi_same(a, bw) && ch > FLT_EPS_ && bw.z > 1e-5f)) return osample_reject();
                wi = hemi_like(wo, bw);
                pdf = mp * safe_div(1, 4 * ch) * st + fabsf(wi.z) / PI_ * dt;
            } else {
                float ct = sqrtf(c2);
                if (ch < 0) ct = -ct;
                v3 bw = vnormalize(vsub(vmulf(H, p.eta * ch - ct), vmulf(a, p.eta)));
                if (!(!hemi_same(a, bw) && ch > FLT_EPS_ && -bw.z > 1e-5f)) return osample_reject();
                wi = vneg(hemi_like(wo, bw));
                pdf = fabsf(mp * jac_refr(p.eta, vdot(bw, H), ch)) * st + fabsf(wi.z) / PI_ * dt;
            }
        }
    } else {
        v3 a = hemi_pos(wo);
        float mp;
        v3 m = prin_vndf(&p, r, a, &mp);
        if (mp <= 1e-5f || vdot(m, m) <= FLT_EPS_) return osample_reject();
        v3 om = vnormalize(m);
        v3 H = signbit(vdot(om, a)) ? vneg(om) : om;
        float ch = vdot(a, H);
        v3 bw = vnormalize(vreflect(a, H));
        if (!(hemi_same(a, bw) && ch > FLT_EPS_ && bw.z > 1e-5f)) return osample_reject();
        wi = hemi_like(wo, bw);
        pdf = fabsf(mp * safe_div(1, 4 * ch)) * sr + fabsf(wi.z) / PI_ * dr;
    }
    if (pdf <= FLT_EPS_) return osample_reject();
    float se = (p.thin || hemi_same(wo, wi)) ? 1.0f : p.eta;
    v3 in = frame_to_world(L, wi);
    return osample_make(in, pdf, vmulf(prin_eval(b, in, out), 1 / pdf), se);
}
/* make_variadic_mix_bsdf (bsdf/mix.art) with k = Fresnel(out) for plastic */
static float plastic_k(const obsdf* b, v3 out) { return fresnel_dielectric_f(b->n1 / b->n2, abs_cos(out, b->surf->local.n)); }
static v3 obsdf_eval(const obsdf* b, v3 in, v3 out) {
    if (b->principled) return prin_eval(b, in, out);
    if (!b->plastic) return lobe_eval(b, b->lobe, in, out);
    return clerp(lobe_eval(b, LOBE_LAMBERT, in, out), lobe_eval(b, b->spec, in, out), plastic_k(b, out));
}
static float obsdf_pdf(const obsdf* b, v3 in, v3 out) {
    if (b->principled) return prin_pdf(b, in, out);
    if (!b->plastic) return lobe_pdf(b, b->lobe, in, out);
    return lerp1(lobe_pdf(b, LOBE_LAMBERT, in, out), lobe_pdf(b, b->spec, in, out), plastic_k(b, out));
}
static osample mix_sample_first(const obsdf* b, int first, int second, rng_t* r, v3 out, float t) {
    osample s1 = lobe_sample(b, first, r, out);
    if (!s1.ok || lobe_specular(second)) return s1;
    float p = lerp1(s1.pdf, lobe_pdf(b, second, s1.dir, out), t);
    v3 c = clerp(vmulf(s1.color, s1.pdf), lobe_eval(b, second, s1.dir, out), t);
    s1.pdf = p;
    s1.color = V(c.x / p, c.y / p, c.z / p);
    return s1;
}
static osample obsdf_sample(const obsdf* b, rng_t* r, v3 out) {
    if (b->principled) return prin_sample(b, r, out);
    if (!b->plastic) return lobe_sample(b, b->lobe, r, out);
    float k = plastic_k(b, out);
    if (k <= 0) return lobe_sample(b, LOBE_LAMBERT, r, out);
    if (k >= 1) return lobe_sample(b, b->spec, r, out);
    if (rng_f32(r) < 1 - k) {
        osample s1 = mix_sample_first(b, LOBE_LAMBERT, b->spec, r, out, k);
        return s1.ok ? s1 : lobe_sample(b, b->spec, r, out);
    }
    osample s1 = mix_sample_first(b, b->spec, LOBE_LAMBERT, r, out, 1 - k);
    return s1.ok ? s1 : lobe_sample(b, LOBE_LAMBERT, r, out);
}

static inline v3 handle_color(const oracle_scene* s, v3 c) {
    float cl = s->desc.technique.clamp;
    if (cl > 0) return V(fminf(c.x, cl), fminf(c.y, cl), fminf(c.z, cl));
    return c;
}

typedef struct {
    uint64_t camera, bounce, shadow;
    otstats tr;
} pstats;

/* The state of one path between two bounces: its next ray and the payload of
 * init_pt_raypayload (technique/pathtracer.art:17-38), plus its RNG and pixel */
typedef struct {
    oray ray;
    uint32_t seed, counter;
    v3 contrib;
    float inv_pdf, eta;
    int depth, x, y;
} opath;

/* make_camera_emitter + make_perspective_camera (driver/emitter.art:6-16,
 * camera/perspective.art:29-66), or the ray-list emitter (emitter.art:18-30) */
static void path_begin(const oracle_scene* s, const oracle_params* p, int x, int y, int sample, int list_index, opath* q,
                       pstats* ps) {
    const igx_camera* cam = &s->desc.camera;
    int width = p->num_rays > 0 ? p->num_rays : p->width;
    int height = p->num_rays > 0 ? 1 : p->height;
    q->seed = oracle_random_seed(sample, p->iteration, p->frame, x, y, p->seed);
    rng_t rnd = {q->seed, 1};
    if (p->num_rays > 0) {
        const float* r = p->rays + 8 * list_index;
        q->ray = make_ray(V(r[0], r[1], r[2]), V(r[3], r[4], r[5]), r[6], r[7], 0);
    } else {
        float rx = rng_f32(&rnd);
        float ry = rng_f32(&rnd);
        float nx = 2 * ((float)x + rx) / (float)width - 1;
        float ny = 1 - 2 * ((float)y + ry) / (float)height;
        float aspect = cam->aspect > 0 ? cam->aspect : (float)width / (float)height;
        float sx, sy;
        if (cam->vertical_fov) { sy = tanf(cam->fov / 2); sx = sy * aspect; }
        else { sx = tanf(cam->fov / 2); sy = sx / aspect; }
        v3 dir = V(cam->dir[0], cam->dir[1], cam->dir[2]), up = V(cam->up[0], cam->up[1], cam->up[2]);
        v3 right = vcross(dir, up);
        right = vmulf(right, 1 / vlen(right));
        v3 v = V(sx * nx, sy * ny, 1);
        v3 w = V(right.x * v.x + up.x * v.y + dir.x * v.z, right.y * v.x + up.y * v.y + dir.y * v.z,
                 right.z * v.x + up.z * v.y + dir.z * v.z);
        q->ray = make_ray(V(cam->eye[0], cam->eye[1], cam->eye[2]), vnormalize(w), cam->near_clip, cam->far_clip, RAY_CAMERA);
    }
    ps->camera++;
    q->counter = rnd.counter;
    q->inv_pdf = 0;
    q->eta = 1;
    q->contrib = V(1, 1, 1);
    q->depth = 1;
    q->x = x;
    q->y = y;
}

/* ---- image environment map, as seen by a ray that leaves the scene --------
 * make_environment_light (light/env.art:161-164): scale * tex(map_env_uv(
 * switch_env_up(transform * dir))) (env.art:13-21) through the image texture of
 * texture/image.art (borders :9-39, texel points :53-77, filters :79-143).
 * Only this emission is restated: sampling the map (its CDF) is not, so the
 * oracle renders such a scene with "nee": false only. */
static int tex_border(int wrap, int x, int w) {
    if (wrap == IGX_WRAP_CLAMP) return x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    if (wrap == IGX_WRAP_MIRROR) {
        int t = x < 0 ? -1 - x : x, i = t / w, k = t - i * w;
        return (i & 1) == 0 ? w - 1 - k : k;
    }
    int t = x % w;
    return t < 0 ? t + w : t;
}
static v3 tex_fetch(const igx_image* im, int x, int y) {
    const size_t at = (size_t)y * (size_t)im->width + (size_t)x;
    if (im->format == IGX_IMAGE_FLOAT4) {
        const float* p = (const float*)im->pixels + 4 * at;
        return V(p[0], p[1], p[2]);
    }
    if (im->format == IGX_IMAGE_MONO8) {
        const float g = ((const uint8_t*)im->pixels)[at] / 255.0f;
        return V(g, g, g);
    }
    const uint8_t* p = (const uint8_t*)im->pixels + 4 * at;
    return V(p[0] / 255.0f, p[1] / 255.0f, p[2] / 255.0f);
}
static float cubic_w0(float a) { return (a * (a * (-a + 3) - 3) + 1) / 6; }
static float cubic_w1(float a) { return (a * a * (3 * a - 6) + 4) / 6; }
static float cubic_w2(float a) { return (a * (a * (-3 * a + 3) + 3) + 1) / 6; }
static float cubic_w3(float a) { return (a * a * a) / 6; }
static v3 tex_lookup(const igx_scene_desc* d, const igx_texture* tx, float u0, float v0) {
    const igx_image* im = &d->images[tx->image];
    const float* m = tx->transform;
    const float u = m[0] * u0 + m[1] * v0 + m[2], v = m[3] * u0 + m[4] * v0 + m[5];
    const int w = im->width, h = im->height;
    const float half = tx->filter == IGX_FILTER_NEAREST ? 0.0f : 0.5f;
    const float pu = u * (float)w - half, pv = v * (float)h - half;
    const float fu = floorf(pu), fv = floorf(pv);
    const int ix = (int)fu, iy = (int)fv;
    const float fx = pu - fu, fy = pv - fv;
    if (tx->filter == IGX_FILTER_NEAREST) return tex_fetch(im, tex_border(tx->wrap_u, ix, w), tex_border(tx->wrap_v, iy, h));
    if (tx->filter == IGX_FILTER_BILINEAR) {
        const int x0 = tex_border(tx->wrap_u, ix, w), x1 = tex_border(tx->wrap_u, ix + 1, w);
        const int y0 = tex_border(tx->wrap_v, iy, h), y1 = tex_border(tx->wrap_v, iy + 1, h);
        return clerp(clerp(tex_fetch(im, x0, y0), tex_fetch(im, x1, y0), fx),
                     clerp(tex_fetch(im, x0, y1), tex_fetch(im, x1, y1), fx), fy);
    }
    const float g0x = cubic_w0(fx) + cubic_w1(fx), g1x = cubic_w2(fx) + cubic_w3(fx);
    const float g0y = cubic_w0(fy) + cubic_w1(fy), g1y = cubic_w2(fy) + cubic_w3(fy);
    const int x0 = tex_border(tx->wrap_u, (int)floorf((float)ix + (cubic_w1(fx) / g0x - 1) + 0.5f), w);
    const int y0 = tex_border(tx->wrap_v, (int)floorf((float)iy + (cubic_w1(fy) / g0y - 1) + 0.5f), h);
    const int x1 = tex_border(tx->wrap_u, (int)floorf((float)ix + (cubic_w3(fx) / g1x + 1) + 0.5f), w);
    const int y1 = tex_border(tx->wrap_v, (int)floorf((float)iy + (cubic_w3(fy) / g1y + 1) + 0.5f), h);
    return vadd(vadd(vmulf(tex_fetch(im, x0, y0), g0x * g0y), vmulf(tex_fetch(im, x1, y0), g1x * g0y)),
                vadd(vmulf(tex_fetch(im, x0, y1), g0x * g1y), vmulf(tex_fetch(im, x1, y1), g1x * g1y)));
}
static v3 envmap_emission(const oracle_scene* s, const olight* L, v3 dir) {
    const igx_light* dl = &s->desc.lights[L->desc_light];
    const float* t = dl->sky_transform;
    const v3 l = V(t[0] * dir.x + t[1] * dir.y + t[2] * dir.z, t[3] * dir.x + t[4] * dir.y + t[5] * dir.z,
                   t[6] * dir.x + t[7] * dir.y + t[8] * dir.z);
    const v3 e = V(l.x, l.z, l.y); /* switch_env_up */
    const float theta = acosf(e.z);
    float phi = atan2f(e.y, e.x);
    if (phi < 0) phi += 2 * PI_;
    float u = phi / (2 * PI_) + 0.25f;
    u -= floorf(u);
    const v3 c = tex_lookup(&s->desc, &s->desc.textures[dl->env_texture], u, 1 - theta / PI_);
    return V(c.x * dl->env_scale[0], c.y * dl->env_scale[1], c.z * dl->env_scale[2]);
}

/* One vertex of technique/pathtracer.art:52-200 for the closest hit `h` of the
 * path's ray (h->ent < 0: a miss): the radiance gathered there (*Lacc: on_hit
 * emission with MIS, or on_miss), the NEE shadow ray and its colour
 * (on_shadow; *has_shadow), and the bounce (on_bounce with Russian roulette):
 * returns 1 when the path continues with q->ray, 0 when it ends. */
static int path_shade(const oracle_scene* s, opath* q, const ohit* h, v3* Lacc, int* has_shadow, oray* sray, v3* scol,
                      pstats* ps) {
    const igx_technique* tech = &s->desc.technique;
    const float uni_pdf = s->num_lights == 0 ? 1.0f : 1.0f / (float)s->num_lights;
    const oray* ray = &q->ray;
    *Lacc = V(0, 0, 0);
    *has_shadow = 0;
    if (h->ent < 0) {
        for (int li = 0; li < s->num_infinite; ++li) {
            const olight* L = &s->lights[li];
            if (L->delta) continue;
            v3 emit = V(L->rad[0], L->rad[1], L->rad[2]);
            if (L->type == IGX_LIGHT_ENVMAP) emit = envmap_emission(s, L, ray->dir);
            float pdf_s = 1 / (4 * PI_);
            float sel = s->selector == IGX_SELECT_UNIFORM ? uni_pdf : select_pdf(s, li, ray->org);
            float mis = tech->nee ? 1 / (1 + q->inv_pdf * sel * pdf_s) : 1.0f;
            *Lacc = vadd(*Lacc, handle_color(s, vmulf(vmul(q->contrib, emit), mis)));
        }
        return 0;
    }
    osurf surf = surface_element(s, h, ray);
    const igx_entity* ent = &s->desc.entities[h->ent];
    const igx_material* mat = &s->desc.materials[ent->material];
    int mlight = s->mat_light[ent->material];
    if (mlight >= 0 && surf.entering) {
        float dt = -vdot(ray->dir, surf.local.n);
        if (dt > FLT_EPS_) {
            const olight* L = &s->lights[mlight];
            v3 emit = V(L->rad[0], L->rad[1], L->rad[2]);
            float pdf_s = area_pdf_direct_solid(s, L, ray->org, dt, h->t * h->t, h->u);
            float sel = s->selector == IGX_SELECT_UNIFORM ? uni_pdf : select_pdf(s, mlight, ray->org);
            float mis = tech->nee ? 1 / (1 + q->inv_pdf * sel * pdf_s) : 1.0f;
            *Lacc = vadd(*Lacc, handle_color(s, vmulf(vmul(q->contrib, emit), mis)));
        }
    }
    igx_material textured;
    if (mat->texture == IGX_TEXTURE_CHECKER) { /* select(checkerboard(uvw * s) == 1, kd1, kd) */
        textured = *mat;
        if (checkerboard3(surf.tu, surf.tv, mat->tex_scale) == 1)
            for (int c = 0; c < 3; ++c) textured.kd[c] = mat->tex_kd1[c];
        mat = &textured;
    }
    rng_t r2 = {q->seed, q->counter};
    v3 out_dir = vneg(ray->dir);
    obsdf bs = obsdf_make(mat, &surf);
    int specular = obsdf_specular(&bs);
    /* on_shadow */
    if (tech->nee && !specular && s->num_lights > 0 && q->depth + 1 <= tech->max_depth) {
        float sel_pdf;
        int lid = select_light(s, &r2, surf.point, &sel_pdf);
        const olight* L = &s->lights[lid];
        odirect ls = light_sample_direct(s, L, &r2, &surf);
        float pdf_l_s = (ls.pdf_solid ? ls.pdf_value : ls.pdf_value * (ls.dist * ls.dist) / ls.cos) * sel_pdf;
        if (pdf_l_s > FLT_EPS_ && ls.cos > FLT_EPS_) {
            float mis = L->delta ? 1.0f : 1 / (1 + obsdf_pdf(&bs, ls.dir, out_dir) / pdf_l_s);
            float factor = ls.pdf_value / pdf_l_s;
            v3 ev = obsdf_eval(&bs, ls.dir, out_dir);
            *scol = handle_color(s, vmulf(vmul(ls.intensity, vmul(q->contrib, ev)), mis * factor));
            *sray = L->infinite ? make_ray(surf.point, ls.dir, 0.001f, FLT_MAX_, RAY_SHADOW)
                                : make_ray(surf.point, vsub(ls.pos, surf.point), 0.001f, 1 - 0.001f, RAY_SHADOW);
            *has_shadow = 1;
            ps->shadow++;
        }
    }
    /* on_bounce */
    if (!(q->depth + 1 <= tech->max_depth)) return 0;
    osample smp = obsdf_sample(&bs, &r2, out_dir);
    if (!smp.ok) return 0;
    v3 c2 = vmul(q->contrib, smp.color);
    float rr = 1.0f;
    if (q->depth + 1 > tech->min_depth) {
        v3 e = vmulf(c2, q->eta * q->eta);
        rr = clampf_(fmaxf(fmaxf(e.x, e.y), e.z), 0.05f, 0.95f);
    }
    if (rng_f32(&r2) >= rr) return 0;
    q->inv_pdf = specular ? 0 : 1 / smp.pdf;
    q->contrib = vmulf(c2, 1 / rr);
    q->eta = q->eta * smp.eta;
    q->depth = q->depth + 1;
    q->counter = r2.counter;
    q->ray = make_ray(surf.point, smp.dir, 0.001f, FLT_MAX_, RAY_BOUNCE);
    ps->bounce++;
    return 1;
}

/* One path to its end, bounce by bounce (the per-path form of the loop: the
 * checker's default, bit-identical per path to the wavefront form below) */
static v3 trace_path(const oracle_scene* s, const oracle_params* p, int x, int y, int sample, int list_index, pstats* ps,
                     v3* Ldirect, v3* Lnee) {
    opath q;
    path_begin(s, p, x, y, sample, list_index, &q, ps);
    v3 Lsum = V(0, 0, 0), Ld = V(0, 0, 0), Ln = V(0, 0, 0);
    for (;;) {
        ohit h;
        trace_scene(s, &q.ray, 0, &h, &ps->tr);
        v3 Lacc, scol;
        oray sr;
        int has_shadow;
        int alive = path_shade(s, &q, &h, &Lacc, &has_shadow, &sr, &scol, ps);
        Lsum = vadd(Lsum, Lacc);
        Ld = vadd(Ld, Lacc); /* aov_di.splat (pathtracer.art:128,158) */
        if (has_shadow) {
            ohit sh;
            if (!trace_scene(s, &sr, 1, &sh, &ps->tr)) {
                Lsum = vadd(Lsum, scol);
                Ln = vadd(Ln, scol); /* aov_nee.splat (pathtracer.art:206) */
            }
        }
        if (!alive) break;
    }
    *Ldirect = Ld;
    *Lnee = Ln;
    return Lsum;
}

/* ------------------------------------------------------------------------ */
/* cpu_trace: 16x16 tiles scheduled over threads (driver/mapping_cpu.art:694-836) */
/* ------------------------------------------------------------------------ */
typedef struct {
    const oracle_scene* s;
    const oracle_params* p;
    float* fb;
    int x0, y0, x1, y1, tiles_x, num_tiles;
    atomic_int next;
    pthread_mutex_t lock;
    pstats total;
} job_t;

/* framebuffer.splat of the CPU accumulator (driver/accumulator.art:23-30): fb[pixel] += colour / spi */
static inline void splat(float* fb, int width, int x, int y, v3 c, float inv) {
    size_t o = 3 * ((size_t)y * width + x);
    fb[o] += c.x * inv;
    fb[o + 1] += c.y * inv;
    fb[o + 2] += c.z * inv;
}

/* cpu_trace's loop for one tile (driver/mapping_cpu.art:694-836; the default
 * CPU target: vector width 1, no vector compaction): the tile's spi * 256
 * camera rays form the primary stream (capacity spi * tile_size^2,
 * cpu_get_stream_capacity, so one generation fills it); then, while rays
 * remain: closest hits for the stream (on_traverse_primary), a counting sort
 * by entity with misses last (cpu_sort_primary, :57-97), hit shading entity by
 * entity and miss shading (on_hit_shade / on_miss_shade: emission splats, NEE
 * rays into the secondary stream, bounces), compaction of the surviving rays
 * (cpu_compact_primary, :199-304), and the any-hit secondary stream, whose
 * unoccluded rays splat their colour (:815-828). */
typedef struct {
    opath* q;       /* primary stream */
    opath* q2;      /* sort / compaction target */
    ohit* hit;
    ohit* hit2;
    oray* sray;     /* secondary stream */
    v3* scol;
    int* spix;      /* 2 ints per secondary ray: its pixel */
    int* count;     /* entities + 2 sort bins */
    int cap;
} ostream;

static void stream_tile(const oracle_scene* s, const oracle_params* p, float* fb, int xs, int ys, int xe, int ye, ostream* S,
                        pstats* ps) {
    int width = p->num_rays > 0 ? p->num_rays : p->width;
    const float inv = 1.0f / (float)p->spi;
    const int N = s->desc.num_entities;
    int n = 0;
    for (int y = ys; y < ye; ++y) /* id = pixel * spi + sample (on_generate) */
        for (int x = xs; x < xe; ++x)
            for (int smp = 0; smp < p->spi; ++smp) path_begin(s, p, x, y, smp, x, &S->q[n++], ps);
    int* count = S->count;
    while (n > 0) {
        for (int i = 0; i < n; ++i) trace_scene(s, &S->q[i].ray, 0, &S->hit[i], &ps->tr);
        /* counting sort by entity, misses (entity N) last */
        memset(count, 0, sizeof(int) * (size_t)(N + 2));
        for (int i = 0; i < n; ++i) count[(S->hit[i].ent < 0 ? N : S->hit[i].ent) + 1]++;
        for (int e = 0; e <= N; ++e) count[e + 1] += count[e];
        for (int i = 0; i < n; ++i) {
            const int k = count[S->hit[i].ent < 0 ? N : S->hit[i].ent]++;
            S->q2[k] = S->q[i];
            S->hit2[k] = S->hit[i];
        }
        /* shading in entity order, then misses; survivors compacted in place */
        int alive_n = 0, ns = 0;
        for (int i = 0; i < n; ++i) {
            opath* q = &S->q2[i];
            v3 Lacc;
            int has_shadow;
            const int px = q->x, py = q->y;
            const int alive = path_shade(s, q, &S->hit2[i], &Lacc, &has_shadow, &S->sray[ns], &S->scol[ns], ps);
            splat(fb, width, px, py, Lacc, inv);
            if (p->aov_direct) splat(p->aov_direct, width, px, py, Lacc, inv);
            if (has_shadow) {
                S->spix[2 * ns] = px;
                S->spix[2 * ns + 1] = py;
                ++ns;
            }
            if (alive) S->q[alive_n++] = *q;
        }
        n = alive_n;
        for (int i = 0; i < ns; ++i) {
            ohit sh;
            if (!trace_scene(s, &S->sray[i], 1, &sh, &ps->tr)) {
                splat(fb, width, S->spix[2 * i], S->spix[2 * i + 1], S->scol[i], inv);
                if (p->aov_nee) splat(p->aov_nee, width, S->spix[2 * i], S->spix[2 * i + 1], S->scol[i], inv);
            }
        }
    }
}

static void* worker(void* arg) {
    job_t* j = (job_t*)arg;
    pstats ps;
    memset(&ps, 0, sizeof(ps));
    const int T = 16;
    int width = j->p->num_rays > 0 ? j->p->num_rays : j->p->width;
    float inv = 1.0f / (float)j->p->spi;
    ostream S;
    memset(&S, 0, sizeof(S));
    if (j->p->stream) { /* the thread's streams (ignis_get_primary_stream / _secondary_stream) */
        S.cap = j->p->spi * T * T;
        S.q = (opath*)malloc(sizeof(opath) * S.cap);
        S.q2 = (opath*)malloc(sizeof(opath) * S.cap);
        S.hit = (ohit*)malloc(sizeof(ohit) * S.cap);
        S.hit2 = (ohit*)malloc(sizeof(ohit) * S.cap);
        S.sray = (oray*)malloc(sizeof(oray) * S.cap);
        S.scol = (v3*)malloc(sizeof(v3) * S.cap);
        S.spix = (int*)malloc(sizeof(int) * 2 * S.cap);
        S.count = (int*)malloc(sizeof(int) * (size_t)(j->s->desc.num_entities + 2));
    }
    for (;;) {
        int t = atomic_fetch_add(&j->next, 1);
        if (t >= j->num_tiles) break;
        int tx = t % j->tiles_x, ty = t / j->tiles_x;
        int xs = j->x0 + tx * T, ys = j->y0 + ty * T;
        if (j->p->stream) {
            stream_tile(j->s, j->p, j->fb, xs, ys, xs + T < j->x1 ? xs + T : j->x1, ys + T < j->y1 ? ys + T : j->y1, &S, &ps);
            continue;
        }
        for (int y = ys; y < ys + T && y < j->y1; ++y)
            for (int x = xs; x < xs + T && x < j->x1; ++x) {
                float r = 0, g = 0, b = 0;
                v3 ad = V(0, 0, 0), an = V(0, 0, 0); /* the AOVs' sums, in the same order */
                for (int smp = 0; smp < j->p->spi; ++smp) {
                    if (j->p->probe_sample && smp != j->p->probe_sample - 1) continue; /* per-path probe */
                    v3 Ld, Ln;
                    v3 L = trace_path(j->s, j->p, x, y, smp, x, &ps, &Ld, &Ln);
                    r += L.x * inv;
                    g += L.y * inv;
                    b += L.z * inv;
                    ad = V(ad.x + Ld.x * inv, ad.y + Ld.y * inv, ad.z + Ld.z * inv);
                    an = V(an.x + Ln.x * inv, an.y + Ln.y * inv, an.z + Ln.z * inv);
                }
                size_t o = 3 * ((size_t)y * width + x);
                j->fb[o] += r;
                j->fb[o + 1] += g;
                j->fb[o + 2] += b;
                if (j->p->aov_direct) {
                    j->p->aov_direct[o] += ad.x;
                    j->p->aov_direct[o + 1] += ad.y;
                    j->p->aov_direct[o + 2] += ad.z;
                }
                if (j->p->aov_nee) {
                    j->p->aov_nee[o] += an.x;
                    j->p->aov_nee[o + 1] += an.y;
                    j->p->aov_nee[o + 2] += an.z;
                }
            }
    }
    free(S.q);
    free(S.q2);
    free(S.hit);
    free(S.hit2);
    free(S.sray);
    free(S.scol);
    free(S.spix);
    free(S.count);
    pthread_mutex_lock(&j->lock);
    j->total.camera += ps.camera;
    j->total.bounce += ps.bounce;
    j->total.shadow += ps.shadow;
    j->total.tr.nodes += ps.tr.nodes;
    j->total.tr.leaves += ps.tr.leaves;
    j->total.tr.tris += ps.tr.tris;
    pthread_mutex_unlock(&j->lock);
    return NULL;
}

int oracle_render(const oracle_scene* s, const oracle_params* p, float* fb, oracle_stats* stats) {
    if (!s || !p || !fb || p->spi < 1) return -1;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    job_t j;
    memset(&j, 0, sizeof(j));
    j.s = s;
    j.p = p;
    j.fb = fb;
    int width = p->num_rays > 0 ? p->num_rays : p->width;
    int height = p->num_rays > 0 ? 1 : p->height;
    j.x0 = p->x1 > 0 ? p->x0 : 0;
    j.y0 = p->x1 > 0 ? p->y0 : 0;
    j.x1 = p->x1 > 0 ? p->x1 : width;
    j.y1 = p->x1 > 0 ? p->y1 : height;
    j.tiles_x = (j.x1 - j.x0 + 15) / 16;
    j.num_tiles = j.tiles_x * ((j.y1 - j.y0 + 15) / 16);
    atomic_init(&j.next, 0);
    pthread_mutex_init(&j.lock, NULL);
    int nt = p->threads > 0 ? p->threads : (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nt < 1) nt = 1;
    if (nt > 256) nt = 256;
    pthread_t th[256];
    for (int i = 0; i < nt; ++i) pthread_create(&th[i], NULL, worker, &j);
    for (int i = 0; i < nt; ++i) pthread_join(th[i], NULL);
    pthread_mutex_destroy(&j.lock);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (stats) {
        stats->camera_rays = j.total.camera;
        stats->bounce_rays = j.total.bounce;
        stats->shadow_rays = j.total.shadow;
        stats->node_visits = j.total.tr.nodes;
        stats->leaf_visits = j.total.tr.leaves;
        stats->tri_tests = j.total.tr.tris;
        stats->seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
        stats->threads = nt;
    }
    return 0;
}

void oracle_trace_hits(const oracle_scene* s, const float* rays, int32_t n, uint32_t flags, int32_t* ent_prim, float* tuv) {
    otstats st = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const float* r = rays + 8 * i;
        oray ray = make_ray(V(r[0], r[1], r[2]), V(r[3], r[4], r[5]), r[6], r[7], flags);
        ohit h;
        trace_scene(s, &ray, 0, &h, &st);
        ent_prim[2 * i] = h.ent;
        ent_prim[2 * i + 1] = h.prim;
        tuv[3 * i] = h.t;
        tuv[3 * i + 1] = h.ent >= 0 ? h.u : 0;
        tuv[3 * i + 2] = h.ent >= 0 ? h.v : 0;
    }
}

void oracle_trace_occlusion(const oracle_scene* s, const float* rays, int32_t n, uint32_t flags, int32_t* occluded) {
    otstats st = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const float* r = rays + 8 * i;
        oray ray = make_ray(V(r[0], r[1], r[2]), V(r[3], r[4], r[5]), r[6], r[7], flags);
        ohit h;
        occluded[i] = trace_scene(s, &ray, 1, &h, &st);
    }
}

int oracle_intersect_tri(const float* tri12, const float* ray8, float* tuv) {
    oray r = make_ray(V(ray8[0], ray8[1], ray8[2]), V(ray8[3], ray8[4], ray8[5]), ray8[6], ray8[7], 0);
    return tri_test(&r, tri12, &tuv[0], &tuv[1], &tuv[2]);
}

int oracle_intersect_box(const float* bmin3, const float* bmax3, const float* ray8, float* t) {
    /* intersect_ray_box_single (intersection.art:183-192) */
    oray r = make_ray(V(ray8[0], ray8[1], ray8[2]), V(ray8[3], ray8[4], ray8[5]), ray8[6], ray8[7], 0);
    float en, ex;
    ray_box(&r, bmin3, bmax3, &en, &ex);
    if ((en <= ex) && (ex >= 0)) {
        *t = en < 1e-5f ? ex : en;
        return 1;
    }
    return 0;
}

/* Test hook (TEST INFRASTRUCTURE, tests/golden/cycles_box_model.py): the
 * principled BSDF of material m times the cosine of wi, in the local frame of
 * a front-facing hit (normal +z), for n direction pairs; `model` selects the
 * diffuse lobe (prin_diffuse_model): 0 the reference's, 1 Disney 2015's split
 * on the roughness input, 2 Burley 2012.  out: 3 floats per pair. */
void oracle_principled_eval(const igx_material* m, int n, const float* wo, const float* wi, int model, float* out) {
    osurf sf;
    memset(&sf, 0, sizeof(sf));
    sf.entering = 1;
    const oprin p = oprin_make(m, &sf);
    const int saved = prin_diffuse_model;
    prin_diffuse_model = model;
    for (int k = 0; k < n; ++k) {
        const v3 c = prin_eval_local(&p, V(wo[3 * k], wo[3 * k + 1], wo[3 * k + 2]), V(wi[3 * k], wi[3 * k + 1], wi[3 * k + 2]));
        out[3 * k] = c.x;
        out[3 * k + 1] = c.y;
        out[3 * k + 2] = c.z;
    }
    prin_diffuse_model = saved;
}
