// The flat scene tables of the device (host side, no HIP): igx_upload_scene
// builds them from an igx_scene_desc with build_scene_tables and copies each
// vector to the device as it is (csrc/igx_device.hip; layouts in
// csrc/device_scene.h and DESIGN.md "HBM layout").  The builder validates
// every index the caller passed, picks the node width, the quantisation and
// the shading variant, and allocates nothing on the device: a scene it
// refuses costs no device memory.
#pragma once

#include "igx.h"

#include "bvh_build.h"
#include "device_scene.h"
#include "image_texture.h"
#include "light_select.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace igx {

// Table elements: the device's float4 / int4 / float2 / int2 (same size and
// alignment, pinned by static_asserts next to the driver's upload)
struct alignas(16) Float4 { float x, y, z, w; };
struct alignas(16) Int4 { int32_t x, y, z, w; };
struct alignas(8) Float2 { float x, y; };
struct alignas(8) Int2 { int32_t x, y; };

// The handle's options that the build reads (igx_set_option)
struct SceneBuildOptions {
    bool rebuild_bvh = false;      // ignore a shape's reference BLAS (igx_shape::ref_bvh)
    bool spatial_splits = false;   // SBVH for BLAS up to SPATIAL_SPLIT_MAX_FACES triangles
    int leaf_size = 4;
    int bvh_bins = 32, bvh_bins_tlas = 32;
    float sah_node_cost = 1.0f;
    int bvh_width_opt = 0;         // 0: auto, 2, 4
    int quantize_opt = -1;         // -1: auto, 0, 1
    bool face_shade_opt = true;    // per-face shading records (fsh)
    bool face_normals_opt = true;  // world-space face normals (fn_tab)
    bool enclosing_opt = true;     // enclosing entities (ent_enc, enc_tab, enc_box)
    bool full_shading_opt = false; // force the full shading variant
    size_t treelet_front = igxd::TREELET_FRONT; // nodes moved to the front in hot order
};

// One vector per device table, and the scalars the driver copies into
// SceneView and the handle
struct SceneTables {
    std::vector<Float4> nodes;   // nf4 per node: every BLAS, then the TLAS, in hot order
    std::vector<Float4> tris;    // Tri1: 3 per triangle slot
    std::vector<Float4> inst;    // 4 per TLAS leaf slot
    std::vector<Float4> spheres; // origin.xyz, radius
    std::vector<Float4> ent;     // ENT_STRIDE per entity
    std::vector<Float4> vtx, nrm; // mesh vertices and vertex normals (object space)
    std::vector<Int4> idx;       // faces: local vertex indices
    std::vector<Float2> uvs;     // texture coordinates, only for scenes with a textured material; behind
                                 // them the image textures' records and texels (igxd::TexRecord), the
                                 // environment maps' sampling tables and the measured BSDFs' words
    std::vector<Float4> fsh;     // per face: vertex normals and indices in one record (SceneView::fsh)
    std::vector<Float4> fn_tab;  // world-space unit face normals (surface_element)
    std::vector<int32_t> ent_fn; // per entity: first face-normal entry, -1 without a table
    std::vector<int32_t> ent_enc; // per entity: enclosing index or -1
    std::vector<Int2> enc_tab;   // per enclosing index: entity, TLAS leaf slot
    std::vector<Float4> enc_box; // per enclosing index: world box lo, hi
    std::vector<igxd::DevMaterial> mats;
    std::vector<igxd::DevLight> lights; // infinite lights first
    LightSelectTables lsel;      // NEE selector tables over the finite lights, in device order

    int tlas_root = -1;          // root node of the TLAS, or its only leaf (one entity)
    int width = 2;               // node width: 2 or 4
    bool quantized = false;      // 4-wide nodes quantised to 64 B (Bvh4QNode)
    int nf4 = 4;                 // Float4s per node
    int num_infinite = 0;
    float scene_radius = 0;      // bbox_radius(scene_bbox) * 1.01
    int tlas_depth = 0, blas_depth = 0; // stack entries the TLAS / the deepest BLAS can occupy
    int scene_depth = 0;         // traversal stack entries a ray can need
    bool full_shading = false;   // the scene needs the full shading variant (variant bit 2)
    bool aov_on = false;         // technique aov_mis
    bool textured = false;       // a material carries a texture
    size_t image_bytes = 0;      // texels of the image textures in uvs
    size_t cdf_bytes = 0;        // sampling tables of the image environment maps in uvs
    size_t measured_bytes = 0;   // words of the measured BSDFs in uvs
};

// Build every table of `desc`.  On failure the status and `error` are what
// igx_upload_scene reports; `out` is then unspecified.
igx_status build_scene_tables(const igx_scene_desc& desc, const SceneBuildOptions& opt, SceneTables& out, std::string& error);

// Hot order of the node array for the LDS treelet (stage_treelet): the
// `front` inner nodes a ray most likely visits move to indices [0, front), so
// a kernel stages any prefix of the array as its treelet.  Visit likelihood
// follows the surface-area heuristic: the TLAS root has 1; a child has its
// parent's times the child box's area over the union of the sibling boxes
// (the chance a ray through the parent also crosses the child); a BLAS root
// collects the likelihood of every TLAS leaf that instances it.  The other
// nodes keep their relative (depth-first) order.  Every inner-node reference
// (node children, instance BLAS roots, the TLAS root) is renumbered; the
// traversal result does not depend on node numbering.
// `format`: 2 (BVH2, 64 B), 4 (4-wide, 128 B) or 5 (quantised 4-wide, 64 B).
void order_hot_nodes(std::vector<Float4>& nodes, int format, std::vector<Float4>& inst, int& tlas_root, size_t front);

// A closed triangle mesh: with vertices welded by position, every edge
// borders exactly two faces (paths that enter it by transmission then hit it
// again before leaving).  Checked up to 1 M faces.
bool closed_mesh(const igx_mesh& m);

} // namespace igx
