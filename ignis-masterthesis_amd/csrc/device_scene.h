// Device-resident scene and stream layouts (shared by the host's table builder,
// host/scene_tables.cpp, the upload code and the kernels; compiles without HIP).
// See DESIGN.md "HBM layout".  All arrays are 16-byte element aligned so every
// record is fetched with global_load_dwordx4.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef __HIPCC__
struct float4_ { float x, y, z, w; };
#endif

#ifdef __HIPCC__
#define IGX_SCENE_HD __host__ __device__
#else
#define IGX_SCENE_HD
#endif

// Order of the local pixel index: 1 = 4 x 2 pixel blocks where the width (tile
// side) allows, 0 = row-major (local_to_global in igx_device.hip; the host
// counts a chunk's film pixels in the same order, host/render_plan.h)
#ifndef IGX_PIXEL_BLOCKS
#define IGX_PIXEL_BLOCKS 1
#endif

namespace igxd {

// Traversal encodings (see host/bvh_build.h)
constexpr int32_t REF_MARKER = (int32_t)0x80000000; // return from a BLAS to the TLAS
constexpr int32_t REF_EXIT = (int32_t)0x80000001;   // bottom of the traversal stack
constexpr int LEAF_COUNT_BITS = 4;

// Kernel variant V (a template parameter): bit 1 = 4-wide nodes (128-B SoA
// node, host Bvh4Node) instead of BVH2 (64-B Node2, host BvhNode); bit 0 =
// the scene's stack need exceeds the LDS stack, so pushes and pops check for
// the spill area; bit 2 = the scene uses materials or lights beyond the basic
// set (igx_kernels.h, bsdf_eval), compiled into the shading kernels only then.
// build_scene_tables (host/scene_tables.cpp) picks the variant per scene.
#ifndef IGX_LDS_STACK
#define IGX_LDS_STACK 16
#endif
constexpr int LDS_STACK = IGX_LDS_STACK; // LDS traversal-stack entries per lane
constexpr int MAX_STACK = 128;           // traversal stack entries (LDS + spill) per ray
IGX_SCENE_HD constexpr int variant_width(int v) { return (v & 2) ? 4 : 2; }
IGX_SCENE_HD constexpr bool variant_spill(int v) { return (v & 1) != 0; }
IGX_SCENE_HD constexpr bool variant_full(int v) { return (v & 4) != 0; }
IGX_SCENE_HD constexpr int node_f4(int width) { return width == 4 ? 8 : 4; }
// Bit 3: the node tables are staged in LDS (stage_scene_lds; set by the
// kernels on their LDS-staged SceneView).  The node steps then skip the
// stack-top peek (IGX_PEEK_POP), whose extra LDS read costs there what it
// saves where the nodes come from global memory.  (One float4 of padding per
// LDS node, round 2, measured neutral and was removed.)
IGX_SCENE_HD constexpr bool variant_lds_nodes(int v) { return (v & 8) != 0; }
// Bit 4: if-if stepping (trav_step advances one inner node or one leaf per
// call) -- set only on k_shadow_refill launches for scenes on the split
// schedule (igx_device.hip, use_shadow_ifif).
IGX_SCENE_HD constexpr bool variant_ifif(int v) { return (v & 16) != 0; }
// Bit 5: the node tables stay in global memory, but the hottest nodes (the
// first SceneView::tree_n of the node array, order_hot_nodes' hot order)
// are staged in LDS (the treelet); node steps below that index read LDS.
// Set by every kernel instantiation that does not stage the whole table.
constexpr int VARIANT_TREE = 32;
// Bit 7: quantised 4-wide nodes (64 B, node_step4q; host Bvh4QNode) instead of
// the 128-B 4-wide nodes -- half the node bytes per visit on scenes whose
// tables stay in global memory.  Set by the upload with bit 1 (option
// "bvh_quantize").
constexpr int VARIANT_Q4 = 128;
IGX_SCENE_HD constexpr bool variant_q4(int v) { return (v & VARIANT_Q4) != 0; }
constexpr int32_t REF_EMPTY = (int32_t)0x80000002; // absent child of a 4-wide node (host kEmptyRef)
IGX_SCENE_HD constexpr bool variant_tree(int v) { return (v & VARIANT_TREE) != 0; }
IGX_SCENE_HD constexpr int kernel_variant(int v, bool lds) { return lds ? (v | 8) : (v | VARIANT_TREE); }

// Instance record (one per TLAS leaf slot): 64 B
//   row0..row2: to_local 3x4 (row-major, xyz = linear row, w = translation)
//   info: x = entity id, y = shape type (0 trimesh, 1 sphere), z = BLAS root node
//         index (trimesh) or sphere index (sphere), w = visibility flags
// The reference's EntityLeaf1 (traversal/bvh.art:52-61) carries the same data
// plus the entity box, which here lives in the parent TLAS node.
// Flag in info.w, next to the visibility bits: the trimesh instance's to_local
// is the identity, so its entity-space ray is the world ray (instance_test
// skips the transform; set by build_scene_tables)
constexpr uint32_t INST_IDENTITY = 1u << 30;
// ... or a pure translation (rows (1 0 0 tx), (0 1 0 ty), (0 0 1 tz)): the
// entity-space ray is (o + t, d), so its reciprocal direction is the world
// ray's (IGX_TRANSLATE_INSTANCES)
constexpr uint32_t INST_TRANSLATE = 1u << 29;

// Per-entity shading record: 3 rows of to_global, 3 rows of normal matrix,
// info (shape, material, vtx_offset, idx_offset) -> 7 x 16 B.
constexpr int ENT_STRIDE = 7;

enum : int32_t { MAT_DIFFUSE = 0, MAT_DIELECTRIC = 1, MAT_CONDUCTOR = 2, MAT_PLASTIC = 3, MAT_PRINCIPLED = 4,
                 MAT_TENSORTREE = 5, MAT_KLEMS = 6 };
// microfacet distribution of conductor / plastic specular lobes
// (BSDF::setupRoughness, src/runtime/bsdf/BSDF.cpp:53-99)
enum : int32_t { MF_DELTA = 0, MF_VNDF_GGX = 1, MF_GGX = 2, MF_BECKMANN = 3 };
struct DevMaterial {   // 128 B
    int32_t type, light, dist, mirror; // mirror: delta conductor with eta = 0, k = 1 (make_mirror_bsdf);
                                       // dielectric: thin interface; principled: flag bits
    float kd[4];        // diffuse reflectance; w = Oren-Nayar roughness (0: Lambert)
    float ks[4];        // specular reflectance; w = n1 (ext ior)
    float kt[4];        // specular transmittance; w = n2 (int ior)
    float eta[4];       // conductor eta; w = alpha_u
    float kappa[4];     // conductor k; w = alpha_v
    float pad[8];       // textured diffuse (igx_material::texture): pad[0] = texture (int bits),
                        // pad[1] = scale, pad[2..4] = the colour where the checker is 1 (kd elsewhere)
                        // image texture (IGX_TEXTURE_IMAGE, also on a principled base_color): pad[1..6] =
                        // the 2x3 uv transform, pad[7] = its TexRecord's place in the uv table (uint bits)
    // Measured BSDFs (MAT_TENSORTREE, MAT_KLEMS; components k = 0..3: front reflection, front
    // transmission, back reflection, back transmission, igx_measured):
    //   dist = ndim (tensor tree); mirror = bit k: component k has data (total > 0), bit 4 + k: its root is a leaf
    //   kd = base colour, kd[3] = front_refl_prob; ks = up, ks[3] = back_refl_prob
    //   kt[k]    (uint bits) first word of component k, in 32-bit words from the start of the uv table
    //   eta[k]   (uint bits) tensor tree: node count; Klems: row thetas | column thetas << 16
    //   kappa[k] (uint bits) tensor tree: max depth; Klems: column patches
    //   pad[0] = 0 (no texture); pad[6..7] = the uv table's address, written into the
    //   shaded copy of the material on the device (bind_measured)
};

enum : int32_t { LIGHT_PLANE = 1, LIGHT_ENV = 2, LIGHT_POINT = 3, LIGHT_SPOT = 4, LIGHT_DIRECTIONAL = 5, LIGHT_SUN = 6,
                   LIGHT_SPHERE = 7, LIGHT_MESH = 8, LIGHT_CIE = 9, LIGHT_ENVMAP = 10 };
// A CIE sky (LIGHT_CIE, host/cie_sky.h) keeps its CieSky record in the 28
// floats from `radiance` on (cie_sky_of); `entity` is unused.  An image
// environment map (LIGHT_ENVMAP, host/image_texture.h) keeps its EnvMap there.
struct DevLight {      // 128 B
    int32_t type, infinite, delta, entity; // entity: emitting entity of sphere / mesh area lights
    float radiance[4];
    float origin[4];   // plane origin / point/spot position; w = plane width; sphere: object-space centre, radius
    float ex[4];       // plane x axis normalised; w = plane height
    float ey[4];       // plane y axis normalised; w = inv_area
    float normal[4];   // plane normal / spot direction; w = area
    float spot[4];     // spot: cos_cutoff, cos_falloff, blend range; sun: cos_angle, sun_area;
                       // sphere: emitter area (compute_ellipsoid_area); mesh: face count
    float pad2[4];
};

// Enclosing entities (trace_enclosed): a path's slot word carries 1 + the
// index of the enclosing entity it is in in its top 5 bits, so at most 31 of
// them; their world boxes are staged in LDS (stage_enc_boxes)
constexpr int MAX_ENCLOSING = 31;
constexpr int MAX_ENC_BOXES = 32;
static_assert(MAX_ENCLOSING <= MAX_ENC_BOXES, "enclosing boxes are staged in LDS (stage_enc_boxes)");

// Limits and thresholds of the table build (host/scene_tables.cpp).
// BLAS with more triangles build without spatial splits (load time; their
// triangles are small next to the scene in the suite's soups)
constexpr uint32_t SPATIAL_SPLIT_MAX_FACES = 1u << 21;
// face instances (faces x entities using them) up to which the upload
// precomputes world-space face normals (16 B each: at most 64 MB)
constexpr size_t FACE_NORMAL_TABLE_MAX = 4u << 20;
// mesh faces (over all shapes) up to which the upload writes the per-face
// shading records SceneView::fsh (48 B each: at most 192 MB)
constexpr size_t FACE_SHADE_MAX = 4u << 20;
// nodes moved to the front of the node array in hot order at upload (the
// largest treelet a kernel may stage: 160 KB of LDS / 128-B nodes)
constexpr size_t TREELET_FRONT = 1280;
// traversal tables beyond this go to the split schedule (use_split in
// igx_device.hip, "Kernel schedule per scene"), and 4-wide nodes of scenes
// estimated beyond it are quantised (build_scene_tables)
constexpr size_t SPLIT_TABLE_BYTES = 64u << 20;

} // namespace igxd

// DevCamera and the camera models' ray arithmetic (shared with the host)
#include "../host/camera_model.h"
