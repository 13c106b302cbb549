/*
 * igx_scene.h — scene description handed across the drop-in boundary.
 *
 * This is the data the reference's loader hands to its device through
 * `IG::SceneSettings` (src/runtime/device/Device.h:25-30), restated as plain C
 * structs.  The reference passes a `SceneDatabase*` whose tables are produced by
 * `TriMeshProvider::handle` (src/runtime/shape/TriMeshProvider.cpp:480-617),
 * `SphereProvider::handle` (src/runtime/shape/SphereProvider.cpp:10-53),
 * `LoaderEntity::load` (src/runtime/loader/LoaderEntity.cpp:32-205) and the
 * light/BSDF serialisers.  The reference turns materials and lights into JIT
 * code; here they are data (material and light tables), because there is no
 * Artic JIT in this build (SURVEY.md §7 "hard parts").
 *
 * All pointers inside an igx_scene_desc are owned by the igx_scene handle that
 * produced them (igx_scene_load_*); igx_upload_scene copies what it needs.
 */
#ifndef IGX_SCENE_H
#define IGX_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shapes ------------------------------------------------------------ */
enum { IGX_SHAPE_TRIMESH = 0, IGX_SHAPE_SPHERE = 1 };

/* Object-space triangle mesh after the shape's own transform and flip_normals
 * were baked in (TriMeshProvider.cpp:529-541).  Indices are 3 per face. */
typedef struct igx_mesh {
    uint32_t num_vertices;
    uint32_t num_faces;
    const float* vertices;   /* 3 * num_vertices */
    const float* normals;    /* 3 * num_vertices (unit) */
    const float* texcoords;  /* 2 * num_vertices */
    const uint32_t* indices; /* 3 * num_faces */
} igx_mesh;

typedef struct igx_shape {
    int32_t type;        /* IGX_SHAPE_* */
    int32_t mesh;        /* index into meshes for TRIMESH, -1 otherwise */
    float sphere[4];     /* origin.xyz, radius for SPHERE */
    float bbox_min[3];   /* local bbox, inflated by 1e-5 (TriMeshProvider.cpp:537-538) */
    float bbox_max[3];
    /* plane representation (TriMesh::getAsPlane, mesh/TriMesh.cpp:520-634) */
    int32_t is_plane;
    float plane_origin[3], plane_x[3], plane_y[3];
    float plane_tex[8];  /* 4 texcoords */
    /* Optional prebuilt BLAS in the reference's GPU layout: one
     * FixTables["trimesh_primbvh"] entry (TriMeshProvider.cpp:307-326, 361-369):
     * u32 node_count, tri_count, 0, 0; Node2[node_count] (64 B,
     * traversal/mapping_gpu.art:3-7; child > 0 inner index + 1, < 0 ~first Tri1,
     * 0 empty); Tri1[tri_count] (48 B, shapes/trimesh.art:107-114; prim_id bit 31
     * ends a leaf).  NULL: igx builds the BLAS itself (host/bvh_build.cpp). */
    const uint8_t* ref_bvh;
    uint64_t ref_bvh_bytes;
} igx_shape;

/* ---- entities ---------------------------------------------------------- */
/* Matrices are 3x4 row-major: m[r*4+c].  normal is 3x3 row-major.  The
 * reference stores the same three matrices per entity, 36 floats
 * (LoaderEntity.cpp:150-162), column-major. */
typedef struct igx_entity {
    int32_t shape;
    int32_t material;
    uint32_t flags;         /* visibility flags 0x1 camera 0x2 light 0x4 bounce 0x8 shadow */
    float to_global[12];
    float to_local[12];
    float normal[9];        /* inverse-transpose of the linear part of to_global */
    float bbox_min[3];      /* world-space bbox = local bbox transformed (LoaderEntity.cpp:141) */
    float bbox_max[3];
} igx_entity;

/* ---- materials --------------------------------------------------------- */
enum {
    IGX_BSDF_DIFFUSE    = 0, /* Lambert / Oren-Nayar (bsdf/diffuse.art) */
    IGX_BSDF_DIELECTRIC = 1, /* pure (smooth) dielectric (bsdf/dielectric.art) */
    IGX_BSDF_CONDUCTOR  = 2, /* mirror / pure / rough conductor (bsdf/conductor.art) */
    IGX_BSDF_PLASTIC    = 3, /* Fresnel mix of diffuse and a conductor lobe (bsdf/plastic.art) */
    IGX_BSDF_PRINCIPLED = 4, /* Disney BSDF (bsdf/principled.art) */
    IGX_BSDF_TENSORTREE = 5, /* measured tensor tree BSDF of a fenestration (bsdf/tensortree.art) */
    IGX_BSDF_KLEMS      = 6  /* measured Klems matrix BSDF of a fenestration (bsdf/klems.art) */
};
/* microfacet distribution of conductor / plastic lobes (BSDF::setupRoughness, BSDF.cpp:53-99) */
enum { IGX_MICROFACET_DELTA = 0, IGX_MICROFACET_VNDF_GGX = 1, IGX_MICROFACET_GGX = 2, IGX_MICROFACET_BECKMANN = 3 };

typedef struct igx_material {
    int32_t bsdf_type;     /* IGX_BSDF_* */
    int32_t light;         /* index of the area light emitting from this material, -1 if none */
    int32_t thin;          /* dielectric: thin interface */
    int32_t distribution;  /* IGX_MICROFACET_* (conductor, plastic) */
    float kd[3];           /* diffuse reflectance */
    float ks[3];           /* specular reflectance */
    float kt[3];           /* specular transmittance */
    float ext_ior, int_ior;
    float eta[3];          /* conductor complex ior: real part */
    float kappa[3];        /* conductor complex ior: imaginary part */
    float alpha_u, alpha_v;/* microfacet roughness (compute_explicit, core/microfacet.art:395-402) */
    float diffuse_alpha;   /* Oren-Nayar roughness, 0 = Lambert */
    float pad;
    /* principled (PrincipledBSDF.cpp:11-60): kd = base_color, alpha_u / alpha_v =
     * roughness_u / roughness_v (already through compute_roughness), thin */
    float ior, diffuse_transmission, specular_transmission, specular_tint, flatness, metallic;
    float sheen, sheen_tint, clearcoat, clearcoat_gloss, clearcoat_roughness;
    int32_t clearcoat_top_only;
    /* diffuse reflectance given by a shading expression the loader recognises
     * (ShadingTree / PExpr): IGX_TEXTURE_CHECKER is
     * select(checkerboard(uvw * tex_scale) == 1, tex_kd1, kd), the 3D
     * checkerboard of texture/checkerboard.art:2 on the surface's texture
     * coordinates (u, v, 0) (shapes/trimesh.art:25); IGX_TEXTURE_NONE: kd */
    int32_t texture;
    float tex_scale;
    float tex_kd1[3];
    /* IGX_TEXTURE_IMAGE: kd (diffuse reflectance, principled base_color) is the
     * image texture `tex_index` of igx_scene_desc::textures at the surface's
     * texture coordinates; -1 (or 0 with another `texture`) otherwise */
    int32_t tex_index;
    /* IGX_BSDF_TENSORTREE / IGX_BSDF_KLEMS (TensorTreeBSDF.cpp, KlemsBSDF.cpp): kd =
     * base_color (default 1), `measured` the index into igx_scene_desc::measured,
     * `up` the unit up vector of the window's own frame (default +Z); the frame is
     * tt_transform_matrix(unflipped normal, up), the identity where up is
     * parallel to the normal (bsdf/tensortree.art:169-177).  Unused otherwise. */
    int32_t measured;
    float up[3];
} igx_material;

enum { IGX_TEXTURE_NONE = 0, IGX_TEXTURE_CHECKER = 1, IGX_TEXTURE_IMAGE = 2 };

/* ---- images and image textures ------------------------------------------ */
/* A decoded image with the reference's semantics (Image.cpp): row 0 is the
 * file's bottom row.  RGBA8 and MONO8 are its "packed" 8-bit images
 * (Image::loadPacked: colour bytes already through byte_color_to_linear unless
 * the texture says `linear`; R in the low byte of each 32-bit texel), unpacked
 * on the device by / 255 (driver/image.art:9-16); FLOAT4 is a float RGBA image
 * (EXR, HDR). */
enum { IGX_IMAGE_RGBA8 = 0, IGX_IMAGE_MONO8 = 1, IGX_IMAGE_FLOAT4 = 2 };
typedef struct igx_image {
    int32_t width, height;
    int32_t format;        /* IGX_IMAGE_* */
    const void* pixels;    /* width * height texels of 4, 1 or 16 bytes */
} igx_image;

/* The "image" texture (pattern/ImagePattern.cpp:19-52; texture/image.art) */
enum { IGX_FILTER_NEAREST = 0, IGX_FILTER_BILINEAR = 1, IGX_FILTER_BICUBIC = 2 };
enum { IGX_WRAP_REPEAT = 0, IGX_WRAP_CLAMP = 1, IGX_WRAP_MIRROR = 2 };
typedef struct igx_texture {
    int32_t image;         /* index into igx_scene_desc::images */
    int32_t filter;        /* IGX_FILTER_*, "filter_type", default bicubic */
    int32_t wrap_u, wrap_v;/* IGX_WRAP_*, "wrap_mode" or "wrap_mode_u" / "wrap_mode_v", default repeat */
    float transform[6];    /* 2x3 row-major: uv' = transform * (u, v, 1) (LoaderUtils::inlineTransformAs2d) */
} igx_texture;

/* ---- measured fenestration BSDFs ------------------------------------------ */
/* One Radiance BSDF XML file after the reference's loaders
 * (measured/TensorTreeLoader.cpp, measured/KlemsLoader.cpp): four components in
 * the order below, after the loaders' front / back renaming, and one array of
 * 32-bit words they point into.  Two components may share their words (the
 * transmission of a file that gives only one side).  The word layout is igx's
 * own:
 *  - tensor tree component at `offset`: node_count int32 node values, then
 *    value_count floats.  Nodes come in groups of 2^ndim child slots, the
 *    root's group first, every child group behind its parent's
 *    (TensorTreeComponent::addNode).  A node value >= 0 is the index of the
 *    child's group (a multiple of 2^ndim); a value < 0 names the leaf whose
 *    values start at -(value + 1).  A leaf is one value with the sign bit set
 *    (its magnitude counts) or 2^ndim values.  root_is_leaf: no nodes, the leaf
 *    at value 0.  max_depth: the most node groups a lookup passes (0 for a
 *    root leaf), at most 16.
 *  - Klems component at `offset`: the row (outgoing) basis as theta_count[0]
 *    records (float centre, lower, upper theta in radians, uint32 phi count),
 *    ascending in upper theta, then theta_count[0] uint32 first-patch numbers;
 *    the column (incoming) basis likewise with theta_count[1]; then the
 *    matrix, entry_count[0] x entry_count[1] floats, row-major.  A component
 *    without data has all four counts 0 and total 0.
 * `total` steers only the choice between reflection and transmission when
 * sampling (TensorTreeNode::computeTotal, KlemsComponent::computeTotal); a
 * component with total <= 0 is never evaluated. */
enum { IGX_MEASURED_TENSORTREE = 0, IGX_MEASURED_KLEMS = 1 };
enum {
    IGX_MEASURED_FRONT_REFLECTION = 0, IGX_MEASURED_FRONT_TRANSMISSION = 1, IGX_MEASURED_BACK_REFLECTION = 2,
    IGX_MEASURED_BACK_TRANSMISSION = 3
};
typedef struct igx_measured_component {
    float total;
    uint32_t offset;         /* first word of the component in igx_measured::words */
    /* tensor tree (zero for Klems) */
    int32_t ndim;            /* 3 or 4, the same in all four components */
    uint32_t node_count, value_count;
    int32_t root_is_leaf;
    int32_t max_depth;
    /* Klems (zero for a tensor tree): [0] rows = outgoing, [1] columns = incoming */
    uint32_t theta_count[2];
    uint32_t entry_count[2];
} igx_measured_component;
typedef struct igx_measured {
    int32_t kind;            /* IGX_MEASURED_* */
    igx_measured_component component[4]; /* IGX_MEASURED_FRONT_REFLECTION ... */
    uint32_t num_words;
    const uint32_t* words;
} igx_measured;

/* ---- lights ------------------------------------------------------------ */
enum {
    IGX_LIGHT_PLANE = 1, /* area light on a planar entity: make_plane_area_emitter (light/area.art:107-240) */
    IGX_LIGHT_ENV   = 2, /* constant environment, spherical sampling (light/env.art:73-98) */
    IGX_LIGHT_POINT = 3, /* light/point.art:1-18 */
    IGX_LIGHT_SPOT  = 4, /* light/spot.art:8-60 */
    IGX_LIGHT_DIRECTIONAL = 5, /* light/directional.art:1-19 */
    IGX_LIGHT_SUN   = 6, /* light/sun.art:4-30 (delta, infinite) */
    IGX_LIGHT_SPHERE = 7, /* area light on a (near-)spherical entity: make_sphere_area_emitter (light/area.art:240-293) */
    IGX_LIGHT_MESH  = 8, /* area light on any triangle entity: make_shape_area_emitter (light/area.art:45-105) */
    IGX_LIGHT_CIE   = 9, /* analytic CIE sky: make_cie_sky_light / make_cie_sunny_light (light/cie.art:9-42) */
    IGX_LIGHT_ENVMAP = 10 /* image environment map: make_environment_light_textured, or make_environment_light
                             without a CDF (light/env.art:112-164) */
};
/* igx_light.sky_kind (CIELight.h CIEType; LoaderLight.cpp:90-97) */
enum { IGX_SKY_UNIFORM = 0, IGX_SKY_CLOUDY = 1, IGX_SKY_CLEAR = 2, IGX_SKY_INTERMEDIATE = 3 };

typedef struct igx_light {
    int32_t type;
    int32_t entity;        /* area lights: emitting entity, -1 otherwise */
    float radiance[3];     /* radiance (area/env), intensity (point/spot), irradiance (directional/sun) */
    float origin[3];       /* plane origin / point position / spot position / sphere centre (object space) */
    float x_axis[3];       /* plane */
    float y_axis[3];       /* plane */
    float normal[3];       /* plane normal, spot / directional / sun propagation direction */
    float area;            /* plane area; sphere: emitter area, compute_ellipsoid_area (shapes/sphere.art:21-27) */
    float cutoff, falloff; /* spot, radians; sun: cutoff = cosine of the sun's half angle */
    float radius;          /* sphere: object-space radius */
    /* what the non-uniform light selectors know of a finite light
     * (Light::position / direction / computeFlux, light/Light.h:22-23;
     * AreaLight.cpp:46-112, PointLight.cpp:12-30, SpotLight.cpp:12-38) */
    float select_position[3];
    float select_direction[3];
    int32_t select_has_direction;
    float select_flux;     /* mean of the light's power colour */
    /* IGX_LIGHT_CIE (CIELight.cpp:42-110); zero for every other type.  The sky
     * is Y-up in its own frame: L(d) is evaluated at sky_transform * d
     * (has_ground: the whole sphere, sampled uniformly; otherwise the upper
     * hemisphere only, cosine-sampled, light/env.art:25-108) */
    int32_t sky_kind;      /* IGX_SKY_* */
    int32_t has_ground;
    float sky_zenith[3], sky_ground[3], sky_scale[3]; /* scale: clear / intermediate only */
    float ground_brightness;
    float sun_direction[3];/* towards the sun, Y-up (ElevationAzimuth::toDirectionYUp) */
    float zenith_ratio;    /* zenith brightness / factor (clear / intermediate) */
    float sky_c2;          /* ground term of the clear / intermediate sky */
    float sky_transform[9];/* transform.linear().transpose().inverse(), row-major */
    /* IGX_LIGHT_ENVMAP (EnvironmentLight.cpp:10-74); zero for every other type.
     * The radiance in direction d is env_scale * texture(map_env_uv(sky_transform * d)),
     * the map Y-up in its own frame.  With env_cdf (property "cdf", default true)
     * and an image larger than 1 x 1 the light is sampled through a 2-D CDF built at
     * upload on a bake of the texture ("compensate", default true: MIS
     * compensation); otherwise uniformly over the sphere.  Both the sampled and
     * the seen radiance carry env_scale ("Image textures"). */
    int32_t env_texture;   /* index into igx_scene_desc::textures */
    float env_scale[3];
    int32_t env_cdf, env_compensate;
} igx_light;

/* ---- camera / technique ------------------------------------------------ */
enum {
    IGX_CAMERA_PERSPECTIVE = 0, /* camera/perspective.art:29-42; with aperture_radius > FLT_EPSILON the
                                   depth-of-field camera (:74-120) */
    IGX_CAMERA_ORTHOGONAL  = 1, /* camera/orthogonal.art:14-46 */
    IGX_CAMERA_FISHLENS    = 2  /* camera/fishlens.art:8-68, circular aspect mode (FishLensCamera.cpp:9) */
};
typedef struct igx_camera {
    float eye[3], dir[3], up[3];
    float fov;             /* radians */
    int32_t vertical_fov;  /* 1: fov is vertical (compute_scale_from_vfov) */
    float aspect;          /* <= 0: use film width / height */
    float near_clip, far_clip;
    /* the fields below are zero for the pinhole perspective camera */
    int32_t type;          /* IGX_CAMERA_* */
    float ortho_scale;     /* orthogonal: half width of the view in world units (scale; height = scale / aspect) */
    float aperture_radius; /* perspective: lens radius, > FLT_EPSILON selects depth of field */
    float focal_length;    /* perspective with depth of field: distance of the plane in focus */
} igx_camera;

/* light selection for next-event estimation (LoaderLight::generateLightSelector,
 * LoaderLight.cpp:423-453; light/light_selector.art) */
enum { IGX_SELECT_UNIFORM = 0, IGX_SELECT_SIMPLE = 1, IGX_SELECT_HIERARCHY = 2 };

typedef struct igx_technique {
    int32_t max_depth;     /* PathTechnique.cpp:11, default 64 */
    int32_t min_depth;     /* default 2 */
    float clamp;           /* <= 0: no clamping */
    int32_t nee;           /* next-event estimation on */
    int32_t light_selector;/* IGX_SELECT_*: "uniform" (default), "simple" (flux CDF), "hierarchy" (light BVH) */
    int32_t aov_mis;       /* PathTechnique.cpp:16: the "Direct Weights" / "NEE Weights" AOVs (igx_get_aov) */
} igx_technique;

typedef struct igx_scene_desc {
    int32_t film_width, film_height;
    igx_camera camera;
    igx_technique technique;
    uint32_t num_meshes;    const igx_mesh* meshes;
    uint32_t num_shapes;    const igx_shape* shapes;
    uint32_t num_entities;  const igx_entity* entities;
    uint32_t num_materials; const igx_material* materials;
    uint32_t num_lights;    const igx_light* lights;
    float scene_bbox_min[3], scene_bbox_max[3];
    uint32_t num_images;    const igx_image* images;
    uint32_t num_textures;  const igx_texture* textures;
    uint32_t num_measured;  const igx_measured* measured; /* igx_material::measured */
} igx_scene_desc;

/* ---- loader C-ABI (stand-in for the reference's Loader, src/runtime/loader) */
typedef struct igx_scene igx_scene;

/* Load a scene JSON file (Ignis schema subset).  Relative mesh paths resolve
 * against the directory of `path`.  Returns NULL and fills err (if given) on
 * failure.  Mirrors SceneParser::loadFromFile + Loader::load
 * (src/runtime/Runtime.cpp:143-163, 202-290). */
igx_scene* igx_scene_load_file(const char* path, char* err, size_t err_len);
/* Same, from a JSON string; `base_dir` resolves external files (may be NULL). */
igx_scene* igx_scene_load_string(const char* json, const char* base_dir, char* err, size_t err_len);
const igx_scene_desc* igx_scene_get_desc(const igx_scene* scene);
void igx_scene_free(igx_scene* scene);
/* Names of a scene from igx_scene_load_*, for bindings that re-index its
 * shading tables by the reference loader's ids: the
 * material id of (BSDF name, emissive entity name or NULL/"" for a shared
 * material, LoaderContext::Material, LoaderContext.h:19-27), -1 if absent;
 * the name of entity `entity`, NULL if out of range (or for scenes built by
 * igx_scene_from_database, which carry no names). */
int32_t igx_scene_find_material(const igx_scene* scene, const char* bsdf, const char* emissive_entity);
const char* igx_scene_entity_name(const igx_scene* scene, uint32_t entity);

/* ---- in-memory scenes: the reference's IG::Scene object model ------------
 * Runtime::loadFromString / loadFromScene parse (or receive) an IG::Scene and
 * call load({}, scene) without a file (Runtime.cpp:164-199).  A binding that
 * holds such a `const Scene*` (Scene.h: technique, camera, film and named
 * textures / bsdfs / shapes / lights / media / entities, each a SceneObject
 * with a plugin type and SceneProperty values, SceneObject.h, SceneProperty.h)
 * rebuilds it here object by object and property by property, and
 * igx_scene_from_objects reads it with the same semantics as the JSON loader
 * -- no file and no second parse.  An in-memory JSON string goes through
 * igx_scene_load_string. */
typedef struct igx_objscene igx_objscene;
/* SceneObject::Type (SceneObject.h:10-22) */
enum {
    IGX_OBJ_BSDF = 0, IGX_OBJ_CAMERA = 1, IGX_OBJ_ENTITY = 2, IGX_OBJ_FILM = 3, IGX_OBJ_LIGHT = 4, IGX_OBJ_MEDIUM = 5,
    IGX_OBJ_SHAPE = 6, IGX_OBJ_TECHNIQUE = 7, IGX_OBJ_TEXTURE = 8, IGX_OBJ_PARAMETER = 9
};
/* SceneProperty::Type (SceneProperty.h:17-28) and the data each takes:
 * BOOL, INTEGER: int32_t[1]; NUMBER: float[1]; STRING: a NUL-terminated char*;
 * TRANSFORM: float[16], row-major 4x4 (Eigen's Transformf::matrix() is
 * column-major: transpose it); VECTOR2 float[2]; VECTOR3 float[3];
 * INTEGER_ARRAY int32_t[count]; NUMBER_ARRAY float[count] */
enum {
    IGX_PROP_BOOL = 1, IGX_PROP_INTEGER = 2, IGX_PROP_NUMBER = 3, IGX_PROP_STRING = 4, IGX_PROP_TRANSFORM = 5,
    IGX_PROP_VECTOR2 = 6, IGX_PROP_VECTOR3 = 7, IGX_PROP_INTEGER_ARRAY = 8, IGX_PROP_NUMBER_ARRAY = 9
};
/* `base_dir` resolves relative file names (mesh files) of objects added
 * without their own directory (SceneObject::baseDir); may be NULL. */
igx_objscene* igx_objscene_create(const char* base_dir);
void igx_objscene_free(igx_objscene* scene);
/* Add an object (Scene::addBSDF / setCamera / ...): a named object replaces
 * one of the same type and name; camera, film and technique ignore `name` and
 * replace the previous one.  `base_dir` may be NULL.  Returns the object's
 * handle (>= 0) or -1 for an unknown type. */
int32_t igx_objscene_add(igx_objscene* scene, int32_t object_type, const char* plugin_type, const char* name,
                         const char* base_dir);
/* SceneObject::setProperty: 0 on success, -1 for a bad handle, type or data. */
int32_t igx_objscene_set_property(igx_objscene* scene, int32_t object, const char* key, int32_t property_type,
                                  const void* data, uint64_t count);
/* Load the object scene like igx_scene_load_string loads a JSON scene.
 * Returns NULL and fills err on unsupported or malformed objects. */
igx_scene* igx_scene_from_objects(const igx_objscene* scene, char* err, size_t err_len);

/* ---- the reference's SceneDatabase as plain C (Device::assignScene seam) --
 * IG::Runtime hands its device a `SceneDatabase*` (Runtime.cpp:477-485,
 * Device.h:25-30; table/SceneDatabase.h:13-20).  A binding passes views of the
 * tables it holds; igx_scene_from_database turns them into an igx_scene whose
 * desc equals what igx_scene_load_file builds from the same scene file. */

/* DynTable lookup entry (table/DynTable.h:6-10), 16 bytes */
typedef struct igx_lookup_entry {
    uint32_t type_id;  /* ShapeProvider::id() for the "shapes" table */
    uint32_t flags;
    uint64_t offset;   /* byte offset of the record in the table data */
} igx_lookup_entry;

/* one DynTable / FixTable / SceneBVH byte array */
typedef struct igx_db_table {
    const uint8_t* data;
    uint64_t bytes;
    const igx_lookup_entry* lookups; /* DynTable only (NULL for a FixTable) */
    uint64_t count;                  /* DynTable: lookup count; FixTable: entryCount() */
} igx_db_table;

typedef struct igx_database_view {
    /* FixTables["entities"]: 36 x 4 B per entity, column-major toLocal 3x4,
     * toGlobal 3x4, normal 3x3, u32 shape_id, u32 material_id, pad
     * (LoaderEntity.cpp:155-162) */
    igx_db_table entities;
    /* DynTables["shapes"]: trimesh records (TriMeshProvider.cpp:583-598:
     * u32 faces, vertices, normals, texcoords; bbox min.xyz, 0, max.xyz, 0;
     * vertices and normals 16 B each; indices 4 x u32 per face; texcoords 8 B
     * each) and sphere records (SphereProvider.cpp:40-47: origin.xyz, radius) */
    igx_db_table shapes;
    uint32_t trimesh_type_id;  /* lookup type_id of the trimesh provider */
    uint32_t sphere_type_id;   /* lookup type_id of the sphere provider */
    /* FixTables["trimesh_primbvh"]: GPU-target BLAS blobs (TriMeshProvider.cpp:
     * 361-369); may be empty (igx then builds the BLAS itself) */
    igx_db_table trimesh_primbvh;
    /* SceneBVHs[provider].Leaves: EntityLeaf1 records (96 B, traversal/bvh.art:
     * 52-61; SceneBVHAdapter.h:88-104) of every provider's TLAS.  They carry the
     * entity visibility flags (LoaderEntity.cpp:120-128) and, in user[0..1],
     * the float offset of the entity's BLAS in trimesh_primbvh */
    const igx_db_table* scene_bvh_leaves;
    uint32_t num_scene_bvhs;
    float scene_bbox_min[3], scene_bbox_max[3]; /* SceneDatabase::SceneBBox */
} igx_database_view;

/* The part of a scene the reference compiles into shader code instead of
 * tables (the TechniqueVariantShaderSet handed to Device::render, Device.h:52):
 * film, camera, technique, the material of every material id
 * (LoaderContext::Materials order, LoaderEntity.cpp:42-103) and the lights
 * (area lights name their entity by its index in the entities table). */
typedef struct igx_shading_view {
    int32_t film_width, film_height;
    igx_camera camera;
    igx_technique technique;
    uint32_t num_materials; const igx_material* materials;
    uint32_t num_lights;    const igx_light* lights;
    /* image textures of the materials (igx_material::tex_index) and the
     * environment maps (igx_light::env_texture); igx_scene_from_database copies
     * the pixels.  A caller that keeps a view and hands it over again (the
     * IG::Device facade, host/Device.h) is taken to have changed an image only
     * if its size, format or `pixels` address changed: texels rewritten in
     * place behind the same address are not looked at, so give a changed image
     * a new buffer. */
    uint32_t num_images;    const igx_image* images;
    uint32_t num_textures;  const igx_texture* textures;
    /* measured BSDFs of the materials (igx_material::measured); the words are
     * copied.  The rule for a view handed over again is that of the images: a
     * table counts as changed if its counts or its `words` address changed. */
    uint32_t num_measured;  const igx_measured* measured;
} igx_shading_view;

/* Build a scene from the reference's tables plus the shading view.  Plane
 * shapes are recognised from the mesh records (TriMesh::getAsPlane, as
 * TriMeshProvider.cpp:562 does); entity world boxes follow
 * BoundingBox::transformed (LoaderEntity.cpp:141).  With a non-empty
 * trimesh_primbvh, every trimesh shape carries its reference BLAS (ref_bvh),
 * which igx_upload_scene then uses instead of building one (option
 * "rebuild_bvh" = 1 ignores it).  Returns NULL and fills err on malformed
 * tables (sizes, offsets, ids out of range). */
igx_scene* igx_scene_from_database(const igx_database_view* db, const igx_shading_view* shading, char* err,
                                   size_t err_len);

/* Write a linear RGB image (row-major, 3 floats per pixel, each multiplied by
 * `scale`, e.g. 1/iteration count) as an uncompressed float OpenEXR file with
 * `channels` = 3 (RGB) or 4 (RGB + alpha 1).  Replaces Image::save
 * (src/runtime/Image.h:92-101) for the framebuffer output.  0 on success. */
int igx_write_exr(const char* path, const float* rgb, int32_t width, int32_t height, int32_t channels, float scale);
/* One file of `n_layers` RGB layers with the channels <names[k]>.R / .G / .B,
 * layer k = planes_rgb[k] (as `rgb` above) times scales[k]: the reference's
 * layout of a render with AOVs (frontend/common/IO.cpp:105-129), where the
 * film is the layer "Default" and every AOV is divided by its own iteration
 * count.  0 on success; -1 for a bad argument (a layer named twice, too). */
int igx_write_exr_layers(const char* path, const char* const* names, const float* const* planes_rgb, int32_t n_layers,
                         int32_t width, int32_t height, const float* scales);

#ifdef __cplusplus
}
#endif
#endif
