// The camera models: one statement of the ray arithmetic for the device
// (gen_path and k_camera_rays, csrc/igx_device.hip) and for the host (native
// checks), the way host/film_tools.h serves the film post-processing.
//   * perspective        -- camera/perspective.art:29-42 (make_perspective_camera)
//   * depth of field     -- camera/perspective.art:74-120 (make_perspective_dof_camera)
//   * orthogonal         -- camera/orthogonal.art:14-46
//   * fishlens, circular -- camera/fishlens.art:8-68 (the only aspect mode the
//                           reference loader produces, FishLensCamera.cpp:9)
// Plain types only.
#pragma once

#include "igx_scene.h"

#include <cmath>
#include <stdint.h>

#ifdef __HIPCC__
#define IGX_CAM_HD __host__ __device__ __forceinline__
#else
#define IGX_CAM_HD inline
#endif

namespace igxd {

// The camera as the kernels read it: SceneView::cam, and the model and lens
// beside it (SceneView::cam_type, cam_aperture, cam_focal), which only the
// full shading variant reads (camera_ray).
struct DevCamera {
    float eye[3], dir[3], up[3], right[3];
    // perspective: tan(fov / 2) per axis; orthogonal: half extent per axis;
    // fishlens: xasp, yasp of the circular aspect mode (fishlens.art:15-20)
    float scale_x, scale_y;
    float tmin, tmax;
};
struct DevLens {
    int32_t type;           // IGX_CAMERA_*
    float aperture_radius, focal_length;
};
struct CameraModel {
    DevCamera cam;
    DevLens lens;
};

constexpr float CAMERA_FLT_EPS = 1.1920928955e-07f; // flt_eps (core/common.art:3)
constexpr float CAMERA_PI = 3.14159265359f;         // flt_pi (core/common.art:7)

IGX_CAM_HD bool camera_has_dof(const DevLens& l) {
    return l.type == IGX_CAMERA_PERSPECTIVE && l.aperture_radius > CAMERA_FLT_EPS; // PerspectiveCamera.cpp:55
}
// the basic shading variant compiles the pinhole perspective camera only
inline bool camera_needs_full(const igx_camera& c) {
    return c.type != IGX_CAMERA_PERSPECTIVE || c.aperture_radius > CAMERA_FLT_EPS;
}

// Device constants of a camera on a width x height film (the scale of
// compute_scale_from_{h,v}fov, perspective.art:2-14; the orthogonal scale of
// OrthogonalCamera.cpp:41; right = normalize(cross(dir, up))).
inline CameraModel make_camera_model(const igx_camera& c, int width, int height) {
    CameraModel m{};
    DevCamera& k = m.cam;
    const float film_aspect = (float)width / (float)height;
    const float aspect = c.aspect > 0 ? c.aspect : film_aspect;
    if (c.type == IGX_CAMERA_ORTHOGONAL) {
        k.scale_x = c.ortho_scale;
        k.scale_y = c.ortho_scale / aspect;
    } else if (c.type == IGX_CAMERA_FISHLENS) {
        // fishlens.art:12-20 (w and h as f32; circular: the image circle touches the short side)
        k.scale_x = film_aspect < 1 ? 1.0f : film_aspect;
        k.scale_y = film_aspect > 1 ? 1.0f : film_aspect;
    } else if (c.vertical_fov) {
        k.scale_y = std::tan(c.fov / 2);
        k.scale_x = k.scale_y * aspect;
    } else {
        k.scale_x = std::tan(c.fov / 2);
        k.scale_y = k.scale_x / aspect;
    }
    float dir[3] = {c.dir[0], c.dir[1], c.dir[2]}, up[3] = {c.up[0], c.up[1], c.up[2]};
    float r[3] = {dir[1] * up[2] - dir[2] * up[1], dir[2] * up[0] - dir[0] * up[2], dir[0] * up[1] - dir[1] * up[0]};
    float rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    float irl = 1 / rl;
    for (int i = 0; i < 3; ++i) {
        k.eye[i] = c.eye[i];
        k.dir[i] = dir[i];
        k.up[i] = up[i];
        k.right[i] = r[i] * irl;
    }
    k.tmin = c.near_clip;
    k.tmax = c.far_clip;
    m.lens.type = c.type;
    m.lens.aperture_radius = c.aperture_radius;
    m.lens.focal_length = c.focal_length;
    return m;
}

struct CamVec {
    float x, y, z;
};
// mat3x3_mul(view, v) with view = (right, up, dir) as columns (core/matrix.art:79-82)
IGX_CAM_HD CamVec camera_to_world(const DevCamera& c, float x, float y, float z) {
    return CamVec{c.right[0] * x + c.up[0] * y + c.dir[0] * z, c.right[1] * x + c.up[1] * y + c.dir[1] * z,
                  c.right[2] * x + c.up[2] * y + c.dir[2] * z};
}
// vec3_normalize (core/vector.art:140): v * (1 / |v|)
IGX_CAM_HD CamVec camera_normalize(CamVec a) {
    const float s = 1.0f / sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
    return CamVec{a.x * s, a.y * s, a.z * s};
}
// safe_div (core/common.art:167)
IGX_CAM_HD float camera_safe_div(float a, float b) { return fabsf(b) <= CAMERA_FLT_EPS ? 0.0f : a / b; }
// square_to_concentric_disk (core/warp.art:2-22)
IGX_CAM_HD void camera_concentric_disk(float u, float v, float& x, float& y) {
    const float a = 2 * u - 1, b = 2 * v - 1;
    if (a == 0 && b == 0) {
        x = 0;
        y = 0;
    } else if (a * a > b * b) {
        const float phi = (CAMERA_PI / 4) * camera_safe_div(b, a);
        x = cosf(phi) * a;
        y = sinf(phi) * a;
    } else {
        const float phi = (CAMERA_PI / 2) - (CAMERA_PI / 4) * camera_safe_div(a, b);
        x = cosf(phi) * b;
        y = sinf(phi) * b;
    }
}

// Camera::generate_ray for the normalised pixel coordinate (nx, ny) in
// [-1, 1]^2 (ny up).  (u, v) are the two lens numbers of the depth-of-field
// camera, the third and fourth draw of the path (ignored by every other
// model, which draws nothing).
IGX_CAM_HD void camera_ray(const DevCamera& c, const DevLens& lens, float nx, float ny, float u, float v, CamVec& org,
                                  CamVec& dir) {
    if (lens.type == IGX_CAMERA_ORTHOGONAL) {
        const CamVec p = camera_to_world(c, c.scale_x * nx, c.scale_y * ny, 0);
        org = CamVec{p.x + c.eye[0], p.y + c.eye[1], p.z + c.eye[2]};
        dir = CamVec{c.dir[0], c.dir[1], c.dir[2]};
        return;
    }
    if (lens.type == IGX_CAMERA_FISHLENS) {
        // compute_d (fishlens.art:36-48), fov = pi
        const float fx = nx * c.scale_x;
        const float fy = ny * c.scale_y;
        const float r = sqrtf(fx * fx + fy * fy);
        const float theta = r * CAMERA_PI / 2;
        const float sT = sinf(theta);
        const float cT = cosf(theta);
        const float sP = r < CAMERA_FLT_EPS ? 0.0f : fy / r;
        const float cP = r < CAMERA_FLT_EPS ? 0.0f : fx / r;
        org = CamVec{c.eye[0], c.eye[1], c.eye[2]};
        dir = camera_normalize(camera_to_world(c, sT * cP, sT * sP, cT));
        return;
    }
    const CamVec d = camera_normalize(camera_to_world(c, c.scale_x * nx, c.scale_y * ny, 1));
    if (camera_has_dof(lens)) {
        // gen_ray (perspective.art:78-88); the lens offset has no component along dir
        float ax, ay;
        camera_concentric_disk(u, v, ax, ay);
        ax *= lens.aperture_radius;
        ay *= lens.aperture_radius;
        const CamVec ap = camera_to_world(c, ax, ay, 0);
        const float f = lens.focal_length;
        org = CamVec{c.eye[0] + ap.x, c.eye[1] + ap.y, c.eye[2] + ap.z};
        dir = camera_normalize(CamVec{d.x * f - ap.x, d.y * f - ap.y, d.z * f - ap.z});
        return;
    }
    org = CamVec{c.eye[0], c.eye[1], c.eye[2]};
    dir = d;
}

} // namespace igxd
