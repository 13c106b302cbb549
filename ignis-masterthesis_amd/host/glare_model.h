// The daylight glare probability (DGP) of a film: one statement of the
// arithmetic of the reference's glare shader (entrypoints/glare.art,
// Device::evaluateGlare, Device.cpp:1689-1723) for the device kernel
// (k_glare_scan, csrc/igx_post.h) and for the host (glare_host below, native
// checks), the way film_tools.h serves tonemap / imageinfo and camera_model.h
// the camera rays.  Plain types only.
//
// Per pixel (x, y) the shader needs
//   * the luminance 179 * Y of the scaled film in cd/m^2 (glare.art:120-122),
//   * the solid angle of the pixel: the spherical quadrilateral between the
//     camera's directions at the four lattice points (x, y), (x, y + 1),
//     (x + 1, y + 1), (x + 1, y) (calc_omega, glare.art:91-117),
// and from them six sums: the vertical illuminance E_v = sum lum * |cos| *
// omega, and over the pixels brighter than the threshold 179 * avg * mul their
// count, sum omega, sum lum * omega, sum x * omega and sum y * omega.  The
// position index (Guth / Iwata, glare.art:31-88) is taken at the omega-weighted
// centre of the source, and glare_finish (glare.art:222-240) puts the DGP
// together.
//
// Deliberate differences from the reference:
//  1. No pixel above the threshold: the reference divides 0 / 0 (avg_lum is
//     NaN, `glare_x as i32` unspecified).  Here avg_lum = avg_omega = 0,
//     num_pixels = 0, the position index is not evaluated, dgp = c1 * E_v + c3.
//  2. A source centred exactly on the view direction: the reference's
//     hv = normalize(dir / cos(sigma) - dir) is normalize(0), NaN, and so is
//     its DGP (a source centred on pixel (w/2, h/2) of an even film).  Here a
//     hv without a length gives position index 1, the model's value as
//     sigma -> 0.
//  3. Depth-of-field cameras: the reference draws successive numbers of one
//     generator seeded 42 for the four corner rays, so its solid angle of a
//     DOF camera is noise.  Here the lens numbers are u = v = 0.5, the lens
//     centre (camera_concentric_disk gives (0, 0)): a DOF camera evaluates as
//     its pinhole.
//  4. One evaluation per pixel: the reference runs six parallel_reduce passes
//     and an overlay pass, each regenerating the four rays.  Here a pixel's
//     solid angle and luminance are evaluated once and feed all six sums, and
//     the sums are fixed trees (glare_host states the order), the same bits on
//     every call.
// Kept as written: the shader's vangle = acos(up . d) - pi / 2 is negative for
// a direction on the `up` side of the view direction, so its `phi < 0` branch
// (Iwata) takes the sources in the upper half of the image and Guth's formula
// the lower half; and its hv is parallel to the ray itself, so tau is the
// angle between `up` and the ray.
#pragma once

#include "camera_model.h"
#include "film_tools.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "igx.h"

#ifdef __HIPCC__
#define IGX_GLARE_HD __host__ __device__ inline
#else
#define IGX_GLARE_HD inline
#endif

namespace igx {

using igxd::CameraModel;
using igxd::CamVec;

constexpr float GLARE_PI = igxd::CAMERA_PI;        // flt_pi
constexpr float GLARE_FLT_EPS = igxd::CAMERA_FLT_EPS;
constexpr float GLARE_WHITE_EFFICIENCY = 179.0f;   // color_builtins::white_efficiency (core/color.art:73)
constexpr int GLARE_SUMS = 6;
// the reduction order of k_glare_scan, which glare_host repeats: a block of
// GLARE_BLOCK threads takes GLARE_CHUNK consecutive pixels, thread t of it the
// GLARE_ITERS groups of 4 pixels at (k * GLARE_BLOCK + t) * 4
constexpr int GLARE_BLOCK = 256, GLARE_ITERS = 8, GLARE_WAVE = 64;
constexpr int GLARE_CHUNK = GLARE_BLOCK * 4 * GLARE_ITERS;

// the six sums; n counts pixels, the rest are float sums
struct GlareSums {
    float ev;       // sum lum * |dot(dir_cam, r1)| * omega over every pixel
    int32_t n;      // pixels with lum > lum_source
    float omega;    // over those: sum omega
    float lum;      //             sum lum * omega
    float x, y;     //             sum x * omega, sum y * omega
};

IGX_GLARE_HD float glare_dot(CamVec a, CamVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
IGX_GLARE_HD CamVec glare_cross(CamVec a, CamVec b) {
    return CamVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// camera_ray's direction at the lattice point (x, y) of a w x h film:
// make_pixelcoord_from_xy with sx = sy = 0 (driver/camera.art:21-29), the
// pixel's corner, not its centre; x may be w and y may be h.  Lens numbers
// u = v = 0.5 (difference 3).
IGX_GLARE_HD CamVec glare_pixel_dir(const CameraModel& m, int w, int h, int x, int y) {
    const float nx = 2 * (float)x / (float)w - 1;
    const float ny = 1 - 2 * (float)y / (float)h;
    CamVec org, dir;
    igxd::camera_ray(m.cam, m.lens, nx, ny, 0.5f, 0.5f, org, dir);
    return dir;
}

// splane (glare.art:92-97): the unit normal of the plane through the origin,
// a and b; zero for a degenerate pair
IGX_GLARE_HD CamVec glare_splane(CamVec a, CamVec b) {
    const CamVec n = glare_cross(a, CamVec{b.x - a.x, b.y - a.y, b.z - a.z});
    if (glare_dot(n, n) > 0) return igxd::camera_normalize(n);
    return CamVec{0, 0, 0};
}

// calc_omega (glare.art:91-117): the solid angle of the spherical
// quadrilateral r1 r2 r3 r4, as the sum of its interior angles less 2 pi
IGX_GLARE_HD float glare_omega(CamVec r1, CamVec r2, CamVec r3, CamVec r4) {
    const CamVec n1 = glare_splane(r1, r2), n2 = glare_splane(r2, r3), n3 = glare_splane(r3, r4), n4 = glare_splane(r4, r1);
    const float a1 = GLARE_PI - fabsf(acosf(glare_dot(n1, n2)));
    const float a2 = GLARE_PI - fabsf(acosf(glare_dot(n2, n3)));
    const float a3 = GLARE_PI - fabsf(acosf(glare_dot(n3, n4)));
    const float a4 = GLARE_PI - fabsf(acosf(glare_dot(n4, n1)));
    const float ang = a1 + a2 + a3 + a4;
    return ang - 2 * GLARE_PI;
}

IGX_GLARE_HD float glare_finite(float a) { return __builtin_isfinite(a) ? a : 0.0f; }

// 179 * srgb_to_xyY(scale * rgb).b, non-finite components read as 0 (glare.art:120-122)
IGX_GLARE_HD float glare_luminance(float r, float g, float b, float scale) {
    return GLARE_WHITE_EFFICIENCY *
           srgb_to_xyY(FilmColor{glare_finite(r) * scale, glare_finite(g) * scale, glare_finite(b) * scale}).b;
}
// the threshold and the overlay's upper end (glare.art:124-125)
IGX_GLARE_HD float glare_lum_source(const igx_glare_settings& s) { return GLARE_WHITE_EFFICIENCY * (s.lum_avg * s.lum_mul); }
IGX_GLARE_HD float glare_lum_max(const igx_glare_settings& s) { return GLARE_WHITE_EFFICIENCY * s.lum_max; }

// calc_posindex (glare.art:31-88) at the lattice point (px, py)
IGX_GLARE_HD float glare_posindex(const CameraModel& m, int w, int h, int px, int py) {
    const CamVec d = glare_pixel_dir(m, w, h, px, py);
    const CamVec up{m.cam.up[0], m.cam.up[1], m.cam.up[2]}, dir{m.cam.dir[0], m.cam.dir[1], m.cam.dir[2]};
    const CamVec right = glare_cross(dir, up); // unnormalised, as there
    const float vangle = acosf(glare_dot(up, d)) - GLARE_PI / 2.0f;
    const float hangle = GLARE_PI / 2.0f - acosf(glare_dot(right, d));
    float sigma = acosf(glare_dot(dir, d));
    const float t = cosf(sigma);
    const float it = 1.0f / t;
    const CamVec hv0{d.x * it - d.x, d.y * it - d.y, d.z * it - d.z};
    if (!(glare_dot(hv0, hv0) > 0)) return 1.0f; // difference 2 (a NaN sigma from a dot product above 1 included)
    const CamVec hv = igxd::camera_normalize(hv0);
    float tau = acosf(glare_dot(up, hv));
    const float deg = 180.0f / GLARE_PI;
    float fact = 0.8f;
    float phi = vangle, theta = hangle;
    if (phi == 0) phi = 0.00001f;
    if (sigma <= 0) sigma = -sigma;
    if (theta == 0) theta = 0.0001f;
    tau = tau * deg;
    sigma = sigma * deg;
    // Guth
    float posindex = expf((35.2f - 0.31889f * tau - 1.22f * expf(-2 * tau / 9)) / 1000 * sigma +
                          (21 + 0.26667f * tau - 0.002963f * tau * tau) / 100000 * sigma * sigma);
    // Iwata
    if (phi < 0.0f) {
        const float dd = 1.0f / tanf(phi);
        const float s = tanf(theta) / tanf(phi);
        float r = sqrtf(1.0f / dd * 1.0f / dd + s * s / dd / dd);
        if (r > 0.6f) fact = 1.2f;
        if (r > 3) {
            fact = 1.2f;
            r = 3.0f;
        }
        posindex = 1.0f + fact * r;
    }
    if (posindex > 16) posindex = 16;
    return posindex;
}

// colormap::inferno (core/colormap.art:56-66), Horner in t per channel
IGX_GLARE_HD FilmColor glare_inferno(float t) {
    const float c[7][3] = {{0.0002189403691192265f, 0.001651004631001012f, -0.01948089843709184f},
                           {0.1065134194856116f, 0.5639564367884091f, 3.932712388889277f},
                           {11.60249308247187f, -3.972853965665698f, -15.9423941062914f},
                           {-41.70399613139459f, 17.43639888205313f, 44.35414519872813f},
                           {77.162935699427f, -33.40235894210092f, -81.80730925738993f},
                           {-71.31942824499214f, 32.62606426397723f, 73.20951985803202f},
                           {25.13112622477341f, -12.24266895238567f, -23.07032500287172f}};
    float o[3];
    for (int k = 0; k < 3; ++k) {
        float v = c[6][k];
        for (int i = 5; i >= 0; --i) v = c[i][k] + v * t;
        o[k] = v;
    }
    return FilmColor{o[0], o[1], o[2]};
}
// the heatmap word of a pixel above the threshold (glare.art:212-218)
IGX_GLARE_HD uint32_t glare_overlay(float lum, float lum_source, float lum_max) {
    const float max_diff = fmaxf(GLARE_FLT_EPS, lum_max - lum_source);
    const float f = (lum - lum_source) / max_diff;
    const FilmColor c = glare_inferno(fminf(1.0f, fmaxf(0.0f, f * f)));
    return packed_color(color_byte(c.r), color_byte(c.g), color_byte(c.b), 255);
}

// What one pixel adds to the sums.  r1..r4: the lattice directions at (x, y),
// (x, y + 1), (x + 1, y + 1), (x + 1, y).  Returns whether the pixel is above
// the threshold (its overlay word is then glare_overlay(lum, ...)).
IGX_GLARE_HD bool glare_add_pixel(GlareSums& s, const CameraModel& m, int x, int y, float lum, float lum_source, CamVec r1, CamVec r2,
                                  CamVec r3, CamVec r4) {
    const float omega = glare_omega(r1, r2, r3, r4);
    const float cos_f = fabsf(glare_dot(CamVec{m.cam.dir[0], m.cam.dir[1], m.cam.dir[2]}, r1));
    s.ev += lum * cos_f * omega;
    if (!(lum > lum_source)) return false;
    s.n += 1;
    s.omega += omega;
    s.lum += lum * omega;
    s.x += (float)x * omega;
    s.y += (float)y * omega;
    return true;
}
IGX_GLARE_HD GlareSums glare_sums_add(const GlareSums& a, const GlareSums& b) {
    return GlareSums{a.ev + b.ev, a.n + b.n, a.omega + b.omega, a.lum + b.lum, a.x + b.x, a.y + b.y};
}

// glare.art:222-240: the six sums (added over the whole film) to the output
inline igx_glare_output glare_finish(const GlareSums& s, const igx_glare_settings& set, const CameraModel& m, int w, int h) {
    const float c1 = 5.87e-5f, c2 = 0.0981f, c3 = 0.16f;
    const float a1 = 2.0f, a2 = 1.0f, a3 = 1.87f, a4 = 2.0f, a5 = 1.0f;
    igx_glare_output out{};
    const float E_v = set.vertical_illuminance < 0 ? s.ev : set.vertical_illuminance;
    out.vertical_illuminance = E_v;
    out.num_pixels = s.n;
    if (s.n <= 0 || !(s.omega > 0)) { // difference 1 (and a source without a solid angle: an orthogonal camera)
        out.dgp = c1 * std::pow(E_v, a5) + c3;
        return out;
    }
    const float glare_omega = s.omega;
    const float glare_lum = s.lum / glare_omega;
    const float glare_x = s.x / glare_omega, glare_y = s.y / glare_omega;
    const float posi = glare_posindex(m, w, h, (int)glare_x, (int)glare_y);
    const float acc = std::pow(glare_lum, a1) / std::pow(posi, a4) * std::pow(glare_omega, a2) / std::pow(E_v, a3);
    const float source_dgp = std::log10(1 + acc);
    out.dgp = c1 * std::pow(E_v, a5) + c2 * source_dgp + c3;
    out.avg_lum = glare_lum;
    out.avg_omega = glare_omega;
    return out;
}

// One block's share of the sums in the kernel's order: every thread adds its
// (at most 32) pixels in a row, a wave of 64 folds by halves (lane i takes
// lane i + 32, then + 16, ... + 1), the four waves add in wave order.
// overlay (may be nullptr): the words of the pixels above the threshold.
inline GlareSums glare_host_block(const float* film, int w, int h, size_t base, const CameraModel& m, float scale, float lum_source,
                                  float lum_max, uint32_t* overlay) {
    const size_t n = (size_t)w * h;
    std::vector<GlareSums> acc(GLARE_BLOCK, GlareSums{0, 0, 0, 0, 0, 0});
    for (int t = 0; t < GLARE_BLOCK; ++t)
        for (int k = 0; k < GLARE_ITERS; ++k) {
            const size_t p0 = base + ((size_t)k * GLARE_BLOCK + t) * 4;
            for (size_t p = p0; p < p0 + 4 && p < n; ++p) {
                const int x = (int)(p % w), y = (int)(p / w);
                const float lum = glare_luminance(film[3 * p], film[3 * p + 1], film[3 * p + 2], scale);
                const bool above = glare_add_pixel(acc[t], m, x, y, lum, lum_source, glare_pixel_dir(m, w, h, x, y),
                                                   glare_pixel_dir(m, w, h, x, y + 1), glare_pixel_dir(m, w, h, x + 1, y + 1),
                                                   glare_pixel_dir(m, w, h, x + 1, y));
                if (above && overlay) overlay[p] = glare_overlay(lum, lum_source, lum_max);
            }
        }
    GlareSums block{0, 0, 0, 0, 0, 0};
    for (int wv = 0; wv < GLARE_BLOCK / GLARE_WAVE; ++wv) {
        GlareSums* v = acc.data() + wv * GLARE_WAVE;
        for (int d = GLARE_WAVE / 2; d > 0; d >>= 1)
            for (int i = 0; i < d; ++i) v[i] = glare_sums_add(v[i], v[i + d]);
        block = wv == 0 ? v[0] : glare_sums_add(block, v[0]);
    }
    return block;
}

// The whole evaluation on the host: blocks in order, then glare_finish.
// film: w * h RGB floats; overlay (w * h words, may be nullptr): a pixel at or
// below the threshold keeps its word.
inline void glare_host(const float* film, int w, int h, const CameraModel& m, const igx_glare_settings& set, uint32_t* overlay,
                       igx_glare_output* out) {
    const size_t n = (size_t)w * h;
    const float lum_source = glare_lum_source(set), lum_max = glare_lum_max(set);
    GlareSums total{0, 0, 0, 0, 0, 0};
    for (size_t base = 0; base < n; base += GLARE_CHUNK)
        total = glare_sums_add(total, glare_host_block(film, w, h, base, m, set.scale, lum_source, lum_max, overlay));
    *out = glare_finish(total, set, m, w, h);
}

} // namespace igx
