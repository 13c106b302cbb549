// The analytic CIE skies: one statement of the sky function for the device
// (shade_step's miss branch and light_sample_direct, full shading variant) and
// for the host (native checks), and the host constants of a clear or
// intermediate sky.
//   * cie_wmean, make_cie_sky_light, make_cie_sunny_light -- light/cie.art:1-42
//   * the constants -- CIELight::serialize (CIELight.cpp:65-92)
// Plain types only.
#pragma once

#include "igx_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>

#ifdef __HIPCC__
#define IGX_SKY_HD __host__ __device__ __forceinline__
#else
#define IGX_SKY_HD inline
#endif

namespace igxd {

// What the sky function reads: the 28 words of a DevLight behind its header
// (csrc/device_scene.h)
struct CieSky {
    float zenith[3], ground_brightness;
    float ground[3], zenith_ratio; // zenith brightness / factor (clear, intermediate)
    float scale[3], c2;            // scale and ground term (clear, intermediate)
    float sun_dir[3];
    int32_t kind_ground;           // IGX_SKY_* | has_ground << 8
    float m[9];                    // transform.linear().transpose().inverse(), row-major
    float pad[3];
};
static_assert(sizeof(CieSky) == 112, "a CieSky fills a DevLight behind its four header words");

struct SkyVec {
    float x, y, z;
};

IGX_SKY_HD int cie_kind(const CieSky& s) { return s.kind_ground & 0xff; }
IGX_SKY_HD bool cie_has_ground(const CieSky& s) { return (s.kind_ground >> 8) != 0; }

inline CieSky make_cie_sky(const igx_light& L) {
    CieSky s{};
    for (int i = 0; i < 3; ++i) {
        s.zenith[i] = L.sky_zenith[i];
        s.ground[i] = L.sky_ground[i];
        s.scale[i] = L.sky_scale[i];
        s.sun_dir[i] = L.sun_direction[i];
    }
    s.ground_brightness = L.ground_brightness;
    s.zenith_ratio = L.zenith_ratio;
    s.c2 = L.sky_c2;
    s.kind_ground = (L.sky_kind & 0xff) | (L.has_ground ? 1 << 8 : 0);
    for (int i = 0; i < 9; ++i) s.m[i] = L.sky_transform[i];
    return s;
}

// mat3x3_mul(transform, v): world direction -> the sky's Y-up frame
IGX_SKY_HD SkyVec cie_to_local(const CieSky& s, SkyVec v) {
    return SkyVec{s.m[0] * v.x + s.m[1] * v.y + s.m[2] * v.z, s.m[3] * v.x + s.m[4] * v.y + s.m[5] * v.z,
                  s.m[6] * v.x + s.m[7] * v.y + s.m[8] * v.z};
}
// mat3x3_left_mul(transform, v) = v^T * transform: a sampled local direction -> world
IGX_SKY_HD SkyVec cie_to_world(const CieSky& s, SkyVec v) {
    return SkyVec{s.m[0] * v.x + s.m[3] * v.y + s.m[6] * v.z, s.m[1] * v.x + s.m[4] * v.y + s.m[7] * v.z,
                  s.m[2] * v.x + s.m[5] * v.y + s.m[8] * v.z};
}

IGX_SKY_HD float cie_clamp1(float v) { return fminf(1.0f, fmaxf(-1.0f, v)); }

// cie_wmean (cie.art:1-7) of zenith * k1 and ground * k2
IGX_SKY_HD SkyVec cie_wmean(float cos_theta, const float* zenith, float k1, const float* ground, float k2) {
    const float a = powf(cos_theta + 1.01f, 10.0f);
    const float f1 = a * a / (a * a + 1);
    const float f2 = 1 / (a * a + 1);
    return SkyVec{zenith[0] * k1 * f1 + ground[0] * k2 * f2, zenith[1] * k1 * f1 + ground[1] * k2 * f2,
                  zenith[2] * k1 * f1 + ground[2] * k2 * f2};
}

// The sky's radiance towards the local (Y-up) direction `dir`: the closure of
// make_cie_sky_light (uniform, cloudy; cie.art:10-19) or make_cie_sunny_light
// (clear, intermediate; cie.art:22-42)
IGX_SKY_HD SkyVec cie_sky_radiance(const CieSky& s, SkyVec dir) {
    const float cos_theta = dir.y;
    if (!cie_has_ground(s) && cos_theta < 0) return SkyVec{0, 0, 0};
    const int kind = cie_kind(s);
    if (kind == IGX_SKY_UNIFORM || kind == IGX_SKY_CLOUDY) {
        const bool cloudy = kind == IGX_SKY_CLOUDY;
        const float c1 = cloudy ? (1 + 2 * cos_theta) / 3 : 1.0f;
        const float c2 = cloudy ? 0.777777777f : 1.0f;
        return cie_wmean(cos_theta, s.zenith, c1, s.ground, s.ground_brightness * c2);
    }
    const float cos_gamma = dir.x * s.sun_dir[0] + dir.y * s.sun_dir[1] + dir.z * s.sun_dir[2];
    const float gamma = acosf(cie_clamp1(cos_gamma));
    float c1;
    if (kind == IGX_SKY_CLEAR) {
        c1 = (0.91f + 10 * expf(-3 * gamma) + 0.45f * cos_gamma * cos_gamma) *
             (cos_theta >= 0.01f ? 1 - expf(-0.32f / cos_theta) : 1.0f);
    } else {
        const float theta = acosf(cie_clamp1(cos_theta));
        const float stheta = acosf(cie_clamp1(s.sun_dir[1]));
        c1 = ((1.35f * sinf(5.631f - 3.59f * theta) + 3.12f) * sinf(4.396f - 2.6f * stheta) + 6.37f - theta) / 2.326f *
             expf(gamma * (-0.563f) * ((2.629f - theta) * (1.562f - stheta) + 0.812f));
    }
    const SkyVec w = cie_wmean(cos_theta, s.zenith, s.zenith_ratio * c1, s.ground, s.ground_brightness * s.c2);
    return SkyVec{s.scale[0] * w.x, s.scale[1] * w.y, s.scale[2] * w.z};
}

// A number as the reference's generated shader text carries it: printed into
// a stream at its default precision (six significant digits)
inline float cie_printed(float v) {
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%g", (double)v);
    return std::strtof(buf, nullptr);
}

// skylight_normalization_factor (CIELight.cpp:28-40)
inline float cie_normalization_factor(float altitude, bool clear) {
    const float clear_approx[5] = {2.766521f, 0.547665f, -0.369832f, 0.009237f, 0.059229f};
    const float interm_approx[5] = {3.5556f, -2.7152f, -1.3081f, 1.0660f, 0.60227f};
    const float pi4 = 0.78539816339744830961f;
    const float x = (altitude - pi4) / pi4;
    const float* arr = clear ? clear_approx : interm_approx;
    float f = arr[4];
    for (int i = 3; i >= 0; --i) f = f * x + arr[i];
    return f;
}

// CIELight::serialize (CIELight.cpp:65-92) for a clear or intermediate sky
// with the sun at `elevation` (radians, already clamped to 87 degrees by the
// caller as CIELight.cpp:66-69 does) and direction sun_y = sun_direction.y:
// zenith brightness / factor and c2, both as printed into the shader
inline void cie_sunny_constants(bool clear, float elevation, float sun_y, float turbidity, float& zenith_ratio, float& c2) {
    const float pi2 = 1.57079632679489661923f, inv_pi = 0.31830988618379067154f;
    const float sky_illum = 203;
    float zb = (1.376f * turbidity - 1.81f) * std::tan(elevation) + 0.38f;
    if (!clear) zb = (zb + 8.6f * sun_y + 0.123f) / 2;
    zb = std::max(0.0f, zb * 1000 / sky_illum);
    float factor;
    if (clear) factor = 0.274f * (0.91f + 10 * std::exp(-3 * (pi2 - elevation)) + 0.45f * sun_y * sun_y);
    else factor = (2.739f + 0.9891f * std::sin(0.3119f + 2.6f * elevation)) * std::exp(-(pi2 - elevation) * (0.4441f + 1.48f * elevation));
    const float norm_factor = cie_normalization_factor(elevation, clear) * inv_pi / factor;
    const float sun_illum = 208;
    const float solar = 1.5e9f / sun_illum * (1.147f - 0.147f / std::max(sun_y, 0.16f));
    const float additive = 6e-5f * inv_pi * solar * sun_y * (clear ? 1.0f : 0.15f);
    zenith_ratio = cie_printed(zb / factor);
    c2 = cie_printed(zb * norm_factor + additive);
}

} // namespace igxd
