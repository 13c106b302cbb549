// Image textures: one statement of the texture arithmetic for the device
// (apply_texture, full shading variant) and for the host (native checks).
//   * the border rules, the two texel mappings and the nearest, bilinear and
//     bicubic filters -- texture/image.art:9-146, as written there
//   * the uv transform -- make_image_texture (texture/image.art:148-152)
//   * the texel unpacking -- driver/image.art:9-16
//   * map_env_uv and its inverse, and the sampling and pdf of the 2-D CDF of an
//     image environment map -- light/env.art:16-21, 112-133; core/cdf.art:40-153
// The mirror border is restated as the reference has it: its select() takes the
// reversed index in the even periods, so the period [0, w) itself reads the
// image reversed (image.art:29-34).
// Plain types only.
#pragma once

#include <cmath>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IGX_TEX_HD __host__ __device__ __forceinline__
#else
#define IGX_TEX_HD inline
#endif

namespace igxd {

// igx_texture::filter / wrap_u / wrap_v and igx_image::format (include/igx_scene.h)
enum : int32_t { TEX_FILTER_NEAREST = 0, TEX_FILTER_BILINEAR = 1, TEX_FILTER_BICUBIC = 2 };
enum : int32_t { TEX_WRAP_REPEAT = 0, TEX_WRAP_CLAMP = 1, TEX_WRAP_MIRROR = 2 };
enum : int32_t { TEX_RGBA8 = 0, TEX_MONO8 = 1, TEX_FLOAT4 = 2 };

// What a texture lookup reads besides the material: 32 B in global memory.
// The records and the texels of a scene follow its texture coordinates in the
// uv table (SceneView::uv); `texels` counts 8-B table elements from its start.
struct TexRecord {
    int32_t width, height;
    int32_t format;          // TEX_RGBA8 / TEX_MONO8 / TEX_FLOAT4
    int32_t filter;          // TEX_FILTER_*
    int32_t wrap_u, wrap_v;  // TEX_WRAP_*
    uint32_t texels;         // first texel of row 0, in 8-B units from the table's start (16-B aligned)
    int32_t pad;
};
static_assert(sizeof(TexRecord) == 32, "a texture record is 32 B");

struct Texel {
    float r, g, b, a;
};

// image_rgba_unpack / image_mono_unpack + make_gray_color (driver/image.art:9-34)
IGX_TEX_HD Texel texel_unpack_rgba8(uint32_t p) {
    return Texel{(float)(p & 0xffu) / 255, (float)((p >> 8) & 0xffu) / 255, (float)((p >> 16) & 0xffu) / 255, (float)(p >> 24) / 255};
}
IGX_TEX_HD Texel texel_unpack_mono8(uint8_t p) {
    const float g = (float)p / 255;
    return Texel{g, g, g, 1.0f};
}

IGX_TEX_HD int tex_border(int wrap, int x, int w) {
    if (wrap == TEX_WRAP_CLAMP) return x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    if (wrap == TEX_WRAP_MIRROR) {
        const int t = x < 0 ? -1 - x : x;
        const int i = t / w;
        const int k = t - i * w;
        return (i & 1) == 0 ? w - 1 - k : k;
    }
    const int t = x % w;
    return t < 0 ? t + w : t;
}

// make_image_texture: mat3x3_transform_point_affine of the 2x3 transform m (row-major)
IGX_TEX_HD void tex_transform(const float* m, float u, float v, float& tu, float& tv) {
    tu = m[0] * u + m[1] * v + m[2] * 1.0f;
    tv = m[3] * u + m[4] * v + m[5] * 1.0f;
}

IGX_TEX_HD float tex_cubic_w0(float a) { return (a * (a * (-a + 3) - 3) + 1) / 6; }
IGX_TEX_HD float tex_cubic_w1(float a) { return (a * a * (3 * a - 6) + 4) / 6; }
IGX_TEX_HD float tex_cubic_w2(float a) { return (a * (a * (-3 * a + 3) + 3) + 1) / 6; }
IGX_TEX_HD float tex_cubic_w3(float a) { return (a * a * a) / 6; }
IGX_TEX_HD float tex_cubic_g0(float a) { return tex_cubic_w0(a) + tex_cubic_w1(a); }
IGX_TEX_HD float tex_cubic_g1(float a) { return tex_cubic_w2(a) + tex_cubic_w3(a); }
IGX_TEX_HD float tex_cubic_h0(float a) { return (tex_cubic_w1(a) / tex_cubic_g0(a)) - 1; }
IGX_TEX_HD float tex_cubic_h1(float a) { return (tex_cubic_w3(a) / tex_cubic_g1(a)) + 1; }

IGX_TEX_HD Texel texel_lerp(Texel a, Texel b, float t) {
    return Texel{(1 - t) * a.r + t * b.r, (1 - t) * a.g + t * b.g, (1 - t) * a.b + t * b.b, (1 - t) * a.a + t * b.a};
}
IGX_TEX_HD Texel texel_mulf(Texel a, float f) { return Texel{a.r * f, a.g * f, a.b * f, a.a * f}; }
IGX_TEX_HD Texel texel_add(Texel a, Texel b) { return Texel{a.r + b.r, a.g + b.g, a.b + b.b, a.a + b.a}; }

// The filtered image at uv (after tex_transform); `pixels(x, y)` returns the
// Texel of an in-range texel.
template <class Pixels>
IGX_TEX_HD Texel tex_filter(int filter, int wrap_u, int wrap_v, int w, int h, float u, float v, const Pixels& pixels) {
    if (filter == TEX_FILTER_NEAREST) {
        // map_uv_to_image_pixel_nearest: edge samples are exactly on the border
        const float fu = u * (float)w, fv = v * (float)h;
        return pixels(tex_border(wrap_u, (int)floorf(fu), w), tex_border(wrap_v, (int)floorf(fv), h));
    }
    // map_uv_to_image_pixel: texels in the middle of each pixel
    const float fu = u * (float)w - 0.5f, fv = v * (float)h - 0.5f;
    const int ix = (int)floorf(fu), iy = (int)floorf(fv);
    const float fx = fu - floorf(fu), fy = fv - floorf(fv);
    if (filter == TEX_FILTER_BILINEAR) {
        const int x0 = tex_border(wrap_u, ix, w), y0 = tex_border(wrap_v, iy, h);
        const int x1 = tex_border(wrap_u, ix + 1, w), y1 = tex_border(wrap_v, iy + 1, h);
        const Texel p00 = pixels(x0, y0), p10 = pixels(x1, y0), p01 = pixels(x0, y1), p11 = pixels(x1, y1);
        return texel_lerp(texel_lerp(p00, p10, fx), texel_lerp(p01, p11, fx), fy);
    }
    const float g0x = tex_cubic_g0(fx), g0y = tex_cubic_g0(fy), g1x = tex_cubic_g1(fx), g1y = tex_cubic_g1(fy);
    const int ix0 = (int)floorf((float)ix + tex_cubic_h0(fx) + 0.5f), iy0 = (int)floorf((float)iy + tex_cubic_h0(fy) + 0.5f);
    const int ix1 = (int)floorf((float)ix + tex_cubic_h1(fx) + 0.5f), iy1 = (int)floorf((float)iy + tex_cubic_h1(fy) + 0.5f);
    const int x0 = tex_border(wrap_u, ix0, w), y0 = tex_border(wrap_v, iy0, h);
    const int x1 = tex_border(wrap_u, ix1, w), y1 = tex_border(wrap_v, iy1, h);
    const Texel p00 = texel_mulf(pixels(x0, y0), g0x * g0y), p10 = texel_mulf(pixels(x1, y0), g1x * g0y);
    const Texel p01 = texel_mulf(pixels(x0, y1), g0x * g1y), p11 = texel_mulf(pixels(x1, y1), g1x * g1y);
    return texel_add(texel_add(p00, p10), texel_add(p01, p11));
}

// Texel (x, y) of an image stored as igx_image::pixels / behind a TexRecord:
// one 4-B load (RGBA8), one byte (MONO8) or one 16-B load (FLOAT4)
IGX_TEX_HD Texel tex_fetch(int format, const void* base, int w, int x, int y) {
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    if (format == TEX_FLOAT4) {
        struct alignas(16) F4 {
            float x, y, z, w;
        };
        const F4 p = static_cast<const F4*>(base)[i];
        return Texel{p.x, p.y, p.z, p.w};
    }
    if (format == TEX_MONO8) return texel_unpack_mono8(static_cast<const uint8_t*>(base)[i]);
    return texel_unpack_rgba8(static_cast<const uint32_t*>(base)[i]);
}

// ---- image environment maps (light/env.art:11-21, 112-164; core/cdf.art) ----
// What an image environment light reads: the 28 words of a DevLight behind
// its header (csrc/device_scene.h), as a CieSky does for a CIE sky.
struct EnvMap {
    float scale[3];
    uint32_t texture;     // its TexRecord's place in the uv table (8-B units)
    float m[9];           // transform.linear().transpose().inverse(), row-major
    uint32_t cdf;         // the CDF table's place in the uv table (8-B units); unused with cdf_w == 0
    int32_t cdf_w, cdf_h; // size of the baked image the CDF was built on; 0: no CDF, uniform sphere sampling
    float uv_transform[6];// the texture's 2x3 uv transform
    float pad[6];
};
static_assert(sizeof(EnvMap) == 112, "an EnvMap fills a DevLight behind its four header words");

struct EnvVec {
    float x, y, z;
};
constexpr float ENV_PI = 3.14159265358979323846f;

// safe_div (core/common.art:167)
IGX_TEX_HD float env_safe_div(float a, float b) { return fabsf(b) <= 1.1920929e-7f ? 0.0f : a / b; }

// switch_env_up(mat3x3_mul(transform, dir)): a world direction in the map's Z-up frame
IGX_TEX_HD EnvVec env_to_local(const EnvMap& e, EnvVec d) {
    const float x = e.m[0] * d.x + e.m[1] * d.y + e.m[2] * d.z, y = e.m[3] * d.x + e.m[4] * d.y + e.m[5] * d.z,
                z = e.m[6] * d.x + e.m[7] * d.y + e.m[8] * d.z;
    return EnvVec{x, z, y};
}
// mat3x3_left_mul(transform, switch_env_up(dir)): a sampled Z-up direction in world space
IGX_TEX_HD EnvVec env_to_world(const EnvMap& e, EnvVec d) {
    const float x = d.x, y = d.z, z = d.y;
    return EnvVec{e.m[0] * x + e.m[3] * y + e.m[6] * z, e.m[1] * x + e.m[4] * y + e.m[7] * z, e.m[2] * x + e.m[5] * y + e.m[8] * z};
}
// map_env_uv (env.art:16-21) of a Z-up direction: v = 1 is up, u turns about the up axis
IGX_TEX_HD void map_env_uv(EnvVec d, float& u, float& v) {
    // the light's printed transform is orthonormal to six digits only: |d.z| may pass 1 by a rounding
    const float theta = acosf(fminf(fmaxf(d.z, -1.0f), 1.0f));
    float phi = atan2f(d.y, d.x);
    if (phi < 0) phi += 2 * ENV_PI;
    const float t = phi / (2 * ENV_PI) + 0.25f;
    u = t - floorf(t);
    v = 1 - theta / ENV_PI;
}
// its inverse as make_environment_light_textured.sample_dir has it (env.art:119-122)
IGX_TEX_HD EnvVec env_dir_from_uv(float u, float v) {
    const float theta = (1 - v) * ENV_PI, phi = (u - 0.25f) * 2 * ENV_PI;
    const float s = sinf(theta), c = cosf(theta);
    return EnvVec{s * cosf(phi), s * sinf(phi), c};
}
// shading::sin_theta of a Z-up direction
IGX_TEX_HD float env_sin_theta(EnvVec d) {
    const float s2 = 1 - d.z * d.z;
    return s2 <= 0.0f ? 0.0f : sqrtf(s2);
}

// A CDF of `n` function values stored as [x1, ..., x_{n-1}, 1] at data[off..]: get(0) = 0 (cdf.art:67-70)
IGX_TEX_HD float cdf_get(const float* data, int off, int i) { return i == 0 ? 0.0f : data[off + i - 1]; }
// make_cdf_1d.sample_continuous (cdf.art:42-55) with interval::binary_search (interval.art:7-23)
IGX_TEX_HD void cdf_sample_continuous(const float* data, int off, int n, float u, int& at, float& pos, float& pdf) {
    int first = 0, len = n + 1;
    while (len > 0) {
        const int half = len / 2, middle = first + half;
        if (cdf_get(data, off, middle) <= u) {
            first = middle + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    int found = first - 1;
    found = found < 0 ? 0 : (found > n ? n : found); // clamp(first - 1, 0, size - 1), size = n + 1
    at = found < n - 1 ? found : n - 1;              // u = 1 is pulled down
    const float lo = cdf_get(data, off, at);
    const float p = cdf_get(data, off, at + 1) - lo;
    const float rem = env_safe_div(u - lo, p);
    const float x = ((float)at + rem) / (float)n;
    pos = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    pdf = p * (float)n;
}
// make_cdf_1d.pdf_continuous (cdf.art:46-49)
IGX_TEX_HD void cdf_pdf_continuous(const float* data, int off, int n, float x, int& at, float& pdf) {
    int i = (int)(x * (float)n);
    at = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    pdf = (cdf_get(data, off, at + 1) - cdf_get(data, off, at)) * (float)n;
}
// make_cdf_2d_from_buffer (cdf.art:102-153): the marginal (h) first, then the rows (w each)
IGX_TEX_HD void cdf2d_sample_continuous(const float* data, int w, int h, float ux, float uy, float& px, float& py, float& pdf) {
    int row, col;
    float p1, p2;
    cdf_sample_continuous(data, 0, h, uy, row, py, p1);
    cdf_sample_continuous(data, h + row * w, w, ux, col, px, p2);
    pdf = p1 * p2;
}
IGX_TEX_HD float cdf2d_pdf_continuous(const float* data, int w, int h, float x, float y) {
    int row, col;
    float p1, p2;
    cdf_pdf_continuous(data, 0, h, y, row, p1);
    cdf_pdf_continuous(data, h + row * w, w, x, col, p2);
    return p1 * p2;
}
// pdf_dir = pdf / (sin(theta) 2 pi^2) with safe_div (env.art:123, 132)
IGX_TEX_HD float env_pdf_solid(float pdf_uv, float sin_theta) { return env_safe_div(pdf_uv, sin_theta * ENV_PI * ENV_PI * 2); }

} // namespace igxd
