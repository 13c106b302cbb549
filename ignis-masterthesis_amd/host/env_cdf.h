// The sampling table of an image environment map (host side, no HIP).
//   * bake -- EnvironmentLight.cpp:37 bakes `radiance` into an image of
//     max(1024, W) x max(512, H) pixels, pixel (x, y) being the texture at uv
//     (x / (w - 1), y / (h - 1)) (entrypoints/bake.art:6), evaluated here with
//     the texture's own filter, wrap and transform (host/image_texture.h)
//   * build -- CDF::computeForImage (CDF.cpp:42-133): MIS compensation, the sin
//     premultiply of the marginal, sequential float sums, the MinEps fallbacks
//     and the forced trailing 1
// Header only: host/scene_tables.cpp, which calls it at upload, stays a
// translation unit that links on its own.
// The table is the marginal (h floats), then the h rows (w floats each), as
// cdf::make_cdf_2d_from_buffer reads it (core/cdf.art:149-153).
#pragma once

#include "igx_scene.h"

#include "image_texture.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace igx {

constexpr int ENV_BAKE_MIN_WIDTH = 1024, ENV_BAKE_MIN_HEIGHT = 512;

// RGB of the baked image, 3 floats per pixel, row 0 at v = 0

inline void bake_env_image(const igx_texture& t, const igx_image& im, int& width, int& height, std::vector<float>& rgb) {
    using namespace igxd;
    width = std::max(ENV_BAKE_MIN_WIDTH, (int)im.width);
    height = std::max(ENV_BAKE_MIN_HEIGHT, (int)im.height);
    rgb.resize((size_t)width * height * 3);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const float u = (float)x / (float)(width - 1), v = (float)y / (float)(height - 1);
            float tu, tv;
            tex_transform(t.transform, u, v, tu, tv);
            const Texel c = tex_filter(t.filter, t.wrap_u, t.wrap_v, im.width, im.height, tu, tv,
                                       [&](int px, int py) { return tex_fetch(im.format, im.pixels, im.width, px, py); });
            float* o = &rgb[((size_t)y * width + x) * 3];
            o[0] = c.r;
            o[1] = c.g;
            o[2] = c.b;
        }
}

// One running-sum table of `count` cells, stored as cdf.art reads it (the leading 0 left out,
// the last entry exactly 1).  `cells` holds the running sums on entry.  A table whose total
// does not pass 1e-5 carries no usable density and becomes the ramp i / (count - 1).
inline void normalise_running_sums(float* cells, size_t count) {
    const float total = cells[count - 1];
    if (total > 1e-5f) {
        const float inv_total = 1.0f / total;
        for (size_t i = 0; i < count; ++i) cells[i] *= inv_total;
    } else {
        const float step = 1.0f / (count - 1);
        for (size_t i = 0; i < count; ++i) cells[i] = i * step;
    }
    cells[count - 1] = 1;
}

// What a pixel weighs in the table: the mean over its channels of what is left of each above
// `floor_rgb` (the map's mean under MIS compensation, zero without)
inline float env_pixel_weight(const float* rgb, const float* floor_rgb) {
    return (std::max(rgb[0] - floor_rgb[0], 0.0f) + std::max(rgb[1] - floor_rgb[1], 0.0f) + std::max(rgb[2] - floor_rgb[2], 0.0f)) / 3;
}

// The table of an RGB image: (height + width * height) floats, the marginal over the rows
// first, then each row's own table.  Every sum runs left to right (top to bottom) in float,
// the arithmetic CDF::computeForImage (CDF.cpp:42-133) fixes: tests/test_env_cdf.py holds the
// result to a float32 restatement bit for bit.
//   * compensate: the image's mean, taken as the sum of max(p, 0) / width over all pixels
//     divided by the height, is subtracted from every pixel first
//   * premultiply_sin: a row's share of the marginal is its total times sin(pi (y + 1/2) / height)
inline void build_env_cdf(const float* rgb, int width, int height, bool premultiply_sin, bool compensate, std::vector<float>& table) {
    const size_t w = (size_t)width, h = (size_t)height;
    table.assign(h + w * h, 0.0f);
    float mean_rgb[3] = {0, 0, 0};
    if (compensate) {
        for (size_t px = 0; px < w * h; ++px)
            for (int c = 0; c < 3; ++c) mean_rgb[c] += std::max(rgb[px * 3 + c], 0.0f) / w;
        for (int c = 0; c < 3; ++c) mean_rgb[c] /= (float)h;
    }
    float* const row_totals = table.data();
    for (size_t y = 0; y < h; ++y) {
        const float* const src = rgb + y * w * 3;
        float* const row = table.data() + h + y * w;
        float running = 0.0f;
        for (size_t x = 0; x < w; ++x) {
            const float weight = env_pixel_weight(src + 3 * x, mean_rgb);
            running = x == 0 ? weight : running + weight; // the first cell is the weight itself, not 0 + weight
            row[x] = running;
        }
        const float latitude = 3.14159265358979323846f * (y + 0.5f) / float(h);
        row_totals[y] = premultiply_sin ? running * std::sin(latitude) : running;
        normalise_running_sums(row, w);
    }
    for (size_t y = 1; y < h; ++y) row_totals[y] += row_totals[y - 1];
    normalise_running_sums(row_totals, h);
}

} // namespace igx
