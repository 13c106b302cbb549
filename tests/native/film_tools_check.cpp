// host/film_tools.h against values worked out by hand from the reference's
// core/color.art:77-142, entrypoints/tonemap.art and entrypoints/imageinfo.art
// (tests/test_film_tools.py compiles it with g++ and runs it; no libigx, no
// GPU).  film_tools.h is the yardstick of the device kernels (csrc/igx_post.h,
// tests/native/film_post_check.cpp), so nothing expected here is computed with
// the header's own functions: every literal below comes from the formulas.
// Prints "ok" when every check passed.
#include "film_tools.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int bad = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++bad;                             \
        }                                      \
    } while (0)

static bool near(float got, double want, double rel = 2e-6) { return std::fabs((double)got - want) <= rel * std::fabs(want) + 1e-30; }

static std::vector<float> grey(const std::vector<float>& v) {
    std::vector<float> f;
    for (float x : v) f.insert(f.end(), {x, x, x});
    return f;
}

int main() {
    // ---- the five curves at L = 0.37 and L = 2.9 ----------------------------
    //  1: L / (1 + L)                       2: L (1 + L / 16) / (1 + L)
    //  3: L (2.51 L + 0.03) / (L (2.43 L + 0.59) + 0.14)
    //  4: f(L) / f(11.2), f(x) = (x (0.15 x + 0.05) + 0.004) / (x (0.15 x + 0.5) + 0.06) - 1 / 15
    const double curve[2][5] = {{0.37, 0.2700730, 0.2763184, 0.5133661, 0.1315660}, {2.9, 0.7435897, 0.8783654, 0.9510394, 0.6099098}};
    // the bytes of a grey pixel of that luminance: (uint8)(min(t, 1) * 255),
    // and with the sRGB curve 1.055 t^(1 / 2.4) - 0.055 first
    const unsigned plain[2][5] = {{94, 68, 70, 130, 33}, {255, 189, 223, 242, 155}};
    const unsigned gamma[2][5] = {{163, 141, 143, 189, 101}, {255, 223, 240, 249, 204}};
    const float lum[2] = {0.37f, 2.9f};
    for (int k = 0; k < 2; ++k)
        for (int m = 0; m < 5; ++m) {
            const float t = igx::tonemap_curve(m, lum[k]);
            CHECK(near(t, curve[k][m], 1e-6), "curve %d at %g: %.8g, expected %.8g", m, lum[k], t, curve[k][m]);
            // sRGB white has Y = 0.2126729 + 0.7151522 + 0.0721750 = 1.0000001
            const float px[3] = {lum[k], lum[k], lum[k]};
            for (int g = 0; g < 2; ++g) {
                uint32_t out = 0;
                igx::tonemap_film(px, 1, 1.0f, m, g != 0, 1.0f, 0.0f, &out);
                const unsigned b = g ? gamma[k][m] : plain[k][m];
                const uint32_t want = 0xff000000u | (b << 16) | (b << 8) | b;
                CHECK(out == want, "method %d gamma %d at %g: %08x, expected %08x", m, g, lum[k], out, want);
            }
        }
    // exposure: the curve runs on factor * Y + offset; scale multiplies the film first:
    // 2 * 0.5 grey = 1, 0.5 * 1 + 0.24 = 0.74, Reinhard 0.74 / 1.74 = 0.4252874 -> 108.4
    {
        const float px[3] = {2, 2, 2};
        uint32_t out = 0;
        igx::tonemap_film(px, 1, 0.5f, 1, false, 0.5f, 0.24f, &out);
        CHECK(out == 0xff6c6c6cu, "exposure: %08x", out);
    }
    // channel order: pure sRGB red through the identity curve stays red:
    // (a << 24) | (r << 16) | (g << 8) | b with 0.8 * 255 = 204
    {
        const float px[3] = {0.8f, 0, 0};
        uint32_t out = 0;
        igx::tonemap_film(px, 1, 1.0f, 0, false, 1.0f, 0.0f, &out);
        const int r = (out >> 16) & 255, g = (out >> 8) & 255, b = out & 255;
        CHECK((out >> 24) == 255 && std::abs(r - 204) <= 1 && g <= 1 && b <= 1, "red: %08x", out);
    }

    // ---- the flag colours (tonemap.art): NaN luminance cyan, infinite pink, ---
    // ---- a negative xyY component (255, 255, 0) -------------------------------
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        // (1, -1, 1): X = 0.2353178, Y = -0.4303043, Z = 0.8504460, sum 0.6554595 > eps, so y < 0
        const float px[12] = {nan, 0, 0, inf, 1, 1, 1, -1, 1, 0.5f, 0.5f, 0.5f};
        uint32_t out[4] = {0, 0, 0, 0};
        igx::tonemap_film(px, 4, 1.0f, 1, true, 1.0f, 0.0f, out);
        CHECK(out[0] == 0xff00ffffu, "NaN pixel: %08x", out[0]);
        CHECK(out[1] == 0xffff0096u, "inf pixel: %08x", out[1]);
        CHECK(out[2] == 0xffffff00u, "negative pixel: %08x", out[2]);
        CHECK(out[3] != 0xff00ffffu && out[3] != 0xffff0096u && out[3] != 0xffffff00u && (out[3] >> 24) == 255, "plain pixel: %08x", out[3]);
    }

    // ---- imageinfo, 3 x 2: not above 10 x 10, the soft values fall back -------
    {
        const std::vector<float> f = grey({1, 2, 3, 4, 5, 6});
        const igx::FilmInfo i = igx::imageinfo_film(f.data(), 3, 2, 1.0f, 0, nullptr, nullptr, nullptr, nullptr, true, false);
        CHECK(near(i.min, 1.0000001) && near(i.max, 6.0000006) && near(i.avg, 3.50000035), "3x2 min/max/avg %g %g %g", i.min, i.max, i.avg);
        CHECK(i.soft_min == i.min && i.soft_max == i.max && i.median == i.avg, "3x2 soft fallback");
        CHECK(i.inf_count == 0 && i.nan_count == 0 && i.neg_count == 0, "3x2 counts");
        // scale: everything scales with it
        const igx::FilmInfo h = igx::imageinfo_film(f.data(), 3, 2, 0.5f, 0, nullptr, nullptr, nullptr, nullptr, true, false);
        CHECK(near(h.min, 0.50000005) && near(h.max, 3.0000003) && near(h.avg, 1.75000018), "3x2 scaled");
    }

    // ---- imageinfo, 12 x 11 ramp v(x, y) = x + 12 y (0 .. 131) ----------------
    // The window of an interior pixel c sorts to c - 13, c - 12, c - 11, c - 1, c,
    // c + 1, c + 11, c + 12, c + 13: 2nd = c - 12, 5th = c, 8th = c + 12.  Interior
    // c runs from 13 to 118, so soft min = 1, soft max = 130, and the median is
    // the mean of c: 5.5 + 12 * 5 = 65.5; min 0, max 131, average 65.5.
    // Histogram (imageinfo.art:109-113): start = min = 0 (min < max), end = soft
    // max = 130 (min < soft max) although max is 131; 7 bins, factor 7 / 130, so
    // the bin edges 18.57, 37.14, 55.71, 74.29, 92.86, 111.43 lie between the
    // integers, and 130 (bin 7) and 131 clamp into the last bin
    {
        std::vector<float> v;
        for (int k = 0; k < 132; ++k) v.push_back((float)k);
        const std::vector<float> f = grey(v);
        int h[4][7];
        const igx::FilmInfo i = igx::imageinfo_film(f.data(), 12, 11, 1.0f, 7, h[0], h[1], h[2], h[3], true, true);
        CHECK(i.min == 0 && near(i.max, 131.0000131) && near(i.avg, 65.50000655), "ramp min/max/avg %g %g %g", i.min, i.max, i.avg);
        CHECK(near(i.soft_min, 1.0000001) && near(i.soft_max, 130.000013) && near(i.median, 65.50000655, 1e-5), "ramp soft %g %g %g",
              i.soft_min, i.soft_max, i.median);
        const int want[7] = {19, 19, 18, 19, 18, 19, 20};
        for (int c = 0; c < 4; ++c)
            for (int b = 0; b < 7; ++b) CHECK(h[c][b] == want[b], "ramp histogram %d bin %d: %d, expected %d", c, b, h[c][b], want[b]);
        // bins = 1: everything in the one bin
        int one[4] = {-1, -1, -1, -1};
        igx::imageinfo_film(f.data(), 12, 11, 1.0f, 1, &one[0], &one[1], &one[2], &one[3], false, true);
        CHECK(one[0] == 132 && one[1] == 132 && one[2] == 132 && one[3] == 132, "one bin");
        // acquire_histogram off leaves the arrays alone
        int keep[4] = {-7, -7, -7, -7};
        igx::imageinfo_film(f.data(), 12, 11, 1.0f, 1, &keep[0], &keep[1], &keep[2], &keep[3], false, false);
        CHECK(keep[0] == -7 && keep[3] == -7, "histogram written without acquire_histogram");
    }

    // ---- a constant film: min == max, so start = 0 and end = start + 1 --------
    // value 2, 4 bins: factor 4, (2 - 0) * 4 = 8 clamps into bin 3
    {
        const std::vector<float> f = grey(std::vector<float>(132, 2.0f));
        int h[4][4];
        const igx::FilmInfo i = igx::imageinfo_film(f.data(), 12, 11, 1.0f, 4, h[0], h[1], h[2], h[3], true, true);
        CHECK(i.min == i.max && near(i.min, 2.0000002) && near(i.avg, 2.0000002, 1e-5), "constant min/max/avg %g %g %g", i.min, i.max, i.avg);
        CHECK(i.soft_min == i.min && i.soft_max == i.max && near(i.median, 2.0000002, 1e-5), "constant soft %g %g %g", i.soft_min, i.soft_max,
              i.median);
        for (int c = 0; c < 4; ++c) CHECK(h[c][0] == 0 && h[c][1] == 0 && h[c][2] == 0 && h[c][3] == 132, "constant histogram %d", c);
        // value 0.3: (0.3 - 0) * 4 = 1.2, bin 1 (with start = min it would be bin 0)
        const std::vector<float> g = grey(std::vector<float>(132, 0.3f));
        igx::imageinfo_film(g.data(), 12, 11, 1.0f, 4, h[0], h[1], h[2], h[3], true, true);
        for (int c = 0; c < 4; ++c) CHECK(h[c][1] == 132, "constant 0.3 histogram %d: %d %d %d %d", c, h[c][0], h[c][1], h[c][2], h[c][3]);
    }

    // ---- non-finite, negative and -0.0 components ------------------------------
    // 4 x 3 of grey 1 (Y = 1.0000001) with five pixels changed; a non-finite
    // component reads as 0 for the luminance:
    //   (+inf, 1, 1) and (-0.0, 1, 1): 0.7151522 + 0.0721750        = 0.7873272
    //   (1, -inf, 1):                  0.2126729 + 0.0721750        = 0.2848479
    //   (1, 1, NaN):                   0.2126729 + 0.7151522        = 0.9278251
    //   (-2, 1, 1):                   -0.4253458 + 0.7873272        = 0.3619814
    // average (7 * 1.0000001 + 3.1493088) / 12 = 0.8457758
    // counts over the raw components: inf 2, NaN 1, sign bit set 3 (-inf, -2, -0.0)
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> f = grey(std::vector<float>(12, 1.0f));
        f[0] = inf;
        f[3 * 3 + 1] = -inf;  // a row end
        f[3 * 5 + 2] = nan;
        f[3 * 6 + 0] = -2.0f;
        f[3 * 11 + 0] = -0.0f; // the last pixel
        const igx::FilmInfo i = igx::imageinfo_film(f.data(), 4, 3, 1.0f, 0, nullptr, nullptr, nullptr, nullptr, true, false);
        CHECK(near(i.min, 0.2848479) && near(i.max, 1.0000001) && near(i.avg, 0.8457758), "flagged min/max/avg %.8g %.8g %.8g", i.min, i.max,
              i.avg);
        CHECK(i.inf_count == 2 && i.nan_count == 1 && i.neg_count == 3, "flagged counts %d %d %d", i.inf_count, i.nan_count, i.neg_count);
        const igx::FilmInfo n = igx::imageinfo_film(f.data(), 4, 3, 1.0f, 0, nullptr, nullptr, nullptr, nullptr, false, false);
        CHECK(n.inf_count == 0 && n.nan_count == 0 && n.neg_count == 0, "counts without acquire_error_stats");
        // histograms: the non-finite components count as 0.  2 bins over [min, max]
        // = [0.2848479, 1.0000001], edge at 0.642424: R holds 0 (inf), 1 x 9, -2,
        // -0.0 -> bin 0: inf, -2, -0.0 = 3; G: -inf -> 0, rest 1 -> 1 / 11; B: NaN
        // -> 0 -> 1 / 11; L: 0.2848479, 0.3619814 below the edge -> 2 / 10
        int h[4][2];
        igx::imageinfo_film(f.data(), 4, 3, 1.0f, 2, h[0], h[1], h[2], h[3], true, true);
        CHECK(h[0][0] == 3 && h[0][1] == 9 && h[1][0] == 1 && h[1][1] == 11 && h[2][0] == 1 && h[2][1] == 11 && h[3][0] == 2 && h[3][1] == 10,
              "flagged histograms %d %d | %d %d | %d %d | %d %d", h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]);
    }

    std::printf(bad ? "failed\n" : "ok\n");
    return bad ? 1 : 0;
}
