// The device tonemap / imageinfo kernels (csrc/igx_post.h, through
// igx_tonemap_film / igx_imageinfo_film and the IG::Device facade) against the
// host loops of host/film_tools.h compiled into this program
// (tests/test_film_post_gpu.py builds it with g++ -ffp-contract=off against
// libigx.so and runs it on the GPU).
//   * tonemap, five methods, both output modes: without gamma the image equals
//     the host's word for word (same IEEE operations); with gamma every channel
//     is within 1 (pow differs by a few ulp, the byte is truncated), alpha and
//     flagged pixels equal;
//   * imageinfo: min, max, soft min, soft max, the counts and the histograms
//     equal the host's; avg and median within 1e-5 relative of a float64 sum of
//     the same float32 terms (1e-5 * mean |L| on films with negative
//     luminances): the device adds at most 32 terms in a row per lane, then a
//     tree of about 20 levels, so at most ~60 roundings of 2^-24 each;
//   * two calls give the same bits; the handle's scratch grows and shrinks
//     without changing a result; films that are not 16-byte aligned take the
//     scalar path to the same result;
//   * the facade's tonemap / imageinfo over a rendered film, the named entry
//     points before the first render, unknown AOV names, a size mismatch.
// Prints "ok" when every check passed.
#include "Device.h"
#include "film_tools.h"
#include "igx_scene.h"
#include "scene_database.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

static int bad = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (bad < 40) {                    \
                std::printf("FAIL: " __VA_ARGS__); \
                std::printf("\n");             \
            }                                  \
            ++bad;                             \
        }                                      \
    } while (0)
#define HIP(e)                                                                      \
    do {                                                                            \
        hipError_t e_ = (e);                                                        \
        if (e_ != hipSuccess) {                                                     \
            std::printf("FAIL: %s: %s\n", #e, hipGetErrorString(e_));               \
            return 1;                                                               \
        }                                                                           \
    } while (0)

struct Lcg {
    uint32_t s;
    double next() { // (0, 1)
        s = s * 1664525u + 1013904223u;
        return ((s >> 8) + 0.5) / 16777216.0;
    }
};

struct Film {
    std::string name;
    int w, h;
    std::vector<float> rgb;
    bool negatives = false;
};

// log-uniform between e^-4 and 1e4: most values small, a long tail
static Film tailed(int w, int h, uint32_t seed) {
    Film f{"tailed " + std::to_string(w) + "x" + std::to_string(h), w, h, std::vector<float>((size_t)w * h * 3)};
    Lcg g{seed};
    for (float& v : f.rgb) v = (float)std::fmin(1e4, std::exp(g.next() * 13.3 - 4.0));
    return f;
}
static Film constant(int w, int h, float v) {
    return Film{"constant " + std::to_string(v) + " " + std::to_string(w) + "x" + std::to_string(h), w, h, std::vector<float>((size_t)w * h * 3, v)};
}
// +inf, -inf, NaN, negatives and -0.0 at fixed positions: the first pixel, the
// last pixel, a row end, and scattered
static Film injected(Film f) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t n = (size_t)f.w * f.h;
    f.name = "injected " + f.name;
    f.negatives = true;
    f.rgb[0] = inf;                              // first pixel, R
    f.rgb[3 * (n - 1) + 2] = nan;                // last pixel, B
    f.rgb[3 * ((size_t)f.w - 1) + 1] = -inf;     // end of row 0, G
    f.rgb[3 * (2 * (size_t)f.w - 1) + 0] = -0.0f; // end of row 1
    f.rgb[3 * ((size_t)f.w) + 0] = -5.0f;        // start of row 1
    for (size_t k = 7; k < 3 * n; k += 97) f.rgb[k] = (k % 5 == 0) ? nan : (k % 5 == 1) ? inf : (k % 5 == 2) ? -inf : (k % 5 == 3) ? -f.rgb[k] : -0.0f;
    for (size_t p = 11; p < n; p += 53) f.rgb[3 * p] = f.rgb[3 * p + 1] = f.rgb[3 * p + 2] = -2.5f; // negative luminance
    return f;
}

static bool flag_word(uint32_t p) { return p == 0xff00ffffu || p == 0xffff0096u || p == 0xffffff00u; }

// the device image against the host's: equal, or with gamma within 1 per channel
static void compare_images(const std::string& what, const std::vector<uint32_t>& got, const std::vector<uint32_t>& want, bool gamma) {
    size_t wrong = 0, first = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        bool ok = got[i] == want[i];
        if (!ok && gamma && !flag_word(want[i]) && !flag_word(got[i]) && (got[i] >> 24) == (want[i] >> 24)) {
            ok = true;
            for (int s = 0; s < 24; s += 8) ok = ok && std::abs((int)((got[i] >> s) & 255) - (int)((want[i] >> s) & 255)) <= 1;
        }
        if (!ok && !wrong++) first = i;
    }
    CHECK(wrong == 0, "%s: %zu of %zu pixels differ, first %zu: %08x, host %08x", what.c_str(), wrong, want.size(), first, got[first], want[first]);
}

struct InfoRun {
    igx_imageinfo_output out{};
    std::vector<int32_t> hist[4];
};
static bool run_info(igx_device* dev, const float* d_film, int w, int h, float scale, int bins, InfoRun& r) {
    for (auto& v : r.hist) v.assign((size_t)(bins > 0 ? bins : 1), -1);
    const igx_imageinfo_settings is{scale, bins, r.hist[0].data(), r.hist[1].data(), r.hist[2].data(), r.hist[3].data(), 1, bins > 0};
    const igx_status st = igx_imageinfo_film(dev, d_film, w, h, &is, &r.out);
    CHECK(st == IGX_OK, "igx_imageinfo_film: %s", igx_last_error(dev));
    return st == IGX_OK;
}
static bool same_info(const InfoRun& a, const InfoRun& b) {
    bool same = std::memcmp(&a.out, &b.out, sizeof(a.out)) == 0;
    for (int c = 0; c < 4; ++c) same = same && a.hist[c] == b.hist[c];
    return same;
}

static void check_info(const std::string& what, const Film& f, float scale, int bins, const InfoRun& r) {
    const size_t n = (size_t)f.w * f.h;
    std::vector<int> hh[4];
    for (auto& v : hh) v.assign((size_t)(bins > 0 ? bins : 1), -1);
    const igx::FilmInfo host = igx::imageinfo_film(f.rgb.data(), f.w, f.h, scale, bins, hh[0].data(), hh[1].data(), hh[2].data(), hh[3].data(), true, bins > 0);
    const igx_imageinfo_output& o = r.out;
    std::printf("%s bins %d: min %.9g max %.9g avg %.9g soft %.9g %.9g median %.9g counts %d %d %d\n", what.c_str(), bins, o.min, o.max, o.avg, o.soft_min,
                o.soft_max, o.median, o.inf_count, o.nan_count, o.neg_count);
    CHECK(o.min == host.min && o.max == host.max, "%s: min / max %.9g %.9g, host %.9g %.9g", what.c_str(), o.min, o.max, host.min, host.max);
    CHECK(o.soft_min == host.soft_min && o.soft_max == host.soft_max, "%s: soft min / max %.9g %.9g, host %.9g %.9g", what.c_str(), o.soft_min, o.soft_max,
          host.soft_min, host.soft_max);
    CHECK(o.inf_count == host.inf_count && o.nan_count == host.nan_count && o.neg_count == host.neg_count, "%s: counts %d %d %d, host %d %d %d",
          what.c_str(), o.inf_count, o.nan_count, o.neg_count, host.inf_count, host.nan_count, host.neg_count);
    // avg and median against float64 sums of the same float32 terms
    auto fin = [&](size_t k) { const float a = f.rgb[k]; return std::isfinite(a) ? a : 0.0f; };
    std::vector<float> L(n);
    double sum = 0, sum_abs = 0;
    for (size_t i = 0; i < n; ++i) {
        L[i] = igx::srgb_to_xyY(igx::FilmColor{fin(3 * i) * scale, fin(3 * i + 1) * scale, fin(3 * i + 2) * scale}).b;
        sum += L[i];
        sum_abs += std::fabs(L[i]);
    }
    const double avg = sum / (double)n;
    const double bound = 1e-5 * (f.negatives ? sum_abs / (double)n : std::fabs(avg));
    CHECK(std::fabs(o.avg - avg) <= bound, "%s: avg %.9g, float64 %.9g (bound %.3g)", what.c_str(), o.avg, avg, bound);
    if (f.w > 10 && f.h > 10) {
        const float mf = igx::film_safe_div(1, (float)((size_t)(f.w - 2) * (f.h - 2)));
        double med = 0, med_abs = 0;
        for (int y = 1; y + 1 < f.h; ++y)
            for (int x = 1; x + 1 < f.w; ++x) {
                float win[9];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) win[3 * i + j] = L[(size_t)(y + i - 1) * f.w + (x + j - 1)];
                std::sort(win, win + 9);
                if (win[4] >= 0) med += (double)win[4] * (double)mf;
                med_abs += std::fabs((double)win[4]) * (double)mf;
            }
        const double mbound = 1e-5 * (f.negatives ? med_abs : std::fabs(med));
        CHECK(std::fabs(o.median - med) <= mbound, "%s: median %.9g, float64 %.9g (bound %.3g)", what.c_str(), o.median, med, mbound);
    } else {
        CHECK(o.median == o.avg && o.soft_min == o.min && o.soft_max == o.max, "%s: soft fallback", what.c_str());
    }
    for (int c = 0; c < 4 && bins > 0; ++c) {
        size_t wrong = 0, first = 0;
        long total = 0;
        for (int b = 0; b < bins; ++b) {
            total += r.hist[c][b];
            if (r.hist[c][b] != hh[c][b] && !wrong++) first = (size_t)b;
        }
        CHECK(wrong == 0, "%s: histogram %d: %zu of %d bins differ, bin %zu: %d, host %d", what.c_str(), c, wrong, bins, first, r.hist[c][first], hh[c][first]);
        CHECK(total == (long)n, "%s: histogram %d holds %ld of %zu", what.c_str(), c, total, n);
    }
}

// a lit plane: diffuse ground, point light (as tests/native/facade_members.cpp)
static igx_objscene* lit_plane() {
    igx_objscene* s = igx_objscene_create(nullptr);
    auto num = [&](int o, const char* k, float v) { igx_objscene_set_property(s, o, k, IGX_PROP_NUMBER, &v, 1); };
    auto vec3 = [&](int o, const char* k, float x, float y, float z) {
        const float v[3] = {x, y, z};
        igx_objscene_set_property(s, o, k, IGX_PROP_VECTOR3, v, 3);
    };
    auto str = [&](int o, const char* k, const char* v) { igx_objscene_set_property(s, o, k, IGX_PROP_STRING, v, 1); };
    int t = igx_objscene_add(s, IGX_OBJ_TECHNIQUE, "path", nullptr, nullptr);
    const int32_t depth = 3;
    igx_objscene_set_property(s, t, "max_depth", IGX_PROP_INTEGER, &depth, 1);
    int c = igx_objscene_add(s, IGX_OBJ_CAMERA, "perspective", nullptr, nullptr);
    num(c, "fov", 90);
    const float xf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1, 0, 0, 0, 1};
    igx_objscene_set_property(s, c, "transform", IGX_PROP_TRANSFORM, xf, 16);
    int f = igx_objscene_add(s, IGX_OBJ_FILM, "image", nullptr, nullptr);
    const float size[2] = {96, 64};
    igx_objscene_set_property(s, f, "size", IGX_PROP_VECTOR2, size, 2);
    int b = igx_objscene_add(s, IGX_OBJ_BSDF, "diffuse", "ground", nullptr);
    vec3(b, "reflectance", 0.8f, 0.5f, 0.3f);
    int sh = igx_objscene_add(s, IGX_OBJ_SHAPE, "rectangle", "Bottom", nullptr);
    num(sh, "width", 2);
    num(sh, "height", 2);
    const int32_t yes = 1;
    igx_objscene_set_property(s, sh, "flip_normals", IGX_PROP_BOOL, &yes, 1);
    int e = igx_objscene_add(s, IGX_OBJ_ENTITY, "", "Bottom", nullptr);
    str(e, "shape", "Bottom");
    str(e, "bsdf", "ground");
    int l = igx_objscene_add(s, IGX_OBJ_LIGHT, "point", "_light", nullptr);
    vec3(l, "position", 0, 0, -2);
    vec3(l, "intensity", 3, 3, 3);
    return s;
}

static int facade_case() {
    IG::Device::SetupSettings setup;
    IG::Device dev(setup);
    // before the first render: nothing to tonemap, all-zero statistics
    {
        uint32_t px[4] = {1, 2, 3, 4};
        const igx_tonemap_settings ts{1, 0, 1.0f, 1.0f, 0.0f};
        CHECK(igx_tonemap(dev.handle(), "", &ts, px, 4) == IGX_OK && px[0] == 1 && px[3] == 4, "tonemap before the first render");
        igx_imageinfo_output o{7, 7, 7, 7, 7, 7, 7, 7, 7};
        const igx_imageinfo_settings is{1.0f, 0, nullptr, nullptr, nullptr, nullptr, 1, 0};
        const igx_imageinfo_output zero{};
        CHECK(igx_imageinfo(dev.handle(), nullptr, &is, &o) == IGX_OK && std::memcmp(&o, &zero, sizeof(o)) == 0, "imageinfo before the first render");
    }
    igx_objscene* os = lit_plane();
    char err[512] = {0};
    igx_scene* sc = igx_scene_from_objects(os, err, sizeof(err));
    igx_objscene_free(os);
    if (!sc) {
        std::printf("FAIL: scene: %s\n", err);
        return 1;
    }
    IG::TechniqueVariantShaderSet shaders = IG::capture_shading(sc);
    IG::SceneDatabase db;
    igx_shading_view unused{};
    IG::serialize_scene(*igx_scene_get_desc(sc), db, unused);
    IG::Device::SceneSettings ss;
    ss.database = &db;
    dev.assignScene(ss);
    IG::Device::RenderSettings rs;
    rs.spi = 4;
    rs.width = 96;
    rs.height = 64;
    dev.render(shaders, rs);
    rs.iteration = 1;
    dev.render(shaders, rs);
    const size_t n = 96 * 64;
    IG::Device::AOVAccessor fb = dev.getFramebufferForHost("");
    CHECK(fb.Data && fb.IterationCount == 2, "film");
    if (!fb.Data) return 1;
    Film film{"facade film", 96, 64, std::vector<float>(fb.Data, fb.Data + n * 3)};
    const float scale = 1.0f * (1.0f / 2.0f);

    std::vector<uint32_t> px(n, 0xdeadbeefu), want(n);
    dev.tonemap(px.data(), IG::TonemapSettings{"", 2, false, 1.0f, 1.0f, 0.0f});
    igx::tonemap_film(film.rgb.data(), n, scale, 2, false, 1.0f, 0.0f, want.data());
    compare_images("facade tonemap", px, want, false);
    size_t lit = 0;
    for (uint32_t p : px) lit += (p & 0xffffffu) != 0;
    CHECK(lit > 100, "facade tonemap: %zu lit pixels", lit);

    InfoRun r;
    for (auto& v : r.hist) v.assign(16, -1);
    IG::ImageInfoSettings is{"Color", 1.0f, 16, r.hist[0].data(), r.hist[1].data(), r.hist[2].data(), r.hist[3].data(), true, true};
    const IG::ImageInfoOutput io = dev.imageinfo(is);
    r.out = igx_imageinfo_output{io.Min, io.Max, io.Average, io.SoftMin, io.SoftMax, io.Median, io.InfCount, io.NaNCount, io.NegCount};
    check_info("facade imageinfo", film, scale, 16, r);

    // an unknown AOV: the output stays as it was, the statistics are zero
    std::vector<uint32_t> keep(n, 0xdeadbeefu);
    dev.tonemap(keep.data(), IG::TonemapSettings{"Normals", 1, false, 1.0f, 1.0f, 0.0f});
    CHECK(keep[0] == 0xdeadbeefu && keep[n - 1] == 0xdeadbeefu, "tonemap of an unknown AOV wrote its output");
    IG::ImageInfoSettings unk{"Normals", 1.0f, 0, nullptr, nullptr, nullptr, nullptr, true, false};
    const IG::ImageInfoOutput uo = dev.imageinfo(unk);
    CHECK(uo.Min == 0 && uo.Max == 0 && uo.Average == 0 && uo.InfCount == 0, "imageinfo of an unknown AOV");
    // the C-ABI itself: unknown name and size mismatch are errors
    const igx_tonemap_settings ts{1, 0, 1.0f, 1.0f, 0.0f};
    CHECK(igx_tonemap(dev.handle(), "Bogus", &ts, keep.data(), n) == IGX_ERR_INVALID_ARGUMENT &&
              std::strstr(igx_last_error(dev.handle()), "unknown aov"),
          "igx_tonemap with an unknown name: %s", igx_last_error(dev.handle()));
    igx_imageinfo_output o{};
    const igx_imageinfo_settings cis{1.0f, 0, nullptr, nullptr, nullptr, nullptr, 1, 0};
    CHECK(igx_imageinfo(dev.handle(), "Bogus", &cis, &o) == IGX_ERR_INVALID_ARGUMENT && std::strstr(igx_last_error(dev.handle()), "unknown aov"),
          "igx_imageinfo with an unknown name");
    CHECK(igx_tonemap(dev.handle(), "", &ts, keep.data(), n - 1) == IGX_ERR_INVALID_ARGUMENT, "igx_tonemap with a wrong pixel count");
    CHECK(keep[0] == 0xdeadbeefu, "a refused igx_tonemap wrote its output");
    dev.releaseAll();
    igx_scene_free(sc);
    return 0;
}

int main() {
    igx_device* dev = nullptr;
    if (igx_create(0, &dev) != IGX_OK) {
        std::printf("FAIL: igx_create\n");
        return 1;
    }
    std::vector<Film> films;
    const int sizes[7][2] = {{1, 1}, {3, 2}, {10, 40}, {11, 11}, {67, 13}, {257, 129}, {640, 360}};
    for (int k = 0; k < 7; ++k) films.push_back(tailed(sizes[k][0], sizes[k][1], 1234u + (uint32_t)k));
    films.push_back(constant(67, 13, 0.0f));
    films.push_back(constant(67, 13, 0.75f));
    films.push_back(constant(3, 2, 2.0f));
    films.push_back(injected(tailed(67, 13, 77u)));
    films.push_back(injected(tailed(257, 129, 78u)));
    const int LDS_BINS_ABOVE = 4096; // 4 * 4096 ints = 64 KB: above the kernels' 32 KB LDS budget, global atomics
    const int bin_counts[4] = {1, 16, 255, LDS_BINS_ABOVE};
    const float scale = 0.5f, ef = 0.7f, eo = 0.01f;

    for (const Film& f : films) {
        const size_t n = (size_t)f.w * f.h;
        // the film twice: 16-byte aligned, and one float further (the scalar paths)
        float* d_film = nullptr;
        uint32_t* d_out = nullptr;
        HIP(hipMalloc((void**)&d_film, (n * 3 + 4) * sizeof(float) * 2));
        HIP(hipMalloc((void**)&d_out, (n + 4) * sizeof(uint32_t)));
        float* d_aligned = d_film;
        float* d_odd = d_film + n * 3 + 4 - (n * 3) % 4 + 1; // 4 bytes past a 16-byte boundary
        HIP(hipMemcpy(d_aligned, f.rgb.data(), n * 3 * sizeof(float), hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_odd, f.rgb.data(), n * 3 * sizeof(float), hipMemcpyHostToDevice));
        CHECK(((uintptr_t)d_aligned & 15) == 0 && ((uintptr_t)d_odd & 15) == 4, "test pointers: alignment");

        std::vector<uint32_t> want(n), got(n);
        for (int method = 0; method < 5; ++method)
            for (int gamma = 0; gamma < 2; ++gamma) {
                igx::tonemap_film(f.rgb.data(), n, scale, method, gamma != 0, ef, eo, want.data());
                const igx_tonemap_settings ts{method, gamma, scale, ef, eo};
                const std::string what = f.name + " method " + std::to_string(method) + (gamma ? " gamma" : "");
                // host output
                std::fill(got.begin(), got.end(), 0u);
                CHECK(igx_tonemap_film(dev, d_aligned, f.w, f.h, &ts, got.data(), 0) == IGX_OK, "%s: %s", what.c_str(), igx_last_error(dev));
                compare_images(what + " (host output)", got, want, gamma != 0);
                // device output, copied back here
                HIP(hipMemset(d_out, 0, (n + 4) * sizeof(uint32_t)));
                CHECK(igx_tonemap_film(dev, d_aligned, f.w, f.h, &ts, d_out, 1) == IGX_OK, "%s: %s", what.c_str(), igx_last_error(dev));
                HIP(hipMemcpy(got.data(), d_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
                compare_images(what + " (device output)", got, want, gamma != 0);
                // a film and an output that are not 16-byte aligned
                HIP(hipMemset(d_out, 0, (n + 4) * sizeof(uint32_t)));
                CHECK(igx_tonemap_film(dev, d_odd, f.w, f.h, &ts, d_out + 1, 1) == IGX_OK, "%s: %s", what.c_str(), igx_last_error(dev));
                HIP(hipMemcpy(got.data(), d_out + 1, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
                compare_images(what + " (unaligned)", got, want, gamma != 0);
                uint32_t edge[2] = {1, 1};
                HIP(hipMemcpy(&edge[0], d_out, sizeof(uint32_t), hipMemcpyDeviceToHost));
                HIP(hipMemcpy(&edge[1], d_out + 1 + n, sizeof(uint32_t), hipMemcpyDeviceToHost));
                CHECK(edge[0] == 0 && edge[1] == 0, "%s: wrote outside the image", what.c_str());
            }
        for (int bins : bin_counts) {
            InfoRun r, odd;
            if (run_info(dev, d_aligned, f.w, f.h, scale, bins, r)) check_info(f.name, f, scale, bins, r);
            if (bins == 16 && run_info(dev, d_odd, f.w, f.h, scale, bins, odd)) CHECK(same_info(r, odd), "%s: the unaligned film gives another result", f.name.c_str());
        }
        // statistics only (no histogram, no error counts)
        {
            igx_imageinfo_output o{};
            const igx_imageinfo_settings is{scale, 0, nullptr, nullptr, nullptr, nullptr, 0, 0};
            CHECK(igx_imageinfo_film(dev, d_aligned, f.w, f.h, &is, &o) == IGX_OK, "%s: %s", f.name.c_str(), igx_last_error(dev));
            CHECK(o.inf_count == 0 && o.nan_count == 0 && o.neg_count == 0, "%s: counts without acquire_error_stats", f.name.c_str());
        }
        HIP(hipFree(d_film));
        HIP(hipFree(d_out));
    }

    // determinism, and scratch growth: small, large, small again on one handle
    {
        const Film &small = films[4], &large = films[6];
        float *d_small = nullptr, *d_large = nullptr;
        HIP(hipMalloc((void**)&d_small, small.rgb.size() * sizeof(float)));
        HIP(hipMalloc((void**)&d_large, large.rgb.size() * sizeof(float)));
        HIP(hipMemcpy(d_small, small.rgb.data(), small.rgb.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_large, large.rgb.data(), large.rgb.size() * sizeof(float), hipMemcpyHostToDevice));
        igx_device* fresh = nullptr;
        CHECK(igx_create(0, &fresh) == IGX_OK, "second handle");
        InfoRun s1, l1, l2, s2;
        if (fresh && run_info(fresh, d_small, small.w, small.h, scale, 255, s1) && run_info(fresh, d_large, large.w, large.h, scale, 255, l1) &&
            run_info(fresh, d_large, large.w, large.h, scale, 255, l2) && run_info(fresh, d_small, small.w, small.h, scale, 255, s2)) {
            CHECK(same_info(l1, l2), "two imageinfo calls on the 640x360 film differ");
            CHECK(same_info(s1, s2), "the small film's result changed after the scratch grew");
            check_info("after growth", small, scale, 255, s2);
            std::vector<uint32_t> a(small.rgb.size() / 3), b(large.rgb.size() / 3), c(a.size()), want(a.size());
            const igx_tonemap_settings ts{3, 0, scale, ef, eo};
            CHECK(igx_tonemap_film(fresh, d_small, small.w, small.h, &ts, a.data(), 0) == IGX_OK &&
                      igx_tonemap_film(fresh, d_large, large.w, large.h, &ts, b.data(), 0) == IGX_OK &&
                      igx_tonemap_film(fresh, d_small, small.w, small.h, &ts, c.data(), 0) == IGX_OK,
                  "tonemap growth: %s", igx_last_error(fresh));
            igx::tonemap_film(small.rgb.data(), a.size(), scale, 3, false, ef, eo, want.data());
            CHECK(a == want && c == want, "the small image changed after the scratch grew");
        }
        if (fresh) igx_destroy(fresh);
        HIP(hipFree(d_small));
        HIP(hipFree(d_large));
    }
    igx_destroy(dev);

    try {
        if (facade_case()) return 1;
    } catch (const std::exception& e) {
        std::printf("FAIL: facade: %s\n", e.what());
        ++bad;
    }
    std::printf(bad ? "failed\n" : "ok\n");
    return bad ? 1 : 0;
}
