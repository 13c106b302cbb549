// host/glare_model.h (the arithmetic of the daylight glare kernel) against
// closed forms and float64 restatements.  Stand-alone: no libigx, no GPU.
// Prints its measurements, then "ok".
//
// The per-pixel bound GLARE_OMEGA_BOUND on |glare_omega (float) - the float64
// evaluation of the same four corners|, by counting rounded operations with
// u = 2^-24 = 5.96e-8:
//   * a plane normal: e2 = b - a (each component within u of its value), the
//     cross product (per component two products and a difference, 3 u |e2|;
//     as a vector 5.2 u |e2| against a length of about |e2|), the
//     normalisation (one more rounding per component): its direction is off by
//     at most 8 u;
//   * a dot product of two normals (near 0, the angles are near pi / 2): the
//     two normals' 16 u and 2 u for its own three products and two additions,
//     18 u = 1.07e-6; acos has slope 1 there;
//   * acos itself, 2 ulp of a value near 1.57 (ulp 1.19e-7): 2.4e-7;
//   * pi - acos, a value near 1.57: half an ulp, 0.6e-7;
//     so an interior angle is within 1.37e-6, the four within 5.5e-6;
//   * their three additions, results near pi, 3 pi / 2 and 2 pi: half ulps of
//     1.2e-7, 2.4e-7 and 2.4e-7, 6e-7; the subtraction of 2 pi is exact;
//   * flt_pi is 8.74e-8 above pi, and 4 flt_pi - 2 flt_pi carries it twice:
//     1.75e-7 (the float64 side uses pi).
// Together 6.3e-6; asserted as 6.5e-6.  (Correctly rounded float32 reaches
// 0.7e-6 .. 0.9e-6 on these shapes.)
//
// The whole-film bound: a perspective film's pixel edges are great-circle
// arcs, so the pixels tile the view pyramid and sum omega = 4 asin(tx ty /
// sqrt((1 + tx^2)(1 + ty^2))).  Over N pixels the flt_pi term is a bias,
// N * 1.75e-7; the rest varies from pixel to pixel with the per-pixel bound as
// an upper limit of its spread, sqrt(N) * 6.5e-6.  The float corners move the
// pyramid's own edges by a relative 1e-7, which is nothing beside it.  (The
// worst case N * 6.5e-6 would be 1.4 % of the sum at 48 x 32 and could not
// tell a corner from a centre, which moves the sum by about 1 / w.)
#include "glare_model.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace igx;
using igxd::CameraModel;

static int failures = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                               \
            std::printf(__VA_ARGS__);                                                                                \
            std::printf("\n");                                                                                       \
            ++failures;                                                                                              \
        }                                                                                                            \
    } while (0)

constexpr double GLARE_OMEGA_BOUND = 6.5e-6;
constexpr double PI = 3.14159265358979323846;

struct V3 { double x, y, z; };
static V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V3 norm(V3 a) { const double l = std::sqrt(dot(a, a)); return V3{a.x / l, a.y / l, a.z / l}; }
static V3 wide(CamVec v) { return V3{v.x, v.y, v.z}; }
static V3 splane64(V3 a, V3 b) {
    const V3 n = cross(a, sub(b, a));
    return dot(n, n) > 0 ? norm(n) : V3{0, 0, 0};
}
static double omega64(V3 r1, V3 r2, V3 r3, V3 r4) {
    const V3 n1 = splane64(r1, r2), n2 = splane64(r2, r3), n3 = splane64(r3, r4), n4 = splane64(r4, r1);
    return (PI - std::acos(dot(n1, n2))) + (PI - std::acos(dot(n2, n3))) + (PI - std::acos(dot(n3, n4))) + (PI - std::acos(dot(n4, n1))) -
           2 * PI;
}

// cameras looking down -z with +y up, as the tests' scenes do
static igx_camera base_camera(int type) {
    igx_camera c{};
    c.dir[2] = -1;
    c.up[1] = 1;
    c.fov = (float)(60.0 * PI / 180.0);
    c.near_clip = 0.01f;
    c.far_clip = 100;
    c.type = type;
    c.ortho_scale = 2;
    return c;
}
// the same cameras' direction at a lattice point in float64 (right = +x)
static V3 dir64(int type, int w, int h, int x, int y) {
    const double nx = 2.0 * x / w - 1, ny = 1 - 2.0 * y / h, aspect = (double)w / h;
    if (type == IGX_CAMERA_FISHLENS) {
        const double fx = nx * (aspect < 1 ? 1 : aspect), fy = ny * (aspect > 1 ? 1 : aspect);
        const double r = std::sqrt(fx * fx + fy * fy), th = r * PI / 2;
        if (r == 0) return V3{0, 0, -1};
        return norm(V3{std::sin(th) * fx / r, std::sin(th) * fy / r, -std::cos(th)});
    }
    const double tx = std::tan(30.0 * PI / 180.0);
    return norm(V3{tx * nx, tx / aspect * ny, -1});
}
static double posindex64(int type, int w, int h, int px, int py, bool* iwata) {
    const V3 d = dir64(type, w, h, px, py), up{0, 1, 0}, dir{0, 0, -1}, right = cross(dir, up);
    double phi = std::acos(dot(up, d)) - PI / 2, theta = PI / 2 - std::acos(dot(right, d)), sigma = std::acos(dot(dir, d));
    const double t = std::cos(sigma);
    const V3 hv = norm(sub(V3{d.x / t, d.y / t, d.z / t}, d));
    double tau = std::acos(dot(up, hv)) * 180 / PI;
    if (phi == 0) phi = 0.00001;
    if (theta == 0) theta = 0.0001;
    sigma = std::fabs(sigma) * 180 / PI;
    double p = std::exp((35.2 - 0.31889 * tau - 1.22 * std::exp(-2 * tau / 9)) / 1000 * sigma +
                        (21 + 0.26667 * tau - 0.002963 * tau * tau) / 100000 * sigma * sigma);
    *iwata = phi < 0;
    if (phi < 0) {
        const double dd = 1 / std::tan(phi), s = std::tan(theta) / std::tan(phi);
        double r = std::sqrt(1 / dd / dd + s * s / dd / dd), fact = 0.8;
        if (r > 0.6) fact = 1.2;
        if (r > 3) r = 3;
        p = 1 + fact * r;
    }
    return p;
}

static void check_film(const char* name, int type, int w, int h, bool tiling) {
    const CameraModel m = igxd::make_camera_model(base_camera(type), w, h);
    double worst = 0, sum32 = 0, sum64 = 0, lo = 1e30, hi = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const CamVec r1 = glare_pixel_dir(m, w, h, x, y), r2 = glare_pixel_dir(m, w, h, x, y + 1),
                         r3 = glare_pixel_dir(m, w, h, x + 1, y + 1), r4 = glare_pixel_dir(m, w, h, x + 1, y);
            const double o32 = glare_omega(r1, r2, r3, r4), o64 = omega64(wide(r1), wide(r2), wide(r3), wide(r4));
            worst = std::fmax(worst, std::fabs(o32 - o64));
            sum32 += o32;
            sum64 += o64;
            lo = std::fmin(lo, o64);
            hi = std::fmax(hi, o64);
            // the float corner is the float64 restatement's corner
            const V3 e = sub(wide(r1), dir64(type, w, h, x, y));
            CHECK(std::sqrt(dot(e, e)) < 1e-6, "%s corner (%d, %d) off by %g", name, x, y, std::sqrt(dot(e, e)));
        }
    std::printf("%-18s %3d x %3d  worst |omega32 - omega64| %.3g  omega in [%.3g, %.3g]  sum %.9g (float64 corners %.9g)\n", name, w, h,
                worst, lo, hi, sum32, sum64);
    CHECK(worst <= GLARE_OMEGA_BOUND, "%s %dx%d per-pixel error %g", name, w, h, worst);
    if (tiling) {
        const double tx = std::tan(30.0 * PI / 180.0), ty = tx * h / w;
        const double closed = 4 * std::asin(tx * ty / std::sqrt((1 + tx * tx) * (1 + ty * ty)));
        const double n = (double)w * h, bound = n * 1.75e-7 + std::sqrt(n) * GLARE_OMEGA_BOUND;
        std::printf("%-18s closed form %.9g  float32 off by %.3g (relative %.3g), bound %.3g\n", "", closed, sum32 - closed,
                    std::fabs(sum32 - closed) / closed, bound);
        CHECK(std::fabs(sum64 - closed) < 1e-6 * closed, "float64 tiling %g vs %g", sum64, closed);
        CHECK(std::fabs(sum32 - closed) <= bound, "float32 tiling %g vs %g", sum32, closed);
    }
}

static void check_posindex() {
    const int F = IGX_CAMERA_FISHLENS, P = IGX_CAMERA_PERSPECTIVE;
    // difference 2: the view direction itself
    CHECK(glare_posindex(igxd::make_camera_model(base_camera(F), 64, 64), 64, 64, 32, 32) == 1.0f, "fishlens centre");
    CHECK(glare_posindex(igxd::make_camera_model(base_camera(P), 48, 32), 48, 32, 24, 16) == 1.0f, "perspective centre");
    // two lattice points per branch against float64
    struct { int type, w, h, x, y; bool iwata; } pts[] = {
        {F, 64, 64, 40, 44, false}, {F, 96, 64, 60, 40, false}, // lower half: Guth
        {F, 64, 64, 40, 20, true},  {P, 67, 45, 11, 7, true},   // upper half: Iwata
    };
    for (const auto& p : pts) {
        bool iwata = false;
        const double want = posindex64(p.type, p.w, p.h, p.x, p.y, &iwata);
        const float got = glare_posindex(igxd::make_camera_model(base_camera(p.type), p.w, p.h), p.w, p.h, p.x, p.y);
        std::printf("posindex type %d %dx%d (%d, %d) %s: %.8g, float64 %.8g\n", p.type, p.w, p.h, p.x, p.y, iwata ? "Iwata" : "Guth", got,
                    want);
        CHECK(iwata == p.iwata, "branch at (%d, %d)", p.x, p.y);
        CHECK(want > 0.5 && want != 1 && want < 16, "hand-picked point (%d, %d) gives %g", p.x, p.y, want);
        CHECK(std::fabs(got - want) <= 1e-5 * want, "posindex %g vs %g", got, want);
    }
    // the cap: far outside the image circle of a 96 x 64 fishlens film, just below the horizon
    bool iwata = true;
    const double raw = posindex64(F, 96, 64, 96, 33, &iwata);
    CHECK(!iwata && raw > 16, "uncapped value %g", raw);
    CHECK(glare_posindex(igxd::make_camera_model(base_camera(F), 96, 64), 96, 64, 96, 33) == 16.0f, "cap");
}

static void check_overlay() {
    const igx_glare_settings set{1.0f, 3.0f, 1.0f, 1.0f, -1.0f};
    const float src = glare_lum_source(set), mx = glare_lum_max(set);
    CHECK(src == 179.0f && mx == 537.0f, "levels %g %g", src, mx);
    const double c[7][3] = {{0.0002189403691192265, 0.001651004631001012, -0.01948089843709184},
                            {0.1065134194856116, 0.5639564367884091, 3.932712388889277},
                            {11.60249308247187, -3.972853965665698, -15.9423941062914},
                            {-41.70399613139459, 17.43639888205313, 44.35414519872813},
                            {77.162935699427, -33.40235894210092, -81.80730925738993},
                            {-71.31942824499214, 32.62606426397723, 73.20951985803202},
                            {25.13112622477341, -12.24266895238567, -23.07032500287172}};
    for (double f : {0.0, 0.5, 1.0, 1.75}) {
        const uint32_t word = glare_overlay((float)(179.0 + f * 358.0), src, mx);
        const double t = std::fmin(1.0, f * f);
        CHECK(word >> 24 == 255, "alpha of %08x", word);
        for (int k = 0; k < 3; ++k) {
            double v = 0;
            for (int i = 6; i >= 0; --i) v = c[i][k] + v * t;
            const int want = (int)(std::fmin(std::fmax(v, 0.0), 1.0) * 255), got = (word >> (16 - 8 * k)) & 255;
            CHECK(std::abs(got - want) <= 1, "f %g channel %d: %d vs %d", f, k, got, want);
        }
    }
    CHECK(glare_overlay(179.0f + 358.0f, src, mx) == glare_overlay(179.0f + 2 * 358.0f, src, mx), "beyond 1 clamps");
}

static void check_finish_and_host() {
    const int w = 67, h = 45;
    const CameraModel m = igxd::make_camera_model(base_camera(IGX_CAMERA_FISHLENS), w, h);
    igx_glare_settings set{1.0f, 8.0f, 0.25f, 5.0f, -1.0f};
    // no source (difference 1)
    GlareSums none{1000.0f, 0, 0, 0, 0, 0};
    igx_glare_output o = glare_finish(none, set, m, w, h);
    CHECK(o.num_pixels == 0 && o.avg_lum == 0 && o.avg_omega == 0 && o.vertical_illuminance == 1000.0f, "no-source output");
    CHECK(std::fabs(o.dgp - (5.87e-5f * 1000.0f + 0.16f)) < 1e-6f, "no-source dgp %g", o.dgp);
    // a given vertical illuminance passes through
    set.vertical_illuminance = 1234.5f;
    o = glare_finish(none, set, m, w, h);
    CHECK(o.vertical_illuminance == 1234.5f, "given E_v");
    GlareSums some{1000.0f, 4, 0.01f, 0.01f * 1432.0f, 30.5f * 0.01f, 30.5f * 0.01f}; // centre (30.5, 30.5): lattice point (30, 30)
    o = glare_finish(some, set, m, w, h);
    CHECK(o.vertical_illuminance == 1234.5f && o.num_pixels == 4 && o.avg_omega == 0.01f && std::fabs(o.avg_lum - 1432.0f) < 1e-3f,
          "source output");
    bool iw = false;
    const double posi = posindex64(IGX_CAMERA_FISHLENS, w, h, 30, 30, &iw);
    const double dgp = 5.87e-5 * 1234.5 + 0.0981 * std::log10(1 + 1432.0 * 1432.0 / (posi * posi) * 0.01 / std::pow(1234.5, 1.87)) + 0.16;
    CHECK(std::fabs(o.dgp - dgp) < 1e-5, "dgp %g vs %g", o.dgp, dgp);

    // glare_host: a 4 x 2 source on a grey film; the overlay keeps every other word
    set.vertical_illuminance = -1;
    std::vector<float> film((size_t)w * h * 3, 0.25f);
    int count = 0;
    for (int y = 10; y < 12; ++y)
        for (int x = 20; x < 24; ++x, ++count)
            for (int k = 0; k < 3; ++k) film[((size_t)y * w + x) * 3 + k] = 8.0f;
    std::vector<uint32_t> overlay((size_t)w * h, 0xdeadbeefu);
    glare_host(film.data(), w, h, m, set, overlay.data(), &o);
    int written = 0;
    for (size_t i = 0; i < overlay.size(); ++i) written += overlay[i] != 0xdeadbeefu;
    CHECK(o.num_pixels == count && written == count, "source pixels %d, words %d", o.num_pixels, written);
    CHECK(overlay[(size_t)10 * w + 20] == glare_overlay(179 * 8.0f, glare_lum_source(set), glare_lum_max(set)), "overlay word");
    CHECK(std::fabs(o.avg_lum - 179 * 8.0) < 1e-2 && o.avg_omega > 0 && o.dgp > 0.16f && std::isfinite(o.dgp), "host output");
    igx_glare_output again{};
    glare_host(film.data(), w, h, m, set, nullptr, &again);
    CHECK(again.dgp == o.dgp && again.vertical_illuminance == o.vertical_illuminance, "same bits without an overlay");
    std::printf("glare_host 67 x 45: dgp %.7g ev %.7g avg_lum %.7g omega %.7g pixels %d\n", o.dgp, o.vertical_illuminance, o.avg_lum,
                o.avg_omega, o.num_pixels);

    // orthogonal camera: every direction is the view direction, every omega 0
    const CameraModel om = igxd::make_camera_model(base_camera(IGX_CAMERA_ORTHOGONAL), 8, 6);
    for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 8; ++x)
            CHECK(glare_omega(glare_pixel_dir(om, 8, 6, x, y), glare_pixel_dir(om, 8, 6, x, y + 1), glare_pixel_dir(om, 8, 6, x + 1, y + 1),
                              glare_pixel_dir(om, 8, 6, x + 1, y)) == 0.0f,
                  "orthogonal omega at (%d, %d)", x, y);
    // a depth-of-field camera evaluates as its pinhole (difference 3): the lens centre, so d * f normalised again
    igx_camera dof = base_camera(IGX_CAMERA_PERSPECTIVE);
    dof.aperture_radius = 0.05f;
    dof.focal_length = 3;
    const CameraModel dm = igxd::make_camera_model(dof, 67, 45), pm = igxd::make_camera_model(base_camera(IGX_CAMERA_PERSPECTIVE), 67, 45);
    CHECK(igxd::camera_has_dof(dm.lens), "the depth-of-field model");
    for (int y = 0; y <= 45; y += 5)
        for (int x = 0; x <= 67; ++x) {
            const CamVec a = glare_pixel_dir(dm, 67, 45, x, y), b = glare_pixel_dir(pm, 67, 45, x, y);
            CHECK(std::fabs(a.x - b.x) <= 2e-7f && std::fabs(a.y - b.y) <= 2e-7f && std::fabs(a.z - b.z) <= 2e-7f, "dof corner (%d, %d)", x, y);
        }
    std::vector<float> bright(8 * 6 * 3, 8.0f);
    glare_host(bright.data(), 8, 6, om, set, nullptr, &o);
    CHECK(o.num_pixels == 48 && o.avg_lum == 0 && o.avg_omega == 0 && o.vertical_illuminance == 0 && o.dgp == 0.16f, "orthogonal: nothing divides by omega");
}

int main() {
    check_film("perspective", IGX_CAMERA_PERSPECTIVE, 48, 32, true);
    check_film("perspective", IGX_CAMERA_PERSPECTIVE, 67, 45, true);
    check_film("fishlens", IGX_CAMERA_FISHLENS, 64, 64, false);
    check_film("fishlens", IGX_CAMERA_FISHLENS, 96, 64, false);
    check_film("fishlens", IGX_CAMERA_FISHLENS, 67, 45, false);
    check_posindex();
    check_overlay();
    check_finish_and_host();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
