// IG::Device::evaluateGlare through the header-only facade host/Device.h
// (tests/test_glare_gpu.py compiles it with g++ against libigx.so and runs it
// on the GPU): a lit plane seen through a fishlens camera, rendered with a
// shader set that carries the glare shader (GlareEnabled) and with one that
// does not.  Prints "ok" when every check passed.
#include "Device.h"
#include "igx_scene.h"
#include "scene_database.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                \
            ++bad;                            \
        }                                     \
    } while (0)

// diffuse ground under a point light, fishlens camera looking at it
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
    int c = igx_objscene_add(s, IGX_OBJ_CAMERA, "fishlens", nullptr, nullptr);
    const float xf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1, 0, 0, 0, 1};
    igx_objscene_set_property(s, c, "transform", IGX_PROP_TRANSFORM, xf, 16);
    int f = igx_objscene_add(s, IGX_OBJ_FILM, "image", nullptr, nullptr);
    const float size[2] = {64, 64};
    igx_objscene_set_property(s, f, "size", IGX_PROP_VECTOR2, size, 2);
    int b = igx_objscene_add(s, IGX_OBJ_BSDF, "diffuse", "ground", nullptr);
    vec3(b, "reflectance", 0.8f, 0.8f, 0.8f);
    int sh = igx_objscene_add(s, IGX_OBJ_SHAPE, "rectangle", "Bottom", nullptr);
    num(sh, "width", 2);
    num(sh, "height", 2);
    const int32_t yes = 1;
    igx_objscene_set_property(s, sh, "flip_normals", IGX_PROP_BOOL, &yes, 1);
    int e = igx_objscene_add(s, IGX_OBJ_ENTITY, "", "Bottom", nullptr);
    str(e, "shape", "Bottom");
    str(e, "bsdf", "ground");
    int l = igx_objscene_add(s, IGX_OBJ_LIGHT, "point", "_light", nullptr);
    vec3(l, "position", 0, 0, -0.5f);
    vec3(l, "intensity", 3, 3, 3);
    return s;
}

int main() {
    IG::Device dev(IG::Device::SetupSettings{});
    igx_objscene* os = lit_plane();
    char err[512] = {0};
    igx_scene* sc = igx_scene_from_objects(os, err, sizeof(err));
    igx_objscene_free(os);
    if (!sc) {
        std::printf("FAIL: scene: %s\n", err);
        return 1;
    }
    IG::TechniqueVariantShaderSet shaders = IG::capture_shading(sc);
    CHECK(!shaders.GlareEnabled, "capture_shading switched the glare shader on");
    IG::SceneDatabase db;
    igx_shading_view unused{};
    IG::serialize_scene(*igx_scene_get_desc(sc), db, unused);
    IG::Device::SceneSettings ss;
    ss.database = &db;
    dev.assignScene(ss);
    IG::Device::RenderSettings rs;
    rs.spi = 4;
    rs.width = 64;
    rs.height = 64;

    // the threshold from imageinfo, as the viewer does (UI.cpp:651)
    const uint32_t mark = 0xdeadbeefu;
    std::vector<uint32_t> px(64 * 64, mark);
    auto settings = [&] {
        const IG::ImageInfoOutput io = dev.imageinfo(IG::ImageInfoSettings{"", 1.0f, 0, nullptr, nullptr, nullptr, nullptr, false, false});
        return IG::GlareSettings{"", 1.0f, io.SoftMax, io.Average, 2.0f, -1.0f};
    };

    // without the glare shader: the empty result, the image untouched
    dev.render(shaders, rs);
    IG::GlareOutput off = dev.evaluateGlare(px.data(), settings());
    size_t touched = 0;
    for (uint32_t p : px) touched += p != mark;
    CHECK(off.DGP == 0 && off.NumPixels == 0 && off.VerticalIlluminance == 0 && touched == 0, "evaluateGlare without GlareEnabled: dgp %g, %zu words",
          off.DGP, touched);

    // with it
    shaders.GlareEnabled = true;
    dev.render(shaders, rs);
    IG::GlareOutput on = dev.evaluateGlare(px.data(), settings());
    touched = 0;
    size_t opaque = 0;
    for (uint32_t p : px) {
        touched += p != mark;
        opaque += p != mark && (p >> 24) == 255u;
    }
    std::printf("glare: dgp %g ev %g avg_lum %g omega %g pixels %d\n", on.DGP, on.VerticalIlluminance, on.AvgLum, on.AvgOmega, on.NumPixels);
    CHECK(on.NumPixels > 0 && (size_t)on.NumPixels == touched && opaque == touched, "source pixels %d, overlay words %zu (%zu opaque)", on.NumPixels,
          touched, opaque);
    CHECK(on.VerticalIlluminance > 0 && on.AvgLum > 0 && on.AvgOmega > 0 && on.AvgOmega < 6.3f, "glare sums");
    CHECK(std::isfinite(on.DGP) && on.DGP > 0.16f, "dgp %g", on.DGP);
    // a null image and a given vertical illuminance
    IG::GlareSettings gs = settings();
    gs.VerticalIlluminance = 1234.5f;
    IG::GlareOutput fixed = dev.evaluateGlare(nullptr, gs);
    CHECK(fixed.VerticalIlluminance == 1234.5f && fixed.NumPixels == on.NumPixels && fixed.AvgLum == on.AvgLum, "given vertical illuminance");
    // an unknown AOV: the empty result
    IG::GlareOutput unk = dev.evaluateGlare(nullptr, IG::GlareSettings{"Bogus", 1, 1, 1, 5, -1});
    CHECK(unk.DGP == 0 && unk.NumPixels == 0, "unknown AOV");

    dev.releaseAll();
    igx_scene_free(sc);
    std::printf(bad ? "failed\n" : "ok\n");
    return bad ? 1 : 0;
}
