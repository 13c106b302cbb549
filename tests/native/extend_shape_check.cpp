// pick_extend_shape (host/extend_shape.h) over the option grid: a launch gets
// a specialised shape of k_extend exactly when it runs the default fused mode
// (dynamic groups front to back, path_classes 4, shadow classes, no ray list,
// no MIS AOVs, not instrumented) and the option allows it; the generate shape
// goes to launches that build their camera paths (gen_n > 0) and to no other.
#include "extend_shape.h"

#include <cstdio>
#include <initializer_list>

using namespace igxh;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);       \
            ++failures;                                            \
        }                                                          \
    } while (0)

// a launch of the default fused mode
static ExtendShapeInput fused(int gen_n) {
    ExtendShapeInput in;
    in.extend_shapes = 1;
    in.gen_n = gen_n;
    in.dynamic = 1;
    in.reverse = 0;
    in.classify = 4;
    in.shadow_classes = 1;
    return in;
}

int main() {
    // the whole grid against the rule written out
    long cases = 0, shaped = 0;
    for (int opt = -1; opt <= 1; ++opt)
    for (int inst = 0; inst <= 1; ++inst)
    for (int gen_n : {0, 1, 64, 8192, 1 << 27})
    for (int dynamic = 0; dynamic <= 1; ++dynamic)
    for (int reverse = 0; reverse <= 1; ++reverse)
    for (int classify = 0; classify <= 4; ++classify)
    for (int shadow_classes = 0; shadow_classes <= 1; ++shadow_classes)
    for (int num_rays : {0, 1, 4096})
    for (int aov = 0; aov <= 1; ++aov) {
        ExtendShapeInput in;
        in.extend_shapes = opt;
        in.instrument = inst != 0;
        in.gen_n = gen_n;
        in.dynamic = dynamic;
        in.reverse = reverse;
        in.classify = classify;
        in.shadow_classes = shadow_classes;
        in.num_rays = num_rays;
        in.mis_aovs = aov != 0;
        const bool on = opt < 0 ? EXTEND_SHAPES_AUTO != 0 : opt != 0;
        const bool eligible = on && !inst && dynamic && !reverse && classify == 4 && shadow_classes && num_rays == 0 && !aov;
        const ExtendShape want = !eligible ? EXTEND_GENERIC : gen_n > 0 ? EXTEND_GENERATE : EXTEND_BOUNCE;
        const ExtendShape got = pick_extend_shape(in);
        CHECK(got == want);
        // bounce 0 without fused generation (gen_n 0) never builds camera paths
        if (gen_n == 0) CHECK(got != EXTEND_GENERATE);
        if (gen_n > 0) CHECK(got != EXTEND_BOUNCE);
        ++cases;
        shaped += got != EXTEND_GENERIC;
    }
    CHECK(cases == 3 * 2 * 5 * 2 * 2 * 5 * 2 * 3 * 2);
    CHECK(shaped > 0 && shaped < cases);

    // the launches of one chunk
    CHECK(pick_extend_shape(fused(8192)) == EXTEND_GENERATE); // bounce 0, fuse_generate 1
    CHECK(pick_extend_shape(fused(0)) == EXTEND_BOUNCE);      // bounce 0 after k_generate, and every later bounce
    { // option 0: generic everywhere
        ExtendShapeInput in = fused(8192);
        in.extend_shapes = 0;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        in.gen_n = 0;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
    }
    { // each option that leaves the default mode, one at a time
        ExtendShapeInput in = fused(0);
        in.instrument = true;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        in = fused(0);
        in.dynamic = 0;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        in = fused(0);
        in.reverse = 1; // group_order 1
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        for (int c = 0; c <= 3; ++c) { // path_classes 3 or less
            in = fused(64);
            in.classify = c;
            CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        }
        in = fused(64);
        in.shadow_classes = 0;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        in = fused(64);
        in.num_rays = 16; // a ray list
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        in = fused(64);
        in.mis_aovs = true; // an aov_mis scene
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        for (int g : {0, 64}) { // stream buffers not laid out as the shapes derive them
            in = fused(g);
            in.streams_packed = false;
            CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
        }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
