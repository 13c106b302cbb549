// host/aov_plan.h at its edges: which iterations get the denoiser's
// info-buffer pass (InfoBufferTechnique.cpp:56-66: the iteration numbered 0,
// or every one) and which AOV names exist with which groups on.
#include "aov_plan.h"

#include <cstdio>
#include <cstring>
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

// the passes of a range, counted one iteration at a time
static int64_t counted(int mode, int64_t first, int64_t count) {
    int64_t n = 0;
    for (int64_t i = first; i < first + count; ++i) n += info_pass_due(mode, i) ? 1 : 0;
    return n;
}

int main() {
    { // mode 0: never
        for (int64_t first : {0, 1, 5})
            for (int64_t count : {1, 3, 100}) CHECK(info_passes_in(INFO_OFF, first, count) == 0);
        CHECK(!info_pass_due(INFO_OFF, 0) && !info_pass_due(INFO_OFF, 7));
    }
    { // mode 1: exactly the iteration numbered 0 inside [first, first + count)
        CHECK(info_pass_due(INFO_FIRST, 0));
        CHECK(!info_pass_due(INFO_FIRST, 1) && !info_pass_due(INFO_FIRST, 1000000));
        CHECK(info_passes_in(INFO_FIRST, 0, 1) == 1);
        CHECK(info_passes_in(INFO_FIRST, 0, 3) == 1);
        CHECK(info_passes_in(INFO_FIRST, 1, 1) == 0);
        CHECK(info_passes_in(INFO_FIRST, 1, 3) == 0);
        CHECK(info_passes_in(INFO_FIRST, 3, 3) == 0);
        CHECK(info_passes_in(INFO_FIRST, 0, 0) == 0); // an empty range, also at 0
        CHECK(info_passes_in(INFO_FIRST, 0, -1) == 0);
    }
    { // mode 2: all of them
        CHECK(info_pass_due(INFO_EVERY, 0) && info_pass_due(INFO_EVERY, 1) && info_pass_due(INFO_EVERY, 12345));
        CHECK(info_passes_in(INFO_EVERY, 0, 1) == 1);
        CHECK(info_passes_in(INFO_EVERY, 0, 3) == 3);
        CHECK(info_passes_in(INFO_EVERY, 1, 3) == 3);
        CHECK(info_passes_in(INFO_EVERY, 7, 0) == 0);
    }
    // the closed form agrees with counting, every mode
    for (int mode : {INFO_OFF, INFO_FIRST, INFO_EVERY})
        for (int64_t first = 0; first < 4; ++first)
            for (int64_t count = 0; count < 5; ++count) CHECK(info_passes_in(mode, first, count) == counted(mode, first, count));
    { // the name table
        CHECK(AOV_COUNT == 5 && AOV_MIS_COUNT == 2 && AOV_INFO_COUNT == 3);
        const char* expect[] = {"Direct Weights", "NEE Weights", "Normals", "Albedo", "Depth"};
        for (int k = 0; k < AOV_COUNT; ++k) CHECK(std::strcmp(AOV_NAMES[k], expect[k]) == 0);
        CHECK(AOV_NORMALS == AOV_INFO_FIRST && AOV_DEPTH == AOV_INFO_FIRST + 2 && AOV_DIRECT_WEIGHTS == AOV_MIS_FIRST);
        for (bool mis : {false, true})
            for (bool info : {false, true}) {
                CHECK(aov_lookup(nullptr, mis, info) == AOV_COLOR);
                CHECK(aov_lookup("", mis, info) == AOV_COLOR);
                CHECK(aov_lookup("Color", mis, info) == AOV_COLOR);
                CHECK(aov_lookup("Direct Weights", mis, info) == (mis ? AOV_DIRECT_WEIGHTS : AOV_UNKNOWN));
                CHECK(aov_lookup("NEE Weights", mis, info) == (mis ? AOV_NEE_WEIGHTS : AOV_UNKNOWN));
                CHECK(aov_lookup("Normals", mis, info) == (info ? AOV_NORMALS : AOV_UNKNOWN));
                CHECK(aov_lookup("Albedo", mis, info) == (info ? AOV_ALBEDO : AOV_UNKNOWN));
                CHECK(aov_lookup("Depth", mis, info) == (info ? AOV_DEPTH : AOV_UNKNOWN));
                CHECK(aov_lookup("Position", mis, info) == AOV_UNKNOWN);
                CHECK(aov_lookup("Normal", mis, info) == AOV_UNKNOWN);  // a prefix
                CHECK(aov_lookup("Normalss", mis, info) == AOV_UNKNOWN); // and an extension
                CHECK(aov_lookup("color", mis, info) == AOV_UNKNOWN);
            }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
