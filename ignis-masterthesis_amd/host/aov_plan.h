// AOV names and the schedule of the denoiser's info-buffer pass (pure host
// code: no HIP call; tests/native/aov_plan_check.cpp exercises its edges).
//
// The film is "Color" (or "" / NULL).  The path tracer's aov_mis adds "Direct
// Weights" and "NEE Weights" (PathTechnique.cpp:16-27); the denoiser adds
// "Normals", "Albedo" and "Depth" (InfoBufferTechnique.cpp:28-30), filled by
// one extra pass with one sample per pixel that leaves the film alone
// (LockFramebuffer, OverrideSPI = 1, InfoBufferTechnique.cpp:37-38).  The pass
// runs in the iteration numbered 0 only, or in every iteration
// (`always || iter == 0`, InfoBufferTechnique.cpp:56-66; Denoiser.
// OnlyFirstIteration, RuntimeSettings.h:8-9).  Each AOV counts its own
// iterations (Device.cpp:1390-1403, 1468-1471).
#pragma once

#include <stdint.h>

namespace igxh {

// igx_get_aov / igx_clear_aov index of a name
enum { AOV_UNKNOWN = -2, AOV_COLOR = -1, AOV_DIRECT_WEIGHTS = 0, AOV_NEE_WEIGHTS, AOV_NORMALS, AOV_ALBEDO, AOV_DEPTH, AOV_COUNT };
constexpr int AOV_MIS_FIRST = AOV_DIRECT_WEIGHTS, AOV_MIS_COUNT = 2;
constexpr int AOV_INFO_FIRST = AOV_NORMALS, AOV_INFO_COUNT = 3;
constexpr const char* AOV_NAMES[AOV_COUNT] = {"Direct Weights", "NEE Weights", "Normals", "Albedo", "Depth"};

// option "denoise_aovs"
enum { INFO_OFF = 0, INFO_FIRST = 1, INFO_EVERY = 2 };

constexpr bool aov_str_eq(const char* a, const char* b) {
    while (*a && *a == *b) {
        ++a;
        ++b;
    }
    return *a == *b;
}

// Index of `name` given which groups exist: the MIS AOVs with the technique's
// aov_mis, the info AOVs with the denoiser on; a name of a group that is off is
// as unknown as any other (the reference logs it and returns no data,
// Device.cpp:1330-1363).
constexpr int aov_lookup(const char* name, bool mis_on, bool info_on) {
    if (!name || !*name || aov_str_eq(name, "Color")) return AOV_COLOR;
    for (int k = 0; k < AOV_COUNT; ++k)
        if (aov_str_eq(name, AOV_NAMES[k])) {
            const bool info = k >= AOV_INFO_FIRST;
            return (info ? info_on : mis_on) ? k : AOV_UNKNOWN;
        }
    return AOV_UNKNOWN;
}

// Does iteration number `iteration` get an info-buffer pass?
constexpr bool info_pass_due(int mode, int64_t iteration) {
    return mode == INFO_EVERY || (mode == INFO_FIRST && iteration == 0);
}

// Passes among the iterations first_iteration .. first_iteration + count - 1
constexpr int64_t info_passes_in(int mode, int64_t first_iteration, int64_t count) {
    if (count <= 0) return 0;
    if (mode == INFO_EVERY) return count;
    if (mode == INFO_FIRST) return first_iteration <= 0 && 0 < first_iteration + count ? 1 : 0;
    return 0;
}

} // namespace igxh
