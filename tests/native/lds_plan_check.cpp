// plan_lds (host/lds_plan.h) at its edges: the wide k_extend layout (1024
// threads, shading tables staged) is chosen exactly when stack + fixed LDS +
// traversal tables + padded shading tables fit the device's LDS per
// workgroup; everything else keeps the 256-thread layout.
#include "lds_plan.h"

#include <cstdio>

using namespace igxh;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);       \
            ++failures;                                            \
        }                                                          \
    } while (0)

// the diamond's tables on a 160 KB device
static LdsPlanInput diamond() {
    LdsPlanInput in;
    in.traversal_bytes = 22368;
    in.traversal_max = 48 * 1024;
    in.shading_bytes[LDS_TAB_ENT] = 9 * 112;
    in.shading_bytes[LDS_TAB_FSH] = 282 * 48;
    in.shading_bytes[LDS_TAB_FN] = 822 * 16;
    in.shading_bytes[LDS_TAB_MATS] = 4 * 128;
    in.shading_bytes[LDS_TAB_LIGHTS] = 128;
    in.shading_bytes[LDS_TAB_ENT_ENC] = 36; // padded to 48
    in.shading_max = 48 * 1024;
    in.shading_on = true;
    in.stack_bytes_per_thread = 64;
    in.fixed_bytes = 1024 + 4608;
    in.lds_per_block = 160 * 1024;
    return in;
}

static bool today(const LdsPlan& p, size_t traversal) {
    return p.block_threads == 256 && p.shading_bytes == 0 && p.traversal_bytes == traversal;
}

int main() {
    const size_t sh = 9 * 112 + 282 * 48 + 822 * 16 + 4 * 128 + 128 + 48;
    {
        const LdsPlanInput in = diamond();
        CHECK(lds_shading_total(in) == sh);
        const LdsPlan p = plan_lds(in);
        CHECK(p.block_threads == 1024 && p.traversal_bytes == 22368 && p.shading_bytes == sh);
    }
    { // exactly fits / one byte over
        LdsPlanInput in = diamond();
        const size_t block = 1024 * 64 + in.fixed_bytes + 22368 + sh;
        in.lds_per_block = block;
        CHECK(plan_lds(in).block_threads == 1024 && plan_lds(in).shading_bytes == sh);
        in.lds_per_block = block - 1;
        CHECK(today(plan_lds(in), 22368));
        // ... and the same edge moved by the tables: one more byte of padded tables
        in.lds_per_block = block;
        in.shading_bytes[LDS_TAB_ENT_ENC] = 49; // pads to 64
        CHECK(today(plan_lds(in), 22368));
    }
    { // the byte cap on the shading tables: at the cap, one byte below it
        LdsPlanInput in = diamond();
        in.shading_max = (int64_t)sh;
        CHECK(plan_lds(in).block_threads == 1024);
        in.shading_max = (int64_t)sh - 1;
        CHECK(today(plan_lds(in), 22368));
        in.shading_max = 1024;
        CHECK(today(plan_lds(in), 22368));
    }
    { // no shading tables: without fsh, without fn_tab, with neither
        LdsPlanInput in = diamond();
        in.shading_bytes[LDS_TAB_FSH] = 0;
        CHECK(today(plan_lds(in), 22368));
        in = diamond();
        in.shading_bytes[LDS_TAB_FN] = 0;
        CHECK(today(plan_lds(in), 22368));
        in = diamond();
        for (size_t& b : in.shading_bytes) b = 0;
        CHECK(today(plan_lds(in), 22368));
    }
    { // option off
        LdsPlanInput in = diamond();
        in.shading_on = false;
        CHECK(today(plan_lds(in), 22368));
    }
    { // traversal tables over lds_scene_max: global tables, nothing staged
        LdsPlanInput in = diamond();
        in.traversal_max = 22367;
        CHECK(today(plan_lds(in), 0));
        in.traversal_max = 22368;
        CHECK(plan_lds(in).block_threads == 1024);
        in.traversal_max = 0;
        CHECK(today(plan_lds(in), 0));
    }
    { // a device with 64 KB of LDS per workgroup: today's layout
        LdsPlanInput in = diamond();
        in.lds_per_block = 64 * 1024;
        CHECK(today(plan_lds(in), 22368));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
