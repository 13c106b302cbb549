// LDS layout of the LDS-staged k_extend for one scene (pure host code: no HIP
// call; tests/native/lds_plan_check.cpp exercises its edges).
//
// Today's layout: 256-thread blocks, each with its own traversal stack and
// its own copy of the traversal tables, as many blocks per CU as fit.  The
// wide layout: one 1024-thread block per CU with one copy of the traversal
// tables, which leaves room for the shading tables (entity records, per-face
// shading records, face normals, materials, lights, enclosing indices) behind
// them (stage_scene_lds).  The wide layout is chosen only when everything the
// block holds fits the device's LDS per workgroup.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace igxh {

constexpr int LDS_PLAN_BLOCK = 256;       // threads per block of every other traversal kernel
constexpr int LDS_PLAN_BLOCK_WIDE = 1024; // threads per block of the wide k_extend
enum { LDS_TAB_ENT = 0, LDS_TAB_FSH, LDS_TAB_FN, LDS_TAB_MATS, LDS_TAB_LIGHTS, LDS_TAB_ENT_ENC, LDS_TAB_COUNT };

struct LdsPlanInput {
    size_t traversal_bytes = 0;              // nodes + instance records + triangles, back to back
    int64_t traversal_max = 0;               // option "lds_scene_max"
    size_t shading_bytes[LDS_TAB_COUNT] = {}; // by table (LDS_TAB_*), unpadded
    int64_t shading_max = 0;                 // option "lds_shading_max"
    bool shading_on = false;                 // option "lds_shading" resolved (auto -> the build's default)
    size_t stack_bytes_per_thread = 0;       // LDS traversal stack of one lane
    size_t fixed_bytes = 0;                  // the block's other static LDS (enclosing boxes, instrumentation)
    size_t lds_per_block = 0;                // device attribute: LDS one workgroup may take
};

struct LdsPlan {
    int block_threads = LDS_PLAN_BLOCK;
    size_t traversal_bytes = 0; // staged per block (0: global tables)
    size_t shading_bytes = 0;   // staged per block behind them, every table padded to 16 B (0: not staged)
};

constexpr size_t lds_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// Bytes the shading tables take in LDS: each table starts 16-B aligned.
inline size_t lds_shading_total(const LdsPlanInput& in) {
    size_t t = 0;
    for (int k = 0; k < LDS_TAB_COUNT; ++k) t += lds_pad16(in.shading_bytes[k]);
    return t;
}

inline LdsPlan plan_lds(const LdsPlanInput& in) {
    LdsPlan p;
    if (in.traversal_max <= 0 || in.traversal_bytes == 0 || (int64_t)in.traversal_bytes > in.traversal_max) return p; // global tables
    p.traversal_bytes = in.traversal_bytes;
    // the shading path the wide kernel compiles reads the per-face records and
    // the face-normal table: without either the scene keeps today's layout
    if (!in.shading_on || in.shading_bytes[LDS_TAB_FSH] == 0 || in.shading_bytes[LDS_TAB_FN] == 0) return p;
    const size_t sh = lds_shading_total(in);
    if ((int64_t)sh > in.shading_max) return p;
    const size_t block = (size_t)LDS_PLAN_BLOCK_WIDE * in.stack_bytes_per_thread + in.fixed_bytes + lds_pad16(in.traversal_bytes) + sh;
    if (block > in.lds_per_block) return p;
    p.block_threads = LDS_PLAN_BLOCK_WIDE;
    p.shading_bytes = sh;
    return p;
}

} // namespace igxh
