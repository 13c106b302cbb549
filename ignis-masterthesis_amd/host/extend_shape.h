// Launch shape of one k_extend launch (pure host code: no HIP call;
// tests/native/extend_shape_check.cpp walks the option grid).
//
// k_extend serves every mode through wave-uniform run-time flags of its
// kernel arguments, all of which stay live across the loop over a wave's
// groups of 64 paths.  Two shapes are compiled with the default fused mode
// folded to constants (dynamic groups, front-to-back order, three path
// classes, shadow classes, no ray list, no MIS AOVs):
//   generate: bounce 0 with the camera paths built in the kernel (no input
//             stream, no slot load);
//   bounce:   every launch that reads its paths from the input stream (no
//             camera code).
// Both also derive their stream pointers from one base per stream (k_extend).
// Any other combination of options, and the instrumented build, runs the
// generic kernel.  shadow_optimistic and the tile fields stay run-time values
// in both shapes (tiled renders of a multi-GPU frame keep the fast path).
#pragma once

namespace igxh {

enum ExtendShape { EXTEND_GENERIC = 0, EXTEND_GENERATE = 1, EXTEND_BOUNCE = 2 };

// the value of FrameArgs::classify the shapes are compiled for (three path classes)
constexpr int EXTEND_SHAPE_CLASSIFY = 4;

struct ExtendShapeInput {
    int extend_shapes = -1;  // option "extend_shapes": -1 auto, 0 generic only, 1 specialised where eligible
    bool instrument = false; // option "instrument": the instrumented kernels are generic
    int gen_n = 0;           // FrameArgs::gen_n of the launch (> 0: bounce 0 with fused generation)
    int dynamic = 0;         // FrameArgs::dynamic
    int reverse = 0;         // FrameArgs::reverse
    int classify = 0;        // FrameArgs::classify
    int shadow_classes = 0;  // FrameArgs::shadow_classes
    int num_rays = 0;        // FrameArgs::num_rays (> 0: ray-list mode)
    bool mis_aovs = false;   // FrameArgs::aov_di or aov_nee set
    // the launch's stream buffers and counter rows lie as the shapes derive
    // them from one pointer each: a path buffer's arrays back to back with the
    // class-C region behind the shards, the shadow stream's likewise, one shard
    // capacity for all, the bounce's three counter rows adjacent
    bool streams_packed = true;
    // every array of those streams is at most 4 GiB, so the shapes reach a
    // record by a wave-uniform array base plus a 32-bit byte offset per lane
    // (streams_offsets_32bit of the launch's shard capacity)
    bool offsets_32bit = true;
};

// The arrays of the packed streams of shard capacity `shard_cap` records
// (NSH shards): byte offsets from the stream's first pointer, and the bytes
// of one array.  A path buffer holds the class-C region behind its shards
// (2 * NSH * shard_cap records per array: p0, p1, p2 of 16 B, p3 of 8 B), the
// shadow stream NSH * shard_cap records per array (s0, s1, s2 of 16 B).
constexpr int EXTEND_SHARDS = 64; // NSH
struct StreamLayout {
    unsigned long long path_records;    // records per path array
    unsigned long long shadow_records;  // records per shadow array
    unsigned long long p_off[4];        // p0, p1, p2, p3 from PathBuf::p0, in bytes
    unsigned long long s_off[3];        // s0, s1, s2 from ShadowBuf::s0, in bytes
    unsigned long long max_array_bytes; // the largest single array
};
constexpr StreamLayout stream_layout(int shard_cap) {
    const unsigned long long recs = (unsigned long long)EXTEND_SHARDS * (unsigned long long)shard_cap;
    return StreamLayout{2 * recs, recs, {0, 32 * recs, 64 * recs, 96 * recs}, {0, 16 * recs, 32 * recs}, 32 * recs};
}
// the byte offset of the last record of the largest array fits 32 bits
constexpr bool streams_offsets_32bit(int shard_cap) {
    return shard_cap >= 0 && stream_layout(shard_cap).max_array_bytes <= (1ull << 32);
}

// auto (-1) of option "extend_shapes"
#ifndef EXTEND_SHAPES_AUTO
#define EXTEND_SHAPES_AUTO 1
#endif

inline ExtendShape pick_extend_shape(const ExtendShapeInput& in) {
    const int opt = in.extend_shapes < 0 ? EXTEND_SHAPES_AUTO : in.extend_shapes;
    if (opt == 0 || in.instrument) return EXTEND_GENERIC;
    if (!in.dynamic || in.reverse || in.classify != EXTEND_SHAPE_CLASSIFY || in.shadow_classes != 1 || in.num_rays > 0 || in.mis_aovs || !in.streams_packed || !in.offsets_32bit)
        return EXTEND_GENERIC;
    return in.gen_n > 0 ? EXTEND_GENERATE : EXTEND_BOUNCE;
}

} // namespace igxh
