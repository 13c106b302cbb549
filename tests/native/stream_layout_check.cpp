// stream_layout / streams_offsets_32bit (host/extend_shape.h).  k_extend's
// shapes add stream_layout's offsets to the first pointer of a stream, and
// the host launches a shape only when the buffers' own pointers lie at those
// offsets (launch_shape), so this checks the one function both use: against
// arrays laid back to back in a real block (the class-C region behind the
// shards), and the 4-GiB rule at, just below and just above the limit: a
// launch whose arrays fail it runs the generic kernel.
#include "extend_shape.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace igxh;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);       \
            ++failures;                                            \
        }                                                          \
    } while (0)

struct F4 { float v[4]; };
struct F2 { float v[2]; };
static_assert(sizeof(F4) == 16 && sizeof(F2) == 8, "record sizes");
// the general buffers: one pointer per array
struct PathPtrs { F4 *p0, *p1, *p2; F2* p3; };
struct ShadowPtrs { F4 *s0, *s1, *s2; };

// the slot allocation: NSH shards of shard_cap records, a path buffer with a
// second set for class C, the arrays of a stream back to back in one block
static size_t path_block_bytes(int shard_cap) { return (size_t)2 * EXTEND_SHARDS * shard_cap * (3 * sizeof(F4) + sizeof(F2)); }
static size_t shadow_block_bytes(int shard_cap) { return (size_t)EXTEND_SHARDS * shard_cap * 3 * sizeof(F4); }
static PathPtrs path_ptrs(char* block, int shard_cap) {
    const size_t precs = (size_t)2 * EXTEND_SHARDS * shard_cap;
    F4* p0 = reinterpret_cast<F4*>(block);
    return PathPtrs{p0, p0 + precs, p0 + 2 * precs, reinterpret_cast<F2*>(p0 + 3 * precs)};
}
static ShadowPtrs shadow_ptrs(char* block, int shard_cap) {
    const size_t recs = (size_t)EXTEND_SHARDS * shard_cap;
    F4* s0 = reinterpret_cast<F4*>(block);
    return ShadowPtrs{s0, s0 + recs, s0 + 2 * recs};
}

static ExtendShapeInput fused(int gen_n, int shard_cap) {
    ExtendShapeInput in;
    in.extend_shapes = 1;
    in.gen_n = gen_n;
    in.dynamic = 1;
    in.classify = EXTEND_SHAPE_CLASSIFY;
    in.shadow_classes = 1;
    in.offsets_32bit = streams_offsets_32bit(shard_cap);
    return in;
}

int main() {
    // derived offsets against real pointers into real blocks
    for (int cap : {64, 128, 192, 1024}) {
        const StreamLayout l = stream_layout(cap);
        std::vector<char> pb(path_block_bytes(cap)), sb(shadow_block_bytes(cap));
        const PathPtrs p = path_ptrs(pb.data(), cap);
        const ShadowPtrs s = shadow_ptrs(sb.data(), cap);
        CHECK(reinterpret_cast<char*>(p.p0) == pb.data() + l.p_off[0]);
        CHECK(reinterpret_cast<char*>(p.p1) == pb.data() + l.p_off[1]);
        CHECK(reinterpret_cast<char*>(p.p2) == pb.data() + l.p_off[2]);
        CHECK(reinterpret_cast<char*>(p.p3) == pb.data() + l.p_off[3]);
        CHECK(reinterpret_cast<char*>(s.s0) == sb.data() + l.s_off[0]);
        CHECK(reinterpret_cast<char*>(s.s1) == sb.data() + l.s_off[1]);
        CHECK(reinterpret_cast<char*>(s.s2) == sb.data() + l.s_off[2]);
        CHECK(l.path_records == (unsigned long long)2 * EXTEND_SHARDS * cap);
        CHECK(l.shadow_records == (unsigned long long)EXTEND_SHARDS * cap);
        // the blocks end where the last arrays end
        CHECK(l.p_off[3] + l.path_records * sizeof(F2) == pb.size());
        CHECK(l.s_off[2] + l.shadow_records * sizeof(F4) == sb.size());
        // the last record of every array, by 32-bit byte offset from the array's base
        const uint32_t last_p = (uint32_t)(l.path_records - 1), last_s = (uint32_t)(l.shadow_records - 1);
        CHECK(reinterpret_cast<char*>(p.p2) + last_p * (uint32_t)sizeof(F4) == reinterpret_cast<char*>(p.p2 + last_p));
        CHECK(reinterpret_cast<char*>(p.p3) + last_p * (uint32_t)sizeof(F2) == reinterpret_cast<char*>(p.p3 + last_p));
        CHECK(reinterpret_cast<char*>(s.s2) + last_s * (uint32_t)sizeof(F4) == reinterpret_cast<char*>(s.s2 + last_s));
        CHECK(l.max_array_bytes == l.path_records * sizeof(F4));
        CHECK(streams_offsets_32bit(cap));
    }

    // the 4-GiB rule.  The largest chunk holds 2^27 paths: 2^21 records per
    // shard, 2^28 per path array with the class-C region, 2^32 bytes
    const int cap_max = 1 << 21;
    CHECK(stream_layout(cap_max).max_array_bytes == (1ull << 32));
    for (int cap : {64, cap_max - 64, cap_max, cap_max + 64, 1 << 22, 1 << 24}) {
        const StreamLayout l = stream_layout(cap);
        // the rule written out: the byte offset of every array's last record fits 32 bits
        const unsigned long long last = (l.path_records - 1) * sizeof(F4);
        const bool fits = last <= 0xFFFFFFFFull && (l.path_records - 1) * sizeof(F2) <= 0xFFFFFFFFull &&
                          (l.shadow_records - 1) * sizeof(F4) <= 0xFFFFFFFFull;
        CHECK(streams_offsets_32bit(cap) == fits);
        CHECK(streams_offsets_32bit(cap) == (cap <= cap_max));
        if (fits) { // and the 32-bit product a lane computes is that offset
            const uint32_t e = (uint32_t)(l.path_records - 1);
            CHECK((unsigned long long)(e * (uint32_t)sizeof(F4)) == last);
        }
        // array offsets from the stream's pointer do not fit 32 bits at the limit: they stay 64-bit scalars
        CHECK(l.p_off[1] == 2 * l.shadow_records * sizeof(F4) && l.p_off[2] == 2 * l.p_off[1] && l.p_off[3] == 3 * l.p_off[1]);
        for (int g : {0, 8192}) {
            const ExtendShape got = pick_extend_shape(fused(g, cap));
            CHECK(got == (fits ? (g > 0 ? EXTEND_GENERATE : EXTEND_BOUNCE) : EXTEND_GENERIC));
        }
    }
    CHECK(streams_offsets_32bit(0));
    CHECK(!streams_offsets_32bit(-64));
    { // the flag alone sends a launch of the default mode to the generic kernel
        ExtendShapeInput in = fused(0, 64);
        CHECK(pick_extend_shape(in) == EXTEND_BOUNCE);
        in.offsets_32bit = false;
        CHECK(pick_extend_shape(in) == EXTEND_GENERIC);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
