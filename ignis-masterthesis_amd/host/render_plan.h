// Chunk plan of one render call (pure host code: no HIP call;
// tests/native/render_plan_check.cpp walks it on the CPU).
//
// A render call covers `count` iterations of the caller's local pixels (the
// whole film, its tile share, or a ray list) at `spi` paths each.  The paths
// are cut into chunks of at most `capacity` paths: a capacity-sized run of
// pixels of one iteration, or, when a whole iteration fits, several
// consecutive iterations.  plan_render works out the sizes, plan_chunk
// enumerates the chunks in the order both render schedules run them,
// tail_threshold gives the live-path count at which a chunk's tail kernel
// takes over, and valid_pixels_in_chunk counts the film pixels among a
// chunk's local pixels (camera_rays of igx_get_stats).
#pragma once

#include "igx.h"
#include "device_scene.h" // IGX_PIXEL_BLOCKS

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace igxh {

constexpr long long MAX_CHUNK_PATHS = 1ll << 27;  // paths per chunk (one wavefront), ~25 GB of stream buffers per slot
constexpr long long AUTO_CHUNK_FLOOR = 1ll << 24; // the automatic chunk is at least 16 M paths ...
constexpr double AUTO_BUDGET_SHARE = 0.3;         // ... and its stream slots take at most this share of the device memory

// The pixels a call renders: the film, or its share of the film's tiles
// (tile_size > 0: tiles tile_offset, tile_offset + tile_stride, ... of the
// row-major tile grid, tiles_x a row), or a ray list (num_rays > 0)
struct TileShare {
    int width = 0, height = 0;
    int num_rays = 0;
    int tile_size = 0, tile_offset = 0, tile_stride = 0, tiles_x = 0;
};

struct RenderPlanInput { // (aggregate: render_impl fills it in this order)
    int width = 0, height = 0, num_rays = 0, tile_size = 0, tile_offset = 0, tile_stride = 0, spi = 0; // igx_render_params
    int count = 1;                            // iterations of the call
    int64_t capacity = 0, slot_budget_mb = 0; // options "capacity", "slot_budget_mb" (0: auto)
    int stream_slots = 2;                     // option "stream_slots"
    size_t mem_total = 0;                     // device memory (bytes)
    int classify = 0;                         // option "path_classes"
    bool split = false, aovs = false;         // the call runs k_trace + k_shade; the MIS AOV slots are on
};

struct RenderPlan {
    igx_status status = IGX_OK;
    const char* error = nullptr;        // the refusal's message
    int width = 0, height = 0, tiles_x = 0; // film (ray-list mode: num_rays x 1)
    long long local_pixels = 0, total_paths = 0; // pixels of this call's share; paths of one iteration
    int count = 1, spi = 1;
    int classify = 0;                   // effective FrameArgs::classify
    // chunking (all 0 when the share owns no pixel)
    long long path_slot_bytes = 0, chunk_pixels_max = 0; // stream bytes per path and slot; local pixels per chunk
    int iters_per_chunk = 0;            // > 1 only when an iteration fits the capacity
    size_t slot_cap = 0;                // paths a slot holds: no chunk has more
};

inline RenderPlan plan_render(const RenderPlanInput& in) {
    RenderPlan pl;
    const auto refuse = [&](const char* msg) {
        pl.status = IGX_ERR_INVALID_ARGUMENT;
        pl.error = msg;
        return pl;
    };
    if (in.spi < 1) return refuse("spi must be >= 1");
    const bool list_mode = in.num_rays > 0;
    const int width = list_mode ? in.num_rays : in.width;
    const int height = list_mode ? 1 : in.height;
    if (width < 1 || height < 1) return refuse("film size must be positive");
    if (in.tile_size > 0 && (in.tile_stride < 1 || in.tile_offset < 0 || in.tile_offset >= in.tile_stride))
        return refuse("invalid tile sharding parameters");
    if (list_mode && in.tile_size > 0) return refuse("ray-list mode cannot be tile-sharded");
    pl.width = width;
    pl.height = height;
    pl.count = in.count;
    pl.spi = in.spi;
    pl.classify = in.classify;
    long long local_pixels;
    if (list_mode) {
        local_pixels = in.num_rays;
    } else if (in.tile_size > 0) {
        pl.tiles_x = (width + in.tile_size - 1) / in.tile_size;
        int tiles_y = (height + in.tile_size - 1) / in.tile_size;
        int tiles = pl.tiles_x * tiles_y;
        int mine = tiles > in.tile_offset ? (tiles - in.tile_offset + in.tile_stride - 1) / in.tile_stride : 0;
        local_pixels = (long long)mine * in.tile_size * in.tile_size;
    } else {
        local_pixels = (long long)width * height;
    }
    pl.local_pixels = local_pixels;
    long long total_paths = local_pixels * in.spi;
    pl.total_paths = total_paths;
    if (total_paths == 0) return pl;
    // default chunk of a multi-iteration render: the largest power of two
    // whose stream slots take at most 30 % of the device memory (MI355X: 128 M
    // paths; two slots of 22.5 GB, 36.9 GB with three path classes).  Fewer,
    // larger chunks leave fewer tails that overlap nothing: diamond frame 193
    // -> 179 ms, S-deep 4096^2 865 -> 823 ms from 32 M to 128 M paths
    // (tools/sweep_frame.py).  Per path and slot: two path buffers (56 B a
    // record; twice that with the class-C region), shadow ray 48 B, hit
    // record 20 B (split schedule), radiance 16 B, and the two MIS AOV slots
    // (32 B) of an aov_mis scene.
    if (in.split && pl.classify >= 4) pl.classify = 3; // hit records have no class-C region
    const long long path_slot_bytes =
        2 * 56 * (pl.classify >= 4 ? 2 : 1) + 48 + (in.split ? 20 : 0) + 16 + (in.aovs ? 32 : 0);
    const long long slot_budget =
        in.slot_budget_mb > 0 ? in.slot_budget_mb * (1ll << 20) : (long long)((double)in.mem_total * AUTO_BUDGET_SHARE);
    long long auto_chunk_paths = AUTO_CHUNK_FLOOR;
    while (auto_chunk_paths < MAX_CHUNK_PATHS && in.stream_slots * (2 * auto_chunk_paths) * path_slot_bytes <= slot_budget)
        auto_chunk_paths *= 2;
    if (in.slot_budget_mb > 0) // an explicit budget also bounds the chunk below 16 M paths
        auto_chunk_paths = std::max<long long>(1ll << 20, std::min<long long>(auto_chunk_paths, slot_budget / (in.stream_slots * path_slot_bytes)));
    // capacity: whole iteration resident when it fits (<= 16M paths), pixel aligned
    long long cap = in.capacity > 0 ? in.capacity
                                    : (in.count > 1 ? auto_chunk_paths : std::min<long long>({total_paths, AUTO_CHUNK_FLOOR, auto_chunk_paths}));
    cap = std::min<long long>(cap, MAX_CHUNK_PATHS);
    cap = std::max<long long>(in.spi, (cap / in.spi) * in.spi);
    pl.path_slot_bytes = path_slot_bytes;
    pl.chunk_pixels_max = std::min<long long>(cap, total_paths) / in.spi;
    pl.iters_per_chunk = total_paths <= cap ? (int)std::min<long long>(in.count, cap / total_paths) : 1;
    pl.slot_cap = (size_t)(pl.chunk_pixels_max * in.spi * pl.iters_per_chunk);
    return pl;
}

// Chunk k of a plan, in the order both schedules run them: iteration groups
// outermost, the pixel runs of a group in order
struct Chunk {
    int it0 = 0;          // first iteration, relative to the call's
    long long px0 = 0;    // first local pixel
    int chunk_iters = 0;  // consecutive iterations the chunk covers
    int chunk_pixels = 0; // local pixels
    long long n = 0;      // paths
    bool last = false;    // the plan's last chunk (its tail overlaps nothing)
};
inline long long chunk_count(const RenderPlan& pl) {
    if (pl.total_paths == 0) return 0;
    const long long runs = (pl.local_pixels + pl.chunk_pixels_max - 1) / pl.chunk_pixels_max;
    const long long groups = ((long long)pl.count + pl.iters_per_chunk - 1) / pl.iters_per_chunk;
    return runs * groups;
}
inline Chunk plan_chunk(const RenderPlan& pl, long long k) {
    const long long runs = (pl.local_pixels + pl.chunk_pixels_max - 1) / pl.chunk_pixels_max;
    Chunk c;
    c.it0 = (int)(k / runs) * pl.iters_per_chunk;
    c.px0 = (k % runs) * pl.chunk_pixels_max;
    c.chunk_iters = std::min(pl.iters_per_chunk, pl.count - c.it0);
    c.chunk_pixels = (int)std::min<long long>(pl.chunk_pixels_max, pl.local_pixels - c.px0);
    c.n = (long long)c.chunk_pixels * pl.spi * c.chunk_iters;
    c.last = c.it0 + pl.iters_per_chunk >= pl.count && c.px0 + pl.chunk_pixels_max >= pl.local_pixels;
    return c;
}

// Live paths at or below which the tail kernel takes over a chunk of n paths.
// Auto (option -1): n / 64, but at most what one pass of k_finish holds
// (fin_lanes: one path per resident lane, lane pairs one per two): beyond
// that the tail kernel's lanes loop over several long paths each and it
// outlasts the overlapping chunk (diamond 32M-path chunks: 500K -> 196K tail
// paths, 204.6 -> 195.0 ms per frame, tools/sweep_frame.py); never below 32768.
// tail_last_opt >= 0 replaces tail_opt on the plan's last chunk.
inline int tail_threshold(long long n, long long fin_lanes, int64_t tail_opt, int64_t tail_last_opt, bool last) {
    const int64_t topt = last && tail_last_opt >= 0 ? tail_last_opt : tail_opt;
    return topt >= 0 ? (int)std::min<int64_t>(topt, 1 << 30) : (int)std::max<long long>(32768, std::min(n / 64, fin_lanes));
}

// Film pixels among the local pixels [chunk_pixel0, chunk_pixel0 + chunk_pixels)
// (tiles at the film's right and bottom edges hang over it): per tile in
// closed form, the valid pixels among a tile's first m row-major pixels being
// min(m / T, h) * w + (m / T < h ? min(m % T, w) : 0).  (A per-pixel loop cost
// 8 ms of host time per 67 M-path config-5 chunk, during which the GPU idled:
// profiles/r04_timeline_gaps.log.)
inline long long valid_pixels_in_chunk(const TileShare& fa, long long chunk_pixel0, long long chunk_pixels) {
    if (fa.num_rays > 0 || fa.tile_size <= 0) return chunk_pixels;
    long long v = 0;
    const long long T = fa.tile_size, TT = T * T;
    const long long c0 = chunk_pixel0, c1 = c0 + chunk_pixels;
    for (long long k = c0 / TT; k * TT < c1; ++k) {
        const long long t = fa.tile_offset + k * fa.tile_stride;
        const long long ty = t / fa.tiles_x, tx = t - ty * fa.tiles_x;
        const long long w = std::max(0ll, std::min(T, fa.width - tx * T)), h = std::max(0ll, std::min(T, fa.height - ty * T));
        auto valid_first = [&](long long m) { // valid pixels among the tile's first m
            if (IGX_PIXEL_BLOCKS && (T & 3) == 0) { // 4 x 2 blocks along row pairs (block_order)
                const long long pairs = m / (2 * T), q = m - pairs * 2 * T, nb = q / 8, rem = q - nb * 8;
                const long long y0 = 2 * pairs, c0 = 4 * nb + std::min(rem, 4ll), c1 = 4 * nb + std::max(0ll, rem - 4);
                return std::min(y0, h) * w + (y0 < h ? std::min(c0, w) : 0) + (y0 + 1 < h ? std::min(c1, w) : 0);
            }
            const long long rows = m / T;
            return std::min(rows, h) * w + (rows < h ? std::min(m % T, w) : 0);
        };
        v += valid_first(std::min(TT, c1 - k * TT)) - valid_first(std::max(0ll, c0 - k * TT));
    }
    return v;
}

} // namespace igxh
