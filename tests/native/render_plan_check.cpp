// The chunk plan of a render call (host/render_plan.h): valid_pixels_in_chunk
// against a per-pixel count through a restated local_to_global, the chunk
// enumeration's invariants, the automatic chunk size, the tail threshold, the
// refusals, and full plans against values worked out from the expressions
// the render driver held before they moved here.
#include "render_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

using namespace igxh;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            if (failures < 50) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

// local_to_global of the kernels, restated: local pixel -> (x, y), false
// outside the film.  4 x 2 blocks along row pairs when the tile side (untiled:
// the width, with an even height) is a multiple of 4, row-major otherwise.
static void block_order(long long r, long long w, long long& x, long long& y) {
    const long long pair = r / (2 * w), q = r - pair * 2 * w;
    x = (q >> 3) * 4 + (q & 3);
    y = 2 * pair + ((q >> 2) & 1);
}
static bool local_to_global(const TileShare& fa, long long lp, long long& x, long long& y) {
    if (fa.num_rays > 0) { x = lp; y = 0; return lp < fa.num_rays; }
    if (fa.tile_size <= 0) {
        if ((fa.width & 3) == 0 && (fa.height & 1) == 0) block_order(lp, fa.width, x, y);
        else { y = lp / fa.width; x = lp - y * fa.width; }
        return true;
    }
    const long long T = fa.tile_size;
    const long long k = lp / (T * T), r = lp - k * T * T;
    long long tx, ty;
    if ((T & 3) == 0) block_order(r, T, tx, ty);
    else { ty = r / T; tx = r - ty * T; }
    const long long t = fa.tile_offset + k * fa.tile_stride;
    const long long tyy = t / fa.tiles_x, txx = t - tyy * fa.tiles_x;
    x = txx * T + tx;
    y = tyy * T + ty;
    return x < fa.width && y < fa.height;
}

static RenderPlanInput film(int w, int h, int spi, int count, int64_t capacity) {
    RenderPlanInput in;
    in.width = w;
    in.height = h;
    in.spi = spi;
    in.count = count;
    in.capacity = capacity;
    in.mem_total = (size_t)288 << 30;
    in.classify = 4;
    return in;
}

static void check_valid_pixels() {
    static_assert(IGX_PIXEL_BLOCKS == 1, "the restated local_to_global is the blocked order");
    const int films[][2] = {{5, 3}, {8, 8}, {13, 7}, {64, 33}, {100, 60}};
    long long windows = 0;
    for (const auto& f : films)
    for (int T : {1, 3, 4, 8, 16})
    for (int stride : {1, 2, 3})
    for (int offset = 0; offset < stride; ++offset) {
        RenderPlanInput in = film(f[0], f[1], 1, 1, 0);
        in.tile_size = T;
        in.tile_offset = offset;
        in.tile_stride = stride;
        const RenderPlan pl = plan_render(in);
        CHECK(pl.status == IGX_OK);
        const TileShare fa{f[0], f[1], 0, T, offset, stride, pl.tiles_x};
        const long long all = pl.local_pixels, TT = (long long)T * T;
        // prefix[i]: film pixels among local pixels [0, i); every film pixel of the share exactly once
        std::vector<long long> prefix(all + 1, 0);
        std::vector<char> seen((size_t)f[0] * f[1], 0);
        for (long long lp = 0; lp < all; ++lp) {
            long long x, y;
            const bool in_film = local_to_global(fa, lp, x, y);
            if (in_film) {
                CHECK(!seen[y * f[0] + x]);
                seen[y * f[0] + x] = 1;
            }
            prefix[lp + 1] = prefix[lp] + (in_film ? 1 : 0);
        }
        if (stride == 1) CHECK(prefix[all] == (long long)f[0] * f[1]);
        const long long marks[] = {0, 1, 7, 8, TT - 1, TT, TT + 1, all};
        for (long long c0 : marks)
        for (long long len : marks) {
            if (c0 < 0 || len < 0 || c0 > all) continue;
            const long long l = std::min(len, all - c0);
            CHECK(valid_pixels_in_chunk(fa, c0, l) == prefix[c0 + l] - prefix[c0]);
            ++windows;
        }
    }
    CHECK(windows >= 2000); // 150 shares, most of them with every window of c0, len in {0, 1, T*T, all} at least
    // untiled and a ray list: every local pixel is a film pixel
    const TileShare untiled{100, 60, 0, 0, 0, 0, 0};
    CHECK(valid_pixels_in_chunk(untiled, 0, 6000) == 6000 && valid_pixels_in_chunk(untiled, 17, 333) == 333);
    const TileShare list{4096, 1, 4096, 0, 0, 0, 0};
    CHECK(valid_pixels_in_chunk(list, 0, 4096) == 4096 && valid_pixels_in_chunk(list, 1000, 96) == 96);
    long long x, y;
    CHECK(local_to_global(list, 4095, x, y) && x == 4095 && y == 0);
}

// chunks tile [0, count) x [0, local_pixels) exactly once, in the order of the
// driver's loops (iteration groups outermost, pixel runs inside)
static void check_enumeration(const RenderPlanInput& in) {
    const RenderPlan pl = plan_render(in);
    CHECK(pl.status == IGX_OK);
    const long long chunks = chunk_count(pl);
    if (pl.local_pixels == 0) {
        CHECK(chunks == 0 && pl.total_paths == 0 && pl.slot_cap == 0);
        return;
    }
    CHECK(pl.total_paths == pl.local_pixels * in.spi);
    CHECK(pl.slot_cap <= (size_t)MAX_CHUNK_PATHS && pl.chunk_pixels_max >= 1 && pl.iters_per_chunk >= 1);
    const long long cap = std::max<long long>(in.spi, in.capacity > 0 ? std::min<long long>(in.capacity, MAX_CHUNK_PATHS) : MAX_CHUNK_PATHS);
    if (pl.iters_per_chunk > 1) CHECK(pl.total_paths <= cap); // several iterations only when one fits the capacity
    if (in.capacity >= in.spi) CHECK((long long)pl.slot_cap <= in.capacity);
    if (in.capacity > 0 && in.capacity < in.spi) CHECK(pl.chunk_pixels_max == 1 && pl.iters_per_chunk == 1); // one pixel's paths
    long long k = 0, covered = 0;
    for (int it0 = 0; it0 < in.count; it0 += pl.iters_per_chunk)
        for (long long px0 = 0; px0 < pl.local_pixels; px0 += pl.chunk_pixels_max, ++k) {
            const Chunk c = plan_chunk(pl, k);
            CHECK(c.it0 == it0 && c.px0 == px0);
            CHECK(c.chunk_iters >= 1 && it0 + c.chunk_iters <= in.count && (c.chunk_iters == pl.iters_per_chunk || it0 + c.chunk_iters == in.count));
            CHECK(c.chunk_pixels >= 1 && px0 + c.chunk_pixels <= pl.local_pixels &&
                  (c.chunk_pixels == pl.chunk_pixels_max || px0 + c.chunk_pixels == pl.local_pixels));
            CHECK((long long)c.chunk_pixels * in.spi * c.chunk_iters == c.n);
            CHECK(c.n <= (long long)pl.slot_cap);
            CHECK(c.last == (k == chunks - 1));
            covered += (long long)c.chunk_pixels * c.chunk_iters;
        }
    CHECK(k == chunks);
    CHECK(covered == pl.local_pixels * in.count);
}

static void check_enumerations() {
    for (long long pixels : {1ll, 7ll, 64ll, 10000ll, 65536ll})
    for (int spi : {1, 2, 7, 64})
    for (int count : {1, 2, 3, 17})
    for (long long capacity : {0ll, 1ll, 5ll, 64ll, 4096ll, 20000ll, 1ll << 20, 1ll << 40}) {
        RenderPlanInput in = film((int)pixels, 1, spi, count, capacity);
        check_enumeration(in);
        in.num_rays = (int)pixels; // the same pixels as a ray list
        in.width = in.height = 0;
        check_enumeration(in);
    }
    { // the setting tests/test_gpu.py uses: 4 chunks per iteration
        const RenderPlan pl = plan_render(film(100, 100, 2, 3, 20000));
        CHECK(pl.chunk_pixels_max == 10000 && pl.iters_per_chunk == 1 && chunk_count(pl) == 3);
        const RenderPlan quarter = plan_render(film(100, 100, 2, 3, 5000));
        CHECK(quarter.chunk_pixels_max == 2500 && quarter.iters_per_chunk == 1 && chunk_count(quarter) == 12);
        CHECK(plan_chunk(quarter, 5).it0 == 1 && plan_chunk(quarter, 5).px0 == 2500 && !plan_chunk(quarter, 5).last && plan_chunk(quarter, 11).last);
        check_enumeration(film(100, 100, 2, 3, 5000));
    }
    { // count 1 keeps a small film's chunk at the film; count > 1 batches iterations up to the automatic chunk
        const RenderPlan one = plan_render(film(100, 100, 2, 1, 0)), many = plan_render(film(100, 100, 2, 5, 0));
        CHECK(one.slot_cap == 20000 && one.iters_per_chunk == 1 && chunk_count(one) == 1);
        CHECK(many.slot_cap == 100000 && many.iters_per_chunk == 5 && chunk_count(many) == 1);
    }
    { // a tile share that owns no tile
        RenderPlanInput in = film(13, 7, 5, 4, 0);
        in.tile_size = 4;
        in.tile_offset = 9;
        in.tile_stride = 10;
        const RenderPlan pl = plan_render(in);
        CHECK(pl.status == IGX_OK && pl.tiles_x == 4 && pl.local_pixels == 0);
        check_enumeration(in);
    }
}

static bool power_of_two(long long v) { return v > 0 && (v & (v - 1)) == 0; }

static void check_auto_chunk() {
    for (int gib : {16, 64, 192, 288})
    for (int slots : {1, 2})
    for (int classify : {3, 4})
    for (int split = 0; split <= 1; ++split)
    for (int aovs = 0; aovs <= 1; ++aovs)
    for (int64_t budget_mb : {(int64_t)0, (int64_t)1, (int64_t)512, (int64_t)100000}) {
        // 2^30 paths an iteration and several iterations: the chunk is the automatic one
        RenderPlanInput in = film(1 << 15, 1 << 15, 1, 2, 0);
        in.mem_total = (size_t)gib << 30;
        in.stream_slots = slots;
        in.classify = classify;
        in.split = split != 0;
        in.aovs = aovs != 0;
        in.slot_budget_mb = budget_mb;
        const RenderPlan pl = plan_render(in);
        CHECK(pl.status == IGX_OK && pl.iters_per_chunk == 1);
        CHECK(pl.classify == (split && classify >= 4 ? 3 : classify));
        CHECK(pl.path_slot_bytes == 2 * 56 * (pl.classify >= 4 ? 2 : 1) + 48 + (split ? 20 : 0) + 16 + (aovs ? 32 : 0));
        const long long chunk = pl.chunk_pixels_max; // spi 1: paths
        // the budget: 30 % of the memory, or the option
        const long long budget = budget_mb > 0 ? budget_mb * (1ll << 20) : (long long)((double)in.mem_total * 0.3);
        const long long floor = budget_mb > 0 ? 1ll << 20 : 1ll << 24;
        if (budget_mb == 0) CHECK(power_of_two(chunk));
        CHECK(chunk >= floor && chunk <= (1ll << 27));
        // the slots fit the budget whenever the floor does not bind
        if (chunk > floor) CHECK(slots * chunk * pl.path_slot_bytes <= budget);
        // and the automatic chunk is the largest such power of two (or the bound)
        if (budget_mb == 0 && chunk < (1ll << 27)) CHECK(slots * (2 * chunk) * pl.path_slot_bytes > budget);
    }
}

static void check_tail_threshold() {
    // explicit option, clamped to 2^30
    CHECK(tail_threshold(1 << 20, 500000, 0, -1, false) == 0);
    CHECK(tail_threshold(1 << 20, 500000, 12345, -1, true) == 12345);
    CHECK(tail_threshold(1 << 20, 500000, (int64_t)1 << 40, -1, false) == 1 << 30);
    // tail_threshold_last: on the last chunk only, and only when set
    CHECK(tail_threshold(1 << 20, 500000, 100, 7, false) == 100);
    CHECK(tail_threshold(1 << 20, 500000, 100, 7, true) == 7);
    CHECK(tail_threshold(1 << 20, 500000, 100, 0, true) == 0);
    CHECK(tail_threshold(1 << 26, 500000, -1, 7, true) == 7);
    CHECK(tail_threshold(1 << 26, 500000, -1, 7, false) == 500000);
    // auto: the 32768 floor, n / 64, fin_lanes
    CHECK(tail_threshold(20000, 500000, -1, -1, false) == 32768);
    CHECK(tail_threshold(64 * 32768, 500000, -1, -1, true) == 32768);
    CHECK(tail_threshold(64 * 32769, 500000, -1, -1, false) == 32769);
    CHECK(tail_threshold(1 << 24, 500000, -1, -1, false) == (1 << 24) / 64);
    CHECK(tail_threshold(64 * 500000ll, 500000, -1, -1, false) == 500000);
    CHECK(tail_threshold(1 << 27, 500000, -1, -1, false) == 500000);
    CHECK(tail_threshold(1 << 27, 1000, -1, -1, false) == 32768);
}

static void check_refusals() {
    const auto refused = [](const RenderPlanInput& in, const char* msg) {
        const RenderPlan pl = plan_render(in);
        return pl.status == IGX_ERR_INVALID_ARGUMENT && pl.error && std::strcmp(pl.error, msg) == 0;
    };
    RenderPlanInput in = film(64, 64, 0, 1, 0);
    CHECK(refused(in, "spi must be >= 1"));
    in.width = 0; // spi is checked first
    CHECK(refused(in, "spi must be >= 1"));
    in.spi = 1;
    CHECK(refused(in, "film size must be positive"));
    in = film(64, -1, 1, 1, 0);
    CHECK(refused(in, "film size must be positive"));
    in = film(64, 64, 1, 1, 0);
    in.tile_size = 16;
    in.tile_stride = 0;
    CHECK(refused(in, "invalid tile sharding parameters"));
    in.tile_stride = 3;
    in.tile_offset = 3;
    CHECK(refused(in, "invalid tile sharding parameters"));
    in.tile_offset = -1;
    CHECK(refused(in, "invalid tile sharding parameters"));
    in.tile_offset = 2;
    CHECK(plan_render(in).status == IGX_OK && plan_render(in).error == nullptr);
    in.num_rays = 100; // a ray list needs no film size, but takes no tiles
    in.width = in.height = 0;
    CHECK(refused(in, "ray-list mode cannot be tile-sharded"));
    in.tile_size = 0;
    CHECK(plan_render(in).status == IGX_OK && plan_render(in).width == 100 && plan_render(in).height == 1);
}

// Full plans, the expected values worked out from the render driver's
// expressions as they stood before they moved into render_plan.h
struct Parity {
    struct {
        int width, height, num_rays, tile_size, tile_offset, tile_stride, spi, count;
        long long capacity, slot_budget_mb;
        int stream_slots;
        unsigned long long mem_total;
        int classify;
        bool split, aovs;
    } in;
    struct {
        int width, height, tiles_x;
        long long local_pixels, total_paths;
        int classify;
        long long path_slot_bytes, chunk_pixels_max;
        int iters_per_chunk;
        unsigned long long slot_cap;
        long long chunks, last_it0, last_px0, last_n;
    } want;
};
static const Parity PARITY[] = {
    {{100, 100, 0, 0, 0, 0, 2, 3, 20000ll, 0ll, 2, 309237645312ull, 4, false, false},
     {100, 100, 0, 10000ll, 20000ll, 4, 288ll, 10000ll, 1, 20000ull, 3ll, 2ll, 0ll, 20000ll}},
    {{100, 100, 0, 0, 0, 0, 2, 1, 0ll, 0ll, 2, 309237645312ull, 4, false, false},
     {100, 100, 0, 10000ll, 20000ll, 4, 288ll, 10000ll, 1, 20000ull, 1ll, 0ll, 0ll, 20000ll}},
    {{64, 64, 0, 0, 0, 0, 8, 1, 4096ll, 0ll, 2, 309237645312ull, 4, false, false},
     {64, 64, 0, 4096ll, 32768ll, 4, 288ll, 512ll, 1, 4096ull, 8ll, 0ll, 3584ll, 4096ll}},
    {{64, 64, 0, 16, 1, 3, 8, 1, 0ll, 0ll, 2, 309237645312ull, 4, false, false},
     {64, 64, 4, 1280ll, 10240ll, 4, 288ll, 1280ll, 1, 10240ull, 1ll, 0ll, 0ll, 10240ll}},
    {{1024, 1024, 0, 0, 0, 0, 8, 16, 0ll, 0ll, 2, 309237645312ull, 4, false, false},
     {1024, 1024, 0, 1048576ll, 8388608ll, 4, 288ll, 1048576ll, 16, 134217728ull, 1ll, 0ll, 0ll, 134217728ll}},
    {{1024, 1024, 0, 0, 0, 0, 8, 16, 0ll, 0ll, 2, 309237645312ull, 4, true, false},
     {1024, 1024, 0, 1048576ll, 8388608ll, 3, 196ll, 1048576ll, 16, 134217728ull, 1ll, 0ll, 0ll, 134217728ll}},
    {{4096, 4096, 0, 0, 0, 0, 8, 8, 0ll, 0ll, 2, 309237645312ull, 4, false, true},
     {4096, 4096, 0, 16777216ll, 134217728ll, 4, 320ll, 16777216ll, 1, 134217728ull, 8ll, 7ll, 0ll, 134217728ll}},
    {{4096, 4096, 0, 0, 0, 0, 8, 8, 0ll, 0ll, 1, 206158430208ull, 3, false, false},
     {4096, 4096, 0, 16777216ll, 134217728ll, 3, 176ll, 16777216ll, 1, 134217728ull, 8ll, 7ll, 0ll, 134217728ll}},
    {{4096, 4096, 0, 0, 0, 0, 8, 1, 0ll, 0ll, 2, 68719476736ull, 4, false, false},
     {4096, 4096, 0, 16777216ll, 134217728ll, 4, 288ll, 2097152ll, 1, 16777216ull, 8ll, 0ll, 14680064ll, 16777216ll}},
    {{1920, 1080, 0, 64, 3, 8, 4, 5, 0ll, 512ll, 2, 309237645312ull, 4, false, false},
     {1920, 1080, 30, 262144ll, 1048576ll, 4, 288ll, 262144ll, 1, 1048576ull, 5ll, 4ll, 0ll, 1048576ll}},
    {{1920, 1080, 0, 64, 3, 8, 4, 5, 0ll, 1ll, 2, 17179869184ull, 4, true, true},
     {1920, 1080, 30, 262144ll, 1048576ll, 3, 228ll, 262144ll, 1, 1048576ull, 5ll, 4ll, 0ll, 1048576ll}},
    {{0, 0, 4096, 0, 0, 0, 3, 2, 1000ll, 0ll, 2, 309237645312ull, 4, false, false},
     {4096, 1, 0, 4096ll, 12288ll, 4, 288ll, 333ll, 1, 999ull, 26ll, 1ll, 3996ll, 300ll}},
    {{13, 7, 0, 4, 9, 10, 5, 4, 0ll, 0ll, 2, 309237645312ull, 4, false, false},
     {13, 7, 4, 0ll, 0ll, 4, 0ll, 0ll, 0, 0ull, 0ll, 0ll, 0ll, 0ll}},
    {{333, 77, 0, 0, 0, 0, 7, 9, 3ll, 0ll, 2, 309237645312ull, 2, false, false},
     {333, 77, 0, 25641ll, 179487ll, 2, 176ll, 1ll, 1, 7ull, 230769ll, 8ll, 25640ll, 7ll}},
    {{2048, 2048, 0, 0, 0, 0, 64, 4, 0ll, 100000ll, 2, 309237645312ull, 4, false, false},
     {2048, 2048, 0, 4194304ll, 268435456ll, 4, 288ll, 2097152ll, 1, 134217728ull, 8ll, 3ll, 2097152ll, 134217728ll}},
    {{512, 512, 0, 0, 0, 0, 16, 40, 1073741824ll, 0ll, 2, 309237645312ull, 4, false, false},
     {512, 512, 0, 262144ll, 4194304ll, 4, 288ll, 262144ll, 32, 134217728ull, 2ll, 32ll, 0ll, 33554432ll}},
};

static void check_parity() {
    static_assert(sizeof(PARITY) / sizeof(PARITY[0]) >= 12, "at least a dozen plans");
    for (const Parity& p : PARITY) {
        RenderPlanInput in;
        in.width = p.in.width;
        in.height = p.in.height;
        in.num_rays = p.in.num_rays;
        in.tile_size = p.in.tile_size;
        in.tile_offset = p.in.tile_offset;
        in.tile_stride = p.in.tile_stride;
        in.spi = p.in.spi;
        in.count = p.in.count;
        in.capacity = p.in.capacity;
        in.slot_budget_mb = p.in.slot_budget_mb;
        in.stream_slots = p.in.stream_slots;
        in.mem_total = (size_t)p.in.mem_total;
        in.classify = p.in.classify;
        in.split = p.in.split;
        in.aovs = p.in.aovs;
        const RenderPlan pl = plan_render(in);
        CHECK(pl.status == IGX_OK);
        CHECK(pl.width == p.want.width && pl.height == p.want.height && pl.tiles_x == p.want.tiles_x);
        CHECK(pl.local_pixels == p.want.local_pixels && pl.total_paths == p.want.total_paths);
        CHECK(pl.classify == p.want.classify);
        CHECK(pl.path_slot_bytes == p.want.path_slot_bytes && pl.chunk_pixels_max == p.want.chunk_pixels_max);
        CHECK(pl.iters_per_chunk == p.want.iters_per_chunk && pl.slot_cap == p.want.slot_cap);
        const long long chunks = chunk_count(pl);
        CHECK(chunks == p.want.chunks);
        if (chunks > 0 && chunks == p.want.chunks) {
            const Chunk c = plan_chunk(pl, chunks - 1);
            CHECK(c.it0 == p.want.last_it0 && c.px0 == p.want.last_px0 && c.n == p.want.last_n && c.last);
        }
        check_enumeration(in);
    }
}

int main() {
    check_valid_pixels();
    check_enumerations();
    check_auto_chunk();
    check_tail_threshold();
    check_refusals();
    check_parity();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
