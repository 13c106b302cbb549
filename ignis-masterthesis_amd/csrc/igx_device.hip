// MI355X (gfx950) wavefront path-tracing device: kernels + host driver + C-ABI.
//
// Hot path = the reference's per-iteration loop gpu_trace
// (src/artic/driver/mapping_gpu.art:728-870) re-designed for CDNA4:
//   * all paths of one or more iterations are resident in HBM as one wavefront
//     ("chunk", up to 128 M paths) instead of refilling a 1M-ray stream
//     (mapping_gpu.art:1125);
//   * one fused "extend" kernel per bounce does closest-hit traversal AND
//     shading (the reference launches traverse, 3 sort kernels with a host scan,
//     one hit-shade kernel per material, miss shade, then compaction with a D2H
//     sync: mapping_gpu.art:45-68, 403-498, 114-205, 229-266, 685-714); scenes
//     whose tables exceed one XCD's L2 split it into a persistent-lane trace
//     kernel and a shade kernel;
//   * surviving paths and shadow rays are compacted on the fly with a 64-lane
//     ballot and one atomic per wave on one of 64 shard counters (no sort, no
//     host round trip);
//   * shadow rays are traced by a separate any-hit kernel over the compacted
//     shadow stream (gpu_traverse_secondary, mapping_gpu.art:70-112);
//   * the last paths of a chunk run to their end in a tail kernel on a second
//     stream, overlapping the next chunk;
//   * radiance is accumulated per path slot with plain read-modify-writes (each
//     slot is owned by exactly one ray at a time), then a resolve kernel adds
//     sum(L_s)/spi to the framebuffer -- deterministic, no float atomics
//     (the reference splats with atomic adds, driver/accumulator.art:4-21).
#include "igx.h"

#include "device_math.h"
#include "device_scene.h"
#include "igx_kernels.h"
#include "../host/scene_tables.h"
#include "../host/lds_plan.h"
#include "../host/extend_shape.h"
#include "../host/render_plan.h"
#include "../host/aov_plan.h"
#include "../host/film_tools.h"
#include "../host/glare_model.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <type_traits>

using namespace igxd;

// The file is compiled once per part (Makefile: -DIGX_PART=n) so the many
// kernel instantiations build in parallel:
//   0 = host driver, C-ABI and the small kernels; 1 = k_extend variants;
//   2 = k_finish variants; 3 = k_trace / k_trace_refill / k_shade / k_shadow /
//   k_shadow_refill variants; 4 = the wide (BLOCK_WIDE-thread) k_extend variants;
//   5 = the k_infobuffer variants; 6 = the film post-processing kernels
//   (igx_post.h); 7 = the wide k_extend's generate and bounce shapes
//   (host/extend_shape.h); 8, 9 = the two shapes of the BLOCK-thread k_extend
//   with LDS-staged and with global tables; 10 = k_camera_rays (igx_camera_rays).
//   Types and device functions are shared.  A part instantiates a kernel by
//   taking its address, in the choosers it defines under its #if IGX_PART == n
//   (plain functions declared for all parts: "Which instantiation a launch
//   runs", below); part 0 launches, sizes grids and raises LDS limits through
//   what they return and takes no such address itself.
#ifndef IGX_PART
#define IGX_PART 0
#endif

namespace igxh {

constexpr int BLOCK = 256;
// The LDS-staged k_extend also comes with one 1024-thread block per CU: one
// copy of the traversal tables instead of four leaves LDS for the shading
// tables (stage_scene_lds; layout chosen per scene, host/lds_plan.h).  Every
// other kernel runs BLOCK threads.
constexpr int BLOCK_WIDE = LDS_PLAN_BLOCK_WIDE;
static_assert(BLOCK == LDS_PLAN_BLOCK, "host/lds_plan.h plans for BLOCK-thread blocks");
[[maybe_unused]] constexpr int MAX_BLOCKS_PER_CU = 8;  // 2048 threads per CU; grids never exceed num_cus * this
constexpr int MAX_BOUNCES = 256;          // path depth is stored in 8 bits (p1.w, above the 24-bit RNG counter)
// MAX_CHUNK_PATHS (paths per chunk, one wavefront) lives in host/render_plan.h
// a path's slot in its chunk takes the low 27 bits of the slot word; the top
// 5 carry 1 + the index of the enclosing entity it is in (at most MAX_ENCLOSING)
constexpr int SLOT_BITS = 27;
constexpr uint32_t SLOT_MASK = (1u << SLOT_BITS) - 1;
static_assert(MAX_CHUNK_PATHS <= (1ll << SLOT_BITS), "path slots must fit the slot bits");
// Occupancy target (waves per SIMD) of k_extend, with global and with
// LDS-staged traversal tables: 4 caps it at 128 VGPRs.  k_finish keeps the
// compiler's choice (it would spill).
#ifndef EXTEND_WAVES
#define EXTEND_WAVES 4
#endif
// the full shading variant on global tables: 3 waves per SIMD (no spills)
// instead of 4 (~150 spilled VGPRs): materials frame 55.3 -> 54.0 ms; the
// basic variant stays at 4 (S-deep 31.5 -> 36.1, primitives 22.0 -> 24.3 ms
// at 3), profiles/r02_ab_extend_waves.log
#ifndef EXTEND_WAVES_FULL
#define EXTEND_WAVES_FULL 3
#endif
#ifndef EXTEND_WAVES_LDS
#define EXTEND_WAVES_LDS 4
#endif


// ---------------------------------------------------------------------------
// Streams (SoA of 16-byte records)
// ---------------------------------------------------------------------------
// Every compacted stream is cut into NSH shards of `shard_cap` records
// (record (s, pos) at index s * shard_cap + pos), each with its own counter:
// a wave appends to the shard of its global wave index, so the append is one
// returning atomic per wave on a word shared by 1/NSH of the waves, and no
// block barrier holds a wave behind the slowest of its block.
constexpr int NSH = 64;             // shards per stream (one per lane of the counting wave)
constexpr int CSTRIDE = 16;         // ints between two shard counters: one 64-B atomic line each
constexpr int CROW = NSH * CSTRIDE; // ints per counter row (one row per stream and bounce)
constexpr int WAVES_PER_BLOCK = BLOCK / 64;
// k_trace_refill stages no treelet: its top nodes stay L2 hits anyway, and
// without one its node fetches are global loads instead of the flat loads
// that serve LDS and global addresses alike (soup-1M 8-iteration frame
// 315.8 / 313.5 -> 305.6 / 307.2 ms, soup-16M 118.2 -> 117.9 ms;
// profiles/r03_ab_trace_global.log).  k_finish_pairs stages none either
// (soup-16M k_finish_pairs 6.0 -> 8.5 ms with one, r05_ab_finish_treelet.log).
// k_extend and the shadow kernels on global-table scenes: LDS treelet (1)
// or none and global node loads (0)
#ifndef EXTEND_TREELET
#define EXTEND_TREELET 1
#endif
#ifndef SHADOW_TREELET
#define SHADOW_TREELET 1
#endif
// k_extend's dynamic groups: the append's atomic round trip also takes the
// wave's next group (1, wave_append_paths) or take_group issues its own (0)
#ifndef IGX_CLAIM_NEXT
#define IGX_CLAIM_NEXT 1
#endif
// bounce b >= 2 launches a grid sized to the paths entering bounce b - 1 (1)
// instead of the chunk's first-bounce grid (0)
#ifndef IGX_LIVE_GRID
#define IGX_LIVE_GRID 1
#endif
[[maybe_unused]] constexpr int GRID_QUANTUM = NSH / WAVES_PER_BLOCK; // grids are multiples of this: every shard gets the same waves

struct PathBuf {
    float4* p0; // org.xyz, slot (int bits; bits 27-31: 1 + the enclosing entity index the path is in, 0: none)
    float4* p1; // dir.xyz, rnd counter
    float4* p2; // contrib.rgb, inv_pdf
    float2* p3; // eta, RNG seed (uint bits): hashed once by k_generate, not per bounce
    int shard_cap;
    int c_base; // record index of the class-C region (FrameArgs::classify 4), 0: none
};
struct ShadowBuf {
    float4* s0; // org.xyz, slot
    float4* s1; // dir.xyz, tmax
    float4* s2; // colour.rgb, -: added to the slot if the ray is unoccluded; for a class-A record
                // under `optimistic` the slot's value before k_extend added the colour (undo.rgb, -),
                // stored back to the slot if the ray is occluded
    int shard_cap;
    float4* aov_nee; // "NEE Weights" per path slot (technique aov_mis), nullptr: off
    int optimistic;  // FrameArgs::shadow_optimistic of the launch that wrote the records
};
struct HitBuf {
    float4* h;  // t, u, v, entity (int bits; -1 = miss)
    int* prim;  // primitive id
};

#ifndef IGX_AOV
#define IGX_AOV 1 // 0: experiment builds without the AOV code (its cost on the default path)
#endif
struct FrameArgs {
    int width, height, spi, iter, frame, seed;
    int tile_size, tile_offset, tile_stride, tiles_x;
    int num_rays;
    const float* rays;   // device copy of the ray list (ray-list mode)
    int chunk_pixel0;    // first local pixel of this chunk
    int chunk_pixels;    // local pixels in this chunk
    int chunk_iters;     // consecutive iterations (iter, iter + 1, ...) the chunk covers
    float inv_spi;
    int gen_n;           // > 0: this k_extend launch is bounce 0 and generates its n camera paths itself
    int classify;        // surviving paths' stream class (see wave_append_paths): 0 all A, 1 B = inside a dielectric (eta != 1), 2 B = after a specular event
    int dynamic;         // k_extend: waves take 64-path groups from per-shard work counters (KernelCounters::work)
    int shadow_classes;  // shadow rays crossing an enclosing entity's box go to the back of their shard (shadow_class_b)
    int shadow_optimistic; // k_extend adds a class-A shadow ray's colour to the radiance slot itself and leaves the
                         // slot's previous value in the record; the shadow kernel restores it if the ray is occluded
    int reverse;         // k_extend: a shard's positions are taken from its end (class C, then B, then A:
                         // the groups whose paths run longest start first, the short ones fill the launch's end)
    int probe_sample;    // test hook (option "probe_sample"): 0 = k_resolve adds every sample; s + 1 = sample s only
    // the path tracer's MIS AOVs (technique aov_mis, PathTechnique.cpp:16-25):
    // per path slot beside L, "Direct Weights" = emission hits and misses
    // (pathtracer.art:128,158), "NEE Weights" = unoccluded shadow rays (:206);
    // nullptr: off (the default path pays one scalar branch per add)
    float4* aov_di;
    float4* aov_nee;
};

// path slot -> (local pixel, sample, iteration): slots run over the chunk's
// pixels x spi samples, one such block per iteration of the chunk
__device__ __forceinline__ void slot_coords(const FrameArgs& fa, int slot, int& lp, int& sample, int& iter) {
    const int per_iter = fa.chunk_pixels * fa.spi;
    const int it = slot / per_iter;
    const int r = slot - it * per_iter;
    const int q = r / fa.spi;
    lp = fa.chunk_pixel0 + q;
    sample = r - q * fa.spi;
    iter = fa.iter + it;
}

// local pixel -> global (x, y); false if the slot lies outside the film
// Pixel order of the local pixel index: eight consecutive pixels (one wave's
// camera group at spi 8) form a 4 x 2 block instead of a 1 x 8 row run, when
// the width (tile side) is a multiple of 4 and the height even: the group's
// camera rays then diverge less in the traversal (IGX_PIXEL_BLOCKS).  Every
// user of the index (generation, resolve, tile packing) maps it here, and a
// path's arithmetic depends on its pixel only, so the film is the same.
// (the macro's default: device_scene.h, shared with host/render_plan.h)
__device__ __forceinline__ void block_order(int r, int w, int& x, int& y) {
    const int pair = r / (2 * w), q = r - pair * 2 * w; // row pair, index in it
    x = (q >> 3) * 4 + (q & 3);
    y = 2 * pair + ((q >> 2) & 1);
}
// BLOCKED false: the row-major order (the packed tile layout of igx_pack_tiles)
template <bool BLOCKED = true>
__device__ __forceinline__ bool local_to_global(const FrameArgs& fa, int lp, int& x, int& y) {
    if (fa.num_rays > 0) { x = lp; y = 0; return lp < fa.num_rays; }
    if (fa.tile_size <= 0) {
        if (BLOCKED && IGX_PIXEL_BLOCKS && (fa.width & 3) == 0 && (fa.height & 1) == 0) block_order(lp, fa.width, x, y);
        else { y = lp / fa.width; x = lp - y * fa.width; }
        return true;
    }
    int T = fa.tile_size;
    int k = lp / (T * T);
    int r = lp - k * T * T;
    int ty, tx;
    if (BLOCKED && IGX_PIXEL_BLOCKS && (T & 3) == 0) block_order(r, T, tx, ty);
    else { ty = r / T; tx = r - ty * T; }
    int t = fa.tile_offset + k * fa.tile_stride;
    int tyy = t / fa.tiles_x, txx = t - tyy * fa.tiles_x;
    x = txx * T + tx;
    y = tyy * T + ty;
    return x < fa.width && y < fa.height;
}

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

template <typename T>
__device__ __forceinline__ T uniform_load(const T* p) {
    return __builtin_amdgcn_readfirstlane(*p);
}

// ---------------------------------------------------------------------------
// Sharded streams (see PathBuf)
// ---------------------------------------------------------------------------
static_assert(NSH == 64 && BLOCK % 64 == 0 && NSH % WAVES_PER_BLOCK == 0, "one shard counter per lane of a wave");
static_assert(BLOCK == TSTACK_STRIDE, "traversal stacks are laid out for BLOCK threads");

// Records of all shards of a counter row: lane l reads shard l; wave-uniform.
// A path-stream counter is two words (class A records from the front of the
// shard, class B from its back, wave_append_paths); other streams leave the
// second word 0.
__device__ __forceinline__ int row_total(const int* row) {
    const int* r = row + lane_id() * CSTRIDE;
    int v = r[0] + r[1] + r[2];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return __builtin_amdgcn_readfirstlane(v);
}

// Wave g of the grid's G waves serves shard s = g % NSH, as the k-th of the
// K = G / NSH waves of that shard (grids are multiples of GRID_QUANTUM blocks).
struct WaveWork {
    int s, k, K;
};
// BT: threads per block of the launch (grids are multiples of NSH / (BT / 64) blocks)
template <int BT = BLOCK>
__device__ __forceinline__ WaveWork wave_work() {
    constexpr int WPB = BT / 64;
    static_assert(BT % 64 == 0 && NSH % WPB == 0, "a block's waves divide the shards");
    const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPB + (int)(threadIdx.x >> 6));
    return WaveWork{g % NSH, g / NSH, (int)gridDim.x * WPB / NSH};
}

// Storage index of path i of a freshly generated chunk: consecutive groups of
// 64 paths go round-robin to the shards, so every wave of the first bounce
// reads 64 neighbouring paths (8 pixels x spi 8).
__device__ __forceinline__ int gen_index(int i, int shard_cap) {
    return ((i >> 6) & (NSH - 1)) * shard_cap + ((i >> 12) << 6) + (i & 63);
}
// Shard counts of a generated chunk of n paths (written by lanes 0..NSH-1).
__device__ __forceinline__ int gen_shard_count(int n, int s) {
    const int rem = (n & (64 * NSH - 1)) - s * 64;
    return (n >> 12) * 64 + (rem < 0 ? 0 : (rem > 64 ? 64 : rem));
}

// Records of path-stream shard s: `a` of class A at offsets [0, a) and ab - a
// of class B at offsets shard_cap - 1 down to shard_cap - (ab - a); with a
// class-C region (PathBuf::c_base, FrameArgs::classify 4) n - ab of class C
// at its offsets [0, n - ab).  Position pos in [0, n) of the shard maps to
// stream index path_index(...) (stream_index for two-class streams), so
// consecutive positions, and so the 64 paths of one wave, share a class.
struct ShardCount {
    int a, ab, n;
};
__device__ __forceinline__ ShardCount shard_count(const int* cnt, int s) {
    const int a = uniform_load(cnt + s * CSTRIDE), b = uniform_load(cnt + s * CSTRIDE + 1);
    const int c = uniform_load(cnt + s * CSTRIDE + 2);
    return ShardCount{a, a + b, a + b + c};
}
__device__ __forceinline__ int stream_index(int s, int pos, int a, int shard_cap) {
    return s * shard_cap + (pos < a ? pos : shard_cap - 1 - (pos - a));
}
__device__ __forceinline__ int path_index(const PathBuf& b, int s, int pos, const ShardCount& sc) {
    return pos < sc.ab ? stream_index(s, pos, sc.a, b.shard_cap) : b.c_base + s * b.shard_cap + (pos - sc.ab);
}

// Wave-level compaction of the surviving paths (class A appended from the
// front of the wave's shard, class B from its back, class C from the front
// of the shard's class-C region: the next bounce's waves then trace paths of
// one class, e.g. all inside a dielectric) and of the shadow rays (A front,
// B back): one returning 64-bit atomic per counter (a/b counts in its two
// words; the class-C count in word 2), lanes 0-2 issue them in one
// instruction; positions inside the wave by ballot prefix.  `dst` is the
// record offset from the start of the shard (c_base added for class C).
// Needs every lane of the wave active.
// `claim` (k_extend's dynamic groups): lane 3 also takes the wave's next group
// of its shard from that shard's work counter in the same round trip
// (`claimed`, wave-uniform; -1 without `claim`), so the next group's path
// loads follow the stores without a second returning atomic in between.
__device__ __forceinline__ void wave_append_paths(bool alive, int cls, bool shadow, bool sh_b, int* cp, int* cs,
                                                  int shard_cap, int c_base, int sh_cap, int& dst, int& sdst,
                                                  int* claim = nullptr, int* claimed = nullptr) {
    const int lane = lane_id();
    const uint64_t ma = __ballot(alive && cls == 0), mb = __ballot(alive && cls == 1), mc = __ballot(alive && cls == 2);
    const uint64_t sa = __ballot(shadow && !sh_b), sb = __ballot(shadow && sh_b);
    const uint64_t below = (1ull << lane) - 1ull;
    const unsigned long long want = lane == 0   ? ((unsigned long long)__popcll(ma) | ((unsigned long long)__popcll(mb) << 32))
                                    : lane == 1 ? ((unsigned long long)__popcll(sa) | ((unsigned long long)__popcll(sb) << 32))
                                                : (unsigned long long)__popcll(mc);
    unsigned long long r = 0;
    int nx = 0;
    if (lane < 3 && want != 0) r = atomicAdd(reinterpret_cast<unsigned long long*>(lane == 0 ? cp : lane == 1 ? cs : cp + 2), want);
    if (claim && lane == 3) nx = atomicAdd(claim, 1);
    if (claim) *claimed = __builtin_amdgcn_readfirstlane(__shfl(nx, 3));
    const int lo = (int)(uint32_t)r, hi = (int)(uint32_t)(r >> 32);
    const int a0 = __shfl(lo, 0), b0 = __shfl(hi, 0), s0 = __shfl(lo, 1), t0 = __shfl(hi, 1), c0 = __shfl(lo, 2);
    dst = cls == 1   ? shard_cap - 1 - (b0 + __popcll(mb & below))
          : cls == 2 ? c_base + c0 + __popcll(mc & below)
                     : a0 + __popcll(ma & below);
    sdst = sh_b ? sh_cap - 1 - (t0 + __popcll(sb & below)) : s0 + __popcll(sa & below);
}
// wave_append_paths in two halves (k_extend's generate and bounce shapes): the
// first issues the one returning atomic (counters and claim), the second
// turns its results into the lanes' positions.  The compiled kernel waits
// for the atomic right behind it (the radiance sum needs the load issued
// ahead of it, and a load and an atomic under lane branches are waited for
// together), so nothing overlaps the round trip but the load.  Same counters,
// same counts, same positions as wave_append_paths.
struct AppendIssued {
    uint64_t ma, mb, mc, sa, sb; // ballots: path classes A, B, C, shadow classes A, B
    unsigned long long r;        // lanes 0-2: the counters' previous values, lane 3: the claimed group
};
__device__ __forceinline__ AppendIssued wave_append_issue(bool alive, int cls, bool shadow, bool sh_b, int* cp, int* cs, int* claim) {
    const int lane = lane_id();
    AppendIssued t;
    t.ma = __ballot(alive && cls == 0), t.mb = __ballot(alive && cls == 1), t.mc = __ballot(alive && cls == 2);
    t.sa = __ballot(shadow && !sh_b), t.sb = __ballot(shadow && sh_b);
    // lane 3 takes the next group in the same instruction: a 64-bit add of 1
    // to the shard's work counter, whose line holds nothing else (its upper
    // word stays 0: the rows are cleared per chunk and a counter stays far
    // below 2^32), so the lower word of the result is what atomicAdd(claim, 1)
    // returns.  One returning atomic per group, and none whose result the
    // compiler's wave-level rewrite of a uniform atomic would need at once.
    const unsigned long long want = lane == 0   ? ((unsigned long long)__popcll(t.ma) | ((unsigned long long)__popcll(t.mb) << 32))
                                    : lane == 1 ? ((unsigned long long)__popcll(t.sa) | ((unsigned long long)__popcll(t.sb) << 32))
                                    : lane == 2 ? (unsigned long long)__popcll(t.mc)
                                                : (claim ? 1ull : 0ull);
    t.r = 0;
    if (lane < 4 && want != 0)
        t.r = atomicAdd(reinterpret_cast<unsigned long long*>(lane == 0 ? cp : lane == 1 ? cs : lane == 2 ? cp + 2 : claim), want);
    return t;
}
__device__ __forceinline__ void wave_append_finish(const AppendIssued& t, int cls, bool sh_b, int shard_cap, int c_base, int sh_cap,
                                                   int& dst, int& sdst, bool claim, int& claimed) {
    const uint64_t below = (1ull << lane_id()) - 1ull;
    const int lo = (int)(uint32_t)t.r, hi = (int)(uint32_t)(t.r >> 32);
    claimed = claim ? __builtin_amdgcn_readfirstlane(__shfl(lo, 3)) : -1;
    const int a0 = __shfl(lo, 0), b0 = __shfl(hi, 0), s0 = __shfl(lo, 1), t0 = __shfl(hi, 1), c0 = __shfl(lo, 2);
    dst = cls == 1   ? shard_cap - 1 - (b0 + __popcll(t.mb & below))
          : cls == 2 ? c_base + c0 + __popcll(t.mc & below)
                     : a0 + __popcll(t.ma & below);
    sdst = sh_b ? sh_cap - 1 - (t0 + __popcll(t.sb & below)) : s0 + __popcll(t.sa & below);
}
// Record at byte offset `off` of an array whose base is wave-uniform (the
// shapes: every array of a stream is at most 4 GiB, streams_offsets_32bit of
// host/extend_shape.h, so a lane's address is the scalar base plus a 32-bit
// offset and needs no 64-bit arithmetic per lane)
template <class T>
__device__ __forceinline__ T* rec_at(T* base, uint32_t off) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off);
}



// ---------------------------------------------------------------------------
// generate: camera rays (gpu_generate_rays, mapping_gpu.art:618-667;
// make_camera_emitter, driver/emitter.art:6-16; perspective camera,
// camera/perspective.art:29-42; uniform pixel sampler, sampler/pixel_sampler.art:4-10).
// Slot i of the chunk holds path i; no compaction (tile padding slots are
// written as dead paths with depth 0), so no atomics.
// ---------------------------------------------------------------------------
// Path i of the chunk at its camera vertex (k_generate, and k_extend's fused
// bounce 0).  Path state layout: see PathState below.
struct GenPath {
    f3 o, d;
    uint32_t counter, seed;
    int depth;
};
// FULL (the full shading variant) goes through camera_ray (host/camera_model.h:
// every camera model; the depth-of-field camera draws its two lens numbers
// after the jitter).  The basic variant keeps the pinhole perspective camera's
// own statement, so its kernels are the ones they were before the other models
// came; camera_ray's pinhole branch is the same arithmetic (a GPU test compares
// the two bit for bit).
template <bool FULL>
__device__ __forceinline__ GenPath gen_path(const FrameArgs& fa, const SceneView& sv, int i) {
    int lp, sample, iter;
    slot_coords(fa, i, lp, sample, iter);
    int x, y;
    GenPath g{mk(0, 0, 0), mk(0, 0, 1), 1, 0, 0}; // depth 0: dead (tile padding)
    if (local_to_global(fa, lp, x, y)) {
        g.depth = 1;
        g.seed = create_random_seed(sample, iter, fa.frame, x, y, fa.seed);
        Rng rnd{g.seed, 1};
        if (fa.num_rays > 0) {
            // make_list_emitter (driver/emitter.art:18-30): no random draws
            const float* r = fa.rays + 8 * x;
            g.o = mk(r[0], r[1], r[2]);
            g.d = mk(r[3], r[4], r[5]);
        } else {
            float rx = rnd.next_f32();
            float ry = rnd.next_f32();
            float nx = 2 * ((float)x + rx) / (float)fa.width - 1;
            float ny = 1 - 2 * ((float)y + ry) / (float)fa.height;
            if constexpr (FULL) {
                const DevLens lens{sv.cam_type, sv.cam_aperture, sv.cam_focal};
                float lu = 0, lv = 0;
                if (camera_has_dof(lens)) {
                    lu = rnd.next_f32();
                    lv = rnd.next_f32();
                }
                CamVec o, d;
                camera_ray(sv.cam, lens, nx, ny, lu, lv, o, d);
                g.o = mk(o.x, o.y, o.z);
                g.d = mk(d.x, d.y, d.z);
            } else {
                const DevCamera& c = sv.cam;
                f3 v = mk(c.scale_x * nx, c.scale_y * ny, 1);
                f3 w = mk(c.right[0] * v.x + c.up[0] * v.y + c.dir[0] * v.z,
                          c.right[1] * v.x + c.up[1] * v.y + c.dir[1] * v.z,
                          c.right[2] * v.x + c.up[2] * v.y + c.dir[2] * v.z);
                g.o = mk(c.eye[0], c.eye[1], c.eye[2]);
                g.d = normalize(w);
            }
        }
        g.counter = rnd.counter;
    }
    return g;
}

#if IGX_PART == 10
// The camera rays of one sample of every pixel (igx_camera_rays): one lane
// per pixel, grid-stride, through gen_path, so the rays are the renderer's.
// `fa` describes one chunk of the whole film at spi = sample + 1, so slot
// lp * spi + sample is that sample of local pixel lp.  Row-major, 8 floats
// per pixel: org, dir, tmin, tmax.
__global__ void __launch_bounds__(BLOCK) k_camera_rays(FrameArgs fa, SceneView sv, float4* rays) {
    const int sample = fa.spi - 1;
    for (int lp = blockIdx.x * BLOCK + threadIdx.x; lp < fa.chunk_pixels; lp += gridDim.x * BLOCK) {
        int x, y;
        if (!local_to_global(fa, lp, x, y)) continue;
        const GenPath g = gen_path<true>(fa, sv, lp * fa.spi + sample);
        const size_t p = (size_t)y * fa.width + x;
        rays[2 * p] = make_float4(g.o.x, g.o.y, g.o.z, g.d.x);
        rays[2 * p + 1] = make_float4(g.d.y, g.d.z, sv.cam.tmin, sv.cam.tmax);
    }
}
#endif

#if IGX_PART == 0
template <bool FULL>
__device__ __forceinline__ void generate_paths(const FrameArgs& fa, const SceneView& sv, const PathBuf& out, float4* L, int* cnt0) {
    const int n = fa.chunk_pixels * fa.spi * fa.chunk_iters;
    if (blockIdx.x == 0 && threadIdx.x < NSH) cnt0[threadIdx.x * CSTRIDE] = gen_shard_count(n, threadIdx.x);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        L[i] = make_float4(0, 0, 0, 0);
        if (IGX_AOV && fa.aov_di) fa.aov_di[i] = fa.aov_nee[i] = make_float4(0, 0, 0, 0);
        const GenPath g = gen_path<FULL>(fa, sv, i);
        const int e = gen_index(i, out.shard_cap);
        out.p0[e] = make_float4(g.o.x, g.o.y, g.o.z, __int_as_float(i));
        out.p1[e] = make_float4(g.d.x, g.d.y, g.d.z, __uint_as_float(g.counter | ((uint32_t)g.depth << 24)));
        out.p2[e] = make_float4(1, 1, 1, 0); // init_pt_raypayload (technique/pathtracer.art:33-38)
        out.p3[e] = make_float2(1.0f, __uint_as_float(g.seed));
    }
}
// the basic and the full shading variant's camera models (gen_path)
__global__ void __launch_bounds__(BLOCK) k_generate(FrameArgs fa, SceneView sv, PathBuf out, float4* L, int* cnt0) {
    generate_paths<false>(fa, sv, out, L, cnt0);
}
__global__ void __launch_bounds__(BLOCK) k_generate_full(FrameArgs fa, SceneView sv, PathBuf out, float4* L, int* cnt0) {
    generate_paths<true>(fa, sv, out, L, cnt0);
}

#endif

// ---------------------------------------------------------------------------
// One bounce of one path: closest hit + technique (gpu_traverse_primary +
// gpu_hit_shade + gpu_miss_shade, restating technique/pathtracer.art:52-200
// on_hit / on_shadow / on_bounce / on_miss).  Shared by the wavefront extend
// kernel and the tail kernel, so both produce bit-identical paths.
// ---------------------------------------------------------------------------
struct KernelCounters {
    int* cnt_in;
    int* cnt_out;
    int* cnt_shadow;
    unsigned long long* stats; // instrumentation counters (igx_get_stats: visits 0-12, phase clocks 16-19)
    int* work;                 // per-shard group counters of this bounce (FrameArgs::dynamic)
};

struct PathState {
    f3 o, d;
    uint32_t counter, seed;
    f3 contrib;
    float inv_pdf, eta;
    int slot, depth;
    int inside; // index of the enclosing entity the path travels in (trace_enclosed), -1: none known
};

struct ShadowRec {
    f3 o, d, color;
    float tmax;
};

// stream class of a surviving path (FrameArgs::classify): 1 B = inside a
// dielectric (eta != 1); 2 B = after a specular event; 3 B = inside a
// dielectric or its next ray crosses the world box of an enclosing entity
// (the paths whose traversal enters a large BLAS and that will likely shade
// a dielectric), A = the rest (wall-to-wall paths: short walks, diffuse)
// (the class only orders the stream, so the slab test may use the hardware
// reciprocal, v_rcp_f32, instead of three IEEE divisions)
__device__ __forceinline__ f3 fast_rcp3(f3 d) {
    return mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
}
__device__ __forceinline__ bool crosses_enclosing_box(const SceneView& sv, f3 o, f3 d) {
    const f3 id = fast_rcp3(d);
    bool hit = false;
    for (int k = 0; k < sv.num_enc && !hit; ++k) {
        const float4 lo = sv.enc_box[2 * k], hi = sv.enc_box[2 * k + 1];
        const float ax = (lo.x - o.x) * id.x, bx = (hi.x - o.x) * id.x;
        const float ay = (lo.y - o.y) * id.y, by = (hi.y - o.y) * id.y;
        const float az = (lo.z - o.z) * id.z, bz = (hi.z - o.z) * id.z;
        const float en = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
        const float ex = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
        hit = en <= ex && ex >= 0.0f;
    }
    return hit;
}
// shadow-ray class (FrameArgs::classify 3): B = the segment [0, tmax] of the
// shadow ray crosses an enclosing entity's box (its any-hit walk enters that
// BLAS), A = the rest; stored like the path classes (shard front / back)
__device__ __forceinline__ bool shadow_class_b(int enabled, const SceneView& sv, f3 o, f3 d, float tmax) {
    if (!enabled) return false;
    const f3 id = fast_rcp3(d);
    bool hit = false;
    for (int k = 0; k < sv.num_enc && !hit; ++k) {
        const float4 lo = sv.enc_box[2 * k], hi = sv.enc_box[2 * k + 1];
        const float ax = (lo.x - o.x) * id.x, bx = (hi.x - o.x) * id.x;
        const float ay = (lo.y - o.y) * id.y, by = (hi.y - o.y) * id.y;
        const float az = (lo.z - o.z) * id.z, bz = (hi.z - o.z) * id.z;
        const float en = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
        const float ex = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
        hit = en <= ex && ex >= 0.0f && en <= tmax;
    }
    return hit;
}
// 4: three classes, C = inside a dielectric, B = its next ray crosses an
// enclosing entity's world box, A = the rest (the fused schedule only: the
// split schedule's hit records have no class-C region)
__device__ __forceinline__ int path_class(int classify, const SceneView& sv, const PathState& ps) {
    switch (classify) {
    case 1: return ps.eta != 1.0f;
    case 2: return ps.inv_pdf == 0.0f;
    case 3: return ps.eta != 1.0f || crosses_enclosing_box(sv, ps.o, ps.d);
    case 4: return ps.eta != 1.0f ? 2 : crosses_enclosing_box(sv, ps.o, ps.d);
    default: return 0;
    }
}

// crosses_enclosing_box of the bounced ray (direction pd, lanes `test_p`) and
// shadow_class_b of the shadow ray (direction sd, segment [0, stmax], lanes
// `test_s`) in one pass over the enclosing boxes, without a branch per lane
// (k_extend's shapes): both rays leave the same point o, so a box is read
// once and its origin-relative corners serve both slab tests, and a ray's
// result is the OR over the boxes where the two loops leave at the first
// hit.  Per ray the float operations are those of the two predicates, in
// their order, so every ray gets the class it gets there.  A wave with no
// lane to test skips the pass by a scalar branch.
__device__ __forceinline__ void class_pass(const SceneView& sv, f3 o, bool test_p, f3 pd, bool test_s, f3 sd, float stmax,
                                           bool& p_hit, bool& s_hit) {
    p_hit = s_hit = false;
    if (sv.num_enc <= 0 || !__ballot(test_p || test_s)) return;
    const f3 ip = fast_rcp3(pd), is = fast_rcp3(sd);
    // one box per trip: the loop vectoriser otherwise takes two boxes at once
    // with packed f32 operations (v_pk_add_f32 / v_pk_mul_f32, 18 of them and
    // the moves that build their register pairs), which cost a wave what the
    // two unpacked operations do (tools/vpk_probe.hip)
#pragma clang loop vectorize(disable)
    for (int k = 0; k < sv.num_enc; ++k) {
        const float4 lo = sv.enc_box[2 * k], hi = sv.enc_box[2 * k + 1];
        const float lx = lo.x - o.x, hx = hi.x - o.x, ly = lo.y - o.y, hy = hi.y - o.y, lz = lo.z - o.z, hz = hi.z - o.z;
        {
            const float ax = lx * ip.x, bx = hx * ip.x, ay = ly * ip.y, by = hy * ip.y, az = lz * ip.z, bz = hz * ip.z;
            const float en = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
            const float ex = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
            p_hit |= en <= ex && ex >= 0.0f;
        }
        {
            const float ax = lx * is.x, bx = hx * is.x, ay = ly * is.y, by = hy * is.y, az = lz * is.z, bz = hz * is.z;
            const float en = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
            const float ex = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
            s_hit |= en <= ex && ex >= 0.0f && en <= stmax;
        }
    }
    p_hit = p_hit && test_p;
    s_hit = s_hit && test_s;
}

__device__ __forceinline__ PathState path_from_records(float4 p0, float4 p1, float4 p2, float2 p3) {
    PathState s;
    s.o = f3of(p0);
    s.d = f3of(p1);
    const uint32_t sw = __float_as_uint(p0.w);
    s.slot = (int)(sw & SLOT_MASK);
    s.inside = (int)(sw >> SLOT_BITS) - 1;
    const uint32_t cd = __float_as_uint(p1.w);
    s.depth = (int)(cd >> 24);
    s.counter = cd & 0xFFFFFFu;
    s.contrib = f3of(p2);
    s.inv_pdf = p2.w;
    s.eta = p3.x;
    s.seed = __float_as_uint(p3.y);
    return s;
}
__device__ __forceinline__ PathState load_path(const PathBuf& in, int i) {
    return path_from_records(in.p0[i], in.p1[i], in.p2[i], in.p3[i]);
}

__device__ __forceinline__ void store_path(const PathBuf& out, int i, const PathState& s) {
    out.p0[i] = make_float4(s.o.x, s.o.y, s.o.z, __uint_as_float((uint32_t)s.slot | ((uint32_t)(s.inside + 1) << SLOT_BITS)));
    out.p1[i] = make_float4(s.d.x, s.d.y, s.d.z, __uint_as_float(s.counter | ((uint32_t)s.depth << 24)));
    out.p2[i] = make_float4(s.contrib.x, s.contrib.y, s.contrib.z, s.inv_pdf);
    out.p3[i] = make_float2(s.eta, __uint_as_float(s.seed));
}

__device__ __forceinline__ f3 handle_color(const SceneView& sv, f3 c) {
    if (sv.clamp > 0) return mk(fminf(c.x, sv.clamp), fminf(c.y, sv.clamp), fminf(c.z, sv.clamp));
    return c;
}

// Ray interval and visibility flags of the ray a path traces at its current
// vertex (camera / list ray at depth 1, bounce ray with the 0.001 offset
// afterwards; pathtracer.art:41, ray.art:21).
__device__ __forceinline__ void ray_extent(const FrameArgs& fa, const SceneView& sv, int depth, int slot, float& tmin,
                                           float& tmax, uint32_t& rflags) {
    if (depth == 1) {
        if (fa.num_rays > 0) {
            int lp, sample, iter;
            slot_coords(fa, slot, lp, sample, iter);
            tmin = fa.rays[8 * lp + 6];
            tmax = fa.rays[8 * lp + 7];
            rflags = 0;
        } else {
            tmin = sv.cam.tmin;
            tmax = sv.cam.tmax;
            rflags = RAY_CAMERA;
        }
    } else {
        tmin = 0.001f; // offset (pathtracer.art:41)
        tmax = FLT_MAX_;
        rflags = RAY_BOUNCE;
    }
}

// Shades the closest hit (or miss, hit_ent < 0) of the path's current ray and
// advances `ps` by one bounce.  Returns whether the path continues (ps then
// holds the bounced ray); fills the radiance gathered at this vertex (Lacc,
// has_l) and the NEE shadow ray (has_shadow, sr).
// A textured diffuse reflectance at the hit (DevMaterial::pad): the checker
// select(checkerboard(uvw * scale) == 1, kd1, kd) of texture/checkerboard.art:2
// on the texture coordinates (u, v, 0), interpolated with the hit's
// barycentrics (vec2_lerp2, shapes/trimesh.art:25; core/vector.art:150-153);
// math::wrap(x, 0, 2) as i32 % 2 per axis (core/math.art:88-91); or an image
// texture (texture/image.art)
__device__ __forceinline__ int checker_bit(float x) {
    const float w = x - 2.0f * floorf(x / 2.0f);
    return ((int)w) % 2;
}
__device__ __forceinline__ void apply_texture(const SceneView& sv, DevMaterial& m, int ent_id, int prim, float hu, float hv) {
    const int kind = __float_as_int(m.pad[0]);
    if (kind != 1 && kind != 2) return;
    const int4 info = *reinterpret_cast<const int4*>(sv.ent + ENT_STRIDE * ent_id + 6); // shape type, material, vtx_off, idx_off
    if (info.x == 1) return; // analytic sphere: refused at upload
    const int4 f = sv.idx[info.w + prim];
    const float2 t0 = sv.uv[info.z + f.x], t1 = sv.uv[info.z + f.y], t2 = sv.uv[info.z + f.z];
    const float u = lerp2(t0.x, t1.x, t2.x, hu, hv), v = lerp2(t0.y, t1.y, t2.y, hu, hv);
    if (kind == 2) {
        // An image texture (host/image_texture.h): pad[1..6] its 2x3 uv transform,
        // pad[7] the place of its TexRecord in the uv table, which names filter,
        // wrap, size and texels.  The colour replaces kd (diffuse reflectance,
        // principled base_color); alpha is not used.
        const TexRecord rec = *reinterpret_cast<const TexRecord*>(sv.uv + __float_as_uint(m.pad[7]));
        const void* const texels = sv.uv + rec.texels;
        float tu, tv;
        tex_transform(&m.pad[1], u, v, tu, tv);
        const Texel c = tex_filter(rec.filter, rec.wrap_u, rec.wrap_v, rec.width, rec.height, tu, tv,
                                   [&](int x, int y) { return tex_fetch(rec.format, texels, rec.width, x, y); });
        m.kd[0] = c.r;
        m.kd[1] = c.g;
        m.kd[2] = c.b;
        return;
    }
    const float sc = m.pad[1];
    // node_checkerboard3(uvw * sc): ((a == b) == (c == 1)) with c of the zero w
    const int a = checker_bit(u * sc), b = checker_bit(v * sc), c = checker_bit(0.0f * sc);
    if ((a == b) == (c == 1)) {
        m.kd[0] = m.pad[2];
        m.kd[1] = m.pad[3];
        m.kd[2] = m.pad[4];
    }
}

// Shading sub-phase clock of the instrumented k_extend (CLK): the wave's
// shader clock since the previous mark goes to sub-phase k of its group's
// class (cls[20 + 4 * bucket + k]); marks sit in the hit path, executed by
// the wave for its active lanes.
template <bool CLK>
__device__ __forceinline__ void sub_mark(TraceStats* st, int k) {
    if constexpr (CLK) {
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        if (first_active_lane()) st->cls[20 + 4 * st->bucket + k] += now - st->t_sub;
        st->t_sub = now;
    }
}

template <bool FULL, bool CLK = false>
__device__ __forceinline__ bool shade_step(const FrameArgs& fa, const SceneView& sv, PathState& ps, int hit_ent,
                                           int hit_prim, float tmax, float hu, float hv, f3& Lacc, bool& has_l,
                                           bool& has_shadow, ShadowRec& sr, TraceStats* clk = nullptr) {
    Lacc = mk(0, 0, 0);
    has_l = false;
    has_shadow = false;
    const f3 rd = ps.d;
    if (hit_ent < 0) {
        // on_miss (pathtracer.art:136-163): every infinite, non-delta light
        for (int li = 0; li < sv.num_infinite; ++li) {
            const DevLight& Lt = sv.lights[li];
            if (Lt.delta) continue;
            f3 emit = mk(Lt.radiance[0], Lt.radiance[1], Lt.radiance[2]);
            float pdf_s = 1 / (4 * PI_);
            // a direction NEE never takes (below a hemispherical sky, darker than a compensated
            // map's mean) belongs to BSDF sampling alone; without this a grazing bounce, whose own
            // pdf is 0 and inv_pdf infinite, would weigh it by 1 / (1 + inf * 0)
            bool nee_blind = false;
            if constexpr (FULL) {
                if (Lt.type == LIGHT_CIE) cie_emission(Lt, rd, emit, pdf_s);
                else if (Lt.type == LIGHT_ENVMAP) env_map_emission(sv, Lt, rd, emit, pdf_s);
                nee_blind = !(pdf_s > 0);
            }
            const float sel = sv.selector == SEL_UNIFORM ? 1.0f / (float)sv.num_lights : select_pdf(sv, li, ps.o);
            float mis = sv.nee ? 1 / (1 + ps.inv_pdf * sel * pdf_s) : 1.0f;
            if constexpr (FULL)
                if (nee_blind) mis = 1.0f;
            Lacc = add(Lacc, handle_color(sv, mulf(mul(ps.contrib, emit), mis)));
            has_l = true;
        }
        return false;
    }
    int mat_id;
    Surface s = surface_element(sv, hit_ent, hit_prim, tmax, hu, hv, ps.o, rd, mat_id);
    // the full variant shades a copy of the material, into which a texture
    // writes its value at the hit; the basic one reads the table in place
    std::conditional_t<FULL, DevMaterial, const DevMaterial&> m = sv.mats[mat_id];
    if constexpr (FULL)
        if (sv.uv) {
            apply_texture(sv, m, hit_ent, hit_prim, hu, hv);
            bind_measured(sv, m);
        }
    sub_mark<CLK>(clk, 0); // surface element + material
    // on_hit (pathtracer.art:114-134)
    if (m.light >= 0 && s.entering) {
        float dt = -dot(rd, s.local.n);
        if (dt > FLT_EPS_) {
            const DevLight& Lt = sv.lights[m.light];
            f3 emit = mk(Lt.radiance[0], Lt.radiance[1], Lt.radiance[2]);
            float pdf_s = light_pdf_direct_solid<FULL>(sv, Lt, ps.o, dt, tmax * tmax, hu, hv);
            const float sel = sv.selector == SEL_UNIFORM ? 1.0f / (float)sv.num_lights : select_pdf(sv, m.light, ps.o);
            float mis = sv.nee ? 1 / (1 + ps.inv_pdf * sel * pdf_s) : 1.0f;
            Lacc = add(Lacc, handle_color(sv, mulf(mul(ps.contrib, emit), mis)));
            has_l = true;
        }
    }
    sub_mark<CLK>(clk, 1); // emission
    // seed of the path's (sample, iteration, frame, pixel, user seed),
    // create_random_seed (core/random.art:34-43), carried in the path state
    Rng rnd{ps.seed, ps.counter};
    f3 out_dir = neg(rd);
    const bool specular = bsdf_is_specular<FULL>(m);
    // on_shadow (pathtracer.art:52-112)
    if (sv.nee && !specular && sv.num_lights > 0 && ps.depth + 1 <= sv.max_depth) {
        float sel_pdf;
        const int lid = select_light(sv, rnd, s.point, sel_pdf);
        const DevLight& Lt = sv.lights[lid];
        DirectSample ls = light_sample_direct<FULL>(sv, Lt, rnd, s);
        float pdf_l_s = pdf_as_solid(ls.pdf_value, ls.pdf_solid, ls.cos, ls.dist * ls.dist) * sel_pdf;
        if (pdf_l_s > FLT_EPS_ && ls.cos > FLT_EPS_) {
            f3 in_dir = ls.dir;
            float mis;
            if (Lt.delta) {
                mis = 1.0f;
            } else {
                float pdf_e_s = bsdf_pdf<FULL>(m, s, in_dir, out_dir); // pdf to sample the light by the bsdf
                mis = 1 / (1 + pdf_e_s / pdf_l_s);
            }
            float factor = ls.pdf_value / pdf_l_s;
            f3 ev = bsdf_eval<FULL>(m, s, in_dir, out_dir);
            sr.color = handle_color(sv, mulf(mul(ls.intensity, mul(ps.contrib, ev)), mis * factor));
            sr.o = s.point;
            if (Lt.infinite) {
                sr.d = in_dir;
                sr.tmax = FLT_MAX_;
            } else {
                sr.d = sub(ls.pos, s.point);
                sr.tmax = 1 - 0.001f;
            }
            has_shadow = true;
        }
    }
    sub_mark<CLK>(clk, 2); // NEE (light sample, BSDF eval / pdf)
    // on_bounce (pathtracer.art:165-200)
    if (!(ps.depth + 1 <= sv.max_depth)) return false;
    BsdfSample bs = bsdf_sample<FULL>(m, s, rnd, out_dir);
    if (!bs.valid) return false;
    f3 c2 = mul(ps.contrib, bs.color);
    float rr = 1.0f;
    if (ps.depth + 1 > sv.min_depth) {
        f3 e = mulf(c2, ps.eta * ps.eta);
        rr = clampf(fmaxf(fmaxf(e.x, e.y), e.z), 0.05f, 0.95f); // russian_roulette_pbrt
    }
    if (rnd.next_f32() >= rr) return false;
    ps.inv_pdf = specular ? 0 : 1 / bs.pdf;
    ps.contrib = mulf(c2, 1 / rr);
    ps.eta = ps.eta * bs.eta;
    // the entity the bounced ray travels in: entering an enclosing entity by
    // transmission puts the path inside it, leaving by transmission or
    // hitting anything else outside; a reflection inside keeps it inside
    const int enc = sv.ent_enc[hit_ent];
    if (enc < 0) {
        ps.inside = -1;
    } else if (dot(bs.in_dir, s.face_normal) * dot(rd, s.face_normal) > 0) { // continued through the surface
        ps.inside = s.entering ? enc : -1;
    } else if (ps.inside != enc) {
        ps.inside = -1;
    }
    ps.o = s.point;
    ps.d = bs.in_dir;
    ps.counter = rnd.counter;
    ps.depth = ps.depth + 1;
    return true;
}

// One bounce of one path: closest hit + shading.  Used by the tail kernel; the
// wavefront runs the same two halves as k_trace + k_shade, so both produce
// bit-identical paths.
// Instrumentation of k_extend's phases: the wave's shader clock (s_memtime,
// a read of the counter) since the previous mark is added to phase k; marks
// sit at wave-uniform points.
__device__ __forceinline__ void phase_mark(TraceStats& st, unsigned long long& last, int k) {
    // the phase's memory operations completed, and no instruction moves across the mark
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    st.cyc[k] += now - last;
    last = now;
}
// a mark inside the store phase (3): the cycles also go to part `part` of
// TraceStats::store_part (0 group take, 1 class tests, 2 append, 3 stores)
__device__ __forceinline__ void store_mark(TraceStats& st, unsigned long long& last, int part) {
    const unsigned long long c = st.cyc[3];
    phase_mark(st, last, 3);
    st.store_part[part] += st.cyc[3] - c;
}
template <bool STATS, int V>
__device__ __forceinline__ bool extend_step(const FrameArgs& fa, const SceneView& sv, const TStack& ts, PathState& ps, f3& Lacc,
                                            bool& has_l, bool& has_shadow, ShadowRec& sr, TraceStats& st) {
    float tmin, tmax;
    uint32_t rflags;
    ray_extent(fa, sv, ps.depth, ps.slot, tmin, tmax, rflags);
    int hit_ent, hit_prim;
    float hu = 0, hv = 0;
    // a ray inside an enclosing entity hits it first: its BLAS alone decides
    // (the full traversal from the TLAS root only when that finds nothing)
    trace_path_ray<STATS, V>(sv, ps.inside, ps.o, ps.d, tmin, tmax, rflags, ts, hit_ent, hit_prim, hu, hv, st);
    if (STATS && hit_ent >= 0) st.hits++;
    return shade_step<variant_full(V)>(fa, sv, ps, hit_ent, hit_prim, tmax, hu, hv, Lacc, has_l, has_shadow, sr);
}

__device__ __forceinline__ void add_radiance(float4* L, int slot, f3 c) {
    float4 l = L[slot];
    L[slot] = make_float4(l.x + c.x, l.y + c.y, l.z + c.z, 0);
}
// an AOV's per-path slot (FrameArgs::aov_di / aov_nee; kernel-argument pointer: a scalar branch)
// ON: compiled in (the wavefront kernels carry it in their full-shading
// variant only, which an aov_mis scene selects; the shadow kernels always)
template <bool ON = true>
__device__ __forceinline__ void add_aov(float4* A, int slot, f3 c) {
    if (ON && IGX_AOV && A) add_radiance(A, slot, c);
}

// extend_step of the instrumented k_extend (STATS): the trace and shade halves
// with phase clocks between them (load -> 0, trace -> 1, shade -> 2), and the
// per-class counters of the wave's group (`bucket`: camera, A, B, C; lane 0
// adds the wave's trace / shade cycles, one group, its wave-level node-loop
// iterations and its lanes' node visits, both reduced over the wave).
// The radiance (Lacc, has_l) is the caller's to add, as with extend_step: the
// slot's read-modify-write falls into the store phase (3).
template <int V>
__device__ __forceinline__ bool extend_step_instrumented(const FrameArgs& fa, const SceneView& sv, const TStack& ts,
                                                      PathState& ps, bool act, int bucket, f3& Lacc, bool& has_l,
                                                      bool& has_shadow, ShadowRec& sr, TraceStats& st,
                                                      unsigned long long& t_last) {
    int hit_ent = -1, hit_prim = -1;
    float hu = 0, hv = 0, tmin = 0, tmax = 0;
    uint32_t rflags = 0;
    bool alive = false;
    phase_mark(st, t_last, 0);
    const unsigned long long wn0 = st.wnodes, ln0 = st.nodes;
    if (act) {
        ray_extent(fa, sv, ps.depth, ps.slot, tmin, tmax, rflags);
        trace_path_ray<true, V>(sv, ps.inside, ps.o, ps.d, tmin, tmax, rflags, ts, hit_ent, hit_prim, hu, hv, st);
        if (hit_ent >= 0) st.hits++;
    }
    const unsigned long long c_tr = st.cyc[1];
    phase_mark(st, t_last, 1);
    // wnodes counts on the first active lane of each iteration, so the wave's
    // iterations are the sum over its lanes (as flush_stats reduces them)
    uint32_t visits = (uint32_t)(st.nodes - ln0), witers = (uint32_t)(st.wnodes - wn0);
    for (int off = 32; off > 0; off >>= 1) {
        visits += __shfl_xor(visits, off);
        witers += __shfl_xor(witers, off);
    }
    if (lane_id() == 0) {
        st.cls[bucket] += st.cyc[1] - c_tr;
        st.cls[8 + bucket] += 1;
        st.cls[12 + bucket] += witers;
        st.cls[16 + bucket] += visits;
    }
    st.bucket = bucket;
    st.t_sub = t_last;
    unsigned long long sub0 = 0;
    for (int k = 0; k < 3; ++k) sub0 += st.cls[20 + 4 * bucket + k];
    if (act) alive = shade_step<variant_full(V), true>(fa, sv, ps, hit_ent, hit_prim, tmax, hu, hv, Lacc, has_l, has_shadow, sr, &st);
    const unsigned long long c_sh = st.cyc[2];
    phase_mark(st, t_last, 2);
    if (lane_id() == 0) {
        st.cls[4 + bucket] += st.cyc[2] - c_sh;
        // sub-phase 3: the rest of the shade phase (BSDF sample, roulette, misses)
        unsigned long long sub1 = 0;
        for (int k = 0; k < 3; ++k) sub1 += st.cls[20 + 4 * bucket + k];
        st.cls[20 + 4 * bucket + 3] += (st.cyc[2] - c_sh) - (sub1 - sub0);
    }
    return alive;
}

template <bool STATS>
__device__ __forceinline__ void flush_stats(const TraceStats& st, unsigned long long* stats, int base, bool with_hits) {
    // slots: base+0..3 nodes/leaves/tris/blas, 8 hits, 9+base/4*2 .. wave node / leaf iterations
    unsigned long long a = st.nodes, b = st.leaves, c = st.tris, e = st.blas, h = st.hits, wn = st.wnodes, wl = st.wleaves;
    unsigned long long tl = st.tlas_nodes, h0 = st.hot[0], h1 = st.hot[1], h2 = st.hot[2];
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
        c += __shfl_down(c, off);
        e += __shfl_down(e, off);
        h += __shfl_down(h, off);
        wn += __shfl_down(wn, off);
        wl += __shfl_down(wl, off);
        tl += __shfl_down(tl, off);
        h0 += __shfl_down(h0, off);
        h1 += __shfl_down(h1, off);
        h2 += __shfl_down(h2, off);
    }
    if (lane_id() == 0) {
        atomicAdd(&stats[base + 0], a);
        atomicAdd(&stats[base + 1], b);
        atomicAdd(&stats[base + 2], c);
        atomicAdd(&stats[base + 3], e);
        if (with_hits) atomicAdd(&stats[8], h);
        atomicAdd(&stats[9 + (base / 4) * 2], wn);
        atomicAdd(&stats[10 + (base / 4) * 2], wl);
        if (base == 0) { // closest-hit node visits: in the TLAS, at hot-order ranks < 256 / 512 / 1280
            atomicAdd(&stats[50], tl);
            atomicAdd(&stats[51], h0);
            atomicAdd(&stats[52], h1);
            atomicAdd(&stats[53], h2);
        }
        if (st.cyc[0] | st.cyc[1] | st.cyc[2] | st.cyc[3]) {
            for (int k = 0; k < 4; ++k) atomicAdd(&stats[16 + k], st.cyc[k]);
            for (int k = 0; k < 4; ++k) atomicAdd(&stats[72 + k], st.store_part[k]); // the store phase by part
            if (st.cls)
                for (int k = 0; k < 20; ++k)
                    if (st.cls[k]) atomicAdd(&stats[20 + k], st.cls[k]);
            if (st.cls) // shading sub-phase clocks by class (surface, emission, NEE, rest)
                for (int k = 0; k < 16; ++k)
                    if (st.cls[20 + k]) atomicAdd(&stats[54 + k], st.cls[20 + k]);
        }
    }
}

// Dynamic distribution of a launch's groups of 64 stream positions: the
// wave takes the next group of shard s from that shard's counter (work +
// s * CSTRIDE, one returning atomic per group); once s is exhausted it marks
// s in the launch's mask of exhausted shards (work + CROW, 64 bits), reads the
// mask (a coherent load: the scalar cache would hold it stale for the whole
// launch) and moves on to the next shard still open.  Returns the group index
// in shard s (s and n updated), or -1 once every shard is exhausted.  Waves
// that drew short paths take more groups, so a launch no longer waits on the
// wave with the slowest fixed share.
// `claimed` >= 0: the wave already took group `claimed` of shard s (k_extend's
// append, wave_append_paths): no atomic for it.
template <class CountOf>
__device__ __forceinline__ int take_group(int* work, int& s, uint64_t& done, int n, CountOf count_of, int claimed = -1) {
    unsigned long long* const done_mask = reinterpret_cast<unsigned long long*>(work + CROW);
    for (;;) {
        if (!((done >> s) & 1ull)) {
            int v = claimed;
            claimed = -1;
            if (v < 0) {
                v = 0;
                if (lane_id() == 0) v = atomicAdd(work + s * CSTRIDE, 1);
                v = __builtin_amdgcn_readfirstlane(v);
            }
            if (v * 64 < n) return v;
            // one atomicOr per shard, not one per wave that finds it exhausted
            if (lane_id() == 0 && !((__hip_atomic_load(done_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> s) & 1ull))
                atomicOr(done_mask, 1ull << s);
            done |= 1ull << s;
        }
        unsigned long long m = 0;
        if (lane_id() == 0) m = __hip_atomic_load(done_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        done |= (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m) |
                ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32);
        const uint64_t open = ~done;
        if (!open) return -1;
        const int r = (s + 1) & (NSH - 1);
        const uint64_t rot = (open >> r) | (r ? (open << (NSH - r)) : 0ull);
        s = (r + __ffsll((unsigned long long)rot) - 1) & (NSH - 1);
        n = count_of(s);
    }
}

// path i of a generated chunk at its camera vertex (k_extend's fused bounce 0)
template <bool FULL>
__device__ __forceinline__ PathState camera_path(const FrameArgs& fa, const SceneView& sv, int i) {
    const GenPath g = gen_path<FULL>(fa, sv, i);
    PathState ps;
    ps.o = g.o;
    ps.d = g.d;
    ps.counter = g.counter;
    ps.seed = g.seed;
    ps.depth = g.depth;
    ps.slot = i;
    ps.contrib = mk(1, 1, 1); // init_pt_raypayload (technique/pathtracer.art:33-38)
    ps.inv_pdf = 0;
    ps.eta = 1.0f;
    ps.inside = -1;
    return ps;
}

// ---------------------------------------------------------------------------
// extend kernel: one bounce for every live path, compacted outputs.  Each
// wave walks its shard of the input stream and appends survivors and shadow
// rays to the same shard of the output streams (wave_append_paths): no block
// barrier, so a wave whose rays finish early moves on to its next 64 paths.
// ---------------------------------------------------------------------------
// BT threads per block: BLOCK, or BLOCK_WIDE for the LDS-staged kernel with
// the shading tables staged too (16 waves, 4 per SIMD: the same 128-VGPR cap).
// SHAPE (host/extend_shape.h, chosen per launch by pick_extend_shape): the
// generate and bounce shapes fold the default fused mode's flags to constants
// (dynamic groups, front-to-back order, three path classes, shadow classes,
// no ray list, no MIS AOVs) and drop the other half of the generate / load
// branch, so those values leave the group loop's live set; the arithmetic of
// a path is the generic kernel's.
template <int V0, bool STATS, bool LDS, int BT = BLOCK, int SHAPE = EXTEND_GENERIC>
__global__ void __launch_bounds__(BT, LDS ? EXTEND_WAVES_LDS : (variant_full(V0) ? EXTEND_WAVES_FULL : EXTEND_WAVES)) k_extend(FrameArgs fa_arg, SceneView gsv, PathBuf in, PathBuf out, ShadowBuf sh,
                                                  float4* L, KernelCounters kc, int tail_threshold) {
    static_assert(BT == BLOCK || (LDS && BT == BLOCK_WIDE), "the wide block is the LDS-staged kernel's");
    static_assert(SHAPE == EXTEND_GENERIC || !STATS, "the instrumented kernel is generic");
    FrameArgs fa = fa_arg;
    if constexpr (SHAPE != EXTEND_GENERIC) {
        fa.dynamic = 1;
        fa.reverse = 0;
        fa.classify = EXTEND_SHAPE_CLASSIFY;
        fa.shadow_classes = 1;
        fa.num_rays = 0;
        fa.rays = nullptr;
        fa.aov_di = fa.aov_nee = nullptr;
        if constexpr (SHAPE == EXTEND_BOUNCE) fa.gen_n = 0;
        // pointer families from one base each (the host checked the layout,
        // streams_packed): both path buffers and the shadow stream share the
        // shard capacity, a path buffer holds the class-C region behind its
        // shards, and the three counter rows of a bounce are neighbours
        // (the arrays' byte offsets: stream_layout, host/extend_shape.h)
        const int cap = out.shard_cap;
        const StreamLayout lay = stream_layout(cap);
        auto at = [](float4* base, unsigned long long off) { return reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + off); };
        auto derive = [&](PathBuf& b) {
            b.shard_cap = cap;
            b.c_base = NSH * cap;
            b.p1 = at(b.p0, lay.p_off[1]);
            b.p2 = at(b.p0, lay.p_off[2]);
            b.p3 = reinterpret_cast<float2*>(at(b.p0, lay.p_off[3]));
        };
        derive(out);
        if constexpr (SHAPE == EXTEND_BOUNCE) derive(in);
        sh.shard_cap = cap;
        sh.s1 = at(sh.s0, lay.s_off[1]);
        sh.s2 = at(sh.s0, lay.s_off[2]);
        kc.cnt_shadow = kc.cnt_in + CROW;
        kc.cnt_out = kc.cnt_in + 2 * CROW;
    }
    constexpr bool SHADE_LDS = BT > BLOCK; // the wide block stages the shading tables too
    constexpr int V = LDS ? kernel_variant(V0, true) : (EXTEND_TREELET ? kernel_variant(V0, false) : V0); // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: treelet (device_scene.h) or global node loads
    __shared__ int stack_mem[LDS_STACK * BT];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack<BT>(stack_mem, LDS_STACK, gsv.spill);
    // gen_n > 0 (bounce 0 with generation fused; the host launches it only
    // when n > tail): the paths are the chunk's camera paths in k_generate's
    // shard order, built here instead of being read from the input stream.
    const bool gen = SHAPE == EXTEND_GENERATE ? true : SHAPE == EXTEND_BOUNCE ? false : fa.gen_n > 0;
    if (!gen && row_total(kc.cnt_in) <= tail_threshold) return; // k_finish takes the remaining paths (block-uniform)
    const SceneView sv = LDS ? stage_scene_lds<BT, SHADE_LDS>(gsv, lds_scene) : stage_treelet<BT>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    __shared__ unsigned long long cls_mem[STATS ? BT / 64 * 36 : 1]; // per-class counters (instrumented), 36 per wave
    if constexpr (STATS) {
        st.cls = cls_mem + 36 * (threadIdx.x >> 6);
        if (lane_id() < 36) st.cls[lane_id()] = 0;
    }
    const WaveWork w = wave_work<BT>();
    // Groups of 64 positions of shard s: statically every K-th group from
    // the wave's own (grid-stride), or (fa.dynamic) the next group a shard
    // counter hands out, moving on to the following shards once the own is
    // exhausted -- waves that drew fast paths take more groups, so a launch
    // does not wait on the wave with the slowest share.  Survivors always go
    // to the shard the group came from (its output never exceeds its input).
    int s = w.s;
    auto count_of = [&](int sh_) {
        if (gen) {
            const int g = gen_shard_count(fa.gen_n, sh_);
            return ShardCount{g, g, g};
        }
        return shard_count(kc.cnt_in, sh_);
    };
    ShardCount sc = count_of(s);
    uint64_t done = 0; // shards this wave knows to be exhausted (dynamic)
    int p0 = w.k * 64;
    int claimed = -1; // next group of shard s, taken by the previous group's append (IGX_CLAIM_NEXT)
    unsigned long long t_last = STATS ? __builtin_amdgcn_s_memtime() : 0; // phase clocks (instrumented builds)
    for (;;) {
        if (fa.dynamic) {
            const int g = take_group(kc.work, s, done, sc.n, [&](int sh_) {
                sc = count_of(sh_);
                return sc.n;
            }, claimed);
            if (g < 0) break;
            p0 = g * 64;
        } else if (p0 >= sc.n) {
            break;
        }
        if constexpr (STATS) store_mark(st, t_last, 0); // group distribution
        const int ns = sc.n;
        int* const c_out = kc.cnt_out + s * CSTRIDE;
        int* const c_sh = kc.cnt_shadow + s * CSTRIDE;
        const int q = p0 + lane_id();
        const int pos = (fa.reverse && !gen) ? ns - 1 - q : q; // reverse: longest classes first
        bool alive = false, has_shadow = false, has_l = false;
        PathState ps;
        ShadowRec sr;
        f3 Lacc = mk(0, 0, 0);
        ps.depth = 0;
        if (q < ns) {
            if (gen) { // inverse of gen_index
                const int i = ((pos >> 6) << 12) | (s << 6) | (pos & 63);
                ps = camera_path<variant_full(V0)>(fa, sv, i);
                if (variant_full(V0) && IGX_AOV && fa.aov_di) fa.aov_di[i] = fa.aov_nee[i] = make_float4(0, 0, 0, 0);
            } else if constexpr (SHAPE != EXTEND_GENERIC) { // load_path by scalar bases (rec_at)
                const uint32_t i = (uint32_t)path_index(in, s, pos, sc);
                ps = path_from_records(*rec_at(in.p0, i * (uint32_t)sizeof(float4)), *rec_at(in.p1, i * (uint32_t)sizeof(float4)),
                                       *rec_at(in.p2, i * (uint32_t)sizeof(float4)), *rec_at(in.p3, i * (uint32_t)sizeof(float2)));
            } else {
                ps = load_path(in, path_index(in, s, pos, sc));
            }
            if (!STATS && ps.depth > 0) alive = extend_step<STATS, V>(fa, sv, ts, ps, Lacc, has_l, has_shadow, sr, st);
        }
        if constexpr (STATS) {
            // class of the wave's group (wave-uniform): camera, A, B, C
            const int pg = (fa.reverse && !gen) ? ns - 1 - p0 : p0;
            const int bucket = gen ? 0 : (pg < sc.a ? 1 : pg < sc.ab ? 2 : 3);
            alive = extend_step_instrumented<V>(fa, sv, ts, ps, q < ns && ps.depth > 0, bucket, Lacc, has_l, has_shadow, sr, st, t_last);
        }
        if constexpr (SHAPE != EXTEND_GENERIC) {
            // The store phase of the shapes writes what the generic kernel's
            // (the other branch, where the steps are described) writes, record
            // for record: both class tests in one pass over the enclosing boxes
            // (class_pass), one returning atomic for the append and the claim,
            // issued as soon as the classes are known (wave_append_issue), and
            // every record addressed as a wave-uniform array base plus a 32-bit
            // byte offset (rec_at).
            // The radiance load goes out first, under no branch and ahead of
            // the class pass, for every lane that may update its slot (a lane
            // that then does not drops the value; the others read slot 0): the
            // compiler waits for a load issued under a branch at the branch's
            // end, so the generic kernel's load and its atomics are two round
            // trips in a row; here the load, the class pass and the atomic
            // overlap and one wait behind the atomic serves both.
            // (a lane past the group's end, q >= ns, holds no path: its ps.slot
            // is undefined, has_l and has_shadow are false there, so it reads
            // slot 0 and stores nothing; a slot index has SLOT_BITS bits, so the
            // byte offset into L fits 32 bits)
            static_assert(SLOT_BITS + 4 <= 32, "a radiance slot's byte offset fits 32 bits");
            const uint32_t l_off = (uint32_t)ps.slot * (uint32_t)sizeof(float4);
            float4 l = make_float4(0, 0, 0, 0);
            if constexpr (SHAPE == EXTEND_BOUNCE) l = *rec_at(L, (has_l || (fa.shadow_optimistic && has_shadow)) ? l_off : 0u);
            bool p_b, sh_b;
            class_pass(sv, has_shadow ? sr.o : ps.o, alive && ps.eta == 1.0f, ps.d, has_shadow, sr.d, sr.tmax, p_b, sh_b);
            const int cls = ps.eta != 1.0f ? 2 : (int)p_b; // path_class, FrameArgs::classify 4
            const bool opt_add = fa.shadow_optimistic && has_shadow && !sh_b;
            const bool upd = gen ? q < ns : (has_l || opt_add);
            int* const claim = (IGX_CLAIM_NEXT && !((done >> s) & 1ull)) ? kc.work + s * CSTRIDE : nullptr;
            const AppendIssued ap = wave_append_issue(alive, cls, has_shadow, sh_b, c_out, c_sh, claim);
            const float w_slot = __uint_as_float((uint32_t)ps.slot | ((uint32_t)(ps.inside + 1) << SLOT_BITS));
            const float w_count = __uint_as_float(ps.counter | ((uint32_t)ps.depth << 24));
            f3 rec = sr.color; // the shadow record's third word
            f3 v = f3of(l);
            if (has_l) v = mk(v.x + Lacc.x, v.y + Lacc.y, v.z + Lacc.z); // add_radiance
            if (opt_add) {
                rec = v; // undo
                v = mk(v.x + sr.color.x, v.y + sr.color.y, v.z + sr.color.z);
            }
            int dst, sdst;
            wave_append_finish(ap, cls, sh_b, out.shard_cap, out.c_base, sh.shard_cap, dst, sdst, claim != nullptr, claimed);
            if (alive) {
                const uint32_t e = (uint32_t)(s * out.shard_cap + dst);
                *rec_at(out.p0, e * (uint32_t)sizeof(float4)) = make_float4(ps.o.x, ps.o.y, ps.o.z, w_slot);
                *rec_at(out.p1, e * (uint32_t)sizeof(float4)) = make_float4(ps.d.x, ps.d.y, ps.d.z, w_count);
                *rec_at(out.p2, e * (uint32_t)sizeof(float4)) = make_float4(ps.contrib.x, ps.contrib.y, ps.contrib.z, ps.inv_pdf);
                *rec_at(out.p3, e * (uint32_t)sizeof(float2)) = make_float2(ps.eta, __uint_as_float(ps.seed));
            }
            if (upd) *rec_at(L, l_off) = make_float4(v.x, v.y, v.z, 0);
            if (has_shadow) {
                const uint32_t e = (uint32_t)(s * sh.shard_cap + sdst) * (uint32_t)sizeof(float4);
                *rec_at(sh.s0, e) = make_float4(sr.o.x, sr.o.y, sr.o.z, __int_as_float(ps.slot));
                *rec_at(sh.s1, e) = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.tmax);
                *rec_at(sh.s2, e) = make_float4(rec.x, rec.y, rec.z, 0);
            }
        } else {
            const bool sh_b = has_shadow && shadow_class_b(fa.shadow_classes, sv, sr.o, sr.d, sr.tmax);
            int cls_marked = 0; // instrumented: the path class, taken ahead of the append for the class-test clock
            if constexpr (STATS) {
                cls_marked = path_class(fa.classify, sv, ps);
                store_mark(st, t_last, 1);
            }
            // The path's radiance slot takes the emission (has_l) and, with
            // shadow_optimistic, the colour of a class-A shadow ray in one
            // read-modify-write: the shadow kernel adds nothing for such a ray and
            // puts `undo` back if it is occluded (ShadowBuf::s2).  A generated path
            // (bounce 0) starts from +0 in registers and writes its slot once, dead
            // and padding paths included (k_generate's zero fill).  The scattered
            // load goes out ahead of the append's returning atomic and is consumed
            // behind it: one round trip for both.
            const bool opt_add = fa.shadow_optimistic && has_shadow && !sh_b;
            const bool upd = gen ? q < ns : (has_l || opt_add);
            float4 l = make_float4(0, 0, 0, 0);
            if (!gen && upd) l = L[ps.slot];
            int dst, sdst;
            // dynamic groups: the append's round trip also takes the next group of
            // shard s, unless s is known exhausted
            int* const claim = (IGX_CLAIM_NEXT && fa.dynamic && !((done >> s) & 1ull)) ? kc.work + s * CSTRIDE : nullptr;
            wave_append_paths(alive, STATS ? cls_marked : path_class(fa.classify, sv, ps), has_shadow, sh_b, c_out, c_sh, out.shard_cap,
                              out.c_base, sh.shard_cap, dst, sdst, claim, &claimed);
            if (!claim) claimed = -1;
            if constexpr (STATS) store_mark(st, t_last, 2); // radiance load and append round trip
            if (alive) store_path(out, s * out.shard_cap + dst, ps);
            f3 rec = sr.color; // the shadow record's third word
            if (upd) {
                f3 v = f3of(l);
                if (has_l) {
                    v = mk(v.x + Lacc.x, v.y + Lacc.y, v.z + Lacc.z); // add_radiance
                    add_aov<variant_full(V0)>(fa.aov_di, ps.slot, Lacc);
                }
                if (opt_add) {
                    rec = v; // undo
                    v = mk(v.x + sr.color.x, v.y + sr.color.y, v.z + sr.color.z);
                }
                L[ps.slot] = make_float4(v.x, v.y, v.z, 0);
            }
            if (has_shadow) {
                const int e = s * sh.shard_cap + sdst;
                sh.s0[e] = make_float4(sr.o.x, sr.o.y, sr.o.z, __int_as_float(ps.slot));
                sh.s1[e] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.tmax);
                sh.s2[e] = make_float4(rec.x, rec.y, rec.z, 0);
            }
            if (!fa.dynamic) p0 += w.K * 64;
            if constexpr (STATS) store_mark(st, t_last, 3); // stores
        }
    }
    if (STATS) flush_stats<STATS>(st, kc.stats, 0, true);
}

// ---------------------------------------------------------------------------
// trace: closest hit of every live path's current ray (gpu_traverse_primary,
// mapping_gpu.art:45-68).  Traversal only, so the kernel stays small enough
// for high occupancy (the latency of the dependent node loads is what bounds
// it); each lane writes its own hit record (same index as its path).
// ---------------------------------------------------------------------------
template <int V0, bool STATS, int WAVES, bool LDS>
__global__ void __launch_bounds__(BLOCK, WAVES) k_trace(FrameArgs fa, SceneView gsv, PathBuf in, HitBuf hits,
                                                      const int* cnt, int tail_threshold, unsigned long long* stats) {
    constexpr int V = LDS ? kernel_variant(V0, true) : V0; // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: global node loads (no treelet)
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    if (row_total(cnt) <= tail_threshold) return; // k_finish takes the remaining paths
    const SceneView sv = LDS ? stage_scene_lds<BLOCK>(gsv, lds_scene) : stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    const WaveWork w = wave_work();
    const ShardCount sc = shard_count(cnt, w.s);
    const int ns = sc.n;
    for (int pos = w.k * 64 + lane_id(); pos < ns; pos += w.K * 64) {
        const int i = path_index(in, w.s, pos, sc);
        float4 p0 = in.p0[i], p1 = in.p1[i];
        int depth = (int)(__float_as_uint(p1.w) >> 24);
        int hit_ent = -1, hit_prim = -1;
        float hu = 0, hv = 0, tmax = 0;
        if (depth > 0) {
            float tmin;
            uint32_t rflags;
            ray_extent(fa, sv, depth, (int)(__float_as_uint(p0.w) & SLOT_MASK), tmin, tmax, rflags);
            trace_ray<false, STATS, V>(sv, f3of(p0), f3of(p1), tmin, tmax, rflags, ts, hit_ent, hit_prim, hu, hv, st);
            if (STATS && hit_ent >= 0) st.hits++;
        }
        hits.h[i] = make_float4(tmax, hu, hv, __int_as_float(hit_ent));
        hits.prim[i] = hit_prim;
    }
    if (STATS) flush_stats<STATS>(st, stats, 0, true);
}

// ---------------------------------------------------------------------------
// shade: the path-tracer step at every hit / miss (gpu_hit_shade +
// gpu_miss_shade, mapping_gpu.art:114-266) for all materials at once, with
// wave-level compaction of surviving paths and shadow rays.
// ---------------------------------------------------------------------------
template <bool FULL>
__global__ void __launch_bounds__(BLOCK) k_shade(FrameArgs fa, SceneView sv, PathBuf in, HitBuf hits, PathBuf out,
                                                 ShadowBuf sh, float4* L, KernelCounters kc, int tail_threshold) {
    if (row_total(kc.cnt_in) <= tail_threshold) return;
    const WaveWork w = wave_work();
    const ShardCount sc = shard_count(kc.cnt_in, w.s);
    const int ns = sc.n;
    int* const c_out = kc.cnt_out + w.s * CSTRIDE;
    int* const c_sh = kc.cnt_shadow + w.s * CSTRIDE;
    for (int p0 = w.k * 64; p0 < ns; p0 += w.K * 64) {
        const int pos = p0 + lane_id();
        const int i = path_index(in, w.s, pos, sc);
        bool alive = false, has_shadow = false;
        PathState ps;
        ShadowRec sr;
        ps.depth = 0;
        if (pos < ns) {
            ps = load_path(in, i);
            if (ps.depth > 0) {
                float4 h = hits.h[i];
                int prim = hits.prim[i];
                f3 Lacc;
                bool has_l;
                alive = shade_step<FULL>(fa, sv, ps, __float_as_int(h.w), prim, h.x, h.y, h.z, Lacc, has_l, has_shadow, sr);
                if (has_l) {
                    add_radiance(L, ps.slot, Lacc);
                    add_aov<FULL>(fa.aov_di, ps.slot, Lacc);
                }
            }
        }
        int dst, sdst;
        wave_append_paths(alive, path_class(fa.classify, sv, ps), has_shadow,
                          has_shadow && shadow_class_b(fa.shadow_classes, sv, sr.o, sr.d, sr.tmax), c_out, c_sh, out.shard_cap,
                          out.c_base, sh.shard_cap, dst, sdst);
        if (alive) store_path(out, w.s * out.shard_cap + dst, ps);
        if (has_shadow) {
            const int e = w.s * sh.shard_cap + sdst;
            sh.s0[e] = make_float4(sr.o.x, sr.o.y, sr.o.z, __int_as_float(ps.slot));
            sh.s1[e] = make_float4(sr.d.x, sr.d.y, sr.d.z, sr.tmax);
            sh.s2[e] = make_float4(sr.color.x, sr.color.y, sr.color.z, 0);
        }
    }
}

// ---------------------------------------------------------------------------
// tail kernel: once few paths remain, each lane runs its path to the end
// (extend + inline any-hit shadow ray per bounce), replacing dozens of nearly
// empty per-bounce launches.  Same per-path arithmetic and the same radiance
// accumulation order as the wavefront kernels.
// ---------------------------------------------------------------------------
template <int V0, bool STATS, bool LDS>
__global__ void __launch_bounds__(BLOCK) k_finish(FrameArgs fa, SceneView gsv, PathBuf in, float4* L, const int* cnt,
                                                  int tail_threshold, unsigned long long* stats,
                                                  unsigned long long* tail_counts) {
    constexpr int V = LDS ? kernel_variant(V0, true) : V0; // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: global node loads (the tail kernel stages no treelet)
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    const int n = row_total(cnt);
    if (n > tail_threshold || n == 0) return; // the wavefront kernels own this bounce
    const SceneView sv = LDS ? stage_scene_lds<BLOCK>(gsv, lds_scene) : stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    TraceStats sst{0, 0, 0, 0, 0, 0, 0};
    unsigned long long bounces = 0, shadows = 0;
    const WaveWork w = wave_work();
    const ShardCount sc = shard_count(cnt, w.s);
    const int ns = sc.n;
    for (int pos = w.k * 64 + lane_id(); pos < ns; pos += w.K * 64) {
        PathState ps = load_path(in, path_index(in, w.s, pos, sc));
        if (ps.depth <= 0) continue;
        for (;;) {
            f3 Lacc;
            bool has_l, has_shadow;
            ShadowRec sr;
            bool alive = extend_step<STATS, V>(fa, sv, ts, ps, Lacc, has_l, has_shadow, sr, st);
            if (has_l) {
                add_radiance(L, ps.slot, Lacc);
                add_aov<variant_full(V0)>(fa.aov_di, ps.slot, Lacc);
            }
            if (has_shadow) {
                ++shadows;
                float tm = sr.tmax;
                int e, p;
                float u, v;
                if (!trace_ray<true, STATS, V>(sv, sr.o, sr.d, 0.001f, tm, RAY_SHADOW, ts, e, p, u, v, sst)) {
                    add_radiance(L, ps.slot, sr.color);
                    add_aov<variant_full(V0)>(fa.aov_nee, ps.slot, sr.color);
                }
            }
            if (!alive) break;
            ++bounces;
        }
    }
    // ray statistics of the tail (continuation rays, valid shadow rays): one atomic per wave
    for (int off = 32; off > 0; off >>= 1) {
        bounces += __shfl_down(bounces, off);
        shadows += __shfl_down(shadows, off);
    }
    if (lane_id() == 0 && (bounces | shadows)) {
        atomicAdd(&tail_counts[0], bounces);
        atomicAdd(&tail_counts[1], shadows);
    }
    if (STATS) {
        flush_stats<STATS>(st, stats, 0, true);
        flush_stats<STATS>(sst, stats, 4, false);
    }
}

// ---------------------------------------------------------------------------
// tail kernel with lane pairs (global-table scenes): on the soups a tail
// path's bounce is two dependent walks through HBM-resident tables (closest
// hit, then the NEE shadow ray), and the longest path sets the tail's length.
// Both rays of a bounce start at the same shading point and do not depend on
// each other, so here the even lane of a pair carries the path and traces its
// closest hits while the odd lane traces the path's shadow rays: the two walks
// overlap, and both lanes step through the same instructions (per-lane any-hit
// flag, trav_step_core).  Radiance is added in the wavefront's order (emission
// of bounce k, shadow ray of bounce k, emission of bounce k + 1), so the image
// is bit-identical to k_finish.
// ---------------------------------------------------------------------------
// occupancy target of k_finish_pairs (waves per SIMD).  The compiler's own
// choice is 212-234 VGPRs = 2 waves; 3 waves (168 VGPRs, ~30 spilled) hides
// more of the long tail's latency: soup-16M frame 70.6 -> 69.4 ms, soup-1M
// 54.3 -> 53.2 ms (tools/exp_n.sh, round 3)
#ifndef FINISH_PAIRS_WAVES
#define FINISH_PAIRS_WAVES 3
#endif
// Pairs step independently (round 6): a wave keeps stepping its busy lanes
// until TAIL_READY pairs have finished both walks (or none is busy), then
// processes those pairs alone (shadow verdict, shading, hand-over, next
// walks), so a pair no longer waits each bounce for the slowest walk of the
// wave.  Soup-1M 2-iteration frame 72.4-72.8 -> 71.8 ms (tail 4.1 -> 3.6-3.7
// ms), soup-16M and S-deep within noise, identical images (4 / 8 / 16 ready
// pairs alike; profiles/r06_ab_tail_pairs_desync.log).  The soup-16M tail
// stays ~5.5 ms: its first 8 bounces (98 K paths) take 3.2 ms of it
// (profiles/r06_tail_vs_max_depth_soup16.log), each a chain of dependent
// node fetches at 3 waves per SIMD.
constexpr int TAIL_READY = 8;
template <int V0, bool STATS>
__global__ void __launch_bounds__(BLOCK, FINISH_PAIRS_WAVES) k_finish_pairs(FrameArgs fa, SceneView gsv, PathBuf in, float4* L, const int* cnt,
                                                        int tail_threshold, unsigned long long* stats,
                                                        unsigned long long* tail_counts) {
    constexpr int V = V0; // global node loads (no treelet)
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    const int n = row_total(cnt);
    if (n > tail_threshold || n == 0) return; // the wavefront kernels own this bounce
    const SceneView sv = stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    TraceStats sst{0, 0, 0, 0, 0, 0, 0};
    unsigned long long bounces = 0, shadows = 0;
    const WaveWork w = wave_work();
    const ShardCount sc = shard_count(cnt, w.s);
    const int ns = sc.n;
    const int lane = lane_id(), partner = lane ^ 1;
    const bool path_lane = (lane & 1) == 0;
    constexpr uint64_t EVEN = 0x5555555555555555ull;
    for (int pos0 = w.k * 32; pos0 < ns; pos0 += w.K * 32) { // 32 paths per wave and pass
        const int pos = pos0 + (lane >> 1);
        PathState ps;
        ps.depth = 0;
        if (path_lane && pos < ns) ps = load_path(in, path_index(in, w.s, pos, sc));
        bool tracing = path_lane && pos < ns && ps.depth > 0; // path lane: its current ray needs a closest hit
        bool sh_trace = false;                                  // odd lane: a shadow ray to trace
        bool had_shadow = false;                                // path lane: its last shadow ray is out
        ShadowRec sr;
        f3 so = mk(0, 0, 0), sd = mk(0, 0, 1);
        float stmax = 0;
        Trav t;
        bool busy = false, enclosed = false;
        bool fresh = false; // this lane's walk has run since its pair was last processed
        TraceStats& tst = path_lane ? st : sst;
        bool start = true;  // the pair is at a bounce boundary: start its walks
        for (;;) {
            // ---- start the walks of the pairs at a bounce boundary ----
            if (start) {
                if (tracing) {
                    float tmin, tmax;
                    uint32_t rflags;
                    ray_extent(fa, sv, ps.depth, ps.slot, tmin, tmax, rflags);
                    enclosed = ps.inside >= 0 && trav_init_enclosed<STATS>(sv, t, ps.inside, ps.o, ps.d, tmin, tmax, rflags, ts, tst);
                    if (!enclosed) trav_init(sv, t, ps.o, ps.d, tmin, tmax, rflags, ts);
                    busy = fresh = true;
                } else if (sh_trace) {
                    trav_init(sv, t, so, sd, 0.001f, stmax, RAY_SHADOW, ts);
                    busy = fresh = true;
                }
                start = false;
            }
            // ---- step the busy lanes until TAIL_READY pairs (or all) have finished
            // both walks: a pair does not wait for the slowest walk of the wave ----
            uint64_t ready;
            for (;;) {
                const uint64_t bm = __ballot(busy), fm = __ballot(fresh);
                ready = ((fm | (fm >> 1)) & EVEN) & ~((bm | (bm >> 1)) & EVEN);
                if (bm == 0 || __popcll(ready) >= TAIL_READY) break;
                if (busy && trav_step_core<2, STATS, V>(sv, t, ts, tst, !path_lane)) {
                    busy = false;
                    if (tracing && enclosed && !t.found) {
                        // an enclosed walk that found nothing: the full traversal from the TLAS root
                        float tmin, tmax;
                        uint32_t rflags;
                        ray_extent(fa, sv, ps.depth, ps.slot, tmin, tmax, rflags);
                        trav_init(sv, t, ps.o, ps.d, tmin, tmax, rflags, ts);
                        enclosed = false;
                        busy = true;
                    }
                }
            }
            if (ready == 0) break; // no walk running and none to process: every pair is done
            if (!((ready >> (lane & ~1)) & 1)) continue;
            // ---- a ready pair: its shadow verdict, then the shading of its hit ----
            fresh = false;
            const bool occluded = __shfl(sh_trace && t.found, partner) != 0;
            if (path_lane && had_shadow && !occluded) {
                add_radiance(L, ps.slot, sr.color);
                add_aov<variant_full(V0)>(fa.aov_nee, ps.slot, sr.color);
            }
            bool cont = false, has_shadow = false;
            if (tracing) {
                if (STATS && t.hit_ent >= 0) st.hits++;
                f3 Lacc;
                bool has_l;
                cont = shade_step<variant_full(V)>(fa, sv, ps, t.hit_ent, t.hit_prim, t.tmax, t.hu, t.hv, Lacc, has_l, has_shadow, sr);
                if (has_l) {
                    add_radiance(L, ps.slot, Lacc);
                    add_aov<variant_full(V0)>(fa.aov_di, ps.slot, Lacc);
                }
                if (has_shadow) ++shadows;
                if (cont) ++bounces;
            }
            tracing = cont;
            had_shadow = has_shadow;
            // ---- hand the shadow ray to the odd lane ----
            const float ox = __shfl(sr.o.x, partner), oy = __shfl(sr.o.y, partner), oz = __shfl(sr.o.z, partner);
            const float dx = __shfl(sr.d.x, partner), dy = __shfl(sr.d.y, partner), dz = __shfl(sr.d.z, partner);
            const float tm = __shfl(sr.tmax, partner);
            const bool ph = __shfl(has_shadow, partner) != 0;
            if (!path_lane) {
                sh_trace = ph;
                so = mk(ox, oy, oz);
                sd = mk(dx, dy, dz);
                stmax = tm;
            }
            start = true;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        bounces += __shfl_down(bounces, off);
        shadows += __shfl_down(shadows, off);
    }
    if (lane_id() == 0 && (bounces | shadows)) {
        atomicAdd(&tail_counts[0], bounces);
        atomicAdd(&tail_counts[1], shadows);
    }
    if (STATS) {
        flush_stats<STATS>(st, stats, 0, true);
        flush_stats<STATS>(sst, stats, 4, false);
    }
}

// ---------------------------------------------------------------------------
// shadow: any-hit traversal; on miss add the NEE contribution
// (gpu_traverse_secondary, mapping_gpu.art:70-112; on_shadow_miss, pathtracer.art:202-209)
// ---------------------------------------------------------------------------
// One shadow ray's any-hit walk; unoccluded, its colour goes to the radiance
// slot (l: the slot's value, loaded before the walk so that the scattered
// read's latency overlaps the walk: diamond shadow time 20.6 -> 20.3 ms per
// frame, round 5).  Returns whether the ray is occluded.
// `undo` (a class-A lane of a group with both classes under
// ShadowBuf::optimistic, see shadow_walk_undo): col is the slot's previous
// value, stored back if the ray is occluded; l is not used.
template <bool STATS, int V>
__device__ __forceinline__ bool shadow_walk(const SceneView& sv, const TStack& ts, float4 s0, float4 s1, float4 col, float4 l,
                                            bool undo, float4* L, float4* aov_nee, TraceStats& st) {
    float tmax = s1.w;
    int e, p;
    float u, v;
    const bool occl = trace_ray<true, STATS, V>(sv, f3of(s0), f3of(s1), 0.001f, tmax, RAY_SHADOW, ts, e, p, u, v, st);
    const int slot = __float_as_int(s0.w);
    if (undo) {
        if (occl) L[slot] = make_float4(col.x, col.y, col.z, 0);
    } else if (!occl) {
        L[slot] = make_float4(l.x + col.x, l.y + col.y, l.z + col.z, 0); // add_radiance
        add_aov(aov_nee, slot, f3of(col));
    }
    return occl;
}
// A class-A ray under ShadowBuf::optimistic: k_extend added its colour
// already, so an unoccluded ray (99.9 % of them on the diamond frame) touches
// neither its slot nor the record's third word; an occluded one stores the
// slot's previous value back (s2: the undo value).  The caller takes this
// path for a wave whose whole group is class A.
template <bool STATS, int V>
__device__ __forceinline__ bool shadow_walk_undo(const SceneView& sv, const TStack& ts, float4 s0, float4 s1, const float4* undo,
                                                 float4* L, TraceStats& st) {
    float tmax = s1.w;
    int e, p;
    float u, v;
    const bool occl = trace_ray<true, STATS, V>(sv, f3of(s0), f3of(s1), 0.001f, tmax, RAY_SHADOW, ts, e, p, u, v, st);
    if (occl) L[__float_as_int(s0.w)] = *undo;
    return occl;
}

template <int V0, bool STATS, bool LDS>
__global__ void __launch_bounds__(BLOCK) k_shadow(SceneView gsv, ShadowBuf sh, float4* L, const int* cnt,
                                                  unsigned long long* stats, int* work) {
    constexpr int V = LDS ? kernel_variant(V0, true) : (SHADOW_TREELET ? kernel_variant(V0, false) : V0); // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: treelet or global node loads
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    if (row_total(cnt) == 0) return;
    const SceneView sv = LDS ? stage_scene_lds<BLOCK>(gsv, lds_scene) : stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    unsigned long long cls_acc[2][6] = {}; // instrumented: per shadow class groups, wave iterations, visits, cycles, occluded, rays
    const WaveWork w = wave_work();
    const int lane = lane_id();
    // groups of 64 shadow rays: grid-stride over the wave's own shard, or
    // (work != nullptr) handed out by take_group
    int s = w.s;
    ShardCount sc = shard_count(cnt, s); // two shadow classes (wave_append_paths)
    // instrumented: the class of the group (wave-uniform), its wave cycles and visits
    unsigned long long c0 = 0;
    uint32_t wn0 = 0, ln0 = 0;
    auto stats_begin = [&]() {
        if constexpr (STATS) {
            c0 = __builtin_amdgcn_s_memtime();
            wn0 = st.wnodes;
            ln0 = st.nodes;
        }
    };
    auto stats_end = [&](int p0, bool act, bool occl) {
        if constexpr (STATS) {
            __builtin_amdgcn_s_waitcnt(0);
            const unsigned long long c1 = __builtin_amdgcn_s_memtime();
            uint32_t visits = st.nodes - ln0, witers = st.wnodes - wn0, occ = occl ? 1 : 0, nr = act ? 1 : 0;
            for (int off = 32; off > 0; off >>= 1) {
                visits += __shfl_xor(visits, off);
                witers += __shfl_xor(witers, off);
                occ += __shfl_xor(occ, off);
                nr += __shfl_xor(nr, off);
            }
            // accumulated per wave (lane 0), flushed once at the end: no atomics in the timed region
            const int cls = p0 < sc.a ? 0 : 1;
            if (lane == 0) {
                cls_acc[cls][0] += 1;
                cls_acc[cls][1] += witers;
                cls_acc[cls][2] += visits;
                cls_acc[cls][3] += c1 - c0;
                cls_acc[cls][4] += occ;
                cls_acc[cls][5] += nr;
            }
        }
    };
    {
        uint64_t done = 0;
        for (int p0 = w.k * 64;; p0 += w.K * 64) {
            if (work) {
                p0 = take_group(work, s, done, sc.n, [&](int sh_) {
                    sc = shard_count(cnt, sh_);
                    return sc.n;
                });
                if (p0 < 0) break;
                p0 *= 64;
            } else if (p0 >= sc.n) {
                break;
            }
            const int pos = p0 + lane;
            stats_begin();
            bool occl = false;
            if (sh.optimistic && p0 + 63 < sc.a) { // a whole group of class A (wave-uniform): the lean path
                const int i = s * sh.shard_cap + pos;
                occl = shadow_walk_undo<STATS, V>(sv, ts, sh.s0[i], sh.s1[i], sh.s2 + i, L, st);
            } else if (pos < sc.n) {
                const int i = stream_index(s, pos, sc.a, sh.shard_cap);
                const bool undo = sh.optimistic && pos < sc.a; // class-A lanes of the shard's one group with both classes
                const float4 s0 = sh.s0[i];
                const float4 l = undo ? make_float4(0, 0, 0, 0) : L[__float_as_int(s0.w)];
                occl = shadow_walk<STATS, V>(sv, ts, s0, sh.s1[i], sh.s2[i], l, undo, L, sh.aov_nee, st);
            }
            stats_end(p0, pos < sc.n, occl);
        }
    }
    if constexpr (STATS) {
        if (lane == 0)
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < 6; ++k)
                    if (cls_acc[c][k]) atomicAdd(&stats[k < 5 ? 40 + 2 * k + c : 70 + c], cls_acc[c][k]);
    }
    if (STATS) flush_stats<STATS>(st, stats, 4, false);
}

// ---------------------------------------------------------------------------
// Persistent-lane variants of trace and shadow (refill_loop) for scenes whose
// traversal tables stay in global memory: there a node step waits on an
// Infinity-Cache / HBM round trip, and refilling idle lanes cuts the number
// of wave-level steps.  Each wave walks the positions k, k + K, ... (in
// groups of 64) of its shard, like the grid-stride kernels.
// ---------------------------------------------------------------------------
// occupancy target of the persistent-lane kernels (waves per SIMD): 6 caps
// them at 80 VGPRs (trace 4.8 -> 4.5 ms per S-deep iteration, soup-16M
// 45.6 -> 43.3); 7 and 8 spill and run slower
#ifndef REFILL_WAVES
#define REFILL_WAVES 6
#endif
// with quantised nodes a node step holds 16 VGPRs of node data instead of 32
#ifndef REFILL_WAVES_Q4
#define REFILL_WAVES_Q4 6
#endif
// the if-if shadow kernel (split-schedule scenes) needs fewer registers: with
// quantised nodes and global stack / node loads it fits 7 waves per SIMD (72
// VGPRs, 2 spilled): soup-1M shadow time per 8-iteration frame 102.0 -> 98.2 ms,
// soup-16M 42.6 -> 42.0 ms (profiles/r03_ab_waves7.log; the trace kernel at 7
// waves spills 23 registers and runs slower, so it stays at 6)
#ifndef SHADOW_IFIF_WAVES
#define SHADOW_IFIF_WAVES 7
#endif
// LDS-staged tables (<= 48 KB + the 16 KB stack per block) allow at most
// 4 blocks per CU: the 6-wave VGPR cap would only force spills
#ifndef REFILL_WAVES_LDS
#define REFILL_WAVES_LDS 4
#endif
// The sequence of stream positions a persistent-lane wave walks
// (refill_loop): virtual position c lies in virtual group c >> 6.  Static
// (work == nullptr): virtual group j is group k + j * K of the wave's own
// shard.  Dynamic: virtual groups come from take_group as the wave reaches
// them.  A window of two slots holds the groups one refill can touch (a
// refill takes at most 64 positions).  All members are wave-uniform.
// CLASSES: the stream holds two path classes (stream_index); otherwise
// position pos of shard s is stored at s * shard_cap + pos.
// TAG_A: at() sets the sign bit of a class-A position's stream index
// (CLASS_A_TAG; indices stay below 2^31), so the lane's finish step knows the
// class without a register of its own.
constexpr int CLASS_A_TAG = (int)0x80000000u;
template <bool CLASSES, bool TAG_A = false>
struct GroupSeq {
    const int* cnt;
    int* work;
    int shard_cap;
    WaveWork w;
    int s;
    uint64_t done;
    bool exhausted;
    int j0;                          // virtual group of slot 0
    int gs[2], gg[2], ga[2], gn[2]; // shard, group (< 0: empty slot), class-A count, count

    __device__ __forceinline__ ShardCount count_of(int sh) const {
        if constexpr (CLASSES) return shard_count(cnt, sh);
        const int n = uniform_load(cnt + sh * CSTRIDE);
        return ShardCount{n, n, n};
    }
    __device__ __forceinline__ void init(const int* cnt_, int* work_, int cap, const WaveWork& w_) {
        cnt = cnt_;
        work = work_;
        shard_cap = cap;
        w = w_;
        s = w.s;
        done = 0;
        exhausted = false;
        j0 = 0;
        gg[0] = gg[1] = -1;
    }
    // load the next virtual group (j0 + k) into slot k
    __device__ __forceinline__ bool fill(int k) {
        if (exhausted) return false;
        ShardCount sc = count_of(s);
        int g;
        if (work) {
            g = take_group(work, s, done, sc.n, [&](int sh_) {
                sc = count_of(sh_);
                return sc.n;
            });
        } else {
            g = w.k + (j0 + k) * w.K;
            if (g * 64 >= sc.n) g = -1;
        }
        if (g < 0) {
            exhausted = true;
            return false;
        }
        gs[k] = s;
        gg[k] = g;
        ga[k] = sc.a;
        gn[k] = sc.n;
        return true;
    }
    // make positions [cursor, cursor + m) resolvable as far as groups remain;
    // false once the sequence has nothing at cursor
    __device__ __forceinline__ bool reserve(int cursor, int m) {
        if (cursor >= (j0 + 1) * 64) { // slide the window
            gs[0] = gs[1];
            gg[0] = gg[1];
            ga[0] = ga[1];
            gn[0] = gn[1];
            gg[1] = -1;
            ++j0;
        }
        if (gg[0] < 0 && !fill(0)) return false;
        if (cursor + m > (j0 + 1) * 64 && gg[1] < 0) fill(1);
        return true;
    }
    // stream index of virtual position c (per lane); false: nothing there
    __device__ __forceinline__ bool at(int c, int& i) const {
        const int k = (c >> 6) - j0;
        const int g = k ? gg[1] : gg[0];
        if (g < 0) return false;
        const int pos = g * 64 + (c & 63);
        if (pos >= (k ? gn[1] : gn[0])) return false;
        const int sh = k ? gs[1] : gs[0];
        const int a = k ? ga[1] : ga[0];
        i = CLASSES ? stream_index(sh, pos, a, shard_cap) : sh * shard_cap + pos;
        if (TAG_A && pos < a) i |= CLASS_A_TAG;
        return true;
    }
};

template <int V0, bool STATS, bool LDS>
__global__ void __launch_bounds__(BLOCK, LDS ? REFILL_WAVES_LDS : (variant_q4(V0) ? REFILL_WAVES_Q4 : REFILL_WAVES)) k_trace_refill(FrameArgs fa, SceneView gsv, PathBuf in, HitBuf hits,
                                                                     const int* cnt, int tail_threshold,
                                                                     unsigned long long* stats, int refill_min, int* work) {
    // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: global node loads (no treelet)
    constexpr int V = LDS ? kernel_variant(V0, true) : V0;
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    if (row_total(cnt) <= tail_threshold) return; // k_finish takes the remaining paths
    const SceneView sv = LDS ? stage_scene_lds<BLOCK>(gsv, lds_scene) : stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    GroupSeq<true> seq;
    seq.init(cnt, work, in.shard_cap, wave_work());
    refill_loop<false, STATS, V>(
        sv, ts, seq, refill_min,
        [&](int i, Trav& t) -> bool {
            const float4 p0 = in.p0[i], p1 = in.p1[i];
            const int depth = (int)(__float_as_uint(p1.w) >> 24);
            if (depth == 0) {
                hits.h[i] = make_float4(0, 0, 0, __int_as_float(-1));
                hits.prim[i] = -1;
                return false;
            }
            float tmin, tmax;
            uint32_t rflags;
            ray_extent(fa, sv, depth, (int)(__float_as_uint(p0.w) & SLOT_MASK), tmin, tmax, rflags);
            trav_init(sv, t, f3of(p0), f3of(p1), tmin, tmax, rflags, ts);
            return true;
        },
        [&](int i, const Trav& t) {
            if (STATS && t.hit_ent >= 0) st.hits++;
            hits.h[i] = make_float4(t.tmax, t.hu, t.hv, __int_as_float(t.hit_ent));
            hits.prim[i] = t.hit_prim;
        },
        st);
    if (STATS) flush_stats<STATS>(st, stats, 0, true);
}

template <int V0, bool STATS, bool LDS>
__global__ void __launch_bounds__(BLOCK, LDS ? REFILL_WAVES_LDS : (variant_ifif(V0) ? SHADOW_IFIF_WAVES : REFILL_WAVES)) k_shadow_refill(SceneView gsv, ShadowBuf sh, float4* L, const int* cnt,
                                                                      unsigned long long* stats, int refill_min, int* work) {
    // LDS-staged tables: bit 3 (node steps skip the stack-top peek); global tables: treelet, except with if-if
    // stepping (the split schedule's scenes), where global node loads beat the
    // treelet's flat loads: soup-1M 32-iteration frame 1179.6 / 1188.1 ->
    // 1154.5 / 1153.5 ms (profiles/r03_ab_treelet_global.log)
    constexpr int V = LDS ? kernel_variant(V0, true) : ((SHADOW_TREELET && !variant_ifif(V0)) ? kernel_variant(V0, false) : V0);
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    extern __shared__ float4 lds_scene[];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, gsv.spill);
    if (row_total(cnt) == 0) return;
    const SceneView sv = LDS ? stage_scene_lds<BLOCK>(gsv, lds_scene) : stage_treelet<BLOCK>(gsv, lds_scene);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    GroupSeq<true, true> seq; // two shadow classes (wave_append_paths), class-A indices tagged
    seq.init(cnt, work, sh.shard_cap, wave_work());
    refill_loop<true, STATS, V>(
        sv, ts, seq, refill_min,
        [&](int it, Trav& t) -> bool {
            const int i = it & ~CLASS_A_TAG;
            const float4 s0 = sh.s0[i], s1 = sh.s1[i];
            trav_init(sv, t, f3of(s0), f3of(s1), 0.001f, s1.w, RAY_SHADOW, ts);
            return true;
        },
        [&](int it, const Trav& t) {
            // a class-A record under ShadowBuf::optimistic: k_extend added the
            // colour, an occluded ray puts the slot's previous value back (s2);
            // any other record: an unoccluded ray adds its colour
            const bool undo = sh.optimistic && it < 0;
            if (t.found != undo) return;
            const int i = it & ~CLASS_A_TAG;
            const int slot = __float_as_int(sh.s0[i].w);
            const float4 rec = sh.s2[i];
            if (undo) {
                L[slot] = rec;
                return;
            }
            add_radiance(L, slot, f3of(rec));
            add_aov(sh.aov_nee, slot, f3of(rec));
        },
        st);
    if (STATS) flush_stats<STATS>(st, stats, 4, false);
}

#if IGX_PART == 0
// resolve: fb += sum_s L_s / spi (driver/accumulator.art:13-19, make_standard_accumulator)
// A block owns 64 pixels; its RES_G waves sum one iteration each (lanes =
// pixels, the sample loop in order) into LDS, and wave 0 adds the iterations
// into the framebuffer in iteration order, so the float sums are those of one
// accumulation per render call.  One pixel per lane with all iterations in one
// lane was latency-bound (2.1 ms per 128M-path chunk); this form takes 1.4 ms.
// Coalesced loads through a 55 KB LDS transpose tile measured slower (3.2 ms):
// the kernel overlaps the next chunk's k_extend, whose LDS-resident BVH leaves
// no room for blocks with a large LDS footprint.
constexpr int RES_G = 8;
__global__ void __launch_bounds__(64 * RES_G) k_resolve(FrameArgs fa, const float4* L, float* fb, int fb_width) {
    __shared__ float part[RES_G][3][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    int x = 0, y = 0;
    const bool in = p < fa.chunk_pixels && local_to_global(fa, fa.chunk_pixel0 + p, x, y);
    const size_t o = 3 * ((size_t)y * fb_width + x);
    float fr = 0, fg = 0, fbb = 0;
    if (w == 0 && in) {
        fr = fb[o + 0];
        fg = fb[o + 1];
        fbb = fb[o + 2];
    }
    for (int it0 = 0; it0 < fa.chunk_iters; it0 += RES_G) { // block-uniform trip count
        const int it = it0 + w;
        if (in && it < fa.chunk_iters) {
            const float4* Li = L + ((size_t)it * fa.chunk_pixels + p) * fa.spi;
            float r = 0, g = 0, b = 0;
            if (fa.probe_sample) { // per-path probes (tests): sample probe_sample - 1 only
                const float4 l = Li[fa.probe_sample - 1];
                r = l.x * fa.inv_spi;
                g = l.y * fa.inv_spi;
                b = l.z * fa.inv_spi;
            } else {
#pragma unroll 8
                for (int s = 0; s < fa.spi; ++s) {
                    float4 l = Li[s];
                    r += l.x * fa.inv_spi;
                    g += l.y * fa.inv_spi;
                    b += l.z * fa.inv_spi;
                }
            }
            part[w][0][lane] = r;
            part[w][1][lane] = g;
            part[w][2][lane] = b;
        }
        __syncthreads();
        if (w == 0 && in) {
            const int m = min(RES_G, fa.chunk_iters - it0);
            for (int k = 0; k < m; ++k) { // one accumulation per iteration, in order
                fr += part[k][0][lane];
                fg += part[k][1][lane];
                fbb += part[k][2][lane];
            }
        }
        __syncthreads();
    }
    if (w == 0 && in) {
        fb[o + 0] = fr;
        fb[o + 1] = fg;
        fb[o + 2] = fbb;
    }
}

__global__ void k_pack_tiles(FrameArgs fa, const float* fb, float* dst, int num_tiles) {
    int T = fa.tile_size;
    long long total = (long long)num_tiles * T * T;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int x, y;
        bool in = local_to_global<false>(fa, (int)i, x, y); // each packed tile row-major
        for (int c = 0; c < 3; ++c) dst[3 * i + c] = in ? fb[3 * ((size_t)y * fa.width + x) + c] : 0.0f;
    }
}

#endif

// hit-level test kernels (one ray per lane)
template <int V>
__global__ void __launch_bounds__(BLOCK) k_trace_hits(SceneView sv, const float* rays, int n, uint32_t flags, int* ent_prim,
                                                      float* tuv, int any) {
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, sv.spill);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const float* r = rays + 8 * i;
        float tmax = r[7];
        int e, p;
        float u = 0, v = 0;
        if (any) {
            bool occ = trace_ray<true, false, V>(sv, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], tmax, flags, ts, e, p, u, v, st);
            ent_prim[i] = occ ? 1 : 0;
        } else {
            trace_ray<false, false, V>(sv, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], tmax, flags, ts, e, p, u, v, st);
            ent_prim[2 * i] = e;
            ent_prim[2 * i + 1] = p;
            tuv[3 * i] = e >= 0 ? tmax : r[7];
            tuv[3 * i + 1] = u;
            tuv[3 * i + 2] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// Denoiser feature buffers: the info-buffer technique (technique/infobuffer.art,
// InfoBufferTechnique.cpp), one extra pass with one sample per pixel that
// fills the AOVs "Normals", "Albedo" and "Depth" and leaves the film alone
// (LockFramebuffer, OverrideSPI = 1, InfoBufferTechnique.cpp:37-38).
//
// One lane per local pixel, grid-stride; the lane owns its pixel, so it adds
// to the three row-major RGB films with plain read-modify-writes, the
// iterations of a multi-iteration call in order inside the lane: no atomics,
// no per-slot buffers, bit-reproducible.  The camera path is sample 0 of the
// iteration (gen_path: the same seed and the same two jitter draws as the
// film's sample 0; in ray-list mode the ray of the list), traced against the
// global tables with the LDS stack of k_trace_hits.
// ---------------------------------------------------------------------------
struct InfoArgs {
    float* normals; // the three films, fb_width pixels per row
    float* albedo;
    float* depth;
    int fb_width;
    int mode;            // option "denoise_aovs" (host/aov_plan.h: INFO_FIRST, INFO_EVERY)
    int follow_specular; // option "denoise_follow_specular" (Denoiser.FollowSpecular)
    int max_depth;       // option "denoise_max_depth" (__tech_ib_max_depth, LoaderTechnique.cpp:133)
};

template <int V>
__global__ void __launch_bounds__(BLOCK) k_infobuffer(FrameArgs fa, SceneView sv, InfoArgs ia) {
    __shared__ int stack_mem[LDS_STACK * BLOCK];
    const TStack ts = make_tstack(stack_mem, LDS_STACK, sv.spill);
    constexpr bool FULL = variant_full(V);
    TraceStats st{0, 0, 0, 0, 0, 0, 0};
    const int iters = fa.chunk_iters, iter0 = fa.iter;
    fa.chunk_iters = 1; // slot lp of `fa` is sample 0 of local pixel lp in iteration fa.iter (spi 1)
    for (int lp = blockIdx.x * BLOCK + threadIdx.x; lp < fa.chunk_pixels; lp += gridDim.x * BLOCK) {
        int x, y;
        if (!local_to_global(fa, lp, x, y)) continue; // tile padding
        const size_t at = 3 * ((size_t)y * ia.fb_width + x);
        f3 nsum = mk(ia.normals[at], ia.normals[at + 1], ia.normals[at + 2]);
        f3 asum = mk(ia.albedo[at], ia.albedo[at + 1], ia.albedo[at + 2]);
        f3 dsum = mk(ia.depth[at], ia.depth[at + 1], ia.depth[at + 2]);
        // PixelCoord::linear = y * w + x (driver/camera.art:24); the list emitter's y is 0
        const uint32_t albedo_seed = hash_combine(0x811C9DC5u, (uint32_t)(y * fa.width + x));
        for (int k = 0; k < iters; ++k) {
            if (!info_pass_due(ia.mode, (int64_t)iter0 + k)) continue; // wave-uniform
            fa.iter = iter0 + k;
            const GenPath g = gen_path<FULL>(fa, sv, lp);
            f3 o = g.o, d = g.d;
            Rng rnd{g.seed, g.counter};
            float tmin, tmax;
            uint32_t rflags;
            ray_extent(fa, sv, 1, lp, tmin, tmax, rflags);
            // IBRayPayload (infobuffer.art:4-22): depth from 1, the distance travelled so far
            float travelled = 0;
            for (int depth = 1;;) {
                int hit_ent, hit_prim;
                float hu = 0, hv = 0;
                trace_ray<false, false, V>(sv, o, d, tmin, tmax, rflags, ts, hit_ent, hit_prim, hu, hv, st);
                if (hit_ent < 0) break; // TechniqueNoMissFunction: nothing is written
                int mat_id;
                const Surface s = surface_element(sv, hit_ent, hit_prim, tmax, hu, hv, o, d, mat_id);
                // the material as shade_step fetches it (a texture writes its value into a copy)
                std::conditional_t<FULL, DevMaterial, const DevMaterial&> m = sv.mats[mat_id];
                if constexpr (FULL)
                    if (sv.uv) {
                        apply_texture(sv, m, hit_ent, hit_prim, hu, hv);
                        bind_measured(sv, m);
                    }
                const f3 out_dir = neg(d);
                if (!(ia.follow_specular && bsdf_is_specular<FULL>(m))) {
                    // on_hit (infobuffer.art:34-61): the albedo from 16 BSDF samples of a
                    // generator of the pixel's own, without the cosine term
                    f3 albedo = mk(0, 0, 0);
                    Rng arnd{albedo_seed, 1};
#pragma unroll 1
                    for (int j = 0; j < 16; ++j) {
                        const BsdfSample bs = bsdf_sample<FULL>(m, s, arnd, out_dir);
                        if (bs.valid) {
                            const float c = absolute_cos(bs.in_dir, s.local.n);
                            albedo = add(albedo, mulf(bs.color, safe_div(bs.pdf, 16.0f * c)));
                        }
                    }
                    nsum = add(nsum, s.local.n);
                    asum = add(asum, mk(fminf(albedo.x, 1.0f), fminf(albedo.y, 1.0f), fminf(albedo.z, 1.0f))); // color_saturate(albedo, 1)
                    const float dist = tmax + (ia.follow_specular ? travelled : 0.0f);
                    dsum = add(dsum, mk(dist, dist, dist));
                    break;
                }
                // on_bounce (infobuffer.art:63-88): follow the specular surface
                if (!(depth <= ia.max_depth)) break;
                const BsdfSample bs = bsdf_sample<FULL>(m, s, rnd, out_dir);
                if (!bs.valid) break;
                travelled = travelled + tmax;
                ++depth;
                o = s.point;
                d = bs.in_dir;
                tmin = 0.001f;
                tmax = FLT_MAX_;
                rflags = RAY_BOUNCE;
            }
        }
        ia.normals[at] = nsum.x;
        ia.normals[at + 1] = nsum.y;
        ia.normals[at + 2] = nsum.z;
        ia.albedo[at] = asum.x;
        ia.albedo[at + 1] = asum.y;
        ia.albedo[at + 2] = asum.z;
        ia.depth[at] = dsum.x;
        ia.depth[at + 1] = dsum.y;
        ia.depth[at + 2] = dsum.z;
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// Two stream "slots" (path double-buffer, shadow stream, radiance, counters)
// alternate between chunks (a chunk = one iteration, or a capacity-sized part
// of it).  The wavefront bounces of chunk k run on the main stream; when the
// live-path count falls to the tail threshold, k_finish and the resolve of
// chunk k are queued on the tail stream and the host moves on to chunk k+1 in
// the other slot, so the latency-bound tail of one chunk overlaps the next
// chunk's full bounces.
struct TimedLaunch {
    hipEvent_t a, b;
    int kind; // 0 extend/shade, 1 shadow, 2 generate, 3 resolve, 4 finish, 5 trace
    int bounce;
};

struct Slot {
    size_t cap = 0;            // paths per chunk
    int shard_cap = 0;         // records per stream shard (NSH * shard_cap >= cap)
    PathBuf pa{}, pb{};
    ShadowBuf sh{};
    HitBuf hb{};
    float4* L = nullptr;
    float4* aov_di = nullptr;  // MIS AOV slots beside L (technique aov_mis): "Direct Weights",
    float4* aov_nee = nullptr; // "NEE Weights" (FrameArgs::aov_di / aov_nee)
    int* ctr = nullptr;        // device shard counters: row 2b = paths entering bounce b, row 2b+1 = shadow rays of bounce b (CROW ints per row)
    int* pinned = nullptr;     // host mirror
    long long n0 = 0;          // paths generated for the chunk (row 0)
    hipEvent_t done = nullptr; // recorded on the tail stream after the resolve
    std::vector<hipEvent_t> bounce_ev;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    std::vector<TimedLaunch> timed;
    // pending statistics of the chunk last run in this slot
    bool pending = false;
    int switch_bounce = 0;     // first bounce handled by k_finish
    int launched = 0;          // extend/shadow launch pairs queued (the last may find its count <= tail and exit at once)
    bool split = true;         // chunk ran k_trace + k_shade
    int tail = 0;
    long long camera = 0;
};

enum { DYN_EXTEND = 1, DYN_SHADOW = 2, DYN_REFILL_TRACE = 4, DYN_REFILL_SHADOW = 8 };
// rows WORK_ROW0 + 4b: k_extend (or k_trace_refill) group counters of bounce b (take_group),
// + 1: its mask of exhausted shards, + 2 / + 3: the same for k_shadow
constexpr int WORK_ROW0 = 2 * MAX_BOUNCES + 4;
// instrumentation counters (igx_get_stats): 0-12 visit counts, 16-19 k_extend
// phase clocks, 20-39 k_extend by group class, 40-49 k_shadow by class, 50-53
// closest-hit node visits in the TLAS and by hot-order rank, 54-69 k_extend
// shading sub-phase clocks by class, 70-71 k_shadow rays by class, 72-75 k_extend
// store phase by part (igx_get_store_split)
[[maybe_unused]] constexpr int DSTATS = 80;
constexpr int CTR_ROWS = WORK_ROW0 + 4 * MAX_BOUNCES;
[[maybe_unused]] constexpr size_t CTR_INTS = (size_t)CTR_ROWS * CROW;

// records in counter row `row` of the slot's host mirror (row 0: generated paths)
inline long long row_total(const Slot& s, int row) {
    if (row == 0) return s.n0;
    long long t = 0;
    const int* r = s.pinned + (size_t)row * CROW;
    for (int k = 0; k < NSH; ++k) t += r[k * CSTRIDE] + r[k * CSTRIDE + 1] + r[k * CSTRIDE + 2]; // classes A, B, C (wave_append_paths)
    return t;
}

} // namespace igxh

using namespace igxh;

struct igx_device {
    int hip_device = 0;
    hipStream_t stream = nullptr;  // main (wavefront) stream
    hipStream_t stream2 = nullptr; // slot 1's wavefront stream under concurrent chunks
    hipStream_t tail_stream = nullptr;
    std::string last_error;
    int num_cus = 256;
    size_t mem_total = 0;     // device memory (bytes)
    // options
    bool timing = false;
    bool instrument = false;
    int64_t capacity_opt = 0;
    // option "slot_budget_mb": device memory the two stream slots of this
    // handle may take (0 = auto: a quarter of the device memory)
    int64_t slot_budget_mb = 0;
    // option "stream_slots": chunks alternate between two slots (chunk k + 1's
    // bounces overlap chunk k's tail), or use one (half the memory; chunk k + 1
    // waits for chunk k).  A rank of a multi-GPU render holds two handles that
    // alternate frames, and a rank's share of a frame is one chunk, so there
    // one slot per handle loses nothing: bench.py sets 1 at N > 1
    int stream_slots = 2;
    // option "concurrent_chunks" (0/1): the fused schedule's chunks run
    // through ChunkScheduler, the two slots' chunks concurrently, each on its
    // own stream (one slot: a chunk still waits for the slot's previous one)
    int concurrent_opt = 1;
    int concurrent_start_pct = 10; // option "concurrent_start_pct": a chunk starts once the running one is down to this share of its paths
    // LDS treelet (stage_treelet) on global-table scenes: nodes staged per
    // kernel (the largest prefix of the hot order that keeps the kernel's
    // register-bound occupancy), recomputed when the scene or option changes.
    // Option "treelet": -1 auto, 0 off, n > 0 at most n nodes
    int tail_pairs_opt = -1;  // k_finish_pairs on global-table scenes (-1 auto = on, 0 off, 1 on)
    // The treelet kernels are k_extend and k_shadow / k_shadow_refill (not the
    // if-if variant): primitives 8.89 -> 8.37, S-deep 48.2 -> 45.8, soup-1M
    // 187.9 -> 184.9 ms per frame
    int64_t treelet_opt = -1;
    bool tree_dirty = true;
    int tree_ext = 0, tree_shadow = 0;
    int64_t tail_opt = -1;   // paths at or below which k_finish takes over (-1 = auto)
    int64_t tail_last_opt = -1; // the same for the last chunk of a render call, whose tail overlaps nothing (-1 = tail_opt)
    bool fuse_generate = true; // bounce 0 of the fused k_extend builds its camera paths (no k_generate pass)
    int split_opt = -1;      // k_trace + k_shade per bounce instead of the fused k_extend (-1: auto = global-table scenes)
    int refill_opt = -1;     // persistent-lane trace / shadow, refilled once this many lanes idle (0: off, -1: auto = 16)
    int shadow_ifif_opt = -1; // if-if stepping in k_shadow_refill (-1: auto = split-schedule scenes)
    int64_t lds_scene_max = 48 * 1024; // stage traversal tables in LDS when they fit (0 = never)
    size_t lds_scene_bytes = 0;        // bytes staged per block for the current scene (0 = global tables)
    // k_extend's LDS layout for the current scene (configure_lds, host/lds_plan.h):
    // option "lds_shading" (-1 auto = LDS_SHADING_AUTO, 0 today's 256-thread
    // kernel exactly, 1 the wide block with the shading tables staged when it
    // fits); option "lds_shading_max" caps the staged shading tables' bytes
    int lds_shading_opt = -1;
    int64_t lds_shading_max = 48 * 1024;
    size_t lds_shading_bytes = 0;      // shading-table bytes staged behind the traversal tables (0: not staged)
    int ext_block = BLOCK;             // threads per block of k_extend (BLOCK_WIDE with the shading tables staged)
    size_t lds_shading_tab[LDS_TAB_COUNT] = {}; // the current scene's shading tables by LdsPlan table
    size_t lds_per_block = 64 * 1024;  // device attribute: LDS one workgroup may take
    size_t table_bytes = 0;            // traversal tables (nodes, instances, triangles) of the current scene
    size_t shading_bytes = 0;          // shading tables (entities, vertices, normals, faces, materials, lights)
    size_t image_bytes = 0, cdf_bytes = 0; // image textures' texels and environment maps' sampling tables (in the uv table)
    size_t measured_bytes = 0;             // measured BSDFs' words (in the uv table)
    int leaf_size = 4;
    // stream class of surviving paths (FrameArgs::classify; option "path_classes"):
    // paths inside a dielectric go to the back of their shard, so the next
    // bounce's waves are all-inside or all-outside (diamond frame 152-155 ->
    // 143-145 ms, S-deep 49.1 -> 47.5 ms per 8-iteration frame; bit-identical)
    // 3: also paths whose next ray crosses an enclosing entity's world box
    // (diamond frame 132.5 -> 119.3 ms, k_extend 1770 -> 1591 us per launch,
    // bit-identical)
    // 4: three classes, the paths inside a dielectric in their own region of
    // the path buffers (class C), apart from those heading for the box (B):
    // diamond frame 109.6 -> 106.4 ms, bit-identical; the split schedule
    // falls back to 3 (its hit records have no class-C region)
    int classify_opt = 4;
    // option "shadow_classes": shadow rays whose segment crosses an enclosing
    // entity's box apart from the rest (shadow_class_b), 0/1: diamond shadow
    // time 26.9 -> 21.7 ms per frame, frame 121.1 -> 118.4 ms, bit-identical
    int shadow_classes_opt = 1;
    // option "shadow_optimistic" (-1 auto, 0 off, 1 on; use_shadow_optimistic):
    // k_extend adds a class-A shadow ray's colour to the radiance slot itself,
    // the shadow kernel only undoes it for the occluded ones (FrameArgs::
    // shadow_optimistic; bit-identical)
    int shadow_optimistic_opt = -1;
    // option "extend_shapes" (-1 auto, 0 generic only, 1 specialised where
    // eligible; pick_extend_shape, host/extend_shape.h): launches of the
    // default fused mode run k_extend's generate / bounce shapes
    // (bit-identical)
    int extend_shapes_opt = -1;
    // option "dynamic" (DYN_* bits): DYN_EXTEND = k_extend waves take their
    // groups of 64 paths from per-shard counters (take_group) instead of a
    // fixed grid stride: diamond frame 142.4 -> 134.3 ms, materials 66.5 ->
    // 54.6, primitives 36.8 -> 33.9, bit-identical images; DYN_SHADOW = the
    // same for k_shadow (measured neutral: shadow rays cost about the same);
    // DYN_REFILL_TRACE / DYN_REFILL_SHADOW: the persistent-lane kernels
    // draw their groups the same way (GroupSeq): soup-1M 8-iteration frame
    // 452 -> 382 ms (k_shadow_refill 220 -> 164, k_trace_refill 205 -> 193),
    // S-deep 52.7 -> 48.6 ms
    int dynamic_opt = DYN_EXTEND | DYN_REFILL_TRACE | DYN_REFILL_SHADOW;
    // option "group_order": 1 = k_extend takes a shard's groups from its end
    // (classes C, B, A: longest paths first), 0 = from its front, -1 = auto
    int group_order_opt = -1;
    // option "face_normals": precomputed world-space face normals for scenes
    // with at most FACE_NORMAL_TABLE_MAX face instances (next upload)
    int face_normals_opt = 1;
    // option "face_shade": per-face shading records (SceneView::fsh) for
    // scenes with at most FACE_SHADE_MAX faces (next upload)
    int face_shade_opt = 1;
    float sah_node_cost = 1.0f;    // option "sah_node_cost_pct" (percent of one triangle test)
    int bvh_bins = 32;             // option "bvh_bins": SAH bins per axis of the BLAS builds (next upload)
    int bvh_bins_tlas = 32;        // option "bvh_bins_tlas": the same for the TLAS
    // SBVH for BLAS up to SPATIAL_SPLIT_MAX_FACES triangles (option "spatial_splits"):
    // off by default -- measured slower on the diamond (196 -> 230 ms per frame)
    // and neutral on primitives, S-deep and soup-1M
    bool spatial_splits = false;
    // 1: build every BLAS here even when the scene carries the reference's own
    // (igx_shape::ref_bvh, from the SceneDatabase adapter)
    bool rebuild_bvh = false;
    // scene
    bool has_scene = false;
    std::vector<void*> scene_allocs;
    SceneView sv{};
    igx_camera cam_desc{};
    // film size, frame and seed of igx_camera_rays: the scene's film until a
    // render call (not in ray-list mode) sets its own
    int rays_w = 0, rays_h = 0, rays_frame = 0, rays_seed = 0;
    int variant = 0;       // traversal variant of the scene (device_scene.h: width, spill)
    int bvh_width = 2;     // node width of the uploaded tables
    bool quantized = false; // the 4-wide nodes are quantised (Bvh4QNode, 64 B; variant bit 7)
    int quantize_opt = -1;  // option "bvh_quantize": -1 auto (4-wide scenes whose tables stay in global memory), 0, 1
    int nf4 = 4;            // float4s per node of the uploaded tables
    int bvh_width_opt = 0; // option "bvh_width": 0 = auto, 2, 4 (applies at the next upload)
    bool full_shading = false;     // the scene needs materials / lights beyond the basic set
    bool full_shading_opt = false; // option "full_shading": 1 = always compile-in the whole set
    // option "enclosing": paths inside a closed, isolated dielectric trace
    // only its BLAS (trace_enclosed); applies at the next upload
    bool enclosing_opt = true;
    int scene_depth = 0;   // worst-case stack entries of the scene
    int* spill_main = nullptr; // spill columns of the main, tail and shadow streams (and of slot 1's stream)
    int* spill_tail = nullptr;
    int* spill_shadow = nullptr;
    int* spill_main2 = nullptr;
    hipStream_t shadow_stream = nullptr; // split schedule: shadow rays of bounce b overlap the trace of bounce b + 1
    int overlap_shadow_opt = 1;           // option "overlap_shadow" (0/1)
    // streams
    Slot slots[2];
    int next_slot = 0;
    unsigned long long* dstats = nullptr;      // instrumentation counters
    unsigned long long* tail_counts = nullptr; // [2]: tail continuation rays, tail shadow rays
    float* ray_list = nullptr;
    size_t ray_list_cap = 0;
    // framebuffer
    float* fb = nullptr;
    size_t fb_count = 0;
    // MIS AOV films ("Direct Weights", "NEE Weights"; technique aov_mis), fb_count floats each
    bool aov_on = false;
    float* aov_fb[2] = {nullptr, nullptr};
    int fb_w = 0, fb_h = 0;
    uint64_t iteration_count = 0;
    // Denoiser feature buffers "Normals", "Albedo", "Depth" (k_infobuffer),
    // fb_count floats each, in ray-list mode too; every one with its own
    // iteration count (Device.cpp:1390-1403, 1468-1471).  Options
    // "denoise_aovs" (host/aov_plan.h: INFO_OFF, INFO_FIRST, INFO_EVERY),
    // "denoise_follow_specular", "denoise_max_depth" (LoaderTechnique.cpp:133)
    int info_mode = INFO_OFF;
    bool info_follow_specular = false;
    int info_max_depth = 8;
    float* info_fb[AOV_INFO_COUNT] = {nullptr, nullptr, nullptr};
    uint64_t info_count[AOV_INFO_COUNT] = {0, 0, 0};
    // option "timing": the event pairs around the info-buffer passes queued
    // since the last drain (folded into ms_generate there)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> info_timed;
    // film post-processing scratch (igx_tonemap / igx_imageinfo, igx_post.h):
    // the luminance plane, the per-block slab, the result + histograms and the
    // packed image; grown on demand, rewritten by every call
    void* post_buf[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t post_cap[4] = {0, 0, 0, 0};
    // stats
    igx_stats stats{};
    // asynchronous rendering (option "async_render"): the worker thread and
    // its queue (render_impl, igx_clear); nullptr until the first queued render
    int async_opt = 1;
    struct AsyncRender* async = nullptr;
    // option "host_wait_us": the chunk scheduler's host thread sleeps this long
    // between polls that found no progress (after a few yields); 0 = yield only
    int host_wait_us = 20;
    // option "fail_chunk" (test hook): the n-th chunk the chunk scheduler
    // starts from now on fails with IGX_ERR_HIP instead
    int64_t fail_chunk_opt = 0;
    // option "probe_sample" (test hook): s + 1 = the film receives sample s of
    // each pixel only (the other paths are traced as usual), 0 = every sample
    int64_t probe_sample_opt = 0;
};
// the worker has queued everything submitted; its first error (part 0)
igx_status wait_idle(igx_device* dev);
igx_status wait_ready(igx_device* dev);
bool reset_async_failure(igx_device* dev);
void stop_async(igx_device* dev);

namespace igxh {

#if IGX_PART == 0
// Set on a handle's async worker thread (async_worker): errors raised there
// go to the worker's own message, which the host thread copies into
// last_error (wait_idle / wait_ready); the host thread alone writes last_error.
thread_local std::string* t_error_sink = nullptr;
igx_status fail(igx_device* d, igx_status s, const std::string& msg) {
    if (t_error_sink) *t_error_sink = msg;
    else if (d) d->last_error = msg;
    return s;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(dev, e_ == hipErrorOutOfMemory ? IGX_ERR_OUT_OF_MEMORY : IGX_ERR_HIP,         \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                           \
    } while (0)

// Copy a host table to the device.  T is the table's host element type
// (host/scene_tables.h), D the type the kernels read it as.
static_assert(sizeof(igx::Float4) == sizeof(float4) && alignof(igx::Float4) == alignof(float4), "igx::Float4 is the device's float4");
static_assert(sizeof(igx::Int4) == sizeof(int4) && alignof(igx::Int4) == alignof(int4), "igx::Int4 is the device's int4");
static_assert(sizeof(igx::Float2) == sizeof(float2) && alignof(igx::Float2) == alignof(float2), "igx::Float2 is the device's float2");
static_assert(sizeof(igx::Int2) == sizeof(int2) && alignof(igx::Int2) == alignof(int2), "igx::Int2 is the device's int2");
template <typename T, typename D>
igx_status upload(igx_device* dev, const std::vector<T>& v, const D** out) {
    static_assert(sizeof(T) == sizeof(D) && alignof(T) == alignof(D), "the host element is the device element");
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    dev->scene_allocs.push_back(p);
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const D*>(p);
    return IGX_OK;
}

void free_scene(igx_device* dev) {
    for (void* p : dev->scene_allocs) (void)hipFree(p);
    dev->scene_allocs.clear();
    dev->spill_main = dev->spill_tail = dev->spill_shadow = dev->spill_main2 = nullptr;
    dev->has_scene = false;
}

// Largest grid any stream kernel is launched with (grid_for).
int max_grid(const igx_device* dev) {
    return std::max(GRID_QUANTUM, dev->num_cus * MAX_BLOCKS_PER_CU / GRID_QUANTUM * GRID_QUANTUM);
}

// Traversal variant of the scene and the spill columns for the stack entries
// beyond the LDS_STACK in LDS: one per grid thread of the largest grid, per
// stream.
igx_status configure_stack(igx_device* dev) {
    const int need = dev->scene_depth;
    const int extra = std::max(0, need - LDS_STACK);
    dev->variant = (dev->bvh_width >= 4 ? 2 : 0) | (extra > 0 ? 1 : 0) | (dev->full_shading ? 4 : 0) | (dev->quantized ? VARIANT_Q4 : 0);
    const size_t threads = (size_t)max_grid(dev) * BLOCK;
    for (int k = 0; k < 4; ++k) {
        int*& old = k == 0 ? dev->spill_main : k == 1 ? dev->spill_tail : k == 2 ? dev->spill_shadow : dev->spill_main2;
        if (old) {
            auto it = std::find(dev->scene_allocs.begin(), dev->scene_allocs.end(), (void*)old);
            if (it != dev->scene_allocs.end()) dev->scene_allocs.erase(it);
            (void)hipFree(old);
            old = nullptr;
        }
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, std::max<size_t>(16, (size_t)extra * threads * sizeof(int))));
        dev->scene_allocs.push_back(p);
        (k == 0 ? dev->spill_main : k == 1 ? dev->spill_tail : k == 2 ? dev->spill_shadow : dev->spill_main2) = static_cast<int*>(p);
    }
    dev->sv.spill = dev->spill_main;
    return IGX_OK;
}

void free_slot_buffers(Slot& s) {
    // a path buffer's four arrays and the shadow stream's three are one block each (ensure_slot)
    void* ptrs[] = {s.pa.p0, s.pb.p0, s.sh.s0, s.L, s.hb.h, s.hb.prim, s.aov_di, s.aov_nee};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    s.pa = PathBuf{};
    s.pb = PathBuf{};
    s.sh = ShadowBuf{};
    s.hb = HitBuf{};
    s.L = nullptr;
    s.aov_di = s.aov_nee = nullptr;
    s.cap = 0;
    s.shard_cap = 0;
}

// `hits`: the chunk runs the split schedule, whose k_trace writes a hit
// record per path (20 B) for k_shade; the fused schedule needs none.
// `region_c`: three path classes (FrameArgs::classify 4), so each path buffer
// holds a second set of records for class C (PathBuf::c_base); `aov`: the
// MIS AOV slots (technique aov_mis)
igx_status ensure_slot(igx_device* dev, Slot& s, size_t cap, bool hits, bool region_c, bool aov) {
    if (!s.ctr) {
        HIPCHK(hipMalloc((void**)&s.ctr, CTR_INTS * sizeof(int)));
        HIPCHK(hipHostMalloc((void**)&s.pinned, CTR_INTS * sizeof(int), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        std::memset(s.pinned, 0, CTR_INTS * sizeof(int));
    }
    if (s.cap >= cap && (!hits || s.hb.h) && (!region_c || s.pa.c_base) && (!aov || s.aov_di)) return IGX_OK;
    free_slot_buffers(s);
    // shard capacity: a generated chunk puts at most ceil(cap / (64 NSH)) groups
    // of 64 paths in one shard, and a shard's outputs never exceed its inputs
    const int shard_cap = (int)((cap + 64 * NSH - 1) / (64 * NSH)) * 64;
    const size_t recs = (size_t)shard_cap * NSH;
    auto alloc4 = [&](float4** p, size_t k) -> igx_status { HIPCHK(hipMalloc((void**)p, k * sizeof(float4))); return IGX_OK; };
    igx_status st;
    const size_t precs = region_c ? 2 * recs : recs;
    // One block per stream, its arrays back to back (p0, p1, p2, then p3; s0,
    // s1, s2): k_extend's shapes derive the arrays from the first pointer and
    // the shard capacity (streams_packed, host/extend_shape.h)
    for (PathBuf* b : {&s.pa, &s.pb}) {
        HIPCHK(hipMalloc((void**)&b->p0, precs * (3 * sizeof(float4) + sizeof(float2))));
        b->p1 = b->p0 + precs;
        b->p2 = b->p0 + 2 * precs;
        b->p3 = reinterpret_cast<float2*>(b->p0 + 3 * precs);
    }
    s.pa.c_base = s.pb.c_base = region_c ? (int)recs : 0;
    if ((st = alloc4(&s.sh.s0, 3 * recs))) return st;
    s.sh.s1 = s.sh.s0 + recs;
    s.sh.s2 = s.sh.s0 + 2 * recs;
    if ((st = alloc4(&s.L, cap))) return st; // radiance is indexed by path slot, not sharded
    if (aov && ((st = alloc4(&s.aov_di, cap)) || (st = alloc4(&s.aov_nee, cap)))) return st;
    if (hits) {
        if ((st = alloc4(&s.hb.h, recs))) return st;
        HIPCHK(hipMalloc((void**)&s.hb.prim, recs * sizeof(int)));
    }
    s.pa.shard_cap = s.pb.shard_cap = s.sh.shard_cap = shard_cap;
    s.cap = cap;
    s.shard_cap = shard_cap;
    return IGX_OK;
}

hipEvent_t slot_event(Slot& s) {
    if (s.ev_next >= s.ev_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        s.ev_pool.push_back(e);
    }
    return s.ev_pool[s.ev_next++];
}

// Grid of a stream kernel: enough blocks for `items`, at most the resident
// blocks, always a multiple of GRID_QUANTUM (every shard gets the same waves).
// `block`: the kernel's threads per block (BLOCK, or the wide k_extend's): the
// quantum is NSH over its waves, and a CU holds 2048 threads of any block
// size, so no grid has more threads than max_grid's (the spill columns).
int grid_for(igx_device* dev, long long items, int blocks_per_cu, int block = BLOCK) {
    const long long q = NSH / (block / 64);
    long long need = (items + block - 1) / block;
    long long cap = (long long)dev->num_cus * std::min(blocks_per_cu, MAX_BLOCKS_PER_CU * BLOCK / block);
    long long g = std::min((need + q - 1) / q * q, std::max(q, cap / q * q));
    return (int)std::max(q, g);
}

#endif // IGX_PART == 0

// Kernel schedule per scene (measured per scene):
//  * traversal tables in LDS (<= 48 KB): fused k_extend, grid-stride k_shadow;
//  * tables in global memory: shadow rays with persistent lanes (k_shadow_refill,
//    a refill once refill_min lanes idle);
//  * tables beyond 64 MiB: also split the bounce into k_trace (persistent
//    lanes) + k_shade -- there most node steps wait on an Infinity-Cache /
//    HBM round trip, and a traversal-only kernel keeps more waves resident
//    and lets lanes refill.  Below, the fused kernel with dynamic groups is
//    faster (no hit records): S-deep (18 MB of tables) 49.4 -> 46.9 ms per
//    8-iteration frame fused, soup-1M (104 MB) 382 split vs 451 fused.
// order in which k_extend's dynamic groups take a shard's positions (option "group_order" -1)
#ifndef GROUP_ORDER_AUTO
#define GROUP_ORDER_AUTO 0
#endif
// tail kernel with lane pairs (k_finish_pairs) on global-table scenes; option "tail_pairs" (-1 auto, 0, 1)
inline bool use_tail_pairs(const igx_device* dev) {
    return dev->lds_scene_bytes == 0 && (dev->tail_pairs_opt < 0 ? true : dev->tail_pairs_opt != 0);
}
// dynamic LDS of a global-table kernel that stages `nodes` treelet nodes
inline size_t tree_bytes(const igx_device* dev, int nodes) { return (size_t)nodes * dev->nf4 * 16; }
inline int refill_min(const igx_device* dev) { return dev->refill_opt >= 0 ? dev->refill_opt : 16; }
// auto: global-table scenes only; an explicit "refill" applies to LDS-staged scenes too
inline bool use_refill(const igx_device* dev) {
    return refill_min(dev) > 0 && (dev->lds_scene_bytes == 0 || dev->refill_opt > 0);
}
inline bool use_split(const igx_device* dev) {
    return dev->split_opt >= 0 ? dev->split_opt != 0 : (dev->lds_scene_bytes == 0 && dev->table_bytes > SPLIT_TABLE_BYTES);
}
// if-if stepping for the persistent-lane shadow kernel (variant bit 4): on the
// big-table scenes of the split schedule a lane at a leaf no longer waits for
// the wave's slowest inner-node walk (any-hit rays end at their first
// occluder, so their lengths vary most); on S-deep-sized tables the while-while
// loop is faster.  Option "shadow_ifif": -1 auto, 0 off, 1 on.
inline bool use_shadow_ifif(const igx_device* dev) {
    return dev->shadow_ifif_opt >= 0 ? dev->shadow_ifif_opt != 0 : use_split(dev);
}
// k_extend adds class-A shadow colours itself and the shadow kernel undoes the
// occluded ones (option "shadow_optimistic": -1 auto, 0 off, 1 on).  Only on
// the fused schedule (k_shade is left as it is) and without the MIS AOVs
// ("NEE Weights" needs the colour in the record); auto also asks for shadow
// classes and an enclosing entity, which give class A its meaning (rays that
// are almost never occluded), 1 takes every front-of-shard record.
inline bool use_shadow_optimistic(const igx_device* dev, bool split, bool aovs) {
    if (dev->shadow_optimistic_opt == 0 || split || aovs) return false;
    return dev->shadow_optimistic_opt > 0 || (dev->shadow_classes_opt && dev->sv.num_enc > 0);
}

// Where a chunk's launches go: the stream of its bounces, of its tail kernel
// and of its shadow kernels (the main stream again unless they overlap the
// next bounce's trace), the spill columns that go with each stream, and the
// camera of the chunk's render call.  The launch helpers take all of it from
// here, none of it from the handle.
struct LaunchCtx {
    hipStream_t main, tail, shadow;
    int *spill_main, *spill_tail, *spill_shadow;
    CameraModel cam;
};
// the scene view of a launch on the stream whose spill columns are `spill`
inline SceneView launch_view(const igx_device* dev, const LaunchCtx& ctx, int* spill) {
    SceneView sv = dev->sv;
    set_camera(sv, ctx.cam);
    sv.spill = spill;
    return sv;
}

// The one switch from the scene's variant word to a kernel's template
// argument: f is called with std::integral_constant<int, V> of the matching
// case and its result returned.  Traversal kernels take the six traversal
// variants (bit 7, VARIANT_Q4: quantised 4-wide nodes, only with bit 1) ...
template <typename F>
auto with_traversal_variant(int v, F&& f) {
    switch (v & (3 | VARIANT_Q4)) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 2 | VARIANT_Q4: return f(std::integral_constant<int, 130>{});
    default: return f(std::integral_constant<int, 131>{});
    }
}
// ... and shading kernels the twelve that add the material/light feature bit
template <typename F>
auto with_shading_variant(int v, F&& f) {
    switch (v & (7 | VARIANT_Q4)) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 2 | VARIANT_Q4: return f(std::integral_constant<int, 130>{});
    case 3 | VARIANT_Q4: return f(std::integral_constant<int, 131>{});
    case 6 | VARIANT_Q4: return f(std::integral_constant<int, 134>{});
    default: return f(std::integral_constant<int, 135>{});
    }
}

// Which instantiation a launch runs is chosen once per kernel family, by a
// chooser that returns what the launch, the occupancy query behind its grid
// and the raise of its dynamic-LDS limit have to agree on.  All instantiations
// of one kernel template share a signature, so the kernel travels as a typed
// pointer.  A kernel's address is taken only in the part that holds its device
// code: each part defines the choosers of its kernels (plain functions, declared
// here for all parts), part 0 launches and queries what they return.
using ExtendKernel = void (*)(FrameArgs, SceneView, PathBuf, PathBuf, ShadowBuf, float4*, KernelCounters, int);
using TraceKernel = void (*)(FrameArgs, SceneView, PathBuf, HitBuf, const int*, int, unsigned long long*);
using TraceRefillKernel = void (*)(FrameArgs, SceneView, PathBuf, HitBuf, const int*, int, unsigned long long*, int, int*);
using ShadeKernel = void (*)(FrameArgs, SceneView, PathBuf, HitBuf, PathBuf, ShadowBuf, float4*, KernelCounters, int);
using ShadowKernel = void (*)(SceneView, ShadowBuf, float4*, const int*, unsigned long long*, int*);
using ShadowRefillKernel = void (*)(SceneView, ShadowBuf, float4*, const int*, unsigned long long*, int, int*);
using FinishKernel = void (*)(FrameArgs, SceneView, PathBuf, float4*, const int*, int, unsigned long long*, unsigned long long*);
using InfoKernel = void (*)(FrameArgs, SceneView, InfoArgs);
template <typename K>
const void* kernel_id(K kernel) { return reinterpret_cast<const void*>(kernel); }
struct KernelChoice {
    // the kernel whose resident blocks per CU size the grid: the launched one,
    // except for the shaped k_extend and the if-if k_shadow_refill (below)
    const void* sized_by = nullptr;
    int block = BLOCK;
    size_t dyn = 0; // dynamic LDS: the staged tables, or the treelet's tree_n nodes
    int tree_n = 0; // SceneView::tree_n of the launch
};
struct ExtendChoice : KernelChoice { ExtendKernel kernel = nullptr; };
// the split schedule's trace and the shadow kernel come with and without
// persistent lanes, two templates with two signatures: one of the two is set
struct TraceChoice : KernelChoice { TraceKernel kernel = nullptr; TraceRefillKernel refill = nullptr; };
struct ShadowChoice : KernelChoice { ShadowKernel kernel = nullptr; ShadowRefillKernel refill = nullptr; };
struct FinishChoice : KernelChoice { FinishKernel kernel = nullptr; };
struct ShadeChoice : KernelChoice { ShadeKernel kernel = nullptr; };
struct InfoChoice : KernelChoice { InfoKernel kernel = nullptr; };

// k_extend spans five parts; each exports the pick among its instantiations
// and choose_extend (part 0) combines them.  The generate and bounce shapes
// (host/extend_shape.h) are never instrumented.
ExtendKernel extend_kernel(int v, bool stats, bool lds);         // part 1: BLOCK threads, LDS-staged or global tables
ExtendKernel extend_kernel_wide(int v, bool stats);              // part 4: BLOCK_WIDE threads, shading tables staged too
ExtendKernel extend_kernel_shaped_wide(int v, ExtendShape shape);   // part 7
ExtendKernel extend_kernel_shaped_lds(int v, ExtendShape shape);    // part 8
ExtendKernel extend_kernel_shaped_global(int v, ExtendShape shape); // part 9
ExtendChoice choose_extend(const igx_device* dev, bool stats, ExtendShape shape);
TraceChoice choose_trace(const igx_device* dev, bool stats);   // part 3
ShadowChoice choose_shadow(const igx_device* dev, bool stats); // part 3
ShadeChoice choose_shade(bool full);                           // part 3
FinishChoice choose_finish(const igx_device* dev, bool stats); // part 2
InfoChoice choose_infobuffer(int v);                           // part 5

#if IGX_PART == 1
ExtendKernel extend_kernel(int v, bool stats, bool lds) {
    return with_shading_variant(v, [&](auto V) -> ExtendKernel {
        constexpr int S = decltype(V)::value;
        if (lds) return stats ? k_extend<S, true, true> : k_extend<S, false, true>;
        return stats ? k_extend<S, true, false> : k_extend<S, false, false>;
    });
}
#endif
#if IGX_PART == 4
ExtendKernel extend_kernel_wide(int v, bool stats) {
    return with_shading_variant(v, [&](auto V) -> ExtendKernel {
        constexpr int S = decltype(V)::value;
        return stats ? k_extend<S, true, true, BLOCK_WIDE> : k_extend<S, false, true, BLOCK_WIDE>;
    });
}
#endif
#if IGX_PART == 7
ExtendKernel extend_kernel_shaped_wide(int v, ExtendShape shape) {
    return with_shading_variant(v, [&](auto V) -> ExtendKernel {
        constexpr int S = decltype(V)::value;
        return shape == EXTEND_GENERATE ? k_extend<S, false, true, BLOCK_WIDE, EXTEND_GENERATE> : k_extend<S, false, true, BLOCK_WIDE, EXTEND_BOUNCE>;
    });
}
#endif
#if IGX_PART == 8
ExtendKernel extend_kernel_shaped_lds(int v, ExtendShape shape) {
    return with_shading_variant(v, [&](auto V) -> ExtendKernel {
        constexpr int S = decltype(V)::value;
        return shape == EXTEND_GENERATE ? k_extend<S, false, true, BLOCK, EXTEND_GENERATE> : k_extend<S, false, true, BLOCK, EXTEND_BOUNCE>;
    });
}
#endif
#if IGX_PART == 9
ExtendKernel extend_kernel_shaped_global(int v, ExtendShape shape) {
    return with_shading_variant(v, [&](auto V) -> ExtendKernel {
        constexpr int S = decltype(V)::value;
        return shape == EXTEND_GENERATE ? k_extend<S, false, false, BLOCK, EXTEND_GENERATE> : k_extend<S, false, false, BLOCK, EXTEND_BOUNCE>;
    });
}
#endif

#if IGX_PART == 2
FinishChoice choose_finish(const igx_device* dev, bool stats) {
    const bool lds = dev->lds_scene_bytes != 0, pairs = use_tail_pairs(dev); // pairs: global tables only
    FinishChoice c;
    c.dyn = dev->lds_scene_bytes; // the tail kernels stage no treelet (tree_n 0)
    c.kernel = with_shading_variant(dev->variant, [&](auto V) -> FinishKernel {
        constexpr int S = decltype(V)::value;
        if (pairs) return stats ? k_finish_pairs<S, true> : k_finish_pairs<S, false>;
        if (lds) return stats ? k_finish<S, true, true> : k_finish<S, false, true>;
        return stats ? k_finish<S, true, false> : k_finish<S, false, false>;
    });
    c.sized_by = kernel_id(c.kernel);
    return c;
}
#endif

#if IGX_PART == 3
TraceChoice choose_trace(const igx_device* dev, bool stats) {
    const bool lds = dev->lds_scene_bytes != 0;
    TraceChoice c;
    c.dyn = dev->lds_scene_bytes; // on global tables neither kernel stages a treelet (tree_n 0)
    with_traversal_variant(dev->variant, [&](auto V) {
        constexpr int S = decltype(V)::value;
        if (use_refill(dev)) {
            if (lds) c.refill = stats ? k_trace_refill<S, true, true> : k_trace_refill<S, false, true>;
            else c.refill = stats ? k_trace_refill<S, true, false> : k_trace_refill<S, false, false>;
        } else {
            // k_trace (the split schedule without persistent lanes): 5 waves per SIMD
            // on global tables; LDS-staged tables set occupancy themselves
            if (lds) c.kernel = stats ? k_trace<S, true, 1, true> : k_trace<S, false, 1, true>;
            else c.kernel = stats ? k_trace<S, true, 5, false> : k_trace<S, false, 5, false>;
        }
    });
    c.sized_by = c.refill ? kernel_id(c.refill) : kernel_id(c.kernel);
    return c;
}
ShadowChoice choose_shadow(const igx_device* dev, bool stats) {
    const bool lds = dev->lds_scene_bytes != 0;
    ShadowChoice c;
    c.tree_n = dev->tree_shadow;
    c.dyn = lds ? dev->lds_scene_bytes : tree_bytes(dev, c.tree_n);
    with_traversal_variant(dev->variant, [&](auto V) {
        constexpr int S = decltype(V)::value;
        if (use_refill(dev)) {
            if (lds) c.refill = stats ? k_shadow_refill<S, true, true> : k_shadow_refill<S, false, true>;
            else c.refill = stats ? k_shadow_refill<S, true, false> : k_shadow_refill<S, false, false>;
            c.sized_by = kernel_id(c.refill);
            // The if-if kernel (variant bit 4, SHADOW_IFIF_WAVES) keeps the grid of the
            // while-while kernel (REFILL_WAVES) it replaces; no reason is recorded, and
            // igx_stats::shadow_blocks_per_cu reports the same figure
            if (!lds && use_shadow_ifif(dev)) c.refill = stats ? k_shadow_refill<S | 16, true, false> : k_shadow_refill<S | 16, false, false>;
        } else {
            if (lds) c.kernel = stats ? k_shadow<S, true, true> : k_shadow<S, false, true>;
            else c.kernel = stats ? k_shadow<S, true, false> : k_shadow<S, false, false>;
            c.sized_by = kernel_id(c.kernel);
        }
    });
    return c;
}
ShadeChoice choose_shade(bool full) {
    ShadeChoice c;
    c.kernel = full ? k_shade<true> : k_shade<false>;
    c.sized_by = kernel_id(c.kernel);
    return c;
}
#endif

#if IGX_PART == 5
InfoChoice choose_infobuffer(int v) {
    InfoChoice c;
    c.kernel = with_shading_variant(v, [](auto V) -> InfoKernel { return k_infobuffer<decltype(V)::value>; });
    c.sized_by = kernel_id(c.kernel); // its grids cover the film, no query
    return c;
}
#endif

// The shape of one k_extend launch: a pure function of the options and the
// launch's FrameArgs (pick_extend_shape, host/extend_shape.h)
inline ExtendShape launch_shape(const igx_device* dev, bool instrumented, const FrameArgs& fa, const PathBuf& pin, const PathBuf& out,
                                const ShadowBuf& sh, const KernelCounters& kc) {
    ExtendShapeInput in;
    in.extend_shapes = dev->extend_shapes_opt;
    in.instrument = instrumented;
    in.gen_n = fa.gen_n;
    in.dynamic = fa.dynamic;
    in.reverse = fa.reverse;
    in.classify = fa.classify;
    in.shadow_classes = fa.shadow_classes;
    in.num_rays = fa.num_rays;
    in.mis_aovs = fa.aov_di != nullptr || fa.aov_nee != nullptr;
    // the layout the shapes derive their pointers from (k_extend)
    // (stream_layout: the offsets k_extend adds to the first pointer of a stream)
    static_assert(EXTEND_SHARDS == NSH, "stream_layout counts NSH shards");
    const StreamLayout lay = stream_layout(out.shard_cap);
    const auto byte_off = [](const void* p, const void* base) {
        return (unsigned long long)(reinterpret_cast<const char*>(p) - reinterpret_cast<const char*>(base));
    };
    const auto packed = [&](const PathBuf& b) {
        return b.shard_cap == out.shard_cap && (unsigned long long)b.c_base == lay.shadow_records && byte_off(b.p1, b.p0) == lay.p_off[1] &&
               byte_off(b.p2, b.p0) == lay.p_off[2] && byte_off(b.p3, b.p0) == lay.p_off[3];
    };
    in.streams_packed = packed(pin) && packed(out) && sh.shard_cap == out.shard_cap && byte_off(sh.s1, sh.s0) == lay.s_off[1] &&
                        byte_off(sh.s2, sh.s0) == lay.s_off[2] && kc.cnt_shadow == kc.cnt_in + CROW && kc.cnt_out == kc.cnt_in + 2 * CROW;
    // and reach a record by a 32-bit byte offset from its array's base
    in.offsets_32bit = streams_offsets_32bit(out.shard_cap);
    return pick_extend_shape(in);
}

// Film post-processing (igx_post.h, part 6): tone curve arguments, the
// per-block partial results of the imageinfo passes (pass 1: one entry per
// POST_CHUNK pixels; pass 2: one per block of 3x3 windows) and the result
// k_info_final leaves in device memory (16 words, the histograms behind it)
struct PostTonemap {
    float scale;
    int method, use_gamma;
    float exposure_factor, exposure_offset;
};
struct PostSlab {
    float *mn, *mx, *sum;
    int *n_inf, *n_nan, *n_neg;
    float *smin, *smax, *med;
};
struct PostResult {
    float min, max, avg, soft_min, soft_max, median;
    int inf_count, nan_count, neg_count;
    float start, factor; // of the histograms
    int pad[5];
};
// histograms of more than this many bytes (4 * bins ints) count in global memory
[[maybe_unused]] constexpr size_t POST_HIST_LDS_MAX = 32 * 1024;
// queue k_tonemap on dev->stream: `pixels` RGB pixels of `film` to packed ARGB in `out` (both device memory)
void launch_tonemap(igx_device* dev, const float* film, size_t pixels, const PostTonemap& a, uint32_t* out);
// slab entries of the two imageinfo passes (pass 2: 0 unless w > 10 && h > 10)
int post_lum_blocks(size_t n);
int post_soft_blocks(int w, int h);
// queue the imageinfo passes on dev->stream; hist (4 * bins ints, zeroed on the stream before) may be nullptr
void launch_imageinfo(igx_device* dev, const float* film, int w, int h, float scale, bool stats, int bins, float* plane, const PostSlab& s,
                      PostResult* res, int* hist);
// Daylight glare (k_glare_scan): the camera on the film, the scale and the two
// luminance levels of glare_model.h; the slab holds the six per-block sums,
// one entry per POST_CHUNK pixels (6 * post_lum_blocks(n) words at `base`)
struct GlareArgs {
    CameraModel cam;
    int w, h;
    float scale, lum_source, lum_max;
};
struct GlareSlab {
    float *ev, *omega, *lum, *x, *y;
    int* n;
};
// queue k_glare_scan on dev->stream; overlay (device memory, a.w * a.h words) may be nullptr
void launch_glare(igx_device* dev, const float* film, const GlareArgs& a, float* slab, uint32_t* overlay);
// the slab copied to the host -> the output (block order, glare_finish)
igx_glare_output glare_finish_slab(float* slab_host, size_t blocks, const igx_glare_settings& set, const CameraModel& cam, int w, int h);
#if IGX_PART == 6
#include "igx_post.h"
#endif

// k_camera_rays (part 10) on dev->stream: `rays` takes 2 float4 per pixel of fa's film
void launch_camera_rays(igx_device* dev, int grid, const FrameArgs& fa, const SceneView& sv, float4* rays);
#if IGX_PART == 10
void launch_camera_rays(igx_device* dev, int grid, const FrameArgs& fa, const SceneView& sv, float4* rays) {
    hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(BLOCK), 0, dev->stream, fa, sv, rays);
}
#endif

#if IGX_PART == 0
// k_extend for the current LDS layout (configure_lds) and the launch's shape.
// The generate and bounce shapes share launch bounds and static LDS with the
// generic instantiation of their layout, so grids and the treelet are sized by
// the generic kernel's resident blocks.
ExtendChoice choose_extend(const igx_device* dev, bool stats, ExtendShape shape) {
    const int v = dev->variant;
    const bool shaped = shape != EXTEND_GENERIC, lds = dev->lds_scene_bytes != 0;
    ExtendChoice c;
    ExtendKernel generic;
    if (dev->ext_block == BLOCK_WIDE) {
        generic = extend_kernel_wide(v, stats);
        c.kernel = shaped ? extend_kernel_shaped_wide(v, shape) : generic;
        c.block = BLOCK_WIDE;
        c.dyn = lds_pad16(dev->lds_scene_bytes) + dev->lds_shading_bytes;
    } else if (lds) {
        generic = extend_kernel(v, stats, true);
        c.kernel = shaped ? extend_kernel_shaped_lds(v, shape) : generic;
        c.dyn = dev->lds_scene_bytes;
    } else {
        generic = extend_kernel(v, stats, false);
        c.kernel = shaped ? extend_kernel_shaped_global(v, shape) : generic;
        c.tree_n = dev->tree_ext;
        c.dyn = tree_bytes(dev, c.tree_n);
    }
    c.sized_by = kernel_id(generic);
    return c;
}

// resident blocks per CU of a kernel (persistent grid sizing)
int resident_blocks(const void* kernel, size_t dyn_lds, int block) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, dyn_lds) != hipSuccess || nb < 1) nb = 1;
    return nb;
}
int blocks_per_cu(const KernelChoice& c) { return resident_blocks(c.sized_by, c.dyn, c.block); }
// a block above 64 KB needs its kernel's dynamic-LDS limit raised
hipError_t raise_dynamic_lds(const void* kernel, size_t dyn) {
    // once per kernel instantiation and device (the caller's current one), the
    // limit only grows
    static std::map<std::pair<const void*, int>, size_t> raised;
    int d = 0;
    (void)hipGetDevice(&d);
    size_t& have = raised[{kernel, d}];
    if (dyn <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e == hipSuccess) have = dyn;
    return e;
}

void launch_extend(igx_device* dev, const LaunchCtx& ctx, Slot& s, int grid, bool stats, const FrameArgs& fa, const PathBuf& in,
                   const PathBuf& out, const KernelCounters& kc, int tail) {
    const ExtendShape shape = launch_shape(dev, stats, fa, in, out, s.sh, kc);
    if (shape != EXTEND_GENERIC) ++dev->stats.launches_extend_shaped[shape == EXTEND_GENERATE ? 0 : 1];
    const ExtendChoice c = choose_extend(dev, stats, shape);
    SceneView sv = launch_view(dev, ctx, ctx.spill_main);
    sv.tree_n = c.tree_n;
    hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, ctx.main, fa, sv, in, out, s.sh, s.L, kc, tail);
}
void launch_trace(igx_device* dev, const LaunchCtx& ctx, Slot& s, int grid, bool stats, const FrameArgs& fa, const PathBuf& in,
                  const int* cnt, int tail, int* work) {
    const TraceChoice c = choose_trace(dev, stats);
    const SceneView sv = launch_view(dev, ctx, ctx.spill_main);
    if (c.refill)
        hipLaunchKernelGGL(c.refill, dim3(grid), dim3(c.block), c.dyn, ctx.main, fa, sv, in, s.hb, cnt, tail, dev->dstats, refill_min(dev), work);
    else hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, ctx.main, fa, sv, in, s.hb, cnt, tail, dev->dstats);
}
void launch_shade(igx_device* dev, const LaunchCtx& ctx, bool full, int grid, const FrameArgs& fa, const PathBuf& in, const HitBuf& hb,
                  const PathBuf& out, const ShadowBuf& sh, float4* L, const KernelCounters& kc, int tail) {
    const ShadeChoice c = choose_shade(full);
    const SceneView sv = launch_view(dev, ctx, ctx.spill_main);
    hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, ctx.main, fa, sv, in, hb, out, sh, L, kc, tail);
}
void launch_shadow(igx_device* dev, const LaunchCtx& ctx, Slot& s, int grid, bool stats, const int* cnt, int* work) {
    const ShadowChoice c = choose_shadow(dev, stats);
    SceneView sv = launch_view(dev, ctx, ctx.spill_shadow); // its own columns where it overlaps the main stream's kernels
    sv.tree_n = c.tree_n;
    if (c.refill)
        hipLaunchKernelGGL(c.refill, dim3(grid), dim3(c.block), c.dyn, ctx.shadow, sv, s.sh, s.L, cnt, dev->dstats, refill_min(dev), work);
    else hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, ctx.shadow, sv, s.sh, s.L, cnt, dev->dstats, work);
}
void launch_finish(igx_device* dev, const LaunchCtx& ctx, Slot& s, int grid, bool stats, const FrameArgs& fa, const PathBuf& in,
                   const int* cnt, int tail) {
    const FinishChoice c = choose_finish(dev, stats);
    SceneView sv = launch_view(dev, ctx, ctx.spill_tail); // k_finish may run concurrently with the main stream's kernels
    sv.tree_n = c.tree_n;
    hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, ctx.tail, fa, sv, in, s.L, cnt, tail, dev->dstats, dev->tail_counts);
}
// the info-buffer pass (k_infobuffer) on `strm`, for the scene view `sv` (the
// caller's copy: its camera and the spill columns of that stream)
void launch_infobuffer(igx_device* dev, int grid, hipStream_t strm, const FrameArgs& fa, const SceneView& sv, const InfoArgs& ia) {
    const InfoChoice c = choose_infobuffer(dev->variant);
    hipLaunchKernelGGL(c.kernel, dim3(grid), dim3(c.block), c.dyn, strm, fa, sv, ia);
}

// k_generate on the main stream, with the camera models of the scene's shading variant
void launch_generate(igx_device* dev, const LaunchCtx& ctx, int grid, const FrameArgs& fa, const PathBuf& out, float4* L, int* cnt0) {
    const SceneView sv = launch_view(dev, ctx, ctx.spill_main);
    if (dev->full_shading) hipLaunchKernelGGL(k_generate_full, dim3(grid), dim3(BLOCK), 0, ctx.main, fa, sv, out, L, cnt0);
    else hipLaunchKernelGGL(k_generate, dim3(grid), dim3(BLOCK), 0, ctx.main, fa, sv, out, L, cnt0);
}

// Wait for the chunk last run in `s` and fold its statistics in.
igx_status harvest(igx_device* dev, Slot& s) {
    if (!s.pending) return IGX_OK;
    HIPCHK(hipEventSynchronize(s.done));
    auto c = [&](int r) { return (uint64_t)row_total(s, r); };
    dev->stats.camera_rays += (uint64_t)s.camera;
    for (int b = 1; b <= s.switch_bounce; ++b) dev->stats.bounce_rays += c(2 * b);
    for (int b = 0; b < s.switch_bounce; ++b) dev->stats.shadow_rays += c(2 * b + 1);
    for (int b = 0; b < s.switch_bounce; ++b) dev->stats.extend_rays += c(2 * b);
    for (int b = 1; b <= s.switch_bounce; ++b) dev->stats.extend_paths_out += c(2 * b);
    // every queued launch counts (as rocprofv3 sees them), including one that
    // found the live count at or below the tail threshold and exited at once
    dev->stats.launches_extend += (uint64_t)s.launched;
    dev->stats.launches_shadow += (uint64_t)s.launched;
    if (s.split) dev->stats.launches_trace += (uint64_t)s.launched;
    bool finished = s.switch_bounce < MAX_BOUNCES && c(2 * s.switch_bounce) > 0;
    dev->stats.launches_finish += finished ? 1 : 0;
    if (dev->timing) {
        for (auto& t : s.timed) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, t.a, t.b);
            if (t.kind == 0) dev->stats.ms_extend += ms;
            else if (t.kind == 1) dev->stats.ms_shadow += ms;
            else if (t.kind == 2) dev->stats.ms_generate += ms;
            else if (t.kind == 3) dev->stats.ms_resolve += ms;
            else if (t.kind == 4 && finished) dev->stats.ms_finish += ms;
            else if (t.kind == 5) dev->stats.ms_trace += ms;
        }
    }
    s.timed.clear();
    s.ev_next = 0;
    s.pending = false;
    return IGX_OK;
}

igx_status drain(igx_device* dev) {
    igx_status st;
    if ((st = ::wait_idle(dev)) || (st = harvest(dev, dev->slots[0])) || (st = harvest(dev, dev->slots[1]))) return st;
    HIPCHK(hipStreamSynchronize(dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream2));
    HIPCHK(hipStreamSynchronize(dev->shadow_stream));
    HIPCHK(hipStreamSynchronize(dev->tail_stream));
    for (auto& t : dev->info_timed) { // info-buffer passes (option "timing")
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.first, t.second) == hipSuccess) dev->stats.ms_generate += ms;
        (void)hipEventDestroy(t.first);
        (void)hipEventDestroy(t.second);
    }
    dev->info_timed.clear();
    unsigned long long tc[2] = {0, 0};
    HIPCHK(hipMemcpy(tc, dev->tail_counts, sizeof(tc), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(dev->tail_counts, 0, sizeof(tc)));
    dev->stats.bounce_rays += tc[0];
    dev->stats.shadow_rays += tc[1];
    dev->stats.tail_bounce_rays += tc[0];
    dev->stats.tail_shadow_rays += tc[1];
    return IGX_OK;
}

// k_extend's LDS layout for the current scene, decided at upload and when an
// option it depends on changes (plan_lds, host/lds_plan.h): today's
// BLOCK-thread kernel with the traversal tables staged (or global), or the
// wide block with the shading tables behind them when all of it fits the
// device's LDS per workgroup.  "lds_shading" -1 takes LDS_SHADING_AUTO.
#ifndef LDS_SHADING_AUTO
#define LDS_SHADING_AUTO 1
#endif
// k_extend's static LDS beside the stack: the enclosing boxes and the
// instrumented build's per-wave class counters (planned for either build)
constexpr size_t EXTEND_FIXED_LDS = 2 * MAX_ENC_BOXES * sizeof(float4) + BLOCK_WIDE / 64 * 36 * sizeof(unsigned long long);
void configure_lds(igx_device* dev) {
    dev->lds_scene_bytes = dev->lds_shading_bytes = 0;
    dev->ext_block = BLOCK;
    if (!dev->has_scene) return;
    LdsPlanInput in;
    in.traversal_bytes = dev->table_bytes;
    in.traversal_max = dev->lds_scene_max;
    for (int k = 0; k < LDS_TAB_COUNT; ++k) in.shading_bytes[k] = dev->lds_shading_tab[k];
    in.shading_max = dev->lds_shading_max;
    in.shading_on = dev->lds_shading_opt < 0 ? LDS_SHADING_AUTO != 0 : dev->lds_shading_opt != 0;
    in.stack_bytes_per_thread = LDS_STACK * sizeof(int);
    in.fixed_bytes = EXTEND_FIXED_LDS;
    in.lds_per_block = dev->lds_per_block;
    const LdsPlan p = plan_lds(in);
    dev->lds_scene_bytes = p.traversal_bytes;
    dev->lds_shading_bytes = p.shading_bytes;
    dev->ext_block = p.block_threads;
    if (dev->ext_block == BLOCK_WIDE) {
        // a block above 64 KB: raise the dynamic-LDS limit of the wide kernels
        // this layout can launch (generic plain and instrumented, generate,
        // bounce), stopping at the first refusal; a refusal keeps today's
        // layout; the text in last_error is advisory (the call that got here
        // still returns IGX_OK)
        (void)hipSetDevice(dev->hip_device);
        const std::pair<bool, ExtendShape> wide[] = {
            {false, EXTEND_GENERIC}, {true, EXTEND_GENERIC}, {false, EXTEND_GENERATE}, {false, EXTEND_BOUNCE}};
        hipError_t e = hipSuccess;
        for (const auto& [stats, shape] : wide) {
            if (e != hipSuccess) break;
            const ExtendChoice c = choose_extend(dev, stats, shape);
            e = raise_dynamic_lds(kernel_id(c.kernel), c.dyn);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            dev->last_error = std::string("lds_shading: the wide k_extend's LDS block was refused (") + hipGetErrorString(e) +
                              "); keeping the 256-thread layout";
            dev->ext_block = BLOCK;
            dev->lds_shading_bytes = 0;
        }
    }
}

// Treelet size of every global-table kernel: the largest prefix of the hot
// node order (order_hot_nodes) whose LDS copy keeps the kernel's resident
// blocks per CU (set by its register budget) -- the treelet takes LDS that
// would otherwise stay unused.  Binary search over hipOccupancy answers.
void configure_treelet(igx_device* dev) {
    dev->tree_ext = dev->tree_shadow = 0;
    dev->tree_dirty = false;
    if (!dev->has_scene || dev->lds_scene_bytes || dev->treelet_opt == 0) return;
    int cap = (int)std::min<size_t>(TREELET_FRONT, (size_t)dev->sv.num_nodes);
    if (dev->treelet_opt > 0) cap = (int)std::min<int64_t>(cap, dev->treelet_opt);
    // asked of the uninstrumented choice's grid-sizing kernel
    auto fit = [&](const KernelChoice& c) {
        const int nb0 = resident_blocks(c.sized_by, 0, c.block);
        int lo = 0, hi = cap;
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (resident_blocks(c.sized_by, tree_bytes(dev, mid), c.block) >= nb0) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    };
    if (EXTEND_TREELET) dev->tree_ext = fit(choose_extend(dev, false, EXTEND_GENERIC));
    // the if-if shadow kernel of the split schedule: global node loads beat a
    // treelet's flat loads there (profiles/r03_ab_treelet_global.log)
    if (SHADOW_TREELET && !(use_refill(dev) && use_shadow_ifif(dev))) dev->tree_shadow = fit(choose_shadow(dev, false));
    // k_trace_refill and the tail kernels: none -- the tail kernel overlaps the
    // next chunk's kernels, and LDS it holds keeps their blocks off the CU
    // (soup-1M frame +4 % with one)
}

CameraModel make_camera(const igx_device* dev, int width, int height) {
    return make_camera_model(dev->cam_desc, width, height); // host/camera_model.h
}

#endif // IGX_PART == 0

} // namespace

#if IGX_PART == 0
// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" const char* igx_version(void) { return "igx 0.2 (gfx950 wavefront path tracer)"; }

extern "C" igx_status igx_create(int hip_device, igx_device** out) {
    if (!out) return IGX_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    igx_device* dev = new igx_device();
    dev->hip_device = hip_device;
    hipError_t e = hipSetDevice(hip_device);
    if (e != hipSuccess) {
        delete dev;
        return IGX_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess) {
        dev->num_cus = prop.multiProcessorCount;
        dev->mem_total = prop.totalGlobalMem;
    }
    int lds_block = 0;
    if (hipDeviceGetAttribute(&lds_block, hipDeviceAttributeMaxSharedMemoryPerBlock, hip_device) == hipSuccess && lds_block > 0)
        dev->lds_per_block = (size_t)lds_block;
    if (hipStreamCreateWithFlags(&dev->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&dev->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&dev->tail_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&dev->shadow_stream, hipStreamNonBlocking) != hipSuccess) {
        delete dev;
        return IGX_ERR_HIP;
    }
    if (hipMalloc((void**)&dev->dstats, DSTATS * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&dev->tail_counts, 2 * sizeof(unsigned long long)) != hipSuccess) {
        delete dev;
        return IGX_ERR_OUT_OF_MEMORY;
    }
    (void)hipMemset(dev->dstats, 0, DSTATS * sizeof(unsigned long long));
    (void)hipMemset(dev->tail_counts, 0, 2 * sizeof(unsigned long long));
    *out = dev;
    return IGX_OK;
}

extern "C" igx_status igx_destroy(igx_device* dev) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(dev->hip_device);
    (void)wait_idle(dev);
    stop_async(dev);
    if (dev->stream) (void)hipStreamSynchronize(dev->stream);
    if (dev->stream2) (void)hipStreamSynchronize(dev->stream2);
    if (dev->tail_stream) (void)hipStreamSynchronize(dev->tail_stream);
    if (dev->shadow_stream) (void)hipStreamSynchronize(dev->shadow_stream);
    free_scene(dev);
    for (auto& s : dev->slots) {
        free_slot_buffers(s);
        if (s.ctr) (void)hipFree(s.ctr);
        if (s.pinned) (void)hipHostFree(s.pinned);
        if (s.done) (void)hipEventDestroy(s.done);
        for (auto& e : s.ev_pool) (void)hipEventDestroy(e);
    }
    if (dev->fb) (void)hipFree(dev->fb);
    for (float* a : dev->aov_fb)
        if (a) (void)hipFree(a);
    for (float* a : dev->info_fb)
        if (a) (void)hipFree(a);
    for (auto& t : dev->info_timed) {
        (void)hipEventDestroy(t.first);
        (void)hipEventDestroy(t.second);
    }
    if (dev->dstats) (void)hipFree(dev->dstats);
    if (dev->tail_counts) (void)hipFree(dev->tail_counts);
    if (dev->ray_list) (void)hipFree(dev->ray_list);
    for (void* b : dev->post_buf)
        if (b) (void)hipFree(b);
    if (dev->stream) (void)hipStreamDestroy(dev->stream);
    if (dev->stream2) (void)hipStreamDestroy(dev->stream2);
    if (dev->tail_stream) (void)hipStreamDestroy(dev->tail_stream);
    if (dev->shadow_stream) (void)hipStreamDestroy(dev->shadow_stream);
    delete dev;
    return IGX_OK;
}

extern "C" const char* igx_last_error(const igx_device* dev) { return dev ? dev->last_error.c_str() : "null device"; }

extern "C" igx_status igx_set_option(igx_device* dev, const char* key, int64_t value) {
    if (!dev || !key) return IGX_ERR_INVALID_ARGUMENT;
    // options change what queued work reads: let the worker drain first
    if (igx_status w = wait_idle(dev); w != IGX_OK) return w;
    std::string k(key);
    dev->tree_dirty = true; // schedule options change which kernels run, and so their treelets
    if (k == "timing") dev->timing = value != 0;
    else if (k == "instrument") dev->instrument = value != 0;
    else if (k == "capacity") dev->capacity_opt = value;
    else if (k == "treelet") {
        if (value < -1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "treelet must be -1 (auto), 0 (off) or a node count");
        dev->treelet_opt = value;
        dev->tree_dirty = true;
    }
    else if (k == "shadow_classes") dev->shadow_classes_opt = value != 0;
    else if (k == "overlap_shadow") dev->overlap_shadow_opt = value != 0;
    else if (k == "bvh_quantize") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "bvh_quantize must be -1 (auto), 0 or 1");
        dev->quantize_opt = (int)value;
    }
    else if (k == "tail_pairs") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "tail_pairs must be -1 (auto), 0 or 1");
        dev->tail_pairs_opt = (int)value;
    }
    else if (k == "stream_slots") {
        if (value != 1 && value != 2) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "stream_slots must be 1 or 2");
        if (value == 1 && dev->slots[1].cap) { // give the second slot's memory back
            igx_status st = harvest(dev, dev->slots[1]);
            if (st != IGX_OK) return st;
            free_slot_buffers(dev->slots[1]);
        }
        dev->stream_slots = (int)value;
    }
    else if (k == "slot_budget_mb") {
        if (value < 0) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "slot_budget_mb must be >= 0 (0 = auto)");
        dev->slot_budget_mb = value;
    }
    else if (k == "concurrent_chunks") dev->concurrent_opt = value != 0 ? 1 : 0;
    else if (k == "async_render") dev->async_opt = value != 0 ? 1 : 0;
    else if (k == "denoise_aovs") {
        if (value < INFO_OFF || value > INFO_EVERY)
            return fail(dev, IGX_ERR_INVALID_ARGUMENT, "denoise_aovs must be 0 (off), 1 (first iteration) or 2 (every iteration)");
        dev->info_mode = (int)value; // the films come and go at the next render
    }
    else if (k == "denoise_follow_specular") dev->info_follow_specular = value != 0;
    else if (k == "denoise_max_depth") {
        if (value < 0) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "denoise_max_depth must be >= 0");
        dev->info_max_depth = (int)std::min<int64_t>(value, 1 << 20);
    }
    else if (k == "probe_sample") dev->probe_sample_opt = std::max<int64_t>(0, value);
    else if (k == "fail_chunk") dev->fail_chunk_opt = std::max<int64_t>(0, value);
    else if (k == "face_shade") dev->face_shade_opt = value != 0 ? 1 : 0;
    else if (k == "host_wait_us") dev->host_wait_us = (int)std::max<int64_t>(0, std::min<int64_t>(value, 10000));
    else if (k == "concurrent_start_pct") {
        if (value < 0 || value > 100) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "concurrent_start_pct must be 0..100");
        dev->concurrent_start_pct = (int)value;
    }
    else if (k == "tail_threshold") dev->tail_opt = value;
    else if (k == "tail_threshold_last") dev->tail_last_opt = value;
    else if (k == "fuse_generate") dev->fuse_generate = value != 0;
    else if (k == "split") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "split must be -1 (auto), 0 or 1");
        dev->split_opt = (int)value;
    }
    else if (k == "shadow_ifif") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "shadow_ifif must be -1 (auto), 0 or 1");
        dev->shadow_ifif_opt = (int)value;
    }
    else if (k == "shadow_optimistic") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "shadow_optimistic must be -1 (auto), 0 or 1");
        dev->shadow_optimistic_opt = (int)value;
    }
    else if (k == "extend_shapes") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "extend_shapes must be -1 (auto), 0 or 1");
        dev->extend_shapes_opt = (int)value;
    }
    else if (k == "refill") {
        if (value < -1 || value > 64) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "refill must be -1 (auto) or in [0, 64]");
        dev->refill_opt = (int)value;
    }
    else if (k == "lds_scene_max") {
        dev->lds_scene_max = value;
        configure_lds(dev);
    }
    else if (k == "lds_shading") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "lds_shading must be -1 (auto), 0 or 1");
        dev->lds_shading_opt = (int)value;
        configure_lds(dev);
    }
    else if (k == "lds_shading_max") {
        dev->lds_shading_max = value;
        configure_lds(dev);
    }
    else if (k == "full_shading") dev->full_shading_opt = value != 0;
    else if (k == "enclosing") dev->enclosing_opt = value != 0;
    else if (k == "bvh_width") {
        if (value != 0 && value != 2 && value != 4) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "bvh_width must be 0 (auto), 2 or 4");
        dev->bvh_width_opt = (int)value;
    }
    else if (k == "spatial_splits") dev->spatial_splits = value != 0;
    else if (k == "rebuild_bvh") dev->rebuild_bvh = value != 0;
    else if (k == "dynamic") dev->dynamic_opt = (int)(value & 15);
    else if (k == "group_order") {
        if (value < -1 || value > 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "group_order must be -1 (auto), 0 (A, B, C) or 1 (C, B, A)");
        dev->group_order_opt = (int)value;
    }
    else if (k == "face_normals") dev->face_normals_opt = value != 0;
    else if (k == "bvh_bins") {
        if (value < 2 || value > 4096) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "bvh_bins must be in [2, 4096]");
        dev->bvh_bins = (int)value;
    }
    else if (k == "bvh_bins_tlas") {
        if (value < 2 || value > 4096) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "bvh_bins_tlas must be in [2, 4096]");
        dev->bvh_bins_tlas = (int)value;
    }
    else if (k == "path_classes") {
        if (value < 0 || value > 4) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "path_classes must be in [0, 4]");
        dev->classify_opt = (int)value;
    }
    else if (k == "sah_node_cost_pct") {
        if (value < 10 || value > 2000) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "sah_node_cost_pct must be in [10, 2000]");
        dev->sah_node_cost = (float)value / 100.0f;
    }
    else if (k == "bvh_leaf_size") {
        if (value < 1 || value > 16) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "bvh_leaf_size must be in [1, 16]");
        dev->leaf_size = (int)value;
    } else return fail(dev, IGX_ERR_INVALID_ARGUMENT, "unknown option '" + k + "'");
    return IGX_OK;
}

extern "C" igx_status igx_wait_ready(igx_device* dev) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    return wait_ready(dev);
}

extern "C" igx_status igx_synchronize(igx_device* dev) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    return drain(dev);
}

// The scene tables are built on the host (host/scene_tables.cpp, which also
// validates the description and picks node width, quantisation and shading
// variant); this copies them to the device and configures the handle.
extern "C" igx_status igx_upload_scene(igx_device* dev, const igx_scene_desc* desc) {
    if (!dev || !desc) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    reset_async_failure(dev); // a new scene starts the handle afresh
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    free_scene(dev);

    igx::SceneBuildOptions opt;
    opt.rebuild_bvh = dev->rebuild_bvh;
    opt.spatial_splits = dev->spatial_splits;
    opt.leaf_size = dev->leaf_size;
    opt.bvh_bins = dev->bvh_bins;
    opt.bvh_bins_tlas = dev->bvh_bins_tlas;
    opt.sah_node_cost = dev->sah_node_cost;
    opt.bvh_width_opt = dev->bvh_width_opt;
    opt.quantize_opt = dev->quantize_opt;
    opt.face_shade_opt = dev->face_shade_opt != 0;
    opt.face_normals_opt = dev->face_normals_opt != 0;
    opt.enclosing_opt = dev->enclosing_opt;
    opt.full_shading_opt = dev->full_shading_opt;
    igx::SceneTables t;
    std::string error;
    if ((st = igx::build_scene_tables(*desc, opt, t, error)) != IGX_OK) return fail(dev, st, error);

    SceneView sv{};
    if ((st = upload(dev, t.nodes, &sv.nodes)) || (st = upload(dev, t.tris, &sv.tris)) || (st = upload(dev, t.inst, &sv.inst)) ||
        (st = upload(dev, t.spheres, &sv.spheres)) || (st = upload(dev, t.ent, &sv.ent)) || (st = upload(dev, t.vtx, &sv.vtx)) ||
        (st = upload(dev, t.nrm, &sv.nrm)) || (st = upload(dev, t.idx, &sv.idx)) || (st = upload(dev, t.mats, &sv.mats)) ||
        (st = upload(dev, t.lights, &sv.lights)) || (st = upload(dev, t.lsel.cdf, &sv.sel_cdf)) ||
        (st = upload(dev, t.lsel.hierarchy, &sv.sel_tree)) || (st = upload(dev, t.ent_enc, &sv.ent_enc)) ||
        (st = upload(dev, t.enc_tab, &sv.enc)) || (st = upload(dev, t.enc_box, &sv.enc_box)) ||
        (st = upload(dev, t.ent_fn, &sv.ent_fn)) || (st = upload(dev, t.fn_tab, &sv.fn_tab)) || (st = upload(dev, t.uvs, &sv.uv)) ||
        (st = upload(dev, t.fsh, &sv.fsh))) {
        free_scene(dev);
        return st;
    }
    if (t.fn_tab.empty()) sv.fn_tab = nullptr; // surface_element computes the normals
    if (t.fsh.empty()) sv.fsh = nullptr;       // ... reads the index and normal tables
    if (t.uvs.empty()) sv.uv = nullptr;
    sv.tlas_root = t.tlas_root;
    sv.num_nodes = (int)(t.nodes.size() / t.nf4);
    sv.node_f4 = t.nf4;
    sv.num_inst = (int)(t.inst.size() / 4);
    sv.num_enc = (int)t.enc_tab.size();
    sv.num_tris = (int)(t.tris.size() / 3);
    sv.num_ent = (int)(t.ent.size() / ENT_STRIDE);
    sv.num_fsh = (int)(t.fsh.size() / 3);
    sv.num_fn = (int)t.fn_tab.size();
    sv.num_mats = (int)t.mats.size();
    sv.num_lights = (int)t.lights.size();
    sv.num_infinite = t.num_infinite;
    sv.selector = t.lsel.selector;
    sv.scene_radius = t.scene_radius;
    sv.max_depth = desc->technique.max_depth;
    sv.min_depth = desc->technique.min_depth;
    sv.nee = desc->technique.nee;
    sv.clamp = desc->technique.clamp;
    dev->sv = sv;
    dev->bvh_width = t.width;
    dev->quantized = t.quantized;
    dev->nf4 = t.nf4;
    // the LDS layout (stage_scene_lds) is the traversal tables back to back; configure_lds below
    dev->table_bytes = ((size_t)sv.num_nodes * t.nf4 + (size_t)sv.num_inst * 4 + (size_t)sv.num_tris * 3) * 16;
    dev->lds_shading_tab[LDS_TAB_ENT] = t.ent.size() * sizeof(t.ent[0]);
    dev->lds_shading_tab[LDS_TAB_FSH] = t.fsh.size() * sizeof(t.fsh[0]);
    dev->lds_shading_tab[LDS_TAB_FN] = t.fn_tab.size() * sizeof(t.fn_tab[0]);
    dev->lds_shading_tab[LDS_TAB_MATS] = t.mats.size() * sizeof(DevMaterial);
    dev->lds_shading_tab[LDS_TAB_LIGHTS] = t.lights.size() * sizeof(t.lights[0]);
    dev->lds_shading_tab[LDS_TAB_ENT_ENC] = t.ent_enc.size() * sizeof(t.ent_enc[0]);
    dev->shading_bytes = t.ent.size() * sizeof(t.ent[0]) + t.vtx.size() * sizeof(t.vtx[0]) + t.nrm.size() * sizeof(t.nrm[0]) +
                         t.idx.size() * sizeof(t.idx[0]) + t.mats.size() * sizeof(DevMaterial) +
                         t.lights.size() * sizeof(t.lights[0]) + t.fn_tab.size() * sizeof(t.fn_tab[0]) +
                         t.fsh.size() * sizeof(t.fsh[0]);
    dev->image_bytes = t.image_bytes;
    dev->cdf_bytes = t.cdf_bytes;
    dev->measured_bytes = t.measured_bytes;
    dev->cam_desc = desc->camera;
    dev->rays_w = desc->film_width;
    dev->rays_h = desc->film_height;
    dev->rays_frame = dev->rays_seed = 0;
    dev->aov_on = t.aov_on;
    dev->scene_depth = t.scene_depth;
    dev->full_shading = t.full_shading;
    if ((st = configure_stack(dev)) != IGX_OK) {
        free_scene(dev);
        return st;
    }
    dev->has_scene = true;
    dev->tree_dirty = true;
    configure_lds(dev); // after configure_stack: the wide k_extend is prepared for the scene's variant
    return IGX_OK;
}

// Concurrent chunks (option "concurrent_chunks", fused schedule with two
// stream slots).  The sequential schedule runs every chunk's bounces on the
// one main stream: chunk k + 1 starts only when chunk k's bounce loop has
// reached its tail threshold, so each chunk's last bounces -- a few hundred K
// long paths, a few hundred microseconds each at low occupancy -- run alone.
// Here slot k's chunk runs on its own stream (dev->stream / dev->stream2,
// spill columns spill_main / spill_main2), and one host thread advances both
// chunks' bounce loops as their lagged counts arrive (hipEventQuery, no
// blocking wait).  The next chunk starts once the running one is down to
// concurrent_start_pct % of its paths, so one chunk's late bounces share the
// GPU with the other's early ones.  The tail kernel runs on the chunk's own
// stream after its bounces; resolves (and framebuffer clears) go to the tail
// stream strictly in submission order, so the framebuffer sums every pixel's
// iterations in the sequential order: bit-identical images.
//
// Asynchronous rendering (option "async_render", on top of concurrent
// chunks): render and clear calls only queue their work for a per-handle
// worker thread that runs the same scheduler over consecutive calls, so the
// last chunk of frame k overlaps the first of frame k + 1 too (one chunk per
// frame on an 8-rank diamond share).  Every other call waits until the queue
// has drained (wait_idle).
struct ChunkPlan { // one render call: its chunking (host/render_plan.h) and what each of its chunks launches with
    RenderPlan rp;
    FrameArgs fa{}; // the call's; begin_chunk fills in the chunk's own fields
    CameraModel cam{};
    int iteration = 0; // the call's first iteration
    bool split = false, aov = false, full = false; // k_trace + k_shade; the MIS AOV slots; the full shading variant
    int max_bounces = 1, ext_bpc = 1, tr_bpc = 1, shade_bpc = 1, sh_bpc = 1, fin_bpc = 1;
    bool pairs = false;
};
struct ChunkRun { // one chunk from begin_chunk to queue_resolve
    FrameArgs fa{};
    long long n = 0; // paths
    int tail = 0, fin_grid = 0;
    bool fuse_gen = false;
    hipEvent_t sh_done = nullptr; // the last shadow launch on a shadow stream of its own
};
// One info-buffer pass (k_infobuffer): the iterations of one render call
struct InfoPass {
    FrameArgs fa{}; // spi 1, one chunk of every local pixel, chunk_iters = the call's iterations
    CameraModel cam{};
    InfoArgs ia{};
    int grid = 1;
};
// What a clear resets (igx_clear: everything; igx_clear_aov: one film):
// bit 0 the film, bit 1 + k the AOV with index k of host/aov_plan.h
constexpr uint32_t CLEAR_FILM = 1u, CLEAR_ALL = (2u << AOV_COUNT) - 1u;
constexpr uint32_t clear_bit(int aov) { return 2u << aov; }
struct SchedItem {
    bool clear = false;
    uint32_t clear_mask = CLEAR_ALL;
    // an info-buffer pass: like a clear, queued on the tail stream in submission order
    std::shared_ptr<const InfoPass> info;
    bool fence() const { return clear || info; } // no chunk of its own
    std::shared_ptr<const ChunkPlan> plan;
    Chunk c;
    bool started = false;
    int slot = 0;
    ChunkRun run;
    int b = 0, switch_b = -1;
    long long live = 0; // paths entering the last bounce whose count arrived
    bool loop_done = false, tail_queued = false;
    hipEvent_t fin_ev = nullptr;
};
struct ChunkScheduler {
    std::deque<SchedItem> items; // submission order
    bool empty() const { return items.empty(); }
    void add(const std::shared_ptr<const ChunkPlan>& plan) {
        for (long long k = 0, chunks = chunk_count(plan->rp); k < chunks; ++k) {
            SchedItem s;
            s.plan = plan;
            s.c = plan_chunk(plan->rp, k);
            items.push_back(s);
        }
    }
    void add_clear(uint32_t mask) {
        SchedItem s;
        s.clear = true;
        s.clear_mask = mask;
        items.push_back(s);
    }
    void add_info(const std::shared_ptr<const InfoPass>& pass) {
        SchedItem s;
        s.info = pass;
        items.push_back(s);
    }
    igx_status step(igx_device* dev, bool& progress);
    // every chunk has started and is down to concurrent_start_pct % of its paths (or done)
    bool all_late(int pct) const {
        for (const SchedItem& r : items) {
            if (r.fence()) continue;
            if (!r.started) return false;
            if (!r.loop_done && r.live * 100 > (long long)pct * r.c.n) return false;
        }
        return true;
    }
};
struct AsyncRender {
    std::thread th;
    std::mutex m;
    std::condition_variable cv, cv_idle;
    struct Job { // a clear (of `clear_mask`), an info-buffer pass, or a render call's plan
        bool clear = false;
        uint32_t clear_mask = CLEAR_ALL;
        std::shared_ptr<const InfoPass> info;
        std::shared_ptr<const ChunkPlan> plan;
    };
    std::deque<Job> jobs;
    bool stop = false, idle = true;
    bool late = true; // every chunk submitted has started and is in its late bounces (igx_wait_ready)
    // a step failed on the worker: everything queued was dropped, so the film
    // and the iteration count no longer agree.  The handle stays failed --
    // every call that waits for the queue returns `err` with `msg` as its last
    // error -- until igx_clear or igx_upload_scene (reset_async_failure)
    igx_status err = IGX_OK;
    std::string msg;
    ChunkScheduler sched; // the worker's
};

// Zero the films `mask` names (CLEAR_*), behind the work queued on `strm`.
static igx_status queue_clear(igx_device* dev, uint32_t mask, hipStream_t strm) {
    const size_t bytes = dev->fb_count * sizeof(float);
    if (dev->fb && (mask & CLEAR_FILM)) HIPCHK(hipMemsetAsync(dev->fb, 0, bytes, strm));
    for (int k = 0; k < AOV_MIS_COUNT; ++k)
        if (dev->aov_fb[k] && (mask & clear_bit(AOV_MIS_FIRST + k))) HIPCHK(hipMemsetAsync(dev->aov_fb[k], 0, bytes, strm));
    for (int k = 0; k < AOV_INFO_COUNT; ++k)
        if (dev->info_fb[k] && (mask & clear_bit(AOV_INFO_FIRST + k))) HIPCHK(hipMemsetAsync(dev->info_fb[k], 0, bytes, strm));
    return IGX_OK;
}

// Launch an info-buffer pass on `strm`, whose spill columns are `spill`.
static igx_status queue_info_pass(igx_device* dev, const InfoPass& ps, hipStream_t strm, int* spill) {
    SceneView sv = dev->sv;
    set_camera(sv, ps.cam);
    sv.spill = spill;
    hipEvent_t a = nullptr, b = nullptr;
    if (dev->timing) {
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, strm));
    }
    launch_infobuffer(dev, ps.grid, strm, ps.fa, sv, ps.ia);
    HIPCHK(hipGetLastError());
    if (b) {
        HIPCHK(hipEventRecord(b, strm));
        dev->info_timed.push_back({a, b});
    }
    return IGX_OK;
}

// ---------------------------------------------------------------------------
// The steps of one chunk, shared by the sequential schedule (render_impl) and
// the concurrent one (ChunkScheduler::step).  Each queues its work on the
// streams of `ctx` and waits for nothing but the slot's previous chunk
// (begin_chunk); when the host waits for counts is the schedules' business.
// ---------------------------------------------------------------------------
// option "timing": an event pair around the launches between the two calls
static void begin_timed(igx_device* dev, Slot& S, int kind, int bounce, hipStream_t strm) {
    if (!dev->timing) return;
    TimedLaunch t{slot_event(S), slot_event(S), kind, bounce};
    (void)hipEventRecord(t.a, strm);
    S.timed.push_back(t);
}
static void end_timed(igx_device* dev, Slot& S, hipStream_t strm) {
    if (!dev->timing) return;
    (void)hipEventRecord(S.timed.back().b, strm);
}
// counter row r of the slot: row 2b = paths entering bounce b, row 2b+1 = shadow rays of bounce b
static int* ctr_row(const Slot& S, int r) { return S.ctr + (size_t)r * CROW; }

// Chunk `c` of the plan moves into slot S: waits for (and harvests) the chunk
// that last ran there, sizes the slot, fills in the chunk's FrameArgs and
// tail threshold, zeroes the counter rows and generates the camera paths
// unless bounce 0 of the fused k_extend will.
static igx_status begin_chunk(igx_device* dev, const LaunchCtx& ctx, Slot& S, const ChunkPlan& pl, const Chunk& c, ChunkRun& r) {
    igx_status st = harvest(dev, S);
    if (st != IGX_OK || (st = ensure_slot(dev, S, pl.rp.slot_cap, pl.split, pl.fa.classify >= 4, pl.aov)) != IGX_OK) return st;
    r = ChunkRun{};
    r.fa = pl.fa;
    // the slot keeps AOV buffers from an earlier aov_mis scene: only a scene
    // with the AOVs (and their films) writes them
    r.fa.aov_di = pl.aov && dev->aov_fb[0] ? S.aov_di : nullptr;
    r.fa.aov_nee = pl.aov && dev->aov_fb[1] ? S.aov_nee : nullptr;
    S.sh.aov_nee = r.fa.aov_nee;
    S.sh.optimistic = r.fa.shadow_optimistic;
    r.fa.iter = pl.iteration + c.it0;
    r.fa.chunk_iters = c.chunk_iters;
    r.fa.chunk_pixel0 = (int)c.px0;
    r.fa.chunk_pixels = c.chunk_pixels;
    r.n = c.n;
    // paths one pass of the tail kernel holds (lane pairs: one path per two lanes)
    const long long fin_lanes = (long long)pl.fin_bpc * dev->num_cus * BLOCK / (pl.pairs ? 2 : 1);
    r.tail = tail_threshold(r.n, fin_lanes, dev->tail_opt, dev->tail_last_opt, c.last);
    S.tail = r.tail;
    const FrameArgs& fa = r.fa;
    const TileShare share{fa.width, fa.height, fa.num_rays, fa.tile_size, fa.tile_offset, fa.tile_stride, fa.tiles_x};
    S.camera = valid_pixels_in_chunk(share, fa.chunk_pixel0, fa.chunk_pixels) * pl.rp.spi * fa.chunk_iters;
    S.n0 = r.n;
    S.split = pl.split;
    S.bounce_ev.clear();
    S.launched = 0;
    r.fin_grid = grid_for(dev, std::min<long long>(r.n, r.tail) * (pl.pairs ? 2 : 1), pl.fin_bpc);
    // camera paths: built by bounce 0 of the fused k_extend when the chunk
    // runs through it (saves the 72 B/path round trip of k_generate)
    r.fuse_gen = dev->fuse_generate && !pl.split && r.n > r.tail;
    HIPCHK(hipMemsetAsync(S.ctr, 0, (size_t)(2 * pl.max_bounces + 4) * CROW * sizeof(int), ctx.main));
    if (dev->dynamic_opt)
        HIPCHK(hipMemsetAsync(S.ctr + (size_t)WORK_ROW0 * CROW, 0, (size_t)4 * pl.max_bounces * CROW * sizeof(int), ctx.main));
    if (!r.fuse_gen) {
        begin_timed(dev, S, 2, -1, ctx.main);
        launch_generate(dev, ctx, grid_for(dev, r.n, 8), r.fa, S.pa, S.L, S.ctr);
        end_timed(dev, S, ctx.main);
        HIPCHK(hipGetLastError());
    }
    return IGX_OK;
}

// Bounce b of the chunk: the fused k_extend, or k_trace + k_shade, then the
// shadow kernel, the copy of the bounce's counts to the host mirror and the
// event behind it (S.bounce_ev[b]).  `bound`: the paths known to remain (the
// count entering bounce b - 1 once it has arrived, an upper bound for bounce
// b's paths and shadow rays): late bounces launch few waves, not a full chip
// of waves that find no group (IGX_LIVE_GRID).
// Split schedule with a shadow stream of its own (ctx.shadow): the shadow rays
// of bounce b overlap the trace of bounce b + 1 (independent: both come from
// shade(b)); shade(b + 1) waits for them, as both add to the radiance slots,
// so the additions keep their order and the image is unchanged.
static igx_status queue_bounce(igx_device* dev, const LaunchCtx& ctx, Slot& S, const ChunkPlan& pl, ChunkRun& r, int b, long long bound) {
    const bool inst = dev->instrument;
    const bool overlap = ctx.shadow != ctx.main;
    const int sh_grid = grid_for(dev, bound, pl.sh_bpc);
    PathBuf in = (b & 1) ? S.pb : S.pa, out = (b & 1) ? S.pa : S.pb;
    KernelCounters kc{ctr_row(S, 2 * b), ctr_row(S, 2 * (b + 1)), ctr_row(S, 2 * b + 1), dev->dstats, ctr_row(S, WORK_ROW0 + 4 * b)};
    if (pl.split) {
        const int tr_grid = grid_for(dev, bound, pl.tr_bpc), shade_grid = grid_for(dev, bound, pl.shade_bpc);
        begin_timed(dev, S, 5, b, ctx.main);
        int* const tr_work = (dev->dynamic_opt & DYN_REFILL_TRACE) ? ctr_row(S, WORK_ROW0 + 4 * b) : nullptr;
        launch_trace(dev, ctx, S, tr_grid, inst, r.fa, in, ctr_row(S, 2 * b), r.tail, tr_work);
        end_timed(dev, S, ctx.main);
        if (r.sh_done) HIPCHK(hipStreamWaitEvent(ctx.main, r.sh_done, 0));
        begin_timed(dev, S, 0, b, ctx.main);
        launch_shade(dev, ctx, pl.full, shade_grid, r.fa, in, S.hb, out, S.sh, S.L, kc, r.tail);
        end_timed(dev, S, ctx.main);
    } else {
        const int ext_grid = grid_for(dev, bound, pl.ext_bpc, dev->ext_block);
        begin_timed(dev, S, 0, b, ctx.main);
        FrameArgs fb = r.fa;
        fb.gen_n = r.fuse_gen && b == 0 ? (int)r.n : 0;
        launch_extend(dev, ctx, S, ext_grid, inst, fb, in, out, kc, r.tail);
        end_timed(dev, S, ctx.main);
    }
    if (overlap) {
        hipEvent_t shaded = slot_event(S);
        HIPCHK(hipEventRecord(shaded, ctx.main));
        HIPCHK(hipStreamWaitEvent(ctx.shadow, shaded, 0));
    }
    begin_timed(dev, S, 1, b, ctx.shadow);
    int* const sh_work =
        (dev->dynamic_opt & (use_refill(dev) ? DYN_REFILL_SHADOW : DYN_SHADOW)) ? ctr_row(S, WORK_ROW0 + 4 * b + 2) : nullptr;
    launch_shadow(dev, ctx, S, sh_grid, inst, ctr_row(S, 2 * b + 1), sh_work);
    end_timed(dev, S, ctx.shadow);
    if (overlap) {
        r.sh_done = slot_event(S);
        HIPCHK(hipEventRecord(r.sh_done, ctx.shadow));
    }
    HIPCHK(hipGetLastError());
    // shadow counts of bounce b and path counts entering bounce b+1 (adjacent rows)
    HIPCHK(hipMemcpyAsync(S.pinned + (size_t)(2 * b + 1) * CROW, ctr_row(S, 2 * b + 1), 2 * CROW * sizeof(int), hipMemcpyDeviceToHost,
                          ctx.main));
    hipEvent_t e = slot_event(S);
    HIPCHK(hipEventRecord(e, ctx.main));
    S.bounce_ev.push_back(e);
    ++S.launched;
    return IGX_OK;
}

// Every bounce is queued and its counts have arrived: the first bounce whose
// paths are at or below the tail threshold
static int find_switch_bounce(const Slot& S, int max_bounces, int tail) {
    for (int b = 1; b <= max_bounces; ++b)
        if (row_total(S, 2 * b) <= tail) return b;
    return max_bounces;
}

// The tail kernel takes the paths entering bounce switch_b to their end (ctx.tail)
static igx_status queue_tail(igx_device* dev, const LaunchCtx& ctx, Slot& S, const ChunkRun& r, int switch_b) {
    S.switch_bounce = switch_b;
    if (switch_b >= MAX_BOUNCES) return IGX_OK;
    PathBuf in = (switch_b & 1) ? S.pb : S.pa;
    begin_timed(dev, S, 4, switch_b, ctx.tail);
    launch_finish(dev, ctx, S, r.fin_grid, dev->instrument, r.fa, in, ctr_row(S, 2 * switch_b), r.tail);
    end_timed(dev, S, ctx.tail);
    HIPCHK(hipGetLastError());
    return IGX_OK;
}

// The chunk's radiance slots go to the film (and the MIS AOVs', resolved like
// it, to theirs) on `strm`; S.done marks the slot free again
static igx_status queue_resolve(igx_device* dev, Slot& S, const ChunkRun& r, int fb_width, hipStream_t strm) {
    const dim3 grid((r.fa.chunk_pixels + 63) / 64), block(64 * RES_G);
    begin_timed(dev, S, 3, -1, strm);
    hipLaunchKernelGGL(k_resolve, grid, block, 0, strm, r.fa, S.L, dev->fb, fb_width);
    if (r.fa.aov_di)
        for (int k = 0; k < 2; ++k) hipLaunchKernelGGL(k_resolve, grid, block, 0, strm, r.fa, k ? S.aov_nee : S.aov_di, dev->aov_fb[k], fb_width);
    end_timed(dev, S, strm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.done, strm));
    S.pending = true;
    return IGX_OK;
}

igx_status ChunkScheduler::step(igx_device* dev, bool& progress) {
    // slot k's chunk runs on a stream of its own, tail kernel included, with
    // that stream's spill columns (the fused schedule: no shadow stream)
    const auto slot_ctx = [&](const SchedItem& r) {
        hipStream_t const strm = r.slot ? dev->stream2 : dev->stream;
        int* const spill = r.slot ? dev->spill_main2 : dev->spill_main;
        return LaunchCtx{strm, strm, strm, spill, spill, spill, r.plan->cam};
    };
    igx_status st;
    // start the next chunk once its slot's previous chunk has resolved and
    // every running chunk is in its late bounces (live paths at most
    // concurrent_start_pct % of its own): two chunks started together only
    // contend for the chip in their heavy early bounces
    SchedItem* nx = nullptr;
    bool late = true;
    for (SchedItem& r : items) {
        if (r.fence()) continue;
        if (!r.started) {
            nx = &r;
            break;
        }
        if (!r.loop_done && r.live * 100 > (long long)dev->concurrent_start_pct * r.c.n) late = false;
    }
    if (nx && late) {
        const int k = dev->stream_slots == 1 ? 0 : dev->next_slot;
        Slot& S = dev->slots[k];
        bool busy = false;
        for (const SchedItem& r : items) busy = busy || (!r.fence() && r.started && r.slot == k);
        if (!busy && S.pending) {
            const hipError_t q = hipEventQuery(S.done);
            if (q == hipErrorNotReady) busy = true;
            else HIPCHK(q);
        }
        if (!busy) {
            SchedItem& r = *nx;
            if (dev->fail_chunk_opt > 0 && --dev->fail_chunk_opt == 0) // test hook (option "fail_chunk")
                return fail(dev, IGX_ERR_HIP, "injected failure (option fail_chunk)");
            r.slot = k;
            if ((st = begin_chunk(dev, slot_ctx(r), S, *r.plan, r.c, r.run)) != IGX_OK) return st;
            if (dev->stream_slots == 2) dev->next_slot ^= 1;
            r.started = true;
            r.live = r.run.n;
            if (r.run.n <= r.run.tail) { // the whole chunk is one tail pass
                r.switch_b = 0;
                r.loop_done = true;
            }
            progress = true;
        }
    }
    // advance every chunk's bounce loop as far as its lagged counts allow
    for (SchedItem& r : items) {
        if (r.fence() || !r.started || r.tail_queued) continue;
        Slot& S = dev->slots[r.slot];
        const ChunkPlan& pl = *r.plan;
        const LaunchCtx ctx = slot_ctx(r);
        while (!r.loop_done) {
            if (r.b >= pl.max_bounces) {
                // every bounce queued: the counts are known once the last one completed
                const hipError_t q = hipEventQuery(S.bounce_ev.back());
                if (q == hipErrorNotReady) break;
                HIPCHK(q);
                r.switch_b = find_switch_bounce(S, pl.max_bounces, r.run.tail);
                r.loop_done = true;
                break;
            }
            if (r.b >= 2) {
                const hipError_t q = hipEventQuery(S.bounce_ev[r.b - 2]);
                if (q == hipErrorNotReady) break;
                HIPCHK(q);
                r.live = row_total(S, 2 * (r.b - 1));
                if (r.live <= r.run.tail) {
                    r.switch_b = r.b - 1;
                    r.loop_done = true;
                    break;
                }
            }
            if ((st = queue_bounce(dev, ctx, S, pl, r.run, r.b, IGX_LIVE_GRID && r.b >= 2 ? r.live : r.run.n)) != IGX_OK) return st;
            ++r.b;
            progress = true;
        }
        if (r.loop_done) {
            if ((st = queue_tail(dev, ctx, S, r.run, r.switch_b)) != IGX_OK) return st;
            r.fin_ev = slot_event(S);
            HIPCHK(hipEventRecord(r.fin_ev, ctx.main));
            r.tail_queued = true;
            progress = true;
        }
    }
    // resolves, framebuffer clears and info-buffer passes strictly in submission order on the tail stream
    while (!items.empty() && (items.front().fence() || items.front().tail_queued)) {
        SchedItem& r = items.front();
        if (r.clear) st = queue_clear(dev, r.clear_mask, dev->tail_stream);
        else if (r.info) st = queue_info_pass(dev, *r.info, dev->tail_stream, dev->spill_tail);
        else {
            HIPCHK(hipStreamWaitEvent(dev->tail_stream, r.fin_ev, 0));
            st = queue_resolve(dev, dev->slots[r.slot], r.run, r.plan->rp.width, dev->tail_stream);
        }
        if (st != IGX_OK) return st;
        items.pop_front();
        progress = true;
    }
    return IGX_OK;
}

// The scheduler's host thread between steps that made no progress (every
// chunk waits on a lagged count): a few yields, then sleeps of host_wait_us,
// so a busy handle does not hold a CPU core at 100 % polling events (ADVICE
// r4).  The lag of two bounces keeps the GPU fed across one sleep.
// host_wait_us 0: yield only (the round-4 behaviour).
struct Backoff {
    int idle = 0;
    void wait(const igx_device* dev) {
        if (dev->host_wait_us <= 0 || idle < 8) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(dev->host_wait_us));
        ++idle;
    }
    void reset() { idle = 0; }
};

// Runs the scheduler in the calling thread until everything queued is resolved.
static igx_status run_scheduler(igx_device* dev, ChunkScheduler& sched) {
    Backoff bo;
    while (!sched.empty()) {
        bool progress = false;
        igx_status st = sched.step(dev, progress);
        if (st != IGX_OK) {
            sched.items.clear();
            return st;
        }
        if (progress) bo.reset();
        else bo.wait(dev);
    }
    return IGX_OK;
}

static void async_worker(igx_device* dev) {
    AsyncRender& a = *dev->async;
    (void)hipSetDevice(dev->hip_device);
    std::string worker_msg;
    t_error_sink = &worker_msg; // fail() on this thread: the handle's last_error is the host thread's
    Backoff bo;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(a.m);
            while (!a.jobs.empty()) {
                const AsyncRender::Job& j = a.jobs.front();
                if (j.clear) a.sched.add_clear(j.clear_mask);
                else if (j.info) a.sched.add_info(j.info);
                else a.sched.add(j.plan);
                a.jobs.pop_front();
            }
            if (a.sched.empty()) {
                a.idle = true;
                a.cv_idle.notify_all();
                if (a.stop) return;
                a.cv.wait(lk, [&] { return a.stop || !a.jobs.empty(); });
                if (a.jobs.empty() && a.stop) return;
                a.idle = false;
                continue;
            }
        }
        bool progress = false;
        igx_status st = a.sched.step(dev, progress);
        if (st != IGX_OK) {
            // drop everything queued (a chunk may be half rendered into the
            // film) and mark the handle failed until a clear or upload
            std::lock_guard<std::mutex> lk(a.m);
            a.sched.items.clear();
            a.jobs.clear();
            if (a.err == IGX_OK) {
                a.err = st;
                a.msg = "async render: " + worker_msg;
            }
            continue;
        }
        if (progress) {
            bo.reset();
            const bool late = a.sched.all_late(dev->concurrent_start_pct);
            std::lock_guard<std::mutex> lk(a.m);
            a.late = late && a.jobs.empty();
            if (a.late) a.cv_idle.notify_all();
        } else {
            bo.wait(dev);
        }
    }
}

// Waits until every chunk submitted has started and is in its late bounces
// (down to concurrent_start_pct % of its paths), the point from which work on
// another handle of the same GPU overlaps it without slowing its heavy
// bounces (bench.py: frame k + 1 on the other handle); or until the queue has
// drained.  No-op without a worker.
igx_status wait_ready(igx_device* dev) {
    if (!dev->async) return IGX_OK;
    AsyncRender& a = *dev->async;
    std::unique_lock<std::mutex> lk(a.m);
    a.cv_idle.wait(lk, [&] { return (a.idle && a.jobs.empty()) || (a.late && a.jobs.empty()); });
    if (a.err != IGX_OK) dev->last_error = a.msg;
    return a.err;
}

// Waits until the worker has queued (on the GPU) everything submitted and
// returns its error, if it failed: the failure stays until igx_clear or
// igx_upload_scene.  No-op without a worker.
igx_status wait_idle(igx_device* dev) {
    if (!dev->async) return IGX_OK;
    AsyncRender& a = *dev->async;
    std::unique_lock<std::mutex> lk(a.m);
    a.cv_idle.wait(lk, [&] { return a.idle && a.jobs.empty(); });
    if (a.err != IGX_OK) dev->last_error = a.msg;
    return a.err;
}

// igx_clear / igx_upload_scene on a failed handle: wait until the worker is
// idle and lift the failure (the caller then resets the film or the scene).
// Returns whether the handle had failed.
bool reset_async_failure(igx_device* dev) {
    if (!dev->async) return false;
    AsyncRender& a = *dev->async;
    std::unique_lock<std::mutex> lk(a.m);
    a.cv_idle.wait(lk, [&] { return a.idle && a.jobs.empty(); });
    const bool failed = a.err != IGX_OK;
    a.err = IGX_OK;
    a.msg.clear();
    return failed;
}

void stop_async(igx_device* dev) {
    if (!dev->async) return;
    {
        std::lock_guard<std::mutex> lk(dev->async->m);
        dev->async->stop = true;
    }
    dev->async->cv.notify_all();
    if (dev->async->th.joinable()) dev->async->th.join();
    delete dev->async;
    dev->async = nullptr;
}

static void submit_async(igx_device* dev, AsyncRender::Job job) {
    if (!dev->async) {
        dev->async = new AsyncRender();
        dev->async->th = std::thread(async_worker, dev);
    }
    {
        std::lock_guard<std::mutex> lk(dev->async->m);
        dev->async->jobs.push_back(std::move(job));
        dev->async->idle = false;
        dev->async->late = false;
    }
    dev->async->cv.notify_all();
}

// Render `count` consecutive iterations (p->iteration, p->iteration + 1, ...).
// Small iterations are batched: one chunk then holds several iterations'
// paths (up to the path capacity), so a shard with few pixels (multi-GPU
// tiles) still fills the device; the film is bit-identical to `count`
// single-iteration calls.
static igx_status render_impl(igx_device* dev, const igx_render_params* p, int count) {
    if (!dev || !p || count < 1) return IGX_ERR_INVALID_ARGUMENT;
    if (!dev->has_scene) return fail(dev, IGX_ERR_NO_SCENE, "no scene uploaded");
    auto t_start = std::chrono::steady_clock::now();
    // schedule: concurrent chunks on the fused schedule with two slots, queued
    // for the handle's worker thread when async_render is on; anything else
    // runs here once the worker has drained
    const bool list_mode = p->num_rays > 0;
    const bool split = use_split(dev);
    const bool conc = !list_mode && !split && dev->concurrent_opt;
    const bool async = conc && dev->async_opt;
    const bool want_aov = dev->aov_on && !list_mode;
    // the call's share of the film and its chunking (host/render_plan.h)
    ChunkPlan plan;
    const RenderPlan& rp = plan.rp = plan_render(RenderPlanInput{
        p->width, p->height, p->num_rays, p->tile_size, p->tile_offset, p->tile_stride, p->spi, count, dev->capacity_opt,
        dev->slot_budget_mb, dev->stream_slots, dev->mem_total, dev->classify_opt, split, want_aov});
    if (rp.status != IGX_OK) return fail(dev, rp.status, rp.error);
    HIPCHK(hipSetDevice(dev->hip_device));
    const int width = rp.width, height = rp.height;
    if (!async) {
        igx_status w = wait_idle(dev);
        if (w != IGX_OK) return w;
    } else if (dev->async) { // a failed handle takes no more work until a clear or upload
        std::lock_guard<std::mutex> lk(dev->async->m);
        if (dev->async->err != IGX_OK) {
            dev->last_error = dev->async->msg;
            return dev->async->err;
        }
    }

    // framebuffer (resize clears, as Device::resize)
    size_t fbc = (size_t)width * height * 3;
    const bool resize = dev->fb_w != width || dev->fb_h != height || !dev->fb || want_aov != (dev->aov_fb[0] != nullptr);
    // the denoiser's three films come and go with option "denoise_aovs"; a
    // resize clears them (and their counts) with the film
    const bool want_info = dev->info_mode != INFO_OFF;
    if (resize || want_info != (dev->info_fb[0] != nullptr)) {
        igx_status dst = drain(dev);
        if (dst != IGX_OK) return dst;
        for (int k = 0; k < AOV_INFO_COUNT; ++k) {
            if (dev->info_fb[k]) HIPCHK(hipFree(dev->info_fb[k]));
            dev->info_fb[k] = nullptr;
            dev->info_count[k] = 0;
            if (want_info) {
                HIPCHK(hipMalloc((void**)&dev->info_fb[k], fbc * sizeof(float)));
                HIPCHK(hipMemsetAsync(dev->info_fb[k], 0, fbc * sizeof(float), dev->tail_stream));
            }
        }
    }
    if (resize) {
        igx_status dst = drain(dev);
        if (dst != IGX_OK) return dst;
        if (dev->fb) HIPCHK(hipFree(dev->fb));
        dev->fb = nullptr;
        for (float*& a : dev->aov_fb) {
            if (a) HIPCHK(hipFree(a));
            a = nullptr;
        }
        HIPCHK(hipMalloc((void**)&dev->fb, fbc * sizeof(float)));
        HIPCHK(hipMemsetAsync(dev->fb, 0, fbc * sizeof(float), dev->tail_stream));
        if (want_aov)
            for (float*& a : dev->aov_fb) {
                HIPCHK(hipMalloc((void**)&a, fbc * sizeof(float)));
                HIPCHK(hipMemsetAsync(a, 0, fbc * sizeof(float), dev->tail_stream));
            }
        dev->fb_w = width;
        dev->fb_h = height;
        dev->fb_count = fbc;
        dev->iteration_count = 0;
    }
    if (!list_mode) {
        dev->rays_w = width;
        dev->rays_h = height;
        dev->rays_frame = p->frame;
        dev->rays_seed = p->seed;
    }
    const CameraModel cam = plan.cam = make_camera(dev, width, height);

    FrameArgs& fa = plan.fa;
    fa.width = width;
    fa.height = height;
    fa.spi = p->spi;
    fa.iter = p->iteration;
    fa.frame = p->frame;
    fa.seed = p->seed;
    fa.inv_spi = 1.0f / (float)p->spi;
    fa.classify = dev->classify_opt;
    fa.shadow_classes = dev->shadow_classes_opt;
    fa.shadow_optimistic = use_shadow_optimistic(dev, split, want_aov);
    fa.dynamic = dev->dynamic_opt & DYN_EXTEND;
    fa.reverse = fa.dynamic ? (dev->group_order_opt < 0 ? GROUP_ORDER_AUTO : dev->group_order_opt) : 0;
    fa.probe_sample = dev->probe_sample_opt > 0 && dev->probe_sample_opt <= p->spi ? (int)dev->probe_sample_opt : 0;
    if (list_mode) {
        // the previous ray list may still be read by a queued tail kernel
        igx_status dst = drain(dev);
        if (dst != IGX_OK) return dst;
        size_t need = (size_t)p->num_rays * 8;
        if (dev->ray_list_cap < need) {
            if (dev->ray_list) HIPCHK(hipFree(dev->ray_list));
            HIPCHK(hipMalloc((void**)&dev->ray_list, need * sizeof(float)));
            dev->ray_list_cap = need;
        }
        HIPCHK(hipMemcpy(dev->ray_list, p->rays, need * sizeof(float), hipMemcpyHostToDevice));
        fa.num_rays = p->num_rays;
        fa.rays = dev->ray_list;
    } else if (p->tile_size > 0) {
        fa.tile_size = p->tile_size;
        fa.tile_offset = p->tile_offset;
        fa.tile_stride = p->tile_stride;
        fa.tiles_x = rp.tiles_x;
    }
    // The denoiser's info-buffer pass of the iterations that get one
    // (InfoBufferTechnique.cpp:56-66), ahead of their chunks as the reference
    // injects it: one launch, queued in call order where clears and resolves
    // are (the tail stream; with async_render by the worker, like a clear).
    if (const int64_t passes = info_passes_in(dev->info_mode, p->iteration, count); passes > 0 && dev->info_fb[0]) {
        for (uint64_t& c : dev->info_count) c += (uint64_t)passes;
        if (rp.local_pixels > 0) {
            auto pass = std::make_shared<InfoPass>();
            pass->fa = fa;
            pass->fa.spi = 1;
            pass->fa.inv_spi = 1.0f;
            pass->fa.probe_sample = 0;
            pass->fa.chunk_pixel0 = 0;
            pass->fa.chunk_pixels = (int)rp.local_pixels;
            pass->fa.chunk_iters = count;
            pass->cam = cam;
            pass->ia = InfoArgs{dev->info_fb[0], dev->info_fb[1], dev->info_fb[2], width,
                                dev->info_mode,  dev->info_follow_specular ? 1 : 0, dev->info_max_depth};
            pass->grid = grid_for(dev, rp.local_pixels, MAX_BLOCKS_PER_CU);
            if (async) {
                AsyncRender::Job job;
                job.info = std::move(pass);
                submit_async(dev, std::move(job));
            } else {
                igx_status st = queue_info_pass(dev, *pass, dev->tail_stream, dev->spill_tail);
                if (st != IGX_OK) return st;
            }
        }
    }
    if (rp.total_paths == 0) {
        dev->iteration_count += count;
        return IGX_OK;
    }
    fa.classify = rp.classify; // the split schedule has no class-C region

    plan.iteration = p->iteration;
    plan.split = split;
    plan.aov = want_aov;
    plan.max_bounces = std::min(std::max(dev->sv.max_depth, 1), MAX_BOUNCES - 1);
    const bool inst = dev->instrument;
    if (dev->tree_dirty) configure_treelet(dev);
    plan.ext_bpc = blocks_per_cu(choose_extend(dev, inst, EXTEND_GENERIC));
    plan.tr_bpc = blocks_per_cu(choose_trace(dev, inst));
    plan.full = variant_full(dev->variant);
    plan.shade_bpc = blocks_per_cu(choose_shade(plan.full));
    plan.sh_bpc = blocks_per_cu(choose_shadow(dev, inst));
    plan.pairs = use_tail_pairs(dev);
    plan.fin_bpc = blocks_per_cu(choose_finish(dev, inst));

    if (conc) {
        dev->iteration_count += count;
        dev->stats.iterations += count;
        const auto shared = std::make_shared<const ChunkPlan>(plan);
        if (async) {
            AsyncRender::Job job;
            job.plan = shared;
            submit_async(dev, std::move(job));
        } else {
            ChunkScheduler sched;
            sched.add(shared);
            igx_status st = run_scheduler(dev, sched);
            if (st != IGX_OK) return st;
        }
    } else {
        // Sequential schedule: every chunk's bounces on the main stream, the
        // slots alternating.  The host learns counts two bounces late (async
        // copies, no per-bounce sync); the device gates k_extend off once the
        // count is <= tail, and the host then queues k_finish for that
        // bounce's buffer and the resolve on the tail stream and moves on.
        const bool overlap = split && dev->overlap_shadow_opt; // shadow kernels on a stream of their own (queue_bounce)
        const LaunchCtx ctx{dev->stream,     dev->tail_stream, overlap ? dev->shadow_stream : dev->stream,
                            dev->spill_main, dev->spill_tail,  overlap ? dev->spill_shadow : dev->spill_main, cam};
        for (long long k = 0, chunks = chunk_count(rp); k < chunks; ++k) {
            const Chunk c = plan_chunk(rp, k);
            Slot& S = dev->slots[dev->stream_slots == 1 ? 0 : dev->next_slot];
            dev->next_slot ^= 1;
            ChunkRun r;
            igx_status st = begin_chunk(dev, ctx, S, plan, c, r); // waits for the chunk two chunks ago (one, with one slot)
            if (st != IGX_OK) return st;
            int switch_b = r.n <= r.tail ? 0 : -1;
            for (int b = 0; switch_b < 0 && b < plan.max_bounces; ++b) {
                long long bound = r.n; // paths known to remain
                if (b >= 2) {
                    HIPCHK(hipEventSynchronize(S.bounce_ev[b - 2]));
                    bound = row_total(S, 2 * (b - 1));
                    if (bound <= r.tail) {
                        switch_b = b - 1;
                        break;
                    }
                }
                if (!IGX_LIVE_GRID) bound = r.n;
                if ((st = queue_bounce(dev, ctx, S, plan, r, b, bound)) != IGX_OK) return st;
            }
            if (switch_b < 0) { // max_bounces launched: drain the lagged counts
                HIPCHK(hipStreamSynchronize(ctx.main));
                switch_b = find_switch_bounce(S, plan.max_bounces, r.tail);
            }
            // tail + resolve on the tail stream, after the main stream (and the
            // shadow stream's last launch) reached this point
            if (r.sh_done) HIPCHK(hipStreamWaitEvent(ctx.main, r.sh_done, 0));
            hipEvent_t reach = slot_event(S);
            HIPCHK(hipEventRecord(reach, ctx.main));
            HIPCHK(hipStreamWaitEvent(ctx.tail, reach, 0));
            if ((st = queue_tail(dev, ctx, S, r, switch_b)) != IGX_OK || (st = queue_resolve(dev, S, r, width, ctx.tail)) != IGX_OK) return st;
        }
        dev->iteration_count += count;
        dev->stats.iterations += count;
    }
    dev->stats.ms_render += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return IGX_OK;
}

extern "C" igx_status igx_set_camera(igx_device* dev, const igx_camera* camera) {
    if (!dev || !camera) return IGX_ERR_INVALID_ARGUMENT;
    // the basic shading variant compiles the pinhole perspective camera only
    if (dev->has_scene && !dev->full_shading && camera_needs_full(*camera))
        return fail(dev, IGX_ERR_UNSUPPORTED, "this camera needs the full shading variant: upload the scene with it, or with option full_shading");
    // queued chunks read the camera from their kernel arguments: no drain needed
    dev->cam_desc = *camera;
    return IGX_OK;
}

extern "C" igx_status igx_camera_rays(igx_device* dev, int32_t iteration, int32_t sample, float* rays8, int32_t device_out) {
    if (!dev || !rays8 || sample < 0) return IGX_ERR_INVALID_ARGUMENT;
    if (!dev->has_scene) return fail(dev, IGX_ERR_NO_SCENE, "no scene uploaded");
    const int w = dev->rays_w, h = dev->rays_h;
    if (w < 1 || h < 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "no film size for camera rays");
    // the kernel numbers (pixel, sample) as a path slot: pixel * (sample + 1) + sample
    if ((long long)w * h * ((long long)sample + 1) > (1ll << 30)) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "film size times sample index too large for camera rays");
    if (device_out && (reinterpret_cast<uintptr_t>(rays8) & 15)) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "device ray buffer must be 16-byte aligned");
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    const size_t bytes = (size_t)w * h * 8 * sizeof(float);
    float4* d_rays = reinterpret_cast<float4*>(rays8);
    if (!device_out) HIPCHK(hipMalloc((void**)&d_rays, bytes));
    FrameArgs fa{};
    fa.width = w;
    fa.height = h;
    fa.spi = sample + 1;
    fa.chunk_pixels = w * h;
    fa.chunk_iters = 1;
    fa.iter = iteration;
    fa.frame = dev->rays_frame;
    fa.seed = dev->rays_seed;
    SceneView sv = dev->sv;
    set_camera(sv, make_camera(dev, w, h));
    launch_camera_rays(dev, grid_for(dev, (long long)w * h, MAX_BLOCKS_PER_CU), fa, sv, d_rays);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e == hipSuccess && !device_out) e = hipMemcpy(rays8, d_rays, bytes, hipMemcpyDeviceToHost);
    if (!device_out) (void)hipFree(d_rays);
    HIPCHK(e);
    return IGX_OK;
}

extern "C" igx_status igx_render(igx_device* dev, const igx_render_params* p) { return render_impl(dev, p, 1); }

extern "C" igx_status igx_render_iterations(igx_device* dev, const igx_render_params* p, int32_t count) {
    if (count < 1) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "iteration count must be >= 1");
    return render_impl(dev, p, count);
}

extern "C" igx_status igx_get_framebuffer(igx_device* dev, float* host_rgb, size_t count, uint64_t* iteration_count) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    if (iteration_count) *iteration_count = dev->iteration_count;
    if (!host_rgb) return IGX_OK;
    if (!dev->fb) {
        std::memset(host_rgb, 0, count * sizeof(float));
        return IGX_OK;
    }
    if (count != dev->fb_count) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "framebuffer size mismatch: expected " + std::to_string(dev->fb_count));
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    HIPCHK(hipMemcpy(host_rgb, dev->fb, count * sizeof(float), hipMemcpyDeviceToHost));
    return IGX_OK;
}

// the path tracer's AOVs (Device::getFramebufferForHost(name), Device.cpp:1330-1363):
// "Color" (or "" / NULL) is the film; "Direct Weights" and "NEE Weights" exist
// with the technique's aov_mis (PathTechnique.cpp:23-27); any other name is an
// unknown AOV (the reference logs it and returns no data)
// and with the denoiser (option "denoise_aovs") "Normals", "Albedo" and "Depth"
// (InfoBufferTechnique.cpp:28-30).  The table: host/aov_plan.h.
static int aov_index(igx_device* dev, const char* name) { return aov_lookup(name, dev->aov_on, dev->info_mode != INFO_OFF); }
// the film of AOV k >= 0 (nullptr before the first render with it) and its
// iteration count: the info AOVs count their own passes, the MIS AOVs
// accumulate with the film
static float* aov_film(igx_device* dev, int k) { return k >= AOV_INFO_FIRST ? dev->info_fb[k - AOV_INFO_FIRST] : dev->aov_fb[k]; }
static uint64_t aov_count(igx_device* dev, int k) { return k >= AOV_INFO_FIRST ? dev->info_count[k - AOV_INFO_FIRST] : dev->iteration_count; }

extern "C" igx_status igx_get_aov(igx_device* dev, const char* name, float* host_rgb, size_t count, uint64_t* iteration_count) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    const int k = aov_index(dev, name);
    if (k == -1) return igx_get_framebuffer(dev, host_rgb, count, iteration_count);
    if (k == -2) return fail(dev, IGX_ERR_INVALID_ARGUMENT, std::string("unknown aov '") + (name ? name : "") + "'");
    if (iteration_count) *iteration_count = aov_count(dev, k);
    if (!host_rgb) return IGX_OK;
    if (!aov_film(dev, k)) {
        std::memset(host_rgb, 0, count * sizeof(float));
        return IGX_OK;
    }
    if (count != dev->fb_count) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "aov size mismatch: expected " + std::to_string(dev->fb_count));
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    HIPCHK(hipMemcpy(host_rgb, aov_film(dev, k), count * sizeof(float), hipMemcpyDeviceToHost));
    return IGX_OK;
}

extern "C" igx_status igx_aov_device_ptr(igx_device* dev, const char* name, float** ptr, size_t* count) {
    if (!dev || !ptr) return IGX_ERR_INVALID_ARGUMENT;
    const int k = aov_index(dev, name);
    if (k == -1) return igx_framebuffer_device_ptr(dev, ptr, count);
    if (k == -2) return fail(dev, IGX_ERR_INVALID_ARGUMENT, std::string("unknown aov '") + (name ? name : "") + "'");
    *ptr = aov_film(dev, k);
    if (count) *count = *ptr ? dev->fb_count : 0;
    return IGX_OK;
}

extern "C" igx_status igx_aov_iteration_count(igx_device* dev, const char* name, uint64_t* iteration_count) {
    if (!dev || !iteration_count) return IGX_ERR_INVALID_ARGUMENT;
    const int k = aov_index(dev, name);
    if (k == AOV_UNKNOWN) return fail(dev, IGX_ERR_INVALID_ARGUMENT, std::string("unknown aov '") + (name ? name : "") + "'");
    *iteration_count = k == AOV_COLOR ? dev->iteration_count : aov_count(dev, k);
    return IGX_OK;
}

extern "C" igx_status igx_framebuffer_device_ptr(igx_device* dev, float** ptr, size_t* count) {
    if (!dev || !ptr) return IGX_ERR_INVALID_ARGUMENT;
    *ptr = dev->fb;
    if (count) *count = dev->fb_count;
    return IGX_OK;
}

// ---------------------------------------------------------------------------
// Film post-processing (Device::tonemap / Device::imageinfo, Device.cpp:1662-1759)
// ---------------------------------------------------------------------------
enum { POST_PLANE = 0, POST_SLAB = 1, POST_RESULT = 2, POST_PIXELS = 3 };
// the handle's scratch buffer `which`, at least `bytes` large (the stream is idle: every post call ends in a wait)
static igx_status post_reserve(igx_device* dev, int which, size_t bytes) {
    if (dev->post_cap[which] >= bytes) return IGX_OK;
    if (dev->post_buf[which]) HIPCHK(hipFree(dev->post_buf[which]));
    dev->post_buf[which] = nullptr;
    dev->post_cap[which] = 0;
    HIPCHK(hipMalloc(&dev->post_buf[which], bytes));
    dev->post_cap[which] = bytes;
    return IGX_OK;
}

// the queue is drained; film: pixels RGB floats in device memory
static igx_status tonemap_run(igx_device* dev, const float* film, size_t pixels, float scale, const igx_tonemap_settings* ts,
                              uint32_t* out, bool out_on_device) {
    uint32_t* dst = out;
    if (!out_on_device) {
        igx_status st = post_reserve(dev, POST_PIXELS, pixels * sizeof(uint32_t));
        if (st != IGX_OK) return st;
        dst = (uint32_t*)dev->post_buf[POST_PIXELS];
    }
    const PostTonemap a{scale, ts->method, ts->use_gamma ? 1 : 0, ts->exposure_factor, ts->exposure_offset};
    launch_tonemap(dev, film, pixels, a, dst);
    HIPCHK(hipGetLastError());
    if (!out_on_device) HIPCHK(hipMemcpyAsync(out, dst, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    return IGX_OK;
}

static igx_status imageinfo_run(igx_device* dev, const float* film, int w, int h, float scale, const igx_imageinfo_settings* is,
                                igx_imageinfo_output* out) {
    const size_t n = (size_t)w * h;
    int32_t* host_hist[4] = {is->histogram_r, is->histogram_g, is->histogram_b, is->histogram_l};
    const bool want_hist = is->acquire_histogram && is->bins > 0 && (host_hist[0] || host_hist[1] || host_hist[2] || host_hist[3]);
    const size_t bins = want_hist ? (size_t)is->bins : 0;
    const size_t b1 = (size_t)post_lum_blocks(n), b2 = (size_t)post_soft_blocks(w, h);
    const size_t result_words = sizeof(PostResult) / sizeof(int) + 4 * bins;
    igx_status st;
    if ((st = post_reserve(dev, POST_PLANE, n * sizeof(float))) || (st = post_reserve(dev, POST_SLAB, (6 * b1 + 3 * b2 + 1) * sizeof(float))) ||
        (st = post_reserve(dev, POST_RESULT, result_words * sizeof(int))))
        return st;
    float* sf = (float*)dev->post_buf[POST_SLAB];
    PostSlab s;
    s.mn = sf, s.mx = sf + b1, s.sum = sf + 2 * b1;
    s.n_inf = (int*)(sf + 3 * b1), s.n_nan = (int*)(sf + 4 * b1), s.n_neg = (int*)(sf + 5 * b1);
    s.smin = sf + 6 * b1, s.smax = sf + 6 * b1 + b2, s.med = sf + 6 * b1 + 2 * b2;
    PostResult* res = (PostResult*)dev->post_buf[POST_RESULT];
    int* hist = want_hist ? (int*)(res + 1) : nullptr;
    HIPCHK(hipMemsetAsync(res, 0, result_words * sizeof(int), dev->stream));
    launch_imageinfo(dev, film, w, h, scale, is->acquire_error_stats != 0, (int)is->bins, (float*)dev->post_buf[POST_PLANE], s, res, hist);
    HIPCHK(hipGetLastError());
    std::vector<int> back(result_words);
    HIPCHK(hipMemcpyAsync(back.data(), res, result_words * sizeof(int), hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    PostResult r;
    std::memcpy(&r, back.data(), sizeof(r));
    *out = igx_imageinfo_output{r.min, r.max, r.avg, r.soft_min, r.soft_max, r.median, r.inf_count, r.nan_count, r.neg_count};
    for (int c = 0; c < 4 && want_hist; ++c)
        if (host_hist[c]) std::memcpy(host_hist[c], back.data() + sizeof(PostResult) / sizeof(int) + c * bins, bins * sizeof(int));
    return IGX_OK;
}

// resolves `name` to the handle's film (nullptr before the first render with
// it) and the scale of one iteration (Device.cpp:1668,1675), after a drain
static igx_status post_named_film(igx_device* dev, const char* name, float scale, const float** film, float* film_scale) {
    const int k = aov_index(dev, name);
    if (k == AOV_UNKNOWN) return fail(dev, IGX_ERR_INVALID_ARGUMENT, std::string("unknown aov '") + (name ? name : "") + "'");
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    *film = k == AOV_COLOR ? dev->fb : aov_film(dev, k);
    const uint64_t iters = k == AOV_COLOR ? dev->iteration_count : aov_count(dev, k);
    *film_scale = scale * (iters > 0 ? 1.0f / (float)iters : 0.0f);
    return IGX_OK;
}

extern "C" igx_status igx_tonemap(igx_device* dev, const char* aov, const igx_tonemap_settings* ts, uint32_t* out_host, size_t pixel_count) {
    if (!dev || !ts || !out_host || pixel_count == 0) return IGX_ERR_INVALID_ARGUMENT;
    const float* film = nullptr;
    float scale = 0;
    igx_status st = post_named_film(dev, aov, ts->scale, &film, &scale);
    if (st != IGX_OK || !film) return st;
    if (pixel_count * 3 != dev->fb_count)
        return fail(dev, IGX_ERR_INVALID_ARGUMENT, "tonemap size mismatch: expected " + std::to_string(dev->fb_count / 3) + " pixels");
    return tonemap_run(dev, film, pixel_count, scale, ts, out_host, false);
}

extern "C" igx_status igx_imageinfo(igx_device* dev, const char* aov, const igx_imageinfo_settings* is, igx_imageinfo_output* out) {
    if (!dev || !is || !out || is->bins < 0) return IGX_ERR_INVALID_ARGUMENT;
    const float* film = nullptr;
    float scale = 0;
    igx_status st = post_named_film(dev, aov, is->scale, &film, &scale);
    if (st != IGX_OK) return st;
    if (!film) {
        *out = igx_imageinfo_output{0, 0, 0, 0, 0, 0, 0, 0, 0};
        return IGX_OK;
    }
    return imageinfo_run(dev, film, dev->fb_w, dev->fb_h, scale, is, out);
}

extern "C" igx_status igx_tonemap_film(igx_device* dev, const float* film_dev, int32_t width, int32_t height, const igx_tonemap_settings* ts,
                                       uint32_t* out_pixels, int32_t out_on_device) {
    if (!dev || !film_dev || !ts || !out_pixels || width <= 0 || height <= 0) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    return tonemap_run(dev, film_dev, (size_t)width * height, ts->scale, ts, out_pixels, out_on_device != 0);
}

extern "C" igx_status igx_imageinfo_film(igx_device* dev, const float* film_dev, int32_t width, int32_t height,
                                         const igx_imageinfo_settings* is, igx_imageinfo_output* out) {
    if (!dev || !film_dev || !is || !out || is->bins < 0 || width <= 0 || height <= 0) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    return imageinfo_run(dev, film_dev, width, height, is->scale, is, out);
}

// Device::evaluateGlare (Device.cpp:1689-1723).  The queue is drained; film:
// w * h RGB floats in device memory.  One k_glare_scan, then the slab (and a
// host overlay's image) comes back and the tail runs on the host.  A host
// overlay keeps the words of the pixels at or below the threshold: the kernel
// writes into a zeroed device image, whose non-zero words (alpha is 255) are
// merged into the caller's buffer.
static igx_status glare_run(igx_device* dev, const float* film, int w, int h, float scale, const igx_glare_settings* gs, uint32_t* overlay,
                            bool overlay_on_device, igx_glare_output* out) {
    const igx_camera& c = dev->cam_desc;
    if (c.dir[0] == 0 && c.dir[1] == 0 && c.dir[2] == 0)
        return fail(dev, IGX_ERR_NO_SCENE, "evaluate_glare needs a camera: upload a scene or call igx_set_camera");
    const size_t n = (size_t)w * h, blocks = (size_t)post_lum_blocks(n);
    igx_glare_settings set = *gs;
    set.scale = scale;
    GlareArgs a{};
    a.cam = make_camera(dev, w, h);
    a.w = w;
    a.h = h;
    a.scale = scale;
    a.lum_source = igx::glare_lum_source(set);
    a.lum_max = igx::glare_lum_max(set);
    igx_status st = post_reserve(dev, POST_SLAB, igx::GLARE_SUMS * blocks * sizeof(float));
    if (st != IGX_OK) return st;
    uint32_t* dst = overlay;
    if (overlay && !overlay_on_device) {
        if ((st = post_reserve(dev, POST_PIXELS, n * sizeof(uint32_t))) != IGX_OK) return st;
        dst = (uint32_t*)dev->post_buf[POST_PIXELS];
        HIPCHK(hipMemsetAsync(dst, 0, n * sizeof(uint32_t), dev->stream));
    }
    float* slab = (float*)dev->post_buf[POST_SLAB];
    launch_glare(dev, film, a, slab, dst);
    HIPCHK(hipGetLastError());
    std::vector<float> back(igx::GLARE_SUMS * blocks);
    std::vector<uint32_t> image(overlay && !overlay_on_device ? n : 0);
    HIPCHK(hipMemcpyAsync(back.data(), slab, back.size() * sizeof(float), hipMemcpyDeviceToHost, dev->stream));
    if (!image.empty()) HIPCHK(hipMemcpyAsync(image.data(), dst, n * sizeof(uint32_t), hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    *out = glare_finish_slab(back.data(), blocks, set, a.cam, w, h);
    for (size_t i = 0; i < image.size(); ++i)
        if (image[i]) overlay[i] = image[i];
    return IGX_OK;
}

extern "C" igx_status igx_evaluate_glare(igx_device* dev, const char* aov, const igx_glare_settings* gs, uint32_t* overlay_host,
                                         size_t pixel_count, igx_glare_output* out) {
    if (!dev || !gs || !out) return IGX_ERR_INVALID_ARGUMENT;
    const float* film = nullptr;
    float scale = 0;
    igx_status st = post_named_film(dev, aov, gs->scale, &film, &scale);
    if (st != IGX_OK) return st;
    if (!film) {
        *out = igx_glare_output{0, 0, 0, 0, 0};
        return IGX_OK;
    }
    if (pixel_count * 3 != dev->fb_count)
        return fail(dev, IGX_ERR_INVALID_ARGUMENT, "evaluate_glare size mismatch: expected " + std::to_string(dev->fb_count / 3) + " pixels");
    return glare_run(dev, film, dev->fb_w, dev->fb_h, scale, gs, overlay_host, false, out);
}

extern "C" igx_status igx_evaluate_glare_film(igx_device* dev, const float* film_dev, int32_t width, int32_t height,
                                              const igx_glare_settings* gs, uint32_t* overlay, int32_t overlay_on_device,
                                              igx_glare_output* out) {
    if (!dev || !film_dev || !gs || !out || width <= 0 || height <= 0) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    return glare_run(dev, film_dev, width, height, gs->scale, gs, overlay, overlay_on_device != 0, out);
}

extern "C" igx_status igx_pack_tiles(igx_device* dev, const igx_render_params* p, float* dst, size_t count) {
    if (!dev || !p || !dst || p->tile_size <= 0) return IGX_ERR_INVALID_ARGUMENT;
    if (!dev->fb) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "no framebuffer");
    if (p->width != dev->fb_w || p->height != dev->fb_h || p->tile_stride <= 0 || p->tile_offset < 0)
        return fail(dev, IGX_ERR_INVALID_ARGUMENT,
                    "pack_tiles: film " + std::to_string(p->width) + "x" + std::to_string(p->height) +
                        " does not match the framebuffer " + std::to_string(dev->fb_w) + "x" + std::to_string(dev->fb_h) +
                        " (or invalid tile offset / stride)");
    FrameArgs fa{};
    fa.width = p->width;
    fa.height = p->height;
    fa.tile_size = p->tile_size;
    fa.tile_offset = p->tile_offset;
    fa.tile_stride = p->tile_stride;
    fa.tiles_x = (p->width + p->tile_size - 1) / p->tile_size;
    int tiles_y = (p->height + p->tile_size - 1) / p->tile_size;
    int tiles = fa.tiles_x * tiles_y;
    int mine = tiles > p->tile_offset ? (tiles - p->tile_offset + p->tile_stride - 1) / p->tile_stride : 0;
    size_t need = (size_t)mine * p->tile_size * p->tile_size * 3;
    if (count < need) return fail(dev, IGX_ERR_INVALID_ARGUMENT, "pack buffer too small, need " + std::to_string(need));
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    hipLaunchKernelGGL(k_pack_tiles, dim3(1024), dim3(256), 0, dev->stream, fa, dev->fb, dst, mine);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(dev->stream));
    return IGX_OK;
}

// Clears the films of `mask` (CLEAR_*) and their iteration counts: queued
// behind the renders submitted so far, like them without waiting.
static igx_status clear_impl(igx_device* dev, uint32_t mask) {
    auto reset_counts = [&]() {
        if (mask & CLEAR_FILM) dev->iteration_count = 0;
        for (int k = 0; k < AOV_INFO_COUNT; ++k)
            if (mask & clear_bit(AOV_INFO_FIRST + k)) dev->info_count[k] = 0;
    };
    bool failed = false;
    if (dev->async) {
        {
            std::lock_guard<std::mutex> lk(dev->async->m);
            failed = dev->async->err != IGX_OK;
        }
        if (!failed) { // ordered behind the queued renders' resolves by the worker
            AsyncRender::Job job;
            job.clear = true;
            job.clear_mask = mask;
            submit_async(dev, std::move(job));
            reset_counts();
            return IGX_OK;
        }
        // a failed handle: the worker dropped its queue; clear here and lift the
        // failure (only a clear of everything does: one film's clear leaves the
        // others out of step with their counts, so it reports the failure)
        if (mask != CLEAR_ALL) {
            std::lock_guard<std::mutex> lk(dev->async->m);
            dev->last_error = dev->async->msg;
            return dev->async->err;
        }
        reset_async_failure(dev);
        igx_status st = drain(dev);
        if (st != IGX_OK) return st;
    }
    if (dev->fb) {
        HIPCHK(hipSetDevice(dev->hip_device));
        // resolves of queued chunks land on the tail stream; clear behind them
        igx_status st = queue_clear(dev, mask, dev->tail_stream);
        if (st != IGX_OK) return st;
    }
    reset_counts();
    return IGX_OK;
}

extern "C" igx_status igx_clear(igx_device* dev) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    return clear_impl(dev, CLEAR_ALL);
}

extern "C" igx_status igx_clear_aov(igx_device* dev, const char* name) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    const int k = aov_index(dev, name);
    if (k == AOV_UNKNOWN) return fail(dev, IGX_ERR_INVALID_ARGUMENT, std::string("unknown aov '") + (name ? name : "") + "'");
    return clear_impl(dev, k == AOV_COLOR ? CLEAR_FILM : clear_bit(k));
}

extern "C" igx_status igx_get_stats(igx_device* dev, igx_stats* out) {
    if (!dev || !out) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    *out = dev->stats;
    out->bvh_depth = dev->scene_depth;
    out->stack_entries = LDS_STACK;
    unsigned long long h[DSTATS] = {0};
    HIPCHK(hipMemcpy(h, dev->dstats, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k) {
        out->shadow_class_groups[k] = h[40 + k];
        out->shadow_class_node_iters[k] = h[42 + k];
        out->shadow_class_node_visits[k] = h[44 + k];
        out->shadow_class_cycles[k] = h[46 + k];
        out->shadow_class_occluded[k] = h[48 + k];
        out->shadow_class_rays[k] = h[70 + k];
    }
    for (int k = 0; k < 16; ++k) out->extend_class_shade_cycles[k] = h[54 + k];
    out->tlas_node_visits = h[50];
    for (int k = 0; k < 3; ++k) out->hot_node_visits[k] = h[51 + k];
    for (int k = 0; k < 8; ++k) out->extend_class_cycles[k] = h[20 + k];
    for (int k = 0; k < 4; ++k) {
        out->extend_class_groups[k] = h[28 + k];
        out->extend_class_node_iters[k] = h[32 + k];
        out->extend_class_node_visits[k] = h[36 + k];
    }
    out->extend_cycles_load = h[16];
    out->extend_cycles_trace = h[17];
    out->extend_cycles_shade = h[18];
    out->extend_cycles_store = h[19];
    out->node_visits = h[0];
    out->leaf_visits = h[1];
    out->tri_tests = h[2];
    out->blas_enters = h[3];
    out->shadow_node_visits = h[4];
    out->shadow_leaf_visits = h[5];
    out->shadow_tri_tests = h[6];
    out->shadow_blas_enters = h[7];
    out->shaded_hits = h[8];
    out->wave_node_iters = h[9];
    out->wave_leaf_iters = h[10];
    out->shadow_wave_node_iters = h[11];
    out->shadow_wave_leaf_iters = h[12];
    out->bvh_width = dev->bvh_width;
    out->node_bytes = dev->nf4 * 16;
    out->lds_scene_bytes = (int32_t)dev->lds_scene_bytes;
    out->lds_shading_bytes = (int32_t)dev->lds_shading_bytes;
    out->extend_block_threads = dev->ext_block;
    if (dev->has_scene && dev->tree_dirty) configure_treelet(dev);
    out->shadow_blocks_per_cu = dev->has_scene ? blocks_per_cu(choose_shadow(dev, false)) : 0;
    out->treelet_nodes[0] = dev->tree_ext;
    out->treelet_nodes[1] = 0; // k_trace_refill: no treelet
    out->treelet_nodes[2] = dev->tree_shadow;
    out->treelet_nodes[3] = 0; // tail kernels: no treelet
    out->table_bytes = dev->table_bytes;
    out->shading_bytes = dev->shading_bytes;
    out->image_bytes = dev->image_bytes;
    out->cdf_bytes = dev->cdf_bytes;
    out->measured_bytes = dev->measured_bytes;
    out->slot_bytes = 0;
    for (const Slot& s : dev->slots)
        out->slot_bytes += (uint64_t)s.shard_cap * NSH * (2 * 56 * (s.pa.c_base ? 2 : 1) + 48 + (s.hb.h ? 20 : 0)) +
                           (uint64_t)s.cap * (16 + (s.aov_di ? 32 : 0));
    return IGX_OK;
}

extern "C" igx_status igx_get_store_split(igx_device* dev, uint64_t out[4]) {
    if (!dev || !out) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    unsigned long long h[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(h, dev->dstats + 72, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) out[k] = h[k];
    return IGX_OK;
}

extern "C" igx_status igx_reset_stats(igx_device* dev) {
    if (!dev) return IGX_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    dev->stats = igx_stats{};
    HIPCHK(hipMemset(dev->dstats, 0, DSTATS * sizeof(unsigned long long)));
    return IGX_OK;
}

static igx_status trace_batch(igx_device* dev, const float* rays, int32_t n, uint32_t flags, int32_t* ent_prim, float* tuv, int any) {
    if (!dev || (n > 0 && (!rays || !ent_prim))) return IGX_ERR_INVALID_ARGUMENT;
    if (!dev->has_scene) return fail(dev, IGX_ERR_NO_SCENE, "no scene uploaded");
    if (n <= 0) return IGX_OK;
    HIPCHK(hipSetDevice(dev->hip_device));
    igx_status st = drain(dev);
    if (st != IGX_OK) return st;
    float *d_rays = nullptr, *d_tuv = nullptr;
    int* d_ep = nullptr;
    HIPCHK(hipMalloc((void**)&d_rays, (size_t)n * 8 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&d_ep, (size_t)n * 2 * sizeof(int)));
    HIPCHK(hipMalloc((void**)&d_tuv, (size_t)n * 3 * sizeof(float)));
    HIPCHK(hipMemcpy(d_rays, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice));
    int grid = grid_for(dev, n, MAX_BLOCKS_PER_CU);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (dev->timing) { // kernel time into ms_trace (traversal-only harness timing)
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, dev->stream));
    }
    with_traversal_variant(dev->variant, [&](auto V) {
        hipLaunchKernelGGL(k_trace_hits<decltype(V)::value>, dim3(grid), dim3(BLOCK), 0, dev->stream, dev->sv, d_rays, n, flags, d_ep, d_tuv, any);
    });
    HIPCHK(hipGetLastError());
    if (e1) HIPCHK(hipEventRecord(e1, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    if (e1) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        dev->stats.ms_trace += ms;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIPCHK(hipMemcpy(ent_prim, d_ep, (size_t)n * (any ? 1 : 2) * sizeof(int), hipMemcpyDeviceToHost));
    if (!any && tuv) HIPCHK(hipMemcpy(tuv, d_tuv, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(d_rays);
    (void)hipFree(d_ep);
    (void)hipFree(d_tuv);
    return IGX_OK;
}

extern "C" igx_status igx_trace_hits(igx_device* dev, const float* rays, int32_t n, uint32_t flags, int32_t* ent_prim, float* tuv) {
    return trace_batch(dev, rays, n, flags, ent_prim, tuv, 0);
}

extern "C" igx_status igx_trace_occlusion(igx_device* dev, const float* rays, int32_t n, uint32_t flags, int32_t* occluded) {
    return trace_batch(dev, rays, n, flags, occluded, nullptr, 1);
}

#endif // IGX_PART == 0
