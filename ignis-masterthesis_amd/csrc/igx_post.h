// Film post-processing on the device (part 6 of igx_device.hip, inside
// namespace igxh): the reference's tonemap and imageinfo device shaders
// (entrypoints/tonemap.art, entrypoints/imageinfo.art) as HIP kernels over a
// float RGB film in device memory.  The colour arithmetic is host/film_tools.h's
// own functions compiled for the device, so with -ffp-contract=off everything
// but the gamma curve's pow gives the bits the host loops give.
//
//   k_tonemap    16 B per pixel; a thread takes 4 consecutive pixels as three
//                16-byte loads and one 16-byte store (scalar for the tail and
//                for a film or output that is not 16-byte aligned)
//   imageinfo    k_info_lum   luminance plane + per-block min / max / sum / counts
//                k_info_soft  3x3 windows of the plane: soft min / max / median
//                k_info_final one block reduces both slabs in a fixed order
//                k_info_hist  four histograms (LDS, flushed with integer atomics)
//   k_glare_scan entrypoints/glare.art in one pass: per pixel the luminance and
//                the solid angle between its four corner directions
//                (host/glare_model.h), per block the six sums of the daylight
//                glare probability, and the overlay words of the glare source
//
// No float atomics: every float sum is a fixed tree (lane run -> wave shuffle
// -> block -> slab -> k_info_final), so a result is the same bits every run.
#pragma once

constexpr int POST_BLOCK = 256;
// k_info_lum: pixels per block (POST_ITERS groups of 4 per thread, so a lane
// adds 4 * POST_ITERS = 32 luminances in a row)
constexpr int POST_ITERS = 8;
constexpr int POST_CHUNK = POST_BLOCK * 4 * POST_ITERS;
// k_info_soft: a block covers POST_BLOCK interior columns by POST_SOFT_ROWS rows
constexpr int POST_SOFT_ROWS = 8;

__device__ inline uint32_t tonemap_pixel(float r, float g, float b, const PostTonemap& a) {
    const igx::FilmColor c = igx::srgb_to_xyY(igx::FilmColor{r * a.scale, g * a.scale, b * a.scale});
    if (__builtin_isnan(c.b)) return igx::packed_color(0, 255, 255, 255);
    if (__builtin_isinf(c.b)) return igx::packed_color(255, 0, 150, 255);
    if (c.r < 0 || c.g < 0 || c.b < 0) return igx::packed_color(255, 255, 0, 255);
    igx::FilmColor o = igx::xyY_to_srgb(igx::FilmColor{c.r, c.g, igx::tonemap_curve(a.method, a.exposure_factor * c.b + a.exposure_offset)});
    if (a.use_gamma) o = igx::FilmColor{igx::srgb_gamma(o.r), igx::srgb_gamma(o.g), igx::srgb_gamma(o.b)};
    return igx::packed_color(igx::color_byte(o.r), igx::color_byte(o.g), igx::color_byte(o.b), 255);
}

// vec: film and out are 16-byte aligned
__global__ void __launch_bounds__(POST_BLOCK) k_tonemap(const float* __restrict__ film, size_t pixels, PostTonemap a,
                                                        uint32_t* __restrict__ out, int vec) {
    const size_t tid = (size_t)blockIdx.x * POST_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * POST_BLOCK;
    size_t first = 0; // the scalar path's first pixel
    if (vec) {
        const size_t groups = pixels / 4;
        const float4* f4 = reinterpret_cast<const float4*>(film);
        uint4* o4 = reinterpret_cast<uint4*>(out);
        for (size_t g = tid; g < groups; g += stride) {
            const float4 v0 = f4[3 * g], v1 = f4[3 * g + 1], v2 = f4[3 * g + 2];
            uint4 o;
            o.x = tonemap_pixel(v0.x, v0.y, v0.z, a);
            o.y = tonemap_pixel(v0.w, v1.x, v1.y, a);
            o.z = tonemap_pixel(v1.z, v1.w, v2.x, a);
            o.w = tonemap_pixel(v2.y, v2.z, v2.w, a);
            o4[g] = o;
        }
        first = groups * 4;
    }
    for (size_t i = first + tid; i < pixels; i += stride) out[i] = tonemap_pixel(film[3 * i], film[3 * i + 1], film[3 * i + 2], a);
}

// Block reductions in a fixed order: the wave by shuffles, the four waves by
// thread 0 in wave order.  The result is valid on thread 0.
template <typename T, typename Op>
__device__ inline T post_block_reduce(T v, Op op, T* lds) {
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_down(v, d, 64));
    __syncthreads(); // lds may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < POST_BLOCK / 64; ++k) v = op(v, lds[k]);
    return v;
}
struct PostMin { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct PostMax { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct PostAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

__device__ inline float post_finite(float a) { return __builtin_isfinite(a) ? a : 0.0f; }

// Pass 1: block b takes pixels [b * POST_CHUNK, ...): luminance of the scaled
// film (non-finite components read as 0) to `plane`, the block's min / max /
// sum to slab entry b, and with `stats` its inf / NaN / negative component
// counts over the raw components.  vec: the film is 16-byte aligned (the plane
// is the handle's own allocation and always is).
__global__ void __launch_bounds__(POST_BLOCK) k_info_lum(const float* __restrict__ film, size_t n, float scale, float* __restrict__ plane,
                                                         PostSlab s, int stats, int vec) {
    __shared__ float lf[POST_BLOCK / 64];
    __shared__ int li[POST_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * POST_CHUNK;
    float mn = INFINITY, mx = -INFINITY, sum = 0;
    int n_inf = 0, n_nan = 0, n_neg = 0;
    for (int k = 0; k < POST_ITERS; ++k) {
        const size_t p = base + ((size_t)k * POST_BLOCK + threadIdx.x) * 4;
        if (p >= n) break;
        const int cnt = n - p < 4 ? (int)(n - p) : 4;
        float c[12];
        if (vec && cnt == 4) {
            const float4* f4 = reinterpret_cast<const float4*>(film + 3 * p);
            const float4 v0 = f4[0], v1 = f4[1], v2 = f4[2];
            c[0] = v0.x, c[1] = v0.y, c[2] = v0.z, c[3] = v0.w, c[4] = v1.x, c[5] = v1.y;
            c[6] = v1.z, c[7] = v1.w, c[8] = v2.x, c[9] = v2.y, c[10] = v2.z, c[11] = v2.w;
        } else {
            for (int j = 0; j < 12; ++j) c[j] = j < 3 * cnt ? film[3 * p + j] : 0.0f;
        }
        float L[4];
        for (int j = 0; j < 4; ++j) {
            L[j] = igx::srgb_to_xyY(igx::FilmColor{post_finite(c[3 * j]) * scale, post_finite(c[3 * j + 1]) * scale,
                                                   post_finite(c[3 * j + 2]) * scale}).b;
            if (j < cnt) {
                mn = fminf(mn, L[j]);
                mx = fmaxf(mx, L[j]);
                sum += L[j];
            }
        }
        if (stats)
            for (int j = 0; j < 3 * cnt; ++j) {
                n_inf += __builtin_isinf(c[j]) ? 1 : 0;
                n_nan += __builtin_isnan(c[j]) ? 1 : 0;
                n_neg += __builtin_signbit(c[j]) ? 1 : 0;
            }
        if (cnt == 4) *reinterpret_cast<float4*>(plane + p) = make_float4(L[0], L[1], L[2], L[3]);
        else
            for (int j = 0; j < cnt; ++j) plane[p + j] = L[j];
    }
    mn = post_block_reduce(mn, PostMin{}, lf);
    mx = post_block_reduce(mx, PostMax{}, lf);
    sum = post_block_reduce(sum, PostAdd{}, lf);
    if (stats) {
        n_inf = post_block_reduce(n_inf, PostAdd{}, li);
        n_nan = post_block_reduce(n_nan, PostAdd{}, li);
        n_neg = post_block_reduce(n_neg, PostAdd{}, li);
    }
    if (threadIdx.x == 0) {
        s.mn[blockIdx.x] = mn;
        s.mx[blockIdx.x] = mx;
        s.sum[blockIdx.x] = sum;
        s.n_inf[blockIdx.x] = n_inf;
        s.n_nan[blockIdx.x] = n_nan;
        s.n_neg[blockIdx.x] = n_neg;
    }
}

// the 2nd, 5th and 8th smallest of nine values: a 25-exchange sorting network
// (7 layers); the exchanges the three ranks do not need fall away as dead code
__device__ inline void post_sort9_ranks(float* v, float& r2, float& r5, float& r8) {
#define POST_CE(a, b)                                                                                                \
    {                                                                                                                \
        const float lo_ = fminf(v[a], v[b]), hi_ = fmaxf(v[a], v[b]);                                                \
        v[a] = lo_;                                                                                                  \
        v[b] = hi_;                                                                                                  \
    }
    POST_CE(0, 3) POST_CE(1, 7) POST_CE(2, 5) POST_CE(4, 8)
    POST_CE(0, 7) POST_CE(2, 4) POST_CE(3, 8) POST_CE(5, 6)
    POST_CE(0, 2) POST_CE(1, 3) POST_CE(4, 5) POST_CE(7, 8)
    POST_CE(1, 4) POST_CE(3, 6) POST_CE(5, 7)
    POST_CE(0, 1) POST_CE(2, 4) POST_CE(3, 5) POST_CE(6, 8)
    POST_CE(2, 3) POST_CE(4, 5) POST_CE(6, 7)
    POST_CE(1, 2) POST_CE(3, 4) POST_CE(5, 6)
#undef POST_CE
    r2 = v[1];
    r5 = v[4];
    r8 = v[7];
}

// Pass 2 (w > 10 && h > 10): a thread walks POST_SOFT_ROWS interior pixels down
// one column, keeping the two upper rows of the 3x3 window in registers (three
// 4-byte taps per pixel).  Only non-negative ranks contribute; the block's soft
// min / soft max / sum of median * mf go to slab entry blockIdx.y * gridDim.x +
// blockIdx.x.
__global__ void __launch_bounds__(POST_BLOCK) k_info_soft(const float* __restrict__ plane, int w, int h, float mf, PostSlab s) {
    __shared__ float lf[POST_BLOCK / 64];
    const int x = 1 + blockIdx.x * POST_BLOCK + threadIdx.x;
    const int y0 = 1 + blockIdx.y * POST_SOFT_ROWS;
    float smin = 3.40282347e38f, smax = 0, med = 0;
    if (x < w - 1) {
        const float* col = plane + (x - 1);
        float win[9];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 3; ++j) win[3 * (i + 1) + j] = col[(size_t)(y0 - 1 + i) * w + j];
        for (int r = 0; r < POST_SOFT_ROWS && y0 + r < h - 1; ++r) {
            for (int j = 0; j < 6; ++j) win[j] = win[j + 3];
            for (int j = 0; j < 3; ++j) win[6 + j] = col[(size_t)(y0 + r + 1) * w + j];
            float v[9], r2, r5, r8;
            for (int j = 0; j < 9; ++j) v[j] = win[j];
            post_sort9_ranks(v, r2, r5, r8);
            if (r2 >= 0) smin = fminf(smin, r2);
            if (r8 >= 0) smax = fmaxf(smax, r8);
            if (r5 >= 0) med += r5 * mf;
        }
    }
    smin = post_block_reduce(smin, PostMin{}, lf);
    smax = post_block_reduce(smax, PostMax{}, lf);
    med = post_block_reduce(med, PostAdd{}, lf);
    if (threadIdx.x == 0) {
        const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        s.smin[b] = smin;
        s.smax[b] = smax;
        s.med[b] = med;
    }
}

// Finalise: one block reduces the b1 entries of pass 1 and the b2 entries of
// pass 2 (0: no soft pass, the soft values are min / max / avg), thread t
// taking entries t, t + POST_BLOCK, ... in order, then the block tree; writes
// the nine outputs and the histogram's start and factor (imageinfo.art:109-113)
__global__ void __launch_bounds__(POST_BLOCK) k_info_final(PostSlab s, int b1, int b2, size_t n, int bins, PostResult* out) {
    __shared__ float lf[POST_BLOCK / 64];
    __shared__ int li[POST_BLOCK / 64];
    float mn = INFINITY, mx = -INFINITY, sum = 0, smin = 3.40282347e38f, smax = 0, med = 0;
    int n_inf = 0, n_nan = 0, n_neg = 0;
    for (int i = threadIdx.x; i < b1; i += POST_BLOCK) {
        mn = fminf(mn, s.mn[i]);
        mx = fmaxf(mx, s.mx[i]);
        sum += s.sum[i];
        n_inf += s.n_inf[i];
        n_nan += s.n_nan[i];
        n_neg += s.n_neg[i];
    }
    for (int i = threadIdx.x; i < b2; i += POST_BLOCK) {
        smin = fminf(smin, s.smin[i]);
        smax = fmaxf(smax, s.smax[i]);
        med += s.med[i];
    }
    mn = post_block_reduce(mn, PostMin{}, lf);
    mx = post_block_reduce(mx, PostMax{}, lf);
    sum = post_block_reduce(sum, PostAdd{}, lf);
    smin = post_block_reduce(smin, PostMin{}, lf);
    smax = post_block_reduce(smax, PostMax{}, lf);
    med = post_block_reduce(med, PostAdd{}, lf);
    n_inf = post_block_reduce(n_inf, PostAdd{}, li);
    n_nan = post_block_reduce(n_nan, PostAdd{}, li);
    n_neg = post_block_reduce(n_neg, PostAdd{}, li);
    if (threadIdx.x != 0) return;
    PostResult r{};
    r.min = mn;
    r.max = mx;
    r.avg = n ? sum / (float)n : 0.0f;
    r.soft_min = b2 ? smin : r.min;
    r.soft_max = b2 ? smax : r.max;
    r.median = b2 ? med : r.avg;
    r.inf_count = n_inf;
    r.nan_count = n_nan;
    r.neg_count = n_neg;
    r.start = r.min < r.max ? r.min : 0.0f;
    const float end = r.min < r.soft_max ? r.soft_max : (r.min < r.max ? r.max : r.start + 1);
    r.factor = igx::film_safe_div((float)bins, fmaxf(0.0f, end - r.start));
    *out = r;
}

// the host's bin: (int)((v - start) * factor) clamped to [0, bins - 1], where
// the host's conversion of a value outside int's range (or NaN) gives INT_MIN
__device__ inline int post_bin(float v, float start, float factor, int bins) {
    const float x = (v - start) * factor;
    const int i = (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : (-2147483647 - 1);
    return min(max(i, 0), bins - 1);
}

// Pass 3: histograms of the scaled R, G, B and of the luminance plane, hist =
// [4][bins] ints zeroed on the stream before.  lds: a block counts in LDS
// (4 * bins ints of dynamic LDS) and flushes its non-zero bins with one global
// atomic each; else every count is a global atomic.  Integer adds commute, so
// the histograms do not depend on the order.
__global__ void __launch_bounds__(POST_BLOCK) k_info_hist(const float* __restrict__ film, const float* __restrict__ plane, size_t n,
                                                          float scale, const PostResult* __restrict__ res, int bins, int* hist, int lds) {
    extern __shared__ int lh[];
    const float start = res->start, factor = res->factor;
    const size_t first = (size_t)blockIdx.x * POST_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * POST_BLOCK;
    // the four bins of pixel i
    auto bins_of = [&](size_t i, int* at) {
        at[0] = post_bin(post_finite(film[3 * i]) * scale, start, factor, bins);
        at[1] = bins + post_bin(post_finite(film[3 * i + 1]) * scale, start, factor, bins);
        at[2] = 2 * bins + post_bin(post_finite(film[3 * i + 2]) * scale, start, factor, bins);
        at[3] = 3 * bins + post_bin(plane[i], start, factor, bins);
    };
    int at[4];
    if (!lds) {
        for (size_t i = first; i < n; i += stride) {
            bins_of(i, at);
            for (int c = 0; c < 4; ++c) atomicAdd(&hist[at[c]], 1);
        }
        return;
    }
    for (int i = threadIdx.x; i < 4 * bins; i += POST_BLOCK) lh[i] = 0;
    __syncthreads();
    for (size_t i = first; i < n; i += stride) {
        bins_of(i, at);
        for (int c = 0; c < 4; ++c) atomicAdd(&lh[at[c]], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * bins; i += POST_BLOCK)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// Daylight glare (entrypoints/glare.art; host/glare_model.h states the
// arithmetic and the order of the sums): block b takes pixels [b * POST_CHUNK,
// ...) as k_info_lum does.  A thread's 4 pixels are consecutive, so within a
// film row the right-hand corner directions of one pixel are the left-hand
// ones of the next and stay in registers (10 camera directions per 4 pixels
// instead of 16; a direction is a pure function of its lattice point, so the
// bits are those of evaluating every corner).  Each pixel's luminance and solid
// angle are evaluated once and feed the six sums, which go to slab entry b;
// with `overlay` the pixels above the threshold store their heat-map word.
// vec: the film is 16-byte aligned.
static_assert(igx::GLARE_BLOCK == POST_BLOCK && igx::GLARE_ITERS == POST_ITERS && igx::GLARE_CHUNK == POST_CHUNK,
              "glare_host repeats this kernel's reduction order");
__global__ void __launch_bounds__(POST_BLOCK) k_glare_scan(const float* __restrict__ film, size_t n, GlareArgs a, GlareSlab s,
                                                           uint32_t* __restrict__ overlay, int vec) {
    __shared__ float lf[POST_BLOCK / 64];
    __shared__ int li[POST_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * POST_CHUNK;
    const int w = a.w, h = a.h;
    igx::GlareSums acc{0, 0, 0, 0, 0, 0};
    for (int k = 0; k < POST_ITERS; ++k) {
        const size_t p = base + ((size_t)k * POST_BLOCK + threadIdx.x) * 4;
        if (p >= n) break;
        const int cnt = n - p < 4 ? (int)(n - p) : 4;
        float c[12];
        if (vec && cnt == 4) {
            const float4* f4 = reinterpret_cast<const float4*>(film + 3 * p);
            const float4 v0 = f4[0], v1 = f4[1], v2 = f4[2];
            c[0] = v0.x, c[1] = v0.y, c[2] = v0.z, c[3] = v0.w, c[4] = v1.x, c[5] = v1.y;
            c[6] = v1.z, c[7] = v1.w, c[8] = v2.x, c[9] = v2.y, c[10] = v2.z, c[11] = v2.w;
        } else {
            for (int j = 0; j < 12; ++j) c[j] = j < 3 * cnt ? film[3 * p + j] : 0.0f;
        }
        int y = (int)(p / (size_t)w);
        int x = (int)(p - (size_t)y * w);
        igx::CamVec r1{}, r2{}, r3{}, r4{};
        bool carry = false; // r4 / r3 of the previous pixel are this one's r1 / r2
        for (int j = 0; j < cnt; ++j) {
            if (carry) {
                r1 = r4;
                r2 = r3;
            } else {
                r1 = igx::glare_pixel_dir(a.cam, w, h, x, y);
                r2 = igx::glare_pixel_dir(a.cam, w, h, x, y + 1);
            }
            r3 = igx::glare_pixel_dir(a.cam, w, h, x + 1, y + 1);
            r4 = igx::glare_pixel_dir(a.cam, w, h, x + 1, y);
            const float lum = igx::glare_luminance(c[3 * j], c[3 * j + 1], c[3 * j + 2], a.scale);
            if (igx::glare_add_pixel(acc, a.cam, x, y, lum, a.lum_source, r1, r2, r3, r4) && overlay)
                overlay[p + j] = igx::glare_overlay(lum, a.lum_source, a.lum_max);
            carry = ++x < w;
            if (x == w) {
                x = 0;
                ++y;
            }
        }
    }
    const float ev = post_block_reduce(acc.ev, PostAdd{}, lf);
    const int cnt = post_block_reduce(acc.n, PostAdd{}, li);
    const float om = post_block_reduce(acc.omega, PostAdd{}, lf);
    const float lm = post_block_reduce(acc.lum, PostAdd{}, lf);
    const float sx = post_block_reduce(acc.x, PostAdd{}, lf);
    const float sy = post_block_reduce(acc.y, PostAdd{}, lf);
    if (threadIdx.x == 0) {
        s.ev[blockIdx.x] = ev;
        s.n[blockIdx.x] = cnt;
        s.omega[blockIdx.x] = om;
        s.lum[blockIdx.x] = lm;
        s.x[blockIdx.x] = sx;
        s.y[blockIdx.x] = sy;
    }
}

static bool post_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

GlareSlab glare_slab(float* base, size_t blocks) {
    return GlareSlab{base, base + blocks, base + 2 * blocks, base + 3 * blocks, base + 4 * blocks, (int*)(base + 5 * blocks)};
}

void launch_glare(igx_device* dev, const float* film, const GlareArgs& a, float* slab, uint32_t* overlay) {
    const size_t n = (size_t)a.w * a.h;
    const int blocks = post_lum_blocks(n);
    hipLaunchKernelGGL(k_glare_scan, dim3(blocks), dim3(POST_BLOCK), 0, dev->stream, film, n, a, glare_slab(slab, blocks), overlay,
                       post_aligned16(film) ? 1 : 0);
}

// the tail of the evaluation, on the host in this part's arithmetic (no
// -fapprox-func): the slab's entries added in block order, then glare_finish
igx_glare_output glare_finish_slab(float* slab_host, size_t blocks, const igx_glare_settings& set, const CameraModel& cam, int w, int h) {
    const GlareSlab s = glare_slab(slab_host, blocks);
    igx::GlareSums total{0, 0, 0, 0, 0, 0};
    for (size_t b = 0; b < blocks; ++b)
        total = igx::glare_sums_add(total, igx::GlareSums{s.ev[b], s.n[b], s.omega[b], s.lum[b], s.x[b], s.y[b]});
    return igx::glare_finish(total, set, cam, w, h);
}

void launch_tonemap(igx_device* dev, const float* film, size_t pixels, const PostTonemap& a, uint32_t* out) {
    const size_t work = (pixels + 3) / 4;
    const int grid = (int)std::min<size_t>((work + POST_BLOCK - 1) / POST_BLOCK, (size_t)dev->num_cus * MAX_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_tonemap, dim3(grid), dim3(POST_BLOCK), 0, dev->stream, film, pixels, a, out,
                       post_aligned16(film) && post_aligned16(out) ? 1 : 0);
}

int post_lum_blocks(size_t n) { return (int)((n + POST_CHUNK - 1) / POST_CHUNK); }
static dim3 post_soft_grid(int w, int h) { return dim3((w - 2 + POST_BLOCK - 1) / POST_BLOCK, (h - 2 + POST_SOFT_ROWS - 1) / POST_SOFT_ROWS); }
int post_soft_blocks(int w, int h) {
    if (!(w > 10 && h > 10)) return 0;
    const dim3 g = post_soft_grid(w, h);
    return (int)(g.x * g.y);
}

void launch_imageinfo(igx_device* dev, const float* film, int w, int h, float scale, bool stats, int bins, float* plane, const PostSlab& s,
                      PostResult* res, int* hist) {
    const size_t n = (size_t)w * h;
    const int b1 = post_lum_blocks(n), b2 = post_soft_blocks(w, h);
    hipLaunchKernelGGL(k_info_lum, dim3(b1), dim3(POST_BLOCK), 0, dev->stream, film, n, scale, plane, s, stats ? 1 : 0,
                       post_aligned16(film) ? 1 : 0);
    if (b2) {
        const float mf = igx::film_safe_div(1, (float)((size_t)(w - 2) * (size_t)(h - 2)));
        hipLaunchKernelGGL(k_info_soft, post_soft_grid(w, h), dim3(POST_BLOCK), 0, dev->stream, plane, w, h, mf, s);
    }
    hipLaunchKernelGGL(k_info_final, dim3(1), dim3(POST_BLOCK), 0, dev->stream, s, b1, b2, n, bins, res);
    if (hist) {
        const size_t lds_bytes = (size_t)4 * bins * sizeof(int);
        const bool lds = lds_bytes <= POST_HIST_LDS_MAX;
        const int grid = (int)std::min<size_t>((n + POST_BLOCK - 1) / POST_BLOCK, (size_t)dev->num_cus * 4);
        hipLaunchKernelGGL(k_info_hist, dim3(grid), dim3(POST_BLOCK), lds ? lds_bytes : 0, dev->stream, film, plane, n, scale, res, bins,
                           hist, lds ? 1 : 0);
    }
}
