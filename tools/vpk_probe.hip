// Price of packed f32 VALU on gfx950 outside MFMA loops (tools only, not part
// of libigx): what the traversal kernels pay when the compiler's SLP
// vectoriser pairs their multiplies and adds into v_pk_mul_f32 / v_pk_add_f32
// and builds the register pairs with v_mov_b32.
//
// One 1024-thread block per CU (4 waves per SIMD, k_extend's occupancy), every
// wave running the same straight-line loop over 8 independent chains:
//   pk        8 v_pk_mul_f32 + 8 v_pk_add_f32 per body
//   scalar    the same arithmetic unpacked: 16 v_mul_f32 + 16 v_add_f32
//   pk_mov    pk with one v_mov_b32 in front of every packed operation, into
//             the high half of the pair it reads (the pair-building move)
//   scalar_mov  scalar with the same 16 moves (the move's own price)
// The loop is one asm block on fixed registers, so the compiler neither
// reorders nor re-packs it.  Time is hipEvent time of one launch; cycles are
// that time at the device's reported clock, per instruction and SIMD (the four
// waves of a SIMD share its issue), so 2.0 is the v_fma_f32 peak rate.
//
// Build: hipcc --offload-arch=gfx950 -O3 tools/vpk_probe.hip -o tools/vpk_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

namespace {

// chain k of the packed forms lives in v[10+2k:11+2k], the scalar forms use
// v10..v25 one by one; v[40:41] the multiplier (1.0), v[42:43] the addend (0.0),
// v30 the moves' source
#define PK(op, lo, hi, c) "v_pk_" op "_f32 v[" #lo ":" #hi "], v[" #lo ":" #hi "], v[" c "]\n"
#define SC(op, r, c) "v_" op "_f32 v" #r ", v" #r ", v" c "\n"
#define MV(r) "v_mov_b32 v" #r ", v30\n"

#define PK8(op, c) PK(op, 10, 11, c) PK(op, 12, 13, c) PK(op, 14, 15, c) PK(op, 16, 17, c) \
                   PK(op, 18, 19, c) PK(op, 20, 21, c) PK(op, 22, 23, c) PK(op, 24, 25, c)
#define MPK(op, lo, hi, c) MV(hi) PK(op, lo, hi, c)
#define MPK8(op, c) MPK(op, 10, 11, c) MPK(op, 12, 13, c) MPK(op, 14, 15, c) MPK(op, 16, 17, c) \
                    MPK(op, 18, 19, c) MPK(op, 20, 21, c) MPK(op, 22, 23, c) MPK(op, 24, 25, c)
#define SC16(op, c) SC(op, 10, c) SC(op, 11, c) SC(op, 12, c) SC(op, 13, c) SC(op, 14, c) SC(op, 15, c) SC(op, 16, c) SC(op, 17, c) \
                    SC(op, 18, c) SC(op, 19, c) SC(op, 20, c) SC(op, 21, c) SC(op, 22, c) SC(op, 23, c) SC(op, 24, c) SC(op, 25, c)
// the scalar form with a move per pair of operations, into the register the second reads
#define MSC2(op, a, b, c) MV(b) SC(op, a, c) SC(op, b, c)
#define MSC16(op, c) MSC2(op, 10, 11, c) MSC2(op, 12, 13, c) MSC2(op, 14, 15, c) MSC2(op, 16, 17, c) \
                     MSC2(op, 18, 19, c) MSC2(op, 20, 21, c) MSC2(op, 22, 23, c) MSC2(op, 24, 25, c)

#define BODY_PK PK8("mul", "40:41") PK8("add", "42:43")
#define BODY_SCALAR SC16("mul", "40") SC16("add", "42")
#define BODY_PK_MOV MPK8("mul", "40:41") MPK8("add", "42:43")
#define BODY_SCALAR_MOV MSC16("mul", "40") MSC16("add", "42")

#define INIT                                                                                              \
    "v_mov_b32 v10, 1.0\n v_mov_b32 v11, 1.0\n v_mov_b32 v12, 1.0\n v_mov_b32 v13, 1.0\n"                 \
    "v_mov_b32 v14, 1.0\n v_mov_b32 v15, 1.0\n v_mov_b32 v16, 1.0\n v_mov_b32 v17, 1.0\n"                 \
    "v_mov_b32 v18, 1.0\n v_mov_b32 v19, 1.0\n v_mov_b32 v20, 1.0\n v_mov_b32 v21, 1.0\n"                 \
    "v_mov_b32 v22, 1.0\n v_mov_b32 v23, 1.0\n v_mov_b32 v24, 1.0\n v_mov_b32 v25, 1.0\n"                 \
    "v_mov_b32 v30, 1.0\n v_mov_b32 v40, 1.0\n v_mov_b32 v41, 1.0\n v_mov_b32 v42, 0\n v_mov_b32 v43, 0\n"
#define CLOBBERS                                                                                                      \
    "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", \
        "v30", "v40", "v41", "v42", "v43", "s20", "scc"

// four bodies per trip of the loop: the three scalar instructions of the loop
// control are 3 in 64 or more VALU
#define PROBE_KERNEL(name, BODY)                                                               \
    __global__ void __launch_bounds__(1024) name(int trips, float* out) {                      \
        float r;                                                                               \
        asm volatile(INIT "s_mov_b32 s20, %1\n"                                                \
                          "L_loop_%=:\n" BODY BODY BODY BODY "s_sub_u32 s20, s20, 1\n"         \
                          "s_cmp_lg_u32 s20, 0\n"                                              \
                          "s_cbranch_scc1 L_loop_%=\n"                                         \
                          "v_add_f32 %0, v10, v25\n"                                           \
                     : "=v"(r)                                                                 \
                     : "s"(trips)                                                              \
                     : CLOBBERS);                                                              \
        out[blockIdx.x * 1024 + threadIdx.x] = r;                                              \
    }

PROBE_KERNEL(k_pk, BODY_PK)
PROBE_KERNEL(k_scalar, BODY_SCALAR)
PROBE_KERNEL(k_pk_mov, BODY_PK_MOV)
PROBE_KERNEL(k_scalar_mov, BODY_SCALAR_MOV)

#define CHECK(x)                                                         \
    do {                                                                 \
        hipError_t e_ = (x);                                             \
        if (e_ != hipSuccess) {                                          \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// best of `reps` launches, in ms
template <class K>
float time_kernel(K k, int cus, int trips, float* out, int reps) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int r = 0; r <= reps; ++r) { // launch 0 warms up
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k, dim3(cus), dim3(1024), 0, 0, trips, out);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r > 0 && ms < best) best = ms;
    }
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return best;
}

} // namespace

int main() {
    int cus = 0, khz = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
    float* out;
    CHECK(hipMalloc(&out, (size_t)cus * 1024 * sizeof(float)));
    const int trips = 20000, reps = 5, waves_per_simd = 4;
    struct Row {
        const char* name;
        float ms;
        int arith, moves; // VALU instructions per body: arithmetic, moves
    } rows[] = {{"pk", time_kernel(k_pk, cus, trips, out, reps), 16, 0},
                {"scalar", time_kernel(k_scalar, cus, trips, out, reps), 32, 0},
                {"pk_mov", time_kernel(k_pk_mov, cus, trips, out, reps), 16, 16},
                {"scalar_mov", time_kernel(k_scalar_mov, cus, trips, out, reps), 32, 16}};
    for (const Row& r : rows) {
        const double bodies = 4.0 * trips * waves_per_simd; // per SIMD
        const double cyc_body = (double)r.ms * 1e-3 * khz * 1e3 / bodies;
        std::printf("{\"probe\": \"%s\", \"ms\": %.3f, \"clock_mhz\": %d, \"valu_per_body\": %d, \"cycles_per_body\": %.2f, "
                    "\"cycles_per_valu\": %.2f, \"cycles_per_f32_op\": %.3f}\n",
                    r.name, r.ms, khz / 1000, r.arith + r.moves, cyc_body, cyc_body / (r.arith + r.moves), cyc_body / 32.0);
    }
    CHECK(hipFree(out));
    return 0;
}
