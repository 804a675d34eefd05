// VALU issue-rate probe: cycles per wave-instruction of integer VALU ops at 1, 2 and 4 waves per SIMD.
//   ./valu_rate        (prints one line per op and occupancy)
//   ./valu_rate select (selects in a mixed stream, see below)
// Each wave runs `iters` x 16 independent instructions on 8 accumulators (no dependency stalls);
// cycles come from s_memtime around the loop, the wall time from hipEvents.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <int Op>
__device__ __forceinline__ void body(uint32_t (&a)[8], uint32_t k) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if constexpr (Op == 0) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 1) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 2) asm volatile("v_bitop3_b32 %0, %0, %1, %1 bitop3:0x96" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 3) asm volatile("v_bcnt_u32_b32 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 4) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 5) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 6) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 7) asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 9) asm volatile("v_cndmask_b32_e64 %0, %0, %1, s[20:21]" : "+v"(a[j]) : "v"(k) : "s20", "s21");
        if constexpr (Op == 10) asm volatile("v_perm_b32 %0, %0, %1, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 11) asm volatile("v_or3_b32 %0, %0, %1, %1" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 12) asm volatile("v_mad_u64_u32 %0, s[20:21], %1, %1, %0" : "+v"(*(uint64_t *)&a[j & 6]) : "v"(k) : "s20", "s21");
        if constexpr (Op == 13) asm volatile("v_and_b32_e32 %0, %1, %0" : "+v"(a[j]) : "v"(k));
        if constexpr (Op == 8) asm volatile("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(*(uint64_t *)&a[j & 6]) : "v"((uint64_t)k));
    }
}

template <int Op>
__global__ __launch_bounds__(1024) void probe(uint32_t *out, uint64_t *cyc, int iters, uint32_t k) {
    uint32_t a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = threadIdx.x + j;
    if constexpr (Op == 4) asm volatile("v_cmp_gt_u32 vcc, %0, 37" :: "v"(threadIdx.x) : "vcc");
    if constexpr (Op == 9) asm volatile("v_cmp_gt_u32 s[20:21], %0, 37" :: "v"(threadIdx.x) : "s20", "s21");
    const uint64_t t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) {
        body<Op>(a, k);
        body<Op>(a, k);
    }
    const uint64_t t1 = __builtin_readcyclecounter();
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) s ^= a[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x % 64 == 0) cyc[(blockIdx.x * blockDim.x + threadIdx.x) / 64] = t1 - t0;
}

template <int Op>
int run(const char *name, uint32_t *out, uint64_t *cyc, uint64_t *hcyc) {
    const int iters = 20000;
    for (int w = 1; w <= 4; w *= 2) {
        const int threads = 256 * w, blocks = 256;  // one block per CU, w waves per SIMD
        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        hipLaunchKernelGGL(probe<Op>, dim3(blocks), dim3(threads), 0, 0, out, cyc, 100, 1u);
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(probe<Op>, dim3(blocks), dim3(threads), 0, 0, out, cyc, iters, 1u);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const int waves = blocks * threads / 64;
        CHECK(hipMemcpy(hcyc, cyc, waves * sizeof(uint64_t), hipMemcpyDeviceToHost));
        double avg = 0;
        for (int i = 0; i < waves; i++) avg += (double)hcyc[i];
        avg /= waves;
        const double instr = (double)iters * 16;
        // per SIMD: w waves each issuing instr instructions in `ms`
        const double ns_per_instr_simd = ms * 1e6 / (instr * w);
        printf("%-16s waves/SIMD=%d  wall %.3f ms  %.3f ns per wave-instr per SIMD (=%.2f cyc @2.4GHz)  memtime/wave-instr %.2f\n",
               name, w, ms, ns_per_instr_simd, ns_per_instr_simd * 2.4, avg / instr);
    }
    return 0;
}

// ---------------------------------------------------------------- selects in a mixed stream ----------
//   ./valu_rate select    (the cases below only, at 1 and 2 waves per SIMD)
// A trip is 32 slots in groups of kGap + 1: kGap fillers (v_perm_b32 and v_and_b32 alternating, on
// eight accumulators) and one select in one of three forms -- v_cndmask_b32 on VCC, v_cndmask_b32_e64
// on an SGPR pair, v_bitop3_b32 (m & x) | (~m & k) on a VGPR mask -- or a filler in its place (the
// baseline).  kMake puts the instruction that makes the condition kDist instructions ahead of the
// select (kDist - 1 of the group's fillers between them): v_cmp into VCC / into the SGPR pair, or
// the mask by v_bfe_i32 of a bit / by v_sub_u32 + v_ashrrev_i32; kMake = 0 makes it once, before the loop.
// The maker's source is a register nothing in the loop writes.
enum { kSelNone = 0, kSelVcc = 1, kSelSgpr = 2, kSelBitop = 3 };
enum { kMakeNone = 0, kMakeCmp = 1, kMakeBfe = 2, kMakeSubAshr = 3 };

template <int J>
__device__ __forceinline__ void filler(uint32_t (&a)[8], uint32_t k) {
    if constexpr (J % 2 == 0) asm volatile("v_perm_b32 %0, %0, %1, %1" : "+v"(a[J % 8]) : "v"(k));
    else asm volatile("v_and_b32_e32 %0, %1, %0" : "+v"(a[J % 8]) : "v"(k));
}

template <int Sel, int Make, int Dist, int Gap, int Base>
__device__ __forceinline__ void group(uint32_t (&a)[8], uint32_t k, uint32_t src, uint32_t &m) {
    static_assert(Dist >= 1 && Dist - 1 <= Gap, "the maker sits inside its group");
    if constexpr (Make == kMakeCmp && Sel == kSelVcc) asm volatile("v_cmp_gt_u32_e32 vcc, 37, %0" ::"v"(src) : "vcc");
    if constexpr (Make == kMakeCmp && Sel == kSelSgpr) asm volatile("v_cmp_lt_u32_e64 s[20:21], 37, %0" ::"v"(src) : "s20", "s21");
    if constexpr (Make == kMakeBfe) asm volatile("v_bfe_i32 %0, %1, 1, 1" : "=v"(m) : "v"(src));
    if constexpr (Make == kMakeSubAshr) asm volatile("v_sub_u32_e32 %0, 37, %1\n\tv_ashrrev_i32_e32 %0, 31, %0" : "=&v"(m) : "v"(src));
    // a VALU read of VCC / an SGPR as a lane mask needs two wait states behind the VALU write: the
    // compiler's own `s_nop 1` between an adjacent v_cmp and v_cndmask (counted with the maker)
    if constexpr (Make == kMakeCmp && Dist == 1) asm volatile("s_nop 1");
    // the selects name no clobber: they only read the condition, and a declared VCC / SGPR use makes
    // the compiler add wait states of its own between the asm statements
    constexpr int kSlot = (Base + Gap) % 8;
    auto select = [&] {
        if constexpr (Sel == kSelNone) filler<Base + Gap>(a, k);
        if constexpr (Sel == kSelVcc) asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(a[kSlot]) : "v"(k));
        if constexpr (Sel == kSelSgpr) asm volatile("v_cndmask_b32_e64 %0, %0, %1, s[20:21]" : "+v"(a[kSlot]) : "v"(k));
        if constexpr (Sel == kSelBitop) asm volatile("v_bitop3_b32 %0, %2, %0, %1 bitop3:0xca" : "+v"(a[kSlot]) : "v"(k), "v"(m));
    };
    if constexpr (Dist >= 2) filler<Base + 0>(a, k);
    if constexpr (Dist >= 3) filler<Base + 1>(a, k);
    if constexpr (Dist >= 4) filler<Base + 2>(a, k);
    select();
    if constexpr (Gap > Dist - 1 + 0) filler<Base + Dist - 1 + 0>(a, k);
    if constexpr (Gap > Dist - 1 + 1) filler<Base + Dist - 1 + 1>(a, k);
    if constexpr (Gap > Dist - 1 + 2) filler<Base + Dist - 1 + 2>(a, k);
    if constexpr (Gap > Dist - 1 + 3) filler<Base + Dist - 1 + 3>(a, k);
    if constexpr (Gap > Dist - 1 + 4) filler<Base + Dist - 1 + 4>(a, k);
    if constexpr (Gap > Dist - 1 + 5) filler<Base + Dist - 1 + 5>(a, k);
    if constexpr (Gap > Dist - 1 + 6) filler<Base + Dist - 1 + 6>(a, k);
}

template <int Sel, int Make, int Dist, int Gap>
__global__ __launch_bounds__(1024) void probe_select(uint32_t *out, uint64_t *cyc, int iters, uint32_t k) {
    static_assert(Gap == 3 || Gap == 7, "groups of 4 or 8 slots");
    uint32_t a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = threadIdx.x + j;
    uint32_t src = threadIdx.x * 0x9E3779B9u, m = 0u;
    asm volatile("v_cmp_gt_u32_e32 vcc, 37, %0" ::"v"(src) : "vcc");
    asm volatile("v_cmp_lt_u32_e64 s[20:21], 37, %0" ::"v"(src) : "s20", "s21");
    asm volatile("v_bfe_i32 %0, %1, 1, 1" : "=v"(m) : "v"(src));
    const uint64_t t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) {
        if constexpr (Gap == 3) {
            group<Sel, Make, Dist, 3, 0>(a, k, src, m);
            group<Sel, Make, Dist, 3, 4>(a, k, src, m);
            group<Sel, Make, Dist, 3, 8>(a, k, src, m);
            group<Sel, Make, Dist, 3, 12>(a, k, src, m);
            group<Sel, Make, Dist, 3, 16>(a, k, src, m);
            group<Sel, Make, Dist, 3, 20>(a, k, src, m);
            group<Sel, Make, Dist, 3, 24>(a, k, src, m);
            group<Sel, Make, Dist, 3, 28>(a, k, src, m);
        } else {
            group<Sel, Make, Dist, 7, 0>(a, k, src, m);
            group<Sel, Make, Dist, 7, 8>(a, k, src, m);
            group<Sel, Make, Dist, 7, 16>(a, k, src, m);
            group<Sel, Make, Dist, 7, 24>(a, k, src, m);
        }
    }
    const uint64_t t1 = __builtin_readcyclecounter();
    uint32_t s = m;
#pragma unroll
    for (int j = 0; j < 8; j++) s ^= a[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x % 64 == 0) cyc[(blockIdx.x * blockDim.x + threadIdx.x) / 64] = t1 - t0;
}

// cycles (wall time x 2.4 GHz) per trip of 32 slots per wave; base[] = the all-filler trip of the same
// gap, filled by the kSelNone case, which has to run first
static double g_base[2][2];  // [gap == 7][waves == 2]
template <int Sel, int Make, int Dist, int Gap>
int run_select(const char *name, uint32_t *out, uint64_t *cyc) {
    const int iters = 10000;
    const int groups = 32 / (Gap + 1), makers = Make == kMakeNone ? 0 : Make == kMakeSubAshr ? 2 : 1;
    for (int w = 1; w <= 2; w *= 2) {
        const int threads = 256 * w, blocks = 256;
        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        hipLaunchKernelGGL((probe_select<Sel, Make, Dist, Gap>), dim3(blocks), dim3(threads), 0, 0, out, cyc, 100, 1u);
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((probe_select<Sel, Make, Dist, Gap>), dim3(blocks), dim3(threads), 0, 0, out, cyc, iters, 1u);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double trip = ms * 1e6 * 2.4 / (iters * (double)w);  // cycles per trip per wave, the SIMD shared by w
        double &base = g_base[Gap == 7][w == 2];
        if (Sel == kSelNone) base = trip;
        const int ins = 32 + groups * (makers + (Make == kMakeCmp && Dist == 1 ? 1 : 0));
        // what one group's select (and the instructions that make its condition) costs when the
        // fillers around it cost what they cost in the all-filler trip
        const double sel = (trip - base * (32 - groups) / 32.0) / groups;
        printf("%-34s 1:%d waves/SIMD=%d  %3d ins/trip  %7.1f cyc/trip  %5.2f cyc/ins  select%s %6.2f cyc (a filler %5.2f)\n",
               name, Gap, w, ins, trip, trip / ins, makers ? "+maker" : "", sel, base / 32.0);
    }
    return 0;
}

template <int Gap>
void run_selects(uint32_t *out, uint64_t *cyc) {
    run_select<kSelNone, kMakeNone, 1, Gap>("fillers only (v_perm / v_and)", out, cyc);
    run_select<kSelVcc, kMakeNone, 1, Gap>("v_cndmask vcc", out, cyc);
    run_select<kSelSgpr, kMakeNone, 1, Gap>("v_cndmask_e64 s[20:21]", out, cyc);
    run_select<kSelBitop, kMakeNone, 1, Gap>("v_bitop3 mask select", out, cyc);
    run_select<kSelVcc, kMakeCmp, 1, Gap>("v_cmp vcc, +1 v_cndmask vcc", out, cyc);
    run_select<kSelVcc, kMakeCmp, 4, Gap>("v_cmp vcc, +4 v_cndmask vcc", out, cyc);
    run_select<kSelSgpr, kMakeCmp, 1, Gap>("v_cmp s[20:21], +1 v_cndmask_e64", out, cyc);
    run_select<kSelSgpr, kMakeCmp, 4, Gap>("v_cmp s[20:21], +4 v_cndmask_e64", out, cyc);
    run_select<kSelBitop, kMakeBfe, 1, Gap>("v_bfe_i32, +1 v_bitop3", out, cyc);
    run_select<kSelBitop, kMakeBfe, 4, Gap>("v_bfe_i32, +4 v_bitop3", out, cyc);
    run_select<kSelBitop, kMakeSubAshr, 1, Gap>("v_sub + v_ashrrev, +1 v_bitop3", out, cyc);
    run_select<kSelBitop, kMakeSubAshr, 4, Gap>("v_sub + v_ashrrev, +4 v_bitop3", out, cyc);
}

int main(int argc, char **argv) {
    if (argc > 1 && argv[1][0] == 's') {
        uint32_t *out;
        uint64_t *cyc;
        CHECK(hipMalloc(&out, 256 * 1024 * sizeof(uint32_t)));
        CHECK(hipMalloc(&cyc, 256 * 16 * sizeof(uint64_t)));
        run_selects<3>(out, cyc);
        run_selects<7>(out, cyc);
        return 0;
    }
    uint32_t *out;
    uint64_t *cyc;
    CHECK(hipMalloc(&out, 256 * 1024 * sizeof(uint32_t)));
    CHECK(hipMalloc(&cyc, 256 * 16 * sizeof(uint64_t)));
    static uint64_t hcyc[256 * 16];
    run<0>("v_add_u32", out, cyc, hcyc);
    run<1>("v_xor_b32", out, cyc, hcyc);
    run<2>("v_bitop3_b32", out, cyc, hcyc);
    run<3>("v_bcnt_u32_b32", out, cyc, hcyc);
    run<4>("v_cndmask_b32", out, cyc, hcyc);
    run<5>("v_mul_hi_u32", out, cyc, hcyc);
    run<6>("v_add_f32", out, cyc, hcyc);
    run<7>("v_pk_add_u16", out, cyc, hcyc);
    run<8>("v_lshl_add_u64", out, cyc, hcyc);
    run<9>("v_cndmask_e64", out, cyc, hcyc);
    run<10>("v_perm_b32", out, cyc, hcyc);
    run<11>("v_or3_b32", out, cyc, hcyc);
    run<12>("v_mad_u64_u32", out, cyc, hcyc);
    run<13>("v_and_b32_e32", out, cyc, hcyc);
    return 0;
}
