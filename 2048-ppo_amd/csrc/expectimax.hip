// expectimax.hip -- exact depth-limited expectimax (g2048_expectimax of include/g2048.h): the maximum
// over the four moves, the expectation over every spawn (each empty cell, a 2 with weight 9, a 4 with
// weight 1), monotonicity and emptiness as the leaf evaluation.  All values are int64 with 16
// fractional bits and every chance node is summed exactly before its one floor division, so the two
// lane mappings below (NARROW, WIDE) give the same integers whatever the order of their reductions.
//
// The subtree of a lane is a compile-time recursion (emax_M<K> / emax_A<K>, K <= 3) over the board in
// four dwords: the loops over actions and empty cells keep one copy of the next level each, the empty
// cells are walked by clearing the lowest set bit of empty_mask16, and nothing is indexed at run time,
// so there is no stack and no scratch (see DESIGN.md for the resource report).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "launch_util.hpp"
#include "../../include/g2048.h"

using namespace g2048;

namespace {

constexpr int64_t kScale = 65536, kMaxWeight = 4096;
constexpr int kMaxDepth = 4;
// AUTO's largest board counts for WIDE, see auto_form
constexpr int64_t kWideLanesPerBoard = 16384, kAutoWideBelow3 = 192;

// S x the three weights (each <= 2^28)
struct EmaxW {
    uint32_t sp, sm, se;
};

// ceil(2^64 / e) for the divisor e = E of a chance node, see div10e
constexpr uint64_t recip64(uint32_t e) { return e < 2u ? 0ull : ~0ull / e + 1ull; }
__device__ const uint64_t kRecipE[17] = {recip64(0),  recip64(1),  recip64(2),  recip64(3),  recip64(4),  recip64(5),
                                         recip64(6),  recip64(7),  recip64(8),  recip64(9),  recip64(10), recip64(11),
                                         recip64(12), recip64(13), recip64(14), recip64(15), recip64(16)};

// floor(x / (10 E)) for x < 2^63, exactly and without the 64-bit division routine:
// floor(x / (10 E)) = floor(floor(x / 10) / E); the division by the constant 10 is the compiler's exact
// multiply-high, and for t = floor(x / 10) < 2^60 and 2 <= E <= 16, m = ceil(2^64 / E) = (2^64 + r) / E
// with 0 <= r < E gives t m / 2^64 = t / E + t r / (E 2^64), where t r < 2^64, so the excess over t / E
// is below 1 / E and the floor of the product is floor(t / E).  E = 0 (an illegal move's lanes, whose
// result is discarded) gives 0.
__device__ __forceinline__ uint64_t div10e(uint64_t x, uint32_t E) {
    const uint64_t t = x / 10u;
    const uint64_t q = __umul64hi(t, kRecipE[E]);
    return E == 1u ? t : q;
}

// H(s) of an after-state
__device__ __forceinline__ int64_t emax_leaf(const uint4 &s, const EmaxW &w) {
    return (int64_t)((uint64_t)w.sm * (uint32_t)monotonicity(s) + (uint64_t)w.se * (uint32_t)emptiness(s));
}

template <int K>
__device__ __forceinline__ int64_t emax_A(const uint4 &s, const EmaxW &w, uint32_t &leaves);

// M(b, K), K >= 1: the best move of a board after its spawn; 0 when it has none.  `leaves` counts the
// A(., 0) evaluations below (< 2^32 per lane: at most (4 x 30)^3 x 4 under one first spawn).
template <int K>
__device__ __forceinline__ int64_t emax_M(const uint4 &b, const EmaxW &w, uint32_t &leaves) {
    int64_t best = 0;
#pragma unroll 1
    for (uint32_t a = 0u; a < 4u; a++) {
        uint32_t pts, mx;
        const uint4 s = apply_move(b, a, pts, mx);
        if (eq4(s, b)) continue;
        const int64_t v = (int64_t)((uint64_t)w.sp * pts) + emax_A<K - 1>(s, w, leaves);
        best = v > best ? v : best;
    }
    return best;
}

// A(s, K) of an after-state: the weighted sum over every empty cell and both tiles, one division
template <int K>
__device__ __forceinline__ int64_t emax_A(const uint4 &s, const EmaxW &w, uint32_t &leaves) {
    if constexpr (K == 0) {
        leaves += 1u;
        return emax_leaf(s, w);
    } else {
        uint32_t em = empty_mask16(s);
        const uint32_t E = (uint32_t)__popc(em);
        uint64_t sum = 0ull;
#pragma unroll 1
        while (em != 0u) {
            const uint32_t c = (uint32_t)__builtin_ctz(em);
            em &= em - 1u;
#pragma unroll 1
            for (uint32_t t = 1u; t <= 2u; t++) {
                uint4 child = s;
                set_cell(child, c, t);
                const uint64_t m = (uint64_t)emax_M<K>(child, w, leaves);
                sum += t == 1u ? 9ull * m : m;
            }
        }
        return (int64_t)div10e(sum, E);
    }
}

// sums over the 32 lanes of a (board, action[, spawn, action]) group: both halves of a wave at once
__device__ __forceinline__ void group_sum32(uint64_t &x, uint64_t &l) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        x += (uint64_t)__shfl_xor((unsigned long long)x, off, 32);
        l += (uint64_t)__shfl_xor((unsigned long long)l, off, 32);
    }
}

// the weighted value of the spawn j = 2 cell + (tile - 1) on the after-state s and its leaf count:
// 9 M or 1 M of the child for an empty cell, nothing for an occupied one or a dead group
template <int K>
__device__ __forceinline__ void spawn_lane(const uint4 &s, uint32_t em, bool group_live, uint32_t j, const EmaxW &w,
                                           uint64_t &x, uint64_t &l) {
    const uint32_t cell = j >> 1, tile = (j & 1u) + 1u;
    x = 0ull;
    l = 0ull;
    if (group_live && ((em >> cell) & 1u)) {
        uint4 child = s;
        set_cell(child, cell, tile);
        uint32_t lv = 0u;
        const uint64_t m = (uint64_t)emax_M<K>(child, w, lv);
        x = tile == 1u ? 9ull * m : m;
        l = lv;
    }
}

// legal mask and best action of a board from its four values (-1 = illegal): the largest value, the
// lowest index among equals, 0xFF without a legal action
__device__ __forceinline__ void write_legal_best(const long long (&v)[4], uint32_t i, uint8_t *__restrict__ legal_out,
                                                 uint8_t *__restrict__ best_out) {
    uint32_t lg = 0u, best = 0xFFu;
    long long bv = -1;
#pragma unroll
    for (uint32_t a = 0u; a < 4u; a++) {
        if (v[a] >= 0) lg |= 1u << a;
        if (v[a] > bv) {
            bv = v[a];
            best = a;
        }
    }
    if (legal_out) legal_out[i] = (uint8_t)lg;
    if (best_out) best_out[i] = (uint8_t)best;
}

// NARROW: one workgroup of 128 lanes per board, lane = (action a, first spawn j): two (board, action)
// groups per wave.  For D >= 2 a live lane (legal a, empty cell) evaluates M(child, D - 1); the group's
// 32 lanes are summed by shuffles, divided once and the move's points added.  D = 1 has no spawn
// level.  Lane 0 then derives legal / best from the four values through LDS.
template <int D>
__global__ __launch_bounds__(128) void emax_narrow_kernel(const uint4 *__restrict__ boards, EmaxW w,
                                                          long long *__restrict__ value, long long *__restrict__ leaves,
                                                          uint8_t *__restrict__ legal_out,
                                                          uint8_t *__restrict__ best_out) {
    __shared__ long long s_val[4];
    const uint32_t i = blockIdx.x, a = threadIdx.x >> 5, j = threadIdx.x & 31u;
    const uint4 root = boards[i];
    uint32_t pts, mx;
    const uint4 moved = apply_move(root, a, pts, mx);
    const bool legal = !eq4(moved, root);
    const int64_t gain = (int64_t)((uint64_t)w.sp * pts);
    long long v;
    uint64_t l;
    if constexpr (D == 1) {
        v = legal ? gain + emax_leaf(moved, w) : -1;
        l = legal ? 1ull : 0ull;
    } else {
        const uint32_t em = empty_mask16(moved);
        uint64_t x;
        spawn_lane<D - 1>(moved, em, legal, j, w, x, l);
        group_sum32(x, l);
        v = legal ? gain + (int64_t)div10e(x, (uint32_t)__popc(em)) : -1;
    }
    if (j == 0u) {
        value[4u * i + a] = v;
        if (leaves) leaves[4u * i + a] = (long long)l;
        s_val[a] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0u && (legal_out || best_out)) {
        const long long vs[4] = {s_val[0], s_val[1], s_val[2], s_val[3]};
        write_legal_best(vs, i, legal_out, best_out);
    }
}

// WIDE (D >= 2): one workgroup of 128 lanes per (board i, action a, first spawn j1), lane = (second
// action a2, second spawn j2).  (1) the weighted sum over j2 and its division inside 32 lanes (D = 2
// has no second spawn level: H of the second after-state); (2) the maximum over a2 across the two
// waves through LDS; (3) lane 0 adds 9 M or 1 M to the (i, a) sum in the workspace with a 64-bit
// atomic and then arrives at the (i, a) counter -- as mc_search_kernel finishes a board.  The last of
// the 32 arrivals divides, adds the move's points and writes value / leaves; the last of a board's
// four writes legal / best.  A workgroup of an illegal action or an occupied cell only arrives.
template <int D>
__global__ __launch_bounds__(128) void emax_wide_kernel(const uint4 *__restrict__ boards, EmaxW w,
                                                        long long *__restrict__ value, long long *__restrict__ leaves,
                                                        uint8_t *__restrict__ legal_out, uint8_t *__restrict__ best_out,
                                                        unsigned long long *__restrict__ ws_sum,
                                                        unsigned long long *__restrict__ ws_leaves,
                                                        uint32_t *__restrict__ arrived_g,
                                                        uint32_t *__restrict__ arrived_b) {
    __shared__ long long s_q[4];
    __shared__ unsigned long long s_l[4];
    const uint32_t g = blockIdx.x >> 5, j1 = blockIdx.x & 31u;  // g = 4 i + a
    const uint32_t i = g >> 2, a = g & 3u;
    const uint32_t a2 = threadIdx.x >> 5, j2 = threadIdx.x & 31u;
    const uint4 root = boards[i];
    uint32_t pts1, mx;
    const uint4 moved1 = apply_move(root, a, pts1, mx);
    const bool legal1 = !eq4(moved1, root);
    const uint32_t em1 = empty_mask16(moved1);
    const uint32_t cell1 = j1 >> 1, tile1 = (j1 & 1u) + 1u;
    const bool live1 = legal1 && ((em1 >> cell1) & 1u);  // uniform over the workgroup
    long long q = -1;
    uint64_t l = 0ull;
    if (live1) {
        uint4 b1 = moved1;
        set_cell(b1, cell1, tile1);
        uint32_t pts2;
        const uint4 moved2 = apply_move(b1, a2, pts2, mx);
        const bool legal2 = !eq4(moved2, b1);
        const int64_t gain2 = (int64_t)((uint64_t)w.sp * pts2);
        if constexpr (D == 2) {
            q = legal2 ? gain2 + emax_leaf(moved2, w) : -1;
            l = legal2 ? 1ull : 0ull;
        } else {
            const uint32_t em2 = empty_mask16(moved2);
            uint64_t x;
            spawn_lane<D - 2>(moved2, em2, legal2, j2, w, x, l);
            group_sum32(x, l);
            q = legal2 ? gain2 + (int64_t)div10e(x, (uint32_t)__popc(em2)) : -1;
        }
    }
    if (j2 == 0u) {
        s_q[a2] = q;
        s_l[a2] = l;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    if (live1) {
        long long m = 0;  // M(b1, D - 1): 0 without a legal move
        unsigned long long lv = 0ull;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            m = s_q[k] > m ? s_q[k] : m;
            lv += s_l[k];
        }
        const unsigned long long x = tile1 == 1u ? 9ull * (unsigned long long)m : (unsigned long long)m;
        __hip_atomic_fetch_add(ws_sum + g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(ws_leaves + g, lv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // release: the sums above are performed before the arrival; acquire: the last arrival reads every
    // other workgroup's
    if (__hip_atomic_fetch_add(arrived_g + g, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != 31u) return;
    const unsigned long long x = __hip_atomic_load(ws_sum + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long lv = __hip_atomic_load(ws_leaves + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long v = legal1 ? (long long)((uint64_t)w.sp * pts1 + div10e(x, (uint32_t)__popc(em1))) : -1;
    __hip_atomic_store(value + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (leaves) leaves[g] = (long long)lv;
    if (__hip_atomic_fetch_add(arrived_b + i, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != 3u) return;
    if (legal_out || best_out) {
        long long vs[4];
#pragma unroll
        for (uint32_t k = 0u; k < 4u; k++)
            vs[k] = __hip_atomic_load(value + 4u * i + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        write_legal_best(vs, i, legal_out, best_out);
    }
}

// the call's own zero-fill of the WIDE workspace: `quads` 16-byte words
__global__ __launch_bounds__(256) void emax_zero_kernel(uint4 *__restrict__ ws, uint32_t quads) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < quads) ws[k] = make_uint4(0u, 0u, 0u, 0u);
}

// AUTO, from tools/time_expectimax.py on an MI355X (Expectimax): a WIDE call costs about
// 2.2 us per board whatever the depth up to 3 (its 128 workgroups per board), a NARROW call the time
// of its longest lane.  Depth <= 2: NARROW at every n.  Depth 3: WIDE below 192 boards (faster at 128,
// slower at 256; 192 interpolates the two).  Depth 4: WIDE wherever its lane count allows (5.5 x
// faster at 1024 boards, the largest n measured), NARROW beyond.  The first guess -- WIDE at depth >= 3
// while NARROW would leave SIMDs without a wave, n < 512 -- was too wide at depth 3 and too narrow at 4.
int auto_form(int64_t n, int64_t depth) {
    if (depth == 3) return n < kAutoWideBelow3 ? G2048_EMAX_WIDE : G2048_EMAX_NARROW;
    if (depth == 4) return n * kWideLanesPerBoard < (int64_t(1) << 31) ? G2048_EMAX_WIDE : G2048_EMAX_NARROW;
    return G2048_EMAX_NARROW;
}

// -1: the arguments are refused
int resolve_form(int64_t n, int64_t depth, int32_t form) {
    if (depth < 1 || depth > kMaxDepth || n < 0 || n >= (int64_t(1) << 31)) return -1;
    if (form == G2048_EMAX_AUTO) form = auto_form(n, depth);
    if (form == G2048_EMAX_NARROW) return n * 128 < (int64_t(1) << 31) ? form : -1;
    if (form == G2048_EMAX_WIDE) return depth >= 2 && n * kWideLanesPerBoard < (int64_t(1) << 31) ? form : -1;
    return -1;
}

// WIDE: sum / leaves [4 n] 64-bit words, arrival counters [4 n] + [n] 32-bit words; NARROW uses none
size_t workspace_bytes(int64_t n, int form) {
    if (form != G2048_EMAX_WIDE) return 16;
    return ((size_t)n * (4 * 8 + 4 * 8 + 4 * 4 + 4) + 15) & ~(size_t)15;
}

}  // namespace

extern "C" {

size_t g2048_expectimax_workspace_bytes(int64_t n, int64_t depth, int32_t form) {
    const int f = resolve_form(n, depth, form);
    return f < 0 ? 0 : workspace_bytes(n < 1 ? 1 : n, f);
}

int g2048_expectimax(g2048_stream_t stream, const int8_t *boards, int64_t n, int64_t depth, int32_t w_points,
                     int32_t w_mono, int32_t w_empt, int32_t form, int64_t *value, int64_t *leaves, uint8_t *legal,
                     uint8_t *best, void *workspace, size_t workspace_bytes_in) {
    const int f = resolve_form(n, depth, form);
    if (f < 0) return G2048_EINVAL;
    if (w_points < 0 || w_points > kMaxWeight || w_mono < 0 || w_mono > kMaxWeight || w_empt < 0 || w_empt > kMaxWeight)
        return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !value || !aligned16(value) || !aligned16(leaves) || !workspace ||
        !aligned16(workspace) || workspace_bytes_in < workspace_bytes(n, f))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const EmaxW w{(uint32_t)(kScale * w_points), (uint32_t)(kScale * w_mono), (uint32_t)(kScale * w_empt)};
    const uint4 *b = (const uint4 *)boards;
    long long *val = (long long *)value, *lv = (long long *)leaves;
    if (f == G2048_EMAX_NARROW) {
        const dim3 grid((unsigned)n), block(128);
        switch (depth) {
        case 1: hipLaunchKernelGGL(emax_narrow_kernel<1>, grid, block, 0, st, b, w, val, lv, legal, best); break;
        case 2: hipLaunchKernelGGL(emax_narrow_kernel<2>, grid, block, 0, st, b, w, val, lv, legal, best); break;
        case 3: hipLaunchKernelGGL(emax_narrow_kernel<3>, grid, block, 0, st, b, w, val, lv, legal, best); break;
        default: hipLaunchKernelGGL(emax_narrow_kernel<4>, grid, block, 0, st, b, w, val, lv, legal, best); break;
        }
        return launch_status();
    }
    const uint32_t quads = (uint32_t)(workspace_bytes(n, f) / 16);
    hipLaunchKernelGGL(emax_zero_kernel, dim3((quads + 255u) / 256u), dim3(256), 0, st, (uint4 *)workspace, quads);
    const int zs = launch_status();
    if (zs != G2048_OK) return zs;
    unsigned long long *ws_sum = (unsigned long long *)workspace, *ws_leaves = ws_sum + 4 * n;
    uint32_t *arrived_g = (uint32_t *)(ws_leaves + 4 * n), *arrived_b = arrived_g + 4 * n;
    const dim3 grid((unsigned)(n * 128)), block(128);
    switch (depth) {
    case 2:
        hipLaunchKernelGGL(emax_wide_kernel<2>, grid, block, 0, st, b, w, val, lv, legal, best, ws_sum, ws_leaves,
                           arrived_g, arrived_b);
        break;
    case 3:
        hipLaunchKernelGGL(emax_wide_kernel<3>, grid, block, 0, st, b, w, val, lv, legal, best, ws_sum, ws_leaves,
                           arrived_g, arrived_b);
        break;
    default:
        hipLaunchKernelGGL(emax_wide_kernel<4>, grid, block, 0, st, b, w, val, lv, legal, best, ws_sum, ws_leaves,
                           arrived_g, arrived_b);
        break;
    }
    return launch_status();
}

}  // extern "C"
