// ntuple_search.hip -- depth-limited expectimax with the n-tuple network at the leaves
// (g2048_ntuple_search of include/g2048_ntuple.h): the maximum over the legal moves, the expectation
// over every spawn (each empty cell, a 2 with weight 9, a 4 with weight 1), V of the after-state at the
// leaves.  All values are int64 in points x 4096 and SIGNED (the weights are any int32): a chance node
// is summed exactly before its one floor division (towards minus infinity), the maximum runs over the
// legal moves only and a board without one is worth 0.  So the two lane mappings below (NARROW, WIDE)
// give the same integers whatever the order of their reductions.
//
// The tree walk is expectimax.hip's compile-time recursion over the board in four dwords (nts_M<P, K, S> /
// nts_A<P, K, S>, P <= 2 plies below a lane, K the tuple length), with no stack and no scratch.  The leaf
// is 8 T dependent-address dword gathers, so the kernels are bound by gather latency: the innermost
// maximum, M(b, 1), issues the gathers of all its legal moves' after-states, tuple by tuple (up to 32
// in flight per lane), before it sums any.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "launch_util.hpp"
#include "ntuple_net.hpp"
#include "../../include/g2048_ntuple.h"

using namespace g2048;

namespace {

constexpr int kMaxDepth = 3;
constexpr long long kIllegal = INT64_MIN;
// AUTO's largest board counts for WIDE, see auto_form
constexpr int64_t kWideLanesPerBoard = 16384, kAutoWideBelow2 = 14, kAutoWideBelow3 = 1024;
// the bias of the signed floor division is 10 E x 2^kBiasBits, see floor_div10e
constexpr int kBiasBits = 40;

// ceil(2^64 / e) for the divisor e = E of a chance node, see div10e
constexpr uint64_t recip64(uint32_t e) { return e < 2u ? 0ull : ~0ull / e + 1ull; }
__device__ const uint64_t kRecipE[17] = {recip64(0),  recip64(1),  recip64(2),  recip64(3),  recip64(4),  recip64(5),
                                         recip64(6),  recip64(7),  recip64(8),  recip64(9),  recip64(10), recip64(11),
                                         recip64(12), recip64(13), recip64(14), recip64(15), recip64(16)};

// floor(x / (10 E)) for 0 <= x < 2^63 and E <= 16, exactly: expectimax.hip's div10e, where the proof is
__device__ __forceinline__ uint64_t div10e(uint64_t x, uint32_t E) {
    const uint64_t t = x / 10u;
    const uint64_t q = __umul64hi(t, kRecipE[E]);
    return E == 1u ? t : q;
}

// floor(x / (10 E)) towards minus infinity for |x| < 2^46 (a chance node's sum: at most 160 weighted
// terms of magnitude < 2^38): x + 10 E 2^40 is in [0, 2^49) and floor((x + 10 E 2^40) / (10 E)) =
// floor(x / (10 E)) + 2^40 exactly.  E = 0 (lanes whose result is discarded) gives -2^40.
__device__ __forceinline__ int64_t floor_div10e(int64_t x, uint32_t E) {
    const uint64_t biased = (uint64_t)x + ((uint64_t)(10u * E) << kBiasBits);
    return (int64_t)div10e(biased, E) - (int64_t(1) << kBiasBits);
}

__device__ __forceinline__ int64_t gain_of(uint32_t pts) { return (int64_t)((uint64_t)pts << kFrac); }

template <int P, int K, bool S>
__device__ __forceinline__ int64_t nts_A(const uint4 &s, const NtArgs &net, uint32_t &leaves);

// M(b, P), P >= 1: the best legal move of a board after its spawn; 0 when it has none.  `leaves` counts
// the A(., 0) evaluations below (< 2^32 per lane).  P = 1: the four after-states are evaluated side
// by side, the 8 gathers of a tuple for every legal move issued before any is summed.
template <int P, int K, bool S>
__device__ __forceinline__ int64_t nts_M(const uint4 &b, const NtArgs &net, uint32_t &leaves) {
    long long best = kIllegal;
    if constexpr (P == 1) {
        uint64_t x[4];
        uint32_t row[4];
        long long v[4];
        bool ok[4];
#pragma unroll
        for (uint32_t a = 0u; a < 4u; a++) {
            uint32_t pts, mx;
            const uint4 s = apply_move(b, a, pts, mx);
            ok[a] = !eq4(s, b);
            x[a] = nt_pack(s);
            row[a] = nt_row<S>(net, x[a]);  // each after-state at its own stage
            v[a] = gain_of(pts);
            leaves += ok[a] ? 1u : 0u;
        }
        for (int t = 0; t < net.T; t++) {
            int32_t w[4][8];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const int32_t *W = net.w + ((size_t)(row[a] + t) << (4 * K));
#pragma unroll
                for (int g = 0; g < 8; g++) w[a][g] = ok[a] ? W[nt_index<K>(x[a], net.cells[8 * t + g])] : 0;
            }
#pragma unroll
            for (int a = 0; a < 4; a++) {
#pragma unroll
                for (int g = 0; g < 8; g++) v[a] += w[a][g];
            }
        }
#pragma unroll
        for (int a = 0; a < 4; a++) best = ok[a] && v[a] > best ? v[a] : best;
    } else {
#pragma unroll 1
        for (uint32_t a = 0u; a < 4u; a++) {
            uint32_t pts, mx;
            const uint4 s = apply_move(b, a, pts, mx);
            if (eq4(s, b)) continue;
            const long long v = gain_of(pts) + nts_A<P - 1, K, S>(s, net, leaves);
            best = v > best ? v : best;
        }
    }
    return best == kIllegal ? 0 : best;  // |v| < 2^39: no legal value is INT64_MIN
}

// A(s, P) of an after-state: the weighted sum over every empty cell and both tiles, one floor division
template <int P, int K, bool S>
__device__ __forceinline__ int64_t nts_A(const uint4 &s, const NtArgs &net, uint32_t &leaves) {
    if constexpr (P == 0) {
        leaves += 1u;
        return nt_value<K, S>(net, nt_pack(s));
    } else {
        uint32_t em = empty_mask16(s);
        const uint32_t E = (uint32_t)__popc(em);
        int64_t sum = 0;
#pragma unroll 1
        while (em != 0u) {
            const uint32_t c = (uint32_t)__builtin_ctz(em);
            em &= em - 1u;
#pragma unroll 1
            for (uint32_t t = 1u; t <= 2u; t++) {
                uint4 child = s;
                set_cell(child, c, t);
                const int64_t m = nts_M<P, K, S>(child, net, leaves);
                sum += t == 1u ? 9 * m : m;
            }
        }
        return floor_div10e(sum, E);
    }
}

// sums over the 32 lanes of a (board, action[, spawn, action]) group: both halves of a wave at once;
// x holds signed terms, which the unsigned adds sum correctly (two's complement)
__device__ __forceinline__ void group_sum32(uint64_t &x, uint64_t &l) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        x += (uint64_t)__shfl_xor((unsigned long long)x, off, 32);
        l += (uint64_t)__shfl_xor((unsigned long long)l, off, 32);
    }
}

// the weighted value of the spawn j = 2 cell + (tile - 1) on the after-state s and its leaf count:
// 9 M or 1 M of the child for an empty cell, nothing for an occupied one or a dead group
template <int P, int K, bool S>
__device__ __forceinline__ void spawn_lane(const uint4 &s, uint32_t em, bool group_live, uint32_t j, const NtArgs &net,
                                           uint64_t &x, uint64_t &l) {
    const uint32_t cell = j >> 1, tile = (j & 1u) + 1u;
    x = 0ull;
    l = 0ull;
    if (group_live && ((em >> cell) & 1u)) {
        uint4 child = s;
        set_cell(child, cell, tile);
        uint32_t lv = 0u;
        const int64_t m = nts_M<P, K, S>(child, net, lv);
        x = (uint64_t)(tile == 1u ? 9 * m : m);
        l = lv;
    }
}

// legal mask and best action of a board from its four q (INT64_MIN = illegal): the largest q of a legal
// action, the lowest index among equals, 0xFF without a legal action
__device__ __forceinline__ void write_legal_best(const long long (&v)[4], uint32_t i, uint8_t *__restrict__ legal_out,
                                                 uint8_t *__restrict__ best_out) {
    uint32_t lg = 0u, best = 0xFFu;
    long long bv = kIllegal;
#pragma unroll
    for (uint32_t a = 0u; a < 4u; a++) {
        if (v[a] == kIllegal) continue;
        lg |= 1u << a;
        if (best == 0xFFu || v[a] > bv) {
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
// level: lane j = 0 of a legal action evaluates V.  Lane 0 then derives legal / best through LDS.
template <int D, int K, bool S>
__global__ __launch_bounds__(128) void nts_narrow_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                         long long *__restrict__ q_out, long long *__restrict__ leaves,
                                                         uint8_t *__restrict__ legal_out,
                                                         uint8_t *__restrict__ best_out) {
    __shared__ long long s_val[4];
    const uint32_t i = blockIdx.x, a = threadIdx.x >> 5, j = threadIdx.x & 31u;
    const uint4 root = boards[i];
    uint32_t pts, mx;
    const uint4 moved = apply_move(root, a, pts, mx);
    const bool legal = !eq4(moved, root);
    long long v = kIllegal;
    uint64_t l = 0ull;
    if constexpr (D == 1) {
        if (legal && j == 0u) {
            v = gain_of(pts) + nt_value<K, S>(net, nt_pack(moved));
            l = 1ull;
        }
    } else {
        const uint32_t em = empty_mask16(moved);
        uint64_t x;
        spawn_lane<D - 1, K, S>(moved, em, legal, j, net, x, l);
        group_sum32(x, l);
        if (legal) v = gain_of(pts) + floor_div10e((int64_t)x, (uint32_t)__popc(em));
    }
    if (j == 0u) {
        q_out[4u * i + a] = v;
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
// has no second spawn level: lane j2 = 0 evaluates V of the second after-state); (2) the maximum over
// the legal a2 across the two waves through LDS; (3) lane 0 adds 9 M or 1 M to the (i, a) sum in the
// workspace with a 64-bit atomic (two's-complement wrap: the unsigned add sums the signed terms) and
// then arrives at the (i, a) counter, as emax_wide_kernel does.  The last of the 32 arrivals divides,
// adds the move's points and writes q / leaves; the last of a board's four writes legal / best.  A
// workgroup of an illegal action or an occupied cell only arrives.
template <int D, int K, bool S>
__global__ __launch_bounds__(128) void nts_wide_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                       long long *__restrict__ q_out, long long *__restrict__ leaves,
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
    long long q = kIllegal;
    uint64_t l = 0ull;
    if (live1) {
        uint4 b1 = moved1;
        set_cell(b1, cell1, tile1);
        uint32_t pts2;
        const uint4 moved2 = apply_move(b1, a2, pts2, mx);
        const bool legal2 = !eq4(moved2, b1);
        if constexpr (D == 2) {
            if (legal2 && j2 == 0u) {
                q = gain_of(pts2) + nt_value<K, S>(net, nt_pack(moved2));
                l = 1ull;
            }
        } else {
            const uint32_t em2 = empty_mask16(moved2);
            uint64_t x;
            spawn_lane<D - 2, K, S>(moved2, em2, legal2, j2, net, x, l);
            group_sum32(x, l);
            if (legal2) q = gain_of(pts2) + floor_div10e((int64_t)x, (uint32_t)__popc(em2));
        }
    }
    if (j2 == 0u) {
        s_q[a2] = q;
        s_l[a2] = l;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    if (live1) {
        long long m = kIllegal;  // M(b1, D - 1): the maximum over the legal moves, 0 without one
        unsigned long long lv = 0ull;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            m = s_q[k] > m ? s_q[k] : m;
            lv += s_l[k];
        }
        m = m == kIllegal ? 0 : m;
        const unsigned long long x = (unsigned long long)(tile1 == 1u ? 9 * m : m);
        __hip_atomic_fetch_add(ws_sum + g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(ws_leaves + g, lv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // release: the sums above are performed before the arrival; acquire: the last arrival reads every
    // other workgroup's
    if (__hip_atomic_fetch_add(arrived_g + g, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != 31u) return;
    const unsigned long long x = __hip_atomic_load(ws_sum + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long lv = __hip_atomic_load(ws_leaves + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long v = legal1 ? gain_of(pts1) + floor_div10e((int64_t)x, (uint32_t)__popc(em1)) : kIllegal;
    __hip_atomic_store(q_out + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (leaves) leaves[g] = (long long)lv;
    if (__hip_atomic_fetch_add(arrived_b + i, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != 3u) return;
    if (legal_out || best_out) {
        long long vs[4];
#pragma unroll
        for (uint32_t k = 0u; k < 4u; k++)
            vs[k] = __hip_atomic_load(q_out + 4u * i + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        write_legal_best(vs, i, legal_out, best_out);
    }
}

// the call's own zero-fill of the WIDE workspace: `quads` 16-byte words
__global__ __launch_bounds__(256) void nts_zero_kernel(uint4 *__restrict__ ws, uint32_t quads) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < quads) ws[k] = make_uint4(0u, 0u, 0u, 0u);
}

// AUTO, from tools/time_ntuple_search.py on an MI355X (DESIGN.md, N-tuple search).  A WIDE call costs
// about 10 us + 2 us per board at depth 2 and 2.7 us (five 4-tuples) to 4 us (the 256 MiB table of 4x6)
// per board at depth 3; a NARROW call the time of its longest lane, 30 us at depth 2 and 2.4 ms at
// depth 3, until the chip fills (8 192 boards: 0.16 ms and 10 ms).  Depth 2: WIDE below 14 boards
// (faster for both presets at 4, 8 and 12, slower at 16).  Depth 3: WIDE below 1 024 boards: faster for
// both presets at every count measured up to 768; at 1 024 WIDE is 8 % faster on the 4-tuples and 11 %
// slower on 4x6, at 8 192 NARROW is 2 x faster.
// expectimax.hip's thresholds (NARROW at depth 2, WIDE below 192 at depth 3), the starting point, were
// too narrow here: the leaf is 8 T gathers instead of arithmetic, and NARROW's longest lane waits for
// them one tree node after the other.  Both bounds are far inside WIDE's lane count.
int auto_form(int64_t n, int64_t depth) {
    if (depth == 2) return n < kAutoWideBelow2 ? G2048_EMAX_WIDE : G2048_EMAX_NARROW;
    if (depth == 3) return n < kAutoWideBelow3 ? G2048_EMAX_WIDE : G2048_EMAX_NARROW;
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

template <int D, int K, bool S>
void launch_narrow(hipStream_t st, int64_t n, const NtArgs &a, const uint4 *b, long long *q, long long *lv,
                   uint8_t *legal, uint8_t *best) {
    hipLaunchKernelGGL((nts_narrow_kernel<D, K, S>), dim3((unsigned)n), dim3(128), 0, st, a, b, q, lv, legal, best);
}

template <int D, int K, bool S>
void launch_wide(hipStream_t st, int64_t n, const NtArgs &a, const uint4 *b, long long *q, long long *lv,
                 uint8_t *legal, uint8_t *best, void *workspace) {
    unsigned long long *ws_sum = (unsigned long long *)workspace, *ws_leaves = ws_sum + 4 * n;
    uint32_t *arrived_g = (uint32_t *)(ws_leaves + 4 * n), *arrived_b = arrived_g + 4 * n;
    hipLaunchKernelGGL((nts_wide_kernel<D, K, S>), dim3((unsigned)(n * 128)), dim3(128), 0, st, a, b, q, lv, legal, best,
                       ws_sum, ws_leaves, arrived_g, arrived_b);
}

}  // namespace

extern "C" {

size_t g2048_ntuple_search_workspace_bytes(int64_t n, int64_t depth, int32_t form) {
    const int f = resolve_form(n, depth, form);
    return f < 0 ? 0 : workspace_bytes(n < 1 ? 1 : n, f);
}

static int nt_call_search(g2048_stream_t stream, const g2048_ntuple_net *net, uint64_t stage_map, const int8_t *boards, int64_t n,
                        int64_t depth, int32_t form, int64_t *q, int64_t *leaves, uint8_t *legal, uint8_t *best,
                        void *workspace, size_t workspace_bytes_in) {
    NtArgs a;
    if (!make_args(net, stage_map, a)) return G2048_EINVAL;
    const int f = resolve_form(n, depth, form);
    if (f < 0) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !q || !aligned16(q) || !aligned16(leaves) || !workspace ||
        !aligned16(workspace) || workspace_bytes_in < workspace_bytes(n, f))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uint4 *b = (const uint4 *)boards;
    long long *qv = (long long *)q, *lv = (long long *)leaves;
    if (f == G2048_EMAX_NARROW) {
        switch (depth) {
        case 1: G2048_NT_DISPATCH(a, net->tuple_len, (launch_narrow<1, kK, kS>(st, n, a, b, qv, lv, legal, best))); break;
        case 2: G2048_NT_DISPATCH(a, net->tuple_len, (launch_narrow<2, kK, kS>(st, n, a, b, qv, lv, legal, best))); break;
        default: G2048_NT_DISPATCH(a, net->tuple_len, (launch_narrow<3, kK, kS>(st, n, a, b, qv, lv, legal, best))); break;
        }
        return launch_status();
    }
    const uint32_t quads = (uint32_t)(workspace_bytes(n, f) / 16);
    hipLaunchKernelGGL(nts_zero_kernel, dim3((quads + 255u) / 256u), dim3(256), 0, st, (uint4 *)workspace, quads);
    const int zs = launch_status();
    if (zs != G2048_OK) return zs;
    if (depth == 2) {
        G2048_NT_DISPATCH(a, net->tuple_len, (launch_wide<2, kK, kS>(st, n, a, b, qv, lv, legal, best, workspace)));
    } else {
        G2048_NT_DISPATCH(a, net->tuple_len, (launch_wide<3, kK, kS>(st, n, a, b, qv, lv, legal, best, workspace)));
    }
    return launch_status();
}

// the entry points: the one-stage call is its twin on a staged net with the map 0
int g2048_ntuple_search(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t n,
                        int64_t depth, int32_t form, int64_t *q, int64_t *leaves, uint8_t *legal, uint8_t *best,
                        void *workspace, size_t workspace_bytes) {
    return nt_call_search(stream, net, 0, boards, n, depth, form, q, leaves, legal, best, workspace, workspace_bytes);
}
int g2048_ntuple_staged_search(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                               int64_t n, int64_t depth, int32_t form, int64_t *q, int64_t *leaves, uint8_t *legal,
                               uint8_t *best, void *workspace, size_t workspace_bytes) {
    return nt_call_search(stream, net ? &net->net : nullptr, net ? net->stage_map : 0, boards, n, depth, form, q, leaves,
                          legal, best, workspace, workspace_bytes);
}

}  // extern "C"
