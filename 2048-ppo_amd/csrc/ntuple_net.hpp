// ntuple_net.hpp -- the n-tuple network as the kernels of ntuple.hip and ntuple_search.hip take it
// (include/g2048_ntuple.h): the kernel argument NtArgs and the host code that packs a g2048_ntuple_net
// into it, the board packed into 16 nibbles, the first tuple row of a board's stage, the table index of
// a (tuple, symmetry) and V(b).  The kernels take the tuple length K and `S`, whether the net has stages,
// as template parameters: the one-stage kernels (S = false) hold no instruction for the stages.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "launch_util.hpp"
#include "../../include/g2048_ntuple.h"

namespace {

using namespace g2048;

constexpr int kMaxT = G2048_NT_MAX_TUPLES, kMaxK = G2048_NT_MAX_LEN, kFrac = G2048_NT_FRAC_BITS;
static_assert(kMaxT * kMaxK == 48, "g2048_ntuple_net.cells holds T x K cells");

// The net as the kernels take it: cells[8 t + g] = the K cells of tuple t under symmetry g, 4 bits each
// (cell j in bits 4 j ..), so that idx_t(g(b)) = sum_j e(b, cell j) << 4 j.  w is [G][T][16^K]: the tables
// of stage g are the tuple rows g T .. g T + T - 1.
struct NtArgs {
    uint32_t cells[8 * kMaxT];
    int32_t *w;
    uint64_t stage_map;  // validated: nibble 0 is 0, every next nibble the one before or one more
    int32_t T;
    int32_t G;  // 1 + nibble 15 of stage_map
};

// min(exponent, 15) of the 16 cells of a board in the nibbles of one word: cell c in bits 4 c .. 4 c + 3
__device__ __forceinline__ uint32_t nt_pack_row(uint32_t r) {
    const uint32_t ge = gem(r, 0x10101010u);   // bit 7 of the bytes >= 16
    const uint32_t m = ge | (ge - (ge >> 7));  // 0xFF in those bytes
    const uint32_t c = (r & ~m) | (m & 0x0F0F0F0Fu);
    const uint32_t p = (c | (c >> 4)) & 0x00FF00FFu;
    return (p | (p >> 8)) & 0xFFFFu;
}
__device__ __forceinline__ uint64_t nt_pack(const uint4 &b) {
    const uint32_t lo = nt_pack_row(b.x) | (nt_pack_row(b.y) << 16), hi = nt_pack_row(b.z) | (nt_pack_row(b.w) << 16);
    return ((uint64_t)hi << 32) | lo;
}

// m(b), the largest of the 16 nibbles of a packed board: 16 bit-field extracts, 8 three-way maxima
__device__ __forceinline__ uint32_t nt_max_nibble(uint64_t x) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    uint32_t m = 0u;
#pragma unroll
    for (int c = 0; c < 8; c++) m = max(m, max((lo >> (4 * c)) & 15u, (hi >> (4 * c)) & 15u));
    return m;
}

__device__ __forceinline__ uint32_t nt_stage(uint64_t stage_map, uint64_t x) {
    return (uint32_t)(stage_map >> (4u * nt_max_nibble(x))) & 15u;
}

// stage(b) T, the first tuple row of the board's stage (below G T: the map is validated); once per board
// evaluated.  S = false: the one-stage net, row 0 and no instruction.
template <bool S>
__device__ __forceinline__ uint32_t nt_row(const NtArgs &net, uint64_t x) {
    if constexpr (S) return nt_stage(net.stage_map, x) * (uint32_t)net.T;
    return 0u;
}

template <int K>
__device__ __forceinline__ uint32_t nt_index(uint64_t x, uint32_t cells) {
    uint32_t idx = 0u;
#pragma unroll
    for (int j = 0; j < K; j++) idx |= ((uint32_t)(x >> (4u * ((cells >> (4 * j)) & 15u))) & 15u) << (4 * j);
    return idx;
}

// V(b): the 8 gathers of a tuple are issued together
template <int K, bool S>
__device__ __forceinline__ int64_t nt_value(const NtArgs &net, uint64_t x) {
    int64_t v = 0;
    const uint32_t row = nt_row<S>(net, x);
    for (int t = 0; t < net.T; t++) {
        const int32_t *W = net.w + ((size_t)(row + t) << (4 * K));
        int32_t w[8];
#pragma unroll
        for (int g = 0; g < 8; g++) w[g] = W[nt_index<K>(x, net.cells[8 * t + g])];
#pragma unroll
        for (int g = 0; g < 8; g++) v += w[g];
    }
    return v;
}

// cell c = 4 r + col under symmetry s of the square: s & 4 transposes, then s & 3 quarter turns
inline int sym_cell(int c, int s) {
    int r = c >> 2, col = c & 3;
    if (s & 4) {
        const int x = r;
        r = col;
        col = x;
    }
    for (int k = 0; k < (s & 3); k++) {
        const int x = r;
        r = col;
        col = 3 - x;
    }
    return 4 * r + col;
}

// false: the net is refused.  stage_map 0: the one-stage net of the calls that take a g2048_ntuple_net
inline bool make_args(const g2048_ntuple_net *net, uint64_t stage_map, NtArgs &out) {
    if (!net) return false;
    const int T = net->num_tuples, K = net->tuple_len;
    if (T < 1 || T > kMaxT || K < 1 || K > kMaxK || !net->weights || !aligned16(net->weights)) return false;
    uint32_t prev = 0u;
    for (int m = 0; m < 16; m++) {
        const uint32_t g = (uint32_t)(stage_map >> (4 * m)) & 15u;
        if (m == 0 ? g != 0u : (g != prev && g != prev + 1u)) return false;
        prev = g;
    }
    out = NtArgs{};
    out.w = net->weights;
    out.stage_map = stage_map;
    out.T = T;
    out.G = (int)prev + 1;
    for (int t = 0; t < T; t++) {
        uint32_t seen = 0u;
        for (int j = 0; j < K; j++) {
            const int c = net->cells[K * t + j];
            if (c < 0 || c > 15 || ((seen >> c) & 1u)) return false;
            seen |= 1u << c;
            for (int s = 0; s < 8; s++) out.cells[8 * t + s] |= (uint32_t)sym_cell(c, s) << (4 * j);
        }
    }
    return true;
}

// fn<kK, kS>(args...) for the run-time tuple length K and kS = whether the net ARGS has stages (the inner
// macros are variadic: CALL reaches them expanded, with commas of its own).  G2048_NT_DISPATCH_BOOL around
// it adds a template switch NAME = COND of the caller's and nests: the whole stays one statement.
#define G2048_NT_DISPATCH_BOOL(COND, NAME, ...)         \
    if (COND) {                                         \
        constexpr bool NAME = true;                     \
        __VA_ARGS__;                                    \
    } else {                                            \
        constexpr bool NAME = false;                    \
        __VA_ARGS__;                                    \
    }
#define G2048_NT_DISPATCH_K(K, ...)  \
    switch (K) {                     \
    case 1: { constexpr int kK = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int kK = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int kK = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int kK = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int kK = 5; __VA_ARGS__; } break; \
    default: { constexpr int kK = 6; __VA_ARGS__; } break; \
    }
#define G2048_NT_DISPATCH(ARGS, K, CALL) \
    G2048_NT_DISPATCH_BOOL((ARGS).stage_map != 0, kS, G2048_NT_DISPATCH_K(K, CALL))

}  // namespace
