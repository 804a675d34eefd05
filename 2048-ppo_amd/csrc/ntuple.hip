// ntuple.hip -- n-tuple network with afterstate TD(0) learning (include/g2048_ntuple.h): the value of
// a board is a sum of 8 T table weights (T tuples x the 8 symmetries of the square), the player takes
// the move of the largest points + value of the after-state, and the TD step moves the weights of the
// previous after-state towards that maximum.  Weights and values are integers (points x 4096), every
// update is an integer add, so n envs learning in parallel on one net are reproducible bit for bit.
//
// One lane per env / board.  The board's exponents are clamped to 15 and packed into the 16 nibbles of
// one 64-bit word; a table index is K nibbles of it, picked by wave-uniform shifts: the cells of
// (tuple, symmetry) are one packed word of the kernel argument (scalar registers), the tuple length K
// is a template parameter.  The gathers are one dword per lane at unrelated addresses; the updates are
// no-return 32-bit atomic adds of the same shape.  A learning step is up to three launches, and stream
// order between them makes every read of a step see what it reads before the step's adds:
// nt_td_eval_kernel only reads the weights (choice, target, D); nt_tc_weights_kernel, under rule TC only
// (temporal-coherence learning: a step size per weight out of 16 bytes of accumulators, E the sum of the
// D a weight received and A the sum of their |D|), reads the records and adds each weight's share of D;
// nt_update_kernel adds D to the weights (TD) or to the records (TC, 64-bit atomics) and steps the env.
// Two template switches beside K and S select what the two writing kernels hold: TC, the rule, and L,
// whether there is a trace (g2048_ntuple_lambda, lambda = 2^-s, trace_len > 0): then D >> k s also goes to
// the after-state k moves older, kept per env in hist.  Without the rule or the trace a kernel holds no
// instruction for it, and an empty struct (one byte behind the others) in place of its arguments.
// A net with stages (stage_map != 0) has G sets of tables, [G][T][16^K]: every board evaluated or updated
// goes to the tuple rows of its own stage (nt_row of ntuple_net.hpp, a function of its largest nibble), in
// kernels instantiated with S = true beside the one-stage ones.  nt_stage_kernel writes the stages of
// boards, nt_promote_kernel adds one stage's tables to another's (g2048_ntuple_promote).  nt_fill_kernel starts
// every weight of a net at one value (optimistic initialisation, g2048_ntuple_fill) and nt_promote_from_kernel
// is the promotion that takes that start off what it adds (g2048_ntuple_promote_from).  nt_downgrade_kernel is
// the players' tile-downgrading (g2048_ntuple_downgrade): a board-to-board map in front of the choose and search
// calls, which stay as they are.
// The carousel (g2048_ntuple_staged_carousel) is a third switch, C, on the reading kernel and on the last
// one: a finished game restarts from a board with which some game entered a stage, out of a pool of one
// slot per (stage, env).  The reading kernel picks every env's donor slot and start stage and leaves them in
// the workspace; the last launch records the boards that enter a stage and applies the restart to the games
// that end, so every read of the pool sees it as it was before the step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "step.hpp"
#include "launch_util.hpp"
#include "ntuple_net.hpp"
#include "../../include/g2048_ntuple.h"

using namespace g2048;

namespace {

constexpr int64_t kMaxD = int64_t(1) << 30;

// D added to each of the 8 T weights V(b) reads, with multiplicity; the weights wrap
template <int K, bool S>
__device__ __forceinline__ void nt_add(const NtArgs &net, uint64_t x, int32_t D) {
    const uint32_t row = nt_row<S>(net, x);
    for (int t = 0; t < net.T; t++) {
        uint32_t *W = (uint32_t *)net.w + ((size_t)(row + t) << (4 * K));
#pragma unroll
        for (int g = 0; g < 8; g++)
            __hip_atomic_fetch_add(W + nt_index<K>(x, net.cells[8 * t + g]), (uint32_t)D, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct NtChoice {
    long long q[4];  // INT64_MIN: illegal
    uint32_t legal, best;
};

template <int K, bool S>
__device__ __forceinline__ NtChoice nt_choose(const NtArgs &net, const uint4 &b) {
    NtChoice c;
    c.legal = 0u;
    c.best = 0xFFu;
    long long bq = INT64_MIN;
#pragma unroll
    for (uint32_t a = 0u; a < 4u; a++) {
        uint32_t pts, mx;
        const uint4 s = apply_move(b, a, pts, mx);
        c.q[a] = INT64_MIN;
        if (!eq4(s, b)) {
            c.q[a] = ((long long)pts << kFrac) + nt_value<K, S>(net, nt_pack(s));
            c.legal |= 1u << a;
            if (c.best == 0xFFu || c.q[a] > bq) {
                bq = c.q[a];
                c.best = a;
            }
        }
    }
    return c;
}

template <int K, bool S>
__global__ __launch_bounds__(256) void nt_value_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                       long long *__restrict__ value, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    value[i] = nt_value<K, S>(net, nt_pack(boards[i]));
}

template <int K, bool S>
__global__ __launch_bounds__(256) void nt_choose_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                        long long *__restrict__ q, uint8_t *__restrict__ legal,
                                                        uint8_t *__restrict__ best, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const NtChoice c = nt_choose<K, S>(net, boards[i]);
    if (q) {
        reinterpret_cast<longlong2 *>(q)[2u * i] = make_longlong2(c.q[0], c.q[1]);
        reinterpret_cast<longlong2 *>(q)[2u * i + 1u] = make_longlong2(c.q[2], c.q[3]);
    }
    if (legal) legal[i] = (uint8_t)c.legal;
    if (best) best[i] = (uint8_t)c.best;
}

// stage[i] = stage(boards[i]); a one-stage net (map 0) gives 0
__global__ __launch_bounds__(256) void nt_stage_kernel(uint64_t stage_map, const uint4 *__restrict__ boards,
                                                       uint8_t *__restrict__ stage, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    stage[i] = (uint8_t)nt_stage(stage_map, nt_pack(boards[i]));
}

// Promotion: to[j] += from[j] (int32, wrapping) over the `quads` 16-byte words of one stage's tables, a
// grid-stride loop of 16-byte loads and stores; the two stages are different, so the ranges are disjoint
constexpr unsigned kPromoteBlocks = 2048;  // 8 workgroups of 256 lanes per compute unit
__global__ __launch_bounds__(256) void nt_promote_kernel(const uint4 *__restrict__ from, uint4 *__restrict__ to,
                                                         uint32_t quads) {
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < quads; j += gridDim.x * 256u) {
        const uint4 f = from[j];
        uint4 t = to[j];
        t.x += f.x;
        t.y += f.y;
        t.z += f.z;
        t.w += f.w;
        to[j] = t;
    }
}

// Optimistic initialisation: w[j] = w0 over the `quads` 16-byte words of all the tables of a net, in
// nt_promote_kernel's shape.  A net of 16 stages of eight 6-tuples has 2^29 words, so the index is 64 bits wide:
// j + stride must not wrap, whatever the grid (nt_fill launches one that covers the words in one pass)
__global__ __launch_bounds__(256) void nt_fill_kernel(uint4 *__restrict__ w, uint32_t w0, uint64_t quads) {
    const uint4 v = make_uint4(w0, w0, w0, w0);
    for (uint64_t j = blockIdx.x * 256u + threadIdx.x; j < quads; j += (uint64_t)gridDim.x * 256u) w[j] = v;
}

// Promotion over a start: to[j] += from[j] - base (int32, wrapping), nt_promote_kernel with the tables' common
// start taken off what is added, so that a stage still at `base` becomes a copy of `from`
__global__ __launch_bounds__(256) void nt_promote_from_kernel(const uint4 *__restrict__ from, uint4 *__restrict__ to,
                                                              uint32_t base, uint32_t quads) {
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < quads; j += gridDim.x * 256u) {
        const uint4 f = from[j];
        uint4 t = to[j];
        t.x += f.x - base;
        t.y += f.y - base;
        t.z += f.z - base;
        t.w += f.w - base;
        to[j] = t;
    }
}

// Tile-downgrading (Tile-downgrading of include/g2048_ntuple.h): one board per lane, in nt_stage_kernel's shape.
// The 16 bytes give the presence mask P (bit u for a cell 1 <= u <= 31); a round finds the largest tile m and the
// largest absent value j in [lo, m) by clz on the mask, moves the mask's bits above j down by one and takes one
// off every byte with j < u <= 31 of the four words (a carry-free byte-wise compare: bit 7 of (u & 0x7F) + 0x7F - j
// is u > j for u <= 127, and `small` marks the bytes <= 31, which a round never changes).  boards and out may be
// the same array, so neither is __restrict__: a lane reads its board before it writes it, and no other lane's.
__global__ __launch_bounds__(256) void nt_downgrade_kernel(const uint4 *boards, uint4 *out, uint8_t *__restrict__ shift,
                                                           uint32_t n, uint32_t from_exp, uint32_t lo_exp,
                                                           uint32_t rounds) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 b = boards[i];
    uint32_t w[4] = {b.x, b.y, b.z, b.w};
    uint32_t small[4];  // 0x01 in every byte <= 31
    uint32_t mask = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t hi = w[k] & 0xE0E0E0E0u;
        small[k] = (~(((hi & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | hi) & 0x80808080u) >> 7;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t u = (w[k] >> (8 * c)) & 0xFFu;
            mask |= u < 32u ? 1u << u : 0u;
        }
    }
    mask &= ~1u;  // an empty cell is no value
    uint32_t done = 0u;
    for (; done < rounds; done++) {
        if (mask == 0u) break;
        const uint32_t m = 31u - (uint32_t)__clz((int)mask);
        if (m < from_exp) break;
        const uint32_t absent = ~mask & ((1u << m) - 1u) & ~((1u << lo_exp) - 1u);  // lo <= j < m, not in P
        if (absent == 0u) break;
        const uint32_t j = 31u - (uint32_t)__clz((int)absent);  // 1 <= j <= 30
        mask = (mask & ((1u << j) - 1u)) | ((mask >> (j + 1u)) << j);
        const uint32_t add = (0x7Fu - j) * 0x01010101u;
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] -= ((((w[k] & 0x7F7F7F7Fu) + add) >> 7) & small[k]);
    }
    out[i] = make_uint4(w[0], w[1], w[2], w[3]);
    if (shift) shift[i] = (uint8_t)done;
}

// The carousel's kernel arguments (Carousel of include/g2048_ntuple.h), last in the list of the two kernels
// that take them; the `false` form is empty, as NtTcArgs / NtTraceArgs below
template <bool C>
struct NtCarArgs;
template <>
struct NtCarArgs<true> {
    uint4 *pool;                  // [G][n]
    uint8_t *valid;               // [n][16]
    uint8_t *next, *origin;       // [n]
    uint8_t *ws_stage;            // [n]: the start stage the reading kernel chose, 0: the reset
    uint4 *ws_board;              // [n]: the donor board, written where ws_stage != 0
    uint64_t ct;                  // rng->counter + t
    const uint64_t *counter_dev;  // nullable
};
template <>
struct NtCarArgs<false> {
    NtCarArgs(const NtCarArgs<true> &) {}
};

// bit k of the result: byte k of w is not 0
__device__ __forceinline__ uint32_t nt_nonzero_bytes(uint32_t w) {
    return ((w & 0xFFu) != 0u ? 1u : 0u) | ((w & 0xFF00u) != 0u ? 2u : 0u) | ((w & 0xFF0000u) != 0u ? 4u : 0u) |
           ((w & 0xFF000000u) != 0u ? 8u : 0u);
}

// Step 3c's choice, in the reading kernel: the donor slot j = (i + c + t) mod n, the sum modulo 2^64, and the
// first stage at or after next[i] that the slot holds; k = 0, and a slot without such a stage, is the reset.
// One 16-byte load brings the 16 flags of the slot.  The donor board is loaded only in the lanes that found a
// stage, not unconditionally from row max(g, 1): that row does not exist in the pool of a one-stage net, and
// the lanes at k = 0 (one in G) and those on an empty slot then move no board at all.  The branch costs one
// test per wave; the lanes behind it issue one 16-byte load and one 16-byte store.
__device__ __forceinline__ void nt_car_choose(const NtArgs &net, const NtCarArgs<true> &car, uint32_t n, uint32_t i) {
    const uint64_t s = car.ct + (car.counter_dev ? *car.counter_dev : 0ull);
    const uint32_t j = (uint32_t)((s + (uint64_t)i) % (uint64_t)n);
    const uint32_t G = (uint32_t)net.G;
    uint32_t k = car.next[i];
    k = k < G ? k : 0u;
    const uint4 f = reinterpret_cast<const uint4 *>(car.valid)[j];
    uint32_t m = nt_nonzero_bytes(f.x) | (nt_nonzero_bytes(f.y) << 4) | (nt_nonzero_bytes(f.z) << 8) |
                 (nt_nonzero_bytes(f.w) << 12);
    m &= ((1u << G) - 1u) & ~((1u << k) - 1u) & ~1u;  // stages max(k, 1) .. G - 1
    const uint32_t g = (k != 0u && m != 0u) ? (uint32_t)__builtin_ctz(m) : 0u;
    car.ws_stage[i] = (uint8_t)g;
    if (g != 0u) car.ws_board[i] = car.pool[(size_t)g * n + j];
}

// TD step, the reading half: the greedy action of the board and the D of the pending after-state (C: and the
// carousel's choice for a game that ends in this step)
template <int K, bool S, bool C>
__global__ __launch_bounds__(256) void nt_td_eval_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                         const uint4 *__restrict__ after,
                                                         const uint8_t *__restrict__ pending, int lr_shift,
                                                         int32_t *__restrict__ ws_d, uint8_t *__restrict__ ws_act,
                                                         uint32_t n, NtCarArgs<C> car) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const NtChoice c = nt_choose<K, S>(net, boards[i]);
    long long target = 0;
#pragma unroll
    for (uint32_t a = 0u; a < 4u; a++) target = c.best == a ? c.q[a] : target;
    const uint32_t p = pending[i];
    long long D = 0;
    if (p != 0u) {
        const long long delta = (p == 2u ? 0 : target) - nt_value<K, S>(net, nt_pack(after[i]));
        D = (delta + (1ll << (lr_shift - 1))) >> lr_shift;
        D = D < -kMaxD ? -kMaxD : D > kMaxD ? kMaxD : D;
    }
    ws_d[i] = (int32_t)D;
    ws_act[i] = (uint8_t)c.best;
    if constexpr (C) nt_car_choose(net, car, n, i);
}

// The end of a step's last launch, the same for both learners: g2048_env_step of env i with the greedy
// action and auto-reset at counter c + t, the running score, the finished game's statistics, and the
// carried state (after, pending).  C, the carousel: a board that enters a stage goes into the env's own pool
// slot of that stage (a 16-byte store and a flag byte, in those lanes only), and a game that ends is
// accounted by its origin and restarts from what the reading kernel chose.
template <bool C>
__device__ __forceinline__ void nt_step_env(const NtArgs &net, uint4 *boards, uint4 *after, uint8_t *pending,
                                            long long *run_score, const uint8_t *ws_act, RngArgs rng, uint64_t t,
                                            long long *stats, uint32_t n, uint32_t i, const NtCarArgs<C> &car) {
    const uint32_t act = ws_act[i];
    const bool has_move = act != 0xFFu;
    const uint32_t a = has_move ? act : 0u;
    uint4 b = boards[i];
    [[maybe_unused]] const uint4 before = b;
    uint32_t pts, mx;
    const uint4 moved = apply_move(b, a, pts, mx);
    const StepResult res = step_board<G2048_RNG_PHILOX>(b, true, a, nullptr, rng, (int64_t)i, rng_counter(rng) + t,
                                                        G2048_OPT_AUTO_RESET);
    long long rs = run_score[i] + (long long)res.pts;
    const bool done = (res.fl & FLAG_DONE) != 0u;
    if constexpr (C) {
        const uint32_t g1 = nt_stage(net.stage_map, nt_pack(b));
        if (!done && g1 != nt_stage(net.stage_map, nt_pack(before))) {  // the stage only grows inside a game: g1 >= 1
            car.pool[(size_t)g1 * n + i] = b;
            car.valid[16u * (size_t)i + g1] = (uint8_t)1;
            if (stats) __hip_atomic_fetch_add(stats + 6, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (done) {
        bool full = true;  // a game from the ordinary reset
        if constexpr (C) full = car.origin[i] == (uint8_t)0;
        if (stats) {
            if (full) {
                __hip_atomic_fetch_add(stats + 0, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(stats + 1, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(stats + 2, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_fetch_add(stats + 4, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(stats + 5, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        rs = 0;
        if constexpr (C) {
            const uint32_t g = car.ws_stage[i];
            if (g != 0u) {
                b = car.ws_board[i];
                if (stats) __hip_atomic_fetch_add(stats + 7, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            car.origin[i] = (uint8_t)g;
            car.next[i] = (uint8_t)(g + 1u == (uint32_t)net.G ? 0u : g + 1u);
        }
    }
    run_score[i] = rs;
    boards[i] = b;
    if (has_move) after[i] = moved;
    pending[i] = (uint8_t)(has_move ? (done ? 2u : 1u) : 0u);
}

// one add per wave of its updates applied; every lane of the wave calls it
__device__ __forceinline__ void nt_count_updates(long long *stats, bool updated) {
    if (stats) {
        const unsigned long long m = __ballot(updated);
        if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m))
            __hip_atomic_fetch_add(stats + 3, (long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// add_i of the TC step: what a weight with the record (E, A) takes of D (include/g2048_ntuple.h)
// Without a branch on A, so that both words of a record are always used and its gather stays one load.
__device__ __forceinline__ int32_t nt_tc_share(long long E, unsigned long long A, int32_t D) {
    const int sh = max(44 - (int)__clzll((long long)A), 0);  // bitlen(A) - 20; __clzll(0) = 64
    const uint32_t a = (uint32_t)(A >> sh);                   // A != 0: 1 <= a < 2^20
    const unsigned long long mag = E < 0 ? 0ull - (unsigned long long)E : (unsigned long long)E;
    const unsigned long long e = min(mag >> sh, (unsigned long long)a);
    const uint32_t absD = D < 0 ? 0u - (uint32_t)D : (uint32_t)D;
    const uint32_t q = (uint32_t)(((unsigned long long)absD * e + (a >> 1)) / max(a, 1u));  // below 2^51; q <= |D|
    return A == 0ull ? D : D < 0 ? -(int32_t)q : (int32_t)q;
}

typedef long long NtRecord __attribute__((ext_vector_type(2)));  // (E, A): one 16-byte load, not two of 8

// TC, to W: the accumulator records of the 8 T weights of x are read (one 16-byte gather each, the 8 of a
// tuple issued together) and each weight takes its share of D.  E and A are only read here.
template <int K, bool S>
__device__ __forceinline__ void nt_tc_share_add(const NtArgs &net, const NtRecord *tc, uint64_t x, int32_t D) {
    const uint32_t row = nt_row<S>(net, x);
    for (int t = 0; t < net.T; t++) {
        const size_t base = (size_t)(row + t) << (4 * K);
        uint32_t idx[8];
        NtRecord r[8];
#pragma unroll
        for (int g = 0; g < 8; g++) {
            idx[g] = nt_index<K>(x, net.cells[8 * t + g]);
            r[g] = tc[base + idx[g]];
        }
#pragma unroll
        for (int g = 0; g < 8; g++)
            __hip_atomic_fetch_add((uint32_t *)net.w + base + idx[g],
                                   (uint32_t)nt_tc_share(r[g].x, (unsigned long long)r[g].y, D), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// TC, to the records: D to E and |D| to A of the same 8 T records (64-bit atomics)
template <int K, bool S>
__device__ __forceinline__ void nt_tc_record_add(const NtArgs &net, unsigned long long *tc, uint64_t x, int32_t D) {
    const unsigned long long dE = (unsigned long long)(long long)D, dA = D < 0 ? 0ull - dE : dE;
    const uint32_t row = nt_row<S>(net, x);
    for (int t = 0; t < net.T; t++) {
        unsigned long long *rec = tc + ((size_t)(row + t) << (4 * K + 1));
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const size_t k = (size_t)nt_index<K>(x, net.cells[8 * t + g]) << 1;
            __hip_atomic_fetch_add(rec + k, dE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(rec + k + 1, dA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the trace (g2048_ntuple_lambda, trace_len > 0): the D of after[i] also goes, shifted right by k s, to
// the after-state k moves older of the same game, k = 1 .. hist_len[i] <= h, out of hist [h][n] boards.
// A lane loads its h rows of hist once, before any store, and only the step's last launch moves them on,
// after its adds.

constexpr int kMaxTrace = G2048_NT_MAX_TRACE;

struct NtTrace {
    uint64_t x[kMaxTrace + 1];  // s_0 = after[i], s_k = hist[k - 1][i], packed
    uint4 rows[kMaxTrace];      // hist[k][i] as loaded
    uint4 after;
    uint32_t len;               // hist_len[i], at most h
};

// rows at or past h are never read from memory; rows in len .. h - 1 are, and are not used
__device__ __forceinline__ NtTrace nt_trace_load(const uint4 *after, const uint4 *hist, const uint8_t *hist_len, int h,
                                                 uint32_t n, uint32_t i) {
    NtTrace tr;
    tr.after = after[i];
    tr.x[0] = nt_pack(tr.after);
    tr.len = h > 0 ? min((uint32_t)hist_len[i], (uint32_t)h) : 0u;
#pragma unroll
    for (int k = 0; k < kMaxTrace; k++) {
        tr.rows[k] = k < h ? hist[(size_t)k * n + i] : make_uint4(0u, 0u, 0u, 0u);
        tr.x[k + 1] = nt_pack(tr.rows[k]);
    }
    return tr;
}

// D_k = sign(D) (|D| >> k s): rounds towards zero, symmetrically; k s <= 28
__device__ __forceinline__ int32_t nt_decay(int32_t D, int ks) {
    const uint32_t m = (D < 0 ? 0u - (uint32_t)D : (uint32_t)D) >> ks;
    return D < 0 ? -(int32_t)m : (int32_t)m;
}

// Step 4 of the lambda step, before nt_step_env overwrites after[i]: the history moves on by the old
// after[i] when that one waited inside its game (p == 1) and a move follows it; otherwise it empties.
__device__ __forceinline__ void nt_trace_store(const NtTrace &tr, uint4 *hist, uint8_t *hist_len, int h, uint32_t p,
                                               bool has_move, uint32_t n, uint32_t i) {
    if (h <= 0) return;
    const bool push = has_move && p == 1u;
    const uint32_t len = push ? min(tr.len + 1u, (uint32_t)h) : 0u;
    if (push) {
#pragma unroll
        for (int k = kMaxTrace - 1; k >= 1; k--)
            if ((uint32_t)k < len) hist[(size_t)k * n + i] = tr.rows[k - 1];
        hist[i] = tr.after;
    }
    hist_len[i] = (uint8_t)len;
}

// f(s_k, D_k) for k = 0 .. tr.len with D_k != 0, k the outer loop, unrolled
template <typename F>
__device__ __forceinline__ void nt_for_trace(const NtTrace &tr, int32_t D, int s, F f) {
#pragma unroll
    for (int k = 0; k <= kMaxTrace; k++) {
        const int32_t Dk = nt_decay(D, k * s);
        if ((uint32_t)k <= tr.len && Dk != 0) f(tr.x[k], Dk);
    }
}

// The optional kernel arguments, last in the list: the `false` ones are empty and take what the `true`
// ones take, so that a launch site is written once
template <bool TC>
struct NtTcArgs {
    NtTcArgs(int64_t *) {}
};
template <>
struct NtTcArgs<true> {
    int64_t *tc;  // [G][T][16^K][2]
};
template <bool L>
struct NtTraceArgs {
    NtTraceArgs(int8_t *, uint8_t *, int, int) {}
};
template <>
struct NtTraceArgs<true> {
    int8_t *hist;
    uint8_t *hist_len;
    int h, s;
};

// The launch between the two others, rule TC only: each weight of the pending after-state (L: and of the
// s_k of its trace) takes its share of D (D_k).  It writes W only; the records are only added to in the next
// launch and hist only moves on there, so every lane sees both as they were before the step.
template <int K, bool S, bool L>
__global__ __launch_bounds__(256) void nt_tc_weights_kernel(NtArgs net, const NtRecord *__restrict__ tc,
                                                            const uint4 *__restrict__ after,
                                                            const uint8_t *__restrict__ pending,
                                                            const int32_t *__restrict__ ws_d, uint32_t n,
                                                            NtTraceArgs<L> trace) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t D = ws_d[i];
    if (pending[i] == 0u || D == 0) return;
    if constexpr (L) {
        const NtTrace tr = nt_trace_load(after, (const uint4 *)trace.hist, trace.hist_len, trace.h, n, i);
        nt_for_trace(tr, D, trace.s, [&](uint64_t x, int32_t Dk) __attribute__((always_inline)) {
            nt_tc_share_add<K, S>(net, tc, x, Dk);
        });
    } else {
        nt_tc_share_add<K, S>(net, tc, nt_pack(after[i]), D);
    }
}

// A step's last launch: D (L: D_k) of the pending after-state (of s_k) to its 8 T weights, or under TC to
// their records; then the history (L) and the env step (C: with the carousel's snapshot and restart)
template <int K, bool S, bool L, bool TC, bool C>
__global__ __launch_bounds__(256) void nt_update_kernel(NtArgs net, uint4 *__restrict__ boards,
                                                        uint4 *__restrict__ after, uint8_t *__restrict__ pending,
                                                        long long *__restrict__ run_score,
                                                        const int32_t *__restrict__ ws_d,
                                                        const uint8_t *__restrict__ ws_act, RngArgs rng, uint64_t t,
                                                        long long *__restrict__ stats, uint32_t n, NtTcArgs<TC> tc,
                                                        NtTraceArgs<L> trace, NtCarArgs<C> car) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < n;
    bool updated = false;
    if (valid) {
        const uint32_t p = pending[i];
        const int32_t D = ws_d[i];
        updated = p != 0u;
        const auto add = [&](uint64_t x, int32_t Dk) __attribute__((always_inline)) {
            if constexpr (TC)
                nt_tc_record_add<K, S>(net, (unsigned long long *)tc.tc, x, Dk);
            else
                nt_add<K, S>(net, x, Dk);
        };
        if constexpr (L) {
            const NtTrace tr = nt_trace_load(after, (const uint4 *)trace.hist, trace.hist_len, trace.h, n, i);
            if (updated) nt_for_trace(tr, D, trace.s, add);
            nt_trace_store(tr, (uint4 *)trace.hist, trace.hist_len, trace.h, p, ws_act[i] != 0xFFu, n, i);
        } else if (updated && D != 0) {
            add(nt_pack(after[i]), D);
        }
        nt_step_env<C>(net, boards, after, pending, run_score, ws_act, rng, t, stats, n, i, car);
    }
    nt_count_updates(stats, updated);
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
size_t td_workspace_bytes(int64_t n) { return align16((size_t)n * 4) + align16((size_t)n); }
// behind the TD step's workspace: the chosen start stage, a byte, and the donor board of every env
size_t car_workspace_bytes(int64_t n) { return td_workspace_bytes(n) + align16((size_t)n) + (size_t)n * 16; }

}  // namespace

extern "C" {

// nt_call_<call>(stream, net, stage_map, ...): the body of g2048_ntuple_<call> (stage_map 0) and of its twin
// g2048_ntuple_staged_<call>, both at the end of the file; the three learning calls share nt_call_step

size_t g2048_ntuple_weight_count(const g2048_ntuple_net *net) {
    NtArgs a;
    if (!make_args(net, 0, a)) return 0;
    return (size_t)net->num_tuples << (4 * net->tuple_len);
}

size_t g2048_ntuple_staged_weight_count(const g2048_ntuple_staged_net *snet) {
    NtArgs a;
    if (!snet || !make_args(&snet->net, snet->stage_map, a)) return 0;
    return ((size_t)a.G * snet->net.num_tuples) << (4 * snet->net.tuple_len);
}

int g2048_ntuple_stage(g2048_stream_t stream, const g2048_ntuple_staged_net *snet, const int8_t *boards,
                       uint8_t *stage, int64_t n) {
    NtArgs a;
    if (!snet || !make_args(&snet->net, snet->stage_map, a) || n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !stage) return G2048_EINVAL;
    hipLaunchKernelGGL(nt_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       a.stage_map, (const uint4 *)boards, stage, (uint32_t)n);
    return launch_status();
}

int g2048_ntuple_promote(g2048_stream_t stream, const g2048_ntuple_staged_net *snet, int32_t from, int32_t to) {
    NtArgs a;
    if (!snet || !make_args(&snet->net, snet->stage_map, a)) return G2048_EINVAL;
    if (from < 0 || from >= a.G || to < 0 || to >= a.G || from == to) return G2048_EINVAL;
    const size_t quads = ((size_t)snet->net.num_tuples << (4 * snet->net.tuple_len)) / 4;  // at most 2^25: K >= 1, a multiple of 4
    const uint4 *w = (const uint4 *)a.w;
    const unsigned blocks = (unsigned)((quads + 255) / 256 < kPromoteBlocks ? (quads + 255) / 256 : kPromoteBlocks);
    hipLaunchKernelGGL(nt_promote_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w + (size_t)from * quads,
                       (uint4 *)a.w + (size_t)to * quads, (uint32_t)quads);
    return launch_status();
}

int g2048_ntuple_promote_from(g2048_stream_t stream, const g2048_ntuple_staged_net *snet, int32_t from, int32_t to,
                              int32_t base) {
    NtArgs a;
    if (!snet || !make_args(&snet->net, snet->stage_map, a)) return G2048_EINVAL;
    if (from < 0 || from >= a.G || to < 0 || to >= a.G || from == to) return G2048_EINVAL;
    const size_t quads = ((size_t)snet->net.num_tuples << (4 * snet->net.tuple_len)) / 4;  // as g2048_ntuple_promote
    const uint4 *w = (const uint4 *)a.w;
    const unsigned blocks = (unsigned)((quads + 255) / 256 < kPromoteBlocks ? (quads + 255) / 256 : kPromoteBlocks);
    hipLaunchKernelGGL(nt_promote_from_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       w + (size_t)from * quads, (uint4 *)a.w + (size_t)to * quads, (uint32_t)base, (uint32_t)quads);
    return launch_status();
}

// w[j] = w0 for the `count` weights of a net make_args accepted: a multiple of 4, at most 2^31.  The grid covers
// the tables in one pass (at most 2^21 workgroups): a store-only loop over kPromoteBlocks resident workgroups
// wrote 256 MB in 46.7 us and 1 GB in 241.7 us on an MI355X, this grid in 38.9 and 156.0 us, the times of
// torch.Tensor.fill_ (Optimistic initialisation)
static int nt_fill(g2048_stream_t stream, const NtArgs &a, size_t count, int32_t w0) {
    const uint64_t quads = count / 4;
    const unsigned blocks = (unsigned)((quads + 255) / 256);
    hipLaunchKernelGGL(nt_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4 *)a.w, (uint32_t)w0,
                       quads);
    return launch_status();
}

int g2048_ntuple_fill(g2048_stream_t stream, const g2048_ntuple_net *net, int32_t w0) {
    NtArgs a;
    if (!make_args(net, 0, a)) return G2048_EINVAL;
    return nt_fill(stream, a, (size_t)net->num_tuples << (4 * net->tuple_len), w0);
}

int g2048_ntuple_staged_fill(g2048_stream_t stream, const g2048_ntuple_staged_net *snet, int32_t w0) {
    NtArgs a;
    if (!snet || !make_args(&snet->net, snet->stage_map, a)) return G2048_EINVAL;
    return nt_fill(stream, a, ((size_t)a.G * snet->net.num_tuples) << (4 * snet->net.tuple_len), w0);
}

int g2048_ntuple_downgrade(g2048_stream_t stream, const int8_t *boards, int8_t *out, uint8_t *shift, int64_t n,
                           int32_t from_exp, int32_t lo_exp, int32_t rounds) {
    if (from_exp < 2 || from_exp > 31 || lo_exp < 1 || lo_exp >= from_exp || rounds < 1 || rounds > 16) return G2048_EINVAL;
    if (n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !out || !aligned16(out)) return G2048_EINVAL;
    hipLaunchKernelGGL(nt_downgrade_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint4 *)boards, (uint4 *)out, shift, (uint32_t)n, (uint32_t)from_exp, (uint32_t)lo_exp,
                       (uint32_t)rounds);
    return launch_status();
}

static int nt_call_value(g2048_stream_t stream, const g2048_ntuple_net *net, uint64_t stage_map, const int8_t *boards,
                         int64_t *value, int64_t n) {
    NtArgs a;
    if (!make_args(net, stage_map, a) || n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !value) return G2048_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    G2048_NT_DISPATCH(a, net->tuple_len, hipLaunchKernelGGL((nt_value_kernel<kK, kS>), grid, block, 0, (hipStream_t)stream, a,
                                                         (const uint4 *)boards, (long long *)value, (uint32_t)n));
    return launch_status();
}

static int nt_call_choose(g2048_stream_t stream, const g2048_ntuple_net *net, uint64_t stage_map, const int8_t *boards, int64_t *q,
                        uint8_t *legal, uint8_t *best, int64_t n) {
    NtArgs a;
    if (!make_args(net, stage_map, a) || n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (!q && !legal && !best) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !aligned16(q)) return G2048_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    G2048_NT_DISPATCH(a, net->tuple_len, hipLaunchKernelGGL((nt_choose_kernel<kK, kS>), grid, block, 0, (hipStream_t)stream, a,
                                                         (const uint4 *)boards, (long long *)q, legal, best,
                                                         (uint32_t)n));
    return launch_status();
}

size_t g2048_ntuple_td_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (int64_t(1) << 28)) return 0;
    return td_workspace_bytes(n < 1 ? 1 : n);
}

size_t g2048_ntuple_tc_workspace_bytes(int64_t n) { return g2048_ntuple_td_workspace_bytes(n); }
size_t g2048_ntuple_lambda_workspace_bytes(int64_t n) { return g2048_ntuple_td_workspace_bytes(n); }
size_t g2048_ntuple_carousel_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (int64_t(1) << 28)) return 0;
    return car_workspace_bytes(n < 1 ? 1 : n);
}

// The three learning calls: `steps` steps of eval, weights (tc != null: rule TC) and update, the two
// writing kernels with the trace where trace_len > 0.  g2048_ntuple_td comes with tc null, trace_len 0 and
// lambda_shift 1; hist and hist_len are looked at only where there is a trace.  carousel: the call is
// g2048_ntuple_staged_carousel, car is required and the two kernels that take it run in their S = true form
// whatever the map (with the map 0 that form computes what S = false computes).
static int nt_call_step(g2048_stream_t stream, const g2048_ntuple_net *net, uint64_t stage_map, int64_t *tc,
                        int8_t *boards, int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending,
                        int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len,
                        int32_t lambda_shift, const g2048_rng *rng, int64_t *stats, void *workspace,
                        size_t workspace_bytes_in, bool carousel = false, const g2048_ntuple_carousel *car = nullptr) {
    NtArgs a;
    if (!make_args(net, stage_map, a) || n < 0 || n >= (int64_t(1) << 28)) return G2048_EINVAL;
    if (steps < 1 || lr_shift < 1 || lr_shift > 30) return G2048_EINVAL;
    if (trace_len < 0 || trace_len > G2048_NT_MAX_TRACE || lambda_shift < 1 || lambda_shift > G2048_NT_MAX_LAMBDA_SHIFT)
        return G2048_EINVAL;
    if (!philox_mode(rng) || !counter_dev_aligned(rng)) return G2048_EINVAL;
    if (!aligned16(tc)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !after || !aligned16(after) || !pending || !run_score ||
        ((uintptr_t)run_score & 7u) || ((uintptr_t)stats & 7u) || !workspace || !aligned16(workspace) ||
        workspace_bytes_in < (carousel ? car_workspace_bytes(n) : td_workspace_bytes(n)))
        return G2048_EINVAL;
    if (trace_len > 0 && (!hist || !aligned16(hist) || !hist_len)) return G2048_EINVAL;
    if (carousel && (!car || !car->pool || !aligned16(car->pool) || !car->valid || !aligned16(car->valid) || !car->next ||
                     !car->origin))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int32_t *ws_d = (int32_t *)workspace;
    uint8_t *ws_act = (uint8_t *)workspace + align16((size_t)n * 4);
    NtCarArgs<true> ca{};
    if (carousel) {
        uint8_t *ws_stage = (uint8_t *)workspace + td_workspace_bytes(n);
        ca = NtCarArgs<true>{(uint4 *)car->pool, car->valid, car->next, car->origin, ws_stage,
                             (uint4 *)(ws_stage + align16((size_t)n)), 0, rng->counter_dev};
    }
    const RngArgs r = rng_args(rng);
    const int K = net->tuple_len, h = trace_len, ls = lambda_shift;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    for (int64_t t = 0; t < steps; t++) {
        ca.ct = rng->counter + (uint64_t)t;
        G2048_NT_DISPATCH_BOOL(carousel, kC, G2048_NT_DISPATCH(a, K,
            hipLaunchKernelGGL((nt_td_eval_kernel<kK, kS || kC, kC>), grid, block, 0, st, a, (const uint4 *)boards,
                               (const uint4 *)after, (const uint8_t *)pending, (int)lr_shift, ws_d, ws_act, (uint32_t)n,
                               NtCarArgs<kC>(ca))));
        int s = launch_status();
        if (s != G2048_OK) return s;
        if (tc) {
            G2048_NT_DISPATCH_BOOL(h > 0, kL, G2048_NT_DISPATCH(a, K,
                hipLaunchKernelGGL((nt_tc_weights_kernel<kK, kS, kL>), grid, block, 0, st, a, (const NtRecord *)tc,
                                   (const uint4 *)after, (const uint8_t *)pending, (const int32_t *)ws_d, (uint32_t)n,
                                   NtTraceArgs<kL>{hist, hist_len, h, ls})));
            s = launch_status();
            if (s != G2048_OK) return s;
        }
        G2048_NT_DISPATCH_BOOL(carousel, kC, G2048_NT_DISPATCH_BOOL(h > 0, kL, G2048_NT_DISPATCH_BOOL(tc != nullptr, kTC,
            G2048_NT_DISPATCH(a, K,
                hipLaunchKernelGGL((nt_update_kernel<kK, kS || kC, kL, kTC, kC>), grid, block, 0, st, a, (uint4 *)boards,
                                   (uint4 *)after, pending, (long long *)run_score, (const int32_t *)ws_d,
                                   (const uint8_t *)ws_act, r, (uint64_t)t, (long long *)stats, (uint32_t)n,
                                   NtTcArgs<kTC>{tc}, NtTraceArgs<kL>{hist, hist_len, h, ls}, NtCarArgs<kC>(ca))))));
        s = launch_status();
        if (s != G2048_OK) return s;
    }
    return G2048_OK;
}

// g2048_ntuple_tc has no TD form: it refuses a null tc, whatever n
static int nt_call_tc(g2048_stream_t stream, const g2048_ntuple_net *net, uint64_t stage_map, int64_t *tc,
                      int8_t *boards, int8_t *after, uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps,
                      int32_t lr_shift, const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes) {
    if (!tc) return G2048_EINVAL;
    return nt_call_step(stream, net, stage_map, tc, boards, after, nullptr, nullptr, pending, run_score, n, steps,
                        lr_shift, 0, 1, rng, stats, workspace, workspace_bytes);
}

// ---- the entry points: a one-stage call is its twin on a staged net with the map 0
#define NT_STAGED(net) ((net) ? &(net)->net : nullptr), ((net) ? (net)->stage_map : 0)

int g2048_ntuple_value(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *value,
                       int64_t n) {
    return nt_call_value(stream, net, 0, boards, value, n);
}
int g2048_ntuple_staged_value(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                              int64_t *value, int64_t n) {
    return nt_call_value(stream, NT_STAGED(net), boards, value, n);
}

int g2048_ntuple_choose(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *q,
                        uint8_t *legal, uint8_t *best, int64_t n) {
    return nt_call_choose(stream, net, 0, boards, q, legal, best, n);
}
int g2048_ntuple_staged_choose(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                               int64_t *q, uint8_t *legal, uint8_t *best, int64_t n) {
    return nt_call_choose(stream, NT_STAGED(net), boards, q, legal, best, n);
}

int g2048_ntuple_td(g2048_stream_t stream, const g2048_ntuple_net *net, int8_t *boards, int8_t *after,
                    uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                    const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes) {
    return nt_call_step(stream, net, 0, nullptr, boards, after, nullptr, nullptr, pending, run_score, n, steps,
                        lr_shift, 0, 1, rng, stats, workspace, workspace_bytes);
}
int g2048_ntuple_staged_td(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int8_t *boards, int8_t *after,
                           uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                           const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes) {
    return nt_call_step(stream, NT_STAGED(net), nullptr, boards, after, nullptr, nullptr, pending, run_score, n, steps,
                        lr_shift, 0, 1, rng, stats, workspace, workspace_bytes);
}

int g2048_ntuple_tc(g2048_stream_t stream, const g2048_ntuple_net *net, int64_t *tc, int8_t *boards, int8_t *after,
                    uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                    const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes) {
    return nt_call_tc(stream, net, 0, tc, boards, after, pending, run_score, n, steps, lr_shift, rng, stats, workspace,
                      workspace_bytes);
}
int g2048_ntuple_staged_tc(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                           int8_t *after, uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps,
                           int32_t lr_shift, const g2048_rng *rng, int64_t *stats, void *workspace,
                           size_t workspace_bytes) {
    return nt_call_tc(stream, NT_STAGED(net), tc, boards, after, pending, run_score, n, steps, lr_shift, rng, stats,
                      workspace, workspace_bytes);
}

int g2048_ntuple_lambda(g2048_stream_t stream, const g2048_ntuple_net *net, int64_t *tc, int8_t *boards, int8_t *after,
                        int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps,
                        int32_t lr_shift, int32_t trace_len, int32_t lambda_shift, const g2048_rng *rng, int64_t *stats,
                        void *workspace, size_t workspace_bytes) {
    return nt_call_step(stream, net, 0, tc, boards, after, hist, hist_len, pending, run_score, n, steps, lr_shift,
                        trace_len, lambda_shift, rng, stats, workspace, workspace_bytes);
}
int g2048_ntuple_staged_lambda(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                               int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score,
                               int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len, int32_t lambda_shift,
                               const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes) {
    return nt_call_step(stream, NT_STAGED(net), tc, boards, after, hist, hist_len, pending, run_score, n, steps,
                        lr_shift, trace_len, lambda_shift, rng, stats, workspace, workspace_bytes);
}

int g2048_ntuple_staged_carousel(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                                 int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score,
                                 int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len, int32_t lambda_shift,
                                 const g2048_rng *rng, const g2048_ntuple_carousel *car, int64_t *stats, void *workspace,
                                 size_t workspace_bytes) {
    return nt_call_step(stream, NT_STAGED(net), tc, boards, after, hist, hist_len, pending, run_score, n, steps,
                        lr_shift, trace_len, lambda_shift, rng, stats, workspace, workspace_bytes, true, car);
}

}  // extern "C"
