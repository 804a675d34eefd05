// mc_search.hip -- pure Monte-Carlo playout search (g2048_mc_search of include/g2048.h):
// mc_search_kernel plays, for every root board and every action, P random-legal games of at most D
// moves out of the kLine11 LDS table and sums their points per (board, action).  It is
// env_rollout_kernel's step (env_rollout.hip) without the trajectory record, the potentials and the
// auto-reset, built with the same flags.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "rowtable.hpp"
#include "line11_lds.hpp"
#include "step.hpp"
#include "launch_util.hpp"
#include "../../include/g2048.h"

using namespace g2048;

namespace {

// Every LDS address the kernel forms is that of a kLine11 record (8 idx, 8 bytes) with every digit
// of the line <= 10: the wave-uniform fast pair starts with every exponent of its playing lanes <= 8
// and a move adds at most 1 to the maximum, so its two steps index boards of exponents <= 9 and
// <= 10; every other step, and the refill after the forced move, zeroes the board it takes addresses
// from in the lanes that hold an exponent > 10 (their reads are discarded: those lanes move on the
// SWAR path from then on, a board's maximum never falls).
static_assert(8u + 1u + 1u <= kMaxLineDigit, "a fast pair (start <= 8) stays inside kLine11");

constexpr int64_t kMaxPlayouts = 4096, kMaxDepth = 65536;

// Per-lane state of one playout carried from step to step.
struct McLane {
    uint4 b;           // current board
    uint32_t legal;    // its legal mask (0: the playout is over)
    uint32_t M;        // its largest exponent (guards the table: > 10 moves on the SWAR path)
    uint2 R[4], C[4];  // the kLine11 records of its rows and columns (valid while M <= 10)
    uint32_t d0, d1;   // the current pair's two step words (words x / y of its stream-1 draw)
    PhiloxState ph;    // draw of the next pair, computed half per step inside the LDS round trip
    uint32_t score;    // points so far (the forced move's included)
    uint32_t moves;    // playout steps executed
};

// One playout step: rollout_step of env_rollout.hip (oracle or_step_word) without what only its
// trajectory record needs.  kOdd = the second step of the pair; kSmall = every playing lane of the
// wave holds a board inside the table for this step (no SWAR fallback, no address masking).
template <bool kOdd, bool kSmall>
__device__ __forceinline__ void mc_step(McLane &s, const uint32_t *__restrict__ tab, uint64_t seed, uint64_t next_pair,
                                        uint32_t env) {
    const uint32_t u = kOdd ? s.d1 : s.d0;
    const uint64_t pa = (uint64_t)u * (uint32_t)__popc(s.legal);
    const uint32_t a = kth_bit4(s.legal, (uint32_t)(pa >> 32)), r = (uint32_t)pa;
    // the move from the carried records: the columns' for UP / DOWN, the rows' otherwise; the
    // start-slid half for UP / LEFT, the end-slid one for DOWN / RIGHT
    const bool vert = a < 2u, rev = (a & 1u) != 0u;
    const uint32_t usel = rev ? kUnpackEndSel : kUnpackStartSel;
    const uint32_t e0 = vert ? s.C[0].x : s.R[0].x, e1 = vert ? s.C[1].x : s.R[1].x;
    const uint32_t e2 = vert ? s.C[2].x : s.R[2].x, e3 = vert ? s.C[3].x : s.R[3].x;
    const uint32_t h0 = vert ? s.C[0].y : s.R[0].y, h1 = vert ? s.C[1].y : s.R[1].y;
    const uint32_t h2 = vert ? s.C[2].y : s.R[2].y, h3 = vert ? s.C[3].y : s.R[3].y;
    const uint4 w = make_uint4(unpack_row(e0, usel), unpack_row(e1, usel), unpack_row(e2, usel), unpack_row(e3, usel));
    uint4 moved = sel4(vert, transpose(w), w);
    // merge points / 4 in bits 16..27 of each record's dword 1, the slid line's maximum in bits 28..31
    uint32_t pts = (((h0 >> 16) & 0xFFFu) + ((h1 >> 16) & 0xFFFu) + ((h2 >> 16) & 0xFFFu) + ((h3 >> 16) & 0xFFFu)) << 2;
    uint32_t Ma = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_elementwise_max(as_u16x2(h0), as_u16x2(h1)),
                                                                         __builtin_elementwise_max(as_u16x2(h2), as_u16x2(h3)))) >> 28;
    if (!kSmall && s.M > kMaxLineDigit) {  // an exponent outside the table: the SWAR compute path
        uint32_t mx;
        moved = apply_move(s.b, a, pts, mx);
        Ma = board_max(moved);
    }
    // spawn on the k-th empty cell (row-major), k = floor(r * empties / 2^32), value 1 if the low
    // word of r * empties is below 0.9 * 2^32
    const uint32_t Zm[4] = {zm(moved.x), zm(moved.y), zm(moved.z), zm(moved.w)};
    const uint32_t n0 = __popc(Zm[0]), n01 = __popc(Zm[1]) + n0, n012 = __popc(Zm[2]) + n01;
    const uint32_t empt_a = __popc(Zm[3]) + n012;
    const uint64_t prod = (uint64_t)r * empt_a;
    const uint32_t k = (uint32_t)(prod >> 32);
    const uint32_t v = (uint32_t)prod < kTwoThreshold ? 1u : 2u;
    const bool r1 = k >= n0, r2 = k >= n01, r3 = k >= n012;  // spawn row >= 1, >= 2, == 3
    const uint32_t kr = k - (r3 ? n012 : r2 ? n01 : r1 ? n0 : 0u);
    const uint32_t z = r3 ? Zm[3] : r2 ? Zm[2] : r1 ? Zm[1] : Zm[0];
    const uint32_t b0 = (z >> 7) & 1u, b01 = b0 + ((z >> 15) & 1u), b012 = b01 + ((z >> 23) & 1u);
    const uint32_t col = (uint32_t)(kr >= b0) + (uint32_t)(kr >= b01) + (uint32_t)(kr >= b012);
    const uint32_t bits = v << (8u * col);
    moved.x |= r1 ? 0u : bits;
    moved.y |= (r1 && !r2) ? bits : 0u;
    moved.z |= (r2 && !r3) ? bits : 0u;
    moved.w |= r3 ? bits : 0u;
    s.b = moved;  // the next board (after the spawn)
    // The step's one LDS round trip: the records of the next board's four rows and four columns (the
    // next move, whatever its direction, and this board's line sums).  Outside the fast pair a lane
    // holding an exponent > 10 takes its addresses from an empty board (its reads are discarded below).
    uint4 ab = moved;
    if (!kSmall) ab = sel4(Ma > kMaxLineDigit, make_uint4(0u, 0u, 0u, 0u), moved);
    uint32_t ra[4], ca[4];
    line11_addrs(ab, ra, ca);
    uint2 R0 = lds_rec(tab, ra[0]), R1 = lds_rec(tab, ra[1]), R2 = lds_rec(tab, ra[2]), R3 = lds_rec(tab, ra[3]);
    uint2 C0 = lds_rec(tab, ca[0]), C1 = lds_rec(tab, ca[1]), C2 = lds_rec(tab, ca[2]), C3 = lds_rec(tab, ca[3]);
    // half of the next pair's Philox rounds fill the round trip: the empty asm statements start them
    // after the table loads are issued (memory clobber) and consume the loaded entries after them
    asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3)::"memory");
    if constexpr (kOdd) philox_rounds<5, 10>(s.ph);
    else philox_rounds<0, 5>(s.ph);
    asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3), "+v"(R0.y), "+v"(R1.y), "+v"(R2.y), "+v"(R3.y),
                      "+v"(C0.y), "+v"(C1.y), "+v"(C2.y), "+v"(C3.y));
    // #lines that can move per direction in nibbles {UP, DOWN, LEFT, RIGHT} of the line-entry sums ->
    // legal bits 0..3 (rollout_step's gather)
    const uint32_t SR = R0.y + R1.y + R2.y + R3.y, SC = C0.y + C1.y + C2.y + C3.y;
    const uint32_t nl = __builtin_amdgcn_perm(SR, SC, 0x0C0C0501u);
    s.legal = (__umul24((nl + 0x7777u) & 0x8888u, 0x249u) >> 12) & 15u;
    if (!kSmall && Ma > kMaxLineDigit) s.legal = legal_mask(moved);  // an exponent outside kLine11
    s.R[0] = R0, s.R[1] = R1, s.R[2] = R2, s.R[3] = R3;
    s.C[0] = C0, s.C[1] = C1, s.C[2] = C2, s.C[3] = C3;
    s.M = max(Ma, v);
    s.score += pts;
    s.moves += 1u;
    if constexpr (kOdd) {
        s.d0 = s.ph.c0;
        s.d1 = s.ph.c1;
        s.ph = philox_start(seed, next_pair, env, 1u);
    }
}

// The playout of one lane from the board after its forced move (s.b, s.legal != 0, s.M set): up to
// `depth` steps, step t on word (c + t) & 1 of the stream-1 draw at counter (c + t) >> 1, stopped
// by the first step that leaves no legal move.  A lane leaves the loops at its own end; the wave
// leaves them when its last lane has.
__device__ __forceinline__ void mc_playout(McLane &s, const uint32_t *__restrict__ tab, uint64_t seed, uint64_t c,
                                           uint32_t env, int depth) {
    {   // the records of the board's lines; a lane holding an exponent > 10 reads the empty line's
        const uint4 ab = sel4(s.M > kMaxLineDigit, make_uint4(0u, 0u, 0u, 0u), s.b);
        uint32_t ra[4], ca[4];
        line11_addrs(ab, ra, ca);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s.R[i] = lds_rec(tab, ra[i]);
            s.C[i] = lds_rec(tab, ca[i]);
        }
    }
    uint64_t pair = c >> 1;
    const uint4 d = philox_draw(seed, pair, env, 1u);
    s.d0 = d.x;
    s.d1 = d.y;
    s.ph = philox_start(seed, pair + 1u, env, 1u);
    int t = 0;
    if (c & 1u) {  // the playout starts on the second step of a pair
        philox_rounds<0, 5>(s.ph);
        mc_step<true, false>(s, tab, seed, pair + 2u, env);
        pair++;
        t = 1;
    }
    for (; s.legal != 0u && t + 2 <= depth; t += 2, pair++) {
        // every playing board of the wave <= 2^8 at the pair's start: both steps stay inside kLine11
        if (__all(s.M < 9u)) {
            mc_step<false, true>(s, tab, seed, pair + 2u, env);
            if (s.legal == 0u) break;
            mc_step<true, true>(s, tab, seed, pair + 2u, env);
        } else {
            mc_step<false, false>(s, tab, seed, pair + 2u, env);
            if (s.legal == 0u) break;
            mc_step<true, false>(s, tab, seed, pair + 2u, env);
        }
    }
    if (s.legal != 0u && t < depth) mc_step<false, false>(s, tab, seed, pair + 2u, env);
}

// Lane L = (4 i + a) P + p plays playout p of action a on root board i (env id env_base + L).
// Workgroups are persistent over lanes (one LDS table per CU); a wave takes 64 consecutive lanes at
// a time, so its lanes form runs of equal (board, action) group.  Each run is summed inside the wave
// (segmented shuffle reduction) and its first lane adds the run's sums to score_sum / move_sum with
// one 64-bit atomic each -- integer addition, so the result does not depend on the order -- and
// then its lane count to the board's arrival counter (workspace, zero on entry).  The run that
// completes a board's 4 P lanes writes its legal mask and best action.
__global__ __launch_bounds__(1024) void mc_search_kernel(const uint4 *__restrict__ boards, uint32_t total,
                                                         uint32_t playouts, int depth, RngArgs rng,
                                                         unsigned long long *__restrict__ score_sum,
                                                         unsigned long long *__restrict__ move_sum,
                                                         uint8_t *__restrict__ legal_out, uint8_t *__restrict__ best_out,
                                                         uint32_t *__restrict__ arrived) {
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kRolloutLdsWords];
    stage_row_table(s_row);
    const uint64_t ctr0 = rng_counter(rng);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * blockDim.x;  // total < 2^31, stride <= 2^18: L0 + stride fits
    for (uint32_t L0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); L0 < total; L0 += stride) {
        const uint32_t L = L0 + lane;
        const bool valid = L < total;
        uint32_t g = 0xFFFFFFFFu, p = 0u;  // the lane's (board, action) group 4 i + a and playout
        uint32_t score = 0u, moves = 0u;
        if (valid) {
            g = L / playouts;
            p = L - g * playouts;
            const uint4 root = boards[g >> 2];
            uint32_t pts0, mx0;
            uint4 moved = apply_move(root, g & 3u, pts0, mx0);
            if (!eq4(moved, root)) {  // the forced move: step_board with a policy action (stream 0 at ctr0)
                const uint32_t env = rng.env_base + L;
                const uint4 ph = philox_draw(rng.seed, ctr0, env, 0u);
                spawn<G2048_RNG_PHILOX>(moved, ph.x, ph.y, nullptr, rng, (int64_t)L);
                McLane s;
                s.b = moved;
                s.legal = legal_mask(moved);
                s.M = board_max(moved);
                s.score = pts0;
                s.moves = 0u;
                if (s.legal != 0u && depth > 0) mc_playout(s, s_row, rng.seed, ctr0, env, depth);
                score = s.score;
                moves = s.moves;
            }
        }
        // sums over each run of equal g (runs are contiguous: after the step of offset d a lane
        // holds the sum over the lanes [l, l + 2d) of its run)
        unsigned long long sc = score;
        uint32_t mv = moves;
#pragma unroll
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const unsigned long long osc = __shfl_down(sc, off);
            const uint32_t omv = __shfl_down(mv, off), og = __shfl_down(g, off);
            if (lane + off < 64u && og == g) {
                sc += osc;
                mv += omv;
            }
        }
        if (valid && (p == 0u || lane == 0u)) {  // the first lane of a run
            const uint32_t len = min(min(playouts - p, 64u - lane), total - L);
            const uint32_t i = g >> 2;
            __hip_atomic_fetch_add(score_sum + g, sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (move_sum) __hip_atomic_fetch_add(move_sum + g, (unsigned long long)mv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // release: the sums above are performed before the arrival; acquire: the run that completes
            // the board reads every other run's sums
            const uint32_t before = __hip_atomic_fetch_add(arrived + i, len, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (before + len == 4u * playouts && (legal_out || best_out)) {
                const uint32_t lg = legal_mask(boards[i]);
                uint32_t best = 0xFFu;
                long long bs = 0;
                for (uint32_t a = 0u; a < 4u; a++) {
                    const long long v = (long long)__hip_atomic_load(score_sum + 4u * i + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((lg >> a) & 1u) && (best == 0xFFu || v > bs)) {
                        best = a;
                        bs = v;
                    }
                }
                if (legal_out) legal_out[i] = (uint8_t)lg;
                if (best_out) best_out[i] = (uint8_t)best;
            }
        }
    }
}

// the call's own zero-fill of what mc_search_kernel accumulates into: the sums ([n][4] 64-bit words
// each, move_sum nullable) and the n arrival counters
__global__ __launch_bounds__(256) void mc_zero_kernel(unsigned long long *__restrict__ score_sum,
                                                      unsigned long long *__restrict__ move_sum,
                                                      uint32_t *__restrict__ arrived, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 z = make_ulonglong2(0ull, 0ull);
    reinterpret_cast<ulonglong2 *>(score_sum)[2u * i] = z;
    reinterpret_cast<ulonglong2 *>(score_sum)[2u * i + 1u] = z;
    if (move_sum) {
        reinterpret_cast<ulonglong2 *>(move_sum)[2u * i] = z;
        reinterpret_cast<ulonglong2 *>(move_sum)[2u * i + 1u] = z;
    }
    arrived[i] = 0u;
}

size_t workspace_bytes(int64_t n) { return (size_t)((n < 1 ? 1 : n) * 4 + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

size_t g2048_mc_search_workspace_bytes(int64_t n, int64_t playouts) {
    (void)playouts;  // one arrival counter per root board, whatever the playout count
    if (n < 0 || n >= (int64_t(1) << 31)) return 0;
    return workspace_bytes(n);
}

int g2048_mc_search(g2048_stream_t stream, const int8_t *boards, int64_t n, int64_t playouts, int64_t depth,
                    const g2048_rng *rng, int64_t *score_sum, int64_t *move_sum, uint8_t *legal, uint8_t *best,
                    void *workspace, size_t workspace_bytes_in) {
    if (!rng || rng->mode != G2048_RNG_PHILOX) return G2048_EINVAL;
    if (playouts < 1 || playouts > kMaxPlayouts || depth < 0 || depth > kMaxDepth) return G2048_EINVAL;
    if (n < 0 || n >= (int64_t(1) << 31) || n * 4 * playouts >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !score_sum || ((uintptr_t)score_sum & 15u) || ((uintptr_t)move_sum & 15u) ||
        !workspace || ((uintptr_t)workspace & 3u) || workspace_bytes_in < workspace_bytes(n) ||
        (rng->counter_dev && ((uintptr_t)rng->counter_dev & 7u)))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (unsigned long long *)score_sum, (unsigned long long *)move_sum, (uint32_t *)workspace,
                       (uint32_t)n);
    const int zs = launch_status();
    if (zs != G2048_OK) return zs;
    // one workgroup per CU holds the LDS table; its size scales with the lane count up to 1024
    // threads, as env_rollout_kernel's does with its board count
    const int64_t total = n * 4 * playouts;
    int64_t threads = (total + 255) / 256;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : ((threads + 63) / 64) * 64;
    int64_t grid = (total + threads - 1) / threads;
    grid = grid > 256 ? 256 : grid;
    hipLaunchKernelGGL(mc_search_kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, st, (const uint4 *)boards,
                       (uint32_t)total, (uint32_t)playouts, (int)depth, rng_args(rng),
                       (unsigned long long *)score_sum, (unsigned long long *)move_sum, legal, best,
                       (uint32_t *)workspace);
    return launch_status();
}

}  // extern "C"
