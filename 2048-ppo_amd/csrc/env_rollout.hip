// env_rollout.hip -- the synthetic random-legal rollout (the bench's headline workload,
// g2048_env_rollout_random / _adv of include/g2048.h): env_rollout_kernel with its per-step helpers
// (the LDS tables and their staging are line11_lds.hpp's, shared with mc_search.hip), in a
// translation unit of its own so that it alone is built with the machine scheduler's occupancy bias
// at 0 (Makefile: one wave per SIMD at the benchmark size, where the issue schedule, not occupancy,
// sets the step time; the rest of libg2048 keeps the default bias).
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

// Every LDS address the kernel forms:
//  - a kLine11 record at 8 idx (8 bytes, or the u16 at + 4) with every digit of the line <= 10.  The
//    wave-uniform fast pair starts with every exponent <= 8 and a move adds at most 1 to the maximum,
//    so its two steps index boards of exponents <= 9 and <= 10; every other step zeroes the board it
//    takes addresses from in the lanes that hold an exponent > 10 (their reads are discarded), and
//    the spawn's pre-spawn lines are the post-spawn ones minus the spawned digit.
static_assert(8u + 1u + 1u <= kMaxLineDigit, "a fast pair (start <= 8) stays inside kLine11");
//  - the kFreshLines addresses (<= kFreshLineAddrMax, checked entry by entry above), which reset_reload
//    reads in the lanes whose game ended
static_assert(lut::kFreshLineAddrMax + 8u <= kLineLdsBytes, "fresh boards' line records inside kLine11");
//  - a kFresh record i <= 959 (60 p1 + 4 k2 + 3, p1 <= 15, k2 <= 14): 16 B of line addresses and 4 B of
//    statistics in fresh_prep (every lane, once per pair), 16 B of board at kFreshBoardBase + 16 i in
//    reset_reload (the ending lanes)
static_assert(60u * 15u + 4u * 14u + 3u == lut::kFreshEntries - 1u, "kFresh index range");
static_assert(kFreshStatBase + 4u * lut::kFreshEntries <= kRolloutLdsWords * 4u, "kFresh reads stay inside the allocation");

// Packed monotonicity statistics of the rollout kernel, one VGPR per board: bits 0..3 pos (the
// first row-major cell holding the maximum), 8..11 L, 12..15 R, 16..19 T, 20..23 B (board.hpp
// MonoStats), 24..27 M.  Bytes 1 and 2 are the low bytes of a board's kLine11 row / column line-entry sums.
__device__ __forceinline__ uint32_t pack_stats(const MonoStats &s) {
    return s.pos | ((uint32_t)s.L << 8) | ((uint32_t)s.R << 12) | ((uint32_t)s.T << 16) | ((uint32_t)s.B << 20) |
           (s.M << 24);
}
// board.hpp mono_value on the packed word: (L, T) and (R, B) as u16 pairs (L, R scaled by 256),
// one packed max and one dot product give 256 (max(L, R) + max(T, B)); x2 for a corner maximum
// (>> 7), floor(/2) otherwise (>> 9).  The bit-field extract reads its offset from bits 0..4 of S.
__device__ __forceinline__ uint32_t mono_value_packed(uint32_t S) {
    const u16x2 m = __builtin_elementwise_max(as_u16x2(S & 0x000F0F00u), as_u16x2((S >> 4) & 0x000F0F00u));
    const uint32_t best256 = __builtin_amdgcn_udot2(m, (u16x2){1, 256}, 0u, false);
    const uint32_t corner = __builtin_amdgcn_ubfe(0x9009u, S, 1u);
    return best256 >> (9u - 2u * corner);
}
// L|R and T|B bytes of a board's kLine11 row sum SR and column sum SC into bytes 1 and 2
__device__ __forceinline__ uint32_t stats_bytes(uint32_t SR, uint32_t SC) {
    return __builtin_amdgcn_perm(SC, SR, 0x0C04000Cu);
}

// Game2048.reset (game.py:942-950) from the four words of one Philox draw: the two spawns of reset()
// on an empty board (same result as fresh_board<Philox>: 16 empties, then 15).
__device__ __forceinline__ uint4 fresh_from_words(const uint4 &r, uint32_t &p1, uint32_t &v1, uint32_t &p2,
                                                  uint32_t &v2) {
    p1 = r.x >> 28;  // (x * 16) >> 32
    v1 = r.y < kTwoThreshold ? 1u : 2u;
    const uint32_t k2 = (uint32_t)(((uint64_t)r.z * 15u) >> 32);
    p2 = k2 + (k2 >= p1 ? 1u : 0u);
    v2 = r.w < kTwoThreshold ? 1u : 2u;
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    set_cell(b, p1, v1);
    set_cell(b, p2, v2);
    return b;
}

// The rollout kernel's auto-reset from two spare words (oracle or_reset_words): cell 1 = a >> 28,
// its value from the other 28 bits of a; cell 2 = floor(bw * 15 / 2^32) among the 15 cells left,
// its value from the low word of bw * 15.
__device__ __forceinline__ uint4 fresh_from_pair(uint32_t a, uint32_t bw, uint32_t &p1, uint32_t &v1, uint32_t &p2,
                                                 uint32_t &v2) {
    p1 = a >> 28;
    v1 = (a << 4) < kTwoThreshold ? 1u : 2u;
    const uint32_t k2 = __umulhi(bw, 15u);
    p2 = k2 + (k2 >= p1 ? 1u : 0u);
    v2 = bw * 15u < kTwoThreshold ? 1u : 2u;
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    set_cell(b, p1, v1);
    set_cell(b, p2, v2);
    return b;
}

// Legal mask and monotonicity statistics of a fresh two-tile board in closed form (tiles v1 at p1,
// v2 at p2, p1 != p2).  A direction is blocked only when both tiles already sit against its edge
// on different lines, or they are the two leading cells of one line with different values.
__device__ __forceinline__ uint32_t fresh_stats(uint32_t p1, uint32_t v1, uint32_t p2, uint32_t v2, MonoStats &s) {
    const uint32_t r1 = p1 >> 2, c1 = p1 & 3u, r2 = p2 >> 2, c2 = p2 & 3u;
    const bool same_row = r1 == r2, same_col = c1 == c2, ne = v1 != v2;
    const uint32_t sc = c1 + c2, sr = r1 + r2;
    // blocked-direction bits as 0/1 integers (bool selects here compile to divergent branches)
    const uint32_t srw = same_row, scl = same_col, nev = ne;
    const uint32_t left_blk = (srw & nev & (uint32_t)(sc == 1u)) | ((srw ^ 1u) & (uint32_t)(sc == 0u));
    const uint32_t right_blk = (srw & nev & (uint32_t)(sc == 5u)) | ((srw ^ 1u) & (uint32_t)(sc == 6u));
    const uint32_t up_blk = (scl & nev & (uint32_t)(sr == 1u)) | ((scl ^ 1u) & (uint32_t)(sr == 0u));
    const uint32_t down_blk = (scl & nev & (uint32_t)(sr == 5u)) | ((scl ^ 1u) & (uint32_t)(sr == 6u));
    const uint32_t legal = 15u ^ (up_blk | (down_blk << 1) | (left_blk << 2) | (right_blk << 3));
    const bool hadj = same_row & ((max(c1, c2) - min(c1, c2)) == 1u);
    const bool vadj = same_col & ((max(r1, r2) - min(r1, r2)) == 1u);
    const uint32_t lv = c1 < c2 ? v1 : v2, rv = c1 < c2 ? v2 : v1;  // left / right tile (same row)
    const uint32_t tv = r1 < r2 ? v1 : v2, bv = r1 < r2 ? v2 : v1;  // top / bottom tile (same column)
    s.L = (int)(hadj & (lv >= rv));
    s.R = (int)(hadj & (rv >= lv));
    s.T = (int)(vadj & (tv >= bv));
    s.B = (int)(vadj & (bv >= tv));
    s.M = max(v1, v2);
    s.pos = v1 > v2 ? p1 : v2 > v1 ? p2 : min(p1, p2);
    return legal;
}

// Per-lane state of the rollout carried from step to step.
struct RolloutLane {
    uint4 b;          // current board (never finished between steps)
    uint32_t legal;   // its legal mask
    uint32_t S;       // its packed monotonicity statistics (pack_stats)
    int empt_b;       // its empty-cell count
    uint2 R[4], C[4]; // the kLine11 records of its rows and columns (valid while its maximum is <= 10;
                      // a board above that moves on the SWAR path, which does not read them)
    uint4 D;          // Philox draw of the current pair of steps: x / y = the two steps' words,
                      // z / w = the words of a reset inside the pair (at most one: a reset board
                      // cannot end again one move later)
    PhiloxState ph;   // draw of the next pair, computed half per step inside the LDS round trip
    uint32_t fbo;     // the board a reset inside the current pair starts (D.z, D.w -> kFresh): its LDS
                      // byte address (kFreshBoardBase + 16 i), read only by the lanes whose game ends ...
    uint32_t flegal;  // ... its legal mask and packed statistics
    uint32_t fS;
    uint4 fla;        // ... and the LDS addresses of the kLine11 records of its rows and columns (8 x u16)
};

// the current pair's auto-reset board in kFresh (fresh_from_pair's board and fresh_stats' results):
// its index, its statistics word and the addresses of the records of its eight lines (kFreshLines),
// read once per pair right after the draw is known, long before a step can need them.  The board and
// the eight records are read by reset_reload, in the lanes whose game ends and nowhere else.
__device__ __forceinline__ void fresh_prep(RolloutLane &s, const uint32_t *__restrict__ tab) {
    const uint32_t a = s.D.z, bw = s.D.w;
    const uint64_t pb = (uint64_t)bw * 15u;  // one v_mad_u64_u32: k2 and the low word
    const uint32_t k2 = (uint32_t)(pb >> 32);
    const uint32_t i = 60u * (a >> 28) + 4u * k2 + ((a << 4) >= kTwoThreshold ? 2u : 0u) +
                       ((uint32_t)pb >= kTwoThreshold ? 1u : 0u);
    const char *t = reinterpret_cast<const char *>(tab);
    s.fbo = kFreshBoardBase + 16u * i;
    s.fla = *reinterpret_cast<const uint4 *>(t + kFreshLineBase + 16u * i);
    const uint32_t st = *reinterpret_cast<const uint32_t *>(t + kFreshStatBase + 4u * i);
    s.flegal = st >> 28;
    s.fS = st & 0x0FFFFFFFu;
}
// The auto-reset of the lanes whose game ended (called under the divergent `if (over)`): the fresh
// board and the records of its eight lines, loaded over the step's own b / R / C.  An exec-masked
// load is a select that costs no VALU: the other lanes keep what the step's round trip loaded, and a
// wave without an ending skips the block.  The empty asm keeps the address unpack inside the block
// (the compiler would otherwise hoist the eight ALU operations into every step).
__device__ __forceinline__ void reset_reload(RolloutLane &s, const uint32_t *__restrict__ tab) {
    uint4 la = s.fla;
    asm volatile("" : "+v"(la.x), "+v"(la.y), "+v"(la.z), "+v"(la.w));
    // the board first: the next step stores it before it picks among the records
    s.b = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(tab) + s.fbo);
    s.R[0] = lds_rec(tab, la.x & 0xFFFFu);
    s.R[1] = lds_rec(tab, la.x >> 16);
    s.R[2] = lds_rec(tab, la.y & 0xFFFFu);
    s.R[3] = lds_rec(tab, la.y >> 16);
    s.C[0] = lds_rec(tab, la.z & 0xFFFFu);
    s.C[1] = lds_rec(tab, la.z >> 16);
    s.C[2] = lds_rec(tab, la.w & 0xFFFFu);
    s.C[3] = lds_rec(tab, la.w >> 16);
}

// the records of the current board's lines from the board itself (launch start; the steps keep them
// up to date from then on).  A lane whose board holds an exponent > 10 reads the empty line's.
__device__ __forceinline__ void refill_lines(RolloutLane &s, const uint32_t *__restrict__ tab) {
    const uint4 ab = sel4((s.S >> 24) > kMaxLineDigit, make_uint4(0u, 0u, 0u, 0u), s.b);
    uint32_t ra[4], ca[4];
    line11_addrs(ab, ra, ca);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s.R[i] = lds_rec(tab, ra[i]);
        s.C[i] = lds_rec(tab, ca[i]);
    }
}

struct TrajRows {  // this lane's element of row t of each time-major trajectory array (advanced by n per step)
    uint4 *b;
    uint8_t *a;
    int32_t *p;
    uint32_t *pot;
    uint8_t *f;
    __device__ __forceinline__ void next(int64_t n) {
        b += n;
        a += n;
        p += n;
        pot += n;
        f += n;
    }
};


// One env step of the synthetic random-legal policy (oracle or_step_word + auto-reset).  kOdd = the
// second step of the pair.  One 32-bit word u per step: action k = floor(u * nlegal / 2^32); the
// low word r of that product (uniform given k) picks the spawn cell and value.
template <bool kOdd, bool kSmall = false>
__device__ __forceinline__ void rollout_step(RolloutLane &s, const uint32_t *__restrict__ tab, const TrajRows &tr,
                                             uint64_t seed, uint64_t next_pair, uint32_t env) {
    *tr.b = s.b;
    const uint32_t u = kOdd ? s.D.y : s.D.x;
    const uint64_t pa = (uint64_t)u * (uint32_t)__popc(s.legal);
    const uint32_t a = kth_bit4(s.legal, (uint32_t)(pa >> 32)), r = (uint32_t)pa;
    // the move from the carried records: the columns' for UP / DOWN, the rows' otherwise; the
    // start-slid half for UP / LEFT, the end-slid one for DOWN / RIGHT (the unpack selector).  No
    // table read and no address arithmetic: the previous step read these records.
    const bool vert = a < 2u, rev = (a & 1u) != 0u;
    const uint32_t usel = rev ? kUnpackEndSel : kUnpackStartSel;
    const uint32_t e0 = vert ? s.C[0].x : s.R[0].x, e1 = vert ? s.C[1].x : s.R[1].x;
    const uint32_t e2 = vert ? s.C[2].x : s.R[2].x, e3 = vert ? s.C[3].x : s.R[3].x;
    const uint32_t h0 = vert ? s.C[0].y : s.R[0].y, h1 = vert ? s.C[1].y : s.R[1].y;
    const uint32_t h2 = vert ? s.C[2].y : s.R[2].y, h3 = vert ? s.C[3].y : s.R[3].y;
    const uint32_t mono_b = mono_value_packed(s.S);
    const uint4 w = make_uint4(unpack_row(e0, usel), unpack_row(e1, usel), unpack_row(e2, usel), unpack_row(e3, usel));
    uint4 moved = sel4(vert, transpose(w), w);
    // merge points / 4 in bits 16..27 of each record's dword 1, the slid line's maximum in bits 28..31
    uint32_t pts = (((h0 >> 16) & 0xFFFu) + ((h1 >> 16) & 0xFFFu) + ((h2 >> 16) & 0xFFFu) + ((h3 >> 16) & 0xFFFu)) << 2;
    uint32_t Ma = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_elementwise_max(as_u16x2(h0), as_u16x2(h1)),
                                                                         __builtin_elementwise_max(as_u16x2(h2), as_u16x2(h3)))) >> 28;
    if (!kSmall && (s.S >> 24) > kMaxLineDigit) {  // an exponent outside the table: the SWAR compute path
        uint32_t mx;
        moved = apply_move(s.b, a, pts, mx);
        Ma = board_max(moved);
    }
    const uint32_t rm[4] = {moved.x, moved.y, moved.z, moved.w};
    const uint32_t Zm[4] = {zm(moved.x), zm(moved.y), zm(moved.z), zm(moved.w)};
    const uint32_t pos_a = first_cell_eq(rm, Ma);
    // spawn on the k-th empty cell (row-major), k = floor(r * empties / 2^32), value 1 if the low
    // word of r * empties is below 0.9 * 2^32 (given k that low word is uniform to within
    // empties / 2^32); the row from the prefix counts of empties, the column inside the row likewise
    const uint32_t n0 = __popc(Zm[0]), n01 = __popc(Zm[1]) + n0, n012 = __popc(Zm[2]) + n01;
    const uint32_t empt_a = __popc(Zm[3]) + n012;
    const uint64_t prod = (uint64_t)r * empt_a;
    const uint32_t k = (uint32_t)(prod >> 32);
    const uint32_t v = (uint32_t)prod < kTwoThreshold ? 1u : 2u;
    const bool r1 = k >= n0, r2 = k >= n01, r3 = k >= n012;  // spawn row >= 1, >= 2, == 3
    const uint32_t kr = k - (r3 ? n012 : r2 ? n01 : r1 ? n0 : 0u);
    const uint32_t z = r3 ? Zm[3] : r2 ? Zm[2] : r1 ? Zm[1] : Zm[0];
    const uint32_t b0 = (z >> 7) & 1u, b01 = b0 + ((z >> 15) & 1u), b012 = b01 + ((z >> 23) & 1u);
    const bool c1 = kr >= b0, c2 = kr >= b01, c3 = kr >= b012;  // spawn column >= 1, >= 2, == 3
    const uint32_t row = (uint32_t)r1 + (uint32_t)r2 + (uint32_t)r3, col = (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3;
    const uint32_t sp = 4u * row + col;
    const uint4 pre = moved;
    const uint32_t bits = v << (8u * col);
    moved.x |= r1 ? 0u : bits;
    moved.y |= (r1 && !r2) ? bits : 0u;
    moved.z |= (r2 && !r3) ? bits : 0u;
    moved.w |= r3 ? bits : 0u;
    s.b = moved;  // the next board (after the spawn)
    // The step's one LDS round trip: the records of the next board's four rows and four columns (the
    // next move, whatever its direction, and this board's line sums), and the line entries of the
    // spawn's row and column before and after the spawn (dword 1's low half), whose difference
    // takes the sums back to the moved board's.  The pre-spawn address is the post-spawn one minus
    // v x 8 x 11^(column / row).  Outside the fast pair a lane holding an exponent > 10 takes its
    // addresses from an empty board (its reads are discarded below).
    uint4 ab = moved;
    uint32_t va = v;
    if (!kSmall) {
        const bool big = Ma > kMaxLineDigit;
        ab = sel4(big, make_uint4(0u, 0u, 0u, 0u), moved);
        va = big ? 0u : v;
    }
    uint32_t ra[4], ca[4];
    line11_addrs(ab, ra, ca);
    constexpr uint64_t kW11 = 0x299803C800580008ull;  // 8 x {1, 11, 121, 1331}
    const uint32_t rq = r3 ? ra[3] : r2 ? ra[2] : r1 ? ra[1] : ra[0], cq = c3 ? ca[3] : c2 ? ca[2] : c1 ? ca[1] : ca[0];
    const uint32_t rp = rq - va * ((uint32_t)(kW11 >> (16u * col)) & 0xFFFFu);
    const uint32_t cp = cq - va * ((uint32_t)(kW11 >> (16u * row)) & 0xFFFFu);
    uint2 R0 = lds_rec(tab, ra[0]), R1 = lds_rec(tab, ra[1]), R2 = lds_rec(tab, ra[2]), R3 = lds_rec(tab, ra[3]);
    uint2 C0 = lds_rec(tab, ca[0]), C1 = lds_rec(tab, ca[1]), C2 = lds_rec(tab, ca[2]), C3 = lds_rec(tab, ca[3]);
    uint32_t fq = lds_half(tab, rq + 4u), gq = lds_half(tab, cq + 4u);
    uint32_t fp = lds_half(tab, rp + 4u), gp = lds_half(tab, cp + 4u);
    // half of the next pair's Philox rounds fill the round trip: the empty asm statements start them
    // after the table loads are issued (memory clobber) and consume the loaded entries after them
    asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3)::"memory");
    if constexpr (kOdd) philox_rounds<5, 10>(s.ph);
    else philox_rounds<0, 5>(s.ph);
    asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3), "+v"(R0.y), "+v"(R1.y), "+v"(R2.y), "+v"(R3.y),
                      "+v"(C0.y), "+v"(C1.y), "+v"(C2.y), "+v"(C3.y), "+v"(fq), "+v"(gq), "+v"(fp), "+v"(gp));
    *tr.a = (uint8_t)a;
    *tr.p = (int32_t)pts;
    // line sums of the next board (bits 16..31 of a sum hold the points / maximum fields' sum, which no
    // byte select below reads) and of the pre-spawn board
    const uint32_t SR = R0.y + R1.y + R2.y + R3.y, SC = C0.y + C1.y + C2.y + C3.y;
    const uint32_t SRp = SR - fq + fp, SCp = SC - gq + gp;
    // #lines that can move per direction in nibbles {UP, DOWN, LEFT, RIGHT} -> legal bits 0..3: a
    // nibble n in 0..4 gets bit 3 set by n + 7; the 24-bit product gathers bits 3, 7, 11, 15 at 12..15
    const uint32_t nl = __builtin_amdgcn_perm(SR, SC, 0x0C0C0501u);
    s.legal = (__umul24((nl + 0x7777u) & 0x8888u, 0x249u) >> 12) & 15u;
    if (!kSmall && Ma > kMaxLineDigit) s.legal = legal_mask(moved);  // an exponent outside kLine11
    const bool over = s.legal == 0u;
    s.R[0] = R0, s.R[1] = R1, s.R[2] = R2, s.R[3] = R3;
    s.C[0] = C0, s.C[1] = C1, s.C[2] = C2, s.C[3] = C3;
    // statistics before the spawn (the record's mono_a) and after it (carried to the next step): the
    // spawned tile changes the maximum / its first cell only when it reaches the maximum
    uint32_t sa = stats_bytes(SRp, SCp) | pos_a;
    const uint32_t pos2 = v > Ma ? sp : v == Ma ? min(pos_a, sp) : pos_a;
    uint32_t S = stats_bytes(SR, SC) | pos2 | (max(Ma, v) << 24);
    if (!kSmall && Ma > kMaxLineDigit) {  // an exponent outside kLine11: the SWAR statistics
        const MonoStats ms = mono_stats(pre);
        sa = pack_stats(ms);
        S = pack_stats(mono_add_tile(ms, pre, sp, v));
    }
    const uint32_t mono_a = mono_value_packed(sa);
    *tr.pot = mono_b | (mono_a << 8) | ((uint32_t)s.empt_b << 16) | (empt_a << 24);
    uint32_t fl = s.legal;
    s.S = S;
    s.empt_b = (int)empt_a - 1;
    // game over: a new game from the pair's spare words (kFresh, prepared with the draw), in the lanes
    // that ended only.  The fresh board and the records of its lines are loaded over the step's own
    // (reset_reload), and its legal mask and statistics -- the word fresh_prep read with the draw, so
    // no round trip is exposed here -- are moved in: nothing of the reset is computed or selected in
    // a lane that plays on, and a wave without an ending skips the block.  It sits at the end of the
    // step (measured faster than right after the legal mask, profiles/r08a): the next step's board
    // store and record pick are the first to need the loads, after its action arithmetic; in the odd
    // step the Philox start and fresh_prep follow and cover them, and fresh_prep overwrites fbo / fla /
    // flegal / fS for the next pair only after this block has used the current pair's.
    if (over) {
        reset_reload(s, tab);
        fl = FLAG_DONE | FLAG_RESET | s.flegal;
        s.legal = s.flegal;
        s.S = s.fS;
        s.empt_b = 14;
    }
    *tr.f = (uint8_t)fl;
    if constexpr (kOdd) {
        s.D = make_uint4(s.ph.c0, s.ph.c1, s.ph.c2, s.ph.c3);
        s.ph = philox_start(seed, next_pair, env, 1u);
        fresh_prep(s, tab);
    }
}

// Synthetic random-legal rollout (the benchmark workload of BASELINE.md): `steps` env steps per
// board per launch, board in registers, auto-reset on done, one time-major trajectory record per
// step: the board the action was taken on [T][N][16], action, points, potentials, flags.
// Step c (absolute Philox counter) takes word c & 1 of the stream-1 draw at counter c >> 1, so one
// Philox draw serves two steps (and the reset that may end one of them).  The legal mask is
// carried from the previous step (the action is always legal), and so are the kLine11 records of
// the board's rows and columns, which hold the move in every direction, its points and the slid
// lines' maximum: a step's only table reads are the records of the board it produces.  A board
// holding an exponent > 10 takes the SWAR compute path.  Workgroups are persistent over boards, so
// large N keeps several waves per SIMD with one LDS table per CU.
__global__ __launch_bounds__(1024) void env_rollout_kernel(uint4 *__restrict__ boards, int64_t n, int64_t steps,
                                                           uint4 *__restrict__ tb, uint8_t *__restrict__ ta,
                                                           int32_t *__restrict__ tp, uint32_t *__restrict__ tpot,
                                                           uint8_t *__restrict__ tf, RngArgs rng,
                                                           uint32_t *__restrict__ ticket = nullptr) {
    // kLine11, then kFresh and kFreshLines (the layout is line11_lds.hpp's, the address bounds are at the top of the file)
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kRolloutLdsWords];
    stage_row_table(s_row);
    const uint64_t ctr0 = rng_counter(rng);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        RolloutLane s;
        s.b = boards[i];
        const uint32_t env = rng.env_base + (uint32_t)i;
        const uint32_t li = (uint32_t)i;
        s.legal = legal_mask(s.b);
        if (s.legal == 0u) {  // a finished board handed in: start a new game first (counter ctr0 + steps)
            uint32_t p1, v1, p2, v2;
            s.b = fresh_from_words(philox_draw(rng.seed, ctr0 + (uint64_t)steps, env, 2u), p1, v1, p2, v2);
            MonoStats ms;
            s.legal = fresh_stats(p1, v1, p2, v2, ms);
            s.S = pack_stats(ms);
        } else {
            s.S = pack_stats(mono_stats(s.b));
        }
        s.empt_b = emptiness(s.b);
        uint64_t pair = ctr0 >> 1;
        s.D = philox_draw(rng.seed, pair, env, 1u);
        s.ph = philox_start(rng.seed, pair + 1u, env, 1u);
        fresh_prep(s, s_row);
        refill_lines(s, s_row);
        // per-lane record addresses, advanced one row (n elements) per step: no array base in an SGPR
        // pair across the loop (the loop's SGPR spills)
        TrajRows tr{tb + li, ta + li, tp + li, tpot + li, tf + li};
        int64_t t = 0;
        if ((ctr0 & 1u) && steps > 0) {  // the launch starts on the second step of a pair
            philox_rounds<0, 5>(s.ph);
            rollout_step<true>(s, s_row, tr, rng.seed, pair + 2u, env);
            tr.next(n);
            pair++;
            t = 1;
        }
        for (; t + 2 <= steps; t += 2, pair++) {
            // every board of the wave <= 2^8 at the pair's start: both steps stay inside kLine11
            // (a move adds at most 1 to the maximum), so the pair runs without the fallback branches
            // and without masking its addresses.  The other pair keeps the carried records valid in
            // every lane whose board is <= 2^10, so a wave changes between the two freely.
            if (__all(s.S < (9u << 24))) {
                rollout_step<false, true>(s, s_row, tr, rng.seed, pair + 2u, env);
                tr.next(n);
                rollout_step<true, true>(s, s_row, tr, rng.seed, pair + 2u, env);
            } else {
                rollout_step<false>(s, s_row, tr, rng.seed, pair + 2u, env);
                tr.next(n);
                rollout_step<true>(s, s_row, tr, rng.seed, pair + 2u, env);
            }
            tr.next(n);
        }
        if (t < steps) rollout_step<false>(s, s_row, tr, rng.seed, pair + 2u, env);
        boards[i] = s.b;
    }
    if (ticket) {
        // g2048_env_rollout_random_adv: the device counter advances by `steps` once every block has
        // read it (each block read it before its boards, i.e. before it arrives here): the last block
        // to arrive adds and puts the ticket back to zero -- no counter-bump kernel between launches.
        // Relaxed: every block's counter read was consumed long before its arrival, the next launch
        // sees the add across the kernel boundary, and an agent-scope release here would write back
        // L2 -- with this launch's records in it (measured +6 us per launch with acq_rel)
        __syncthreads();
        if (threadIdx.x == 0 &&
            __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
            __hip_atomic_fetch_add(const_cast<uint64_t *>(rng.counter_dev), (uint64_t)steps, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" {

static int rollout_launch(g2048_stream_t stream, int8_t *boards, int64_t n, int64_t steps, int8_t *traj_boards,
                          uint8_t *traj_actions, int32_t *traj_points, int8_t *traj_pot, uint8_t *traj_flags,
                          const g2048_rng *rng, uint32_t *ticket);

int g2048_env_rollout_random(g2048_stream_t stream, int8_t *boards, int64_t n, int64_t steps, int8_t *traj_boards,
                             uint8_t *traj_actions, int32_t *traj_points, int8_t *traj_pot, uint8_t *traj_flags,
                             const g2048_rng *rng) {
    return rollout_launch(stream, boards, n, steps, traj_boards, traj_actions, traj_points, traj_pot, traj_flags, rng,
                          nullptr);
}

int g2048_env_rollout_random_adv(g2048_stream_t stream, int8_t *boards, int64_t n, int64_t steps, int8_t *traj_boards,
                                 uint8_t *traj_actions, int32_t *traj_points, int8_t *traj_pot, uint8_t *traj_flags,
                                 const g2048_rng *rng, uint32_t *ticket) {
    if (!rng || !rng->counter_dev || !ticket || ((uintptr_t)rng->counter_dev & 7u) || ((uintptr_t)ticket & 3u))
        return G2048_EINVAL;
    return rollout_launch(stream, boards, n, steps, traj_boards, traj_actions, traj_points, traj_pot, traj_flags, rng,
                          ticket);
}

static int rollout_launch(g2048_stream_t stream, int8_t *boards, int64_t n, int64_t steps, int8_t *traj_boards,
                          uint8_t *traj_actions, int32_t *traj_points, int8_t *traj_pot, uint8_t *traj_flags,
                          const g2048_rng *rng, uint32_t *ticket) {
    // n < 2^28: a lane's byte offset into a trajectory row (16 * board id) fits the 32-bit saddr offset
    if (n < 0 || n >= (int64_t(1) << 28) || steps < 0 || !rng || rng->mode != G2048_RNG_PHILOX) return G2048_EINVAL;
    if (n == 0 || steps == 0) return G2048_OK;
    if (!boards || !traj_boards || !traj_actions || !traj_points || !traj_pot || !traj_flags || !aligned16(boards) ||
        !aligned16(traj_boards) || ((uintptr_t)traj_pot & 3u) || ((uintptr_t)traj_points & 3u))
        return G2048_EINVAL;
    // one workgroup per CU holds the 149 KiB LDS tables; its size scales with N up to 1024 threads
    // so that large N runs 4 waves per SIMD while N = 65 536 still spreads over all 256 CUs
    int64_t threads = (n + 255) / 256;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : ((threads + 63) / 64) * 64;
    int64_t grid = (n + threads - 1) / threads;
    grid = grid > 256 ? 256 : grid;
    hipLaunchKernelGGL(env_rollout_kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, (hipStream_t)stream,
                       (uint4 *)boards, n, steps, (uint4 *)traj_boards, traj_actions, traj_points, (uint32_t *)traj_pot,
                       traj_flags, rng_args(rng), ticket);
    return launch_status();
}

}  // extern "C"
