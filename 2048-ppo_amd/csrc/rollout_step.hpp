// rollout_step.hpp -- the one random-legal env step played out of the kLine11 LDS table
// (line11_lds.hpp), shared by env_rollout.hip's env_rollout_kernel (kTraj = true: the step writes its
// trajectory record, carries the potentials' statistics and restarts a finished game) and
// mc_search.hip's mc_search_kernel (kTraj = false: the step only sums points and counts moves, and a
// finished game stays finished): the lane state carried from step to step, the packed monotonicity
// statistics, the auto-reset helpers and rollout_step itself.  Both kernels sit at the register
// ceiling of a 1024-thread block, so the step is one statement sequence with `if constexpr (kTraj)`
// around what has an effect only in the record; cutting it into helper functions changes the
// register allocation of both (Monte-Carlo playout search).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "rowtable.hpp"
#include "line11_lds.hpp"
#include "step.hpp"

namespace {

using namespace g2048;

// Every LDS address a step forms:
//  - a kLine11 record at 8 idx (8 bytes, or the u16 at + 4) with every digit of the line <= 10.  The
//    wave-uniform fast pair starts with every exponent <= 8 and a move adds at most 1 to the maximum,
//    so its two steps index boards of exponents <= 9 and <= 10; every other step, and refill_lines,
//    zeroes the board it takes addresses from in the lanes that hold an exponent > 10 (their reads are
//    discarded: those lanes move on the SWAR path), and the spawn's pre-spawn lines are the post-spawn
//    ones minus the spawned digit.  (The kTraj step outside the fast pair moves a board whose maximum
//    is exactly 10 on the SWAR path as well, for the points sum below; its addresses and its statistics
//    still come from the table while the moved board stays <= 10.)
constexpr uint32_t kFastPairMax = 8u;  // a pair runs with kSmall when every board's maximum is <= this
static_assert(kFastPairMax + 1u + 1u <= kMaxLineDigit, "a fast pair (start <= 8) stays inside kLine11");
//  - the kFreshLines addresses (<= kFreshLineAddrMax, checked entry by entry by fresh_lines_ok), which
//    reset_reload reads in the lanes whose game ended
static_assert(lut::kFreshLineAddrMax + 8u <= kLineLdsBytes, "fresh boards' line records inside kLine11");
//  - a kFresh record i <= 959 (60 p1 + 4 k2 + 3, p1 <= 15, k2 <= 14): 16 B of line addresses and the 8 B
//    pair of statistics and line sums in fresh_prep (every lane, once per pair), 16 B of board at
//    kFreshBoardBase + 16 i in reset_reload (the ending lanes)
static_assert(60u * 15u + 4u * 14u + 3u == lut::kFreshEntries - 1u, "kFresh index range");
static_assert(kFreshStatBase + 8u * lut::kFreshEntries <= kRolloutLdsWords * 4u, "kFresh reads stay inside the allocation");

// What the kTraj step takes from the carried line sums (RolloutLane hsR / hsC): bits 16..27 of the sum of
// the four second words of an orientation are the move's points / 4 while that sum stays below 2^12 (the
// low halves, line_entry, sum to at most 12 per nibble and never carry into bit 16).  A line of
// exponents <= e scores at most two merges of 2^(e + 1) points.  The step reads the sums of a board whose
// maximum is <= kFastPairMax + 1 in the fast pair's second step and <= kMaxLineDigit - 1 in the other
// pair, whose lanes at kMaxLineDigit and above move on the SWAR path (sixteen 2^10 tiles would sum to
// exactly 2^12).
constexpr uint32_t line_points4_max(uint32_t e) { return 4u * 2u * ((2u << e) >> 2); }  // four lines
static_assert(line_points4_max(kFastPairMax + 1u) < 4096u && line_points4_max(kMaxLineDigit - 1u) < 4096u &&
              line_points4_max(kMaxLineDigit) == 4096u, "carried points sums stay inside their 12 bits");

// Packed monotonicity statistics, one VGPR per board (step.hpp carry_pack): bits 0..3 pos (the first
// row-major cell holding the maximum), 8..11 L, 12..15 R, 16..19 T, 20..23 B (board.hpp MonoStats),
// 24..27 M.  Bytes 1 and 2 are the low bytes of a board's kLine11 row / column line-entry sums.
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

// Per-lane state carried from step to step.  A kernel sets and reads the members of its kind of
// step only; the others never exist (a local struct is split into its members).  The member order
// is part of env_rollout_kernel's register allocation: keep it.
struct RolloutLane {
    uint4 b;          // current board (kTraj: never finished between steps)
    uint32_t legal;   // its legal mask (!kTraj: 0 = the playout is over)
    uint32_t M;       // !kTraj: its largest exponent (guards the table: > 10 moves on the SWAR path)
    uint32_t S;       // kTraj: its packed monotonicity statistics (carry_pack); bits 24.. guard the table
    int empt_b;       // kTraj: its empty-cell count
    uint2 R[4], C[4]; // the kLine11 records of its rows and columns (valid while its maximum is <= 10;
                      // a board above that moves on the SWAR path, which does not read them).  kTraj: the
                      // first words only; of the second words the step that loads them keeps ...
    uint32_t hsR, hsC;  // kTraj: ... their sum over the rows and over the columns (bits 16..27: the points / 4
                        // of a horizontal / vertical move of this board) ...
    uint32_t hmR, hmC;  // kTraj: ... and their unsigned maximum (bits 28..31: the largest tile that move leaves)
    uint4 D;          // Philox draw of the current pair of steps: x / y = the two steps' words,
                      // z / w = the words of a reset inside the pair (at most one: a reset board
                      // cannot end again one move later; !kTraj: unused)
    PhiloxState ph;   // draw of the next pair, computed half per step inside the LDS round trip
    // kTraj only:
    uint32_t fbo;     // the board a reset inside the current pair starts (D.z, D.w -> kFresh): its LDS
                      // byte address (kFreshBoardBase + 16 i), read only by the lanes whose game ends ...
    uint2 fst;        // ... its kFresh pair, as loaded: x = legal mask in bits 28..31, packed statistics below;
                      // y = its line sums (rowtable.hpp: hsR and hmR as it stands, hsC and hmC << 16)
    uint4 fla;        // ... and the LDS addresses of the kLine11 records of its rows and columns (8 x u16)
    // !kTraj only:
    uint32_t score;   // points so far
    uint32_t moves;   // steps executed
};

// the current pair's auto-reset board in kFresh (fresh_from_pair's board and fresh_stats' results):
// its index, its pair of statistics and line sums and the addresses of the records of its eight lines
// (kFreshLines), read once per pair right after the draw is known, long before a step can need them.
// The board and the eight records are read by reset_reload, in the lanes whose game ends and nowhere else.
__device__ __forceinline__ void fresh_prep(RolloutLane &s, const uint32_t *__restrict__ tab) {
    const uint32_t a = s.D.z, bw = s.D.w;
    const uint64_t pb = (uint64_t)bw * 15u;  // one v_mad_u64_u32: k2 and the low word
    const uint32_t k2 = (uint32_t)(pb >> 32);
    const uint32_t i = 60u * (a >> 28) + 4u * k2 + ((a << 4) >= kTwoThreshold ? 2u : 0u) +
                       ((uint32_t)pb >= kTwoThreshold ? 1u : 0u);
    const char *t = reinterpret_cast<const char *>(tab);
    s.fbo = kFreshBoardBase + 16u * i;
    s.fla = *reinterpret_cast<const uint4 *>(t + kFreshLineBase + 16u * i);
    // kept as loaded (one ds_read_b64): splitting it here would stop the wave at this load once per pair,
    // and nothing needs its fields before a game ends (reset_reload's caller splits it, in the ending lanes)
    s.fst = *reinterpret_cast<const uint2 *>(t + kFreshStatBase + 8u * i);
}
// The auto-reset of the lanes whose game ended (called under the divergent `if (over)`): the fresh
// board and the first words of the records of its eight lines, loaded over the step's own b / R / C
// (what a step needs of the second words comes from the kFresh pair, with no load here).  An
// exec-masked load is a select that costs no VALU: the other lanes keep what the step's round trip
// loaded, and a wave without an ending skips the block.  The empty asm keeps the address unpack inside
// the block (the compiler would otherwise hoist the eight ALU operations into every step).
__device__ __forceinline__ void reset_reload(RolloutLane &s, const uint32_t *__restrict__ tab) {
    uint4 la = s.fla;
    asm volatile("" : "+v"(la.x), "+v"(la.y), "+v"(la.z), "+v"(la.w));
    // the board first: the next step stores it before it picks among the records
    s.b = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(tab) + s.fbo);
    // (In index order.  The wait-count pass guards every first touch of these registers in the next step
    // by a wait of its own, and issuing the loads in the reverse of that order makes one wait cover all
    // eight: 506 -> 502 instructions and 13 -> 9 waits on the fast pair's path -- and 0.9 % slower in six
    // rounds of six, profiles/r18a/ab_arms.log)
    s.R[0].x = lds_word(tab, la.x & 0xFFFFu);
    s.R[1].x = lds_word(tab, la.x >> 16);
    s.R[2].x = lds_word(tab, la.y & 0xFFFFu);
    s.R[3].x = lds_word(tab, la.y >> 16);
    s.C[0].x = lds_word(tab, la.z & 0xFFFFu);
    s.C[1].x = lds_word(tab, la.z >> 16);
    s.C[2].x = lds_word(tab, la.w & 0xFFFFu);
    s.C[3].x = lds_word(tab, la.w >> 16);
}

// How a step (and refill_lines) turns a board into the eight line addresses: line11_addrs (packed-u16
// VALU, about 28 instructions) or line11_addrs_mfma (one int8 MFMA against the wave's A fragment `fa`,
// which the kernel loads at its start with every lane active, and 8 multiply-adds).  The MFMA form is
// env_rollout_kernel's where its grid covers every board (5 % faster at one wave per SIMD, 4 % at two to
// four with the narrow record stores; env_rollout.hip's host picks); mc_search_kernel keeps the VALU form,
// the default (rounds 15 and 16).
constexpr int kAddrValu = 0, kAddrMfma = 1;

// the records of the current board's lines from the board itself (launch start; the steps keep them
// up to date from then on), and (kTraj) the sums and maxima of their second words.  A lane whose board
// holds an exponent > 10 (mx = its maximum) reads the empty line's.
template <int kAddr = kAddrValu, bool kTraj = false>
__device__ __forceinline__ void refill_lines(RolloutLane &s, const uint32_t *__restrict__ tab, uint32_t mx, const i32x4 &fa = i32x4{}) {
    const uint4 ab = sel4(mx > kMaxLineDigit, make_uint4(0u, 0u, 0u, 0u), s.b);
    uint32_t ra[4], ca[4];
    if constexpr (kAddr == kAddrValu) line11_addrs(ab, ra, ca);
    else line11_addrs_mfma(ab, fa, ra, ca);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s.R[i] = lds_rec(tab, ra[i]);
        s.C[i] = lds_rec(tab, ca[i]);
    }
    if constexpr (kTraj) {
        s.hsR = s.R[0].y + s.R[1].y + s.R[2].y + s.R[3].y;
        s.hsC = s.C[0].y + s.C[1].y + s.C[2].y + s.C[3].y;
        s.hmR = max(max(s.R[0].y, s.R[1].y), max(s.R[2].y, s.R[3].y));
        s.hmC = max(max(s.C[0].y, s.C[1].y), max(s.C[2].y, s.C[3].y));
    }
}

// s_waitcnt lgkmcnt(0) as the operand of __builtin_amdgcn_s_waitcnt (gfx9 encoding: vmcnt in bits 0..3
// and 14..15, expcnt in 4..6, both left at their maximum, i.e. not waited for; lgkmcnt in 8..11)
constexpr int kWaitLds = 0xC07F;

// Where a step's record goes: this lane's element of row t of each time-major trajectory array, advanced
// by one row (n elements) per step.  Two forms (env_rollout.hip's host picks):
//  - TrajRows, the wide form: five per-lane 64-bit pointers, valid at every shape.
//  - TrajRowsNarrow: the five array bases, wave-uniform and constant (SGPR pairs), and three per-lane
//    32-bit BYTE offsets -- o1 into actions and flags, o4 into points and potentials, o16 into boards --
//    that start at i, 4 i, 16 i and advance by n, 4 n, 16 n.  A store is `base + zext(offset)`, the
//    scalar-base form of global_store (no 64-bit vector add), so the largest offset formed for a store,
//    16 (n steps - 1), has to fit 32 bits: valid while 16 n steps <= 2^32.  (The advance behind the last
//    step may wrap; nothing is stored through it.)
struct TrajRows {
    uint4 *b;
    uint8_t *a;
    int32_t *p;
    uint32_t *pot;
    uint8_t *f;
    // board i's row 0
    __device__ __forceinline__ static TrajRows at(uint4 *tb, uint8_t *ta, int32_t *tp, uint32_t *tpot, uint8_t *tf, uint32_t i) {
        return TrajRows{tb + i, ta + i, tp + i, tpot + i, tf + i};
    }
    __device__ __forceinline__ void next(int64_t n) {
        b += n;
        a += n;
        p += n;
        pot += n;
        f += n;
    }
    __device__ __forceinline__ void put_b(const uint4 &v) const { *b = v; }
    __device__ __forceinline__ void put_a(uint32_t v) const { *a = (uint8_t)v; }
    __device__ __forceinline__ void put_p(uint32_t v) const { *p = (int32_t)v; }
    __device__ __forceinline__ void put_pot(uint32_t v) const { *pot = v; }
    __device__ __forceinline__ void put_f(uint32_t v) { *f = (uint8_t)v; }
};
struct TrajRowsNarrow {
    char *b, *a, *p, *pot, *f;
    uint32_t o1, o4, o16;
    // board i's row 0 (i < 2^28)
    __device__ __forceinline__ static TrajRowsNarrow at(uint4 *tb, uint8_t *ta, int32_t *tp, uint32_t *tpot, uint8_t *tf, uint32_t i) {
        return TrajRowsNarrow{(char *)tb, (char *)ta, (char *)tp, (char *)tpot, (char *)tf, i, 4u * i, 16u * i};
    }
    // One add per offset and step.  The empty asm makes each sum a value of its own: without it the
    // compiler keeps the even step's offsets across the pair and forms the odd step's beside them,
    // three more adds per pair.
    __device__ __forceinline__ void next(int64_t n) {
        const uint32_t n1 = (uint32_t)n;
        o1 += n1;
        o4 += 4u * n1;
        o16 += 16u * n1;
        asm("" : "+v"(o1), "+v"(o4), "+v"(o16));
    }
    __device__ __forceinline__ void put_b(const uint4 &v) const { *reinterpret_cast<uint4 *>(b + o16) = v; }
    __device__ __forceinline__ void put_a(uint32_t v) const { *reinterpret_cast<uint8_t *>(a + o1) = (uint8_t)v; }
    __device__ __forceinline__ void put_p(uint32_t v) const { *reinterpret_cast<int32_t *>(p + o4) = (int32_t)v; }
    __device__ __forceinline__ void put_pot(uint32_t v) const { *reinterpret_cast<uint32_t *>(pot + o4) = v; }
    // The flags store stands behind the masked reset block, in a basic block of its own, and instruction
    // selection works block by block: it would see the zero-extended offset as a 64-bit value from another
    // block and add it to the base with a v_lshl_add_u64 (and keep a zero register for the high half).
    // The empty asm redefines o1 in the store's block, in place (no copy: every later use reads the
    // redefined value), so the extension is selected with the store, into its scalar-base form.
    __device__ __forceinline__ void put_f(uint32_t v) {
        asm("" : "+v"(o1));
        *reinterpret_cast<uint8_t *>(f + o1) = (uint8_t)v;
    }
};

// One env step of the synthetic random-legal policy (oracle or_step_word; kTraj: + auto-reset).
// kOdd = the second step of the pair; kSmall = every board of the wave is inside the table for this
// step (no SWAR fallback, no address masking).  One 32-bit word u per step: action
// k = floor(u * nlegal / 2^32); the low word r of that product (uniform given k) picks the spawn cell
// and value.  kTraj = false never touches tr.
template <bool kOdd, bool kSmall, bool kTraj, int kAddr = kAddrValu, class Rows = TrajRows>
__device__ __forceinline__ void rollout_step(RolloutLane &s, const uint32_t *__restrict__ tab, Rows &tr,
                                             uint64_t seed, uint64_t next_pair, uint32_t env, const i32x4 &fa = i32x4{}) {
    // kTraj: explicit waits for every LDS load in flight (a reset's reload, fresh_prep's two reads), so
    // that the wait-count pass sees an empty queue behind them.  Where the fast pair joins the path
    // that leaves the other pair the pass merges that pair's pending reloads into the fast pair's state
    // and guards each first touch of R / C, and of the registers the step reuses, with a wait of its
    // own: ten staged lgkmcnt(8)..(0) in the even step, which on the way from the loop header find the
    // counter at zero and cost an issue slot each, and five in the odd step behind the masked reload.
    // Three waits replace them: at the top of every even step (in the loop header, see below), where
    // the fast pair's even step leaves the part it shares with the other pair's, and at the top of the
    // fast pair's odd step.  They pay only together: the first alone, the first two, and the last two
    // were each slower than none, all three are 1.1-1.6 % faster.
    if constexpr (kTraj && (!kOdd || kSmall)) __builtin_amdgcn_s_waitcnt(kWaitLds);
    if constexpr (kTraj) tr.put_b(s.b);
    const uint32_t u = kOdd ? s.D.y : s.D.x;
    const uint64_t pa = (uint64_t)u * (uint32_t)__popc(s.legal);
    const uint32_t a = kth_bit4(s.legal, (uint32_t)(pa >> 32)), r = (uint32_t)pa;
    // the move from the carried records: the columns' for UP / DOWN, the rows' otherwise; the
    // start-slid half for UP / LEFT, the end-slid one for DOWN / RIGHT (the pack selector of
    // line11_lds.hpp's orient_rows).  No table read and no address arithmetic: the previous step read
    // these records.
    const bool vert = a < 2u, rev = (a & 1u) != 0u;
    const uint32_t e0 = vert ? s.C[0].x : s.R[0].x, e1 = vert ? s.C[1].x : s.R[1].x;
    const uint32_t e2 = vert ? s.C[2].x : s.R[2].x, e3 = vert ? s.C[3].x : s.R[3].x;
    // !kTraj: the second words of the chosen records, carried like the first
    uint32_t h0 = 0u, h1 = 0u, h2 = 0u, h3 = 0u;
    if constexpr (!kTraj) {
        h0 = vert ? s.C[0].y : s.R[0].y, h1 = vert ? s.C[1].y : s.R[1].y;
        h2 = vert ? s.C[2].y : s.R[2].y, h3 = vert ? s.C[3].y : s.R[3].y;
    }
    const uint32_t mono_b = kTraj ? mono_value_packed(s.S) : 0u;
    // (two selects and an add: kPackEndAdd is wider than a 24-bit multiply-add takes.  The mask form --
    // v_bfe_i32 and v_and_or behind the select by vert, two VALU fewer per step -- measured 1.5 % slower
    // than this one, as the unpack selector's did in round 13, and a select among the four constants
    // costs scratch: DESIGN.md section 6, round 14)
    const uint32_t pbase = vert ? kPackColsSel : kPackRowsSel;
    const uint32_t psel = rev ? pbase + kPackEndAdd : pbase;
    uint4 moved = orient_rows(e0, e1, e2, e3, psel, vert);
    // merge points / 4 in bits 16..27 of each record's dword 1, the slid line's maximum in bits 28..31
    uint32_t pts, Ma;
    if constexpr (kTraj) {
        // from what the previous step kept of the second words: the orientation's sum (its bits 16..27 are
        // the points / 4: line_points4_max above) and its unsigned maximum (the maximum field is on top)
        const uint32_t hs = vert ? s.hsC : s.hsR, hm = vert ? s.hmC : s.hmR;
        pts = (hs >> 14) & 0x3FFCu;
        Ma = hm >> 28;
    } else {
        pts = (((h0 >> 16) & 0xFFFu) + ((h1 >> 16) & 0xFFFu) + ((h2 >> 16) & 0xFFFu) + ((h3 >> 16) & 0xFFFu)) << 2;
        Ma = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_elementwise_max(as_u16x2(h0), as_u16x2(h1)),
                                                                    __builtin_elementwise_max(as_u16x2(h2), as_u16x2(h3)))) >> 28;
    }
    // up to here the even step is the same in both pairs, and the compiler runs it in the pair loop's
    // header, ahead of the branch to either pair; the join the waits are about lies behind that branch
    if constexpr (kTraj && kSmall && !kOdd) __builtin_amdgcn_s_waitcnt(kWaitLds);
    // an exponent outside the table: the SWAR compute path, exact for every board.  kTraj: from an exponent
    // equal to kMaxLineDigit on, where the carried points sum can leave its field (line_points4_max)
    if (!kSmall && (kTraj ? (s.S >> 24) >= kMaxLineDigit : s.M > kMaxLineDigit)) {
        uint32_t mx;
        moved = apply_move(s.b, a, pts, mx);
        Ma = board_max(moved);
    }
    const uint32_t rm[4] = {moved.x, moved.y, moved.z, moved.w};
    const uint32_t Zm[4] = {zm(moved.x), zm(moved.y), zm(moved.z), zm(moved.w)};
    // the first cell of the maximum, for the statistics.  Unlike the other arithmetic that only the
    // record needs, it has to be switched off by hand: first_cell_eq's v_ffbl_b32 is written-out asm,
    // which stays in the IR up to instruction selection when unused and moves the schedule of the
    // kTraj = false step (119 instead of 117 VGPRs, + 0.8 % on the search: profiles/r09a/time_mc_search_ab.log)
    uint32_t pos_a = 0u;
    if constexpr (kTraj && kAddr == kAddrValu) pos_a = first_cell_eq(rm, Ma);
    // spawn on the k-th empty cell (row-major), k = floor(r * empties / 2^32), value 1 if the low
    // word of r * empties is below 0.9 * 2^32 (given k that low word is uniform to within
    // empties / 2^32); the row from the prefix counts of empties, the column inside the row likewise
    const uint32_t n0 = __popc(Zm[0]), n01 = __popc(Zm[1]) + n0, n012 = __popc(Zm[2]) + n01;
    const uint32_t empt_a = __popc(Zm[3]) + n012;
    const uint64_t prod = (uint64_t)r * empt_a;
    const uint32_t k = (uint32_t)(prod >> 32);
    const uint32_t v = (uint32_t)prod < kTwoThreshold ? 1u : 2u;
    // The row without a compare or a select: bytes 0..2 of P hold the empties above rows 1, 2, 3
    // (byte 3 stays 0), and bit 7 of a byte of (0x80 + k - P_i) says k >= P_i: k <= 15 and P_i <= 12, so
    // no byte borrows or carries.  The row is the count of those bits, the empties above it byte
    // row - 1 of P (v_bfe_u32 reads its offset from bits 0..4: row 0 reads byte 3, a zero).  The column
    // inside the row z likewise, from the prefix counts of its cells 0..2 (a multiply sums bits 0, 8,
    // 16 of z >> 7 into bytes 0..2; v_mul_u32_u24 drops bit 24, cell 3, and what the product leaves in
    // byte 3 is masked off).  The picks by row and column (z, the address of the spawn's row / column
    // record, the dword the tile goes into) take the two bits of the index as lane masks.
    const uint4 pre = moved;
    uint32_t row, col, mr0 = 0u, mr1 = 0u, mc0 = 0u, mc1 = 0u;
    bool r1 = false, r2 = false, r3 = false, c1 = false, c2 = false, c3 = false;
    if constexpr (kTraj) {
        const uint32_t P = n0 | (n01 << 8) | (n012 << 16);
        const uint32_t ger = (__umul24(k, 0x010101u) + (0x808080u - P)) & 0x808080u;
        row = __popc(ger);
        const uint32_t kr = k - __builtin_amdgcn_ubfe(P, 8u * row - 8u, 8u);
        mr0 = (uint32_t)__builtin_amdgcn_sbfe((int)row, 0u, 1u), mr1 = (uint32_t)__builtin_amdgcn_sbfe((int)ger, 15u, 1u);
        asm("" : "+v"(mr0), "+v"(mr1));
        const uint32_t z = pick4m(mr0, mr1, Zm[0], Zm[1], Zm[2], Zm[3]);
        const uint32_t PC = __umul24(z >> 7, 0x010101u);
        const uint32_t gec = (__umul24(kr, 0x010101u) + (0x808080u - PC)) & 0x808080u;
        col = __popc(gec);
        mc0 = (uint32_t)__builtin_amdgcn_sbfe((int)col, 0u, 1u), mc1 = (uint32_t)__builtin_amdgcn_sbfe((int)gec, 15u, 1u);
        asm("" : "+v"(mc0), "+v"(mc1));
        const uint32_t bits = v << (8u * col);
        const uint32_t blo = bop3<~kA & kB>(mr1, bits, 0u), bhi = mr1 & bits;  // the tile for rows 0 / 1, for rows 2 / 3
        moved.x = bop3<kA | (~kB & kC)>(moved.x, mr0, blo);
        moved.y = bop3<kA | (kB & kC)>(moved.y, mr0, blo);
        moved.z = bop3<kA | (~kB & kC)>(moved.z, mr0, bhi);
        moved.w = bop3<kA | (kB & kC)>(moved.w, mr0, bhi);
    } else {
        // the search's step keeps the compare-and-select form: at its 117 VGPRs the masks and the packed
        // words above cost it 11 more registers and scratch, and it ran 2.3 % slower with them
        // (profiles/r13a/time_mc_search_ab_masks.log)
        r1 = k >= n0, r2 = k >= n01, r3 = k >= n012;  // spawn row >= 1, >= 2, == 3
        const uint32_t kr = k - (r3 ? n012 : r2 ? n01 : r1 ? n0 : 0u);
        const uint32_t z = r3 ? Zm[3] : r2 ? Zm[2] : r1 ? Zm[1] : Zm[0];
        const uint32_t b0 = (z >> 7) & 1u, b01 = b0 + ((z >> 15) & 1u), b012 = b01 + ((z >> 23) & 1u);
        c1 = kr >= b0, c2 = kr >= b01, c3 = kr >= b012;  // spawn column >= 1, >= 2, == 3
        row = (uint32_t)r1 + (uint32_t)r2 + (uint32_t)r3, col = (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3;
        const uint32_t bits = v << (8u * col);
        moved.x |= r1 ? 0u : bits;
        moved.y |= (r1 && !r2) ? bits : 0u;
        moved.z |= (r2 && !r3) ? bits : 0u;
        moved.w |= r3 ? bits : 0u;
    }
    const uint32_t sp = 4u * row + col;
    s.b = moved;  // the next board (after the spawn)
    // The step's one LDS round trip: the records of the next board's four rows and four columns (the
    // next move, whatever its direction, and this board's line sums), and (kTraj) the line entries of
    // the spawn's row and column before and after the spawn (dword 1's low half), whose difference
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
    if constexpr (kAddr == kAddrValu) {
        line11_addrs(ab, ra, ca);
    } else {
        // The MFMA's result is ready 12 issue slots after it issues, and the compiler pads what the
        // schedule leaves of them with s_nop.  first_cell_eq needs the moved board and its maximum only,
        // so in source order behind the MFMA its ~20 instructions fill that shadow (the multipliers
        // below follow them): no s_nop is left in the fast pair (profiles/r15a, arm m1a).
        const i32x16 limbs = line11_limbs_mfma(ab, fa);
        if constexpr (kTraj) pos_a = first_cell_eq(rm, Ma);
        line11_addrs_from_limbs(limbs, ra, ca);
    }
    constexpr uint64_t kW11 = 0x299803C800580008ull;  // 8 x {1, 11, 121, 1331}
    const uint32_t rq = kTraj ? pick4m(mr0, mr1, ra[0], ra[1], ra[2], ra[3]) : r3 ? ra[3] : r2 ? ra[2] : r1 ? ra[1] : ra[0];
    const uint32_t cq = kTraj ? pick4m(mc0, mc1, ca[0], ca[1], ca[2], ca[3]) : c3 ? ca[3] : c2 ? ca[2] : c1 ? ca[1] : ca[0];
    const uint32_t rp = rq - va * ((uint32_t)(kW11 >> (16u * col)) & 0xFFFFu);
    const uint32_t cp = cq - va * ((uint32_t)(kW11 >> (16u * row)) & 0xFFFFu);
    uint2 R0 = lds_rec(tab, ra[0]), R1 = lds_rec(tab, ra[1]), R2 = lds_rec(tab, ra[2]), R3 = lds_rec(tab, ra[3]);
    uint2 C0 = lds_rec(tab, ca[0]), C1 = lds_rec(tab, ca[1]), C2 = lds_rec(tab, ca[2]), C3 = lds_rec(tab, ca[3]);
    uint32_t fq = 0u, gq = 0u, fp = 0u, gp = 0u;
    if constexpr (kTraj) {
        fq = lds_half(tab, rq + 4u), gq = lds_half(tab, cq + 4u);
        fp = lds_half(tab, rp + 4u), gp = lds_half(tab, cp + 4u);
    }
    // half of the next pair's Philox rounds fill the round trip: the empty asm statements start them
    // after the table loads are issued (memory clobber) and consume the loaded entries after them
    asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3)::"memory");
    if constexpr (kOdd) philox_rounds<5, 10>(s.ph);
    else philox_rounds<0, 5>(s.ph);
    if constexpr (kTraj)
        asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3), "+v"(R0.y), "+v"(R1.y), "+v"(R2.y), "+v"(R3.y),
                          "+v"(C0.y), "+v"(C1.y), "+v"(C2.y), "+v"(C3.y), "+v"(fq), "+v"(gq), "+v"(fp), "+v"(gp));
    else
        asm volatile("" : "+v"(s.ph.c0), "+v"(s.ph.c1), "+v"(s.ph.c2), "+v"(s.ph.c3), "+v"(R0.y), "+v"(R1.y), "+v"(R2.y), "+v"(R3.y),
                          "+v"(C0.y), "+v"(C1.y), "+v"(C2.y), "+v"(C3.y));
    if constexpr (kTraj) {
        tr.put_a(a);
        tr.put_p(pts);
    }
    // line sums of the next board (bits 16..31 of a sum hold the points / maximum fields' sum, which no
    // byte select below reads: kTraj carries the sums for them, with the maxima of the same words, and
    // nothing else of the second words reaches the next step) and of the pre-spawn board
    const uint32_t SR = R0.y + R1.y + R2.y + R3.y, SC = C0.y + C1.y + C2.y + C3.y;
    if constexpr (kTraj) {
        s.hsR = SR, s.hsC = SC;
        s.hmR = max(max(R0.y, R1.y), max(R2.y, R3.y));  // v_max3_u32 and v_max_u32: no packed-operand hazard
        s.hmC = max(max(C0.y, C1.y), max(C2.y, C3.y));
    }
    const uint32_t SRp = SR - fq + fp, SCp = SC - gq + gp;
    // #lines that can move per direction in nibbles {UP, DOWN, LEFT, RIGHT} -> legal bits 0..3: a
    // nibble n in 0..4 gets bit 3 set by n + 7; the 24-bit product gathers bits 3, 7, 11, 15 at 12..15
    const uint32_t nl = __builtin_amdgcn_perm(SR, SC, 0x0C0C0501u);
    s.legal = (__umul24((nl + 0x7777u) & 0x8888u, 0x249u) >> 12) & 15u;
    if (!kSmall && Ma > kMaxLineDigit) s.legal = legal_mask(moved);  // an exponent outside kLine11
    const bool over = s.legal == 0u;
    if constexpr (kTraj) {
        s.R[0].x = R0.x, s.R[1].x = R1.x, s.R[2].x = R2.x, s.R[3].x = R3.x;
        s.C[0].x = C0.x, s.C[1].x = C1.x, s.C[2].x = C2.x, s.C[3].x = C3.x;
    } else {
        s.R[0] = R0, s.R[1] = R1, s.R[2] = R2, s.R[3] = R3;
        s.C[0] = C0, s.C[1] = C1, s.C[2] = C2, s.C[3] = C3;
    }
    if constexpr (kTraj) {
        // statistics before the spawn (the record's mono_a) and after it (carried to the next step): the
        // spawned tile changes the maximum / its first cell only when it reaches the maximum
        uint32_t sa = stats_bytes(SRp, SCp) | pos_a;
        const uint32_t pos2 = v > Ma ? sp : v == Ma ? min(pos_a, sp) : pos_a;
        uint32_t S = stats_bytes(SR, SC) | pos2 | (max(Ma, v) << 24);
        if (!kSmall && Ma > kMaxLineDigit) {  // an exponent outside kLine11: the SWAR statistics
            const MonoStats ms = mono_stats(pre);
            sa = carry_pack(ms);
            S = carry_pack(mono_add_tile(ms, pre, sp, v));
        }
        const uint32_t mono_a = mono_value_packed(sa);
        tr.put_pot(mono_b | (mono_a << 8) | ((uint32_t)s.empt_b << 16) | (empt_a << 24));
        uint32_t fl = s.legal;
        s.S = S;
        s.empt_b = (int)empt_a - 1;
        // game over: a new game from the pair's spare words (kFresh, prepared with the draw), in the lanes
        // that ended only.  The fresh board and the records of its lines are loaded over the step's own
        // (reset_reload), and its legal mask and statistics -- the word fresh_prep read with the draw, so
        // no round trip is exposed here, split here -- are moved in: nothing of the reset is computed or
        // selected in a lane that plays on, and a wave without an ending skips the block.  It sits at the
        // end of the step (measured faster than right after the legal mask, profiles/r08a): the next
        // step's board store and record pick are the first to need the loads, after its action
        // arithmetic.  In the odd step fresh_prep follows and overwrites fbo / fla / fst for the next pair
        // only after this block has used the current pair's.  Nothing covers the loads there: the loop
        // tail issues fresh_prep's two reads and branches back without a wait, and the loop header (the
        // next pair's record pick) waits first for the reload's records (lgkmcnt(2): LDS returns in
        // order, fresh_prep's two reads may stay in flight), 23 instructions after the back edge; the
        // step's own lgkmcnt(0) (top of rollout_step) follows it there.
        if (over) {
            reset_reload(s, tab);
            uint32_t st = s.fst.x, hw = s.fst.y;
            asm volatile("" : "+v"(st), "+v"(hw));  // the split stays inside the block, like reset_reload's unpack
            s.legal = st >> 28;
            s.S = st & 0x0FFFFFFFu;
            // the fresh board's line sums (rowtable.hpp FreshTable): the rows' fields stand where a sum
            // and a maximum have theirs, the columns' 16 bits below
            s.hsR = hw, s.hmR = hw;
            s.hsC = hw << 16, s.hmC = hw << 16;
            fl = FLAG_DONE | FLAG_RESET | s.legal;
            s.empt_b = 14;
        }
        tr.put_f(fl);
    } else {  // the finished game stays (legal == 0 ends the playout); only the table guard is carried
        s.M = max(Ma, v);
        s.score += pts;
        s.moves += 1u;
    }
    if constexpr (kOdd) {
        s.D = make_uint4(s.ph.c0, s.ph.c1, s.ph.c2, s.ph.c3);
        s.ph = philox_start(seed, next_pair, env, 1u);
        if constexpr (kTraj) fresh_prep(s, tab);
    }
}

}  // namespace
