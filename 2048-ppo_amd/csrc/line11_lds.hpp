// line11_lds.hpp -- the kLine11 line table in LDS, shared by the kernels that play random-legal 2048
// out of it (env_rollout.hip's env_rollout_kernel, mc_search.hip's mc_search_kernel, through the step
// they share in rollout_step.hpp): the table
// objects of the code object, the LDS layout, the LDS-DMA staging and the per-line address / record
// helpers.  Everything has internal linkage: each translation unit holds its own copy of the tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "rowtable.hpp"

namespace {

__device__ const g2048::lut::Line11Table kLine11 __attribute__((aligned(16))) = g2048::lut::Line11Table();
static_assert(g2048::lut::line11_table_ok(g2048::lut::Line11Table()), "kLine11 fields against slide_entry / line_entry");

// LDS layout of env_rollout_kernel: kLine11 at byte 0 (8-byte records, 115 KiB with its padding),
// then the auto-reset boards (kFresh), the addresses of their line records (kFreshLines) and their
// statistics.
__device__ const g2048::lut::FreshTable kFresh __attribute__((aligned(16))) = g2048::lut::FreshTable();
__device__ const g2048::lut::FreshLineTable kFreshLines __attribute__((aligned(16))) = g2048::lut::FreshLineTable();
static_assert(g2048::lut::fresh_lines_ok(g2048::lut::FreshTable(), g2048::lut::FreshLineTable()), "kFreshLines against the kFresh boards");
static_assert(g2048::lut::fresh_sums_ok(g2048::lut::FreshTable(), g2048::lut::FreshLineTable(), g2048::lut::Line11Table()),
              "kFresh line sums against the kLine11 records of the kFresh boards");
constexpr uint32_t kLineLdsBytes = g2048::lut::kFusedEntriesPadded * 8u;             // 117 760
constexpr uint32_t kFreshBoardBase = kLineLdsBytes;                           // 15 KiB of boards
constexpr uint32_t kFreshLineBase = kFreshBoardBase + g2048::lut::kFreshEntries * 16u;  // 15 KiB of line addresses
constexpr uint32_t kFreshStatBase = kFreshLineBase + g2048::lut::kFreshEntries * 16u;   // 8 KiB of {stats, line sums}
constexpr uint32_t kFreshStatPieces = 8u;
constexpr uint32_t kRolloutLdsWords = (kFreshStatBase + 1024u * kFreshStatPieces) / 4u;  // 156 672 B
static_assert(kRolloutLdsWords * 4u <= 160u * 1024u, "the tables fit the 160 KiB of LDS");
// mc_search_kernel plays out of kLine11 alone.  It keeps the allocation and the staging it was measured
// with, which end behind the first half of the statistics pairs (it reads nothing past kLine11).
constexpr uint32_t kSearchStatPieces = 4u;
constexpr uint32_t kSearchLdsWords = (kFreshStatBase + 1024u * kSearchStatPieces) / 4u;  // 152 576 B
// A kLine11 record sits at 8 idx (8 bytes, or the u16 at + 4) with every digit of the line <= 10.
constexpr uint32_t kMaxLineDigit = g2048::lut::kLineBase - 1u;
static_assert(8u * g2048::lut::line11_index(kMaxLineDigit, kMaxLineDigit, kMaxLineDigit, kMaxLineDigit) + 8u <= g2048::lut::kFusedEntries * 8u &&
              g2048::lut::kFusedEntries * 8u <= kLineLdsBytes, "kLine11 reads stay inside the table");
static_assert(g2048::lut::line11_index(kMaxLineDigit, kMaxLineDigit, kMaxLineDigit, kMaxLineDigit) < 65536u, "column indices fit the packed-u16 sums");

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u16x2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }

// LDS byte addresses (8 idx) of the kLine11 records of a board's four rows (a row read left to
// right) and four columns (top to bottom), from the rows' digit pairs: A_i = cells (i, 0) and
// (i, 2), B_i = cells (i, 1) and (i, 3) as u16 halves (the bytes themselves, one v_perm each: every
// exponent of the board is <= 10).  Rows: two packed-u16 dot products each, weights 8 x 11^j.
// Columns: column pairs (0, 2) and (1, 3) at once as packed-u16 multiply-adds over the rows; the
// byte address (up to 117 120) does not fit 16 bits, so the halves hold idx and are scaled after.
__device__ __forceinline__ void line11_addrs(const uint4 &b, uint32_t (&ra)[4], uint32_t (&ca)[4]) {
    const u16x2 k02 = {8, 968}, k13 = {88, 10648};
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
    u16x2 A[4], B[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        A[i] = as_u16x2(__builtin_amdgcn_perm(0u, w[i], 0x0C020C00u));
        B[i] = as_u16x2(__builtin_amdgcn_perm(0u, w[i], 0x0C030C01u));
        ra[i] = __builtin_amdgcn_udot2(B[i], k13, __builtin_amdgcn_udot2(A[i], k02, 0u, false), false);
    }
    const u16x2 c02 = A[0] + A[1] * (u16x2){11, 11} + A[2] * (u16x2){121, 121} + A[3] * (u16x2){1331, 1331};
    const u16x2 c13 = B[0] + B[1] * (u16x2){11, 11} + B[2] * (u16x2){121, 121} + B[3] * (u16x2){1331, 1331};
    const uint32_t p02 = __builtin_bit_cast(uint32_t, c02), p13 = __builtin_bit_cast(uint32_t, c13);
    ca[0] = (p02 & 0xFFFFu) << 3;
    ca[1] = (p13 & 0xFFFFu) << 3;
    ca[2] = (p02 >> 16) << 3;
    ca[3] = (p13 >> 16) << 3;
}

// The same eight addresses from the matrix pipe: every address is linear in the 16 board bytes, so one
// v_mfma_i32_32x32x32_i8 with the board as the B operand (lane l already holds its board's 16 bytes in
// 4 VGPRs, which is one lane's B fragment: nothing moves between lanes) and a constant A operand gives a
// lane 16 dot products of its own board.  8 x 1331 does not fit int8, so an address comes as two limbs,
// lo = 8 d0 + 88 d1 (<= 960) and hi = d2 + 11 d3 (<= 120), addr = lo + 968 hi (one v_mad_u32_u24):
// output q < 8 is the lo limb of line q (rows 0..3 left to right, then columns 0..3 top to bottom, as
// line11_addrs reads them), output q + 8 its hi limb.
//   C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), so lane (h, n) receives
//   the 16 rows m with ((m >> 2) & 1) == h, row m in register q = (m & 3) + 4 (m >> 3).
//   A: row m lives in lanes (0, m) and (1, m), one half of k each.  Lane (h', m) holds the weights of
//   output q when ((m >> 2) & 1) == h' and zero otherwise, so the row sums over the boards of lane half
//   h' only, and register q of every lane is the dot product of the lane's own board with weights q.
// Of the k-map the scheme needs only that element j of A meets element j of B within a lane half and
// that the halves do not mix (line_mfma_model; tests/test_gpu_rollout_line_addrs.py checks it on the
// hardware with every table index through every line).
// MFMA reads its operands in every lane whatever EXEC says: the A fragment has to be loaded with all 64
// lanes active and never rewritten under a partial EXEC (env_rollout_kernel loads it at its start).
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr uint32_t kLineHiScale = 8u * g2048::lut::kLineBase * g2048::lut::kLineBase;  // 968
// weight of board byte c = 4 row + col in output q
constexpr int line_mfma_weight(uint32_t q, uint32_t c) {
    const uint32_t line = q & 7u, r = c >> 2, col = c & 3u;
    const uint32_t pos = line < 4u ? (r == line ? col : 4u) : (col == line - 4u ? r : 4u);  // the cell's place in the line
    if (q < 8u) return pos == 0u ? 8 : pos == 1u ? 8 * (int)g2048::lut::kLineBase : 0;
    return pos == 2u ? 1 : pos == 3u ? (int)g2048::lut::kLineBase : 0;
}
struct LineMfmaTable {  // the A fragment of lane l: 16 int8, byte j of dword w pairs with board byte 4 w + j
    uint32_t a[64][4];
    constexpr LineMfmaTable() : a() {
        for (uint32_t l = 0u; l < 64u; l++) {
            const uint32_t m = l & 31u, q = (m & 3u) + 4u * (m >> 3);
            if (((m >> 2) & 1u) != (l >> 5)) continue;
            for (uint32_t c = 0u; c < 16u; c++) a[l][c >> 2] |= ((uint32_t)line_mfma_weight(q, c) & 0xFFu) << (8u * (c & 3u));
        }
    }
};
// register `reg` of lane (h, n) after the instruction, from the B fragments of lanes (0, n) and (1, n)
constexpr int32_t line_mfma_model(const LineMfmaTable &t, const uint32_t (&b0)[4], const uint32_t (&b1)[4], uint32_t h, uint32_t reg) {
    const uint32_t m = (reg & 3u) + 8u * (reg >> 2) + 4u * h;
    int32_t d = 0;
    for (uint32_t hh = 0u; hh < 2u; hh++)
        for (uint32_t j = 0u; j < 16u; j++) {
            const int32_t av = (int8_t)(t.a[32u * hh + m][j >> 2] >> (8u * (j & 3u)));
            const int32_t bv = (int8_t)((hh ? b1 : b0)[j >> 2] >> (8u * (j & 3u)));
            d += av * bv;
        }
    return d;
}
constexpr bool line_mfma_weights_int8() {
    for (uint32_t q = 0u; q < 16u; q++)
        for (uint32_t c = 0u; c < 16u; c++)
            if (line_mfma_weight(q, c) < 0 || line_mfma_weight(q, c) > 127) return false;
    return true;
}
// every digit 0..10 in every position of every line (digit (k + 3 col + 5 row) mod 11 in cell (row,
// col)), in either lane half, with another board in the other half
constexpr bool line_mfma_ok() {
    const LineMfmaTable t;
    for (uint32_t k = 0u; k < 11u; k++)
        for (uint32_t h = 0u; h < 2u; h++) {
            uint32_t c[16] = {}, mine[4] = {0u, 0u, 0u, 0u}, other[4] = {0u, 0u, 0u, 0u};
            for (uint32_t i = 0u; i < 16u; i++) {
                c[i] = (k + 3u * (i & 3u) + 5u * (i >> 2)) % 11u;
                mine[i >> 2] |= c[i] << (8u * (i & 3u));
                other[i >> 2] |= ((c[i] + 1u + i) % 11u) << (8u * (i & 3u));
            }
            for (uint32_t r = 0u; r < 4u; r++) {
                const uint32_t lo_r = (uint32_t)line_mfma_model(t, h ? other : mine, h ? mine : other, h, r);
                const uint32_t hi_r = (uint32_t)line_mfma_model(t, h ? other : mine, h ? mine : other, h, 8u + r);
                const uint32_t lo_c = (uint32_t)line_mfma_model(t, h ? other : mine, h ? mine : other, h, 4u + r);
                const uint32_t hi_c = (uint32_t)line_mfma_model(t, h ? other : mine, h ? mine : other, h, 12u + r);
                if (lo_r > 960u || hi_r > 120u || lo_c > 960u || hi_c > 120u) return false;
                if (lo_r + kLineHiScale * hi_r != 8u * g2048::lut::line11_index(c[4 * r], c[4 * r + 1], c[4 * r + 2], c[4 * r + 3])) return false;
                if (lo_c + kLineHiScale * hi_c != 8u * g2048::lut::line11_index(c[r], c[4 + r], c[8 + r], c[12 + r])) return false;
            }
        }
    return true;
}
static_assert(line_mfma_weights_int8(), "the MFMA address weights fit int8");
static_assert(line_mfma_ok(), "the MFMA address model against line11_index");
__device__ const LineMfmaTable kLineMfmaA __attribute__((aligned(16))) = LineMfmaTable();
// this lane's A fragment; call it with all 64 lanes of the wave active
__device__ __forceinline__ i32x4 line_mfma_frag() {
    return *reinterpret_cast<const i32x4 *>(kLineMfmaA.a[threadIdx.x & 63u]);
}
// the 16 limbs of a board (q < 8 lo, q + 8 hi) and the addresses from them
__device__ __forceinline__ i32x16 line11_limbs_mfma(const uint4 &b, const i32x4 &fa) {
    const i32x4 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w};
    const i32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, bv, zero, 0, 0, 0);
}
__device__ __forceinline__ void line11_addrs_from_limbs(const i32x16 &d, uint32_t (&ra)[4], uint32_t (&ca)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ra[i] = __umul24((uint32_t)d[8 + i], kLineHiScale) + (uint32_t)d[i];
        ca[i] = __umul24((uint32_t)d[12 + i], kLineHiScale) + (uint32_t)d[4 + i];
    }
}
// line11_addrs' interface plus the A fragment
__device__ __forceinline__ void line11_addrs_mfma(const uint4 &b, const i32x4 &fa, uint32_t (&ra)[4], uint32_t (&ca)[4]) {
    line11_addrs_from_limbs(line11_limbs_mfma(b, fa), ra, ca);
}
__device__ __forceinline__ uint2 lds_rec(const uint32_t *tab, uint32_t addr) {
    return *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(tab) + addr);
}
__device__ __forceinline__ uint32_t lds_word(const uint32_t *tab, uint32_t addr) {  // a record's first word
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(tab) + addr);
}
__device__ __forceinline__ uint32_t lds_half(const uint32_t *tab, uint32_t addr) {
    return *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(tab) + addr);
}

// nibble-packed line (dword 0 of a kLine11 record) -> line dword with one exponent per byte, the
// start-slid half (bits 0..15) or the end-slid half (bits 16..31) by the selector: nibble j of a half
// is the low nibble of byte j/2 of e (j even) or of e >> 4 (j odd), so one v_perm over (e >> 4, e)
// places all four and a mask clears the high nibbles ("unpack_row": the step did this per line up to
// round 13; unpack_transpose_model below keeps it as the reference of the network that replaced it).
constexpr uint32_t kUnpackStartSel = 0x05010400u;  // bytes {n0, n1, n2, n3}: an interleave of the low byte pairs
constexpr uint32_t kUnpackEndSel = 0x07030602u;    // bytes {n4, n5, n6, n7}: of the high byte pairs

// The moved board from dword 0 of the four slid lines' records e0..e3 (rows for a horizontal move,
// columns for a vertical one) without an unpack per line, a transpose and a select per row.  One
// v_perm packs the chosen halves of two lines into a register (lines 0 and 2, lines 1 and 3), in the
// byte order {A.b0, A.b1, B.b0, B.b1} for a horizontal move and {A.b0, B.b0, A.b1, B.b1} for a vertical
// one; the end-slid half is the start-slid selector + 2 in every byte.  Split into low and high
// nibbles, the 16 digits d(line, position) then sit one per byte:
//                 horizontal                 vertical
//   xl02   d00 d02 d20 d22            d00 d20 d02 d22
//   xh02   d01 d03 d21 d23            d01 d21 d03 d23
//   xl13   d10 d12 d30 d32            d10 d30 d12 d32
//   xh13   d11 d13 d31 d33            d11 d31 d13 d33
// and every row of the board is the same byte interleave in both orientations (kUnpackStartSel for
// rows 0 / 1, kUnpackEndSel for rows 2 / 3); only one source of each pair depends on the orientation:
// rows 0 / 2 interleave xl02 with xh02 (horizontal: d00 d01 d02 d03) or xl13 (vertical: d00 d10 d20
// d30), rows 1 / 3 interleave xl13 (horizontal) or xh02 (vertical) with xh13.  2 perms, 2 shifts, 4
// ands, 2 selects and 4 perms behind the selector, for 12 + 8 + 4 of unpack_row x 4, transpose, sel4.
constexpr uint32_t kPackRowsSel = 0x05040100u;  // horizontal, start-slid: bytes {A.b0, A.b1, B.b0, B.b1}
constexpr uint32_t kPackColsSel = 0x05010400u;  // vertical, start-slid: bytes {A.b0, B.b0, A.b1, B.b1}
constexpr uint32_t kPackEndAdd = 0x02020202u;   // + this: the end-slid halves
// v_perm_b32 for the selector bytes the step uses (0..3 bytes of lo, 4..7 bytes of hi, 0x0C zero)
constexpr uint32_t perm_model(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0u;
    for (uint32_t j = 0u; j < 4u; j++) {
        const uint32_t s = (sel >> (8u * j)) & 0xFFu;
        r |= (s < 8u ? (uint32_t)(src >> (8u * s)) & 0xFFu : 0u) << (8u * j);
    }
    return r;
}
struct Rows4 {  // uint4 has no constexpr constructor
    uint32_t x, y, z, w;
};
constexpr Rows4 orient_rows_model(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, bool vert, bool rev) {
    const uint32_t psel = (vert ? kPackColsSel : kPackRowsSel) + (rev ? kPackEndAdd : 0u);
    const uint32_t x02 = perm_model(e2, e0, psel), x13 = perm_model(e3, e1, psel);
    const uint32_t xl02 = x02 & 0x0F0F0F0Fu, xh02 = (x02 >> 4) & 0x0F0F0F0Fu;
    const uint32_t xl13 = x13 & 0x0F0F0F0Fu, xh13 = (x13 >> 4) & 0x0F0F0F0Fu;
    const uint32_t pA = vert ? xl13 : xh02, pB = vert ? xh02 : xl13;
    return Rows4{perm_model(pA, xl02, kUnpackStartSel), perm_model(xh13, pB, kUnpackStartSel),
                 perm_model(pA, xl02, kUnpackEndSel), perm_model(xh13, pB, kUnpackEndSel)};
}
// unpack_row x 4, board.hpp's transpose and sel4(vert, ...), the form the network replaces
constexpr Rows4 unpack_transpose_model(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, bool vert, bool rev) {
    const uint32_t usel = rev ? kUnpackEndSel : kUnpackStartSel;
    const uint32_t w[4] = {perm_model(e0 >> 4, e0, usel) & 0x0F0F0F0Fu, perm_model(e1 >> 4, e1, usel) & 0x0F0F0F0Fu,
                           perm_model(e2 >> 4, e2, usel) & 0x0F0F0F0Fu, perm_model(e3 >> 4, e3, usel) & 0x0F0F0F0Fu};
    const uint32_t p = perm_model(w[1], w[0], 0x05010400u), q = perm_model(w[1], w[0], 0x07030602u);
    const uint32_t u = perm_model(w[3], w[2], 0x05010400u), v = perm_model(w[3], w[2], 0x07030602u);
    if (!vert) return Rows4{w[0], w[1], w[2], w[3]};
    return Rows4{perm_model(u, p, 0x05040100u), perm_model(u, p, 0x07060302u), perm_model(v, q, 0x05040100u),
                 perm_model(v, q, 0x07060302u)};
}
// both orientations, both halves, and record words that put every digit 0..10 in every nibble
// position of every one of the four records (digit (k + 3 j + 5 i) mod 11 in nibble j of record i)
constexpr bool orient_rows_ok() {
    for (uint32_t k = 0u; k < 11u; k++) {
        uint32_t e[4] = {0u, 0u, 0u, 0u};
        for (uint32_t i = 0u; i < 4u; i++)
            for (uint32_t j = 0u; j < 8u; j++) e[i] |= ((k + 3u * j + 5u * i) % 11u) << (4u * j);
        for (uint32_t o = 0u; o < 4u; o++) {
            const Rows4 n = orient_rows_model(e[0], e[1], e[2], e[3], (o & 2u) != 0u, (o & 1u) != 0u);
            const Rows4 r = unpack_transpose_model(e[0], e[1], e[2], e[3], (o & 2u) != 0u, (o & 1u) != 0u);
            if (n.x != r.x || n.y != r.y || n.z != r.z || n.w != r.w) return false;
        }
    }
    return true;
}
static_assert(orient_rows_ok(), "the orientation network against unpack_row, transpose and sel4");
// psel = the pack selector of the move (orient_rows_model's)
__device__ __forceinline__ uint4 orient_rows(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t psel, bool vert) {
    const uint32_t x02 = __builtin_amdgcn_perm(e2, e0, psel), x13 = __builtin_amdgcn_perm(e3, e1, psel);
    const uint32_t xl02 = x02 & 0x0F0F0F0Fu, xh02 = (x02 >> 4) & 0x0F0F0F0Fu;
    const uint32_t xl13 = x13 & 0x0F0F0F0Fu, xh13 = (x13 >> 4) & 0x0F0F0F0Fu;
    const uint32_t pA = vert ? xl13 : xh02, pB = vert ? xh02 : xl13;
    return make_uint4(__builtin_amdgcn_perm(pA, xl02, kUnpackStartSel), __builtin_amdgcn_perm(xh13, pB, kUnpackStartSel),
                      __builtin_amdgcn_perm(pA, xl02, kUnpackEndSel), __builtin_amdgcn_perm(xh13, pB, kUnpackEndSel));
}

// Copy the tables (kLine11, kFresh, kFreshLines) into LDS by LDS-DMA: each wave instruction moves 1 KiB (16 B per lane)
// straight from global memory into LDS with no VGPR staging, and every piece of the wave is in
// flight before the single wait (one L2/MALL round trip per launch instead of one per batch).
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;
// kStatPieces = how much of the statistics pairs the kernel's allocation holds (kFreshStatPieces: all of
// them, kRolloutLdsWords; kSearchStatPieces: kSearchLdsWords).
template <uint32_t kStatPieces = kFreshStatPieces>
__device__ __forceinline__ void stage_row_table(uint32_t *s_row) {
    constexpr int kLinePieces = (int)(kLineLdsBytes / 1024u);                 // 115 pieces of 1 KiB
    constexpr int kFreshPieces = (int)(g2048::lut::kFreshEntries * 16u / 1024u);     // + 15 boards + 15 line addresses + 8 stats
    static_assert(kLineLdsBytes % 1024u == 0u && g2048::lut::kFreshEntries * 16u % 1024u == 0u, "whole 1 KiB pieces");
    static_assert(sizeof(kLine11.v) == kLineLdsBytes && sizeof(kFresh.b) == kFreshPieces * 1024 &&
                  sizeof(kFreshLines.a) == kFreshPieces * 1024 && sizeof(kFresh.st) == 1024u * kFreshStatPieces &&
                  kStatPieces <= kFreshStatPieces, "table sizes");
    constexpr int kAll = kLinePieces + 2 * kFreshPieces + (int)kStatPieces;  // the LDS layout is the pieces in this order
    static_assert(kAll * 1024 == (int)(kFreshStatBase + 1024u * kStatPieces), "the pieces fill the allocation");
    const char *src = reinterpret_cast<const char *>(kLine11.v);
    const char *src2 = reinterpret_cast<const char *>(kFresh.b);
    const char *src3 = reinterpret_cast<const char *>(kFreshLines.a);
    const char *src4 = reinterpret_cast<const char *>(kFresh.st);
    char *dst = reinterpret_cast<char *>(s_row);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int c = wave; c < kAll; c += nw) {
        const char *g;
        if (c < kLinePieces) g = src + 1024 * c;
        else if (c < kLinePieces + kFreshPieces) g = src2 + 1024 * (c - kLinePieces);
        else if (c < kLinePieces + 2 * kFreshPieces) g = src3 + 1024 * (c - kLinePieces - kFreshPieces);
        else g = src4 + 1024 * (c - kLinePieces - 2 * kFreshPieces);
        __builtin_amdgcn_global_load_lds((glb_void_t *)(g + 16 * lane), (lds_void_t *)(dst + 1024 * c), 16, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) lgkmcnt(0): this wave's pieces have landed
    __syncthreads();
}

}  // namespace
