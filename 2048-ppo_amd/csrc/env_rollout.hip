// env_rollout.hip -- the synthetic random-legal rollout (the bench's headline workload,
// g2048_env_rollout_random / _adv of include/g2048.h): env_rollout_kernel, the fresh_* helpers of its
// launch start and the C ABI.  The step itself (rollout_step<kOdd, kSmall, kTraj = true>, the lane state,
// the auto-reset) is rollout_step.hpp's and the LDS tables and their staging are line11_lds.hpp's, both
// shared with mc_search.hip.  A translation unit of its own so that it alone is built with the machine scheduler's occupancy bias
// at 0 (Makefile: one wave per SIMD at the benchmark size, where the issue schedule, not occupancy,
// sets the step time; the rest of libg2048 keeps the default bias).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "board.hpp"
#include "rowtable.hpp"
#include "line11_lds.hpp"
#include "step.hpp"
#include "rollout_step.hpp"
#include "launch_util.hpp"
#include "../../include/g2048.h"

using namespace g2048;

namespace {

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

// Synthetic random-legal rollout (the benchmark workload of BASELINE.md): `steps` env steps per
// board per launch, board in registers, auto-reset on done, one time-major trajectory record per
// step: the board the action was taken on [T][N][16], action, points, potentials, flags.
// Step c (absolute Philox counter) takes word c & 1 of the stream-1 draw at counter c >> 1, so one
// Philox draw serves two steps (and the reset that may end one of them).  The legal mask is
// carried from the previous step (the action is always legal), and so are the kLine11 records of
// the board's rows and columns, which hold the move in every direction (their first words; of the
// second words, the sum and the maximum per orientation, which give the move's points and the slid
// lines' maximum): a step's only table reads are the records of the board it produces.  A board
// holding an exponent > 10 takes the SWAR compute path.  Workgroups are persistent over boards, so
// large N keeps several waves per SIMD with one LDS table per CU.
// kAddr = how a step forms its line addresses (rollout_step.hpp): the host takes the MFMA form where the
// grid covers every board (up to 262 144 boards, one trip through the board loop; the benchmark's 65 536
// boards, one wave per SIMD, among them: the kernel is issue-bound there and the form is 5 % faster) and
// the VALU form above that.  With the wide stores the MFMA form lost at four waves per SIMD (profiles/r15a:
// its per-pair scratch reload and the wait behind it); with the narrow stores, which leave no scratch, it
// is 4 % faster than the VALU form at 98 304 .. 524 288 boards in every round and within the noise of the
// measurement at 2^20 and 2^21 (profiles/r16a/ab_large_n*.log), so the several-trips sizes keep the VALU form.
// kWide = how a step addresses its record (rollout_step.hpp TrajRows / TrajRowsNarrow): the narrow form,
// uniform array bases and 32-bit lane offsets, wherever 16 n steps <= 2^32 (the benchmark's 2^26 env-steps
// per launch among them), the wide form's 64-bit lane pointers above that (rollout_form below).
template <int kAddr, bool kWide>
__global__ __launch_bounds__(1024) void env_rollout_kernel(uint4 *__restrict__ boards, int64_t n, int64_t steps,
                                                           uint4 *__restrict__ tb, uint8_t *__restrict__ ta,
                                                           int32_t *__restrict__ tp, uint32_t *__restrict__ tpot,
                                                           uint8_t *__restrict__ tf, RngArgs rng,
                                                           uint32_t *__restrict__ ticket) {
    // kLine11, then kFresh and kFreshLines (the layout is line11_lds.hpp's, the address bounds are rollout_step.hpp's)
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kRolloutLdsWords];
    // The MFMA's constant operand, loaded once per wave here, where all 64 lanes are active: the
    // instruction reads its operands in every lane whatever EXEC says, so a fragment written (or
    // rematerialised) under the board loop's partial EXEC would leave garbage in the rows that belong
    // to the inactive lanes, for every board of the wave.  The empty asm behind the barrier makes the
    // registers an asm result -- nothing the compiler can recompute or sink into the loop -- and costs
    // no instruction; a pin at the use site would cost two v_mov_b64 per step.
    i32x4 fa{};
    if constexpr (kAddr != kAddrValu) fa = line_mfma_frag();
    stage_row_table(s_row);
    if constexpr (kAddr != kAddrValu) asm volatile("" : "+v"(fa));
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
            s.S = carry_pack(ms);
        } else {
            s.S = carry_pack(mono_stats(s.b));
        }
        s.empt_b = emptiness(s.b);
        uint64_t pair = ctr0 >> 1;
        s.D = philox_draw(rng.seed, pair, env, 1u);
        s.ph = philox_start(rng.seed, pair + 1u, env, 1u);
        fresh_prep(s, s_row);
        refill_lines<kAddr, true>(s, s_row, s.S >> 24, fa);
        // the record addresses of this board, from its own index in every trip of the board loop: wide,
        // per-lane pointers advanced one row (n elements) per step and no array base in an SGPR pair across
        // the loop; narrow, the five bases in SGPR pairs and three lane offsets advanced per step
        using Rows = std::conditional_t<kWide, TrajRows, TrajRowsNarrow>;
        Rows tr = Rows::at(tb, ta, tp, tpot, tf, li);
        uint64_t left = (uint64_t)steps;  // steps still to run
        if ((ctr0 & 1u) && left > 0u) {  // the launch starts on the second step of a pair
            philox_rounds<0, 5>(s.ph);
            rollout_step<true, false, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
            tr.next(n);
            pair++;
            left--;
        }
        // The pair loop counts down to zero.  A 64-bit `t + 2 <= steps` has no scalar compare: it was a
        // v_mov_b64 + v_cmp_le_i64 feeding the back edge's s_cbranch_vccz plus two 64-bit scalar adds
        // per pair; `!= 0` is one s_cmp_lg_u64 (-6 instructions per pair, -2.3 % per launch: DESIGN.md
        // section 6, round 11)
        for (uint64_t pairs = left >> 1; pairs != 0u; pairs--, pair++) {
            // every board of the wave <= 2^8 at the pair's start: both steps stay inside kLine11
            // (a move adds at most 1 to the maximum), so the pair runs without the fallback branches
            // and without masking its addresses.  The other pair keeps the carried records valid in
            // every lane whose board is <= 2^10, so a wave changes between the two freely.
            if (__all(s.S < ((kFastPairMax + 1u) << 24))) {
                rollout_step<false, true, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
                tr.next(n);
                rollout_step<true, true, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
            } else {
                rollout_step<false, false, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
                tr.next(n);
                rollout_step<true, false, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
            }
            tr.next(n);
        }
        if (left & 1u) rollout_step<false, false, true, kAddr, Rows>(s, s_row, tr, rng.seed, pair + 2u, env, fa);
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
    if (!rng || !rng->counter_dev || !ticket || !counter_dev_aligned(rng) || ((uintptr_t)ticket & 3u))
        return G2048_EINVAL;
    return rollout_launch(stream, boards, n, steps, traj_boards, traj_actions, traj_points, traj_pot, traj_flags, rng,
                          ticket);
}

// The kernel a launch of n boards x steps takes, as G2048_ROLLOUT_FORM_* bits (include/g2048.h); a refused
// shape gives G2048_EINVAL.
//  - n < 2^28: a lane's byte offset into a trajectory row (16 * board id) fits 32 bits.
//  - MFMA line addresses where the grid covers every board, i.e. up to 256 workgroups x 1024 threads (the
//    kernel's comment): that kernel never makes a second trip through its board loop.
//  - narrow record addressing while a lane's byte offset into the whole boards record fits 32 bits:
//    16 n steps <= 2^32, compared as steps <= floor(2^28 / n) (n * steps may not fit 64 bits).
static int rollout_form(int64_t n, int64_t steps) {
    if (n < 0 || n >= (int64_t(1) << 28) || steps < 0) return G2048_EINVAL;
    int form = 0;
    const PersistentShape sh = persistent_shape(n);
    if ((int64_t)sh.grid * sh.threads >= n) form |= G2048_ROLLOUT_FORM_MFMA;
    if (n > 0 && steps > (int64_t(1) << 28) / n) form |= G2048_ROLLOUT_FORM_WIDE;
    return form;
}

int g2048_env_rollout_form(int64_t n, int64_t steps) { return rollout_form(n, steps); }

// g2048_env_rollout_force_wide: read by every launch after it is set
static std::atomic<int> g_force_wide{0};

int g2048_env_rollout_force_wide(int on) { return g_force_wide.exchange(on != 0); }

static int rollout_launch(g2048_stream_t stream, int8_t *boards, int64_t n, int64_t steps, int8_t *traj_boards,
                          uint8_t *traj_actions, int32_t *traj_points, int8_t *traj_pot, uint8_t *traj_flags,
                          const g2048_rng *rng, uint32_t *ticket) {
    int form = rollout_form(n, steps);
    if (form < 0 || !philox_mode(rng)) return G2048_EINVAL;
    if (n == 0 || steps == 0) return G2048_OK;
    if (!boards || !traj_boards || !traj_actions || !traj_points || !traj_pot || !traj_flags || !aligned16(boards) ||
        !aligned16(traj_boards) || ((uintptr_t)traj_pot & 3u) || ((uintptr_t)traj_points & 3u))
        return G2048_EINVAL;
    if (g_force_wide.load(std::memory_order_relaxed)) form |= G2048_ROLLOUT_FORM_WIDE;
    const PersistentShape sh = persistent_shape(n);
    const bool mfma = form & G2048_ROLLOUT_FORM_MFMA, wide = form & G2048_ROLLOUT_FORM_WIDE;
    const auto kernel = mfma ? (wide ? env_rollout_kernel<kAddrMfma, true> : env_rollout_kernel<kAddrMfma, false>)
                             : (wide ? env_rollout_kernel<kAddrValu, true> : env_rollout_kernel<kAddrValu, false>);
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(sh.threads), 0, (hipStream_t)stream,
                       (uint4 *)boards, n, steps, (uint4 *)traj_boards, traj_actions, traj_points, (uint32_t *)traj_pot,
                       traj_flags, rng_args(rng), ticket);
    return launch_status();
}

}  // extern "C"
