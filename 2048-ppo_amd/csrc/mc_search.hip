// mc_search.hip -- pure Monte-Carlo playout search (g2048_mc_search of include/g2048.h):
// mc_search_kernel plays, for every root board and every action, P random-legal games of at most D
// moves out of the kLine11 LDS table and sums their points per (board, action).  A playout step is
// env_rollout_kernel's (rollout_step.hpp) with kTraj = false: no trajectory record, no potentials and
// no auto-reset.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.hpp"
#include "rowtable.hpp"
#include "line11_lds.hpp"
#include "step.hpp"
#include "rollout_step.hpp"
#include "launch_util.hpp"
#include "../../include/g2048.h"

using namespace g2048;

namespace {

constexpr int64_t kMaxPlayouts = 4096, kMaxDepth = 65536;

// The playout of one lane from the board after its forced move (s.b, s.legal != 0, s.M set): up to
// `depth` steps of rollout_step<kOdd, kSmall, kTraj = false>, step t on word (c + t) & 1 of the
// stream-1 draw at counter (c + t) >> 1, stopped by the first step that leaves no legal move.  A lane
// leaves the loops at its own end; the wave leaves them when its last lane has.
__device__ __forceinline__ void mc_playout(RolloutLane &s, const uint32_t *__restrict__ tab, uint64_t seed, uint64_t c,
                                           uint32_t env, int depth) {
    refill_lines(s, tab, s.M);
    const TrajRows none{};  // no record: a kTraj = false step does not touch it
    uint64_t pair = c >> 1;
    s.D = philox_draw(seed, pair, env, 1u);
    s.ph = philox_start(seed, pair + 1u, env, 1u);
    int t = 0;
    if (c & 1u) {  // the playout starts on the second step of a pair
        philox_rounds<0, 5>(s.ph);
        rollout_step<true, false, false>(s, tab, none, seed, pair + 2u, env);
        pair++;
        t = 1;
    }
    for (; s.legal != 0u && t + 2 <= depth; t += 2, pair++) {
        // every playing board of the wave <= 2^8 at the pair's start: both steps stay inside kLine11
        if (__all(s.M <= kFastPairMax)) {
            rollout_step<false, true, false>(s, tab, none, seed, pair + 2u, env);
            if (s.legal == 0u) break;
            rollout_step<true, true, false>(s, tab, none, seed, pair + 2u, env);
        } else {
            rollout_step<false, false, false>(s, tab, none, seed, pair + 2u, env);
            if (s.legal == 0u) break;
            rollout_step<true, false, false>(s, tab, none, seed, pair + 2u, env);
        }
    }
    if (s.legal != 0u && t < depth) rollout_step<false, false, false>(s, tab, none, seed, pair + 2u, env);
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
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kSearchLdsWords];
    stage_row_table<kSearchStatPieces>(s_row);
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
                RolloutLane s;
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
    if (!philox_mode(rng)) return G2048_EINVAL;
    if (playouts < 1 || playouts > kMaxPlayouts || depth < 0 || depth > kMaxDepth) return G2048_EINVAL;
    if (n < 0 || n >= (int64_t(1) << 31) || n * 4 * playouts >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !score_sum || !aligned16(score_sum) || !aligned16(move_sum) || !workspace ||
        ((uintptr_t)workspace & 3u) || workspace_bytes_in < workspace_bytes(n) || !counter_dev_aligned(rng))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (unsigned long long *)score_sum, (unsigned long long *)move_sum, (uint32_t *)workspace,
                       (uint32_t)n);
    const int zs = launch_status();
    if (zs != G2048_OK) return zs;
    const int64_t total = n * 4 * playouts;
    const PersistentShape sh = persistent_shape(total);
    hipLaunchKernelGGL(mc_search_kernel, dim3(sh.grid), dim3(sh.threads), 0, st, (const uint4 *)boards,
                       (uint32_t)total, (uint32_t)playouts, (int)depth, rng_args(rng),
                       (unsigned long long *)score_sum, (unsigned long long *)move_sum, legal, best,
                       (uint32_t *)workspace);
    return launch_status();
}

}  // extern "C"
