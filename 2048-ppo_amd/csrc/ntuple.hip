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
// no-return 32-bit atomic adds of the same shape.  A TD step is two launches: nt_td_eval_kernel only
// reads the weights (choice, target, delta), nt_td_update_kernel only adds to them and steps the env,
// and stream order between the two makes every read see the weights before the step's updates.
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
template <int K>
__device__ __forceinline__ void nt_add(const NtArgs &net, uint64_t x, int32_t D) {
    for (int t = 0; t < net.T; t++) {
        uint32_t *W = (uint32_t *)net.w + ((size_t)t << (4 * K));
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

template <int K>
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
            c.q[a] = ((long long)pts << kFrac) + nt_value<K>(net, nt_pack(s));
            c.legal |= 1u << a;
            if (c.best == 0xFFu || c.q[a] > bq) {
                bq = c.q[a];
                c.best = a;
            }
        }
    }
    return c;
}

template <int K>
__global__ __launch_bounds__(256) void nt_value_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                       long long *__restrict__ value, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    value[i] = nt_value<K>(net, nt_pack(boards[i]));
}

template <int K>
__global__ __launch_bounds__(256) void nt_choose_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                        long long *__restrict__ q, uint8_t *__restrict__ legal,
                                                        uint8_t *__restrict__ best, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const NtChoice c = nt_choose<K>(net, boards[i]);
    if (q) {
        reinterpret_cast<longlong2 *>(q)[2u * i] = make_longlong2(c.q[0], c.q[1]);
        reinterpret_cast<longlong2 *>(q)[2u * i + 1u] = make_longlong2(c.q[2], c.q[3]);
    }
    if (legal) legal[i] = (uint8_t)c.legal;
    if (best) best[i] = (uint8_t)c.best;
}

// TD step, the reading half: the greedy action of the board and the D of the pending after-state
template <int K>
__global__ __launch_bounds__(256) void nt_td_eval_kernel(NtArgs net, const uint4 *__restrict__ boards,
                                                         const uint4 *__restrict__ after,
                                                         const uint8_t *__restrict__ pending, int lr_shift,
                                                         int32_t *__restrict__ ws_d, uint8_t *__restrict__ ws_act,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const NtChoice c = nt_choose<K>(net, boards[i]);
    long long target = 0;
#pragma unroll
    for (uint32_t a = 0u; a < 4u; a++) target = c.best == a ? c.q[a] : target;
    const uint32_t p = pending[i];
    long long D = 0;
    if (p != 0u) {
        const long long delta = (p == 2u ? 0 : target) - nt_value<K>(net, nt_pack(after[i]));
        D = (delta + (1ll << (lr_shift - 1))) >> lr_shift;
        D = D < -kMaxD ? -kMaxD : D > kMaxD ? kMaxD : D;
    }
    ws_d[i] = (int32_t)D;
    ws_act[i] = (uint8_t)c.best;
}

// TD step, the writing half: the update of the pending after-state, then g2048_env_step with the
// greedy action and auto-reset at counter c + t, the running score and the carried state
template <int K>
__global__ __launch_bounds__(256) void nt_td_update_kernel(NtArgs net, uint4 *__restrict__ boards,
                                                           uint4 *__restrict__ after, uint8_t *__restrict__ pending,
                                                           long long *__restrict__ run_score,
                                                           const int32_t *__restrict__ ws_d,
                                                           const uint8_t *__restrict__ ws_act, RngArgs rng, uint64_t t,
                                                           long long *__restrict__ stats, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < n;
    bool updated = false;
    if (valid) {
        const uint32_t p = pending[i];
        const int32_t D = ws_d[i];
        updated = p != 0u;
        if (updated && D != 0) nt_add<K>(net, nt_pack(after[i]), D);
        const uint32_t act = ws_act[i];
        const bool has_move = act != 0xFFu;
        const uint32_t a = has_move ? act : 0u;
        uint4 b = boards[i];
        uint32_t pts, mx;
        const uint4 moved = apply_move(b, a, pts, mx);
        const StepResult res = step_board<G2048_RNG_PHILOX>(b, true, a, nullptr, rng, (int64_t)i, rng_counter(rng) + t,
                                                            G2048_OPT_AUTO_RESET);
        long long rs = run_score[i] + (long long)res.pts;
        const bool done = (res.fl & FLAG_DONE) != 0u;
        if (done) {
            if (stats) {
                __hip_atomic_fetch_add(stats + 0, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(stats + 1, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(stats + 2, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            rs = 0;
        }
        run_score[i] = rs;
        boards[i] = b;
        if (has_move) after[i] = moved;
        pending[i] = (uint8_t)(has_move ? (done ? 2u : 1u) : 0u);
    }
    if (stats) {  // one add per wave of its updates applied
        const unsigned long long m = __ballot(updated);
        if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m))
            __hip_atomic_fetch_add(stats + 3, (long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
size_t td_workspace_bytes(int64_t n) { return align16((size_t)n * 4) + align16((size_t)n); }

}  // namespace

extern "C" {

size_t g2048_ntuple_weight_count(const g2048_ntuple_net *net) {
    NtArgs a;
    if (!make_args(net, a)) return 0;
    return (size_t)net->num_tuples << (4 * net->tuple_len);
}

int g2048_ntuple_value(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *value,
                       int64_t n) {
    NtArgs a;
    if (!make_args(net, a) || n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !value) return G2048_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    G2048_NT_DISPATCH(net->tuple_len, hipLaunchKernelGGL(nt_value_kernel<kK>, grid, block, 0, (hipStream_t)stream, a,
                                                         (const uint4 *)boards, (long long *)value, (uint32_t)n));
    return launch_status();
}

int g2048_ntuple_choose(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *q,
                        uint8_t *legal, uint8_t *best, int64_t n) {
    NtArgs a;
    if (!make_args(net, a) || n < 0 || n >= (int64_t(1) << 31)) return G2048_EINVAL;
    if (!q && !legal && !best) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !aligned16(q)) return G2048_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    G2048_NT_DISPATCH(net->tuple_len, hipLaunchKernelGGL(nt_choose_kernel<kK>, grid, block, 0, (hipStream_t)stream, a,
                                                         (const uint4 *)boards, (long long *)q, legal, best,
                                                         (uint32_t)n));
    return launch_status();
}

size_t g2048_ntuple_td_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (int64_t(1) << 28)) return 0;
    return td_workspace_bytes(n < 1 ? 1 : n);
}

int g2048_ntuple_td(g2048_stream_t stream, const g2048_ntuple_net *net, int8_t *boards, int8_t *after,
                    uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                    const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes_in) {
    NtArgs a;
    if (!make_args(net, a) || n < 0 || n >= (int64_t(1) << 28)) return G2048_EINVAL;
    if (steps < 1 || lr_shift < 1 || lr_shift > 30) return G2048_EINVAL;
    if (!philox_mode(rng) || !counter_dev_aligned(rng)) return G2048_EINVAL;
    if (n == 0) return G2048_OK;
    if (!boards || !aligned16(boards) || !after || !aligned16(after) || !pending || !run_score ||
        ((uintptr_t)run_score & 7u) || ((uintptr_t)stats & 7u) || !workspace || !aligned16(workspace) ||
        workspace_bytes_in < td_workspace_bytes(n))
        return G2048_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int32_t *ws_d = (int32_t *)workspace;
    uint8_t *ws_act = (uint8_t *)workspace + align16((size_t)n * 4);
    const RngArgs r = rng_args(rng);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    for (int64_t t = 0; t < steps; t++) {
        G2048_NT_DISPATCH(net->tuple_len,
                          hipLaunchKernelGGL(nt_td_eval_kernel<kK>, grid, block, 0, st, a, (const uint4 *)boards,
                                             (const uint4 *)after, (const uint8_t *)pending, (int)lr_shift, ws_d, ws_act,
                                             (uint32_t)n));
        int s = launch_status();
        if (s != G2048_OK) return s;
        G2048_NT_DISPATCH(net->tuple_len,
                          hipLaunchKernelGGL(nt_td_update_kernel<kK>, grid, block, 0, st, a, (uint4 *)boards,
                                             (uint4 *)after, pending, (long long *)run_score, (const int32_t *)ws_d,
                                             (const uint8_t *)ws_act, r, (uint64_t)t, (long long *)stats, (uint32_t)n));
        s = launch_status();
        if (s != G2048_OK) return s;
    }
    return G2048_OK;
}

}  // extern "C"
