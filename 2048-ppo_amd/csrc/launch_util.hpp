// launch_util.hpp -- host-side helpers shared by the libg2048 translation units that launch the
// env and search kernels (g2048.hip, env_rollout.hip, mc_search.hip, expectimax.hip, ntuple.hip,
// ntuple_search.hip): the launch status, the alignment and g2048_rng checks, the RngArgs copy and the
// launch shape of the kernels that keep the kLine11 tables in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "step.hpp"
#include "../../include/g2048.h"

namespace {

inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : (int)e;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0u; }

// the g2048_rng checks of the Philox-only entry points: the mode, and the 8-byte alignment of the
// device counter where the caller gives one
inline bool philox_mode(const g2048_rng *r) { return r && r->mode == G2048_RNG_PHILOX; }
inline bool counter_dev_aligned(const g2048_rng *r) { return ((uintptr_t)r->counter_dev & 7u) == 0u; }

inline g2048::RngArgs rng_args(const g2048_rng *r) {
    g2048::RngArgs a{};
    if (r) {
        a.seed = r->seed;
        a.counter = r->counter;
        a.counter_dev = r->counter_dev;
        a.env_base = r->env_base;
        a.mt = r->mt_state;
        a.inject = r->inject;
    }
    return a;
}

// Launch shape of env_rollout_kernel and mc_search_kernel over `total` lanes: one workgroup per CU
// holds the 149 KiB LDS tables and is persistent over the lanes; its size scales with the lane count
// up to 1024 threads (whole waves), so that a large count runs 4 waves per SIMD while 65 536 lanes
// still spread over all 256 CUs.
struct PersistentShape {
    unsigned grid, threads;
};
inline PersistentShape persistent_shape(int64_t total) {
    int64_t threads = (total + 255) / 256;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : ((threads + 63) / 64) * 64;
    int64_t grid = (total + threads - 1) / threads;
    grid = grid > 256 ? 256 : grid;
    return PersistentShape{(unsigned)grid, (unsigned)threads};
}

}  // namespace
