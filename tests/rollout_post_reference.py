"""What runs between the rollout and the update -- the reward / return-to-go scan with its moment
state (rtg_prepare / rtg_kernel / rtg_reduce / rtg_finalize), the episode scan, the 23 rollout
statistics and the masked-softmax sampler of csrc/g2048.hip -- restated in plain float64 numpy (no
torch, no kernel), plus the case tables tests/test_gpu_rollout_post_edges.py feeds the kernels.
tests/test_rollout_post_host.py proves every function here on the CPU first.

Conventions (include/g2048.h): trajectories are time-major [T, n]; pot [T, n, 4] int8 holds
(mono before, mono after, empt before, empt after); flag bytes carry the legal mask in bits 0-3,
RESET 0x20, INACTIVE 0x40, DONE 0x80; the RTG state is eight doubles
(mu, m2, first moment, step, mu_corrected, std, batch_mean, batch_var).

Sums are taken with math.fsum (correctly rounded), means and variances are two-pass: the reference
carries no summation error of its own, so the bounds of the GPU tests measure the kernels' alone."""

from __future__ import annotations

import math

import numpy as np

FLAG_RESET, FLAG_INACTIVE, FLAG_DONE = 0x20, 0x40, 0x80
KBLOCK = 256      # csrc/g2048.hip kBlock
RTG_UNROLL = 16   # kRtgU
STATS_CHUNK = 8   # rollout_stats_kernel's kChunk
FINAL_STRIDE = 64  # rollout_stats_final_kernel: lanes stride the block partials by 64
EPS = 1e-8
U53 = 2.0 ** -53

GAMMA, W_POINTS, W_MONO, W_EMPT = 0.97, 0.1, 0.3, 0.7
CFG = (GAMMA, W_POINTS, W_MONO, W_EMPT)


# ------------------------------------------------------------------------------ RTG moments -----
def rtg_prepare_terms(state, beta):
    """rtg_prepare_kernel: the bias-corrected mean / std of the PREVIOUS moments, with the branches taken."""
    s = np.array(state, np.float64)
    step = 1.0 if s[3] < 1.0 else float(s[3])
    pw = math.pow(beta, step)
    raw_bc = 1.0 - pw
    bc = max(raw_bc, EPS)
    mu_c, m2_c = s[0] / bc, s[1] / bc
    raw_var = m2_c - mu_c * mu_c
    s[4] = mu_c
    s[5] = math.sqrt(max(raw_var, EPS))
    return {"state": s, "pow": pw, "bc": bc, "bc_clamped": raw_bc < EPS, "var_clamped": raw_var < EPS,
            "step_clamped": float(state[3]) < 1.0}


def rtg_prepare(state, beta):
    return rtg_prepare_terms(state, beta)["state"]


def _ema(state, mean, var, beta):
    s = np.array(state, np.float64)
    s[6], s[7] = mean, var
    mu = beta * s[0] + (1.0 - beta) * mean
    s[1] = beta * s[1] + (1.0 - beta) * (var + mean * mean)
    s[0] = mu
    s[2] = mu
    s[3] = s[3] + 1.0
    return s


def rtg_finalize(state, partials, beta):
    """rtg_finalize_kernel from the three sums (sum dv, sum dv^2, count), dv = G - mu_corrected: the
    kernel's own one-pass formula.  No live step: the state is returned untouched."""
    s1, s2, n = (float(x) for x in partials)
    if n <= 0.0:
        return np.array(state, np.float64)
    m1 = s1 / n
    mean = float(state[4]) + m1
    var = 0.0 if n <= 1.0 else max(s2 / n - m1 * m1, 0.0)
    return _ema(state, mean, var, beta)


def rtg_finalize_exact(state, mean, var, cnt, beta):
    """The same EMA update from the EXACT batch mean / variance rtg_scan returns."""
    if cnt <= 0:
        return np.array(state, np.float64)
    return _ema(state, mean, var, beta)


def rtg_scan(points, pot, flags, value, cfg, state):
    """rtg_kernel on [T, n]: the reward in the kernel's documented operation order (train.py:702-719,
    float64, every product and sum rounded on its own), the reverse discounted scan, the normalisation
    with state[4] / state[5] (dividing, as train.py:751 does) and the advantage.

    Returns reward, g_raw, g_norm, adv (float64 [T, n], zeros on inactive steps), live (bool), the three
    sums s1 = sum dv, s2 = sum dv^2 (dv = fl(G - mu_c), dv^2 = fl(dv * dv): the kernel's fp64 terms,
    summed exactly), cnt, their absolute sums, and the exact batch mean / variance of G over live steps."""
    gamma, wp, wm, we = (float(x) for x in cfg)
    points = np.asarray(points)
    T, n = points.shape
    pot = np.asarray(pot, np.int8).reshape(T, n, 4).astype(np.float64)
    flags = np.asarray(flags, np.uint8).reshape(T, n)
    value = np.asarray(value, np.float32).reshape(T, n).astype(np.float64)
    mu_c, std = float(state[4]), float(state[5])
    out = {k: np.zeros((T, n), np.float64) for k in ("reward", "g_raw", "g_norm", "adv")}
    live = (flags & FLAG_INACTIVE) == 0
    done = (flags & FLAG_DONE) != 0
    G = np.zeros(n, np.float64)
    for t in range(T - 1, -1, -1):
        mb, eb = pot[t, :, 0], pot[t, :, 2]
        ma = np.where(done[t], 0.0, pot[t, :, 1])
        ea = np.where(done[t], 0.0, pot[t, :, 3])
        shaped = wm * (gamma * ma - mb)
        shaped = shaped + we * (gamma * ea - eb)
        r = points[t].astype(np.float64) * wp + shaped
        G = np.where(done[t], 0.0, G)
        G = np.where(live[t], r + gamma * G, 0.0)
        gn = (G - mu_c) / (std + EPS)
        out["reward"][t] = np.where(live[t], r, 0.0)
        out["g_raw"][t] = G
        out["g_norm"][t] = np.where(live[t], gn, 0.0)
        out["adv"][t] = np.where(live[t], gn - value[t], 0.0)
    g = out["g_raw"][live]
    dv = g - mu_c
    cnt = int(live.sum())
    out.update(live=live, cnt=cnt, s1=math.fsum(dv), s2=math.fsum(dv * dv), abs1=math.fsum(np.abs(dv)))
    out["mean"] = math.fsum(g) / cnt if cnt else 0.0
    out["var"] = math.fsum((g - out["mean"]) ** 2) / cnt if cnt > 1 else 0.0
    return out


def sum_bound(T, n):
    """(T + log2 n + 4) 2^-53: the additions one term passes through on its way into a kernel sum (T serial
    ones in the lane, log2 of the lanes / waves / blocks in the trees) plus four for the divisions and the
    final subtraction, each worth half an ulp of the running |sum|."""
    return (T + math.log2(max(n, 1)) + 4.0) * U53


def kernel_order_sums(g_live_tn, live, mu_c):
    """s1, s2 of rtg_kernel + rtg_reduce_kernel in THEIR order of addition, emulated in numpy: per env
    serial over t descending; 64-lane xor butterflies; the block's four waves in order; then the reduce
    kernel (thread k takes blocks k, k + 256, ...; butterflies; waves in order).  g_live_tn: G [T, n]."""
    T, n = g_live_tn.shape
    s1, s2 = np.zeros(n), np.zeros(n)
    for t in range(T - 1, -1, -1):
        dv = g_live_tn[t] - mu_c
        s1 = np.where(live[t], s1 + dv, s1)
        s2 = np.where(live[t], s2 + dv * dv, s2)

    def block_tree(v):  # [blocks * 256] -> [blocks]
        v = v.reshape(-1, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        w = v[:, 0].reshape(-1, KBLOCK // 64)
        t = np.zeros(len(w))
        for k in range(KBLOCK // 64):
            t = t + w[:, k]
        return t

    def reduce(v):
        nb = -(-n // KBLOCK)
        pad = np.zeros(nb * KBLOCK)
        pad[:n] = v
        part = block_tree(pad)
        th = np.zeros(KBLOCK)
        for k0 in range(0, nb, KBLOCK):
            chunk = part[k0:k0 + KBLOCK]
            th[:len(chunk)] = th[:len(chunk)] + chunk
        return float(block_tree(th)[0])
    return reduce(s1), reduce(s2)


def moment_regimes():
    """The four regimes of the variance bound as scan inputs: name -> (case, cfg, mu_c).  gamma = 0 and no
    shaping, so G = points * w_points: returns of spread 3 around 0 (mu_c 0.1), the same at offset 10^6,
    spread 10^-3 at 3 * 10^4 (the one-pass variance loses its leading digit there), and mu_c 2.5 * 10^5 away
    from the data.  T = 37 and n = 300: neither a multiple of the 16-step group nor of the block."""
    g = np.random.default_rng(20)
    T, n = 37, 300
    z = g.standard_normal((T, n))
    flags = np.where(g.random((T, n)) < 0.05, FLAG_INACTIVE, 0).astype(np.uint8)
    base = {"pot": np.zeros((T, n, 4), np.int8), "flags": flags, "value": np.zeros((T, n), np.float32), "T": T, "n": n}

    def case(points):
        return dict(base, points=points.astype(np.int32))
    k3 = np.rint(z * 3000.0)
    return {"centred": (case(k3), (0.0, 1e-3, 0.0, 0.0), 0.1),
            "offset_1e6": (case(1.0e9 + k3), (0.0, 1e-3, 0.0, 0.0), 0.0),
            "tiny_spread_3e4": (case(3.0e8 + np.rint(z * 10.0)), (0.0, 1e-4, 0.0, 0.0), 0.0),
            "mu_c_far": (case(k3), (0.0, 1e-3, 0.0, 0.0), -2.5e5)}


# ------------------------------------------------------------------------------ RTG case tables --
def rtg_case(T, n, seed=0, all_inactive=False):
    """One [T, n] trajectory for the scan.  pot: full int8 range, the four bytes of a step pairwise
    different, -128 / -1 / 127 present; points up to 2^17; the flag table of flag_regimes()."""
    g = np.random.default_rng(1000 * T + n + 7919 * seed)
    points = g.integers(0, (1 << 17) + 1, size=(T, n)).astype(np.int32)
    points[g.random((T, n)) < 0.25] = 0
    # four pairwise different bytes: a random start and three distinct non-zero offsets mod 256
    base = g.integers(0, 256, size=(T, n, 1))
    offs = np.stack([g.permutation(255)[:3] + 1 for _ in range(T * n)]).reshape(T, n, 3) if T * n else \
        np.zeros((T, n, 3), np.int64)
    pot = np.concatenate([base, (base + offs) % 256], axis=2).astype(np.uint8)
    for k in range(min(4, T * n)):   # -128, -1 and 127 in one step, in every rotation of the byte lanes
        pot[(k * 5) % T, (k * 11) % n] = np.roll([0x80, 0xFF, 0x7F, 0x2A], k)
    pot = pot.view(np.int8)
    flags = np.zeros((T, n), np.uint8)
    flags[g.random((T, n)) < 0.08] = FLAG_DONE
    col = {}
    if n >= 1 and T >= 1:
        # dedicated columns, wrapped into range for tiny n: later ones overwrite earlier ones there
        col = {"done_first": 0 % n, "done_last": 1 % n, "inactive_mid": 2 % n, "inactive_tail": 3 % n,
               "all_inactive": 4 % n}
        flags[:, col["done_first"]] &= ~np.uint8(FLAG_INACTIVE)
        flags[0, col["done_first"]] = FLAG_DONE
        flags[T - 1, col["done_last"]] = FLAG_DONE
        if T >= 3:
            e = col["inactive_mid"]
            flags[:, e] = 0
            flags[T // 2, e] = FLAG_INACTIVE            # alone, live steps on both sides
        if T >= 2:
            e = col["inactive_tail"]
            flags[:, e] = 0
            flags[T // 2:, e] = FLAG_INACTIVE | FLAG_DONE
        if n >= 5:
            flags[:, col["all_inactive"]] = FLAG_INACTIVE | FLAG_DONE
        # more of each at random
        rnd = g.random((T, n))
        free = np.ones(n, bool)
        free[list(col.values())] = False
        flags[(rnd < 0.03) & free] = FLAG_INACTIVE
        flags[(rnd > 0.98) & free] = FLAG_INACTIVE | FLAG_DONE
    if all_inactive:
        flags[:] = FLAG_INACTIVE
        flags[g.random((T, n)) < 0.5] |= FLAG_DONE
    noise = (g.integers(0, 16, size=(T, n)) | np.where(g.random((T, n)) < 0.5, FLAG_RESET, 0)
             | np.where(g.random((T, n)) < 0.2, 0x10, 0)).astype(np.uint8)
    flags = flags | noise                             # RESET, INVALID and the legal bits: ignored by the scan
    value = g.standard_normal((T, n)).astype(np.float32)
    return {"points": points, "pot": pot, "flags": flags, "value": value, "T": T, "n": n, "columns": col}


def flag_regimes(case):
    """Counts of each flag regime in an rtg_case (steps unless stated)."""
    f, T = case["flags"], case["T"]
    ina, done = (f & FLAG_INACTIVE) != 0, (f & FLAG_DONE) != 0
    live = ~ina
    mid = np.zeros_like(ina)
    if T >= 3:  # an inactive step with a live step somewhere before AND after it in its column
        before = np.cumsum(live, axis=0) - live > 0
        after = (np.cumsum(live[::-1], axis=0)[::-1] - live) > 0
        mid = ina & before & after
    return {"done": int((done & live).sum()), "inactive_alone_mid": int((mid & ~done).sum()),
            "inactive_done": int((ina & done).sum()), "done_t0": int((done & live)[0].sum()) if T else 0,
            "done_tlast": int((done & live)[T - 1].sum()) if T else 0,
            "inactive_columns": int(ina.all(axis=0).sum()) if T else 0,
            "reset_bits": int(((f & FLAG_RESET) != 0).sum()), "legal_bits": int(((f & 0x0F) != 0).sum()),
            "live": int(live.sum())}


def pot_regimes(case):
    p = case["pot"].astype(np.int64).reshape(-1, 4)
    srt = np.sort(p, axis=1)
    return {"min128": int((p == -128).sum()), "minus1": int((p == -1).sum()), "max127": int((p == 127).sum()),
            "negative": int((p < 0).sum()),
            "pairwise_different": bool((np.diff(srt, axis=1) != 0).all()) if len(p) else True}


RTG_SHAPES = [(1, 1), (15, 255), (16, 256), (17, 257), (33, 513), (16, 1), (1, 513), (33, 255), (17, 256)]
PREPARE_STEPS = (0.0, 1.0, 2.0, 1000.0)
PREPARE_BETAS = (0.0, 0.9, 1.0 - 1e-9, 1.0)


def prepare_table():
    """(state[0..3], beta) rows: every step x every beta, then one state with m2_c < mu_c^2."""
    rows = [([1.5 + 0.25 * i, 40.0 + j, 1.5, step], beta)
            for i, step in enumerate(PREPARE_STEPS) for j, beta in enumerate(PREPARE_BETAS)]
    rows.append(([3.0, 2.0, 3.0, 5.0], 0.5))   # m2 / bc < (mu / bc)^2: the variance clamp
    return rows


# ------------------------------------------------------------------------------ episode scan -----
def board_max(boards):
    """Per board, the UNSIGNED byte maximum (the kernel's bytemax)."""
    return np.asarray(boards, np.int8).view(np.uint8).max(axis=-1).astype(np.int64)


def episode_walk(points, boards, max_tile, flags, run_score, run_max):
    """episode_scan_kernel: scores int64 / tiles int32 [T, n] (-1 where no game ends) and the carried
    (run_score, run_max) after the T steps.  DONE|INACTIVE ends nothing but its points still count."""
    points = np.asarray(points, np.int64)
    T, n = points.shape
    bm = board_max(np.asarray(boards)[:T]) if T else np.zeros((0, n), np.int64)
    mt = np.asarray(max_tile, np.int8).astype(np.int64)
    flags = np.asarray(flags, np.uint8)
    rs, rm = np.array(run_score, np.int64), np.array(run_max, np.int64)
    scores, tiles = np.full((T, n), -1, np.int64), np.full((T, n), -1, np.int32)
    for t in range(T):
        rs = rs + points[t]
        rm = np.maximum(rm, np.maximum(bm[t], mt[t]))
        ends = ((flags[t] & FLAG_DONE) != 0) & ((flags[t] & FLAG_INACTIVE) == 0)
        scores[t] = np.where(ends, rs, -1)
        tiles[t] = np.where(ends, rm, -1)
        rs, rm = np.where(ends, 0, rs), np.where(ends, 0, rm)
    return scores, tiles, rs, rm.astype(np.int32)


# ------------------------------------------------------------------------------ rollout stats ----
STAT_NAMES = ("rows", "reward_mean", "reward_var", "reward_zero_pct", "adv_mean", "adv_var", "adv_l2", "adv_min",
              "adv_max", "gnorm_mean", "gnorm_std", "gnorm_min", "gnorm_max", "graw_std", "value_std", "g0",
              "score_mean", "score_median", "score_max", "tile9_pct", "tile10_pct", "tile11_pct", "finished")
MEAN_TYPE = {1: "r", 4: "a", 9: "gn"}
VAR_TYPE = {2: "r", 5: "a"}
STD_TYPE = {10: "gn", 13: "gr", 14: "v"}


def metric_reward_f32(points, pot, flags, cfg):
    """The metric's reward in float32, operation for operation as the kernel's __f*_rn chain."""
    gamma, wp, wm, we = (np.float32(x) for x in cfg)
    p = np.asarray(pot, np.int8).astype(np.float32)
    nd = np.where((np.asarray(flags) & FLAG_DONE) != 0, np.float32(0), np.float32(1))
    x1 = (gamma * p[..., 1]) * nd - p[..., 0]
    x2 = (gamma * p[..., 3]) * nd - p[..., 2]
    r = (np.asarray(points, np.int32).astype(np.float32) * wp + wm * x1) + we * x2
    assert r.dtype == np.float32
    return r


def _moments(x):
    n = len(x)
    mean = math.fsum(x) / n
    return mean, math.fsum((x - mean) ** 2) / n, math.fsum(x * x)


def rollout_stats(points, pot, flags, value, g_raw, g_norm, adv, boards, max_tile, episodic, cfg, run_score,
                  run_max):
    """The 23 entries of rollout_stats_final_kernel's o[23] in float64, plus what the tests scale their
    bounds with.  Returns (out [23], aux): aux holds keys (the finished scores), zero_rows, the carried
    run_score / run_max (fixed horizon), mean_abs / mean_sq per field."""
    points = np.asarray(points, np.int32)
    T, n = points.shape
    flags = np.asarray(flags, np.uint8)
    live = (flags & FLAG_INACTIVE) == 0
    rows = live if episodic else np.ones((T, n), bool)
    f = {"r": metric_reward_f32(points, pot, flags, cfg).astype(np.float64)[rows]}
    for k, a in (("a", adv), ("gn", g_norm), ("gr", g_raw), ("v", value)):
        f[k] = np.asarray(a, np.float32).astype(np.float64)[rows]
    nr = int(rows.sum())
    mom = {k: _moments(v) for k, v in f.items()}
    graw = np.asarray(g_raw, np.float32).astype(np.float64)
    starts = np.zeros((T, n), bool)
    if episodic:
        starts[0] = True
    else:
        starts[1:] = (flags[:-1] & FLAG_RESET) != 0
    g0 = math.fsum(graw[starts]) / max(int(starts.sum()), 1)
    aux = {}
    if episodic:
        keys = np.where(live, points.astype(np.int64), 0).sum(axis=0)
        tiles = board_max(np.asarray(boards)[T])
    else:
        sc, ti, rs, rm = episode_walk(points, boards, max_tile, flags, run_score, run_max)
        keys, tiles = sc[sc >= 0], ti[sc >= 0].astype(np.int64)
        aux.update(run_score=rs, run_max=rm)
    cnt = len(keys)
    cf = max(cnt, 1)
    srt = np.sort(keys)
    out = np.array([
        nr, mom["r"][0], mom["r"][1], int((f["r"] == 0).sum()) / nr * 100.0,
        mom["a"][0], mom["a"][1], math.sqrt(mom["a"][2]), f["a"].min(), f["a"].max(),
        mom["gn"][0], math.sqrt(mom["gn"][1]), f["gn"].min(), f["gn"].max(),
        math.sqrt(mom["gr"][1]), math.sqrt(mom["v"][1]), g0,
        math.fsum(keys) / cf, float(srt[(cnt - 1) // 2]) if cnt else -1.0, float(srt[-1]) if cnt else -1.0,
        int((tiles >= 9).sum()) / cf * 100.0, int((tiles >= 10).sum()) / cf * 100.0,
        int((tiles >= 11).sum()) / cf * 100.0, cnt], np.float64)
    aux.update(keys=keys, zero_rows=int((f["r"] == 0).sum()), starts=int(starts.sum()),
               mean_abs={k: math.fsum(np.abs(v)) / nr for k, v in f.items()},
               mean_sq={k: mom[k][2] / nr for k in f},
               g0_mean_abs=math.fsum(np.abs(graw[starts])) / max(int(starts.sum()), 1))
    return out, aux


STATS_T = (1, 7, 8, 9, 17)
STATS_N = (1, 64, 255, 257, 513)
STATS_SHAPES = [(1, 1), (7, 64), (8, 255), (9, 257), (17, 513), (17, 1), (1, 513), (8, 64)]
WRAP_SHAPE = (3, FINAL_STRIDE * KBLOCK + 3)   # more than 64 blocks: the final kernel's `b += 64` wraps


def stats_case(T, n, episodic, seed=0):
    """One rollout's inputs for episode_scan / rollout_stats.  Boards hold tiles up to 17; max_tile lies
    above, below and at the board maximum; DONE|INACTIVE steps carry points; RESET sits on step T-1 too.
    Episodic: every env's game ends at a random step and the rest of its column is inactive (with points
    that must not count); the FINAL boards' maxima are 8..12 while earlier boards hold higher tiles."""
    g = np.random.default_rng(977 * T + n + (1 << 20) * episodic + 31337 * seed)
    pts = np.where(g.random((T, n)) < 0.3, 0, g.integers(0, 2048, size=(T, n))).astype(np.int32)
    pot = (g.integers(-128, 128, size=(T, n, 4)) * (g.random((T, n, 1)) >= 0.3)).astype(np.int8)
    # rows whose reward is 0 only in the float32 chain: 0.99f * 100 rounds to 99.0f, minus 99 -> exactly 0
    # (in float64 it is 9.5e-7); they count as zero rewards where the step is not DONE
    pts[::5, ::7] = 0
    pot[::5, ::7] = (99, 100, 0, 0)
    boards = g.integers(0, 18, size=(T + 1, n, 16)).astype(np.int8)
    boards[g.random((T + 1, n, 16)) < 0.5] = 0
    # an env's boards are capped at 6..13 (so the >= 9 / 10 / 11 shares differ), one board in twenty is not
    cap = np.where(g.random((T + 1, n)) < 0.05, 17, 6 + np.arange(n) % 8)
    boards = np.minimum(boards, cap[:, :, None]).astype(np.int8)
    bm = board_max(boards[:T])
    mt = np.clip(bm + g.integers(-1, 2, size=(T, n)), 0, 17).astype(np.int8)
    if episodic:
        end = g.integers(1, T + 1, size=n)
        tt = np.arange(T)[:, None]
        fl = np.where(tt == end - 1, FLAG_DONE, 0) | np.where(tt >= end, FLAG_INACTIVE, 0)
        if T > 1 and n > 2:
            fl[:, 1] = FLAG_INACTIVE                       # a column that never played: score 0
            fl[0, 2], fl[1:, 2] = FLAG_DONE, FLAG_INACTIVE | FLAG_DONE
        boards[:T, :, 0] = np.maximum(boards[:T, :, 0], 13)   # earlier boards: higher tiles than any final one
        final = 8 + (np.arange(n) % 5)
        boards[T] = np.minimum(boards[T], final[:, None])
        boards[T, np.arange(n), g.integers(0, 16, size=n)] = final
    else:
        fl = np.where(g.random((T, n)) < 0.15, FLAG_DONE, 0) | np.where(g.random((T, n)) < 0.2, FLAG_RESET, 0)
        fl = fl | np.where(g.random((T, n)) < 0.08, FLAG_INACTIVE, 0)
        fl[T - 1, ::3] |= FLAG_RESET                      # starts nothing inside this rollout
        if n > 1:
            fl[0, 1] |= FLAG_RESET
    fl = (fl | g.integers(0, 16, size=(T, n))).astype(np.uint8)
    value, g_raw, g_norm, adv = ((g.standard_normal((T, n)) * s + o).astype(np.float32)
                                 for s, o in ((1.0, 0.3), (30.0, 12.0), (1.0, -0.2), (1.5, 0.1)))
    return {"points": pts, "pot": pot, "flags": fl, "value": value, "g_raw": g_raw, "g_norm": g_norm, "adv": adv,
            "boards": boards if episodic else boards[:T].copy(), "max_tile": mt, "T": T, "n": n,
            "episodic": bool(episodic)}


def stats_regimes(case):
    f, T = case["flags"], case["T"]
    ina, done = (f & FLAG_INACTIVE) != 0, (f & FLAG_DONE) != 0
    out = {"done_inactive_with_points": int((ina & done & (case["points"] > 0)).sum()),
           "inactive_with_points": int((ina & (case["points"] > 0)).sum()),
           "reset_last_step": int(((f[T - 1] & FLAG_RESET) != 0).sum()),
           "reset_before_last": int(((f[:T - 1] & FLAG_RESET) != 0).sum()),
           "tile17": int((case["boards"] == 17).sum())}
    cfg = (0.99, 0.1, 1.0, 0.5)
    p = case["pot"].astype(np.float64)
    nd = ((f & FLAG_DONE) == 0).astype(np.float64)
    g, wp, wm, we = (float(np.float32(x)) for x in cfg)
    r64 = case["points"] * wp + wm * (g * p[..., 1] * nd - p[..., 0]) + we * (g * p[..., 3] * nd - p[..., 2])
    out["zero_in_float32_only"] = int(((metric_reward_f32(case["points"], case["pot"], f, cfg) == 0) & (r64 != 0)).sum())
    if not case["episodic"]:
        bm = board_max(case["boards"][:T])
        mt = case["max_tile"].astype(np.int64)
        out.update(mt_above=int((mt > bm).sum()), mt_below=int((mt < bm).sum()), mt_equal=int((mt == bm).sum()))
    else:
        fin = board_max(case["boards"][T])
        out.update(final_maxima=sorted(set(fin.tolist())),
                   earlier_higher=int((board_max(case["boards"][:T]).max(axis=0) > fin).sum()))
    return out


def key_sets():
    """name -> the finished scores the radix select is fed (int64, each < 2^31), in injection order."""
    g = np.random.default_rng(5)
    big = g.integers(1 << 22, 1 << 31, size=300)
    big[:3] = [(1 << 31) - 1, 1 << 22, (1 << 30) + 12345]
    return {"none": np.zeros(0, np.int64),
            "one": np.array([777], np.int64),
            "two_different": np.array([90001, 17], np.int64),
            "all_zero": np.zeros(40, np.int64),
            "all_equal": np.full(41, 123457, np.int64),
            "three_digit_passes": big.astype(np.int64),
            "bit0_only": (0x2AAAAAA0 | g.integers(0, 2, size=101)).astype(np.int64),
            "top_bit_only": (0x00012345 | (g.integers(0, 2, size=100) << 30)).astype(np.int64),
            "many_duplicates": g.choice(np.array([3, 4096, 4097, 70000, 70001, 1 << 21]), size=2600).astype(np.int64)}


def key_case(keys, T=3):
    """Fixed-horizon inputs whose finished scores are exactly `keys`: env e finishes once, at step e % T,
    with score run_score[e] + the points up to there; envs beyond len(keys) (at least one) finish nothing."""
    keys = np.asarray(keys, np.int64)
    k = len(keys)
    n = k + 3
    c = stats_case(T, n, False, seed=k)
    fl = (c["flags"] & ~np.uint8(FLAG_DONE | FLAG_INACTIVE)).astype(np.uint8)
    pts = c["points"] % 64
    e = np.arange(k)
    fl[e % T, e] |= FLAG_DONE
    upto = np.where(np.arange(T)[:, None] <= (e % T)[None, :], pts[:, :k], 0).sum(axis=0)
    small = upto > keys                      # the points alone would exceed the key: none, all from the state
    pts[:, :k][:, small] = 0
    take = np.where(small, 0, upto)
    rs = np.zeros(n, np.int64)
    rs[:k] = keys - take
    rs[k:] = 5
    c.update(points=pts.astype(np.int32), flags=fl, run_score=rs, run_max=np.zeros(n, np.int32))
    return c


# ------------------------------------------------------------------------------ sampler ----------
def masked_sampler(logits, legal, u):
    """The fp64 masked softmax over legal & 0xF and the inverse-CDF draw.  Returns logp (-inf where
    illegal), entropy (over p > 0), cdf, action, and each row's distance from u to the nearest CDF
    boundary that decides between two actions (the last legal action's boundary, 1, decides nothing:
    rows with fewer than two legal moves get distance inf).  legal == 0: action 0, entropy 0, all -inf.
    logits None: zeros."""
    legal = np.asarray(legal, np.int64) & 0xF
    n = len(legal)
    bits = ((legal[:, None] >> np.arange(4)) & 1).astype(bool)
    lg = np.zeros((n, 4)) if logits is None else np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.where(bits, lg, -np.inf)          # NaN / inf in an illegal column never enters
        m = lg.max(axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.where(bits, np.exp(lg - m), 0.0)
        s = e.sum(axis=1, keepdims=True)
        p = e / np.where(s > 0, s, 1.0)
        logp = np.where(bits, (lg - m) - np.log(np.where(s > 0, s, 1.0)), -np.inf)
        ent = -np.where(p > 0, p * np.where(p > 0, logp, 0.0), 0.0).sum(axis=1)
    cdf = np.cumsum(p, axis=1)
    u = np.asarray(u, np.float64)
    hit = bits & (u[:, None] < cdf)
    last = np.where(bits.any(axis=1), 3 - np.argmax(bits[:, ::-1], axis=1), 0)
    action = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
    deciding = bits & (np.arange(4)[None, :] < last[:, None])
    dist = np.where(deciding, np.abs(cdf - u[:, None]), np.inf).min(axis=1)
    return {"logp": logp, "entropy": ent, "p": p, "cdf": cdf, "action": action.astype(np.int64), "dist": dist,
            "bits": bits}


NEAR_BOUNDARY = 4.0 * 2.0 ** -24     # four float32 roundings of the running sum
SAMPLER_SEED, SAMPLER_COUNTER, SAMPLER_ENV_BASE = 2048, 9, 3
LOGIT_PATTERNS = ("equal", "random", "gap30", "gap100", "gap1e4", "offset+1e4", "offset-1e4", "nan_illegal",
                  "posinf_illegal", "neginf_illegal")
SAMPLER_REPEATS = 6


def sampler_table():
    """All 16 legal masks x LOGIT_PATTERNS x SAMPLER_REPEATS rows: logits float32 [n, 4], legal uint8 [n]
    (low nibble only), pattern [n] (index into LOGIT_PATTERNS)."""
    g = np.random.default_rng(44)
    rows, legal, pat = [], [], []
    for mask in range(16):
        for pi, name in enumerate(LOGIT_PATTERNS):
            for rep in range(SAMPLER_REPEATS):
                x = g.uniform(-10.0, 10.0, size=4)
                if name == "equal":
                    x = np.full(4, float(g.integers(-5, 6)))
                elif name.startswith("gap"):
                    x = x * 0.05 + float(name[3:]) * g.permutation(4)
                elif name.startswith("offset"):
                    x = x + float(name[6:])
                elif name.endswith("_illegal"):
                    bad = {"nan": np.nan, "posinf": np.inf, "neginf": -np.inf}[name.split("_")[0]]
                    x = np.where([(mask >> a) & 1 for a in range(4)], x, bad)
                rows.append(x)
                legal.append(mask)
                pat.append(pi)
    return {"logits": np.array(rows, np.float32), "legal": np.array(legal, np.uint8), "pattern": np.array(pat)}


def uniforms(words):
    """The sampler's uniform from the first Philox word: the top 24 bits, exactly as the kernel's float."""
    return (np.asarray(words, np.uint32) >> 8).astype(np.float64) / 2.0 ** 24
