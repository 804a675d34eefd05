"""The PPO-clip / entropy / smooth-L1 loss of one trajectory row, its gradient with respect to the five
head outputs, the KL diagnostic and the nine training statistics, restated in plain numpy (no torch) --
the reference that tests/test_gpu_ppo_loss_edges.py holds every kernel that inlines csrc/ppo_common.hpp
(row_loss, kl_row, stats_block) to, branch by branch.

The reference follows g2048.ppo.ppo_losses and torch's backward conventions:
  * log_softmax is (x - max) - log(sum exp(x - max)) over the legal actions;
  * clamp passes the gradient AT its bounds (mask = lo <= x <= hi) and cuts it outside;
  * minimum(t1, t2) gives the gradient to the smaller side and splits a tie in halves -- the branch
    every in-range row takes, because there the clipped ratio IS the ratio and t1 == t2;
  * the clip bounds are the fp32 values the C ABI forms, 1.0f -+ clip_eps, not Python doubles;
  * illegal logits enter the ENTROPY's softmax at -20 (masked_fill(-inf) then clamp(-20, 20)), but add
    no term to the entropy sum and get no gradient;
  * smooth_l1 (beta 1) switches at |v - ret| = 1, where both formulas agree: its gradient is
    clamp(v - ret, -1, 1).
tests/test_ppo_loss_host.py proves it against float64 autograd of ppo_losses on the whole table.

With dtype=np.float32 every intermediate is rounded to fp32 (numpy's own expf / logf).  That emulation
is used for one thing only: to size the tolerances of the GPU tests (UNITS below)."""

from __future__ import annotations

import numpy as np

CLIP_EPS = 0.2
CLIP_LO = float(np.float32(1.0) - np.float32(CLIP_EPS))   # 0.800000011920929: 1.0f - clip_eps
CLIP_HI = float(np.float32(1.0) + np.float32(CLIP_EPS))   # 1.2000000476837158
STAT_KEYS = ("loss", "policy_loss", "entropy_loss", "value_loss", "grad_norm", "entropy", "kl_total", "kl_average",
             "kl_max")

# ---- margins of the branch table (asserted on the fp64 row values by the host test) ----------------
MARGIN_LOG_RATIO = 0.5     # distance of the log-ratio from +-20
MARGIN_RATIO = 0.05        # distance of the ratio from the clip bounds
MARGIN_LOGIT = 0.5         # distance of a legal logit from +-20
MARGIN_VALUE = 0.2         # distance of |v - ret| from 1, unless it is exactly 1

# ---- tolerance budget of the GPU tests --------------------------------------------------------------
# UNITS[q] = the largest |fp32 emulation - fp64| over the branch table, in units of 2^-23 of the
# quantity's scale (loss_scales), as tests/test_ppo_loss_host.py measures and prints it with numpy's
# libm (7.070 / 0.696 / 0.344 / 5.947 / 0.688 / 0.611), plus 5 % for another host libm, rounded up to two
# decimals.  The host test fails when a measurement exceeds its constant or falls more than that headroom
# below it, so the constants stay the measured counts.  The GPU tests allow DEVICE_FACTOR times these:
# the device's expf / logf are 1-2 ulp where numpy's are <= 1, inside a chain of about four such calls
# (log-sum-exp, exp of the log-ratio; log-sum-exp, exp of the entropy's log-probabilities).  Neither
# number is tuned against kernel output.
UNITS = {"ppo": 7.43, "ent": 0.74, "vl": 0.37, "dz": 6.25, "dv": 0.73, "kl": 0.65}
UNITS_HEADROOM = 0.05
DEVICE_FACTOR = 4.0
U23 = 2.0 ** -23


def bf16_round(x):
    """fp32 -> the nearest bf16 value (ties to even), returned as float64."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def is_bf16(x) -> bool:
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(bf16_round(x.astype(np.float32)), x))


def _legal_bits(legal):
    return ((np.asarray(legal, np.int64)[:, None] >> np.arange(4)) & 1).astype(bool)


def row_terms(z, act, legal, old_logp, adv, ret, beta, critic, clip_lo, clip_hi, inv_m, dtype=np.float64):
    """Everything row_loss_ref returns plus the intermediate values and branch indicators of each row
    (for the table audit): a dict of arrays over the m rows."""
    T = np.dtype(dtype).type
    z = np.asarray(z, dtype)
    m = z.shape[0]
    act = np.asarray(act, np.int64)
    lg = _legal_bits(legal)
    old = np.asarray(old_logp, np.float32).astype(dtype)
    A = np.asarray(adv, np.float32).astype(dtype)
    ret = np.asarray(ret, np.float32).astype(dtype)
    beta, critic, inv_m = T(beta), T(critic), T(inv_m)
    lo, hi = T(np.float32(clip_lo)), T(np.float32(clip_hi))
    rows = np.arange(m)
    c20 = T(20.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        # masked log_softmax over the legal actions
        mk = np.where(lg, z[:, :4], T(-np.inf))
        mx = mk.max(1, keepdims=True)
        e = np.where(lg, np.exp(mk - mx), T(0))
        lse_c = np.log(e.sum(1, keepdims=True, dtype=dtype))
        lp = np.where(lg, (mk - mx) - lse_c, T(-np.inf))
        sm = np.where(lg, np.exp(lp), T(0))
        # PPO-clip term
        dlt = lp[rows, act] - old[rows, act]
        in20 = (dlt >= -c20) & (dlt <= c20)
        ratio = np.exp(np.clip(dlt, -c20, c20))
        rc = np.clip(ratio, lo, hi)
        inr = (ratio >= lo) & (ratio <= hi)
        t1, t2 = A * ratio, A * rc
        ppo = np.minimum(t1, t2)
        half = T(0.5) * A
        dp = np.where(t1 < t2, A, np.where(t1 > t2, np.where(inr, A, T(0)), half + np.where(inr, half, T(0))))
        dd = np.where(in20, dp * ratio, T(0))           # d ppo / d log-ratio
        onehot = (np.arange(4)[None, :] == act[:, None]).astype(dtype)
        dppo = dd[:, None] * (onehot - sm)              # d ppo / d logits (legal ones)
        # entropy of softmax(clamp(masked, -20, 20)), summed over the legal actions
        ck = np.clip(mk, -c20, c20)
        cmx = ck.max(1, keepdims=True)
        lse2 = np.log(np.exp(ck - cmx).sum(1, keepdims=True, dtype=dtype))
        lp2 = (ck - cmx) - lse2
        p2 = np.exp(lp2)
        ent = -np.where(lg, p2 * lp2, T(0)).sum(1, dtype=dtype)
        w = np.where(lg, p2 * (lp2 + T(1)), T(0))
        S = w.sum(1, keepdims=True, dtype=dtype)
        cpass = lg & (mk >= -c20) & (mk <= c20)
        dent = np.where(cpass, -(w - p2 * S), T(0))     # d ent / d logits
        # smooth-L1 value loss
        dv0 = z[:, 4] - ret
        av = np.abs(dv0)
        vl = np.where(av < T(1), T(0.5) * dv0 * dv0, av - T(0.5))
        dvl = np.clip(dv0, T(-1), T(1))
        dz = np.zeros((m, 5), dtype)
        dz[:, :4] = np.where(lg, -inv_m * (dppo + beta * dent), T(0))
        dz[:, 4] = inv_m * critic * dvl
    return {"ppo": ppo, "ent": ent, "vl": vl, "dz": dz, "masked": mk, "logp": lp, "dlt": dlt, "ratio": ratio,
            "rc": rc, "in20": in20, "inr": inr, "side": np.sign(t1 - t2), "above": ratio > hi, "cpass": cpass,
            "hi_logit": lg & (mk > c20), "lo_logit": lg & (mk < -c20), "dv0": dv0, "quad": av < T(1), "legal": lg}


def row_loss_ref(z, act, legal, old_logp, adv, ret, beta, critic, clip_lo, clip_hi, inv_m, dtype=np.float64):
    """z [m,5] = 4 logits + value; act [m]; legal [m] bit masks; old_logp [m,4]; adv, ret [m].
    Returns ppo [m], ent [m], vl [m], dz [m,5] = d(-inv_m sum(ppo - critic vl + beta ent)) / dz, masked [m,4]."""
    t = row_terms(z, act, legal, old_logp, adv, ret, beta, critic, clip_lo, clip_hi, inv_m, dtype)
    return t["ppo"], t["ent"], t["vl"], t["dz"], t["masked"]


def loss_scales(t, adv, beta, critic, inv_m):
    """The scale of each quantity's rounding error (one unit = 2^-23 of it), from fp64 row terms:
    ppo |A| max(ratio, clipped ratio); ent absolute; vl relative; dz[0..3] (|A| ratio + beta) inv_m;
    dz[4] inv_m critic."""
    a = np.abs(np.asarray(adv, np.float64))
    return {"ppo": a * np.maximum(t["ratio"], t["rc"]), "ent": np.ones_like(a), "vl": np.abs(t["vl"]),
            "dz": (a * t["ratio"] + beta) * inv_m, "dv": np.full_like(a, inv_m * critic)}


def kl_row_ref(old_masked, new_logits, dtype=np.float64):
    """KL(old || new) over the actions legal in old (old illegal = -inf), ppo.kl_old_new."""
    T = np.dtype(dtype).type
    o = np.asarray(old_masked, np.float32).astype(dtype)
    ok = o != T(-np.inf)
    n = np.where(ok, np.asarray(new_logits, dtype), T(-np.inf))
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        def lsm(x):
            mx = x.max(1, keepdims=True)
            e = np.where(ok, np.exp(x - mx), T(0))
            return (x - mx) - np.log(e.sum(1, keepdims=True, dtype=dtype))
        lo, ln = lsm(o), lsm(n)
        return np.where(ok, np.exp(lo) * (lo - ln), T(0)).sum(1, dtype=dtype)


def kl_scale(old_masked, new_logits):
    """Rounding scale of one row's KL: 1 + the spread of the old and of the new legal logits (the
    log-probabilities' magnitude; KL = sum p (lo - ln) with sum p = 1)."""
    o = np.asarray(old_masked, np.float64)
    ok = np.isfinite(o)
    n = np.asarray(new_logits, np.float64)
    spread = lambda x: np.where(ok, x, -np.inf).max(1) - np.where(ok, x, np.inf).min(1)  # noqa: E731
    return 1.0 + spread(o) + spread(n)


def stats_ref(sums, kl_sum, kl_max, gn, beta, critic, m):
    """One minibatch's contribution to the nine statistics, STAT_KEYS order (kl_max: the value to max in)."""
    s_ppo, s_ent, s_v = (float(s) / m for s in sums)
    return np.array([-(s_ppo - critic * s_v + beta * s_ent), -s_ppo, -beta * s_ent, critic * s_v, gn, s_ent, kl_sum,
                     kl_sum / m, kl_max], np.float64)


# ---------------------------------------------------------------------------------------------------
# The branch table
# ---------------------------------------------------------------------------------------------------
# log-ratio targets, each strictly inside its regime at the margins above
#   ln(0.8 - 0.05) = -0.2877, ln(0.8 + 0.05) = -0.1625, ln(1.2 - 0.05) = 0.1398, ln(1.2 + 0.05) = 0.2231
LOG_RATIO_REGIMES = {
    "lr_below_m20": (-40.0, -23.0, -20.75),
    "lr_low": (-19.25, -3.0, -0.3),
    "lr_in": (-0.16, 0.0, 0.13),
    "lr_high": (0.23, 3.0, 19.25),
    "lr_above_p20": (20.75, 23.0, 40.0),
}
ADV_REGIMES = {"adv_pos": (0.5, 1.25, 2.0), "adv_neg": (-0.5, -1.25, -2.0), "adv_zero": (0.0, 0.0, 0.0)}
VALUE_GAPS = (-3.0, -1.0, -0.4, 0.0, 0.75, 1.0, 2.5)
BIG = 9984.0   # bf16(1e4)

# (name, legal mask, action, 4 logits); every logit bf16-representable
PLAIN_PATTERNS = [
    ("plain", 0b1111, 0, (0.5, -1.25, 2.0, -0.75)),
    ("plain", 0b1111, 2, (-0.375, 1.5, 0.25, 3.0)),
    ("plain", 0b0110, 1, (7.0, 0.75, -0.5, -7.0)),
    ("plain", 0b1011, 3, (1.0, -2.0, 5.0, 0.125)),
    ("plain", 0b1101, 2, (-1.5, 4.0, -0.25, 2.5)),
    ("plain", 0b0011, 0, (0.25, 1.75, -3.0, 6.0)),
]
LOGIT_PATTERNS = [
    ("logit_hi_taken", 0b1111, 0, (24.0, 1.0, -0.5, 0.25)),
    ("logit_hi_taken", 0b0110, 2, (0.5, 1.0, 26.0, -0.25)),
    ("logit_hi_taken", 0b1011, 3, (19.0, -2.0, 50.0, 21.0)),
    ("logit_hi_taken", 0b0010, 1, (0.5, 23.0, 1.0, -0.25)),
    ("logit_hi_other", 0b1111, 1, (24.0, 1.0, -0.5, 0.25)),
    ("logit_hi_other", 0b1101, 0, (2.0, 3.0, 0.5, 30.0)),
    ("logit_hi_other", 0b0110, 1, (-1.0, 18.0, 21.0, 0.5)),
    ("logit_hi_other", 0b1110, 3, (0.25, 27.0, 25.0, 19.0)),
    ("logit_lo_taken", 0b1111, 0, (-24.0, 1.0, -0.5, 0.25)),
    ("logit_lo_taken", 0b1010, 3, (2.0, 0.5, 1.0, -28.0)),
    ("logit_lo_taken", 0b0111, 1, (-19.0, -21.0, -18.0, 3.0)),
    ("logit_lo_taken", 0b0100, 2, (1.0, 0.5, -22.0, 2.0)),
    ("logit_lo_other", 0b1111, 1, (-24.0, 1.0, -0.5, 0.25)),
    ("logit_lo_other", 0b0111, 2, (0.75, -21.0, -1.0, 0.5)),
    ("logit_lo_other", 0b1100, 3, (5.0, 6.0, -23.0, -19.0)),
    ("logit_lo_other", 0b1011, 0, (-18.0, 0.5, 1.0, -26.0)),
    ("illegal_huge", 0b1011, 0, (0.5, -1.0, BIG, 1.5)),
    ("illegal_huge", 0b1110, 3, (BIG, 0.25, -0.75, 1.0)),
    ("illegal_huge", 0b0101, 2, (1.0, BIG, -0.5, BIG)),
    ("illegal_huge", 0b0010, 1, (BIG, 0.5, BIG, BIG)),
    ("legal_1", 0b0100, 2, (3.0, -1.0, 0.5, 2.0)),
    ("legal_1", 0b0001, 0, (2.0, 5.0, -4.0, 0.25)),
    ("legal_1", 0b1000, 3, (0.5, 0.25, 1.0, 25.0)),
    ("legal_1", 0b0010, 1, (1.0, -25.0, 2.0, 0.5)),
    ("legal_2", 0b1001, 3, (1.0, 8.0, -8.0, -0.5)),
    ("legal_2", 0b0110, 2, (4.0, -0.25, 0.75, 4.0)),
    ("legal_2", 0b0011, 1, (1.5, -0.5, 6.0, 6.0)),
    ("legal_2", 0b1100, 2, (-3.0, 2.0, 0.25, 1.75)),
    ("legal_3", 0b1110, 1, (9.0, 0.5, -1.0, 1.25)),
    ("legal_3", 0b0111, 0, (-0.5, 1.5, 0.25, -9.0)),
    ("legal_3", 0b1011, 3, (2.5, 7.0, -1.25, 0.5)),
    ("legal_3", 0b1101, 2, (0.75, -6.0, 1.0, -0.25)),
    ("taken_100_below", 0b1111, 1, (100.0, 0.0, 1.0, -1.0)),
    ("taken_100_below", 0b1111, 3, (2.0, 101.0, 0.5, 1.0)),
    ("taken_100_below", 0b0101, 0, (-88.0, 50.0, 12.0, 3.0)),
    ("taken_100_below", 0b1100, 2, (1.0, 1.0, -60.0, 40.0)),
    ("all_p1000", 0b1111, 0, (1000.0, 1004.0, 996.0, 1000.0)),
    ("all_p1000", 0b1111, 1, (1000.0, 1004.0, 996.0, 1000.0)),
    ("all_p1000", 0b1011, 3, (1004.0, 992.0, 1000.0, 1000.0)),
    ("all_p1000", 0b0110, 2, (996.0, 1000.0, 1004.0, 1008.0)),
    ("all_m1000", 0b1111, 2, (-1000.0, -1004.0, -996.0, -1000.0)),
    ("all_m1000", 0b1111, 3, (-1000.0, -1004.0, -996.0, -1000.0)),
    ("all_m1000", 0b1101, 0, (-1004.0, -992.0, -1000.0, -996.0)),
    ("all_m1000", 0b0011, 1, (-1000.0, -996.0, -1008.0, -992.0)),
]
# the stored action is illegal: log-ratio -inf, clamped to -20, zero gradient from the ppo term
ILLEGAL_ACTION_PATTERNS = [
    ("act_illegal", 0b1110, 0, (0.5, -1.25, 2.0, -0.75)),
    ("act_illegal", 0b0101, 1, (1.0, 3.0, 0.25, BIG)),
    ("act_illegal", 0b0011, 3, (-0.5, 0.75, 1.0, 2.0)),
    ("act_illegal", 0b1000, 2, (1.5, 0.5, -2.0, 0.25)),
]
VALUES = (0.5, -1.25, 3.0, 0.0)  # bf16-representable value-head outputs


def _logp64(z4, legal):
    lg = _legal_bits(np.array([legal]))[0]
    x = np.where(lg, np.asarray(z4, np.float64), -np.inf)
    return (x - x.max()) - np.log(np.exp(x - x.max()).sum())


def branch_table():
    """The named rows: a dict of arrays (z [n,5] float64, act, legal uint8, old_logp [n,4] float32, adv, ret
    float32) plus `tags` (a tuple of regime names per row) and `target` (the log-ratio aimed at).  Built
    without randomness; every row sits strictly inside one regime of each kind."""
    rows = []
    counter = [0]

    def add(pattern, lr_name, target, adv_name, adv, extra=()):
        name, legal, act, z4 = pattern
        i = counter[0]
        counter[0] += 1
        gap = VALUE_GAPS[i % len(VALUE_GAPS)]
        v = VALUES[i % len(VALUES)]
        lp = _logp64(z4, legal)
        old = np.full(4, -np.inf, np.float32)
        for k in range(4):  # the other legal entries differ from the taken one's (a wrong index shows)
            if legal >> k & 1:
                old[k] = np.float32(lp[k] + 0.125 * (k + 1))
        if legal >> act & 1:
            old[act] = np.float32(lp[act] - target)   # steers the log-ratio to `target`
        else:
            old[act] = np.float32(-1.5)               # finite: the log-ratio is -inf, not NaN
        rows.append({"z": np.array(list(z4) + [v], np.float64), "act": act, "legal": legal, "old_logp": old,
                     "adv": np.float32(adv), "ret": np.float32(np.float32(v) - np.float32(gap)), "target": target,
                     "tags": (name, lr_name, adv_name, "gap_%g" % gap, "legal_%d" % bin(legal).count("1")) + extra})

    # every log-ratio target x advantage sign on the plain patterns (>= 6 (legal, action) pairs each)
    for lr_name, targets in LOG_RATIO_REGIMES.items():
        for target in targets:
            for adv_name, advs in ADV_REGIMES.items():
                for j, pat in enumerate(PLAIN_PATTERNS):
                    add(pat, lr_name, target, adv_name, advs[j % 3])
    # every logit pattern x one target per log-ratio regime x advantage sign
    for pat in LOGIT_PATTERNS:
        for r, (lr_name, targets) in enumerate(LOG_RATIO_REGIMES.items()):
            for a, (adv_name, advs) in enumerate(ADV_REGIMES.items()):
                add(pat, lr_name, targets[(r + a) % 3], adv_name, advs[(r + 2 * a) % 3])
    for pat in ILLEGAL_ACTION_PATTERNS:
        for adv_name, advs in ADV_REGIMES.items():
            for j in range(2):
                add(pat, "lr_minus_inf", -np.inf, adv_name, advs[j])
    tab = {k: np.stack([r[k] for r in rows]) for k in ("z", "old_logp")}
    tab["act"] = np.array([r["act"] for r in rows], np.uint8)
    tab["legal"] = np.array([r["legal"] for r in rows], np.uint8)
    tab["adv"] = np.array([r["adv"] for r in rows], np.float32)
    tab["ret"] = np.array([r["ret"] for r in rows], np.float32)
    tab["target"] = np.array([r["target"] for r in rows], np.float64)
    tab["tags"] = [r["tags"] for r in rows]
    return tab


REQUIRED_REGIMES = (tuple(LOG_RATIO_REGIMES) + ("lr_minus_inf",) + tuple(ADV_REGIMES)
                    + tuple(sorted({p[0] for p in LOGIT_PATTERNS})) + ("act_illegal", "plain")
                    + tuple("gap_%g" % g for g in VALUE_GAPS) + ("legal_1", "legal_2", "legal_3", "legal_4"))


def table_terms(tab, beta, critic, inv_m, dtype=np.float64):
    return row_terms(tab["z"], tab["act"], tab["legal"], tab["old_logp"], tab["adv"], tab["ret"], beta, critic,
                     CLIP_LO, CLIP_HI, inv_m, dtype)


def branch_key(t):
    """The branch every row takes, as one integer array per decision (equal in fp64 and the fp32 emulation
    on every table row, or a tolerance would have to forgive a flip)."""
    return {"in20": t["in20"], "inr": t["inr"], "above": t["above"], "side": t["side"], "cpass": t["cpass"],
            "hi_logit": t["hi_logit"], "lo_logit": t["lo_logit"], "quad": t["quad"]}


def kl_table():
    """Rows of the KL diagnostic: old masked logits (fp32, -inf = illegal) and new logits (bf16-representable,
    so a one-hot head GEMM reproduces them exactly), with a name per row."""
    rows = [
        ("one_legal", (-np.inf, 0.7, -np.inf, -np.inf), (1.0, -3.0, 2.0, 0.5)),
        ("one_legal", (-np.inf, -np.inf, -np.inf, -4.25), (0.25, BIG, 2.0, 7.0)),
        ("old_60_below", (2.0, -58.0, 0.5, -np.inf), (1.0, 3.0, -2.0, 7.0)),
        ("old_60_below", (-61.5, -1.5, -np.inf, -0.3), (-0.5, 0.25, 1.0, 4.0)),
        ("new_p1000", (0.3, -1.1, 0.9, -np.inf), (1000.0, 1004.0, 996.0, 1000.0)),
        ("new_p1000", (-0.2, 1.4, -np.inf, 0.6), (996.0, 1000.0, 1008.0, 1004.0)),
        ("new_m1000", (0.3, -1.1, 0.9, 1.7), (-1000.0, -1004.0, -996.0, -1000.0)),
        ("new_m1000", (-np.inf, 1.4, 0.1, 0.6), (-996.0, -1000.0, -1008.0, -1004.0)),
        ("illegal_huge", (0.3, -np.inf, 0.9, -0.4), (1.0, BIG, -0.5, 0.25)),
        ("illegal_huge", (-np.inf, -np.inf, 0.9, -0.4), (BIG, BIG, 2.0, -1.0)),
        ("old_eq_new", (1.5, -0.75, 0.25, 3.0), (1.5, -0.75, 0.25, 3.0)),
        ("old_eq_new", (-np.inf, 2.0, -1.25, -np.inf), (0.0, 2.0, -1.25, 0.0)),
        ("generic", (0.1, -2.3, 1.7, 0.4), (0.5, -1.0, 1.25, -0.25)),
        ("generic", (-1.9, -np.inf, 0.2, 2.2), (2.0, 0.0, -3.0, 0.75)),
        ("generic", (3.3, 0.4, -np.inf, -np.inf), (-1.5, 1.5, 0.0, 0.0)),
    ]
    return {"name": [r[0] for r in rows], "old": np.array([r[1] for r in rows], np.float32),
            "new": np.array([r[2] for r in rows], np.float64)}
