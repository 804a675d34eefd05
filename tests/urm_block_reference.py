"""The training-path kernels between GameURM's projections (csrc/urm.hip: the attention core and its
head_dim-16 backward with the Philox dropout mask, the SwiGLU + depthwise conv and its backward with the
partial rows, the residual RMSNorm and its backward), restated in plain numpy (no torch) in float64 WITH the
kernels' rounding points -- the reference tests/test_gpu_urm_block_edges.py holds every stored output to,
element by element.

Every function returns, for each stored output, the unrounded float64 value `x` the kernel rounds (taken
after every intermediate rounding point) and two allowances, `arith` and `flip`:
  * arith -- the fp32 arithmetic between the rounding points: a sum of N terms gets (N + c) 2^-24 sum|term|,
    a hardware exp / rcp / rsqrt a relative budget (the UNITS below times DEVICE_FACTOR), one 2^-24 |x| for
    the last fp32 operation, and FLOOR for values the hardware may flush to zero;
  * flip  -- an intermediate bf16 rounding (P km, dS, silu(gate)) whose unrounded value lies within its own
    arithmetic error of a rounding boundary may land on either side: the candidates' distance, propagated to
    first order to every output the intermediate feeds.
The GPU test asserts bf16(x - a) <= output <= bf16(x + a) with a = arith + flip (check_bf16: the output is
a correctly rounded bf16 of some value in [x - a, x + a]; the interval ends pass through fp32 on their
way to bf16, which the 2^-24 |x| of `arith` covers), or |output - x| <= a + one fp32 step (check_f32).
tests/test_urm_block_host.py proves the reference against float64 autograd with the rounding points
switched off (rounding=False), measures the UNITS, and asserts that `flip` exceeds `arith` on at most
FLIP_SHARE of the outputs of every Gaussian case, so the tight bound stays the test."""

from __future__ import annotations

import numpy as np

from ppo_loss_reference import bf16_round

U24 = 2.0 ** -24
U23 = 2.0 ** -23
FLOOR = 2.0 ** -120      # subnormal P / sigmoid: whether exp, rcp and the MFMA flush them is not relied on
FLIP_SHARE = 0.05
# dQ and dK sum 16 dS roundings each.  With the worst-case sum bound above on dP = dO V^T and on rs (16 terms
# each, about 150 2^-24 of dS at N(0, 1.5^2)) and the P budget (about as much), 1.5-2 % of the dS roundings are
# ambiguous whatever DEVICE_FACTOR is (1.5 % at factor 1), so 12-24 % of the dQ / dK outputs carry a flip term:
# FLIP_SHARE cannot hold for them under a sound budget.  It is asserted on the dS roundings themselves, and
# the dQ / dK share is held to the union bound 16 x (the case's dS share) and to this cap.
FLIP_SHARE_DS_FANIN = 0.30

# ---- the hardware-intrinsic budgets -------------------------------------------------------------------
# UNITS[q] = the largest |fp32 numpy emulation - fp64| in units of 2^-23 of the quantity's scale, as
# tests/test_urm_block_host.py measures and prints it with numpy's libm (run with -s), plus UNITS_HEADROOM
# for another host libm, rounded up to two decimals.  The host test fails when a measurement exceeds its
# constant or falls more than the headroom below it.
#   P     softmax probability, scale P (2 + (|s - max| + max_j sum_d |q k| / sqrt(d)) / 2): the exp argument's
#         own rounding grows with |argument|, the dot products' with their absolute sum; the 2 is the exp, the
#         sum of 16, the division and the product at |argument| 0
#   sig   sigmoid, scale sig (1 + |x| (1 - sig))
#   rsqrt (mean s^2 + eps)^-1/2 of a 64-wide row, relative
# DEVICE_FACTOR is ASSUMED, not measured: v_exp_f32 / v_rcp_f32 / v_rsq_f32 are documented at about 1 ulp
# where numpy's expf / division / sqrt are <= 0.5-1, __expf adds the rounding of x log2(e), and the MFMA's
# accumulation order is not numpy's; no test in this repository pins the device intrinsics' error.  Neither
# number is tuned against kernel output.
UNITS = {"P": 1.28, "sig": 1.16, "rsqrt": 1.10}   # measured 1.214 / 1.103 / 1.043
UNITS_HEADROOM = 0.05
DEVICE_FACTOR = 4.0


def budget(q: str) -> float:
    return DEVICE_FACTOR * UNITS[q] * U23


def bf16_ulp(x):
    """One bf16 step at |x| (2^-133 below the normal range)."""
    ax = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return 2.0 ** (np.clip(np.where(ax > 0, e, -126.0), -126.0, 127.0) - 7.0)


def _bf(x):
    with np.errstate(over="ignore"):
        return bf16_round(np.asarray(x, np.float64).astype(np.float32))


def round_point(x, err, rounding=True):
    """An intermediate bf16 rounding of x known to +-err: the nominal rounded value and how far the
    other candidates lie from it (0 where the whole interval rounds to one value)."""
    if not rounding:
        return x, np.zeros_like(x)
    r, lo, hi = _bf(x), _bf(x - err), _bf(x + err)
    return r, np.maximum(hi - r, r - lo)


def check_bf16(got, x, allow):
    """Element mask: got (bf16 values as float64) is a correctly rounded bf16 of a value in x +- allow."""
    got = np.asarray(got, np.float64)
    return (_bf(x - allow) <= got) & (got <= _bf(x + allow))


def check_f32(got, x, allow):
    got = np.asarray(got, np.float64)
    with np.errstate(over="ignore"):
        step = np.abs(np.spacing(np.asarray(x, np.float64).astype(np.float32))).astype(np.float64)
    return np.abs(got - x) <= allow + step


# ---------------------------------------------------------------------------------------------------
# Attention dropout mask
# ---------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Vectorised Philox4x32-10: ctr [..., 4], key [..., 2] (broadcast), uint32 words -> [..., 4]."""
    ctr = np.asarray(ctr, np.uint64)
    key = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def drop_args(p):
    """(thr, scale) as attn_drop_args forms them in fp32: thr = lrintf(p 65536), scale = 1.0f / (1.0f - p).
    thr == 0 (p < 2^-17) means no mask and no scale."""
    p32 = np.float32(p)
    thr = int(np.rint(np.float64(p32) * 65536.0))   # p 2^16 is exact in fp32; rint = lrintf's ties-to-even
    with np.errstate(divide="ignore"):
        scale = float(np.float32(1.0) / (np.float32(1.0) - p32))
    return thr, scale


def keep_mask(n, heads, p, seed, counter, offset=0):
    """Keep multipliers [n, heads, 16 queries, 16 keys] (0 or scale; all 1 when thr == 0): one draw per
    (board, head, query, key group of 4), counter {board, head << 8 | query << 2 | group, lo32(c), hi32(c)}
    with c = counter + offset (mod 2^64), key = the seed's two words, words x and y = four 16-bit uniforms."""
    thr, scale = drop_args(p)
    if thr == 0:
        return np.ones((n, heads, 16, 16))
    c = (int(counter) + int(offset)) & (2 ** 64 - 1)
    b, hh, i, g = np.meshgrid(np.arange(n), np.arange(heads), np.arange(16), np.arange(4), indexing="ij")
    ctr = np.stack([b & 0xFFFFFFFF, (hh << 8) | (i << 2) | g, np.full_like(b, c & 0xFFFFFFFF), np.full_like(b, c >> 32)],
                   -1)
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]))
    x, y = r[..., 0].astype(np.int64), r[..., 1].astype(np.int64)
    u = np.stack([x & 0xFFFF, x >> 16, y & 0xFFFF, y >> 16], -1).reshape(n, heads, 16, 16)
    return np.where(u >= thr, scale, 0.0)


# ---------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------
def split_heads(qkv, heads):
    """[16 n, 3 h] -> q, k, v [n, heads, 16, head_dim]."""
    qkv = np.asarray(qkv, np.float64)
    n, h = qkv.shape[0] // 16, qkv.shape[1] // 3
    x = qkv.reshape(n, 16, 3, heads, h // heads).transpose(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def merge_heads(x):
    """[n, heads, 16, d] -> [16 n, heads d]."""
    n, heads, _, d = x.shape
    return x.transpose(0, 2, 1, 3).reshape(16 * n, heads * d)


def attn_probs(q, k, rounding=True, dtype=np.float64):
    """P = softmax over the 16 keys of q k^T / sqrt(head_dim) and its error budget errP.  With
    dtype=np.float32 every step is rounded to fp32 (sequential dot products, numpy's expf): the emulation
    that sizes UNITS["P"], nothing else."""
    hd = q.shape[-1]
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd))) if rounding else hd ** -0.5
    if dtype == np.float32:
        q32, k32 = q.astype(np.float32), k.astype(np.float32)
        s = np.zeros(q.shape[:-1] + (16,), np.float32)
        for d in range(hd):
            s = s + q32[..., :, None, d] * k32[..., None, :, d]
        s = s * np.float32(scale)
        with np.errstate(under="ignore"):
            e = np.exp(s - s.max(-1, keepdims=True))
            return e * (np.float32(1.0) / e.sum(-1, keepdims=True, dtype=np.float32)), None
    kt = np.swapaxes(k, -1, -2)
    a = (q @ kt) * scale
    a = a - a.max(-1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(a)
        P = e / e.sum(-1, keepdims=True)
        w = 2.0 + 0.5 * (np.abs(a) + scale * (np.abs(q) @ np.abs(kt)).max(-1, keepdims=True))
        return P, P * (budget("P") * w) + FLOOR


def attn_fwd(q, k, v, km=None, rounding=True):
    """One (board, head): q, k, v [..., 16, head_dim] bf16 values, km [..., 16, 16] keep multipliers or None.
    O = bf16(P km) V, stored as bf16."""
    P, errP = attn_probs(q, k, rounding)
    x = P if km is None else P * km
    e = errP if km is None else errP * km + U24 * np.abs(x)
    Pd, dev = round_point(x, e, rounding)
    av = np.abs(v)
    with np.errstate(under="ignore"):
        return {"P": P, "errP": errP, "Pd": Pd, "devPd": dev, "O": Pd @ v,
                "O_arith": 18 * U24 * (np.abs(Pd) @ av) + U24 * np.abs(Pd @ v) + FLOOR, "O_flip": dev @ av}


def attn_bwd(q, k, v, dO, km=None, rounding=True):
    """head_dim 16: dQ, dK, dV [..., 16, 16] of sum(O dO), stored as bf16.  P enters rs and dS unrounded;
    dS and Pd = P km enter their products as bf16."""
    f = attn_fwd(q, k, v, km, rounding)
    P, errP, Pd, devPd = f["P"], f["errP"], f["Pd"], f["devPd"]
    one = np.ones_like(P) if km is None else km
    T = lambda x: np.swapaxes(x, -1, -2)  # noqa: E731
    with np.errstate(under="ignore"):
        dP = dO @ T(v)
        e_dP = 18 * U24 * (np.abs(dO) @ np.abs(T(v)))
        t = P * one * dP
        rs = t.sum(-1, keepdims=True)
        e_rs = (one * (errP * np.abs(dP) + P * e_dP)).sum(-1, keepdims=True) + 20 * U24 * np.abs(t).sum(-1, keepdims=True)
        u = one * dP - rs
        xs = P * u
        e_dS = errP * np.abs(u) + P * (one * e_dP + e_rs + U24 * (np.abs(one * dP) + np.abs(u))) + U24 * np.abs(xs)
        dS, devS = round_point(xs, e_dS + (FLOOR if rounding else 0.0), rounding)
        sc = 0.25 if rounding else q.shape[-1] ** -0.5
        out = {"P": P, "Pd": Pd, "dS": dS, "devS": devS, "rs": rs}
        for name, a, b, da in (("dQ", dS, k, devS), ("dK", T(dS), q, T(devS)), ("dV", T(Pd), dO, T(devPd))):
            s = 1.0 if name == "dV" else sc
            x = s * (a @ b)
            out[name] = x
            out[name + "_arith"] = 18 * U24 * s * (np.abs(a) @ np.abs(b)) + U24 * np.abs(x) + FLOOR
            out[name + "_flip"] = s * (da @ np.abs(b))
    return out


# ---------------------------------------------------------------------------------------------------
# SwiGLU + depthwise conv (kernel 2)
# ---------------------------------------------------------------------------------------------------
def sigm(x, dtype=np.float64):
    """sigmoid = rcp(1 + exp(-x)) and its relative error budget (the scale of UNITS["sig"])."""
    if dtype == np.float32:
        x = np.asarray(x, np.float32)
        with np.errstate(over="ignore", under="ignore"):
            return np.float32(1.0) / (np.float32(1.0) + np.exp(-x)), None
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sg = 1.0 / (1.0 + np.exp(-x))
        return sg, budget("sig") * (1.0 + np.where(sg < 1.0, np.abs(x) * (1.0 - sg), 0.0))


def dsilu(x):
    """silu'(x) = sg (1 + x (1 - sg)) and the absolute error of its fp32 evaluation."""
    sg, rel = sigm(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xt = np.where((sg < 1.0) & (sg > 0.0), x * (1.0 - sg), 0.0)
        d = sg * (1.0 + xt)
        err = sg * (rel * (1.0 + 2.0 * np.abs(xt) + np.where(sg < 1.0, np.abs(x) * sg, 0.0))
                    + 4 * U24 * (1.0 + np.abs(xt))) + FLOOR
    return d, err


SILU_LIP = 1.1     # sup |silu'| = 1.0998
DSILU_SPAN = 1.2   # silu' ranges over [-0.0998, 1.0998]


def silu_change(x, d1, a):
    """|silu(x + e) - silu(x)| for |e| <= a: second order about x (|silu''| <= 1/2), never more than silu's
    Lipschitz constant allows -- which keeps the bound a few fp32 steps where x is huge."""
    return np.minimum(np.abs(d1) * a + 0.25 * a * a, SILU_LIP * a)


def dsilu_change(x, a):
    """|silu'(x + e) - silu'(x)| for |e| <= a: a sup |silu''| over the interval, with |silu''(t)| =
    s (1 - s) |2 + t (1 - 2 s)| <= min(1/2, (2 + |t|) e^-|t|), decreasing in |t|, taken at the interval's
    point nearest 0; never more than the span of silu'."""
    m = np.maximum(np.abs(x) - a, 0.0)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        curv = np.minimum(0.5, (2.0 + m) * np.exp(-m))
        return np.minimum(np.where(a > 0, a * curv, 0.0), DSILU_SPAN)


def swiglu_conv(g, u, w, b, dact=None, rounding=True):
    """g, u [nb, 16, inter] bf16 values (gate, up), w [inter, 2], b [inter] fp32 values, dact [nb, 16, inter].
    Forward: y = bf16(bf16(silu g) u), y2 = y_{t-1} w0 + y_t w1 + b (y_{-1} = 0 per board), act = bf16(silu y2).
    Backward: d2 = dact silu'(y2), dy_t = d2_t w1 + d2_{t+1} w0 (no t + 1 term at token 15),
    dgate = bf16(dy u silu'(g)), dup = bf16(dy bf16(silu g)); per board and channel the terms of
    dw0 = sum d2 y_{t-1}, dw1 = sum d2 y, db = sum d2 (summed over boards by partial_rows)."""
    w0, w1 = w[:, 0], w[:, 1]
    sg, relg = sigm(g)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xs = g * sg
        e_sl = np.abs(xs) * (relg + U24) + FLOOR
        if rounding:
            sl, lo, hi = _bf(xs), _bf(xs - e_sl), _bf(xs + e_sl)
            y = _bf(sl * u)
            dev_sl = np.maximum(hi - sl, sl - lo)
            dev_y = np.maximum(np.abs(_bf(hi * u) - y), np.abs(_bf(lo * u) - y))
        else:
            sl, y, dev_sl, dev_y = xs, xs * u, np.zeros_like(xs), np.zeros_like(xs)
        yp = np.concatenate([np.zeros_like(y[:, :1]), y[:, :-1]], 1)
        dev_yp = np.concatenate([np.zeros_like(y[:, :1]), dev_y[:, :-1]], 1)
        y2 = yp * w0 + y * w1 + b
        F2 = np.abs(w0) * dev_yp + np.abs(w1) * dev_y
        A2 = 4 * U24 * (np.abs(yp * w0) + np.abs(y * w1) + np.abs(b))
        s2, rel2 = sigm(y2)
        d1, e_d1 = dsilu(y2)
        act = y2 * s2
        A_act = silu_change(y2, d1, A2)
        T_act = silu_change(y2, d1, A2 + F2)
        out = {"sl": sl, "dev_sl": dev_sl, "y": y, "dev_y": dev_y, "y2": y2, "act": act,
               "act_flip": T_act - A_act,
               "act_arith": A_act + np.abs(act) * (rel2 + 2 * U24) + FLOOR,
               "act_scale": np.abs(yp * w0) + np.abs(y * w1) + np.abs(b)}
        if dact is None:
            return out
        d2 = dact * d1
        ad = np.abs(dact)
        A_d1 = dsilu_change(y2, A2)
        F_d2, A_d2 = ad * (dsilu_change(y2, A2 + F2) - A_d1), ad * (A_d1 + e_d1) + U24 * np.abs(d2)
        nx = lambda x: np.concatenate([x[:, 1:], np.zeros_like(x[:, :1])], 1)  # noqa: E731
        dy = d2 * w1 + nx(d2) * w0
        F_dy = np.abs(w1) * F_d2 + np.abs(w0) * nx(F_d2)
        A_dy = np.abs(w1) * A_d2 + np.abs(w0) * nx(A_d2) + 3 * U24 * (np.abs(d2 * w1) + np.abs(nx(d2) * w0))
        dg1, e_dg1 = dsilu(g)
        # the magnitude of each output's own terms before any cancellation (silu' = sg + x sg (1 - sg) cancels
        # near -1.2785): what the allowances are small against (tests/test_urm_block_host.py)
        dmag = lambda x, s: s * (1.0 + np.where(s < 1.0, np.abs(x) * (1.0 - s), 0.0))  # noqa: E731
        d2mag = ad * dmag(y2, s2)
        dy_scale = np.abs(w1) * d2mag + np.abs(w0) * nx(d2mag)
        out["dgate"] = dy * u * dg1
        out["dgate_scale"], out["dup_scale"] = dy_scale * np.abs(u) * dmag(g, sg), dy_scale * np.abs(sl)
        out["dgate_flip"] = F_dy * np.abs(u * dg1)
        out["dgate_arith"] = A_dy * np.abs(u * dg1) + np.abs(dy * u) * e_dg1 + 3 * U24 * np.abs(out["dgate"]) + FLOOR
        out["dup"] = dy * sl
        out["dup_flip"] = F_dy * np.abs(sl) + np.abs(dy) * dev_sl
        out["dup_arith"] = A_dy * np.abs(sl) + 2 * U24 * np.abs(out["dup"]) + FLOOR
        # the terms of the three parameter gradients: [nb, 16, inter] each with value and allowance
        out["terms"], out["term_scale"] = {}, {}
        for name, other, dev_o in (("s0", yp, dev_yp), ("s1", y, dev_y), ("sb", np.ones_like(y), np.zeros_like(y))):
            out["terms"][name] = (d2 * other, (F_d2 + A_d2) * np.abs(other) + np.abs(d2) * dev_o)
            out["term_scale"][name] = (d2mag * np.abs(other), np.zeros_like(y))
        out["d2"] = d2
    return out


def partial_rows(terms, nrows):
    """The partial sums as the backward kernels assign boards to rows: row r sums boards r, r + nrows, ...
    (16 tokens each, in order).  terms: swiglu_conv()["terms"].  Returns value and allowance [nrows, 3, inter]
    in the kernels' column order (s0, s1, sb)."""
    val, allow = [], []
    for name in ("s0", "s1", "sb"):
        x, e = terms[name]
        nb, _, inter = x.shape
        pad = (-nb) % nrows
        z = np.zeros((pad, 16, inter))
        xr = np.concatenate([x, z]).reshape(-1, nrows, 16, inter)
        er = np.concatenate([e, z]).reshape(-1, nrows, 16, inter)
        cnt = 16 * xr.shape[0]
        val.append(xr.sum((0, 2)))
        allow.append(er.sum((0, 2)) + (cnt + 2) * U24 * np.abs(xr).sum((0, 2)) + FLOOR)
    return np.stack(val, 1), np.stack(allow, 1)


def sc_rows(nb):
    """Partial rows of nb boards (sc_blocks)."""
    return min(int(nb), 2048)


def colsum(part):
    """dw [inter, 2], db [inter] from partial rows [nblk, 3, inter] (as read back, float64 of fp32): the
    fp64 sums and the bound of an fp32 sum of nblk terms in any order."""
    nblk = part.shape[0]
    s = part.sum(0)
    allow = (nblk + 2) * U24 * np.abs(part).sum(0) + FLOOR
    return np.stack([s[0], s[1]], -1), s[2], np.stack([allow[0], allow[1]], -1), allow[2]


# ---------------------------------------------------------------------------------------------------
# Residual RMSNorm
# ---------------------------------------------------------------------------------------------------
def rms_res_fwd(h, a, eps, dtype=np.float64):
    """h fp32 values, a bf16 or fp32 values [rows, 64]: s = h + a, r = (mean s^2 + eps)^-1/2, out = s r.
    Returns out, r and their allowances (outb = bf16(out) is checked bitwise against the device's out).
    dtype=np.float32: the emulation that sizes UNITS["rsqrt"]."""
    if dtype == np.float32:
        s = h.astype(np.float32) + a.astype(np.float32)
        with np.errstate(under="ignore"):
            ms = (s * s).sum(-1, keepdims=True, dtype=np.float32) * np.float32(1.0 / 64.0)
            r = np.float32(1.0) / np.sqrt(ms + np.float32(eps))
        return s * r, r[:, 0]
    s = h + a
    eps = float(np.float32(eps))
    with np.errstate(under="ignore"):
        ms = (s * s).mean(-1, keepdims=True)
        r = (ms + eps) ** -0.5
        out = s * r
        # s carries one rounding (2^-24 |s|, so 2 2^-24 in s^2), the 64-term sum (64 + 2) 2^-24: half of
        # that reaches r, plus the rsqrt's own budget
        rel_r = 0.5 * (64 + 2 + 2 + 1) * U24 + budget("rsqrt")
        return {"out": out, "out_allow": np.abs(out) * (rel_r + 2 * U24) + FLOOR, "r": r[:, 0],
                "r_allow": r[:, 0] * rel_r}


def rms_res_bwd(out, r, dout=None, dpool=None, doutb=None):
    """out, r: the forward's stored fp32 values.  g = dout | dpool[row >> 4], + float(doutb) when given;
    ds = r (g - out mean(g out)); dh = ds (fp32), da = bf16(ds) or fp32."""
    rows = out.shape[0]
    g = np.zeros_like(out) if dout is None else dout.copy()
    if dpool is not None:
        g = dpool[np.arange(rows) >> 4].copy()
    e_g = np.zeros_like(g)
    if doutb is not None:
        g = g + doutb
        e_g = U24 * np.abs(g)
    r = r[:, None]
    with np.errstate(under="ignore"):
        go = g * out
        mg = go.mean(-1, keepdims=True)
        e_mg = ((64 + 3) * U24 * np.abs(go).sum(-1, keepdims=True) + (e_g * np.abs(out)).sum(-1, keepdims=True)) / 64.0
        ds = r * (g - out * mg)
        allow = r * (e_g + np.abs(out) * e_mg + 2 * U24 * (np.abs(g) + np.abs(out * mg))) + 2 * U24 * np.abs(ds) + FLOOR
    return ds, allow


def flip_count(flip, arith):
    """How many outputs have a flip term larger than their arithmetic term.  A flip term of the floor's own
    order (an intermediate that is exactly 0, known to +-FLOOR) is the floor, not a rounding that can land
    either way, and does not count."""
    flip = np.asarray(flip)
    return int(((flip > np.asarray(arith)) & (flip > 1024 * FLOOR)).sum())


def flip_share(flip, arith):
    """The share of outputs whose flip term exceeds their arithmetic term."""
    return flip_count(flip, arith) / np.asarray(flip).size


# ---------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_urm_block_edges.py (built here so the host test can audit them)
# ---------------------------------------------------------------------------------------------------
ATTN_KINDS = ("gauss", "q0", "onehot", "twomax", "vcancel")
DOUT_KINDS = ("gauss", "onehot", "zero")


def _bfv(x):
    return _bf(np.asarray(x, np.float64))


def attn_case(kind, n, h, heads, seed=0, dout_kind="gauss"):
    """qkv [16 n, 3 h], dout [16 n, h] as float64 arrays of bf16 values.
      gauss    N(0, 1.5^2)
      q0       q = 0: every P is exactly 1/16
      onehot   scores of +-200 (or +200 against 0 at head_dim >= 16, a different key per query): P is exactly
               one-hot, the other exponentials underflow to 0 in fp32
      twomax   the same with two equal maxima: P is exactly 1/2, 1/2
      vcancel  gauss / 4 scores, v = +-64 alternating over the keys plus N(0, 1): O cancels to a few units"""
    g = np.random.default_rng([seed, n, h, heads, ATTN_KINDS.index(kind)])
    hd = h // heads
    q, k, v = (_bfv(g.normal(size=(n, heads, 16, hd)) * 1.5) for _ in range(3))
    if kind == "q0":
        q = np.zeros_like(q)
    elif kind in ("onehot", "twomax"):
        A, B = 32.0, float(_bfv(6.25 * np.sqrt(hd)))
        q, k = np.zeros_like(q), np.zeros_like(k)
        for b in range(n):
            for hh in range(heads):
                sh = (3 * b + 5 * hh + 1) % 16
                if hd >= 16:   # query i meets key i - sh (and i - sh - 8) with +200, every other key with 0
                    q[b, hh, np.arange(16), np.arange(16)] = A
                    k[b, hh, np.arange(16), (np.arange(16) + sh) % 16] = B
                    if kind == "twomax":
                        k[b, hh, np.arange(16), (np.arange(16) + sh + 8) % 16] = B
                else:          # every query meets key sh (and sh + 8) with +200, every other key with -200
                    q[b, hh, :, 0] = A
                    k[b, hh, :, 0] = -B
                    k[b, hh, sh, 0] = B
                    if kind == "twomax":
                        k[b, hh, (sh + 8) % 16, 0] = B
    elif kind == "vcancel":
        q, k = _bfv(q / 4), _bfv(k / 4)
        v = _bfv(64.0 * (1 - 2 * (np.arange(16) % 2))[None, None, :, None] + g.normal(size=v.shape))
    qkv = np.concatenate([merge_heads(x) for x in (q, k, v)], 1)
    if dout_kind == "gauss":
        dout = _bfv(g.normal(size=(16 * n, h)))
    elif dout_kind == "onehot":
        dout = np.zeros((n, heads, 16, hd))
        dout[:, :, np.arange(16), np.arange(16) % hd] = 16.0
        dout = merge_heads(dout)
    else:
        dout = np.zeros((16 * n, h))
    return qkv, dout


def mask_probe(n, h, heads, part=0):
    """q = k = 0 and V[j][d] = 16 (j == part head_dim + d): O[i][d] = bf16(scale / 16) 16 keep[i][part head_dim
    + d], which reads the device mask back exactly (head_dim >= 16 needs one part, head_dim 4 four)."""
    hd = h // heads
    v = np.zeros((n, heads, 16, hd))
    d = np.arange(hd)
    ok = part * hd + d < 16
    v[:, :, (part * hd + d)[ok], d[ok]] = 16.0
    z = np.zeros((16 * n, h))
    return np.concatenate([z, z, merge_heads(v)], 1)


# silu'(x) = 0 at x = -1.2784645...; the bf16 value next to it
SILU_FLAT = float(_bfv(-1.2785))
GATE_EDGES = (0.0, -0.0, SILU_FLAT, 20.0, -20.0, 88.5, -88.5, 100.0, -100.0, float(_bfv(3e38)), -float(_bfv(3e38)))  # 88.5 = bf16(88.7)


def swiglu_case(kind, nb, inter, seed=0):
    """gu [16 nb, 2 inter] (bf16 values), w [inter, 2], b [inter] (fp32 values), dact [16 nb, inter] (bf16).
      gauss     N(0, 1.5^2) gate and up, w N(0, 0.5^2), b N(0, 0.1^2)
      edges     the gate takes GATE_EDGES in turn over (board, token, channel), |up| <= 1/2, |w| <= 1/4 and a
                small dact keep y, y2 and every sum finite
      w0zero / w1zero   gauss with that tap 0
      leak      token 15 of every board has y = 2^100 (gate 2^100, up 1) and w0 = 1: a read of the previous
                board's last token by token 0 is enormous; dact is 0 at token 15 so the sums stay finite
      flat      b and w chosen so that y2 is exactly SILU_FLAT on token 0 (w1 = 0, b = SILU_FLAT)"""
    g = np.random.default_rng([seed, nb, inter, sum(map(ord, kind))])
    gate = _bfv(g.normal(size=(nb, 16, inter)) * 1.5)
    up = _bfv(g.normal(size=(nb, 16, inter)) * 1.5)
    w = g.normal(size=(inter, 2)).astype(np.float32).astype(np.float64) * 0.5
    b = (g.normal(size=inter) * 0.1).astype(np.float32).astype(np.float64)
    dact = _bfv(g.normal(size=(nb, 16, inter)))
    if kind == "edges":
        idx = (np.arange(nb)[:, None, None] * 7 + np.arange(16)[None, :, None] * 3 + np.arange(inter)[None, None, :])
        gate = np.asarray(GATE_EDGES)[idx % len(GATE_EDGES)]
        gate = np.where((idx // len(GATE_EDGES)) % 3 == 2, _bfv(g.normal(size=gate.shape) * 1.5), gate)
        up = _bfv(np.clip(up, -2, 2) / 4)
        w = np.clip(w, -0.25, 0.25)
        dact = _bfv(dact * 2.0 ** -12)
    elif kind == "w0zero":
        w[:, 0] = 0.0
    elif kind == "w1zero":
        w[:, 1] = 0.0
    elif kind == "leak":
        gate[:, 15], up[:, 15] = 2.0 ** 100, 1.0
        w[:, 0] = 1.0
        dact[:, 15] = 0.0
    elif kind == "flat":
        w[:, 1] = 0.0
        b[:] = SILU_FLAT
    elif kind != "gauss":
        raise ValueError(kind)
    gu = np.concatenate([gate, up], -1).reshape(16 * nb, 2 * inter)
    return gu, w, b, dact.reshape(16 * nb, inter)


def split_gu(gu, inter):
    x = np.asarray(gu, np.float64).reshape(-1, 16, 2 * inter)
    return x[..., :inter], x[..., inter:]


RMS_EPS = 1e-6


def rms_case(rows, a_bf16, seed=0):
    """h fp32, a bf16 or fp32 values [rows, 64]; row r takes class r % 4 where rows allow: 0 Gaussian (h 2 sigma),
    1 all zero, 2 entries of magnitude 1e-20 (eps decides r), 3 entries of magnitude 1e18.  Rows past
    4096 x 16 (the grid-stride wrap) follow the same cycle."""
    g = np.random.default_rng([seed, rows, int(a_bf16)])
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
    h = f32(g.normal(size=(rows, 64)) * 2)
    a = g.normal(size=(rows, 64))
    cls = np.arange(rows) % 4 if rows > 1 else np.zeros(1, np.int64)
    for c, mag in ((1, 0.0), (2, 1e-20), (3, 1e18)):   # |h + a| <= 1.5e18: the fp32 sum of 64 squares stays finite
        h[cls == c] = f32(g.uniform(-1, 1, size=(int((cls == c).sum()), 64)) * mag)
        a[cls == c] = g.uniform(-0.5, 0.5, size=(int((cls == c).sum()), 64)) * mag
    a = _bfv(a) if a_bf16 else f32(a)
    return h, a, cls


# ---------------------------------------------------------------------------------------------------
# The Gaussian runs of the GPU file, listed once: tests/test_gpu_urm_block_edges.py runs exactly these and
# tests/test_urm_block_host.py audits the flip share of exactly these
# ---------------------------------------------------------------------------------------------------
MASK_SEED = 0x9E3779B97F4A7C15   # the dropout seed of every test: both key words set
GENERIC_SHAPES = [(64, 1), (64, 2), (36, 3), (20, 5), (80, 4), (196, 4), (12, 4), (4, 4)]   # (h, heads)
# family -> (h, heads, n, backward too)
ATTN_FAMILIES = {
    "board": [(16 * hd, hd, n, True) for hd in (1, 2, 3, 4) for n in (1, 3, 4, 5, 9)],
    "head": [(64, 4, 5, True), (128, 8, 3, True), (512, 32, 3, True)],
    "generic": [(h, hd, 5, False) for h, hd in GENERIC_SHAPES],
}


def attn_gauss_runs(bwd):
    """(input seed, dout kind, p, counter, offset) of the Gaussian runs of one shape."""
    runs = [(0, dk, 0.0, 0, 0) for dk in (DOUT_KINDS if bwd else ("gauss",))]
    return runs + [(1, "gauss", p, 2 ** 33 + 5, 1) for p in (0.1, 0.5, 0.9)]


SWIGLU_INTERS = (1, 2, 64, 119, 120, 127, 128)
SWIGLU_WRAPS = (2049, 4099, 16385)
COLSUM_NBLK = (1, 15, 16, 17, 127, 128, 129, 2048)
# (kind, boards, inter, seed) of every Gaussian SwiGLU-conv run
SWIGLU_SHAPE_RUNS = {inter: [("gauss", nb, inter, 0) for nb in (1, 3, 4, 5)] + [(k, 5, inter, 0) for k in ("w0zero", "w1zero")]
                     for inter in SWIGLU_INTERS}
SWIGLU_WRAP_RUNS = [("gauss", nb, 8, 0) for nb in SWIGLU_WRAPS]
SWIGLU_COLSUM_RUNS = [("gauss", nblk, 8, 1) for nblk in COLSUM_NBLK]
SWIGLU_VALUE_RUNS = [(kind, 5, inter, 0) for kind in ("edges", "leak", "flat") for inter in (8, 119)] + [("leak", 2049, 8, 0)]
