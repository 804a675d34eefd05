"""The GameMLP layer kernels (csrc/ppo_update.hip with csrc/ln_row.hpp and csrc/ppo_common.hpp: the dropout keep
mask, the LayerNorm + ReLU + dropout + residual block forward and backward, the fused Linear + block forward,
the input and weight gradients, the column sums and the rollout heads), restated in plain numpy (no torch) in
float64 WITH the kernels' rounding points -- the reference tests/test_gpu_mlp_layer_edges.py holds every stored
output to, element by element.

As tests/urm_block_reference.py, every function returns for each stored output the unrounded float64 value
`x` the kernel rounds and the allowances `arith` (the fp32 arithmetic between the rounding points) and, where
there is one, `flip` (the ReLU gate of the backward is the one discontinuity: an element whose |z| lies within
its own arithmetic error may take either branch; its whole contribution is propagated to first order to the
row's dg through both row means and to the column's dgamma / dbeta).  The rounding points, read off the
kernels:
  * G = bf16(fp32 sum_k x w) is stored and the block normalises the ROUNDED G (round_g), so the GPU test
    holds G to linear() and mean / rstd / y to ln_block_fwd evaluated on the kernel's own G bits;
  * mean, rstd are fp32 (eps = 1e-5f, biased variance); y, dg, P are one bf16 rounding of an fp32 value;
  * the backward reads the stored fp32 mean / rstd: it is evaluated from GIVEN statistics, so it is judged
    independently of the forward;
  * the rollout heads use bf16(weight) (head_fwd_kernel converts the fp32 head weights once: a rounding of
    an input, exact and deterministic, so it is restated, not allowed for) and fp32 biases;
  * thr = trunc(double(p) 2^16 + 0.5) (0x10000 from p 2^16 >= 65536), scale = 1.0f / (1.0f - p).
ppo_update.hip is built with contraction on, ln_fwd_kernel takes 1.0f / sqrtf and ln_row.hpp v_rsq_f32 with
explicit fmas: every `arith` covers a fused and an unfused evaluation (one rounding per operation written).
A sum of N fp32 terms in any order gets (N + 2) 2^-24 sum|term|; the reductions over rows go through lanes,
waves, blocks and the column sum, so a term passes through at most `chain` additions and the sum gets
chain 2^-24 sum|term|.  tests/test_mlp_layer_host.py proves the reference against float64 autograd, measures
the rsqrt unit at the row widths used here and audits the caps of every case listed at the end of this file.
No number is tuned against kernel output."""

from __future__ import annotations

import numpy as np

from ppo_loss_reference import bf16_round  # noqa: F401  (re-exported for the tests)
from urm_block_reference import (DEVICE_FACTOR, FLIP_SHARE, U23, U24, UNITS, UNITS_HEADROOM, _bf, budget,  # noqa: F401
                                 check_bf16, check_f32, philox4x32_10, round_point)

LN_EPS = float(np.float32(1e-5))
# The rsqrt unit of urm_block_reference (1.10, measured on 64-wide rows) re-measured the same way -- the largest
# |fp32 numpy emulation of the whole mean / variance / 1 / sqrt chain - fp64| / rstd in units of 2^-23 -- at the row
# widths 4, 196 and 1024 over the gauss, mean256 and outlier rows gives 1.216 / 1.903 / 2.208: the constant does
# not hold here, so this file has its own, the measurement plus UNITS_HEADROOM rounded up to two decimals
# (tests/test_mlp_layer_host.py measures it and holds the constant both ways).  DEVICE_FACTOR stays assumed.
LN_RSQRT_UNIT = 2.32
LN_WIDTHS = (4, 196, 1024)


def ln_budget():
    return DEVICE_FACTOR * LN_RSQRT_UNIT * U23


def ln_rstd_f32(g, h):
    """The fp32 numpy emulation of the statistics chain (pairwise sums, 1 / sqrt): what sizes LN_RSQRT_UNIT."""
    g32 = np.asarray(g, np.float32)
    inv = np.float32(1.0) / np.float32(h)
    mean = g32.sum(1, keepdims=True, dtype=np.float32) * inv
    dv = g32 - mean
    var = (dv * dv).sum(1, keepdims=True, dtype=np.float32) * inv
    return (np.float32(1.0) / np.sqrt(var + np.float32(1e-5)))[:, 0].astype(np.float64)
DY_MAX_P = 4
MASK_SEED = 0x9E3779B97F4A7C15   # both key words set
LAYER_MAX, PASS_MAX = 255, 4095  # c1base = layer << 12 | pass << 20 beside the 7-bit pair index of h <= 1024


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def bfv(x):
    return _bf(np.asarray(x, np.float64))


# ---------------------------------------------------------------------------------------------------
# Dropout keep mask (ppo_common.hpp)
# ---------------------------------------------------------------------------------------------------
def drop_args(p):
    """(thr, scale) as ppo_common.hpp's drop_args forms them: a double product, + 0.5, truncation; fp32
    1 / (1 - p).  p <= 0: (0, 1.0), no mask."""
    p32 = np.float32(p)
    if not p32 > 0:
        return 0, 1.0
    t = float(p32) * 65536.0
    thr = 0x10000 if t >= 65536.0 else int(t + 0.5)
    with np.errstate(divide="ignore"):
        scale = float(np.float32(1.0) / (np.float32(1.0) - p32))
    return thr, scale


def pair_of(cg):
    """The Philox call index of column group cg = 8 a + 4 half + b: 4 a + b."""
    cg = np.asarray(cg)
    return ((cg >> 3) << 2) | (cg & 3)


def keep_mask(m, h, p, layer=0, pass_=0, seed=MASK_SEED, counter=0, counter_dev=None):
    """(mask uint8 [m, h], thr, scale): element (r, 4 cg + e) is kept iff its 16-bit uniform >= thr; the uniforms
    of groups cg and cg ^ 4 are the 8 half-words of philox({r, pair | layer << 12 | pass << 20, lo(c), hi(c)},
    key = the seed's words), c = counter + *counter_dev mod 2^64: words x, y for cg & 4 == 0, z, w otherwise,
    low half first."""
    thr, scale = drop_args(p)
    if thr == 0 and not np.float32(p) > 0:
        return np.ones((m, h), np.uint8), thr, scale
    c = (int(counter) + (0 if counter_dev is None else int(counter_dev))) & (2 ** 64 - 1)
    r, cg = np.meshgrid(np.arange(m, dtype=np.int64), np.arange(h // 4, dtype=np.int64), indexing="ij")
    c1 = pair_of(cg) | ((int(layer) << 12) & 0xFFFFFFFF) | ((int(pass_) << 20) & 0xFFFFFFFF)
    ctr = np.stack([r & 0xFFFFFFFF, c1, np.full_like(r, c & 0xFFFFFFFF), np.full_like(r, c >> 32)], -1)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])).astype(np.int64)
    hi = (cg & 4) != 0
    a, b = np.where(hi, w[..., 2], w[..., 0]), np.where(hi, w[..., 3], w[..., 1])
    u = np.stack([a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16], -1).reshape(m, h)
    return (u >= thr).astype(np.uint8), thr, scale


# ---------------------------------------------------------------------------------------------------
# LayerNorm + ReLU + dropout + residual
# ---------------------------------------------------------------------------------------------------
def ln_block_fwd(g, gamma, beta, res=None, mask=None, scale=1.0):
    """g [m, h] bf16 values, gamma / beta fp32 values, res bf16 values or None, mask 0 / 1 or None.
    mean, rstd (fp32 outputs) and y = res + mask scale max(xhat gamma + beta, 0) (bf16 output), each with its
    allowance.  There is no intermediate rounding point."""
    g = np.asarray(g, np.float64)
    h = g.shape[1]
    mean = g.mean(1, keepdims=True)
    # the sum of h values in any order, the product with fp32(1 / h) (its own rounding and the result's)
    e_mean = (h + 2) * U24 * np.abs(g).sum(1, keepdims=True) / h + 3 * U24 * np.abs(mean)
    dv = g - mean
    e_dv = e_mean + U24 * np.abs(dv)
    var = (dv * dv).mean(1, keepdims=True)
    e_var = ((2 * np.abs(dv) * e_dv + e_dv * e_dv).sum(1, keepdims=True) + (h + 4) * U24 * (dv * dv).sum(1, keepdims=True)) / h \
        + 3 * U24 * var
    ve = var + LN_EPS
    rstd = ve ** -0.5
    rel_r = 0.5 * (e_var + U24 * ve) / ve + ln_budget()
    xhat = dv * rstd
    z = xhat * gamma + beta
    e_z = np.abs(gamma) * (np.abs(xhat) * rel_r + e_dv * rstd + 2 * U24 * np.abs(xhat)) + 2 * U24 * (np.abs(xhat * gamma) + np.abs(beta))
    k = scale if mask is None else np.asarray(mask, np.float64) * scale
    a = np.maximum(z, 0.0) * k
    y = a if res is None else res + a
    # a cut or dropped element adds an exact 0: y is res (or 0) bit for bit
    y_arith = (k * e_z + U24 * np.abs(a) + U24 * np.abs(y)) * ((z > -e_z) & (k > 0))
    return {"mean": mean[:, 0], "mean_allow": e_mean[:, 0], "rstd": rstd[:, 0], "rstd_allow": (rstd * rel_r)[:, 0],
            "y": y, "y_arith": y_arith, "z": z, "z_err": e_z}


def bwd_blocks(m, h, tile196):
    """Partial rows and the row -> partial row map of g2048_ln_act_bwd: the h = 196 tile kernel gives 16-row tiles
    to 8 waves per block, the generic kernel row pairs to 16 waves per block."""
    r = np.arange(m)
    if tile196:
        nb = max(1, min(256, -(-(-(-m // 16)) // 8), min(2048, max(1, -(-m // 16)))))
        return nb, ((r // 16) // 8) % nb, -(-m // (16 * 8 * nb))
    nb = max(1, min(256, -(-m // 64)))
    return nb, ((r // 2) // 16) % nb, 2 * -(-m // (2 * 16 * nb))


def bwd_chain(m, h, tile196):
    """(additions a term of a partial row passes through at most, and of dgamma / dbeta): the rows of one lane's
    accumulator, the 16-lane rotate sum or the block's waves (<= 16 + 6 with slack), then the column sum over the nb
    partial rows in any order."""
    nb, _, per_acc = bwd_blocks(m, h, tile196)
    return per_acc + 16 + 6, per_acc + 16 + 6 + nb + 8


def ln_block_bwd(g, mean, rstd, gamma, beta, dres=None, ps=(), head=None, mask=None, scale=1.0, tile196=False,
                 rounding=True):
    """Backward of ln_block_fwd from the GIVEN fp32 statistics.  head = (dz [m, >= 5], wa [4, h], wv [h] or None).
    Returns dy (dres_out, fp32), dg (bf16), the per-block partial rows part [nb, 2 h] (dgamma | dbeta) and their
    sums, each with arith and flip allowances."""
    g = np.asarray(g, np.float64)
    m, h = g.shape
    mean, rstd = np.asarray(mean, np.float64).reshape(m, 1), np.asarray(rstd, np.float64).reshape(m, 1)
    terms = []
    if head is not None:
        dz, wa, wv = head
        terms += [dz[:, k:k + 1] * wa[k][None, :] for k in range(4)]
        if wv is not None:
            terms.append(dz[:, 4:5] * np.asarray(wv).reshape(1, h))
    if dres is not None:
        terms.append(np.asarray(dres, np.float64))
    terms += [np.asarray(p, np.float64) for p in ps]
    dy = sum(terms) if terms else np.zeros((m, h))
    mag = sum(np.abs(t) for t in terms) if terms else np.zeros((m, h))
    single = len(terms) <= 1 and head is None
    e_dy = np.zeros((m, h)) if single or not rounding else (len(terms) + 2) * U24 * mag
    u = U24 if rounding else 0.0
    xhat = (g - mean) * rstd
    e_xh = 2 * u * np.abs(xhat)
    z = xhat * gamma + beta
    e_z = np.abs(gamma) * e_xh + 2 * u * (np.abs(xhat * gamma) + np.abs(beta))
    on = z > 0
    amb = (np.abs(z) <= e_z) & (e_z > 0)
    k = np.ones((m, h)) if mask is None else np.asarray(mask, np.float64) * scale
    dzr = np.where(on, dy * k, 0.0)
    e_dzr = np.where(on | amb, k * e_dy + u * np.abs(dy * k), 0.0)
    f_dzr = np.where(amb, np.abs(dy * k), 0.0)
    dxh = dzr * gamma
    e_dxh, f_dxh = np.abs(gamma) * e_dzr + u * np.abs(dxh), np.abs(gamma) * f_dzr
    s1 = dxh.mean(1, keepdims=True)
    s2 = (dxh * xhat).mean(1, keepdims=True)
    e_s1 = (e_dxh.sum(1, keepdims=True) + (h + 3) * u * np.abs(dxh).sum(1, keepdims=True)) / h + 2 * u * np.abs(s1)
    e_s2 = ((e_dxh * np.abs(xhat) + np.abs(dxh) * e_xh).sum(1, keepdims=True)
            + (h + 3) * u * np.abs(dxh * xhat).sum(1, keepdims=True)) / h + 2 * u * np.abs(s2)
    f_s1, f_s2 = f_dxh.sum(1, keepdims=True) / h, (f_dxh * np.abs(xhat)).sum(1, keepdims=True) / h
    dg = rstd * (dxh - s1 - xhat * s2)
    dg_arith = rstd * (e_dxh + e_s1 + np.abs(xhat) * e_s2 + e_xh * np.abs(s2)
                       + 3 * u * (np.abs(dxh) + np.abs(s1) + np.abs(xhat * s2))) + 2 * u * np.abs(dg)
    dg_flip = rstd * (f_dxh + f_s1 + np.abs(xhat) * f_s2)
    # dgamma | dbeta: the terms, their partial rows and sums
    t = np.concatenate([dzr * xhat, dzr], 1)
    e_t = np.concatenate([e_dzr * np.abs(xhat) + np.abs(dzr) * e_xh + u * np.abs(dzr * xhat), e_dzr], 1)
    f_t = np.concatenate([f_dzr * np.abs(xhat), f_dzr], 1)
    nb, blk, per_acc = bwd_blocks(m, h, tile196)
    part, part_arith, part_flip = (np.zeros((nb, 2 * h)) for _ in range(3))
    absp = np.zeros((nb, 2 * h))
    np.add.at(part, blk, t)
    np.add.at(part_arith, blk, e_t)
    np.add.at(part_flip, blk, f_t)
    np.add.at(absp, blk, np.abs(t))
    chain_p, chain = bwd_chain(m, h, tile196)
    part_arith += chain_p * u * absp
    return {"dy": dy, "dy_arith": e_dy, "dg": dg, "dg_arith": dg_arith, "dg_flip": dg_flip, "z": z, "amb": amb,
            "nb": nb, "part": part, "part_arith": part_arith, "part_flip": part_flip,
            "dgamma": t[:, :h].sum(0), "dbeta": t[:, h:].sum(0),
            "dgamma_arith": (e_t.sum(0) + chain * u * np.abs(t).sum(0))[:h], "dbeta_arith": (e_t.sum(0) + chain * u * np.abs(t).sum(0))[h:],
            "dgamma_flip": f_t.sum(0)[:h], "dbeta_flip": f_t.sum(0)[h:], "terms": t, "terms_err": e_t, "terms_flip": f_t,
            "chain": chain}


# ---------------------------------------------------------------------------------------------------
# The GEMMs
# ---------------------------------------------------------------------------------------------------
def linear(x, w, rounding=True):
    """G = bf16(fp32 sum_k x w^T): x [m, K], w [N, K] bf16 values.  (G unrounded, arith)."""
    K = x.shape[1]
    G = x @ w.T
    return G, ((K + 2) * U24 * (np.abs(x) @ np.abs(w).T) if rounding else np.zeros_like(G))


def dgrad(dg, w, rounding=True):
    """P = bf16(fp32 sum_n dg w): dg [m, N], w [N, K]."""
    N = dg.shape[1]
    P = dg @ w
    return P, ((N + 2) * U24 * (np.abs(dg) @ np.abs(w)) if rounding else np.zeros_like(P))


def wgrad(a, b, rounding=True):
    """out [n1, n2] = fp32 sum_r a[r, :]^T b[r, :] over per-block partials and the column sum: any order."""
    m = a.shape[0]
    out = a.T @ b
    return out, ((m + 2) * U24 * (np.abs(a).T @ np.abs(b)) if rounding else np.zeros_like(out))


def colsum(part, segs, max_col=-1):
    """part [nb, cols] fp32 values -> per segment (value, allowance): the column sums in any order, the column
    max_col taking the maximum (exact)."""
    part = np.asarray(part, np.float64)
    nb = part.shape[0]
    s = part.sum(0)
    allow = (nb + 2) * U24 * np.abs(part).sum(0)
    if max_col >= 0:
        s[max_col], allow[max_col] = part[:, max_col].max(), 0.0
    out, off = [], 0
    for n in segs:
        out.append((s[off:off + n], allow[off:off + n]))
        off += n
    assert off == part.shape[1]
    return out


def head_fwd(x, wa, ba, wv, bv):
    """logits [m, 4] = x bf16(wa)^T + ba, value [m] = x bf16(wv) + bv (fp32 outputs) and their allowances."""
    h = x.shape[1]
    w = bfv(np.concatenate([np.asarray(wa, np.float64).reshape(4, h), np.asarray(wv, np.float64).reshape(1, h)]))
    b = np.concatenate([np.asarray(ba, np.float64).reshape(4), np.asarray(bv, np.float64).reshape(1)])
    z = x @ w.T + b
    allow = (h + 3) * U24 * (np.abs(x) @ np.abs(w).T + np.abs(b))
    return z[:, :4], z[:, 4], allow[:, :4], allow[:, 4]


def exact_in_any_order(terms, unit, axis=0):
    """Every term is an integer multiple of `unit` and sum|term| stays below 2^24 units along `axis`: every partial
    sum in every order is an integer below 2^24 units, i.e. exact in fp32."""
    t = np.asarray(terms, np.float64) / unit
    return bool((t == np.rint(t)).all() and (np.abs(t).sum(axis) < 2 ** 24).all())


def flip_share(flip, arith):
    return float((np.asarray(flip) > np.asarray(arith)).mean())


# ---------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------
ROW_KINDS = ("gauss", "const", "mean256", "outlier", "gamma0", "betaneg", "zero_gate", "near_gate")
NEAR_GATE_COLS = 2


def ln_case(kind, m, h, seed=0):
    """g [m, h] bf16 values, gamma, beta fp32 values, res bf16 values.
      gauss      g N(0.5, 3^2), gamma U(0.5, 1.5), beta N(0, 0.1^2)
      const      every row constant (variance exactly 0: rstd = eps^-1/2)
      mean256    mean 256 with deviations of one bf16 step (2): the variance is lost unless centred
      outlier    one 1e4 entry per row
      gamma0     gamma = 0: y = bf16(res + k max(beta, 0))
      betaneg    beta = -1e4: ReLU cuts everything, y = res exactly
      zero_gate  gamma = beta = 0: z == 0 exactly, the backward gate (z > 0) must cut the gradient
      near_gate  gauss with beta[j] = -fp32(xhat[j][j] gamma[j]) for j < NEAR_GATE_COLS (xhat from the fp32 statistics
                 the backward is given): z[j][j] lies within its own rounding of 0, either branch is right and the
                 flip allowance is what holds dg of those rows and dgamma / dbeta of those columns"""
    r = np.random.default_rng([seed, m, h, ROW_KINDS.index(kind)])
    g = bfv(r.normal(size=(m, h)) * 3 + 0.5)
    gamma = f32(r.uniform(0.5, 1.5, size=h))
    beta = f32(r.normal(size=h) * 0.1)
    res = bfv(r.normal(size=(m, h)))
    if kind == "const":
        g = np.repeat(bfv(r.normal(size=(m, 1)) * 3), h, 1)
    elif kind == "mean256":
        g = 256.0 + 2.0 * r.integers(-1, 2, size=(m, h))
    elif kind == "outlier":
        g[np.arange(m), r.integers(0, h, size=m)] = float(bfv(1e4))
    elif kind == "gamma0":
        gamma[:] = 0.0
    elif kind == "betaneg":
        beta[:] = -1e4
    elif kind == "zero_gate":
        gamma[:] = 0.0
        beta[:] = 0.0
    elif kind == "near_gate":
        mean, rstd = given_stats(g)
        for j in range(min(NEAR_GATE_COLS, m, h)):
            beta[j] = f32(-(g[j, j] - mean[j]) * rstd[j] * gamma[j])
    return g, gamma, beta, res


def positive_case(m, h, seed=0):
    """ReLU(LN) > 0 everywhere (gamma = 1/4, beta = 8 against |xhat| <= sqrt(h) <= 32) and res = 1, so that
    y == res marks exactly the dropped elements: the mask a consumer applies, read back."""
    r = np.random.default_rng([seed, m, h, 99])
    return bfv(r.normal(size=(m, h))), np.full(h, 0.25), np.full(h, 8.0), np.ones((m, h))


def signed_perm(n, k, seed=0):
    """W [n, k] with one +-1 per row at column pi(row) (pi a permutation of k extended cyclically): G[r][j] =
    +- x[r][pi(j)] exactly, whatever the summation order."""
    r = np.random.default_rng([seed, n, k, 7])
    pi = np.concatenate([r.permutation(k) for _ in range(-(-n // k))])[:n]
    w = np.zeros((n, k))
    w[np.arange(n), pi] = r.choice([-1.0, 1.0], size=n)
    return w


def small_ints(shape, seed, lo=-2, hi=2):
    return np.random.default_rng([seed, *shape]).integers(lo, hi + 1, size=shape).astype(np.float64)


def backward_case(kind, m, h, np_src, head, with_dres, seed=0):
    """The inputs of one ln_act_bwd run: (g, gamma, beta, dres, ps, head)."""
    g, gamma, beta, _ = ln_case(kind, m, h, seed)
    r = np.random.default_rng([seed, m, h, np_src, 5])
    dres = f32(r.normal(size=(m, h))) if with_dres else None
    ps = [bfv(r.normal(size=(m, h))) for _ in range(np_src)]
    hd = None
    if head is not None:
        dz = np.zeros((m, 8))
        dz[:, :5] = f32(r.normal(size=(m, 5)) * 0.1)
        hd = (dz, f32(r.normal(size=(4, h)) * 0.05), f32(r.normal(size=h) * 0.05) if head == "coupled" else None)
    return g, gamma, beta, dres, ps, hd


def given_stats(g):
    """The fp32-rounded statistics the GPU test feeds the backward kernels."""
    f = ln_block_fwd(g, 1.0, 0.0)
    return f32(f["mean"]), f32(f["rstd"])


# ---------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_mlp_layer_edges.py, listed once: the GPU file runs exactly these and
# tests/test_mlp_layer_host.py audits the caps of exactly these
# ---------------------------------------------------------------------------------------------------
MASK_HS = (4, 36, 196, 256, 260, 1024)
MASK_PS = (2.0 ** -16, 1.5 * 2.0 ** -16, 0.1, 0.5, 1 - 2.0 ** -16)
MASK_COUNTERS = ((0, None), (2 ** 32 - 1, 1), (2 ** 33 + 5, None), (0, 2 ** 32 + 7))
MASK_LAYER_PASS = ((1, 0), (2, 0), (1, 1), (2, 1), (LAYER_MAX, PASS_MAX))   # the updater's blocks and passes; the largest

LN_FWD_HS = (4, 60, 196, 256, 260, 512, 516, 768, 772, 1024)
LN_FWD_MS = (1, 15, 16, 17)
LN_FWD_WRAP = (32769, 4)          # 16 rows per block, 2048 blocks: one row past a full sweep

# generic ln_bwd_kernel: (h, m, np_src, head, with_dres, p)
LN_BWD_GENERIC = [(h, m, n_src, head, dres, p)
                  for h, m, n_src, head, dres, p in (
                      (4, 1, 0, None, True, 0.0), (60, 3, 1, "coupled", False, 0.1), (196, 4, 3, "coupled", False, 0.1),
                      (196, 5, 3, "decoupled", False, 0.0), (256, 63, 2, None, True, 0.5), (260, 64, 0, "coupled", True, 0.1),
                      (512, 65, 1, "decoupled", True, 0.0), (516, 5, 4, None, False, 0.1), (768, 17, 1, "coupled", True, 0.0),
                      (772, 4, 2, None, True, 0.1), (1024, 33, 1, "coupled", True, 0.1), (196, 65, 1, None, True, 0.1),
                      (64, 8193, 1, "coupled", True, 0.1))]
# ln_bwd196_kernel: every (DROP, HEAD, NP) at the ragged and full tile counts
LN_BWD_196_MS = (1, 15, 16, 17, 127, 128, 129)
LN_BWD_196 = [(196, LN_BWD_196_MS[(3 * i + j) % len(LN_BWD_196_MS)], n_src, head, False, p)
              for i, (p, head) in enumerate(((0.0, None), (0.0, "coupled"), (0.1, None), (0.1, "coupled"), (0.5, "decoupled")))
              for j, n_src in enumerate((0, 1, 2))]
LN_BWD_WRAP_196 = 32769           # 256 blocks x 8 waves x 16 rows = 32768
LN_BWD_WRAP_GENERIC = 8193        # 256 blocks x 16 waves x 2 rows = 8192

MLP_FWD_NS = (4, 16, 20, 32, 36, 48, 52, 64, 68, 96, 100, 128, 132, 160, 164, 192, 196, 208, 212, 256)
MLP_FWD_KS = (4, 36, 48)
MLP_FWD_MS = (1, 15, 16, 17, 63, 64, 65, 129)
MLP_FWD_PATHS = {"generic13": [(196, 100), (208, 4)], "ks7": [(208, 208), (200, 224)], "ks2": [(208, 36), (200, 64)],
                 "wide": [(196, 196), (196, 48)]}
MLP_FWD_WRAP_SLAB, MLP_FWD_WRAP_WIDE = 16449, 32785

DGRAD_HS = (64, 128, 196)
DGRAD_MS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
DGRAD_WRAPS = {64: 65569, 128: 65569, 196: 32801}

WGRAD_SHAPES = [(64, 48), (64, 128), (32, 224), (128, 224), (128, 32), (68, 36), (68, 52), (224, 48), (132, 52),
                (196, 196), (16, 196), (4, 8)]
WGRAD_MS = (1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
WGRAD_WRAP = 131137

MLP_WGRAD_HS = (196, 192, 128, 64, 32)
MLP_WGRAD_MS = (1, 31, 32, 33, 4099)
MLP_WGRAD_WRAP = {196: 32801, 192: 8225, 128: 8225, 64: 8225, 32: 8225}   # past 256 x 32 rows of every product

COLSUM_NBS = (1, 31, 32, 33, 255, 256, 2048)
COLSUM_COLS = (2, 63, 64, 65, 392)

HEAD_HS = (4, 32, 36, 196, 256)
HEAD_MS = (1, 15, 16, 17, 4099)


def wg_plan(m, n1, n2, rows_target=512):
    """(bi, wi, ny, nb, rows) as csrc/ppo_update.hip's wg_plan chooses them."""
    TI, TJ0 = -(-n1 // 16), -(-n2 // 16)
    ny = 2 if TJ0 >= 4 else 1
    TJ = -(-TJ0 // ny)
    for bi, bj in ((2, 2), (4, 4), (7, 4)):
        for wi, wj in ((2, 2), (4, 1), (1, 4)):
            if wi * bi >= TI and wj * bj >= TJ:
                nb = min(256, max(1, m // rows_target))
                rows = -(-(-(-m // nb)) // 64) * 64
                return bi, wi, ny, -(-m // rows), rows
    return None


def ln_fwd_runs():
    """(kind, m, h, with_res, p) of every ln_act_fwd run."""
    runs = []
    for i, h in enumerate(LN_FWD_HS):
        for j, m in enumerate(LN_FWD_MS):
            runs.append(("gauss", m, h, (i + j) % 2 == 0, (0.0, 0.1, 0.5)[(i + 2 * j) % 3]))
        runs.append(("gauss", 17, h, True, 0.0))
        runs.append(("gauss", 17, h, False, 0.1))
    for kind in ROW_KINDS[1:-1]:
        for h in (4, 196, 516, 1024):
            runs.append((kind, 17, h, True, 0.5 if kind in ("gamma0", "betaneg") else 0.0))
    runs.append(("gauss", LN_FWD_WRAP[0], LN_FWD_WRAP[1], True, 0.1))
    runs.append(("gauss", 4099, 196, True, 0.1))
    return runs


def ln_bwd_runs():
    """(kind, h, m, np_src, head, with_dres, p, tile196) of every Gaussian / row-kind ln_act_bwd run."""
    runs = [("gauss",) + c + (False,) for c in LN_BWD_GENERIC] + [("gauss",) + c + (True,) for c in LN_BWD_196]
    for kind in ROW_KINDS[1:]:
        runs.append((kind, 196, 65 if kind == "near_gate" else 17, 1, "coupled", False, 0.1, True))
        runs.append((kind, 260, 65 if kind == "near_gate" else 5, 1, "coupled", True, 0.1, False))
    runs.append(("gauss", 196, 1000, 2, "coupled", False, 0.1, True))
    return runs
