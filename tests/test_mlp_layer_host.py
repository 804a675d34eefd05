"""The fp64 reference of the GameMLP layer kernels (tests/mlp_layer_reference.py) is right before any kernel is
compared with it: with its rounding switched off it equals float64 autograd of y = res + Dropout(ReLU(LayerNorm(
x W^T))), of the weight and input gradients and of dgamma / dbeta; the numpy keep mask equals a second, scalar,
straight-from-the-paper Philox under ppo_common.hpp's layout; thr / scale take the values drop_args forms; the
rsqrt unit is measured here (printed: run with -s) and held against the module's constant both ways; and every
case tests/test_gpu_mlp_layer_edges.py runs keeps the caps: the flip term exceeds the arithmetic term on at most
FLIP_SHARE of each output, every allowance is finite, the allowance of a Gaussian case stays below one bf16
step, and the exact cases are exact in fp32 in any summation order.  CPU only."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_layer_reference as R

SEED = R.MASK_SEED


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


# ---------------------------------------------------------------------------------------------------
# Against float64 autograd
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,p,head", [(37, 196, 0.1, "coupled"), (9, 260, 0.5, "decoupled"), (5, 4, 0.0, None),
                                        (33, 64, 0.25, "coupled")])
def test_reference_without_rounding_is_float64_autograd(m, h, p, head):
    g = np.random.default_rng([m, h])
    x, w = g.normal(size=(m, h)), g.normal(size=(h, h)) / h ** 0.5
    gamma, beta = g.uniform(0.5, 1.5, size=h), g.normal(size=h) * 0.1
    mask, _, scale = R.keep_mask(m, h, p, 2, 1, SEED, 5) if p > 0 else (None, 0, 1.0)
    dres, ps = g.normal(size=(m, h)), [g.normal(size=(m, h)) for _ in range(2)]
    hd = None
    if head is not None:
        hd = (g.normal(size=(m, 8)), g.normal(size=(4, h)), g.normal(size=h) if head == "coupled" else None)
    tx, tw, tg, tb = (_t(a).requires_grad_(True) for a in (x, w, gamma, beta))
    tG = tx @ tw.T
    tG.retain_grad()
    a = torch.relu(F.layer_norm(tG, (h,), tg, tb, eps=R.LN_EPS))
    if mask is not None:
        a = a * _t(mask) * scale
    ty = tx + a
    tdy = _t(dres) + sum(_t(q) for q in ps)
    if hd is not None:
        tdy = tdy + _t(hd[0][:, :4]) @ _t(hd[1]) + (_t(hd[0][:, 4:5]) @ _t(hd[2]).view(1, h) if hd[2] is not None else 0)
    ty.backward(tdy)

    G, G_allow = R.linear(x, w, rounding=False)
    assert not G_allow.any()
    np.testing.assert_allclose(G, tG.detach().numpy(), rtol=1e-12, atol=1e-14)
    f = R.ln_block_fwd(G, gamma, beta, x, mask, scale)
    np.testing.assert_allclose(f["y"], ty.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(f["mean"], tG.detach().mean(1).numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(f["rstd"], (tG.detach().var(1, unbiased=False) + R.LN_EPS).rsqrt().numpy(), rtol=1e-12)
    b = R.ln_block_bwd(G, f["mean"], f["rstd"], gamma, beta, dres, ps, hd, mask, scale, rounding=False)
    np.testing.assert_allclose(b["dy"], tdy.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(b["dg"], tG.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b["dgamma"], tg.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b["dbeta"], tb.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b["part"].sum(0), np.concatenate([b["dgamma"], b["dbeta"]]), rtol=1e-12, atol=1e-12)
    assert not b["dg_flip"].any() or b["amb"].any()
    dw, _ = R.wgrad(b["dg"], x, rounding=False)
    np.testing.assert_allclose(dw, tw.grad.numpy(), rtol=1e-12, atol=1e-12)
    dx, _ = R.dgrad(b["dg"], w, rounding=False)
    np.testing.assert_allclose(dx + b["dy"], tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    # both partial layouts sum the same terms
    b2 = R.ln_block_bwd(G, f["mean"], f["rstd"], gamma, beta, dres, ps, hd, mask, scale, tile196=True, rounding=False)
    np.testing.assert_allclose(b2["part"].sum(0), b["part"].sum(0), rtol=1e-12, atol=1e-12)


def test_partial_rows_follow_the_kernels_row_assignment():
    """Generic kernel: row pairs to 16 waves per block; h = 196 kernel: 16-row tiles to 8 waves per block."""
    nb, blk, per = R.bwd_blocks(8193, 64, False)
    assert nb == 129 and blk[0] == blk[31] == 0 and blk[32] == 1 and blk[32 * 129] == 0 and per == 4
    nb, blk, per = R.bwd_blocks(32769, 196, True)
    assert nb == 256 and blk[127] == 0 and blk[128] == 1 and blk[32768] == 0 and per == 2
    nb, blk, _ = R.bwd_blocks(17, 196, True)
    assert nb == 1 and not blk.any()
    assert R.bwd_blocks(129, 196, True)[0] == 2 and R.bwd_blocks(65, 260, False)[0] == 2


def test_colsum_and_head_reference():
    g = np.random.default_rng(3)
    part = R.f32(g.normal(size=(33, 10)))
    (a, ea), (b, eb) = R.colsum(part, (7, 3), max_col=8)
    np.testing.assert_allclose(np.concatenate([a, b[:1], b[2:]]), part.sum(0)[[0, 1, 2, 3, 4, 5, 6, 7, 9]], rtol=1e-13)
    assert b[1] == part[:, 8].max() and eb[1] == 0.0 and (ea > 0).all()
    x, wa, wv = R.bfv(g.normal(size=(5, 36))), R.f32(g.normal(size=(4, 36))), R.f32(g.normal(size=36))
    lg, v, el, ev = R.head_fwd(x, wa, [1, 2, 3, 4], wv, [5])
    np.testing.assert_allclose(lg, x @ R.bfv(wa).T + np.arange(1, 5), rtol=1e-13)
    np.testing.assert_allclose(v, x @ R.bfv(wv) + 5, rtol=1e-13)
    assert not np.array_equal(R.bfv(wa), wa) and (el > 0).all() and (ev > 0).all()


# ---------------------------------------------------------------------------------------------------
# The keep mask
# ---------------------------------------------------------------------------------------------------
def _philox_scalar(ctr, key):
    """Philox4x32-10 as the paper (Salmon et al., SC'11) writes it, one counter at a time in Python integers."""
    M0, M1, W0, W1, m32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c, k = list(ctr), list(key)
    for _ in range(10):
        hi0, lo0 = (M0 * c[0]) >> 32, (M0 * c[0]) & m32
        hi1, lo1 = (M1 * c[2]) >> 32, (M1 * c[2]) & m32
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + W0) & m32, (k[1] + W1) & m32]
    return c


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10."""
    assert _philox_scalar([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_scalar([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox_scalar([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("counter,counter_dev", R.MASK_COUNTERS)
def test_keep_mask_is_the_scalar_philox_in_the_kernels_layout(counter, counter_dev):
    m, h, p, layer, pass_ = 70, 1024, 0.3, 2, 1
    mask, thr, scale = R.keep_mask(m, h, p, layer, pass_, SEED, counter, counter_dev)
    assert thr == 19661 and scale == float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    c = (counter + (counter_dev or 0)) % 2 ** 64
    for row, cg in ((0, 0), (0, 4), (3, 7), (69, 255), (17, 12), (17, 8), (5, 131), (5, 135)):
        pair = ((cg >> 3) << 2) | (cg & 3)
        w = _philox_scalar([row, pair | layer << 12 | pass_ << 20, c & 0xFFFFFFFF, c >> 32], [SEED & 0xFFFFFFFF, SEED >> 32])
        a, b = (w[2], w[3]) if cg & 4 else (w[0], w[1])
        want = [int(u >= thr) for u in (a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16)]
        assert mask[row, 4 * cg:4 * cg + 4].tolist() == want, (row, cg)
    # the pairing rule: cg and cg ^ 4 share one call
    cg = np.arange(256)
    assert np.array_equal(R.pair_of(cg), R.pair_of(cg ^ 4)) and len(set(R.pair_of(cg).tolist())) == 128
    assert int(R.pair_of(cg).max()) == 127 < 1 << 12    # the layer field starts above the pair index


def test_drop_args_thresholds():
    """thr = trunc(p 2^16 + 0.5): 1.5 2^-16 sits on the half-way point and goes UP (lrintf's ties-to-even would
    also give 2; 2.5 2^-16 tells them apart: 3 here, 2 by ties-to-even)."""
    assert R.drop_args(0.0) == (0, 1.0) and R.drop_args(-1.0) == (0, 1.0)
    assert R.drop_args(2.0 ** -16) == (1, float(np.float32(1) / (np.float32(1) - np.float32(2.0 ** -16))))
    assert R.drop_args(1.5 * 2.0 ** -16)[0] == 2 and R.drop_args(2.5 * 2.0 ** -16)[0] == 3
    assert R.drop_args(0.5) == (32768, 2.0) and R.drop_args(0.1)[0] == 6554
    assert R.drop_args(1 - 2.0 ** -16) == (65535, 65536.0)
    assert R.drop_args(1.0)[0] == 0x10000 and R.drop_args(2.0 ** -18)[0] == 0
    for p in R.MASK_PS:
        mask, thr, _ = R.keep_mask(64, 1024, p, 1, 0, SEED, 3)
        assert abs(mask.mean() - (1 - thr / 65536.0)) < 4 * (0.25 / mask.size) ** 0.5 + 1e-9, p


# ---------------------------------------------------------------------------------------------------
# The measured unit
# ---------------------------------------------------------------------------------------------------
def test_measured_rsqrt_unit():
    """max |fp32 emulation - fp64| / rstd in units of 2^-23 at the row widths of this family: no larger than the
    module's constant and no more than the headroom below it.  urm_block_reference's 64-wide constant is
    printed beside it: it does not hold at these widths, which is why this family has its own."""
    worst = {}
    for h in R.LN_WIDTHS:
        w = 0.0
        for kind in ("gauss", "mean256", "outlier"):
            g, _, _, _ = R.ln_case(kind, 4096, h, 5)
            r64 = R.ln_block_fwd(g, 1.0, 0.0)["rstd"]
            w = max(w, float((np.abs(R.ln_rstd_f32(g, h) - r64) / r64).max() / R.U23))
        worst[h] = w
    print("measured rsqrt chain units of 2^-23 per width:", {h: round(w, 3) for h, w in worst.items()}, "constant:",
          R.LN_RSQRT_UNIT, "urm constant:", R.UNITS["rsqrt"], "device factor (assumed):", R.DEVICE_FACTOR)
    u = max(worst.values())
    assert u <= R.LN_RSQRT_UNIT
    assert R.LN_RSQRT_UNIT <= (1.0 + R.UNITS_HEADROOM) * u + 0.01
    assert R.DEVICE_FACTOR == 4.0


# ---------------------------------------------------------------------------------------------------
# The caps of every case the GPU file runs
# ---------------------------------------------------------------------------------------------------
def _bwd(run, seed=0):
    kind, h, m, n_src, head, dres, p, t196 = run
    g, gamma, beta, dr, ps, hd = R.backward_case(kind, m, h, n_src, head, dres, seed)
    mean, rstd = R.given_stats(g)
    mask, _, scale = R.keep_mask(m, h, p, 1, 0, SEED, 3) if p > 0 else (None, 0, 1.0)
    return R.ln_block_bwd(g, mean, rstd, gamma, beta, dr, ps, hd, mask, scale, tile196=t196)


def test_backward_cases_keep_the_caps():
    worst, amb_cases = {}, 0
    for run in R.ln_bwd_runs():
        b = _bwd(run)
        for name in ("dg", "dgamma", "dbeta", "part"):
            assert np.isfinite(b[name + "_arith"]).all() and np.isfinite(b[name + "_flip"]).all(), (run, name)
            share = R.flip_share(b[name + "_flip"], b[name + "_arith"])
            assert share <= R.FLIP_SHARE, (run, name, share)
            worst[name] = max(worst.get(name, 0.0), share)
        assert np.isfinite(b["dy_arith"]).all()
        amb_cases += bool(b["amb"].any())
        if run[0] == "gauss" and run[4] is not None or run[3]:
            nz = np.abs(b["dg"]) > 0
            if run[0] == "gauss" and nz.any():
                med = float(np.median(b["dg_arith"][nz] / np.abs(b["dg"][nz])))
                assert med < 2.0 ** -8, (run, med)
        if run[0] == "near_gate":   # the case reaches the branch it is named for
            assert b["amb"][:R.NEAR_GATE_COLS, :R.NEAR_GATE_COLS].diagonal().all(), run
        if run[0] == "zero_gate":
            assert not b["amb"].any() and not b["dg"].any() and not b["dgamma"].any() and not b["dbeta"].any()
    print("largest flip share per output:", {k: round(v, 4) for k, v in worst.items()}, "cases with an ambiguous gate:",
          amb_cases)
    assert amb_cases >= 2


def test_forward_cases_keep_the_caps():
    worst = 0.0
    for kind, m, h, with_res, p in R.ln_fwd_runs():
        if m > 5000:
            m = 257    # the wrap run repeats the Gaussian rows of its shape: audited on its first rows
        g, gamma, beta, res = R.ln_case(kind, m, h)
        mask, _, scale = R.keep_mask(m, h, p, 1, 0, SEED, 3) if p > 0 else (None, 0, 1.0)
        f = R.ln_block_fwd(g, gamma, beta, res if with_res else None, mask, scale)
        for name in ("mean_allow", "rstd_allow", "y_arith"):
            assert np.isfinite(f[name]).all(), (kind, m, h, name)
        if kind == "gauss":
            nz = np.abs(f["y"]) > 0
            med = float(np.median(f["y_arith"][nz] / np.abs(f["y"][nz])))
            assert med < 2.0 ** -8, (kind, m, h, med)
            worst = max(worst, med)
        if kind == "betaneg":
            assert with_res and np.array_equal(f["y"], res) and not f["y_arith"].any()
        if kind == "const":
            assert np.allclose(f["rstd"], R.LN_EPS ** -0.5, rtol=1e-12)
    print("largest median arith / |y| of a Gaussian case, in bf16 steps:", round(worst * 256, 4))


@pytest.mark.parametrize("h,m", [(196, 1000), (1024, 300), (64, 4099)])
def test_gate_ambiguous_rows_are_rare(h, m):
    """A crude estimate with a worst-case h 2^-24 bound on z (as if the statistics carried the error of an h-term
    sum): the share of rows with a gate the backward could take either way stays below 3 %.  With the GIVEN fp32
    statistics no sum enters z and the reference's own e_z is a few 2^-24: its share is printed beside it."""
    g, gamma, beta, dres, ps, hd = R.backward_case("gauss", m, h, 1, "coupled", False, 0)
    mean, rstd = R.given_stats(g)
    b = R.ln_block_bwd(g, mean, rstd, gamma, beta, dres, ps, hd)
    xh = (g - mean[:, None]) * rstd[:, None]
    crude = float((np.abs(b["z"]) <= h * R.U24 * (np.abs(xh * gamma) + np.abs(beta))).any(1).mean())
    own = float(b["amb"].any(1).mean())
    print(f"h {h} m {m}: gate-ambiguous rows, crude {100 * crude:.3f} %, the reference's own {100 * own:.3f} %")
    assert own <= crude <= 0.03


# ---------------------------------------------------------------------------------------------------
# The exact cases are exact
# ---------------------------------------------------------------------------------------------------
def test_exact_cases_are_exact_in_any_order():
    for n1, n2 in R.WGRAD_SHAPES:
        m = R.WGRAD_WRAP if (n1, n2) == (196, 196) else max(R.WGRAD_MS)
        a, b = R.small_ints((m, n1), 1), R.small_ints((m, n2), 2)
        assert np.abs(a).max() == 2 and np.abs(b).max() == 2 and np.array_equal(R.bfv(a), a)
        assert 4 * m < 2 ** 24
        if m <= 1025:
            assert R.exact_in_any_order(a[:, :, None] * b[:, None, :4], 1.0)
    for n, k in [(n, k) for n in R.MLP_FWD_NS for k in R.MLP_FWD_KS + (n,)] + sum(R.MLP_FWD_PATHS.values(), []):
        w = R.signed_perm(n, k)
        assert (np.abs(w).sum(1) == 1).all() and set(np.unique(w)) <= {-1.0, 0.0, 1.0}
        x = R.bfv(np.random.default_rng(n).normal(size=(3, k)))
        G, _ = R.linear(x, w)
        assert np.array_equal(R.bfv(G), G)      # one nonzero term per sum: G is a signed copy of bf16 values
    for h in R.DGRAD_HS:
        w = R.signed_perm(h, h)
        assert (np.abs(w).sum(0) == 1).all()    # a permutation both ways: P = dG W is a signed permuted copy
    # dbeta at the wrapping row counts: integer dy in [-2, 2] times k in {0, 1, 2}
    for m in (R.LN_BWD_WRAP_196, R.LN_BWD_WRAP_GENERIC):
        assert R.exact_in_any_order(2.0 * np.abs(R.small_ints((m, 8), 3)), 1.0)
    # colsum: integers below 2^24 / nb
    for nb in R.COLSUM_NBS:
        assert R.exact_in_any_order(R.small_ints((nb, 4), 4, -1000, 1000), 1.0)


def test_wgrad_shapes_reach_every_plan():
    """(bi, wi, ny) over all n1, n2 <= 224 by enumeration of wg_plan: the shapes of the GPU file reach each."""
    plans = {R.wg_plan(512, n1, n2)[:3] for n1 in range(4, 225, 4) for n2 in range(4, 225, 4)}
    hit = {R.wg_plan(512, n1, n2)[:3] for n1, n2 in R.WGRAD_SHAPES}
    print("wg_plan (bi, wi, ny):", sorted(plans))
    assert len(plans) == 10 and hit == plans
    # the wrap: 228 blocks of 576 rows, the last with 385 = 12 k-blocks of 32 rows and one ragged row (an odd count)
    assert R.wg_plan(R.WGRAD_WRAP, 196, 196)[3:] == (228, 576) and R.WGRAD_WRAP - 227 * 576 == 385


def test_mlp_fwd_shapes_reach_every_instance():
    nts = {(-(-n // 16)) for n in R.MLP_FWD_NS}
    inst = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8, 9: 10, 10: 10, 11: 12, 12: 12, 13: 13}
    assert {inst.get(t, 16) for t in nts} == {1, 2, 3, 4, 6, 8, 10, 12, 13, 16}
    for lo, hi in zip(R.MLP_FWD_NS[1::2], R.MLP_FWD_NS[2::2]):
        assert hi == lo + 4     # both ends of each instance's range
