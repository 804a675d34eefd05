"""The fp64 reference of the URM block kernels (tests/urm_block_reference.py) is right before any kernel is
compared with it: with its rounding points switched off it equals float64 autograd of the attention core,
the module's SwiGLU-conv composite and agent.rms_norm(h + a); with them on it stays within the propagated
bf16 steps; the numpy Philox equals the oracle's; thr / scale take the values attn_drop_args forms; the
intrinsic budgets are measured here (printed: run with -s) and held against the module's constants both
ways; the flip term stays rare in every Gaussian case; and every constructed case reaches the branch it is
named for.  CPU only."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import urm_block_reference as R

# (h, heads) of every attention family of tests/test_gpu_urm_block_edges.py
ATTN_SHAPES = sorted({(h, heads) for fam in R.ATTN_FAMILIES.values() for h, heads, _, _ in fam})
DROP_PS = (2.0 ** -16, 0.1, 0.5, 0.9, 1 - 2.0 ** -16, 1 - 2.0 ** -18, 1e-6)
SEED = R.MASK_SEED


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


@pytest.mark.parametrize("h,heads", [(64, 4), (196, 4), (20, 5), (4, 4)])
def test_attention_reference_without_rounding_is_float64_autograd(h, heads):
    n = 3
    qkv, dout = R.attn_case("gauss", n, h, heads, 1)
    q, k, v = R.split_heads(qkv, heads)
    km = R.keep_mask(n, heads, 0.3, SEED, 5)
    dO = R.split_heads(np.concatenate([dout] * 3, 1), heads)[0]
    tq, tk, tv = (_t(x).requires_grad_(True) for x in (q, k, v))
    o = (torch.softmax(tq @ tk.transpose(-1, -2) / (h // heads) ** 0.5, -1) * _t(km)) @ tv
    (o * _t(dO)).sum().backward()
    f = R.attn_fwd(q, k, v, km, rounding=False)
    np.testing.assert_allclose(f["O"], o.detach().numpy(), rtol=1e-12, atol=1e-14)
    if h // heads == 16:
        b = R.attn_bwd(q, k, v, dO, km, rounding=False)
        for name, t in (("dQ", tq), ("dK", tk), ("dV", tv)):
            np.testing.assert_allclose(b[name], t.grad.numpy(), rtol=1e-12, atol=1e-13, err_msg=name)
    # rounding on: every Pd is within half a bf16 step of P km; P itself moves only by the fp32 form of 1/sqrt(d)
    # (relative 2^-24 of every score, so at most 2 2^-24 max|s| of P; nothing at head_dim 16, where 1/4 is exact)
    r = R.attn_fwd(q, k, v, km)
    smax = np.abs(q @ np.swapaxes(k, -1, -2)).max(-1, keepdims=True) / (h // heads) ** 0.5
    dP = np.abs(f["P"] * km) * (2 * R.U24 * smax if (h // heads) != 16 else 0.0)
    half = lambda x: 0.5 * R.bf16_ulp(x) * (1 + 1e-9)  # noqa: E731
    assert (np.abs(r["O"] - f["O"]) <= (half(r["Pd"]) + dP * (1 + 2.0 ** -8)) @ np.abs(v) + 1e-300).all()
    if h // heads == 16:   # backward: dS and Pd each within half a step, through to dQ / dK / dV
        T = lambda x: np.swapaxes(x, -1, -2)  # noqa: E731
        br = R.attn_bwd(q, k, v, dO, km)
        assert np.array_equal(br["P"], b["P"])
        assert (np.abs(br["dS"] - b["dS"]) <= half(br["dS"])).all() and (np.abs(br["Pd"] - b["Pd"]) <= half(br["Pd"])).all()
        assert (np.abs(br["dQ"] - b["dQ"]) <= 0.25 * (half(br["dS"]) @ np.abs(k)) + 1e-300).all()
        assert (np.abs(br["dK"] - b["dK"]) <= 0.25 * (T(half(br["dS"])) @ np.abs(q)) + 1e-300).all()
        assert (np.abs(br["dV"] - b["dV"]) <= T(half(br["Pd"])) @ np.abs(dO) + 1e-300).all()


def test_swiglu_reference_without_rounding_is_float64_autograd():
    """Against agent.GameConvSwiGLU itself in float64: its Conv1d (kernel 2, padding 1, trimmed to 16 tokens) on
    silu(gate) up, which proves the tap order (w[:, 0] on the previous token, w[:, 1] on the current one), and
    its whole forward / backward (gate_up_proj, the module's own kernel-2 expression, down_proj)."""
    import agent
    nb, inter = 5, 16
    gu, w, b, dact = R.swiglu_case("gauss", nb, inter, 2)
    g, u = R.split_gu(gu, inter)
    mod = agent.GameConvSwiGLU(24, 0.75, 2).double()
    assert mod.inter == inter
    with torch.no_grad():
        mod.dwconv.weight.copy_(_t(w).view(inter, 1, 2))
        mod.dwconv.bias.copy_(_t(b))
    tg, tu = (_t(x).requires_grad_(True) for x in (g, u))
    tw, tb = mod.dwconv.weight, mod.dwconv.bias
    y = F.silu(tg) * tu
    act = F.silu(mod.dwconv(y.transpose(1, 2))[..., :16].transpose(1, 2))
    (act * _t(dact.reshape(nb, 16, inter))).sum().backward()
    r = R.swiglu_conv(g, u, w, b, dact.reshape(nb, 16, inter), rounding=False)
    # the whole module: gu = x W_gu^T, out = act W_d^T; dact = dout W_d, dx = dgu W_gu
    gen = np.random.default_rng(9)
    x, dout = gen.normal(size=(nb, 16, 24)), gen.normal(size=(nb, 16, 24))
    wgu, wd = mod.gate_up_proj.weight.detach().numpy(), mod.down_proj.weight.detach().numpy()
    gm, um = np.split(x @ wgu.T, 2, -1)
    rm = R.swiglu_conv(gm, um, w, b, dout @ wd, rounding=False)
    saved = (tw.grad.clone(), tb.grad.clone())
    mod.zero_grad()
    tx = _t(x).requires_grad_(True)
    out = mod(tx)
    (out * _t(dout)).sum().backward()
    np.testing.assert_allclose(rm["act"] @ wd.T, out.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(np.concatenate([rm["dgate"], rm["dup"]], -1) @ wgu, tx.grad.numpy(), rtol=1e-12, atol=1e-13)
    pm, _ = R.partial_rows(rm["terms"], 1)
    dwm, dbm, _, _ = R.colsum(pm)
    np.testing.assert_allclose(dwm, tw.grad.view(inter, 2).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dbm, tb.grad.numpy(), rtol=1e-12, atol=1e-13)
    tw.grad, tb.grad = saved[0], saved[1]
    np.testing.assert_allclose(r["act"], act.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["dgate"], tg.grad.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["dup"], tu.grad.numpy(), rtol=1e-12, atol=1e-14)
    part, _ = R.partial_rows(r["terms"], 2)   # rows 0, 1 take boards 0 2 4 and 1 3
    dw, db, _, _ = R.colsum(part)
    np.testing.assert_allclose(dw, tw.grad.view(inter, 2).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-12, atol=1e-13)
    one = R.partial_rows({k: (v[0][[0, 2, 4]], v[1][[0, 2, 4]]) for k, v in r["terms"].items()}, 1)[0]
    np.testing.assert_allclose(part[0], one[0], rtol=1e-13)
    # rounding on: y within one step of silu's rounding times |u| plus its own, act within silu' <= 1.1 of that
    q = R.swiglu_conv(g, u, w, b)
    step_y = 0.5 * R.bf16_ulp(q["sl"]) * np.abs(u) + 0.5 * R.bf16_ulp(q["y"])
    assert (np.abs(q["y"] - r["y"]) <= step_y).all()
    prev_step = np.concatenate([np.zeros_like(step_y[:, :1]), step_y[:, :-1]], 1)
    assert (np.abs(q["act"] - r["act"]) <= 1.1 * (np.abs(w[:, 0]) * prev_step + np.abs(w[:, 1]) * step_y) + 1e-12).all()


def test_rms_reference_is_float64_autograd_of_rms_norm():
    import agent
    h, a, _ = R.rms_case(37, True, 3)
    th, ta = _t(h).requires_grad_(True), _t(a).requires_grad_(True)
    eps = float(np.float32(R.RMS_EPS))
    # agent.rms_norm computes in float32 whatever its input (x.to(torch.float32)), so float64 autograd runs through
    # its expression written out in float64, and the module function is held to that at fp32 precision
    ts = th + ta
    out = ts * torch.rsqrt(ts.pow(2).mean(-1, keepdim=True) + eps)
    with torch.no_grad():
        mod = agent.rms_norm((th + ta).float(), eps).double()
    assert float((mod - out).abs().max()) <= 4 * 2.0 ** -24 * float(out.abs().max())
    g = np.random.default_rng(0)
    dout, doutb = g.normal(size=h.shape), R._bfv(g.normal(size=h.shape))
    (out * _t(dout + doutb)).sum().backward()
    r = R.rms_res_fwd(h, a, R.RMS_EPS)
    np.testing.assert_allclose(r["out"], out.detach().numpy(), rtol=1e-12, atol=1e-300)
    ds, _ = R.rms_res_bwd(r["out"], r["r"], dout=dout, doutb=doutb)
    np.testing.assert_allclose(ds, th.grad.numpy(), rtol=1e-12, atol=0)   # every row class, the 1e18 rows' 1e-17 too
    assert np.array_equal(th.grad.numpy(), ta.grad.numpy())
    # the mean-pool broadcast: row r takes dpool[r >> 4]
    rows = 48
    h, a, _ = R.rms_case(rows, False, 4)
    r = R.rms_res_fwd(h, a, R.RMS_EPS)
    dpool = g.normal(size=(3, 64))
    ds, _ = R.rms_res_bwd(r["out"], r["r"], dpool=dpool)
    want, _ = R.rms_res_bwd(r["out"], r["r"], dout=np.repeat(dpool, 16, 0))
    assert np.array_equal(ds, want)


def test_numpy_philox_is_the_oracles():
    from oracle import oracle
    g = np.random.default_rng(7)
    ctr = g.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    ctr[:50, 3] = 0
    ctr[50:60] = [[0, 0, 0, 0]] * 5 + [[2 ** 32 - 1] * 4] * 5
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], np.uint64)
    assert key[1] != 0 and (ctr[:, 3] != 0).sum() > 200
    got = R.philox4x32_10(ctr, key)
    for c, r in zip(ctr, got):
        assert np.array_equal(r, oracle.philox4x32_10(c.astype(np.uint32), key.astype(np.uint32)))
    got0 = R.philox4x32_10(ctr[:20], np.array([5, 0]))
    for c, r in zip(ctr[:20], got0):
        assert np.array_equal(r, oracle.philox4x32_10(c.astype(np.uint32), [5, 0]))


def test_keep_mask_counter_layout_and_carry():
    """One element recomputed by hand from the oracle; counter + offset carries into the high word."""
    from oracle import oracle
    n, heads, p = 2, 32, 0.5
    for counter, offset in ((0, 0), (2 ** 32 - 1, 3), (2 ** 33 + 5, 0), (2 ** 64 - 1, 2)):
        km = R.keep_mask(n, heads, p, SEED, counter, offset)
        c = (counter + offset) % 2 ** 64
        for b, hh, i, j in ((0, 0, 0, 0), (1, 31, 15, 15), (1, 7, 9, 6)):
            r = oracle.philox4x32_10([b, (hh << 8) | (i << 2) | (j >> 2), c & 0xFFFFFFFF, c >> 32],
                                     [SEED & 0xFFFFFFFF, SEED >> 32])
            word = int(r[(j & 3) >> 1])
            u = (word >> 16) if j & 1 else (word & 0xFFFF)
            assert km[b, hh, i, j] == (2.0 if u >= 32768 else 0.0)
    assert not np.array_equal(R.keep_mask(n, heads, p, SEED, 2 ** 32 - 1, 3), R.keep_mask(n, heads, p, SEED, 2, 0))


def test_threshold_and_scale_at_the_probability_edges():
    want = {2.0 ** -16: (1, None), 0.1: (6554, None), 0.5: (32768, 2.0), 0.9: (58982, None),
            1 - 2.0 ** -16: (65535, 65536.0), 1 - 2.0 ** -18: (65536, 2.0 ** 18), 1e-6: (0, None)}
    assert set(want) == set(DROP_PS)
    for p, (thr, scale) in want.items():
        t, s = R.drop_args(p)
        assert t == thr, (p, t)
        assert s == float(np.float32(1) / (np.float32(1) - np.float32(p)))
        if scale is not None:
            assert s == scale
    assert R.drop_args(2.0 ** -17)[0] == 0 and R.drop_args(np.nextafter(np.float32(2.0 ** -17), np.float32(1)))[0] == 1
    assert R.drop_args(np.nextafter(np.float32(1 - 2.0 ** -17), np.float32(0)))[0] == 65535
    assert R.drop_args(1 - 2.0 ** -17)[0] == 65536
    # thr 0: all ones, no scale; thr 65536: everything dropped; p 0.9: some row of some head fully dropped
    assert (R.keep_mask(2, 4, 1e-6, SEED, 9) == 1.0).all()
    assert (R.keep_mask(2, 4, 1 - 2.0 ** -18, SEED, 9) == 0.0).all()
    km = R.keep_mask(5, 4, 0.9, SEED, 0)
    assert (km.max(-1) == 0).any() and (km > 0).any()
    lo = R.keep_mask(64, 4, 2.0 ** -16, SEED, 0)
    assert 0 < (lo == 0).sum() < 10 and lo.max() == R.drop_args(2.0 ** -16)[1]
    hi = R.keep_mask(64, 4, 1 - 2.0 ** -16, SEED, 0)
    assert 0 < (hi > 0).sum() < 10 and hi.max() == 65536.0


def _measure_P():
    worst = 0.0
    for h, heads in ATTN_SHAPES:
        for kind in R.ATTN_KINDS:
            qkv, _ = R.attn_case(kind, 5, h, heads, 11)
            q, k, _ = R.split_heads(qkv, heads)
            P, errP = R.attn_probs(q, k)
            P32, _ = R.attn_probs(q, k, dtype=np.float32)
            scale = (errP - R.FLOOR) / R.budget("P") * R.U23
            err = np.abs(P32.astype(np.float64) - P)
            worst = max(worst, float((np.maximum(err - 2.0 ** -126, 0) / np.maximum(scale, 1e-300)).max()))
    # the wide-score regime of the issue's probe (|s| up to ~200)
    g = np.random.default_rng(3)
    q, k = (R._bfv(g.normal(size=(64, 4, 16, 16)) * 5.0) for _ in range(2))
    P, errP = R.attn_probs(q, k)
    P32, _ = R.attn_probs(q, k, dtype=np.float32)
    err = np.abs(P32.astype(np.float64) - P)
    scale = (errP - R.FLOOR) / R.budget("P") * R.U23
    return max(worst, float((np.maximum(err - 2.0 ** -126, 0) / np.maximum(scale, 1e-300)).max()))


def _measure_sig():
    x = np.concatenate([R._bfv(np.random.default_rng(4).normal(size=200000) * 1.5), R._bfv(np.linspace(-87, 87, 40001)),
                        np.array(R.GATE_EDGES)])
    sg, rel = R.sigm(x)
    s32, _ = R.sigm(x, np.float32)
    err = np.maximum(np.abs(s32.astype(np.float64) - sg) - 2.0 ** -126, 0)
    return float((err / np.maximum(sg * rel / R.budget("sig") * R.U23, 1e-300)).max())


def _measure_rsqrt():
    worst = 0.0
    for abf in (True, False):
        h, a, _ = R.rms_case(4096, abf, 5)
        r = R.rms_res_fwd(h, a, R.RMS_EPS)
        _, r32 = R.rms_res_fwd(h, a, R.RMS_EPS, np.float32)
        worst = max(worst, float((np.abs(r32.astype(np.float64) - r["r"]) / r["r"]).max() / R.U23))
    return worst


def test_measured_intrinsic_budgets():
    """max |fp32 emulation - fp64| in units of 2^-23 of each quantity's scale: no larger than the module's
    constants and no more than their headroom below them (the constants ARE the measurements)."""
    units = {"P": _measure_P(), "sig": _measure_sig(), "rsqrt": _measure_rsqrt()}
    print("measured units of 2^-23:", {q: round(u, 3) for q, u in units.items()}, "constants:", R.UNITS,
          "device factor (assumed):", R.DEVICE_FACTOR)
    for q, u in units.items():
        assert u <= R.UNITS[q], (q, u)
        assert R.UNITS[q] <= (1.0 + R.UNITS_HEADROOM) * u + 0.01, (q, u)
    assert R.DEVICE_FACTOR == 4.0 and R.FLOOR == 2.0 ** -120


ATTN_TESTS = ([("board", hd) for hd in (1, 2, 3, 4)] + [("head", i) for i in range(len(R.ATTN_FAMILIES["head"]))]
              + [("generic", i) for i in range(len(R.ATTN_FAMILIES["generic"]))])


@pytest.mark.parametrize("family,which", ATTN_TESTS)
def test_flip_term_is_rare_in_the_gaussian_attention_cases(family, which):
    """Exactly the Gaussian runs of each attention test of tests/test_gpu_urm_block_edges.py (R.ATTN_FAMILIES x
    R.attn_gauss_runs), pooled per test: one run of one board and one head has 256 outputs, where a single
    ambiguous P row is already 6.25 %, so a run alone cannot resolve 5 %."""
    shapes = R.ATTN_FAMILIES[family]
    shapes = [x for x in shapes if x[1] == which] if family == "board" else [shapes[which]]
    cnt = {}

    def add(name, flagged, size):
        c = cnt.setdefault(name, [0, 0])
        c[0] += flagged
        c[1] += size
    for h, heads, n, bwd in shapes:
        for seed, dk, p, counter, offset in R.attn_gauss_runs(bwd):
            qkv, dout = R.attn_case("gauss", n, h, heads, seed, dk)
            q, k, v = R.split_heads(qkv, heads)
            km = None if R.drop_args(p)[0] == 0 else R.keep_mask(n, heads, p, R.MASK_SEED, counter, offset)
            f = R.attn_fwd(q, k, v, km)
            add("O", R.flip_count(f["O_flip"], f["O_arith"]), f["O"].size)
            if bwd:
                b = R.attn_bwd(q, k, v, R.split_heads(np.concatenate([dout] * 3, 1), heads)[0], km)
                for x in ("dQ", "dK", "dV"):
                    add(x, R.flip_count(b[x + "_flip"], b[x + "_arith"]), b[x].size)
                add("dS", int((b["devS"] > 1024 * R.FLOOR).sum()), b["dS"].size)
    share = {x: c[0] / c[1] for x, c in cnt.items()}
    print(family, which, {x: round(v, 4) for x, v in share.items()})
    for x in ("dQ", "dK"):   # 16 dS roundings feed each output: see FLIP_SHARE_DS_FANIN
        if x in share:
            assert share.pop(x) <= min(16 * share["dS"], R.FLIP_SHARE_DS_FANIN), (x, cnt)
    assert max(share.values()) <= R.FLIP_SHARE, share


SWIGLU_TESTS = [("shapes", i) for i in R.SWIGLU_INTERS] + [("wrap", i) for i in range(len(R.SWIGLU_WRAP_RUNS))] + [("colsum", 0)]


@pytest.mark.parametrize("group,which", SWIGLU_TESTS)
def test_flip_term_is_rare_in_the_gaussian_swiglu_cases(group, which):
    """Exactly the Gaussian runs of each SwiGLU-conv test of the GPU file, pooled per test (inter 1 at one board
    has 16 outputs); the column-sum runs, 8 channels wide down to one board, pooled over the eight nblk."""
    runs = (R.SWIGLU_SHAPE_RUNS[which] if group == "shapes" else [R.SWIGLU_WRAP_RUNS[which]] if group == "wrap"
            else R.SWIGLU_COLSUM_RUNS)
    cnt = {x: [0, 0] for x in ("act", "dgate", "dup")}
    for kind, nb, inter, seed in runs:
        gu, w, b, dact = R.swiglu_case(kind, nb, inter, seed)
        g, u = R.split_gu(gu, inter)
        r = R.swiglu_conv(g, u, w, b, dact.reshape(nb, 16, inter))
        for x in cnt:
            cnt[x][0] += R.flip_count(r[x + "_flip"], r[x + "_arith"])
            cnt[x][1] += r[x].size
    share = {x: c[0] / c[1] for x, c in cnt.items()}
    print(group, which, {x: round(v, 4) for x, v in share.items()})
    assert max(share.values()) <= R.FLIP_SHARE, (share, cnt)


def test_constructed_swiglu_allowances_stay_finite_and_small(monkeypatch):
    """Every value run (gate edges up to +-3e38, the 2^100 leak, y2 on silu''s zero): bf16(x +- a) is finite for
    every output, so an inf from the kernel fails; and with the floor set aside (it is absolute: 2^-120 of a
    flushed sigmoid times a 3e38 factor is not small) a is at most 16 bf16 steps of the output's own terms
    before cancellation (|y_{t-1} w0| + |y_t w1| + |b| for act, the two dy terms times the factor for dgate /
    dup; the largest, 7.8, is a flipped y through silu'' where silu' is small), 2^-6 of a step where none flips, and the partial rows' allowance at most
    2^-6 of their absolute sum (median 2^-13) -- a huge value is held as tightly, relatively, as a small one."""
    for floor in (R.FLOOR, 0.0):
        monkeypatch.setattr(R, "FLOOR", floor)
        for kind, nb, inter, seed in R.SWIGLU_VALUE_RUNS:
            gu, w, b, dact = R.swiglu_case(kind, nb, inter, seed)
            g, u = R.split_gu(gu, inter)
            r = R.swiglu_conv(g, u, w, b, dact.reshape(nb, 16, inter))
            val, allow = R.partial_rows(r["terms"], R.sc_rows(nb))
            assert np.isfinite(val).all() and np.isfinite(allow).all() and np.isfinite(val.astype(np.float32)).all()
            for x in ("act", "dgate", "dup"):
                a = r[x + "_arith"] + r[x + "_flip"]
                assert np.isfinite(r[x]).all() and np.isfinite(a).all(), (kind, x)
                assert np.isfinite(R._bf(r[x] - a)).all() and np.isfinite(R._bf(r[x] + a)).all(), (kind, inter, x)
                if floor == 0.0:
                    steps = a / R.bf16_ulp(np.maximum(np.abs(r[x]), r[x + "_scale"]))
                    assert steps.max() <= 16.0, (kind, inter, x, float(steps.max()))
                    tight = r[x + "_flip"] == 0
                    assert tight.mean() > 0.9 and (steps[tight] <= 2.0 ** -6).all(), (kind, inter, x, float(steps[tight].max()))
            if floor == 0.0:
                mag = R.partial_rows(r["term_scale"], R.sc_rows(nb))[0]   # |dact| (sg + |y2| sg (1 - sg)) |y|: uncancelled
                ratio = allow / (mag + 1e-300)   # one bf16 step of every y at the worst; fp32 sums where none flips
                assert ratio.max() <= 2.0 ** -6 and np.median(ratio) <= 2.0 ** -13, (kind, inter, float(ratio.max()))


def test_saturated_attention_cases_reach_their_branches():
    for h, heads in ((64, 4), (512, 32), (196, 4), (20, 5), (4, 4)):
        for kind, want in (("q0", 1 / 16), ("onehot", 1.0), ("twomax", 0.5)):
            qkv, _ = R.attn_case(kind, 3, h, heads, 0)
            q, k, v = R.split_heads(qkv, heads)
            P32, _ = R.attn_probs(q, k, dtype=np.float32)
            assert set(np.unique(P32)) == ({want, 0.0} if want != 1 / 16 else {want}), (h, kind)
            assert (np.sort(P32, -1)[..., -2:].sum(-1) == (1.0 if want != 1 / 16 else 0.125)).all()
            f = R.attn_fwd(q, k, v)
            assert np.array_equal(f["Pd"], P32.astype(np.float64))
            assert R.flip_share(f["O_flip"], f["O_arith"]) == 0.0
            if kind != "q0":
                s = (q @ np.swapaxes(k, -1, -2)) / np.sqrt(h // heads)
                assert 190 <= s.max() <= 210 and (s.max(-1) - np.sort(s, -1)[..., -3] >= 190).all()
                win = P32.argmax(-1)
                assert len(np.unique(win)) > 1    # not every row picks the same key
    qkv, _ = R.attn_case("vcancel", 3, 64, 4, 0)
    q, k, v = R.split_heads(qkv, 4)
    f = R.attn_fwd(q, k, v)
    assert np.abs(f["O"]).max() <= 0.2 * (np.abs(f["Pd"]) @ np.abs(v)).min()
    _, dz = R.attn_case("gauss", 2, 64, 4, 0, "zero")
    _, d1 = R.attn_case("gauss", 2, 64, 4, 0, "onehot")
    assert not dz.any() and (np.count_nonzero(d1, 1) == 4).all()


def test_mask_probe_reads_the_mask_back():
    n, p = 2, 0.5
    for h, heads in ((64, 4), (512, 32), (64, 1), (20, 5), (36, 3)):
        hd = h // heads
        km = R.keep_mask(n, heads, p, SEED, 1)
        parts = -(-16 // hd)
        seen = np.zeros_like(km)
        for part in range(parts):
            q, k, v = R.split_heads(R.mask_probe(n, h, heads, part), heads)
            f = R.attn_fwd(q, k, v, km)
            assert not f["devPd"].any() and not f["O_flip"].any()
            w = min(hd, 16 - part * hd)
            assert np.array_equal(f["O"][..., :w], 2.0 * km[..., part * hd:part * hd + w] / 16 * 16 / 2)
            seen[..., part * hd:part * hd + w] = f["O"][..., :w]
        assert np.array_equal(seen, km)


def test_swiglu_value_cases_reach_their_branches():
    nb, inter = 4, 8
    gu, w, b, dact = R.swiglu_case("edges", nb, inter, 0)
    g, u = R.split_gu(gu, inter)
    for e in R.GATE_EDGES:
        assert ((g == e) & (np.signbit(g) == np.signbit(e))).sum() >= 4, e
    r = R.swiglu_conv(g, u, w, b, dact.reshape(nb, 16, inter))
    part, allow = R.partial_rows(r["terms"], nb)
    for x in (r["y"], r["y2"], r["act"], r["dgate"], r["dup"], part, allow):
        assert np.isfinite(x).all()
    assert np.abs(r["y"]).max() > 1e37 and abs(R.dsilu(np.array(R.SILU_FLAT))[0]) < 2e-3
    # silu(-88.5) is below the floor whether or not the hardware flushes it; silu(+-2.99e38) is gate or -0
    sg, _ = R.sigm(np.array([-88.5, -100.0]))
    assert (np.abs(np.array([-88.5, -100.0]) * sg) < R.FLOOR).all()
    # flat: y2 sits exactly on the bf16 value next to silu''s zero at token 0 of every board
    gu, w, b, dact = R.swiglu_case("flat", nb, inter, 0)
    r = R.swiglu_conv(*R.split_gu(gu, inter), w, b, dact.reshape(nb, 16, inter))
    assert (r["y2"][:, 0] == R.SILU_FLAT).all() and np.abs(r["d2"][:, 0]).max() < 1e-2
    # leak: token 15's y is 2^100 with w0 = 1: token 0 of the next board would see it
    gu, w, b, dact = R.swiglu_case("leak", nb, inter, 0)
    r = R.swiglu_conv(*R.split_gu(gu, inter), w, b, dact.reshape(nb, 16, inter))
    assert (r["y"][:, 15] == 2.0 ** 100).all() and np.abs(r["y2"][:, 0]).max() < 100 and (w[:, 0] == 1).all()
    part, _ = R.partial_rows(r["terms"], nb)
    assert np.isfinite(part).all()
    for kind, col in (("w0zero", 0), ("w1zero", 1)):
        assert not R.swiglu_case(kind, nb, inter, 0)[1][:, col].any()


def test_rms_row_classes_reach_their_branches():
    h, a, cls = R.rms_case(17, True, 0)
    r = R.rms_res_fwd(h, a, R.RMS_EPS)
    eps = float(np.float32(R.RMS_EPS))
    assert set(cls) == {0, 1, 2, 3}
    assert not r["out"][cls == 1].any() and (r["r"][cls == 1] == eps ** -0.5).all()
    tiny = cls == 2
    assert (np.abs(r["r"][tiny] / eps ** -0.5 - 1) < 1e-30).all() and np.abs(r["out"][tiny]).max() < 1e-15  # eps decides
    assert r["out"][tiny].any()
    big = cls == 3
    assert (r["r"][big] < 1e-17).all() and (np.abs((r["out"][big] ** 2).mean(-1) - 1) < 1e-9).all()
    assert ((h + a)[big] ** 2).sum(-1).max() < 3e38   # the fp32 sum of squares stays finite
    assert R.rms_case(1, True, 0)[2].tolist() == [0]
