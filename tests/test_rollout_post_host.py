"""The float64 reference of the RTG scan, the episode scan, the rollout statistics and the sampler
(tests/rollout_post_reference.py) is right before any kernel is compared with it: against
oracle.reward_rtg_normalize and the five golden cases of calculate_advantage, against the trainer's old
torch expression restated in float64, against a per-step loop, against the golden sampler rows and
oracle.masked_policy; every case table holds the regimes it claims; the share of sampler rows too close
to a CDF boundary to compare actions on is capped; and the variance bound of the GPU test holds for a
numpy emulation of the kernels' order of addition (printed: run with -s).  CPU only."""

import math

import numpy as np
import pytest
import torch

import rollout_post_reference as R
from conftest import golden
from oracle import oracle as O


# ------------------------------------------------------------------------------ RTG --------------
def _flat(T, n, live):
    """Episode order of a [T, n] trajectory: env-major, time ascending, live steps only."""
    tt, ee = np.nonzero(live.T)[1], np.nonzero(live.T)[0]
    return tt, ee


@pytest.mark.parametrize("T,n,beta,state0", [(37, 23, 0.95, [3.0, 40.0, 3.0, 5.0]), (16, 5, 0.5, [0.0, 1.0, 0.0, 1.0]),
                                             (1, 7, 0.99, [-2.0, 9.0, -2.0, 0.0])])
def test_rtg_reference_matches_oracle(T, n, beta, state0):
    g = np.random.default_rng(T + n)
    points = (g.integers(0, 500, size=(T, n)) * 4).astype(np.int32)
    pot = g.integers(-128, 128, size=(T, n, 4)).astype(np.int8)
    flags = np.where(g.random((T, n)) < 0.1, R.FLAG_DONE, 0).astype(np.uint8)
    tail = g.integers(max(T // 2, 1), T + 1, size=n)
    for e in range(n):
        flags[tail[e]:, e] = R.FLAG_INACTIVE | R.FLAG_DONE
    value = g.standard_normal((T, n)).astype(np.float32)
    st = R.rtg_prepare(state0 + [0, 1, 0, 0], beta)
    r = R.rtg_scan(points, pot, flags, value, R.CFG, st)
    sel = _flat(T, n, r["live"])
    tt, ee = sel
    done = (flags[sel] & R.FLAG_DONE) != 0
    o = O.reward_rtg_normalize(points[sel], pot[sel][:, 0], pot[sel][:, 1], pot[sel][:, 2], pot[sel][:, 3], done,
                               value[sel], done | (tt == tail[ee] - 1), R.GAMMA, R.W_POINTS, R.W_MONO, R.W_EMPT,
                               beta, state0[1], state0[0], int(state0[3]), state0[2])
    assert np.array_equal(r["reward"][sel], o["reward"])
    assert np.array_equal(r["g_raw"][sel], o["g_raw"])
    np.testing.assert_allclose(r["g_norm"][sel], o["g_norm"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["adv"][sel], o["adv"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose([st[4], st[5]], [o["mu_c"], o["std"]], rtol=1e-15)
    np.testing.assert_allclose([r["mean"], r["var"]], o["batch"], rtol=1e-12)
    exact = R.rtg_finalize_exact(st, r["mean"], r["var"], r["cnt"], beta)
    np.testing.assert_allclose(exact[:3], o["moments"], rtol=1e-12)
    assert exact[3] == state0[3] + 1
    # the kernel's one-pass formula from the exact sums agrees with the two-pass values at this scale
    one = R.rtg_finalize(st, (r["s1"], r["s2"], r["cnt"]), beta)
    np.testing.assert_allclose(one[6:8], [r["mean"], r["var"]], rtol=1e-10)
    for k in ("reward", "g_raw", "g_norm", "adv"):
        assert (r[k][~r["live"]] == 0).all()


@pytest.mark.parametrize("case", range(5))
def test_rtg_reference_matches_golden_advantage(case):
    """The golden episodes as columns of one [T, 16] trajectory with inactive tails: reward bit-identical,
    the rest at rtol 1e-12."""
    a = golden("advantage.npz")
    gamma, wp, wm, we, beta, m2, mu, step = (float(x) for x in a["cases"][case])
    ep = a["episode"]
    ids = list(dict.fromkeys(ep.tolist()))
    lens = [int((ep == i).sum()) for i in ids]
    T, n = max(lens), len(ids)
    points, pot = np.zeros((T, n), np.int32), np.zeros((T, n, 4), np.int8)
    flags = np.full((T, n), R.FLAG_INACTIVE | R.FLAG_DONE, np.uint8)
    value = np.zeros((T, n), np.float32)
    v64 = np.zeros((T, n))
    where = np.zeros((len(ep), 2), np.int64)
    for e, i in enumerate(ids):
        idx = np.nonzero(ep == i)[0]
        t = np.arange(len(idx))
        where[idx, 0], where[idx, 1] = t, e
        points[t, e] = a["points"][idx]
        pot[t, e] = np.stack([a["mono_b"][idx], a["mono_a"][idx], a["empt_b"][idx], a["empt_a"][idx]], axis=1)
        flags[t, e] = np.where(a["done"][idx] != 0, R.FLAG_DONE, 0)
        v64[t, e] = a["value"][idx]
    st = R.rtg_prepare([mu, m2, mu, step, 0, 1, 0, 0], beta)
    r = R.rtg_scan(points, pot, flags, value, (gamma, wp, wm, we), st)
    sel = (where[:, 0], where[:, 1])
    assert np.array_equal(r["reward"][sel], a[f"c{case}_reward"])
    np.testing.assert_allclose(r["g_raw"][sel], a[f"c{case}_g_raw"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["g_norm"][sel], a[f"c{case}_g_norm"], rtol=1e-12, atol=0)
    # the golden values are float64, the scan's are float32 inputs: subtract them here (value = 0 above)
    np.testing.assert_allclose(r["adv"][sel] - v64[sel], a[f"c{case}_adv"], rtol=1e-12, atol=1e-12)
    s = R.rtg_finalize_exact(st, r["mean"], r["var"], r["cnt"], beta)
    np.testing.assert_allclose([s[0], s[1], s[2]], a[f"c{case}_moments"], rtol=1e-12)


def test_rtg_prepare_table_hits_every_branch():
    rows = R.prepare_table()
    terms = [R.rtg_prepare_terms(s + [0, 1, 0, 0], b) for s, b in rows]
    assert {s[3] for s, _ in rows} >= set(R.PREPARE_STEPS) and {b for _, b in rows} >= set(R.PREPARE_BETAS)
    assert sum(t["bc_clamped"] for t in terms) >= 2      # beta = 1 and beta = 1 - 1e-9 at a small step
    assert sum(t["var_clamped"] for t in terms) >= 1
    assert sum(not t["bc_clamped"] and not t["var_clamped"] for t in terms) >= 4
    assert sum(t["step_clamped"] for t in terms) >= len(R.PREPARE_BETAS)
    s, b = rows[-1]
    assert s[1] / (1 - b ** s[3]) < (s[0] / (1 - b ** s[3])) ** 2
    for t in terms:
        assert np.isfinite(t["state"]).all() and t["state"][5] >= math.sqrt(R.EPS)
    # no live step: finalize leaves every word alone
    st = terms[0]["state"]
    assert np.array_equal(R.rtg_finalize(st, (0.0, 0.0, 0.0), 0.9), st)
    one = R.rtg_finalize(st, (2.0, 4.0, 1.0), 0.9)
    assert one[7] == 0.0 and one[6] == st[4] + 2.0 and one[3] == st[3] + 1


def test_rtg_case_tables_hold_their_regimes():
    assert {T for T, _ in R.RTG_SHAPES} == {1, 15, 16, 17, 33} and {n for _, n in R.RTG_SHAPES} == {1, 255, 256, 257, 513}
    assert R.KBLOCK == 256 and R.RTG_UNROLL == 16
    total = {}
    for T, n in R.RTG_SHAPES:
        c = R.rtg_case(T, n)
        fr, pr = R.flag_regimes(c), R.pot_regimes(c)
        assert pr["pairwise_different"] and pr["min128"] >= 1 and pr["minus1"] >= 1 and pr["max127"] >= 1
        assert int(c["points"].max()) <= 1 << 17
        if T >= 15 and n >= 255:
            assert fr["done"] >= 100 and fr["inactive_alone_mid"] >= 20 and fr["inactive_done"] >= 20
            assert fr["done_t0"] >= 1 and fr["done_tlast"] >= 1 and fr["inactive_columns"] >= 1
            assert fr["reset_bits"] >= 100 and fr["legal_bits"] >= 100 and pr["negative"] >= 1000
            assert int(c["points"].max()) > 1 << 16
            e = c["columns"]["inactive_mid"]
            f = c["flags"][:, e] & 0xC0
            assert f[T // 2] == R.FLAG_INACTIVE and (np.delete(f, T // 2) == 0).all()
        for k, v in fr.items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    c = R.rtg_case(17, 257, all_inactive=True)
    assert R.flag_regimes(c)["live"] == 0 and R.flag_regimes(c)["inactive_columns"] == 257


def test_variance_bound_holds_for_the_kernel_order_of_addition():
    """B = (T + log2 n + 4) 2^-53 s2 / cnt bounds the error of the kernel's one-pass variance
    s2/n - m1^2 around mu_c (and the same factor times mean|G - mu_c| the error of its mean) when the sums
    are taken in the kernels' order -- per env serial over t descending, then the trees -- in all four
    regimes.  The ratios err / B are printed."""
    for name, (c, cfg, mu_c) in R.moment_regimes().items():
        T, n = c["T"], c["n"]
        st = np.array([0.0, 1.0, 0.0, 1.0, mu_c, 1.0, 0.0, 0.0])
        r = R.rtg_scan(c["points"], c["pot"], c["flags"], c["value"], cfg, st)
        assert 0.9 * T * n < r["cnt"] < T * n
        s1, s2 = R.kernel_order_sums(r["g_raw"], r["live"], mu_c)
        cnt = float(r["cnt"])
        got = R.rtg_finalize(st, (s1, s2, cnt), 0.9)
        mean, var = r["mean"], r["var"]
        f = R.sum_bound(T, n)
        B, Bm = f * r["s2"] / cnt, f * r["abs1"] / cnt
        assert abs(s1 - r["s1"]) <= f * r["abs1"] and abs(s2 - r["s2"]) <= f * r["s2"]
        rv, rm = abs(got[7] - var) / B, abs(got[6] - mean) / Bm
        print(f"variance bound, {name}: var {var:.6e} kernel-order {got[7]:.6e} err/B {rv:.4f}; mean err/B {rm:.4f}; "
              f"relative variance error {abs(got[7] - var) / var:.3e}")
        assert rv <= 1.0 and rm <= 1.0, (name, rv, rm)


# ------------------------------------------------------------------------------ episode scan -----
@pytest.mark.parametrize("T,n", [(9, 257), (1, 5), (17, 64)])
def test_episode_walk_matches_per_step_loop(T, n):
    """The per-step loop of test_episode_scan_matches_loop in torch on the CPU, over two rollouts."""
    rs = torch.arange(n, dtype=torch.int64) * 3
    rm = torch.arange(n, dtype=torch.int32) % 7
    crs, crm = rs.numpy().copy(), rm.numpy().copy()
    for it in range(2):
        c = R.stats_case(T, n, False, seed=it)
        pts, boards = torch.from_numpy(c["points"]), torch.from_numpy(c["boards"])
        mt, fl = torch.from_numpy(c["max_tile"]), torch.from_numpy(c["flags"])
        sc, ti, crs, crm = R.episode_walk(c["points"], c["boards"], c["max_tile"], c["flags"], crs, crm)
        done = ((fl & 0x80) != 0) & ((fl & 0x40) == 0)
        for t in range(T):
            rs = rs + pts[t]
            rm = torch.maximum(rm, torch.maximum(boards[t].max(dim=1).values.to(torch.int32), mt[t].to(torch.int32)))
            d = done[t]
            assert torch.equal(torch.from_numpy(sc[t]), torch.where(d, rs, -1))
            assert torch.equal(torch.from_numpy(ti[t]), torch.where(d, rm, -1))
            rs, rm = torch.where(d, 0, rs), torch.where(d, 0, rm)
        assert np.array_equal(crs, rs.numpy()) and np.array_equal(crm, rm.numpy())
    # the byte maximum is unsigned: 0x80 as a board byte is 128, not -128
    b = np.zeros((1, 1, 16), np.int8)
    b[0, 0, 3], b[0, 0, 5] = -128, 17
    _, ti, _, rm1 = R.episode_walk(np.zeros((1, 1), np.int32), b, np.zeros((1, 1), np.int8),
                                   np.full((1, 1), R.FLAG_DONE, np.uint8), np.zeros(1, np.int64), np.zeros(1, np.int32))
    assert ti[0, 0] == 128 and rm1[0] == 0


# ------------------------------------------------------------------------------ rollout stats ----
def _stats_torch64(c, scores_tiles, cfg):
    """test_gpu_train._rollout_stats_torch restated in torch float64 on the CPU; the fixed-horizon scores
    come from episode_walk.  The metric's reward stays the float32 expression (it IS float32 in the trainer)."""
    gamma, wp, wm, we = cfg
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items() if isinstance(v, np.ndarray)}
    pts, pot, sf = t["points"], t["pot"], t["flags"]
    T, n = pts.shape
    done = ((sf & 0x80) != 0).float()
    p = pot.float()
    r = (pts.float() * wp + wm * (gamma * p[..., 1] * (1 - done) - p[..., 0])
         + we * (gamma * p[..., 3] * (1 - done) - p[..., 2]))
    assert r.dtype == torch.float32
    fields = [r.double(), t["adv"].double(), t["g_norm"].double(), t["g_raw"].double(), t["value"].double()]
    if c["episodic"]:
        valid = torch.nonzero(((sf & 0x40) == 0).reshape(-1)).squeeze(1)
        fields = [f.reshape(-1).index_select(0, valid) for f in fields]
    else:
        fields = [f.reshape(-1) for f in fields]
    r, a, gn, gr, v = fields
    starts = torch.zeros_like(sf, dtype=torch.bool)
    if c["episodic"]:
        starts[0] = True
    else:
        starts[1:] = (sf[:-1] & 0x20) != 0
    g0 = (t["g_raw"].double() * starts).sum() / starts.sum().clamp(min=1)
    if c["episodic"]:
        scores = torch.where((sf & 0x40) == 0, pts, 0).sum(0)
        tiles = t["boards"][T].max(dim=1).values.to(torch.int32)
        fin = torch.ones_like(scores, dtype=torch.bool)
    else:
        scores, tiles = (torch.from_numpy(x) for x in scores_tiles)
        fin = scores >= 0
    s_flat = torch.where(fin, scores, -1).reshape(-1).to(torch.int32)
    cnt = fin.sum()
    cntf = cnt.double().clamp(min=1.0)
    srt = torch.sort(s_flat).values
    med_idx = (s_flat.numel() - cnt + (cnt - 1).clamp(min=0) // 2).clamp(max=s_flat.numel() - 1)
    return torch.stack([
        torch.tensor(float(r.numel()), dtype=torch.float64), r.mean(), r.var(unbiased=False),
        (r == 0).double().mean() * 100, a.mean(), a.var(unbiased=False), a.pow(2).sum().sqrt(), a.min(), a.max(),
        gn.mean(), gn.std(unbiased=False), gn.min(), gn.max(), gr.std(unbiased=False), v.std(unbiased=False), g0,
        torch.where(fin, scores, 0).sum().double() / cntf, srt[med_idx].double(), s_flat.max().double(),
        (fin & (tiles >= 9)).sum().double() / cntf * 100, (fin & (tiles >= 10)).sum().double() / cntf * 100,
        (fin & (tiles >= 11)).sum().double() / cntf * 100, cnt.double()]).numpy()


@pytest.mark.parametrize("episodic", [False, True])
@pytest.mark.parametrize("T,n", [(9, 257), (17, 64), (1, 513), (8, 1)])
def test_rollout_stats_reference_matches_torch_float64(episodic, T, n):
    cfg = (0.99, 0.1, 1.0, 0.5)
    rs, rm = np.arange(n, dtype=np.int64) * 11, (np.arange(n) % 9).astype(np.int32)
    for it in range(2):
        c = R.stats_case(T, n, episodic, seed=it)
        st = None
        if not episodic:
            sc, ti, rs2, rm2 = R.episode_walk(c["points"], c["boards"], c["max_tile"], c["flags"], rs, rm)
            st = (sc, ti)
        out, aux = R.rollout_stats(c["points"], c["pot"], c["flags"], c["value"], c["g_raw"], c["g_norm"], c["adv"],
                                   c["boards"], c["max_tile"], episodic, cfg, rs, rm)
        want = _stats_torch64(c, st, cfg)
        assert len(out) == 23 == len(R.STAT_NAMES)
        np.testing.assert_allclose(out, want, rtol=1e-12, atol=0, err_msg=str(list(zip(R.STAT_NAMES, out, want))))
        if not episodic:
            assert np.array_equal(aux["run_score"], rs2) and np.array_equal(aux["run_max"], rm2)
            rs, rm = rs2, rm2


def test_metric_reward_is_float32_step_by_step():
    """Each operation of the chain rounds to float32: on a row where float64 evaluation followed by one
    rounding differs, the reference keeps the step-by-step value."""
    c = R.stats_case(17, 513, False)
    r32 = R.metric_reward_f32(c["points"], c["pot"], c["flags"], R.CFG)
    p = c["pot"].astype(np.float64)
    nd = ((c["flags"] & R.FLAG_DONE) == 0).astype(np.float64)
    g, wp, wm, we = (float(np.float32(x)) for x in R.CFG)
    r64 = c["points"] * wp + wm * (g * p[..., 1] * nd - p[..., 0]) + we * (g * p[..., 3] * nd - p[..., 2])
    assert r32.dtype == np.float32
    assert (r32 != r64.astype(np.float32)).sum() > 100
    assert np.abs(r32 - r64).max() <= 8 * 2.0 ** -24 * np.abs(r64).max()


def test_stats_case_tables_hold_their_regimes():
    assert {T for T, _ in R.STATS_SHAPES} == set(R.STATS_T) and {n for _, n in R.STATS_SHAPES} == set(R.STATS_N)
    assert R.STATS_CHUNK == 8 and R.WRAP_SHAPE[1] == 64 * 256 + 3 and -(-R.WRAP_SHAPE[1] // R.KBLOCK) > R.FINAL_STRIDE
    c = R.stats_case(17, 513, False)
    s = R.stats_regimes(c)
    assert s["done_inactive_with_points"] >= 20 and s["reset_last_step"] >= 100 and s["reset_before_last"] >= 100
    assert s["mt_above"] >= 100 and s["mt_below"] >= 100 and s["mt_equal"] >= 100 and s["tile17"] >= 100
    assert s["zero_in_float32_only"] >= 100      # at gamma 0.99 (the GPU test's): zero rewards a float64 chain misses
    c = R.stats_case(17, 513, True)
    s = R.stats_regimes(c)
    assert s["final_maxima"] == [8, 9, 10, 11, 12] and s["earlier_higher"] == 513 and s["inactive_with_points"] >= 100
    out, aux = R.rollout_stats(c["points"], c["pot"], c["flags"], c["value"], c["g_raw"], c["g_norm"], c["adv"],
                               c["boards"], None, True, R.CFG, None, None)
    # final maxima 8..12 in equal shares (n = 513: 103 / 103 / 103 / 102 / 102): the three thresholds differ
    assert out[19] > out[20] > out[21] > 0 and out[22] == 513
    assert out[0] < 17 * 513 and aux["starts"] == 513


def test_key_sets_hold_their_regimes():
    ks = R.key_sets()
    assert len(ks["none"]) == 0 and len(ks["one"]) == 1 and len(ks["two_different"]) == 2
    assert ks["two_different"][0] > ks["two_different"][1]
    assert (ks["all_zero"] == 0).all() and len(ks["all_zero"]) > 2
    assert len(set(ks["all_equal"].tolist())) == 1 and ks["all_equal"][0] > 0
    b = ks["three_digit_passes"]
    assert b.min() >= 1 << 22 and b.max() == (1 << 31) - 1 and int(b.max()).bit_length() > 22   # 11 + 11 + more bits
    for name, bit in (("bit0_only", 0), ("top_bit_only", 30)):
        v = ks[name]
        assert set((v ^ v[0]).tolist()) == {0, 1 << bit}
    d = ks["many_duplicates"]
    assert len(d) > 2048 and len(set(d.tolist())) <= 6
    for name, keys in ks.items():
        c = R.key_case(keys)
        assert c["n"] > len(keys) and int(c["points"].min()) >= 0
        out, aux = R.rollout_stats(c["points"], c["pot"], c["flags"], c["value"], c["g_raw"], c["g_norm"], c["adv"],
                                   c["boards"], c["max_tile"], False, R.CFG, c["run_score"], c["run_max"])
        assert sorted(aux["keys"].tolist()) == sorted(keys.tolist()), name
        want = np.sort(keys)[(len(keys) - 1) // 2] if len(keys) else -1
        assert out[17] == want and out[18] == (keys.max() if len(keys) else -1) and out[22] == len(keys)
    assert R.rollout_stats.__doc__ and out[17] >= 0


# ------------------------------------------------------------------------------ sampler ----------
def test_masked_sampler_matches_golden_and_oracle():
    """Against oracle.masked_policy (float64) at 1e-12, and against the golden rows.  tests/golden/sampler.npz
    stores probs and logp as float32 and an entropy computed from them, so the file itself is only good to
    float32: it is compared at 2^-22 relative plus 1e-6 (the bound test_oracle holds the oracle to), the
    float64 oracle at 1e-12."""
    g = golden("sampler.npz")
    n = len(g["logits"])
    legal = np.array([sum(1 << a for a in range(4) if not g["invalid"][i, a]) for i in range(n)], np.uint8)
    assert (legal != 0).all()
    r = R.masked_sampler(g["logits"], legal | 0xF0, np.full(n, 0.5))
    p, ent, logp = O.masked_policy(g["logits"], g["invalid"])
    fin = np.isfinite(logp)
    assert np.array_equal(np.isfinite(r["logp"]), fin) and (r["logp"][~fin] == -np.inf).all()
    np.testing.assert_allclose(r["logp"][fin], logp[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["entropy"], ent, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["p"], p, rtol=1e-12, atol=1e-12)
    gfin = np.isfinite(g["logp"])
    assert np.array_equal(gfin, fin)
    worst = {"logp": float(np.abs(r["logp"][fin] - g["logp"][fin]).max()),
             "entropy": float(np.abs(r["entropy"] - g["entropy"]).max()), "p": float(np.abs(r["p"] - g["probs"]).max())}
    print("fp64 sampler reference vs the float32 golden rows, worst absolute difference:", worst)
    np.testing.assert_allclose(r["logp"][fin], g["logp"][fin], rtol=2.0 ** -22, atol=1e-6)
    np.testing.assert_allclose(r["entropy"], g["entropy"], rtol=2.0 ** -22, atol=1e-6)
    np.testing.assert_allclose(r["p"], g["probs"], rtol=2.0 ** -22, atol=1e-7)
    cdf = np.cumsum(np.where(g["invalid"], 0.0, p), axis=1)
    u = np.linspace(0.001, 0.999, n)
    r = R.masked_sampler(g["logits"], legal, u)
    expect = np.array([int(np.argmax((u[i] < cdf[i]) & ~g["invalid"][i])) for i in range(n)])
    far = np.abs(cdf - u[:, None]).min(axis=1) > 1e-9
    assert np.array_equal(r["action"][far], expect[far]) and far.sum() > n - 5


def test_sampler_table_holds_its_regimes_and_edge_rows():
    t = R.sampler_table()
    n = len(t["legal"])
    assert n == 16 * len(R.LOGIT_PATTERNS) * R.SAMPLER_REPEATS
    for mask in range(16):
        for pi in range(len(R.LOGIT_PATTERNS)):
            assert ((t["legal"] == mask) & (t["pattern"] == pi)).sum() == R.SAMPLER_REPEATS
    bits = ((t["legal"][:, None] >> np.arange(4)) & 1).astype(bool)
    assert np.isfinite(t["logits"][bits]).all()              # NaN / inf only ever in illegal columns
    for name, test in (("nan_illegal", np.isnan), ("posinf_illegal", np.isposinf), ("neginf_illegal", np.isneginf)):
        rows = t["pattern"] == R.LOGIT_PATTERNS.index(name)
        assert test(t["logits"][rows][~bits[rows]]).all() and test(t["logits"][rows]).sum() >= 32 * R.SAMPLER_REPEATS
    assert np.abs(t["logits"][t["pattern"] == 1]).max() <= 10.0
    for name, gap in (("gap30", 30.0), ("gap100", 100.0), ("gap1e4", 1e4)):
        x = np.sort(t["logits"][t["pattern"] == R.LOGIT_PATTERNS.index(name)], axis=1)
        assert (np.diff(x, axis=1) > gap - 1.5).all()
    assert t["logits"][t["pattern"] == R.LOGIT_PATTERNS.index("offset+1e4")].min() > 9.9e3
    assert t["logits"][t["pattern"] == R.LOGIT_PATTERNS.index("offset-1e4")].max() < -9.9e3
    r = R.masked_sampler(t["logits"], t["legal"], np.full(n, 0.25))
    assert not np.isnan(r["logp"]).any() and not np.isnan(r["entropy"]).any() and not np.isnan(r["cdf"]).any()
    none = t["legal"] == 0
    assert (r["action"][none] == 0).all() and (r["entropy"][none] == 0).all() and np.isneginf(r["logp"][none]).all()
    single = bits.sum(axis=1) == 1
    assert single.sum() == 4 * len(R.LOGIT_PATTERNS) * R.SAMPLER_REPEATS
    assert (r["entropy"][single] == 0).all() and (r["logp"][single][bits[single]] == 0).all()
    assert np.array_equal(r["action"][single], np.argmax(bits[single], axis=1))
    r0 = R.masked_sampler(None, t["legal"], np.full(n, 0.25))
    k = bits.sum(axis=1)
    some = k > 0
    np.testing.assert_allclose(r0["entropy"][some], np.log(k[some]), rtol=1e-15, atol=1e-15)
    assert np.array_equal(r0["logp"][bits], -np.log(np.repeat(k, k)))
    assert (bits[np.arange(n), r["action"]] | none).all()


def test_sampler_near_boundary_rows_are_capped():
    """Rows whose uniform lies within 4 * 2^-24 of a CDF boundary that decides between two actions are left
    out of the GPU test's action comparison; with this table, seed, counter and env base they are at most
    1 % of it, for the table's logits and for logits = None, with and without the high flag bits."""
    t = R.sampler_table()
    n = len(t["legal"])
    u = R.uniforms(O.philox_draws(R.SAMPLER_SEED, R.SAMPLER_COUNTER, n, 1, env_base=R.SAMPLER_ENV_BASE)[:, 0])
    assert (u >= 0).all() and (u < 1).all() and len(set(u.tolist())) > n - 3
    for logits in (t["logits"], None):
        for hi in (0, 0xF0):
            r = R.masked_sampler(logits, t["legal"] | hi, u)
            near = r["dist"] < R.NEAR_BOUNDARY
            print(f"sampler rows within 4 * 2^-24 of a deciding CDF boundary: {int(near.sum())} of {n} "
                  f"({100.0 * near.mean():.3f} %), logits {'table' if logits is not None else 'None'}, high bits {hi:#x}")
            assert near.mean() <= 0.01
