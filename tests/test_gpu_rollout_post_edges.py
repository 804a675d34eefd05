"""The kernels between the rollout and the update -- rtg_prepare / rtg_kernel / rtg_reduce / rtg_finalize,
episode_scan_kernel, rollout_stats_kernel<kEpi> + rollout_stats_final_kernel and sample_kernel of
csrc/g2048.hip -- against the float64 numpy reference of tests/rollout_post_reference.py (proven on the CPU
by tests/test_rollout_post_host.py), at the shapes where they take another path: a partial last group of
the 16-step loads, a partial last block, one env, one step, more than 64 blocks; negative potentials in
every byte lane; every flag combination; every branch of the moment update; every digit pass of the radix
select; every legal mask and logits the softmax has to survive.

Expected values come from the numpy reference alone.  Bounds: what is the same fp64 (or integer) operation
sequence is compared bit for bit; a float32 store of a value whose fp64 source differs by 1-2 ulp (reciprocal
for division) may move by one float32 step; an fp64 sum of N terms taken in the kernel's order differs from
the exact sum by at most (depth + 4) 2^-53 sum|term| (reference.sum_bound); a float32 output of an fp64
statistic carries 2^-24 relative rounding, allowed as 2^-22 of the quantity's scale."""

import math

import numpy as np
import pytest
import torch

import rollout_post_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BETA = 0.95
STATE0 = [3.0, 40.0, 3.0, 5.0, 0.0, 1.0, 0.0, 0.0]
U22 = 2.0 ** -22
SENTINEL = 7.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    return torch.device("cuda:0")


def _ord(x):
    """float32 -> an integer that counts representable values in order (one step = one ulp)."""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(got, want64):
    return np.abs(_ord(got) - _ord(np.asarray(want64, np.float64).astype(np.float32)))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _cfg(cfg, beta):
    from g2048 import _lib as L
    return L.RewardCfg(*cfg, beta)


def _scan(dev, c, cfg, beta, state, with_reward=True, prepare=True, finalize=True, plain=False):
    """prepare -> scan -> finalize on the device.  Returns the outputs, the partials and the state after
    prepare and after finalize, as numpy."""
    from g2048 import _lib as L
    T, n = c["T"], c["n"]
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    st = torch.tensor(list(state), dtype=torch.float64, device=dev)
    rc = _cfg(cfg, beta)
    outs = [torch.full((T, n), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    rew = torch.full((T, n), SENTINEL, dtype=torch.float64, device=dev) if with_reward else None
    part = torch.full((3,), SENTINEL, dtype=torch.float64, device=dev)
    ws = torch.zeros(L.rtg_workspace_bytes(n), dtype=torch.uint8, device=dev)
    if prepare:
        L.rtg_prepare(st, rc)
    st1 = st.cpu().numpy().copy()
    ins = [td(c["points"]), td(c["pot"]), td(c["flags"]), td(c["value"])]
    if plain:   # g2048_reward_rtg itself (the Python wrapper always goes through g2048_reward_rtg_ex)
        import ctypes
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        L._call("g2048_reward_rtg", L._stream(st), *(ptr(x) for x in ins), T, n, ctypes.byref(rc), ptr(st),
                *(ptr(o) for o in outs), ptr(part), ptr(ws), ws.numel())
    else:
        L.reward_rtg(*ins, st, *outs, part, ws, rc, reward=rew)
    if finalize:
        L.rtg_finalize(st, part, rc)
    torch.cuda.synchronize()
    return {"g_raw": outs[0].cpu().numpy(), "g_norm": outs[1].cpu().numpy(), "adv": outs[2].cpu().numpy(),
            "reward": rew.cpu().numpy() if with_reward else None, "part": part.cpu().numpy(), "state1": st1,
            "state2": st.cpu().numpy()}


def _check_moments(got, r, st1, beta, T, n, label):
    """The partials and the finalized state against the reference's exact sums, mean and variance."""
    f = R.sum_bound(T, n)
    cnt = r["cnt"]
    assert got["part"][2] == cnt
    assert abs(got["part"][0] - r["s1"]) <= f * r["abs1"], (label, got["part"][0], r["s1"])
    assert abs(got["part"][1] - r["s2"]) <= f * r["s2"], (label, got["part"][1], r["s2"])
    B, Bm = f * r["s2"] / cnt, f * r["abs1"] / cnt
    s = got["state2"]
    em, ev = abs(s[6] - r["mean"]), abs(s[7] - r["var"])
    print(f"{label}: T {T} n {n} live {cnt}  batch mean err/bound {em / Bm:.4f}  batch var err/B {ev / B:.4f}  "
          f"(var {r['var']:.6e}, kernel {s[7]:.6e})")
    assert em <= Bm, (label, s[6], r["mean"], Bm)
    assert ev <= B, (label, s[7], r["var"], B)
    want = R.rtg_finalize_exact(st1, r["mean"], r["var"], cnt, beta)
    # the EMA passes (1 - beta) of the batch errors on and rounds its own four operations
    e_mu = (1 - beta) * Bm + 4 * R.U53 * abs(want[0])
    e_m2 = (1 - beta) * (B + 2 * abs(r["mean"]) * Bm + Bm * Bm) + 4 * R.U53 * abs(want[1])
    assert abs(s[0] - want[0]) <= e_mu and abs(s[2] - want[2]) <= e_mu and abs(s[1] - want[1]) <= e_m2, label
    assert s[2] == s[0] and s[3] == st1[3] + 1.0
    assert _bits_equal(s[4:6], st1[4:6])
    return ev / B, em / Bm


# ------------------------------------------------------------------------------ RTG scan ---------
@pytest.mark.parametrize("T,n", R.RTG_SHAPES)
def test_rtg_scan_tails_signs_and_flags(dev, T, n):
    c = R.rtg_case(T, n)
    got = _scan(dev, c, R.CFG, BETA, STATE0)
    assert got["state1"][4] != 0.0 and got["state1"][5] != 1.0     # non-trivial starting moments
    # the scan is compared with the reference scan from the DEVICE's mu_c / std (so its outputs can be held
    # bit for bit); those two against the reference's: pow to 2 ulp through 1 - beta^step, and for the std the
    # cancellation of m2_c - mu_c^2 (176.9 - 175.9 here), which multiplies a relative error of 1 / bc by
    # (m2_c + 2 mu_c^2) / (2 var)
    t = R.rtg_prepare_terms(STATE0, BETA)
    mu_c, std = t["state"][4], t["state"][5]
    rtol = 4 * 2.0 ** -52 * (1.0 + t["pow"] / t["bc"])
    amp = (STATE0[1] / t["bc"] + 2 * mu_c * mu_c) / (2 * std * std)
    assert not t["bc_clamped"] and not t["var_clamped"] and amp > 100
    assert abs(got["state1"][4] - mu_c) <= rtol * abs(mu_c)
    assert abs(got["state1"][5] - std) <= rtol * (amp + 1) * std
    r = R.rtg_scan(c["points"], c["pot"], c["flags"], c["value"], R.CFG, got["state1"])
    live = r["live"]
    assert _bits_equal(got["reward"], r["reward"]), "reward (fp64) differs from the reference"
    assert _bits_equal(got["g_raw"], r["g_raw"].astype(np.float32)), "g_raw != float32(reference)"
    for k in ("g_norm", "adv"):
        u = _ulps(got[k], r[k])
        assert u.max() <= 1, (k, int(u.max()), np.argwhere(u > 1)[:4])
    for k in ("reward", "g_raw", "g_norm", "adv"):   # inactive steps: exact (+0) zeros
        assert not got[k][~live].view(np.uint32 if got[k].dtype == np.float32 else np.uint64).any(), k
    for plain in (False, True):   # reward = nullptr through _ex, and g2048_reward_rtg itself
        again = _scan(dev, c, R.CFG, BETA, STATE0, with_reward=False, plain=plain)
        for k in ("g_raw", "g_norm", "adv"):
            assert _bits_equal(again[k], got[k]), f"{k}: the path without a reward output differs (plain {plain})"
        assert _bits_equal(again["part"], got["part"]) and _bits_equal(again["state2"], got["state2"])
    if r["cnt"] == 0:
        assert not got["part"].any() and _bits_equal(got["state2"], got["state1"])
    else:
        _check_moments(got, r, got["state1"], BETA, T, n, "rtg scan")


@pytest.mark.parametrize("name", ["centred", "offset_1e6", "tiny_spread_3e4", "mu_c_far"])
def test_rtg_batch_variance_within_bound(dev, name):
    """state[7] = s2/n - m1^2 around mu_c stays within B = (T + log2 n + 4) 2^-53 s2/cnt of the exact batch
    variance in the four regimes of the host test (prints err / B)."""
    c, cfg, mu_c = R.moment_regimes()[name]
    state = [0.5, 2.0, 0.5, 3.0, mu_c, 1.0, 0.0, 0.0]
    got = _scan(dev, c, cfg, 0.9, state, prepare=False)
    r = R.rtg_scan(c["points"], c["pot"], c["flags"], c["value"], cfg, state)
    assert _bits_equal(got["g_raw"], r["g_raw"].astype(np.float32)) and _bits_equal(got["reward"], r["reward"])
    _check_moments(got, r, np.array(state), 0.9, c["T"], c["n"], f"variance regime {name}")


def test_rtg_all_columns_inactive_leaves_the_state_alone(dev):
    c = R.rtg_case(17, 257, all_inactive=True)
    got = _scan(dev, c, R.CFG, BETA, STATE0)
    assert _bits_equal(got["part"], np.zeros(3)), got["part"]
    assert _bits_equal(got["state2"], got["state1"])
    assert _bits_equal(got["state2"][[0, 1, 2, 3, 6, 7]], np.array(STATE0)[[0, 1, 2, 3, 6, 7]])
    for k in ("reward", "g_raw", "g_norm", "adv"):
        assert not got[k].any(), k


@pytest.mark.parametrize("T,n", [(0, 5), (0, 300), (4, 0), (0, 0)])
def test_rtg_empty_shapes_are_ok_and_write_nothing(dev, T, n):
    from g2048 import _lib as L
    rc = _cfg(R.CFG, BETA)
    st = torch.tensor(STATE0, dtype=torch.float64, device=dev)
    L.rtg_prepare(st, rc)
    st1 = st.clone()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    outs = [torch.full((64,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    rew = torch.full((64,), SENTINEL, dtype=torch.float64, device=dev)
    part = torch.full((3,), SENTINEL, dtype=torch.float64, device=dev)
    ws = torch.zeros(L.rtg_workspace_bytes(n), dtype=torch.uint8, device=dev)
    L.reward_rtg(z((T, n), torch.int32), z((T, n, 4), torch.int8), z((T, n), torch.uint8), z((T, n), torch.float32),
                 st, *outs, part, ws, rc, reward=rew)      # a non-zero status raises
    L.rtg_finalize(st, part, rc)
    torch.cuda.synchronize()
    assert _bits_equal(part.cpu().numpy(), np.zeros(3))
    assert all(bool((o == SENTINEL).all()) for o in outs + [rew])
    assert torch.equal(st, st1)


def test_rtg_prepare_every_branch(dev):
    from g2048 import _lib as L
    hit = {"bc": 0, "var": 0, "step": 0}
    for s4, beta in R.prepare_table():
        state = s4 + [-3.0, -4.0, -5.0, -6.0]
        t = R.rtg_prepare_terms(state, beta)
        st = torch.tensor(state, dtype=torch.float64, device=dev)
        L.rtg_prepare(st, _cfg(R.CFG, beta))
        got = st.cpu().numpy()
        rtol = 4 * 2.0 ** -52 * (1.0 + t["pow"] / t["bc"])
        for k in (4, 5):
            assert abs(got[k] - t["state"][k]) <= rtol * abs(t["state"][k]), (s4, beta, k, got[k], t["state"][k])
        assert _bits_equal(got[[0, 1, 2, 3, 6, 7]], np.array(state)[[0, 1, 2, 3, 6, 7]])
        hit["bc"] += t["bc_clamped"]
        hit["var"] += t["var_clamped"]
        hit["step"] += t["step_clamped"]
    assert hit["bc"] >= 2 and hit["var"] >= 1 and hit["step"] >= 1, hit


def test_rtg_tracker_chain_of_three(dev):
    """Three RTGTracker.compute calls on different trajectories against the reference chained the same way
    (prepare -> scan -> the kernel's one-pass finalize from the exact sums).  The state differs from the
    reference's by the summation bound, a few 1e-15 relative here: g_raw stays bit-identical, g_norm / adv
    within one float32 step, the moments within 1e-11."""
    from g2048.advantage import RewardWeights, RTGTracker
    T, n = 17, 257
    w = RewardWeights(gamma=R.GAMMA, points=R.W_POINTS, mono=R.W_MONO, emptiness=R.W_EMPT, rtg_beta=0.9)
    tr = RTGTracker(n, dev, w)
    ref = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0])
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    for it in range(3):
        c = R.rtg_case(T, n, seed=it + 1)
        outs = [torch.full((T, n), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
        tr.compute(td(c["points"]), td(c["pot"]), td(c["flags"]), td(c["value"]), *outs)
        ref = R.rtg_prepare(ref, 0.9)
        r = R.rtg_scan(c["points"], c["pot"], c["flags"], c["value"], R.CFG, ref)
        ref = R.rtg_finalize(ref, (r["s1"], r["s2"], r["cnt"]), 0.9)
        assert _bits_equal(outs[0].cpu().numpy(), r["g_raw"].astype(np.float32))
        assert _ulps(outs[1].cpu().numpy(), r["g_norm"]).max() <= 1
        assert _ulps(outs[2].cpu().numpy(), r["adv"]).max() <= 1
        got = tr.state.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=0, err_msg=f"compute {it}")
        assert got[3] == 2.0 + it
        m = tr.moments()
        assert m["rtg_step"] == 2 + it and m["batch_var"] == got[7] and m["std"] == got[5]


# ------------------------------------------------------------------------------ episode scan -----
@pytest.mark.parametrize("T,n", R.STATS_SHAPES)
def test_episode_scan_equals_walk(dev, T, n):
    from g2048 import _lib as L
    rs0, rm0 = np.arange(n, dtype=np.int64) * 7 + 1, (np.arange(n) % 11).astype(np.int32)
    rs, rm = torch.from_numpy(rs0).to(dev), torch.from_numpy(rm0).to(dev)
    for it in range(2):
        c = R.stats_case(T, n, False, seed=it)
        sc = torch.full((T, n), -5, dtype=torch.int64, device=dev)
        ti = torch.full((T, n), -5, dtype=torch.int32, device=dev)
        td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        L.episode_scan(td(c["points"]), td(c["boards"]), td(c["max_tile"]), td(c["flags"]), rs, rm, sc, ti)
        wsc, wti, rs0, rm0 = R.episode_walk(c["points"], c["boards"], c["max_tile"], c["flags"], rs0, rm0)
        assert np.array_equal(sc.cpu().numpy(), wsc) and np.array_equal(ti.cpu().numpy(), wti), f"rollout {it}"
        assert np.array_equal(rs.cpu().numpy(), rs0) and np.array_equal(rm.cpu().numpy(), rm0), f"carry {it}"


# ------------------------------------------------------------------------------ rollout stats ----
STATS_CFG = (0.99, 0.1, 1.0, 0.5)


class _Stats:
    def __init__(self, dev, T, n):
        from g2048 import _lib as L
        self.dev, self.L = dev, L
        self.ws = torch.zeros(L.rollout_stats_workspace_bytes(T, n), dtype=torch.uint8, device=dev)
        self.out = torch.full((L.ROLLOUT_STATS,), float("nan"), dtype=torch.float32, device=dev)
        self.cfg = _cfg(STATS_CFG, 0.9)

    def run(self, c, rs, rm):
        td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)  # noqa: E731
        a = [td(c[k]) for k in ("points", "pot", "flags", "value", "g_raw", "g_norm", "adv", "boards")]
        self.out.fill_(float("nan"))
        if c["episodic"]:
            self.L.rollout_stats(*a, None, True, self.cfg, None, None, self.ws, self.out)
        else:
            self.L.rollout_stats(*a, td(c["max_tile"]), False, self.cfg, rs, rm, self.ws, self.out)
        torch.cuda.synchronize()
        assert int(self.ws[:4].view(torch.int32)[0]) == 0, "the key counter is not left 0"
        return self.out.cpu().numpy().copy()


def _check_stats(got, ref, aux, label):
    f32 = lambda x: np.float32(x)  # noqa: E731
    nr = int(ref[0])
    assert got[0] == nr, label
    zc = float(got[3]) * nr / 100.0
    assert abs(zc - round(zc)) < 0.01 and round(zc) == aux["zero_rows"], (label, zc, aux["zero_rows"])
    for j in (17, 18, 22):
        assert got[j] == f32(ref[j]), (label, R.STAT_NAMES[j], got[j], ref[j])
    for j in (19, 20, 21):
        assert _ulps(got[j], ref[j]) <= 1, (label, R.STAT_NAMES[j], got[j], ref[j])
    for j in (7, 8, 11, 12):
        assert got[j] == f32(ref[j]), (label, R.STAT_NAMES[j], got[j], ref[j])
    worst = 0.0

    def within(j, bound):
        nonlocal worst
        err = abs(float(got[j]) - ref[j])
        assert err <= bound, (label, R.STAT_NAMES[j], float(got[j]), ref[j], err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    for j, k in R.MEAN_TYPE.items():
        within(j, U22 * aux["mean_abs"][k])
    within(15, U22 * aux["g0_mean_abs"])
    within(16, U22 * abs(ref[16]))
    for j, k in R.VAR_TYPE.items():
        within(j, U22 * aux["mean_sq"][k])
    within(6, U22 * ref[6])
    for j, k in R.STD_TYPE.items():
        d = U22 * aux["mean_sq"][k]          # the variance's bound; sqrt(v + d) - sqrt(v) <= min(d / 2 sqrt v, sqrt d)
        within(j, min(d / (2 * ref[j]), math.sqrt(d)) if ref[j] > 0 else math.sqrt(d))
    return worst


@pytest.mark.parametrize("episodic", [False, True], ids=["fixed", "episodic"])
@pytest.mark.parametrize("T,n", R.STATS_SHAPES + [R.WRAP_SHAPE])
def test_rollout_stats_against_float64_reference(dev, episodic, T, n):
    rollouts = 1 if (T, n) == R.WRAP_SHAPE else 3   # the wrap shape: more than 64 blocks of partials, once
    s = _Stats(dev, T, n)
    rs0, rm0 = np.arange(n, dtype=np.int64) * 13 % 5000, (np.arange(n) % 9).astype(np.int32)
    rs, rm = torch.from_numpy(rs0).to(dev), torch.from_numpy(rm0).to(dev)
    worst = 0.0
    for it in range(rollouts):
        c = R.stats_case(T, n, episodic, seed=it)
        before = (rs.clone(), rm.clone())
        got = s.run(c, rs, rm)
        ref, aux = R.rollout_stats(c["points"], c["pot"], c["flags"], c["value"], c["g_raw"], c["g_norm"], c["adv"],
                                   c["boards"], c["max_tile"], episodic, STATS_CFG, rs0, rm0)
        assert not np.isnan(got).any(), got
        worst = max(worst, _check_stats(got, ref, aux, f"{'episodic' if episodic else 'fixed'} T {T} n {n} rollout {it}"))
        if not episodic:
            rs0, rm0 = aux["run_score"], aux["run_max"]
            assert np.array_equal(rs.cpu().numpy(), rs0) and np.array_equal(rm.cpu().numpy(), rm0)
        else:
            assert torch.equal(rs, before[0]) and torch.equal(rm, before[1])
        rs2, rm2 = before[0].clone(), before[1].clone()     # the same inputs and workspace again
        assert _bits_equal(s.run(c, rs2, rm2), got), "a second call differs"
    print(f"rollout stats T {T} n {n} {'episodic' if episodic else 'fixed'}: worst moment error / bound {worst:.4f}")


@pytest.mark.parametrize("name", list(R.key_sets()))
def test_radix_select_key_sets(dev, name):
    keys = R.key_sets()[name]
    c = R.key_case(keys)
    s = _Stats(dev, c["T"], c["n"])
    rs, rm = torch.from_numpy(c["run_score"]).to(dev), torch.from_numpy(c["run_max"]).to(dev)
    got = s.run(c, rs, rm)
    ref, aux = R.rollout_stats(c["points"], c["pot"], c["flags"], c["value"], c["g_raw"], c["g_norm"], c["adv"],
                               c["boards"], c["max_tile"], False, STATS_CFG, c["run_score"], c["run_max"])
    k = len(keys)
    srt = np.sort(keys)
    assert got[22] == k
    assert got[17] == np.float32(srt[(k - 1) // 2] if k else -1), (name, got[17], srt[(k - 1) // 2] if k else -1)
    assert got[18] == np.float32(srt[-1] if k else -1), (name, got[18])
    assert abs(float(got[16]) - ref[16]) <= U22 * abs(ref[16])
    assert ref[17] == (srt[(k - 1) // 2] if k else -1)
    _check_stats(got, ref, aux, name)


# ------------------------------------------------------------------------------ sampler ----------
@pytest.fixture(scope="module")
def sampler_ref():
    t = R.sampler_table()
    n = len(t["legal"])
    u = R.uniforms(O.philox_draws(R.SAMPLER_SEED, R.SAMPLER_COUNTER, n, 1, env_base=R.SAMPLER_ENV_BASE)[:, 0])
    return t, u, R.masked_sampler(t["logits"], t["legal"], u), R.masked_sampler(None, t["legal"], u)


@pytest.mark.parametrize("high", [0, 0xF0], ids=["low-nibble", "high-bits-set"])
@pytest.mark.parametrize("way", ["contiguous", "stride8", "none"])
def test_sampler_masks_logits_and_call_shapes(dev, sampler_ref, way, high):
    from g2048 import _lib as L
    t, u, ref_table, ref_none = sampler_ref
    ref = ref_none if way == "none" else ref_table
    n = len(t["legal"])
    fl = torch.from_numpy((t["legal"] | high).astype(np.uint8)).to(dev)
    if way == "contiguous":
        lg = torch.from_numpy(t["logits"]).to(dev)
    elif way == "stride8":
        big = torch.full((n, 8), float("nan"), dtype=torch.float32, device=dev)
        big[:, :4] = torch.from_numpy(t["logits"]).to(dev)
        lg = big[:, :4]
        assert lg.stride(0) == 8
    else:
        lg = None
    act = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    lp = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
    ent = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    L.sample_actions(lg, fl, act, lp, ent, L.make_rng(L.RNG_PHILOX, R.SAMPLER_SEED, R.SAMPLER_COUNTER,
                                                      R.SAMPLER_ENV_BASE))
    torch.cuda.synchronize()
    lpn, en, an = lp.cpu().numpy(), ent.cpu().numpy(), act.cpu().numpy().astype(np.int64)
    bits = ref["bits"]
    assert not np.isnan(lpn).any() and not np.isnan(en).any()
    assert np.isneginf(lpn[~bits]).all() and np.isfinite(lpn[bits]).all()
    e_lp = np.abs(lpn[bits].astype(np.float64) - ref["logp"][bits])
    e_en = np.abs(en.astype(np.float64) - ref["entropy"])
    tol_lp = 1e-5 + U22 * np.abs(ref["logp"][bits])
    tol_en = 1e-5 + U22 * np.abs(ref["entropy"])
    gap = np.isin(t["pattern"], [R.LOGIT_PATTERNS.index(k) for k in ("gap30", "gap100", "gap1e4")])
    print(f"sampler {way} high {high:#x}: worst |logp - ref| {e_lp.max():.3e} (worst error / tolerance "
          f"{(e_lp / tol_lp).max():.3f}), worst |entropy - ref| {e_en.max():.3e} ({(e_en / tol_en).max():.3f}); "
          f"gap rows: entropy {e_en[gap].max():.3e}; where |logp| <= 25: {e_lp[np.abs(ref['logp'][bits]) <= 25].max():.3e}")
    assert (e_lp <= tol_lp).all(), (float(e_lp.max()), int(np.argmax(e_lp / tol_lp)))
    assert (e_en <= tol_en).all(), (float(e_en.max()), int(np.argmax(e_en / tol_en)))
    k = bits.sum(axis=1)
    single, none = k == 1, k == 0
    assert (lpn[single][bits[single]] == 0).all() and (en[single] == 0).all()
    assert np.array_equal(an[single], np.argmax(bits[single], axis=1))
    assert (an[none] == 0).all() and (en[none] == 0).all() and np.isneginf(lpn[none]).all()
    if way == "none":
        some = k > 0
        assert np.abs(en[some] - np.log(k[some])).max() <= 1e-5 + U22 * math.log(4)
        assert np.abs(lpn[bits] + np.log(np.repeat(k, k))).max() <= 1e-5 + U22 * math.log(4)
    assert (an < 4).all() and (bits[np.arange(n), an] | none).all(), "an illegal action was sampled"
    far = ref["dist"] >= R.NEAR_BOUNDARY
    assert far.mean() >= 0.99
    assert np.array_equal(an[far], ref["action"][far]), np.argwhere(an[far] != ref["action"][far])[:5]


def test_sampler_thirds_property(dev):
    """2^18 rows of logits (0, 0, 0) on three legal moves: the float32 thirds sum below 1, and still every
    action is legal and each is drawn a third of the time within 5 sigma."""
    from g2048 import _lib as L
    n = 1 << 18
    logits = torch.zeros(n, 4, device=dev)
    logits[:, 1] = 50.0                                    # the illegal move: would win if it were read
    fl = torch.full((n,), 0b1101 | 0x60, dtype=torch.uint8, device=dev)
    act = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    L.sample_actions(logits, fl, act, None, None, L.make_rng(L.RNG_PHILOX, 5, 1, 1000))
    counts = torch.bincount(act.long(), minlength=4).cpu().numpy()
    assert len(counts) == 4 and counts[1] == 0 and counts.sum() == n
    sigma = math.sqrt((1 / 3) * (2 / 3) / n)
    assert np.abs(counts[[0, 2, 3]] / n - 1 / 3).max() <= 5 * sigma, counts
