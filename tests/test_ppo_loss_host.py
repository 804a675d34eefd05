"""The fp64 row reference of the PPO loss (tests/ppo_loss_reference.py) is right before any kernel is
compared with it: against float64 autograd of g2048.ppo.ppo_losses and against ppo.kl_old_new on the whole
branch table; the table holds every regime at its stated margin; the fp32 emulation takes the same branch
as fp64 on every row; and the rounding budget the GPU tests allow is measured here (printed: run with -s),
in units of 2^-23 of each quantity's scale, and held against the constants of the reference module.
CPU only."""

import numpy as np
import pytest
import torch

import ppo_loss_reference as R

BETA, CRITIC = 0.05, 0.7


@pytest.fixture(scope="module")
def tab():
    return R.branch_table()


@pytest.fixture(scope="module")
def terms(tab):
    inv_m = 1.0 / len(tab["act"])
    return R.table_terms(tab, BETA, CRITIC, inv_m), R.table_terms(tab, BETA, CRITIC, inv_m, np.float32), inv_m


def _autograd(tab, beta, critic, clip_eps):
    from g2048.ppo import invalid_from_legal, ppo_losses
    z = torch.from_numpy(tab["z"]).requires_grad_(True)
    legal = torch.from_numpy(tab["legal"])
    loss, parts = ppo_losses(z[:, :4], z[:, 4], torch.from_numpy(tab["act"]), invalid_from_legal(legal),
                             torch.from_numpy(tab["old_logp"]).double(), torch.from_numpy(tab["adv"]).double(),
                             torch.from_numpy(tab["ret"]).double(), beta, critic, clip_eps)
    loss.backward()
    return {"ppo": parts["ppo"].detach().numpy(), "ent": parts["entropy"].detach().numpy(),
            "vl": parts["vloss"].detach().numpy(), "masked": parts["masked"].detach().numpy(),
            "grad": z.grad.numpy()}


def test_clip_bounds_are_the_abi_fp32_values():
    assert R.CLIP_LO == float(np.float32(1.0) - np.float32(0.2)) != 0.8
    assert R.CLIP_HI == float(np.float32(1.0) + np.float32(0.2)) != 1.2
    assert abs(R.CLIP_LO - 0.8) < 2 ** -24 and abs(R.CLIP_HI - 1.2) < 2 ** -23


def test_row_reference_matches_float64_autograd(tab, terms):
    """ppo, ent, vl and all five gradients at 1e-12 of each quantity's scale.  ppo_losses forms both clip
    bounds from one double clip_eps, the ABI from fp32 1.0f -+ clip_eps, which are not symmetric about 1: so
    autograd runs twice, with clip_eps = CLIP_HI - 1 (its upper bound is then CLIP_HI exactly) for the rows
    whose ratio is above 1 and with clip_eps = 1 - CLIP_LO (lower bound CLIP_LO exactly) for the others --
    the rows are independent, a row only ever meets the bound on its side of 1."""
    t, _, inv_m = terms
    m = len(tab["act"])
    up, dn = _autograd(tab, BETA, CRITIC, R.CLIP_HI - 1.0), _autograd(tab, BETA, CRITIC, 1.0 - R.CLIP_LO)
    assert 1.0 + (R.CLIP_HI - 1.0) == R.CLIP_HI and 1.0 - (1.0 - R.CLIP_LO) == R.CLIP_LO
    hi_side = t["ratio"] > 1.0
    parts = {k: np.where(hi_side.reshape((m,) + (1,) * (up[k].ndim - 1)), up[k], dn[k]) for k in up}
    grad = parts["grad"]
    sc = R.loss_scales(t, tab["adv"], BETA, inv_m=inv_m, critic=CRITIC)
    worst = {}
    for key, got, want, scale in (("ppo", t["ppo"], parts["ppo"], sc["ppo"] + 1e-300),
                                  ("ent", t["ent"], parts["ent"], sc["ent"]),
                                  ("vl", t["vl"], parts["vl"], sc["vl"] + 1e-300),
                                  ("dz", t["dz"][:, :4], grad[:, :4], sc["dz"][:, None]),
                                  ("dv", t["dz"][:, 4], grad[:, 4], sc["dv"])):
        err = np.abs(got - want) / scale
        worst[key] = float(err.max())
        assert worst[key] <= 1e-12, (key, worst[key], int(np.argmax(err.reshape(m, -1).max(1))))
    assert np.array_equal(t["masked"], parts["masked"])
    print("fp64 reference vs float64 autograd, worst error / scale:", worst)


def test_kl_reference_matches_kl_old_new():
    from g2048.ppo import kl_old_new
    k = R.kl_table()
    old = torch.from_numpy(k["old"]).double()
    want = kl_old_new(old, torch.from_numpy(k["new"]), torch.isinf(old)).numpy()
    got = R.kl_row_ref(k["old"], k["new"])
    assert np.abs(got - want).max() <= 1e-12 * R.kl_scale(k["old"], k["new"]).max()
    name = np.array(k["name"])
    assert np.array_equal(got[name == "one_legal"], np.zeros(2))
    assert np.abs(got[name == "old_eq_new"]).max() <= 1e-15
    assert got.min() >= -1e-15 and got.max() > 1.0
    for want_name in ("one_legal", "old_60_below", "new_p1000", "new_m1000", "illegal_huge", "old_eq_new"):
        assert (name == want_name).sum() >= 2


def test_stats_reference_matches_the_eager_updater_stack():
    """stats_ref against the expressions PPOUpdater._post stacks (loss, -mean ppo, -beta mean H, ...)."""
    g = np.random.default_rng(1)
    m, beta, critic, gn = 37, 0.03, 0.6, 1.9
    ppo, ent, vl, kl = g.normal(size=m), g.random(m), g.random(m), g.random(m)
    want = [-(ppo - critic * vl + beta * ent).mean(), -ppo.mean(), -beta * ent.mean(), critic * vl.mean(), gn,
            ent.mean(), kl.sum(), kl.mean(), kl.max()]
    got = R.stats_ref((ppo.sum(), ent.sum(), vl.sum()), kl.sum(), kl.max(), gn, beta, critic, m)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    assert len(got) == len(R.STAT_KEYS)
    from g2048.ppo import STAT_KEYS
    assert tuple(STAT_KEYS) == R.STAT_KEYS


def test_table_holds_every_regime(tab):
    tags = tab["tags"]
    have = {t for row in tags for t in row}
    missing = [r for r in R.REQUIRED_REGIMES if r not in have]
    assert not missing, missing
    # every regime appears with >= 4 different (legal mask, action) pairs: the pattern groups (the first tag of
    # a row: plain, the logit regimes, legal_1 .. legal_3, act_illegal) by their own rows alone, the other
    # regimes (log-ratio, advantage, value gap, legal count) over all rows that carry the tag
    own, pairs = {}, {}
    for i, row in enumerate(tags):
        pair = (int(tab["legal"][i]), int(tab["act"][i]))
        own.setdefault(row[0], set()).add(pair)
        for t in row[1:]:
            pairs.setdefault(t, set()).add(pair)
    groups = {p[0] for p in R.PLAIN_PATTERNS + R.LOGIT_PATTERNS + R.ILLEGAL_ACTION_PATTERNS}
    assert groups == set(own)
    short = {r: len(v) for r, v in list(own.items()) + list(pairs.items()) if len(v) < 4}
    assert not short, short
    # ... and every log-ratio regime with every advantage sign, each again on >= 4 pairs
    for lr in tuple(R.LOG_RATIO_REGIMES) + ("lr_minus_inf",):
        for adv in R.ADV_REGIMES:
            got = {(int(tab["legal"][i]), int(tab["act"][i])) for i, row in enumerate(tags) if lr in row and adv in row}
            assert len(got) >= 4, (lr, adv, len(got))
    # every value gap in every log-ratio regime
    for lr in R.LOG_RATIO_REGIMES:
        for gap in R.VALUE_GAPS:
            assert any(lr in row and "gap_%g" % gap in row for row in tags), (lr, gap)
    assert R.is_bf16(tab["z"])
    lg = ((tab["legal"][:, None] >> np.arange(4)) & 1).astype(bool)
    assert lg.any(1).all()
    act_legal = lg[np.arange(len(tags)), tab["act"]]
    assert np.array_equal(~act_legal, np.array(["act_illegal" in row for row in tags]))
    assert np.isfinite(tab["old_logp"][np.arange(len(tags)), tab["act"]]).all()
    assert np.array_equal(np.isfinite(tab["old_logp"]) | ~act_legal[:, None], lg | ~act_legal[:, None])


def test_rows_sit_at_their_margins(tab, terms):
    """From the fp64 row values: the log-ratio >= 0.5 from +-20 and within 1e-6 of its target, the ratio
    >= 0.05 from the clip bounds, every legal logit >= 0.5 from +-20, |v - ret| exactly 1 or >= 0.2 from
    it; and each row lies in the regime its name says."""
    t, _, _ = terms
    tags = tab["tags"]
    fin = np.isfinite(t["dlt"])
    assert np.array_equal(~fin, np.array(["lr_minus_inf" in row for row in tags]))
    assert (t["dlt"][~fin] == -np.inf).all()
    dlt = t["dlt"][fin]
    assert np.abs(dlt - tab["target"][fin]).max() <= 4 * 2.0 ** -24 * (np.abs(tab["old_logp"]).max(1, initial=0,
                                                                      where=np.isfinite(tab["old_logp"]))[fin]).max()
    assert (np.abs(np.abs(dlt) - 20.0) >= R.MARGIN_LOG_RATIO).all()
    ratio = t["ratio"]
    assert (np.abs(ratio - R.CLIP_LO) >= R.MARGIN_RATIO).all() and (np.abs(ratio - R.CLIP_HI) >= R.MARGIN_RATIO).all()
    mk = t["masked"]
    lgl = np.isfinite(mk)
    assert (np.abs(np.abs(mk[lgl]) - 20.0) >= R.MARGIN_LOGIT).all()
    av = np.abs(t["dv0"])
    assert ((av == 1.0) | (np.abs(av - 1.0) >= R.MARGIN_VALUE)).all()
    assert (av == 1.0).sum() >= 8
    want = {"lr_below_m20": lambda i: t["dlt"][i] < -20, "lr_minus_inf": lambda i: t["dlt"][i] == -np.inf,
            "lr_low": lambda i: t["in20"][i] and ratio[i] < R.CLIP_LO, "lr_in": lambda i: t["inr"][i],
            "lr_high": lambda i: t["in20"][i] and ratio[i] > R.CLIP_HI, "lr_above_p20": lambda i: t["dlt"][i] > 20,
            "adv_pos": lambda i: tab["adv"][i] > 0, "adv_neg": lambda i: tab["adv"][i] < 0,
            "adv_zero": lambda i: tab["adv"][i] == 0,
            "logit_hi_taken": lambda i: t["hi_logit"][i, tab["act"][i]],
            "logit_lo_taken": lambda i: t["lo_logit"][i, tab["act"][i]],
            "logit_hi_other": lambda i: t["hi_logit"][i].any() and not t["hi_logit"][i, tab["act"][i]],
            "logit_lo_other": lambda i: t["lo_logit"][i].any() and not t["lo_logit"][i, tab["act"][i]],
            "illegal_huge": lambda i: (tab["z"][i, :4][~t["legal"][i]] == R.BIG).any(),
            "taken_100_below": lambda i: mk[i].max() - mk[i, tab["act"][i]] >= 100,
            "all_p1000": lambda i: (tab["z"][i, :4] >= 990).all(), "all_m1000": lambda i: (tab["z"][i, :4] <= -990).all()}
    for i, row in enumerate(tags):
        for tag in row:
            if tag in want:
                assert want[tag](i), (i, tag)
            elif tag.startswith("gap_"):
                assert abs(t["dv0"][i] - float(tag[4:])) < 1e-6, (i, tag)
            elif tag.startswith("legal_"):
                assert t["legal"][i].sum() == int(tag[6:]), (i, tag)
    # the tie rule: every in-range row has t1 == t2; out of range the two sides differ unless A == 0
    assert (t["side"][t["inr"]] == 0).all()
    out = ~t["inr"] & (tab["adv"] != 0)
    assert (t["side"][out] != 0).all()


def test_fp32_emulation_takes_the_same_branches(tab, terms):
    t64, t32, _ = terms
    k64, k32 = R.branch_key(t64), R.branch_key(t32)
    for name in k64:
        assert np.array_equal(k64[name], k32[name]), (name, np.nonzero(np.asarray(k64[name] != k32[name]))[0][:8])
    assert all(v.dtype == np.float32 for v in (t32["ppo"], t32["ent"], t32["vl"], t32["dz"], t32["ratio"], t32["logp"]))


def test_one_legal_action_gives_an_exactly_zero_logit_gradient_in_fp32(tab, terms):
    """With one legal action the ppo term's (onehot - softmax) is 1 - 1; the entropy's softmax still holds
    the three illegal slots at -20, which add 3 e^(-20 - z) to its sum: below 2^-25 for the table's lone
    logits (z >= 0.25, or outside the clamp where the gradient is cut), so fp32 gives exactly 0 and fp64 a
    value below a tenth of one unit of the budget."""
    t64, t32, inv_m = terms
    one = t64["legal"].sum(1) == 1
    assert one.sum() >= 30
    z = t64["masked"][one].max(1)
    assert ((z >= 0.25) | (np.abs(z) > 20)).all()
    assert (t32["dz"][one, :4] == 0).all()
    assert np.abs(t64["dz"][one, :4]).max() <= 0.1 * R.U23 * BETA * inv_m


def test_measured_rounding_budget(tab, terms):
    """max |fp32 emulation - fp64| over the table in units of 2^-23 of each quantity's scale: printed, and no
    larger than the constants the GPU tests multiply by DEVICE_FACTOR, which carry 5 % over these counts."""
    t64, t32, inv_m = terms
    sc = R.loss_scales(t64, tab["adv"], BETA, CRITIC, inv_m)
    tiny = 1e-300
    meas = {"ppo": np.abs(t32["ppo"] - t64["ppo"]) / (sc["ppo"] + tiny),
            "ent": np.abs(t32["ent"] - t64["ent"]) / sc["ent"],
            "vl": np.abs(t32["vl"] - t64["vl"]) / (sc["vl"] + tiny),
            "dz": (np.abs(t32["dz"][:, :4] - t64["dz"][:, :4]) / sc["dz"][:, None]).max(1),
            "dv": np.abs(t32["dz"][:, 4] - t64["dz"][:, 4]) / sc["dv"]}
    k = R.kl_table()
    meas["kl"] = np.abs(R.kl_row_ref(k["old"], k["new"], np.float32) - R.kl_row_ref(k["old"], k["new"])) / \
        R.kl_scale(k["old"], k["new"])
    units = {q: float(v.max() / R.U23) for q, v in meas.items()}
    print("measured fp32 rounding budget, units of 2^-23 of scale:", {q: round(u, 2) for q, u in units.items()},
          "constants:", R.UNITS, "device factor:", R.DEVICE_FACTOR)
    for q, u in units.items():
        assert u <= R.UNITS[q], (q, u, int(np.argmax(meas[q])))
        assert R.UNITS[q] <= (1.0 + R.UNITS_HEADROOM) * u + 0.01, (q, u)  # the constant IS the measurement
    assert R.DEVICE_FACTOR == 4.0
