"""The fused policy rollout (g2048_policy_rollout, csrc/policy_rollout.hip) where its env step is its
own code: step_board_carry (csrc/step.hpp) carries the monotonicity statistics and the empty-cell
count from step to step (mono_add_tile, csrc/board.hpp) and recomputes them after an auto-reset; the
legal mask of a launch's first step comes from flags[t0]; 32 boards share a wave with their own spawn
draws; the grid is persistent over groups of 256 boards.  Rollouts from Rollout.reset() boards of 12
to 40 steps (test_gpu_policy_rollout.py) end almost no game and see no tile above 2^6, so the boards
here are constructed: games that end at a chosen step, boards dead at launch start, tiles up to 2^17,
long runs, a second pass of the persistent loop, saturated logits.

Every scenario asserts (a) fused records == per-step records (obs_encode -> FusedPolicy ->
sample_actions -> env_step), bitwise, on all nine fields; (b) boards / flags / points / max_tile / pot
== rollout_reference.replay() of the recorded actions on the CPU oracle, exactly; (c) that the path it
was built for was taken, read from the oracle replay.  The sampler's edges are checked against the
float64 sampler_reference at the project's tolerances (test_sampler_matches_reference_masked_softmax:
rtol 1e-5 / atol 1e-5, the action outside a 1e-5 band around the CDF boundaries).

Counts observed on an MI355X (printed by the tests; resets / inactive env-steps / largest exponent
from the oracle replay, excluded rows from the float64 reference):

  scenario                            resets     inactive env-steps   largest exponent   excluded rows
  1 ends at step 0, n = 273 / 33 / 1  11 / 7 / 1   0                  8                  -
  2 ends mid-buffer                   11           0                  8                  -
  3 dead at launch, auto / episodic   3 / 0        0 / 18             3                  -
  4 episodic tails                    0            825                8                  -
  5 high tiles, h = 196 / 128         421 / 367    0                  17                 -
  6 long run, auto, h = 32 / 196      585 / 802    0                  9 / 8              -
  6 long run, episodic, h = 32 / 196  0            66 174 / 82 086    9 / 8              -
  7 second pass                       4            0                  8                  -
  8 saturated logits                  0            0                  4                  1 of 2 048
  sampler edges, [n, 4] and [n, 8]    -            -                  -                  0 of 8 192

Scenario 5 also saw 59 / 36 spawns above the board's maximum, 284 / 75 spawns that tie it in front of
it and change its corner status, 40 / 55 steps of 65 536 points and 5 / 7 of 131 072; scenario 8's
smallest log-probability of a legal action was -6 285.9.
"""

import numpy as np
import pytest
import torch

from oracle import oracle as O
from policy_rollout_util import _assert_same, _model, _run
from rollout_reference import (C, D, DT, FLAG_DONE, FLAG_INACTIVE, FLAG_INVALID, FLAG_RESET, OPT_AUTO_RESET,
                               OPT_SKIP_DONE, replay, sampler_reference)
from test_gpu_env_carry import random_boards

pytestmark = pytest.mark.gpu

SEED = 9         # _run's Philox seed
COUNTER = 1      # the device counter after Rollout.reset()
ENDED = FLAG_DONE | FLAG_RESET
ONE = np.array([1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1, 0, 2, 1, 2, 0], np.int8)  # RIGHT is the only legal move


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    return torch.device("cuda:0")


def _inject(boards, which):
    """A _run hook: boards[which] replace the envs `which` of row t0."""
    def hook(ro, t0):
        idx = torch.as_tensor(np.nonzero(which)[0], device=ro.buf.boards.device)
        ro.buf.boards[t0][idx] = torch.as_tensor(np.ascontiguousarray(boards[which])).to(ro.buf.boards.device)
    return hook


def _place(n, placements):
    boards, which = np.zeros((n, 16), np.int8), np.zeros(n, bool)
    for envs, board in placements:
        boards[list(envs)] = board
        which[list(envs)] = True
    return boards, which


def _both(dev, m, n, T, episodic, hook, chunks=None, t0=0, env_base=0):
    """(a) and (b); returns the records (numpy) and the oracle replay from row t0 on as a dict."""
    ref = _run(dev, m, n, T, fused=False, episodic=episodic, chunks=chunks, env_base=env_base, hook=hook)
    got = _run(dev, m, n, T, fused=True, episodic=episodic, chunks=chunks, env_base=env_base, hook=hook)
    _assert_same(ref, got)
    rec = {k: v.cpu().numpy() for k, v in got.items()}
    rp = _replay(rec, t0, T, env_base, episodic)
    _assert_replay(rec, rp, t0, T)
    return rec, rp


def _replay(rec, t0, t1, env_base, episodic):
    opts = OPT_SKIP_DONE if episodic else OPT_AUTO_RESET
    out = replay(rec["boards"][t0], rec["actions"][t0:t1], SEED, COUNTER + 2 * t0, env_base, opts)
    return dict(zip(("boards", "flags", "points", "max_tile", "pot"), out))


def _assert_replay(rec, rp, t0, t1, envs=slice(None)):
    for k in ("boards", "flags"):
        x, y = rec[k][t0 + 1:t1 + 1][:, envs], rp[k][1:][:, envs]
        assert np.array_equal(x, y), (k, np.argwhere((x != y).reshape(x.shape[0], x.shape[1], -1).any(-1))[:5].tolist())
    assert np.array_equal(rec["flags"][t0][envs] & 0xF, rp["flags"][0][envs])
    for k in ("points", "max_tile", "pot"):
        x, y = rec[k][t0:t1][:, envs], rp[k][:, envs]
        assert np.array_equal(x, y), (k, np.argwhere((x != y).reshape(x.shape[0], x.shape[1], -1).any(-1))[:5].tolist())


def _counts(name, rp):
    fl = rp["flags"][1:]
    c = {"resets": int(((fl & FLAG_RESET) != 0).sum()), "inactive": int(((fl & FLAG_INACTIVE) != 0).sum()),
         "largest": int(rp["boards"].max())}
    print(f"{name}: {c}")
    return c


def _ending_envs(n):
    d = sorted({e for e in (0, 15, 16, 31, 32, 255, 256, n - 1) if e < n})
    dt = sorted({e for e in (1, 17, 33) if e < n} - set(d))
    return d, dt


# ------------------------------------------------------------------ 1, 2: games that end -------
@pytest.mark.parametrize("n", [256 + 17, 33, 1])
def test_game_ends_at_first_step_auto_reset(dev, n):
    """D / DT (every legal move ends the game) in the first and last lanes of waves, MFMA tiles and
    workgroups: the DONE | RESET branch of step_board_carry on the launch's first step, the fresh
    boards then moved for five steps on the carry recomputed after the reset."""
    T = 6
    d, dt = _ending_envs(n)
    boards, which = _place(n, [(d, D), (dt, DT)])
    rec, rp = _both(dev, _model(dev, 196, 1000 + n), n, T, False, _inject(boards, which))
    ended = (rp["flags"][1] & ENDED) == ENDED
    assert np.array_equal(np.nonzero(ended)[0], np.nonzero(which)[0])
    fresh = O.reset(n, O.RNG_PHILOX, SEED, step_idx=COUNTER + 1)
    assert np.array_equal(rp["boards"][1][which], fresh[which])
    # every later step is a real move of the reset game: its potentials come from the new carry
    assert not (rp["flags"][2:][:, which] & (FLAG_INVALID | FLAG_DONE)).any()
    assert (rp["pot"][1:][:, which, 2] >= 14 - np.arange(T - 1)[:, None]).all()  # empt_b of a two-tile game
    c = _counts(f"ends at step 0, n={n}", rp)
    assert c["resets"] == which.sum() and c["inactive"] == 0


def test_game_ends_mid_buffer(dev):
    """The same boards written into row 5 of a 9-row buffer whose steps 0..4 were played first; the
    launch at t0 = 5 restarts the carry from the injected row, the launch at t0 = 6 from reset boards
    (so this pins the launch-start state; the carry recomputed after a reset is scenario 1's)."""
    n, T, t0 = 256 + 17, 9, 5
    d, dt = _ending_envs(n)
    boards, which = _place(n, [(d, D), (dt, DT)])
    m = _model(dev, 196, 77)
    chunks = [(0, 5), (5, 6), (6, 9)]
    rec, rp = _both(dev, m, n, T, False, {t0: _inject(boards, which)}, chunks=chunks, t0=t0)
    ended = (rp["flags"][1] & ENDED) == ENDED
    assert np.array_equal(np.nonzero(ended)[0], np.nonzero(which)[0])
    assert not (rp["flags"][2:][:, which] & (FLAG_INVALID | FLAG_DONE)).any()
    # the rows played before the injection (row 5 itself only where it was not overwritten)
    head = _replay(rec, 0, 5, 0, False)
    _assert_replay(rec, {k: v[:5] if k in ("boards", "flags") else v[:4] for k, v in head.items()}, 0, 4)
    assert np.array_equal(rec["boards"][5][~which], head["boards"][5][~which])
    assert np.array_equal(rec["points"][4], head["points"][4]) and np.array_equal(rec["pot"][4], head["pot"][4])
    c = _counts("ends mid-buffer", rp)
    assert c["resets"] == which.sum()


# ------------------------------------------------------------------ 3: dead at launch start ----
@pytest.mark.parametrize("episodic", [False, True])
def test_dead_board_at_launch_start(dev, episodic):
    """C (no legal move, flags[t0] = 0) in envs 0, 31 and 40, and a board with a single legal move in
    envs 1 and 32: the sampler's empty and one-action masks, the INVALID branch with legal == 0 and
    its reset, or -- episodic -- the inactive early return from the first step on."""
    n, T = 73, 6
    dead, one = [0, 31, 40], [1, 32]
    boards, which = _place(n, [(dead, C), (one, ONE)])
    rec, rp = _both(dev, _model(dev, 196, 31), n, T, episodic, _inject(boards, which))
    assert not rec["flags"][0][dead].any() and (rec["flags"][0][one] == 0b1000).all()
    # the sampler on an empty mask: action 0, entropy 0, four -inf; on a single action: that action
    assert not rec["actions"][0][dead].any() and not rec["entropy"][0][dead].any()
    assert np.isneginf(rec["logp"][0][dead]).all()
    assert (rec["actions"][0][one] == O.RIGHT).all() and not rec["entropy"][0][one].any()
    assert np.isneginf(rec["logp"][0][one][:, :3]).all() and (np.abs(rec["logp"][0][one][:, 3]) <= 1e-7).all()
    for k in ("points", "max_tile", "pot"):
        assert not rp[k][0][dead].any()
    if episodic:
        assert (rp["flags"][1:][:, dead] == (FLAG_INACTIVE | FLAG_DONE)).all()
        assert (rp["boards"][:, dead] == C).all() and (rec["boards"][:, dead] == C).all()
    else:
        fresh = O.reset(n, O.RNG_PHILOX, SEED, step_idx=COUNTER + 1)
        assert np.array_equal(rp["flags"][1][dead], FLAG_INVALID | FLAG_DONE | FLAG_RESET | O.legal_mask(fresh)[dead])
        assert np.array_equal(rp["boards"][1][dead], fresh[dead])
        assert not (rp["flags"][2:][:, dead] & (FLAG_INVALID | FLAG_DONE)).any()  # the game goes on
        assert (rp["boards"][2:][:, dead] != rp["boards"][1:-1][:, dead]).any(axis=2).all()
    _counts(f"dead at launch, episodic={episodic}", rp)
    rest = rp["flags"][1:][:, ~which]  # two-tile games: six steps cannot end them
    assert not (rest & (FLAG_DONE | FLAG_INACTIVE | FLAG_INVALID)).any()


# ------------------------------------------------------------------ 4: episodic tails ----------
def test_episodic_tails(dev):
    """D / DT in every fourth env: live at step 0, inactive at steps 1..11 (the early return every
    finished game of an episodic rollout takes); two-tile games cannot end within 12 steps."""
    n, T = 300, 12
    ends = np.arange(0, n, 4)
    boards, which = _place(n, [(ends[0::2], D), (ends[1::2], DT)])
    rec, rp = _both(dev, _model(dev, 64, 4), n, T, True, _inject(boards, which))
    fl = rp["flags"]
    assert (fl[1][which] == FLAG_DONE).all()
    assert (fl[2:][:, which] == (FLAG_INACTIVE | FLAG_DONE)).all()
    assert not (fl[1:][:, ~which] & (FLAG_INACTIVE | FLAG_DONE)).any()
    assert (rp["boards"][2:][:, which] == rp["boards"][1][which]).all()
    c = _counts("episodic tails", rp)
    assert c["inactive"] == len(ends) * (T - 1) == 825 and c["resets"] == 0


# ------------------------------------------------------------------ 5: high tiles --------------
def _high_tile_boards(n):
    b = random_boards(n, 500, hi=15, p_empty=0.3)
    pos = np.random.default_rng(5).integers(0, 3, n)
    for j in range(40):  # envs 0..31: two adjacent 15s, envs 32..39: two adjacent 16s
        i, v = j, 15 if j < 32 else 16
        if j % 2 == 0:  # in row j % 4
            r, c = j % 4, pos[j]
            b[i, 4 * r + c] = b[i, 4 * r + c + 1] = v
        else:  # in column j % 4
            c, r = j % 4, pos[j]
            b[i, 4 * r + c] = b[i, 4 * r + 4 + c] = v
    for j in range(32):  # the "max tie" boards: one tile of exponent 1 or 2 at each of the 16 cells
        b[64 + j] = 0
        b[64 + j, j % 16] = 1 + j // 16
    return b


def _spawn_cases(rp, actions):
    """Per step of the replay: the spawn's (cell, value) against the moved board's first maximum --
    counts of spawns above the maximum and of ties in front of it that change its corner status."""
    above = tie_moves = 0
    for t in range(len(actions)):
        moved, _, _ = O.move(rp["boards"][t], actions[t].astype(np.int64) & 3)
        ok = (rp["flags"][t + 1] & (FLAG_INVALID | FLAG_RESET | FLAG_INACTIVE)) == 0
        diff = rp["boards"][t + 1] != moved
        ok &= diff.sum(axis=1) == 1
        p = np.argmax(diff, axis=1)
        v = rp["boards"][t + 1][np.arange(len(p)), p]
        M = moved.max(axis=1)
        pos = np.argmax(moved == M[:, None], axis=1)
        corner = np.isin(np.arange(16), (0, 3, 12, 15))
        above += int((ok & (v > M)).sum())
        tie_moves += int((ok & (v == M) & (p < pos) & (corner[p] != corner[pos])).sum())
    return above, tie_moves


@pytest.mark.parametrize("h", [196, 128])
def test_high_tiles(dev, h):
    """Exponents up to 17: the maximum field (bits 24..31) of the carried statistics, the stem's obs
    fragments of large tiles, 65 536 and 131 072 points; and spawns that tie or exceed the maximum
    (mono_add_tile's pos).  h = 128 is the instantiation no other test runs."""
    n, T = 512, 24
    boards = _high_tile_boards(n)
    rec, rp = _both(dev, _model(dev, h, 50 + h), n, T, False, _inject(boards, np.ones(n, bool)))
    c = _counts(f"high tiles, h={h}", rp)
    above, tie_moves = _spawn_cases(rp, rec["actions"])
    print(f"high tiles, h={h}: spawns above the maximum {above}, ties that move pos across a corner {tie_moves}, "
          f"65536-point steps {int((rp['points'] == 65536).sum())}, 131072-point steps {int((rp['points'] == 131072).sum())}")
    assert (rp["boards"][1:] == 16).any() and (rp["max_tile"] == 16).any() and (rp["points"] == 65536).any()
    assert c["largest"] == 17 and (rp["max_tile"] == 17).any() and (rp["points"] == 131072).any()
    assert above > 0 and tie_moves > 0


# ------------------------------------------------------------------ 6: long mixed run ----------
@pytest.mark.parametrize("episodic", [False, True])
@pytest.mark.parametrize("h", [32, 196])
def test_long_mixed_run(dev, h, episodic):
    """256 steps from crowded small boards: the policy decides when games end, so the coverage is only
    'at least one'; scenarios 1-4 hold the guaranteed cases."""
    n, T = 512, 256
    boards = random_boards(n, 600 + h, hi=4, p_empty=0.2)
    rec, rp = _both(dev, _model(dev, h, 60 + h), n, T, episodic, _inject(boards, np.ones(n, bool)))
    c = _counts(f"long run, h={h}, episodic={episodic}", rp)
    assert c["inactive"] > 0 if episodic else c["resets"] > 0


# ------------------------------------------------------------------ 7: second pass -------------
def test_second_pass_of_persistent_loop(dev):
    """65 536 + 300 envs: 258 groups on the 256-workgroup grid, so workgroups 0 and 1 take a second
    group -- a full one, and the last with one full wave, a wave of 12 boards and six empty waves.
    D sits at both ends of both."""
    n, T = 65536 + 300, 3
    ends = [65536, 65791, 65792, n - 1]
    boards, which = _place(n, [(ends, D)])
    rec, rp = _both(dev, _model(dev, 196, 7), n, T, False, _inject(boards, which))
    ended = (rp["flags"][1] & ENDED) == ENDED
    assert np.nonzero(ended)[0].tolist() == ends
    assert not (rp["flags"][2:] & (FLAG_DONE | FLAG_INVALID)).any()
    c = _counts("second pass", rp)
    assert c["resets"] == 4


# ------------------------------------------------------------------ 8: saturated logits --------
def test_saturated_logits(dev):
    """action_head scaled by a further 50: logits hundreds apart.  sample_row against the float64
    reference on the logits FusedPolicy gives for the recorded boards."""
    from g2048 import _lib as L
    from g2048.rollout import FusedPolicy
    n, T = 256, 8
    m = _model(dev, 64, 8)
    with torch.no_grad():
        m.action_head.weight.mul_(50.0)
    rec, rp = _both(dev, m, n, T, False, None)
    pol = FusedPolicy(m)
    obs = torch.zeros(n, 48, dtype=torch.bfloat16, device=dev)
    excluded, gap_max = 0, 0.0
    for t in range(T):
        L.obs_encode(torch.from_numpy(rec["boards"][t]).to(dev), obs)
        logits = pol(obs)[0].cpu().numpy()
        legal = rp["flags"][t] & 0xF
        u32 = O.philox_draws(SEED, COUNTER + 2 * t, n, 1, 0)[:, 0]
        logp, ent, act, dist = sampler_reference(logits, legal, u32)
        fin = np.isfinite(logp)
        assert np.array_equal(np.isfinite(rec["logp"][t]), fin) and np.isneginf(rec["logp"][t][~fin]).all()
        np.testing.assert_allclose(rec["logp"][t][fin], logp[fin], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(rec["entropy"][t], ent, rtol=1e-5, atol=1e-5)
        far = dist > 1e-5
        assert np.array_equal(rec["actions"][t][far], act[far])
        assert ((legal >> rec["actions"][t]) & 1).all()
        excluded += int((~far).sum())
        gap_max = max(gap_max, float(-logp[fin].min()))
    print(f"saturated logits: excluded rows {excluded} of {n * T}, largest -logp of a legal action {gap_max:.1f}")
    assert gap_max > 104.0  # below fp32's smallest denormal: that action's exp is exactly 0
    _counts("saturated logits", rp)


# ------------------------------------------------------------------ sampler edges --------------
EDGE_SEED, EDGE_RNG = 3, (41, 6, 17)  # logit generator seed; Philox (seed, counter, env_base)
PATTERNS = ("zeros", "normal", "plus40", "spread300", "pm1e4", "equal_max", "ulp_max", "tiny_last")


def _edge_rows():
    """8 192 rows: 16 legal masks x 8 logit patterns x 64 draws."""
    g = np.random.default_rng(EDGE_SEED)
    n = 16 * 8 * 64
    r = np.arange(n)
    mask, pat = (r // 512).astype(np.uint8), (r // 64) % 8
    lg = np.zeros((n, 4), np.float32)
    for i in range(n):
        legal = [a for a in range(4) if (mask[i] >> a) & 1]
        p = PATTERNS[pat[i]]
        x = g.normal(size=4)
        if p == "zeros":
            x[:] = 0
        elif p == "normal":
            x *= 2.0
        elif p == "plus40":
            x[g.integers(4)] += 40.0
        elif p == "spread300":
            x = g.uniform(-300.0, 300.0, 4)
        elif p == "pm1e4":
            x = np.where(g.random(4) < 0.5, -1e4, 1e4)
        elif p in ("equal_max", "ulp_max"):
            pool = legal if len(legal) >= 2 else list(range(4))
            a, b = g.choice(pool, 2, replace=False)
            top = np.float32(x.max() + 1.0)
            x = x.astype(np.float32)
            x[a] = top
            x[b] = top if p == "equal_max" else np.nextafter(top, np.float32(np.inf))
        elif p == "tiny_last" and len(legal) >= 2:  # the last legal action below 2^-30
            x[legal[-1]] = max(x[a] for a in legal[:-1]) - 25.0
        lg[i] = x
    return lg, mask, pat


def _sample(dev, logits, mask, rng_args):
    from g2048 import _lib as L
    n = len(mask)
    fl = torch.from_numpy(mask).to(dev)
    act = torch.zeros(n, dtype=torch.uint8, device=dev)
    lp = torch.zeros(n, 4, dtype=torch.float32, device=dev)
    ent = torch.zeros(n, dtype=torch.float32, device=dev)
    L.sample_actions(logits, fl, act, lp, ent, L.make_rng(L.RNG_PHILOX, *rng_args))
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy(), ent.cpu().numpy()


@pytest.mark.parametrize("stride", [4, 8])
def test_sampler_edges(dev, stride):
    """g2048_sample_actions (sample_kernel, bitwise sample_row's code) on every legal mask x saturated,
    tied and vanishing logits, through a contiguous [n, 4] tensor and through columns 0..3 of an
    [n, 8] tensor whose other columns hold NaN."""
    lg, mask, pat = _edge_rows()
    n = len(mask)
    u32 = O.philox_draws(EDGE_RNG[0], EDGE_RNG[1], n, 1, EDGE_RNG[2])[:, 0]
    logp, ent, act, dist = sampler_reference(lg, mask, u32)
    far = dist > 1e-5
    print(f"sampler edges: excluded rows {int((~far & (mask != 0)).sum())} of {n}")
    assert (~far & (mask != 0)).sum() <= 8  # the cap: 4 boundaries x 2e-5 x 8 192 rows < 1 expected
    wide = torch.full((n, stride), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :4] = torch.from_numpy(lg).to(dev)
    view = wide[:, :4]
    assert view.stride(0) == stride
    a, lp, en = _sample(dev, view, mask, EDGE_RNG)
    ok = ((mask[:, None] >> np.arange(4)) & 1).astype(bool)
    assert np.array_equal(np.isfinite(lp), ok) and np.isneginf(lp[~ok]).all()
    np.testing.assert_allclose(lp[ok], logp[ok], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(en, ent, rtol=1e-5, atol=1e-5)
    single = ok.sum(axis=1) == 1
    assert (np.abs(lp[single][ok[single]]) <= 1e-7).all() and not en[single].any()
    none = mask == 0
    assert not a[none].any() and not en[none].any()
    assert ((mask[~none] >> a[~none]) & 1).all()
    sel = far & ~none
    assert np.array_equal(a[sel], act[sel]), (PATTERNS, np.bincount(pat[sel][a[sel] != act[sel]], minlength=8))


def test_sampler_null_logits_uniform(dev):
    """logits == NULL: uniform over the legal actions, 2^18 rows per mask, each frequency within 4
    sigma of 1 / (number of legal actions)."""
    n = 1 << 18
    for j, mask in enumerate((0b1111, 0b1011, 0b0110)):
        a, lp, en = _sample(dev, None, np.full(n, mask, np.uint8), (51 + j, 2, 0))
        k = bin(mask).count("1")
        freq = np.bincount(a, minlength=4) / n
        sigma = np.sqrt((1 / k) * (1 - 1 / k) / n)
        print(f"NULL logits, mask {mask:04b}: frequencies {freq.tolist()}, 4 sigma {4 * sigma:.2e}")
        for act in range(4):
            if (mask >> act) & 1:
                assert abs(freq[act] - 1 / k) <= 4 * sigma
                np.testing.assert_allclose(lp[:, act], -np.log(k), rtol=1e-5, atol=1e-5)
            else:
                assert freq[act] == 0 and np.isneginf(lp[:, act]).all()
        np.testing.assert_allclose(en, np.log(k), rtol=1e-5, atol=1e-5)
