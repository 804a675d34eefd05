"""CPU pins of tests/rollout_reference.py, the checker of test_gpu_policy_rollout_edges.py: replay()
on the constructed boards (every legal move of D / DT ends the game, C has no legal move) in both
rollout modes, and sampler_reference() against the oracle's masked_policy on the reference's golden
rows."""

import numpy as np
import pytest

from conftest import golden
from oracle import oracle as O
from rollout_reference import (C, D, DT, FLAG_DONE, FLAG_INACTIVE, FLAG_INVALID, FLAG_RESET, OPT_AUTO_RESET,
                               OPT_SKIP_DONE, replay, sampler_reference)

SEEDS = range(8)
N = 64


def test_constructed_boards():
    assert O.legal_mask(np.stack([D, DT, C])).tolist() == [0b1100, 0b0011, 0]
    assert np.array_equal(DT.reshape(4, 4), D.reshape(4, 4).T)


@pytest.mark.parametrize("board,acts", [(D, (O.LEFT, O.RIGHT)), (DT, (O.UP, O.DOWN))])
def test_every_legal_move_of_d_ends_the_game_and_resets(board, acts):
    """8 seeds x 64 envs reach both spawn values at every cell the move empties; with OPT_AUTO_RESET the
    next board is O.reset's at the step's own counter, the flags DONE | RESET | its legal mask."""
    cells, vals = set(), set()
    for seed in SEEDS:
        for a in acts:
            b0 = np.tile(board, (N, 1))
            act = np.full((3, N), a, np.uint8)
            act[1:] = O.UP
            nb, f, _, moved = O.step(b0, a, O.RNG_PHILOX, seed, step_idx=5 + 1, env_base=11)
            assert f["done"].all() and not f["invalid"].any() and (f["points"] == 64).all()
            spawn = np.argmax(nb != moved, axis=1)
            cells |= set(spawn.tolist())
            vals |= set(nb[np.arange(N), spawn].tolist())
            boards, flags, points, max_tile, pot = replay(b0, act, seed, 5, 11, OPT_AUTO_RESET)
            fresh = O.reset(N, O.RNG_PHILOX, seed, step_idx=6, env_base=11)
            assert np.array_equal(boards[1], fresh)
            assert np.array_equal(flags[1], FLAG_DONE | FLAG_RESET | O.legal_mask(fresh))
            assert (points[0] == 64).all() and (max_tile[0] == 6).all()
            assert np.array_equal(pot[0, :, 0], O.potentials(b0)[0]) and (pot[0, :, 2] == 0).all()
            assert (pot[0, :, 3] == 1).all()  # one merge: one empty cell before the spawn
            # the game goes on from the fresh board: step 1 is O.step on it at the next step's counter
            nb1, f1, _, _ = O.step(fresh, act[1], O.RNG_PHILOX, seed, step_idx=8, env_base=11)
            assert np.array_equal(boards[2], nb1) and np.array_equal(points[1], f1["points"])
            assert np.array_equal(flags[2] & FLAG_INVALID != 0, f1["invalid"].astype(bool))
            # episodic: the finished board stays, every later step is inactive
            boards, flags, points, max_tile, pot = replay(b0, act, seed, 5, 11, OPT_SKIP_DONE)
            assert np.array_equal(boards[1], nb) and (flags[1] == FLAG_DONE).all()
            assert (flags[2:] == (FLAG_INACTIVE | FLAG_DONE)).all()
            assert np.array_equal(boards[2], nb) and np.array_equal(boards[3], nb)
            assert not points[1:].any() and not max_tile[1:].any() and not pot[1:].any()
    assert len(cells) == 2 and vals == {1, 2}  # LEFT and RIGHT (UP and DOWN) empty one cell each


def test_checkerboard_is_invalid_done_then_reset():
    b0 = np.tile(C, (N, 1))
    act = np.zeros((2, N), np.uint8)
    boards, flags, points, max_tile, pot = replay(b0, act, 3, 1, 0, OPT_AUTO_RESET)
    fresh = O.reset(N, O.RNG_PHILOX, 3, step_idx=2, env_base=0)
    assert (flags[0] == 0).all()
    assert np.array_equal(boards[1], fresh)
    assert np.array_equal(flags[1], FLAG_INVALID | FLAG_DONE | FLAG_RESET | O.legal_mask(fresh))
    assert not points[0].any() and not max_tile[0].any() and not pot[0].any()
    assert not (flags[2] & FLAG_DONE).any()  # the fresh game goes on
    # no option: the no-op with invalid = done = 1, again and again
    boards, flags, _, _, pot = replay(b0, act, 3, 1, 0, 0)
    assert (boards == C).all() and (flags[1:] == (FLAG_INVALID | FLAG_DONE)).all() and not pot.any()
    # episodic: inactive from the first step
    boards, flags, _, _, _ = replay(b0, act, 3, 1, 0, OPT_SKIP_DONE)
    assert (boards == C).all() and (flags[1:] == (FLAG_INACTIVE | FLAG_DONE)).all()


def test_illegal_action_is_a_noop_with_invalid():
    b0 = np.tile(D, (4, 1))
    boards, flags, points, _, pot = replay(b0, np.full((1, 4), O.UP, np.uint8), 1, 1, 0, OPT_AUTO_RESET)
    assert (boards[1] == D).all() and (flags[1] == (FLAG_INVALID | 0b1100)).all()
    assert not points.any() and not pot.any()


def test_high_tile_merges():
    b0 = np.zeros((2, 16), np.int8)
    b0[0, :2] = 15
    b0[1, :2] = 16
    _, _, points, max_tile, _ = replay(b0, np.full((1, 2), O.LEFT, np.uint8), 1, 1, 0, OPT_AUTO_RESET)
    assert points[0].tolist() == [65536, 131072] and max_tile[0].tolist() == [16, 17]


def test_sampler_reference_equals_masked_policy_on_golden_rows():
    g = golden("sampler.npz")
    n = len(g["logits"])
    legal = (~g["invalid"] * (1 << np.arange(4))).sum(axis=1).astype(np.uint8)
    u32 = O.philox_draws(77, 12, n, 1, env_base=5)[:, 0]
    logp, ent, act, dist = sampler_reference(g["logits"], legal, u32)
    p, e, lp = O.masked_policy(g["logits"], g["invalid"])
    assert np.array_equal(np.isfinite(logp), ~g["invalid"])
    fin = ~g["invalid"]
    np.testing.assert_allclose(logp[fin], lp[fin], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ent, e, rtol=0, atol=1e-12)
    # and the reference's own fp32 rows
    np.testing.assert_allclose(logp[fin], g["logp"][fin], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ent, g["entropy"], rtol=1e-5, atol=1e-5)
    # the action: inverse CDF of masked_policy's probabilities; dist = the distance to its boundaries
    u = (u32 >> 8).astype(np.float64) / 2 ** 24
    cdf = np.cumsum(p, axis=1)
    assert np.array_equal(act, np.argmax(u[:, None] < cdf, axis=1))
    assert ((legal >> act) & 1).all()
    np.testing.assert_allclose(dist, np.where(fin, np.abs(cdf - u[:, None]), np.inf).min(axis=1), rtol=0, atol=1e-12)


def test_sampler_reference_edges():
    lg = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [5, 5, 5, 5], [0, 1e4, -1e4, 0], [0, 0, 0, 0]], np.float64)
    legal = np.array([0, 0b0100, 0b1010, 0b0111, 0b1111], np.uint8)
    u32 = np.array([123, 0xFFFFFFFF, 0x7FFFFF00, 0xFFFFFFFF, 0x80000000], np.uint32)
    logp, ent, act, dist = sampler_reference(lg, legal, u32)
    assert np.isneginf(logp[0]).all() and ent[0] == 0 and act[0] == 0 and np.isinf(dist[0])
    assert logp[1, 2] == 0 and np.isneginf(logp[1, [0, 1, 3]]).all() and ent[1] == 0 and act[1] == 2
    assert np.allclose(logp[2, [1, 3]], np.log(0.5)) and np.isclose(ent[2], np.log(2)) and act[2] == 1
    assert logp[3, 1] == 0 and logp[3, 2] == -2e4 and ent[3] == 0 and act[3] == 1
    assert act[4] == 2 and dist[4] == 0  # u = 0.5 sits on the boundary after action 1: u < cdf is strict
    lp0, e0, a0, _ = sampler_reference(None, legal, u32)
    assert np.isclose(e0[3], np.log(3)) and np.allclose(lp0[4], np.log(0.25))
