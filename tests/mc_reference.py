"""CPU reference of the Monte-Carlo playout search (g2048_mc_search, g2048/search.py), composed of
oracle functions only: the policy-action step (O.step) and the random rollout's word-per-step record
(O.random_rollout_record).  Shared by tests/test_gpu_mc_search.py; not a test module itself."""

import numpy as np

from conftest import golden
from oracle import oracle as O


def mc_ref_lanes(boards, P, D, seed, ctr, env_base=0, stepped_max=False):
    """Per lane L = (4 i + a) P + p: (points, playout moves, invalid forced move, alive after it);
    with stepped_max also [D, lanes]: the largest exponent of the board the lane steps at playout step
    t, -1 where it steps none (an invalid forced move, or its playout is over)."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    n = len(boards)
    rep = np.repeat(boards, 4 * P, axis=0)
    acts = np.tile(np.repeat(np.arange(4), P), n)
    b1, f, _, _ = O.step(rep, acts, seed=seed, step_idx=ctr, env_base=env_base)
    invalid = f["invalid"].astype(bool)
    alive = (O.legal_mask(b1) != 0) & ~invalid
    if D == 0:
        res = (np.where(invalid, 0, f["points"]).astype(np.int64), np.zeros(len(rep), np.int64), invalid, alive)
        return res + (np.zeros((0, len(rep)), np.int64),) if stepped_max else res
    _, rec = O.random_rollout_record(b1.copy(), D, seed, step0=ctr, env_base=env_base)
    done = (rec["flags"] & 0x80) != 0
    first = np.where(done.any(0), done.argmax(0), D - 1)
    m = (np.arange(D)[:, None] <= first[None, :]) & alive[None, :]
    pts = np.where(invalid, 0, f["points"] + (rec["points"].astype(np.int64) * m).sum(0))
    res = (pts.astype(np.int64), m.sum(0).astype(np.int64), invalid, alive)
    if stepped_max:
        res += (np.where(m, rec["boards"].reshape(D, len(rep), 16).max(2).astype(np.int64), -1),)
    return res


def mc_ref(boards, P, D, seed, ctr, env_base=0):
    """-> (score_sum [n, 4], move_sum [n, 4], invalid [n, 4]) of g2048_mc_search."""
    pts, moves, invalid, _ = mc_ref_lanes(boards, P, D, seed, ctr, env_base)
    n = len(pts) // (4 * P)
    return pts.reshape(n, 4, P).sum(2), moves.reshape(n, 4, P).sum(2), invalid.reshape(n, 4, P)[:, :, 0]


def legal_best(score_sum, invalid):
    """-> (legal uint8 [n] bits 0-3, best uint8 [n]: the legal action of the largest sum, lowest index
    among equals, 0xFF without a legal action)."""
    ok = ~invalid
    legal = (ok * (1 << np.arange(4))).sum(1).astype(np.uint8)
    masked = np.where(ok, score_sum, np.iinfo(np.int64).min)
    best = np.where(ok.any(1), masked.argmax(1), 0xFF).astype(np.uint8)
    return legal, best


def roots():
    """The 30 root boards: 16 mid-game boards, 8 finished ones, 6 of the best game (up to 2^11)."""
    g = golden("games.npz")
    last = [np.nonzero(g["game"] == k)[0][-1] for k in range(8)]
    bg = golden("best_game.npz")["before"][[0, 300, 900, 1200, 1240, 1248]]
    return np.ascontiguousarray(np.concatenate([g["before"][::400][:16], g["after"][last], bg]).astype(np.int8))


def cpu_play(num_games, P, D, max_moves, game_seed, seed=0x2048, env_base=0):
    """MonteCarloPlayer.play_games on Philox games with the oracle: reset at counter 0, move m searched
    at counter m max(D, 1) and stepped at counter m + 1.  -> (scores, moves, boards)."""
    boards = O.reset(num_games, seed=game_seed, step_idx=0)
    scores = np.zeros(num_games, np.int64)
    moves = np.zeros(num_games, np.int64)
    for m in range(max_moves):
        active = O.legal_mask(boards) != 0
        if not active.any():
            break
        sc, _, inv = mc_ref(boards, P, D, seed, m * max(D, 1), env_base)
        _, best = legal_best(sc, inv)
        b2, f, _, _ = O.step(boards, np.where(active, best, 0), seed=game_seed, step_idx=m + 1)
        boards = np.where(active[:, None], b2, boards)
        scores += np.where(active, f["points"], 0)
        moves += active
    return scores, moves, boards
