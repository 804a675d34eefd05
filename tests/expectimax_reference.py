"""CPU reference of the exact expectimax search (g2048_expectimax, g2048/search.py's ExpectimaxPlayer),
level by level in numpy and built only from oracle functions: O.move (the move, its points and -- as
move(b, a) != b -- its legality), O.potentials (the leaf) and O.legal_mask (the legal output).  All
values are int64 with 16 fractional bits, as include/g2048.h defines them.  Shared by
tests/test_expectimax_host.py and tests/test_gpu_expectimax.py; not a test module itself."""

import numpy as np

from oracle import oracle as O

S = 65536
WEIGHTS = (1, 64, 128)
CROWDED = [2, 4, 6, 9, 13, 14, 25, 27]  # the roots of mc_reference.roots() that depth 4 is run on


def _expand(boards, k, w, stats):
    """The four moves of every board [m, 16] with k moves left to look ahead -> (value int64 [m, 4]
    = S w_points pts + A(moved, k - 1), -1 for an illegal move; leaves int64 [m, 4])."""
    m = len(boards)
    val = np.full(4 * m, -1, np.int64)
    lv = np.zeros(4 * m, np.int64)
    if m:
        rep = np.repeat(boards, 4, axis=0)
        moved, pts, _ = O.move(rep, np.tile(np.arange(4), m))
        legal = (moved != rep).any(1)
        if legal.any():
            a, l = _chance(moved[legal], k - 1, w, stats)
            val[legal] = S * w[0] * pts[legal].astype(np.int64) + a
            lv[legal] = l
    return val.reshape(m, 4), lv.reshape(m, 4)


def _max(boards, k, w, stats):
    """M(b, k) of the boards [m, 16] (after a spawn) -> (M int64 [m], leaves int64 [m])."""
    val, lv = _expand(boards, k, w, stats)
    stats["dead"] += int((val < 0).all(1).sum())
    return np.maximum(val.max(1, initial=0), 0), lv.sum(1)


def _chance(after, k, w, stats):
    """A(s, k) of the after-states [m, 16] -> (A int64 [m], leaves int64 [m])."""
    m = len(after)
    if k == 0:
        mono, empt = O.potentials(after)
        stats["leaves"] += m
        return S * (w[1] * mono.astype(np.int64) + w[2] * empt.astype(np.int64)), np.ones(m, np.int64)
    idx, cell = np.nonzero(after == 0)
    E = np.bincount(idx, minlength=m).astype(np.int64)
    assert (E >= 1).all()  # a legal move leaves an empty cell
    owner = np.repeat(idx, 2)
    child = after[owner].copy()
    child[np.arange(len(child)), np.repeat(cell, 2)] = np.tile(np.array([1, 2], np.int8), len(idx))
    mv, lv = _max(child, k, w, stats)
    num = np.zeros(m, np.int64)
    np.add.at(num, owner, np.tile(np.array([9, 1], np.int64), len(idx)) * mv)
    leaves = np.zeros(m, np.int64)
    np.add.at(leaves, owner, lv)
    return num // (10 * E), leaves


def expectimax_ref(boards, depth, weights=WEIGHTS, stats=None):
    """-> (value int64 [n, 4], leaves int64 [n, 4]) of g2048_expectimax.  stats (optional dict) receives
    "leaves" (A(., 0) evaluations), "dead" (nodes with M = 0: boards without a legal move, finished
    roots included) and "dead_roots" (the finished roots among them)."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    w = tuple(int(x) for x in weights)
    assert 1 <= depth <= 4 and all(0 <= x <= 4096 for x in w)
    st = {"leaves": 0, "dead": 0}
    val, lv = _expand(boards, depth, w, st)
    st["dead_roots"] = int((val < 0).all(1).sum())
    st["dead"] += st["dead_roots"]
    if stats is not None:
        stats.update(st)
    return val, lv


def legal_best(boards, value):
    """-> (legal uint8 [n] bits 0-3, best uint8 [n]: the legal action of the largest value, the lowest
    index among equals, 0xFF without a legal action)."""
    legal = O.legal_mask(boards)
    ok = value >= 0
    assert np.array_equal(legal, (ok * (1 << np.arange(4))).sum(1).astype(np.uint8))  # move(b, a) != b
    best = np.where(ok.any(1), value.argmax(1), 0xFF).astype(np.uint8)
    return legal, best


def cpu_play(num_games, depth, max_moves, game_seed, weights=WEIGHTS):
    """ExpectimaxPlayer.play_games on Philox games with the oracle: reset at counter 0, move m stepped
    at counter m + 1.  -> (scores, moves, boards)."""
    boards = O.reset(num_games, seed=game_seed, step_idx=0)
    scores = np.zeros(num_games, np.int64)
    moves = np.zeros(num_games, np.int64)
    for m in range(max_moves):
        active = O.legal_mask(boards) != 0
        if not active.any():
            break
        val, _ = expectimax_ref(boards, depth, weights)
        _, best = legal_best(boards, val)
        b2, f, _, _ = O.step(boards, np.where(active, best, 0), seed=game_seed, step_idx=m + 1)
        boards = np.where(active[:, None], b2, boards)
        scores += np.where(active, f["points"], 0)
        moves += active
    return scores, moves, boards
