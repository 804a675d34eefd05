"""CPU reference of the n-tuple expectimax search (g2048_ntuple_search of include/g2048_ntuple.h,
g2048/ntuple.py's NTuplePlayer with depth >= 2), level by level in numpy and built only from O.move (the
move, its points and -- as move(b, a) != b -- its legality), O.legal_mask (the legal output) and
ntuple_reference.value (the leaf).  All values are int64 in points x 4096 and signed: INT64_MIN marks an
illegal action, the maximum runs over the legal moves only, a board without one is worth 0, and the one
division of a chance node is numpy's //, the floor towards minus infinity.  Shared by
tests/test_ntuple_search_host.py and tests/test_gpu_ntuple_search.py; not a test module itself."""

import numpy as np

import ntuple_reference as R
from oracle import oracle as O

S = R.S
I64_MIN = R.I64_MIN
WEIGHT_SEED = 7  # the 32-bit random weights of the search tests: R.random_weights(cells, 7, bits=32)
# (net, weight seed) of the bit-exact GPU test.  Under seed 7 the 16 weights of t1k1 give no negative
# chance sum at all and t2k6 no root q at depth 3 that a truncating division would change, so these two
# nets run a second time under seed 8, where every depth has such a root (test_ntuple_search_host.py).
GPU_CASES = [("lines-squares-4", 7), ("t1k1", 7), ("t8k3", 7), ("t2k6", 7), ("t1k1", 8), ("t2k6", 8)]


def _div(num, den, floor):
    """num // den; floor = False: C's truncating division instead (what the kernel must NOT do)."""
    if floor:
        return num // den
    return np.sign(num) * (np.abs(num) // den)


def _expand(boards, k, net, stats, floor):
    """The four moves of every board [m, 16] with k moves left to look ahead -> (q int64 [m, 4]
    = S pts + A(moved, k - 1), INT64_MIN for an illegal move; leaves int64 [m, 4])."""
    m = len(boards)
    val = np.full(4 * m, I64_MIN, np.int64)
    lv = np.zeros(4 * m, np.int64)
    if m:
        rep = np.repeat(boards, 4, axis=0)
        moved, pts, _ = O.move(rep, np.tile(np.arange(4), m))
        legal = (moved != rep).any(1)
        if legal.any():
            a, l = _chance(moved[legal], k - 1, net, stats, floor)
            val[legal] = S * pts[legal].astype(np.int64) + a
            lv[legal] = l
    return val.reshape(m, 4), lv.reshape(m, 4)


def _max(boards, k, net, stats, floor):
    """M(b, k) of the boards [m, 16] (after a spawn) -> (M int64 [m], leaves int64 [m]): the maximum over
    the legal moves, 0 for a board without one."""
    val, lv = _expand(boards, k, net, stats, floor)
    dead = (val == I64_MIN).all(1)
    stats["dead"] += int(dead.sum())
    return np.where(dead, 0, val.max(1, initial=I64_MIN)), lv.sum(1)


def _chance(after, k, net, stats, floor):
    """A(s, k) of the after-states [m, 16] -> (A int64 [m], leaves int64 [m])."""
    m = len(after)
    if k == 0:
        stats["leaves"] += m
        return R.value(net[0], net[1], after), np.ones(m, np.int64)
    idx, cell = np.nonzero(after == 0)
    E = np.bincount(idx, minlength=m).astype(np.int64)
    assert (E >= 1).all()  # a legal move leaves an empty cell
    owner = np.repeat(idx, 2)
    child = after[owner].copy()
    child[np.arange(len(child)), np.repeat(cell, 2)] = np.tile(np.array([1, 2], np.int8), len(idx))
    mv, lv = _max(child, k, net, stats, floor)
    num = np.zeros(m, np.int64)
    np.add.at(num, owner, np.tile(np.array([9, 1], np.int64), len(idx)) * mv)
    leaves = np.zeros(m, np.int64)
    np.add.at(leaves, owner, lv)
    stats["neg_nondiv"] += int(((num < 0) & (num % (10 * E) != 0)).sum())
    stats["max_abs_sum"] = max(stats["max_abs_sum"], int(np.abs(num).max()))
    return _div(num, 10 * E, floor), leaves


def search_ref(cells, weights, boards, depth, stats=None, floor=True):
    """-> (q int64 [n, 4], leaves int64 [n, 4], legal uint8 [n], best uint8 [n]) of g2048_ntuple_search.
    stats (optional dict) receives "leaves" (A(., 0) evaluations), "dead" (inner boards without a legal
    move, M = 0; the finished roots are not counted), "neg_nondiv" (chance nodes whose sum is negative and
    not divisible by 10 E: where a truncating division differs) and "max_abs_sum" (the largest |sum|)."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    assert 1 <= depth <= 3
    st = {"leaves": 0, "dead": 0, "neg_nondiv": 0, "max_abs_sum": 0}
    q, lv = _expand(boards, depth, (cells, np.asarray(weights)), st, floor)
    ok = q != I64_MIN
    legal = (ok * (1 << np.arange(4))).sum(1).astype(np.uint8)
    assert np.array_equal(legal, O.legal_mask(boards))
    best = np.where(ok.any(1), q.argmax(1), 0xFF).astype(np.uint8)  # argmax: the lowest index among equals
    if stats is not None:
        stats.update(st)
    return q, lv, legal, best


def cpu_play(cells, weights, depth, num_games, max_moves, game_seed):
    """NTuplePlayer(net, depth).play_games on Philox games with the oracle: reset at counter 0, move m
    stepped at counter m + 1.  -> (scores, moves, boards)."""
    boards = O.reset(num_games, seed=game_seed, step_idx=0)
    scores = np.zeros(num_games, np.int64)
    moves = np.zeros(num_games, np.int64)
    for m in range(max_moves):
        active = O.legal_mask(boards) != 0
        if not active.any():
            break
        _, _, _, best = search_ref(cells, weights, boards, depth)
        b2, f, _, _ = O.step(boards, np.where(active, best, 0), seed=game_seed, step_idx=m + 1)
        boards = np.where(active[:, None], b2, boards)
        scores += np.where(active, f["points"], 0)
        moves += active
    return scores, moves, boards
