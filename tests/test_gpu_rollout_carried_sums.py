"""GPU parity of env_rollout_kernel's carried line sums (rollout_step.hpp): a step keeps, of the second
words of the eight line records it loads, only their sum and their unsigned maximum per orientation, and
the next step takes its points (bits 16..27 of the chosen sum) and the moved board's maximum (the top
nibble of the chosen maximum) from those four words; a game that ends takes the four words of its new
board from the kFresh pair.  Every case is compared bit for bit with oracle.random_rollout_record in all
five records and the final boards, from an even and an odd counter (the odd one peels a first step in
the other pair's form).

  extremes of the points sum   64 and 150 boards, 4 to 8 steps: sixteen 2^8 tiles on every board (the fast
      pair: 4 096 points in the first step, 2^9 pairs in the second); the same with one board per wave of
      sixteen 2^9 tiles (the other pair, table lanes beside it); sixteen 2^10 tiles (the sum that would
      leave its twelve bits: those lanes move on the SWAR path); three rows of 2^10 over a row of 2^9 and
      the transpose (the largest sum that stays inside); a 2^11 tile (a SWAR lane before and after).
  pair-kind changes   waves of fresh boards with boards at 2^8, 2^9 and 2^10 between them, 8 steps: the
      reference's own record says which waves start a pair with every board <= 2^8, and at least one wave
      leaves the fast pair and one enters it during the run, with the four words live.
  resets   boards one move from the end between fresh ones, 6 steps: the four words come from kFresh
      under a partial mask, on the even and on the odd step of a pair.
  coverage   2 048 boards x 512 steps: thousands of resets, most of the 480 fresh boards, and more than a
      thousand first moves after a reset that score (the kFresh points field, not only its zero).
  launch start   0- and 1-step launches from finished boards: the new game comes from fresh_from_words
      and its four words from refill_lines.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
DTYPE = {"boards": ((16,), torch.int8), "actions": ((), torch.uint8), "points": ((), torch.int32),
         "pot": ((4,), torch.int8), "flags": ((), torch.uint8)}
SEED, ENV_BASE = 0x18A, 5
GUARD = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def launch(dev, init, steps, step0, rows=None):
    """One launch of `steps` steps into sentinel-filled records of `rows` rows; (final boards, records)."""
    n = len(init)
    rows = steps if rows is None else rows
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    rec = {}
    for k, (tail, dt) in DTYPE.items():
        raw = torch.full((rows * n * int(np.prod(tail, dtype=np.int64)) * dt.itemsize,), GUARD, dtype=torch.uint8, device=dev)
        rec[k] = raw.view(dt).view((rows, n) + tail)
    L().env_rollout_random(b, steps, *(rec[k] for k in FIELDS), L().make_rng(L().RNG_PHILOX, SEED, step0, ENV_BASE))
    torch.cuda.synchronize()
    return b.cpu().numpy(), {k: rec[k].cpu().numpy() for k in FIELDS}


def check(dev, init, steps, step0, expect=None):
    ob, want = expect if expect is not None else O.random_rollout_record(init, steps, SEED, step0=step0, env_base=ENV_BASE)
    boards, got = launch(dev, init, steps, step0)
    for k in FIELDS:
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(bad), bad[:4].tolist())
    assert np.array_equal(boards, ob), "final boards"


def fresh_boards(rng, n):
    b = np.zeros((n, 16), np.int8)
    for i in range(n):
        b[i, rng.choice(16, 2, replace=False)] = rng.integers(1, 3, 2)
    return b


# ---------------------------------------------------------------- extremes of the points sum ----
def extreme_boards(kind, n):
    b = np.full((n, 16), 8, np.int8)
    if kind == "all_256":
        pass
    elif kind == "one_512_per_wave":
        for w in range(0, n, 64):
            b[w + 7 * (w // 64 + 1) % min(64, n - w)] = 9
    elif kind == "all_1024":
        b[:] = 10
    elif kind == "three_rows_1024":
        rows = np.array([10] * 12 + [9] * 4, np.int8)
        b[0::2] = rows
        b[1::2] = rows.reshape(4, 4).T.reshape(16)
    elif kind == "tile_2048":
        rng = np.random.default_rng(SEED + n)
        b = rng.integers(0, 11, size=(n, 16)).astype(np.int8)
        b[np.arange(n), rng.integers(0, 16, n)] = 11
        b[0::3] = 10          # sixteen 2^10 tiles: the move makes 2^11 tiles
        b[1::3, :8] = 11      # and pairs of 2^11
    else:
        raise KeyError(kind)
    return b


EXTREMES = [("all_256", 4), ("one_512_per_wave", 6), ("all_1024", 5), ("three_rows_1024", 7), ("tile_2048", 8)]


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("n", [64, 150])
@pytest.mark.parametrize("kind,steps", EXTREMES)
def test_extremes_of_the_points_sum(dev, kind, steps, n, step0):
    init = extreme_boards(kind, n)
    ob, want = O.random_rollout_record(init, steps, SEED, step0=step0, env_base=ENV_BASE)
    # the case is what its name says: the first move of a full board of equal tiles merges all eight pairs
    if kind == "all_256":
        assert (want["points"][0] == 8 * 512).all() and want["points"][1].max() >= 2 * 1024
    if kind == "one_512_per_wave":
        assert [int((init[w:w + 64].max(axis=1) == 9).sum()) for w in range(0, n, 64)] == [1] * len(range(0, n, 64))
        assert (want["points"][0] == 8 * 512).sum() == n - len(range(0, n, 64)) and (want["points"][0] == 8 * 1024).sum() == len(range(0, n, 64))
    if kind == "all_1024":
        assert (want["points"][0] == 8 * 2048).all()  # points / 4 = 4 096: one more than the field holds
    if kind == "three_rows_1024":
        # along the 2^10 lines 3 x 2 merges of 2^10 pairs and 2 of 2^9 pairs (points / 4 = 3 584, the
        # largest sum a table lane ... would form; these lanes are at 2^10 and move on the SWAR path),
        # across them one merge per line
        assert set(np.unique(want["points"][0]).tolist()) == {6 * 2048 + 2 * 1024, 4 * 2048}
    if kind == "tile_2048":
        assert (init.max(axis=1) >= 10).all() and want["boards"].max() >= 12
    check(dev, init, steps, step0, (ob, want))


# ---------------------------------------------------------------- pair-kind changes -------------
PAIR_N, PAIR_STEPS = 64 * 11 + 22, 8
END = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3], np.int8)  # one merge left, then most likely none


@functools.lru_cache(maxsize=None)
def pair_boards():
    """Waves 0, 1: fresh boards and boards with two 2^8 tiles in opposite corners, which take at least two
    moves to merge (the wave starts in the fast pair from either counter and leaves it when a pair
    merges).  Wave 2: fresh boards and boards at 2^8, 2^9 and 2^10 (the other pair throughout).  Waves
    3 .. 11: fresh boards and one board at 2^9 or 2^10 that is one move from the likely end of its game
    (the wave enters the fast pair once it has ended)."""
    rng = np.random.default_rng(SEED + 77)
    b = fresh_boards(rng, PAIR_N)
    for i in range(0, 128, 11):
        r = np.zeros(16, np.int8)
        r[[0, 15] if i % 2 else [3, 12]] = 8
        r[rng.choice(np.arange(4, 12), 2, replace=False)] = rng.integers(1, 3, 2)
        b[i] = r
    for i in range(128, 192, 3):
        r = rng.integers(0, 9, 16).astype(np.int8)
        r[rng.random(16) < 0.3] = 0
        r[rng.choice(16, 2, replace=False)] = (8, 9, 10)[i % 3]
        r[rng.integers(0, 16)] = (8, 9, 10)[(i // 3) % 3]
        b[i] = r
    for w in range(3, 12):
        e = END.reshape(4, 4).T.reshape(16).copy() if w % 2 == 0 else END.copy()
        e[0] = 9 + w % 3 % 2
        b[64 * w + w] = e
    return b


def fast_pairs(boards_rec, step0):
    """[pairs, waves]: every board of the wave <= 2^8 at the first step of a whole pair of the run"""
    starts = [t for t in range(len(boards_rec) - 1) if (step0 + t) % 2 == 0]
    return np.array([[boards_rec[t, w:w + 64].max() <= 8 for w in range(0, boards_rec.shape[1], 64)] for t in starts])


@pytest.mark.parametrize("step0", [0, 1])
def test_pair_kind_changes(dev, step0):
    init = pair_boards()
    ob, want = O.random_rollout_record(init, PAIR_STEPS, SEED, step0=step0, env_base=ENV_BASE)
    fast = fast_pairs(want["boards"], step0)
    leaves = (fast[:-1] & ~fast[1:]).any(axis=0)
    enters = (~fast[:-1] & fast[1:]).any(axis=0)
    print("fast pairs by wave:", fast.T.astype(int).tolist())
    assert fast[0, :2].all() and leaves[:2].any() and enters[3:].any(), (leaves.tolist(), enters.tolist())
    assert not fast[:, 2].any()  # wave 2 holds 2^9 / 2^10 boards to the end
    check(dev, init, PAIR_STEPS, step0, (ob, want))


# ---------------------------------------------------------------- resets ------------------------
@functools.lru_cache(maxsize=None)
def ending_boards(n):
    """Every third board is one move from (most likely) the end of its game: a full board whose only merge
    is the pair of 8s at the end of the last row, or the transpose (the pair in the last column); the
    move leaves one empty cell, and a spawned 2 there, nine times in ten, leaves no move.  The rest are
    fresh boards of two tiles."""
    rng = np.random.default_rng(SEED + 1000 + n)
    b = np.zeros((n, 16), np.int8)
    for i in range(n):
        if i % 3 == 0:
            b[i] = END if i % 2 == 0 else END.reshape(4, 4).T.reshape(16)
        else:
            c = rng.choice(16, 2, replace=False)
            b[i, c] = rng.integers(1, 3, 2)
    return b


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("n", [64, 150])
def test_resets(dev, n, step0):
    steps = 6
    init = ending_boards(n)
    ob, want = O.random_rollout_record(init, steps, SEED, step0=step0, env_base=ENV_BASE)
    reset = (want["flags"] & L().FLAG_RESET) != 0
    for w in range(0, n - 63, 64):  # every whole wave ends some games in the first step and plays on in others
        assert 3 <= reset[0, w:w + 64].sum() < 64, w
    check(dev, init, steps, step0, (ob, want))


COVER_N, COVER_STEPS = 2048, 512


def test_reset_coverage(dev):
    """2 048 boards x 512 steps from counter 0.  From the reference's own records: the run restarts
    thousands of games, on at least 380 distinct fresh boards (of the 480 there are), and at least 1 000 of
    the first moves after a restart score -- the kFresh word's points and maximum fields at work, in both
    orientations.  Then everything is equal."""
    init = O.reset(COVER_N, seed=0x2048)
    ob, want = O.random_rollout_record(init, COVER_STEPS, SEED, step0=0, env_base=ENV_BASE)
    t, i = np.nonzero((want["flags"][:-1] & L().FLAG_RESET) != 0)
    fresh = want["boards"][t + 1, i]
    assert ((fresh != 0).sum(axis=1) == 2).all() and fresh.max() <= 2
    distinct = len(np.unique(fresh, axis=0))
    first = want["points"][t + 1, i]
    scoring = int((first > 0).sum())
    vertical = int(((first > 0) & (want["actions"][t + 1, i] < 2)).sum())
    print(f"resets {len(t)}  distinct fresh boards {distinct}  scoring first moves {scoring} ({vertical} vertical)")
    assert distinct >= 380 and scoring >= 1000 and 0 < vertical < scoring
    check(dev, init, COVER_STEPS, 0, (ob, want))


# ---------------------------------------------------------------- launch start ------------------
def finished_boards(n):
    """Boards with no move left (two checkerboards, one with large tiles) and, every fifth, a fresh board."""
    rng = np.random.default_rng(SEED + 2000 + n)
    chk = (np.add.outer(np.arange(4), np.arange(4)) % 2).reshape(16).astype(np.int8)
    b = np.where(np.arange(n)[:, None] % 2 == 0, chk + 1, 9 * chk + 2).astype(np.int8)  # 2 / 4 and 4 / 2^11
    b[::5] = fresh_boards(rng, len(range(0, n, 5)))
    return b


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("n", [64, 150])
def test_one_step_from_finished_boards(dev, n, step0):
    init = finished_boards(n)
    ob, want = O.random_rollout_record(init, 1, SEED, step0=step0, env_base=ENV_BASE)
    started = np.arange(n) % 5 != 0
    assert ((want["boards"][0][started] != 0).sum(axis=1) == 2).all()  # the record shows the new game's board
    assert (want["points"][0][started] > 0).any()                      # and some first moves score
    check(dev, init, 1, step0, (ob, want))


@pytest.mark.parametrize("step0", [0, 1])
def test_zero_step_launch(dev, step0):
    init = finished_boards(150)
    boards, got = launch(dev, init, 0, step0, rows=1)
    assert np.array_equal(boards, init)
    for k in FIELDS:
        assert (got[k].view(np.uint8) == GUARD).all(), k
