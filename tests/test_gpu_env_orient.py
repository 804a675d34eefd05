"""GPU parity of the step's orientation network (line11_lds.hpp orient_rows: the moved board from the
four slid lines' records in one pack / split / interleave for all four directions) vs the CPU oracle,
bit for bit, on inputs chosen so that the oracle's own record shows every way through the network.

70 boards x 48 steps from counter 0 and 1 (every board meets both step forms), as n = 64 (one whole
wave) and n = 70 (a second wave of six lanes), seed 0x14A:
  boards 0 .. 15   hand-placed: a full board of 1 .. 4 without equal neighbours, a 6 on cell c, one cell
                   emptied so that one line slides: the first step leaves the maximum on cell c
  boards 16 .. 69  dense random boards of exponents <= 6 (two empty cells on average): they meet every
                   direction, merge, fill up and end within the launch
No board reaches 2^9 within the launch (asserted), so the wave-uniform fast pair plays them.  The
coverage is asserted on the oracle's record, with its counts pinned, before anything is compared with
the GPU.  One more set puts 2^9, 2^10 and 2^11 into three lanes of the 70: the other pair variant and
the SWAR lanes run the same network beside table lanes.  The first 64 boards also go through
g2048_mc_search (the kTraj = false step) against tests/mc_reference.py.
"""

import functools

import numpy as np
import pytest
import torch

from mc_reference import legal_best, mc_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
N, STEPS, SEED, ENV_BASE = 70, 48, 0x14A, 2
FLAG_RESET = 0x20
CASES = [(64, 0), (64, 1), (70, 0), (70, 1)]
# per case, from the oracle's record: the smallest count over (action, parity of the step in its pair)
# of the steps taken, of those whose board slides differently to the two ends of the axis, the
# smallest count over the 16 cells of the moved board's first maximum, the moved boards that hold
# their maximum twice or more, and the games that end in an even / an odd step
PINNED = {
    (64, 0): (370, 370, 55, 949, 25, 24),
    (64, 1): (362, 362, 82, 968, 23, 23),
    (70, 0): (413, 413, 62, 1079, 27, 25),
    (70, 1): (394, 394, 90, 1079, 24, 27),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def placed_boards(rng):
    """One board per cell c whose first step, whatever its direction, leaves the maximum (a 6) on c: a
    full board of 1 .. 4 in which the parity of a cell's exponent is that of i + j (no equal neighbours),
    one cell outside c's row and column emptied (the moves slide one line, never c's)."""
    out = []
    for c in range(16):
        while True:
            g = (np.add.outer(np.arange(4), np.arange(4)) % 2 + 1 + 2 * rng.integers(0, 2, (4, 4))).astype(np.int8)
            g[c // 4, c % 4] = 6
            e = int(rng.integers(16))
            if e // 4 == c // 4 or e % 4 == c % 4:
                continue
            g[e // 4, e % 4] = 0
            b = g.reshape(16)
            moved = [O.move(b[None], np.array([a]))[0][0] for a in range(4)]
            legal = int(O.legal_mask(b[None])[0])
            if all(int(np.argmax(moved[a] == 6)) == c for a in range(4) if legal >> a & 1):
                out.append(b.copy())
                break
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def boards(high=False):
    rng = np.random.default_rng(SEED)
    b = np.zeros((N, 16), np.int8)
    b[:16] = placed_boards(rng)
    d = rng.integers(1, 7, size=(N - 16, 16)).astype(np.int8)
    d[rng.random(d.shape) < 0.125] = 0
    b[16:] = d
    if high:  # 2^9, 2^10, 2^11 in lanes of both waves, on a cell that leaves the board a move
        for lane, hi in ((21, 9), (40, 10), (66, 11)):
            b[lane, 5] = hi
            b[lane, 6] = 0
    return b


@functools.lru_cache(maxsize=None)
def oracle_record(n, step0, high=False):
    return O.random_rollout_record(boards(high)[:n], STEPS, SEED, step0=step0, env_base=ENV_BASE)


def coverage(n, step0):
    """The counts PINNED names, from the oracle's record alone."""
    ob, rec = oracle_record(n, step0)
    before = rec["boards"].reshape(STEPS * n, 16)
    acts = rec["actions"].astype(np.int64).reshape(-1)
    assert before.max() <= 8 and ob.max() <= 8  # the fast pair throughout
    moved = O.move(before, acts)[0]
    other = O.move(before, acts ^ 1)[0]  # the same lines slid to the other end
    differ = (moved != other).any(axis=1)
    parity = ((step0 + np.arange(STEPS)) & 1).repeat(n)
    taken = [int(((acts == a) & (parity == p)).sum()) for a in range(4) for p in range(2)]
    taken_differ = [int(((acts == a) & (parity == p) & differ).sum()) for a in range(4) for p in range(2)]
    mx = moved.max(axis=1, keepdims=True)
    first = np.argmax(moved == mx, axis=1)
    cells = np.bincount(first, minlength=16)
    twice = int(((moved == mx).sum(axis=1) >= 2).sum())
    ended = (rec["flags"].reshape(-1) & FLAG_RESET) != 0
    return (min(taken), min(taken_differ), int(cells.min()), twice, int((ended & (parity == 0)).sum()),
            int((ended & (parity == 1)).sum()))


@pytest.mark.parametrize("n,step0", CASES)
def test_oracle_record_covers_the_network(n, step0):
    cov = coverage(n, step0)
    print(n, step0, cov)
    assert all(c >= 1 for c in cov), cov  # every action in both parities, every cell, a double maximum, both endings
    assert cov == PINNED[(n, step0)]


def test_high_boards_leave_the_fast_pair():
    ob, rec = oracle_record(N, 0, True)
    mx0 = rec["boards"][0].max(axis=1)
    assert (mx0[21], mx0[40], mx0[66]) == (9, 10, 11) and (np.delete(mx0, (21, 40, 66)) <= 6).all()
    # each of the three is still on the board after the first pair (no game of theirs ends in it)
    assert (rec["boards"][2, (21, 40, 66)].max(axis=1) >= (9, 10, 11)).all()


def launch(dev, init, step0):
    lib = L()
    n = len(init)
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    tb = torch.zeros(STEPS, n, 16, dtype=torch.int8, device=dev)
    ta = torch.zeros(STEPS, n, dtype=torch.uint8, device=dev)
    tp = torch.zeros(STEPS, n, dtype=torch.int32, device=dev)
    tpot = torch.zeros(STEPS, n, 4, dtype=torch.int8, device=dev)
    tf = torch.zeros(STEPS, n, dtype=torch.uint8, device=dev)
    lib.env_rollout_random(b, STEPS, tb, ta, tp, tpot, tf, lib.make_rng(lib.RNG_PHILOX, SEED, step0, ENV_BASE), None)
    torch.cuda.synchronize()
    return b, (tb, ta, tp, tpot, tf)


@pytest.mark.parametrize("n,step0", CASES)
def test_launch_matches_oracle(dev, n, step0):
    b, out = launch(dev, boards()[:n], step0)
    ob, rec = oracle_record(n, step0)
    for k, t in zip(FIELDS, out):
        assert np.array_equal(t.cpu().numpy(), rec[k]), k
    assert np.array_equal(b.cpu().numpy(), ob)


@pytest.mark.parametrize("step0", [0, 1])
def test_launch_with_high_boards_matches_oracle(dev, step0):
    b, out = launch(dev, boards(True), step0)
    ob, rec = oracle_record(N, step0, True)
    for k, t in zip(FIELDS, out):
        assert np.array_equal(t.cpu().numpy(), rec[k]), k
    assert np.array_equal(b.cpu().numpy(), ob)


@pytest.mark.parametrize("ctr", [0, 1])
def test_mc_search_matches_reference(dev, ctr):
    """The first 64 boards through the kTraj = false step: P = 1, D = 4, from an even and an odd counter."""
    init, P, D = boards()[:64], 1, 4
    n = len(init)
    lib = L()
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    score = torch.empty(n, 4, dtype=torch.int64, device=dev)
    moves = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.mc_search_workspace_bytes(n, P), dtype=torch.uint8, device=dev)
    lib.mc_search(b, P, D, lib.make_rng(lib.RNG_PHILOX, SEED, ctr, ENV_BASE), score, moves, legal, best, ws)
    torch.cuda.synchronize()
    sc, mv, inv = mc_ref(init, P, D, SEED, ctr, ENV_BASE)
    rl, rb = legal_best(sc, inv)
    assert np.array_equal(score.cpu().numpy(), sc), "score_sum"
    assert np.array_equal(moves.cpu().numpy(), mv), "move_sum"
    assert np.array_equal(legal.cpu().numpy(), rl), "legal"
    assert np.array_equal(best.cpu().numpy(), rb), "best"
