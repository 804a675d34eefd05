"""GPU parity of the step's action pick and spawn arithmetic (kth_bit4, the byte-wise row / column of the
spawn, the picks by index masks) vs the CPU oracle, bit for bit, on inputs chosen so that the oracle's
own record shows every value those pieces can take.

256 boards x 16 steps from counter 0 and 1 (so every board meets both step forms), seed 0x13A:
  wave 0        small random boards beside boards holding 2^9 .. 2^12 and one whose only moves merge
                11 + 11 -> 12: the wave changes between the two pair variants, SWAR lanes beside table lanes
  waves 1 .. 3  boards that never exceed 2^8 within the launch (asserted), so the wave-uniform fast pair
                plays them throughout: directed boards of every legal mask 1..15, boards of one or two
                low tiles (the spawn against the maximum), random boards of every fill
The coverage is asserted on the oracle's record before anything is compared with the GPU.  The same
boards then go through g2048_mc_search (the kTraj = false step) against tests/mc_reference.py at one
playout per action and depth 4: depth 0 plays no step, and 4 is the smallest depth at which the pair
loop runs behind an odd first step and in front of an odd last one.
"""

import functools

import numpy as np
import pytest
import torch

from mc_reference import legal_best, mc_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
N, STEPS, SEED, ENV_BASE = 256, 16, 0x13A, 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def symmetries(g):
    for k in range(4):
        r = np.rot90(g, k)
        yield r
        yield r[:, ::-1]


def mask_boards(rng):
    """12 boards per legal mask 1..15: a full board without equal neighbours (the parity of a cell's
    exponent is that of i + j), with cells emptied or one pair made equal, in its 8 symmetries; the
    oracle's legal mask sorts them."""
    patterns = [[(0, 0), (0, 1), (0, 2), (0, 3)], [(0, 0)], [(0, 1)], [(1, 1)], "pair"]
    found = {m: [] for m in range(1, 16)}
    while any(len(v) < 12 for v in found.values()):
        g = (np.add.outer(np.arange(4), np.arange(4)) % 2 + 1 + 2 * rng.integers(0, 3, (4, 4))).astype(np.int8)
        pat = patterns[rng.integers(len(patterns))]
        if pat == "pair":
            g[1, 0] = g[0, 0]
        else:
            for c in pat:
                g[c] = 0
        for s in symmetries(g):
            b = np.ascontiguousarray(s).reshape(16)
            m = int(O.legal_mask(b[None])[0])
            if m and len(found[m]) < 12:
                found[m].append(b.copy())
    return np.stack([b for m in range(1, 16) for b in found[m]])


@functools.lru_cache(maxsize=None)
def boards():
    rng = np.random.default_rng(SEED)
    b = np.zeros((N, 16), np.int8)
    # wave 0: small random boards, and in lanes 3, 17, 30, 44, 58 the high tiles
    w0 = rng.integers(1, 5, size=(64, 16)).astype(np.int8)
    w0[rng.random(w0.shape) < 0.5] = 0
    w0[:, 5] = 1
    for lane, hi in ((3, 9), (17, 10), (30, 11), (44, 12)):
        w0[lane, 10] = hi
    w0[58] = np.array([11, 11, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.int8)  # LEFT / RIGHT only, both merge the 11s
    b[:64] = w0
    # waves 1 .. 3: 180 directed mask boards, 8 boards of one or two low tiles, 4 random boards
    mb = mask_boards(rng)
    b[64:64 + len(mb)] = mb
    low = np.zeros((8, 16), np.int8)
    for i, (c0, v0, c1, v1) in enumerate([(8, 1, 8, 1), (7, 1, 7, 1), (0, 1, 0, 1), (15, 1, 15, 1), (5, 2, 5, 2),
                                          (10, 2, 10, 2), (3, 1, 12, 1), (6, 1, 9, 2)]):
        low[i, c0], low[i, c1] = v0, v1
    b[244:252] = low
    rnd = rng.integers(1, 4, size=(4, 16)).astype(np.int8)
    rnd[rng.random(rnd.shape) < 0.6] = 0
    rnd[:, 0] = 1
    b[252:] = rnd
    assert len(mb) == 180
    return b


@functools.lru_cache(maxsize=None)
def oracle_record(step0):
    ob, rec = O.random_rollout_record(boards(), STEPS, SEED, step0=step0, env_base=ENV_BASE)
    return ob, rec


def coverage(step0):
    """The sets the docstring names, from the oracle's record alone; small waves only (lanes 64..)."""
    ob, rec = oracle_record(step0)
    before = rec["boards"].astype(np.int64)                       # [T, N, 16]
    nxt = np.concatenate([before[1:], ob[None].astype(np.int64)])  # the board after the step (and a reset)
    acts = rec["actions"].astype(np.int64)
    reset = (rec["flags"] & 0x20) != 0
    T = STEPS
    flat = before.reshape(T * N, 16).astype(np.int8)
    legal = O.legal_mask(flat).astype(np.int64).reshape(T, N)
    moved, _, _ = O.move(flat, acts.reshape(-1))
    moved = moved.astype(np.int64).reshape(T, N, 16)
    idx = np.array([[bin(int(legal[t, i]) & ((1 << int(acts[t, i])) - 1)).count("1") for i in range(N)] for t in range(T)])
    small = np.zeros((T, N), bool)
    small[:, 64:] = True
    assert before[:, 64:].max() <= 8 and ob[64:].max() <= 8       # waves 1 .. 3 stay on the fast pair
    cov = {"action": set(), "spawn": set(), "row_empties": set(), "vs_max": set()}
    for t in range(T):
        for i in range(64, N):
            cov["action"].add((int(legal[t, i]), int(idx[t, i])))
            if reset[t, i]:
                continue
            d = nxt[t, i] - moved[t, i]
            (cell,) = np.nonzero(d)
            assert len(cell) == 1 and d[cell[0]] in (1, 2) and moved[t, i, cell[0]] == 0
            c, v = int(cell[0]), int(d[cell[0]])
            cov["spawn"].add((c, v))
            cov["row_empties"].add((c, int((moved[t, i].reshape(4, 4)[c // 4] == 0).sum())))
            mx = int(moved[t, i].max())
            first = int(np.argmax(moved[t, i] == mx))
            cov["vs_max"].add("above" if v > mx else "below" if v < mx else "equal, before" if c < first else "equal, after")
    return cov, before, moved


@pytest.mark.parametrize("step0", [0, 1])
def test_oracle_record_covers_the_step(step0):
    cov, before, moved = coverage(step0)
    assert cov["action"] == {(m, k) for m in range(1, 16) for k in range(bin(m).count("1"))}      # 32 pairs
    assert cov["spawn"] == {(c, v) for c in range(16) for v in (1, 2)}                            # 32 pairs
    assert cov["row_empties"] == {(c, e) for c in range(16) for e in (1, 2, 3, 4)}
    assert cov["vs_max"] == {"above", "below", "equal, before", "equal, after"}
    # wave 0 at the first step: boards <= 2^8 beside 2^9, 2^10, 2^11 and 2^12, and the 11 + 11 -> 12 merge
    mx0 = before[0, :64].max(axis=1)
    assert (mx0 <= 8).sum() >= 32 and {9, 10, 11, 12} <= set(mx0.tolist())
    assert mx0[58] == 11 and moved[0, 58].max() == 12
    # ... and the wave comes back to the fast pair or stays off it, either is fine: both variants ran
    assert (before[:, :64].max(axis=(1, 2)) > 8).any()


@pytest.mark.parametrize("step0", [0, 1])
def test_launch_matches_oracle(dev, step0):
    init = boards()
    lib = L()
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    tb = torch.zeros(STEPS, N, 16, dtype=torch.int8, device=dev)
    ta = torch.zeros(STEPS, N, dtype=torch.uint8, device=dev)
    tp = torch.zeros(STEPS, N, dtype=torch.int32, device=dev)
    tpot = torch.zeros(STEPS, N, 4, dtype=torch.int8, device=dev)
    tf = torch.zeros(STEPS, N, dtype=torch.uint8, device=dev)
    lib.env_rollout_random(b, STEPS, tb, ta, tp, tpot, tf, lib.make_rng(lib.RNG_PHILOX, SEED, step0, ENV_BASE), None)
    torch.cuda.synchronize()
    ob, rec = oracle_record(step0)
    for k, t in zip(FIELDS, (tb, ta, tp, tpot, tf)):
        assert np.array_equal(t.cpu().numpy(), rec[k]), k
    assert np.array_equal(b.cpu().numpy(), ob)


@pytest.mark.parametrize("ctr", [0, 1])
def test_mc_search_matches_reference(dev, ctr):
    """The same boards through the kTraj = false step: P = 1, D = 4, from an even and an odd counter."""
    init, P, D = boards(), 1, 4
    lib = L()
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    score = torch.empty(N, 4, dtype=torch.int64, device=dev)
    moves = torch.empty(N, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(N, dtype=torch.uint8, device=dev)
    best = torch.empty(N, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.mc_search_workspace_bytes(N, P), dtype=torch.uint8, device=dev)
    lib.mc_search(b, P, D, lib.make_rng(lib.RNG_PHILOX, SEED, ctr, ENV_BASE), score, moves, legal, best, ws)
    torch.cuda.synchronize()
    sc, mv, inv = mc_ref(init, P, D, SEED, ctr, ENV_BASE)
    rl, rb = legal_best(sc, inv)
    assert np.array_equal(score.cpu().numpy(), sc), "score_sum"
    assert np.array_equal(moves.cpu().numpy(), mv), "move_sum"
    assert np.array_equal(legal.cpu().numpy(), rl), "legal"
    assert np.array_equal(best.cpu().numpy(), rb), "best"
