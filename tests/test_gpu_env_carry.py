"""GPU parity of env_rollout_kernel's carried line records (kLine11) vs the CPU oracle, bit for bit.

The kernel carries the table records of the current board's rows and columns from step to step and
reads the tables only for the board a step produces.  These tests aim at the places where the carried
state is rebuilt or replaced: launch start, the odd first step, the fast-pair bound (every exponent
<= 8), the top table digit (10), the hand-over to the SWAR path and back, and auto-resets at either
step of a pair.  Every record is compared with O.random_rollout_record.
"""

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def random_boards(n, seed, hi, p_empty):
    rng = np.random.default_rng(seed)
    b = rng.integers(1, hi + 1, size=(n, 16)).astype(np.int8)
    b[rng.random(b.shape) < p_empty] = 0
    return b


class Rollout:
    """Boards on the device and one launch's record buffers; launch() returns the record as numpy."""

    def __init__(self, dev, init, steps):
        n = len(init)
        self.n, self.steps = n, steps
        self.b = torch.as_tensor(np.ascontiguousarray(init)).to(torch.int8).to(dev)
        self.tb = torch.zeros(steps, n, 16, dtype=torch.int8, device=dev)
        self.ta = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        self.tp = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        self.tpot = torch.zeros(steps, n, 4, dtype=torch.int8, device=dev)
        self.tf = torch.zeros(steps, n, dtype=torch.uint8, device=dev)

    def launch(self, seed, step0, env_base):
        lib = L()
        lib.env_rollout_random(self.b, self.steps, self.tb, self.ta, self.tp, self.tpot, self.tf,
                               lib.make_rng(lib.RNG_PHILOX, seed, step0, env_base))
        torch.cuda.synchronize()
        got = (self.tb, self.ta, self.tp, self.tpot, self.tf)
        return {k: t.cpu().numpy() for k, t in zip(FIELDS, got)}

    def boards(self):
        return self.b.cpu().numpy()


def assert_launch(dev, init, steps, seed, step0, env_base=0):
    """One launch against the oracle; returns the oracle's record."""
    ro = Rollout(dev, init, steps)
    got = ro.launch(seed, step0, env_base)
    ob, rec = O.random_rollout_record(init, steps, seed, step0=step0, env_base=env_base)
    for k in FIELDS:
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(ro.boards(), ob)
    return rec


@pytest.mark.parametrize("step0", [10, 11])
@pytest.mark.parametrize("steps", [1, 2, 3, 65])
@pytest.mark.parametrize("n", [64, 256])
def test_fast_path_chained_launches(dev, n, steps, step0):
    """Boards of exponents <= 6 (every wave starts in the fast pair), eight launches chained on the
    same boards from an even and an odd counter: the carried records are rebuilt at every launch
    start and kept through the odd first step (an odd step count flips the parity every launch)."""
    init = random_boards(n, 100 + n + steps, hi=6, p_empty=0.4)
    init[O.legal_mask(init) == 0] = 0
    init[:, 0] = np.where(init.any(axis=1), init[:, 0], 1)
    seed, launches = 0x51 + steps, 8
    ob, rec = O.random_rollout_record(init, launches * steps, seed, step0=step0, env_base=3)
    ro = Rollout(dev, init, steps)
    for j in range(launches):
        got = ro.launch(seed, step0 + j * steps, 3)
        for k in FIELDS:
            assert np.array_equal(got[k], rec[k][j * steps:(j + 1) * steps]), (k, j)
    assert np.array_equal(ro.boards(), ob)


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("m", [8, 9, 10])
def test_table_boundary(dev, m, step0):
    """Two waves whose every board has maximum exactly m and two adjacent m's: the moves create
    m + 1 -- past the fast-pair bound (9), at the top table digit (10), and outside the table (11:
    the SWAR path, left again by the auto-reset)."""
    n, steps = 128, 300
    init = random_boards(n, 200 + m, hi=m - 1, p_empty=0.25)
    pos = np.random.default_rng(m).integers(0, 3, n)
    for i in range(n):
        if i % 2 == 0:  # a horizontal pair in row i % 4
            r, c = i % 4, pos[i]
            init[i, 4 * r + c] = init[i, 4 * r + c + 1] = m
        else:  # a vertical pair in column i % 4
            c, r = i % 4, pos[i]
            init[i, 4 * r + c] = init[i, 4 * r + 4 + c] = m
    assert (init.max(axis=1) == m).all()
    rec = assert_launch(dev, init, steps, 0x77 + m, step0, env_base=9)
    assert (rec["boards"].reshape(steps, n, 16).max(axis=2) == m + 1).any()  # the merge happened
    assert (rec["flags"] & 0x80).sum() > 0                                     # and games ended and restarted
    if m == 10:  # a board that held an 11 was reset and played on through the table
        had11 = (rec["boards"].max(axis=2) == 11).any(axis=0)
        reset = ((rec["flags"] & 0x80) != 0)[:-1].any(axis=0)
        assert (had11 & reset).any()


def find_interleave_seed(init, lane, steps, step0):
    """The first seed whose oracle rollout ends lane's game between steps 2 and 20 of the launch while
    every other board stays below 2^9 -- the wave leaves the fast pair until then and returns to it."""
    for seed in range(1, 400):
        _, rec = O.random_rollout_record(init, steps, seed, step0=step0, env_base=0)
        ends = np.nonzero(rec["flags"][:, lane] & 0x80)[0]
        others = np.delete(rec["boards"], lane, axis=1)
        if len(ends) and 2 <= ends[0] <= 20 and others.max() < 9:
            return seed, int(ends[0])
    return None, None


@pytest.mark.parametrize("step0", [0, 1])
def test_fast_slow_interleaving(dev, step0):
    """One wave: a nearly full board holding a 9 among 63 small boards.  While the 9 is there the
    wave runs the non-fast pair; its game ends within a few steps (a seed found with the oracle) and
    the wave goes back to the fast pair with records the non-fast pair and the reset left."""
    n, steps, lane = 64, 40, 21
    init = random_boards(n, 300, hi=3, p_empty=0.6)
    init[:, 5] = 1
    init[lane] = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 9, 3, 3], np.int8)
    seed, t_end = find_interleave_seed(init, lane, steps, step0)
    assert seed is not None
    rec = assert_launch(dev, init, steps, seed, step0)
    assert rec["flags"][t_end, lane] & 0x80                 # the oracle record shows the reset ...
    assert rec["boards"][:t_end + 1, lane].max() == 9       # ... of the board that kept the wave slow
    assert rec["boards"][t_end + 1:].max() < 9              # and a small wave afterwards


@pytest.mark.parametrize("step0", [6, 7])
def test_resets_under_carried_state(dev, step0):
    """Boards one move from the end of their game (a full board with a single merge) in lanes 0, 31,
    32 and 63 of two waves, launched from an even and an odd counter so that the game ends at either
    step of a pair; 130 steps, so reset boards are then moved in all four directions."""
    n, steps = 128, 130
    init = random_boards(n, 400, hi=4, p_empty=0.5)
    init[:, 3] = 2
    base = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3], np.int8)
    lanes = np.array([0, 31, 32, 63, 64, 95, 96, 127])
    init[lanes] = base
    init[lanes[4:]] = base.reshape(4, 4).T.reshape(16)  # the merge in a column
    rec = assert_launch(dev, init, steps, 0x99, step0, env_base=2)
    fired = (rec["flags"] & 0x80) != 0
    assert fired[0, lanes].any()  # a constructed board ended on the launch's first step
    parity = (step0 + np.nonzero(fired)[0]) & 1
    assert (parity == 0).any() and (parity == 1).any()
    t, i = np.nonzero(fired[:-1])
    assert set(rec["actions"][t + 1, i].tolist()) == {0, 1, 2, 3}  # the fresh boards' first moves
