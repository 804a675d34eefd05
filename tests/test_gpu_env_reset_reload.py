"""GPU parity of env_rollout_kernel's auto-reset vs the CPU oracle, bit for bit.

A lane whose game ends loads the fresh board and the table records of its eight lines under the exec
mask of the ending lanes (a wave without an ending skips the block); every other lane keeps what the
step's own table reads loaded.  These tests aim at that masked load: a full mask, a partial last wave,
a single lane at either end of the wave, no lane at all, endings on consecutive steps of both parities
(the next pair's reset preparation runs next to a reload), an ending on a launch's last step, and a
board above the table that ends and returns to it.  Every record and the final boards are compared
with O.random_rollout_record, and each case asserts on the oracle's record that its input still
exercises the path it is meant for.
"""

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")

# legal mask 12 (LEFT / RIGHT only); either move followed by either spawn value ends the game
A = np.array([1, 2, 1, 2, 2, 1, 2, 1, 3, 2, 1, 3, 5, 5, 7, 8], np.int8)
SPARSE = np.zeros(16, np.int8)
SPARSE[[0, 5, 10]] = (1, 2, 1)


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
        self.b = torch.as_tensor(np.ascontiguousarray(init)).to(torch.int8).to(dev)
        self.tb = torch.zeros(steps, n, 16, dtype=torch.int8, device=dev)
        self.ta = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        self.tp = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        self.tpot = torch.zeros(steps, n, 4, dtype=torch.int8, device=dev)
        self.tf = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        self.steps = steps

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


def ended(rec):
    return (rec["flags"] & 0x80) != 0


def test_fixed_boards():
    """The two constructed boards are what the cases below rely on (CPU only, no launch)."""
    assert int(O.legal_mask(A[None])[0]) == 12
    assert int(O.legal_mask(SPARSE[None])[0]) != 0


@pytest.mark.parametrize("seed", [1, 2, 0x99])
@pytest.mark.parametrize("step0", [0, 1, 6, 7])
@pytest.mark.parametrize("n", [64, 70])
def test_every_lane_ends(dev, n, step0, seed):
    """Every board one move from its end: the full exec mask, and a partial last wave (n = 70)."""
    init = np.tile(A, (n, 1))
    rec = assert_launch(dev, init, 4, seed, step0)
    fired = ended(rec)
    assert fired[0].all() and not fired[1].any()


@pytest.mark.parametrize("step0", [2, 3])
@pytest.mark.parametrize("lane", [0, 63])
def test_one_lane_ends(dev, lane, step0):
    """A single-lane mask at either end of the wave: the neighbours' carried records stay untouched."""
    init = np.tile(SPARSE, (64, 1))
    init[lane] = A
    rec = assert_launch(dev, init, 6, 0x41, step0)
    fired = ended(rec)
    assert fired.sum() == 1 and fired[0, lane]


def test_nobody_ends(dev):
    """No ending in any lane of either wave: the masked block is skipped throughout."""
    init = np.tile(SPARSE, (70, 1))
    rec = assert_launch(dev, init, 9, 0x42, 1)
    assert not ended(rec).any()


def consecutive_boards():
    init = random_boards(128, 500, hi=5, p_empty=0.06)
    init[O.legal_mask(init) == 0] = A
    return init


@pytest.mark.parametrize("step0", [4, 5])
def test_consecutive_endings(dev, step0):
    """Nearly full boards: endings at steps 0 through 6 of the launch, in different lanes, at both
    parities -- the next pair's reset preparation runs next to a reload.  Every exponent stays <= 8,
    so every pair is the fast one."""
    init = consecutive_boards()
    rec = assert_launch(dev, init, 24, 0x31, step0, env_base=5)
    fired = ended(rec)
    t = np.nonzero(fired.any(axis=1))[0]
    assert set(range(7)) <= set(t.tolist())
    parity = (step0 + t) & 1
    assert (parity == 0).any() and (parity == 1).any()
    assert (np.diff(t) == 1).any()
    assert rec["boards"].max() <= 8


@pytest.mark.parametrize("step0", [4, 5])
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_ending_on_last_step(dev, steps, step0):
    """The boards of test_consecutive_endings in eight chained launches of 1, 2 and 3 steps against
    one oracle record: a game that ends on a launch's last step hands the fresh board to the next
    launch, which rebuilds the carried records from it."""
    init = consecutive_boards()
    launches = 8
    ob, rec = O.random_rollout_record(init, launches * steps, 0x31, step0=step0, env_base=5)
    last = ended(rec)[steps - 1::steps]
    assert last.any()  # some launch's last step ends a game
    ro = Rollout(dev, init, steps)
    for j in range(launches):
        got = ro.launch(0x31, step0 + j * steps, 5)
        for k in FIELDS:
            assert np.array_equal(got[k], rec[k][j * steps:(j + 1) * steps]), (k, j)
    assert np.array_equal(ro.boards(), ob)


def test_above_the_table(dev):
    """tests/test_gpu_env_carry.py's table-boundary construction with m = 10 at n = 64: a board that
    reaches 2^11 moves on the SWAR path, ends, and returns to the table path through the reload."""
    m, n, steps = 10, 64, 130
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
    rec = assert_launch(dev, init, steps, 0x77 + m, 0, env_base=9)
    had11 = (rec["boards"].max(axis=2) == 11).any(axis=0)
    reset = ended(rec)[:-1].any(axis=0)
    assert (had11 & reset).any()  # a board that held an 11 was reset before the last step
