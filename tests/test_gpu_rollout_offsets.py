"""GPU parity of env_rollout_kernel's two record addressings (rollout_step.hpp): narrow -- the five array
bases in scalar registers and three per-lane 32-bit byte offsets advanced once per step -- and wide -- five
per-lane 64-bit pointers.  Every case is compared bit for bit with oracle.random_rollout_record in all five
records and the final boards, once in the form the library picks for the shape (narrow at every shape
here) and once with the wide form forced (g2048_env_rollout_force_wide, the test-only switch).

Every launch writes into guarded buffers: each record array is the interior of an allocation with one
extra row in front and one behind (and a few spare bytes), filled with a sentinel.  The interior is
therefore a view at a non-zero offset of one row -- 16 n, 4 n or n bytes, which for odd n is aligned to
what the ABI demands and no more -- so a base folded wrongly into an offset shows, and both guard rows
and everything behind the last row's last element must still hold the sentinel after the launch.

  partial and tiny waves, both pair phases   n in {1, 63, 64, 65, 300} x steps in {1, 2, 3, 7, 8} from an
      even and an odd counter (the odd one peels a first step, which advances the offsets before the pair
      loop).  Boards of digits 0..10, an eighth with an exponent 11..17 (the other pair's stores) and a few
      finished boards handed in.
  second trip of the board loop   n = 262 144 + 65, 3 steps from an odd counter: the grid is 256 x 1 024,
      so 65 lanes walk a second board, whose offsets have to restart from its own index.
  largest single-trip launch   n = 262 144 - 63, 3 steps from an odd counter: workgroups of 1 024 threads, the
      last wave with one lane, the largest shape class that runs the MFMA address form.
  game ends inside the run   boards one move from a dead position mixed with fresh two-tile boards: the
      flags store stands behind the masked reset block, so it runs on both sides of that branch; the
      ending falls on the even or the odd step of a pair by the counter.
  graph replay   three g2048_env_rollout_random_adv launches (device counter, ticket) captured in one
      graph and replayed twice: 6 x steps consecutive steps of one oracle run.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
SEED, ENV_BASE = 0x16A, 7
GUARD = 0xA5
SLACK = 64  # spare bytes behind the rear guard row and in front of the front one (n = 1: a row is a byte)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


@pytest.fixture(params=[False, True], ids=["narrow", "wide"])
def wide(request):
    """Runs the test in the form of its shape (narrow for every shape of this file) and with wide forced."""
    lib = L()
    lib.env_rollout_force_wide(request.param)
    try:
        yield request.param
    finally:
        lib.env_rollout_force_wide(False)


class Guarded:
    """The five record arrays of `rows` x n, each the interior of a sentinel-filled allocation: SLACK bytes
    (a multiple of 16), a guard row, the array, a guard row, SLACK bytes."""

    SPEC = {"boards": ((16,), torch.int8, 16), "actions": ((), torch.uint8, 1), "points": ((), torch.int32, 4),
            "pot": ((4,), torch.int8, 4), "flags": ((), torch.uint8, 1)}

    def __init__(self, dev, rows, n):
        self.rows, self.n, self.raw, self.view, self.span = rows, n, {}, {}, {}
        for k, (tail, dtype, elem) in self.SPEC.items():
            row = n * elem
            buf = torch.full((2 * SLACK + (rows + 2) * row,), GUARD, dtype=torch.uint8, device=dev)
            lo = SLACK + row
            hi = lo + rows * row
            self.raw[k], self.span[k] = buf, (lo, hi)
            self.view[k] = buf[lo:hi].view(dtype).view((rows, n) + tail)
            assert lo > 0 and self.view[k].data_ptr() == buf.data_ptr() + lo and self.view[k].data_ptr() % elem == 0

    def args(self, t0=0, steps=None):
        r = slice(t0, self.rows if steps is None else t0 + steps)
        return tuple(self.view[k][r] for k in FIELDS)

    def record(self):
        torch.cuda.synchronize()
        return {k: self.view[k].cpu().numpy() for k in FIELDS}

    def assert_guards(self):
        for k in FIELDS:
            whole = self.raw[k].cpu().numpy()
            lo, hi = self.span[k]
            front, back = np.flatnonzero(whole[:lo] != GUARD), np.flatnonzero(whole[hi:] != GUARD)
            assert len(front) == 0, (k, "written in front of row 0 at byte", int(front[-1]) - lo)
            assert len(back) == 0, (k, "written behind the last row at byte", int(back[0]))


def assert_equal(got, rec, boards, ob):
    for k in FIELDS:
        bad = np.argwhere(got[k] != rec[k])
        assert len(bad) == 0, (k, len(bad), bad[:4].tolist())
    assert np.array_equal(boards, ob), "final boards"


def check(dev, init, steps, step0, expect):
    assert L().env_rollout_form(len(init), steps) & L().ROLLOUT_FORM_WIDE == 0  # narrow unless forced
    ob, rec = expect
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    g = Guarded(dev, steps, len(init))
    L().env_rollout_random(b, steps, *g.args(), L().make_rng(L().RNG_PHILOX, SEED, step0, ENV_BASE))
    assert_equal(g.record(), rec, b.cpu().numpy(), ob)
    g.assert_guards()


@functools.lru_cache(maxsize=None)
def random_boards(n):
    rng = np.random.default_rng(SEED + n)
    b = rng.integers(0, 11, size=(n, 16)).astype(np.int8)
    b[rng.random(b.shape) < 0.3] = 0
    b[:, 3] = np.where(b.any(axis=1), b[:, 3], 2)                 # no empty board
    high = rng.random(n) < 0.125                                  # an exponent 11..17 somewhere on the board
    cell = rng.integers(0, 16, n)
    b[np.nonzero(high)[0], cell[high]] = rng.integers(11, 18, int(high.sum()))
    full = ((np.add.outer(np.arange(4), np.arange(4)) % 2) + 1).reshape(16).astype(np.int8)  # no move left
    for lane in () if n == 1 else {0, n // 3, n - 1} if n < 1000 else {5, 63, 262080, min(262144, n - 2), n - 1}:
        b[lane] = full
    return b


@functools.lru_cache(maxsize=None)
def expected(kind, n, steps, step0):
    init = {"random": random_boards, "ending": ending_boards}[kind](n)
    return O.random_rollout_record(init, steps, SEED, step0=step0, env_base=ENV_BASE)


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3, 7, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_partial_and_tiny_waves(dev, wide, n, steps, step0):
    check(dev, random_boards(n), steps, step0, expected("random", n, steps, step0))


def test_second_trip_of_the_board_loop(dev, wide):
    n = 262144 + 65
    assert L().env_rollout_form(n, 3) == 0  # the VALU address form, narrow
    check(dev, random_boards(n), 3, 1, expected("random", n, 3, 1))


def test_largest_single_trip_launch(dev, wide):
    """262 144 - 63 boards: 256 workgroups of 1 024 threads, four waves per SIMD, the last wave with one lane:
    the largest shape class that takes the MFMA address form, whose constant operand every lane reads
    whatever the execution mask."""
    n = 262144 - 63
    assert L().env_rollout_form(n, 3) == L().ROLLOUT_FORM_MFMA
    check(dev, random_boards(n), 3, 1, expected("random", n, 3, 1))


@functools.lru_cache(maxsize=None)
def ending_boards(n):
    """Every third board is one move from (most likely) the end of its game: a full board whose only merge
    is the pair of 8s at the end of the last row, or the transpose (the pair in the last column); the
    move leaves one empty cell, and a spawned 2 there, nine times in ten, leaves no move.  The rest are
    fresh boards of two tiles."""
    rng = np.random.default_rng(SEED + 1000 + n)
    end = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3], np.int8)
    b = np.zeros((n, 16), np.int8)
    for i in range(n):
        if i % 3 == 0:
            b[i] = end if i % 2 == 0 else end.reshape(4, 4).T.reshape(16)
        else:
            c = rng.choice(16, 2, replace=False)
            b[i, c] = rng.integers(1, 3, 2)
    return b


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("n", [64, 150])
def test_game_ends_inside_the_run(dev, wide, n, step0):
    steps = 6
    exp = expected("ending", n, steps, step0)
    done = (exp[1]["flags"] & L().FLAG_DONE) != 0
    ends = np.arange(n) % 3 == 0
    # the first step (the even one of a pair from counter 0, the odd one from counter 1) ends games in some
    # lanes of every wave and plays on in others: the reset block and the store behind it run under a partial mask
    for w in range(0, n - 63, 64):  # (about 21 such boards per wave; the move toward the pair's side ends none)
        assert 3 <= done[0, w:w + 64].sum() < 64 and not done[0, w:w + 64][~ends[w:w + 64]].any(), w
    assert done[1].any() and not done[1][~ends].any()  # and the pair's other step ends some that played on
    check(dev, ending_boards(n), steps, step0, exp)


def test_graph_replay(dev, wide):
    """Three launches of `steps` steps in one graph, replayed twice: rows 0 .. 3 steps of the record hold the
    oracle's steps 0 .. 3 steps after the first replay and 3 steps .. 6 steps after the second."""
    from g2048.dist import graph
    lib = L()
    n, steps = 70, 3
    # (no finished board handed in: its new game is drawn at the launch's counter + steps, which differs
    # between three launches of `steps` and one run of 6 x steps)
    init = ending_boards(n)
    ob, rec = expected("ending", n, 6 * steps, 0)
    # the first launch of a process loads the kernel: outside the capture, on buffers of its own
    warm = Guarded(dev, steps, n)
    lib.env_rollout_random(torch.as_tensor(init).to(dev), steps, *warm.args(), lib.make_rng(lib.RNG_PHILOX, SEED, 0, ENV_BASE))
    torch.cuda.synchronize()
    b = torch.as_tensor(init).to(dev)
    g = Guarded(dev, 3 * steps, n)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = lib.make_rng(lib.RNG_PHILOX, SEED, 0, ENV_BASE, counter_dev=ctr)
    cg = torch.cuda.CUDAGraph()
    with graph(cg):
        for j in range(3):  # an even, an odd and an even starting counter; odd, even, odd in the second replay
            lib.env_rollout_random(b, steps, *g.args(j * steps, steps), rng, ticket)
    for r in range(2):
        cg.replay()
        got = g.record()
        for k in FIELDS:
            assert np.array_equal(got[k], rec[k][3 * steps * r:3 * steps * (r + 1)]), (k, r)
        assert int(ctr.item()) == 3 * steps * (r + 1) and int(ticket.item()) == 0
    assert np.array_equal(b.cpu().numpy(), ob)
    g.assert_guards()
