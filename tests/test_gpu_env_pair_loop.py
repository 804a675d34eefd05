"""GPU parity of env_rollout_kernel's pair loop and record addressing vs the CPU oracle, bit for bit.

The kernel runs its steps two at a time (one Philox draw per pair), with an odd first step when the
launch starts on an odd counter and an odd last one when steps are left over; its workgroups are
persistent over the boards; every step writes one row of five time-major record arrays.  These tests
aim at the loop's entries and exits, at the per-board setup behind the persistent stride, at the row
addresses (guarded buffers), at launches chained on the device counter inside one graph and at the
change between the two pair variants with games ending in either.  Every record array and the final
boards are compared with O.random_rollout_record.
"""

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
# one move from the end of the game: a full board whose only merge is the pair of 3s
ENDING = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3], np.int8)


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
    b[:, 0] = np.where(b.any(axis=1), b[:, 0], 1)  # no empty board
    return b


class Rollout:
    """Boards on the device and the record buffers of `steps` steps; launch() runs `steps` steps (or a
    slice of the rows, for chained launches) and record() returns the arrays as numpy."""

    def __init__(self, dev, init, steps):
        n = len(init)
        self.n, self.steps = n, steps
        self.b = torch.as_tensor(np.ascontiguousarray(init)).to(torch.int8).to(dev)
        self.tb = torch.zeros(steps, n, 16, dtype=torch.int8, device=dev)
        self.ta = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        self.tp = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        self.tpot = torch.zeros(steps, n, 4, dtype=torch.int8, device=dev)
        self.tf = torch.zeros(steps, n, dtype=torch.uint8, device=dev)

    def launch(self, rng, t0=0, steps=None, ticket=None):
        steps = self.steps - t0 if steps is None else steps
        rows = slice(t0, t0 + steps)
        L().env_rollout_random(self.b, steps, self.tb[rows], self.ta[rows], self.tp[rows], self.tpot[rows],
                               self.tf[rows], rng, ticket)

    def record(self):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(FIELDS, (self.tb, self.ta, self.tp, self.tpot, self.tf))}

    def boards(self):
        return self.b.cpu().numpy()


def assert_launch(dev, init, steps, seed, step0, env_base=0):
    """One launch against the oracle; returns the oracle's record."""
    ro = Rollout(dev, init, steps)
    ro.launch(L().make_rng(L().RNG_PHILOX, seed, step0, env_base))
    got = ro.record()
    ob, rec = O.random_rollout_record(init, steps, seed, step0=step0, env_base=env_base)
    for k in FIELDS:
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(ro.boards(), ob)
    return rec


@pytest.mark.parametrize("n", [64, 70])
@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5, 6, 7])
def test_loop_entry_and_exit(dev, steps, step0, n):
    """Zero to three trips of the pair loop, with and without the odd first and the odd last step; 70
    boards leave the second wave partly filled."""
    init = random_boards(n, 500 + n, hi=6, p_empty=0.4)
    assert_launch(dev, init, steps, 0x61 + steps, step0, env_base=5)


def test_persistent_stride(dev):
    """256 x 1024 + 70 boards: the launch is 256 workgroups of 1024 lanes, and 70 lanes walk a second
    board, for which the record addresses, the trip count and the lane's Philox constants are set up
    again.  An odd first step, one pair.  Compared on 16 seeded runs of 256 boards and the last 70."""
    n, steps, seed, step0, env_base = 256 * 1024 + 70, 3, 0x71, 1, 11
    init = random_boards(n, 600, hi=6, p_empty=0.4)
    ro = Rollout(dev, init, steps)
    ro.launch(L().make_rng(L().RNG_PHILOX, seed, step0, env_base))
    got, gb = ro.record(), ro.boards()
    starts = np.random.default_rng(601).integers(0, n - 70 - 256, 16).tolist()
    runs = [(s, s + 256) for s in starts] + [(n - 70, n)]
    assert sum(e - s for s, e in runs) >= 4096 + 70
    for s, e in runs:
        ob, rec = O.random_rollout_record(init[s:e], steps, seed, step0=step0, env_base=env_base + s)
        for k in FIELDS:
            assert np.array_equal(got[k][:, s:e], rec[k]), (k, s)
        assert np.array_equal(gb[s:e], ob), s


def test_row_addressing_guarded(dev):
    """257 boards, 4 steps, every record array inside a larger buffer filled with a guard byte: 64 guard
    elements on either side, the array's base 16-byte aligned and not 256-byte aligned.  The records
    equal the oracle's and no guard element is touched."""
    n, steps, seed, step0, env_base, guard = 257, 4, 0x81, 0, 2, 0x5A
    init = random_boards(n, 700, hi=6, p_empty=0.4)
    b = torch.as_tensor(init).to(dev)
    shapes = {"boards": ((steps, n, 16), torch.int8, 16), "actions": ((steps, n), torch.uint8, 1),
              "points": ((steps, n), torch.int32, 4), "pot": ((steps, n, 4), torch.int8, 4),
              "flags": ((steps, n), torch.uint8, 1)}
    raw, view, span = {}, {}, {}
    for k, (shape, dtype, elem) in shapes.items():
        size = int(np.prod(shape)) * dtype.itemsize
        buf = torch.full((size + 2 * 64 * elem + 512,), guard, dtype=torch.uint8, device=dev)
        # the first offset behind 64 guard elements that is 16 mod 256
        lo = next(o for o in range(64 * elem, 64 * elem + 512) if (buf.data_ptr() + o) % 256 == 16)
        raw[k], span[k] = buf, (lo, lo + size)
        view[k] = buf[lo:lo + size].view(dtype).view(shape)
        assert view[k].data_ptr() % 16 == 0 and view[k].data_ptr() % 256 != 0
        assert lo >= 64 * elem and len(buf) - (lo + size) >= 64 * elem
    L().env_rollout_random(b, steps, view["boards"], view["actions"], view["points"], view["pot"], view["flags"],
                           L().make_rng(L().RNG_PHILOX, seed, step0, env_base))
    torch.cuda.synchronize()
    ob, rec = O.random_rollout_record(init, steps, seed, step0=step0, env_base=env_base)
    for k in FIELDS:
        assert np.array_equal(view[k].cpu().numpy(), rec[k]), k
        lo, hi = span[k]
        whole = raw[k].cpu().numpy()
        assert (whole[:lo] == guard).all() and (whole[hi:] == guard).all(), k
    assert np.array_equal(b.cpu().numpy(), ob)


def test_chained_launches_in_one_graph(dev):
    """Three launches of 3 steps through g2048_env_rollout_random_adv, captured in one graph and replayed
    once from counter 0: they start on an even, an odd and an even counter.  One oracle run of 9 steps."""
    from g2048.dist import graph
    n, seed, env_base = 70, 0x91, 4
    init = random_boards(n, 800, hi=6, p_empty=0.4)
    lib = L()
    # the first launch of a process loads the kernel: outside the capture, on buffers of its own
    warm = Rollout(dev, init, 3)
    warm.launch(lib.make_rng(lib.RNG_PHILOX, seed, 0, env_base))
    torch.cuda.synchronize()
    ro = Rollout(dev, init, 9)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = lib.make_rng(lib.RNG_PHILOX, seed, 0, env_base, counter_dev=ctr)
    g = torch.cuda.CUDAGraph()
    with graph(g):
        for j in range(3):
            ro.launch(rng, t0=3 * j, steps=3, ticket=ticket)
    g.replay()
    got = ro.record()
    ob, rec = O.random_rollout_record(init, 9, seed, step0=0, env_base=env_base)
    for k in FIELDS:
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(ro.boards(), ob)
    assert int(ctr.item()) == 9 and int(ticket.item()) == 0


@pytest.mark.parametrize("step0", [0, 1])
def test_fast_slow_switching_with_endings(dev, step0):
    """One wave of small boards of which one holds a 2^9 tile (the wave runs the other pair while it is
    there) and two are one move from the end of their game: six steps from an even and an odd counter,
    so both pair variants and the reset blocks of both steps run."""
    n, steps = 64, 6
    init = random_boards(n, 900, hi=3, p_empty=0.6)
    init[:, 5] = 1
    init[21] = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 9, 3, 3], np.int8)
    init[0] = ENDING
    init[63] = ENDING.reshape(4, 4).T.reshape(16)  # the merge in a column
    # whether the merge ends the game depends on the spawn: the first seed (by the oracle) with which a
    # constructed board ends on the launch's first step, the even or the odd step of a pair by step0
    for seed in range(1, 200):
        _, rec = O.random_rollout_record(init, steps, seed, step0=step0, env_base=1)
        if (rec["flags"][0, [0, 63]] & 0x80).any():
            break
    else:
        pytest.fail("no seed ends a constructed board on the first step")
    assert rec["boards"][0].max() == 9
    assert_launch(dev, init, steps, seed, step0, env_base=1)
