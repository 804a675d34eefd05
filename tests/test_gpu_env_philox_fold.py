"""GPU parity of env_rollout_kernel vs the CPU oracle, bit for bit, where no other test goes: a pair
counter that crosses 2^32 and a seed whose high word is not zero.

The cases were written for a fold of Philox rounds 0-1 into per-lane words that hold for one high
word of the pair counter (measured slower, not adopted: DESIGN.md section 6, round 11).  They stay
as the check of what any such change has to keep, and of the kernel's own pair and step
bookkeeping (a countdown of pairs since round 11): the pair counter's high word changing inside a
launch (at its first, second and a later pair, both parities of the first step), between two
launches and under a device counter, with both key words non-zero; and plain seeds.  Every launch
starts from copies of test_gpu_env_reset_reload.py's board A, so every lane ends at step 0 and the
first pair uses the draw's reset words.  All five record arrays and the final boards are compared
with O.random_rollout_record.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")

# legal mask 12 (LEFT / RIGHT only); either move followed by either spawn value ends the game
A = np.array([1, 2, 1, 2, 2, 1, 2, 1, 3, 2, 1, 3, 5, 5, 7, 8], np.int8)

SEED = 0xDEADBEEF12345678
ENV_BASE = 0xFFFF0000
CROSS = 1 << 33  # step counter at which the pair counter's high word changes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def reference(n, steps, seed, step0, env_base):
    """The oracle's record of `steps` steps from n copies of A, with the preconditions every case
    relies on: all games end at step 0, and no exponent above 8 (every pair is the fast one)."""
    ob, rec = O.random_rollout_record(np.tile(A, (n, 1)), steps, seed, step0=step0, env_base=env_base)
    assert ((rec["flags"][0] & 0x80) != 0).all()
    assert rec["boards"].max() == 8 and ob.max() <= 8
    for v in rec.values():
        v.setflags(write=False)
    ob.setflags(write=False)
    return ob, rec


class Chain:
    """n copies of A on the device, stepped by launches of any length; each returns its record."""

    def __init__(self, dev, n):
        self.dev, self.n = dev, n
        self.b = torch.as_tensor(np.tile(A, (n, 1))).to(dev)

    def launch(self, steps, rng, ticket=None):
        n, dev = self.n, self.dev
        tb = torch.zeros(steps, n, 16, dtype=torch.int8, device=dev)
        ta = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        tp = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        tpot = torch.zeros(steps, n, 4, dtype=torch.int8, device=dev)
        tf = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
        L().env_rollout_random(self.b, steps, tb, ta, tp, tpot, tf, rng, ticket)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(FIELDS, (tb, ta, tp, tpot, tf))}

    def boards(self):
        return self.b.cpu().numpy()


def assert_chain(dev, n, lengths, seed, step0, env_base):
    """Launches of the given lengths, one after the other, against one oracle record."""
    ob, rec = reference(n, sum(lengths), seed, step0, env_base)
    ch = Chain(dev, n)
    t = 0
    for steps in lengths:
        got = ch.launch(steps, L().make_rng(L().RNG_PHILOX, seed, step0 + t, env_base))
        for k in FIELDS:
            assert np.array_equal(got[k], rec[k][t:t + steps]), (k, t)
        t += steps
    assert np.array_equal(ch.boards(), ob)


@pytest.mark.parametrize("step0", [CROSS - 4, CROSS - 3, CROSS - 1])
def test_counter_crossing(dev, step0):
    """The pair counter's high word changes inside the launch, at the launch's later, second and first
    pair: one full wave and a partial one, both parities of the first step, both key words non-zero."""
    assert_chain(dev, 70, (8,), SEED, step0, ENV_BASE)


@pytest.mark.parametrize("step0", [CROSS - 4, CROSS - 3, CROSS - 1])
def test_chained_across_crossing(dev, step0):
    """The same record from launches of 3 + 5 steps: every launch starts from the counter alone."""
    assert_chain(dev, 70, (3, 5), SEED, step0, ENV_BASE)


def test_device_counter(dev):
    """g2048_env_rollout_random_adv: the counter comes from device memory (2^33 - 5), two launches
    of 4 steps, each advancing it; the crossing falls into the second launch."""
    n, step0 = 70, CROSS - 5
    ob, rec = reference(n, 8, SEED, step0, ENV_BASE)
    ctr = torch.full((1,), step0, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = L().make_rng(L().RNG_PHILOX, SEED, 0, ENV_BASE, counter_dev=ctr)
    ch = Chain(dev, n)
    for j in range(2):
        got = ch.launch(4, rng, ticket)
        for k in FIELDS:
            assert np.array_equal(got[k], rec[k][4 * j:4 * j + 4]), (k, j)
        assert int(ctr.item()) == step0 + 4 * (j + 1) and int(ticket.item()) == 0
    assert np.array_equal(ch.boards(), ob)


@pytest.mark.parametrize("step0", [0, 1])
def test_plain_seed(dev, step0):
    """Seed 1 (second key word zero), counters 0 and 1, env_base 0: one full wave, 6 steps."""
    assert_chain(dev, 64, (6,), 1, step0, 0)
