"""GPU parity of the rollout step's line addresses from the matrix pipe (line11_lds.hpp
line11_addrs_mfma: the LDS addresses of a board's four row records and four column records as the 16
outputs of one v_mfma_i32_32x32x32_i8 of the board against a per-lane constant) vs the CPU oracle, bit
for bit in every record: boards, actions, points, potentials, flags and final boards.

  every table index through every line   14 641 boards whose row i holds the base-11 digits of
      (k + 3331 i) mod 14641, and their transposes, for 2 steps: the first step plays out of the records
      refill_lines read, the second out of the records the first step's own addresses read.  Every index
      of kLine11 goes through every row (3331 is a unit mod 14641) and, transposed, every column, so a
      wrong limb, weight or byte order in any of the eight lines changes a record.
  partial and tiny waves, both pair phases   n in {1, 63, 64, 65, 100} x steps in {1, 2, 3, 7} from an
      even and an odd counter, random boards of digits 0..10, an eighth of them with an exponent 11..17
      (the masked-address path) and a few finished boards handed in: the instruction reads its constant
      operand in every lane whatever the execution mask, so these are the shapes at which a constant
      written or rebuilt under a partial mask goes wrong.
  second persistent iteration with a partial wave   n = 262 144 + 65 for 2 steps: the grid is 256 x 1 024,
      so the last 65 boards run in a second trip of the kernel's board loop with most lanes off.

The host launches the MFMA form for workgroups of up to 256 threads (up to 65 536 boards, one trip through
the board loop) and the VALU form above, so the first two groups run the MFMA form and the last one
checks the form the library picks for that shape.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("boards", "actions", "points", "pot", "flags")
SEED, ENV_BASE = 0x15A, 3
ENTRIES = 11 ** 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def launch(dev, init, steps, step0):
    lib = L()
    n = len(init)
    b = torch.as_tensor(np.ascontiguousarray(init)).to(dev)
    tb = torch.zeros(steps, n, 16, dtype=torch.int8, device=dev)
    ta = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
    tp = torch.zeros(steps, n, dtype=torch.int32, device=dev)
    tpot = torch.zeros(steps, n, 4, dtype=torch.int8, device=dev)
    tf = torch.zeros(steps, n, dtype=torch.uint8, device=dev)
    lib.env_rollout_random(b, steps, tb, ta, tp, tpot, tf, lib.make_rng(lib.RNG_PHILOX, SEED, step0, ENV_BASE), None)
    torch.cuda.synchronize()
    return b, (tb, ta, tp, tpot, tf)


def check(dev, init, steps, step0):
    ob, rec = O.random_rollout_record(init, steps, SEED, step0=step0, env_base=ENV_BASE)
    b, out = launch(dev, init, steps, step0)
    for k, t in zip(FIELDS, out):
        got = t.cpu().numpy()
        bad = np.argwhere(got != rec[k])
        assert len(bad) == 0, (k, len(bad), bad[:4].tolist())
    assert np.array_equal(b.cpu().numpy(), ob), "final boards"


@functools.lru_cache(maxsize=None)
def index_boards():
    """Board k: row i = the base-11 digits (cell j = digit j) of (k + 3331 i) mod 14641; then the transposes."""
    k = np.arange(ENTRIES, dtype=np.int64)
    idx = (k[:, None] + 3331 * np.arange(4)[None, :]) % ENTRIES                   # [k][row]
    g = (idx[:, :, None] // 11 ** np.arange(4)[None, None, :]) % 11               # [k][row][col]
    return np.concatenate([g, g.transpose(0, 2, 1)]).reshape(2 * ENTRIES, 16).astype(np.int8)


def test_index_boards_put_every_index_through_every_line():
    g = index_boards().reshape(2, ENTRIES, 4, 4).astype(np.int64)
    w = 11 ** np.arange(4)
    for i in range(4):
        assert np.array_equal(np.sort((g[0, :, i, :] * w).sum(axis=1)), np.arange(ENTRIES))  # row i
        assert np.array_equal(np.sort((g[1, :, :, i] * w).sum(axis=1)), np.arange(ENTRIES))  # column i, transposed


@pytest.mark.parametrize("step0", [0, 1])
def test_every_table_index_through_every_line(dev, step0):
    check(dev, index_boards(), 2, step0)


@functools.lru_cache(maxsize=None)
def random_boards(n):
    rng = np.random.default_rng(SEED + n)
    b = rng.integers(0, 11, size=(n, 16)).astype(np.int8)
    high = rng.random(n) < 0.125                                  # an exponent 11..17 somewhere on the board
    cell = rng.integers(0, 16, n)
    b[np.nonzero(high)[0], cell[high]] = rng.integers(11, 18, int(high.sum()))
    full = ((np.add.outer(np.arange(4), np.arange(4)) % 2) + 1).reshape(16).astype(np.int8)  # no move left
    for lane in () if n == 1 else {0, n // 3, n - 1} if n < 1000 else {5, 63, 262143, 262144, n - 1}:
        b[lane] = full
    return b


def test_random_boards_mix():
    b = random_boards(100)
    assert (O.legal_mask(b) == 0).sum() >= 3 and ((b.max(axis=1) > 10).sum() >= 5) and (b.max(axis=1) <= 10).sum() >= 50


@pytest.mark.parametrize("step0", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_partial_and_tiny_waves(dev, n, steps, step0):
    check(dev, random_boards(n), steps, step0)


def test_second_persistent_iteration_with_a_partial_wave(dev):
    check(dev, random_boards(262144 + 65), 2, 0)
