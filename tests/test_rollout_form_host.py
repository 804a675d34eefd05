"""Host-only checks of g2048_env_rollout_form (include/g2048.h): which env_rollout_kernel a launch of
n boards x steps takes.  Two independent bits:

  ROLLOUT_FORM_MFMA   the line addresses from the matrix pipe where the grid covers every board, i.e. up to
                      262 144 boards (256 workgroups of up to 1 024 threads); the VALU form above.  (With the
                      wide stores alone the boundary stood at 65 536 boards, workgroups of 256 threads: both
                      sides of that one are checked to take the MFMA form.)
  ROLLOUT_FORM_WIDE   64-bit lane pointers for the record stores; narrow (array bases + 32-bit byte
                      offsets) while the largest offset, below 16 n steps, fits 32 bits: n steps <= 2^28.

The function is pure: no device, and the test-only force-wide switch does not change its answer.
"""

import re

import pytest

from conftest import ROOT
from g2048 import _lib

M, W = 1, 2
LIM = 1 << 28
MFMA_MAX = 256 * 1024


def form(n, steps):
    return _lib.env_rollout_form(n, steps)


def test_header_declares_and_library_exports():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("g2048_env_rollout_form", "g2048_env_rollout_force_wide"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert (_lib.ROLLOUT_FORM_MFMA, _lib.ROLLOUT_FORM_WIDE) == (M, W)


# n * steps = 2^28 - 1 (= 3 * 5 * 29 * 43 * 113 * 127), 2^28 and 2^28 + 1 (= 17 * 15 790 321), each split both ways
@pytest.mark.parametrize("n, steps, wide", [
    (14351, 18705, False), (18705, 14351, False), (1, LIM - 1, False),
    (65536, 4096, False), (1, LIM, False), (1 << 27, 2, False), (4096, 65536, False),
    (17, 15790321, True), (15790321, 17, True), (1, LIM + 1, True),
    (65536, 4095, False), (65536, 4097, True),
])
def test_narrow_wide_boundary(n, steps, wide):
    assert n * steps in (LIM - 1, LIM, LIM + 1) or n == 65536
    assert bool(form(n, steps) & W) == wide, (n, steps, form(n, steps))
    assert bool(form(n, steps) & M) == (n <= MFMA_MAX)


def test_mfma_valu_boundary():
    for steps in (1, 1024, 4095):  # the earlier boundary: one and two waves per SIMD, both MFMA
        assert form(65536, steps) == M and form(65537, steps) == M, steps
    assert form(65536, 4097) == M | W and form(65537, 4096) == M | W  # the two bits are independent
    assert form(65537, 4095) == M                                      # 65 537 * 4 095 = 2^28 - 61 441
    for steps in (1, 64, 1023):    # the boundary: the last board count that the grid covers
        assert form(MFMA_MAX, steps) == M and form(MFMA_MAX + 1, steps) == 0, steps
    assert form(MFMA_MAX, 1025) == M | W and form(MFMA_MAX + 1, 1024) == W
    assert form(MFMA_MAX - 63, 3) == M and form(MFMA_MAX + 65, 3) == 0


def test_edge_inputs():
    assert form(1, 1) == M and form(1, 1024) == M
    assert form(LIM - 1, 1) == 0 and form(LIM - 1, 2) == W        # the largest n: narrow for one step only
    assert form(3, 1 << 62) == M | W                              # n * steps does not fit 64 bits
    assert form(65537, (1 << 63) - 1) == M | W and form(MFMA_MAX + 1, (1 << 63) - 1) == W
    assert form(0, 0) >= 0 and form(0, 7) >= 0 and form(7, 0) >= 0  # accepted: the launch is a no-op
    assert not form(7, 0) & W and not form(0, 1 << 40) & W
    for n, steps in ((-1, 1), (LIM, 1), (LIM + 1, 1), (1 << 40, 1), (1, -1), (65536, -1024), (-1, -1)):
        assert form(n, steps) == _lib.EINVAL, (n, steps)


def test_the_force_wide_switch_does_not_change_the_predicate():
    assert _lib.env_rollout_force_wide(True) is False
    try:
        assert form(65536, 1024) == M and form(MFMA_MAX + 1, 64) == 0
        assert _lib.env_rollout_force_wide(True) is True  # returns the previous setting
    finally:
        assert _lib.env_rollout_force_wide(False) is True
    assert _lib.env_rollout_force_wide(False) is False
