"""CPU-side checks of the expectimax search: the numpy reference (tests/expectimax_reference.py)
against an independent scalar recursion in Python ints written from the definition in include/g2048.h,
its pinned leaf counts on the roots the GPU tests use, and the seams (C ABI declaration and export, the
wrapper's refusal of CPU tensors, the player's argument checks, the `play-expectimax` command's
options).

Pinned with weights (1, 64, 128) on the 30 roots of mc_reference.roots(): 76 / 3 107 / 207 395 leaves
at depth 1 / 2 / 3; the depth-3 tree holds 31 boards without a legal move (M = 0): the 8 finished roots
and 23 below them; the best action changes on 11 roots from depth 1 to 2 and on 7 more from 2 to 3;
at depth 1 the two top values tie on 14 roots, at depth 3 on none.  Depth 4 on the eight crowded
roots: 277 923 leaves, 224 boards without a legal move, all below the roots."""

import functools
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from expectimax_reference import CROWDED, S, WEIGHTS, expectimax_ref, legal_best
from mc_reference import roots
from oracle import oracle as O


# ---- the scalar recursion: Python ints, one board at a time, written from the header's definition ----
def _move(b, a):
    out, pts, _ = O.move(np.array(b, np.int8)[None], a)
    return tuple(int(x) for x in out[0]), int(pts[0])


def _leaf(s, w):
    mono, empt = O.potentials(np.array(s, np.int8)[None])
    return S * (w[1] * int(mono[0]) + w[2] * int(empt[0]))


def scalar_A(s, k, w, count):
    if k == 0:
        count[0] += 1
        return _leaf(s, w)
    cells = [c for c in range(16) if s[c] == 0]
    total = 0
    for c in reversed(cells):  # any order: the sum is exact
        for tile, weight in ((2, 1), (1, 9)):
            total += weight * scalar_M(s[:c] + (tile,) + s[c + 1:], k, w, count)
    return total // (10 * len(cells))


def scalar_M(b, k, w, count):
    best = 0
    for a in range(4):
        s, pts = _move(b, a)
        if s != b:
            best = max(best, S * w[0] * pts + scalar_A(s, k - 1, w, count))
    return best


def scalar_values(b, d, w):
    b = tuple(int(x) for x in b)
    values, leaves = [], []
    for a in range(4):
        s, pts = _move(b, a)
        count = [0]
        values.append(S * w[0] * pts + scalar_A(s, d - 1, w, count) if s != b else -1)
        leaves.append(count[0])
    return values, leaves


@pytest.mark.parametrize("weights", [WEIGHTS, (3, 0, 4096)])
def test_reference_matches_scalar_recursion(weights):
    """Three small roots (3, 1 and 1 empty cells, each with an illegal action) at depth 1..3."""
    small = roots()[[5, 15, 25]]
    assert O.legal_mask(small).tolist() == [13, 13, 7]
    for d in (1, 2, 3):
        val, lv = expectimax_ref(small, d, weights)
        for i, b in enumerate(small):
            sv, sl = scalar_values(b, d, weights)
            assert val[i].tolist() == sv and lv[i].tolist() == sl, (d, i)


@functools.lru_cache(maxsize=None)
def _ref(d):
    st = {}
    val, lv = expectimax_ref(roots(), d, WEIGHTS, st)
    return val, lv, st


def _top_two_tie(val):
    s = np.sort(val, 1)
    return (s[:, 3] >= 0) & (s[:, 3] == s[:, 2])


def test_pinned_leaf_counts():
    R = roots()
    assert len(R) == 30 and int((O.legal_mask(R) == 0).sum()) == 8
    assert int((R[9] == 0).sum()) == 0 and O.legal_mask(R[9:10])[0] != 0  # live, no empty cell
    assert int((R == 0).sum(1).max()) == 14                                 # full fan-out
    for d, leaves in ((1, 76), (2, 3107), (3, 207395)):
        val, lv, st = _ref(d)
        assert st["leaves"] == leaves == int(lv.sum())
        assert (lv[val < 0] == 0).all() and (lv[val >= 0] > 0).all()
    assert _ref(3)[2]["dead"] == 31 and _ref(3)[2]["dead_roots"] == 8
    best = [legal_best(R, _ref(d)[0])[1] for d in (1, 2, 3)]
    assert int((best[0] != best[1]).sum()) == 11 and int((best[1] != best[2]).sum()) == 7
    assert int(_top_two_tie(_ref(1)[0]).sum()) == 14 and int(_top_two_tie(_ref(3)[0]).sum()) == 0
    st = {}
    _, lv = expectimax_ref(R[CROWDED], 4, WEIGHTS, st)
    assert st == {"leaves": 277923, "dead": 224, "dead_roots": 0} and int(lv.sum()) == 277923


def test_values_are_bounded_and_illegal_is_minus_one():
    val = _ref(3)[0]
    assert val.min() == -1 and val.max() < 1 << 50
    finished = O.legal_mask(roots()) == 0
    assert (val[finished] == -1).all() and (legal_best(roots(), val)[1][finished] == 0xFF).all()


def test_header_declares_and_library_exports():
    from g2048 import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("g2048_expectimax_workspace_bytes", "g2048_expectimax"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert (_lib.EMAX_AUTO, _lib.EMAX_NARROW, _lib.EMAX_WIDE) == (0, 1, 2)


def test_workspace_bytes():
    """Host-only: the size of every accepted shape, 0 for what the call refuses."""
    from g2048 import _lib
    N, W, A = _lib.EMAX_NARROW, _lib.EMAX_WIDE, _lib.EMAX_AUTO
    assert _lib.expectimax_workspace_bytes(1, 1, N) >= 16
    assert _lib.expectimax_workspace_bytes(30, 3, W) >= 30 * (4 * 8 + 4 * 8 + 4 * 4 + 4)
    for n, d, f in ((30, 3, W), (191, 3, W), (192, 3, N), (30, 2, N), (30, 1, N), (1024, 4, W), (1 << 17, 4, N)):
        assert _lib.expectimax_workspace_bytes(n, d, A) == _lib.expectimax_workspace_bytes(n, d, f), (n, d)  # AUTO
    assert _lib.expectimax_workspace_bytes(0, 2, W) > 0
    for n, d, f in ((1, 0, N), (1, 5, N), (1, 1, W), (1, 2, 3), (1, 2, -1), (-1, 2, N), (1 << 24, 2, N), (1 << 17, 2, W),
                    (1 << 62, 2, N), (1 << 62, 4, A)):
        assert _lib.expectimax_workspace_bytes(n, d, f) == 0, (n, d, f)
    assert _lib.expectimax_workspace_bytes((1 << 24) - 1, 2, N) > 0
    assert _lib.expectimax_workspace_bytes((1 << 17) - 1, 2, W) > 0


def test_cpu_tensors_are_rejected():
    from g2048 import _lib
    n = 4
    with pytest.raises(_lib.G2048Error):
        _lib.expectimax(torch.zeros(n, 16, dtype=torch.int8), 2, WEIGHTS, torch.zeros(n, 4, dtype=torch.int64),
                        torch.zeros(n, 4, dtype=torch.int64), torch.zeros(n, dtype=torch.uint8),
                        torch.zeros(n, dtype=torch.uint8), torch.zeros(1024, dtype=torch.uint8))


@pytest.mark.parametrize("depth,weights,form", [(0, WEIGHTS, "auto"), (5, WEIGHTS, "auto"), (-1, WEIGHTS, "narrow"),
                                                (2, (1, 64, 4097), "auto"), (2, (-1, 64, 128), "auto"),
                                                (2, (1, 64), "auto"), (2, WEIGHTS, "broad"), (2, WEIGHTS, 1),
                                                (1, WEIGHTS, "wide")])
def test_player_rejects_bad_arguments(depth, weights, form):
    from g2048.search import ExpectimaxPlayer
    with pytest.raises(ValueError):
        ExpectimaxPlayer(depth, weights, "cuda", form)


def test_player_accepts_the_range_ends():
    from g2048.search import ExpectimaxPlayer
    for depth, weights, form in ((1, (0, 0, 0), "narrow"), (4, (4096, 4096, 4096), "wide"), (3, WEIGHTS, "auto")):
        p = ExpectimaxPlayer(depth, weights, "cuda", form)  # no device is touched before a search
        assert (p.depth, p.weights, p.form) == (depth, weights, form)
    assert ExpectimaxPlayer(2).weights == WEIGHTS


def test_play_expectimax_help_lists_its_options():
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["play-expectimax", "--help"])
    assert r.exit_code == 0, r.output
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    for opt in ("--games", "-g", "--depth", "--w-points", "--w-mono", "--w-empt", "--max-moves"):
        assert opt in out, opt
