"""Tile-downgrading without a GPU (Tile-downgrading of include/g2048_ntuple.h; g2048_ntuple_downgrade,
downgrade_boards, NTuplePlayer(downgrade=...), play-ntuple --downgrade-from / --reach): the numpy reference of
tests/ntuple_downgrade_reference.py against the sentences of the rule and against everything the header says
follows from it, on the boards the GPU test uses; the argument checks of the Python layer, which come before any
library call; the refusals of the entry point with fake pointers (a refused call enqueues nothing, so no device is
needed); and the command's option checks."""

import ctypes
import re

import numpy as np
import pytest
import torch

import ntuple_downgrade_reference as DG
from conftest import ROOT
from oracle import oracle as O

PARAMS = DG.PARAMS


def all_boards():
    hand = DG.hand_boards()
    return np.ascontiguousarray(np.concatenate([DG.random_boards(), np.stack(list(hand.values()))]))


def unsigned(b):
    return np.asarray(b, np.int8).view(np.uint8).astype(np.int64)


# ------------------------------------------------------------------------------------- the rule -----
def test_the_paper_example_and_the_hand_made_boards():
    hand = DG.hand_boards()

    def run(name, f, l, R):
        out, shift = DG.downgrade(hand[name][None], f, l, R)
        return unsigned(out[0]).tolist(), int(shift[0])

    assert run("paper", 15, 1, 1) == ([14, 13, 12, 11] + [0] * 12, 1)  # 32768, 16384, 8192, 2048 -> 16384, 8192, 4096, 2048
    for f, l, R in PARAMS:
        assert run("empty", f, l, R) == ([0] * 16, 0)
        assert run("ladder", f, l, R) == (list(range(15, 0, -1)) + [0], 0)
        assert run("foreign_only", f, l, R) == (unsigned(hand["foreign_only"]).tolist(), 0)
    assert run("gap_below_lo", 12, 3, 3) == (unsigned(hand["gap_below_lo"]).tolist(), 0)
    assert run("gap_below_lo", 12, 2, 3) == ([11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1] + [0] * 5, 1)
    assert run("gap_at_lo", 12, 3, 3) == ([11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 3, 11, 0, 0, 0], 1)
    assert run("gaps", 15, 1, 1) == ([14, 13, 12, 9, 8, 8, 4, 1, 14, 2] + [0] * 6, 1)      # 14 first
    assert run("gaps", 12, 3, 3) == ([12, 11, 10, 9, 8, 8, 4, 1, 12, 2] + [0] * 6, 3)      # 14, then 11 and 10
    assert run("equal", 12, 3, 3) == ([11] * 16, 2)  # 13 -> 12 -> 11, then the largest is below f
    assert run("equal", 8, 2, 16) == ([7] * 16, 6)
    assert run("below_14", 15, 1, 1)[1] == 0 and run("below_11", 12, 3, 3)[1] == 0
    assert run("below_7", 8, 2, 16)[1] == 0 and run("ones", 2, 1, 16)[1] == 0
    # u > 31 is copied and is no member of P: 15, 14, 13, 12, 9, 2, 2 take part, 11 is the gap
    assert run("foreign", 15, 1, 1) == ([255, 14, 128, 12, 32, 127, 11, 33, 9, 64, 0, 13, 100, 2, 2, 254], 1)
    assert run("many_rounds", 15, 1, 1) == ([14, 1, 14, 1] + [0] * 12, 1)
    assert run("many_rounds", 8, 2, 16) == ([7, 1, 7, 1] + [0] * 12, 8)
    assert run("max31", 2, 1, 16) == ([15, 14, 13, 5] + [0] * 12, 16)


@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_the_vector_reference_is_the_rule_sentence_by_sentence(params):
    boards = all_boards()
    out, shift = DG.downgrade(boards, *params)
    assert out.dtype == np.int8 and shift.dtype == np.uint8
    for i in list(range(0, len(boards), 16)) + list(range(DG.N_RANDOM, len(boards))):
        u, s = DG.scalar_downgrade(boards[i], *params)
        assert unsigned(out[i]).tolist() == u and int(shift[i]) == s, i


@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_the_boards_are_not_the_identity_only(params):
    """At least a quarter of the random boards are translated under every parameter set, and at least a quarter
    twice under every set with two rounds or more; some hand-made board is still not done after its R rounds."""
    f, l, R = params
    shift = DG.downgrade(DG.random_boards(), f, l, R)[1]
    print(params, "shift >= 1: %.3f, >= 2: %.3f, max %d" % ((shift >= 1).mean(), (shift >= 2).mean(), shift.max()))
    assert (shift >= 1).mean() >= 0.25
    if R >= 2:
        assert (shift >= 2).mean() >= 0.25
    hand = np.stack(list(DG.hand_boards().values()))
    out, s = DG.downgrade(hand, f, l, R)
    assert ((s == R) & (DG.downgrade(out, f, l, 1)[1] == 1)).any()


@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_what_follows_from_the_rule(params):
    f, l, R = params
    boards = all_boards()
    gaps = []
    out, shift = DG.downgrade(boards, f, l, R, gaps=gaps)
    u0, u1 = unsigned(boards), unsigned(out)
    part = (u0 >= 1) & (u0 <= 31)
    s = shift.astype(np.int64)
    # m falls by exactly one per round applied
    m0, m1 = np.where(part, u0, 0).max(1), np.where(part, u1, 0).max(1)
    assert np.array_equal(m0 - m1, s) and s.max() <= R and (s[m0 < f] == 0).all()
    # <, == and > between any two cells
    assert np.array_equal(np.sign(u0[:, :, None] - u0[:, None, :]), np.sign(u1[:, :, None] - u1[:, None, :]))
    # empty cells stay empty, cells that take no part are copied, shift 0 is the board byte for byte
    assert np.array_equal(u0 == 0, u1 == 0) and np.array_equal(u0[~part], u1[~part])
    assert np.array_equal(out[s == 0], boards[s == 0]) and (out[s > 0] != boards[s > 0]).any(1).all()
    # round by round: the gap was absent and in [l, m), cells <= j are untouched, the cell map is that of the round
    cur = boards
    for j in gaps:
        uc = unsigned(cur)
        go = j >= 0
        assert not (uc[go] == j[go, None]).any() and (j[go] >= l).all()
        assert (j[go] < np.where((uc >= 1) & (uc <= 31), uc, 0).max(1)[go]).all()
        nxt = DG.apply_round(cur, j)
        assert np.array_equal(unsigned(nxt)[uc <= j[:, None]], uc[uc <= j[:, None]])
        cur = nxt
    assert np.array_equal(cur, out) and np.array_equal(sum((j >= 0).astype(np.int64) for j in gaps), s)
    # a board that is done stays done: no gap is skipped and taken later
    done = s < R
    assert (DG.downgrade(out[done], f, l, 1)[1] == 0).all()


@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_moves_and_legality_are_those_of_the_original(params):
    """On the boards the engine can hold (every cell 0..17): the legal mask is kept, and move(., a) commutes with
    every round, move(D(b), a) = D(move(b, a)) cell for cell -- the same tiles go to the same cells.  Merge points
    are not kept: those of halved tiles are halved, which some board must show."""
    f, l, R = params
    boards = all_boards()
    boards = boards[((boards >= 0) & (boards <= 17)).all(1)]
    gaps = []
    out, shift = DG.downgrade(boards, f, l, R, gaps=gaps)
    assert np.array_equal(O.legal_mask(out), O.legal_mask(boards))
    n = len(boards)
    acts = np.tile(np.arange(4), n)
    cur = boards
    halved = 0
    for j in gaps:
        nxt = DG.apply_round(cur, j)
        mc, pc, _ = O.move(np.repeat(cur, 4, axis=0), acts)
        mn, pn, _ = O.move(np.repeat(nxt, 4, axis=0), acts)
        assert np.array_equal(mn, DG.apply_round(mc, np.repeat(j, 4)))
        assert (pn <= pc).all()
        halved += int((pn < pc).sum())
        cur = nxt
    assert np.array_equal(cur, out) and halved > 0


# ----------------------------------------------------------------------- the header and the ABI -----
def test_header_and_exports():
    from g2048 import _lib
    raw = (ROOT / "include" / "g2048_ntuple.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bg2048_ntuple_downgrade\s*\(", text)
    flat = " ".join(raw.replace(" * ", " ").split())
    for phrase in ("Tile-downgrading (g2048_ntuple_downgrade", "tests/ntuple_downgrade_reference.py",
                   "j = the largest value with l <= j < m that is not in P", "every cell with j < u <= 31 becomes u - 1",
                   "m falls by exactly one", "shift == 0 leaves the board byte for byte",
                   "32768, 16384, 8192, 2048 becomes 16384, 8192, 4096, 2048", "What is NOT preserved",
                   # the old sentences stay
                   "The choice.  move(b, a), its merge points pts(b, a) and legality", "Optimistic initialisation",
                   "8 T w0", "Carousel (g2048_ntuple_staged_carousel", "The search (g2048_ntuple_search)",
                   "At d = 1 this is g2048_ntuple_choose bit for bit"):
        assert " ".join(phrase.split()) in flat, phrase
    lib = _lib.load()
    assert lib.g2048_ntuple_downgrade.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_int32] * 3
    assert lib.g2048_ntuple_downgrade.restype is ctypes.c_int and callable(_lib.ntuple_downgrade)


def test_library_refusals():
    """Host-only, with fake pointers: every refusal of the header returns G2048_EINVAL before anything is enqueued,
    and n = 0 is accepted with any pointers."""
    from g2048 import _lib
    fn = _lib.load().g2048_ntuple_downgrade
    E, B, OUT, SH = _lib.EINVAL, 0x1000, 0x2000, 0x3001
    for f, l, R in ((1, 1, 1), (32, 1, 1), (0, 1, 1), (-15, 1, 1), (15, 0, 1), (15, 15, 1), (15, 16, 1), (2, 2, 1),
                    (15, -1, 1), (15, 1, 0), (15, 1, 17), (15, 1, -1)):
        assert fn(None, B, OUT, SH, 64, f, l, R) == E, (f, l, R)
        assert fn(None, B, OUT, SH, 0, f, l, R) == E, (f, l, R)  # also without boards
    for n in (-1, 1 << 31, 1 << 40):
        assert fn(None, B, OUT, SH, n, 15, 1, 1) == E, n
    for b, o in ((None, OUT), (B, None), (None, None), (B + 8, OUT), (B, OUT + 4), (B + 1, B + 1)):
        assert fn(None, b, o, SH, 64, 15, 1, 1) == E, (b, o)
        assert fn(None, b, o, None, 64, 15, 1, 1) == E, (b, o)
    for f, l, R in ((2, 1, 1), (31, 30, 16), (15, 1, 1)):
        assert fn(None, None, None, None, 0, f, l, R) == 0  # n = 0: a no-op


# ------------------------------------------------------------------------------ the Python layer -----
BAD_TRIPLES = [(2, 2, 1), (3, 2, 1), (65536, 2, 1), (0, 2, 1), (-4, 2, 1), (4096, 1, 1), (4096, 0, 1), (4096, 3, 1),
               (4096, 4096, 1), (4096, 8192, 1), (4, 4, 1), (4096, 2, 0), (4096, 2, 17), (4096, 2, -1), (4096.0, 2, 1),
               (4096, 2, 1.5), (True, 2, 1), ("4096", 2, 1)]


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from g2048 import _lib
    from g2048.ntuple import NTupleNet, NTuplePlayer, downgrade_params, downgrade_boards

    def no(*a, **kw):
        raise AssertionError("a library call before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no)
    monkeypatch.setattr(_lib, "_call", no)
    boards = torch.zeros(4, 16, dtype=torch.int8)
    net = NTupleNet("lines-squares-4", "cpu")
    for bad in BAD_TRIPLES:
        with pytest.raises(ValueError):
            downgrade_boards(boards, *bad)
        with pytest.raises(ValueError):
            NTuplePlayer(net, downgrade=bad)
    for bad in ((4096, 2), (4096,), 4096, (4096, 2, 1, 1), "4096,2,1"):
        with pytest.raises(ValueError):
            NTuplePlayer(net, downgrade=bad)
    assert downgrade_params(4, 2, 1) == (2, 1, 1) and downgrade_params(32768, 16384, 16) == (15, 14, 16)
    assert downgrade_params(32768) == (15, 1, 1)
    assert downgrade_params(np.int64(4096), np.uint8(2), np.int32(3)) == (12, 1, 3)  # what operator.index takes
    for bad in ((np.float64(4096), 2, 1), (np.bool_(True), 2, 1), (4096, 2, np.float32(1))):
        with pytest.raises(ValueError):
            downgrade_params(*bad)
    p = NTuplePlayer(net, 2, "wide", downgrade=[np.int64(4096), 2, 2])
    assert p.downgrade == (4096, 2, 2) and p._downgrade_exps == (12, 1, 2)
    plain = NTuplePlayer(net)
    assert plain.downgrade is None and plain._downgrade_exps is None
    assert NTuplePlayer(net, 3).depth == 3  # the old signature, positionally


def test_a_cpu_tensor_is_refused_by_the_binding():
    from g2048 import _lib
    from g2048.ntuple import downgrade_boards
    with pytest.raises(_lib.G2048Error):
        downgrade_boards(torch.zeros(4, 16, dtype=torch.int8), 4096)
    b = torch.zeros(4, 16, dtype=torch.int8)
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_downgrade(b, torch.zeros(3, 16, dtype=torch.int8), None, 12, 1, 1)
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_downgrade(b, b, torch.zeros(3, dtype=torch.uint8), 12, 1, 1)


# ---------------------------------------------------------------------------------- the command -----
def test_command_options(tmp_path):
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["play-ntuple", "--help"])
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    assert r.exit_code == 0, out
    for opt in ("--downgrade-from", "--downgrade-lo", "--downgrade-rounds", "--reach", "--depth", "--max-moves"):
        assert opt in out, opt
    model = str(tmp_path / "none.pt")  # never read: every refusal comes before the net is loaded
    for extra, word in ((["--downgrade-lo", "4"], "--downgrade-lo needs --downgrade-from"),
                        (["--downgrade-rounds", "2"], "--downgrade-rounds needs --downgrade-from"),
                        (["--downgrade-from", "3"], "from_tile"), (["--downgrade-from", "2"], "from_tile"),
                        (["--downgrade-from", "65536"], "from_tile"),
                        (["--downgrade-from", "4096", "--downgrade-lo", "4096"], "lo_tile"),
                        (["--downgrade-from", "4096", "--downgrade-lo", "1"], "lo_tile"),
                        (["--downgrade-from", "4096", "--downgrade-rounds", "0"], "rounds"),
                        (["--downgrade-from", "4096", "--downgrade-rounds", "17"], "rounds"),
                        (["--reach", "4096,x"], "--reach"), (["--reach", "3"], "--reach"),
                        (["--reach", "0"], "--reach"), (["--depth", "4"], "--depth")):
        r = CliRunner().invoke(train.app, ["play-ntuple", model] + extra)
        lines = r.output.strip().splitlines()
        assert r.exit_code == 1 and len(lines) == 1 and lines[0].startswith("Error:") and word in lines[0], (extra, r.output)
    text = (ROOT / "README.md").read_text() + (ROOT / "INTEGRATION.md").read_text()
    assert "--downgrade-from" in text and "--reach" in text


def test_the_command_without_the_new_options_parses_as_before(monkeypatch, tmp_path):
    """No GPU: the net's loader and the player are replaced, and what the command hands them is what it handed them
    before -- the model path, the depth, no downgrade -- and its two result lines are the old ones alone."""
    from typer.testing import CliRunner
    import g2048.ntuple as NT
    import train
    seen = {}

    class Player:
        def __init__(self, net, depth=1, form="auto", downgrade=None):
            seen.update(net=net, depth=depth, form=form, downgrade=downgrade)

        def play_games(self, games, max_moves, seeds=None):
            seen.update(games=games, max_moves=max_moves, seeds=seeds)
            return {"scores": [100, 300, 200, 400], "max_tiles": [512, 1024, 4096, 256]}

    monkeypatch.setattr(NT.NTupleNet, "load", classmethod(lambda cls, path, device="cuda": ("net", str(path))))
    monkeypatch.setattr(NT, "NTuplePlayer", Player)
    old = ["Eval Results - Max: 400, Avg: 250.0, Median: 300", "Tiles Reached - 512: 75.0%, 1024: 50.0%, 2048: 25.0%"]
    r = CliRunner().invoke(train.app, ["play-ntuple", "m.pt", "-g", "4", "--max-moves", "9", "--depth", "2"])
    assert r.exit_code == 0 and r.output.strip().splitlines() == old, r.output
    assert seen == dict(net=("net", "m.pt"), depth=2, form="auto", downgrade=None, games=4, max_moves=9, seeds=[0, 1, 2, 3])
    r = CliRunner().invoke(train.app, ["play-ntuple", "m.pt", "-g", "4", "--downgrade-from", "2048", "--downgrade-rounds",
                                       "3", "--reach", "256,4096, 8192"])
    assert r.exit_code == 0, r.output
    assert r.output.strip().splitlines() == old + ["Tiles Reached (--reach) - 256: 100.0%, 4096: 25.0%, 8192: 0.0%"]
    assert seen["downgrade"] == (2048, 2, 3) and seen["depth"] == 1
