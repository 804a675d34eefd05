"""CPU-side checks of the n-tuple network: the numpy reference (tests/ntuple_reference.py) against an
independent scalar implementation in Python ints written from the definition in include/g2048_ntuple.h,
the properties the definition promises (symmetry invariance, the clamp at exponent 15), the pinned
counts of the cases the GPU tests rely on, and the seams (C ABI declaration and export, the wrappers'
refusal of CPU tensors, the argument checks of net / trainer / player, the two commands' options, a
save / load round trip).

Pinned on the reference (TD_STEPS = 200 steps, game seed 31): see PINNED below -- per TD case the envs
that ended a game (pending = 2), the dead boards met, the steps in which two envs add to one weight,
the updates hitting one weight twice, and the negative deltas the rounding rule takes to 0 where a
floor would give -1."""

import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import ntuple_reference as R
from conftest import ROOT
from mc_reference import roots
from oracle import oracle as O

S = 4096


# ---- the scalar implementation: Python ints, one board at a time, written from the header ----
def _sym_maps():
    """The 8 symmetries as coordinate maps (r, c) -> (r', c'): 4 quarter turns x an optional mirror."""
    turn = [lambda r, c: (r, c), lambda r, c: (c, 3 - r), lambda r, c: (3 - r, 3 - c), lambda r, c: (3 - c, r)]
    maps = []
    for mirror in (False, True):
        for f in turn:
            maps.append((lambda r, c, f=f, m=mirror: f(r, 3 - c) if m else f(r, c)))
    return maps


def scalar_apply(b, m):
    """g(b): the tile of (r, c) goes to m(r, c)."""
    out = [0] * 16
    for r in range(4):
        for c in range(4):
            r2, c2 = m(r, c)
            out[4 * r2 + c2] = b[4 * r + c]
    return tuple(out)


def scalar_hits(cells, b):
    """The 8 T (tuple, index) pairs V(b) reads, with multiplicity."""
    hits = []
    for m in _sym_maps():
        gb = scalar_apply(b, m)
        for t, tup in enumerate(cells):
            hits.append((t, sum(min(gb[c], 15) << (4 * j) for j, c in enumerate(tup))))
    return hits


def scalar_value(cells, w, b):
    return sum(int(w[t][i]) for t, i in scalar_hits(cells, b))


def _move(b, a):
    out, pts, _ = O.move(np.array(b, np.int8)[None], a)
    return tuple(int(x) for x in out[0]), int(pts[0])


def scalar_choose(cells, w, b):
    q, best = [], 0xFF
    for a in range(4):
        s, pts = _move(b, a)
        q.append(S * pts + scalar_value(cells, w, s) if s != b else None)
        if q[a] is not None and (best == 0xFF or q[a] > q[best]):
            best = a
    return q, best


def _wrap32(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def scalar_td(cells, w, boards, steps, lr_shift, seed, counter):
    """The TD step of the header, env by env; w: list of lists of Python ints, updated in place."""
    n = len(boards)
    boards = [tuple(int(x) for x in b) for b in boards]
    after, pending, run = [None] * n, [0] * n, [0] * n
    stats = [0, 0, 0, 0]
    for s in range(steps):
        adds, plan = [], []
        for i in range(n):  # every read sees the weights before the step's updates
            q, best = scalar_choose(cells, w, boards[i])
            target = q[best] if best != 0xFF else 0
            if pending[i]:
                delta = (0 if pending[i] == 2 else target) - scalar_value(cells, w, after[i])
                D = max(-(1 << 30), min(1 << 30, (delta + (1 << (lr_shift - 1))) >> lr_shift))
                adds += [(t, k, D) for t, k in scalar_hits(cells, after[i])]
                stats[3] += 1
            plan.append(best)
        for t, k, D in adds:
            w[t][k] = _wrap32(w[t][k] + D)
        acts = [0 if a == 0xFF else a for a in plan]
        nb, pts, done = R.env_step_auto_reset(np.array(boards, np.int8), np.array(acts), seed, counter + s)
        for i in range(n):
            run[i] += int(pts[i])
            if done[i]:
                stats[0] += 1
                stats[1] += run[i]
                stats[2] = max(stats[2], run[i])
                run[i] = 0
            if plan[i] != 0xFF:
                after[i] = _move(boards[i], plan[i])[0]
                pending[i] = 2 if done[i] else 1
            else:
                pending[i] = 0
            boards[i] = tuple(int(x) for x in nb[i])
    return boards, after, pending, run, stats


def small_boards():
    """Three roots, a finished one, the ending and the dead board, one with exponents 15 and 16."""
    big = np.array([16, 15, 14, 0, 1, 1, 2, 0, 0, 3, 3, 0, 15, 16, 0, 0], np.int8)
    return np.stack([*roots()[[5, 15, 25, 17]], R.ENDING, R.DEAD, big])


@pytest.mark.parametrize("net", ["lines-squares-4", "t1k1", "t8k3"])
def test_reference_matches_scalar_value_and_choice(net):
    cells = R.NETS[net]
    w = R.random_weights(cells, 3)
    boards = small_boards()
    val = R.value(cells, w, boards)
    q, legal, best, _ = R.choose(cells, w, boards)
    assert (legal == 0).sum() >= 2 and ((legal != 0) & (legal != 15)).any()
    for i, b in enumerate(boards):
        b = tuple(int(x) for x in b)
        assert int(val[i]) == scalar_value(cells, w, b)
        sq, sbest = scalar_choose(cells, w, b)
        assert [R.I64_MIN if x is None else x for x in sq] == q[i].tolist() and sbest == int(best[i])


@pytest.mark.parametrize("rand", [False, True])
def test_reference_matches_scalar_td(rand):
    """Six envs (ending, fresh, dead boards), 20 steps at lr_shift 4, where games end and restart, two
    envs add to one weight and D is clamped."""
    cells = R.NETS["lines-squares-4"]
    w0 = R.random_weights(cells, 5, bits=20) if rand else np.zeros((5, 65536), np.int32)
    seed = 3 if rand else 9
    boards = O.reset(6, seed=seed, step_idx=0)
    boards[0], boards[2], boards[5] = R.ENDING, R.ENDING, R.DEAD
    ev = {}
    st = R.td(R.TDState(cells, w0, boards), 20, 4, seed=seed, counter=1, events=ev)
    assert ev["ended"] > 0 and ev["dead"] > 0 and ev["double"] > 0 and ev["shared"] > 0
    assert ev["clamped"] > 0  # 40 adds of delta / 16 overshoot: the weights diverge until D is clamped
    w = [[int(x) for x in row] for row in w0]
    sb, sa, sp, sr, ss = scalar_td(cells, w, boards, 20, 4, seed, 1)
    assert np.array_equal(st.weights, np.array(w, np.int64).astype(np.int32))
    assert np.array_equal(st.boards, np.array(sb, np.int8)) and st.pending.tolist() == sp
    assert st.run_score.tolist() == sr and st.stats.tolist() == ss
    for i in range(6):
        if sp[i]:
            assert tuple(st.after[i]) == sa[i]


def test_td_wraps_and_clamps():
    """One env whose pending after-state reads weights near the int32 ends: D is clamped to -2^30 and the
    weights wrap."""
    cells = [[0, 1], [2, 3]]
    after = np.zeros((1, 16), np.int8)  # the empty board: all 8 symmetries of both tuples read index 0
    top, bottom = (1 << 31) - 1, -(1 << 31)
    # the after-state of ENDING (LEFT, 16 points) has one empty cell: it reads no index 0, target = 16 S
    w = np.zeros((2, 256), np.int32)
    w[0, 0] = top
    st = R.TDState(cells, w, R.ENDING[None], after, pending=[1])
    ev = {}
    R.td(st, 1, 1, seed=1, counter=0, events=ev)
    # V(after) = 8 (2^31 - 1): (delta + 1) >> 1 = 32772 - 2^33 < -2^30, so D = -2^30, added 8 times
    assert ev["clamped"] == 1 and ev["double"] == 1
    assert st.weights[:, 0].tolist() == [_wrap32(top - 8 * (1 << 30)), _wrap32(-8 * (1 << 30))]
    assert st.weights[0, 0] != _wrap32(top + 8 * (32772 - (1 << 33)))  # what no clamp would give
    w[:, 0] = top, bottom
    st = R.TDState(cells, w, R.ENDING[None], after, pending=[1])
    R.td(st, 1, 1, seed=1, counter=0, events=ev)
    # V(after) = -8, delta = 16 S + 8, D = 32772: the first weight wraps past 2^31 - 1
    assert ev["clamped"] == 1
    assert st.weights[:, 0].tolist() == [bottom + 8 * 32772 - 1, bottom + 8 * 32772]


def test_value_is_invariant_under_the_eight_symmetries():
    rng = np.random.default_rng(11)
    boards = rng.integers(0, 17, size=(40, 16)).astype(np.int8)
    for net in ("lines-squares-4", "t8k3"):
        cells = R.NETS[net]
        w = R.random_weights(cells, 4)
        v = R.value(cells, w, boards)
        seen = set()
        for m in _sym_maps():
            gb = np.array([scalar_apply(tuple(b), m) for b in boards], np.int8)
            seen.add(gb[0].tobytes())
            assert np.array_equal(R.value(cells, w, gb), v)
        assert len(seen) == 8
        assert len({int(R.value(cells, w, b[None])[0]) for b in boards}) > 30  # not a constant


def test_exponents_clamp_at_15():
    """A 16 indexes like a 15; a 14 does not."""
    cells = R.NETS["t1k1"]
    w = R.random_weights(cells, 8)
    b = np.zeros((3, 16), np.int8)
    b[0, 5], b[1, 5], b[2, 5] = 16, 15, 14
    v = R.value(cells, w, b)
    assert v[0] == v[1] != v[2]
    assert int(R.indices(cells, b).max()) == 15


@functools.lru_cache(maxsize=None)
def td_events(name):
    cells, w, boards, lr_shift = R.td_start(name)
    ev = {}
    st = R.td(R.TDState(cells, w, boards), R.TD_STEPS, lr_shift, R.TD_SEED, 1, events=ev)
    return ev, st


PINNED = {  # name: (ended, dead, shared, double, neg_round, games finished, updates applied)
    "n1-zero": (1, 0, 0, 198, 18, 1, 199), "n1-random": (2, 0, 0, 189, 5, 2, 199),
    "n64-zero": (47, 1, 199, 12348, 175, 48, 12735), "n64-random": (102, 1, 199, 11851, 422, 103, 12735),
    "n300-zero": (191, 1, 199, 57736, 446, 192, 59699), "n300-random": (500, 1, 199, 55721, 1975, 501, 59699),
    "n64-t8k3": (110, 1, 199, 12735, 412, 111, 12735),
}


@pytest.mark.parametrize("name", sorted(R.TD_CASES))
def test_pinned_td_counts(name):
    ev, st = td_events(name)
    got = (ev["ended"], ev["dead"], ev["shared"], ev["double"], ev["neg_round"], int(st.stats[0]), int(st.stats[3]))
    assert got == PINNED[name]
    n = R.TD_CASES[name][1]
    assert ev["ended"] > 0 and ev["double"] > 0 and ev["neg_round"] > 0 and ev["clamped"] == 0
    assert (ev["dead"] > 0 and ev["shared"] > 0) == (n > 1)


def test_value_boards_cover_the_cases():
    b = R.value_boards()
    legal = O.legal_mask(b)
    assert len(b) == 33 and (legal == 0).sum() == 8 and ((legal != 0) & (legal != 15)).any()
    assert (b == 15).any() and (b == 16).any()


def test_header_declares_and_library_exports():
    from g2048 import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048_ntuple.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_weight_count", "g2048_ntuple_value", "g2048_ntuple_choose",
                 "g2048_ntuple_td_workspace_bytes", "g2048_ntuple_td"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert "g2048_ntuple.h" in _lib.HEADERS
    assert (_lib.NT_MAX_TUPLES, _lib.NT_MAX_LEN, _lib.NT_FRAC_BITS) == (8, 6, 12)
    assert ctypes.sizeof(_lib.NtNet) == 208 and _lib.NtNet.weights.offset == 200
    assert "wrap" in (ROOT / "include" / "g2048_ntuple.h").read_text().lower()  # the range is documented


def test_weight_count_and_workspace_bytes():
    """Host-only: sizes of what is accepted, 0 for what the calls refuse."""
    from g2048 import _lib
    lib = _lib.load()

    def count(cells, K=None, ptr=0x1000):
        flat = [c for t in cells for c in t]
        net = _lib.NtNet(len(cells), K if K is not None else len(cells[0]), (ctypes.c_int32 * 48)(*flat), ptr)
        return lib.g2048_ntuple_weight_count(ctypes.byref(net))

    assert count(R.PRESETS["lines-squares-4"]) == 5 * 16 ** 4 and count(R.PRESETS["4x6"]) == 4 * 16 ** 6
    assert count([[5]]) == 16 and count([[0, 1, 2, 3, 4, 5]] * 8) == 8 * 16 ** 6
    assert count([[0, 1]], ptr=0) == 0 and count([[0, 1]], ptr=0x1008) == 0      # null / misaligned weights
    assert count([[0, 16]]) == 0 and count([[0, -1]]) == 0 and count([[3, 3]]) == 0  # cell range, repeats
    assert count([[0, 1], [2, 2]]) == 0 and count([[0]] * 9, K=1) == 0 and count([[0]], K=0) == 0
    assert count([[0, 1, 2, 3, 4, 5, 6]], K=7) == 0
    assert lib.g2048_ntuple_weight_count(None) == 0
    assert _lib.ntuple_td_workspace_bytes(300) >= 300 * 5 and _lib.ntuple_td_workspace_bytes(0) > 0
    assert _lib.ntuple_td_workspace_bytes((1 << 28) - 1) > 0
    assert _lib.ntuple_td_workspace_bytes(1 << 28) == 0 and _lib.ntuple_td_workspace_bytes(-1) == 0


def test_cpu_tensors_are_rejected():
    from g2048 import _lib
    n = 4
    w = torch.zeros(5, 65536, dtype=torch.int32)
    with pytest.raises(_lib.G2048Error):
        _lib.make_ntuple_net(R.PRESETS["lines-squares-4"], w)
    net = _lib.NtNet(1, 1, (ctypes.c_int32 * 48)(5), 0x1000)  # never dereferenced: refused before
    b = torch.zeros(n, 16, dtype=torch.int8)
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_value(net, b, torch.zeros(n, dtype=torch.int64))
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_choose(net, b, torch.zeros(n, 4, dtype=torch.int64), torch.zeros(n, dtype=torch.uint8),
                           torch.zeros(n, dtype=torch.uint8))
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_td(net, b, b.clone(), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64), 1, 10,
                       _lib.make_rng(), torch.zeros(4, dtype=torch.int64), torch.zeros(1024, dtype=torch.uint8))


@pytest.mark.parametrize("cells", ["no-such-preset", [], [[0]] * 9, [[0, 1], [2]], [[0, 1, 2, 3, 4, 5, 6]],
                                   [[0, 16]], [[-1, 2]], [[4, 4]], [[]]])
def test_net_rejects_bad_cells(cells):
    from g2048.ntuple import NTupleNet
    with pytest.raises(ValueError):
        NTupleNet(cells, "cpu")


def test_net_trainer_player_argument_checks():
    from g2048.ntuple import PRESETS, NTupleNet, NTuplePlayer, NTupleTrainer
    assert PRESETS == R.PRESETS
    net = NTupleNet("lines-squares-4", "cpu")
    assert net.cells == R.PRESETS["lines-squares-4"] and net.weights.shape == (5, 65536)
    assert net.weights.dtype == torch.int32 and int(net.weights.abs().sum()) == 0
    assert NTupleNet([[0, 1, 2]], "cpu").weights.shape == (1, 4096)
    for bad in (torch.zeros(5, 65536), torch.zeros(4, 65536, dtype=torch.int32)):
        with pytest.raises(ValueError):
            NTupleNet("lines-squares-4", "cpu", bad)
    for kw in ({"envs": 0}, {"envs": 1 << 28}, {"lr_shift": 0}, {"lr_shift": 31}):
        with pytest.raises(ValueError):
            NTupleTrainer(net, **kw)
    tr = NTupleTrainer(net, envs=(1 << 28) - 1, lr_shift=30, seed=3)  # no device is touched before train()
    assert (tr.envs, tr.lr_shift, tr.seed) == ((1 << 28) - 1, 30, 3)
    assert (NTupleTrainer(net).envs, NTupleTrainer(net).lr_shift) == (256, 10)
    with pytest.raises(ValueError):
        tr.train(0)
    with pytest.raises(ValueError):
        NTuplePlayer("lines-squares-4")
    assert NTuplePlayer(net).device == torch.device("cpu")


def test_save_load_round_trip(tmp_path):
    from g2048.ntuple import NTupleNet
    cells = R.NETS["t8k3"]
    net = NTupleNet(cells, "cpu", torch.from_numpy(R.random_weights(cells, 2)))
    net.save(tmp_path / "net.pt")
    back = NTupleNet.load(tmp_path / "net.pt", "cpu")
    assert back.cells == cells and torch.equal(back.weights, net.weights) and back.weights.dtype == torch.int32


def test_commands_list_their_options():
    from typer.testing import CliRunner
    import train
    for cmd, opts in (("train-ntuple", ("--steps", "--envs", "--lr-shift", "--tuples", "--seed", "--out", "--print-freq")),
                      ("play-ntuple", ("MODEL", "--games", "-g", "--max-moves"))):
        r = CliRunner().invoke(train.app, [cmd, "--help"])
        assert r.exit_code == 0, r.output
        out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
        for opt in opts:
            assert opt in out, (cmd, opt)
