"""CPU-side checks of the multi-stage n-tuple network (Stages of include/g2048_ntuple.h): with the map 0 the
staged numpy reference (tests/ntuple_stage_reference.py) is the one-stage references byte for byte (R.td,
C.td_tc, LR.td_lambda, R.choose, search_ref, one existing case each); the stage of a board by hand, under the
8 symmetries and at exponent 16; the map of a stage list and the validity of a map; promotion; a staged
value against a scalar sum written from the header; and the seams (the staged struct, the two new entry
points and the staged twins of the C ABI, what the library, the wrapper, the net, the trainer and the command refuse)."""

import ctypes
import re

import numpy as np
import pytest
import torch

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_search_reference as SR
import ntuple_stage_reference as SG
import ntuple_tc_reference as C
from conftest import ROOT

MAP3 = SG.stage_map_of(SG.STAGES)
FULL = tuple(1 << m for m in range(1, 16))  # a stage per exponent: G = 16


def _same(a, b, tc_a=None, tc_b=None):
    for k in ("weights", "boards", "after", "pending", "run_score", "stats"):
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    assert (tc_a is None) == (tc_b is None) and (tc_a is None or tc_a.tobytes() == tc_b.tobytes())


def test_map_zero_is_td():
    cells, w, boards, lr = R.td_start("n64-random")
    want = R.td(R.TDState(cells, w, boards), 60, lr, R.TD_SEED, 1)
    got = SG.td_stage(LR.LState(cells, w, boards, 0), None, 60, lr, 1, R.TD_SEED, 1, 0)
    _same(got, want)
    assert (want.weights != w).any()


def test_map_zero_is_tc():
    cells, w, boards, lr, tc = C.tc_start("n64-zero", "prefilled")
    tc2 = tc.copy()
    want = C.td_tc(R.TDState(cells, w, boards), tc, 60, lr, C.TC_SEED, 1)
    got = SG.td_stage(LR.LState(cells, w, boards, 0), tc2, 60, lr, 1, C.TC_SEED, 1, 0)
    _same(got, want, tc2, tc)
    assert (want.weights != w).any()


def test_map_zero_is_lambda():
    cells, w, boards, lr, _ = LR.start("td", "n64-random", None)
    ev_a, ev_b = {}, {}
    want = LR.td_lambda(LR.LState(cells, w, boards, 3), None, 60, lr, 1, LR.SEED, 1, events=ev_a)
    got = SG.td_stage(LR.LState(cells, w, boards, 3), None, 60, lr, 1, LR.SEED, 1, 0, events=ev_b)
    _same(got, want)
    assert got.hist.tobytes() == want.hist.tobytes() and got.hist_len.tobytes() == want.hist_len.tobytes()
    assert all(ev_a[k] == ev_b[k] for k in LR.EVENTS) and ev_a["traced"] > 0
    assert len(ev_b["stage_updates"]) == 1 and ev_b["stage_updates"][0] >= want.stats[3] > 0
    assert ev_b["cross_stage"] == ev_b["terminal_high"] == ev_b["trace_cross"] == 0


def test_map_zero_is_choose_and_search():
    cells = R.NETS["lines-squares-4"]
    w = R.random_weights(cells, 7)
    b = R.value_boards()
    for got, want in zip(SG.choose(cells, w, b, 0), R.choose(cells, w, b)):
        assert got.tobytes() == want.tobytes()
    assert SG.value(cells, w, b).tobytes() == R.value(cells, w, b).tobytes()
    for got, want in zip(SG.search_ref(cells, w, b, 2), SR.search_ref(cells, w, b, 2)):
        assert got.tobytes() == want.tobytes()


def test_stage_map_of():
    assert SG.stage_map_of(()) == 0
    # 16 = 2^4, 64 = 2^6, 128 = 2^7: stage 0 for exponents 0-3, 1 for 4-5, 2 for 6, 3 from 7 on
    assert SG.nibbles(MAP3) == [0, 0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3]
    assert MAP3 == 0x3333333332110000
    assert SG.nibbles(SG.stage_map_of((2048,))) == [0] * 11 + [1] * 5
    assert SG.nibbles(SG.stage_map_of(FULL)) == list(range(16)) and SG.num_stages(SG.stage_map_of(FULL)) == 16
    assert SG.num_stages(0) == 1 and SG.num_stages(MAP3) == 4
    from g2048.ntuple import stage_map_of
    for st in ((), SG.STAGES, (2048,), (2048, 4096, 8192), FULL, (2,), (32768,)):
        assert stage_map_of(st) == SG.stage_map_of(st)
    for bad in ((16, 16), (64, 16), (3,), (1,), (65536,), (0,)):
        with pytest.raises(ValueError):
            stage_map_of(bad)


def test_map_validity():
    assert SG.valid_map(0) and SG.valid_map(MAP3) and SG.valid_map(SG.stage_map_of(FULL))
    assert SG.valid_map(0x2222222221100000)       # 0, 1, 1, 2, 2, ..: no gap
    assert not SG.valid_map(0x3333333331100000)   # a gap: 1 -> 3
    assert not SG.valid_map(0x1111111101110000)   # a decrease
    assert not SG.valid_map(0x0000000000000001)   # nibble 0 is not 0
    assert not SG.valid_map(0x1111111111111111)


def test_stage_by_hand_symmetries_and_clamp():
    boards = np.zeros((6, 16), np.int8)
    boards[1, 5] = 3
    boards[2, [0, 9]] = 4, 2
    boards[3, 15] = 6
    boards[4, 7] = 7
    boards[5, [2, 3]] = 16, 1
    assert SG.stage(MAP3, boards).tolist() == [0, 0, 1, 2, 3, 3]
    assert SG.stage(0, boards).tolist() == [0] * 6
    full = SG.stage_map_of(FULL)
    assert SG.stage(full, boards).tolist() == [0, 3, 4, 6, 7, 15]    # the empty board: m = 0; 16 clamps to 15
    b15 = boards[5].copy()
    b15[2] = 15
    assert SG.stage(full, b15[None]).tolist() == [15]
    rng = np.random.default_rng(5)
    rand = rng.integers(0, rng.integers(2, 18, size=(50, 1)), size=(50, 16)).astype(np.int8)  # a cap per board
    rand[rng.random(rand.shape) < 0.5] = 0
    for smap in (MAP3, full):
        want = SG.stage(smap, rand)
        assert len(set(want.tolist())) > 2
        for p in R.SYMS:
            assert np.array_equal(SG.stage(smap, rand[:, p]), want)


def test_staged_value_against_a_scalar_sum():
    """V(b) = sum over t and the 8 symmetries of W[stage(b)][t][idx_t(g(b))], in Python ints."""
    cells = R.NETS["t8k3"]
    w = SG.random_staged_weights(cells, MAP3, 3)
    boards = R.value_boards()
    stages = SG.stage(MAP3, boards)
    assert len(set(stages.tolist())) >= 3
    got = SG.value(cells, w, boards, MAP3)
    for i, b in enumerate(boards):
        e = [min(int(x), 15) for x in b]
        v = 0
        for p in R.SYMS:
            for t, tup in enumerate(cells):
                v += int(w[stages[i], t, sum(e[p[c]] << (4 * j) for j, c in enumerate(tup))])
        assert v == got[i]
    assert not np.array_equal(got, R.value(cells, w[0], boards))


def test_promote_wraps():
    w = np.zeros((4, 1, 16), np.int32)
    w[1, 0, :4] = 5, -7, 2 ** 31 - 1, -2 ** 31
    w[2, 0, :4] = 1, 1, 1, -1
    before = w.copy()
    SG.promote(w, MAP3, 1, 3)
    assert np.array_equal(w[3], before[1])                       # onto zeros: a copy
    SG.promote(w, MAP3, 1, 2)
    assert w[2, 0, :4].tolist() == [6, -6, -2 ** 31, 2 ** 31 - 1]  # the int32 sum wraps
    assert np.array_equal(w[:2], before[:2])


def test_trainer_model_cuts_do_not_depend_on_the_chunking():
    cells = [[0, 1], [4, 5]]
    runs = []
    for chunks in ((90,), (7, 40, 43), (30, 30, 30)):
        tr = SG.TrainerRef(cells, SG.STAGES, envs=16, lr_shift=6, promote_every=30)
        for k in chunks:
            tr.train(k)
        runs.append((tr.st.weights.tobytes(), tr.st.boards.tobytes(), tuple(tr.promoted)))
    assert runs[0] == runs[1] == runs[2] and len(runs[0][2]) >= 2
    off = SG.TrainerRef(cells, SG.STAGES, envs=16, lr_shift=6, promote_every=0)
    off.train(90)
    assert off.promoted == [] and off.st.weights.tobytes() != runs[0][0]


# ------------------------------------------------------------------------------------ the seams -----
def test_header_struct_and_exports():
    from g2048 import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048_ntuple.h").read_text(), flags=re.S)
    lib = _lib.load()
    twins = ("weight_count", "value", "choose", "td", "tc", "lambda", "search")
    for name in ("g2048_ntuple_stage", "g2048_ntuple_promote") + tuple("g2048_ntuple_staged_" + t for t in twins):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for t in twins[1:]:  # a twin takes its one-stage call's arguments, the staged struct in the place of the net
        one, two = getattr(lib, "g2048_ntuple_" + t).argtypes, getattr(lib, "g2048_ntuple_staged_" + t).argtypes
        assert one[1] is ctypes.POINTER(_lib.NtNet) and two[1] is ctypes.POINTER(_lib.NtStagedNet)
        assert one[:1] + one[2:] == two[:1] + two[2:], t
    # the one-stage struct is the struct of before; the staged one is that struct and the map behind it
    assert [f for f, _ in _lib.NtNet._fields_] == ["num_tuples", "tuple_len", "cells", "weights"]
    assert ctypes.sizeof(_lib.NtNet) == 208
    assert _lib.NtStagedNet._fields_ == [("net", _lib.NtNet), ("stage_map", ctypes.c_uint64)]
    assert _lib.NtStagedNet.stage_map.offset == 208 and ctypes.sizeof(_lib.NtStagedNet) == 216
    assert _lib.NT_MAX_STAGES == 16
    flat = [c for t in R.PRESETS["lines-squares-4"] for c in t]
    net = _lib.NtNet(5, 4, (ctypes.c_int32 * 48)(*flat), 0x1000)
    assert lib.g2048_ntuple_weight_count(ctypes.byref(net)) == 5 * 16 ** 4
    assert _lib.NtStagedNet(net).stage_map == 0  # zero-initialised: the one-stage net


def _net(smap, ptr=0x1000):
    from g2048 import _lib
    flat = [c for t in R.PRESETS["lines-squares-4"] for c in t]
    return _lib.NtStagedNet(_lib.NtNet(5, 4, (ctypes.c_int32 * 48)(*flat), ptr), smap)


def test_library_refusals():
    """Host-only: the weight count of a staged net, 0 and G2048_EINVAL for what the calls refuse."""
    from g2048 import _lib
    lib = _lib.load()
    count = lambda smap: lib.g2048_ntuple_staged_weight_count(ctypes.byref(_net(smap)))
    assert count(0) == 5 * 16 ** 4 and count(MAP3) == 4 * 5 * 16 ** 4
    assert count(SG.stage_map_of(FULL)) == 16 * 5 * 16 ** 4 and count(SG.stage_map_of((32768,))) == 2 * 5 * 16 ** 4
    for bad in (0x3333333331100000, 0x1111111101110000, 1, 0x1111111111111111, 0x2000000000000000):
        assert not SG.valid_map(bad) and count(bad) == 0
        assert lib.g2048_ntuple_promote(None, ctypes.byref(_net(bad)), 0, 1) == _lib.EINVAL
        assert lib.g2048_ntuple_stage(None, ctypes.byref(_net(bad)), 0x1000, 0x1000, 4) == _lib.EINVAL
    net = _net(MAP3)
    for src, dst in ((0, 0), (2, 2), (-1, 0), (0, -1), (4, 0), (0, 4), (0, 16)):
        assert lib.g2048_ntuple_promote(None, ctypes.byref(net), src, dst) == _lib.EINVAL
    assert lib.g2048_ntuple_promote(None, ctypes.byref(_net(0)), 0, 1) == _lib.EINVAL      # one stage: nothing to promote
    assert lib.g2048_ntuple_promote(None, None, 0, 1) == _lib.EINVAL and lib.g2048_ntuple_staged_weight_count(None) == 0
    assert lib.g2048_ntuple_staged_value(None, None, 0x1000, 0x1000, 4) == _lib.EINVAL
    for bad in (1, 0x3333333331100000):  # the twins refuse an invalid map before anything else
        assert lib.g2048_ntuple_staged_value(None, ctypes.byref(_net(bad)), 0x1000, 0x1000, 4) == _lib.EINVAL
        assert lib.g2048_ntuple_staged_choose(None, ctypes.byref(_net(bad)), 0x1000, 0x1000, None, None, 4) == _lib.EINVAL
    assert lib.g2048_ntuple_staged_value(None, ctypes.byref(net), 0x1000, 0x1000, 0) == 0  # n = 0: a no-op
    assert lib.g2048_ntuple_promote(None, ctypes.byref(_net(MAP3, ptr=0)), 0, 1) == _lib.EINVAL
    stage = lambda b, out, n: lib.g2048_ntuple_stage(None, ctypes.byref(net), b, out, n)
    assert stage(0x1000, None, 4) == _lib.EINVAL and stage(None, 0x1000, 4) == _lib.EINVAL
    assert stage(0x1008, 0x1000, 4) == _lib.EINVAL and stage(0x1000, 0x1000, -1) == _lib.EINVAL
    assert stage(0x1000, 0x1000, 1 << 31) == _lib.EINVAL
    assert stage(None, None, 0) == 0                                                         # n = 0: a no-op


def test_net_trainer_and_wrapper_checks(tmp_path):
    from g2048 import _lib
    from g2048.ntuple import NTupleNet, NTupleTrainer
    net = NTupleNet("lines-squares-4", "cpu", stages=SG.STAGES)
    assert tuple(net.weights.shape) == (4, 5, 65536) and net.stages == SG.STAGES and net.stage_map == MAP3
    plain = NTupleNet("lines-squares-4", "cpu")
    assert tuple(plain.weights.shape) == (5, 65536) and plain.stages == () and plain.stage_map == 0
    with pytest.raises(ValueError):
        NTupleNet("lines-squares-4", "cpu", torch.zeros(5, 65536, dtype=torch.int32), stages=SG.STAGES)
    with pytest.raises(ValueError):
        NTupleNet("lines-squares-4", "cpu", stages=(16, 16))
    with pytest.raises(ValueError):
        NTupleNet("lines-squares-4", "cpu", stages=(24,))
    with pytest.raises(ValueError):
        NTupleTrainer(plain, promote_every=5)
    with pytest.raises(ValueError):
        NTupleTrainer(net, promote_every=-1)
    assert NTupleTrainer(net, promote_every=5).promote_every == 5 and NTupleTrainer(plain).promote_every == 0
    for src, dst in ((0, 0), (0, 4), (-1, 1)):
        with pytest.raises(ValueError):
            net.promote(src, dst)
    with pytest.raises(ValueError):
        plain.promote(0, 1)
    with pytest.raises(_lib.G2048Error):                           # a CPU tensor has no device pointer
        net.stage(torch.zeros(4, 16, dtype=torch.int8))
    # save / load keep the stages; a checkpoint without the key is a one-stage net
    small = NTupleNet([[0, 1]], "cpu", torch.arange(3 * 256, dtype=torch.int32).reshape(3, 1, 256), stages=(8, 512))
    small.save(tmp_path / "a.pt")
    back = NTupleNet.load(tmp_path / "a.pt", "cpu")
    assert back.stages == (8, 512) and torch.equal(back.weights, small.weights) and back.cells == [[0, 1]]
    assert torch.load(tmp_path / "a.pt", weights_only=True)["stages"] == [8, 512]
    NTupleNet([[0, 1]], "cpu").save(tmp_path / "old.pt")        # a one-stage net writes the keys it always wrote
    assert sorted(torch.load(tmp_path / "old.pt", weights_only=True)) == ["cells", "weights"]
    old = NTupleNet.load(tmp_path / "old.pt", "cpu")
    assert old.stages == () and tuple(old.weights.shape) == (1, 256)


def test_command_options_are_declared():
    src = (ROOT / "2048-ppo_amd" / "train.py").read_text()
    assert '"--stages"' in src and '"--promote-every"' in src
