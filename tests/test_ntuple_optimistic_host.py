"""Optimistic initialisation and the resumable n-tuple trainer, without a GPU (Optimistic initialisation of
include/g2048_ntuple.h; NTupleNet(v_init=...), NTupleTrainer.state_dict / from_state_dict, train-ntuple --v-init /
--checkpoint / --resume): the numpy reference of tests/ntuple_optimistic_reference.py against the references it
stands on, the host side of the Python layer on CPU tensors, and the refusals of the new entry points with fake
pointers (a refused call enqueues nothing, so no device is needed)."""

import ctypes
import re

import numpy as np
import pytest
import torch

import ntuple_optimistic_reference as OR
import ntuple_reference as R
import ntuple_stage_reference as SG
from conftest import ROOT

MAP = SG.stage_map_of(SG.STAGES)
LS4 = R.PRESETS["lines-squares-4"]


# ------------------------------------------------------------------------------------ the start -----
def test_w0_of_rounds_to_nearest_and_refuses():
    from g2048.ntuple import w0_of
    assert w0_of(0, 5) == 0 and w0_of(20000, 5) == 2048000 == OR.w0_of(20000, 5)
    assert w0_of(1, 1) == 512 and w0_of(1, 8) == 64
    # 4096 v / (8 T) with a fraction: T = 5 gives 102.4 per point, T = 3 gives 170.67, T = 7 gives 73.14
    assert [w0_of(v, 5) for v in (1, 2, 3, 4, 5)] == [102, 205, 307, 410, 512]
    assert w0_of(1, 3) == 171 and w0_of(1, 7) == 73 and w0_of(3, 7) == 219
    for v in (0, 1, 7, 1000, 65535, 320000):
        for T in range(1, 9):
            w0 = w0_of(v, T)
            assert w0 == OR.w0_of(v, T) and abs(8 * T * w0 - 4096 * v) <= 4 * T  # V(b) within half a weight step
    assert w0_of(2 ** 21, 1) == 2 ** 30  # the largest start
    for bad in ((-1, 5), (2 ** 21 + 1, 1), (2 ** 24 + 1, 8), (1, 0), (1, 9)):
        with pytest.raises(ValueError):
            w0_of(*bad)


@pytest.mark.parametrize("name,smap", [("lines-squares-4", 0), ("lines-squares-4", MAP), ("t8k3", MAP), ("diag", 0)])
def test_a_filled_net_is_worth_8_T_w0_everywhere(name, smap):
    """"diag" is one tuple on the main diagonal: the transposition maps it onto itself, so every board reads some
    weight twice, and the multiplicities must still add up to 8 T."""
    cells = [[0, 5, 10, 15]] if name == "diag" else R.NETS[name]
    T, G = len(cells), SG.num_stages(smap)
    boards = np.concatenate([R.value_boards(), np.zeros((1, 16), np.int8)])
    if name == "diag":
        idx = R.indices(cells, boards)  # [8, T, n]
        assert any(len(set(idx[:, 0, i].tolist())) < 8 for i in range(len(boards)))
    for w0 in (1, -1, -2 ** 31, 2048000):
        w = np.full((G, T, 16 ** len(cells[0])) if smap else (T, 16 ** len(cells[0])), w0, np.int32)
        v = SG.value(cells, w, boards, smap)
        assert v.dtype == np.int64 and (v == 8 * T * w0).all()
        q, legal, best, _ = SG.choose(cells, w, boards, smap)
        ok = q != SG.I64_MIN
        assert ((q - 8 * T * w0)[ok] % SG.S == 0).all()  # what is left of q is the points alone


# ------------------------------------------------------------------------------------ promotion -----
def test_promote_from_reference():
    rng = np.random.default_rng(5)
    w = SG.random_staged_weights(R.NETS["t8k3"], MAP, 5)
    # base 0 is SG.promote
    a, b = w.copy(), w.copy()
    OR.promote_from(a, MAP, 1, 3, 0)
    SG.promote(b, MAP, 1, 3)
    assert np.array_equal(a, b) and not np.array_equal(a, w)
    # onto a stage that still holds base everywhere: a copy, the others untouched
    base = 2048000
    a = w.copy()
    a[2] = base
    OR.promote_from(a, MAP, 1, 2, base)
    assert np.array_equal(a[2], w[1]) and np.array_equal(a[[0, 1, 3]], w[[0, 1, 3]])
    # onto a stage that learned d over base: base + d + (W[from] - base)
    d = rng.integers(-1000, 1000, size=w[2].shape)
    a = w.copy()
    a[1] = base + rng.integers(-5000, 5000, size=w[1].shape)
    a[2] = base + d
    src = a[1].copy()
    OR.promote_from(a, MAP, 1, 2, base)
    assert np.array_equal(a[2], base + d + (src - base))
    # wrap-around at int32, both ways, and a base at the ends of the range
    a = np.zeros((4, 8, 4096), np.int32)
    a[0, 0, :4] = 2 ** 31 - 1, -2 ** 31, 5, -5
    a[1, 0, :4] = 1, -1, 2 ** 31 - 1, -2 ** 31
    OR.promote_from(a, MAP, 0, 1, -1)          # to += from + 1
    assert a[1, 0, :4].tolist() == [-2 ** 31 + 1, -2 ** 31, -2 ** 31 + 5, 2 ** 31 - 4] and a[1, 1, 0] == 1
    c = a.copy()
    OR.promote_from(c, MAP, 1, 2, -2 ** 31)    # to += from + 2^31: the sign bit flips
    assert c[2, 0, :2].tolist() == [1, 0] and c[2, 1, 0] == -2 ** 31 + 1
    wide = w[1].astype(np.int64) + w[3].astype(np.int64) - 12345
    a = w.copy()
    OR.promote_from(a, MAP, 1, 3, 12345)
    assert ((wide >= 2 ** 31) | (wide < -2 ** 31)).sum() > 1000
    assert np.array_equal(a[3].astype(np.int64) % 2 ** 32, wide % 2 ** 32)


def _net(smap, ptr=0x1000, T=5, K=4, cells=None):
    from g2048 import _lib
    flat = [c for t in LS4 for c in t] if cells is None else cells
    return _lib.NtStagedNet(_lib.NtNet(T, K, (ctypes.c_int32 * 48)(*flat), ptr), smap)


def test_header_and_exports():
    from g2048 import _lib
    raw = (ROOT / "include" / "g2048_ntuple.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_fill", "g2048_ntuple_staged_fill", "g2048_ntuple_promote_from"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert "Optimistic initialisation" in raw and "8 T w0" in raw
    assert lib.g2048_ntuple_fill.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.NtNet), ctypes.c_int32]
    assert lib.g2048_ntuple_staged_fill.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.NtStagedNet), ctypes.c_int32]
    assert lib.g2048_ntuple_promote_from.argtypes == lib.g2048_ntuple_promote.argtypes + [ctypes.c_int32]
    assert callable(_lib.ntuple_fill) and callable(_lib.ntuple_promote_from)


def test_library_refusals():
    """Host-only, with fake pointers: fill refuses exactly the nets the weight counts refuse, promote_from what
    g2048_ntuple_promote refuses; nothing is enqueued by a refused call."""
    from g2048 import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    bad_nets = [_net(MAP, ptr=0), _net(MAP, ptr=0x1008), _net(0x3333333331100000), _net(MAP | 1), _net(MAP, T=0),
                _net(MAP, T=9), _net(MAP, K=0), _net(MAP, K=7), _net(MAP, cells=[0, 1, 2, 16] + [0, 1, 2, 3] * 4),
                _net(MAP, cells=[0, 1, 1, 3] + [0, 1, 2, 3] * 4), _net(0, ptr=0), _net(0, ptr=0x1004)]
    for i, net in enumerate(bad_nets):
        assert lib.g2048_ntuple_staged_weight_count(ctypes.byref(net)) == 0, i
        assert lib.g2048_ntuple_staged_fill(None, ctypes.byref(net), 7) == E, i
        assert lib.g2048_ntuple_promote_from(None, ctypes.byref(net), 0, 1, 7) == E, i
        if net.stage_map in (0, MAP):  # the one-stage struct has no map to be wrong
            assert lib.g2048_ntuple_weight_count(ctypes.byref(net.net)) == 0, i
            assert lib.g2048_ntuple_fill(None, ctypes.byref(net.net), 7) == E, i
    assert lib.g2048_ntuple_fill(None, None, 7) == E and lib.g2048_ntuple_staged_fill(None, None, 7) == E
    assert lib.g2048_ntuple_promote_from(None, None, 0, 1, 7) == E
    good = _net(MAP)
    assert lib.g2048_ntuple_staged_weight_count(ctypes.byref(good)) == 4 * 5 * 65536
    for src, dst in ((0, 0), (4, 0), (0, 4), (-1, 2), (2, -1)):
        assert lib.g2048_ntuple_promote_from(None, ctypes.byref(good), src, dst, 7) == E, (src, dst)
        assert lib.g2048_ntuple_promote(None, ctypes.byref(good), src, dst) == E, (src, dst)
    assert lib.g2048_ntuple_promote_from(None, ctypes.byref(_net(0)), 0, 1, 7) == E  # one stage: nothing to promote
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_fill(good, 2 ** 31)
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_promote_from(good, 0, 1, -2 ** 31 - 1)


# -------------------------------------------------------------------------------------- the net -----
def test_net_v_init_on_cpu_and_its_checkpoint(tmp_path):
    from g2048.ntuple import NTupleNet
    net = NTupleNet("lines-squares-4", "cpu", stages=SG.STAGES, v_init=20000)
    assert net.w0 == 2048000 and tuple(net.weights.shape) == (4, 5, 65536) and net.weights.dtype == torch.int32
    assert bool((net.weights == 2048000).all())
    zero = NTupleNet("lines-squares-4", "cpu")
    assert zero.w0 == 0 and not zero.weights.any()
    given = torch.arange(5 * 65536, dtype=torch.int32).reshape(5, 65536)
    rec = NTupleNet("lines-squares-4", "cpu", given, v_init=100)  # explicit weights: w0 is only recorded
    assert rec.w0 == OR.w0_of(100, 5) and torch.equal(rec.weights, given)
    with pytest.raises(ValueError):
        NTupleNet("lines-squares-4", "cpu", v_init=-1)
    with pytest.raises(ValueError):
        NTupleNet([[0]], "cpu", v_init=2 ** 21 + 1)
    # with "w0"
    net.weights[1, 2, 3] = -7
    net.save(tmp_path / "opt.pt")
    ck = torch.load(tmp_path / "opt.pt", map_location="cpu", weights_only=True)
    assert sorted(ck) == ["cells", "stages", "w0", "weights"] and ck["w0"] == 2048000
    back = NTupleNet.load(tmp_path / "opt.pt", "cpu")
    assert back.w0 == 2048000 and back.stages == SG.STAGES and back.cells == net.cells
    assert torch.equal(back.weights, net.weights)
    # without: a zero-start checkpoint is what it was, and loads with w0 = 0
    zero.save(tmp_path / "zero.pt")
    assert sorted(torch.load(tmp_path / "zero.pt", map_location="cpu", weights_only=True)) == ["cells", "weights"]
    assert NTupleNet.load(tmp_path / "zero.pt", "cpu").w0 == 0
    staged = NTupleNet("lines-squares-4", "cpu", stages=SG.STAGES)
    staged.save(tmp_path / "staged.pt")
    assert sorted(torch.load(tmp_path / "staged.pt", map_location="cpu", weights_only=True)) == ["cells", "stages", "weights"]
    ck["w0"] = -3
    torch.save(ck, tmp_path / "bad.pt")
    with pytest.raises(ValueError):
        NTupleNet.load(tmp_path / "bad.pt", "cpu")


# ---------------------------------------------------------------------------------- the trainer -----
CONFIG = dict(envs=6, lr_shift=7, seed=99, rule="tc", trace_len=2, lambda_shift=3, promote_every=40, carousel=True)
CARRIED = ("boards", "after", "pending", "run_score", "tc", "hist", "hist_len", "pool", "valid", "next_stage", "origin")


def _small_net(v_init=64, stages=(16, 64)):
    from g2048.ntuple import NTupleNet
    return NTupleNet([[0, 1], [4, 5]], "cpu", stages=stages, v_init=v_init)  # G = 3, T = 2, 256 weights a table


def _started(cfg=CONFIG, seed=0, **net_kw):
    """A trainer with a hand-built started state: every carried tensor of its configuration drawn at random in
    its dtype, counter 57, promoted_upto 1.  No library call is made."""
    from g2048.ntuple import NTupleTrainer
    net = _small_net(**net_kw)
    tr = NTupleTrainer(net, **cfg)
    g = torch.Generator().manual_seed(seed)
    dims = (tr.envs, tr.trace_len, net.num_stages, tuple(net.weights.shape))
    net.weights.copy_(torch.randint(-2 ** 31, 2 ** 31, net.weights.shape, generator=g, dtype=torch.int64).to(torch.int32))
    for k in tr._carried_names(tr.rule):
        dtype, shape = NTupleTrainer._CARRIED[k]
        info = torch.iinfo(dtype)
        lo, hi = (info.min, info.max) if dtype != torch.int64 else (-2 ** 62, 2 ** 62)
        setattr(tr, k, torch.randint(lo, hi, shape(*dims), generator=g, dtype=torch.int64).to(dtype))
    tr.counter, tr.promoted_upto = 57, 1 if net.num_stages > 1 else 0
    return tr


def _same_run(a, b, rule_changed=False):
    assert a.net.cells == b.net.cells and a.net.stages == b.net.stages and a.net.w0 == b.net.w0
    assert torch.equal(a.net.weights, b.net.weights) and a.net.weights.dtype == b.net.weights.dtype
    for k in ("envs", "seed", "trace_len", "lambda_shift", "promote_every", "carousel", "counter", "promoted_upto"):
        assert getattr(a, k) == getattr(b, k) and type(getattr(a, k)) is type(getattr(b, k)), k
    for k in CARRIED:
        if k == "tc" and rule_changed:
            continue
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k


def test_state_dict_of_a_trainer_not_started(tmp_path):
    from g2048.ntuple import TRAINER_FORMAT, NTupleTrainer
    tr = NTupleTrainer(_small_net(), **CONFIG)
    sd = tr.state_dict()
    assert sd["format"] == TRAINER_FORMAT and sd["counter"] == 0 and sd["promoted_upto"] == 0
    assert not any(k in sd for k in CARRIED) and "stats" not in sd and "workspace" not in sd
    assert all(sd[k] == v for k, v in CONFIG.items()) and sd["w0"] == tr.net.w0 == OR.w0_of(64, 2)
    assert sd["cells"] == [[0, 1], [4, 5]] and sd["stages"] == [16, 64]
    back = NTupleTrainer.from_state_dict(sd, "cpu")
    _same_run(tr, back)
    assert back.boards is None and back.tc is None and back.rule == "tc" and back.lr_shift == 7
    tr.save(tmp_path / "new.pt")
    _same_run(tr, NTupleTrainer.load(tmp_path / "new.pt", "cpu"))
    # the overrides of a run that has not started are plain configuration
    td = NTupleTrainer.load(tmp_path / "new.pt", "cpu", rule="td", lr_shift=12)
    assert td.rule == "td" and td.lr_shift == 12 and td.tc is None and td.boards is None


@pytest.mark.parametrize("cfg", [CONFIG, dict(envs=5, rule="td"), dict(envs=3, rule="tc", trace_len=0),
                                 dict(envs=4, rule="td", trace_len=4, promote_every=3)],
                         ids=["everything", "plain-td", "tc", "td-trace"])
def test_state_dict_round_trip_of_a_started_trainer(tmp_path, cfg):
    from g2048.ntuple import NTupleTrainer
    tr = _started(cfg)
    sd = tr.state_dict()
    want = set(tr._carried_names(tr.rule))
    assert {k for k in CARRIED if k in sd} == want and "stats" not in sd and "workspace" not in sd
    assert all(isinstance(sd[k], torch.Tensor) and sd[k].device.type == "cpu" for k in want | {"weights"})
    assert sd["weights"].data_ptr() != tr.net.weights.data_ptr()  # copies: a later step does not reach the dict
    _same_run(tr, NTupleTrainer.from_state_dict(sd, "cpu"))
    tr.save(tmp_path / "run.pt")
    loaded = torch.load(tmp_path / "run.pt", map_location="cpu", weights_only=True)  # tensors, ints, strings, lists
    assert sorted(loaded) == sorted(sd)
    back = NTupleTrainer.load(tmp_path / "run.pt", "cpu")
    _same_run(tr, back)
    assert back.rule == tr.rule and back.lr_shift == tr.lr_shift and back.workspace is None and back.stats is None


def test_a_one_stage_run_round_trips():
    from g2048.ntuple import NTupleTrainer
    tr = _started(dict(envs=5, rule="tc"), stages=(), v_init=0)
    assert tuple(tr.net.weights.shape) == (2, 256) and tuple(tr.tc.shape) == (2, 256, 2)
    _same_run(tr, NTupleTrainer.from_state_dict(tr.state_dict(), "cpu"))


def test_rule_and_lr_shift_overrides():
    from g2048.ntuple import NTupleTrainer
    td = _started(dict(envs=5, rule="td", trace_len=2))
    sd = td.state_dict()
    assert "tc" not in sd
    tc = NTupleTrainer.from_state_dict(sd, "cpu", rule="tc")       # td -> tc: never-updated accumulators
    _same_run(td, tc, rule_changed=True)
    assert tc.rule == "tc" and tuple(tc.tc.shape) == (3, 2, 256, 2) and tc.tc.dtype == torch.int64 and not tc.tc.any()
    assert tc.lr_shift == td.lr_shift
    full = _started(CONFIG)
    sd = full.state_dict()
    assert "tc" in sd
    back = NTupleTrainer.from_state_dict(sd, "cpu", rule="td", lr_shift=3)  # tc -> td drops them
    _same_run(full, back, rule_changed=True)
    assert back.rule == "td" and back.tc is None and back.lr_shift == 3
    same = NTupleTrainer.from_state_dict(sd, "cpu", rule="tc", lr_shift=30)
    assert torch.equal(same.tc, full.tc) and same.lr_shift == 30
    for bad in (dict(rule="sarsa"), dict(lr_shift=0), dict(lr_shift=31)):
        with pytest.raises(ValueError):
            NTupleTrainer.from_state_dict(sd, "cpu", **bad)


def test_every_refusal_of_a_checkpoint():
    from g2048.ntuple import NTupleTrainer
    sd = _started(CONFIG).state_dict()

    def refused(**change):
        bad = dict(sd)
        for k, v in change.items():
            if v is None:
                del bad[k]
            else:
                bad[k] = v
        with pytest.raises(ValueError):
            NTupleTrainer.from_state_dict(bad, "cpu")

    NTupleTrainer.from_state_dict(dict(sd), "cpu")  # the unchanged dict is accepted
    # the tag
    refused(format="g2048-ntuple-trainer-0")
    refused(format=None)
    with pytest.raises(ValueError):
        NTupleTrainer.from_state_dict({"cells": sd["cells"], "weights": sd["weights"]}, "cpu")  # a net's checkpoint
    # shapes: every carried tensor one env short, and the weights against cells and stages
    n = CONFIG["envs"]
    for k in CARRIED:
        t = sd[k]
        axis = list(t.shape).index(n) if k != "tc" else 1
        refused(**{k: t.narrow(axis, 0, t.shape[axis] - 1).contiguous()})
        refused(**{k: None})                                     # and each one missing
    refused(weights=sd["weights"][:2].contiguous())
    refused(stages=[16])
    refused(hist=sd["hist"][:1].contiguous())                    # a trace shorter than trace_len
    refused(pool=sd["pool"][:2].contiguous())                    # a pool of fewer stages
    # dtypes
    for k in CARRIED:
        refused(**{k: sd[k].to(torch.float32)})
    refused(boards=sd["boards"].to(torch.uint8), pending=sd["pending"].to(torch.int8))
    refused(weights=sd["weights"].to(torch.int64))
    refused(boards=sd["boards"].tolist())
    # the configuration
    refused(envs=0)
    refused(rule="sarsa")
    refused(trace_len=5)
    refused(lambda_shift=0)
    refused(promote_every=-1)
    refused(carousel=1)
    refused(envs="6")
    refused(seed=None)
    refused(w0=-1)
    refused(w0=2 ** 30 + 1)
    refused(counter=-1)
    refused(promoted_upto=3)
    refused(counter=0)                                           # not started, yet it carries tensors
    # what a run of this configuration does not carry
    refused(stats=torch.zeros(8, dtype=torch.int64))
    td = _started(dict(envs=5, rule="td")).state_dict()
    for k in ("tc", "hist", "hist_len", "pool", "valid", "next_stage", "origin"):
        with pytest.raises(ValueError):
            NTupleTrainer.from_state_dict(dict(td, **{k: sd[k]}), "cpu")
    # a forbidden override: only rule and lr_shift may differ from the saved run
    for extra in (dict(envs=6), dict(seed=1), dict(trace_len=2), dict(carousel=True), dict(promote_every=40)):
        with pytest.raises(ValueError):
            NTupleTrainer.from_state_dict(dict(sd), "cpu", **extra)


def test_loading_makes_no_library_call(monkeypatch):
    from g2048 import _lib
    from g2048.ntuple import NTupleTrainer
    sd = _started(CONFIG).state_dict()

    def no(*a, **kw):
        raise AssertionError("a library call while loading a checkpoint")

    monkeypatch.setattr(_lib, "load", no)
    monkeypatch.setattr(_lib, "_call", no)
    tr = NTupleTrainer.from_state_dict(sd, "cpu", rule="td")
    assert tr.counter == 57 and tr.net._c is None


# ---------------------------------------------------------------------------------- the command -----
def test_command_options_and_resume_checks(tmp_path):
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["train-ntuple", "--help"])
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    assert r.exit_code == 0, out
    for opt in ("--v-init", "--checkpoint", "--resume"):
        assert opt in out, opt
    flat = re.sub(r"[\s│]+", " ", out)
    assert "5 GB" in flat and "--resume a.pt --rule tc" in flat
    ck = tmp_path / "run.pt"
    _started(CONFIG).save(ck)
    for extra in (["--envs", "64"], ["--v-init", "5"], ["--stages", "16,64"], ["--seed", "1"], ["--trace", "1"],
                  ["--carousel"], ["--tuples", "4x6"], ["--promote-every", "40"], ["--lambda-shift", "2"]):
        r = CliRunner().invoke(train.app, ["train-ntuple", "--resume", str(ck), "--steps", "1"] + extra)
        assert r.exit_code == 1 and "--resume" in r.output and extra[0] in r.output, (extra, r.output)
    r = CliRunner().invoke(train.app, ["train-ntuple", "--resume", str(tmp_path / "none.pt"), "--steps", "1"])
    assert r.exit_code == 1 and "no such file" in r.output
    r = CliRunner().invoke(train.app, ["train-ntuple", "--v-init", "-5", "--steps", "1"])  # refused before any device
    assert r.exit_code == 1 and "--v-init" in r.output
    r = CliRunner().invoke(train.app, ["train-ntuple", "--v-init", "99999999", "--steps", "1"])
    assert r.exit_code == 1 and "--v-init" in r.output
    text = (ROOT / "README.md").read_text() + (ROOT / "INTEGRATION.md").read_text()
    assert "--v-init" in text and "--checkpoint" in text and "--resume" in text
