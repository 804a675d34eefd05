"""CPU-side checks of the carousel of the staged n-tuple trainer (Carousel of include/g2048_ntuple.h): the numpy
reference (tests/ntuple_carousel_reference.py) with one stage is SG.td_stage byte for byte; the donors of a step
are a permutation; a run does not depend on how its steps are split into calls; the selection rule on hand-made
valid / next tables; the cases of the GPU tests show what covers() asks of them; and the seams (the struct, the
two entry points, every refusal of the library, the trainer's and the command's argument checks)."""

import ctypes
import re

import numpy as np
import pytest
import torch

import ntuple_carousel_reference as CR
import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_stage_reference as SG
from conftest import ROOT

MAP = SG.stage_map_of(SG.STAGES)


# ------------------------------------------------------------------------------- the reference -----
@pytest.mark.parametrize("rule,name,fill,h", [("td", "n64-random", None, 0), ("tc", "n64-zero", "prefilled", 3)])
def test_one_stage_is_td_stage(rule, name, fill, h):
    """G = 1: nothing is recorded or restarted, and every array td_stage knows is td_stage's."""
    cells, w, boards, lr, tc = SG.start(rule, name, fill, 0)
    tc2 = None if tc is None else tc.copy()
    want = SG.td_stage(LR.LState(cells, w, boards, h), tc, 60, lr, 1, LR.SEED, 1, 0)
    ev = {}
    got = CR.td_carousel(CR.CState(cells, w, boards, h, 1), tc2, 60, lr, 1, LR.SEED, 1, 0, events=ev)
    for k in ("weights", "boards", "after", "hist", "hist_len", "pending", "run_score"):
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
    assert got.stats[:4].tobytes() == want.stats.tobytes() and want.stats[0] > 0 and (got.stats[4:] == 0).all()
    assert (tc is None) or tc.tobytes() == tc2.tobytes()
    assert not got.pool.any() and not got.valid.any() and not got.next.any() and not got.origin.any()
    assert ev["recorded"] == [0] and ev["served"] == [0] and all(ev[k] == 0 for k in CR.EVENTS)
    assert (want.weights != w).any()


def test_donors_are_a_permutation():
    """A permutation of the slots wherever i + c + t does not pass 2^64 among the n envs of the step (and, for an n
    that divides 2^64, there too)."""
    for n in (1, 2, 64, 300):
        for ctr in (0, 1, 63, 64, 299, 300, 12345, 1 << 63, (1 << 64) - 300):
            j = CR.donors(n, ctr)
            assert sorted(j.tolist()) == list(range(n)), (n, ctr)
    for n in (1, 2, 64):
        assert sorted(CR.donors(n, (1 << 64) - 7).tolist()) == list(range(n))
    assert CR.donors(5, 7).tolist() == [2, 3, 4, 0, 1]
    # the sum wraps modulo 2^64 before the modulo n: 2^64 - 1 + 1 = 0, not 2^64
    assert CR.donors(3, (1 << 64) - 1).tolist() == [((1 << 64) - 1) % 3, 0, 1]
    assert CR.donors(300, 300).tolist() == list(range(300))      # a multiple of n: every env is its own donor


def test_selection_by_hand():
    G = 4
    valid = np.zeros((6, 16), np.uint8)
    valid[0, [1, 3]] = 1          # slot 0 holds stages 1 and 3
    valid[1, 2] = 7               # any non-zero byte counts
    valid[2, [0, 5]] = 1          # flags of row 0 and of stages >= G are never looked at
    valid[3, 1] = 1
    valid[5, [1, 2, 3]] = 1
    j = np.array([0, 0, 0, 0, 1, 1, 1, 2, 3, 3, 5, 5, 4])
    nxt = np.array([0, 1, 2, 3, 1, 2, 3, 1, 1, 2, 2, 4, 1], np.uint8)
    k, g = CR.select(valid, nxt, j, G)
    #                    k=0 reset; 1 -> 1; 2 invalid -> 3; 3 -> 3; slot 1: 1 -> 2, 2 -> 2, 3 -> none
    assert g.tolist() == [0, 1, 3, 3, 2, 2, 0, 0, 1, 0, 2, 0, 0]
    assert k.tolist() == [0, 1, 2, 3, 1, 2, 3, 1, 1, 2, 2, 0, 1]   # next >= G reads as 0: the reset
    assert CR.select(valid, np.full(13, 200, np.uint8), j, G)[1].tolist() == [0] * 13
    k16, g16 = CR.select(valid, np.array([5, 6], np.uint8), np.array([2, 2]), 16)
    assert g16.tolist() == [5, 0]                                  # with 16 stages flag 5 is a stage


def test_a_run_does_not_depend_on_the_split():
    runs = []
    for splits in ((90,), (1, 40, 49), (30, 30, 30)):
        st, tc = CR.run("n64-td-trace", splits)
        runs.append(tuple(getattr(st, k).tobytes() for k in CR.ARRAYS if k != "hist") +
                    (LR.valid_hist(st.hist, st.hist_len).tobytes(),))
    assert runs[0] == runs[1] == runs[2]


def test_a_restart_is_accounted_apart():
    """One env, its own donor, on a dead board, whose slot holds a dead board of stage 1: the first game ends at once
    as a full game (of no points); the second starts from the snapshot and ends at once too, as a restarted game;
    the third finds no stage 2 or 3 in the slot and starts from the reset."""
    cells = R.NETS["lines-squares-4"]
    w = np.zeros((4, 5, 65536), np.int32)
    pool, valid = np.zeros((4, 1, 16), np.int8), np.zeros((1, 16), np.uint8)
    pool[1, 0] = CR.stage_board(MAP, 1, None, dead=True)
    valid[0, 1] = 1
    st = CR.CState(cells, w, R.DEAD[None], 0, 4, pool=pool, valid=valid, next=np.array([1], np.uint8))
    ev = {}
    CR.td_carousel(st, None, 1, 12, 1, LR.SEED, 1, MAP, events=ev)
    assert st.stats.tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    assert np.array_equal(st.boards[0], pool[1, 0]) and st.origin[0] == 1 and st.next[0] == 2
    CR.td_carousel(st, None, 1, 12, 1, LR.SEED, 2, MAP, events=ev)
    assert st.stats.tolist() == [1, 0, 0, 0, 1, 0, 0, 1]
    assert st.origin[0] == 0 and st.next[0] == 1 and ev["restart_ended"] == 1 and ev["fell_to_reset"] == 1
    assert st.pending[0] == 0 and SG.stage(MAP, st.boards)[0] == 0 and (st.boards[0] != 0).sum() == 2
    assert ev["served"] == [0, 1, 0, 0] and ev["recorded"] == [0, 0, 0, 0]


@pytest.mark.parametrize("case", sorted(CR.CASES))
def test_cases_cover(case):
    st, tc, ev = CR.ref_case(case)
    CR.covers(case, ev)
    assert st.stats[6] == sum(ev["recorded"]) and st.stats[7] == sum(ev["served"]) and st.stats[4] == ev["restart_ended"]
    assert st.stats[0] > 0 and st.stats[3] > 0


# ------------------------------------------------------------------------------------ the seams -----
def test_header_struct_and_exports():
    from g2048 import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048_ntuple.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_carousel_workspace_bytes", "g2048_ntuple_staged_carousel"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert "Carousel" in (ROOT / "include" / "g2048_ntuple.h").read_text()
    assert [f for f, _ in _lib.NtCarousel._fields_] == ["pool", "valid", "next", "origin"]
    assert all(t is ctypes.c_void_p for _, t in _lib.NtCarousel._fields_) and ctypes.sizeof(_lib.NtCarousel) == 32
    lam, car = lib.g2048_ntuple_staged_lambda.argtypes, lib.g2048_ntuple_staged_carousel.argtypes
    assert len(car) == len(lam) + 1 and car[:15] == lam[:15]         # stream .. rng: the staged-lambda prefix
    assert car[15] is ctypes.POINTER(_lib.NtCarousel) and car[16:] == lam[15:]
    assert lib.g2048_ntuple_carousel_workspace_bytes.argtypes == [ctypes.c_int64]
    assert lib.g2048_ntuple_carousel_workspace_bytes.restype is ctypes.c_size_t


def _net(smap, ptr=0x1000):
    from g2048 import _lib
    flat = [c for t in R.PRESETS["lines-squares-4"] for c in t]
    return _lib.NtStagedNet(_lib.NtNet(5, 4, (ctypes.c_int32 * 48)(*flat), ptr), smap)


def test_library_refusals():
    """Host-only, with fake pointers: nothing is enqueued by a refused call."""
    from g2048 import _lib
    lib = _lib.load()
    wsb = lib.g2048_ntuple_carousel_workspace_bytes
    n = 300
    assert wsb(-1) == 0 and wsb(1 << 28) == 0
    assert wsb(n) >= lib.g2048_ntuple_lambda_workspace_bytes(n) + 17 * n and wsb(n) % 16 == 0 and wsb(0) > 0
    P = 0x10000
    good = dict(net=_net(MAP), tc=None, boards=P, after=P, hist=P, hist_len=P, pending=P, run_score=P, n=n, steps=1,
                lr=10, h=3, s=1, rng=_lib.Rng(_lib.RNG_PHILOX, 0, 1, 1, None, None, None),
                car=_lib.NtCarousel(P, P, P, P), stats=P, ws=P, wsn=wsb(n))

    def call(**kw):
        a = dict(good, **kw)
        return lib.g2048_ntuple_staged_carousel(
            None, None if a["net"] is None else ctypes.byref(a["net"]), a["tc"], a["boards"], a["after"], a["hist"],
            a["hist_len"], a["pending"], a["run_score"], a["n"], a["steps"], a["lr"], a["h"], a["s"],
            None if a["rng"] is None else ctypes.byref(a["rng"]), None if a["car"] is None else ctypes.byref(a["car"]),
            a["stats"], a["ws"], a["wsn"])

    E = _lib.EINVAL
    # the carousel's own refusals
    assert call(car=None) == E
    for member in range(4):
        ptrs = [P] * 4
        ptrs[member] = None
        assert call(car=_lib.NtCarousel(*ptrs)) == E, member
    assert call(car=_lib.NtCarousel(P + 8, P, P, P)) == E and call(car=_lib.NtCarousel(P, P + 8, P, P)) == E
    assert call(wsn=wsb(n) - 1) == E and call(wsn=lib.g2048_ntuple_lambda_workspace_bytes(n)) == E
    # those of g2048_ntuple_staged_lambda
    assert call(net=None) == E and call(net=_net(0x3333333331100000)) == E and call(net=_net(MAP, ptr=0)) == E
    assert call(steps=0) == E and call(lr=0) == E and call(lr=31) == E and call(n=-1) == E and call(n=1 << 28) == E
    assert call(h=-1) == E and call(h=5) == E and call(s=0) == E and call(s=8) == E
    assert call(rng=_lib.Rng(_lib.RNG_MT19937, 0, 1, 1, None, None, None)) == E and call(rng=None) == E
    assert call(tc=P + 8) == E
    for key in ("boards", "after", "pending", "run_score", "ws", "hist", "hist_len"):
        assert call(**{key: None}) == E, key
    for key in ("boards", "after", "ws", "hist"):
        assert call(**{key: P + 8}) == E, key
    # n = 0 is a no-op, whatever car is
    assert call(n=0, car=None, boards=None, ws=None, wsn=0) == 0


def test_trainer_and_command_checks():
    from g2048.ntuple import NTupleNet, NTupleTrainer
    plain = NTupleNet("lines-squares-4", "cpu")
    staged = NTupleNet("lines-squares-4", "cpu", stages=SG.STAGES)
    with pytest.raises(ValueError):
        NTupleTrainer(plain, carousel=True)
    assert NTupleTrainer(staged, carousel=True).carousel is True and NTupleTrainer(staged).carousel is False
    assert NTupleTrainer(plain).carousel is False
    src = (ROOT / "2048-ppo_amd" / "train.py").read_text()
    assert '"--carousel"' in src
    from g2048 import _lib
    z = torch.zeros(4, 16, dtype=torch.int8)
    with pytest.raises(_lib.G2048Error):                           # the pool of 4 envs and 4 stages needs 256 bytes
        _lib.ntuple_carousel(_net(MAP), None, z, z, None, None, z, z, 1, 10, 0, 1, _lib.make_rng(), z, z, z, z, None, z)
