"""Optimistic initialisation and exact resume of the n-tuple trainer on the GPU (Optimistic initialisation of
include/g2048_ntuple.h: nt_fill_kernel and nt_promote_from_kernel of csrc/ntuple.hip; NTupleNet(v_init=...),
NTupleTrainer.save / load, train-ntuple --v-init / --checkpoint / --resume), bit for bit against the numpy
reference of tests/ntuple_optimistic_reference.py.  Nothing here has a tolerance: fill and promotion are integer
stores, the learners are those of the other n-tuple tests started from other weights, and a resumed run is
compared with the uninterrupted run of the same device as well as with the reference.

The trainer cases run lines-squares-4 with the stages (16, 64, 128) and 64 envs.  Before a device result is
compared, the reference run of a case must show what the case is there for: that every promotion landed on a
stage that had already learned (so the subtraction of w0 counts), or that the resumed segment promotes and
restarts games from snapshots taken before the checkpoint."""

import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_lambda_reference as LR
import ntuple_optimistic_reference as OR
import ntuple_reference as R
import ntuple_stage_reference as SG
from conftest import PKG
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MAP = SG.stage_map_of(SG.STAGES)
LS4 = R.PRESETS["lines-squares-4"]
K6 = [[0, 1, 2, 3, 4, 5]]  # one table of 16^6 weights, 2^22 16-byte words a stage: 16 384 workgroups of the fill, and
#                            eight passes of the promotion's grid-stride loop over its 2 048
SENTINEL = 0x5EA7BEEF
NETS = {"t1k1": (R.NETS["t1k1"], ()), "ls4": (LS4, ()), "ls4-staged": (LS4, SG.STAGES), "k6-two-stages": (K6, (2048,))}
W0S = (1, -1, -2 ** 31, 0xA5C3E)  # the last: 20 bits
V_INIT, W0 = 20000, 2048000
CARRIED = ("boards", "after", "pending", "run_score", "tc", "hist", "hist_len", "pool", "valid", "next_stage", "origin")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def guarded(shape, dev, fill=None):
    """-> (buf, view): an int32 buffer with four sentinel words on either side of `view`, the weights of `shape`
    (16-byte aligned: the allocation is, and 16 bytes are skipped)."""
    count = int(np.prod(shape))
    buf = torch.full((count + 8,), SENTINEL, dtype=torch.int32, device=dev)
    view = buf[4:4 + count].view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    if fill is not None:
        view.copy_(fill)
    return buf, view


def sentinels_intact(buf):
    return bool((buf[:4] == SENTINEL).all()) and bool((buf[-4:] == SENTINEL).all())


@pytest.fixture(scope="module")
def boards():
    """R.value_boards(), the empty board and 200 random boards; the last 40 are spread so thin that many have no
    two equal neighbours: no move of theirs merges, and all their legal moves tie."""
    rng = np.random.default_rng(17)
    rnd = rng.integers(0, 13, size=(200, 16)).astype(np.int8)
    rnd[rng.random(rnd.shape) < 0.4] = 0
    rnd[160:][rng.random((40, 16)) < 0.7] = 0
    b = np.ascontiguousarray(np.concatenate([R.value_boards(), np.zeros((1, 16), np.int8), rnd]))
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def choice_of_a_flat_net(boards):
    """-> (pts int64 [n, 4], ok bool [n, 4]): with one value for every board, q[a] = S pts(b, a) + that value."""
    n = len(boards)
    rep = np.repeat(boards, 4, axis=0)
    moved, pts, _ = O.move(rep, np.tile(np.arange(4), n))
    return pts.astype(np.int64).reshape(n, 4), (moved != rep).any(1).reshape(n, 4)


# ----------------------------------------------------------------------------------------- fill -----
@pytest.mark.parametrize("name", sorted(NETS))
def test_fill(dev, name, boards, choice_of_a_flat_net):
    cells, stages = NETS[name]
    smap = SG.stage_map_of(stages)
    T, G = len(cells), len(stages) + 1
    shape = ((G,) if stages else ()) + (T, 16 ** len(cells[0]))
    buf, view = guarded(shape, dev)
    net = L().make_ntuple_net(cells, view, smap)
    assert isinstance(net, L().NtStagedNet) == bool(stages)
    pts, ok = choice_of_a_flat_net
    n = len(boards)
    b = to_dev(boards, dev)
    value = torch.empty(n, dtype=torch.int64, device=dev)
    q = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    flat = ok.any(1) & (np.where(ok, pts, 0).max(1) == 0)  # boards whose legal moves merge nothing
    assert flat.sum() >= 20 and (ok.sum(1)[flat] >= 2).sum() >= 20
    lowest = np.where(ok.any(1), ok.argmax(1), 0xFF).astype(np.uint8)
    for w0 in W0S:
        L().ntuple_fill(net, w0, dev)
        L().ntuple_value(net, b, value)
        L().ntuple_choose(net, b, q, legal, best)
        torch.cuda.synchronize()
        assert bool((view == w0).all()), w0
        assert sentinels_intact(buf), w0
        assert (value.cpu().numpy() == 8 * T * w0).all(), w0
        want_q = np.where(ok, SG.S * pts + 8 * T * w0, SG.I64_MIN)
        want_best = np.where(ok.any(1), want_q.argmax(1), 0xFF).astype(np.uint8)
        got_best = best.cpu().numpy()
        assert np.array_equal(q.cpu().numpy(), want_q) and np.array_equal(got_best, want_best), w0
        assert np.array_equal(legal.cpu().numpy(), O.legal_mask(boards))
        assert np.array_equal(got_best[flat], lowest[flat]), w0  # every legal move ties: the lowest index wins


def test_fill_through_the_staged_entry_with_the_map_zero(dev):
    """A staged struct with stage_map 0 is the one-stage net: g2048_ntuple_staged_fill fills its T 16^K weights."""
    buf, view = guarded((5, 65536), dev)
    net = L().NtStagedNet(L().make_ntuple_net(LS4, view, 0), 0)
    L().ntuple_fill(net, -77, dev)
    torch.cuda.synchronize()
    assert bool((view == -77).all()) and sentinels_intact(buf)


def test_fill_refusals(dev):
    """Null or misaligned weights and an invalid map: G2048_EINVAL, and nothing was written anywhere."""
    import ctypes
    buf, view = guarded((4, 5, 65536), dev)
    flat = (ctypes.c_int32 * 48)(*[c for t in LS4 for c in t])
    ptr = view.data_ptr()
    staged = lambda p, smap: L().NtStagedNet(L().NtNet(5, 4, flat, p), smap)  # noqa: E731
    bad = [staged(None, MAP), staged(ptr + 4, MAP), staged(ptr + 8, MAP), staged(ptr, MAP | 1),
           staged(ptr, 0x3333333331100000), L().NtNet(5, 4, flat, None), L().NtNet(5, 4, flat, ptr + 4),
           L().NtNet(0, 4, flat, ptr), L().NtNet(5, 7, flat, ptr)]
    for i, net in enumerate(bad):
        with pytest.raises(L().G2048Error):
            L().ntuple_fill(net, 123, dev)
    with pytest.raises(L().G2048Error):
        L().ntuple_fill(staged(ptr, MAP), 2 ** 31, dev)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    L().ntuple_fill(staged(ptr, MAP), 123, dev)  # the same struct with nothing wrong is accepted
    torch.cuda.synchronize()
    assert bool((view == 123).all()) and sentinels_intact(buf)


# ------------------------------------------------------------------------------------ promotion -----
@pytest.mark.parametrize("name,moves", [("ls4-staged", ((1, 2), (3, 0), (0, 3))), ("k6-two-stages", ((0, 1),))])
def test_promote_from(dev, name, moves):
    cells, stages = NETS[name]
    smap = SG.stage_map_of(stages)
    G, T, size = len(stages) + 1, len(cells), 16 ** len(cells[0])
    gen = torch.Generator(device=dev).manual_seed(11)
    start = torch.randint(-2 ** 31, 2 ** 31, (G, T, size), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
    w = start.cpu().numpy()
    buf, view = guarded((G, T, size), dev, start)
    net = L().make_ntuple_net(cells, view, smap)
    bases = [int(v) for v in np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, size=len(moves))]
    want = w.copy()
    wrapped = 0
    for (src, dst), base in zip(moves, bases):
        wide = want[dst].astype(np.int64) + want[src].astype(np.int64) - base
        wrapped += int(((wide >= 2 ** 31) | (wide < -2 ** 31)).sum())
        before = want.copy()
        OR.promote_from(want, smap, src, dst, base)
        L().ntuple_promote_from(net, src, dst, base, dev)
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        assert np.array_equal(got, want), (src, dst)
        others = [g for g in range(G) if g != dst]
        assert np.array_equal(got[others], before[others]) and not np.array_equal(got[dst], before[dst])
    assert wrapped > 1000 and sentinels_intact(buf)
    # base 0 is g2048_ntuple_promote byte for byte
    src, dst = moves[0]
    a, b = start.clone(), start.clone()
    L().ntuple_promote_from(L().make_ntuple_net(cells, a, smap), src, dst, 0, dev)
    L().ntuple_promote(L().make_ntuple_net(cells, b, smap), src, dst, dev)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, start)
    # onto a stage that still holds base everywhere: a copy
    a = start.clone()
    a[dst] = W0
    L().ntuple_promote_from(L().make_ntuple_net(cells, a, smap), src, dst, W0, dev)
    torch.cuda.synchronize()
    assert torch.equal(a[dst], start[src]) and torch.equal(a[src], start[src])


def test_promote_from_refusals(dev):
    start = to_dev(SG.random_staged_weights(LS4, MAP, 5), dev)
    buf, view = guarded((4, 5, 65536), dev, start)
    net = L().make_ntuple_net(LS4, view, MAP)
    for src, dst in ((0, 0), (4, 0), (0, 4), (-1, 2), (2, -1)):
        with pytest.raises(L().G2048Error):
            L().ntuple_promote_from(net, src, dst, 5, dev)
    with pytest.raises(L().G2048Error):
        L().ntuple_promote_from(L().make_ntuple_net(LS4, view[0], 0), 0, 1, 5, dev)  # one stage
    with pytest.raises(L().G2048Error):
        L().ntuple_promote_from(L().NtStagedNet(net.net, MAP | 1), 0, 1, 5, dev)     # an invalid map
    with pytest.raises(L().G2048Error):
        L().ntuple_promote_from(net, 0, 1, 2 ** 31, dev)
    torch.cuda.synchronize()
    assert torch.equal(view, start) and sentinels_intact(buf)


# --------------------------------------------------------------------- learners from a filled net -----
@pytest.mark.parametrize("rule,h", [("td", 0), ("tc", 3)])
def test_learners_from_a_filled_net(dev, rule, h):
    """64 envs on the staged net, the weights as g2048_ntuple_staged_fill left them (never uploaded): 24 steps in
    two calls give the weights, accumulators and carried state of SG.td_stage from np.full(w0)."""
    cells, w, start_boards, lr_shift, tc = SG.start(rule, "n64-zero", "zero" if rule == "tc" else None, MAP)
    n = len(start_boards)
    st = LR.LState(cells, np.full(w.shape, W0, np.int32), start_boards, h)
    SG.td_stage(st, tc, 24, lr_shift, 1, LR.SEED, 1, MAP)
    assert st.stats[3] > 0 and (st.weights != W0).sum() > 1000 and (st.weights == W0).sum() > 1000
    wd = torch.empty(w.shape, dtype=torch.int32, device=dev)
    net = L().make_ntuple_net(cells, wd, MAP)
    L().ntuple_fill(net, W0, dev)
    tcd = None if tc is None else torch.zeros(w.shape + (2,), dtype=torch.int64, device=dev)
    b = to_dev(start_boards, dev)
    after = torch.zeros(n, 16, dtype=torch.int8, device=dev)
    hist = torch.zeros(h, n, 16, dtype=torch.int8, device=dev) if h else None
    hist_len = torch.zeros(n, dtype=torch.uint8, device=dev) if h else None
    pending = torch.zeros(n, dtype=torch.uint8, device=dev)
    run_score = torch.zeros(n, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = torch.full((L().ntuple_lambda_workspace_bytes(n),), 0x5A, dtype=torch.uint8, device=dev)
    for counter, steps in ((1, 11), (12, 13)):
        rng = L().make_rng(L().RNG_PHILOX, LR.SEED, counter)
        if h:
            L().ntuple_lambda(net, tcd, b, after, hist, hist_len, pending, run_score, steps, lr_shift, h, 1, rng, stats, ws)
        else:
            L().ntuple_td(net, b, after, pending, run_score, steps, lr_shift, rng, stats, ws)
    torch.cuda.synchronize()
    got = {"weights": wd, "boards": b, "after": after, "pending": pending, "run_score": run_score, "stats": stats}
    want = {k: getattr(st, k) for k in got}
    if tc is not None:
        got["tc"], want["tc"] = tcd, tc
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    if h:
        assert np.array_equal(hist_len.cpu().numpy(), st.hist_len)
        assert np.array_equal(LR.valid_hist(hist.cpu().numpy(), st.hist_len), LR.valid_hist(st.hist, st.hist_len))


# ------------------------------------------------------------------------ the trainer with optimism -----
def trainer_state(tr):
    """What a checkpoint carries of a device trainer, as numpy, under the names of OR.TrainerRef.state()."""
    torch.cuda.synchronize()
    out = {"counter": tr.counter, "promoted_upto": tr.promoted_upto, "weights": tr.net.weights.cpu().numpy()}
    for k in CARRIED:
        if getattr(tr, k) is not None:
            out[k] = getattr(tr, k).cpu().numpy()
    return out


def assert_is_reference(got, ref):
    want = ref.state()
    got = dict(got)
    if "hist" in got:
        got["hist"] = LR.valid_hist(got["hist"], got["hist_len"])
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        if isinstance(v, int):
            assert got[k] == v, k
        else:
            assert got[k].dtype == v.dtype and np.array_equal(got[k].reshape(v.shape), v), k


@pytest.mark.parametrize("rule,h", [("td", 0), ("tc", 3)])
def test_trainer_with_optimism(dev, rule, h):
    """v_init 20 000 on lines-squares-4 (w0 2 048 000), promote_every 40, 100 steps: the reference promotes the
    stages 1, 2 and 3, each onto a stage that already differs from w0, so a promotion that forgot the base, or
    that only copied, leaves other weights."""
    from g2048.ntuple import NTupleNet, NTupleTrainer
    ref = OR.TrainerRef(LS4, SG.STAGES, envs=64, w0=OR.w0_of(V_INIT, 5), rule=rule, h=h, lr_shift=10, promote_every=40)
    want = ref.train(100)
    assert ref.w0 == W0 and ref.promoted == [1, 2, 3] and ref.onto_learned == 3
    net = NTupleNet("lines-squares-4", dev, stages=SG.STAGES, v_init=V_INIT)
    assert net.w0 == W0 and bool((net.weights == W0).all())
    tr = NTupleTrainer(net, envs=64, lr_shift=10, rule=rule, trace_len=h, promote_every=40)
    outs = [tr.train(k) for k in (37, 63)]
    assert_is_reference(trainer_state(tr), ref)
    assert sum((o["promoted"] for o in outs), []) == want["promoted"] == [1, 2, 3]
    for key in ("games", "score_sum", "updates"):
        assert sum(o[key] for o in outs) == want[key], key
    assert max(o["max_score"] for o in outs) == want["max_score"]
    doubled = OR.TrainerRef(LS4, SG.STAGES, envs=64, w0=0, rule=rule, h=h, lr_shift=10, promote_every=40)
    doubled.st.weights[...] = W0  # the same start promoted without its base: g2048_ntuple_promote on an optimistic net
    doubled.train(100)
    assert not np.array_equal(doubled.st.weights, ref.st.weights)


# ------------------------------------------------------------------------------------ exact resume -----
RESUME = {
    # name: (stages, v_init, trainer configuration, first segment, second segment, rule on load)
    "tc-trace-carousel": (SG.STAGES, 0, dict(lr_shift=5, rule="tc", trace_len=3, promote_every=40, carousel=True), 50, 250, None),
    "td-one-stage": ((), 0, dict(lr_shift=10, rule="td"), 30, 30, None),
    "td-then-tc": ((), 0, dict(lr_shift=10, rule="td"), 30, 30, "tc"),
    "optimistic-td-then-tc": (SG.STAGES, V_INIT, dict(lr_shift=10, rule="td", promote_every=40), 50, 50, "tc"),
}


@pytest.mark.parametrize("case", sorted(RESUME))
def test_exact_resume(dev, tmp_path, case):
    """Run A: train(first), train(second) on one trainer.  Run B: train(first), save, a new net and trainer from
    load, train(second).  Everything carried, the counter, promoted_upto and the second train()'s result are equal
    between the two, and A's end state is the reference's.  With a rule on load, A is the reference that goes on
    with that rule from the saved weights (zero accumulators for "tc") and B the loaded trainer alone."""
    from g2048.ntuple import NTupleNet, NTupleTrainer
    stages, v_init, cfg, first, second, new_rule = RESUME[case]
    ref = OR.TrainerRef(LS4, stages, envs=64, w0=OR.w0_of(v_init, 5), rule=cfg["rule"], h=cfg.get("trace_len", 0),
                        lr_shift=cfg["lr_shift"], promote_every=cfg.get("promote_every", 0),
                        carousel=cfg.get("carousel", False))
    want1 = ref.train(first)
    if new_rule:
        ref.switch_rule(new_rule)
    want2 = ref.train(second)
    if case == "tc-trace-carousel":
        # the resumed segment starts mid-interval, promotes, and restarts games from snapshots taken before the save
        assert first % 40 != 0 and len(want1["promoted"]) > 0 and want1["recorded"] > 0 and want1["restarts"] == 0
        assert len(want2["promoted"]) > 0 and want2["restarts"] > 0 and want2["restart_games"] > 0
    if case == "optimistic-td-then-tc":
        assert len(want1["promoted"]) > 0 and len(want2["promoted"]) > 0 and ref.onto_learned > 0

    def fresh():
        return NTupleTrainer(NTupleNet("lines-squares-4", dev, stages=stages, v_init=v_init), envs=64, **cfg)

    b = fresh()
    b1 = b.train(first)
    b.save(tmp_path / "run.pt")
    saved = trainer_state(b)
    del b
    loaded = NTupleTrainer.load(tmp_path / "run.pt", dev, rule=new_rule)
    assert loaded.net.weights.is_cuda and loaded.workspace is None and loaded.net.w0 == OR.w0_of(v_init, 5)
    at_load = trainer_state(loaded)
    if new_rule == "tc":
        assert not at_load.pop("tc").any()
    assert sorted(at_load) == sorted(saved) and all(np.array_equal(at_load[k], saved[k]) for k in saved)
    b2 = loaded.train(second)
    got_b = trainer_state(loaded)
    assert b1 == want1 and b2 == want2
    if new_rule is None:
        a = fresh()
        a1, a2 = a.train(first), a.train(second)
        got_a = trainer_state(a)
        assert a1 == b1 and a2 == b2
        assert sorted(got_a) == sorted(got_b)
        for k in got_a:
            assert np.array_equal(got_a[k], got_b[k]), k
        assert_is_reference(got_a, ref)
    assert_is_reference(got_b, ref)
    assert loaded.rule == (new_rule or cfg["rule"])


# --------------------------------------------------------------------------------------- the command -----
def test_commands(dev, tmp_path):
    """`train-ntuple --stages 16,64,128 --v-init 20000 --envs 64 --steps 60 --checkpoint run.pt --out a.pt`, then
    `--resume run.pt --steps 40 --out b.pt`: b.pt is the net of the uninterrupted 100 steps (the reference's), and
    the resumed log goes on after step 60."""
    ref = OR.TrainerRef(LS4, SG.STAGES, envs=64, w0=W0)
    ref.train(60)
    at60 = ref.st.weights.copy()
    ref.train(40)
    assert not np.array_equal(at60, ref.st.weights)
    base = [sys.executable, str(PKG / "train.py"), "train-ntuple"]
    run, a, b = tmp_path / "run.pt", tmp_path / "a.pt", tmp_path / "b.pt"
    r = subprocess.run(base + ["--stages", "16,64,128", "--v-init", str(V_INIT), "--envs", "64", "--steps", "60",
                               "--checkpoint", str(run), "--out", str(a)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert any(ln.startswith("n-tuple net lines-squares-4") and f"v_init {V_INIT} (w0 {W0})" in ln
               for ln in r.stdout.splitlines()), r.stdout[-3000:]
    ck = torch.load(a, map_location="cpu", weights_only=True)
    assert sorted(ck) == ["cells", "stages", "w0", "weights"] and ck["w0"] == W0
    assert np.array_equal(ck["weights"].numpy(), at60)
    r = subprocess.run(base + ["--resume", str(run), "--steps", "40", "--print-freq", "25", "--out", str(b)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = [int(s) for s in re.findall(r"^step (\d+):", r.stdout, flags=re.M)]
    assert steps == [85, 100] and min(steps) >= 61, r.stdout[-3000:]
    ck = torch.load(b, map_location="cpu", weights_only=True)
    assert ck["w0"] == W0 and ck["stages"] == list(SG.STAGES)
    assert np.array_equal(ck["weights"].numpy(), ref.st.weights)
