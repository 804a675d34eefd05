"""The multi-stage n-tuple network on the GPU (Stages of include/g2048_ntuple.h: nt_row in every gather and
add of csrc/ntuple.hip and csrc/ntuple_search.hip, nt_stage_kernel, nt_promote_kernel; NTupleNet(stages=...),
NTupleTrainer(promote_every=...), train-ntuple --stages / --promote-every), bit for bit against the numpy
reference of tests/ntuple_stage_reference.py.  Every add is still an integer fixed by reads that see the state
before the step's adds, so what n envs learned in parallel must be the CPU's bytes.

All learner cases use the stage list (16, 64, 128): G = 4, a stage for the largest exponents 0-3, 4-5, 6 and
7+.  The starts are those of R.td_start / C.tc_start with the weights (and prefilled accumulators) drawn for
the staged shape (ntuple_stage_reference.start), 200 steps from counter 1 under game seed 31, the workspace
filled with garbage.  Before a device result is compared, the reference run of the case must show that every
stage received updates, that a target crossed a stage (cross_stage), that a game ended above stage 0
(terminal_high) and, with a trace, that an update reached an after-state of a lower stage (trace_cross):
ntuple_stage_reference.covers.  Every case met that under its own seed and step count; none was changed."""

import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_stage_reference as SG
from conftest import PKG

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
MAP = SG.stage_map_of(SG.STAGES)
FULL = tuple(1 << m for m in range(1, 16))
KEYS = ("weights", "tc", "boards", "after", "hist", "hist_len", "pending", "run_score", "stats")
TRAIN_P, TRAIN_STEPS = 40, 100  # the trainer case: cuts after 40 and 80 of 100 steps


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


def value_boards():
    """R.value_boards() (exponents 15 and 16, finished boards) and the empty board."""
    return np.ascontiguousarray(np.concatenate([R.value_boards(), np.zeros((1, 16), np.int8)]))


# ------------------------------------------------------------------------------------ the stage -----
@pytest.mark.parametrize("stages", [(), SG.STAGES, FULL], ids=["one", "four", "sixteen"])
def test_stage(dev, stages):
    smap = SG.stage_map_of(stages)
    cells = R.NETS["t1k1"]
    w = torch.zeros(len(stages) + 1, 1, 16, dtype=torch.int32, device=dev)
    net = L().make_ntuple_net(cells, w, smap)
    boards = value_boards()
    want = SG.stage(smap, boards)
    assert want.max() == len(stages) and (stages != SG.STAGES or set(want.tolist()) == {0, 1, 2, 3})
    b = to_dev(boards, dev)
    out = torch.full((len(boards) + 3,), 0xEE, dtype=torch.uint8, device=dev)
    L().ntuple_stage(net, b, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:len(boards)], want) and (got[len(boards):] == 0xEE).all()
    assert np.array_equal(b.cpu().numpy(), boards)
    from g2048.ntuple import NTupleNet
    assert np.array_equal(NTupleNet(cells, dev, stages=stages).stage(b).cpu().numpy(), want)


def test_stage_more_than_one_block(dev):
    rng = np.random.default_rng(3)
    boards = rng.integers(0, rng.integers(2, 18, size=(600, 1)), size=(600, 16)).astype(np.int8)
    w = torch.zeros(4, 1, 16, dtype=torch.int32, device=dev)
    out = torch.empty(600, dtype=torch.uint8, device=dev)
    L().ntuple_stage(L().make_ntuple_net([[5]], w, MAP), to_dev(boards, dev), out)
    assert np.array_equal(out.cpu().numpy(), SG.stage(MAP, boards))


# ---------------------------------------------------------------------------- value and choice -----
@pytest.mark.parametrize("name,stages", [("lines-squares-4", SG.STAGES), ("t1k1", SG.STAGES), ("t8k3", SG.STAGES),
                                         ("t2k6", (2048,))])
def test_value_and_choice_bit_exact(dev, name, stages):
    """Staged random 32-bit weights, a seed per stage; t2k6 with two stages is 256 MB of tables.  A kernel that
    ignored the stage would give the values of stage 0's tables: the results must differ from those."""
    smap = SG.stage_map_of(stages)
    cells = R.NETS[name]
    w = SG.random_staged_weights(cells, smap, 7)
    boards = value_boards()
    assert len(set(SG.stage(smap, boards).tolist())) == len(stages) + 1
    wd, b = to_dev(w, dev), to_dev(boards, dev)
    net = L().make_ntuple_net(cells, wd, smap)
    n = len(boards)
    value = torch.empty(n, dtype=torch.int64, device=dev)
    q = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    L().ntuple_value(net, b, value)
    L().ntuple_choose(net, b, q, legal, best)
    torch.cuda.synchronize()
    want_v = SG.value(cells, w, boards, smap)
    want_q, want_legal, want_best, _ = SG.choose(cells, w, boards, smap)
    assert np.array_equal(value.cpu().numpy(), want_v) and np.array_equal(q.cpu().numpy(), want_q)
    assert np.array_equal(legal.cpu().numpy(), want_legal) and np.array_equal(best.cpu().numpy(), want_best)
    assert not np.array_equal(want_v, R.value(cells, w[0], boards))
    assert not np.array_equal(want_q, R.choose(cells, w[0], boards)[0])
    assert np.array_equal(wd.cpu().numpy(), w)


# ----------------------------------------------------------------------------------- the search -----
def test_search_reference_crosses_a_stage():
    """Under (16, 64, 128) some roots of value_boards() have leaves at a higher stage than their own."""
    cells, boards = R.NETS["lines-squares-4"], R.value_boards()
    w = SG.random_staged_weights(cells, MAP, 7)
    crossed = 0
    for i in range(len(boards)):
        st = {}
        SG.search_ref(cells, w, boards[i:i + 1], 2, MAP, stats=st)
        crossed += bool(st["leaves"]) and max(st["leaf_stages"]) > int(SG.stage(MAP, boards[i:i + 1])[0])
    assert crossed > 0


@pytest.mark.parametrize("depth", [2, 3])
def test_search_bit_exact(dev, depth):
    from g2048 import _lib
    cells, boards = R.NETS["lines-squares-4"], R.value_boards()
    w = SG.random_staged_weights(cells, MAP, 7)
    st = {}
    want = SG.search_ref(cells, w, boards, depth, MAP, stats=st)
    assert len(st["leaf_stages"]) == 4
    wd, b = to_dev(w, dev), to_dev(boards, dev)
    net = _lib.make_ntuple_net(cells, wd, MAP)
    n = len(boards)
    for form in (_lib.EMAX_NARROW, _lib.EMAX_WIDE):
        q = torch.empty(n, 4, dtype=torch.int64, device=dev)
        leaves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        legal = torch.empty(n, dtype=torch.uint8, device=dev)
        best = torch.empty(n, dtype=torch.uint8, device=dev)
        ws = torch.full((_lib.ntuple_search_workspace_bytes(n, depth, form),), GARBAGE, dtype=torch.uint8, device=dev)
        _lib.ntuple_search(net, b, depth, q, leaves, legal, best, ws, form)
        torch.cuda.synchronize()
        for got, ref in zip((q, leaves, legal, best), want):
            assert np.array_equal(got.cpu().numpy(), ref), form
    one = SG.search_ref(cells, w[0], boards, depth)
    assert not np.array_equal(one[0], want[0])  # the values of stage 0's tables alone are others


# --------------------------------------------------------------------------------- the learners -----
class Run:
    """The device state of one staged learner run: h = 0 and tc None -> g2048_ntuple_td, h = 0 -> g2048_ntuple_tc,
    otherwise g2048_ntuple_lambda."""

    def __init__(self, dev, cells, weights, boards, tc, h, smap):
        n = len(boards)
        self.n, self.h = n, h
        self.w = to_dev(weights, dev)
        self.net = L().make_ntuple_net(cells, self.w, smap)
        self.tc = None if tc is None else to_dev(tc, dev)
        self.boards = to_dev(boards, dev)
        self.after = torch.zeros(n, 16, dtype=torch.int8, device=dev)
        self.hist = torch.zeros(h, n, 16, dtype=torch.int8, device=dev) if h > 0 else None
        self.hist_len = torch.zeros(n, dtype=torch.uint8, device=dev) if h > 0 else None
        self.pending = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.run_score = torch.zeros(n, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws = torch.empty(L().ntuple_lambda_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def call(self, steps, lr_shift, s, counter, seed=LR.SEED):
        self.ws.fill_(GARBAGE)
        rng = L().make_rng(L().RNG_PHILOX, seed, counter)
        if self.h > 0:
            L().ntuple_lambda(self.net, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                              self.run_score, steps, lr_shift, self.h, s, rng, self.stats, self.ws)
        elif self.tc is not None:
            L().ntuple_tc(self.net, self.tc, self.boards, self.after, self.pending, self.run_score, steps, lr_shift,
                          rng, self.stats, self.ws)
        else:
            L().ntuple_td(self.net, self.boards, self.after, self.pending, self.run_score, steps, lr_shift, rng,
                          self.stats, self.ws)

    def results(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in KEYS[2:] if getattr(self, k) is not None}
        out["weights"] = self.w.cpu().numpy()
        if self.tc is not None:
            out["tc"] = self.tc.cpu().numpy()
        if self.h > 0:
            out["hist"] = LR.valid_hist(out["hist"], out["hist_len"])
        return out


def assert_equal(got, st, tc):
    want = {k: getattr(st, k) for k in KEYS if k not in ("tc", "hist")}
    if tc is not None:
        want["tc"] = tc
    if st.h > 0:
        want["hist"] = LR.valid_hist(st.hist, st.hist_len)
    else:
        del want["hist_len"]
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def device_run(dev, rule, name, fill, h, s, splits, n=None, smap=MAP):
    cells, w, boards, lr_shift, tc = SG.start(rule, name, fill, smap)
    run = Run(dev, cells, w, boards[:n], tc, h, smap)
    counter = 1
    for steps in splits:
        run.call(steps, lr_shift, s, counter)
        counter += steps
    return run.results()


LEARNERS = [("td", "n1-zero", None, 0, 1), ("td", "n64-random", None, 0, 1), ("td", "n300-zero", None, 0, 1),
            ("tc", "n64-zero", "prefilled", 0, 1), ("td", "n64-random", None, 3, 1), ("tc", "n64-zero", "zero", 3, 1)]


@pytest.mark.parametrize("rule,name,fill,h,s", LEARNERS)
def test_learners_bit_exact(dev, rule, name, fill, h, s):
    st, tc, ev = SG.ref_case(rule, name, fill, h, s)
    SG.covers(ev, h)
    got = device_run(dev, rule, name, fill, h, s, [SG.STEPS])
    assert_equal(got, st, tc)
    if name != "n300-zero":  # the same start on stage 0's tables alone (the one-stage net) learns other weights
        cells, w, boards, lr_shift, tc0 = SG.start(rule, name, fill, MAP)
        plain = SG.td_stage(LR.LState(cells, w[0], boards, h), None if tc0 is None else tc0[0].copy(), SG.STEPS,
                            lr_shift, s, LR.SEED, 1, 0)
        assert not np.array_equal(got["weights"][0], plain.weights)


@pytest.mark.parametrize("rule,name,fill,h", [("td", "n64-random", None, 0), ("tc", "n64-zero", "zero", 3)])
def test_continuation(dev, rule, name, fill, h):
    """120 + 80 steps, the counter advanced by 120, equal 200."""
    st, tc, _ = SG.ref_case(rule, name, fill, h, 1)
    one = device_run(dev, rule, name, fill, h, 1, [200])
    two = device_run(dev, rule, name, fill, h, 1, [120, 80])
    assert sorted(one) == sorted(two) and all(one[k].tobytes() == two[k].tobytes() for k in one)
    assert_equal(two, st, tc)


def test_ragged_last_block(dev):
    """n = 257: one lane in the second block; the first 257 envs of n300-zero."""
    ev = {}
    st, tc = SG.run("td", "n300-zero", None, 0, 1, SG.STEPS, MAP, n=257, events=ev)
    SG.covers(ev, 0)
    assert_equal(device_run(dev, "td", "n300-zero", None, 0, 1, [SG.STEPS], n=257), st, tc)


def test_map_zero_is_the_one_stage_call(dev):
    """A staged struct built with stage_map explicitly 0 through g2048_ntuple_staged_td and the one-stage struct
    through g2048_ntuple_td give the same bytes on n64-random, and those are the one-stage reference's."""
    cells, w, boards, lr_shift = R.td_start("n64-random")
    want = R.td(R.TDState(cells, w, boards), R.TD_STEPS, lr_shift, R.TD_SEED, 1)
    outs = []
    for explicit in (True, False):
        run = Run(dev, cells, w, boards, None, 0, 0)
        flat = [c for t in cells for c in t]
        args = (len(cells), len(cells[0]), (ctypes.c_int32 * 48)(*flat), run.w.data_ptr())
        run.net = L().NtStagedNet(L().NtNet(*args), 0) if explicit else L().NtNet(*args)
        run.call(R.TD_STEPS, lr_shift, 1, 1, R.TD_SEED)
        outs.append(run.results())
    for got in outs:
        for k in ("weights", "boards", "after", "pending", "run_score", "stats"):
            assert got[k].tobytes() == np.asarray(getattr(want, k)).tobytes(), k
    assert (want.weights != w).any()


# ------------------------------------------------------------------------------------ promotion -----
def test_promote(dev):
    cells = R.NETS["lines-squares-4"]
    w = SG.random_staged_weights(cells, MAP, 5)
    w[2] = 0
    w[3, 0, :4] = 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31
    w[1, 0, :4] = 1, -1, 2 ** 31 - 1, -2 ** 31          # pairs whose int32 sum overflows, both ways
    wd = to_dev(w, dev)
    tc = torch.full((4, 5, 65536, 2), 3, dtype=torch.int64, device=dev)
    net = L().make_ntuple_net(cells, wd, MAP)
    L().ntuple_promote(net, 1, 2, dev)                   # onto a zero stage: a copy
    torch.cuda.synchronize()
    got = wd.cpu().numpy()
    assert np.array_equal(got[2], w[1]) and np.array_equal(got[[0, 1, 3]], w[[0, 1, 3]])
    L().ntuple_promote(net, 1, 3, dev)                   # onto random weights: the wrapping sum
    L().ntuple_promote(net, 3, 0, dev)                   # downwards too: any two different stages
    torch.cuda.synchronize()
    want = w.copy()
    SG.promote(want, MAP, 1, 2)
    SG.promote(want, MAP, 1, 3)
    SG.promote(want, MAP, 3, 0)
    got = wd.cpu().numpy()
    assert np.array_equal(got, want)
    assert want[3, 0, :4].tolist() == [-2 ** 31, 2 ** 31 - 1, -2, 0]
    wide = w[1].astype(np.int64) + w[3].astype(np.int64)
    assert ((wide >= 2 ** 31) | (wide < -2 ** 31)).sum() > 1000   # the random pairs overflow as well
    assert bool((tc == 3).all())
    for src, dst in ((0, 0), (4, 0), (0, 4), (-1, 2)):
        with pytest.raises(L().G2048Error):
            L().ntuple_promote(net, src, dst, dev)
    one = L().make_ntuple_net(cells, wd[0], 0)
    with pytest.raises(L().G2048Error):
        L().ntuple_promote(one, 0, 1, dev)
    torch.cuda.synchronize()
    assert np.array_equal(wd.cpu().numpy(), want)


def test_promote_six_cell_tables(dev):
    """The largest tables, 4x6 with two stages (512 MB): the grid-stride loop covers them."""
    cells = R.PRESETS["4x6"]
    smap = SG.stage_map_of((2048,))
    wd = torch.zeros(2, 4, 16 ** 6, dtype=torch.int32, device=dev)
    wd[0] = torch.arange(4 * 16 ** 6, dtype=torch.int32, device=dev).reshape(4, -1)
    wd[1] = 1
    L().ntuple_promote(L().make_ntuple_net(cells, wd, smap), 0, 1, dev)
    torch.cuda.synchronize()
    assert bool((wd[1] == wd[0] + 1).all())


# -------------------------------------------------------------------------- trainer and commands -----
@pytest.fixture(scope="module")
def trainer_ref():
    tr = SG.TrainerRef(R.PRESETS["lines-squares-4"], SG.STAGES, envs=64, promote_every=TRAIN_P)
    tr.train(TRAIN_STEPS)
    assert len(tr.promoted) >= 2 and tr.onto_nonzero >= 1, (tr.promoted, tr.onto_nonzero)
    return tr


def _trainer(dev, chunks, P):
    from g2048.ntuple import NTupleNet, NTupleTrainer
    net = NTupleNet("lines-squares-4", dev, stages=SG.STAGES)
    tr = NTupleTrainer(net, envs=64, promote_every=P)
    outs = [tr.train(k) for k in chunks]
    torch.cuda.synchronize()
    return net, tr, outs


def test_trainer(dev, trainer_ref):
    """64 envs, lines-squares-4, the defaults otherwise: the cuts fall after 40 and 80 steps however train()
    is called; the reference promotes 1 and 2 at the first (both onto stages that had learned) and 3 at the
    second."""
    ref = trainer_ref
    results = []
    for chunks in ((37, 63), (13, 50, 37), (100,)):
        net, tr, outs = _trainer(dev, chunks, TRAIN_P)
        assert np.array_equal(net.weights.cpu().numpy(), ref.st.weights), chunks
        assert np.array_equal(tr.boards.cpu().numpy(), ref.st.boards), chunks
        assert sum((o["promoted"] for o in outs), []) == ref.promoted and tr.promoted_upto == max(ref.promoted)
        assert sum(o["updates"] for o in outs) == ref.st.stats[3] and tr.counter == 1 + TRAIN_STEPS
        results.append(outs)
    assert results[0][0]["promoted"] == [] and results[1][1]["promoted"] == ref.promoted[:-1]
    net, tr, outs = _trainer(dev, (100,), 0)
    assert outs[0]["promoted"] == [] and not np.array_equal(net.weights.cpu().numpy(), ref.st.weights)
    off = SG.TrainerRef(R.PRESETS["lines-squares-4"], SG.STAGES, envs=64)
    off.train(TRAIN_STEPS)
    assert np.array_equal(net.weights.cpu().numpy(), off.st.weights)


def test_trainer_tc_with_trace(dev):
    """Rule tc with a trace on a staged net: the accumulators have the staged shape and are not promoted."""
    from g2048.ntuple import NTupleNet, NTupleTrainer
    ref = SG.TrainerRef(R.PRESETS["lines-squares-4"], SG.STAGES, envs=64, rule="tc", h=3, promote_every=TRAIN_P)
    ref.train(60)
    net = NTupleNet("lines-squares-4", dev, stages=SG.STAGES)
    tr = NTupleTrainer(net, envs=64, rule="tc", trace_len=3, promote_every=TRAIN_P)
    out = tr.train(60)
    torch.cuda.synchronize()
    assert out["promoted"] == ref.promoted and len(ref.promoted) >= 1
    assert tuple(tr.tc.shape) == (4, 5, 65536, 2) and np.array_equal(tr.tc.cpu().numpy(), ref.tc)
    assert np.array_equal(net.weights.cpu().numpy(), ref.st.weights)


def test_commands(dev, tmp_path, trainer_ref):
    """`train-ntuple --stages 16,64,128 --promote-every 40 --envs 64 --steps 100 --out f` writes the reference's
    weights and stages; `play-ntuple f -g 4 --max-moves 40 --depth 2` prints the scores of the oracle-driven
    games on the staged reference; --stages 16,16 and --promote-every without --stages are refused."""
    ref = trainer_ref
    out = tmp_path / "net.pt"
    base = [sys.executable, str(PKG / "train.py")]
    cmd = base + ["train-ntuple", "--stages", "16,64,128", "--promote-every", str(TRAIN_P), "--envs", "64", "--steps",
                  str(TRAIN_STEPS), "--print-freq", "30", "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert any(ln.startswith("n-tuple net lines-squares-4") and "stages 16,64,128, promote_every 40" in ln
               for ln in r.stdout.splitlines())
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert np.array_equal(ck["weights"].numpy(), ref.st.weights) and ck["stages"] == list(SG.STAGES)
    r = subprocess.run(base + ["play-ntuple", str(out), "-g", "4", "--max-moves", "40", "--depth", "2"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    scores, boards = SG.cpu_play(ref.st.cells, ref.st.weights, 2, [0, 1, 2, 3], 40, MAP)
    s = scores.tolist()
    assert f"Eval Results - Max: {max(s):.0f}, Avg: {sum(s) / 4:.1f}, Median: {sorted(s)[2]:.0f}" in r.stdout
    plain = SG.cpu_play(ref.st.cells, ref.st.weights[0], 2, [0, 1, 2, 3], 40, 0)[0]
    assert plain.tolist() != s                                   # stage 0's tables alone play other games
    for extra, msg in ((["--stages", "16,16"], "--stages must be"), (["--promote-every", "5"], "--promote-every must be")):
        r = subprocess.run(base + ["train-ntuple", "--steps", "10"] + extra, cwd=tmp_path, capture_output=True, text=True,
                           timeout=170)
        assert r.returncode != 0 and msg in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
