"""TD(lambda) and TC(lambda) learning of the n-tuple network on the GPU (g2048_ntuple_lambda: nt_tc_weights_kernel
and nt_update_kernel of csrc/ntuple.hip with the trace; NTupleTrainer(trace_len=...); train-ntuple --trace), bit for bit
against the numpy reference of tests/ntuple_lambda_reference.py: every add is an integer fixed by reads
that see the state before the step's adds, so the weights, the accumulators and the carried history
after n envs learned in parallel must be the CPU's bytes whatever the order of the atomics.  The
workspace is filled with garbage before every call.

The cases are ntuple_lambda_reference.CASES x TRACES: the starts of R.td_start at the rule's own lr_shift,
200 steps from counter 1, (trace_len, lambda_shift) in (1, 1), (3, 1), (4, 2).  Before a device result is
compared, the reference run of the case must show what the test claims to cover
(ntuple_lambda_reference.covers).  Rows of hist at or beyond hist_len hold nothing and are not compared.

Changed to meet the coverage: n1-zero runs under game seed 34 instead of 31 (ntuple_lambda_reference.SEEDS:
under 31 its one env ends no second game within 200 steps at (3, 1), so no history is ever cut and no
terminal update reaches one).
Rule tc on n300-random starts envs 4..298 on mid-game boards instead of R.td_start's ending and fresh ones
(ntuple_lambda_reference.start has the reason and the figures): with R.td_start's boards its weights
diverge in the first updates and no error ever decays to 0 at s = 2; with the changed boards one does, once
in the run.  Its net, weights, accumulators, lr_shift 4, step count and game seed are the case's own."""

import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_stage_reference as SR
import ntuple_tc_reference as C
from conftest import PKG

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
KEYS = ("weights", "tc", "boards", "after", "hist", "hist_len", "pending", "run_score", "stats")


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


class Run:
    """The device state of one g2048_ntuple_lambda run; tc None: rule TD; h = 0 with null hist / hist_len."""

    def __init__(self, dev, cells, weights, boards, tc, h):
        n = len(boards)
        self.dev, self.n, self.h = dev, n, h
        self.w = to_dev(weights, dev)
        self.net = L().make_ntuple_net(cells, self.w)
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
        L().ntuple_lambda(self.net, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                          self.run_score, steps, lr_shift, self.h, s, L().make_rng(L().RNG_PHILOX, seed, counter),
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
    """Everything the call carries, against the reference state."""
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


def assert_same(a, b):
    assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def device_run(dev, rule, name, fill, h, s, splits, n=None, start=None):
    """The case (or the given start) on the device in calls of `splits` steps each, the counter advanced from 1."""
    cells, w, boards, lr_shift, tc = start or LR.start(rule, name, fill)
    run = Run(dev, cells, w, boards[:n], tc, h)
    counter = 1
    for steps in splits:
        run.call(steps, lr_shift, s, counter, LR.seed_of(name))
        counter += steps
    return run.results()


@pytest.mark.parametrize("h,s", LR.TRACES)
@pytest.mark.parametrize("rule,name,fill", LR.CASES)
def test_lambda_bit_exact(dev, rule, name, fill, h, s):
    st, tc, ev = LR.ref_case(rule, name, fill, h, s)
    LR.covers(name, s, ev)
    got = device_run(dev, rule, name, fill, h, s, [LR.STEPS])
    assert_equal(got, st, tc)
    if (name, h) in (("n64-random", 3), ("n64-zero", 3)):  # a path that dropped the trace fails here
        cells, w, boards, lr_shift, tc0 = LR.start(rule, name, fill)
        plain = LR.td_lambda(LR.LState(cells, w, boards, 0), tc0, LR.STEPS, lr_shift, s, LR.seed_of(name), 1)
        assert not np.array_equal(got["weights"], plain.weights)


@pytest.mark.parametrize("rule", ["td", "tc"])
def test_trace_zero_is_td_and_tc(dev, rule):
    """h = 0 with null hist / hist_len gives g2048_ntuple_td / g2048_ntuple_tc bit for bit, whatever lambda_shift:
    on n300-random as R.td_start / C.tc_start give it."""
    start = C.tc_start("n300-random", "prefilled") if rule == "tc" else R.td_start("n300-random") + (None,)
    cells, w, boards, lr_shift, tc0 = start
    got = device_run(dev, rule, "n300-random", None, 0, 5, [LR.STEPS], start=start)
    assert "hist" not in got and "hist_len" not in got
    n = len(boards)
    wd, b = to_dev(w, dev), to_dev(boards, dev)
    net = L().make_ntuple_net(cells, wd)
    after = torch.zeros(n, 16, dtype=torch.int8, device=dev)
    pending = torch.zeros(n, dtype=torch.uint8, device=dev)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    rng = L().make_rng(L().RNG_PHILOX, LR.SEED, 1)
    ws = torch.empty(L().ntuple_td_workspace_bytes(n), dtype=torch.uint8, device=dev)
    old = {}
    if rule == "tc":
        acc = to_dev(tc0, dev)
        L().ntuple_tc(net, acc, b, after, pending, score, LR.STEPS, lr_shift, rng, stats, ws)
        old["tc"] = acc
    else:
        L().ntuple_td(net, b, after, pending, score, LR.STEPS, lr_shift, rng, stats, ws)
    old.update(weights=wd, boards=b, after=after, pending=pending, run_score=score, stats=stats)
    torch.cuda.synchronize()
    assert_same(got, {k: v.cpu().numpy() for k, v in old.items()})
    assert (got["weights"] != w).any() and got["stats"][3] > 0


@pytest.mark.parametrize("staged", [False, True], ids=["one-stage", "staged"])
@pytest.mark.parametrize("rule", ["td", "tc"])
def test_trace_zero_leaves_hist_alone(dev, rule, staged):
    """h = 0 with hist int8 [4, n, 16] and hist_len uint8 [n] given all the same: the call runs the kernels
    without a trace, both buffers keep their guard byte and everything else is g2048_ntuple_td / _tc's, byte for
    byte.  n = 65 (one full wave and one lane), 20 steps, the first 65 envs of n300-random with the usual and
    with SR.STAGES' tables."""
    n, steps, guard = 65, 20, 0xA5
    smap = SR.stage_map_of(SR.STAGES) if staged else 0
    cells, w, boards, lr_shift, tc0 = SR.start(rule, "n300-random", "prefilled" if rule == "tc" else None, smap)

    def state():
        s = dict(weights=to_dev(w, dev), boards=to_dev(boards[:n], dev),
                 after=torch.zeros(n, 16, dtype=torch.int8, device=dev),
                 pending=torch.zeros(n, dtype=torch.uint8, device=dev),
                 run_score=torch.zeros(n, dtype=torch.int64, device=dev),
                 stats=torch.zeros(4, dtype=torch.int64, device=dev))
        if rule == "tc":
            s["tc"] = to_dev(tc0, dev)
        return s, L().make_ntuple_net(cells, s["weights"], smap)

    rng = L().make_rng(L().RNG_PHILOX, LR.SEED, 1)
    ws = torch.full((L().ntuple_lambda_workspace_bytes(n),), GARBAGE, dtype=torch.uint8, device=dev)
    hist = torch.full((4, n, 16), guard - 256, dtype=torch.int8, device=dev)
    hist_len = torch.full((n,), guard, dtype=torch.uint8, device=dev)
    new, net = state()
    L().ntuple_lambda(net, new.get("tc"), new["boards"], new["after"], hist, hist_len, new["pending"],
                      new["run_score"], steps, lr_shift, 0, 5, rng, new["stats"], ws)
    old, net = state()
    ws.fill_(GARBAGE)
    if rule == "tc":
        L().ntuple_tc(net, old["tc"], old["boards"], old["after"], old["pending"], old["run_score"], steps, lr_shift,
                      rng, old["stats"], ws)
    else:
        L().ntuple_td(net, old["boards"], old["after"], old["pending"], old["run_score"], steps, lr_shift, rng,
                      old["stats"], ws)
    torch.cuda.synchronize()
    assert bool((hist == guard - 256).all()) and bool((hist_len == guard).all())
    new, old = ({k: v.cpu().numpy() for k, v in s.items()} for s in (new, old))
    assert_same(new, old)
    assert (new["weights"] != w).any() and new["stats"][3] > 0


@pytest.mark.parametrize("rule,name,fill", [("td", "n64-random", None), ("tc", "n64-zero", "prefilled")])
def test_continuation(dev, rule, name, fill):
    """200 steps equal 120 + 80 steps with the counter advanced by 120: hist and hist_len are carried."""
    st, tc, _ = LR.ref_case(rule, name, fill, 3, 1)
    one = device_run(dev, rule, name, fill, 3, 1, [200])
    two = device_run(dev, rule, name, fill, 3, 1, [120, 80])
    assert_same(one, two)
    assert_equal(two, st, tc)


def test_determinism(dev):
    a = device_run(dev, "td", "n300-zero", None, 3, 1, [LR.STEPS])
    b = device_run(dev, "td", "n300-zero", None, 3, 1, [LR.STEPS])
    assert_same(a, b)
    assert (a["weights"] != 0).any() and int(a["hist_len"].max()) == 3


@pytest.mark.parametrize("rule", ["td", "tc"])
def test_no_envs_is_a_noop(dev, rule):
    cells, w, boards, lr_shift, tc0 = LR.start(rule, "n64-zero", "prefilled" if rule == "tc" else None)
    w = R.random_weights(cells, 3)
    run = Run(dev, cells, w, boards[:0], tc0, 3)
    run.stats.fill_(7)
    run.call(5, lr_shift, 1, 1)
    got = run.results()
    assert np.array_equal(got["weights"], w) and got["stats"].tolist() == [7] * 4
    assert tc0 is None or np.array_equal(got["tc"], tc0)
    assert bool((run.ws == GARBAGE).all())


@pytest.mark.parametrize("rule", ["td", "tc"])
def test_ragged_last_block(dev, rule):
    """n = 257: one lane in the second block.  The first 257 envs of n300-zero for 60 steps at (3, 1); env 256
    starts on the board one move from its end."""
    fill = "zero" if rule == "tc" else None
    cells, w, boards, lr_shift, tc = LR.start(rule, "n300-zero", fill)
    ev = {}
    st = LR.td_lambda(LR.LState(cells, w, boards[:257], 3), tc, 60, lr_shift, 1, LR.SEED, 1, events=ev)
    assert ev["traced"] > 0 and ev["full"] > 0 and ev["cut"] > 0 and ev["terminal_traced"] > 0 and ev["shared"] > 0
    assert st.hist_len[256] > 0 or st.stats[0] > 0
    got = device_run(dev, rule, "n300-zero", fill, 3, 1, [60], n=257)
    assert_equal(got, st, tc)


# ------------------------------------------------------------------------- trainer and command -----
def _trainer_reference(rule, steps=50, envs=64, lr_shift=10, seed=0x2048, h=3, s=1):
    from oracle import oracle as O
    cells = R.PRESETS["lines-squares-4"]
    st = LR.LState(cells, np.zeros((5, 65536), np.int32), O.reset(envs, seed=seed, step_idx=0), h)
    tc = np.zeros((5, 65536, 2), np.int64) if rule == "tc" else None
    LR.td_lambda(st, tc, steps, lr_shift, s, seed, 1)
    return st, tc


@pytest.mark.parametrize("rule", ["td", "tc"])
def test_trainer(dev, rule):
    """NTupleTrainer(trace_len=3) for 50 steps of 64 envs (the defaults otherwise) equals the reference."""
    from g2048.ntuple import NTupleNet, NTupleTrainer
    st, tc = _trainer_reference(rule)
    net = NTupleNet("lines-squares-4", dev)
    tr = NTupleTrainer(net, envs=64, rule=rule, trace_len=3)
    first, second = tr.train(20), tr.train(30)
    torch.cuda.synchronize()
    assert (tr.lr_shift, tr.seed, tr.lambda_shift, tr.counter) == (10, 0x2048, 1, 51)
    assert np.array_equal(net.weights.cpu().numpy(), st.weights) and (st.weights != 0).any()
    assert np.array_equal(tr.boards.cpu().numpy(), st.boards) and np.array_equal(tr.after.cpu().numpy(), st.after)
    assert tuple(tr.hist.shape) == (3, 64, 16) and np.array_equal(tr.hist_len.cpu().numpy(), st.hist_len)
    assert np.array_equal(LR.valid_hist(tr.hist.cpu().numpy(), st.hist_len), LR.valid_hist(st.hist, st.hist_len))
    if rule == "tc":
        assert np.array_equal(tr.tc.cpu().numpy(), tc)
    assert [first[k] + second[k] for k in ("games", "score_sum", "updates")] == st.stats[[0, 1, 3]].tolist()
    assert second["updates"] > 0


def test_commands(dev, tmp_path):
    """`train-ntuple --trace 3 --lambda-shift 1 --envs 64 --steps 50` in a child process writes the net of
    the trainer's run (the reference's weights); `--trace 5` is refused."""
    st, _ = _trainer_reference("td")
    out = tmp_path / "net.pt"
    cmd = [sys.executable, str(PKG / "train.py"), "train-ntuple", "--trace", "3", "--lambda-shift", "1", "--envs", "64",
           "--steps", "50", "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert any(ln.startswith("n-tuple net lines-squares-4") and "trace 3, lambda_shift 1, rule td" in ln
               for ln in r.stdout.splitlines())
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert np.array_equal(ck["weights"].numpy(), st.weights)
    cmd = [sys.executable, str(PKG / "train.py"), "train-ntuple", "--trace", "5", "--steps", "50"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode != 0 and "--trace must be in 0..4, got 5" in r.stdout
