"""Temporal-coherence learning of the n-tuple network on the GPU (g2048_ntuple_tc: nt_tc_weights_kernel,
nt_update_kernel of csrc/ntuple.hip; NTupleTrainer(rule="tc")), bit for bit against the numpy
reference of tests/ntuple_tc_reference.py: the weights' adds are integer quotients of accumulators read
before the step's adds, and the accumulators' adds are integer sums, so the weights and the
accumulators after n envs learned in parallel must be the CPU's bytes whatever the order of the atomics.
The workspace is filled with garbage before every call.

The cases are ntuple_tc_reference.TC_CASES: the starts of the TD(0) cases at lr_shift 8 (zero weights)
and 4 (random weights), 200 steps, each from zero accumulators and from prefilled ones (up to 62 bits,
|E| > A); tests/test_ntuple_tc_host.py pins what happens in them (fresh, damped and zeroed hits, the
shift of accumulators beyond 20 bits, the clamped rate, double hits, weights wrapping), and each test
asserts on the reference that it occurs."""

import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_reference as R
import ntuple_tc_reference as C
from conftest import PKG
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
KEYS = ("weights", "tc", "boards", "after", "pending", "run_score", "stats")


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


def garbage(*tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(GARBAGE)


def is_garbage(t):
    return bool((t.view(torch.uint8) == GARBAGE).all())


class TC:
    """The device state of one g2048_ntuple_tc run."""

    def __init__(self, dev, cells, weights, boards, tc, counter_dev=None):
        n = len(boards)
        self.dev, self.n = dev, n
        self.w = to_dev(weights, dev)
        self.net = L().make_ntuple_net(cells, self.w)
        self.tc = to_dev(tc, dev)
        self.boards = to_dev(boards, dev)
        self.after = torch.zeros(n, 16, dtype=torch.int8, device=dev)
        self.pending = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.run_score = torch.zeros(n, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws = torch.empty(L().ntuple_tc_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.counter_dev = counter_dev

    def call(self, steps, lr_shift, seed, counter):
        garbage(self.ws)
        L().ntuple_tc(self.net, self.tc, self.boards, self.after, self.pending, self.run_score, steps, lr_shift,
                      L().make_rng(L().RNG_PHILOX, seed, counter, counter_dev=self.counter_dev), self.stats, self.ws)

    def results(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in KEYS[1:]} | {"weights": self.w.cpu().numpy()}


def assert_tc_equal(got, st, tc):
    for k in KEYS:
        assert np.array_equal(got[k], tc if k == "tc" else getattr(st, k)), k


def ref_steps(name, fill, steps, stats=None):
    cells, w, boards, lr_shift, tc = C.tc_start(name, fill)
    st = C.td_tc(R.TDState(cells, w, boards, stats=stats), tc, steps, lr_shift, C.TC_SEED, 1)
    return st, tc


@pytest.mark.parametrize("name,fill", C.TC_CASES)
def test_tc_bit_exact(dev, name, fill):
    st, tc_ref, ev = C.ref_case(name, fill)
    C.covers(name, fill, ev)
    cells, w, boards, lr_shift, tc0 = C.tc_start(name, fill)
    tc = TC(dev, cells, w, boards, tc0)
    tc.call(C.TC_STEPS, lr_shift, C.TC_SEED, 1)
    got = tc.results()
    assert_tc_equal(got, st, tc_ref)
    if (name, fill) == ("n64-zero", "zero"):  # a TC path that ran plain TD(0) fails here
        td = R.td(R.TDState(cells, w, boards), C.TC_STEPS, lr_shift, C.TC_SEED, 1)
        assert not np.array_equal(got["weights"], td.weights)


def test_tc_split_invariance(dev):
    """100 steps equal 50 + 50 with the counter advanced by 50, and the reference."""
    cells, w, boards, lr_shift, tc0 = C.tc_start("n64-random", "prefilled")
    st, tc_ref = ref_steps("n64-random", "prefilled", 100)
    one, two = TC(dev, cells, w, boards, tc0), TC(dev, cells, w, boards, tc0)
    one.call(100, lr_shift, C.TC_SEED, 1)
    two.call(50, lr_shift, C.TC_SEED, 1)
    two.call(50, lr_shift, C.TC_SEED, 51)
    a, b = one.results(), two.results()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert_tc_equal(a, st, tc_ref)


def test_tc_stats_accumulate_and_are_optional(dev):
    """stats is added to, not zeroed (the largest score by maximum); a null stats changes nothing else."""
    cells, w, boards, lr_shift, tc0 = C.tc_start("n64-zero", "zero")
    st, tc_ref = ref_steps("n64-zero", "zero", 30, stats=[5, 1000, 1 << 40, 7])
    assert st.stats[0] > 5 and st.stats[2] == 1 << 40 and st.stats[3] > 7
    tc = TC(dev, cells, w, boards, tc0)
    tc.stats.copy_(torch.tensor([5, 1000, 1 << 40, 7]))
    tc.call(30, lr_shift, C.TC_SEED, 1)
    assert_tc_equal(tc.results(), st, tc_ref)
    tc = TC(dev, cells, w, boards, tc0)
    garbage(tc.stats)
    keep, tc.stats = tc.stats, None
    tc.call(30, lr_shift, C.TC_SEED, 1)
    tc.stats = keep
    got = tc.results()
    assert is_garbage(keep)
    for k in KEYS[:-1]:
        assert np.array_equal(got[k], tc_ref if k == "tc" else getattr(st, k)), k


def test_tc_graph_replay(dev):
    """One captured steps = 8 call replayed three times with the device counter bumped by 8 equals 24
    eager steps (and the reference)."""
    cells, w, boards, lr_shift, tc0 = C.tc_start("n64-random", "zero")
    st, tc_ref = ref_steps("n64-random", "zero", 24)
    eager = TC(dev, cells, w, boards, tc0)
    eager.call(24, lr_shift, C.TC_SEED, 1)
    want = eager.results()
    assert_tc_equal(want, st, tc_ref)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    tc = TC(dev, cells, w, boards, tc0, counter_dev=ctr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = TC(dev, cells, w, boards, tc0, counter_dev=ctr)
        warm.call(8, lr_shift, C.TC_SEED, 1)  # warm-up outside the capture, on state of its own
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            L().ntuple_tc(tc.net, tc.tc, tc.boards, tc.after, tc.pending, tc.run_score, 8, lr_shift,
                          L().make_rng(L().RNG_PHILOX, C.TC_SEED, 1, counter_dev=ctr), tc.stats, tc.ws)
    torch.cuda.current_stream().wait_stream(side)
    garbage(tc.ws)
    for k in range(3):
        ctr.fill_(8 * k)
        g.replay()
    got = tc.results()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_tc_einval_and_empty(dev):
    """Every refusal of g2048_ntuple_td, and a null or misaligned tc: -1 and nothing enqueued."""
    import ctypes
    lib = L()
    cells, w, boards, lr_shift, tc0 = C.tc_start("n64-zero", "prefilled")
    tc = TC(dev, cells, w, boards, tc0)
    n0 = tc.n
    outs = (tc.ws, tc.after, tc.pending, tc.run_score, tc.stats)
    garbage(*outs)
    stream = lib._stream(tc.boards)
    rng = lib.make_rng(lib.RNG_PHILOX, C.TC_SEED, 1)

    def bad_net(T=5, K=4, cells=R.PRESETS["lines-squares-4"], ptr=tc.w.data_ptr()):
        flat = [c for t in cells for c in t]
        return lib.NtNet(T, K, (ctypes.c_int32 * 48)(*flat), ptr)

    bad_nets = [bad_net(T=0), bad_net(T=9), bad_net(K=0), bad_net(K=7), bad_net(ptr=None), bad_net(ptr=tc.w.data_ptr() + 4),
                bad_net(cells=[[0, 1, 2, 16]] * 5), bad_net(cells=[[0, 1, 2, -1]] * 5), bad_net(cells=[[0, 1, 2, 2]] * 5)]

    def s_tc(net=tc.net, acc=tc.tc.data_ptr(), boards=tc.boards.data_ptr(), after=tc.after.data_ptr(),
             pending=tc.pending.data_ptr(), run_score=tc.run_score.data_ptr(), n=n0, steps=3, lr=lr_shift, rng=rng,
             stats=tc.stats.data_ptr(), ws=tc.ws.data_ptr(), ws_bytes=tc.ws.numel()):
        return lib.load().g2048_ntuple_tc(stream, ctypes.byref(net) if net is not None else None, acc, boards, after,
                                          pending, run_score, n, steps, lr, ctypes.byref(rng) if rng is not None else None,
                                          stats, ws, ws_bytes)

    assert s_tc(net=None) == -1
    for bn in bad_nets:
        assert s_tc(net=bn) == -1
    assert s_tc(acc=None) == -1 and s_tc(acc=tc.tc.data_ptr() + 8) == -1  # a null, a misaligned tc
    assert s_tc(n=-1) == -1 and s_tc(n=1 << 40) == -1 and s_tc(n=1 << 28) == -1
    assert s_tc(boards=None) == -1 and s_tc(boards=tc.boards.data_ptr() + 8) == -1
    assert s_tc(n=0) == 0  # a no-op
    for steps in (0, -1):
        assert s_tc(steps=steps) == -1
    for lr in (0, 31, -1):
        assert s_tc(lr=lr) == -1
    assert s_tc(rng=None) == -1
    assert s_tc(rng=lib.make_rng(lib.RNG_INJECT, 1, 1)) == -1 and s_tc(rng=lib.make_rng(lib.RNG_MT19937, 1, 1)) == -1
    for null in ("after", "pending", "run_score", "ws"):
        assert s_tc(**{null: None}) == -1
    assert s_tc(after=tc.after.data_ptr() + 8) == -1 and s_tc(ws=tc.ws.data_ptr() + 8) == -1
    need = lib.ntuple_tc_workspace_bytes(n0)
    assert need == tc.ws.numel() and s_tc(ws_bytes=need - 1) == -1
    torch.cuda.synchronize()
    assert all(is_garbage(t) for t in outs)  # nothing was enqueued by any of them
    assert np.array_equal(tc.w.cpu().numpy(), w) and np.array_equal(tc.tc.cpu().numpy(), tc0)
    assert np.array_equal(tc.boards.cpu().numpy(), boards)
    # the range ends of lr_shift are accepted
    for lr in (30, 1):
        acc = tc0.copy()
        st = C.td_tc(R.TDState(cells, w, boards), acc, 3, lr, C.TC_SEED, 1)
        tc = TC(dev, cells, w, boards, tc0)
        tc.call(3, lr, C.TC_SEED, 1)
        assert_tc_equal(tc.results(), st, acc)


# --------------------------------------------------------------------- trainer, quality, commands -----
def test_tc_training_quality(dev):
    """Train lines-squares-4 with 256 envs for 600 steps at lr_shift 10, seed 5 under rule "tc": the weights,
    the accumulators and the statistics are the CPU's, bit for bit.  Then 32 Philox games (game seed 7)
    played to the end are the CPU loop's, and their mean score, 8 816.75 on the CPU, exceeds the zero
    net's 3 090.625 on the same games; no game needs the cap of 4 096 moves (the longest takes 889).
    Printed, not asserted: TD(0) of the same run scores 8 726.625 (test_gpu_ntuple.test_training_quality);
    32 games of one seed do not carry a ranking."""
    from g2048.ntuple import NTupleNet, NTuplePlayer, NTupleTrainer
    cells = R.PRESETS["lines-squares-4"]
    st = R.TDState(cells, np.zeros((5, 65536), np.int32), O.reset(256, seed=5, step_idx=0))
    acc = np.zeros((5, 65536, 2), np.int64)
    C.td_tc(st, acc, 600, 10, 5, 1)
    net = NTupleNet("lines-squares-4", dev)
    tr = NTupleTrainer(net, envs=256, lr_shift=10, seed=5, rule="tc")
    stats = tr.train(600)
    torch.cuda.synchronize()
    assert np.array_equal(net.weights.cpu().numpy(), st.weights)
    assert tuple(tr.tc.shape) == (5, 65536, 2) and np.array_equal(tr.tc.cpu().numpy(), acc)
    E, A = tr.accumulators()
    assert np.array_equal(E.cpu().numpy(), acc[..., 0]) and np.array_equal(A.cpu().numpy(), acc[..., 1])
    assert np.array_equal(tr.boards.cpu().numpy(), st.boards)
    assert [stats["games"], stats["score_sum"], stats["max_score"], stats["updates"]] == st.stats.tolist()
    assert stats["games"] > 0 and tr.counter == 601
    cap = 4096
    res = NTuplePlayer(net).play_games(32, max_moves=cap, game_seed=7)
    scores, moves, boards = R.cpu_play(cells, st.weights, 32, cap, 7)
    zero, _, zero_boards = R.cpu_play(cells, np.zeros_like(st.weights), 32, cap, 7)
    assert moves.max() < cap and (O.legal_mask(boards) == 0).all() and (O.legal_mask(zero_boards) == 0).all()
    assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist()
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
    print("TC mean", scores.mean(), "zero-net mean", zero.mean(), "TD(0) mean of the same run 8726.625; longest game",
          int(moves.max()), "moves")
    assert np.mean(res["scores"]) > zero.mean()
    assert (scores.mean(), zero.mean()) == (8816.75, 3090.625)


def test_tc_commands_run(tmp_path):
    """`train-ntuple --rule tc` then `play-ntuple` as a user runs them, each in a fresh child process, and the
    refusal of an unknown rule."""
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    out = tmp_path / "nets" / "net.pt"
    cmd = [sys.executable, str(PKG / "train.py"), "train-ntuple", "--rule", "tc", "--steps", "50", "--print-freq", "25",
           "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("n-tuple net lines-squares-4") and ln.endswith("rule tc") for ln in lines)
    assert sum(ln.startswith("step ") and "games " in ln and "mean score " in ln for ln in lines) == 2
    assert out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert sorted(ck) == ["cells", "weights"]  # the net only
    assert ck["cells"] == R.PRESETS["lines-squares-4"] and ck["weights"].dtype == torch.int32
    assert int((ck["weights"] != 0).sum()) > 0
    cmd = [sys.executable, str(PKG / "train.py"), "play-ntuple", str(out), "-g", "4", "--max-moves", "30"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert any(ln.startswith("Eval Results - Max: ") and "Avg: " in ln for ln in r.stdout.splitlines())
    cmd = [sys.executable, str(PKG / "train.py"), "train-ntuple", "--rule", "nope", "--steps", "50"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 1 and "Unknown learning rule: nope" in r.stdout
