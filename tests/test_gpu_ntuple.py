"""The n-tuple network on the GPU (csrc/ntuple.hip, g2048/ntuple.py), bit for bit against the numpy
reference of tests/ntuple_reference.py: every value is an integer and every update an integer add, so
the weights after n envs learned in parallel must be the CPU's bytes whatever the order of the atomics.
Outputs and the workspace are filled with garbage before every call.

value / choose: the 33 boards of value_boards() (8 finished roots, live roots with illegal actions,
exponents 15 and 16) under random signed weights on four nets: every tuple length the dispatch
instantiates that a test can afford, the longest (K = 6, a 128 MiB table) included.  td: the cases of
ntuple_reference.TD_CASES, 200 steps from boards of which half are one move from their end and one is
dead; tests/test_ntuple_host.py pins what happens in them (games ending, the dead board, two envs adding
to one weight, a self-symmetric tuple's double hit, the small negative deltas the rounding rule takes
to 0), and each test asserts on the reference that they occur.
"""

import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_reference as R
from conftest import PKG
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A


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


@functools.lru_cache(maxsize=None)
def net_weights(net):
    w = R.random_weights(R.NETS[net], 3)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def ref_choice(net):
    """-> (value, q, legal, best) of the reference on value_boards() (read-only, shared)."""
    cells, w, b = R.NETS[net], net_weights(net), R.value_boards()
    q, legal, best, _ = R.choose(cells, w, b)
    out = (R.value(cells, w, b), q, legal, best)
    for a in out:
        a.setflags(write=False)
    return out


class Net:
    def __init__(self, dev, cells, weights):
        self.w = to_dev(weights, dev)
        self.c = L().make_ntuple_net(cells, self.w)


@pytest.fixture(scope="module")
def nets(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Net(dev, R.NETS[name], net_weights(name))
        return cache[name]
    return get


def run_choice(dev, net, boards):
    n = len(boards)
    b = to_dev(boards, dev)
    value = torch.empty(n, dtype=torch.int64, device=dev)
    q = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    garbage(value, q, legal, best)
    L().ntuple_value(net.c, b, value)
    L().ntuple_choose(net.c, b, q, legal, best)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (value, q, legal, best))


@pytest.mark.parametrize("name", ["lines-squares-4", "t1k1", "t8k3", "t2k6"])
def test_value_and_choice_bit_exact(dev, nets, name):
    val, q, legal, best = ref_choice(name)
    assert (legal == 0).sum() == 8 and (best[legal == 0] == 0xFF).all()   # finished boards
    assert ((legal != 0) & (legal != 15)).any() and (q == R.I64_MIN).any()  # illegal actions of live boards
    assert (R.value_boards() >= 15).any(1).sum() == 3                     # the clamp at exponent 15
    assert np.abs(val).max() > 1 << 32                                    # sums beyond 32 bits
    got = run_choice(dev, nets(name), R.value_boards())
    for g, r, nm in zip(got, (val, q, legal, best), ("value", "q", "legal", "best")):
        assert np.array_equal(g, r), nm


@pytest.mark.parametrize("n", [1, 3])
def test_small_shapes(dev, nets, n):
    boards = R.value_boards()[[5, 26, 31][:n]]
    val, q, legal, best = ref_choice("lines-squares-4")
    got = run_choice(dev, nets("lines-squares-4"), boards)
    for g, r in zip(got, (val, q, legal, best)):
        assert np.array_equal(g, r[[5, 26, 31][:n]])


def test_ties_take_the_lowest_index(dev):
    """Zero weights: q = S points, and the two top actions tie on boards of the set."""
    cells = R.NETS["lines-squares-4"]
    w = np.zeros((5, 65536), np.int32)
    q, legal, best, _ = R.choose(cells, w, R.value_boards())
    s = np.sort(q, 1)
    tie = (s[:, 3] > R.I64_MIN) & (s[:, 3] == s[:, 2])
    assert tie.sum() >= 5 and (best[tie] == q[tie].argmax(1)).all()
    got = run_choice(dev, Net(dev, cells, w), R.value_boards())
    assert np.array_equal(got[1], q) and np.array_equal(got[3], best) and (got[0] == 0).all()


def test_nullable_outputs(dev, nets):
    """q, legal and best are each optional; what is written does not depend on the others."""
    net, b = nets("t8k3"), to_dev(R.value_boards(), dev)
    n = len(R.value_boards())
    _, q_ref, legal_ref, best_ref = ref_choice("t8k3")
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
        q = torch.empty(n, 4, dtype=torch.int64, device=dev)
        legal = torch.empty(n, dtype=torch.uint8, device=dev)
        best = torch.empty(n, dtype=torch.uint8, device=dev)
        garbage(q, legal, best)
        L().ntuple_choose(net.c, b, *(t if k else None for t, k in zip((q, legal, best), keep)))
        torch.cuda.synchronize()
        for t, k, r in zip((q, legal, best), keep, (q_ref, legal_ref, best_ref)):
            assert np.array_equal(t.cpu().numpy(), r) if k else is_garbage(t)


# ------------------------------------------------------------------------------------- TD -----
class TD:
    """The device state of one g2048_ntuple_td run."""

    def __init__(self, dev, cells, weights, boards, counter_dev=None):
        n = len(boards)
        self.dev, self.n = dev, n
        self.net = Net(dev, cells, weights)
        self.boards = to_dev(boards, dev)
        self.after = torch.zeros(n, 16, dtype=torch.int8, device=dev)
        self.pending = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.run_score = torch.zeros(n, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws = torch.empty(L().ntuple_td_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.counter_dev = counter_dev

    def call(self, steps, lr_shift, seed, counter):
        garbage(self.ws)
        L().ntuple_td(self.net.c, self.boards, self.after, self.pending, self.run_score, steps, lr_shift,
                      L().make_rng(L().RNG_PHILOX, seed, counter, counter_dev=self.counter_dev), self.stats, self.ws)

    def results(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("boards", "after", "pending", "run_score", "stats")} | {
            "weights": self.net.w.cpu().numpy()}


def assert_td_equal(got, st):
    for k in ("weights", "boards", "after", "pending", "run_score", "stats"):
        assert np.array_equal(got[k], getattr(st, k)), k


@functools.lru_cache(maxsize=None)
def ref_td(name):
    cells, w, boards, lr_shift = R.td_start(name)
    ev = {}
    st = R.td(R.TDState(cells, w, boards), R.TD_STEPS, lr_shift, R.TD_SEED, 1, events=ev)
    return st, ev


@pytest.mark.parametrize("name", sorted(R.TD_CASES))
def test_td_bit_exact(dev, name):
    st, ev = ref_td(name)
    n = R.TD_CASES[name][1]
    assert ev["ended"] > 0 and (st.stats[0] > 0)            # games ending: pending = 2, the finished score
    assert ev["double"] > 0                                   # a self-symmetric tuple's double hit
    assert ev["neg_round"] > 0                                # -2^(lr_shift - 1) <= delta < 0 rounds to 0, not to -1
    if n > 1:
        assert ev["dead"] > 0 and ev["shared"] > 0            # a caller's dead board; two envs on one weight
    cells, w, boards, lr_shift = R.td_start(name)
    td = TD(dev, cells, w, boards)
    td.call(R.TD_STEPS, lr_shift, R.TD_SEED, 1)
    assert_td_equal(td.results(), st)


def test_td_split_invariance(dev):
    """100 steps equal 50 + 50 with the counter advanced by 50, and the reference."""
    cells, w, boards, lr_shift = R.td_start("n64-zero")
    st = R.td(R.TDState(cells, w, boards), 100, lr_shift, R.TD_SEED, 1)
    one, two = TD(dev, cells, w, boards), TD(dev, cells, w, boards)
    one.call(100, lr_shift, R.TD_SEED, 1)
    two.call(50, lr_shift, R.TD_SEED, 1)
    two.call(50, lr_shift, R.TD_SEED, 51)
    a, b = one.results(), two.results()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert_td_equal(a, st)


def test_td_stats_accumulate_and_are_optional(dev):
    """stats is added to, not zeroed (the largest score by maximum); a null stats changes nothing else."""
    cells, w, boards, lr_shift = R.td_start("n64-zero")
    st = R.td(R.TDState(cells, w, boards, stats=[5, 1000, 1 << 40, 7]), 30, lr_shift, R.TD_SEED, 1)
    assert st.stats[0] > 5 and st.stats[2] == 1 << 40
    td = TD(dev, cells, w, boards)
    td.stats.copy_(torch.tensor([5, 1000, 1 << 40, 7]))
    td.call(30, lr_shift, R.TD_SEED, 1)
    assert_td_equal(td.results(), st)
    td = TD(dev, cells, w, boards)
    garbage(td.stats)
    keep, td.stats = td.stats, None
    td.call(30, lr_shift, R.TD_SEED, 1)
    td.stats = keep
    got = td.results()
    assert is_garbage(keep) and np.array_equal(got["weights"], st.weights) and np.array_equal(got["boards"], st.boards)


def test_td_graph_replay(dev):
    """One captured steps = 8 call replayed three times with the device counter bumped by 8 equals 24
    eager steps (and the reference)."""
    cells, w, boards, lr_shift = R.td_start("n64-random")
    st = R.td(R.TDState(cells, w, boards), 24, lr_shift, R.TD_SEED, 1)
    eager = TD(dev, cells, w, boards)
    eager.call(24, lr_shift, R.TD_SEED, 1)
    want = eager.results()
    assert_td_equal(want, st)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    td = TD(dev, cells, w, boards, counter_dev=ctr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = TD(dev, cells, w, boards, counter_dev=ctr)
        warm.call(8, lr_shift, R.TD_SEED, 1)  # warm-up outside the capture, on state of its own
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            L().ntuple_td(td.net.c, td.boards, td.after, td.pending, td.run_score, 8, lr_shift,
                          L().make_rng(L().RNG_PHILOX, R.TD_SEED, 1, counter_dev=ctr), td.stats, td.ws)
    torch.cuda.current_stream().wait_stream(side)
    garbage(td.ws)
    for k in range(3):
        ctr.fill_(8 * k)
        g.replay()
    got = td.results()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_einval_and_empty(dev, nets):
    import ctypes
    lib = L()
    net = nets("lines-squares-4")
    cells, w, boards, lr_shift = R.td_start("n64-zero")
    td = TD(dev, cells, w, boards)
    n0 = td.n
    q = torch.empty(n0, 4, dtype=torch.int64, device=dev)
    value = torch.empty(n0, dtype=torch.int64, device=dev)
    legal = torch.empty(n0, dtype=torch.uint8, device=dev)
    best = torch.empty(n0, dtype=torch.uint8, device=dev)
    outs = (q, value, legal, best, td.ws, td.after, td.pending, td.run_score, td.stats)
    garbage(*outs)
    before = {k: v.copy() for k, v in td.results().items()}
    stream = lib._stream(td.boards)
    rng = lib.make_rng(lib.RNG_PHILOX, R.TD_SEED, 1)

    def bad_net(T=5, K=4, cells=R.PRESETS["lines-squares-4"], ptr=net.w.data_ptr()):
        flat = [c for t in cells for c in t]
        return lib.NtNet(T, K, (ctypes.c_int32 * 48)(*flat), ptr)

    bad_nets = [bad_net(T=0), bad_net(T=9), bad_net(K=0), bad_net(K=7), bad_net(ptr=None), bad_net(ptr=net.w.data_ptr() + 4),
                bad_net(cells=[[0, 1, 2, 16]] * 5), bad_net(cells=[[0, 1, 2, -1]] * 5), bad_net(cells=[[0, 1, 2, 2]] * 5)]

    def s_value(net=net.c, boards=td.boards.data_ptr(), value=value.data_ptr(), n=n0):
        return lib.load().g2048_ntuple_value(stream, ctypes.byref(net) if net is not None else None, boards, value, n)

    def s_choose(net=net.c, boards=td.boards.data_ptr(), q=q.data_ptr(), legal=legal.data_ptr(), best=best.data_ptr(),
                 n=n0):
        return lib.load().g2048_ntuple_choose(stream, ctypes.byref(net) if net is not None else None, boards, q, legal,
                                              best, n)

    def s_td(net=td.net.c, boards=td.boards.data_ptr(), after=td.after.data_ptr(), pending=td.pending.data_ptr(),
             run_score=td.run_score.data_ptr(), n=n0, steps=3, lr=lr_shift, rng=rng, stats=td.stats.data_ptr(),
             ws=td.ws.data_ptr(), ws_bytes=td.ws.numel()):
        return lib.load().g2048_ntuple_td(stream, ctypes.byref(net) if net is not None else None, boards, after,
                                          pending, run_score, n, steps, lr, ctypes.byref(rng) if rng is not None else None,
                                          stats, ws, ws_bytes)

    for fn in (s_value, s_choose, s_td):
        assert fn(net=None) == -1
        for bn in bad_nets:
            assert fn(net=bn) == -1
        assert fn(n=-1) == -1 and fn(n=1 << 40) == -1
        assert fn(boards=None) == -1 and fn(boards=td.boards.data_ptr() + 8) == -1
        assert fn(n=0) == 0  # a no-op
    assert s_value(value=None) == -1 and s_value(n=1 << 31) == -1
    assert s_choose(q=None, legal=None, best=None) == -1 and s_choose(q=q.data_ptr() + 8) == -1
    assert s_choose(n=1 << 31) == -1
    assert s_td(n=1 << 28) == -1
    for steps in (0, -1):
        assert s_td(steps=steps) == -1
    for lr in (0, 31, -1):
        assert s_td(lr=lr) == -1
    assert s_td(rng=None) == -1
    assert s_td(rng=lib.make_rng(lib.RNG_INJECT, 1, 1)) == -1 and s_td(rng=lib.make_rng(lib.RNG_MT19937, 1, 1)) == -1
    for null in ("after", "pending", "run_score", "ws"):
        assert s_td(**{null: None}) == -1
    assert s_td(after=td.after.data_ptr() + 8) == -1 and s_td(ws=td.ws.data_ptr() + 8) == -1
    need = lib.ntuple_td_workspace_bytes(n0)
    assert need == td.ws.numel() and s_td(ws_bytes=need - 1) == -1
    torch.cuda.synchronize()
    assert all(is_garbage(t) for t in outs)  # nothing was enqueued by any of them
    assert np.array_equal(td.net.w.cpu().numpy(), before["weights"]) and np.array_equal(td.boards.cpu().numpy(), boards)
    # the range ends of lr_shift are accepted
    for lr in (30, 1):
        st = R.td(R.TDState(cells, w, boards), 3, lr, R.TD_SEED, 1)
        td = TD(dev, cells, w, boards)
        td.call(3, lr, R.TD_SEED, 1)
        assert_td_equal(td.results(), st)


# ------------------------------------------------------------------ player, quality, commands -----
def test_player_exact(dev, nets):
    """8 Philox games of 60 moves under random weights: score for score and board for board the CPU loop."""
    from g2048.ntuple import NTupleNet, NTuplePlayer
    cells, w = R.NETS["lines-squares-4"], net_weights("lines-squares-4")
    player = NTuplePlayer(NTupleNet(cells, dev, torch.from_numpy(np.array(w))))
    res = player.play_games(8, max_moves=60, game_seed=99)
    scores, moves, boards = R.cpu_play(cells, w, 8, 60, 99)
    assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist()
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
    best, q, legal = player.choose(to_dev(R.value_boards(), dev))
    torch.cuda.synchronize()
    _, q_ref, legal_ref, best_ref = ref_choice("lines-squares-4")
    assert np.array_equal(best.cpu().numpy(), best_ref) and np.array_equal(q.cpu().numpy(), q_ref)
    assert np.array_equal(legal.cpu().numpy(), legal_ref)


def test_player_mt_games(dev):
    """Seeded MT19937 games run in the shared game loop; the zero net plays greedy on points."""
    from g2048.ntuple import NTupleNet, NTuplePlayer
    a = NTuplePlayer(NTupleNet("lines-squares-4", dev)).play_games(4, max_moves=20, seeds=[0, 1, 2, 3])
    b = NTuplePlayer(NTupleNet("4x6", dev)).play_games(4, max_moves=20, seeds=[0, 1, 2, 3])
    assert a["moves"] == [20] * 4 and a["scores"] == b["scores"] and torch.equal(a["boards"], b["boards"])


def test_training_quality(dev):
    """Train lines-squares-4 with 256 envs for 600 steps at lr_shift 10, seed 5 (NTupleTrainer: the reset
    at counter 0, the TD call at counter 1): the weights are the CPU's, bit for bit.  Then 32 Philox games
    (game seed 7) played to the end are the CPU loop's, and their mean score, 8 726.625 on the CPU,
    exceeds the zero net's (greedy on points) on the same games, 3 090.625 on the CPU; no game needs the
    cap of 4 096 moves (the longest takes 898)."""
    from g2048.ntuple import NTupleNet, NTuplePlayer, NTupleTrainer
    cells = R.PRESETS["lines-squares-4"]
    st = R.TDState(cells, np.zeros((5, 65536), np.int32), O.reset(256, seed=5, step_idx=0))
    R.td(st, 600, 10, 5, 1)
    net = NTupleNet("lines-squares-4", dev)
    tr = NTupleTrainer(net, envs=256, lr_shift=10, seed=5)
    stats = tr.train(600)
    torch.cuda.synchronize()
    assert np.array_equal(net.weights.cpu().numpy(), st.weights)
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
    print("trained mean", scores.mean(), "zero-net mean", zero.mean())
    assert np.mean(res["scores"]) > zero.mean()
    assert (scores.mean(), zero.mean()) == (8726.625, 3090.625)


def test_commands_run(tmp_path):
    """`train-ntuple` then `play-ntuple` as a user runs them, each in a fresh child process."""
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    out = tmp_path / "nets" / "net.pt"
    cmd = [sys.executable, str(PKG / "train.py"), "train-ntuple", "--steps", "50", "--print-freq", "25", "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert sum(ln.startswith("step ") and "games " in ln and "mean score " in ln for ln in lines) == 2
    assert out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["cells"] == R.PRESETS["lines-squares-4"] and ck["weights"].dtype == torch.int32
    assert int((ck["weights"] != 0).sum()) > 0
    cmd = [sys.executable, str(PKG / "train.py"), "play-ntuple", str(out), "-g", "4", "--max-moves", "30"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Eval Results - Max: ") and "Avg: " in ln and "Median: " in ln for ln in lines)
    assert any(ln.startswith("Tiles Reached - 512: ") and "2048: " in ln for ln in lines)
