"""The n-tuple expectimax search on the GPU (csrc/ntuple_search.hip, g2048_ntuple_search, NTuplePlayer
with depth >= 2), bit for bit against the level-by-level numpy reference of
tests/ntuple_search_reference.py: every value is an integer and every chance node is summed exactly
before its one floor division, so both lane mappings must give the CPU's bytes whatever the order of
their shuffles and atomics.  Outputs and the workspace are filled with garbage before every call.

The roots are the 33 boards of ntuple_reference.value_boards() (8 finished ones, live ones with illegal
actions, exponents 15 and 16) under 32-bit random signed weights; tests/test_ntuple_search_host.py pins
what they exercise (chance sums that are negative and not divisible, root q values a truncating division
would change, best moves that differ from depth 1's, dead inner boards) and checks the reference against
a scalar recursion.
"""

import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_reference as R
import ntuple_search_reference as SR
from conftest import PKG

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
AUTO, NARROW, WIDE = 0, 1, 2
FORMS = {1: (AUTO, NARROW), 2: (AUTO, NARROW, WIDE), 3: (AUTO, NARROW, WIDE)}
NAMES = ("q", "leaves", "legal", "best")


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
def net_weights(net, seed=SR.WEIGHT_SEED):
    w = R.random_weights(R.NETS[net], seed, bits=32)
    w.setflags(write=False)
    return w


def frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref(net, depth, seed=SR.WEIGHT_SEED):
    """-> (q, leaves, legal, best) of the reference on value_boards() (read-only, shared)."""
    return frozen(SR.search_ref(R.NETS[net], net_weights(net, seed), R.value_boards(), depth))


class Net:
    def __init__(self, dev, cells, weights):
        self.w = to_dev(weights, dev)
        self.c = L().make_ntuple_net(cells, self.w)


@pytest.fixture(scope="module")
def nets(dev):
    cache = {}

    def get(name, seed=SR.WEIGHT_SEED):
        if (name, seed) not in cache:
            if len(R.NETS[name][0]) == 6:
                cache.clear()  # one 128 MiB table at a time
            cache[(name, seed)] = Net(dev, R.NETS[name], net_weights(name, seed))
        return cache[(name, seed)]
    return get


class Call:
    """The device buffers of one g2048_ntuple_search call on `boards`."""

    def __init__(self, dev, boards, depth, form):
        n = len(boards)
        self.depth, self.form = depth, form
        self.boards = to_dev(boards, dev)
        self.q = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.leaves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.legal = torch.empty(n, dtype=torch.uint8, device=dev)
        self.best = torch.empty(n, dtype=torch.uint8, device=dev)
        nbytes = L().ntuple_search_workspace_bytes(n, depth, form)
        assert nbytes > 0 and nbytes % 16 == 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def outs(self):
        return self.q, self.leaves, self.legal, self.best

    def run(self, net, keep=(1, 1, 1)):
        garbage(*self.outs(), self.ws)
        leaves, legal, best = (t if k else None for t, k in zip(self.outs()[1:], keep))
        L().ntuple_search(net.c, self.boards, self.depth, self.q, leaves, legal, best, self.ws, self.form)

    def results(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in self.outs())


def search(dev, net, boards, depth, form):
    c = Call(dev, boards, depth, form)
    c.run(net)
    return c.results()


def assert_equal(got, want, what=""):
    for g, r, nm in zip(got, want, NAMES):
        assert np.array_equal(g, r), (nm, what)


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("name,seed", SR.GPU_CASES)
def test_search_bit_exact(dev, nets, name, seed, depth):
    want = ref(name, depth, seed)
    q, lv, legal, best = want
    assert (legal == 0).sum() == 8 and (best[legal == 0] == 0xFF).all() and (lv[legal == 0] == 0).all()
    assert ((legal != 0) & (legal != 15)).any() and (q == R.I64_MIN).any() and (lv[q == R.I64_MIN] == 0).all()
    assert int(lv.sum()) == {1: 86, 2: 3661, 3: 244639}[depth]
    first = None
    for form in FORMS[depth]:
        got = search(dev, nets(name, seed), R.value_boards(), depth, form)
        assert_equal(got, want, form)
        first = first or got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first)), form  # identical between forms


@pytest.mark.parametrize("name", ["lines-squares-4", "t1k1", "t8k3", "t2k6"])
def test_depth_one_is_ntuple_choose(dev, nets, name):
    net, n = nets(name), len(R.value_boards())
    b = to_dev(R.value_boards(), dev)
    q = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    garbage(q, legal, best)
    L().ntuple_choose(net.c, b, q, legal, best)
    torch.cuda.synchronize()
    for form in FORMS[1]:
        got = search(dev, net, R.value_boards(), 1, form)
        assert got[0].tobytes() == q.cpu().numpy().tobytes()
        assert np.array_equal(got[2], legal.cpu().numpy()) and np.array_equal(got[3], best.cpu().numpy())
        assert np.array_equal(got[1], (got[0] != R.I64_MIN).astype(np.int64))


@pytest.mark.parametrize("form", [AUTO, NARROW, WIDE])
@pytest.mark.parametrize("n", [1, 3])
def test_small_shapes(dev, nets, n, form):
    pick = [5, 26, 31][:n]
    got = search(dev, nets("lines-squares-4"), R.value_boards()[pick], 2, form)
    assert_equal(got, [r[pick] for r in ref("lines-squares-4", 2)])


def auto_form(n, depth):
    """The form AUTO resolves to: the one whose workspace size AUTO's equals (WIDE's is the larger)."""
    wb = L().ntuple_search_workspace_bytes
    return WIDE if wb(n, depth, AUTO) == wb(n, depth, WIDE) else NARROW


@pytest.mark.parametrize("n", [200, 1100])
def test_auto_at_depth_three(dev, nets, n):
    """value_boards() tiled and permuted to n boards at depth 3.  200 boards run AUTO and both forms; 1 100
    boards run AUTO alone, and the two counts lie on the two sides of AUTO's depth-3 threshold."""
    assert auto_form(200, 3) == WIDE and auto_form(1100, 3) == NARROW
    pick = np.random.default_rng(5).permutation(np.arange(n) % 33)
    assert len(set(pick.tolist())) == 33
    want = [r[pick] for r in ref("lines-squares-4", 3)]
    for form in (FORMS[3] if n == 200 else (AUTO,)):
        assert_equal(search(dev, nets("lines-squares-4"), R.value_boards()[pick], 3, form), want, form)


@functools.lru_cache(maxsize=None)
def const_case(fill, depth):
    """t8k3 (T = 8: |V| reaches the header's bound 64 x 2^31) with every weight `fill`."""
    cells = R.NETS["t8k3"]
    w = np.full((len(cells), 16 ** 3), fill, np.int64).astype(np.int32)
    st = {}
    out = frozen(SR.search_ref(cells, w, R.value_boards(), depth, stats=st))
    return w, out, st


@pytest.mark.parametrize("fill,depth", [(-(1 << 31), 3), ((1 << 31) - 1, 3), (0, 2), (0, 3)])
def test_signs(dev, fill, depth):
    """All-negative, all-positive and zero nets: the bound of the header and the signed floor."""
    w, want, st = const_case(fill, depth)
    q = want[0]
    live = q != R.I64_MIN
    assert live.sum() == 86 and st["dead"] >= 3
    if fill < 0:  # V = -2^37 everywhere: sums near the bound 160 x 2^37, negative and not divisible
        assert (q[live] < 0).sum() > 50 and q[live].min() < -(1 << 37) + (1 << 31) and st["neg_nondiv"] > 1000
        assert 1 << 44 < st["max_abs_sum"] < 1 << 46
    elif fill > 0:
        assert (q[live] > 0).all() and q[live].max() > 1 << 37 and 1 << 44 < st["max_abs_sum"] < 1 << 46
    else:         # the points alone
        assert (q[live] > 0).all() and st["neg_nondiv"] == 0
    net = Net(dev, R.NETS["t8k3"], w)
    for form in FORMS[depth]:
        assert_equal(search(dev, net, R.value_boards(), depth, form), want, form)


SYMMETRIC = np.array([0, 0, 0, 0, 0, 2, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.int8)  # its own transpose: UP = LEFT, DOWN = RIGHT


@pytest.mark.parametrize("depth", [2, 3])
def test_ties_and_dead_boards(dev, depth):
    """Zero net: on a board that is its own transpose the two best actions tie and the lower index wins;
    the dead board has no q at all; the ending board walks into dead children, whose M is 0."""
    cells = R.NETS["lines-squares-4"]
    w = np.zeros((5, 65536), np.int32)
    boards = np.concatenate([np.stack([SYMMETRIC, R.DEAD, R.ENDING]), R.value_boards()])
    st = {}
    want = SR.search_ref(cells, w, boards, depth, stats=st)
    q, lv, legal, best = want
    assert legal[0] == 15 and q[0, 0] == q[0, 2] and q[0, 1] == q[0, 3] and best[0] == (0 if q[0, 0] >= q[0, 1] else 1)
    s = np.sort(q, 1)
    assert ((s[:, 3] > R.I64_MIN) & (s[:, 3] == s[:, 2])).sum() >= 3
    assert (q[1] == R.I64_MIN).all() and best[1] == 0xFF and legal[1] == 0 and (lv[1] == 0).all()
    st_end = {}
    SR.search_ref(cells, w, R.ENDING[None], depth, stats=st_end)
    assert st_end["dead"] >= 1 and bin(int(legal[2])).count("1") >= 1
    net = Net(dev, cells, w)
    for form in FORMS[depth]:
        assert_equal(search(dev, net, boards, depth, form), want, form)


@pytest.mark.parametrize("form", [NARROW, WIDE])
def test_nullable_outputs(dev, nets, form):
    """leaves, legal and best are each optional; what is written does not depend on the others."""
    net, want = nets("t8k3"), ref("t8k3", 2)
    call = Call(dev, R.value_boards(), 2, form)
    for keep in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
        call.run(net, keep)
        torch.cuda.synchronize()
        assert np.array_equal(call.q.cpu().numpy(), want[0])
        for t, k, r in zip(call.outs()[1:], keep, want[1:]):
            assert np.array_equal(t.cpu().numpy(), r) if k else is_garbage(t)


def test_einval_and_empty(dev, nets):
    lib = L()
    net = nets("lines-squares-4")
    call = Call(dev, R.value_boards(), 3, WIDE)
    n0 = len(R.value_boards())
    garbage(*call.outs(), call.ws)
    stream = lib._stream(call.boards)
    need = {(d, f): lib.ntuple_search_workspace_bytes(n0, d, f) for d in (1, 2, 3) for f in (NARROW, WIDE)}
    assert need[(3, WIDE)] == call.ws.numel() and need[(2, WIDE)] == need[(3, WIDE)] and need[(1, WIDE)] == 0
    assert need[(1, NARROW)] == need[(3, NARROW)] == 16

    def bad_net(T=5, K=4, cells=R.PRESETS["lines-squares-4"], ptr=net.w.data_ptr()):
        flat = [c for t in cells for c in t]
        return lib.NtNet(T, K, (ctypes.c_int32 * 48)(*flat), ptr)

    def s(net=net.c, boards=call.boards.data_ptr(), n=n0, depth=3, form=WIDE, q=call.q.data_ptr(),
          leaves=call.leaves.data_ptr(), legal=call.legal.data_ptr(), best=call.best.data_ptr(),
          ws=call.ws.data_ptr(), ws_bytes=call.ws.numel()):
        return lib.load().g2048_ntuple_search(stream, ctypes.byref(net) if net is not None else None, boards, n, depth,
                                              form, q, leaves, legal, best, ws, ws_bytes)

    assert s(net=None) == -1
    for bn in (bad_net(T=0), bad_net(T=9), bad_net(K=0), bad_net(K=7), bad_net(ptr=None),
               bad_net(ptr=net.w.data_ptr() + 4), bad_net(cells=[[0, 1, 2, 16]] * 5), bad_net(cells=[[0, 1, 2, 2]] * 5)):
        assert s(net=bn) == -1
    for depth in (0, 4, -1, 1 << 40):
        assert s(depth=depth) == -1 and s(depth=depth, form=NARROW) == -1 and s(depth=depth, form=AUTO) == -1
    for form in (3, -1, 1 << 20):
        assert s(form=form) == -1
    assert s(depth=1, form=WIDE) == -1
    assert s(n=-1) == -1 and s(n=1 << 40) == -1 and s(n=1 << 31) == -1
    assert s(n=1 << 17) == -1 and s(n=1 << 24, form=NARROW) == -1   # lane counts of 2^31
    assert s(boards=None) == -1 and s(boards=call.boards.data_ptr() + 8) == -1
    assert s(q=None) == -1 and s(q=call.q.data_ptr() + 8) == -1
    assert s(leaves=call.leaves.data_ptr() + 8) == -1
    assert s(ws=None) == -1 and s(ws=call.ws.data_ptr() + 8) == -1
    assert s(ws_bytes=need[(3, WIDE)] - 1) == -1 and s(depth=2, ws_bytes=need[(2, WIDE)] - 1) == -1
    for d in (1, 2, 3):
        assert s(depth=d, form=NARROW, ws_bytes=15) == -1 and s(depth=d, form=AUTO, ws_bytes=15) == -1
    for d, f in ((1, AUTO), (1, NARROW), (2, AUTO), (2, NARROW), (2, WIDE), (3, AUTO), (3, NARROW), (3, WIDE)):
        assert s(n=0, depth=d, form=f) == 0  # a no-op
    torch.cuda.synchronize()
    assert all(is_garbage(t) for t in (*call.outs(), call.ws))  # nothing was enqueued by any of them
    assert np.array_equal(call.boards.cpu().numpy(), R.value_boards())
    # the exact workspace size is accepted, in every form
    for d, f in ((3, WIDE), (2, WIDE), (1, NARROW), (3, NARROW)):
        garbage(*call.outs(), call.ws)
        assert s(depth=d, form=f, ws_bytes=need[(d, f)]) == 0
        torch.cuda.synchronize()
        assert_equal(tuple(t.cpu().numpy() for t in call.outs()), ref("lines-squares-4", d), (d, f))
    assert np.array_equal(call.boards.cpu().numpy(), R.value_boards())  # boards is only read


def test_graph_replay(dev, nets):
    """One captured WIDE depth-3 call on 8 boards, replayed three times with garbage in the outputs and
    in the workspace before every replay: the call zero-fills its workspace itself."""
    pick = [0, 5, 9, 14, 20, 26, 30, 31]
    net = nets("lines-squares-4")
    want = [r[pick] for r in ref("lines-squares-4", 3)]
    assert (want[2] != 0).sum() >= 6
    call = Call(dev, R.value_boards()[pick], 3, WIDE)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.run(net)  # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            L().ntuple_search(net.c, call.boards, 3, call.q, call.leaves, call.legal, call.best, call.ws, WIDE)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        garbage(*call.outs(), call.ws)
        g.replay()
        assert_equal(call.results(), want)


@pytest.mark.parametrize("depth,games,moves", [(2, 8, 40), (3, 4, 12)])
def test_player_exact(dev, depth, games, moves):
    """Philox games under random weights: score for score and board for board the CPU loop."""
    from g2048.ntuple import NTupleNet, NTuplePlayer
    cells, w = R.NETS["lines-squares-4"], net_weights("lines-squares-4")
    player = NTuplePlayer(NTupleNet(cells, dev, torch.from_numpy(np.array(w))), depth=depth)
    res = player.play_games(games, max_moves=moves, game_seed=99)
    scores, mv, boards = SR.cpu_play(cells, w, depth, games, moves, 99)
    assert res["scores"] == scores.tolist() and res["moves"] == mv.tolist()
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
    greedy = R.cpu_play(cells, w, games, moves, 99)
    assert not np.array_equal(greedy[2], boards)  # the search plays other moves than the greedy player
    best, q, legal = player.choose(to_dev(R.value_boards(), dev))
    torch.cuda.synchronize()
    q_ref, _, legal_ref, best_ref = ref("lines-squares-4", depth)
    assert np.array_equal(best.cpu().numpy(), best_ref) and np.array_equal(q.cpu().numpy(), q_ref)
    assert np.array_equal(legal.cpu().numpy(), legal_ref)


def test_command_runs(tmp_path):
    """`play-ntuple MODEL --depth 2` as a user runs it, in a fresh child process; --depth 4 is refused."""
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    from g2048.ntuple import NTupleNet
    cells = R.NETS["lines-squares-4"]
    out = tmp_path / "net.pt"
    NTupleNet(cells, "cpu", torch.from_numpy(R.random_weights(cells, 7, bits=20))).save(out)
    cmd = [sys.executable, str(PKG / "train.py"), "play-ntuple", str(out), "-g", "4", "--max-moves", "20"]
    r = subprocess.run(cmd + ["--depth", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Eval Results - Max: ") and "Avg: " in ln and "Median: " in ln for ln in lines)
    assert any(ln.startswith("Tiles Reached - 512: ") and "2048: " in ln for ln in lines)
    r = subprocess.run(cmd + ["--depth", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode != 0 and "--depth" in r.stdout + r.stderr
