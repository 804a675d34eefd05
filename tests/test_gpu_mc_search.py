"""g2048_mc_search (csrc/mc_search.hip) and g2048/search.py's MonteCarloPlayer on the GPU, bit for bit
against the CPU composition of oracle functions in tests/mc_reference.py: every output is an integer.

The 30 root boards (mc_reference.roots) hold mid-game boards, finished boards (no legal move) and
boards of the best game up to 2^11 (the SWAR path beside the table path).  Checked on the CPU for
P = 16 at counter 7: 44 of the 120 (board, action) pairs are illegal, and 24 % / 47 % / 99.9 % of the
live playouts end before D = 16 / 64 / 256, so the early stop, the depth cap, illegal roots and
finished roots all occur; test_bit_exact asserts each kind on the reference it compares with.
"""

import ctypes
import functools
import importlib.util

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from mc_reference import cpu_play, legal_best, mc_ref, mc_ref_lanes, roots
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x2048
GARBAGE = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def ref_lanes(P, D, ctr, env_base):
    return mc_ref_lanes(roots(), P, D, SEED, ctr, env_base)


def ref_roots(P, D, ctr, env_base):
    pts, moves, invalid, _ = ref_lanes(P, D, ctr, env_base)
    n = len(roots())
    return pts.reshape(n, 4, P).sum(2), moves.reshape(n, 4, P).sum(2), invalid.reshape(n, 4, P)[:, :, 0]


class Search:
    """Device buffers of one search shape, filled with garbage before every call: the call itself
    zero-fills what it accumulates into."""

    def __init__(self, dev, boards, P, D):
        n = len(boards)
        self.b = torch.from_numpy(np.ascontiguousarray(boards)).to(dev)
        self.P, self.D = P, D
        self.score = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.moves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.legal = torch.empty(n, dtype=torch.uint8, device=dev)
        self.best = torch.empty(n, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(L().mc_search_workspace_bytes(n, P), dtype=torch.uint8, device=dev)

    def garbage(self):
        for t in (self.score, self.moves, self.legal, self.best, self.ws):
            t.view(torch.uint8).fill_(GARBAGE)

    def call(self, rng):
        L().mc_search(self.b, self.P, self.D, rng, self.score, self.moves, self.legal, self.best, self.ws)

    def run(self, ctr, env_base=0):
        self.garbage()
        self.call(L().make_rng(L().RNG_PHILOX, SEED, ctr, env_base))
        return self.results()

    def results(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.score, self.moves, self.legal, self.best))


def assert_equal(got, ref):
    sc, mv, inv = ref
    legal, best = legal_best(sc, inv)
    assert np.array_equal(got[0], sc), "score_sum"
    assert np.array_equal(got[1], mv), "move_sum"
    assert np.array_equal(got[2], legal), "legal"
    assert np.array_equal(got[3], best), "best"


CASES = [(1, 1, 0), (5, 16, 7), (16, 32, 6), (64, 64, 3), (96, 256, 1), (16, 0, 4)]


@pytest.mark.parametrize("env_base", [0, 1000])
@pytest.mark.parametrize("P,D,ctr", CASES)
def test_bit_exact(dev, P, D, ctr, env_base):
    ref = ref_roots(P, D, ctr, env_base)
    _, moves, invalid, alive = ref_lanes(P, D, ctr, env_base)
    finished = np.repeat(O.legal_mask(roots()) == 0, 4 * P)
    assert finished.any() and (invalid & ~finished).any()  # finished roots, illegal moves of live roots
    if (P, D) in ((5, 16), (16, 32), (64, 64)):
        assert (alive & (moves < D)).any()  # playouts that stop early ...
        assert (moves == D).any()           # ... and playouts that run to the depth cap
    assert_equal(Search(dev, roots(), P, D).run(ctr, env_base), ref)


def test_more_lanes_than_one_grid_pass(dev):
    """524 288 lanes: every persistent workgroup takes a second batch of lanes."""
    boards = golden("mlp196.npz")["boards"]
    assert_equal(Search(dev, boards, 256, 4).run(9), mc_ref(boards, 256, 4, SEED, 9))


@pytest.mark.parametrize("n,P", [(3, 5), (1, 1)])
def test_small_groups(dev, n, P):
    """P = 5: a wave spans several (board, action) groups; n = P = 1: four lanes in all."""
    boards = roots()[[0, 26, 5][:n]]
    for ctr in (4, 5):
        assert_equal(Search(dev, boards, P, 16).run(ctr, 3), mc_ref(boards, P, 16, SEED, ctr, 3))


def boundary_roots(m):
    """8 boards of maximum exactly m with two adjacent m's (test_gpu_env_carry.test_table_boundary's)."""
    rng = np.random.default_rng(200 + m)
    b = rng.integers(1, m, size=(8, 16)).astype(np.int8)
    b[rng.random(b.shape) < 0.25] = 0
    pos = np.random.default_rng(m).integers(0, 3, 8)
    for i in range(8):
        if i % 2 == 0:  # a horizontal pair in row i % 4
            r, c = i % 4, pos[i]
            b[i, 4 * r + c] = b[i, 4 * r + c + 1] = m
        else:  # a vertical pair in column i % 4
            c, r = i % 4, pos[i]
            b[i, 4 * r + c] = b[i, 4 * r + 4 + c] = m
    assert (b.max(axis=1) == m).all()
    return b


@pytest.mark.parametrize("ctr", [4, 5])
@pytest.mark.parametrize("m", [8, 9, 10])
def test_table_boundary(dev, m, ctr):
    """Playouts that create m + 1 while they run -- past the fast-pair bound (9: the wave leaves the
    fast pair), at the top table digit (10) and outside the table (11: the SWAR path) -- in waves
    (P = 64: one per (board, action)) where other lanes never do: the playout step's own carry of the
    maximum decides each lane's path."""
    P, D, env_base = 64, 8, 7
    boards = boundary_roots(m)
    pts, moves, invalid, _, mx = mc_ref_lanes(boards, P, D, SEED, ctr, env_base, stepped_max=True)
    grew = (mx == m + 1).any(axis=0).reshape(-1, 64)  # per wave and lane: it steps a board holding m + 1
    played = (mx >= 0).any(axis=0).reshape(-1, 64)
    assert grew.any()
    assert (grew.any(axis=1) & (played & ~grew).any(axis=1)).any()  # a wave of both kinds of lane
    ref = pts.reshape(8, 4, P).sum(2), moves.reshape(8, 4, P).sum(2), invalid.reshape(8, 4, P)[:, :, 0]
    assert_equal(Search(dev, boards, P, D).run(ctr, env_base), ref)


def test_same_sums_from_existing_kernels(dev):
    """The device's own g2048_env_step + g2048_env_rollout_random + a torch reduction
    (tools/time_mc_search.py composed_sums) give the kernel's sums."""
    spec = importlib.util.spec_from_file_location("time_mc_search", ROOT / "tools" / "time_mc_search.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    s = Search(dev, roots(), 16, 32)
    got = s.run(6, 1000)
    cs, cm = tool.composed_sums(s.b, 16, 32, SEED, 6, 1000)
    assert np.array_equal(cs.cpu().numpy(), got[0]) and np.array_equal(cm.cpu().numpy(), got[1])
    assert got[1].sum() > 0


def test_graph_replay(dev):
    """One captured call with a device counter, replayed at two counters over garbage-filled outputs."""
    P, D, c0 = 16, 32, 6
    s = Search(dev, roots(), P, D)
    ctr = torch.full((1,), c0, dtype=torch.int64, device=dev)
    rng = L().make_rng(L().RNG_PHILOX, SEED, 0, 0, counter_dev=ctr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.call(rng)  # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.call(rng)
    torch.cuda.current_stream().wait_stream(side)
    for c in (c0, c0 + D):
        ctr.fill_(c)
        s.garbage()
        g.replay()
        got = s.results()
        assert_equal(got, ref_roots(P, D, c, 0))
        eager = Search(dev, roots(), P, D).run(c, 0)
        assert all(np.array_equal(x, y) for x, y in zip(got, eager))


def test_einval_and_empty(dev):
    lib = L()
    s = Search(dev, roots(), 4, 4)

    def status(P=4, D=4, rng=None, ws=s.ws, n=len(roots())):
        """The raw status of the C call (the wrapper would raise)."""
        rng = rng or lib.make_rng(lib.RNG_PHILOX, SEED, 0, 0)
        return lib.load().g2048_mc_search(lib._stream(s.b), s.b.data_ptr(), n, P, D, ctypes.byref(rng),
                                          s.score.data_ptr(), s.moves.data_ptr(), s.legal.data_ptr(),
                                          s.best.data_ptr(), ws.data_ptr(), ws.numel())

    s.garbage()
    mt = torch.zeros(625 * 30, dtype=torch.int32, device=dev)
    assert status(rng=lib.make_rng(lib.RNG_MT19937, 1, 0, 0, mt_state=mt)) == -1
    assert status(rng=lib.make_rng(lib.RNG_INJECT, 1, 0, 0)) == -1
    for P in (0, -1, 4097):
        assert status(P=P) == -1
    for D in (-1, 65537):
        assert status(D=D) == -1
    assert status(n=(1 << 31) // 16) == -1  # n x 4 x P == 2^31
    assert status(n=1 << 40) == -1
    assert status(ws=s.ws[:lib.mc_search_workspace_bytes(30, 4) - 1]) == -1
    assert status(n=0) == 0  # a no-op
    torch.cuda.synchronize()
    for t in (s.score, s.moves, s.legal, s.best):  # nothing was enqueued by any of them
        assert bool((t.view(torch.uint8) == GARBAGE).all())
    assert status(P=4096, D=65536, n=1) == 0  # the largest playout count and depth are accepted
    torch.cuda.synchronize()
    assert int(s.legal[0]) == int(O.legal_mask(roots()[:1])[0]) and int(s.moves[0].sum()) > 4096 * 65


@pytest.fixture(scope="module")
def player16(dev):
    from g2048.search import MonteCarloPlayer
    return MonteCarloPlayer(16, 32, dev)


def test_player_exact(player16):
    """8 Philox games of 60 moves: score for score and board for board the CPU loop."""
    res = player16.play_games(8, max_moves=60, game_seed=99)
    scores, moves, boards = cpu_play(8, 16, 32, 60, 99)
    assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist()
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
    assert res["max_tiles"] == [1 << int(e) for e in boards.max(1)]


def test_player_choose(player16, dev):
    best, sc, mv, legal = player16.choose(torch.from_numpy(roots()).to(dev), 3)
    torch.cuda.synchronize()
    assert_equal(tuple(t.cpu().numpy() for t in (sc, mv, legal, best)), ref_roots(16, 32, 3 * 32, 0))


def test_player_quality(player16, dev):
    """16 searched games are all alive at move 150 with a mean score above the mean final score of 16
    uniform-random games played to the end on the same game seed."""
    from g2048.env import VecEnv
    lib = L()
    res = player16.play_games(16, max_moves=150, game_seed=99)
    assert res["moves"] == [150] * 16
    assert bool((O.legal_mask(res["boards"].cpu().numpy()) != 0).all())
    env = VecEnv(16, dev, rng="philox", seed=99)
    env.reset()
    total = torch.zeros(16, dtype=torch.int64, device=dev)
    for chunk in range(400):
        for _ in range(16):
            total += env.step(None, skip_done=True).points
        if bool(((env.flags & lib.FLAG_LEGAL) == 0).all()):
            break
    else:
        pytest.fail("uniform-random games did not end")
    assert np.mean(res["scores"]) > float(total.double().mean())


def test_player_deterministic(player16):
    a = player16.play_games(6, max_moves=40, game_seed=7)
    b = player16.play_games(6, max_moves=40, game_seed=7)
    assert a["scores"] == b["scores"] and a["moves"] == b["moves"] and a["max_tiles"] == b["max_tiles"]
    assert torch.equal(a["boards"], b["boards"])
    mt = player16.play_games(4, max_moves=20, seeds=[0, 1, 2, 3])
    assert len(mt["scores"]) == 4 and all(m == 20 for m in mt["moves"])
