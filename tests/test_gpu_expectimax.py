"""g2048_expectimax (csrc/expectimax.hip) and g2048/search.py's ExpectimaxPlayer on the GPU, bit for bit
against the level-by-level numpy reference of tests/expectimax_reference.py: every output is an integer
and no result depends on a summation order, so both lane mappings (NARROW, WIDE) must give the same
bytes as the CPU.

The 30 root boards (mc_reference.roots) hold eight finished boards, a live board without an empty cell
(root 9), boards with 14 empty cells (the full fan-out) and live boards with illegal actions; the
depth-2 and depth-3 trees hold boards below the roots without a legal move, and at depth 1 the two
top values tie on 14 roots (tests/test_expectimax_host.py pins the counts).  Each test asserts on the
reference that the cases it claims to cover occur.  `leaves` must equal the reference's counts, which
proves that the whole tree was walked.
"""

import functools

import numpy as np
import pytest
import torch

from conftest import golden
from expectimax_reference import CROWDED, WEIGHTS, cpu_play, expectimax_ref, legal_best
from mc_reference import roots
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
WEIGHT_SETS = [WEIGHTS, (1, 0, 0), (0, 4096, 4096)]
FORMS = ("narrow", "wide", "auto")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def form_id(form):
    return {"auto": L().EMAX_AUTO, "narrow": L().EMAX_NARROW, "wide": L().EMAX_WIDE}[form]


@functools.lru_cache(maxsize=None)
def ref_roots(depth, weights, crowded=False):
    """-> (value, leaves, legal, best, stats) of the reference on the roots (read-only, shared)."""
    boards = roots()[CROWDED] if crowded else roots()
    st = {}
    val, lv = expectimax_ref(boards, depth, weights, st)
    legal, best = legal_best(boards, val)
    for a in (val, lv, legal, best):
        a.setflags(write=False)
    return val, lv, legal, best, st


def ref_of(boards, depth, weights=WEIGHTS):
    val, lv = expectimax_ref(boards, depth, weights)
    return (val, lv) + legal_best(boards, val)


class Search:
    """Device buffers of one search shape, filled with garbage before every call: the call itself
    zero-fills what it accumulates into."""

    def __init__(self, dev, boards, depth, weights=WEIGHTS, form="narrow"):
        n = len(boards)
        self.b = torch.from_numpy(np.ascontiguousarray(boards)).to(dev)
        self.depth, self.weights, self.form = depth, weights, form_id(form)
        self.value = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.leaves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.legal = torch.empty(n, dtype=torch.uint8, device=dev)
        self.best = torch.empty(n, dtype=torch.uint8, device=dev)
        nbytes = L().expectimax_workspace_bytes(n, depth, self.form)
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def outputs(self):
        return self.value, self.leaves, self.legal, self.best

    def garbage(self):
        for t in self.outputs() + (self.ws,):
            t.view(torch.uint8).fill_(GARBAGE)

    def call(self):
        L().expectimax(self.b, self.depth, self.weights, self.value, self.leaves, self.legal, self.best, self.ws,
                       self.form)

    def run(self):
        self.garbage()
        self.call()
        return self.results()

    def results(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in self.outputs())


def assert_equal(got, ref):
    for g, r, name in zip(got, ref, ("value", "leaves", "legal", "best")):
        assert np.array_equal(g, r), name


BIT_EXACT = [(d, f) for d in (1, 2, 3) for f in ("narrow", "wide") if not (f == "wide" and d < 2)]


@pytest.mark.parametrize("weights", WEIGHT_SETS)
@pytest.mark.parametrize("depth,form", BIT_EXACT)
def test_bit_exact(dev, depth, form, weights):
    val, lv, legal, best, st = ref_roots(depth, weights)
    finished = legal == 0
    assert finished.sum() == 8 and (best[finished] == 0xFF).all()   # finished roots
    assert ((legal != 0) & (legal != 15)).any()                      # illegal actions of live roots
    assert int(lv.sum()) == st["leaves"] and (lv[val < 0] == 0).all()
    if depth >= 2:
        assert st["dead"] > st["dead_roots"]                         # boards below the roots without a move
    if depth == 1 and weights == WEIGHTS:
        s = np.sort(val, 1)
        tie = (s[:, 3] >= 0) & (s[:, 3] == s[:, 2])
        assert tie.sum() == 14                                       # the lowest index among equals
        assert (best[tie] == val[tie].argmax(1)).all()
    assert_equal(Search(dev, roots(), depth, weights, form).run(), (val, lv, legal, best))


@pytest.mark.parametrize("form", ["narrow", "wide"])
def test_depth_4_on_the_crowded_roots(dev, form):
    val, lv, legal, best, st = ref_roots(4, WEIGHTS, crowded=True)
    assert st["leaves"] == 277923 and st["dead"] == 224 and st["dead_roots"] == 0
    assert (legal != 15).any()
    assert_equal(Search(dev, roots()[CROWDED], 4, WEIGHTS, form).run(), (val, lv, legal, best))


def test_forms_agree(dev):
    """512 boards at depth 2: NARROW, WIDE and AUTO give identical bytes (and the reference's)."""
    boards = golden("mlp196.npz")["boards"]
    got = [Search(dev, boards, 2, WEIGHTS, form).run() for form in FORMS]
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert x.tobytes() == y.tobytes()
    assert_equal(got[0], ref_of(boards, 2))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 3])
def test_small_shapes(dev, n, form):
    """n = 1 and n = 3 (a wave half-filled) at depth 3, where AUTO takes WIDE; root 26 has an illegal action."""
    boards = roots()[[5, 26, 0][:n]]
    assert_equal(Search(dev, boards, 3, WEIGHTS, form).run(), ref_of(boards, 3))


def test_nullable_outputs(dev):
    """leaves / legal / best are optional in both forms; value is what it is with them."""
    boards = roots()
    for form, depth in (("narrow", 1), ("narrow", 2), ("wide", 2)):
        s = Search(dev, boards, depth, WEIGHTS, form)
        s.garbage()
        L().expectimax(s.b, depth, WEIGHTS, s.value, None, None, None, s.ws, s.form)
        torch.cuda.synchronize()
        assert np.array_equal(s.value.cpu().numpy(), ref_roots(depth, WEIGHTS)[0])
        for t in (s.leaves, s.legal, s.best):
            assert bool((t.view(torch.uint8) == GARBAGE).all())


@pytest.mark.parametrize("form", ["narrow", "wide"])
def test_graph_replay(dev, form):
    """One captured call replayed twice over re-garbaged outputs and workspace, the board tensor
    overwritten in place between the replays: each replay equals the eager results for its boards."""
    first, second = roots(), np.ascontiguousarray(roots()[::-1])
    s = Search(dev, first, 2, WEIGHTS, form)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.call()  # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.call()
    torch.cuda.current_stream().wait_stream(side)
    for boards in (first, second):
        s.b.copy_(torch.from_numpy(boards))
        s.garbage()
        g.replay()
        got = s.results()
        eager = Search(dev, boards, 2, WEIGHTS, form).run()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, eager))
        assert_equal(got, ref_of(boards, 2))


def test_einval_and_empty(dev):
    lib = L()
    n0 = len(roots())
    s = Search(dev, roots(), 2, WEIGHTS, "wide")  # the WIDE workspace covers every call below
    N, W = lib.EMAX_NARROW, lib.EMAX_WIDE

    def status(n=n0, depth=2, w=WEIGHTS, form=N, boards=s.b.data_ptr(), value=s.value.data_ptr(),
               leaves=s.leaves.data_ptr(), ws=s.ws.data_ptr(), ws_bytes=s.ws.numel()):
        """The raw status of the C call (the wrapper would raise)."""
        return lib.load().g2048_expectimax(lib._stream(s.b), boards, n, depth, w[0], w[1], w[2], form, value, leaves,
                                           s.legal.data_ptr(), s.best.data_ptr(), ws, ws_bytes)

    s.garbage()
    for depth in (0, 5, -1):
        assert status(depth=depth) == -1
    for k in range(3):
        for bad in (-1, 4097):
            w = list(WEIGHTS)
            w[k] = bad
            assert status(w=w) == -1
    for form in (3, -1):
        assert status(form=form) == -1
    assert status(depth=1, form=W) == -1
    assert status(n=-1) == -1
    assert status(n=1 << 24, form=N) == -1   # 128 n = 2^31 lanes
    assert status(n=1 << 17, form=W) == -1   # 16 384 n = 2^31 lanes
    assert status(n=1 << 40) == -1
    for null in ("boards", "value", "ws"):
        assert status(**{null: None}) == -1
    for name, t in (("boards", s.b), ("value", s.value), ("leaves", s.leaves), ("ws", s.ws)):
        assert status(**{name: t.data_ptr() + 8}) == -1
    need = lib.expectimax_workspace_bytes(n0, 2, W)
    assert need == s.ws.numel() and status(form=W, ws_bytes=need - 1) == -1
    assert status(form=N, ws_bytes=lib.expectimax_workspace_bytes(n0, 2, N) - 1) == -1
    assert status(n=0) == 0 and status(n=0, form=W) == 0  # a no-op
    torch.cuda.synchronize()
    for t in s.outputs() + (s.ws,):  # nothing was enqueued by any of them
        assert bool((t.view(torch.uint8) == GARBAGE).all())
    w = (4096, 4096, 4096)  # the largest weights and depth are accepted
    crowded = s.b[CROWDED].contiguous()
    assert status(n=len(CROWDED), depth=4, w=w, form=W, boards=crowded.data_ptr()) == 0
    torch.cuda.synchronize()
    val, lv = expectimax_ref(roots()[CROWDED], 4, w)
    assert np.array_equal(s.value[:len(CROWDED)].cpu().numpy(), val)
    assert np.array_equal(s.leaves[:len(CROWDED)].cpu().numpy(), lv)


@pytest.fixture(scope="module")
def player2(dev):
    from g2048.search import ExpectimaxPlayer
    return ExpectimaxPlayer(2, WEIGHTS, dev)


def test_player_exact(player2):
    """8 Philox games of 60 moves: score for score and board for board the CPU loop."""
    res = player2.play_games(8, max_moves=60, game_seed=99)
    scores, moves, boards = cpu_play(8, 2, 60, 99)
    assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist()
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
    assert res["max_tiles"] == [1 << int(e) for e in boards.max(1)]


def test_player_choose(dev):
    from g2048.search import ExpectimaxPlayer
    for form in ("auto", "wide"):
        best, value, leaves, legal = ExpectimaxPlayer(3, WEIGHTS, dev, form).choose(torch.from_numpy(roots()).to(dev))
        torch.cuda.synchronize()
        assert_equal(tuple(t.cpu().numpy() for t in (value, leaves, legal, best)), ref_roots(3, WEIGHTS)[:4])


def test_player_quality(player2, dev):
    """Deterministic, because the player is exact: 16 Philox games at depth 2 are the CPU loop's, all
    alive at move 150, with a mean score (1540.75 on the CPU) above the mean final score of 16
    uniform-random games played to the end on the same game seed (878.5 on the CPU)."""
    from g2048.env import VecEnv
    lib = L()
    res = player2.play_games(16, max_moves=150, game_seed=99)
    scores, moves, boards = cpu_play(16, 2, 150, 99)
    assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist() == [150] * 16
    assert np.array_equal(res["boards"].cpu().numpy(), boards)
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
    print("expectimax mean", np.mean(res["scores"]), "uniform-random mean", float(total.double().mean()))
    assert np.mean(res["scores"]) > float(total.double().mean())


def test_player_mt_games_and_forms(dev):
    """MT19937-parity games run, and the form does not change a game."""
    from g2048.search import ExpectimaxPlayer
    a = ExpectimaxPlayer(2, WEIGHTS, dev, "narrow").play_games(4, max_moves=20, seeds=[0, 1, 2, 3])
    b = ExpectimaxPlayer(2, WEIGHTS, dev, "wide").play_games(4, max_moves=20, seeds=[0, 1, 2, 3])
    assert a["moves"] == [20] * 4 and a["scores"] == b["scores"] and torch.equal(a["boards"], b["boards"])
