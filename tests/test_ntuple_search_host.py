"""CPU-side checks of the n-tuple expectimax search: the level-by-level numpy reference
(tests/ntuple_search_reference.py) against an independent scalar recursion in Python ints written from
the definition in include/g2048_ntuple.h, depth 1 against ntuple_reference.choose, the pinned counts of
what makes the GPU tests' inputs meaningful (see PINNED: chance nodes whose sum is negative and not
divisible, root q values a truncating division would change, roots whose best move changes with the
depth, dead inner boards), and the seams (the header's declarations, the wrappers' refusal of CPU
tensors, NTuplePlayer's argument checks, `play-ntuple --depth`)."""

import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import ntuple_reference as R
import ntuple_search_reference as SR
from conftest import ROOT
from oracle import oracle as O

S = 4096


# ---- the scalar recursion: Python ints, one board at a time, written from the header ----
def _sym_perms():
    """The 8 symmetries of the square as cell permutations p, g(b)[c] = b[p[c]]: 4 quarter turns x an
    optional mirror."""
    perms = []
    for mirror in (False, True):
        for turns in range(4):
            p = []
            for r in range(4):
                for c in range(4):
                    r2, c2 = (r, 3 - c) if mirror else (r, c)
                    for _ in range(turns):
                        r2, c2 = c2, 3 - r2
                    p.append(4 * r2 + c2)
            perms.append(p)
    assert len({tuple(p) for p in perms}) == 8
    return perms


class Scalar:
    """A(s, k), M(b, k) and the root's q of the header for one net; w: lists of Python ints."""

    def __init__(self, cells, weights):
        self.cells = cells
        self.w = [[int(x) for x in row] for row in weights]
        self.perms = _sym_perms()
        self.moves = {}
        self.memo = {}

    def value(self, b):
        v = 0
        for p in self.perms:
            for t, tup in enumerate(self.cells):
                v += self.w[t][sum(min(b[p[c]], 15) << (4 * j) for j, c in enumerate(tup))]
        return v

    def move4(self, b):
        """-> [(after-state, points) or None for an illegal action] of the four actions."""
        if b not in self.moves:
            out, pts, _ = O.move(np.array([b] * 4, np.int8), np.arange(4))
            res = [(tuple(int(x) for x in out[a]), int(pts[a])) for a in range(4)]
            self.moves[b] = [None if s == b else (s, p) for s, p in res]
        return self.moves[b]

    def A(self, s, k):
        """-> (A(s, k), leaves)."""
        if k == 0:
            return self.value(s), 1
        key = (s, k)
        if key not in self.memo:
            empty = [c for c in range(16) if s[c] == 0]
            total = leaves = 0
            for c in empty:
                for tile, weight in ((1, 9), (2, 1)):
                    m, l = self.M(s[:c] + (tile,) + s[c + 1:], k)
                    total += weight * m
                    leaves += l
            self.memo[key] = (total // (10 * len(empty)), leaves)  # Python's //: the floor
        return self.memo[key]

    def M(self, b, k):
        best, leaves = None, 0
        for mv in self.move4(b):
            if mv is not None:
                a, l = self.A(mv[0], k - 1)
                leaves += l
                best = S * mv[1] + a if best is None else max(best, S * mv[1] + a)
        return (0 if best is None else best), leaves

    def root(self, b, d):
        """-> (q [4] with None for an illegal action, leaves [4], best)."""
        q, lv, best = [], [], 0xFF
        for a, mv in enumerate(self.move4(b)):
            if mv is None:
                q.append(None)
                lv.append(0)
                continue
            v, l = self.A(mv[0], d - 1)
            q.append(S * mv[1] + v)
            lv.append(l)
            if best == 0xFF or q[a] > q[best]:
                best = a
        return q, lv, best


def weights_of(net, seed=SR.WEIGHT_SEED):
    return R.random_weights(R.NETS[net], seed, bits=32)


@functools.lru_cache(maxsize=None)
def ref(net, depth, floor=True, seed=SR.WEIGHT_SEED):
    st = {}
    out = SR.search_ref(R.NETS[net], weights_of(net, seed), R.value_boards(), depth, stats=st, floor=floor)
    return out, st


@pytest.mark.parametrize("net,depth", [("t1k1", 1), ("t1k1", 2), ("t1k1", 3), ("lines-squares-4", 1),
                                       ("lines-squares-4", 2)])
def test_reference_matches_scalar_recursion(net, depth):
    boards = R.value_boards()
    live = np.nonzero(O.legal_mask(boards) != 0)[0]
    assert len(live) == 25
    (q, lv, legal, best), _ = ref(net, depth)
    sc = Scalar(R.NETS[net], weights_of(net))
    for i in live:
        sq, slv, sbest = sc.root(tuple(int(x) for x in boards[i]), depth)
        assert [R.I64_MIN if x is None else x for x in sq] == q[i].tolist(), i
        assert slv == lv[i].tolist() and sbest == int(best[i]), i
        assert [x is not None for x in sq] == [bool((legal[i] >> a) & 1) for a in range(4)]


@pytest.mark.parametrize("net", ["lines-squares-4", "t1k1", "t8k3"])
def test_depth_one_is_the_greedy_choice(net):
    (q, lv, legal, best), st = ref(net, 1)
    cq, clegal, cbest, _ = R.choose(R.NETS[net], weights_of(net), R.value_boards())
    assert np.array_equal(q, cq) and np.array_equal(legal, clegal) and np.array_equal(best, cbest)
    assert np.array_equal(lv, (cq != R.I64_MIN).astype(np.int64)) and st["leaves"] == int(lv.sum())
    assert (legal == 0).sum() == 8 and (best[legal == 0] == 0xFF).all() and (q[legal == 0] == R.I64_MIN).all()


# (net, depth): (leaves, dead inner boards, chance nodes with a negative non-divisible sum, root q a
# truncating division changes, live roots whose best move differs from depth 1's)
PINNED = {
    ("lines-squares-4", 2): (3661, 3, 7, 7, 10),
    ("lines-squares-4", 3): (244639, 32, 147, 2, 14),
    ("t8k3", 2): (3661, 3, 31, 31, 15),
    ("t8k3", 3): (244639, 32, 2216, 19, 15),
}


@pytest.mark.parametrize("net,depth", sorted(PINNED))
def test_pinned_counts(net, depth):
    (q, lv, legal, best), st = ref(net, depth)
    (qt, lvt, _, _), _ = ref(net, depth, False)
    live = legal != 0
    trunc_sensitive = int((q != qt).sum())
    differs = int((best[live] != ref(net, 1)[0][3][live]).sum())
    got = (st["leaves"], st["dead"], st["neg_nondiv"], trunc_sensitive, differs)
    print(net, depth, got, "largest leaves of a board", int(lv.sum(1).max()), "largest |sum|", st["max_abs_sum"])
    want = PINNED[(net, depth)]
    assert got == want
    assert int(lv.sum(1).max()) == (424 if depth == 2 else 43232)  # the largest tree of one board
    assert np.array_equal(lv, lvt) and int(lv.sum()) == st["leaves"] and live.sum() == 25
    assert trunc_sensitive >= 1 and differs >= 1 and st["dead"] >= 1
    assert st["max_abs_sum"] < 1 << 46 and (q[q != R.I64_MIN] < 0).any() and (q > 0).any()


@pytest.mark.parametrize("depth", [2, 3])
def test_every_gpu_net_has_truncation_sensitive_roots(depth):
    """Per net of the GPU test, some weight seed it runs has a root q that flooring and truncating tell
    apart and a live root whose best move is not depth 1's.  Seed 7 alone has neither negative sums for
    t1k1 nor, at depth 3, a sensitive root for t2k6: hence their second seed."""
    assert {n for n, _ in SR.GPU_CASES} == set(R.NETS) and all((n, SR.WEIGHT_SEED) in SR.GPU_CASES for n in R.NETS)
    sensitive = {}
    for net, seed in SR.GPU_CASES:
        (q, _, legal, best), st = ref(net, depth, True, seed)
        (qt, _, _, _), _ = ref(net, depth, False, seed)
        assert (best[legal != 0] != ref(net, 1, True, seed)[0][3][legal != 0]).any()
        sensitive[(net, seed)] = int((q != qt).sum())
        assert sensitive[(net, seed)] <= st["neg_nondiv"]
    print(depth, sensitive)
    assert sensitive[("t1k1", 7)] == 0 and (depth == 2 or sensitive[("t2k6", 7)] == 0)
    for net in R.NETS:
        assert max(v for (n, _), v in sensitive.items() if n == net) >= 1, net


def test_ending_board_walks_into_dead_children():
    """R.ENDING has one legal merge; at depth 2 some of its spawns leave a board without a move, worth 0."""
    cells, w = R.NETS["lines-squares-4"], weights_of("lines-squares-4")
    st = {}
    q, lv, legal, best = SR.search_ref(cells, w, np.stack([R.ENDING, R.DEAD]), 2, stats=st)
    assert st["dead"] >= 1 and (legal[0] != 0) and legal[1] == 0 and best[1] == 0xFF and (q[1] == R.I64_MIN).all()
    sc = Scalar(cells, w)
    sq, slv, sbest = sc.root(tuple(int(x) for x in R.ENDING), 2)
    assert [R.I64_MIN if x is None else x for x in sq] == q[0].tolist() and slv == lv[0].tolist()


# ------------------------------------------------------------------------------- the seams -----
def test_header_declares_and_library_exports():
    from g2048 import _lib
    raw = (ROOT / "include" / "g2048_ntuple.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_search_workspace_bytes", "g2048_ntuple_search"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert len(lib.g2048_ntuple_search.argtypes) == 12 and lib.g2048_ntuple_search.restype is ctypes.c_int
    assert lib.g2048_ntuple_search_workspace_bytes.restype is ctypes.c_size_t
    for word in ("floor", "INT64_MIN", "2^46", "Depth 4 is out of scope"):
        assert word in raw, word  # the signed semantics and the bound are specified


def test_workspace_bytes_of_what_is_accepted_and_refused():
    """Host-only: a size for every accepted (n, depth, form), 0 for what the call refuses; AUTO never
    resolves to a refused form."""
    from g2048 import _lib
    wb = _lib.ntuple_search_workspace_bytes
    A, N, W = _lib.EMAX_AUTO, _lib.EMAX_NARROW, _lib.EMAX_WIDE
    for depth in (1, 2, 3):
        assert wb(33, depth, N) > 0 and wb(0, depth, A) > 0 and wb(33, depth, A) > 0
        assert wb(-1, depth, A) == 0 and wb(1 << 31, depth, A) == 0 and wb(33, depth, 3) == 0 and wb(33, depth, -1) == 0
        assert wb((1 << 24) - 1, depth, N) > 0 and wb(1 << 24, depth, N) == 0  # 128 lanes per board
        for n in (1, 100, 191, 192, 200, 1 << 17, (1 << 24) - 1):
            assert wb(n, depth, A) > 0, (n, depth)
    assert wb(33, 0, A) == 0 and wb(33, 4, A) == 0 and wb(33, 1, W) == 0
    for depth in (2, 3):
        assert wb(33, depth, W) >= 33 * (4 * 8 + 4 * 8 + 4 * 4 + 4) and wb(33, depth, W) % 16 == 0
        assert wb((1 << 17) - 1, depth, W) > 0 and wb(1 << 17, depth, W) == 0   # 16 384 lanes per board


def test_cpu_tensors_are_rejected():
    from g2048 import _lib
    n = 4
    net = _lib.NtNet(1, 1, (ctypes.c_int32 * 48)(5), 0x1000)  # never dereferenced: refused before
    b = torch.zeros(n, 16, dtype=torch.int8)
    q = torch.zeros(n, 4, dtype=torch.int64)
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_search(net, b, 2, q, q.clone(), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8),
                           torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_search(net, b, 2, None, workspace=torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(_lib.G2048Error):
        _lib.ntuple_search(net, b, 2, q)  # no workspace


def test_player_argument_checks():
    from g2048.ntuple import NTupleNet, NTuplePlayer
    net = NTupleNet("lines-squares-4", "cpu")
    p = NTuplePlayer(net)
    assert (p.depth, p.form, p.device) == (1, "auto", torch.device("cpu"))
    for depth, form in ((1, "narrow"), (2, "auto"), (2, "wide"), (3, "narrow"), (3, "wide")):
        p = NTuplePlayer(net, depth, form)
        assert (p.depth, p.form) == (depth, form)
    assert NTuplePlayer(net, depth=3).depth == 3
    for kw in ({"depth": 0}, {"depth": 4}, {"depth": -1}, {"form": "deep"}, {"form": "wide"}, {"depth": 1, "form": "wide"}):
        with pytest.raises(ValueError):
            NTuplePlayer(net, **kw)
    with pytest.raises(ValueError):
        NTuplePlayer("lines-squares-4", depth=2)


def test_play_ntuple_lists_depth():
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["play-ntuple", "--help"])
    assert r.exit_code == 0, r.output
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    for opt in ("MODEL", "--games", "-g", "--max-moves", "--depth"):
        assert opt in out, opt
    assert "1..3" in re.sub(r"[\s│]+", " ", out)
    r = CliRunner().invoke(train.app, ["play-ntuple", "no-such-net.pt", "--depth", "4"])
    assert r.exit_code != 0 and "--depth" in r.output
