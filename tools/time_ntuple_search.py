"""Time g2048_ntuple_search in its two lane mappings, NARROW and WIDE, at depth 2 and 3 for the presets
`lines-squares-4` (five 256 KiB tables) and `4x6` (a 256 MiB table) on 1 to 8 192 root boards of
tests/golden/games.npz, on one GPU in one process.

The weights are random 20-bit integers drawn on the device: the time of a search depends on which table
entries its boards read, not on what they hold.  Per (net, depth, n, form): a warm-up call sizes a graph
of K back-to-back calls (about `--graph-ms` of work, 1 <= K <= 256); after a warm-up replay the graph is
replayed `--repeats` times with HIP events around each replay, and the median time per call is reported
with the leaf after-states per call (the sum of the `leaves` output) and the leaves per second that
follow from the two.  The two forms must give the same outputs before a time is printed.  The last
column names the form AUTO takes, so that csrc/ntuple_search.hip's rule can be weighed against the
times.  With `--play MODEL` it instead times whole games of NTuplePlayer on a net saved by `train-ntuple`,
at depth 1, 2 and 3 on `play-ntuple`'s seeds: a short warm-up, then `--games` games to their end between
two device synchronisations, host clock.  There is no pass / fail threshold: this is a measuring tool,
and what it printed on an MI355X is recorded in DESIGN.md (N-tuple search).

    python tools/time_ntuple_search.py [--tuples lines-squares-4 4x6 --depths 2 3
                                        --boards 1 32 128 256 1024 8192 --repeats 7 --graph-ms 20]
    python tools/time_ntuple_search.py --play net.pt [--games 100]
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))

from g2048 import _lib as L  # noqa: E402
from g2048.ntuple import PRESETS, NTupleNet, NTuplePlayer  # noqa: E402


def sample_boards(n: int) -> np.ndarray:
    """n boards spread evenly over the recorded games (n = 1: a mid-game board)."""
    before = np.load(ROOT / "tests" / "golden" / "games.npz")["before"]
    if n > len(before):
        raise SystemExit(f"the recorded games hold {len(before)} boards, fewer than {n}")
    step = max(1, len(before) // n)
    return np.ascontiguousarray(before[step // 2::step][:n].astype(np.int8))


class Case:
    def __init__(self, net, boards, depth, form, dev):
        n = boards.shape[0]
        self.net, self.boards, self.depth, self.form = net, boards, depth, form
        self.q = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.leaves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.legal = torch.empty(n, dtype=torch.uint8, device=dev)
        self.best = torch.empty(n, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(L.ntuple_search_workspace_bytes(n, depth, form), dtype=torch.uint8, device=dev)

    def call(self):
        L.ntuple_search(self.net.c, self.boards, self.depth, self.q, self.leaves, self.legal, self.best, self.ws,
                        self.form)

    def outputs(self):
        return self.q.clone(), self.leaves.clone(), self.legal.clone(), self.best.clone()


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def time_case(case: Case, repeats: int, graph_ms: float):
    """-> (median ms per call, calls per graph)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        case.call()  # loads the kernel
        torch.cuda.synchronize()
        one = event_ms(case.call)
        calls = int(min(256, max(1, graph_ms / max(one, 1e-3))))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(calls):
                case.call()
        g.replay()  # warm-up replay
        torch.cuda.synchronize()
        times = [event_ms(g.replay) / calls for _ in range(repeats)]
    torch.cuda.current_stream().wait_stream(side)
    return float(np.median(times)), calls


def auto_name(n: int, depth: int) -> str:
    """The form AUTO resolves to: the one whose workspace size AUTO's equals (WIDE's is the larger)."""
    auto = L.ntuple_search_workspace_bytes(n, depth, L.EMAX_AUTO)
    return "wide" if auto == L.ntuple_search_workspace_bytes(n, depth, L.EMAX_WIDE) else "narrow"


def time_play(path: Path, games: int, dev):
    net = NTupleNet.load(path, dev)
    seeds = list(range(games))
    print(f"{path.name}: {len(net.cells)} tuples of {len(net.cells[0])} cells; {games} games per depth")
    print(f"{'depth':>5} {'mean score':>10} {'2048':>6} {'moves':>8} {'seconds':>8} {'ms/game':>8} {'us/move':>8}")
    for depth in (1, 2, 3):
        player = NTuplePlayer(net, depth)
        player.play_games(games, 32, seeds=seeds)  # loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = player.play_games(games, None, seeds=seeds)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        longest = max(res["moves"])  # the game loop makes one search and one env step per move of the longest game
        print(f"{depth:>5} {sum(res['scores']) / games:>10.1f} {sum(t >= 2048 for t in res['max_tiles']) / games:>6.0%} "
              f"{longest:>8} {dt:>8.3f} {dt / games * 1e3:>8.2f} {dt / longest * 1e6:>8.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--play", type=Path, help="a net saved by train-ntuple: time whole games on it instead")
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--tuples", nargs="+", default=["lines-squares-4", "4x6"], choices=sorted(PRESETS))
    ap.add_argument("--depths", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--boards", type=int, nargs="+", default=[1, 32, 128, 256, 1024, 8192])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--graph-ms", type=float, default=20.0, help="work captured into one graph, about")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_search needs a ROCm device")
    dev = torch.device("cuda", 0)
    if a.play is not None:
        return time_play(a.play, a.games, dev)
    print(f"per call: median of {a.repeats} graph replays")
    print(f"{'net':>15} {'depth':>5} {'boards':>6} {'form':>6} {'calls':>5} {'us/call':>12} {'leaves/call':>12} "
          f"{'leaves/s':>10} {'auto':>6}")
    for tuples in a.tuples:
        cells = PRESETS[tuples]
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randint(-(1 << 19), 1 << 19, (len(cells), 16 ** len(cells[0])), dtype=torch.int32, device=dev,
                          generator=gen)
        net = NTupleNet(tuples, dev, w)
        for depth in a.depths:
            for n in a.boards:
                boards = torch.from_numpy(sample_boards(n)).to(dev)
                rows, outs = [], []
                for name, form in (("narrow", L.EMAX_NARROW), ("wide", L.EMAX_WIDE)):
                    case = Case(net, boards, depth, form, dev)
                    ms, calls = time_case(case, a.repeats, a.graph_ms)
                    leaves = int(case.leaves.sum())
                    outs.append(case.outputs())
                    rows.append((name, calls, ms, leaves))
                if not all(torch.equal(x, y) for x, y in zip(*outs)):
                    raise SystemExit(f"{tuples}, depth {depth}, {n} boards: NARROW and WIDE differ")
                for name, calls, ms, leaves in rows:
                    print(f"{tuples:>15} {depth:>5} {n:>6} {name:>6} {calls:>5} {ms * 1e3:>12.1f} {leaves:>12} "
                          f"{leaves / (ms * 1e-3):>10.3g} {auto_name(n, depth):>6}", flush=True)
        del net, w


if __name__ == "__main__":
    main()
