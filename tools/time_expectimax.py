"""Time g2048_expectimax in its two lane mappings, NARROW and WIDE, at depth 2, 3 and 4 for 1, 16 and
1024 root boards of tests/golden/games.npz, on one GPU in one process.

Per (form, depth, n): a warm-up call sizes a graph of K back-to-back calls (about `--graph-ms` of work,
1 <= K <= 256); after a warm-up replay the graph is replayed `--repeats` times with HIP events around
each replay, and the median time per call is reported with the leaf after-states per call (the sum of
the `leaves` output) and the leaves per second that follow from the two.  The two forms must give the
same values and leaf counts before a time is printed.  There is no pass / fail threshold: this is a
measuring tool, and what it printed on an MI355X is recorded in DESIGN.md (Expectimax), where the AUTO
rule of csrc/expectimax.hip is weighed against it.

    python tools/time_expectimax.py [--depths 2 3 4 --boards 1 16 1024 --repeats 7 --graph-ms 20]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))

from g2048 import _lib as L  # noqa: E402

WEIGHTS = (1, 64, 128)


def sample_boards(n: int) -> np.ndarray:
    """n boards spread evenly over the recorded games (n = 1: a mid-game board)."""
    before = np.load(ROOT / "tests" / "golden" / "games.npz")["before"]
    pool = before[::max(1, len(before) // 1024)][:1024]
    step = max(1, len(pool) // n)
    return np.ascontiguousarray(pool[step // 2::step][:n].astype(np.int8))


class Case:
    def __init__(self, boards, depth, form, dev):
        n = boards.shape[0]
        self.boards, self.depth, self.form = boards, depth, form
        self.value = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.leaves = torch.empty(n, 4, dtype=torch.int64, device=dev)
        self.legal = torch.empty(n, dtype=torch.uint8, device=dev)
        self.best = torch.empty(n, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(L.expectimax_workspace_bytes(n, depth, form), dtype=torch.uint8, device=dev)

    def call(self):
        L.expectimax(self.boards, self.depth, WEIGHTS, self.value, self.leaves, self.legal, self.best, self.ws,
                     self.form)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--boards", type=int, nargs="+", default=[1, 16, 1024])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--graph-ms", type=float, default=20.0, help="work captured into one graph, about")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_expectimax needs a ROCm device")
    dev = torch.device("cuda", 0)
    print(f"weights {WEIGHTS}; per call: median of {a.repeats} graph replays")
    print(f"{'depth':>5} {'boards':>6} {'form':>6} {'calls':>5} {'us/call':>12} {'leaves/call':>12} {'leaves/s':>10}")
    for depth in a.depths:
        for n in a.boards:
            boards = torch.from_numpy(sample_boards(n)).to(dev)
            rows, outs = [], []
            for name, form in (("narrow", L.EMAX_NARROW), ("wide", L.EMAX_WIDE)):
                case = Case(boards, depth, form, dev)
                ms, calls = time_case(case, a.repeats, a.graph_ms)
                leaves = int(case.leaves.sum())
                outs.append((case.value.clone(), case.leaves.clone(), case.legal.clone(), case.best.clone()))
                rows.append((name, calls, ms, leaves))
            if not all(torch.equal(x, y) for x, y in zip(*outs)):
                raise SystemExit(f"depth {depth}, {n} boards: NARROW and WIDE differ")
            for name, calls, ms, leaves in rows:
                print(f"{depth:>5} {boards.shape[0]:>6} {name:>6} {calls:>5} {ms * 1e3:>12.1f} {leaves:>12} "
                      f"{leaves / (ms * 1e-3):>10.3g}", flush=True)


if __name__ == "__main__":
    main()
