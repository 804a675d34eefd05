"""Time g2048_mc_search against the composition of the older public entry points that computes the
same sums, at the evaluation shape (1024 root boards of tests/golden/games.npz, P = 64 playouts per
action, depth D = 64), on one GPU:

  new       one g2048_mc_search call (score_sum, move_sum, legal, best)
  composed  the boards replicated 4 P times, one g2048_env_step with the forced actions,
            g2048_env_rollout_random for D steps into its five trajectory arrays, and a torch
            reduction truncated at each lane's first DONE flag (`composed_sums`, also what
            tests/test_gpu_mc_search.py checks the kernel against on the device)

The two alternate in one process, five timed repeats each after a warm-up of both, HIP events around
`--calls` back-to-back calls per repeat.  The sums of the two must agree bit for bit before any
time is reported.

    python tools/time_mc_search.py [--roots 1024 --playouts 64 --depth 64 --repeats 5]
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


class Composed:
    """The buffers of `composed_sums` for one shape (allocated once, like a caller's would be)."""

    def __init__(self, n, P, D, dev):
        N = n * 4 * P
        self.n, self.P, self.D = n, P, D
        self.acts = torch.arange(4, dtype=torch.uint8, device=dev).repeat_interleave(P).repeat(n)
        self.rep = torch.empty(N, 16, dtype=torch.int8, device=dev)
        self.pts0 = torch.empty(N, dtype=torch.int32, device=dev)
        self.fl0 = torch.empty(N, dtype=torch.uint8, device=dev)
        T = max(D, 1)
        self.tb = torch.empty(T, N, 16, dtype=torch.int8, device=dev)
        self.ta = torch.empty(T, N, dtype=torch.uint8, device=dev)
        self.tp = torch.empty(T, N, dtype=torch.int32, device=dev)
        self.tpot = torch.empty(T, N, 4, dtype=torch.int8, device=dev)
        self.tf = torch.empty(T, N, dtype=torch.uint8, device=dev)
        self.steps = torch.arange(T, device=dev)[:, None]


def composed_sums(boards, P, D, seed, ctr, env_base=0, bufs: Composed | None = None):
    """(score_sum, move_sum) int64 [n, 4] of g2048_mc_search from g2048_env_step +
    g2048_env_rollout_random + torch."""
    n = boards.shape[0]
    c = bufs or Composed(n, P, D, boards.device)
    c.rep.view(n, 4 * P, 16).copy_(boards[:, None, :])
    rng = L.make_rng(L.RNG_PHILOX, seed, ctr, env_base)
    L.env_step(c.rep, c.rep, c.acts, None, c.pts0, None, None, c.fl0, rng)
    invalid = (c.fl0 & L.FLAG_INVALID) != 0
    alive = ((c.fl0 & L.FLAG_LEGAL) != 0) & ~invalid
    pts = c.pts0.to(torch.int64)
    moves = torch.zeros_like(pts)
    if D > 0:
        L.env_rollout_random(c.rep, D, c.tb, c.ta, c.tp, c.tpot, c.tf, rng)
        done = (c.tf & L.FLAG_DONE) != 0
        first = torch.where(done.any(0), done.to(torch.uint8).argmax(0), D - 1)
        m = (c.steps <= first[None, :]) & alive[None, :]
        pts = pts + (c.tp * m).sum(0)
        moves = m.sum(0)
    pts = torch.where(invalid, 0, pts)
    return pts.view(n, 4, P).sum(2), moves.view(n, 4, P).sum(2)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000, help="back-to-back calls per timed repeat")
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--counter", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mc_search needs a ROCm device")
    dev = torch.device("cuda", 0)
    before = np.load(ROOT / "tests" / "golden" / "games.npz")["before"]
    roots = before[::max(1, len(before) // a.roots)][:a.roots]
    boards = torch.from_numpy(np.ascontiguousarray(roots)).to(dev)
    n, P, D = boards.shape[0], a.playouts, a.depth
    score = torch.empty(n, 4, dtype=torch.int64, device=dev)
    moves = torch.empty(n, 4, dtype=torch.int64, device=dev)
    legal = torch.empty(n, dtype=torch.uint8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.mc_search_workspace_bytes(n, P), dtype=torch.uint8, device=dev)
    rng = L.make_rng(L.RNG_PHILOX, a.seed, a.counter, 0)
    bufs = Composed(n, P, D, dev)

    def new():
        L.mc_search(boards, P, D, rng, score, moves, legal, best, ws)

    def composed():
        return composed_sums(boards, P, D, a.seed, a.counter, 0, bufs)

    for _ in range(2):  # warm-up of both, and the agreement the comparison rests on
        new()
        cs, cm = composed()
    torch.cuda.synchronize()
    if not (torch.equal(cs, score) and torch.equal(cm, moves)):
        raise SystemExit("the composed sums differ from g2048_mc_search's")
    executed = int(moves.sum())
    print(f"shape: {n} roots, P = {P}, D = {D}: {n * 4 * P} lanes, {executed} playout steps executed, sums agree")
    t_new, t_comp = [], []
    for r in range(a.repeats):
        t_new.append(timed(new, a.calls))
        t_comp.append(timed(composed, max(1, a.calls // 5)))
        print(f"repeat {r}: new {t_new[-1]:.4f} ms/call   composed {t_comp[-1]:.4f} ms/call")
    mn, mc = float(np.median(t_new)), float(np.median(t_comp))
    print(f"median: new {mn:.4f} ms, composed {mc:.4f} ms, composed / new = {mc / mn:.2f}")
    print(f"executed playout steps/s (new, median): {executed / (mn * 1e-3):.4g}")


if __name__ == "__main__":
    main()
