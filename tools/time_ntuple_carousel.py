"""Time a step of g2048_ntuple_staged_carousel against g2048_ntuple_staged_lambda on one GPU in one process: by
default the net `4x6` with the stages 2048,4096,8192, rule tc, a trace of 3, at 4 096 and 65 536 envs.

Per env count: a plain trainer learns for `--warm-steps` steps from zero weights, so that the timed steps run on
mid-game boards; its state (weights, accumulators, boards, after-states, history) is then the start of every
timed call: before each call it is copied back, outside the timed region, so that every repeat of a call does the
same work and the spread is the run-to-run spread alone.  A call is `--steps` steps, timed with HIP events;
`--repeats` repeats, the two calls alternating; the median, minimum and maximum are reported.  The carousel
starts from an empty pool with next[i] = i mod G.  With G2048_LIB set to another build of the library every call
goes to that build; a build from before the carousel existed runs the lambda rows only: run the two builds
alternately in one session to compare them.  There is no pass / fail threshold: this is a measuring tool, and
what it printed on an MI355X is recorded in DESIGN.md (Carousel restarts).

    [G2048_LIB=old/libg2048.so] python tools/time_ntuple_carousel.py [--envs 4096 65536]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))

from g2048 import _lib as L  # noqa: E402
from g2048.ntuple import PRESETS, NTupleNet, NTupleTrainer  # noqa: E402

KEYS = ("tc", "boards", "after", "hist", "hist_len", "pending", "run_score")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", default="4x6", choices=sorted(PRESETS))
    ap.add_argument("--stages", default="2048,4096,8192")
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--lr-shift", type=int, default=12)
    ap.add_argument("--trace", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_carousel needs a ROCm device")
    if os.environ.get("G2048_LIB"):
        L._lib = L.load(os.environ["G2048_LIB"])  # every wrapper then calls this build
    print("library:", L.load()._name)
    has_carousel = hasattr(L.load(), "g2048_ntuple_staged_carousel")
    dev = torch.device("cuda", 0)
    stages = tuple(int(v) for v in a.stages.split(","))
    rows = []
    for n in a.envs:
        net = NTupleNet(a.tuples, dev, stages=stages)
        tr = NTupleTrainer(net, n, a.lr_shift, seed=1, rule="tc", trace_len=a.trace)
        warm = tr.train(a.warm_steps)
        start = {k: getattr(tr, k).clone() for k in KEYS}
        start_w = net.weights.clone()
        G = net.num_stages
        pool = torch.zeros(G, n, 16, dtype=torch.int8, device=dev)
        valid = torch.zeros(n, 16, dtype=torch.uint8, device=dev)
        nxt = torch.zeros(n, dtype=torch.uint8, device=dev)
        origin = torch.zeros(n, dtype=torch.uint8, device=dev)
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        ws = torch.empty(L.ntuple_carousel_workspace_bytes(n) if has_carousel else L.ntuple_lambda_workspace_bytes(n),
                         dtype=torch.uint8, device=dev)
        rng = L.make_rng(L.RNG_PHILOX, 1, tr.counter)

        def restore():
            net.weights.copy_(start_w)
            for k in KEYS:
                getattr(tr, k).copy_(start[k])
            pool.zero_(), valid.zero_(), origin.zero_(), stats.zero_()
            nxt.copy_(torch.arange(n, device=dev) % G)

        def lam():
            L.ntuple_lambda(net.c, tr.tc, tr.boards, tr.after, tr.hist, tr.hist_len, tr.pending, tr.run_score, a.steps,
                            a.lr_shift, a.trace, 1, rng, stats[:4], ws)

        def car():
            L.ntuple_carousel(net.c, tr.tc, tr.boards, tr.after, tr.hist, tr.hist_len, tr.pending, tr.run_score, a.steps,
                              a.lr_shift, a.trace, 1, rng, pool, valid, nxt, origin, stats, ws)

        calls = {"lambda": lam, "carousel": car} if has_carousel else {"lambda": lam}
        times, last = {k: [] for k in calls}, {}
        for rep in range(a.repeats + 1):  # the first repeat loads the kernels and is dropped
            for name, fn in calls.items():
                restore()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                last[name] = stats.tolist()
        for name, t in times.items():
            rows.append({"envs": n, "call": name, "us_per_step": float(np.median(t)), "min_us": min(t), "max_us": max(t)})
            print(f"{n} envs, {name}: median of {a.repeats} calls of {a.steps} steps {np.median(t):.1f} us per step "
                  f"(min {min(t):.1f}, max {max(t):.1f}); warm-up finished {warm['games']} games; last call's stats {last[name]}",
                  flush=True)
        del tr, net, start, start_w
        torch.cuda.empty_cache()
    print(json.dumps({"library": L.load()._name, "tuples": a.tuples, "stages": a.stages, "rule": "tc", "trace": a.trace,
                      "lr_shift": a.lr_shift, "warm_steps": a.warm_steps, "steps": a.steps, "rows": rows}))


if __name__ == "__main__":
    main()
