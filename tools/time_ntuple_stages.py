"""Time the n-tuple trainer's step on one-stage and multi-stage nets, and g2048_ntuple_promote, on one GPU in
one process: by default `train-ntuple`'s default net (`lines-squares-4`) at 65 536 envs, rules td and tc, the
stage lists none, 2048,4096,8192 (nearly every env stays in stage 0) and 16,64,128 (the envs spread over
the four stages).

Per (rule, stage list): a fresh trainer learns for `--warm-steps` steps from zero weights, so that the timed
steps run on mid-game boards; then `--repeats` calls of `--steps` steps are timed with HIP events, each
continuing the games of the one before; the median, minimum and maximum are reported, and how the boards
are spread over the stages at the end.  Promotion is timed on the tables of `4x6` (256 MiB per stage), the
median of `--repeats` x 4 single calls; its traffic is two reads and one write of a stage.  With G2048_LIB
set to another build of the library every call goes to that build; a build from before the stages existed
runs the one-stage rows only (`--stages none`, no promotion): run the two alternately in one session to
compare them.  There is no pass / fail threshold: this is a measuring tool, and what it printed on an
MI355X is recorded in DESIGN.md (Multi-stage networks).

    [G2048_LIB=old/libg2048.so] python tools/time_ntuple_stages.py [--rules td tc --stages none 16,64,128]
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

PEAK_GBS = 8000.0  # the HBM peak of an MI355X


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", default="lines-squares-4", choices=sorted(PRESETS))
    ap.add_argument("--rules", nargs="+", default=list(NTupleTrainer.RULES), choices=NTupleTrainer.RULES)
    ap.add_argument("--stages", nargs="+", default=["none", "2048,4096,8192", "16,64,128"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--lr-shift", type=int, default=18)
    ap.add_argument("--warm-steps", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-promote", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_stages needs a ROCm device")
    if os.environ.get("G2048_LIB"):
        L._lib = L.load(os.environ["G2048_LIB"])  # every wrapper then calls this build
    print("library:", L.load()._name)
    staged_build = hasattr(L.load(), "g2048_ntuple_promote")
    dev = torch.device("cuda", 0)
    rows = []
    for rule in a.rules:
        for text in a.stages:
            stages = () if text == "none" else tuple(int(v) for v in text.split(","))
            if stages and not staged_build:
                continue
            net = NTupleNet(a.tuples, dev, stages=stages)
            tr = NTupleTrainer(net, a.envs, a.lr_shift, seed=1, rule=rule)
            warm = tr.train(a.warm_steps)
            times = [event_ms(lambda: tr.train(a.steps)) for _ in range(a.repeats)]  # train() ends in a device read
            ms = float(np.median(times))
            spread = torch.bincount(net.stage(tr.boards).long(), minlength=len(stages) + 1).tolist() if staged_build else None
            rows.append({"rule": rule, "stages": text, "us_per_step": ms * 1e3 / a.steps,
                         "min_us": min(times) * 1e3 / a.steps, "max_us": max(times) * 1e3 / a.steps, "envs_per_stage": spread})
            print(f"{rule} stages {text}: median of {a.repeats} calls of {a.steps} steps {ms * 1e3 / a.steps:.1f} us per "
                  f"step (min {min(times) * 1e3 / a.steps:.1f}, max {max(times) * 1e3 / a.steps:.1f}); envs per stage "
                  f"{spread}; warm-up finished {warm['games']} games", flush=True)
            del tr, net
    promote = None
    if staged_build and not a.no_promote:
        net = NTupleNet("4x6", dev, stages=(2048,))
        net.weights[0].fill_(1)
        net.promote(0, 1)  # the first call loads the kernel
        torch.cuda.synchronize()
        times = [event_ms(lambda: net.promote(0, 1)) for _ in range(4 * a.repeats)]
        us = float(np.median(times)) * 1e3
        stage_bytes = net.weights[0].numel() * 4
        promote = {"us": us, "min_us": min(times) * 1e3, "max_us": max(times) * 1e3, "stage_bytes": stage_bytes,
                   "gb_per_s": 3 * stage_bytes / (us * 1e-6) / 1e9}
        print(f"promote 4x6 ({stage_bytes >> 20} MiB per stage): median {us:.1f} us (min {promote['min_us']:.1f}, max "
              f"{promote['max_us']:.1f}) = {promote['gb_per_s']:.0f} GB/s of {PEAK_GBS:.0f} GB/s peak "
              f"({100 * promote['gb_per_s'] / PEAK_GBS:.0f} %)", flush=True)
        assert bool((net.weights[1] == 4 * a.repeats + 1).all())
    print(json.dumps({"library": L.load()._name, "tuples": a.tuples, "envs": a.envs, "lr_shift": a.lr_shift, "rows": rows,
                      "promote": promote}))


if __name__ == "__main__":
    main()
