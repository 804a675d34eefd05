"""Time the n-tuple trainer's step with and without an eligibility trace on one GPU in one process:
g2048_ntuple_td / g2048_ntuple_tc (trace 0) and g2048_ntuple_lambda (trace > 0) under both rules, by default
on `train-ntuple`'s default net (`lines-squares-4`) at 65 536 envs.

Per (rule, trace): a fresh trainer learns for `--warm-steps` steps from zero weights, so that the timed
steps run on mid-game boards with full traces; then `--repeats` calls of `--steps` steps are timed with
HIP events, each continuing the games of the one before; the median is reported.  With G2048_LIB set to
another build of the library every call goes to that build (an older one has trace 0 only): run the two
alternately in one session to compare them.  There is no pass / fail threshold: this is a measuring
tool, and what it printed on an MI355X is recorded in DESIGN.md (TD(lambda) and TC(lambda)).

    [G2048_LIB=old/libg2048.so] python tools/time_ntuple_lambda.py [--rules td tc --traces 0 1 3 --lambda-shift 1]
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
    ap.add_argument("--traces", nargs="+", type=int, default=[0, 1, 3])
    ap.add_argument("--lambda-shift", type=int, default=1)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--lr-shift", type=int, default=18)
    ap.add_argument("--warm-steps", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_lambda needs a ROCm device")
    if os.environ.get("G2048_LIB"):
        L._lib = L.load(os.environ["G2048_LIB"])  # every wrapper then calls this build
    print("library:", L.load()._name)
    dev = torch.device("cuda", 0)
    rows = []
    for rule in a.rules:
        for h in a.traces:
            net = NTupleNet(a.tuples, dev)
            tr = NTupleTrainer(net, a.envs, a.lr_shift, seed=1, rule=rule, trace_len=h, lambda_shift=a.lambda_shift)
            warm = tr.train(a.warm_steps)
            times = [event_ms(lambda: tr.train(a.steps)) for _ in range(a.repeats)]  # train() ends in a device read
            ms = float(np.median(times))
            full = int((tr.hist_len == h).sum()) if h > 0 else a.envs
            rows.append({"rule": rule, "trace": h, "us_per_step": ms * 1e3 / a.steps, "min_us": min(times) * 1e3 / a.steps,
                         "max_us": max(times) * 1e3 / a.steps, "env_steps_per_s": a.envs * a.steps / (ms * 1e-3)})
            print(f"{rule} trace {h}: median of {a.repeats} calls of {a.steps} steps {ms * 1e3 / a.steps:.1f} us per step "
                  f"(min {min(times) * 1e3 / a.steps:.1f}, max {max(times) * 1e3 / a.steps:.1f}) = "
                  f"{a.envs * a.steps / (ms * 1e-3):.3g} env-steps/s; {full} of {a.envs} envs with a full trace; warm-up "
                  f"finished {warm['games']} games", flush=True)
    print(json.dumps({"library": L.load()._name, "tuples": a.tuples, "envs": a.envs, "lr_shift": a.lr_shift,
                      "lambda_shift": a.lambda_shift, "rows": rows}))


if __name__ == "__main__":
    main()
