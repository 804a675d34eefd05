"""Time g2048_ntuple_fill and g2048_ntuple_promote_from on one GPU in one process: by default the net `4x6` with one
stage (256 MB of tables) and with the stages 2048,4096,8192 (G = 4, 1 GB).

fill (all stages of the net in one launch) is timed against torch.Tensor.fill_ on the same tensor; promote_from (one
stage onto another, with a non-zero base) against g2048_ntuple_promote on the same two stages, out of `--parent-lib`
(a build of the library from before promote_from existed) when that is given, else out of this build, whose
nt_promote_kernel is the parent's instruction for instruction.  The calls of a pair alternate; a call is timed
with HIP events around `--calls` back-to-back launches, so that a window is milliseconds and not one launch;
`--repeats` windows, the first dropped (it loads the kernels); the median, minimum and maximum per launch and the
bytes moved over the median are reported.  A one-stage net has nothing to promote: its rows are the fill's.
The results of the calls are checked once, outside the timed region.  There is no pass / fail threshold: this is a
measuring tool, and what it printed on an MI355X is recorded in DESIGN.md (Optimistic initialisation).

    python tools/time_ntuple_init.py [--parent-lib old/libg2048.so] [--stages "" 2048,4096,8192]
"""

from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))

from g2048 import _lib as L  # noqa: E402
from g2048.ntuple import PRESETS, NTupleNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", default="4x6", choices=sorted(PRESETS))
    ap.add_argument("--stages", nargs="+", default=["", "2048,4096,8192"], help="stage lists, '' for one stage")
    ap.add_argument("--w0", type=int, default=2048000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_init needs a ROCm device")
    dev = torch.device("cuda", 0)
    print("library:", L.load()._name)
    parent = L.load(a.parent_lib) if a.parent_lib else L.load()
    print("promote comparator:", parent._name)
    rows = []
    for stage_text in a.stages:
        stages = tuple(int(v) for v in stage_text.split(",") if v.strip())
        net = NTupleNet(a.tuples, dev, stages=stages)
        w, G = net.weights, net.num_stages
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        staged = L._staged(net.c)

        def fill():
            L.ntuple_fill(net.c, a.w0, dev)

        def torch_fill():
            w.fill_(a.w0)

        def promote_from():
            L.ntuple_promote_from(net.c, 0, 1, a.w0, dev)

        def promote():
            status = parent.g2048_ntuple_promote(stream, ctypes.byref(staged), 0, 1)
            if status != 0:
                raise SystemExit(f"g2048_ntuple_promote of {parent._name} failed with status {status}")

        # each call once, checked: fill leaves w0 everywhere; from there promote_from(base w0) is a copy and
        # promote doubles
        w.zero_()
        fill()
        torch.cuda.synchronize()
        assert bool((w == a.w0).all())
        stage_bytes = w[0].numel() * 4 if stages else 0
        calls = {"fill": (fill, w.numel() * 4), "torch.fill_": (torch_fill, w.numel() * 4)}
        if G > 1:
            w[0].add_(5)
            promote_from()
            torch.cuda.synchronize()
            assert bool((w[1] == a.w0 + 5).all())
            promote()
            torch.cuda.synchronize()
            assert bool((w[1] == 2 * a.w0 + 10).all())
            calls["promote_from"] = (promote_from, 3 * stage_bytes)  # two loads and a store per weight
            calls["promote (comparator)"] = (promote, 3 * stage_bytes)
        times = {k: [] for k in calls}
        for rep in range(a.repeats + 1):
            for name, (fn, _) in calls.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for name, t in times.items():
            med, nbytes = float(np.median(t)), calls[name][1]
            rows.append({"stages": stage_text, "G": G, "call": name, "us": med, "min_us": min(t), "max_us": max(t),
                         "bytes": nbytes, "GB_per_s": nbytes / med / 1e3})
            print(f"{a.tuples} G={G}, {name}: median of {a.repeats} windows of {a.calls} launches {med:.1f} us per launch "
                  f"(min {min(t):.1f}, max {max(t):.1f}); {nbytes / 2 ** 20:.0f} MiB moved, {nbytes / med / 1e3:.0f} GB/s",
                  flush=True)
        del net, w
        torch.cuda.empty_cache()
    print(json.dumps({"library": L.load()._name, "comparator": parent._name, "tuples": a.tuples, "w0": a.w0,
                      "calls": a.calls, "repeats": a.repeats, "rows": rows}))


if __name__ == "__main__":
    main()
