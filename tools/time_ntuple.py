"""Time the n-tuple network's two calls on one GPU in one process: g2048_ntuple_td, or with `--rule tc`
g2048_ntuple_tc (TD env-steps per second), and g2048_ntuple_choose (boards per second), by default with
the `4x6` preset (four 6-tuples, a 256 MiB table; under `--rule tc` 1 GiB of accumulators beside it) at
65 536 envs.

The envs first learn for `--warm-steps` TD steps from zero weights, so that the timed steps run on
mid-game boards spread over the table and not on 65 536 fresh boards hitting the same few weights.  TD:
`--td-steps` steps per call (two launches per step, three under `--rule tc`), `--repeats` calls timed
with HIP events, each continuing the games of the one before; the median is reported.  choose: on the
boards the TD run left,
a graph of `--choose-calls` calls replayed `--repeats` times.  There is no pass / fail threshold: this
is a measuring tool, and what it printed on an MI355X is recorded in DESIGN.md (N-tuple network).

    python tools/time_ntuple.py [--rule td --tuples 4x6 --envs 65536 --warm-steps 512 --td-steps 256 --repeats 7]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))

from g2048.ntuple import PRESETS, NTupleNet, NTuplePlayer, NTupleTrainer  # noqa: E402


def event_ms(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", default="4x6", choices=sorted(PRESETS))
    ap.add_argument("--rule", default="td", choices=NTupleTrainer.RULES)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--lr-shift", type=int, default=18)
    ap.add_argument("--warm-steps", type=int, default=512)
    ap.add_argument("--td-steps", type=int, default=256)
    ap.add_argument("--choose-calls", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple needs a ROCm device")
    dev = torch.device("cuda", 0)
    net = NTupleNet(a.tuples, dev)
    tr = NTupleTrainer(net, a.envs, a.lr_shift, seed=1, rule=a.rule)
    warm = tr.train(a.warm_steps)
    print(f"{a.tuples}: {len(net.cells)} tuples of {len(net.cells[0])} cells, {net.weights.numel() * 4 / 2**20:.0f} MiB "
          f"of weights; {a.envs} envs, lr_shift {a.lr_shift}, rule {a.rule}; after {a.warm_steps} warm-up steps: {warm['games']} games "
          f"finished, mean score {warm['mean_score']:.0f}, {int((net.weights != 0).sum())} weights touched")
    times, games = [], 0
    for _ in range(a.repeats):
        out = {}
        times.append(event_ms(lambda: out.update(tr.train(a.td_steps))))  # train() ends in a device read
        games += out["games"]
    ms = float(np.median(times))
    print(f"{a.rule}: {a.td_steps} steps per call, median of {a.repeats} calls {ms:.2f} ms (min {min(times):.2f}, max "
          f"{max(times):.2f}) = {ms * 1e3 / a.td_steps:.1f} us per step, {a.envs * a.td_steps / (ms * 1e-3):.3g} "
          f"env-steps/s; {games} games finished meanwhile")

    player = NTuplePlayer(net)
    bufs = player._buffers(a.envs)
    boards = tr.boards
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        player._search(boards, 0, bufs)  # loads the kernel
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(a.choose_calls):
                player._search(boards, 0, bufs)
        g.replay()  # warm-up replay
        torch.cuda.synchronize()
        times = [event_ms(g.replay) / a.choose_calls for _ in range(a.repeats)]
    torch.cuda.current_stream().wait_stream(side)
    ms = float(np.median(times))
    legal = int(((bufs[2].to(torch.int32).unsqueeze(1) >> torch.arange(4, device=dev)) & 1).sum())
    print(f"choose: median of {a.repeats} replays of {a.choose_calls} calls {ms * 1e3:.1f} us per call (min "
          f"{min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) = {a.envs / (ms * 1e-3):.3g} boards/s; {legal} legal "
          f"moves = {legal * 8 * len(net.cells)} gathers per call")


if __name__ == "__main__":
    main()
