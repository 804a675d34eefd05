"""Time tile-downgrading (g2048_ntuple_downgrade, NTuplePlayer(downgrade=...)) on one GPU in one process.

(a) The launch alone, at 65 536 and 4 096 boards: g2048_ntuple_downgrade (out of place, with shift, the parameters
(12, 3, 3) under which most of the boards take the rounds' branch) beside g2048_ntuple_stage, the existing kernel of
the same shape (16 bytes in per lane; one byte out where the downgrade writes 17) -- the yardstick.  The two calls
alternate; a call is timed with HIP events around `--calls` back-to-back launches, so that a window is
milliseconds and not one launch; `--repeats` windows, the first dropped (it loads the kernels); the median,
minimum and maximum per launch.  The boards are those of tests/ntuple_downgrade_reference.py, repeated.
(b) The cost per move: NTuplePlayer.play_games at depth 1 and at depth 3 with downgrade=None against
downgrade=(32768, 2, 1) on the same zero-start `4x6` net and the same Philox games.  No 32768 appears in such games,
so the two play move for move the same game (checked: the same scores, moves and boards) and differ by the one
launch per move alone.  A window is `--plays` whole play_games calls between two device synchronisations on the
host clock, divided by the moves of the longest game (the game loop makes one search of all boards and one env step
per move until the last game ends); five windows each, alternating, after a warm-up; medians and spreads.
There is no pass / fail threshold: this is a measuring tool, and what it printed on an MI355X is recorded in
DESIGN.md (Tile-downgrading).

    python tools/time_ntuple_downgrade.py [--games 100] [--plays 10 2]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "2048-ppo_amd"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

from g2048 import _lib as L  # noqa: E402
from g2048.ntuple import NTupleNet, NTuplePlayer  # noqa: E402


def time_launches(dev, a, rows):
    import ntuple_downgrade_reference as DG
    base = DG.random_boards()
    net = NTupleNet([[0]], dev, stages=(2048, 4096, 8192))
    for n in a.boards:
        boards = torch.from_numpy(np.ascontiguousarray(np.tile(base, (-(-n // len(base)), 1))[:n])).to(dev)
        out = torch.empty_like(boards)
        shift = torch.empty(n, dtype=torch.uint8, device=dev)
        stage = torch.empty(n, dtype=torch.uint8, device=dev)
        calls = {"downgrade": lambda: L.ntuple_downgrade(boards, out, shift, 12, 3, 3),
                 "stage": lambda: L.ntuple_stage(net.c, boards, stage)}
        calls["downgrade"]()
        torch.cuda.synchronize()
        want, want_shift = DG.downgrade(boards.cpu().numpy(), 12, 3, 3)  # checked once, outside the timed region
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(shift.cpu().numpy(), want_shift)
        times = {k: [] for k in calls}
        for rep in range(a.repeats + 1):
            for name, fn in calls.items():
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
            rows.append({"part": "launch", "boards": n, "call": name, "us": float(np.median(t)), "min_us": min(t),
                         "max_us": max(t), "active": float((want_shift > 0).mean())})
            print(f"{n} boards, {name}: median of {a.repeats} windows of {a.calls} launches {np.median(t):.2f} us per "
                  f"launch (min {min(t):.2f}, max {max(t):.2f})", flush=True)


def time_games(dev, a, rows):
    net = NTupleNet("4x6", dev)
    for depth, plays in zip((1, 3), a.plays):
        players = {"none": NTuplePlayer(net, depth), "(32768, 2, 1)": NTuplePlayer(net, depth, downgrade=(32768, 2, 1))}
        res = {k: p.play_games(a.games, game_seed=a.game_seed) for k, p in players.items()}  # the warm-up, and the check
        x, y = res["none"], res["(32768, 2, 1)"]
        assert x["scores"] == y["scores"] and x["moves"] == y["moves"] and torch.equal(x["boards"], y["boards"])
        assert max(x["max_tiles"]) < 32768
        longest = max(x["moves"])
        times = {k: [] for k in players}
        for _ in range(a.windows):
            for k, p in players.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(plays):
                    p.play_games(a.games, game_seed=a.game_seed)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e6 / (plays * longest))
        for k, t in times.items():
            rows.append({"part": "games", "depth": depth, "downgrade": k, "games": a.games, "longest_game": longest,
                         "plays": plays, "us_per_move": float(np.median(t)), "min_us": min(t), "max_us": max(t)})
            print(f"depth {depth}, {a.games} games (longest {longest} moves, largest tile {max(x['max_tiles'])}), "
                  f"downgrade {k}: median of {a.windows} windows of {plays} plays {np.median(t):.2f} us per move "
                  f"(min {min(t):.2f}, max {max(t):.2f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--game-seed", type=int, default=0x5EED)
    ap.add_argument("--plays", type=int, nargs=2, default=[10, 2], help="play_games calls per window at depth 1 and 3")
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ntuple_downgrade needs a ROCm device")
    dev = torch.device("cuda", 0)
    print("library:", L.load()._name)
    rows = []
    time_launches(dev, a, rows)
    time_games(dev, a, rows)
    print(json.dumps({"library": L.load()._name, "calls": a.calls, "repeats": a.repeats, "windows": a.windows,
                      "rows": rows}))


if __name__ == "__main__":
    main()
