"""bench.py as a command: a plain run prints the headline line only, and --dump-outputs writes the
trajectory record of its last timed launch -- checked against the same launches made here."""

import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

ENVS, CHUNK, STEPS, WARMUP = 4096, 8, 3, 1
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"}
FULL_ONLY = {"sweep", "single_step", "train_loop", "urm", "cpu_baseline"}


@pytest.mark.gpu
def test_plain_run_dumps_its_last_timed_step(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--envs", str(ENVS), "--chunk", str(CHUNK), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert PLAIN_KEYS <= set(res) and not FULL_ONLY & set(res)
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(ENVS * CHUNK / (res["ms_per_step"] / 1e3), rel=1e-9)

    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(got) == {"env_index", "final_boards", "traj_boards", "traj_actions", "traj_points",
                        "traj_potentials", "traj_flags"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64e6

    # the same launches here: one outside the capture, then warm-up + timed steps from the graph
    import bench
    rb = bench.RolloutBench(ENVS, CHUNK, 0, torch.device("cuda:0"))
    rb.capture(1)
    rb.run(WARMUP + STEPS)
    torch.cuda.synchronize()
    idx = got["env_index"].astype(np.int64)
    assert len(idx) == ENVS and np.array_equal(idx, np.arange(ENVS))  # small enough to be written whole
    want = {"final_boards": rb.env.boards, "traj_boards": rb.tb, "traj_actions": rb.ta, "traj_points": rb.tp,
            "traj_potentials": rb.tpot, "traj_flags": rb.tf}
    for name, t in want.items():
        assert np.array_equal(got[name], t.cpu().numpy().astype(np.float32)), name
    assert got["traj_boards"].shape == (CHUNK, ENVS, 16) and got["traj_boards"].max() > 0
