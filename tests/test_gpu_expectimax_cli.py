"""`train.py play-expectimax` as a user runs it, in a fresh child process: four short seeded games."""

import subprocess
import sys

import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu


def test_play_expectimax_runs(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    cmd = [sys.executable, str(PKG / "train.py"), "play-expectimax", "-g", "4", "--depth", "2", "--max-moves", "40"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Eval Results - Max: ") and "Avg: " in ln and "Median: " in ln for ln in lines)
    assert any(ln.startswith("Tiles Reached - 512: ") and "2048: " in ln for ln in lines)
