"""CPU-side checks of the Monte-Carlo search's seams: the C ABI declaration and export, the ctypes
wrapper's refusal of CPU tensors, the player's argument checks and the `play-mc` command's options."""

import re

import pytest
import torch

from conftest import ROOT


def test_header_declares_and_library_exports():
    from g2048 import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "g2048.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("g2048_mc_search_workspace_bytes", "g2048_mc_search"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header


def test_workspace_bytes():
    from g2048 import _lib
    assert _lib.mc_search_workspace_bytes(1, 1) >= 4
    assert _lib.mc_search_workspace_bytes(1024, 64) >= 4 * 1024


def test_cpu_tensors_are_rejected():
    from g2048 import _lib
    n = 4
    with pytest.raises(_lib.G2048Error):
        _lib.mc_search(torch.zeros(n, 16, dtype=torch.int8), 4, 4, _lib.make_rng(_lib.RNG_PHILOX, 1, 0, 0),
                       torch.zeros(n, 4, dtype=torch.int64), torch.zeros(n, 4, dtype=torch.int64),
                       torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8),
                       torch.zeros(64, dtype=torch.uint8))


@pytest.mark.parametrize("playouts,depth", [(0, 8), (-3, 8), (4097, 8), (8, -1), (8, 65537)])
def test_player_rejects_out_of_range(playouts, depth):
    from g2048.search import MonteCarloPlayer
    with pytest.raises(ValueError):
        MonteCarloPlayer(playouts, depth, "cuda")


def test_player_accepts_the_range_ends():
    from g2048.search import MonteCarloPlayer
    for playouts, depth in ((1, 0), (4096, 65536)):
        p = MonteCarloPlayer(playouts, depth, "cuda")  # no device is touched before a search
        assert (p.playouts, p.depth) == (playouts, depth)


def test_play_mc_help_lists_its_options():
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["play-mc", "--help"])
    assert r.exit_code == 0, r.output
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    for opt in ("--games", "-g", "--playouts", "--depth", "--max-moves"):
        assert opt in out, opt
