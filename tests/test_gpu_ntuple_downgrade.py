"""Tile-downgrading on the GPU (Tile-downgrading of include/g2048_ntuple.h: nt_downgrade_kernel of csrc/ntuple.hip,
g2048_ntuple_downgrade; downgrade_boards, NTuplePlayer(downgrade=...), play-ntuple --downgrade-from / --reach), byte
for byte against the numpy reference of tests/ntuple_downgrade_reference.py.  The map is integer and per board, so
there is no tolerance anywhere: boards, shift, and the best / q / legal of a player that chooses on the translated
boards are the CPU's bytes.  The boards are the reference's 4 096 Philox boards and its hand-made ones; the host
test shows that no parameter set leaves them all alone."""

import ctypes

import numpy as np
import pytest
import torch

import ntuple_downgrade_reference as DG
import ntuple_reference as R
import ntuple_search_reference as SR
import ntuple_stage_reference as SG

pytestmark = pytest.mark.gpu

PARAMS = DG.PARAMS
GUARD = 0x77
STAGES3 = (1024, 8192)  # the 3-stage variant of the player tests: largest exponent 0-9, 10-12, 13+
PLAYER_DG = (4096, 2, 2)
PLAYER_PARAMS = (12, 1, 2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


def L():
    from g2048 import _lib
    return _lib


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def all_boards():
    """The hand-made boards first, then the random ones."""
    return np.ascontiguousarray(np.concatenate([np.stack(list(DG.hand_boards().values())), DG.random_boards()]))


def run_guarded(dev, boards, params, in_place=False, with_shift=True):
    """One call with guard rows around out and guard bytes around shift -> (out, shift or None), after the guards
    and (out of place) the input were found untouched."""
    n = len(boards)
    big = torch.full((n + 2, 16), GUARD, dtype=torch.int8, device=dev)
    sh = torch.full((n + 8,), GUARD, dtype=torch.uint8, device=dev)
    out = big[1:n + 1]
    if in_place:
        out.copy_(to_dev(boards, dev))
        src = out
    else:
        src = to_dev(boards, dev)
    L().ntuple_downgrade(src, out, sh[3:3 + n] if with_shift else None, *params)
    torch.cuda.synchronize()
    g, s = big.cpu().numpy(), sh.cpu().numpy()
    assert (g[0] == GUARD).all() and (g[n + 1] == GUARD).all()
    assert (s[:3] == GUARD).all() and (s[3 + n:] == GUARD).all() and (with_shift or (s == GUARD).all())
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), boards)
    return g[1:n + 1], s[3:3 + n] if with_shift else None


# ------------------------------------------------------------------------------------ the kernel -----
@pytest.mark.parametrize("params", PARAMS, ids=str)
def test_every_board_bit_exact(dev, params):
    """4 111 boards, 17 workgroups: out of place, in place and without shift give the reference's bytes."""
    boards = all_boards()
    want, want_shift = DG.downgrade(boards, *params)
    assert (want_shift >= 1).mean() >= 0.25 and (params[2] < 2 or (want_shift >= 2).mean() >= 0.25)
    got, shift = run_guarded(dev, boards, params)
    assert np.array_equal(got, want) and np.array_equal(shift, want_shift)
    got, shift = run_guarded(dev, boards, params, in_place=True)
    assert np.array_equal(got, want) and np.array_equal(shift, want_shift)
    got, shift = run_guarded(dev, boards, params, with_shift=False)
    assert np.array_equal(got, want) and shift is None
    for name, i in zip(DG.hand_boards(), range(len(boards))):
        assert np.array_equal(got[i], want[i]), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_board_counts(dev, n):
    """The wave and block tails; the slice starts at the hand-made board of several gaps."""
    boards = all_boards()[5:5 + n]
    for params in PARAMS:
        want, want_shift = DG.downgrade(boards, *params)
        assert want_shift.any()
        got, shift = run_guarded(dev, boards, params)
        assert np.array_equal(got, want) and np.array_equal(shift, want_shift), params
        got, shift = run_guarded(dev, boards, params, in_place=True)
        assert np.array_equal(got, want) and np.array_equal(shift, want_shift), params


def test_refusals_and_empty(dev):
    """Every refusal returns G2048_EINVAL and leaves out and shift untouched; n = 0 writes nothing."""
    lib, E = L().load(), L().EINVAL
    boards = all_boards()[:64]
    b = to_dev(boards, dev)
    out = torch.full((64, 16), GUARD, dtype=torch.int8, device=dev)
    sh = torch.full((64,), GUARD, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    B, O, S = b.data_ptr(), out.data_ptr(), sh.data_ptr()

    def call(bp, op, sp, n, f, l, r):
        return lib.g2048_ntuple_downgrade(stream, bp, op, sp, n, f, l, r)

    for f, l, r in ((1, 1, 1), (32, 1, 1), (0, 1, 1), (15, 0, 1), (15, 15, 1), (15, 16, 1), (2, 2, 1), (15, 1, 0),
                    (15, 1, 17), (15, 1, -1)):
        assert call(B, O, S, 64, f, l, r) == E, (f, l, r)
    for n in (-1, 1 << 31):
        assert call(B, O, S, n, 15, 1, 1) == E, n
    for bp, op in ((None, O), (B, None), (B + 8, O), (B, O + 4), (B + 1, O)):
        assert call(bp, op, S, 63, 15, 1, 1) == E, (bp, op)
    assert call(B, O, S, 0, 15, 1, 1) == 0 and call(None, None, None, 0, 2, 1, 16) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all() and (sh.cpu().numpy() == GUARD).all()
    assert np.array_equal(b.cpu().numpy(), boards)
    assert call(B, O, None, 64, 31, 30, 16) == 0 and call(B, O, S, 64, 2, 1, 16) == 0  # the ends of the ranges
    torch.cuda.synchronize()
    want, want_shift = DG.downgrade(boards, 2, 1, 16)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(sh.cpu().numpy(), want_shift)


def test_downgrade_boards(dev):
    from g2048.ntuple import downgrade_boards
    boards = all_boards()[:300]
    b = to_dev(boards, dev)
    for (ft, lt, r), params in (((32768, 2, 1), (15, 1, 1)), ((4096, 8, 3), (12, 3, 3)), ((256, 4, 16), (8, 2, 16)),
                                ((4, 2, 16), (2, 1, 16))):
        want, want_shift = DG.downgrade(boards, *params)
        out, shift = downgrade_boards(b, ft, lt, r)
        assert out.dtype == torch.int8 and shift.dtype == torch.uint8 and out.data_ptr() != b.data_ptr()
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(shift.cpu().numpy(), want_shift)
        assert np.array_equal(b.cpu().numpy(), boards)
    out, shift = downgrade_boards(b, 32768)  # the defaults are the paper's rule
    assert np.array_equal(out.cpu().numpy(), DG.downgrade(boards, 15, 1, 1)[0])
    mine = b.clone()
    out, shift = downgrade_boards(mine, 256, 4, 16, out=mine)
    assert out is mine and np.array_equal(mine.cpu().numpy(), DG.downgrade(boards, 8, 2, 16)[0])


def test_graph_capture(dev):
    """One launch, no allocation and no synchronisation: the call is captured and replayed on new boards."""
    boards = all_boards()[:257]
    b = to_dev(np.zeros_like(boards), dev)
    out = torch.zeros(257, 16, dtype=torch.int8, device=dev)
    sh = torch.zeros(257, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L().ntuple_downgrade(b, out, sh, 12, 3, 3)  # loads the kernel outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            L().ntuple_downgrade(b, out, sh, 12, 3, 3)
    torch.cuda.current_stream().wait_stream(side)
    b.copy_(to_dev(boards, dev))
    graph.replay()
    torch.cuda.synchronize()
    want, want_shift = DG.downgrade(boards, 12, 3, 3)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(sh.cpu().numpy(), want_shift)


# ------------------------------------------------------------------------------------ the player -----
def player_boards(n):
    """Boards the engine can hold with high tiles on them: the hand-made ones without foreign cells, then random
    ones; most are translated under PLAYER_PARAMS, some twice, and some into a lower stage of STAGES3."""
    b = all_boards()
    b = b[((b >= 0) & (b <= 15)).all(1)][:n]
    t, shift = DG.downgrade(b, *PLAYER_PARAMS)
    smap = SG.stage_map_of(STAGES3)
    assert (shift >= 1).mean() >= 0.25 and (shift == 2).any() and (shift == 0).any()
    assert (SG.stage(smap, t) != SG.stage(smap, b)).any() and len(set(SG.stage(smap, t).tolist())) == 3
    return np.ascontiguousarray(b), t


def player_net(dev, stages):
    from g2048.ntuple import NTupleNet
    cells = R.NETS["lines-squares-4"]
    smap = SG.stage_map_of(stages)
    w = SG.random_staged_weights(cells, smap, 11, bits=21) if stages else R.random_weights(cells, 11, bits=21)
    assert np.abs(w.astype(np.int64)).max() < 1 << 20
    return cells, w, smap, NTupleNet(cells, dev, to_dev(w, dev), stages=stages)


@pytest.mark.parametrize("stages", [(), STAGES3], ids=["one-stage", "three-stages"])
def test_player_depth_1(dev, stages):
    from g2048.ntuple import NTuplePlayer
    boards, translated = player_boards(256)
    cells, w, smap, net = player_net(dev, stages)
    q, legal, best, _ = SG.choose(cells, w, translated, smap) if stages else R.choose(cells, w, translated)
    b = to_dev(boards, dev)
    gb, gq, gl = NTuplePlayer(net, downgrade=PLAYER_DG).choose(b)
    pb, pq, pl = NTuplePlayer(net).choose(b)
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy(), best) and np.array_equal(gq.cpu().numpy(), q)
    assert np.array_equal(gl.cpu().numpy(), legal) and np.array_equal(gl.cpu().numpy(), pl.cpu().numpy())
    assert np.array_equal(b.cpu().numpy(), boards)
    plain_q = pq.cpu().numpy()
    assert not np.array_equal(plain_q, q) and not np.array_equal(pb.cpu().numpy(), best)  # not the plain player
    ok = legal != 0
    assert ((legal[ok] >> best[ok]) & 1).all() and (best[~ok] == 0xFF).all()  # a legal action of the original


@pytest.mark.parametrize("form", ["narrow", "wide"])
@pytest.mark.parametrize("stages", [(), STAGES3], ids=["one-stage", "three-stages"])
def test_player_depth_2(dev, stages, form):
    from g2048.ntuple import NTuplePlayer
    boards, translated = player_boards(32)
    cells, w, smap, net = player_net(dev, stages)
    if stages:
        q, _, legal, best = SG.search_ref(cells, w, translated, 2, smap)
    else:
        q, _, legal, best = SR.search_ref(cells, w, translated, 2)
    b = to_dev(boards, dev)
    gb, gq, gl = NTuplePlayer(net, 2, form, downgrade=PLAYER_DG).choose(b)
    pb, pq, pl = NTuplePlayer(net, 2, form).choose(b)
    torch.cuda.synchronize()
    assert np.array_equal(gb.cpu().numpy(), best) and np.array_equal(gq.cpu().numpy(), q)
    assert np.array_equal(gl.cpu().numpy(), legal) and np.array_equal(gl.cpu().numpy(), pl.cpu().numpy())
    assert not np.array_equal(pq.cpu().numpy(), q)


def test_player_without_downgrade_has_no_buffer(dev):
    from g2048.ntuple import NTupleNet, NTuplePlayer
    net = NTupleNet("lines-squares-4", dev)
    assert len(NTuplePlayer(net)._buffers(8)) == 3 and len(NTuplePlayer(net, 2)._buffers(8)) == 4
    bufs = NTuplePlayer(net, 2, downgrade=PLAYER_DG)._buffers(8)
    assert len(bufs) == 5 and bufs[-1].dtype == torch.int8 and tuple(bufs[-1].shape) == (8, 16)
    assert len(NTuplePlayer(net, downgrade=PLAYER_DG)._buffers(8)) == 4


# ------------------------------------------------------------------------------------- the games -----
def test_play_games(dev):
    """The zero net plays greedy on points.  Below a 32768 the paper's rule never acts: the games are the plain
    player's.  From an 8 on, with four rounds, the points the player sees are those of halved tiles and the games
    part from the plain ones; they are the host loop's, which chooses on the reference's translated boards."""
    from g2048.ntuple import NTupleNet, NTuplePlayer
    cells = R.NETS["lines-squares-4"]
    net = NTupleNet(cells, dev)
    zero = np.zeros((5, 65536), np.int32)
    plain = NTuplePlayer(net).play_games(8, max_moves=200, game_seed=77)
    late = NTuplePlayer(net, downgrade=(32768, 2, 1)).play_games(8, max_moves=200, game_seed=77)
    assert max(plain["max_tiles"]) < 32768
    assert late["scores"] == plain["scores"] and late["moves"] == plain["moves"]
    assert torch.equal(late["boards"], plain["boards"])
    early = NTuplePlayer(net, downgrade=(8, 2, 4)).play_games(8, max_moves=200, game_seed=77)
    assert early["scores"] != plain["scores"] and not torch.equal(early["boards"], plain["boards"])  # else vacuous
    short = NTuplePlayer(net, downgrade=(8, 2, 4)).play_games(2, max_moves=40, game_seed=77)
    for res, (games, cap) in ((short, (2, 40)), (early, (8, 200))):  # the host loop is quick: all 200 moves too
        scores, moves, boards = DG.play(lambda b: R.choose(cells, zero, b)[2], games, cap, 77, (3, 1, 4))
        assert res["scores"] == scores.tolist() and res["moves"] == moves.tolist(), games
        assert np.array_equal(res["boards"].cpu().numpy(), boards), games


def test_command(dev, tmp_path):
    """play-ntuple with the new options on a tiny saved net, in this process: the two old lines, then the new one."""
    from typer.testing import CliRunner
    import train
    from g2048.ntuple import NTupleNet, NTuplePlayer
    w = torch.from_numpy(R.random_weights([[0, 1], [4, 5]], 3, bits=16))
    NTupleNet([[0, 1], [4, 5]], "cpu", w).save(tmp_path / "tiny.pt")
    r = CliRunner().invoke(train.app, ["play-ntuple", str(tmp_path / "tiny.pt"), "-g", "4", "--max-moves", "50",
                                       "--downgrade-from", "8", "--reach", "8,16"])
    assert r.exit_code == 0, r.output
    lines = r.output.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Eval Results - Max: ") and "Median: " in lines[0]
    assert lines[1].startswith("Tiles Reached - 512: ") and "2048: " in lines[1]
    # the games are those of the player with (8, 2, 1), and the new line counts their largest tiles
    res = NTuplePlayer(NTupleNet.load(tmp_path / "tiny.pt", dev), downgrade=(8, 2, 1)).play_games(4, 50, seeds=[0, 1, 2, 3])
    s, tiles = res["scores"], res["max_tiles"]
    assert lines[0] == f"Eval Results - Max: {max(s):.0f}, Avg: {sum(s) / 4:.1f}, Median: {sorted(s)[2]:.0f}"
    assert lines[2] == "Tiles Reached (--reach) - " + ", ".join(
        f"{v}: {sum(t >= v for t in tiles) * 25:.1f}%" for v in (8, 16))
