"""The n-tuple network trained by afterstate TD(0) (include/g2048_ntuple.h): the table-based 2048
learner (Szubert & Jaskowski 2014; Yeh et al. 2016), on the device.

NTupleNet: T tuples of K board cells and one int32 table of 16^K weights per tuple; the value of a
board is the sum of the 8 T weights its tuples index under the 8 symmetries of the square, in points x
4096.  NTupleTrainer: `envs` games learning in parallel on one net (g2048_ntuple_td): every env plays the
move of the largest points + value and moves the weights of its previous after-state towards that
maximum; the updates are integer adds, so a run is reproducible bit for bit.  With rule="tc" every
weight sets its own step size from the sums of its past updates (temporal-coherence learning,
g2048_ntuple_tc), integer too.  With trace_len > 0 the error of an after-state is also passed back, halved
(or shifted by lambda_shift) per move, to the trace_len after-states before it: TD(lambda) / TC(lambda) with
lambda = 2^-lambda_shift (g2048_ntuple_lambda).  With `stages` a net keeps one set of tables per stage of
the game, the stage of a board given by its largest tile (Yeh et al. 2016; Jaskowski 2018), and the trainer's
promote_every starts every stage from the tables of the one below it.  With v_init every weight starts at
w0_of(v_init, T) instead of zero, so that every board is worth v_init points until it is learned otherwise
(optimistic initialisation, Guei et al. 2021: the exploration of a greedy learner; g2048_ntuple_fill), and
promotion subtracts that start (g2048_ntuple_promote_from).  NTupleTrainer.save / load keep and continue a
whole run, byte for byte the run that was not interrupted.  NTuplePlayer: the greedy
player of a net (g2048_ntuple_choose) or, with depth 2..3, its expectimax player (g2048_ntuple_search) in
search.py's game loop; with `downgrade` it chooses on the tile-downgraded board (downgrade_boards,
g2048_ntuple_downgrade; Guei et al. 2021): the tiles above a missing value halved, so that a board with tiles the
net has hardly seen becomes one it knows.
"""

from __future__ import annotations

import operator

import torch

from . import _lib as L
from .search import EMAX_FORMS, _SearchPlayer

PRESETS = {
    "lines-squares-4": [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 4, 5], [1, 2, 5, 6], [5, 6, 9, 10]],
    "4x6": [[0, 1, 2, 3, 4, 5], [4, 5, 6, 7, 8, 9], [0, 1, 2, 4, 5, 6], [4, 5, 6, 8, 9, 10]],
}
MAX_TUPLES, MAX_LEN, FRAC_BITS = L.NT_MAX_TUPLES, L.NT_MAX_LEN, L.NT_FRAC_BITS
MAX_ENVS = (1 << 28) - 1
MAX_SEARCH_DEPTH = 3
MAX_TRACE, MAX_LAMBDA_SHIFT = L.NT_MAX_TRACE, L.NT_MAX_LAMBDA_SHIFT
MAX_STAGES = L.NT_MAX_STAGES
MAX_W0 = 1 << 30
MAX_DOWNGRADE_ROUNDS = 16
TRAINER_FORMAT = "g2048-ntuple-trainer-1"


def _check_cells(cells) -> list[list[int]]:
    if isinstance(cells, str):
        if cells not in PRESETS:
            raise ValueError(f"unknown tuple preset {cells!r}: one of {sorted(PRESETS)}")
        cells = PRESETS[cells]
    cells = [[int(c) for c in tup] for tup in cells]
    if not 1 <= len(cells) <= MAX_TUPLES:
        raise ValueError(f"a net has 1..{MAX_TUPLES} tuples, got {len(cells)}")
    k = len(cells[0])
    if not 1 <= k <= MAX_LEN or any(len(tup) != k for tup in cells):
        raise ValueError(f"every tuple has the same 1..{MAX_LEN} cells, got {cells}")
    for tup in cells:
        if any(not 0 <= c <= 15 for c in tup) or len(set(tup)) != k:
            raise ValueError(f"the cells of a tuple are distinct and in 0..15, got {tup}")
    return cells


def _check_stages(stages) -> tuple[int, ...]:
    stages = tuple(int(v) for v in stages)
    if any(v < 2 or v > 32768 or v & (v - 1) for v in stages) or any(a >= b for a, b in zip(stages, stages[1:])):
        raise ValueError(f"stages are strictly increasing tile values, each a power of two in 2..32768, got {stages}")
    return stages


def stage_map_of(stages) -> int:
    """The stage_map of g2048_ntuple_net for a list of tile values: nibble m = the number of listed tiles that
    are <= 2^m (exponent 15 stands for every larger tile too); 0 for no stages."""
    stages = _check_stages(stages)
    return sum(sum(1 for v in stages if v <= 1 << m) << (4 * m) for m in range(1, 16))


def w0_of(v_init: int, T: int) -> int:
    """The start of every weight for an initial value of v_init points on a net of T tuples: v_init x 4096 /
    (8 T), rounded to nearest, so that V(b) = 8 T w0 is v_init points x 4096 up to that rounding.  Raises for a
    negative v_init and for a start above 2^30."""
    v_init, T = int(v_init), int(T)
    if not 1 <= T <= MAX_TUPLES:
        raise ValueError(f"a net has 1..{MAX_TUPLES} tuples, got {T}")
    if v_init < 0:
        raise ValueError(f"v_init must not be negative, got {v_init}")
    w0 = (v_init * (1 << FRAC_BITS) + 4 * T) // (8 * T)
    if w0 > MAX_W0:
        raise ValueError(f"v_init {v_init} on {T} tuples starts every weight at {w0}, above 2^30")
    return w0


def downgrade_params(from_tile, lo_tile=2, rounds=1) -> tuple[int, int, int]:
    """(from_tile, lo_tile, rounds) as tile values -> (from_exp, lo_exp, rounds) of g2048_ntuple_downgrade.  Each is
    an integer (a Python int, or what operator.index takes, such as a numpy integer); a bool, a float or a string
    raises ValueError like a value out of range."""
    def integer(v, name):
        try:
            if isinstance(v, bool):
                raise TypeError
            return operator.index(v)
        except TypeError:
            raise ValueError(f"{name} must be an integer, got {v!r}") from None

    def tile(v, name):
        v = integer(v, name)
        if v < 2 or v & (v - 1):
            raise ValueError(f"{name} must be a tile value (a power of two), got {v!r}")
        return v.bit_length() - 1

    f, l, rounds = tile(from_tile, "from_tile"), tile(lo_tile, "lo_tile"), integer(rounds, "rounds")
    if not 2 <= f <= 15:
        raise ValueError(f"from_tile must be a power of two in 4..32768, got {from_tile}")
    if not 1 <= l < f:
        raise ValueError(f"lo_tile must be a power of two in 2..from_tile / 2 = {(1 << f) // 2}, got {lo_tile}")
    if not 1 <= rounds <= MAX_DOWNGRADE_ROUNDS:
        raise ValueError(f"rounds must be in [1, {MAX_DOWNGRADE_ROUNDS}], got {rounds!r}")
    return f, l, rounds


def downgrade_boards(boards: torch.Tensor, from_tile: int, lo_tile: int = 2, rounds: int = 1,
                     out: torch.Tensor | None = None):
    """Tile-downgrading (Tile-downgrading of include/g2048_ntuple.h) of boards int8 [n, 16] -> (boards' int8 [n, 16],
    shift uint8 [n]).  A board whose largest tile is at least from_tile and that lacks a tile value in lo_tile ..
    below its largest has every tile above the largest such gap halved; that is one round, and at most `rounds` are
    applied, shift counting them.  Empty cells, the tiles up to the gap, the order between any two cells and so
    the legal moves are kept; merge points are not.  out: where to write (boards itself is allowed); None: a new
    tensor.  Raises ValueError for tiles that are no powers of two, from_tile outside 4..32768, lo_tile outside
    2..from_tile / 2 and rounds outside 1..16."""
    f, l, rounds = downgrade_params(from_tile, lo_tile, rounds)
    if out is None:
        out = torch.empty_like(boards)
    shift = torch.empty(boards.shape[0], dtype=torch.uint8, device=boards.device)
    L.ntuple_downgrade(boards, out, shift, f, l, rounds)
    return out, shift


class NTupleNet:
    """cells: a preset name or T tuples of K cell indices (4 row + col).  stages: strictly increasing tile
    values (powers of two in 2..32768); the stage of a board is the number of them that are <= its largest
    tile, and every stage has tables of its own (G = len(stages) + 1 of them).  weights: int32 [T, 16^K]
    without stages, [G, T, 16^K] with them, on `device`, zero at the start (the greedy-on-points player).
    v_init (points): every weight starts at self.w0 = w0_of(v_init, T) instead, filled by the library on a GPU
    device (g2048_ntuple_fill); with explicit weights w0 is only recorded, as the base that promote() subtracts."""

    def __init__(self, cells="lines-squares-4", device="cuda", weights: torch.Tensor | None = None, stages=(),
                 v_init: int = 0):
        self.cells = _check_cells(cells)
        self.w0 = w0_of(v_init, len(self.cells))
        self.device = torch.device(device)
        self.stages = _check_stages(stages)
        self.stage_map = stage_map_of(self.stages)
        shape = (len(self.cells), 16 ** len(self.cells[0]))
        if self.stages:
            shape = (len(self.stages) + 1,) + shape
        self._c = None
        if weights is None and self.w0 == 0:
            weights = torch.zeros(shape, dtype=torch.int32, device=self.device)
        elif weights is None and self.device.type == "cuda":
            self.weights = torch.empty(shape, dtype=torch.int32, device=self.device)
            L.ntuple_fill(self.c, self.w0, self.device)
            return
        elif weights is None:  # a host net: there is no library call on the CPU
            weights = torch.full(shape, self.w0, dtype=torch.int32, device=self.device)
        else:
            if not isinstance(weights, torch.Tensor):
                raise ValueError(f"weights must be an int32 tensor {shape}, got {type(weights).__name__}")
            if weights.dtype != torch.int32 or tuple(weights.shape) != shape:
                raise ValueError(f"weights must be int32 {shape}, got {weights.dtype} {tuple(weights.shape)}")
            weights = weights.to(self.device).contiguous()
        self.weights = weights

    @property
    def c(self):
        """The host struct the library reads (the first use needs the device): an L.NtNet, or an L.NtStagedNet
        for a net with stages."""
        if self._c is None:
            self._c = L.make_ntuple_net(self.cells, self.weights, self.stage_map)
        return self._c

    @property
    def num_stages(self) -> int:
        return len(self.stages) + 1

    def stage(self, boards: torch.Tensor) -> torch.Tensor:
        """The stage of boards int8 [n, 16] -> uint8 [n]."""
        out = torch.empty(boards.shape[0], dtype=torch.uint8, device=boards.device)
        L.ntuple_stage(self.c, boards, out)
        return out

    def promote(self, src: int, dst: int) -> None:
        """Adds the tables of stage src, less the start w0, to those of stage dst (int32, wrapping): a copy onto a
        stage that still holds w0 everywhere."""
        src, dst = int(src), int(dst)
        if not (0 <= src < self.num_stages and 0 <= dst < self.num_stages) or src == dst:
            raise ValueError(f"promote needs two different stages in 0..{self.num_stages - 1}, got {src} -> {dst}")
        if self.w0 != 0:
            L.ntuple_promote_from(self.c, src, dst, self.w0, self.device)
        else:
            L.ntuple_promote(self.c, src, dst, self.device)

    def value(self, boards: torch.Tensor) -> torch.Tensor:
        """V of boards int8 [n, 16] -> int64 [n] (points x 4096)."""
        out = torch.empty(boards.shape[0], dtype=torch.int64, device=boards.device)
        L.ntuple_value(self.c, boards, out)
        return out

    def save(self, path) -> None:
        """cells and weights, for a net with stages the key "stages" and for one with a start other than zero the
        key "w0"; a one-stage or zero-start checkpoint is unchanged."""
        ck = {"cells": self.cells, "weights": self.weights.cpu()}
        if self.stages:
            ck["stages"] = list(self.stages)
        if self.w0 != 0:
            ck["w0"] = self.w0
        torch.save(ck, path)

    @classmethod
    def load(cls, path, device="cuda") -> "NTupleNet":
        ck = torch.load(path, map_location="cpu", weights_only=True)
        return cls._with_w0(ck["cells"], device, ck["weights"], ck.get("stages", ()), ck.get("w0", 0))

    @classmethod
    def _with_w0(cls, cells, device, weights, stages, w0) -> "NTupleNet":
        """A net of given weights whose recorded start is w0 itself, not that of a v_init."""
        if isinstance(w0, bool) or not isinstance(w0, int) or not 0 <= w0 <= MAX_W0:
            raise ValueError(f"w0 must be an int in [0, 2^30], got {w0!r}")
        net = cls(cells, device, weights, stages)
        net.w0 = w0
        return net


class NTupleTrainer:
    """`envs` Philox games keyed by `seed`: the reset at counter 0, TD step s at counter 1 + s.
    lr_shift in 1..30: an update adds delta / 2^lr_shift to each of the 8 T weights; concurrent envs add
    up on shared weights, so a usable lr_shift grows with envs (10 at 256).
    rule "td": plain TD(0) (g2048_ntuple_td).  rule "tc": temporal-coherence learning (g2048_ntuple_tc):
    every weight keeps the signed and the absolute sum of the updates it received (self.tc, int64
    [T, 16^K, 2], zero at the start: 16 bytes per weight on top of its 4) and takes the share
    |signed sum| / absolute sum of an update; lr_shift is then the base rate at which a fresh weight
    starts.  The accumulators belong to the trainer, not to the net: NTupleNet.save keeps the net only
    (a new trainer on a saved net starts from zero accumulators); NTupleTrainer.save keeps them, below.
    trace_len in 0..4, lambda_shift in 1..7: with trace_len > 0 either rule runs as g2048_ntuple_lambda, and
    an update's D is also applied, shifted right by k lambda_shift (towards zero), to the after-state k
    moves older of the same game, k = 1..trace_len (self.hist int8 [trace_len, envs, 16], self.hist_len
    uint8 [envs]); a game's end reaches the trace of that game, and a new game starts an empty one.
    trace_len 0 is exactly the calls above, whatever lambda_shift is.
    promote_every P > 0 (a net with stages only): the trainer cuts its step sequence at every multiple of P
    steps since its start, however train() is called; at a cut it reads the highest stage g* any of its
    boards is in and promotes g - 1 -> g for every g in promoted_upto + 1 .. g*, in ascending order.  So every
    stage is promoted once, from the stage below it, the first time a cut sees a board at or above it;
    what the stage learned before that cut is kept, since promotion adds.  The accumulators of rule "tc"
    are not promoted.  0: never, exactly the calls above.
    carousel (a net with stages only): every env remembers the board with which its game entered each stage
    (self.pool int8 [G, envs, 16], self.valid uint8 [envs, 16]) and a finished game restarts from such a board
    of another env's slot, going round the stages in turn (self.next_stage, self.origin uint8 [envs]):
    g2048_ntuple_staged_carousel for every rule and trace.  train() then also returns restart_games and
    restart_points (finished games that started from a snapshot, and their points since), recorded (snapshots
    taken) and restarts; games / mean_score / max_score stay those of full games from the ordinary reset.  The
    pool belongs to the trainer, like the accumulators.  False: exactly the calls above.
    state_dict() / from_state_dict() (save / load on top of them) keep a whole run: the net with its start w0,
    the configuration, counter, promoted_upto and every carried tensor that exists, as one dict of CPU tensors,
    ints, strings and lists (torch.load(weights_only=True) reads it); not the workspace, and not stats, which
    train() zeroes per call.  A loaded trainer continues byte for byte as the saved one would have: the same
    weights, accumulators, carried arrays and train() results, wherever the run was cut.  On load only lr_shift
    and rule may differ from the saved run: "td" -> "tc" starts zero accumulators ("never updated": optimistic TD,
    then TC fine-tuning on the same weights), "tc" -> "td" drops them."""

    RULES = ("td", "tc")
    # the carried tensors of a started run: name -> (dtype, shape from (n, trace_len, G, weights shape))
    _CARRIED = {
        "boards": (torch.int8, lambda n, h, G, w: (n, 16)),
        "after": (torch.int8, lambda n, h, G, w: (n, 16)),
        "pending": (torch.uint8, lambda n, h, G, w: (n,)),
        "run_score": (torch.int64, lambda n, h, G, w: (n,)),
        "tc": (torch.int64, lambda n, h, G, w: w + (2,)),
        "hist": (torch.int8, lambda n, h, G, w: (h, n, 16)),
        "hist_len": (torch.uint8, lambda n, h, G, w: (n,)),
        "pool": (torch.int8, lambda n, h, G, w: (G, n, 16)),
        "valid": (torch.uint8, lambda n, h, G, w: (n, 16)),
        "next_stage": (torch.uint8, lambda n, h, G, w: (n,)),
        "origin": (torch.uint8, lambda n, h, G, w: (n,)),
    }
    _CONFIG = ("envs", "lr_shift", "seed", "rule", "trace_len", "lambda_shift", "promote_every", "carousel")

    def __init__(self, net: NTupleNet, envs: int = 256, lr_shift: int = 10, seed: int = 0x2048, rule: str = "td",
                 trace_len: int = 0, lambda_shift: int = 1, promote_every: int = 0, carousel: bool = False):
        envs, lr_shift, trace_len, lambda_shift = int(envs), int(lr_shift), int(trace_len), int(lambda_shift)
        promote_every = int(promote_every)
        if promote_every < 0:
            raise ValueError(f"promote_every must not be negative, got {promote_every}")
        if promote_every > 0 and not net.stages:
            raise ValueError("promote_every needs a net with stages")
        if carousel and not net.stages:
            raise ValueError("carousel needs a net with stages")
        if not 1 <= envs <= MAX_ENVS:
            raise ValueError(f"envs must be in [1, {MAX_ENVS}], got {envs}")
        if not 1 <= lr_shift <= 30:
            raise ValueError(f"lr_shift must be in [1, 30], got {lr_shift}")
        if rule not in self.RULES:
            raise ValueError(f"rule must be one of {self.RULES}, got {rule!r}")
        if not 0 <= trace_len <= MAX_TRACE:
            raise ValueError(f"trace_len must be in [0, {MAX_TRACE}], got {trace_len}")
        if not 1 <= lambda_shift <= MAX_LAMBDA_SHIFT:
            raise ValueError(f"lambda_shift must be in [1, {MAX_LAMBDA_SHIFT}], got {lambda_shift}")
        self.net, self.envs, self.lr_shift, self.seed, self.rule = net, envs, lr_shift, int(seed), rule
        self.trace_len, self.lambda_shift = trace_len, lambda_shift
        self.promote_every, self.promoted_upto = promote_every, 0
        self.carousel = bool(carousel)
        self.pool = self.valid = self.next_stage = self.origin = None
        self.counter = 0
        self.boards = self.after = self.pending = self.run_score = None
        self.tc = None
        self.hist = self.hist_len = None
        self.stats = self.workspace = None

    def _scratch(self):
        """What a checkpoint does not hold: stats and the workspace of the calls this configuration makes."""
        d, n = self.net.device, self.envs
        self.stats = torch.zeros(8 if self.carousel else 4, dtype=torch.int64, device=d)
        if self.carousel:
            nbytes = L.ntuple_carousel_workspace_bytes(n)
        elif self.trace_len > 0:
            nbytes = L.ntuple_lambda_workspace_bytes(n)
        else:
            nbytes = L.ntuple_tc_workspace_bytes(n) if self.rule == "tc" else L.ntuple_td_workspace_bytes(n)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)

    def _start(self):
        d, n = self.net.device, self.envs
        self.boards = torch.zeros(n, 16, dtype=torch.int8, device=d)
        self.after = torch.zeros(n, 16, dtype=torch.int8, device=d)
        self.pending = torch.zeros(n, dtype=torch.uint8, device=d)
        self.run_score = torch.zeros(n, dtype=torch.int64, device=d)
        if self.rule == "tc":
            self.tc = torch.zeros(*self.net.weights.shape, 2, dtype=torch.int64, device=d)
        if self.trace_len > 0:
            self.hist = torch.zeros(self.trace_len, n, 16, dtype=torch.int8, device=d)
            self.hist_len = torch.zeros(n, dtype=torch.uint8, device=d)
        if self.carousel:
            self.pool = torch.zeros(self.net.num_stages, n, 16, dtype=torch.int8, device=d)
            self.valid = torch.zeros(n, 16, dtype=torch.uint8, device=d)
            self.next_stage = torch.zeros(n, dtype=torch.uint8, device=d)
            self.origin = torch.zeros(n, dtype=torch.uint8, device=d)
        L.env_reset(self.boards, None, L.make_rng(L.RNG_PHILOX, self.seed, 0))
        self.counter = 1

    def _steps(self, steps: int) -> None:
        rng = L.make_rng(L.RNG_PHILOX, self.seed, self.counter)
        if self.carousel:
            L.ntuple_carousel(self.net.c, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                              self.run_score, steps, self.lr_shift, self.trace_len, self.lambda_shift, rng, self.pool,
                              self.valid, self.next_stage, self.origin, self.stats, self.workspace)
        elif self.trace_len > 0:
            L.ntuple_lambda(self.net.c, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                            self.run_score, steps, self.lr_shift, self.trace_len, self.lambda_shift, rng, self.stats,
                            self.workspace)
        elif self.rule == "tc":
            L.ntuple_tc(self.net.c, self.tc, self.boards, self.after, self.pending, self.run_score, steps, self.lr_shift,
                        rng, self.stats, self.workspace)
        else:
            L.ntuple_td(self.net.c, self.boards, self.after, self.pending, self.run_score, steps, self.lr_shift, rng,
                        self.stats, self.workspace)
        self.counter += steps

    def _cut(self) -> list[int]:
        """A cut of promote_every: promotes the stages up to the highest one a board is in, each once."""
        top = int(self.net.stage(self.boards).max())  # a host read
        promoted = list(range(self.promoted_upto + 1, top + 1))
        for g in promoted:
            self.net.promote(g - 1, g)
        self.promoted_upto = max(self.promoted_upto, top)
        return promoted

    @torch.no_grad()
    def train(self, steps: int) -> dict:
        """`steps` more TD steps of every env -> the statistics of these steps: games finished, their
        mean and largest score (0 without a finished game), the updates applied and the stages promoted."""
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"steps must be positive, got {steps}")
        if self.boards is None:
            self._start()
        if self.workspace is None:  # the first call, of a new run or of a loaded one
            self._scratch()
        self.stats.zero_()
        promoted, P = [], self.promote_every
        while steps > 0:
            k = min(steps, P - (self.counter - 1) % P) if P > 0 else steps  # counter - 1 steps since the start
            self._steps(k)
            steps -= k
            if P > 0 and (self.counter - 1) % P == 0:
                promoted += self._cut()
        games, score_sum, best, updates, *car = self.stats.tolist()
        out = {"games": games, "mean_score": score_sum / games if games else 0.0, "max_score": best,
               "updates": updates, "score_sum": score_sum, "promoted": promoted}
        if self.carousel:
            out.update(zip(("restart_games", "restart_points", "recorded", "restarts"), car))
        return out

    def accumulators(self):
        """-> (E, A): views int64 [T, 16^K] ([G, T, 16^K] with stages) of a weight's signed and absolute update sums under rule "tc" (A
        is unsigned: read its int64 as uint64); None, None before the first train()."""
        if self.rule != "tc":
            raise ValueError('only rule "tc" keeps accumulators')
        if self.tc is None:
            return None, None
        return self.tc[..., 0], self.tc[..., 1]

    def _carried_names(self, rule: str) -> list[str]:
        """The carried tensors a started run of this configuration holds under `rule`."""
        names = ["boards", "after", "pending", "run_score"]
        if rule == "tc":
            names.append("tc")
        if self.trace_len > 0:
            names += ["hist", "hist_len"]
        if self.carousel:
            names += ["pool", "valid", "next_stage", "origin"]
        return names

    def state_dict(self) -> dict:
        """The whole run as one dict of CPU tensors, ints, strings and lists (the class docstring); with a
        device net it reads the device.  The tensors are copies."""
        def host(t):
            return t.cpu() if t.is_cuda else t.clone()

        net = self.net
        sd = {"format": TRAINER_FORMAT, "cells": [list(t) for t in net.cells], "stages": list(net.stages),
              "w0": net.w0, "weights": host(net.weights), "envs": self.envs, "lr_shift": self.lr_shift,
              "seed": self.seed, "rule": self.rule, "trace_len": self.trace_len, "lambda_shift": self.lambda_shift,
              "promote_every": self.promote_every, "carousel": self.carousel, "counter": self.counter,
              "promoted_upto": self.promoted_upto}
        if self.boards is not None:
            for k in self._carried_names(self.rule):
                sd[k] = host(getattr(self, k))
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict, device="cuda", rule: str | None = None, lr_shift: int | None = None,
                        **other) -> "NTupleTrainer":
        """A new net (trainer.net) and trainer on `device` that continue the run of a state_dict().  rule and
        lr_shift, when given, replace the saved ones (the class docstring); nothing else may differ.  Raises
        ValueError for an unknown format, a missing or surplus entry and a tensor whose dtype or shape does not
        fit the saved configuration.  Makes no library call: the first train() does."""
        if other:
            raise ValueError(f"only rule and lr_shift may differ from the saved run, got {sorted(other)}")
        if not isinstance(sd, dict) or sd.get("format") != TRAINER_FORMAT:
            raise ValueError(f"not a checkpoint of an n-tuple trainer (format {TRAINER_FORMAT!r}): got "
                             f"{sd.get('format') if isinstance(sd, dict) else type(sd).__name__!r}")
        need = ("cells", "stages", "w0", "weights", "counter", "promoted_upto") + cls._CONFIG
        missing = [k for k in need if k not in sd]
        if missing:
            raise ValueError(f"the checkpoint lacks {missing}")
        for k in ("envs", "lr_shift", "seed", "trace_len", "lambda_shift", "promote_every", "counter", "promoted_upto"):
            if isinstance(sd[k], bool) or not isinstance(sd[k], int):
                raise ValueError(f"{k} must be an int, got {sd[k]!r}")
        if not isinstance(sd["carousel"], bool):
            raise ValueError(f"carousel must be a bool, got {sd['carousel']!r}")
        if sd["rule"] not in cls.RULES:
            raise ValueError(f"rule must be one of {cls.RULES}, got {sd['rule']!r}")
        net = NTupleNet._with_w0(sd["cells"], device, sd["weights"], sd["stages"], sd["w0"])
        tr = cls(net, sd["envs"], sd["lr_shift"] if lr_shift is None else lr_shift, sd["seed"],
                 sd["rule"] if rule is None else rule, sd["trace_len"], sd["lambda_shift"], sd["promote_every"],
                 sd["carousel"])
        counter, upto = sd["counter"], sd["promoted_upto"]
        if counter < 0 or not 0 <= upto < net.num_stages or (counter == 0 and upto != 0):
            raise ValueError(f"counter {counter} and promoted_upto {upto} do not fit a run of {net.num_stages} stages")
        saved = tr._carried_names(sd["rule"]) if counter > 0 else []
        known = set(need) | {"format"} | set(cls._CARRIED)
        surplus = [k for k in sd if k not in known or (k in cls._CARRIED and k not in saved)]
        if surplus:
            raise ValueError(f"the checkpoint holds {surplus}, which a run of its configuration does not carry")
        dims = (tr.envs, tr.trace_len, net.num_stages, tuple(net.weights.shape))
        for k in saved:
            dtype, shape = cls._CARRIED[k][0], cls._CARRIED[k][1](*dims)
            t = sd.get(k)
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else repr(type(t).__name__)
                raise ValueError(f"{k} must be {dtype} {shape}, got {got}")
        for k in saved:
            if k != "tc" or tr.rule == "tc":  # "tc" -> "td" drops the accumulators
                setattr(tr, k, sd[k].contiguous().to(net.device, copy=True))
        if counter > 0 and tr.rule == "tc" and tr.tc is None:  # "td" -> "tc": never updated, the base rate
            tr.tc = torch.zeros(*net.weights.shape, 2, dtype=torch.int64, device=net.device)
        tr.counter, tr.promoted_upto = counter, upto
        return tr

    def save(self, path) -> None:
        """state_dict() to a file.  The accumulators of rule "tc" are 16 bytes per weight beside its 4: 4x6 with four
        stages is about 5 GB."""
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path, device="cuda", rule: str | None = None, lr_shift: int | None = None) -> "NTupleTrainer":
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), device, rule, lr_shift)


class NTuplePlayer(_SearchPlayer):
    """Plays the move of the largest points + V(after-state) of `net` (depth 1, g2048_ntuple_choose) or of
    the largest expectimax value over `depth` in 2..3 moves, the root move included, with V at the leaves
    (g2048_ntuple_search; form "auto" / "narrow" / "wide": the lane mapping, the results do not depend on
    it).  It draws nothing.
    downgrade: None, or (from_tile, lo_tile, rounds) as downgrade_boards takes them: every search then runs on the
    tile-downgraded boards (one more launch and an int8 [n, 16] buffer per search), for a staged net at the stage of
    the translated board.  The legal moves of the two boards are the same, so the move chosen is a legal move of
    the board given; q are the values of the translated board (its merge points are those of halved tiles): they
    rank its moves and are not scores of the original.  None is the player without it: no buffer, no launch."""

    def __init__(self, net: NTupleNet, depth: int = 1, form: str = "auto", downgrade=None):
        if not isinstance(net, NTupleNet):
            raise ValueError(f"NTuplePlayer needs an NTupleNet, got {type(net).__name__}")
        depth = int(depth)
        if not 1 <= depth <= MAX_SEARCH_DEPTH:
            raise ValueError(f"depth must be in [1, {MAX_SEARCH_DEPTH}], got {depth}")
        if form not in EMAX_FORMS:
            raise ValueError(f"form must be one of {sorted(EMAX_FORMS)}, got {form!r}")
        if form == "wide" and depth < 2:
            raise ValueError("form 'wide' needs depth >= 2")
        self.downgrade = self._downgrade_exps = None  # the triple as given (tile values), and as the library takes it
        if downgrade is not None:
            if not isinstance(downgrade, (tuple, list)) or len(downgrade) != 3:
                raise ValueError(f"downgrade must be None or (from_tile, lo_tile, rounds), got {downgrade!r}")
            f, l, rounds = self._downgrade_exps = downgrade_params(*downgrade)
            self.downgrade = (1 << f, 1 << l, rounds)
        self.net, self.depth, self.form = net, depth, form
        self.device = net.device

    def _buffers(self, n: int):
        d = self.device
        bufs = (torch.empty(n, dtype=torch.uint8, device=d), torch.empty(n, 4, dtype=torch.int64, device=d),
                torch.empty(n, dtype=torch.uint8, device=d))
        if self.depth > 1:
            nbytes = L.ntuple_search_workspace_bytes(n, self.depth, EMAX_FORMS[self.form])
            if nbytes == 0:
                raise ValueError(f"{n} boards are too many for form {self.form!r}")
            bufs += (torch.empty(nbytes, dtype=torch.uint8, device=d),)
        if self.downgrade is not None:  # the translated boards, last
            bufs += (torch.empty(n, 16, dtype=torch.int8, device=d),)
        return bufs

    def _search(self, boards, move_index: int, bufs):
        if self.downgrade is not None:
            L.ntuple_downgrade(boards, bufs[-1], None, *self._downgrade_exps)
            boards, bufs = bufs[-1], bufs[:-1]
        if self.depth == 1:
            best, q, legal = bufs
            L.ntuple_choose(self.net.c, boards, q, legal, best)
        else:
            best, q, legal, ws = bufs
            L.ntuple_search(self.net.c, boards, self.depth, q, None, legal, best, ws, EMAX_FORMS[self.form])

    def choose(self, boards: torch.Tensor):
        """boards int8 [n, 16] -> (best uint8 [n] (0xFF: no legal move), q int64 [n, 4] (INT64_MIN:
        illegal), legal uint8 [n]).  With downgrade, q belongs to the translated boards (the class docstring);
        best and legal hold for the boards given."""
        bufs = self._buffers(boards.shape[0])
        self._search(boards, 0, bufs)
        return bufs[:3]
