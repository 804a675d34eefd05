"""Search players without a network: the baselines a trained agent's score is compared with.

MonteCarloPlayer: for every legal move of a board, `playouts` random games of at most `depth` moves
are played on the device (g2048_mc_search, one playout per lane) and the move with the largest summed
score is taken.  ExpectimaxPlayer: exact depth-limited expectimax (g2048_expectimax), the maximum over
the moves and the expectation over every spawn, monotonicity and emptiness at the leaves; it draws
nothing.  `choose` is one search; `play_games` plays whole games with it in a `VecEnv`.
"""

from __future__ import annotations

import torch

from . import _lib as L
from .env import StepOut, VecEnv

MAX_PLAYOUTS, MAX_DEPTH = 4096, 65536
CHECK_EVERY = 16  # moves between two reads of the all-games-finished flag
MAX_EMAX_DEPTH, MAX_EMAX_WEIGHT = 4, 4096
EMAX_FORMS = {"auto": L.EMAX_AUTO, "narrow": L.EMAX_NARROW, "wide": L.EMAX_WIDE}


class _SearchPlayer:
    """The game loop both players share.  A player supplies `device`, `_buffers(n)` (element 0 = the
    chosen actions, uint8 [n]) and `_search(boards, move_index, bufs)`."""

    @torch.no_grad()
    def play_games(self, num_games: int, max_moves: int | None = None, seeds=None, game_seed: int = 0x5EED,
                   cap: int = 1 << 15) -> dict:
        """Play `num_games` games to the end (or `max_moves` moves each).  seeds given: game i spawns
        like CPython random.seed(seeds[i]) (MT19937); otherwise Philox keyed by `game_seed`, the reset
        at counter 0 and move m at counter m + 1.  One search and one env step per move; whether
        every game has ended is read from the device once per CHECK_EVERY moves.  Returns scores,
        moves, max_tiles (as episodes.play_games does) and the final boards."""
        n, dev = int(num_games), self.device
        if seeds is not None:
            env = VecEnv(n, dev, rng="mt19937", seeds=seeds)
        else:
            env = VecEnv(n, dev, rng="philox", seed=game_seed)
        env.reset()
        limit = int(max_moves) if max_moves and max_moves > 0 else cap
        bufs = self._buffers(n)
        pts = torch.zeros(CHECK_EVERY, n, dtype=torch.int32, device=dev)
        flg = torch.zeros(CHECK_EVERY, n, dtype=torch.uint8, device=dev)
        o = env.out
        rows = [StepOut(env.boards, o.actions, pts[k], o.max_tile, o.pot, flg[k]) for k in range(CHECK_EVERY)]
        scores = torch.zeros(n, dtype=torch.int64, device=dev)
        moves = torch.zeros(n, dtype=torch.int64, device=dev)
        m = 0
        while m < limit:
            k = min(CHECK_EVERY, limit - m)
            for j in range(k):
                self._search(env.boards, m + j, bufs)
                env.step(bufs[0], skip_done=True, out=rows[j])  # a finished game ignores its 0xFF
            m += k
            scores += pts[:k].sum(0)
            moves += ((flg[:k] & L.FLAG_INACTIVE) == 0).sum(0)
            if bool(((flg[k - 1] & L.FLAG_LEGAL) == 0).all()):
                break
        maxexp = env.boards.max(dim=1).values.to(torch.int64)
        return {"scores": scores.tolist(), "moves": moves.tolist(),
                "max_tiles": [0 if e == 0 else 1 << e for e in maxexp.tolist()], "boards": env.boards.clone(),
                "limit": limit}


class MonteCarloPlayer(_SearchPlayer):
    """playouts P in [1, 4096] per action, depth D in [0, 65 536] playout moves (0: the one-ply
    greedy-points player).  Searches are keyed by (`seed`, counter, `env_base` + lane)."""

    def __init__(self, playouts: int, depth: int, device="cuda", seed: int = 0x2048, env_base: int = 0):
        playouts, depth = int(playouts), int(depth)
        if not 1 <= playouts <= MAX_PLAYOUTS:
            raise ValueError(f"playouts must be in [1, {MAX_PLAYOUTS}], got {playouts}")
        if not 0 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth must be in [0, {MAX_DEPTH}], got {depth}")
        self.playouts, self.depth = playouts, depth
        self.device = torch.device(device)
        self.seed, self.env_base = int(seed), int(env_base)

    def _buffers(self, n: int):
        d = self.device
        return (torch.empty(n, dtype=torch.uint8, device=d), torch.empty(n, 4, dtype=torch.int64, device=d),
                torch.empty(n, 4, dtype=torch.int64, device=d), torch.empty(n, dtype=torch.uint8, device=d),
                torch.empty(L.mc_search_workspace_bytes(n, self.playouts), dtype=torch.uint8, device=d))

    def _search(self, boards, move_index: int, bufs):
        best, score_sum, move_sum, legal, ws = bufs
        rng = L.make_rng(L.RNG_PHILOX, self.seed, int(move_index) * max(self.depth, 1), self.env_base)
        L.mc_search(boards, self.playouts, self.depth, rng, score_sum, move_sum, legal, best, ws)

    def choose(self, boards: torch.Tensor, move_index: int):
        """One search on boards int8 [n, 16] at Philox counter move_index * max(depth, 1) ->
        (best uint8 [n] (0xFF: no legal move), score_sum int64 [n, 4], move_sum int64 [n, 4],
        legal uint8 [n])."""
        bufs = self._buffers(boards.shape[0])
        self._search(boards, move_index, bufs)
        return bufs[0], bufs[1], bufs[2], bufs[3]


class ExpectimaxPlayer(_SearchPlayer):
    """depth in [1, 4] moves looked ahead (the root move included), weights = (w_points, w_mono,
    w_empt), integers in [0, 4096], form "auto" / "narrow" / "wide" (the lane mapping; the results do
    not depend on it).  The search is exact and draws nothing: a game depends on its spawns alone."""

    def __init__(self, depth: int, weights=(1, 64, 128), device="cuda", form: str = "auto"):
        depth, weights = int(depth), tuple(int(w) for w in weights)
        if not 1 <= depth <= MAX_EMAX_DEPTH:
            raise ValueError(f"depth must be in [1, {MAX_EMAX_DEPTH}], got {depth}")
        if len(weights) != 3 or not all(0 <= w <= MAX_EMAX_WEIGHT for w in weights):
            raise ValueError(f"weights must be three integers in [0, {MAX_EMAX_WEIGHT}], got {weights}")
        if form not in EMAX_FORMS:
            raise ValueError(f"form must be one of {sorted(EMAX_FORMS)}, got {form!r}")
        if form == "wide" and depth < 2:
            raise ValueError("form 'wide' needs depth >= 2")
        self.depth, self.weights, self.form = depth, weights, form
        self.device = torch.device(device)

    def _buffers(self, n: int):
        d = self.device
        nbytes = L.expectimax_workspace_bytes(n, self.depth, EMAX_FORMS[self.form])
        if nbytes == 0:
            raise ValueError(f"{n} boards are too many for form {self.form!r}")
        return (torch.empty(n, dtype=torch.uint8, device=d), torch.empty(n, 4, dtype=torch.int64, device=d),
                torch.empty(n, 4, dtype=torch.int64, device=d), torch.empty(n, dtype=torch.uint8, device=d),
                torch.empty(nbytes, dtype=torch.uint8, device=d))

    def _search(self, boards, move_index: int, bufs):
        best, value, leaves, legal, ws = bufs
        L.expectimax(boards, self.depth, self.weights, value, leaves, legal, best, ws, EMAX_FORMS[self.form])

    def choose(self, boards: torch.Tensor):
        """One search on boards int8 [n, 16] -> (best uint8 [n] (0xFF: no legal move), value int64
        [n, 4] (-1: illegal), leaves int64 [n, 4], legal uint8 [n])."""
        bufs = self._buffers(boards.shape[0])
        self._search(boards, 0, bufs)
        return bufs[0], bufs[1], bufs[2], bufs[3]
