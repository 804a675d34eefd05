"""CPU reference of tile-downgrading (Tile-downgrading of include/g2048_ntuple.h; g2048_ntuple_downgrade,
g2048.ntuple.downgrade_boards, NTuplePlayer(downgrade=...)), in numpy: the rule restated round by round on all
boards at once, the boards of the tests (a Philox generator and hand-made ones) and the host loop of a game played
on translated boards.  Shared by tests/test_ntuple_downgrade_host.py and tests/test_gpu_ntuple_downgrade.py; not a
test module itself."""

import functools

import numpy as np

from oracle import oracle as O

# (from_exp, lo_exp, rounds) of the tests: the paper's rule, a middle one, every round there is, and the widest
PARAMS = [(15, 1, 1), (12, 3, 3), (8, 2, 16), (2, 1, 16)]
SEED, N_RANDOM = 2048, 4096


def downgrade(boards, from_exp, lo_exp, rounds, gaps=None):
    """-> (boards' int8 [n, 16], shift uint8 [n]).  gaps (optional list) receives one int64 [n] per round: the j
    of the round applied to each board, -1 where the board was done."""
    assert 2 <= from_exp <= 31 and 1 <= lo_exp < from_exp and 1 <= rounds <= 16
    u = np.array(boards, np.int8).reshape(-1, 16).view(np.uint8).astype(np.int64)  # a cell as its unsigned byte
    n = len(u)
    shift = np.zeros(n, np.uint8)
    values = np.arange(32)
    for _ in range(rounds):
        part = (u >= 1) & (u <= 31)                                     # the cells that take part
        present = (part[:, :, None] & (u[:, :, None] == values)).any(1)  # [n, 32]: P
        m = np.where(present, values, 0).max(1)
        absent = ~present & (values >= lo_exp) & (values < m[:, None])
        j = np.where(absent, values, -1).max(1)                          # the largest gap, -1 without one
        go = (m >= from_exp) & (j >= 0)
        j = np.where(go, j, -1)
        if gaps is not None:
            gaps.append(j.copy())
        u -= go[:, None] & part & (u > j[:, None])
        shift += go.astype(np.uint8)
    return u.astype(np.uint8).view(np.int8), shift


def apply_round(cells, j):
    """The cell map of one round with the gap j (int64 [n], -1: none) on any int8 [n, ...] cells of those boards:
    u -> u - [j < u <= 31].  It is the round itself on the board the j came from."""
    u = np.asarray(cells, np.int8).view(np.uint8).astype(np.int64)
    jj = np.asarray(j).reshape((-1,) + (1,) * (u.ndim - 1))
    return (u - ((jj >= 0) & (u > jj) & (u <= 31))).astype(np.uint8).view(np.int8)


def scalar_downgrade(board, from_exp, lo_exp, rounds):
    """The rule on one board in plain Python, sentence by sentence: -> (list of 16 unsigned bytes, shift)."""
    u = [int(v) & 0xFF for v in board]
    shift = 0
    for _ in range(rounds):
        P = {v for v in u if 1 <= v <= 31}
        m = max(P) if P else 0
        if m < from_exp:
            break
        free = [j for j in range(lo_exp, m) if j not in P]
        if not free:
            break
        j = max(free)
        u = [v - 1 if j < v <= 31 else v for v in u]
        shift += 1
    return u, shift


@functools.lru_cache(maxsize=None)
def random_boards(n=N_RANDOM, seed=SEED):
    """int8 [n, 16], read-only: each value 1..15 is present with probability 0.6, and 4..16 random cells are filled
    from the present values (so with duplicates and empty cells; no present value: the empty board)."""
    rng = np.random.Generator(np.random.Philox(seed))
    out = np.zeros((n, 16), np.int8)
    for i in range(n):
        present = np.arange(1, 16)[rng.random(15) < 0.6]
        k = int(rng.integers(4, 17))
        cells = rng.permutation(16)[:k]
        if len(present):
            out[i, cells] = rng.choice(present, size=k)
    out.setflags(write=False)
    return out


def hand_boards():
    """name -> int8 [16]; the names say what each is for under PARAMS."""
    def row(*v):
        return np.array(list(v) + [0] * (16 - len(v)), np.int64).astype(np.uint8).view(np.int8)

    return {
        "empty": row(),
        "paper": row(15, 14, 13, 11),                                    # -> 14, 13, 12, 11 under (15, 1, 1)
        "ladder": row(*range(15, 0, -1)),                                # 15..1, no gap at all
        "gap_below_lo": row(12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 1),         # only 2 is missing: ignored with l = 3
        "gap_at_lo": row(12, 11, 10, 9, 8, 7, 6, 5, 4, 2, 1, 4, 12),     # only 3 is missing: taken with l = 3
        "gaps": row(15, 13, 12, 9, 8, 8, 4, 1, 15, 2),                   # 14, 11-10, 7-5, 3: the largest first
        "equal": row(*[13] * 16),                                        # all 16 cells equal
        "below_14": row(14, 13, 9, 2),                                   # largest f - 1 for f = 15
        "below_11": row(11, 9, 2, 2),                                    # ... for f = 12
        "below_7": row(7, 5, 1),                                         # ... for f = 8
        "ones": row(1, 1, 0, 1),                                         # ... for f = 2
        "foreign": row(-1, 15, -128, 13, 32, 127, 12, 33, 9, 64, 0, 14, 100, 2, 2, -2),  # u > 31: copied, not in P
        "foreign_only": row(-1, 32, 127, -128, 200, 255),
        "many_rounds": row(15, 1, 15, 1),                                # 13 gaps: more rounds than any R < 13
        "max31": row(31, 30, 28, 5),                                     # exponents above 15 take part up to 31
    }


def play(choose, num_games, max_moves, game_seed, params):
    """NTuplePlayer(..., downgrade=...).play_games on Philox games with the oracle, as R.cpu_play: choose(boards)
    -> best is called on the downgraded boards, the step is taken on the real ones.  -> (scores, moves, boards)."""
    boards = O.reset(num_games, seed=game_seed, step_idx=0)
    scores = np.zeros(num_games, np.int64)
    moves = np.zeros(num_games, np.int64)
    for m in range(max_moves):
        active = O.legal_mask(boards) != 0
        if not active.any():
            break
        best = choose(downgrade(boards, *params)[0])
        b2, f, _, _ = O.step(boards, np.where(active, best, 0), seed=game_seed, step_idx=m + 1)
        boards = np.where(active[:, None], b2, boards)
        scores += np.where(active, f["points"], 0)
        moves += active
    return scores, moves, boards
