"""CPU reference of the n-tuple network and its afterstate TD(0) step (include/g2048_ntuple.h,
g2048/ntuple.py), in numpy and built only from oracle functions: O.move (the move, its points and -- as
move(b, a) != b -- its legality), O.legal_mask, O.step (the env step with auto-reset done here from
O.reset, as g2048_env_step does it) and O.reset.  All values are int64 in points x 4096; the weights
are int32 and wrap.  Shared by tests/test_ntuple_host.py and tests/test_gpu_ntuple.py; not a test module
itself."""

import numpy as np

from oracle import oracle as O

S = 4096
I64_MIN = np.iinfo(np.int64).min
PRESETS = {
    "lines-squares-4": [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 4, 5], [1, 2, 5, 6], [5, 6, 9, 10]],
    "4x6": [[0, 1, 2, 3, 4, 5], [4, 5, 6, 7, 8, 9], [0, 1, 2, 4, 5, 6], [4, 5, 6, 8, 9, 10]],
}


NETS = {  # the nets of the value / choose tests: every tuple length the tests run, the longest included
    "lines-squares-4": PRESETS["lines-squares-4"],
    "t1k1": [[5]],
    "t8k3": [[0, 1, 2], [4, 5, 6], [0, 4, 8], [1, 5, 9], [0, 1, 4], [5, 6, 10], [3, 6, 9], [15, 10, 5]],
    "t2k6": PRESETS["4x6"][:2],
}
ENDING = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3], np.int8)  # one legal merge, then the end
DEAD = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.int8)    # no legal move
TD_STEPS = 200
# the TD cases of the GPU tests: name -> (net, n, lr_shift, random weights)
TD_CASES = {
    "n1-zero": ("lines-squares-4", 1, 12, False), "n1-random": ("lines-squares-4", 1, 20, True),
    "n64-zero": ("lines-squares-4", 64, 12, False), "n64-random": ("lines-squares-4", 64, 20, True),
    "n300-zero": ("lines-squares-4", 300, 12, False), "n300-random": ("lines-squares-4", 300, 20, True),
    "n64-t8k3": ("t8k3", 64, 20, True),
}  # lr_shift 12 from zero weights and 20 from random ones: where every case meets the rounding rule's window
TD_SEED = 31


def value_boards():
    """The 30 roots of mc_reference.roots() (8 finished, live ones with illegal actions) and three boards
    holding exponents 15 and 16 (2^16 indexes like 2^15)."""
    from mc_reference import roots
    big = np.array([[16, 15, 14, 0, 1, 1, 2, 0, 0, 3, 3, 0, 15, 16, 0, 0],
                    [15, 15, 0, 0, 16, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 1],
                    [16, 1, 16, 2, 3, 15, 4, 15, 15, 5, 16, 6, 7, 16, 8, 0]], np.int8)
    return np.ascontiguousarray(np.concatenate([roots(), big]))


def random_weights(cells, seed, bits=32):
    """int32 [T, 16^K], uniform over the signed `bits`-bit range."""
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(len(cells), 16 ** len(cells[0])),
                        dtype=np.int64).astype(np.int32)


def td_start(name):
    """-> (cells, weights, boards, lr_shift) of a TD case: the even envs start on the board one move from
    its end, the odd ones on fresh boards (O.reset at counter 0), the last env (n > 1) on a dead board."""
    net, n, lr_shift, rand = TD_CASES[name]
    cells = NETS[net]
    w = random_weights(cells, 7, bits=22) if rand else np.zeros((len(cells), 16 ** len(cells[0])), np.int32)
    boards = O.reset(n, seed=TD_SEED, step_idx=0)
    boards[::2] = ENDING
    if n > 1:
        boards[n - 1] = DEAD
    return cells, w, boards, lr_shift


def _symmetries():
    """The 8 cell permutations p of the square's symmetry group: g(b)[c] = b[p[c]]."""
    grid = np.arange(16).reshape(4, 4)
    out = []
    for m in (grid, grid.T):
        for k in range(4):
            out.append(np.rot90(m, k).reshape(16).copy())
    assert len({tuple(p) for p in out}) == 8
    return out


SYMS = _symmetries()


def indices(cells, boards):
    """-> int64 [8, T, n]: idx_t(g(b)) for the 8 symmetries g."""
    cells = np.asarray(cells, np.int64)
    e = np.minimum(np.asarray(boards, np.int8).reshape(-1, 16), 15).astype(np.int64)
    out = np.zeros((8, len(cells), len(e)), np.int64)
    for g, p in enumerate(SYMS):
        gb = e[:, p]
        for t, tup in enumerate(cells):
            for j, c in enumerate(tup):
                out[g, t] |= gb[:, c] << (4 * j)
    return out


def value(cells, weights, boards):
    """V(b) int64 [n]; weights int32 [T, 16^K]."""
    idx = indices(cells, boards)
    w = np.asarray(weights).astype(np.int64)
    return w[np.arange(len(w))[None, :, None], idx].sum((0, 1))


def choose(cells, weights, boards):
    """-> (q int64 [n, 4] (INT64_MIN: illegal), legal uint8 [n], best uint8 [n] (0xFF: none),
    after int8 [n, 4, 16] = move(b, a))."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    n = len(boards)
    rep = np.repeat(boards, 4, axis=0)
    moved, pts, _ = O.move(rep, np.tile(np.arange(4), n))
    ok = (moved != rep).any(1)
    q = np.where(ok, S * pts.astype(np.int64) + value(cells, weights, moved), I64_MIN).reshape(n, 4)
    ok = ok.reshape(n, 4)
    legal = (ok * (1 << np.arange(4))).sum(1).astype(np.uint8)
    assert np.array_equal(legal, O.legal_mask(boards))
    best = np.where(ok.any(1), q.argmax(1), 0xFF).astype(np.uint8)  # argmax: the lowest index among equals
    return q, legal, best, moved.reshape(n, 4, 16)


def env_step_auto_reset(boards, actions, seed, ctr, env_base=0):
    """g2048_env_step with policy actions and G2048_OPT_AUTO_RESET -> (boards, points int64, done bool)."""
    b, f, _, _ = O.step(boards, actions, O.RNG_PHILOX, seed=seed, step_idx=ctr, env_base=env_base)
    done = f["done"].astype(bool)
    if done.any():
        fresh = O.reset(len(b), O.RNG_PHILOX, seed=seed, step_idx=ctr, env_base=env_base)
        b = np.where(done[:, None], fresh, b)
    return b, f["points"].astype(np.int64), done


class TDState:
    """The carried state of g2048_ntuple_td, all numpy: weights int32 [T, 16^K] (updated in place),
    boards / after int8 [n, 16], pending uint8 [n], run_score int64 [n], stats int64 [4]."""

    def __init__(self, cells, weights, boards, after=None, pending=None, run_score=None, stats=None):
        self.cells = [list(t) for t in cells]
        self.weights = np.array(weights, np.int32)
        self.boards = np.array(boards, np.int8).reshape(-1, 16)
        n = len(self.boards)
        self.after = np.zeros((n, 16), np.int8) if after is None else np.array(after, np.int8)
        self.pending = np.zeros(n, np.uint8) if pending is None else np.array(pending, np.uint8)
        self.run_score = np.zeros(n, np.int64) if run_score is None else np.array(run_score, np.int64)
        self.stats = np.zeros(4, np.int64) if stats is None else np.array(stats, np.int64)


def td(st: TDState, steps, lr_shift, seed, counter, env_base=0, events=None):
    """`steps` TD steps on st, in place.  events (optional dict) counts what the GPU tests claim to cover:
    "ended" (steps that set pending = 2), "dead" (boards without a legal move), "shared" (steps in which
    two envs add to one weight), "double" (an env hitting one weight twice in one update), "neg_round"
    (negative deltas of magnitude <= 2^(lr_shift - 1) and > 0: floor would give -1, the rule gives 0),
    "clamped"."""
    n = len(st.boards)
    T = len(st.cells)
    ev = dict.fromkeys(("ended", "dead", "shared", "double", "neg_round", "clamped"), 0)
    tcol = np.arange(T)[None, :, None]
    for s in range(steps):
        q, legal, best, moved = choose(st.cells, st.weights, st.boards)
        has = legal != 0
        a = np.where(has, best, 0)
        target = np.where(has, q[np.arange(n), a], 0)
        sprime = moved[np.arange(n), a]
        upd = st.pending != 0
        if upd.any():
            idx = indices(st.cells, st.after[upd])                       # [8, T, m], read before any add
            va = st.weights.astype(np.int64)[tcol, idx].sum((0, 1))
            delta = np.where(st.pending[upd] == 2, 0, target[upd]) - va
            raw = (delta + (1 << (lr_shift - 1))) >> lr_shift
            D = np.clip(raw, -(1 << 30), 1 << 30)
            ev["clamped"] += int((raw != D).sum())
            ev["neg_round"] += int(((delta < 0) & (-delta <= (1 << (lr_shift - 1)))).sum())
            flat = (tcol * st.weights.shape[1] + idx)                    # [8, T, m]
            if events is not None:
                per_env = np.sort(flat.reshape(8 * T, -1), axis=0)       # [8 T, m]: the weights of each env
                ev["double"] += int((np.diff(per_env, axis=0) == 0).any(0).sum())
                pairs = np.unique(np.stack([per_env.reshape(-1), np.tile(np.arange(per_env.shape[1]), 8 * T)]), axis=1)
                ev["shared"] += int((np.unique(pairs[0], return_counts=True)[1] > 1).any())
            acc = st.weights.astype(np.int64).reshape(-1)
            np.add.at(acc, flat.reshape(-1), np.broadcast_to(D, idx.shape).reshape(-1))
            st.weights[...] = acc.astype(np.uint64).astype(np.uint32).view(np.int32).reshape(st.weights.shape)  # wrap
            st.stats[3] += int(upd.sum())
        st.boards, pts, done = env_step_auto_reset(st.boards, a, seed, counter + s, env_base)
        st.run_score += pts
        if done.any():
            fin = st.run_score[done]
            st.stats[0] += len(fin)
            st.stats[1] += int(fin.sum())
            st.stats[2] = max(int(st.stats[2]), int(fin.max()))
            st.run_score[done] = 0
        st.after = np.where(has[:, None], sprime, st.after)
        st.pending = np.where(has, np.where(done, 2, 1), 0).astype(np.uint8)
        ev["ended"] += int((st.pending == 2).sum())
        ev["dead"] += int((~has).sum())
    if events is not None:
        for k, v in ev.items():
            events[k] = events.get(k, 0) + v
    return st


def cpu_play(cells, weights, num_games, max_moves, game_seed):
    """NTuplePlayer.play_games on Philox games with the oracle: reset at counter 0, move m stepped at
    counter m + 1.  -> (scores, moves, boards)."""
    boards = O.reset(num_games, seed=game_seed, step_idx=0)
    scores = np.zeros(num_games, np.int64)
    moves = np.zeros(num_games, np.int64)
    for m in range(max_moves):
        active = O.legal_mask(boards) != 0
        if not active.any():
            break
        _, _, best, _ = choose(cells, weights, boards)
        b2, f, _, _ = O.step(boards, np.where(active, best, 0), seed=game_seed, step_idx=m + 1)
        boards = np.where(active[:, None], b2, boards)
        scores += np.where(active, f["points"], 0)
        moves += active
    return scores, moves, boards
