"""CPU reference of the lambda step of the n-tuple network (the lambda step of include/g2048_ntuple.h,
g2048_ntuple_lambda): TD(lambda) and TC(lambda) with a truncated eligibility trace and lambda = 2^-s, in
numpy on tests/ntuple_reference.py (R.choose: the greedy action and the target, R.indices: the 8 T
weights of an after-state, R.env_step_auto_reset) and ntuple_tc_reference.tc_adds (the share a weight
takes under rule TC).  The carried history is hist int8 [h, n, 16] and hist_len uint8 [n] beside the
TDState.  Shared by tests/test_ntuple_lambda_host.py and tests/test_gpu_ntuple_lambda.py; not a test
module itself."""

import functools

import numpy as np

import ntuple_reference as R
import ntuple_tc_reference as C

STEPS = 200
SEED = R.TD_SEED
# The game seed of a case where R.TD_SEED does not show what covers() asks for.  n1-zero: its one env ends
# its first game on the first move (the start board) with an empty history; under seed 31 no second game
# ends within 200 steps at (3, 1), so "cut" and "terminal_traced" stay 0 there; under seed 34 a second
# game ends at all three traces.
SEEDS = {"n1-zero": 34}
TRACES = [(1, 1), (3, 1), (4, 2)]  # (trace_len h, lambda_shift s)
TD_NAMES = ["n1-zero", "n64-random", "n300-zero", "n64-t8k3"]
TC_NAMES = ["n64-zero", "n300-random"]
# (rule, case, accumulators): the starts of R.td_start, at the rule's own lr_shift (R.TD_CASES / C.TC_LR)
CASES = [("td", name, None) for name in TD_NAMES] + [("tc", name, fill) for name in TC_NAMES for fill in ("zero", "prefilled")]
EVENTS = ("traced", "decayed_out", "full", "cut", "terminal_traced", "cross", "ended", "dead", "shared", "double",
          "neg_round", "clamped")


def decay(D, k, s):
    """D_k = sign(D) (|D| >> k s), elementwise on int64: towards zero, symmetrically."""
    D = np.asarray(D, np.int64)
    return np.sign(D) * (np.abs(D) >> (k * s))


class LState(R.TDState):
    """R.TDState and the history of the lambda step: hist int8 [h, n, 16], hist_len uint8 [n]."""

    def __init__(self, cells, weights, boards, h, hist=None, hist_len=None, **kw):
        super().__init__(cells, weights, boards, **kw)
        n = len(self.boards)
        self.h = int(h)
        self.hist = np.zeros((self.h, n, 16), np.int8) if hist is None else np.array(hist, np.int8).reshape(self.h, n, 16)
        self.hist_len = np.zeros(n, np.uint8) if hist_len is None else np.array(hist_len, np.uint8)


def _wrap32(acc):
    return acc.astype(np.uint64).astype(np.uint32).view(np.int32)


def td_lambda(st: LState, tc, steps, lr_shift, s, seed, counter, events=None):
    """`steps` lambda steps on st (and tc, int64 [T, 16^K, 2], under rule TC; None: rule TD), in place, with the
    trace length st.h and lambda = 2^-s.  events (optional dict) counts: "traced" (hits of a weight with k
    >= 1 and D_k != 0), "decayed_out" ((env, k) with k <= hist_len, D != 0 and D_k == 0), "full" (steps of an
    env that left hist_len = h > 0), "cut" (hist_len going from > 0 to 0), "terminal_traced" (p == 2 updates
    with hist_len > 0), "cross" ((env, weight) pairs hit from two different k in one step); and as R.td:
    "ended", "dead", "shared" (steps in which two envs add to one weight), "double" ((env, k) hitting one
    weight twice), "neg_round", "clamped"."""
    n, T, h = len(st.boards), len(st.cells), st.h
    assert 0 <= h <= 4 and 1 <= s <= 7 and st.hist.shape == (h, n, 16)
    if tc is not None:
        assert tc.dtype == np.int64 and tc.shape == st.weights.shape + (2,) and tc.flags.c_contiguous
        Ef, Af = tc.reshape(-1, 2)[:, 0], tc.reshape(-1, 2)[:, 1].view(np.uint64)  # views: updated in place
    ev = dict.fromkeys(EVENTS, 0)
    tcol = np.arange(T)[None, :, None]
    size = st.weights.shape[1]
    for step in range(steps):
        q, legal, best, moved = R.choose(st.cells, st.weights, st.boards)
        has = legal != 0
        a = np.where(has, best, 0)
        target = np.where(has, q[np.arange(n), a], 0)
        sprime = moved[np.arange(n), a]
        p = st.pending.copy()
        hl = np.minimum(st.hist_len.astype(np.int64), h)
        upd = p != 0
        if upd.any():
            w64 = st.weights.astype(np.int64)
            va = w64[tcol, R.indices(st.cells, st.after[upd])].sum((0, 1))  # read before any add
            delta = np.where(p[upd] == 2, 0, target[upd]) - va
            raw = (delta + (1 << (lr_shift - 1))) >> lr_shift
            Du = np.clip(raw, -(1 << 30), 1 << 30)
            ev["clamped"] += int((raw != Du).sum())
            ev["neg_round"] += int(((delta < 0) & (-delta <= (1 << (lr_shift - 1)))).sum())
            ev["terminal_traced"] += int(((p == 2) & (hl > 0)).sum())
            D = np.zeros(n, np.int64)
            D[upd] = Du
            flats, Ds, envs, ks = [], [], [], []
            for k in range(h + 1):
                reach = upd & (hl >= k)
                Dk = decay(D, k, s)
                ev["decayed_out"] += int((reach & (D != 0) & (Dk == 0)).sum())
                sel = np.nonzero(reach & (Dk != 0))[0]
                if len(sel) == 0:
                    continue
                sk = st.after[sel] if k == 0 else st.hist[k - 1][sel]
                flat = tcol * size + R.indices(st.cells, sk)               # [8, T, m]
                flats.append(flat.reshape(-1))
                Ds.append(np.broadcast_to(Dk[sel], flat.shape).reshape(-1))
                envs.append(np.broadcast_to(sel, flat.shape).reshape(-1))
                ks.append(np.full(flat.size, k, np.int64))
                if k >= 1:
                    ev["traced"] += flat.size
            if flats:
                flat, Dh, env, kk = (np.concatenate(x) for x in (flats, Ds, envs, ks))
                if events is not None:
                    nw = st.weights.size
                    trip, cnt = np.unique((env * (h + 1) + kk) * nw + flat, return_counts=True)  # distinct (env, k, weight)
                    ev["double"] += len(np.unique(trip[cnt > 1] // nw))
                    pair, cnt = np.unique(trip // (nw * (h + 1)) * nw + trip % nw, return_counts=True)  # distinct (env, weight)
                    ev["cross"] += int((cnt > 1).sum())
                    ev["shared"] += int((np.diff(np.sort(pair % nw)) == 0).any())
                if tc is None:
                    add = Dh
                else:
                    add = C.tc_adds(Ef[flat], Af[flat], Dh)[0]              # the records before this step's adds
                acc = w64.reshape(-1).copy()
                np.add.at(acc, flat, add)
                st.weights[...] = _wrap32(acc).reshape(st.weights.shape)
                if tc is not None:
                    np.add.at(Ef, flat, Dh)                                 # int64 and uint64 adds wrap
                    np.add.at(Af, flat, np.abs(Dh).astype(np.uint64))
            st.stats[3] += int(upd.sum())
        st.boards, pts, done = R.env_step_auto_reset(st.boards, a, seed, counter + step)
        st.run_score += pts
        if done.any():
            fin = st.run_score[done]
            st.stats[0] += len(fin)
            st.stats[1] += int(fin.sum())
            st.stats[2] = max(int(st.stats[2]), int(fin.max()))
            st.run_score[done] = 0
        if h > 0:
            push = has & (p == 1)
            for k in range(h - 1, 0, -1):
                st.hist[k][push] = st.hist[k - 1][push]
            st.hist[0][push] = st.after[push]
            new_len = np.where(push, np.minimum(hl + 1, h), 0)
            ev["full"] += int((new_len == h).sum())
            ev["cut"] += int(((hl > 0) & (new_len == 0)).sum())
            st.hist_len = new_len.astype(np.uint8)
        st.after = np.where(has[:, None], sprime, st.after)
        st.pending = np.where(has, np.where(done, 2, 1), 0).astype(np.uint8)
        ev["ended"] += int((st.pending == 2).sum())
        ev["dead"] += int((~has).sum())
    if events is not None:
        for k, v in ev.items():
            events[k] = events.get(k, 0) + v
    return st


def midgame_boards(n):
    """int8 [n, 16]: exponents 1..15 drawn by default_rng(0), then a fifth of the cells emptied."""
    rng = np.random.default_rng(0)
    boards = rng.integers(1, 16, size=(n, 16)).astype(np.int8)
    boards[rng.random(boards.shape) < 0.2] = 0
    return boards


def start(rule, name, fill):
    """-> (cells, weights, boards, lr_shift, tc or None) of a case: R.td_start at the rule's own lr_shift.
    Rule tc on n300-random starts envs 4..298 on mid-game boards (midgame_boards) instead of R.td_start's
    ending and fresh ones; envs 0..3 and the dead board of env 299 stay.  With R.td_start's boards no error
    of that case ever decays to 0 at s = 2 (covers()): at its lr_shift 4 the 150 envs that start on the one
    ending board add 150 full D to the same fresh weights in their first update, the median |D| is 4.5e5
    at the first update and 2.8e8 at the third, and no |D| of 59 699 is below 256; game seeds 31..79
    did not change that.  On distinct mid-game boards the weights diverge a few steps later, and one error
    of the run (|D| < 256 with a full history) decays to 0 at k = 4 before they do; 1 of 90 draws of such
    boards showed one, none showed more."""
    if rule == "tc":
        cells, w, boards, lr_shift, tc = C.tc_start(name, fill)
        if name == "n300-random":
            boards = boards.copy()
            boards[4:299] = midgame_boards(300)[4:299]
        return cells, w, boards, lr_shift, tc
    return R.td_start(name) + (None,)


def seed_of(name):
    return SEEDS.get(name, SEED)


def run(rule, name, fill, h, s, steps, counter=1, events=None):
    """A fresh reference run of a case -> (LState, tc or None)."""
    cells, w, boards, lr_shift, tc = start(rule, name, fill)
    st = td_lambda(LState(cells, w, boards, h), tc, steps, lr_shift, s, seed_of(name), counter, events=events)
    return st, tc


@functools.lru_cache(maxsize=None)
def ref_case(rule, name, fill, h, s):
    """-> (LState, tc or None, events) after STEPS steps of a case: computed once per process, read-only."""
    ev = {}
    st, tc = run(rule, name, fill, h, s, STEPS, events=ev)
    for a in (st.weights, st.boards, st.after, st.hist, st.hist_len, st.pending, st.run_score, st.stats) + \
            (() if tc is None else (tc,)):
        a.setflags(write=False)
    return st, tc, ev


def covers(name, s, ev):
    """What a case must show on the reference before a device result is compared with it."""
    n = R.TD_CASES[name][1]
    for k in ("traced", "full", "cut", "terminal_traced", "cross"):
        assert ev[k] > 0, (k, ev)
    if s == 2:
        assert ev["decayed_out"] > 0, ev
    if n > 1:
        assert ev["shared"] > 0 and ev["dead"] > 0, ev


def valid_hist(hist, hist_len):
    """hist with the rows at or beyond hist_len zeroed: what two runs must agree on."""
    keep = np.arange(hist.shape[0])[:, None] < np.asarray(hist_len, np.int64)[None, :]
    return np.where(keep[:, :, None], hist, 0)
