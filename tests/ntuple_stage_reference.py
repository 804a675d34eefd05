"""CPU reference of the multi-stage n-tuple network (Stages of include/g2048_ntuple.h; g2048_ntuple_stage,
g2048_ntuple_promote and every other call of that header on a net with a stage_map), in numpy on
tests/ntuple_reference.py (R.indices, R.env_step_auto_reset), ntuple_tc_reference.tc_adds,
ntuple_lambda_reference (LState, decay) and the oracle's move.  A staged net is the one-stage net with the
tuple row stage(b) T + t in the place of t in every index: weights int32 [G, T, 16^K] are read as [G T, 16^K]
(and [T, 16^K] for the map 0), tc int64 likewise.  Shared by tests/test_ntuple_stage_host.py and
tests/test_gpu_ntuple_stage.py; not a test module itself."""

import functools

import numpy as np

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_tc_reference as C
from oracle import oracle as O

S = R.S
I64_MIN = R.I64_MIN
STAGES = (16, 64, 128)  # the stage list of the GPU tests: G = 4, stages at largest exponent 0-3, 4-5, 6, 7+
STEPS = 200
EVENTS = LR.EVENTS + ("cross_stage", "terminal_high", "trace_cross")


def stage_map_of(stages):
    """The stage_map of a strictly increasing list of tile values (powers of two in 2..32768): nibble m = the
    number of listed tiles that are <= 2^m."""
    stages = [int(v) for v in stages]
    assert all(2 <= v <= 32768 and v & (v - 1) == 0 for v in stages), stages
    assert all(a < b for a, b in zip(stages, stages[1:])), stages
    return sum(sum(1 for v in stages if v <= 1 << m) << (4 * m) for m in range(1, 16))


def nibbles(smap):
    return [(int(smap) >> (4 * m)) & 15 for m in range(16)]


def valid_map(smap):
    """Nibble 0 is 0 and every next nibble equals the one before it or is one more."""
    nb = nibbles(smap)
    return 0 <= int(smap) < 1 << 64 and nb[0] == 0 and all(b in (a, a + 1) for a, b in zip(nb, nb[1:]))


def num_stages(smap):
    assert valid_map(smap), hex(smap)
    return 1 + nibbles(smap)[15]


def stage(smap, boards):
    """stage(b) uint8 [n]: nibble m(b) of the map, m(b) the largest exponent of the board clamped to 15."""
    m = np.minimum(np.asarray(boards, np.int8).reshape(-1, 16), 15).max(1).astype(np.int64)
    return np.array(nibbles(smap), np.uint8)[m]


def flat_rows(weights, smap, T):
    """The weights as [G T, 16^K]: a view of the array itself."""
    w = np.asarray(weights)
    G = num_stages(smap)
    assert w.shape[:-1] in ((G, T), (T,) if G == 1 else None), (w.shape, G, T)
    return w.reshape(G * T, w.shape[-1])


def flat_indices(cells, smap, size, boards):
    """-> int64 [8, T, n]: the flat positions, in [G T 16^K], of the 8 T weights V(b) reads."""
    T = len(cells)
    row = stage(smap, boards).astype(np.int64)[None, None, :] * T + np.arange(T)[None, :, None]
    return row * size + R.indices(cells, boards)


def value(cells, weights, boards, smap=0):
    """V(b) int64 [n] of a staged net."""
    wf = flat_rows(weights, smap, len(cells))
    return wf.reshape(-1).astype(np.int64)[flat_indices(cells, smap, wf.shape[1], boards)].sum((0, 1))


def choose(cells, weights, boards, smap=0):
    """R.choose on a staged net: every after-state is evaluated at its own stage."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    n = len(boards)
    rep = np.repeat(boards, 4, axis=0)
    moved, pts, _ = O.move(rep, np.tile(np.arange(4), n))
    ok = (moved != rep).any(1)
    q = np.where(ok, S * pts.astype(np.int64) + value(cells, weights, moved, smap), I64_MIN).reshape(n, 4)
    ok = ok.reshape(n, 4)
    legal = (ok * (1 << np.arange(4))).sum(1).astype(np.uint8)
    assert np.array_equal(legal, O.legal_mask(boards))
    best = np.where(ok.any(1), q.argmax(1), 0xFF).astype(np.uint8)  # argmax: the lowest index among equals
    return q, legal, best, moved.reshape(n, 4, 16)


def promote(weights, smap, src, dst):
    """W[dst] += W[src] in place, int32 and wrapping; weights int32 [G, T, 16^K]."""
    G = num_stages(smap)
    assert weights.shape[0] == G and 0 <= src < G and 0 <= dst < G and src != dst
    weights[dst] = (weights[dst].view(np.uint32) + weights[src].view(np.uint32)).view(np.int32)


def _wrap32(acc):
    return acc.astype(np.uint64).astype(np.uint32).view(np.int32)


def td_stage(st: LR.LState, tc, steps, lr_shift, s, seed, counter, smap=0, events=None):
    """`steps` steps of rule TD (tc None) or TC (tc int64, the shape of the weights + (2,)) with the trace
    st.h >= 0 and lambda = 2^-s on a staged net, in place: LR.td_lambda with the row stage * T + t in every
    index.  events (optional dict) counts what LR.td_lambda counts and: "stage_updates" (a list: per stage,
    the (env, k) updates applied to an after-state of that stage), "cross_stage" (p == 1 updates with a legal
    move where stage(after) differs from the stage of the after-state that supplied the target),
    "terminal_high" (p == 2 updates of an after-state at a stage > 0), "trace_cross" (updates in which some
    s_k, 1 <= k <= hist_len, is at a lower stage than s_0)."""
    n, T, h = len(st.boards), len(st.cells), st.h
    G = num_stages(smap)
    assert 0 <= h <= 4 and 1 <= s <= 7 and st.hist.shape == (h, n, 16)
    wf = flat_rows(st.weights, smap, T)
    assert np.shares_memory(wf, st.weights)
    size = wf.shape[1]
    if tc is not None:
        assert tc.dtype == np.int64 and tc.shape == st.weights.shape + (2,) and tc.flags.c_contiguous
        Ef, Af = tc.reshape(-1, 2)[:, 0], tc.reshape(-1, 2)[:, 1].view(np.uint64)  # views: updated in place
    ev = dict.fromkeys(EVENTS, 0)
    per_stage = np.zeros(G, np.int64)
    for step in range(steps):
        q, legal, best, moved = choose(st.cells, st.weights, st.boards, smap)
        has = legal != 0
        a = np.where(has, best, 0)
        target = np.where(has, q[np.arange(n), a], 0)
        sprime = moved[np.arange(n), a]
        p = st.pending.copy()
        hl = np.minimum(st.hist_len.astype(np.int64), h)
        upd = p != 0
        if upd.any():
            w64 = wf.reshape(-1).astype(np.int64)
            va = w64[flat_indices(st.cells, smap, size, st.after[upd])].sum((0, 1))  # read before any add
            delta = np.where(p[upd] == 2, 0, target[upd]) - va
            raw = (delta + (1 << (lr_shift - 1))) >> lr_shift
            Du = np.clip(raw, -(1 << 30), 1 << 30)
            ev["clamped"] += int((raw != Du).sum())
            ev["neg_round"] += int(((delta < 0) & (-delta <= (1 << (lr_shift - 1)))).sum())
            ev["terminal_traced"] += int(((p == 2) & (hl > 0)).sum())
            sa = stage(smap, st.after).astype(np.int64)
            ev["cross_stage"] += int(((p == 1) & has & (sa != stage(smap, sprime))).sum())
            ev["terminal_high"] += int(((p == 2) & (sa > 0)).sum())
            lower = np.zeros(n, bool)
            for k in range(1, h + 1):
                lower |= upd & (hl >= k) & (stage(smap, st.hist[k - 1]).astype(np.int64) < sa)
            ev["trace_cross"] += int(lower.sum())
            D = np.zeros(n, np.int64)
            D[upd] = Du
            flats, Ds, envs, ks = [], [], [], []
            for k in range(h + 1):
                reach = upd & (hl >= k)
                Dk = LR.decay(D, k, s)
                ev["decayed_out"] += int((reach & (D != 0) & (Dk == 0)).sum())
                sk_all = st.after if k == 0 else st.hist[k - 1]
                per_stage += np.bincount(stage(smap, sk_all[reach]), minlength=G)[:G]
                sel = np.nonzero(reach & (Dk != 0))[0]
                if len(sel) == 0:
                    continue
                flat = flat_indices(st.cells, smap, size, sk_all[sel])     # [8, T, m]
                flats.append(flat.reshape(-1))
                Ds.append(np.broadcast_to(Dk[sel], flat.shape).reshape(-1))
                envs.append(np.broadcast_to(sel, flat.shape).reshape(-1))
                ks.append(np.full(flat.size, k, np.int64))
                if k >= 1:
                    ev["traced"] += flat.size
            if flats:
                flat, Dh, env, kk = (np.concatenate(x) for x in (flats, Ds, envs, ks))
                if events is not None:
                    nw = wf.size
                    trip, cnt = np.unique((env * (h + 1) + kk) * nw + flat, return_counts=True)  # distinct (env, k, weight)
                    ev["double"] += len(np.unique(trip[cnt > 1] // nw))
                    pair, cnt = np.unique(trip // (nw * (h + 1)) * nw + trip % nw, return_counts=True)  # distinct (env, weight)
                    ev["cross"] += int((cnt > 1).sum())
                    ev["shared"] += int((np.diff(np.sort(pair % nw)) == 0).any())
                if tc is None:
                    add = Dh
                else:
                    add = C.tc_adds(Ef[flat], Af[flat], Dh)[0]              # the records before this step's adds
                acc = w64.copy()
                np.add.at(acc, flat, add)
                wf[...] = _wrap32(acc).reshape(wf.shape)
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
        events["stage_updates"] = (np.array(events.get("stage_updates", [0] * G), np.int64) + per_stage).tolist()
    return st


# ---------------------------------------------------------------------------------- the search -----
def search_ref(cells, weights, boards, depth, smap=0, stats=None):
    """g2048_ntuple_search on a staged net, level by level as ntuple_search_reference.search_ref -> (q int64
    [n, 4], leaves int64 [n, 4], legal uint8 [n], best uint8 [n]).  stats (optional dict) receives "leaves" and
    "leaf_stages": the sorted stages of the leaf after-states."""
    boards = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 16))
    assert 1 <= depth <= 3
    seen = {"leaves": 0, "leaf_stages": set()}

    def expand(b, k):
        m = len(b)
        val = np.full(4 * m, I64_MIN, np.int64)
        lv = np.zeros(4 * m, np.int64)
        if m:
            rep = np.repeat(b, 4, axis=0)
            moved, pts, _ = O.move(rep, np.tile(np.arange(4), m))
            legal = (moved != rep).any(1)
            if legal.any():
                a, l = chance(moved[legal], k - 1)
                val[legal] = S * pts[legal].astype(np.int64) + a
                lv[legal] = l
        return val.reshape(m, 4), lv.reshape(m, 4)

    def chance(after, k):
        m = len(after)
        if k == 0:
            seen["leaves"] += m
            seen["leaf_stages"] |= set(stage(smap, after).tolist())
            return value(cells, weights, after, smap), np.ones(m, np.int64)
        idx, cell = np.nonzero(after == 0)
        E = np.bincount(idx, minlength=m).astype(np.int64)
        assert (E >= 1).all()  # a legal move leaves an empty cell
        owner = np.repeat(idx, 2)
        child = after[owner].copy()
        child[np.arange(len(child)), np.repeat(cell, 2)] = np.tile(np.array([1, 2], np.int8), len(idx))
        val, lv = expand(child, k)
        dead = (val == I64_MIN).all(1)
        mv = np.where(dead, 0, val.max(1, initial=I64_MIN))
        num = np.zeros(m, np.int64)
        np.add.at(num, owner, np.tile(np.array([9, 1], np.int64), len(idx)) * mv)
        leaves = np.zeros(m, np.int64)
        np.add.at(leaves, owner, lv.sum(1))
        return num // (10 * E), leaves  # the floor towards minus infinity

    q, lv = expand(boards, depth)
    ok = q != I64_MIN
    legal = (ok * (1 << np.arange(4))).sum(1).astype(np.uint8)
    assert np.array_equal(legal, O.legal_mask(boards))
    best = np.where(ok.any(1), q.argmax(1), 0xFF).astype(np.uint8)
    if stats is not None:
        stats.update(leaves=seen["leaves"], leaf_stages=sorted(seen["leaf_stages"]))
    return q, lv, legal, best


def cpu_play(cells, weights, depth, seeds, max_moves, smap=0):
    """NTuplePlayer(net, depth).play_games(len(seeds), max_moves, seeds=seeds), the games of `play-ntuple`, with
    the oracle: game i spawns like random.seed(seeds[i]).  Every game must still be running at its last move
    (the caller picks max_moves so).  -> (scores, boards)."""
    mt = O.MTStates(seeds)
    boards = O.reset(len(seeds), O.RNG_MT, mt=mt)
    scores = np.zeros(len(seeds), np.int64)
    for _ in range(max_moves):
        assert (O.legal_mask(boards) != 0).all()
        best = search_ref(cells, weights, boards, depth, smap)[3]
        boards, f, _, _ = O.step(boards, best, O.RNG_MT, mt=mt)
        scores += f["points"]
    return scores, boards


# ------------------------------------------------------------------------------ the learner cases -----
def random_staged_weights(cells, smap, seed, bits=32):
    """int32 [G, T, 16^K]: R.random_weights with the seed `seed` + g for stage g."""
    return np.stack([R.random_weights(cells, seed + g, bits) for g in range(num_stages(smap))])


def start(rule, name, fill, smap):
    """-> (cells, weights [G, T, 16^K], boards, lr_shift, tc or None): the start of R.td_start / C.tc_start for the
    staged shape.  Zero weights stay zero in every stage, random ones (22 bits) are drawn per stage under the
    seeds 7, 8, ..; prefilled accumulators are C.prefilled drawn for the staged shape."""
    G = num_stages(smap)
    cells, w, boards, lr_shift = R.td_start(name)
    if R.TD_CASES[name][3]:
        w = np.stack([R.random_weights(cells, 7 + g, bits=22) for g in range(G)])
    else:
        w = np.zeros((G,) + w.shape, np.int32)
    tc = None
    if rule == "tc":
        lr_shift = C.TC_LR[name]
        tc = C.prefilled(w.shape) if fill == "prefilled" else np.zeros(w.shape + (2,), np.int64)
    return cells, w, boards, lr_shift, tc


def run(rule, name, fill, h, s, steps, smap, n=None, seed=LR.SEED, events=None):
    cells, w, boards, lr_shift, tc = start(rule, name, fill, smap)
    st = td_stage(LR.LState(cells, w, boards[:n], h), tc, steps, lr_shift, s, seed, 1, smap, events=events)
    return st, tc


@functools.lru_cache(maxsize=None)
def ref_case(rule, name, fill, h, s, stages=STAGES, seed=LR.SEED):
    """-> (LState, tc or None, events) after STEPS steps of a case: computed once per process, read-only."""
    ev = {}
    st, tc = run(rule, name, fill, h, s, STEPS, stage_map_of(stages), seed=seed, events=ev)
    for a in (st.weights, st.boards, st.after, st.hist, st.hist_len, st.pending, st.run_score, st.stats) + \
            (() if tc is None else (tc,)):
        a.setflags(write=False)
    return st, tc, ev


def covers(ev, h):
    """What a staged case must show on the reference before a device result is compared with it."""
    assert all(u > 0 for u in ev["stage_updates"]), ev
    assert ev["cross_stage"] > 0 and ev["terminal_high"] > 0, ev
    if h > 0:
        assert ev["trace_cross"] > 0 and ev["traced"] > 0, ev


# ----------------------------------------------------------------------------------- the trainer -----
class TrainerRef:
    """NTupleTrainer on a staged net with promote_every P: `envs` Philox games under `seed` from the reset at
    counter 0, step s at counter 1 + s; the step sequence is cut at every multiple of P steps since the
    start, and at a cut the stages promoted_upto + 1 .. (the highest stage of a board) are promoted, g - 1 ->
    g in ascending order."""

    def __init__(self, cells, stages, envs=64, lr_shift=10, seed=0x2048, rule="td", h=0, s=1, promote_every=0):
        self.smap = stage_map_of(stages)
        G, T, size = num_stages(self.smap), len(cells), 16 ** len(cells[0])
        self.st = LR.LState(cells, np.zeros((G, T, size), np.int32), O.reset(envs, seed=seed, step_idx=0), h)
        self.tc = np.zeros((G, T, size, 2), np.int64) if rule == "tc" else None
        self.lr_shift, self.seed, self.s, self.P = lr_shift, seed, s, promote_every
        self.done, self.promoted_upto, self.promoted = 0, 0, []
        self.onto_nonzero = 0  # promotions that landed on a stage that had already learned

    def train(self, steps):
        """-> the stages promoted during these steps."""
        out = []
        while steps > 0:
            k = min(steps, self.P - self.done % self.P) if self.P > 0 else steps
            td_stage(self.st, self.tc, k, self.lr_shift, self.s, self.seed, 1 + self.done, self.smap)
            self.done += k
            steps -= k
            if self.P > 0 and self.done % self.P == 0:
                top = int(stage(self.smap, self.st.boards).max())
                for g in range(self.promoted_upto + 1, top + 1):
                    self.onto_nonzero += int((self.st.weights[g] != 0).any())
                    promote(self.st.weights, self.smap, g - 1, g)
                    out.append(g)
                self.promoted_upto = max(self.promoted_upto, top)
        self.promoted += out
        return out
