"""CPU reference of the carousel step of the staged n-tuple trainer (Carousel of include/g2048_ntuple.h,
g2048_ntuple_staged_carousel), in numpy on tests/ntuple_stage_reference.py: a carousel step is one step of
SG.td_stage (steps 1, 2, 3a and 4, unchanged) with what that step's env step returned (points, DONE) looked at
once more for 3b and 3c.  td_stage accounts every finished game as a full one; this module takes that back and
accounts the game by its origin.  The carried state is SG's LState with stats int64 [8] and pool int8 [G, n, 16],
valid uint8 [n, 16], next / origin uint8 [n].  Shared by tests/test_ntuple_carousel_host.py and
tests/test_gpu_ntuple_carousel.py; not a test module itself."""

import contextlib
import functools

import numpy as np

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_stage_reference as SG
from oracle import oracle as O

M64 = (1 << 64) - 1
STEPS = 200
FULL = tuple(1 << m for m in range(1, 16))  # a stage per exponent: G = 16
EVENTS = ("fell_through", "fell_to_reset", "wrapped", "self_donor", "same_step", "restart_ended")


class CState(LR.LState):
    """LR.LState with stats int64 [8] and the carousel's carried arrays for G stages, zero-filled unless given."""

    def __init__(self, cells, weights, boards, h, G, pool=None, valid=None, next=None, origin=None, stats=None, **kw):
        super().__init__(cells, weights, boards, h, stats=np.zeros(8, np.int64) if stats is None else stats, **kw)
        n = len(self.boards)
        assert self.stats.shape == (8,)
        self.G = int(G)
        self.pool = np.zeros((self.G, n, 16), np.int8) if pool is None else np.array(pool, np.int8).reshape(self.G, n, 16)
        self.valid = np.zeros((n, 16), np.uint8) if valid is None else np.array(valid, np.uint8).reshape(n, 16)
        self.next = np.zeros(n, np.uint8) if next is None else np.array(next, np.uint8)
        self.origin = np.zeros(n, np.uint8) if origin is None else np.array(origin, np.uint8)


def donors(n, ctr):
    """j[i] = (i + ctr) mod n, the sum modulo 2^64: int64 [n]."""
    return np.array([((i + (int(ctr) & M64)) & M64) % n for i in range(n)], np.int64)


def select(valid, next, j, G):
    """The start stage of step 3c for every env, as if its game ended now -> (k, g) int64 [n]: k = next if next <
    G else 0; g = the smallest g' in max(k, 1) .. G - 1 with valid[j][g'] != 0 if k >= 1 and there is one, else 0."""
    k = np.where(np.asarray(next, np.int64) < G, np.asarray(next, np.int64), 0)
    col = np.arange(16)[None, :]
    cand = (np.asarray(valid)[j] != 0) & (col >= np.maximum(k, 1)[:, None]) & (col < G)
    g = np.where((k >= 1) & cand.any(1), cand.argmax(1), 0)
    return k, g


@contextlib.contextmanager
def _env_steps_seen():
    """While open, what R.env_step_auto_reset returns is also appended to the list this yields: td_stage keeps the
    points and DONE of its env step to itself."""
    seen, real = [], R.env_step_auto_reset

    def tap(*a, **kw):
        out = real(*a, **kw)
        seen.append(out)
        return out

    R.env_step_auto_reset = tap
    try:
        yield seen
    finally:
        R.env_step_auto_reset = real


def td_carousel(st: CState, tc, steps, lr_shift, s, seed, counter, smap=0, events=None, stage_events=None):
    """`steps` carousel steps on st (and tc under rule TC), in place.  events (optional dict) counts, beside the
    lists "recorded" and "served" (snapshots and restarts per stage): "fell_through" (restarts where valid[j][k]
    was 0 and a later stage was taken), "fell_to_reset" (k >= 1 but g = 0), "wrapped" (next going from G - 1 to
    0), "self_donor" (restarts with j == i from a snapshot env i recorded itself in this run), "same_step" (games
    ending with a donor j != i that records in the same step a stage the choice looks at: reading the new flags
    or board would change what the env gets), "restart_ended" (games with origin > 0 that finished).
    stage_events (optional dict) is handed to SG.td_stage as its events ("stage_updates" and the others)."""
    n, G = len(st.boards), SG.num_stages(smap)
    assert G == st.G and st.pool.shape == (G, n, 16)
    ev = dict.fromkeys(EVENTS, 0)
    rec_n, srv_n = np.zeros(G, np.int64), np.zeros(G, np.int64)
    own = getattr(st, "_own", None)
    if own is None:
        own = st._own = np.zeros((n, 16), bool)  # (i, g): env i recorded pool[g][i] itself
    idx = np.arange(n)
    for t in range(steps):
        before, rs, head = st.boards.copy(), st.run_score.copy(), st.stats[:3].copy()
        j = donors(n, counter + t)
        k, g = select(st.valid, st.next, j, G)                      # before this step's writes
        donor_board = st.pool[g, j].copy()
        with _env_steps_seen() as seen:
            SG.td_stage(st, tc, 1, lr_shift, s, seed, counter + t, smap, events=stage_events)
        (_, pts, done), = seen
        st.stats[:3] = head                                          # td_stage counted every game as a full one
        # 3b
        sb, sa = SG.stage(smap, before).astype(np.int64), SG.stage(smap, st.boards).astype(np.int64)
        rec = ~done & (sa != sb)
        assert (sa[rec] > sb[rec]).all()
        # 3c
        fin = rs + pts
        full, part = done & (st.origin == 0), done & (st.origin != 0)
        if full.any():
            st.stats[0] += int(full.sum())
            st.stats[1] += int(fin[full].sum())
            st.stats[2] = max(int(st.stats[2]), int(fin[full].max()))
        st.stats[4] += int(part.sum())
        st.stats[5] += int(fin[part].sum())
        assert (st.run_score[done] == 0).all() and np.array_equal(st.run_score[~done], fin[~done])
        served = done & (g >= 1)
        ev["restart_ended"] += int(part.sum())
        ev["fell_through"] += int((served & (st.valid[j, k] == 0)).sum())
        ev["fell_to_reset"] += int((done & (k >= 1) & (g == 0)).sum())
        ev["wrapped"] += int((done & (k == G - 1) & (g == G - 1) & (G > 1)).sum())
        ev["self_donor"] += int((served & (j == idx) & own[idx, g]).sum())
        lo = np.maximum(k, 1)
        ev["same_step"] += int((done & (k >= 1) & (j != idx) & rec[j] & (sa[j] >= lo) & ((g == 0) | (sa[j] <= g))).sum())
        np.add.at(srv_n, g[served], 1)
        np.add.at(rec_n, sa[rec], 1)
        st.boards[served] = donor_board[served]
        st.stats[7] += int(served.sum())
        st.origin[done] = g[done]
        st.next[done] = (g[done] + 1) % G
        st.pool[sa[rec], idx[rec]] = st.boards[rec]
        st.valid[idx[rec], sa[rec]] = 1
        own[idx[rec], sa[rec]] = True
        st.stats[6] += int(rec.sum())
    if events is not None:
        for key, v in ev.items():
            events[key] = events.get(key, 0) + v
        events["recorded"] = (np.array(events.get("recorded", [0] * G), np.int64) + rec_n).tolist()
        events["served"] = (np.array(events.get("served", [0] * G), np.int64) + srv_n).tolist()
    return st


# ------------------------------------------------------------------------------------- the cases -----
def top_exponent(smap, g):
    """The largest exponent whose stage is g."""
    return max(m for m, v in enumerate(SG.nibbles(smap)) if v == g)


def stage_board(smap, g, rng, dead=False):
    """A board of stage g >= 1, m the stage's largest exponent.  Live: two neighbouring tiles m in the top row (their
    merge enters the next stage), exponents 1..min(m, 3) on two thirds of the other cells.  Dead (m >= 2): m and m - 1
    in a chequerboard, so that a game restarted from it ends at once; with m = 1 there is no dead board, and a
    live one is returned."""
    m = top_exponent(smap, g)
    if dead and m >= 2:
        b = np.where((np.arange(16) + np.arange(16) // 4) % 2 == 0, m, m - 1).astype(np.int8)
        assert O.legal_mask(b[None])[0] == 0 and SG.stage(smap, b[None])[0] == g
        return b
    b = rng.integers(1, min(m, 3) + 1, size=16).astype(np.int8)
    b[rng.random(16) < 0.34] = 0
    b[0] = b[1] = m
    assert SG.stage(smap, b[None])[0] == g
    return b


def prefill(smap, n, seed, dead_every=3):
    """-> (pool, valid, next) of the cases' start: next[i] = i mod G; about half of the (slot, stage) pairs hold a
    board of their stage, drawn by default_rng(seed); every third filled pair holds a dead one."""
    G = SG.num_stages(smap)
    rng = np.random.default_rng(seed)
    pool, valid = np.zeros((G, n, 16), np.int8), np.zeros((n, 16), np.uint8)
    filled = 0
    for i in range(n):
        for g in range(1, G):
            if rng.random() < 0.5:
                pool[g, i] = stage_board(smap, g, rng, dead=filled % dead_every == 1)
                valid[i, g] = 1
                filled += 1
    return pool, valid, (np.arange(n) % G).astype(np.uint8)


# (rule, case of SG.start, accumulators, trace_len h, lambda_shift s, stages, first counter, prefill seed, steps)
# The first counter of a case puts a multiple of n among the counters of its steps, so that a step with j == i for
# every env (self_donor) is among them.  Counter and prefill seed were picked on the CPU, reference alone, as the
# first of a short list (counters 1 / 30 / 50 at n = 64 and 150 / 200 / 250 / .. at n = 300, prefill seeds from 11
# up) under which the case shows every event of covers(): self_donor and same_step are rare (an env whose game
# ends in one of the steps with j == i; a donor that enters a stage in the very step its reader's game ends) and
# most picks show one of the two, not both.  n64-tc-zero plays best and ends the fewest games (some 60 in its 200
# steps): one pick of the 270 tried (3 counters x prefill seeds 11..100) shows both.  n1-td runs 400 steps: the
# games of its one env take 40 to 160.
CASES = {
    "n1-td": ("td", "n1-random", None, 0, 1, SG.STAGES, 1, 11, 400),
    "n64-td": ("td", "n64-random", None, 0, 1, SG.STAGES, 1, 22, STEPS),
    "n300-td": ("td", "n300-zero", None, 0, 1, SG.STAGES, 200, 16, STEPS),
    "n64-td-trace": ("td", "n64-random", None, 3, 1, SG.STAGES, 1, 22, STEPS),
    "n64-tc-zero": ("tc", "n64-zero", "zero", 0, 1, SG.STAGES, 50, 92, STEPS),
    "n300-tc-prefilled-trace": ("tc", "n300-random", "prefilled", 3, 1, SG.STAGES, 150, 11, STEPS),
    "n64-t8k3": ("td", "n64-t8k3", None, 0, 1, SG.STAGES, 1, 12, STEPS),
    "n64-sixteen": ("td", "n64-zero", None, 0, 1, FULL, 1, 12, STEPS),
}
# The game seed of a case where LR.SEED does not show what covers() asks for.  n1-td: under seeds 31 and 33..50 its
# env either never enters stage 3 within 400 steps or its next never comes round to 3; under 32 it does both.
SEEDS = {"n1-td": 32}
# What a case cannot show, by name (covers()).
#   n1-td: its one env is its own donor in every step, so no other env's slot is ever read (same_step).  The flags of
#     a slot are never cleared and the env that owns it enters the stages in ascending order, so its slot never
#     holds a later stage without the wanted one (fell_through).  fell_to_reset needs next at a stage the slot does
#     not hold yet; in a run that also serves every stage next would have to come round twice, eight games, and a
#     game of this env takes 40 to 160 steps: not within 400.
#   n64-sixteen: with a stage per exponent the reset board (tiles 2 and 4) is already in stage 1 or 2; no game ever
#     enters stage 1, so it is never recorded: the header's own example.  The prefilled slots still serve it.
EXCUSED = {
    "n1-td": ("same_step", "fell_through", "fell_to_reset"),
    "n64-sixteen": ("recorded[1]",),
}


def start(case):
    """-> (CState, tc or None, lr_shift, s, smap, counter) of a case."""
    rule, name, fill, h, s, stages, counter, fill_seed, _ = CASES[case]
    smap = SG.stage_map_of(stages)
    cells, w, boards, lr_shift, tc = SG.start(rule, name, fill, smap)
    pool, valid, nxt = prefill(smap, len(boards), fill_seed)
    st = CState(cells, w, boards, h, SG.num_stages(smap), pool=pool, valid=valid, next=nxt)
    return st, tc, lr_shift, s, smap, counter


def seed_of(case):
    return SEEDS.get(case, LR.SEED)


def steps_of(case):
    return CASES[case][8]


def run(case, splits=None, events=None):
    st, tc, lr_shift, s, smap, counter = start(case)
    for k in splits or (steps_of(case),):
        td_carousel(st, tc, k, lr_shift, s, seed_of(case), counter, smap, events=events)
        counter += k
    return st, tc


ARRAYS = ("weights", "boards", "after", "hist", "hist_len", "pending", "run_score", "stats", "pool", "valid", "next",
          "origin")


@functools.lru_cache(maxsize=None)
def ref_case(case):
    """-> (CState, tc or None, events) after the steps_of(case) steps of a case: computed once per process, read-only."""
    ev = {}
    st, tc = run(case, events=ev)
    for a in tuple(getattr(st, k) for k in ARRAYS) + (() if tc is None else (tc,)):
        a.setflags(write=False)
    return st, tc, ev


def covers(case, ev):
    """What a case must show on the reference before a device result is compared with it."""
    skip = EXCUSED.get(case, ())
    G = len(ev["recorded"])
    for g in range(1, G):
        assert f"recorded[{g}]" in skip or ev["recorded"][g] > 0, (case, g, ev)
        assert f"served[{g}]" in skip or ev["served"][g] > 0, (case, g, ev)
    for key in EVENTS:
        assert key in skip or ev[key] > 0, (case, key, ev)


# ----------------------------------------------------------------------------------- the trainer -----
class TrainerRef(SG.TrainerRef):
    """NTupleTrainer(carousel=True): SG.TrainerRef with the carousel step in the place of td_stage, the carried
    arrays zero at the start."""

    def __init__(self, cells, stages, envs=64, **kw):
        super().__init__(cells, stages, envs=envs, **kw)
        old = self.st
        self.st = CState(old.cells, old.weights, old.boards, old.h, SG.num_stages(self.smap))
        self.events = {}

    def train(self, steps):
        out = []
        while steps > 0:
            k = min(steps, self.P - self.done % self.P) if self.P > 0 else steps
            td_carousel(self.st, self.tc, k, self.lr_shift, self.s, self.seed, 1 + self.done, self.smap, events=self.events)
            self.done += k
            steps -= k
            if self.P > 0 and self.done % self.P == 0:
                top = int(SG.stage(self.smap, self.st.boards).max())
                for g in range(self.promoted_upto + 1, top + 1):
                    SG.promote(self.st.weights, self.smap, g - 1, g)
                    out.append(g)
                self.promoted_upto = max(self.promoted_upto, top)
        self.promoted += out
        return out
