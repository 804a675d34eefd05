"""CPU reference of optimistic initialisation and of the resumable trainer (Optimistic initialisation of
include/g2048_ntuple.h: g2048_ntuple_fill, g2048_ntuple_promote_from; NTupleNet(v_init=...), NTupleTrainer.save /
load), in numpy on tests/ntuple_stage_reference.py and tests/ntuple_carousel_reference.py.  Those references run
every learner from any start weights, so no learning rule is restated here: a filled net is np.full(w0), and the
trainer is theirs with that start and the promotion over it.  Shared by tests/test_ntuple_optimistic_host.py and
tests/test_gpu_ntuple_optimistic.py; not a test module itself."""

import numpy as np

import ntuple_carousel_reference as CR
import ntuple_lambda_reference as LR
import ntuple_stage_reference as SG

S = SG.S
W0_MAX = 1 << 30
CARRIED = ("boards", "after", "pending", "run_score", "tc", "hist", "hist_len", "pool", "valid", "next_stage", "origin")


def w0_of(v_init, T):
    """The start of every weight for v_init points on T tuples: v_init S / (8 T) rounded to nearest (halves up)."""
    assert v_init >= 0 and 1 <= T <= 8
    w0 = (v_init * S + 4 * T) // (8 * T)
    assert w0 <= W0_MAX
    return w0


def promote_from(weights, smap, src, dst, base):
    """W[dst] += W[src] - base in place: int64 arithmetic, wrapped to int32; weights int32 [G, T, 16^K]."""
    G = SG.num_stages(smap)
    assert weights.dtype == np.int32 and weights.shape[0] == G and 0 <= src < G and 0 <= dst < G and src != dst
    assert -2 ** 31 <= base < 2 ** 31
    wide = weights[dst].astype(np.int64) + weights[src].astype(np.int64) - int(base)
    weights[dst] = ((wide + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


class TrainerRef(CR.TrainerRef, SG.TrainerRef):
    """NTupleTrainer on NTupleNet(v_init=...): SG.TrainerRef (carousel: CR.TrainerRef) with every weight at w0 at the
    start and promote_from(.., base = w0) at the cuts.  train() runs one segment and returns what the device's
    train() returns for it; st.stats holds the statistics of the last segment alone, as the device's stats do.
    state() is everything a checkpoint carries, to be compared field by field."""

    def __init__(self, cells, stages, envs=64, w0=0, carousel=False, rule="td", **kw):
        SG.TrainerRef.__init__(self, cells, stages, envs=envs, rule=rule, **kw)
        self.w0, self.carousel, self.rule = int(w0), bool(carousel), rule
        self.st.weights[...] = self.w0
        if self.carousel:
            old = self.st
            self.st = CR.CState(old.cells, old.weights, old.boards, old.h, SG.num_stages(self.smap))
        self.events, self.stage_events = {}, {}
        self.onto_learned = 0  # promotions that landed on a stage that already differed from w0

    def switch_rule(self, rule):
        """What loading a checkpoint with another rule does: "tc" starts zero accumulators, "td" drops them."""
        assert rule in ("td", "tc")
        if rule == "tc" and self.rule != "tc":
            self.tc = np.zeros(self.st.weights.shape + (2,), np.int64)
        if rule == "td":
            self.tc = None
        self.rule = rule

    def train(self, steps):
        out = []
        self.st.stats[...] = 0
        while steps > 0:
            k = min(steps, self.P - self.done % self.P) if self.P > 0 else steps
            if self.carousel:
                CR.td_carousel(self.st, self.tc, k, self.lr_shift, self.s, self.seed, 1 + self.done, self.smap,
                               events=self.events, stage_events=self.stage_events)
            else:
                SG.td_stage(self.st, self.tc, k, self.lr_shift, self.s, self.seed, 1 + self.done, self.smap,
                            events=self.stage_events)
            self.done += k
            steps -= k
            if self.P > 0 and self.done % self.P == 0:
                top = int(SG.stage(self.smap, self.st.boards).max())
                for g in range(self.promoted_upto + 1, top + 1):
                    self.onto_learned += int((self.st.weights[g] != self.w0).any())
                    promote_from(self.st.weights, self.smap, g - 1, g, self.w0)
                    out.append(g)
                self.promoted_upto = max(self.promoted_upto, top)
        self.promoted += out
        games, score_sum, best, updates, *car = (int(v) for v in self.st.stats)
        res = {"games": games, "mean_score": score_sum / games if games else 0.0, "max_score": best,
               "updates": updates, "score_sum": score_sum, "promoted": out}
        if self.carousel:
            res.update(zip(("restart_games", "restart_points", "recorded", "restarts"), car))
        return res

    def state(self):
        """-> dict: counter, promoted_upto, weights and every carried array under the trainer's names; hist with
        the rows at or beyond hist_len zeroed (LR.valid_hist: they hold nothing)."""
        st = self.st
        out = {"counter": 1 + self.done, "promoted_upto": self.promoted_upto, "weights": st.weights,
               "boards": st.boards, "after": st.after, "pending": st.pending, "run_score": st.run_score}
        if self.tc is not None:
            out["tc"] = self.tc
        if st.h > 0:
            out["hist"], out["hist_len"] = LR.valid_hist(st.hist, st.hist_len), st.hist_len
        if self.carousel:
            out.update(pool=st.pool, valid=st.valid, next_stage=st.next, origin=st.origin)
        return out
