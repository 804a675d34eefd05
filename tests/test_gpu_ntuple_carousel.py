"""The carousel of the staged n-tuple trainer on the GPU (Carousel of include/g2048_ntuple.h: nt_car_choose in
nt_td_eval_kernel, the snapshot and the restart in nt_step_env of nt_update_kernel, csrc/ntuple.hip;
NTupleTrainer(carousel=True), train-ntuple --carousel), bit for bit against the numpy reference of
tests/ntuple_carousel_reference.py: the weights, the accumulators, every carried array and all eight stats, hist
through LR.valid_hist.  Nothing here has a tolerance.

The cases (ntuple_carousel_reference.CASES) start from SG.start's weights and boards with next[i] = i mod G and a
pool filled for about half of its (slot, stage) pairs, a third of those with dead boards, and run 200 steps (n1-td: 400) with
the workspace filled with garbage.  Before a device result is compared, the reference run of the case must have
recorded and served every stage and shown a fall-through, a fall to the reset, a wrap of next, a self-donor, a
slot written in the step that reads it and the end of a restarted game: ntuple_carousel_reference.covers, with
what a case cannot show excused there by name."""

import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ntuple_carousel_reference as CR
import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_stage_reference as SG
from conftest import PKG

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A
CARRIED = ("boards", "after", "hist", "hist_len", "pending", "run_score", "stats", "pool", "valid", "next", "origin")
TRAIN_P, TRAIN_STEPS, TRAIN_PRINT = 40, 300, 100
# 64 envs at lr_shift 5 overshoot (the header's Range note) and play short games: an env's second game ends, and so
# restarts from every stage happen, within 300 steps; at the default 10 the first restart comes after step 300.
TRAIN_LR = 5


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


class Run:
    """The device state of one carousel run, from a CState (and tc) of the reference."""

    def __init__(self, dev, st, tc, smap):
        self.h = st.h
        self.w = to_dev(st.weights, dev)
        self.net = L().make_ntuple_net(st.cells, self.w, smap) if smap else L().NtStagedNet(
            L().make_ntuple_net(st.cells, self.w, 0), 0)
        self.tc = None if tc is None else to_dev(tc, dev)
        for k in CARRIED:
            a = getattr(st, k)
            setattr(self, k, to_dev(a, dev) if a.size else None)
        n = len(st.boards)
        self.ws = torch.empty(L().ntuple_carousel_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.lam_ws = torch.empty(L().ntuple_lambda_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def call(self, steps, lr_shift, s, counter, seed=LR.SEED, carousel=True):
        rng = L().make_rng(L().RNG_PHILOX, seed, counter)
        if carousel:
            self.ws.fill_(GARBAGE)
            L().ntuple_carousel(self.net, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                                self.run_score, steps, lr_shift, self.h, s, rng, self.pool, self.valid, self.next,
                                self.origin, self.stats, self.ws)
        else:
            self.lam_ws.fill_(GARBAGE)
            L().ntuple_lambda(self.net, self.tc, self.boards, self.after, self.hist, self.hist_len, self.pending,
                              self.run_score, steps, lr_shift, self.h, s, rng, self.stats[:4], self.lam_ws)

    def results(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in CARRIED if getattr(self, k) is not None}
        out["weights"] = self.w.cpu().numpy()
        if self.tc is not None:
            out["tc"] = self.tc.cpu().numpy()
        if self.h > 0:
            out["hist"] = LR.valid_hist(out["hist"], out["hist_len"])
        return out


def expected(st, tc):
    want = {k: getattr(st, k) for k in CARRIED + ("weights",) if getattr(st, k).size}
    if tc is not None:
        want["tc"] = tc
    if st.h > 0:
        want["hist"] = LR.valid_hist(st.hist, st.hist_len)
    else:
        want.pop("hist_len", None)
    return want


def assert_equal(got, st, tc):
    want = expected(st, tc)
    if st.h == 0:
        got = {k: v for k, v in got.items() if k != "hist_len"}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


def device_run(dev, case, splits):
    st, tc, lr_shift, s, smap, counter = CR.start(case)
    if st.h == 0:
        st.hist_len = np.zeros(0, np.uint8)
    run = Run(dev, st, tc, smap)
    for steps in splits:
        run.call(steps, lr_shift, s, counter, CR.seed_of(case))
        counter += steps
    return run.results()


@pytest.mark.parametrize("case", sorted(CR.CASES))
def test_carousel_bit_exact(dev, case):
    st, tc, ev = CR.ref_case(case)
    CR.covers(case, ev)
    assert_equal(device_run(dev, case, [CR.steps_of(case)]), st, tc)


@pytest.mark.parametrize("case", ["n64-td", "n300-tc-prefilled-trace"])
def test_continuation(dev, case):
    """120 + 80 steps, the counter advanced by 120, equal 200."""
    st, tc, _ = CR.ref_case(case)
    one = device_run(dev, case, [200])
    two = device_run(dev, case, [120, 80])
    assert sorted(one) == sorted(two) and all(one[k].tobytes() == two[k].tobytes() for k in one)
    assert_equal(two, st, tc)


@pytest.mark.parametrize("rule,name,fill,h", [("td", "n64-random", None, 3), ("tc", "n300-random", "zero", 0)])
def test_map_zero_is_the_staged_lambda_call(dev, rule, name, fill, h):
    """stage_map == 0: g2048_ntuple_staged_carousel and g2048_ntuple_staged_lambda leave the same bytes in the
    weights, tc, every carried array and stats[0..3]; nothing is recorded or restarted."""
    outs = []
    for carousel in (True, False):
        cells, w, boards, lr_shift, tc = SG.start(rule, name, fill, 0)
        st = CR.CState(cells, w, boards, h, 1)
        if h == 0:
            st.hist_len = np.zeros(0, np.uint8)
        run = Run(dev, st, tc, 0)
        run.call(SG.STEPS, lr_shift, 1, 1, carousel=carousel)
        outs.append(run.results())
    car, lam = outs
    assert sorted(car) == sorted(lam)
    for k in car:
        assert car[k].tobytes() == lam[k].tobytes(), k
    assert car["stats"][0] > 0 and car["stats"][3] > 0 and not car["stats"][4:].any()
    assert not car["pool"].any() and not car["valid"].any() and not car["next"].any() and not car["origin"].any()
    assert (car["weights"] != SG.start(rule, name, fill, 0)[1]).any()


# -------------------------------------------------------------------------- trainer and command -----
@pytest.fixture(scope="module")
def trainer_ref():
    tr = CR.TrainerRef(R.PRESETS["lines-squares-4"], SG.STAGES, envs=64, lr_shift=TRAIN_LR, promote_every=TRAIN_P)
    per_interval = []
    for _ in range(TRAIN_STEPS // TRAIN_PRINT):
        before = tr.st.stats.copy()
        tr.train(TRAIN_PRINT)
        per_interval.append((tr.st.stats - before)[4:].tolist())
    assert len(tr.promoted) >= 2 and tr.st.stats[4] > 0 and all(v > 0 for v in tr.events["served"][1:]), tr.st.stats
    return tr, per_interval


def test_trainer(dev, trainer_ref):
    """NTupleTrainer(carousel=True, promote_every=40), 64 envs from the reset and an empty pool, 300 steps in uneven
    chunks: the weights, the boards, the pool and what train() returns are the reference trainer's."""
    from g2048.ntuple import NTupleNet, NTupleTrainer
    ref, _ = trainer_ref
    net = NTupleNet("lines-squares-4", dev, stages=SG.STAGES)
    tr = NTupleTrainer(net, envs=64, lr_shift=TRAIN_LR, promote_every=TRAIN_P, carousel=True)
    outs = [tr.train(k) for k in (130, 170)]
    torch.cuda.synchronize()
    assert np.array_equal(net.weights.cpu().numpy(), ref.st.weights)
    for k, dev_k in (("boards", "boards"), ("pool", "pool"), ("valid", "valid"), ("next", "next_stage"),
                     ("origin", "origin"), ("run_score", "run_score")):
        assert np.array_equal(getattr(tr, dev_k).cpu().numpy(), getattr(ref.st, k)), k
    assert sum((o["promoted"] for o in outs), []) == ref.promoted
    for i, key in ((0, "games"), (1, "score_sum"), (3, "updates"), (4, "restart_games"), (5, "restart_points"),
                   (6, "recorded"), (7, "restarts")):
        assert sum(o[key] for o in outs) == ref.st.stats[i], key
    assert max(o["max_score"] for o in outs) == ref.st.stats[2]
    plain = NTupleTrainer(NTupleNet("lines-squares-4", dev, stages=SG.STAGES), envs=64, promote_every=TRAIN_P)
    out = plain.train(TRAIN_STEPS)
    assert sorted(out) == ["games", "max_score", "mean_score", "promoted", "score_sum", "updates"]
    assert plain.stats.numel() == 4 and plain.pool is None


def test_command(dev, tmp_path, trainer_ref):
    """`train-ntuple --stages 16,64,128 --promote-every 40 --carousel --envs 64 --steps 300 --print-freq 100` prints the
    reference's restart counters interval by interval and saves its weights; --carousel without --stages is refused."""
    ref, per_interval = trainer_ref
    out = tmp_path / "net.pt"
    base = [sys.executable, str(PKG / "train.py"), "train-ntuple"]
    cmd = base + ["--stages", "16,64,128", "--promote-every", str(TRAIN_P), "--carousel", "--envs", "64", "--lr-shift", str(TRAIN_LR), "--steps",
                  str(TRAIN_STEPS), "--print-freq", str(TRAIN_PRINT), "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    found = re.findall(r"restarts (\d+) \(recorded (\d+), restarted games (\d+), their points (\d+)\)", r.stdout)
    want = [(str(s[3]), str(s[2]), str(s[0]), str(s[1])) for s in per_interval]
    assert found == want, r.stdout[-3000:]
    assert any(ln.startswith("n-tuple net") and ln.endswith(", carousel") for ln in r.stdout.splitlines())
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert np.array_equal(ck["weights"].numpy(), ref.st.weights) and sorted(ck) == ["cells", "stages", "weights"]
    r = subprocess.run(base + ["--steps", "10", "--carousel"], cwd=tmp_path, capture_output=True, text=True, timeout=170)
    assert r.returncode != 0 and "--carousel needs --stages" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
