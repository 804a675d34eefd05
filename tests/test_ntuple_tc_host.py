"""CPU-side checks of temporal-coherence learning on the n-tuple network (the TC step of
include/g2048_ntuple.h): the rule on hand-made accumulator records, worked out by hand; the numpy
reference (tests/ntuple_tc_reference.py) against a scalar implementation in Python ints written from
the header; what the rule promises (zero accumulators give TD(0) for the first hit of every weight, D =
0 changes nothing, a self-symmetric tuple's double hit reads one record and adds twice); the pinned
counts of the events the GPU tests rely on; and the seams (the C ABI declaration and export, the
wrapper's checks, the trainer's and the command's `rule`).

Pinned on the reference (TC_STEPS = 200 steps, game seed 31): see PINNED below."""

import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import ntuple_reference as R
import ntuple_tc_reference as C
import test_ntuple_host as H  # the scalar value / choice / move in Python ints
from conftest import ROOT
from oracle import oracle as O

I64_MIN = -(1 << 63)


# ---- the rule in Python ints, one record at a time, written from the header ----
def scalar_share(E, A, D):
    """add_i for E in [-2^63, 2^63), A in [0, 2^64), |D| <= 2^30."""
    if A == 0:
        return D
    sh = max(A.bit_length() - 20, 0)
    a = A >> sh
    e = min(abs(E) >> sh, a)
    q = (abs(D) * e + (a >> 1)) // a
    return q if D > 0 else -q


def _wrap(x, bits):
    return (x + (1 << (bits - 1))) % (1 << bits) - (1 << (bits - 1))


# (E, A, D) -> add, every expected value worked out by hand from the header
HAND = [
    ((0, 0, 5), 5), ((123, 0, -7), -7),                                  # A = 0: plain TD(0), whatever E holds
    ((1000, 1000, 12345), 12345), ((-1000, 1000, 12345), 12345),         # E = +-A: the full rate
    ((1000, 1000, -12345), -12345), ((-1000, 1000, -12345), -12345),
    ((0, 1000, 12345), 0), ((0, 1000, -(1 << 30)), 0),                   # E = 0: (0 + 500) // 1000
    ((500, 1000, 12345), 6173), ((500, 1000, -12345), -6173),            # 6172.5 + 0.5: half, away from zero
    ((5000, 1000, 77), 77), ((-5000, 1000, -77), -77),                   # |E| > A: the rate is clamped to 1
    # the shift boundary: A = 2^20 - 1 keeps every bit (a = A, e = 1: (2^21 + 524287) // 1048575 = 2),
    # A = 2^20 drops one (sh = 1, a = 2^19, e = 1 >> 1 = 0: 2^18 // 2^19 = 0)
    (((1, (1 << 20) - 1, 1 << 21)), 2), ((1, 1 << 20, 1 << 21), 0),
    ((1 << 19, (1 << 20) - 1, 1000), 500), ((1 << 19, 1 << 20, 1000), 500),  # (1001 x 2^18) // 2^19
    (((1 << 39), (1 << 40) + 12345, -999), -500),                        # sh = 21, a = 2^19, e = 2^18: 999 / 2 + 1 / 2
    ((1 << 62, 1 << 63, 1001), 501),                                     # A = 2^63: sh = 44, a = 2^19, e = 2^18
    ((I64_MIN, (1 << 64) - 1, -(1 << 30)), -((1 << 29) + 512)),          # |INT64_MIN| = 2^63; a = 2^20 - 1, e = 2^19
    ((I64_MIN, 1 << 63, 1 << 30), 1 << 30), ((I64_MIN, 1 << 63, -(1 << 30)), -(1 << 30)),  # D = +-2^30 at the full rate
    ((1 << 62, 1 << 62, 1 << 30), 1 << 30), ((3, 3, -(1 << 30)), -(1 << 30)),
    # the rounding: floor(x + 1/2) on the magnitude, so exactly half goes away from zero in both signs
    ((1, 2, 1), 1), ((1, 2, -1), -1), ((-1, 2, 1), 1), ((1, 4, 2), 1), ((1, 4, -2), -1),
    ((1, 4, 1), 0), ((1, 4, -1), 0),                                     # a quarter: to 0
    ((1, 3, 1), 0), ((2, 3, 1), 1), ((1, 3, 2), 1), ((1, 3, -2), -1),    # odd a: a >> 1 = 1; 1/3 -> 0, 2/3 -> 1
]


def test_rule_on_hand_made_records():
    for (E, A, D), want in HAND:
        assert scalar_share(E, A, D) == want, (E, A, D)
    E = np.array([h[0][0] for h in HAND], np.int64)
    A = np.array([h[0][1] for h in HAND], np.uint64)
    D = np.array([h[0][2] for h in HAND], np.int64)
    add, sh, clamped = C.tc_adds(E, A, D)
    assert add.tolist() == [h[1] for h in HAND]
    assert sh.tolist() == [a.bit_length() - 20 for a in A.tolist()]
    assert clamped.tolist() == [a != 0 and (abs(e) >> max(a.bit_length() - 20, 0)) > (a >> max(a.bit_length() - 20, 0))
                                for e, a in zip(E.tolist(), A.tolist())]
    assert clamped.sum() == 2


def test_rule_matches_scalar_on_random_records():
    """20 000 records of every magnitude up to 64 bits, the ends of D included; |add| <= |D| and the sign is D's."""
    rng = np.random.default_rng(3)
    n = 20000
    A = rng.integers(0, 1 << 64, n, dtype=np.uint64) >> rng.integers(0, 65, n).astype(np.uint64).clip(0, 63)
    A[rng.random(n) < 0.05] = 0
    E = rng.integers(-(1 << 63), 1 << 63, n, dtype=np.int64) >> rng.integers(0, 64, n)
    D = rng.integers(-(1 << 30), (1 << 30) + 1, n) >> rng.integers(0, 31, n)
    D[:4] = 1 << 30, -(1 << 30), 0, 1
    E[:2], A[:2] = I64_MIN, (1 << 64) - 1
    add, _, _ = C.tc_adds(E, A, D)
    assert add.tolist() == [scalar_share(e, a, d) for e, a, d in zip(E.tolist(), A.tolist(), D.tolist())]
    assert (np.abs(add) <= np.abs(D)).all() and (add * D >= 0).all() and (add[D == 0] == 0).all()
    assert C.bitlen(np.array([0, 1, 2, 3, (1 << 20) - 1, 1 << 20, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)).tolist() \
        == [0, 1, 2, 2, 20, 21, 63, 64, 64]


def scalar_tc(cells, w, E, A, boards, steps, lr_shift, seed, counter):
    """The TC step of the header, env by env, in Python ints; w, E, A: lists of lists, updated in place."""
    n = len(boards)
    boards = [tuple(int(x) for x in b) for b in boards]
    after, pending, run = [None] * n, [0] * n, [0] * n
    stats = [0, 0, 0, 0]
    for s in range(steps):
        adds, plan = [], []
        for i in range(n):  # every read sees W, E and A before the step's adds
            q, best = H.scalar_choose(cells, w, boards[i])
            target = q[best] if best != 0xFF else 0
            if pending[i]:
                delta = (0 if pending[i] == 2 else target) - H.scalar_value(cells, w, after[i])
                D = max(-(1 << 30), min(1 << 30, (delta + (1 << (lr_shift - 1))) >> lr_shift))
                adds += [(t, k, D, scalar_share(E[t][k], A[t][k], D)) for t, k in H.scalar_hits(cells, after[i])]
                stats[3] += 1
            plan.append(best)
        for t, k, D, add in adds:
            w[t][k] = _wrap(w[t][k] + add, 32)
            E[t][k] = _wrap(E[t][k] + D, 64)
            A[t][k] = (A[t][k] + abs(D)) % (1 << 64)
        acts = [0 if a == 0xFF else a for a in plan]
        nb, pts, done = R.env_step_auto_reset(np.array(boards, np.int8), np.array(acts), seed, counter + s)
        for i in range(n):
            run[i] += int(pts[i])
            if done[i]:
                stats[0] += 1
                stats[1] += run[i]
                stats[2] = max(stats[2], run[i])
                run[i] = 0
            if plan[i] != 0xFF:
                after[i] = H._move(boards[i], plan[i])[0]
                pending[i] = 2 if done[i] else 1
            else:
                pending[i] = 0
            boards[i] = tuple(int(x) for x in nb[i])
    return boards, after, pending, run, stats


@pytest.mark.parametrize("fill", ["zero", "prefilled"])
def test_reference_matches_scalar_tc(fill):
    """Six envs (ending, fresh, dead boards), 30 steps at lr_shift 4 on a small net (two 2-tuples, so that
    the few envs meet on weights and the accumulators grow past 20 bits), from zero and from prefilled
    accumulators."""
    cells = [[0, 1], [5, 6]]
    w0 = R.random_weights(cells, 5, bits=20)
    seed = 3
    boards = O.reset(6, seed=seed, step_idx=0)
    boards[0], boards[2], boards[5] = R.ENDING, R.ENDING, R.DEAD
    tc = C.prefilled(w0.shape) if fill == "prefilled" else np.zeros(w0.shape + (2,), np.int64)
    tc0 = tc.copy()
    ev = {}
    st = C.td_tc(R.TDState(cells, w0, boards), tc, 30, 4, seed=seed, counter=1, events=ev)
    assert ev["ended"] > 0 and ev["dead"] > 0 and ev["double"] > 0 and ev["shared"] > 0
    assert ev["damped"] > 0 and ev["shifted"] > 0 and (ev["fresh"] > 0 or fill == "prefilled")
    assert (ev["rate_clamped"] > 0 and ev["zeroed"] > 0) == (fill == "prefilled")
    w = [[int(x) for x in row] for row in w0]
    E = [[int(x) for x in row] for row in tc0[..., 0]]
    A = [[int(x) for x in row] for row in tc0[..., 1].view(np.uint64)]
    sb, sa, sp, sr, ss = scalar_tc(cells, w, E, A, boards, 30, 4, seed, 1)
    assert st.weights.tolist() == w
    assert tc[..., 0].tolist() == E and tc[..., 1].view(np.uint64).tolist() == A
    assert np.array_equal(st.boards, np.array(sb, np.int8)) and st.pending.tolist() == sp
    assert st.run_score.tolist() == sr and st.stats.tolist() == ss
    for i in range(6):
        if sp[i]:
            assert tuple(st.after[i]) == sa[i]


def test_zero_accumulators_start_as_td():
    """From zero accumulators the first hit of every weight is plain TD(0): one step from pending = 0
    updates nothing, and the second step -- every record it reads is still zero, a double hit's too --
    gives R.td's weights, with E = the sum of the D of those adds and A >= |E|.  Later steps differ: 20 do."""
    cells, w, boards, lr_shift, tc = C.tc_start("n64-zero", "zero")
    for steps in (1, 2):
        tc[...] = 0
        a = C.td_tc(R.TDState(cells, w, boards), tc, steps, lr_shift, C.TC_SEED, 1)
        b = R.td(R.TDState(cells, w, boards), steps, lr_shift, C.TC_SEED, 1)
        for k in ("weights", "boards", "after", "pending", "run_score", "stats"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (steps, k)
        assert (tc != 0).any() == (steps == 2)
    assert (a.weights != 0).any() and np.array_equal(tc[..., 0], a.weights)  # from zero weights: W = the sum of D = E
    assert (tc[..., 1] >= np.abs(tc[..., 0])).all() and ((tc[..., 1] != 0) | (tc[..., 0] == 0)).all()
    tc[...] = 0
    a = C.td_tc(R.TDState(cells, w, boards), tc, 20, lr_shift, C.TC_SEED, 1)
    b = R.td(R.TDState(cells, w, boards), 20, lr_shift, C.TC_SEED, 1)
    assert not np.array_equal(a.weights, b.weights)


def test_double_hit_and_zero_d():
    """The empty after-state under two 2-tuples: all 8 symmetries of a tuple read index 0, so one record is
    read 8 times as it was and W, E, A receive 8 adds.  Then D = 0: nothing changes."""
    cells = [[0, 1], [2, 3]]
    after = np.zeros((1, 16), np.int8)
    # the after-state of ENDING (LEFT, 16 points) reads no index 0: target = 16 S with zero weights elsewhere
    w = np.zeros((2, 256), np.int32)
    w[:, 0] = 100, -100                       # V(after) = 0, delta = 16 S = 65536, D = 65536 >> 4 = 4096 at lr_shift 4
    tc = np.zeros((2, 256, 2), np.int64)
    tc[0, 0] = -300, 1200                     # rate 1/4: add = 1024, 8 times
    tc[1, 0] = 7, 0                           # A = 0: add = D whatever E holds
    st = R.TDState(cells, w, R.ENDING[None], after, pending=[1])
    ev = {}
    C.td_tc(st, tc, 1, 4, seed=1, counter=0, events=ev)
    assert ev["double"] == 1 and ev["fresh"] == 8 and ev["damped"] == 8
    assert st.weights[:, 0].tolist() == [100 + 8 * 1024, -100 + 8 * 4096]
    assert tc[:, 0].tolist() == [[-300 + 8 * 4096, 1200 + 8 * 4096], [7 + 8 * 4096, 8 * 4096]]
    assert int(np.abs(st.weights[:, 1:]).sum()) == 0 and int(np.abs(tc[:, 1:]).sum()) == 0
    # D = 0: pending = 2 (target 0) and V(after) = 0
    w[:, 0] = 100, -100
    tc[0, 0], tc[1, 0] = (-300, 1200), (7, 0)
    keep = tc.copy()
    st = R.TDState(cells, w, R.ENDING[None], after, pending=[2])
    C.td_tc(st, tc, 1, 4, seed=1, counter=0)
    assert np.array_equal(st.weights, w) and np.array_equal(tc, keep) and st.stats[3] == 1  # still an update applied


PINNED = {  # (case, accumulators): (fresh, damped, zeroed, shifted, rate_clamped, wrapped, double, shared, games, updates)
    ("n1-random", "zero"): (2136, 4242, 0, 3862, 0, 0, 185, 0, 2, 199),
    ("n1-random", "prefilled"): (43, 2456, 2149, 6250, 3307, 0, 183, 0, 1, 199),
    ("n1-zero", "zero"): (2102, 4114, 34, 0, 0, 0, 198, 0, 2, 199),
    ("n1-zero", "prefilled"): (24, 774, 3952, 5756, 3037, 0, 194, 0, 2, 199),
    ("n300-random", "zero"): (44914, 2289292, 100, 2342524, 0, 103253, 54331, 199, 424, 59699),
    ("n300-random", "prefilled"): (648, 1555781, 166532, 2372349, 663779, 64339, 54691, 199, 411, 59699),
    ("n300-zero", "zero"): (36350, 2297432, 6, 2317440, 0, 209, 55633, 199, 462, 59699),
    ("n300-zero", "prefilled"): (399, 468910, 965952, 1811201, 946785, 0, 57938, 199, 216, 59699),
    ("n64-random", "zero"): (18180, 468074, 32, 491062, 0, 10226, 11664, 199, 106, 12735),
    ("n64-random", "prefilled"): (295, 294536, 61921, 502674, 152237, 3609, 11680, 199, 91, 12735),
    ("n64-t8k3", "zero"): (11478, 786266, 60, 803254, 0, 52600, 12735, 199, 98, 12735),
    ("n64-t8k3", "prefilled"): (280, 526269, 51941, 810784, 236162, 33424, 12735, 199, 94, 12735),
    ("n64-zero", "zero"): (19434, 449644, 3700, 68872, 0, 0, 12544, 199, 42, 12735),
    ("n64-zero", "prefilled"): (276, 80776, 220814, 352996, 205943, 0, 12293, 199, 62, 12735),
}


@pytest.mark.parametrize("name,fill", C.TC_CASES)
def test_pinned_tc_counts(name, fill):
    st, tc, ev = C.ref_case(name, fill)
    got = tuple(ev[k] for k in ("fresh", "damped", "zeroed", "shifted", "rate_clamped", "wrapped", "double", "shared"))
    assert got + (int(st.stats[0]), int(st.stats[3])) == PINNED[(name, fill)]
    C.covers(name, fill, ev)


def test_cases_cover_the_wrap_and_wide_accumulators():
    assert C.TC_CASES == [(n, f) for n in sorted(R.TD_CASES) for f in ("zero", "prefilled")] and len(C.TC_CASES) == 14
    assert {C.TC_LR[n] for n in C.TC_LR} == {4, 8} and all((C.TC_LR[n] == 4) == R.TD_CASES[n][3] for n in C.TC_LR)
    assert sum(C.ref_case(n, f)[2]["wrapped"] > 0 for n, f in C.TC_CASES) >= 6  # the int32 wrap of the weights
    pre = C.prefilled((5, 65536))
    E, A = pre[..., 0], pre[..., 1]
    assert A.min() == 0 and C.bitlen(A.view(np.uint64)).max() == 62 and (np.abs(E) > A).any() and (E < 0).any()
    assert np.array_equal(pre, C.prefilled((5, 65536)))


# --------------------------------------------------------------------------------- the seams -----
def test_header_declares_and_library_exports():
    from g2048 import _lib
    raw = (ROOT / "include" / "g2048_ntuple.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_tc_workspace_bytes", "g2048_ntuple_tc"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert len(lib.g2048_ntuple_tc.argtypes) == 14 and lib.g2048_ntuple_tc.argtypes[2] is ctypes.c_void_p
    for word in ("A_i == 0", "bitlen", "With D = 0 nothing changes", "plain TD(0)"):
        assert word in raw, word  # the rule and its two special cases are in the specification


def test_workspace_bytes():
    from g2048 import _lib
    for n in (0, 1, 300, (1 << 28) - 1):
        assert _lib.ntuple_tc_workspace_bytes(n) == _lib.ntuple_td_workspace_bytes(n) > 0
    assert _lib.ntuple_tc_workspace_bytes(1 << 28) == 0 and _lib.ntuple_tc_workspace_bytes(-1) == 0


def test_wrapper_checks_tc_and_rejects_cpu_tensors():
    from g2048 import _lib
    n = 4
    net = _lib.NtNet(1, 1, (ctypes.c_int32 * 48)(5), 0x1000)  # never dereferenced: refused before
    b = torch.zeros(n, 16, dtype=torch.int8)
    rest = (b, b.clone(), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64), 1, 10, _lib.make_rng(),
            torch.zeros(4, dtype=torch.int64), torch.zeros(1024, dtype=torch.uint8))
    for tc, why in ((None, "tc must be int64"), (torch.zeros(16, 2, dtype=torch.int32), "tc must be int64"),
                    (torch.zeros(16, dtype=torch.int64), "tc must be int64 with 32 elements"),
                    (torch.zeros(17, 2, dtype=torch.int64), "tc must be int64 with 32 elements"),
                    (torch.zeros(16, 2, dtype=torch.int64), "ROCm device")):
        with pytest.raises(_lib.G2048Error, match=why):
            _lib.ntuple_tc(net, tc, *rest)
    with pytest.raises(_lib.G2048Error, match="workspace"):
        _lib.ntuple_tc(net, torch.zeros(16, 2, dtype=torch.int64), *rest[:-1], None)


def test_trainer_rule_argument():
    from g2048.ntuple import NTupleNet, NTupleTrainer
    net = NTupleNet("lines-squares-4", "cpu")
    for bad in ("nope", "TC", "", None):
        with pytest.raises(ValueError):
            NTupleTrainer(net, rule=bad)
    assert NTupleTrainer(net).rule == "td" and NTupleTrainer(net, 8, 10, 3).rule == "td"
    tr = NTupleTrainer(net, envs=8, lr_shift=10, seed=3, rule="tc")  # no device is touched before train()
    assert tr.rule == "tc" and tr.tc is None and tr.accumulators() == (None, None)
    with pytest.raises(ValueError):
        NTupleTrainer(net).accumulators()
    with pytest.raises(ValueError):
        tr.train(0)


def test_command_rule_option():
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["train-ntuple", "--help"])
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    assert r.exit_code == 0 and "--rule" in out, out
    assert "fresh weight" in inspect.signature(train.train_ntuple).parameters["lr_shift"].default.help
    r = CliRunner().invoke(train.app, ["train-ntuple", "--rule", "nope", "--steps", "1"])  # refused before any device
    assert r.exit_code == 1 and "Unknown learning rule: nope" in r.output and "td, tc" in r.output
