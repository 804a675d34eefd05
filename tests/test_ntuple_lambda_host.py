"""CPU-side checks of the lambda step of the n-tuple network (include/g2048_ntuple.h: TD(lambda) and
TC(lambda) with a truncated trace, lambda = 2^-s): the decay D_k worked out by hand; one step on a
one-tuple net worked out by hand under both rules; the numpy reference (tests/ntuple_lambda_reference.py)
against a scalar implementation in Python ints written from the header, on a three-step one-env trace
and on six envs; h = 0 against the TD and the TC reference; the coverage the GPU tests rely on; and the
seams (the C ABI declaration, export and refusals, the wrapper's checks, the trainer's and the
command's options)."""

import ctypes
import re

import numpy as np
import pytest
import torch

import ntuple_lambda_reference as LR
import ntuple_reference as R
import ntuple_tc_reference as C
import test_ntuple_host as H  # the scalar value / choice / move in Python ints
import test_ntuple_tc_host as HC  # the scalar share of the TC rule
from conftest import ROOT
from oracle import oracle as O

STATE = ("weights", "boards", "after", "pending", "run_score", "stats")


def test_decay_by_hand():
    """D_k = sign(D) (|D| >> k s) for k = 0..4: towards zero in both signs."""
    want = {
        (5, 1): [5, 2, 1, 0, 0], (5, 2): [5, 1, 0, 0, 0], (5, 7): [5, 0, 0, 0, 0],
        (1, 1): [1, 0, 0, 0, 0], (1, 2): [1, 0, 0, 0, 0], (1, 7): [1, 0, 0, 0, 0],
        (0, 1): [0, 0, 0, 0, 0], (0, 2): [0, 0, 0, 0, 0], (0, 7): [0, 0, 0, 0, 0],
        (1 << 30, 1): [1 << 30, 1 << 29, 1 << 28, 1 << 27, 1 << 26],
        (1 << 30, 2): [1 << 30, 1 << 28, 1 << 26, 1 << 24, 1 << 22],
        (1 << 30, 7): [1 << 30, 1 << 23, 1 << 16, 1 << 9, 1 << 2],
    }
    for (D, s), row in want.items():
        for sign in (1, -1):
            got = [int(LR.decay(np.array([sign * D]), k, s)[0]) for k in range(5)]
            assert got == [sign * x for x in row], (sign * D, s)
    # a floor (an arithmetic shift of D itself) would give -3, -2, -1, -1 for D = -5 at s = 1
    assert [int(LR.decay(np.array([-5]), k, 1)[0]) for k in range(5)] != [-5 >> k for k in range(5)]
    assert 4 * 7 == 28 < 31  # the largest shift k s


def _corners(a, b, c, d):
    board = np.full(16, 9, np.int8)  # the net below reads the four corners only
    board[[0, 3, 12, 15]] = a, b, c, d
    return board


def _hand_state(tc_rule):
    """One env on the one-tuple net [[0]] (V = 2 x the sum of W over the four corners' exponents), a dead
    board, p = 2 (target 0), h = 3 with hist_len = 2: hist[2] holds an after-state that must not be hit."""
    w = np.zeros((1, 16), np.int32)
    w[0, :4] = 100, -300, 50, 7
    hist = np.stack([_corners(3, 3, 0, 0), _corners(2, 2, 2, 2), _corners(1, 1, 1, 1)])[:, None, :]
    st = LR.LState([[0]], w, R.DEAD[None], 3, hist=hist, hist_len=[2], after=_corners(1, 0, 0, 2)[None], pending=[2])
    tc = np.zeros((1, 16, 2), np.int64) if tc_rule else None
    return st, tc


def test_one_step_by_hand_td():
    """V(after) = 2 (-300 + 100 + 100 + 50) = -100, delta = 100, lr_shift 2: D = 102 >> 2 = 25, D_1 = 12, D_2 = 6.
    after hits W[1] and W[2] twice and W[0] four times; hist[0] hits W[3] and W[0] four times each; hist[1]
    hits W[2] eight times.  All from the weights before the step."""
    st, _ = _hand_state(False)
    ev = {}
    LR.td_lambda(st, None, 1, 2, 1, seed=1, counter=0, events=ev)
    assert st.weights[0, :5].tolist() == [100 + 4 * 25 + 4 * 12, -300 + 2 * 25, 50 + 2 * 25 + 8 * 6, 7 + 4 * 12, 0]
    assert int(np.abs(st.weights[0, 4:]).sum()) == 0
    assert (ev["traced"], ev["cross"], ev["terminal_traced"], ev["cut"], ev["double"]) == (16, 2, 1, 1, 3)
    assert st.stats[3] == 1 and st.hist_len.tolist() == [0] and st.pending.tolist() == [0]  # a dead board: no move
    # s = 2: D_1 = 6, D_2 = 1;  s = 7: D_1 = D_2 = 0, the plain TD update
    st, _ = _hand_state(False)
    LR.td_lambda(st, None, 1, 2, 2, seed=1, counter=0, events=ev)
    assert st.weights[0, :4].tolist() == [100 + 4 * 25 + 4 * 6, -250, 100 + 8 * 1, 7 + 4 * 6]
    st, _ = _hand_state(False)
    ev = {}
    LR.td_lambda(st, None, 1, 2, 7, seed=1, counter=0, events=ev)
    assert st.weights[0, :4].tolist() == [200, -250, 100, 7] and ev["decayed_out"] == 2 and ev["traced"] == 0


def test_one_step_by_hand_tc():
    """The same step under rule TC: zero records take D_k itself, however often they are hit in the step
    (every hit reads the record before the step's adds); the record of W[3], E = -300 and A = 1200, takes
    (12 x 300 + 600) // 1200 = 3 of D_1 = 12."""
    st, tc = _hand_state(True)
    tc[0, 3] = -300, 1200
    LR.td_lambda(st, tc, 1, 2, 1, seed=1, counter=0)
    assert st.weights[0, :4].tolist() == [248, -250, 148, 7 + 4 * 3]
    assert tc[0, :5, 0].tolist() == [148, 50, 98, -300 + 48, 0] and tc[0, :5, 1].tolist() == [148, 50, 98, 1248, 0]


def scalar_lambda(cells, w, E, A, boards, steps, lr_shift, h, s, seed, counter):
    """The lambda step of the header, env by env, in Python ints; w (and E, A under rule TC, else None): lists
    of lists, updated in place.  -> (boards, after, hist (per env: the newest first), pending, run, stats)."""
    n = len(boards)
    boards = [tuple(int(x) for x in b) for b in boards]
    after, pending, run, hist = [None] * n, [0] * n, [0] * n, [[] for _ in range(n)]
    stats = [0, 0, 0, 0]
    for step in range(steps):
        adds, plan = [], []
        for i in range(n):  # every read sees W, E and A before the step's adds
            q, best = H.scalar_choose(cells, w, boards[i])
            target = q[best] if best != 0xFF else 0
            if pending[i]:
                delta = (0 if pending[i] == 2 else target) - H.scalar_value(cells, w, after[i])
                D = max(-(1 << 30), min(1 << 30, (delta + (1 << (lr_shift - 1))) >> lr_shift))
                for k, sk in enumerate([after[i]] + hist[i]):
                    Dk = (abs(D) >> (k * s)) * (1 if D > 0 else -1)
                    if Dk:
                        adds += [(t, j, Dk, Dk if E is None else HC.scalar_share(E[t][j], A[t][j], Dk))
                                 for t, j in H.scalar_hits(cells, sk)]
                stats[3] += 1
            plan.append(best)
        for t, j, Dk, add in adds:
            w[t][j] = HC._wrap(w[t][j] + add, 32)
            if E is not None:
                E[t][j] = HC._wrap(E[t][j] + Dk, 64)
                A[t][j] = (A[t][j] + abs(Dk)) % (1 << 64)
        acts = [0 if a == 0xFF else a for a in plan]
        nb, pts, done = R.env_step_auto_reset(np.array(boards, np.int8), np.array(acts), seed, counter + step)
        for i in range(n):
            run[i] += int(pts[i])
            if done[i]:
                stats[0] += 1
                stats[1] += run[i]
                stats[2] = max(stats[2], run[i])
                run[i] = 0
            if plan[i] != 0xFF:
                hist[i] = ([after[i]] + hist[i])[:h] if pending[i] == 1 else []
                after[i] = H._move(boards[i], plan[i])[0]
                pending[i] = 2 if done[i] else 1
            else:
                hist[i] = []
                pending[i] = 0
            boards[i] = tuple(int(x) for x in nb[i])
    return boards, after, hist, pending, run, stats


def _assert_matches_scalar(st, tc, scalar, w, E, A):
    sb, sa, sh, sp, sr, ss = scalar
    assert st.weights.tolist() == w
    if tc is not None:
        assert tc[..., 0].tolist() == E and tc[..., 1].view(np.uint64).tolist() == A
    assert np.array_equal(st.boards, np.array(sb, np.int8)) and st.pending.tolist() == sp
    assert st.run_score.tolist() == sr and st.stats.tolist() == ss
    assert st.hist_len.tolist() == [len(x) for x in sh]
    for i in range(len(sb)):
        if sp[i]:
            assert tuple(st.after[i]) == sa[i]
        for k, row in enumerate(sh[i]):
            assert tuple(st.hist[k, i]) == row, (i, k)


def test_three_step_trace_of_one_env():
    """One env from a fresh board on the one-tuple net [[0, 1, 4, 5]], h = 3, s = 1, step by step: the first step
    updates nothing, the second only its after-state (the history is empty), the third its after-state with D
    and the one before with D >> 1; the history grows by the old after-state each time.  Every step
    equals the scalar implementation."""
    cells = [[0, 1, 4, 5]]
    w0 = R.random_weights(cells, 4, bits=16)
    boards = O.reset(1, seed=12, step_idx=0)
    st = LR.LState(cells, w0, boards, 3)
    afters = []
    for step in range(1, 4):
        before = st.weights.copy()
        old_after, p = st.after[0].copy(), int(st.pending[0])
        ev = {}
        LR.td_lambda(st, None, 1, 3, 1, seed=12, counter=step, events=ev)
        assert st.pending.tolist() == [1] and st.hist_len.tolist() == [step - 1] and st.stats[3] == step - 1
        assert (ev["traced"] > 0) == (step == 3) and (p == 0) == (step == 1)
        if step == 1:
            assert np.array_equal(st.weights, before)
        else:
            q, best = H.scalar_choose(cells, before, tuple(int(x) for x in prev_board))
            D = (q[best] - H.scalar_value(cells, before, tuple(int(x) for x in old_after)) + 4) >> 3  # lr_shift 3
            want = before.astype(np.int64).copy()
            for k, sk in enumerate([old_after] + afters[-2::-1][:step - 2]):
                for t, j in H.scalar_hits(cells, tuple(int(x) for x in sk)):
                    want[t, j] += (abs(D) >> k) * (1 if D > 0 else -1)
            assert D != 0 and np.array_equal(st.weights, want.astype(np.int32))
            assert np.array_equal(st.hist[0, 0], old_after)
        for k in range(step - 1):
            assert np.array_equal(st.hist[k, 0], afters[-1 - k])  # the newest first
        afters.append(st.after[0].copy())
        prev_board = st.boards[0].copy()
    w = [[int(x) for x in row] for row in w0]
    sc = scalar_lambda(cells, w, None, None, boards, 3, 3, 3, 1, 12, 1)
    _assert_matches_scalar(st, None, sc, w, None, None)


@pytest.mark.parametrize("rule,fill", [("td", None), ("tc", "zero"), ("tc", "prefilled")])
@pytest.mark.parametrize("h,s", [(3, 1), (4, 2), (1, 7)])
def test_reference_matches_scalar_lambda(rule, fill, h, s):
    """Six envs (ending, fresh, dead boards), 30 steps at lr_shift 4 on a small net (two 2-tuples, so that
    the few envs and the few k meet on weights)."""
    cells = [[0, 1], [5, 6]]
    w0 = R.random_weights(cells, 5, bits=20)
    seed = {None: 6, "zero": 4, "prefilled": 12}[fill]  # where a game ends after more than one move at every trace
    boards = O.reset(6, seed=seed, step_idx=0)
    boards[0], boards[2], boards[5] = R.ENDING, R.ENDING, R.DEAD
    tc = None if rule == "td" else C.prefilled(w0.shape) if fill == "prefilled" else np.zeros(w0.shape + (2,), np.int64)
    tc0 = None if tc is None else tc.copy()
    ev = {}
    st = LR.td_lambda(LR.LState(cells, w0, boards, h), tc, 30, 4, s, seed=seed, counter=1, events=ev)
    assert ev["ended"] > 0 and ev["dead"] > 0 and ev["double"] > 0 and ev["shared"] > 0 and ev["cut"] > 0
    assert ev["full"] > 0 and ev["terminal_traced"] > 0 and (ev["traced"] > 0 and ev["cross"] > 0 or s == 7)
    w = [[int(x) for x in row] for row in w0]
    E = A = None
    if tc is not None:
        E = [[int(x) for x in row] for row in tc0[..., 0]]
        A = [[int(x) for x in row] for row in tc0[..., 1].view(np.uint64)]
    sc = scalar_lambda(cells, w, E, A, boards, 30, 4, h, s, seed, 1)
    _assert_matches_scalar(st, tc, sc, w, E, A)


def test_trace_zero_is_the_td_and_the_tc_reference():
    cells, w, boards, lr_shift = R.td_start("n64-random")
    a = LR.td_lambda(LR.LState(cells, w, boards, 0), None, 60, lr_shift, 1, LR.SEED, 1)
    b = R.td(R.TDState(cells, w, boards), 60, lr_shift, LR.SEED, 1)
    for k in STATE:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.weights != w).any() and a.hist.shape == (0, 64, 16)
    tc1 = np.zeros(w.shape + (2,), np.int64)
    tc2 = tc1.copy()
    a = LR.td_lambda(LR.LState(cells, w, boards, 0), tc1, 60, lr_shift, 3, LR.SEED, 1)
    c = C.td_tc(R.TDState(cells, w, boards), tc2, 60, lr_shift, LR.SEED, 1)
    for k in STATE:
        assert np.array_equal(getattr(a, k), getattr(c, k)), k
    assert np.array_equal(tc1, tc2) and not np.array_equal(a.weights, b.weights)
    d = LR.td_lambda(LR.LState(cells, w, boards, 3), None, 60, lr_shift, 1, LR.SEED, 1)
    assert not np.array_equal(d.weights, b.weights)  # a trace changes the run


@pytest.mark.parametrize("rule,name,fill", LR.CASES)
@pytest.mark.parametrize("h,s", LR.TRACES)
def test_cases_cover_what_the_gpu_tests_claim(rule, name, fill, h, s):
    st, tc, ev = LR.ref_case(rule, name, fill, h, s)
    LR.covers(name, s, ev)
    assert int(st.hist_len.max()) == h and st.stats[3] > 0


def test_cases_are_the_named_ones():
    assert LR.TRACES == [(1, 1), (3, 1), (4, 2)] and LR.STEPS == 200
    assert [c[1:] for c in LR.CASES if c[0] == "td"] == [("n1-zero", None), ("n64-random", None), ("n300-zero", None),
                                                        ("n64-t8k3", None)]
    assert [c[1:] for c in LR.CASES if c[0] == "tc"] == [("n64-zero", "zero"), ("n64-zero", "prefilled"),
                                                        ("n300-random", "zero"), ("n300-random", "prefilled")]
    for rule, name, fill in LR.CASES:
        assert LR.start(rule, name, fill)[3] == (R.TD_CASES[name][2] if rule == "td" else C.TC_LR[name])


# --------------------------------------------------------------------------------- the seams -----
def test_header_declares_and_library_exports():
    from g2048 import _lib
    raw = (ROOT / "include" / "g2048_ntuple.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for name in ("g2048_ntuple_lambda_workspace_bytes", "g2048_ntuple_lambda"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name  # bound from the header
    assert len(lib.g2048_ntuple_lambda.argtypes) == 18 and lib.g2048_ntuple_lambda.argtypes[2] is ctypes.c_void_p
    assert (_lib.NT_MAX_TRACE, _lib.NT_MAX_LAMBDA_SHIFT) == (4, 7)
    assert ctypes.sizeof(_lib.NtNet) == 208  # the net struct did not change
    for word in ("The lambda step", "hist_len", "rounds towards zero", "D_k = sign(D)", "k s <= 4 x 7 = 28"):
        assert word in raw, word


def test_workspace_bytes():
    from g2048 import _lib
    for n in (0, 1, 300, (1 << 28) - 1):
        assert _lib.ntuple_lambda_workspace_bytes(n) == _lib.ntuple_td_workspace_bytes(n) > 0
    assert _lib.ntuple_lambda_workspace_bytes(1 << 28) == 0 and _lib.ntuple_lambda_workspace_bytes(-1) == 0


def test_every_refusal_returns_einval():
    """Through the loaded library, on the host: every argument is refused before any pointer is
    dereferenced or anything is enqueued, so made-up addresses do."""
    from g2048 import _lib
    lib = _lib.load()
    P = 0x10000  # 16-B aligned, never dereferenced
    n0 = 64
    need = _lib.ntuple_lambda_workspace_bytes(n0)
    rng = _lib.make_rng(_lib.RNG_PHILOX, 1, 1)

    def net(T=1, K=2, cells=(0, 1), ptr=P):
        return _lib.NtNet(T, K, (ctypes.c_int32 * 48)(*cells), ptr)

    def call(net=net(), tc=None, boards=P, after=P, hist=P, hist_len=P, pending=P, run_score=P, n=n0, steps=3, lr=10,
             h=3, s=1, rng=rng, stats=P, ws=P, ws_bytes=need):
        return lib.g2048_ntuple_lambda(None, ctypes.byref(net) if net is not None else None, tc, boards, after, hist,
                                       hist_len, pending, run_score, n, steps, lr, h, s,
                                       ctypes.byref(rng) if rng is not None else None, stats, ws, ws_bytes)

    # those of g2048_ntuple_td / _tc
    assert call(net=None) == -1
    for bad in (net(T=0), net(T=9), net(K=0), net(K=7), net(ptr=None), net(ptr=P + 4), net(cells=(0, 16)),
                net(cells=(0, -1)), net(cells=(3, 3))):
        assert call(net=bad) == -1
    assert call(n=-1) == -1 and call(n=1 << 28) == -1 and call(n=1 << 40) == -1
    assert call(steps=0) == -1 and call(steps=-1) == -1
    assert call(lr=0) == -1 and call(lr=31) == -1 and call(lr=-1) == -1
    assert call(rng=None) == -1
    assert call(rng=_lib.make_rng(_lib.RNG_INJECT, 1, 1)) == -1 and call(rng=_lib.make_rng(_lib.RNG_MT19937, 1, 1)) == -1
    odd = _lib.make_rng(_lib.RNG_PHILOX, 1, 1)
    odd.counter_dev = P + 4
    assert call(rng=odd) == -1
    for null in ("boards", "after", "pending", "run_score", "ws"):
        assert call(**{null: None}) == -1, null
    for mis in ("boards", "after", "ws"):
        assert call(**{mis: P + 8}) == -1, mis
    assert call(run_score=P + 4) == -1 and call(stats=P + 4) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    # those of the lambda step, under either rule
    for tc in (None, P):
        for h in (-1, 5, 1 << 20):
            assert call(tc=tc, h=h) == -1
        for s in (0, 8, -1):
            assert call(tc=tc, s=s) == -1
            assert call(tc=tc, s=s, h=0, hist=None, hist_len=None) == -1  # lambda_shift is checked without a trace too
        for h in (1, 4):
            assert call(tc=tc, h=h, hist=None) == -1 and call(tc=tc, h=h, hist=P + 8) == -1
            assert call(tc=tc, h=h, hist_len=None) == -1
    assert call(tc=P + 8) == -1 and call(tc=P + 8, n=0) == -1  # a misaligned tc
    # n = 0 is a no-op: nothing is read, nothing is enqueued
    assert call(n=0) == 0 and call(n=0, tc=P) == 0 and call(n=0, h=0, hist=None, hist_len=None) == 0
    assert call(n=0, boards=None, after=None, pending=None, run_score=None, ws=None, ws_bytes=0) == 0


def test_wrapper_checks_and_rejects_cpu_tensors():
    from g2048 import _lib
    n = 4
    net = _lib.NtNet(1, 1, (ctypes.c_int32 * 48)(5), 0x1000)  # never dereferenced: refused before
    b = torch.zeros(n, 16, dtype=torch.int8)
    hist, hl = torch.zeros(3, n, 16, dtype=torch.int8), torch.zeros(n, dtype=torch.uint8)
    tail = (torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64), 1, 10, 3, 1, _lib.make_rng(),
            torch.zeros(4, dtype=torch.int64), torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(_lib.G2048Error, match="tc must be int64 with 32 elements"):
        _lib.ntuple_lambda(net, torch.zeros(16, dtype=torch.int64), b, b.clone(), hist, hl, *tail)
    with pytest.raises(_lib.G2048Error, match="needs hist and hist_len"):
        _lib.ntuple_lambda(net, None, b, b.clone(), None, hl, *tail)
    with pytest.raises(_lib.G2048Error, match="needs hist and hist_len"):
        _lib.ntuple_lambda(net, None, b, b.clone(), hist, None, *tail)
    with pytest.raises(_lib.G2048Error, match="hist holds 128 elements, needs 192"):
        _lib.ntuple_lambda(net, None, b, b.clone(), hist[:2].contiguous(), hl, *tail)
    with pytest.raises(_lib.G2048Error, match="workspace"):
        _lib.ntuple_lambda(net, None, b, b.clone(), hist, hl, *tail[:-1], None)
    with pytest.raises(_lib.G2048Error, match="ROCm device"):
        _lib.ntuple_lambda(net, None, b, b.clone(), hist, hl, *tail)


def test_trainer_trace_arguments():
    from g2048.ntuple import MAX_LAMBDA_SHIFT, MAX_TRACE, NTupleNet, NTupleTrainer
    assert (MAX_TRACE, MAX_LAMBDA_SHIFT) == (4, 7)
    net = NTupleNet("lines-squares-4", "cpu")
    for kw in ({"trace_len": -1}, {"trace_len": 5}, {"lambda_shift": 0}, {"lambda_shift": 8},
               {"trace_len": 0, "lambda_shift": 0}):
        for rule in NTupleTrainer.RULES:
            with pytest.raises(ValueError):
                NTupleTrainer(net, rule=rule, **kw)
    tr = NTupleTrainer(net)
    assert (tr.trace_len, tr.lambda_shift, tr.hist, tr.hist_len) == (0, 1, None, None)
    tr = NTupleTrainer(net, 8, 10, 3, "tc", 4, 7)  # no device is touched before train()
    assert (tr.rule, tr.trace_len, tr.lambda_shift, tr.hist) == ("tc", 4, 7, None)
    with pytest.raises(ValueError):
        tr.train(0)


def test_command_trace_options():
    from typer.testing import CliRunner
    import train
    r = CliRunner().invoke(train.app, ["train-ntuple", "--help"])
    out = re.sub(r"\x1b\[[0-9;]*m", "", r.output)
    assert r.exit_code == 0 and "--trace" in out and "--lambda-shift" in out, out
    for args, word in ((["--trace", "5"], "--trace must be in 0..4, got 5"), (["--trace", "-1"], "--trace must be in 0..4"),
                       (["--lambda-shift", "0"], "--lambda-shift must be in 1..7, got 0"),
                       (["--trace", "2", "--lambda-shift", "8"], "--lambda-shift must be in 1..7, got 8")):
        r = CliRunner().invoke(train.app, ["train-ntuple", "--steps", "1"] + args)  # refused before any device
        assert r.exit_code == 1 and word in r.output, r.output
