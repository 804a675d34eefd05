"""CPU reference of the temporal-coherence step of the n-tuple network (the TC step of
include/g2048_ntuple.h, g2048_ntuple_tc), in numpy on tests/ntuple_reference.py: R.choose (the greedy
action and the target), R.indices (the 8 T weights of an after-state) and R.env_step_auto_reset.  The
accumulators are one int64 array tc [T, 16^K, 2]: tc[..., 0] = E, tc[..., 1] = A read as uint64; both
wrap, like the int32 weights.  Shared by tests/test_ntuple_tc_host.py and tests/test_gpu_ntuple_tc.py;
not a test module itself."""

import functools

import numpy as np

import ntuple_reference as R

TC_STEPS = 200
TC_SEED = R.TD_SEED
# the TC cases: the starts of R.TD_CASES (R.td_start), at lr_shift 8 from zero weights and 4 from the 22-bit
# random ones -- the 12 and 20 of the TD(0) cases keep A below 2^20 for 200 steps, and the shift is never
# taken -- each from zero accumulators and from prefilled ones
TC_LR = {name: (4 if case[3] else 8) for name, case in R.TD_CASES.items()}
TC_CASES = [(name, fill) for name in sorted(R.TD_CASES) for fill in ("zero", "prefilled")]


def prefilled(shape):
    """int64 shape + (2,): A = U[0, 2^62) >> U[0, 62) and E = U[-2^62, 2^62) >> U[0, 62) (arithmetic), four
    independent draws of default_rng(11) in this order: 62-bit accumulators, and |E| > A."""
    rng = np.random.default_rng(11)
    A = rng.integers(0, 1 << 62, size=shape, dtype=np.int64) >> rng.integers(0, 62, size=shape, dtype=np.int64)
    E = rng.integers(-(1 << 62), 1 << 62, size=shape, dtype=np.int64) >> rng.integers(0, 62, size=shape, dtype=np.int64)
    return np.ascontiguousarray(np.stack([E, A], axis=-1))


def tc_start(name, fill):
    """-> (cells, weights, boards, lr_shift, tc) of a TC case."""
    cells, w, boards, _ = R.td_start(name)
    tc = prefilled(w.shape) if fill == "prefilled" else np.zeros(w.shape + (2,), np.int64)
    return cells, w, boards, TC_LR[name], tc


def bitlen(x):
    """Bit length of every element of a uint64 array -> int64."""
    x = np.array(x, np.uint64)
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = x >= np.uint64(1 << s)
        n += np.where(big, s, 0)
        x = np.where(big, x >> np.uint64(s), x)
    return n + (x != 0)


def tc_adds(E, A, D):
    """add_i of the rule for records (E int64, A uint64) and updates D int64, elementwise -> (add int64,
    sh int64 (bitlen(A) - 20 before the max), rate_clamped bool)."""
    E, A, D = np.asarray(E, np.int64), np.asarray(A, np.uint64), np.asarray(D, np.int64)
    bl = bitlen(A)
    sh = np.maximum(bl - 20, 0).astype(np.uint64)
    a = A >> sh
    mag = np.where(E < 0, ~E.view(np.uint64) + np.uint64(1), E.view(np.uint64))  # 2^63 for INT64_MIN
    e_raw = mag >> sh
    e = np.minimum(e_raw, a)
    absD = np.abs(D).astype(np.uint64)
    a1 = np.where(A == 0, np.uint64(1), a)
    q = ((absD * e + (a >> np.uint64(1))) // a1).astype(np.int64)  # the numerator is below 2^51
    add = np.where(A == 0, D, np.sign(D) * q)
    return add, bl - 20, (A != 0) & (e_raw > a)


def _wrap32(acc):
    return acc.astype(np.uint64).astype(np.uint32).view(np.int32)


def td_tc(st: R.TDState, tc, steps, lr_shift, seed, counter, events=None):
    """`steps` TC steps on st and tc (int64 [T, 16^K, 2]), both in place: R.td with step 2 replaced.  events
    (optional dict) counts, per hit of a weight: "fresh" (A = 0), "damped" (add != D and add != 0), "zeroed"
    (add = 0 while D != 0), "shifted" (bitlen(A) > 20), "rate_clamped" (|E| >> sh > a); and as R.td:
    "double" (an env hitting one weight twice in one update), "shared" (steps in which two envs add to
    one weight), "ended", "dead", "clamped"; and "wrapped" (weights a step's adds took past the int32 range)."""
    n = len(st.boards)
    T = len(st.cells)
    assert tc.dtype == np.int64 and tc.shape == st.weights.shape + (2,) and tc.flags.c_contiguous
    Ef, Af = tc.reshape(-1, 2)[:, 0], tc.reshape(-1, 2)[:, 1].view(np.uint64)  # views: updated in place
    ev = dict.fromkeys(("fresh", "damped", "zeroed", "shifted", "rate_clamped", "wrapped", "double", "shared", "ended",
                        "dead", "clamped"), 0)
    tcol = np.arange(T)[None, :, None]
    for s in range(steps):
        q, legal, best, moved = R.choose(st.cells, st.weights, st.boards)
        has = legal != 0
        a = np.where(has, best, 0)
        target = np.where(has, q[np.arange(n), a], 0)
        sprime = moved[np.arange(n), a]
        upd = st.pending != 0
        if upd.any():
            idx = R.indices(st.cells, st.after[upd])                     # [8, T, m], read before any add
            va = st.weights.astype(np.int64)[tcol, idx].sum((0, 1))
            delta = np.where(st.pending[upd] == 2, 0, target[upd]) - va
            raw = (delta + (1 << (lr_shift - 1))) >> lr_shift
            D = np.clip(raw, -(1 << 30), 1 << 30)
            ev["clamped"] += int((raw != D).sum())
            flat = (tcol * st.weights.shape[1] + idx).reshape(-1)        # [8 T m]
            Dh = np.broadcast_to(D, idx.shape).reshape(-1)
            add, sh, rc = tc_adds(Ef[flat], Af[flat], Dh)                # the records before this step's adds
            ev["fresh"] += int((Af[flat] == 0).sum())
            ev["damped"] += int(((add != Dh) & (add != 0)).sum())
            ev["zeroed"] += int(((Dh != 0) & (add == 0)).sum())
            ev["shifted"] += int((sh > 0).sum())
            ev["rate_clamped"] += int(rc.sum())
            if events is not None:
                per_env = np.sort(flat.reshape(8 * T, -1), axis=0)       # [8 T, m]: the weights of each env
                ev["double"] += int((np.diff(per_env, axis=0) == 0).any(0).sum())
                pairs = np.unique(np.stack([per_env.reshape(-1), np.tile(np.arange(per_env.shape[1]), 8 * T)]), axis=1)
                ev["shared"] += int((np.unique(pairs[0], return_counts=True)[1] > 1).any())
            acc = st.weights.astype(np.int64).reshape(-1)
            np.add.at(acc, flat, add)
            ev["wrapped"] += int(((acc < -(1 << 31)) | (acc >= 1 << 31)).sum())
            st.weights[...] = _wrap32(acc).reshape(st.weights.shape)
            np.add.at(Ef, flat, Dh)                                      # int64 and uint64 adds wrap
            np.add.at(Af, flat, np.abs(Dh).astype(np.uint64))
            st.stats[3] += int(upd.sum())
        st.boards, pts, done = R.env_step_auto_reset(st.boards, a, seed, counter + s)
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


@functools.lru_cache(maxsize=None)
def ref_case(name, fill):
    """-> (TDState, tc, events) after TC_STEPS steps of a TC case: computed once per process, read-only."""
    cells, w, boards, lr_shift, tc = tc_start(name, fill)
    ev = {}
    st = td_tc(R.TDState(cells, w, boards), tc, TC_STEPS, lr_shift, TC_SEED, 1, events=ev)
    for a in (st.weights, st.boards, st.after, st.pending, st.run_score, st.stats, tc):
        a.setflags(write=False)
    return st, tc, ev


def covers(name, fill, ev):
    """What a TC case must show on the reference before a device result is compared with it."""
    n = R.TD_CASES[name][1]
    assert ev["fresh"] > 0 and ev["damped"] > 0 and ev["double"] > 0 and ev["ended"] > 0
    if fill == "prefilled":
        assert ev["zeroed"] > 0 and ev["shifted"] > 0 and ev["rate_clamped"] > 0
    else:
        assert ev["rate_clamped"] == 0                       # from zeros |E| <= A holds without the min
        assert (ev["shifted"] > 0) == (name != "n1-zero")
    assert (ev["dead"] > 0 and ev["shared"] > 0) == (n > 1)
