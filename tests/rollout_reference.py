"""CPU replay of a policy rollout and the fp64 sampler.  TEST INFRASTRUCTURE ONLY.

replay() restates what g2048_env_step / g2048_policy_rollout do to the env for recorded actions
(step_board, csrc/step.hpp; include/g2048.h) with the CPU oracle's game.step and reset, one Philox
counter per step as g2048/rollout.py lays them out: the sampler of step t draws at counter_base + 2t,
the env step (spawn, and the fresh board of an auto-reset) at counter_base + 2t + 1.

sampler_reference() restates the rollout's masked softmax / entropy / log_softmax
(train.py:266-291, :326; oracle.masked_policy) and the inverse-CDF action of g2048_sample_actions in
float64.  tests/test_rollout_reference_host.py pins both.
"""

import numpy as np

from oracle import oracle as O

OPT_AUTO_RESET, OPT_SKIP_DONE = 1, 2
FLAG_INVALID, FLAG_RESET, FLAG_INACTIVE, FLAG_DONE = 0x10, 0x20, 0x40, 0x80

D = np.array([3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 5, 5, 7, 8], np.int8)   # legal: LEFT, RIGHT; either ends the game
DT = np.ascontiguousarray(D.reshape(4, 4).T).reshape(16)                  # legal: UP, DOWN; either ends the game
C = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.int8)   # no legal move


def replay(boards0, actions, seed, counter_base, env_base, opts):
    """boards0 int8 [n, 16], actions [T, n] -> boards int8 [T+1, n, 16], flags uint8 [T+1, n]
    (flags[0] = the legal mask of boards0, flags[t+1] what step t writes), points int32 [T, n],
    max_tile int8 [T, n], pot int8 [T, n, 4] = (mono_b, mono_a, empt_b, empt_a)."""
    b0 = np.asarray(boards0, np.int8).reshape(-1, 16)
    actions = np.asarray(actions)
    T, n = actions.shape
    boards = np.zeros((T + 1, n, 16), np.int8)
    flags = np.zeros((T + 1, n), np.uint8)
    points = np.zeros((T, n), np.int32)
    max_tile = np.zeros((T, n), np.int8)
    pot = np.zeros((T, n, 4), np.int8)
    boards[0] = b0
    flags[0] = O.legal_mask(b0)
    for t in range(T):
        ctr = counter_base + 2 * t + 1
        b = boards[t]
        nb, f, _, _ = O.step(b, actions[t].astype(np.int64) & 3, O.RNG_PHILOX, seed, step_idx=ctr, env_base=env_base)
        invalid, done = f["invalid"].astype(bool), f["done"].astype(bool)
        assert np.array_equal(nb[invalid], b[invalid])  # an illegal action is a no-op
        fl = O.legal_mask(nb).astype(np.int64) | np.where(invalid, FLAG_INVALID, 0) | np.where(done, FLAG_DONE, 0)
        pts, mx = f["points"].copy(), f["max_tile"].copy()
        po = np.stack([f["mono_b"], f["mono_a"], f["empt_b"], f["empt_a"]], axis=1)
        if opts & OPT_SKIP_DONE:  # a game already over: untouched, nothing earned
            inactive = O.legal_mask(b) == 0
            nb[inactive] = b[inactive]
            fl[inactive] = FLAG_INACTIVE | FLAG_DONE
            pts[inactive], mx[inactive], po[inactive] = 0, 0, 0
            done = done & ~inactive
        if opts & OPT_AUTO_RESET:
            fresh = O.reset(n, O.RNG_PHILOX, seed, step_idx=ctr, env_base=env_base)
            nb[done] = fresh[done]
            fl[done] = (fl[done] & ~0xF) | FLAG_RESET | O.legal_mask(fresh)[done]
        boards[t + 1], flags[t + 1] = nb, fl
        points[t], max_tile[t], pot[t] = pts, mx, po
    return boards, flags, points, max_tile, pot


def sampler_reference(logits, legal, u32):
    """float64 masked sampler of n rows: logits [n, 4] (None: zeros), legal uint8 [n] (bit a: action a
    legal), u32 uint32 [n] (word x of the row's stream-1 Philox draw).  Returns (logp [n, 4] with -inf
    on illegal actions, entropy [n] over p > 0, action [n] = the first legal a with u < cdf[a] at
    u = (u32 >> 8) / 2^24 -- the last legal action if there is none, 0 for an empty mask --, dist [n]
    = |u - nearest CDF boundary of a legal action|, inf for an empty mask)."""
    legal = np.asarray(legal, np.int64)
    n = len(legal)
    lg = np.zeros((n, 4)) if logits is None else np.asarray(logits, np.float64).copy()
    ok = ((legal[:, None] >> np.arange(4)) & 1).astype(bool)
    some = ok.any(axis=1)
    lg[~ok] = -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(some, lg.max(axis=1), 0.0)[:, None]
        e = np.where(ok, np.exp(lg - m), 0.0)
        s = e.sum(axis=1, keepdims=True)
        p = np.where(ok, e / np.where(s > 0, s, 1.0), 0.0)
        logp = np.where(ok, (lg - m) - np.log(np.where(s > 0, s, 1.0)), -np.inf)
        ent = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=1)
    ent = np.where(some, ent, 0.0)
    u = (np.asarray(u32, np.uint32) >> 8).astype(np.float64) / 2.0 ** 24
    cdf = np.cumsum(p, axis=1)
    hit = ok & (u[:, None] < cdf)
    last = 3 - np.argmax(ok[:, ::-1], axis=1)
    action = np.where(hit.any(axis=1), np.argmax(hit, axis=1), np.where(some, last, 0))
    dist = np.where(ok, np.abs(cdf - u[:, None]), np.inf).min(axis=1)
    return logp, ent, action.astype(np.uint8), dist
