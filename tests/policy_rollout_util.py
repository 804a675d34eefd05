"""Shared helpers of the fused policy rollout tests (test_gpu_policy_rollout.py and
test_gpu_policy_rollout_edges.py): a GameMLP with non-trivial heads, one rollout through the fused
kernel or the per-step path, and the bitwise comparison of two sets of records."""

import torch

FIELDS = ("boards", "flags", "actions", "logp", "entropy", "value", "points", "max_tile", "pot")


def _model(dev, h, seed):
    import agent
    torch.manual_seed(seed)
    m = agent.GameMLP(agent.MLPConfig(hidden_dim=h, num_layers=2)).to(dev)
    with torch.no_grad():  # non-trivial heads and LayerNorm affines (the trainer zeroes the heads)
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.05)
        m.action_head.weight.mul_(20.0)
    return m.eval()


def _run(dev, m, n, T, fused, episodic=False, seed=9, chunks=None, env_base=0, hook=None):
    """One rollout's records.  `hook(ro, t0)` is called after ro.reset() -- and, given as a dict
    {t0: hook}, before the first chunk that starts at t0 -- and may overwrite ro.buf.boards[t0] for
    chosen envs; ro.buf.flags[t0] is then recomputed from the boards (g2048_legal_mask, legal bits)."""
    from g2048 import _lib as L
    from g2048.rollout import FusedPolicy, Rollout
    pol = FusedPolicy(m)
    ro = Rollout(n, T, dev, seed=seed, env_base=env_base, episodic=episodic)
    ro.use_fused = fused
    assert ro.fused(pol) == fused
    ro.reset()
    hooks = hook if isinstance(hook, dict) else ({} if hook is None else {(chunks or [(0, T)])[0][0]: hook})
    for t0, t1 in chunks or [(0, T)]:
        if t0 in hooks:
            hooks[t0](ro, t0)
            L.legal_mask(ro.buf.boards[t0], ro.buf.flags[t0])
            ro.buf.flags[t0].bitwise_and_(L.FLAG_LEGAL)
        ro.steps(t0, t1, pol)
    torch.cuda.synchronize()
    return {k: getattr(ro.buf, k).clone() for k in FIELDS}


def _assert_same(a, b):
    for k in FIELDS:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:  # bitwise, -inf included
            x, y = x.view(torch.int32), y.view(torch.int32)
        bad = (x != y).reshape(x.shape[0], x.shape[1], -1).any(-1)
        assert not bool(bad.any()), (k, int(bad.sum()), torch.nonzero(bad)[:5].tolist())
