"""The fp64 optimizer reference (tests/optim_reference.py) is right before anything is compared with
it: its AdamW and Muon momentum against torch.optim on fp64 parameters, its Newton-Schulz against the
scalar quintic on gradients of known singular values, and the proof that the comparisons of
tests/test_gpu_optim.py separate a wrong coefficient, momentum, decay, learning rate or step count
from rounding noise.  CPU only."""

import math

import pytest
import torch

import optim_reference as R

F64 = torch.float64
SPECTRAL_SHAPES = [(196, 196), (196, 48), (32, 32), (4, 196), (128, 128)]


def test_reference_adamw_matches_torch_adamw():
    """5 steps, two groups of different lr, wd 0.1: parameters and both moments at rtol 1e-12."""
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, dtype=F64, generator=gen)) for n in (7, 1031)]
    lrs, b1, b2, eps, wd = (2e-3, 5e-4), 0.9, 0.999, 1e-8, 0.1
    opt = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], betas=(b1, b2), eps=eps,
                            weight_decay=wd)
    ref = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    for t in range(1, 6):
        for k, p in enumerate(ps):
            p.grad = torch.randn(p.shape, dtype=F64, generator=gen) * (p.detach().abs() > 0.3)  # some exact zeros
            ref[k] = R.adamw(*ref[k][:1], p.grad, *ref[k][1:], t, lrs[k], 1.0, b1, b2, eps, wd)
        opt.step()
        for k, p in enumerate(ps):
            st = opt.state[p]
            torch.testing.assert_close(ref[k][0], p.detach(), rtol=1e-12, atol=0)
            torch.testing.assert_close(ref[k][1], st["exp_avg"], rtol=1e-12, atol=0)
            torch.testing.assert_close(ref[k][2], st["exp_avg_sq"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("nesterov", [True, False])
def test_reference_momentum_matches_torch_muon(nesterov):
    """3 steps of torch.optim.Muon on an fp64 matrix: state[p]["momentum_buffer"] at atol 1e-15."""
    gen = torch.Generator().manual_seed(4)
    p = torch.nn.Parameter(torch.randn(12, 20, dtype=F64, generator=gen) / 4)
    opt = torch.optim.Muon([p], lr=2e-3, weight_decay=0.01, momentum=0.95, nesterov=nesterov,
                           adjust_lr_fn="match_rms_adamw")
    buf = torch.zeros_like(p)
    for _ in range(3):
        p.grad = torch.randn(p.shape, dtype=F64, generator=gen)
        buf, _ = R.muon_momentum(p.grad, buf, 1.0, 0.95, nesterov)
        opt.step()
        torch.testing.assert_close(buf, opt.state[p]["momentum_buffer"], rtol=0, atol=1e-15)


def test_zero_gradient_muon_step_is_pure_decay():
    """A zero-gradient torch.optim.Muon step is exactly p (1 - lr wd); the reference gives the same bits."""
    gen = torch.Generator().manual_seed(5)
    p = torch.nn.Parameter(torch.randn(12, 20, dtype=F64, generator=gen))
    p0 = p.detach().clone()
    lr, wd = 2e-3, 0.25
    opt = torch.optim.Muon([p], lr=lr, weight_decay=wd, adjust_lr_fn="match_rms_adamw")
    p.grad = torch.zeros_like(p)
    opt.step()
    assert torch.equal(p.detach(), p0 * (1 - lr * wd))
    _, u = R.muon_momentum(p.grad, torch.zeros_like(p0), 1.0, 0.95, True)
    assert torch.equal(R.muon_apply(p0, R.muon_direction(u, 5), lr, wd, *p0.shape), p.detach())


def _coefficients(shape, k, ns=R.NS):
    g, u, v, s = R.spectral(*shape)
    return R.spectral_coefficients(R.muon_direction(g, k, ns), u, v), s


@pytest.mark.parametrize("shape", SPECTRAL_SHAPES)
@pytest.mark.parametrize("k", [1, 5])
def test_reference_newton_schulz_is_the_quintic_on_singular_values(shape, k):
    """G = sum_i s_i u_i v_i^T.  The iteration itself is the quintic: from the unrounded G / ||s|| the
    c_i = u_i^T X_k v_i are phi(s_i / ||s||, k) to 1e-12.  Through muon_input they are phi(sigma_i, k) within
    1e-3 for sigma_i = u_i^T X_0 v_i, the coefficients of the bf16 input the iteration really starts from, and
    those lie within three bf16 roundings (element, norm, quotient: 3 * 2^-8 of ||X_0||_F = 1) of s_i / ||s||.
    phi(s_i / ||s||, k) itself is NOT met within 1e-3: ||G||_F = ||s|| = 0.99499 rounds to the bf16 255/256,
    1.1e-3 too large, which every bf16 mantissa M / 128 divided by it answers by rounding up to (M + 1) / 128 --
    a systematic shift of every sigma_i by about 5e-4 that phi'(sigma) sigma turns into 1.3e-3 .. 2.1e-3 at
    k = 5 (printed below)."""
    g, u, v, s = R.spectral(*shape)
    sn = s / s.norm()
    tr = shape[0] > shape[1]
    exact = R.newton_schulz((g.T if tr else g) / float(s.norm()), *R.NS, k)
    ce = R.spectral_coefficients(exact.T if tr else exact, u, v)
    assert float((ce - torch.tensor([R.phi(float(x), k) for x in sn], dtype=F64)).abs().max()) <= 1e-12
    x0 = R.muon_input(g, tr)
    sig = R.spectral_coefficients(x0.T if tr else x0, u, v)
    assert float((sig - sn).abs().max()) <= 3 * 2.0 ** -8
    c, _ = _coefficients(shape, k)
    want = torch.tensor([R.phi(float(x), k) for x in sig], dtype=F64)
    err = float((c - want).abs().max())
    naive = float((c - torch.tensor([R.phi(float(x), k) for x in sn], dtype=F64)).abs().max())
    print(f"spectral {shape} k={k}: max |c - phi(sigma)| = {err:.2e}, max |c - phi(s / ||s||)| = {naive:.2e}")
    assert err <= 1e-3, (c, want)


@pytest.mark.parametrize("shape", SPECTRAL_SHAPES)
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("which,factor", [(0, 1.01), (1, 1.02), (2, 1.05)])
def test_spectral_coefficients_expose_a_wrong_newton_schulz_coefficient(shape, k, which, factor):
    """a off by 1 %, b by 2 % or c by 5 % moves some c_i by at least 2.5e-2: far above the bf16 noise the
    GPU spectral comparison allows, so that comparison fails on a wrong coefficient."""
    c, _ = _coefficients(shape, k)
    ns = list(R.NS)
    ns[which] *= factor
    wrong, _ = _coefficients(shape, k, tuple(ns))
    d = float((wrong - c).abs().max())
    print(f"sensitivity {shape} k={k} coefficient {which} x {factor}: {d:.2e}")
    assert d >= 2.5e-2


# ---- the bounds of tests/test_gpu_optim.py reject a wrong term: the reference fed a wrong input against
# ---- the reference itself, with the GPU tests' tolerances (optim_reference.*_tol)

def _fp32(x):
    return x.to(torch.float32).to(F64)


def test_momentum_bound_rejects_a_momentum_of_0_90():
    gen = torch.Generator().manual_seed(6)
    g = _fp32(torch.randn(64, 120, dtype=F64, generator=gen))
    buf = _fp32(torch.randn(64, 120, dtype=F64, generator=gen) * 0.3)
    good, _ = R.muon_momentum(g, buf, 0.7, 0.95, True)
    bad, _ = R.muon_momentum(g, buf, 0.7, 0.90, True)
    tol = R.momentum_tol(g, buf, 0.7)
    assert ((_fp32(good) - good).abs() <= tol).all()  # an fp32 rounding of the right value passes
    assert ((bad - good).abs() > tol).any()


def test_decay_bound_rejects_a_dropped_decay_and_the_other_groups_lr():
    gen = torch.Generator().manual_seed(7)
    p = _fp32(torch.randn(64, 64, dtype=F64, generator=gen) / 8)
    zero = torch.zeros_like(p)
    wd = 0.25
    for lr, other in ((2e-3, 5e-4), (5e-4, 2e-3), (2e-3 * 0.37, 5e-4 * 0.37)):
        good = R.muon_apply(p, zero, lr, wd, 64, 64)
        tol = R.decay_tol(p)
        assert ((_fp32(good) - good).abs() <= tol).all()
        assert ((R.muon_apply(p, zero, lr, 0.0, 64, 64) - good).abs() > tol).any()    # decay dropped
        assert ((R.muon_apply(p, zero, other, wd, 64, 64) - good).abs() > tol).any()  # the other group's lr
        a_good = R.adamw(p[0], zero[0], zero[0], zero[0], 1, lr, 1.0, 0.9, 0.999, 1e-8, wd)[0]
        a_other = R.adamw(p[0], zero[0], zero[0], zero[0], 1, other, 1.0, 0.9, 0.999, 1e-8, wd)[0]
        a_none = R.adamw(p[0], zero[0], zero[0], zero[0], 1, lr, 1.0, 0.9, 0.999, 1e-8, 0.0)[0]
        assert ((a_other - a_good).abs() > R.decay_tol(p[0])).any() and ((a_none - a_good).abs() > R.decay_tol(p[0])).any()


@pytest.mark.parametrize("t0", [0, 1, 999])
def test_adamw_bounds_reject_a_step_count_off_by_one(t0):
    """t + 1 for t moves the parameter change outside adamw_move_tol (the first of the GPU test's three
    steps; the moments do not depend on t, so the parameter move is what sees it).  Not at t0 = 99 999:
    both bias corrections are 1 there whatever the count, which is what that case of the GPU test is for."""
    gen = torch.Generator().manual_seed(8)
    p = _fp32(torch.randn(1031, dtype=F64, generator=gen))
    g = _fp32(torch.randn(1031, dtype=F64, generator=gen))
    z = torch.zeros_like(p)
    args = (2e-3, 0.8, 0.9, 0.999, 1e-8, 0.1)
    good = R.adamw(p, g, z, z, t0 + 1, *args)[0]
    bad = R.adamw(p, g, z, z, t0 + 2, *args)[0]
    assert ((bad - good).abs() > R.adamw_move_tol(good - p, p)).any()
    # and the moments' rtol sees a wrong momentum coefficient / a dropped clip coefficient
    _, m, v = R.adamw(p, g, z, z, t0 + 1, *args)
    _, m2, v2 = R.adamw(p, g, z, z, t0 + 1, 2e-3, 1.0, 0.9, 0.999, 1e-8, 0.1)
    assert ((m2 - m).abs() > R.MOMENT_RTOL * m.abs()).any() and ((v2 - v).abs() > R.MOMENT_RTOL * v.abs()).any()


def test_phi_is_the_quintic():
    a, b, c = R.NS
    assert math.isclose(R.phi(0.5, 1), a * 0.5 + b * 0.125 + c * 0.03125, rel_tol=1e-15)
    assert math.isclose(R.phi(0.5, 2), R.phi(R.phi(0.5, 1), 1), rel_tol=1e-15)
