"""The fused Muon + AdamW step (g2048/optim.py FusedMuonAdamW, csrc/optim.hip) term by term against the
fp64 restatement tests/optim_reference.py (itself checked by tests/test_optim_host.py): the clip's norm
and coefficient, the momentum buffers, the weight decay with each group's learning rate, lr = 0, the
Newton-Schulz iterate, AdamW's moments and parameter move, step() against step_clipped, and the bf16
copies.  Every expected value is the fp64 reference's, elementwise and with no element left out; only
test_step_equals_step_clipped compares two kernels of the project (and says why).

The optimizers run on a stub module whose get_param_groups returns exactly the matrices and 1-D tensors a
case asks for, in agent._split_param_groups' order: the matrices alternate between the "other" group
(lr 2e-3) and the value group (lr 5e-4), so an update made with the wrong group's rate is visible.

The Newton-Schulz bound is relative to torch's own bf16 error: E = ||X - X_ref||_F / ||X_ref||_F (Gaussian
gradients) and D = max_i |c_i - c_i,ref| (gradients of known singular vectors, c_i = u_i^T X v_i) are
measured for the kernel and for MuonAdamW._newton_schulz (torch bf16 ops on the device) against the fp64
iteration from the same bf16 input, and the kernel must stay within 2 x torch's + 1e-3: both round to bf16
at the same three points per iteration, in different accumulation orders.  tests/test_optim_host.py shows
that 1 % / 2 % / 5 % of error in a / b / c moves some c_i by >= 2.5e-2.  Observed on an MI355X (kernel /
torch):

    shape        E, 1 step            E, 5 steps           D, 1 step            D, 5 steps
    [196,196]    1.66e-3 / 1.66e-3    1.07e-2 / 1.09e-2    3.73e-5 / 3.68e-5    8.15e-4 / 8.15e-4
    [192,192]    1.67e-3 / 1.67e-3    1.08e-2 / 1.11e-2
    [128,128]    1.64e-3 / 1.64e-3    1.09e-2 / 1.07e-2    8.25e-5 / 8.24e-5    3.20e-4 / 2.75e-4
    [64,64]      1.65e-3 / 1.65e-3    1.27e-2 / 1.27e-2
    [32,32]      1.68e-3 / 1.68e-3    1.37e-2 / 1.37e-2    2.67e-4 / 2.67e-4    2.69e-3 / 2.69e-3
    [196,48]     1.66e-3 / 1.66e-3    1.54e-2 / 1.53e-2    1.94e-4 / 1.94e-4    1.07e-3 / 7.87e-4
    [4,196]      1.94e-3 / 1.94e-3    1.48e-2 / 1.48e-2    1.01e-3 / 1.01e-3    9.59e-3 / 9.59e-3
    [1,196]      1.14e-2 / 1.14e-2    9.69e-3 / 9.69e-3
    [64,3]       2.17e-3 / 2.17e-3    1.88e-2 / 1.88e-2
    [240,64]     1.68e-3 / 1.68e-3    1.37e-2 / 1.41e-2
    [64,120]     1.66e-3 / 1.66e-3    1.45e-2 / 1.45e-2

([196,196] and [192,192] on one CU, 5 steps: the multi-CU figures to the digits shown.  [1,196]'s E is the
bf16 rounding of the one Gram entry its iteration turns on.  ||p_new||_F / expected: 0.991 .. 1.021, the
widest on the rank-4 gradients at 5 steps.)
"""

import math

import pytest
import torch
from torch import nn

import optim_reference as R

pytestmark = pytest.mark.gpu

LR, CRITIC_LR = 2e-3, 5e-4  # the "other" groups / the value groups
# the smallest shapes that take each code path of muon_kernel
SHAPES = [(196, 196),   # multi-CU at the default MUON_PARTS
          (192, 192),
          (128, 128), (64, 64), (32, 32),  # the square schedules
          (196, 48),    # transposed
          (4, 196),     # head, wide
          (1, 196),     # rank 1: Newton-Schulz is a normalisation
          (64, 3),      # the per-element pass
          (240, 64), (64, 120)]  # generic, the GameURM shapes
SPECTRAL_SHAPES = [(196, 196), (196, 48), (32, 32), (4, 196), (128, 128)]
ONES = (7, 1031)  # the 1-D groups: no multiples of 4, the second spans more than one 1 024-thread block
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_schedules(monkeypatch):
    for name in ("G2048_MUON_PARTS", "G2048_MUON_GENERIC", "G2048_MUON_ONE_CU"):
        monkeypatch.delenv(name, raising=False)


class Stub(nn.Module):
    """`mats` [rows, cols] matrices (even positions: the other group, odd: the value group; every numel a
    multiple of 4, so the GradBucket views stay 16-byte aligned) and the two 1-D tensors of `ones` = (other,
    value) elements (0: none)."""

    def __init__(self, mats, ones, seed, zero):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        assert all((r * c) % 4 == 0 for r, c in mats)
        self.mats = nn.ParameterList(
            nn.Parameter(torch.zeros(r, c) if zero else torch.randn(r, c, generator=gen) / math.sqrt(c)) for r, c in mats)
        self.ones = nn.ParameterList(nn.Parameter(torch.randn(max(n, 1), generator=gen)) for n in ones)
        self.have = [n > 0 for n in ones]

    def get_param_groups(self, value_lr, other_lr):
        mats = list(self.mats)
        return [{"params": mats[0::2], "lr": other_lr}, {"params": [self.ones[0]] if self.have[0] else [], "lr": other_lr},
                {"params": mats[1::2], "lr": value_lr}, {"params": [self.ones[1]] if self.have[1] else [], "lr": value_lr}]


def _make(dev, mats, ones=ONES, seed=0, zero=False, copies=False, cls=None, **kw):
    """-> (optimizer, GradBucket ordered as the optimizer tests order it: Muon matrices, then the AdamW groups)."""
    from g2048.dist import GradBucket
    from g2048.optim import FusedMuonAdamW
    model = Stub(mats, ones, seed, zero).to(dev)
    opt = (cls or FusedMuonAdamW)(model, LR, CRITIC_LR, **kw)
    if cls is None:
        assert opt.supported
    order = [p for p, _ in opt.muon] + [p for grp in opt.adam_groups for p in grp["params"]]
    bk = GradBucket(order)
    assert sum(p.numel() for p in order) == sum(r * c for r, c in mats) + sum(ones)
    if copies:
        opt.copies = {p: torch.zeros_like(p, dtype=torch.bfloat16) for p, _ in opt.muon}
        opt.set_bf16_copies(opt.copies)
    return opt, bk


def _group_lr(gi, scale=1.0):
    return (LR if gi < 2 else CRITIC_LR) * scale


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _run(opt, bk, entry):
    """One step through `entry`; -> the clip coefficient the fp64 reference gives for it."""
    flat = bk.flat.cpu()
    if entry == "step":
        opt.step()
        coef = 1.0
    else:
        opt.step_clipped(bk.flat, 1.0)
        coef = R.clip(flat, 1.0)[1]
    torch.cuda.synchronize()
    return coef


def _grads(opt):
    return [R.f64(p.grad) for p, _ in opt.muon], [R.f64(opt._flat_grad(g)) for g in opt.adam_groups]


def _state(opt):
    return {"p": [R.f64(p) for p, _ in opt.muon], "buf": [R.f64(b) for b in opt.muon_buf],
            "flat": [R.f64(g["flat"]) for g in opt.adam_groups], "m": [R.f64(g["m"]) for g in opt.adam_groups],
            "v": [R.f64(g["v"]) for g in opt.adam_groups]}


def _within(got, want, tol, what):
    err = (R.f64(got) - want).abs()
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst " \
                          f"|err| {float(err.max()):.3e} (err / bound {float((err / tol.clamp(min=1e-300))[bad].max()):.2f})"


def _check_momentum(opt, before, grads, coef, mu, nesterov):
    for (p, _), prev, g, buf in zip(opt.muon, before["buf"], grads, opt.muon_buf):
        want, _ = R.muon_momentum(g, prev, coef, mu, nesterov)
        _within(buf, want, R.momentum_tol(g, prev, coef), f"muon_buf {tuple(p.shape)}")


def _check_moments(opt, before, grads1d, coef):
    for grp, m0, v0, g in zip(opt.adam_groups, before["m"], before["v"], grads1d):
        _, m, v = R.adamw(g, g, m0, v0, 1, 0.0, coef, B1, B2, ADAM_EPS, 0.0)
        _within(grp["m"], m, R.MOMENT_RTOL * m.abs(), f"exp_avg of group {grp['idx']}")
        _within(grp["v"], v, R.MOMENT_RTOL * v.abs(), f"exp_avg_sq of group {grp['idx']}")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- (a) the clip --------------------------------------------------------------------------------------
CLIP_STUBS = {4: ([(1, 4)], (0, 0)), 5: ([(1, 4)], (1, 0)), 7: ([(1, 4)], (0, 3)), 1023: ([(4, 196)], (7, 232)),
              65539: ([(196, 196), (128, 128)], (7, 10732))}


@pytest.mark.parametrize("n", [4, 5, 7, 1023, 65539])
def test_clip_norm_and_coefficient(dev, n):
    """step_clipped(flat, 1.0) without given partials: norm_t and coef_t against fp64 at rtol 2e-6 (fp32 sums
    of at most n / 65 536 + 20 positive terms per lane, then a tree) for N(0, 3^2) gradients; the same
    gradients scaled to a norm of 0.5 and the all-zero gradient give a coefficient of exactly 1."""
    opt, bk = _make(dev, *CLIP_STUBS[n])
    assert bk.flat.numel() == n
    g = _randn(n, n, 3.0)
    small = g * (0.5 / float(g.double().norm()))
    for name, grad in (("clipped", g), ("below 1", small), ("zero", torch.zeros(n))):
        bk.flat.copy_(grad)
        out = opt.step_clipped(bk.flat, 1.0)
        torch.cuda.synchronize()
        assert out is opt.norm_t
        norm, coef = R.clip(grad, 1.0)
        got_n, got_c = float(opt.norm_t), float(opt.coef_t)
        print(f"clip n={n} {name}: norm {got_n!r} (fp64 {norm!r}), coef {got_c!r} (fp64 {coef!r})")
        if name == "zero":
            assert got_n == 0.0 and got_c == 1.0
            continue
        assert math.isclose(got_n, norm, rel_tol=2e-6), (name, got_n, norm)
        assert math.isclose(got_c, coef, rel_tol=2e-6), (name, got_c, coef)
        assert (coef < 1.0) if name == "clipped" else (coef == 1.0 and got_c == 1.0)
    assert float(opt.step_t) == 3.0


@pytest.mark.parametrize("L", [1, 63, 64, 65, 511, 512, 513, 1024])
def test_clip_from_given_partials(dev, L):
    """step_clipped(..., sq=) with L hand-filled positive partials (the boundaries of clip_sumsq's 8 x 64
    unrolled loop): norm_t = sqrt(sum sq) at rtol 2e-6, and the coefficient it gives is the one the momentum
    buffers were built with.  The step count is advanced here, as g2048_colsum_batch_sq would."""
    opt, bk = _make(dev, [(4, 196), (64, 3)], (7, 0))
    sq = torch.rand(L, generator=torch.Generator().manual_seed(L)) * 4 + 0.01
    for k, part in enumerate((sq * (9.0 / float(sq.sum())), sq * (0.25 / float(sq.double().sum())))):
        # (an element keeps its sign over the two steps: exp_avg does not cancel, see test_adamw_moments_and_move)
        bk.flat.copy_(_randn(bk.flat.shape, 100 * L + k).abs() * torch.sign(_randn(bk.flat.shape, L)))
        before, (g2d, g1d) = _state(opt), _grads(opt)
        opt.step_t.add_(1)
        opt.step_clipped(bk.flat, 1.0, sq=part.to(dev))
        torch.cuda.synchronize()
        norm = math.sqrt(float(part.double().sum()))
        coef = min(1.0 / (norm + 1e-6), 1.0)
        assert math.isclose(float(opt.norm_t), norm, rel_tol=2e-6), (L, float(opt.norm_t), norm)
        assert math.isclose(float(opt.coef_t), coef, rel_tol=2e-6), (L, float(opt.coef_t), coef)
        assert (coef < 0.34) if k == 0 else (float(opt.coef_t) == 1.0)
        _check_momentum(opt, before, g2d, coef, 0.95, True)
        _check_moments(opt, before, g1d, coef)
        assert float(opt.step_t) == k + 1.0


# ---- (b) momentum --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("momentum", [0.95, 0.5])
def test_momentum_buffers(dev, nesterov, momentum):
    """Every shape, 3 steps (step 0 clipped, the others of norm < 1): after each step every momentum buffer
    is the fp64 muon_momentum of the gradient, the buffer before the step and the fp64 clip coefficient,
    within 8 * 2^-24 (|coef g| + |buf_prev|) elementwise (three fp32 roundings, the coefficient's error)."""
    opt, bk = _make(dev, SHAPES, momentum=momentum, nesterov=nesterov)
    n = bk.flat.numel()
    for s in range(3):
        bk.flat.copy_(_randn(n, 10 + s, 3.0 if s == 0 else 0.5 / math.sqrt(n)))
        before, (g2d, _) = _state(opt), _grads(opt)
        coef = _run(opt, bk, "step_clipped")
        assert (coef < 1e-2) if s == 0 else (coef == 1.0)
        _check_momentum(opt, before, g2d, coef, momentum, nesterov)


# ---- (c) weight decay and the group's learning rate ---------------------------------------------------
@pytest.mark.parametrize("entry", ["step_clipped", "step"])
def test_pure_decay_uses_each_groups_learning_rate(dev, entry):
    """weight_decay 0.25, zero gradient, zero buffers: the update is exactly zero, so every Muon matrix and
    AdamW tensor becomes p (1 - lr_group wd) within 2^-23 |p| -- the two groups' factors differ by 3.75e-4.
    Again after set_lr_scale(0.37)."""
    opt, bk = _make(dev, SHAPES, weight_decay=0.25)
    for t, scale in enumerate((1.0, 0.37), 1):
        if scale != 1.0:
            opt.set_lr_scale(scale)
        before = _state(opt)
        assert _run(opt, bk, entry) == 1.0
        for (p, gi), p0, buf in zip(opt.muon, before["p"], opt.muon_buf):
            want = R.muon_apply(p0, torch.zeros_like(p0), _group_lr(gi, scale), 0.25, *p.shape)
            _within(p, want, R.decay_tol(p0), f"matrix {tuple(p.shape)} of group {gi} at lr scale {scale}")
            assert not buf.any()
        for grp, p0 in zip(opt.adam_groups, before["flat"]):
            z = torch.zeros_like(p0)
            want = R.adamw(p0, z, z, z, t, _group_lr(grp["idx"], scale), 1.0, B1, B2, ADAM_EPS, 0.25)[0]
            _within(grp["flat"], want, R.decay_tol(p0), f"1-D group {grp['idx']} at lr scale {scale}")
            assert not grp["m"].any() and not grp["v"].any()
            assert grp["params"][0].data_ptr() == grp["flat"].data_ptr()  # the model's tensor is what moved


# ---- (d) lr = 0 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step_clipped", "step"])
def test_lr_zero_leaves_parameters_bitwise_unchanged(dev, entry):
    """The first step of every scheduled run (cosine_with_warmup(0) = 0): after set_lr_scale(0.0) one step
    with N(0, 1) gradients leaves every parameter bitwise unchanged (p * 1 - x * 0 and p - 0 * m / (...) with
    finite x), every registered bf16 copy is RNE(bf16) of its parameter, and the momentum buffers, AdamW's
    moments and the step count advance as with any other rate."""
    opt, bk = _make(dev, SHAPES, copies=True)
    opt.set_lr_scale(0.0)
    bk.flat.copy_(_randn(bk.flat.shape, 40))
    before, (g2d, g1d) = _state(opt), _grads(opt)
    bits = [_bits(p.detach()).clone() for p, _ in opt.muon] + [_bits(g["flat"]).clone() for g in opt.adam_groups]
    coef = _run(opt, bk, entry)
    assert (coef < 1e-2) if entry == "step_clipped" else (coef == 1.0)
    after = [_bits(p.detach()) for p, _ in opt.muon] + [_bits(g["flat"]) for g in opt.adam_groups]
    for k, (a, b) in enumerate(zip(after, bits)):
        assert torch.equal(a, b), f"tensor {k}: {int((a != b).sum())} elements changed at lr = 0"
    for p, c in opt.copies.items():
        assert torch.equal(_bits(c), _bits(p.detach().to(torch.bfloat16))), tuple(p.shape)
    _check_momentum(opt, before, g2d, coef, 0.95, True)
    _check_moments(opt, before, g1d, coef)
    assert float(opt.step_t) == 1.0


# ---- (e) Newton-Schulz ---------------------------------------------------------------------------------
def _ns_run(dev, steps, kind, shapes=None):
    """First step from zero buffers, zero parameters and wd = 0 through step() (coefficient exactly 1): the
    kernel's iterate is X = -p_new / (lr 0.2 sqrt(max(R, C))).  -> {shape: record}."""
    from g2048.optim import MuonAdamW
    shapes = shapes or (SHAPES if kind == "gaussian" else SPECTRAL_SHAPES)
    opt, bk = _make(dev, shapes, (0, 0), zero=True, copies=True, weight_decay=0.0, ns_steps=steps)
    yard, _ = _make(dev, [(4, 4)], (0, 0), cls=MuonAdamW, ns_steps=steps)
    basis = {}
    for p, _ in opt.muon:
        r, c = p.shape
        if kind == "gaussian":
            p.grad.copy_(_randn((r, c), 1000 * r + c))
        else:
            g, u, v, _ = R.spectral(r, c)
            p.grad.copy_(g.float())
            basis[(r, c)] = (u, v)
    g2d, _ = _grads(opt)
    assert _run(opt, bk, "step") == 1.0
    out = {}
    for (p, gi), g in zip(opt.muon, g2d):
        r, c = p.shape
        _, u = R.muon_momentum(g, torch.zeros_like(g), 1.0, 0.95, True)
        rec = {"scale": _group_lr(gi) * 0.2 * math.sqrt(max(r, c)), "p": p.detach().cpu(), "copy": opt.copies[p].cpu(),
               "x_ref": R.muon_direction(u, steps), "x_torch": R.f64(yard._newton_schulz(u.float().to(dev))),
               "basis": basis.get((r, c))}
        rec["x"] = -R.f64(p) / rec["scale"]
        out[(r, c)] = rec
    out["parts"] = opt._cfg.parts
    return out


_NS_CACHE = {}


def _ns_case(dev, steps, kind):
    if (steps, kind) not in _NS_CACHE:
        _NS_CACHE[(steps, kind)] = _ns_run(dev, steps, kind)
    return _NS_CACHE[(steps, kind)]


def _check_ns(recs, steps, kind, tag=""):
    failures = []
    for shape, rec in recs.items():
        if shape == "parts":
            continue
        x, ref, xt = rec["x"], rec["x_ref"], rec["x_torch"]
        assert torch.isfinite(x).all(), shape
        if kind == "gaussian":
            mk, mt = float((x - ref).norm() / ref.norm()), float((xt - ref).norm() / ref.norm())
            name = "E"
        else:
            cr = R.spectral_coefficients(ref, *rec["basis"])
            mk = float((R.spectral_coefficients(x, *rec["basis"]) - cr).abs().max())
            mt = float((R.spectral_coefficients(xt, *rec["basis"]) - cr).abs().max())
            name = "D"
        # the move's scale: ||p_new||_F against lr 0.2 sqrt(max(R, C)) ||X_ref||_F, with E's bound
        te = float((xt - ref).norm() / ref.norm())
        size = float(R.f64(rec["p"]).norm()) / (rec["scale"] * float(ref.norm()))
        print(f"NS {kind}{tag} steps={steps} {shape}: {name}_kernel {mk:.2e} {name}_torch {mt:.2e} |p_new| / expected {size:.5f}")
        if not mk <= 2 * mt + 1e-3:
            failures.append(f"{shape}: {name}_kernel {mk:.3e} > 2 * {name}_torch {mt:.3e} + 1e-3")
        if not abs(size - 1.0) <= 2 * te + 1e-3:
            failures.append(f"{shape}: |p_new|_F / expected {size:.5f} outside 1 +- (2 * E_torch {te:.3e} + 1e-3)")
    assert not failures, f"{kind} {steps} steps: " + "; ".join(failures)


@pytest.mark.parametrize("steps", [1, 5])
def test_newton_schulz_on_gaussian_gradients(dev, steps):
    """ns_steps 1 and 5 on every shape with N(0, 1) gradients: E_kernel <= 2 E_torch + 1e-3, and the move has
    the match_rms_adamw size.  [196, 196] and [192, 192] run on the default 13 CUs each."""
    recs = _ns_case(dev, steps, "gaussian")
    assert recs["parts"] == 13
    _check_ns(recs, steps, "gaussian")


@pytest.mark.parametrize("steps", [1, 5])
def test_newton_schulz_on_known_singular_vectors(dev, steps):
    """Gradients sum_i s_i u_i v_i^T of rank <= 4: the kernel's coefficients c_i = u_i^T X v_i stay within
    2 D_torch + 1e-3 of the fp64 iteration's.  A wrong a, b or c moves them by >= 2.5e-2
    (tests/test_optim_host.py)."""
    _check_ns(_ns_case(dev, steps, "spectral"), steps, "spectral")


def test_newton_schulz_on_one_cu(dev, monkeypatch):
    """[196, 196] and [192, 192] on the one-CU square schedule (G2048_MUON_PARTS=1), 5 steps."""
    monkeypatch.setenv("G2048_MUON_PARTS", "1")
    for kind in ("gaussian", "spectral"):
        recs = _ns_run(dev, 5, kind, [(196, 196)] if kind == "spectral" else [(196, 196), (192, 192)])
        assert recs["parts"] == 0
        _check_ns(recs, 5, kind, " one-CU")


# ---- (h) the bf16 copies -------------------------------------------------------------------------------
def test_bf16_copies_are_the_rounded_parameters(dev):
    """Every registered copy of the Gaussian five-step case is bitwise RNE(bf16) of its updated fp32
    parameter, [64, 3]'s per-element path and the transposed [196, 48] included."""
    recs = _ns_case(dev, 5, "gaussian")
    for shape, rec in recs.items():
        if shape == "parts":
            continue
        assert rec["p"].any(), shape
        assert torch.equal(_bits(rec["copy"]), _bits(rec["p"].to(torch.bfloat16))), shape


# ---- (f) AdamW -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step_clipped", "step"])
@pytest.mark.parametrize("t0", [0, 1, 999, 99999])
def test_adamw_moments_and_move(dev, entry, t0):
    """The two 1-D groups, wd 0.1, 3 steps from step count t0 through step_clipped (the Muon launch's AdamW
    blocks) and through step() (adamw_kernel): after each step the moments at rtol 5e-6 and the parameter
    move within 1e-4 |dp_ref| + 2^-23 |p| of one fp64 AdamW step from the state before it.  The gradients
    are N(0, 1) with exact zeros; an element keeps its sign over the three steps, so exp_avg never cancels
    and its relative bound means what it says."""
    opt, bk = _make(dev, [(4, 196)], weight_decay=0.1)
    opt.step_t.fill_(float(t0))
    n = bk.flat.numel()
    sign = torch.sign(_randn(n, 50 + t0))
    sign[::5] = 0.0
    for s in range(3):
        bk.flat.copy_(_randn(n, 60 + s).abs() * sign)
        before, (_, g1d) = _state(opt), _grads(opt)
        coef = _run(opt, bk, entry)
        t = t0 + s + 1
        assert float(opt.step_t) == float(t)
        for grp, p0, m0, v0, g in zip(opt.adam_groups, before["flat"], before["m"], before["v"], g1d):
            assert (g == 0).any() and (g != 0).any()
            p, m, v = R.adamw(p0, g, m0, v0, t, _group_lr(grp["idx"]), coef, B1, B2, ADAM_EPS, 0.1)
            what = f"group {grp['idx']} ({g.numel()} elements), step {t}"
            _within(grp["m"], m, R.MOMENT_RTOL * m.abs(), "exp_avg of " + what)
            _within(grp["v"], v, R.MOMENT_RTOL * v.abs(), "exp_avg_sq of " + what)
            _within(R.f64(grp["flat"]) - p0, p - p0, R.adamw_move_tol(p - p0, p0), "parameter move of " + what)


# ---- (g) step() against step_clipped -------------------------------------------------------------------
def test_step_equals_step_clipped(dev):
    """From the same state and gradients of norm < 1 (coefficient exactly 1.0), step() -- g2048_muon_step
    without clip plus g2048_adamw_step, the path PPOUpdater takes -- and step_clipped(flat, 1.0) leave
    parameters, momentum buffers and moments bitwise equal, over two steps of one stub holding every shape.
    The one comparison of two kernels here: it states that the two entry points are the same arithmetic;
    either is pinned to fp64 by the tests above."""
    outs = []
    for entry in ("step", "step_clipped"):
        opt, bk = _make(dev, SHAPES, copies=True)
        n = bk.flat.numel()
        for s in range(2):
            bk.flat.copy_(_randn(n, 70 + s, 0.5 / math.sqrt(n)))
            assert _run(opt, bk, entry) == 1.0
        if entry == "step_clipped":
            assert float(opt.coef_t) == 1.0
        outs.append([p.detach() for p, _ in opt.muon] + list(opt.muon_buf) + list(opt.copies.values()) +
                    [t for g in opt.adam_groups for t in (g["flat"], g["m"], g["v"])] + [opt.step_t])
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(_bits(a), _bits(b)), f"tensor {k} {tuple(a.shape)}: {int((_bits(a) != _bits(b)).sum())} elements differ"
