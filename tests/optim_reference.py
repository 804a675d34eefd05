"""fp64 restatement of one optimizer step (g2048/optim.py, csrc/optim.hip), stage by stage, in plain
torch-CPU float64: the gradient clip, Muon's momentum, the bf16 cast and normalisation of its update,
the Newton-Schulz iteration (fp64, no intermediate rounding), the decayed and scaled update, and
AdamW.  Every stage is a function of its inputs alone, so a test compares one stage at a time.
Shared by tests/test_optim_host.py (which checks these functions against torch.optim.Muon / AdamW and
against the scalar quintic) and tests/test_gpu_optim.py; not a test module itself."""

import math

import torch

F64 = torch.float64
NS = (3.4445, -4.775, 2.0315)   # torch.optim.Muon's default Newton-Schulz coefficients
NS_EPS = 1e-7
SPECTRUM = (0.8, 0.5, 0.3, 0.1)  # the singular values of the spectral cases


def f64(t):
    return torch.as_tensor(t).detach().to("cpu", F64)


def clip(flat, max_norm):
    """clip_grad_norm_'s -> (norm, coef = min(max_norm / (norm + 1e-6), 1)), Python floats."""
    norm = math.sqrt(float((f64(flat) ** 2).sum()))
    return norm, min(max_norm / (norm + 1e-6), 1.0)


def muon_momentum(g, buf, coef, mu, nesterov):
    """torch.optim.Muon's momentum on the clipped gradient coef * g: buf.lerp_(g, 1 - mu), then the
    update g.lerp(buf, mu) (nesterov) or buf.  -> (new buffer, update u)."""
    gc = f64(g) * coef
    buf = f64(buf)
    new = buf + (1.0 - mu) * (gc - buf)
    u = gc + mu * (new - gc) if nesterov else new
    return new, u


def bf16(x):
    """x rounded to bf16 (round to nearest even), as fp64."""
    return f64(x).to(torch.float32).to(torch.bfloat16).to(F64)


def muon_input(u, transpose, eps=NS_EPS):
    """The Newton-Schulz input of update u: u rounded to bf16, on the wide orientation (transposed when
    `transpose`), divided by max(bf16(its Frobenius norm), eps) -- x.norm() of a bf16 tensor is a bf16
    value -- and the quotient rounded to bf16 like every bf16 tensor operation's result."""
    x = bf16(u)
    if transpose:
        x = x.T
    nrm = max(float(bf16(torch.linalg.matrix_norm(x))), eps)
    return bf16(x / nrm)


def newton_schulz(x0, a, b, c, steps):
    """`steps` iterations of G = X X^T; U = b G + c G G; X = a X + U X in fp64."""
    x = f64(x0)
    for _ in range(steps):
        g = x @ x.T
        x = a * x + (b * g + c * (g @ g)) @ x
    return x


def muon_direction(u, steps, ns=NS, eps=NS_EPS):
    """The orthogonalised update of u in u's own orientation (muon_input, newton_schulz, transposed back)."""
    tr = u.shape[0] > u.shape[1]
    x = newton_schulz(muon_input(u, tr, eps), *ns, steps)
    return x.T if tr else x


def muon_apply(p, x, lr, wd, rows, cols):
    """Decoupled weight decay and the match_rms_adamw-scaled update."""
    return f64(p) * (1.0 - lr * wd) - f64(x) * (lr * 0.2 * math.sqrt(max(rows, cols)))


def adamw(p, g, m, v, t, lr, coef, b1, b2, eps, wd):
    """One torch.optim.AdamW step (decoupled decay, bias corrections at step count t, the one AFTER the
    increment) on the clipped gradient coef * g.  -> (p, exp_avg, exp_avg_sq)."""
    gc = f64(g) * coef
    p, m, v = f64(p), f64(m), f64(v)
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (gc - m)
    v = b2 * v + (1.0 - b2) * gc * gc
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


# The bounds of the GPU comparisons, stated once: tests/test_gpu_optim.py asserts them and
# tests/test_optim_host.py shows that each one rejects a wrong term.
MOMENT_RTOL = 5e-6  # exp_avg / exp_avg_sq: 4 fp32 roundings, twice the clip coefficient's error for exp_avg_sq


def momentum_tol(g, buf_prev, coef):
    """|muon_buf - ref| elementwise: three fp32 roundings plus the clip coefficient's error."""
    return 8 * 2.0 ** -24 * ((f64(g) * coef).abs() + f64(buf_prev).abs())


def decay_tol(p):
    """|p_new - p (1 - lr wd)| of a pure-decay step: the roundings of 1 - lr wd and of the product."""
    return 2.0 ** -23 * f64(p).abs()


def adamw_move_tol(dp_ref, p):
    """|dp - dp_ref|: 1e-4 relative (what a bias correction 1 - b2^t formed in fp32 may cost: up to
    2^-24 b2 / (1 - b2) = 6e-5 at t = 1) plus one rounding of the parameter."""
    return 1e-4 * f64(dp_ref).abs() + 2.0 ** -23 * f64(p).abs()


def phi(sigma, k, ns=NS):
    """The scalar quintic a s + b s^3 + c s^5 iterated k times: what Newton-Schulz does to a singular value."""
    a, b, c = ns
    s = float(sigma)
    for _ in range(k):
        s = a * s + b * s ** 3 + c * s ** 5
    return s


def spectral(rows, cols, seed=0):
    """-> (G [rows, cols] fp64 = sum_i s_i u_i v_i^T of rank min(4, rows, cols), U [rows, k], V [cols, k], s [k]):
    singular values SPECTRUM, singular vectors from seeded fp64 QR factorisations."""
    k = min(4, rows, cols)
    gen = torch.Generator().manual_seed(1000 * rows + cols + seed)
    u = torch.linalg.qr(torch.randn(rows, k, dtype=F64, generator=gen))[0]
    v = torch.linalg.qr(torch.randn(cols, k, dtype=F64, generator=gen))[0]
    s = torch.tensor(SPECTRUM[:k], dtype=F64)
    return (u * s) @ v.T, u, v, s


def spectral_coefficients(x, u, v):
    """c_i = u_i^T X v_i for X in G's orientation."""
    return torch.einsum("ri,rc,ci->i", u, f64(x), v)
