"""The GameMLP layer kernels (csrc/ppo_update.hip with csrc/ln_row.hpp / csrc/ppo_common.hpp: the dropout keep mask,
ln_act_fwd / ln_act_bwd, mlp_fwd with its slab, fixed-shape and wide kernels, linear_dgrad, wgrad / wgrad_pair,
colsum_batch, head_fwd), each called raw through g2048._lib with its outputs pre-filled with NaN or a sentinel
and held element by element to the fp64 reference of tests/mlp_layer_reference.py (proved on the CPU by
tests/test_mlp_layer_host.py): every stored bf16 output is a correctly rounded bf16 of a value within the
reference's allowance, every fp32 output within the allowance plus one fp32 step; the keep mask, the exact
inputs (signed permutations, small integers: every sum exact in fp32 in any order) and the kernel families'
bitwise contracts exactly.  No element is skipped, bytes past an output stay the sentinel, and every test prints
its worst error / tolerance."""

import numpy as np
import pytest
import torch

import mlp_layer_reference as R

pytestmark = pytest.mark.gpu

SEED = R.MASK_SEED
PAD = 64           # sentinel elements kept past every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible: GPU tests must run on an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from g2048 import _lib
    _lib.load()
    return _lib


# ---------------------------------------------------------------------------------------------------
# Buffers and checks
# ---------------------------------------------------------------------------------------------------
def _bf(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).bfloat16()


def _f32(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


class Out:
    """An output pre-filled with a sentinel (NaN; 0xA5 bytes for uint8) with PAD sentinel elements past its end;
    shift: the view starts `shift` elements past the (256-byte aligned) allocation."""

    def __init__(self, dev, shape, dtype, shift=0):
        n = int(np.prod(shape))
        self.buf = (torch.full((shift + n + PAD,), 0xA5, dtype=dtype, device=dev) if dtype == torch.uint8
                    else torch.full((shift + n + PAD,), float("nan"), dtype=dtype, device=dev))
        self.t = self.buf[shift:shift + n].view(shape)
        self.n, self.shift = n, shift

    def np(self):
        """The output as float64; the bytes before and past it must still be the sentinel."""
        torch.cuda.synchronize()
        rest = torch.cat([self.buf[:self.shift], self.buf[self.shift + self.n:]])
        bad = (rest != 0xA5) if rest.dtype == torch.uint8 else ~torch.isnan(rest)
        assert not bool(bad.any()), "bytes outside the output were written"
        return self.t.float().cpu().numpy().astype(np.float64)


class Worst:
    """The largest error / tolerance of a test, printed at its end."""

    def __init__(self, name):
        self.name, self.w, self.n = name, 0.0, 0

    def add(self, got, x, allow, bf16):
        x, allow = np.broadcast_to(x, got.shape), np.broadcast_to(allow, got.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            step = 0.5 * R_ulp_bf16(np.abs(x) + allow) if bf16 else np.abs(np.spacing(x.astype(np.float32))).astype(np.float64)
            r = np.abs(got - x) / (allow + step)
        self.w = max(self.w, float(np.nanmax(r)) if r.size else 0.0)
        self.n += got.size

    def report(self):
        print(f"\n{self.name}: worst error / tolerance {self.w:.3f} over {self.n} elements")


def R_ulp_bf16(x):
    from urm_block_reference import bf16_ulp
    return bf16_ulp(x)


def _hold(ok, what, got, x, allow):
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} outside the allowance; first at {i}: got {got[i]!r}, "
                             f"reference {np.broadcast_to(x, ok.shape)[i]!r} +- {np.broadcast_to(allow, ok.shape)[i]!r}")


def hold_bf16(w, what, got, x, allow):
    assert got.shape == np.broadcast_shapes(got.shape, np.shape(x))
    _hold(R.check_bf16(got, x, allow), what, got, x, allow)
    w.add(got, x, allow, True)


def hold_f32(w, what, got, x, allow):
    _hold(R.check_f32(got, x, allow), what, got, x, allow)
    w.add(got, x, allow, False)


def hold_equal(w, what, got, want):
    """Bit for bit as values (an exact zero may carry either sign)."""
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    _hold(np.asarray(got == want), what, got, want, 0.0)
    w.n += got.size


def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


class Drop:
    """A g2048_dropout with its device counter kept alive, and the reference's mask of the same draw."""

    def __init__(self, L, dev, p, layer=1, pass_=0, counter=3, counter_dev=None):
        self.args = (p, layer, pass_, SEED, counter, counter_dev)
        self.ctr = None if counter_dev is None else torch.tensor([_signed(counter_dev)], dtype=torch.int64, device=dev)
        self.c = L.make_dropout(p, layer, pass_, SEED, counter, self.ctr) if p > 0 else None

    def mask(self, m, h):
        p, layer, pass_, seed, counter, counter_dev = self.args
        if not p > 0:
            return None, 1.0
        mask, _, scale = R.keep_mask(m, h, p, layer, pass_, seed, counter, counter_dev)
        return mask, scale


# ---------------------------------------------------------------------------------------------------
# a. The dropout mask, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", R.MASK_HS)
def test_dropout_mask_is_the_reference_philox(L, dev, h):
    w = Worst(f"dropout_mask h={h}")
    i = 0
    for p in R.MASK_PS:
        for counter, counter_dev in R.MASK_COUNTERS:
            layer, pass_ = R.MASK_LAYER_PASS[i % len(R.MASK_LAYER_PASS)]
            i += 1
            m = 70 if h <= 260 else 19
            d = Drop(L, dev, p, layer, pass_, counter, counter_dev)
            out = Out(dev, (m, h), torch.uint8)
            L.dropout_mask(m, h, d.c, out.t)
            hold_equal(w, f"p={p} counter={counter}+{counter_dev} layer={layer} pass={pass_}", out.np(), d.mask(m, h)[0].astype(np.float64))
    w.report()


def test_dropout_mask_rows_past_65536(L, dev):
    w = Worst("dropout_mask m=65540")
    m, h = 65540, 4
    d = Drop(L, dev, 0.5, 2, 1, 2 ** 32 - 1, 1)
    out = Out(dev, (m, h), torch.uint8)
    L.dropout_mask(m, h, d.c, out.t)
    hold_equal(w, "mask", out.np(), d.mask(m, h)[0].astype(np.float64))
    w.report()


@pytest.mark.parametrize("h", R.MASK_HS)
def test_consumers_apply_the_reference_mask(L, dev, h):
    """ReLU(LN) > 0 everywhere and no residual: y == 0 marks exactly the dropped elements of ln_act_fwd and of
    every mlp_fwd kernel that takes the shape."""
    w = Worst(f"consumer masks h={h}")
    m = 65540 if h == 4 else (70 if h <= 260 else 19)
    g, gamma, beta, _ = R.positive_case(m, h)
    for i, p in enumerate(R.MASK_PS):
        counter, counter_dev = R.MASK_COUNTERS[i % len(R.MASK_COUNTERS)]
        layer, pass_ = R.MASK_LAYER_PASS[(i + 1) % len(R.MASK_LAYER_PASS)]
        d = Drop(L, dev, p, layer, pass_, counter, counter_dev)
        want = d.mask(m, h)[0].astype(np.float64)
        y, mean, rstd = Out(dev, (m, h), torch.bfloat16), Out(dev, (m,), torch.float32), Out(dev, (m,), torch.float32)
        L.ln_act_fwd(_bf(dev, g), _f32(dev, gamma), _f32(dev, beta), None, y.t, mean.t, rstd.t, d.c)
        got = y.np()
        assert np.isfinite(got).all()
        hold_equal(w, f"ln_act_fwd p={p}", (got != 0).astype(np.float64), want)
        if h <= 256 and L.mlp_fwd_supported(h, h):   # G = x I^T = x: the first rows through mlp_fwd
            eye, mm = _bf(dev, np.eye(h)), min(m, 70)
            for shift in ((0, 4) if h == 196 else (0,)):   # 196: the wide kernel, then (y 8-byte aligned) the slab one
                y2 = Out(dev, (mm, h), torch.bfloat16, shift)
                L.mlp_fwd(_bf(dev, g[:mm]), eye, _f32(dev, gamma), _f32(dev, beta), False, None, y2.t, None, None, d.c)
                hold_equal(w, f"mlp_fwd p={p} shift={shift}", (y2.np() != 0).astype(np.float64), want[:mm])
    w.report()


# ---------------------------------------------------------------------------------------------------
# b. ln_act_fwd
# ---------------------------------------------------------------------------------------------------
def _ln_fwd_check(L, dev, w, kind, m, h, with_res, p, chunk=8192):
    g, gamma, beta, res = R.ln_case(kind, m, h)
    d = Drop(L, dev, p)
    y, mean, rstd = Out(dev, (m, h), torch.bfloat16), Out(dev, (m,), torch.float32), Out(dev, (m,), torch.float32)
    L.ln_act_fwd(_bf(dev, g), _f32(dev, gamma), _f32(dev, beta), _bf(dev, res) if with_res else None, y.t, mean.t, rstd.t, d.c)
    gy, gmean, grstd = y.np(), mean.np(), rstd.np()
    mask, scale = d.mask(m, h)
    what = f"ln_act_fwd {kind} m={m} h={h} res={with_res} p={p}"
    for r0 in range(0, m, chunk):
        s = slice(r0, min(m, r0 + chunk))
        f = R.ln_block_fwd(g[s], gamma, beta, res[s] if with_res else None, None if mask is None else mask[s], scale)
        hold_f32(w, what + " mean", gmean[s], f["mean"], f["mean_allow"])
        hold_f32(w, what + " rstd", grstd[s], f["rstd"], f["rstd_allow"])
        hold_bf16(w, what + " y", gy[s], f["y"], f["y_arith"])


@pytest.mark.parametrize("h", R.LN_FWD_HS)
def test_ln_act_fwd(L, dev, h):
    w = Worst(f"ln_act_fwd h={h}")
    for kind, m, hh, with_res, p in R.ln_fwd_runs():
        if hh == h and m < 4000:
            _ln_fwd_check(L, dev, w, kind, m, h, with_res, p)
    w.report()


def test_ln_act_fwd_wraps_its_grid(L, dev):
    w = Worst("ln_act_fwd wrap")
    for kind, m, h, with_res, p in R.ln_fwd_runs():
        if m >= 4000:
            _ln_fwd_check(L, dev, w, kind, m, h, with_res, p)
    w.report()


# ---------------------------------------------------------------------------------------------------
# c. ln_act_bwd
# ---------------------------------------------------------------------------------------------------
def _ln_bwd_run(L, dev, g, mean, rstd, gamma, beta, dres, ps, hd, d, with_dres_out, alias, shift_dg):
    m, h = g.shape
    dg = Out(dev, (m, h), torch.bfloat16, 4 if shift_dg else 0)
    t_dres = _f32(dev, dres) if dres is not None else None
    dout = None
    if with_dres_out:
        dout = Out(dev, (m, h), torch.float32)
        if alias:
            dout.t.copy_(t_dres)
            t_dres = dout.t
    head = None
    if hd is not None:
        head = (_f32(dev, hd[0]), _f32(dev, hd[1]), _f32(dev, hd[2]) if hd[2] is not None else None)
    npart = L.ln_act_bwd_partials(m, h)
    part = Out(dev, (npart,), torch.float32)
    dgamma, dbeta = Out(dev, (h,), torch.float32), Out(dev, (h,), torch.float32)
    tps = [_bf(dev, q) for q in ps]
    L.ln_act_bwd(None, None, _bf(dev, g), _f32(dev, mean), _f32(dev, rstd), _f32(dev, gamma), _f32(dev, beta), dg.t,
                 dout.t if dout is not None else None, part.t, dgamma.t, dbeta.t, d.c, dy=L.make_dy(t_dres, tps, head))
    # (the scratch past the partial rows is the column sum's own)
    return dg.np(), None if dout is None else dout.np(), part.np(), dgamma.np(), dbeta.np()


def _ln_bwd_check(L, dev, w, run, alias=False):
    kind, h, m, n_src, head, with_dres, p, t196 = run
    g, gamma, beta, dres, ps, hd = R.backward_case(kind, m, h, n_src, head, with_dres, 0)
    mean, rstd = R.given_stats(g)
    d = Drop(L, dev, p)
    mask, scale = d.mask(m, h)
    tile_ok = h == 196 and n_src <= 2 and not with_dres
    shift = tile_ok and not t196          # the same shape forced onto the generic kernel: dg 8- but not 16-byte aligned
    assert t196 <= tile_ok
    dres_out = with_dres or (not t196 and not tile_ok and (m + h) % 2 == 0)
    gdg, gdy, part, gdgamma, gdbeta = _ln_bwd_run(L, dev, g, mean, rstd, gamma, beta, dres, ps, hd, d, dres_out and not t196,
                                                  alias and with_dres, shift)
    b = R.ln_block_bwd(g, mean, rstd, gamma, beta, dres, ps, hd, mask, scale, tile196=t196)
    what = f"ln_act_bwd {run}"
    hold_bf16(w, what + " dg", gdg, b["dg"], b["dg_arith"] + b["dg_flip"])
    if gdy is not None:
        hold_f32(w, what + " dres_out", gdy, b["dy"], b["dy_arith"])
        if hd is None and len(ps) + (dres is not None) <= 1:
            hold_equal(w, what + " dres_out of one source", gdy, R.f32(b["dy"]))
    nb = b["nb"]
    hold_f32(w, what + " partial rows", part[:nb * 2 * h].reshape(nb, 2 * h), b["part"], b["part_arith"] + b["part_flip"])
    hold_f32(w, what + " dgamma", gdgamma, b["dgamma"], b["dgamma_arith"] + b["dgamma_flip"])
    hold_f32(w, what + " dbeta", gdbeta, b["dbeta"], b["dbeta_arith"] + b["dbeta_flip"])
    if kind == "zero_gate":
        assert not gdg.any() and not gdgamma.any() and not gdbeta.any(), what + ": z == 0 must cut the gradient"


def test_ln_act_bwd_generic_kernel(L, dev):
    w = Worst("ln_act_bwd generic")
    for i, run in enumerate(r for r in R.ln_bwd_runs() if not r[7]):
        _ln_bwd_check(L, dev, w, run, alias=i % 2 == 0)
    w.report()


def test_ln_act_bwd_196_tile_kernel(L, dev):
    w = Worst("ln_act_bwd h=196 tile kernel")
    for run in (r for r in R.ln_bwd_runs() if r[7]):
        _ln_bwd_check(L, dev, w, run)
    w.report()


def test_ln_act_bwd_196_shape_forced_onto_the_generic_kernel(L, dev):
    """Three sources, and a dg that is 8- but not 16-byte aligned: both leave the tile kernel."""
    w = Worst("ln_act_bwd h=196 forced generic")
    for m, n_src, head, p in ((129, 3, "coupled", 0.1), (129, 1, "coupled", 0.1), (17, 2, None, 0.0)):
        _ln_bwd_check(L, dev, w, ("gauss", 196, m, n_src, head, False, p, False))
    w.report()


@pytest.mark.parametrize("h,m,p", [(196, R.LN_BWD_WRAP_196, 0.5), (196, R.LN_BWD_WRAP_196, 0.0),
                                   (64, R.LN_BWD_WRAP_GENERIC, 0.5), (64, R.LN_BWD_WRAP_GENERIC, 0.0)])
def test_ln_act_bwd_wraps_its_grid_with_an_exact_dbeta(L, dev, h, m, p):
    """One row past a full sweep of the grid.  Every gate is open (gamma 1/4, beta 8) and dy is one bf16 source of
    integers in [-2, 2] times k in {0, 2}: dbeta is exactly summable and must equal the integer sum bit for bit;
    dg of every row is held to the reference."""
    w = Worst(f"ln_act_bwd wrap h={h} m={m} p={p}")
    g, gamma, beta, _ = R.positive_case(m, h)
    mean, rstd = R.given_stats(g)
    dy = R.small_ints((m, h), 11)
    d = Drop(L, dev, p)
    mask, scale = d.mask(m, h)
    gdg, _, part, gdgamma, gdbeta = _ln_bwd_run(L, dev, g, mean, rstd, gamma, beta, None, [dy], None, d, False, False, False)
    k = np.ones((m, h)) if mask is None else mask * scale
    hold_equal(w, "dbeta", gdbeta, (dy * k).sum(0))
    nb, blk, _ = R.bwd_blocks(m, h, h == 196)
    want = np.zeros((nb, h))
    np.add.at(want, blk, dy * k)
    hold_equal(w, "dbeta partial rows", part[:nb * 2 * h].reshape(nb, 2 * h)[:, h:], want)
    dgam, e_dgam, a_dgam = np.zeros(h), np.zeros(h), np.zeros(h)
    for r0 in range(0, m, 4096):
        s = slice(r0, min(m, r0 + 4096))
        b = R.ln_block_bwd(g[s], mean[s], rstd[s], gamma, beta, None, [dy[s]], None, None if mask is None else mask[s], scale)
        assert not b["amb"].any() and (b["z"] > 0).all()
        hold_bf16(w, "dg", gdg[s], b["dg"], b["dg_arith"])
        dgam += b["terms"][:, :h].sum(0)
        e_dgam += b["terms_err"][:, :h].sum(0)
        a_dgam += np.abs(b["terms"][:, :h]).sum(0)
    hold_f32(w, "dgamma", gdgamma, dgam, e_dgam + R.bwd_chain(m, h, h == 196)[1] * R.U24 * a_dgam)
    w.report()


# ---------------------------------------------------------------------------------------------------
# d. mlp_fwd
# ---------------------------------------------------------------------------------------------------
def _mlp_fwd_check(L, dev, w, m, n, k, res, p, exact, shift_y=False, tag=""):
    rg = np.random.default_rng([m, n, k, int(res), int(exact)])
    x = R.bfv(rg.normal(size=(m, k)))
    wt = R.signed_perm(n, k, 1) if exact else R.bfv(rg.normal(size=(n, k)) / k ** 0.5)
    gamma, beta = R.f32(rg.uniform(0.5, 1.5, size=n)), R.f32(rg.normal(size=n) * 0.1)
    d = Drop(L, dev, p, 2, 1, 2 ** 32 - 1, 1)
    tx, tw, tga, tbe = _bf(dev, x), _bf(dev, wt), _f32(dev, gamma), _f32(dev, beta)
    sh = 4 if shift_y else 0
    G, Y = Out(dev, (m, n), torch.bfloat16), Out(dev, (m, n), torch.bfloat16, sh)
    mean, rstd = Out(dev, (m,), torch.float32), Out(dev, (m,), torch.float32)
    L.mlp_fwd(tx, tw, tga, tbe, res, G.t, Y.t, mean.t, rstd.t, d.c)
    gG, gY, gmean, grstd = G.np(), Y.np(), mean.np(), rstd.np()
    what = f"mlp_fwd{tag} m={m} n={n} k={k} res={res} p={p} {'exact' if exact else 'gauss'}"
    xG, aG = R.linear(x, wt, rounding=not exact)
    if exact:
        hold_equal(w, what + " G", gG, xG)
    else:
        hold_bf16(w, what + " G", gG, xG, aG)
    mask, scale = d.mask(m, n)
    for r0 in range(0, m, 8192):
        s = slice(r0, min(m, r0 + 8192))
        f = R.ln_block_fwd(gG[s], gamma, beta, x[s] if res else None, None if mask is None else mask[s], scale)   # the kernel's own G bits
        hold_f32(w, what + " mean", gmean[s], f["mean"], f["mean_allow"])
        hold_f32(w, what + " rstd", grstd[s], f["rstd"], f["rstd_allow"])
        hold_bf16(w, what + " y", gY[s], f["y"], f["y_arith"])
    # g = NULL (and the inference form without statistics): bitwise the Y, mean and rstd of the storing call
    Y2, mean2, rstd2 = Out(dev, (m, n), torch.bfloat16, sh), Out(dev, (m,), torch.float32), Out(dev, (m,), torch.float32)
    L.mlp_fwd(tx, tw, tga, tbe, res, None, Y2.t, mean2.t, rstd2.t, d.c)
    hold_equal(w, what + " y without g", Y2.np(), gY)
    hold_equal(w, what + " mean without g", mean2.np(), gmean)
    hold_equal(w, what + " rstd without g", rstd2.np(), grstd)
    Y3 = Out(dev, (m, n), torch.bfloat16, sh)
    L.mlp_fwd(tx, tw, tga, tbe, res, None, Y3.t, None, None, d.c)
    hold_equal(w, what + " y without g or statistics", Y3.np(), gY)


def _variants(n, k):
    return [(res, p) for res in ((False, True) if n == k else (False,)) for p in (0.0, 0.1)]


@pytest.mark.parametrize("n", R.MLP_FWD_NS)
def test_mlp_fwd_every_instance(L, dev, n):
    """Both ends of every NT instance's range, k in {4, 36, 48} and k = n (the residual form) where supported."""
    w = Worst(f"mlp_fwd n={n}")
    i = 0
    for k in dict.fromkeys(R.MLP_FWD_KS + (n,)):
        if not L.mlp_fwd_supported(n, k):
            continue
        for res, p in _variants(n, k):
            for exact in (True, False):
                m = R.MLP_FWD_MS[i % len(R.MLP_FWD_MS)]
                i += 1
                _mlp_fwd_check(L, dev, w, m, n, k, res, p, exact)
    assert i > 0
    w.report()


@pytest.mark.parametrize("path", ["generic13", "ks7", "ks2", "wide", "slab196", "unaligned196"])
def test_mlp_fwd_paths(L, dev, path, monkeypatch):
    """The generic NT = 13 instance, the two fixed-KS kernels, the wide kernel, the h = 196 shapes on the slab kernels
    (G2048_MLP_FWD_SLAB) and the slab fallback of a y that is only 8-byte aligned; every m, all variants."""
    w = Worst(f"mlp_fwd {path}")
    shapes = R.MLP_FWD_PATHS.get(path, R.MLP_FWD_PATHS["wide"])
    if path == "slab196":
        monkeypatch.setenv("G2048_MLP_FWD_SLAB", "1")
    for n, k in shapes:
        for j, (res, p) in enumerate(_variants(n, k)):
            for i, m in enumerate(R.MLP_FWD_MS):
                _mlp_fwd_check(L, dev, w, m, n, k, res, p, exact=(i + j) % 2 == 0, shift_y=path == "unaligned196", tag=" " + path)
    w.report()


@pytest.mark.parametrize("path,n,k,m", [("slab", 208, 208, R.MLP_FWD_WRAP_SLAB), ("slab", 64, 36, R.MLP_FWD_WRAP_SLAB),
                                        ("slab196", 196, 196, R.MLP_FWD_WRAP_SLAB), ("wide", 196, 196, R.MLP_FWD_WRAP_WIDE),
                                        ("wide", 196, 48, R.MLP_FWD_WRAP_WIDE)])
def test_mlp_fwd_wraps_its_grid(L, dev, path, n, k, m, monkeypatch):
    w = Worst(f"mlp_fwd wrap {path} n={n} k={k} m={m}")
    if path == "slab196":
        monkeypatch.setenv("G2048_MLP_FWD_SLAB", "1")
    _mlp_fwd_check(L, dev, w, m, n, k, n == k, 0.1, exact=True, tag=" wrap")
    if (n, k) == (196, 196):
        _mlp_fwd_check(L, dev, w, m, n, k, True, 0.1, exact=False, tag=" wrap")
    w.report()


# ---------------------------------------------------------------------------------------------------
# e. linear_dgrad
# ---------------------------------------------------------------------------------------------------
def _dgrad_check(L, dev, w, m, h, exact):
    rg = np.random.default_rng([m, h, int(exact)])
    dg = R.bfv(rg.normal(size=(m, h)))
    wt = R.signed_perm(h, h, 2) if exact else R.bfv(rg.normal(size=(h, h)) / h ** 0.5)
    out = Out(dev, (m, h), torch.bfloat16)
    L.linear_dgrad(_bf(dev, dg), _bf(dev, wt), out.t)
    P, a = R.dgrad(dg, wt, rounding=not exact)
    what = f"linear_dgrad m={m} h={h} {'exact' if exact else 'gauss'}"
    if exact:
        hold_equal(w, what, out.np(), P)
    else:
        hold_bf16(w, what, out.np(), P, a)


@pytest.mark.parametrize("h", R.DGRAD_HS)
def test_linear_dgrad(L, dev, h):
    w = Worst(f"linear_dgrad h={h}")
    assert L.linear_dgrad_supported(h, h)
    for m in R.DGRAD_MS + (R.DGRAD_WRAPS[h],):
        for exact in (True, False):
            _dgrad_check(L, dev, w, m, h, exact)
    w.report()


# ---------------------------------------------------------------------------------------------------
# f. wgrad, wgrad_pair
# ---------------------------------------------------------------------------------------------------
def _wgrad_check(L, dev, w, m, n1, n2, exact, pair=False):
    rg = np.random.default_rng([m, n1, n2, int(exact)])
    mk = (lambda s, seed: R.small_ints(s, seed)) if exact else (lambda s, seed: R.bfv(rg.normal(size=s)))
    ab = [(mk((m, n1), 2 * i + 1), mk((m, n2), 2 * i + 2)) for i in range(2 if pair else 1)]
    npart = L.wgrad_pair_partials(m, n1, n2) if pair else L.wgrad_partials(m, n1, n2)
    assert npart > 0
    outs = [Out(dev, (n1, n2), torch.float32) for _ in ab]
    parts = [Out(dev, (npart,), torch.float32) for _ in ab]
    t = [(_bf(dev, a), _bf(dev, b)) for a, b in ab]
    if pair:
        L.wgrad_pair(t[0][0], t[0][1], t[1][0], t[1][1], parts[0].t, parts[1].t, outs[0].t, outs[1].t)
    else:
        L.wgrad(t[0][0], t[0][1], parts[0].t, outs[0].t)
    for i, ((a, b), o) in enumerate(zip(ab, outs)):
        x, allow = R.wgrad(a, b, rounding=not exact)
        what = f"wgrad{'_pair' if pair else ''}[{i}] m={m} ({n1},{n2}) {'exact' if exact else 'gauss'}"
        if exact:
            hold_equal(w, what, o.np(), x)
        else:
            hold_f32(w, what, o.np(), x, allow)


@pytest.mark.parametrize("n1,n2", R.WGRAD_SHAPES)
def test_wgrad_every_plan(L, dev, n1, n2):
    w = Worst(f"wgrad ({n1},{n2})")
    for m in R.WGRAD_MS:
        _wgrad_check(L, dev, w, m, n1, n2, True)
        _wgrad_check(L, dev, w, m, n1, n2, False)
    for m in (1, 65, 1025, 2049):
        _wgrad_check(L, dev, w, m, n1, n2, True, pair=True)
    _wgrad_check(L, dev, w, 513, n1, n2, False, pair=True)
    w.report()


@pytest.mark.parametrize("nw4", [False, True])
def test_wgrad_196_long_reduction(L, dev, nw4, monkeypatch):
    """131 137 rows: 228 blocks of 576 rows, the last with twelve 32-row k-blocks and one ragged row -- an odd count
    for the k-split 8-wave kernel; small integers, so the sum must be exact.  Once with G2048_WGRAD_NW4."""
    w = Worst(f"wgrad (196,196) m={R.WGRAD_WRAP} nw4={nw4}")
    if nw4:
        monkeypatch.setenv("G2048_WGRAD_NW4", "1")
        for m in (1, 33, 65, 1025):
            _wgrad_check(L, dev, w, m, 196, 196, True)
            _wgrad_check(L, dev, w, m, 196, 196, False)
    _wgrad_check(L, dev, w, R.WGRAD_WRAP, 196, 196, True)
    w.report()


@pytest.mark.parametrize("h", R.MLP_WGRAD_HS)
def test_mlp_wgrad(L, dev, h):
    """The four products of one launch: head [16, h] = dz^T H2, stem [h, 48] = dG0^T x0, blocks [h, h] = dG^T H."""
    w = Worst(f"mlp_wgrad h={h}")
    for m in R.MLP_WGRAD_MS + (R.MLP_WGRAD_WRAP[h],):
        for exact in ((True, False) if m <= 1025 else (True,)):
            rg = np.random.default_rng([m, h, int(exact)])
            mk = (lambda s, seed: R.small_ints(s, seed)) if exact else (lambda s, seed: R.bfv(rg.normal(size=s)))
            shapes = [((m, 16), (m, h)), ((m, h), (m, 48)), ((m, h), (m, h)), ((m, h), (m, h))]
            ab = [(mk(sa, 2 * i + 1), mk(sb, 2 * i + 2)) for i, (sa, sb) in enumerate(shapes)]
            t = [(_bf(dev, a), _bf(dev, b)) for a, b in ab]
            npart = L.mlp_wgrad_partials(m, h)
            assert npart > 0
            part = Out(dev, (npart,), torch.float32)
            outs = [Out(dev, (a.shape[1], b.shape[1]), torch.float32) for a, b in ab]
            L.mlp_wgrad(m, t[0][0], t[0][1], [t[1][0], t[2][0], t[3][0]], [t[1][1], t[2][1], t[3][1]], part.t, outs[0].t,
                        [o.t for o in outs[1:]])
            part.np()
            for name, (a, b), o in zip(("head", "stem", "block 1", "block 2"), ab, outs):
                x, allow = R.wgrad(a, b, rounding=not exact)
                what = f"mlp_wgrad {name} m={m} h={h} {'exact' if exact else 'gauss'}"
                if exact:
                    hold_equal(w, what, o.np(), x)
                else:
                    hold_f32(w, what, o.np(), x, allow)
    w.report()


# ---------------------------------------------------------------------------------------------------
# g. colsum_batch, head_fwd
# ---------------------------------------------------------------------------------------------------
def _segments(cols):
    if cols < 4:
        return (cols,)
    a = max(1, cols // 7)
    b = max(1, cols // 3)
    return (a, b, 1, cols - a - b - 1)


@pytest.mark.parametrize("nb", R.COLSUM_NBS)
def test_colsum_batch(L, dev, nb):
    """Every (nb, cols) in one batch per input kind: uneven segments, max_col -1 and 1, a part that is only 4-byte
    aligned (the one-column-per-lane form) beside the float2 form."""
    w = Worst(f"colsum_batch nb={nb}")
    for exact in (True, False):
        jobs, checks, keep = [], [], []
        for i, cols in enumerate(R.COLSUM_COLS):
            for max_col in (-1, 1):
                rg = np.random.default_rng([nb, cols, max_col + 1, int(exact)])
                part = R.small_ints((nb, cols), 5, -1000, 1000) if exact else R.f32(rg.normal(size=(nb, cols)))
                shift = 1 if (i + max_col) % 2 == 0 else 0
                buf = torch.zeros(shift + nb * cols, dtype=torch.float32, device=dev)
                tp = buf[shift:]
                tp.copy_(_f32(dev, part).view(-1))
                segs = _segments(cols)
                outs = [Out(dev, (n,), torch.float32) for n in segs]
                job = L.ColsumJob()
                job.part, job.nb, job.cols, job.max_col, job.nseg = tp.data_ptr(), nb, cols, max_col, len(segs)
                for s, (o, n) in enumerate(zip(outs, segs)):
                    job.dst[s], job.len[s] = o.t.data_ptr(), n
                jobs.append(job)
                keep.append(buf)
                checks.append((part, segs, max_col, outs, cols))
        assert len(jobs) <= L.COLSUM_MAX_JOBS
        L.colsum_batch(jobs)
        first = [[o.np() for o in c[3]] for c in checks]
        # colsum_batch_sq, as far as its header documents it: the same sums, sq[b] of the blocks past the launch's
        # grid zero, the sum of sq = the sum of squares of the segments marked in pad_, *tick += 1
        for j, job in enumerate(jobs):
            job.pad_ = 0b101 if j % 2 == 0 else 0
        nblk = L.colsum_batch_blocks(jobs)
        assert 0 < nblk <= L.COLSUM_SQ_MAX
        sq, tick = Out(dev, (nblk + 3,), torch.float32), torch.full((1,), 41.0, device=dev)
        for c in checks:
            for o in c[3]:
                o.t.fill_(float("nan"))
        L.colsum_batch_sq(jobs, sq.t, tick)
        gsq = sq.np()
        assert float(tick.item()) == 42.0 and not gsq[nblk:].any()
        marked = np.concatenate([first[j][s] for j in range(len(jobs)) if j % 2 == 0 for s in (0, 2) if s < len(first[j])])
        hold_f32(w, f"colsum_batch_sq nb={nb} sum of squares", gsq.sum(keepdims=True), (marked ** 2).sum(keepdims=True),
                 (marked.size + nblk + 4) * R.U24 * (marked ** 2).sum(keepdims=True))
        for c, f in zip(checks, first):
            for o, x in zip(c[3], f):
                hold_equal(w, f"colsum_batch_sq nb={nb} sums", o.np(), x)
        for part, segs, max_col, outs, cols in checks:
            for s, ((x, allow), o) in enumerate(zip(R.colsum(part, segs, max_col), outs)):
                what = f"colsum nb={nb} cols={cols} max_col={max_col} segment {s} {'exact' if exact else 'gauss'}"
                if exact:
                    hold_equal(w, what, o.np(), x)
                else:
                    hold_f32(w, what, o.np(), x, allow)
    w.report()


@pytest.mark.parametrize("h", R.HEAD_HS)
def test_head_fwd(L, dev, h):
    w = Worst(f"head_fwd h={h}")
    for i, m in enumerate(R.HEAD_MS):
        for onehot in (True, False):
            rg = np.random.default_rng([m, h, int(onehot)])
            x = R.bfv(rg.normal(size=(m, h)))
            if onehot:    # head a reads feature (a * 7 + 3) % h: the outputs are copies of x plus a bias
                wa, wv = np.zeros((4, h)), np.zeros(h)
                cols = [(a * 7 + 3) % h for a in range(5)]
                wa[np.arange(4), cols[:4]] = (1.0, -1.0, 2.0, -0.5)
                wv[cols[4]] = 1.0
                ba, bv = np.zeros(4), np.zeros(1)
            else:
                wa, wv = R.f32(rg.normal(size=(4, h)) * 0.05), R.f32(rg.normal(size=h) * 0.05)
                ba, bv = R.f32(rg.normal(size=4) * 0.1), R.f32(rg.normal(size=1) * 0.1)
            stride = 4 if (i + onehot) % 2 == 0 else 6
            lg, val = Out(dev, (m, stride), torch.float32), Out(dev, (m,), torch.float32)
            L.head_fwd(_bf(dev, x), _f32(dev, wa), _f32(dev, ba), _f32(dev, wv), _f32(dev, bv), lg.t, val.t)
            glg, gval = lg.np(), val.np()
            assert np.isnan(glg[:, 4:]).all(), "the padding of a wider logits row must stay the sentinel"
            xl, xv, al, av = R.head_fwd(x, wa, ba, wv, bv)
            what = f"head_fwd m={m} h={h} stride={stride} {'one-hot' if onehot else 'gauss'}"
            if onehot:
                hold_equal(w, what + " logits", glg[:, :4], xl)
                hold_equal(w, what + " value", gval, xv)
            else:
                hold_f32(w, what + " logits", glg[:, :4], xl, al)
                hold_f32(w, what + " value", gval, xv, av)
    w.report()
