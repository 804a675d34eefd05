"""The URM training-path kernels between the projections (csrc/urm.hip: attention forward / backward with the
Philox dropout mask, SwiGLU-conv forward / backward / column sum, residual RMSNorm forward / backward), each
called raw through g2048._lib and held element by element to the fp64 reference of
tests/urm_block_reference.py (proved on the CPU by tests/test_urm_block_host.py): every stored bf16 output is
a correctly rounded bf16 of a value within the reference's allowance, every fp32 output within the allowance
plus one fp32 step; the dropout mask, the thr == 0 convention, the all-dropped edge and the kernel families'
bitwise contracts (board = head kernels, pair = one-channel kernels, forward mask = backward mask) exactly.
No element is skipped."""

import numpy as np
import pytest
import torch

import urm_block_reference as R

pytestmark = pytest.mark.gpu

SEED = R.MASK_SEED                 # both key words set
COUNTERS = ((0, 0), (2 ** 32 - 1, 3), (2 ** 33 + 5, 0))   # (counter, offset): low word, a carry, the high word
DROP_PS = (2.0 ** -16, 0.1, 0.5, 0.9, 1 - 2.0 ** -16, 1 - 2.0 ** -18, 1e-6)
GENERIC = R.GENERIC_SHAPES


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


def _shift(t, elems):
    """The same values `elems` elements past an allocation's (256-byte aligned) start."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _bf(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).bfloat16()


def _f32(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def _np(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy().astype(np.float64)


def _hold(ok, what, got, x, allow):
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} outside the allowance; first at {i}: got {got[i]!r}, "
                             f"reference {x[i]!r} +- {np.broadcast_to(allow, ok.shape)[i]!r}")


def hold_bf16(what, got, x, allow):
    _hold(R.check_bf16(got, x, allow), what, got, x, allow)


def hold_f32(what, got, x, allow):
    _hold(R.check_f32(got, x, allow), what, got, x, allow)


# ---------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------
def _attn_run(L, dev, qkv, dout, heads, p=0.0, counter=0, offset=0, shift=False, bwd=True):
    """out [16 n, h] and dqkv [16 n, 3 h] (None without bwd) as float64; shift: buffers 8 bytes past a 16-byte
    boundary, which selects the per-(board, head) kernels for head_dim 16."""
    sh = (lambda t: _shift(t, 4)) if shift else (lambda t: t)
    q = sh(_bf(dev, qkv))
    out = sh(torch.full((qkv.shape[0], qkv.shape[1] // 3), float("nan"), dtype=torch.bfloat16, device=dev))
    ctr = torch.tensor([counter - 2 ** 64 if counter >= 2 ** 63 else counter], dtype=torch.int64, device=dev)
    if shift:
        assert q.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
    L.urm_attention(q, out, heads, p, SEED, ctr, offset)
    dq = None
    if bwd:
        d = sh(_bf(dev, dout))
        dq = sh(torch.full(tuple(qkv.shape), float("nan"), dtype=torch.bfloat16, device=dev))
        L.urm_attention_bwd(q, d, dq, heads, p, SEED, ctr, offset)
    return _np(out), None if dq is None else _np(dq)


def _attn_hold(what, qkv, dout, heads, p, counter, offset, out, dq):
    n, h = qkv.shape[0] // 16, qkv.shape[1] // 3
    q, k, v = R.split_heads(qkv, heads)
    thr, _ = R.drop_args(p)
    km = None if thr == 0 else R.keep_mask(n, heads, p, SEED, counter, offset)
    f = R.attn_fwd(q, k, v, km)
    hold_bf16(what + " O", out, R.merge_heads(f["O"]), R.merge_heads(f["O_arith"] + f["O_flip"]))
    if dq is None:
        return
    dO = R.split_heads(np.concatenate([dout] * 3, 1), heads)[0]
    b = R.attn_bwd(q, k, v, dO, km)
    for i, name in enumerate(("dQ", "dK", "dV")):
        hold_bf16(f"{what} {name}", dq[:, i * h:(i + 1) * h], R.merge_heads(b[name]),
                  R.merge_heads(b[name + "_arith"] + b[name + "_flip"]))
    if not dout.any():
        assert not dq.any(), what + ": zero dout must give exactly zero gradients"


def _attn_classes(L, dev, n, h, heads, shift, bwd, what):
    for kind in R.ATTN_KINDS[1:]:
        for dk in (R.DOUT_KINDS if bwd and kind == "onehot" else ("gauss",)):
            qkv, dout = R.attn_case(kind, n, h, heads, 0, dk)
            out, dq = _attn_run(L, dev, qkv, dout, heads, shift=shift, bwd=bwd)
            _attn_hold(f"{what} {kind}/{dk}", qkv, dout, heads, 0.0, 0, 0, out, dq)
    for seed, dk, p, counter, offset in R.attn_gauss_runs(bwd):   # the runs the host test audits
        qkv, dout = R.attn_case("gauss", n, h, heads, seed, dk)
        out, dq = _attn_run(L, dev, qkv, dout, heads, p, counter, offset, shift=shift, bwd=bwd)
        _attn_hold(f"{what} gauss/{dk} p={p}", qkv, dout, heads, p, counter, offset, out, dq)


@pytest.mark.parametrize("heads", [1, 2, 3, 4])
def test_attention_board_kernels(L, dev, heads):
    """One wave per board, four boards per block: n 1, 3, 4, 5, 9 include a partial last block."""
    for h, hd, n, bwd in R.ATTN_FAMILIES["board"]:
        if hd == heads:
            _attn_classes(L, dev, n, h, heads, False, bwd, f"board n={n} heads={heads}")


@pytest.mark.parametrize("h,heads,n,bwd", R.ATTN_FAMILIES["head"])
def test_attention_head_kernels(L, dev, h, heads, n, bwd):
    """One wave per (board, head): on 8-byte-shifted buffers at h <= 64, always above."""
    _attn_classes(L, dev, n, h, heads, h <= 64, bwd, f"head h={h}")


@pytest.mark.parametrize("h,heads,n,bwd", R.ATTN_FAMILIES["generic"])
def test_attention_generic_forward(L, dev, h, heads, n, bwd):
    """urm_attn_kernel at head_dim 64, 32 (whole chunks), 12, 4, 20 (a padded last chunk) and 49, 3, 1 (the
    unaligned scalar path), with and without dropout."""
    _attn_classes(L, dev, n, h, heads, False, bwd, f"generic h={h} heads={heads}")


def _mask_bits(L, dev, n, h, heads, p, counter, offset, shift, bwd):
    """The device mask read back through q = k = 0, V = 16 I: forward O and (head_dim 16) backward dV."""
    hd = h // heads
    km = R.keep_mask(n, heads, p, SEED, counter, offset)
    dout = np.zeros((n, heads, 16, hd))
    dout[:, :, np.arange(16), np.arange(16) % hd] = 16.0
    dout = R.merge_heads(dout)
    for part in range(-(-16 // hd)):
        qkv = R.mask_probe(n, h, heads, part)
        out, dq = _attn_run(L, dev, qkv, dout, heads, p, counter, offset, shift=shift, bwd=bwd)
        q, k, v = R.split_heads(qkv, heads)
        f = R.attn_fwd(q, k, v, km)
        assert not f["O_flip"].any()
        what = f"mask h={h} heads={heads} p={p} counter={counter}+{offset} part={part}"
        assert np.array_equal(out, R.merge_heads(f["O"])), what + ": forward"
        if bwd:
            b = R.attn_bwd(q, k, v, R.split_heads(np.concatenate([dout] * 3, 1), heads)[0], km)
            assert not b["dV_flip"].any()
            assert np.array_equal(dq[:, 2 * h:], R.merge_heads(b["dV"])), what + ": backward dV"
            assert not dq[:, :2 * h].any()


@pytest.mark.parametrize("family", ["board", "head", "h512", "generic"])
def test_attention_dropout_mask_bit_for_bit(L, dev, family):
    """Every keep bit of every (board, head, query, key), at every threshold edge and counter word, in the
    forward and (head_dim 16) through dV = Pd^T dO in the backward."""
    shapes = {"board": [(64, 4, False, True), (48, 3, False, True)], "head": [(64, 4, True, True)],
              "h512": [(512, 32, False, True)], "generic": [(hh, hd, False, False) for hh, hd in GENERIC]}[family]
    for h, heads, shift, bwd in shapes:
        for p in DROP_PS[:-1]:
            for counter, offset in (COUNTERS if p in (0.5, 2.0 ** -16) else COUNTERS[1:2]):
                _mask_bits(L, dev, 5 if h < 512 else 3, h, heads, p, counter, offset, shift, bwd)


@pytest.mark.parametrize("h,heads,shift,bwd", [(64, 4, False, True), (64, 4, True, True), (512, 32, False, True),
                                               (36, 3, False, False), (196, 4, False, False)])
def test_attention_threshold_zero_and_all_dropped(L, dev, h, heads, shift, bwd):
    """p = 1e-6 rounds to thr 0: bitwise the p = 0 outputs (no mask, no scale).  p = 1 - 2^-18 rounds to thr
    65536: everything dropped at scale 2^18, outputs and gradients exactly 0 (not NaN)."""
    qkv, dout = R.attn_case("gauss", 5, h, heads, 2)
    base = _attn_run(L, dev, qkv, dout, heads, shift=shift, bwd=bwd)
    tiny = _attn_run(L, dev, qkv, dout, heads, 1e-6, 7, 0, shift=shift, bwd=bwd)
    gone = _attn_run(L, dev, qkv, dout, heads, 1 - 2.0 ** -18, 7, 0, shift=shift, bwd=bwd)
    for a, b, c in zip(base, tiny, gone):
        if a is not None:
            assert np.array_equal(a, b) and a.any()
            assert np.array_equal(c, np.zeros_like(c))


# ---------------------------------------------------------------------------------------------------
# SwiGLU + depthwise conv
# ---------------------------------------------------------------------------------------------------
def _swiglu_run(L, dev, gu, w, b, dact, shift):
    """act, dgu, partial rows [nrows, 3, inter], dw, db as float64.  shift: gu / act / dact / dgu 2 bytes past a
    4-byte boundary, which selects the one-channel kernels at an even inter."""
    inter = dact.shape[1]
    nb = gu.shape[0] // 16
    sh = (lambda t: _shift(t, 1)) if shift else (lambda t: t)
    g, d = sh(_bf(dev, gu)), sh(_bf(dev, dact))
    if shift:
        assert g.data_ptr() % 4 == 2 and d.data_ptr() % 4 == 2
    act = sh(torch.full((16 * nb, inter), float("nan"), dtype=torch.bfloat16, device=dev))
    dgu = sh(torch.full((16 * nb, 2 * inter), float("nan"), dtype=torch.bfloat16, device=dev))
    wt, bt = _f32(dev, w), _f32(dev, b)
    nrows = R.sc_rows(nb)
    assert L.urm_swiglu_conv_partials(nb, inter) == nrows * 3 * inter
    part = torch.full((nrows, 3, inter), float("nan"), device=dev)
    dw, db = torch.full((inter, 2), float("nan"), device=dev), torch.full((inter,), float("nan"), device=dev)
    L.urm_swiglu_conv_fwd(g, wt, bt, act)
    L.urm_swiglu_conv_bwd(g, wt, bt, d, dgu, dw, db, part)
    return _np(act), _np(dgu), _np(part), _np(dw), _np(db)


def _swiglu_hold(what, gu, w, b, dact, res):
    act, dgu, part, dw, db = res
    inter = dact.shape[1]
    nb = gu.shape[0] // 16
    g, u = R.split_gu(gu, inter)
    r = R.swiglu_conv(g, u, w, b, dact.reshape(nb, 16, inter))
    flat = lambda x: x.reshape(16 * nb, inter)  # noqa: E731
    hold_bf16(what + " act", act, flat(r["act"]), flat(r["act_arith"] + r["act_flip"]))
    hold_bf16(what + " dgate", dgu[:, :inter], flat(r["dgate"]), flat(r["dgate_arith"] + r["dgate_flip"]))
    hold_bf16(what + " dup", dgu[:, inter:], flat(r["dup"]), flat(r["dup_arith"] + r["dup_flip"]))
    val, allow = R.partial_rows(r["terms"], R.sc_rows(nb))
    hold_f32(what + " partial rows", part, val, allow)
    wdw, wdb, adw, adb = R.colsum(part)
    hold_f32(what + " dw", dw, wdw, adw)
    hold_f32(what + " db", db, wdb, adb)


def _swiglu_both(L, dev, what, gu, w, b, dact):
    """Aligned run held to the reference; at an even inter also the 2-byte-shifted run (the one-channel
    kernels), bit for bit the aligned (pair) run."""
    res = _swiglu_run(L, dev, gu, w, b, dact, False)
    _swiglu_hold(what, gu, w, b, dact, res)
    if dact.shape[1] % 2 == 0:
        one = _swiglu_run(L, dev, gu, w, b, dact, True)
        _swiglu_hold(what + " (one-channel)", gu, w, b, dact, one)
        for name, x, y in zip(("act", "dgu", "partial rows", "dw", "db"), res, one):
            assert np.array_equal(x, y), (f"{what}: pair and one-channel kernels differ in {name}: "
                                          f"{int((x != y).sum())} of {x.size}, first at {tuple(np.argwhere(x != y)[0])}")


@pytest.mark.parametrize("inter", R.SWIGLU_INTERS)
def test_swiglu_conv_shapes(L, dev, inter):
    for kind, nb, _, seed in R.SWIGLU_SHAPE_RUNS[inter]:
        _swiglu_both(L, dev, f"swiglu {kind} n={nb} inter={inter}", *R.swiglu_case(kind, nb, inter, seed))


@pytest.mark.parametrize("kind", ["edges", "leak", "flat"])
@pytest.mark.parametrize("inter", [8, 119])
def test_swiglu_conv_values(L, dev, kind, inter):
    """Gate edges (+-0, silu''s zero, +-20, +-88.5, +-100, +-3e38), y2 on silu''s zero, and a 2^100 last
    token with w0 = 1 that a read across the board boundary would carry into the next board's token 0."""
    _swiglu_both(L, dev, f"swiglu {kind} inter={inter}", *R.swiglu_case(kind, 5, inter, 0))


@pytest.mark.parametrize("nb", R.SWIGLU_WRAPS)
def test_swiglu_conv_grid_wraps(L, dev, nb):
    """Past 2048 partial rows / one-channel blocks a row takes boards row, row + 2048, ...; past 4096 x 4
    boards the pair forward wraps.  Both families at inter 8."""
    _swiglu_both(L, dev, f"swiglu wrap n={nb}", *R.swiglu_case("gauss", nb, 8, 0))
    if nb == 2049:   # a y carried over from the board a thread handled before is enormous here
        _swiglu_both(L, dev, f"swiglu wrap leak n={nb}", *R.swiglu_case("leak", nb, 8, 0))


@pytest.mark.parametrize("nblk", R.COLSUM_NBLK)
def test_swiglu_conv_colsum(L, dev, nblk):
    """The column sum's 8-deep unrolled loop (k + 112 < nblk) and its tail: dw / db against the fp64 sum of the
    partial rows read back, the rows against the reference's per-row sums."""
    gu, w, b, dact = R.swiglu_case("gauss", nblk, 8, 1)
    res = _swiglu_run(L, dev, gu, w, b, dact, False)
    assert res[2].shape[0] == nblk
    _swiglu_hold(f"colsum nblk={nblk}", gu, w, b, dact, res)


# ---------------------------------------------------------------------------------------------------
# Residual RMSNorm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 48, 65537, 65552])
@pytest.mark.parametrize("a_bf16", [True, False])
def test_residual_rms(L, dev, rows, a_bf16):
    """Forward with and without the bf16 copy (bitwise bf16(out)), backward from dout, doutb, both, and -- at
    whole boards -- dpool and dpool + doutb; zero, 1e-20, 1e18 and Gaussian rows; 65 537 rows pass the
    grid-stride wrap at 4096 blocks x 16 rows."""
    h, a, _ = R.rms_case(rows, a_bf16, 0)
    ht = _f32(dev, h)
    at = _bf(dev, a) if a_bf16 else _f32(dev, a)
    ref = R.rms_res_fwd(h, a, R.RMS_EPS)
    outs = []
    for with_b in (False, True):
        out = torch.full((rows, 64), float("nan"), device=dev)
        rstd = torch.full((rows,), float("nan"), device=dev)
        outb = torch.full((rows, 64), float("nan"), dtype=torch.bfloat16, device=dev) if with_b else None
        L.urm_rms_res_fwd(ht, at, out, rstd, R.RMS_EPS, outb)
        hold_f32("rms out", _np(out), ref["out"], ref["out_allow"])
        hold_f32("rms rstd", _np(rstd), ref["r"], ref["r_allow"])
        if with_b:
            assert torch.equal(outb, out.bfloat16())
        outs.append((out, rstd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    out, rstd = outs[0]
    o64, r64 = _np(out), _np(rstd)
    g = np.random.default_rng(rows)
    dout = g.normal(size=(rows, 64)).astype(np.float32).astype(np.float64)
    doutb = R._bfv(g.normal(size=(rows, 64)))
    dpool = g.normal(size=(max(rows // 16, 1), 64)).astype(np.float32).astype(np.float64)
    modes = [("dout", dout, None, None), ("doutb", None, None, doutb), ("dout+doutb", dout, None, doutb)]
    if rows % 16 == 0:
        modes += [("dpool", None, dpool, None), ("dpool+doutb", None, dpool, doutb)]
    for name, d, dp, db in modes:
        dh = torch.full((rows, 64), float("nan"), device=dev)
        da = torch.full((rows, 64), float("nan"), dtype=torch.bfloat16 if a_bf16 else torch.float32, device=dev)
        L.urm_rms_res_bwd(None if d is None else _f32(dev, d), out, rstd, dh, da,
                          doutb=None if db is None else _bf(dev, db), dpool=None if dp is None else _f32(dev, dp))
        ds, allow = R.rms_res_bwd(o64, r64, dout=d, dpool=dp, doutb=db)
        hold_f32(f"rms dh ({name})", _np(dh), ds, allow)
        if a_bf16:
            assert torch.equal(da, dh.bfloat16()), name
            hold_bf16(f"rms da ({name})", _np(da), ds, allow)
        else:
            assert torch.equal(da, dh), name
