"""Every kernel that inlines csrc/ppo_common.hpp's row_loss / kl_row / stats_block, at every template
instance that differs in code, against the fp64 row reference of tests/ppo_loss_reference.py on its branch
table: the +-20 clamp of the log-ratio, the clip bounds, torch.minimum's tie, the +-20 clamp of the logits
inside the entropy, illegal actions, the smooth-L1 switch (tests/test_ppo_loss_host.py proves the reference
and audits the table on the CPU).

Where the heads are a plain GEMM on a bf16 input the logits are fed EXACTLY: one-hot head weights
(wa[k][k] = 1, wv[4] = 1), zero biases and x[r][0..4] = the table's z (all bf16-representable), so the
kernel's z is the table's bit for bit -- asserted first, on `masked`.  The trajectory columns are longer
than the minibatch and idx walks them backwards with a stride, so a kernel that reads column[r] for
column[idx[r]] fails.  Columns 5.. of x and of the weights carry random values on disjoint columns (x on the
even ones, weights on the odd ones): the logits stay exact, dx = dz W and dW = dz^T x are not trivial.

Tolerances (ppo_loss_reference.UNITS x DEVICE_FACTOR, in units of 2^-23 of each quantity's scale) are
measured on the CPU by the fp32 emulation, not tuned against kernel output; sums add the classical
(m - 1) 2^-24 sum |term| of an fp32 summation in any order."""

import numpy as np
import pytest
import torch

import ppo_loss_reference as R

pytestmark = pytest.mark.gpu

BETA, CRITIC, CLIP = 0.05, 0.7, 0.2
F = R.DEVICE_FACTOR
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    return torch.device("cuda:0")


class Table:
    """The branch table on the device as trajectory columns (row i of the table at position pos[i] =
    M - 1 - 2 i; decoy rows between), and its fp64 row values at inv_m = 1."""

    def __init__(self, dev):
        tab = R.branch_table()
        self.tab, self.n = tab, len(tab["act"])
        n = self.n
        self.M = 2 * n + 3
        self.pos = (self.M - 1 - 2 * np.arange(n)).astype(np.int64)
        act = np.zeros(self.M, np.uint8)
        legal = np.full(self.M, 15, np.uint8)
        logp = np.zeros((self.M, 4), np.float32)
        adv = np.full(self.M, 7.0, np.float32)
        ret = np.full(self.M, -7.0, np.float32)
        act[self.pos], legal[self.pos], logp[self.pos] = tab["act"], tab["legal"], tab["old_logp"]
        adv[self.pos], ret[self.pos] = tab["adv"], tab["ret"]
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        self.cols = {"action": up(act), "legal": up(legal), "logp": up(logp), "adv": up(adv), "ret": up(ret)}
        self.t = R.table_terms(tab, BETA, CRITIC, 1.0)
        self.sc = R.loss_scales(self.t, tab["adv"], BETA, CRITIC, 1.0)
        self.dev = dev

    def batch(self, sel, rows=None):
        from g2048 import _lib as L
        idx = torch.from_numpy(self.pos[sel]).to(self.dev)
        c = self.cols
        b = L.make_ppo_batch(idx, c["action"], c["legal"], c["logp"], c["adv"], c["ret"], rows=rows)
        b.keepalive = (idx, rows)   # the struct holds raw device pointers: the tensors must outlive it
        return b, idx

    def features(self, sel, h, dtype=torch.bfloat16, seed=0):
        """x [m, h]: columns 0..4 = z of the selected rows, even columns >= 6 random bf16 values, the rest 0."""
        g = np.random.default_rng(seed)
        x = np.zeros((len(sel), h), np.float64)
        x[:, :5] = self.tab["z"][sel]
        ev = np.arange(6, h, 2)
        x[:, ev] = R.bf16_round(g.normal(size=(len(sel), len(ev))).astype(np.float32))
        return torch.from_numpy(x).to(self.dev).to(dtype), x

    def heads(self, h, seed=1):
        """One-hot heads on columns 0..4, random fp32 weights on the odd columns >= 5 (where x is 0)."""
        g = np.random.default_rng(seed)
        w = np.zeros((5, h), np.float32)
        w[np.arange(5), np.arange(5)] = 1.0
        od = np.arange(5, h, 2)
        w[:, od] = g.normal(size=(5, len(od))).astype(np.float32)
        to = lambda a: torch.from_numpy(a).to(self.dev)  # noqa: E731
        z = lambda k: torch.zeros(k, device=self.dev)  # noqa: E731
        return to(w[:4].copy()), z(4), to(w[4:5].copy()), z(1), w.astype(np.float64)

    # ---- reference values of a minibatch `sel` (valid rows only) at inv_m ---------------------------
    def ref(self, sel, inv_m):
        t, sc = self.t, self.sc
        out = {k: t[k][sel] for k in ("ppo", "ent", "vl", "masked")}
        out["dz"] = t["dz"][sel] * inv_m
        tol = np.empty((len(sel), 5))
        tol[:, :4] = (F * R.UNITS["dz"] * R.U23 * inv_m * sc["dz"][sel])[:, None]
        tol[:, 4] = F * R.UNITS["dv"] * R.U23 * inv_m * sc["dv"][sel]
        out["tol_dz"] = tol
        for q in ("ppo", "ent", "vl"):
            out["tol_" + q] = F * R.UNITS[q] * R.U23 * sc[q][sel]
        return out


@pytest.fixture(scope="module")
def table(dev):
    return Table(dev)


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_masked(masked, ref_masked):
    """Bitwise the table's logits on legal entries, -inf elsewhere (fp32 holds the bf16 table values exactly)."""
    got = masked.detach().cpu().numpy()
    want = ref_masked.astype(np.float32)
    assert want.astype(np.float64).tobytes() == ref_masked.tobytes()
    assert got.tobytes() == want.tobytes(), np.nonzero((got != want).any(1))[0][:8]


def _check_rows(name, got, want, tol, tags=None):
    """Every entry of got finite and within tol of want (a NaN the kernel left or computed is outside)."""
    assert np.isfinite(got).all(), (name, np.argwhere(~np.isfinite(got))[:8])
    assert np.isfinite(want).all() and np.isfinite(tol).all(), name
    err = np.abs(got - want)
    bad = np.nonzero(np.atleast_2d((~(err <= tol)).T).any(0))[0]
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{name}: worst error / tolerance {worst:.3f}")
    assert bad.size == 0, (name, bad[:8], [tags[i] for i in bad[:4]] if tags is not None else None,
                           got[bad[:4]], want[bad[:4]])


def _check_sums(name, got, r, m):
    """sums[3] of a minibatch against the fp64 sums: the per-row budgets plus (m - 1) 2^-24 sum |term|."""
    for j, q in enumerate(("ppo", "ent", "vl")):
        want = float(r[q].sum())
        tol = float(r["tol_" + q].sum()) + (m - 1) * U24 * float(np.abs(r[q]).sum())
        print(f"{name} sums[{q}]: got {got[j]:.9g} want {want:.9g} tol {tol:.3g}")
        assert np.isfinite(got[j]) and abs(got[j] - want) <= tol, (name, q, got[j], want, tol)


# h -> the head_loss_kernel<J, KS, MULTI> instance g2048_ppo_head_loss dispatches ((h + 31) / 32 k-steps of
# 32 columns in registers up to h = 256: the staged, single-pass form; wider: 256-column chunks, J per lane)
HEAD_LOSS_INSTANCES = [(20, "J1_KS1_staged", False), (64, "J1_KS2_staged", True), (96, "J1_KS3_staged", False),
                       (128, "J1_KS4_staged", True), (160, "J1_KS5_staged", False), (192, "J1_KS6_staged", True),
                       (196, "J1_KS7_staged", False), (256, "J1_KS8_staged", True), (260, "J2_KS8_multi", False),
                       (516, "J3_KS8_multi", True), (1024, "J4_KS8_multi", False), (300, "J2_KS8_multi", True)]


def _head_loss(L, x, heads, batch, m, h, decouple, want_dx, dev):
    wa, ba, wv, bv = heads
    out = {"masked": torch.full((m, 4), float("nan"), device=dev), "dz": torch.full((m, 8), float("nan"), device=dev),
           "dx": torch.full((m, h), float("nan"), device=dev) if want_dx else None,
           "dwa": torch.empty(4, h, device=dev), "dba": torch.empty(4, device=dev),
           "dwv": torch.empty(1, h, device=dev), "dbv": torch.empty(1, device=dev), "sums": torch.empty(3, device=dev)}
    part = torch.empty(L.ppo_head_partials(m, h), device=dev)
    L.ppo_head_loss(x, wa, ba, wv, bv, batch, torch.tensor(BETA, device=dev), CRITIC, CLIP, decouple, out["masked"],
                    out["dx"], part, out["dwa"], out["dba"], out["dwv"], out["dbv"], out["sums"], dz=out["dz"])
    return out


@pytest.mark.parametrize("h,instance,decouple", HEAD_LOSS_INSTANCES)
def test_head_loss_whole_table(dev, table, h, instance, decouple):
    """g2048_ppo_head_loss, the dx and the dz-only form, on the whole table as one padded minibatch (the last
    9 rows are padding): masked bitwise, per-row dz, zero dz on the padding, sums, dx and the four head
    gradients against fp64 products of the reference dz."""
    from g2048 import _lib as L
    n = table.n
    pad = 9
    sel = np.concatenate([np.arange(n), np.arange(pad)])   # the padding repeats real rows: they must not count
    m = n + pad
    rows = torch.tensor([n], dtype=torch.int64, device=dev)
    batch, _ = table.batch(sel, rows)
    x, x64 = table.features(sel, h, seed=h)
    *heads, w64 = table.heads(h, seed=h + 1)
    r = table.ref(np.arange(n), 1.0 / n)
    a = _head_loss(L, x, heads, batch, m, h, decouple, True, dev)
    b = _head_loss(L, x, heads, batch, m, h, decouple, False, dev)
    torch.cuda.synchronize()
    for k in ("dz", "dwa", "dba", "dwv", "dbv", "sums"):
        assert torch.equal(a[k], b[k]), k
    _check_masked(a["masked"][:n], r["masked"])
    dz = _np(a["dz"])
    assert not dz[n:].any() and not dz[:, 5:].any()
    tags = table.tab["tags"]
    _check_rows("dz", dz[:n, :5], r["dz"], r["tol_dz"], tags)
    one = table.t["legal"].sum(1) == 1
    assert not dz[:n][one, :4].any()   # one legal action: exactly zero (see the host test)
    _check_sums("table", _np(a["sums"]), r, n)
    # dx = dz[:, :4] wa + dz[:, 4] wv (no value term when the critic is decoupled): the kernel forms it in
    # fp32 from its own fp32 dz, 5 products
    wd = w64.copy()
    if decouple:
        wd[4] = 0.0
    dx_ref = r["dz"] @ wd
    tol_dx = r["tol_dz"] @ np.abs(wd) + 6 * U24 * (np.abs(r["dz"]) @ np.abs(wd))
    dx = _np(a["dx"])
    assert not dx[n:].any()
    _check_rows("dx", dx[:n], dx_ref, tol_dx, tags)
    if decouple:
        assert not dx[:, 4].any()
    # dW = dz^T x, db = column sums of dz: fp32 accumulation over the rows in the kernel's order
    xv = x64[:n]
    dw_ref = r["dz"].T @ xv
    tol_dw = r["tol_dz"].T @ np.abs(xv) + (n + 8) * U24 * (np.abs(r["dz"]).T @ np.abs(xv))
    got_dw = np.concatenate([_np(a["dwa"]), _np(a["dwv"])])
    _check_rows("dW", got_dw, dw_ref, tol_dw)
    db_ref = r["dz"].sum(0)
    tol_db = r["tol_dz"].sum(0) + (n + 8) * U24 * np.abs(r["dz"]).sum(0)
    _check_rows("db", np.concatenate([_np(a["dba"]), _np(a["dbv"])]), db_ref, tol_db)


@pytest.mark.parametrize("h,instance", [(20, "J1_KS1_staged"), (260, "J2_KS8_multi")])
def test_head_loss_each_row_alone(dev, table, h, instance):
    """Each table row as a minibatch of m = 1 (inv_m = 1): sums are that row's ppo, ent and vl, each held to
    the reference at the per-row budget, and dz again with no other row beside it."""
    from g2048 import _lib as L
    n = table.n
    sel = np.arange(n)
    _, idx = table.batch(sel)
    x, _ = table.features(sel, h, seed=3)
    wa, ba, wv, bv, _ = table.heads(h, seed=4)
    c = table.cols
    masked, dz, sums = (torch.full((n, k), float("nan"), device=dev) for k in (4, 8, 3))
    part = torch.empty(L.ppo_head_partials(1, h), device=dev)
    dwa, dba, dwv, dbv = (torch.empty(s, device=dev) for s in ((4, h), 4, (1, h), 1))
    beta = torch.tensor(BETA, device=dev)
    for i in range(n):
        batch = L.make_ppo_batch(idx[i:i + 1], c["action"], c["legal"], c["logp"], c["adv"], c["ret"])
        L.ppo_head_loss(x[i:i + 1], wa, ba, wv, bv, batch, beta, CRITIC, CLIP, False, masked[i:i + 1], None, part,
                        dwa, dba, dwv, dbv, sums[i], dz=dz[i:i + 1])
    torch.cuda.synchronize()
    r = table.ref(sel, 1.0)
    _check_masked(masked, r["masked"])
    got = _np(sums)
    tags = table.tab["tags"]
    for j, q in enumerate(("ppo", "ent", "vl")):
        _check_rows(q, got[:, j], r[q], r["tol_" + q], tags)
    _check_rows("dz", _np(dz)[:, :5], r["dz"], r["tol_dz"], tags)


# ------------------------------------------------------------------------------------------ GameURM ----
def _urm_loss(L, pooled, heads, batch, m, h, dev, sync):
    wa, ba, wv, bv = heads
    out = {"dz": torch.full((m, 8), float("nan"), device=dev), "masked": torch.full((m, 4), float("nan"), device=dev),
           "sums": torch.empty(3, device=dev), "loss": torch.empty(1, device=dev)}
    part = torch.empty(L.urm_head_loss_partials(m, h), device=dev)
    L.urm_head_loss(pooled, wa, ba, wv, bv, batch, torch.tensor(BETA, device=dev), CRITIC, CLIP, out["dz"],
                    out["masked"], part, sync, out["sums"], out["loss"])
    return out


def _check_urm_loss(name, out, r, m):
    got = _np(out["sums"])
    _check_sums(name, got, r, m)
    inv_m = 1.0 / m
    want = -inv_m * float((r["ppo"] - CRITIC * r["vl"] + BETA * r["ent"]).sum())
    tol = sum(w * (float(r["tol_" + q].sum()) + (m + 3) * U24 * float(np.abs(r[q]).sum()))
              for q, w in (("ppo", 1.0), ("vl", CRITIC), ("ent", BETA))) * inv_m
    loss = float(out["loss"][0])
    print(f"{name} loss: got {loss:.9g} want {want:.9g} tol {tol:.3g}")
    assert np.isfinite(loss) and abs(loss - want) <= tol


@pytest.mark.parametrize("h", [32, 64])
@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16], ids=["pooled_fp32", "pooled_bf16"])
def test_urm_head_loss_whole_table(dev, table, h, pdt):
    """urm_head_loss_kernel<32> and <64>, pooled fp32 and bf16, on the whole table: masked bitwise, per-row
    dz, sums and loss[0]; then urm_head_loss_bwd_kernel<h>: dpooled = bf16(sum_k bf16(go dz_k) bf16(W_k)) in
    fp64 at those rounding points from the kernel's own dz (one bf16 step allowed), the head gradients dy^T
    bf16(pooled) and the column sums of dy, and accumulate = 1 onto a non-zero buffer = buffer + the
    accumulate = 0 result, bitwise."""
    from g2048 import _lib as L
    n = table.n
    sel = np.arange(n)
    batch, _ = table.batch(sel)
    pooled, x64 = table.features(sel, h, dtype=pdt, seed=h)
    wa, ba, wv, bv, _ = table.heads(h, seed=h + 1)
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _urm_loss(L, pooled, (wa, ba, wv, bv), batch, n, h, dev, sync)
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    r = table.ref(sel, 1.0 / n)
    _check_masked(out["masked"], r["masked"])
    dz = _np(out["dz"])
    assert not dz[:, 5:].any()
    _check_rows("dz", dz[:, :5], r["dz"], r["tol_dz"], table.tab["tags"])
    assert not dz[table.t["legal"].sum(1) == 1, :4].any()
    _check_urm_loss("urm table", out, r, n)
    # ---- backward ----
    go = torch.tensor(0.75, device=dev)
    res = []
    base = [torch.full(s, 0.375, device=dev) for s in ((4, h), (4,), (1, h), (1,))]
    for acc in (False, True):
        dp = torch.full((n, h), float("nan"), device=dev).to(pdt)
        grads = [b.clone() if acc else torch.full_like(b, float("nan")) for b in base]
        part = torch.empty(L.urm_head_loss_partials(n, h), device=dev)
        L.urm_head_loss_bwd(pooled, wa, wv, out["dz"], go, dp, part, sync, grads[0], grads[1], grads[2], grads[3],
                            accumulate=acc)
        res.append((dp, grads))
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    assert torch.equal(res[0][0], res[1][0])
    for g0, g1, b in zip(res[0][1], res[1][1], base):
        assert torch.equal(g1, b + g0)
    dz32 = out["dz"].detach().cpu().numpy()[:, :5]
    dy = R.bf16_round(np.float32(0.75) * dz32)                     # bf16(go dz), go dz formed in fp32
    wb = R.bf16_round(np.concatenate([wa.cpu().numpy(), wv.cpu().numpy()]))
    want_dp = R.bf16_round((dy @ wb).astype(np.float32))
    got_dp = _np(res[0][0])
    # one bf16 step is <= 2^-7 of the value; where the five products cancel, the kernel's fp32 sum of them
    # differs from the fp64 one by up to 5 x 2^-24 of their magnitudes before that rounding
    step = 2.0 ** -7 * np.abs(want_dp) + 5 * U24 * (np.abs(dy) @ np.abs(wb)) + 1e-37
    assert np.isfinite(dz32).all() and np.isfinite(got_dp).all() and np.isfinite(want_dp).all()
    bad = ~(np.abs(got_dp - want_dp) <= step)
    assert not bad.any(), (np.argwhere(bad)[:4], got_dp[bad][:4], want_dp[bad][:4])
    assert float(np.abs(want_dp).max()) > 0
    xb = x64                                                        # bf16-representable already
    dw_ref, db_ref = dy.T @ xb, dy.sum(0)
    tol_dw = (n + 8) * U24 * (np.abs(dy).T @ np.abs(xb))
    g0 = res[0][1]
    _check_rows("dW", np.concatenate([_np(g0[0]), _np(g0[2])]), dw_ref, tol_dw)
    _check_rows("db", np.concatenate([_np(g0[1]), _np(g0[3])]), db_ref, (n + 8) * U24 * np.abs(dy).sum(0))


@pytest.mark.parametrize("h", [32, 64])
def test_urm_head_loss_each_row_alone(dev, table, h):
    """Each table row alone (m = 1): sums = the row's ppo, ent, vl; loss[0] = -(ppo - critic vl + beta ent)."""
    from g2048 import _lib as L
    n = table.n
    sel = np.arange(n)
    _, idx = table.batch(sel)
    pooled, _ = table.features(sel, h, dtype=torch.float32, seed=5)
    wa, ba, wv, bv, _ = table.heads(h, seed=6)
    c = table.cols
    masked, dz, sums, loss = (torch.full((n, k), float("nan"), device=dev) for k in (4, 8, 4, 4))
    part = torch.empty(L.urm_head_loss_partials(1, h), device=dev)
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    beta = torch.tensor(BETA, device=dev)
    for i in range(n):
        batch = L.make_ppo_batch(idx[i:i + 1], c["action"], c["legal"], c["logp"], c["adv"], c["ret"])
        L.urm_head_loss(pooled[i:i + 1], wa, ba, wv, bv, batch, beta, CRITIC, CLIP, dz[i:i + 1], masked[i:i + 1], part,
                        sync, sums[i], loss[i])
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    r = table.ref(sel, 1.0)
    _check_masked(masked, r["masked"])
    got = _np(sums)
    tags = table.tab["tags"]
    for j, q in enumerate(("ppo", "ent", "vl")):
        _check_rows(q, got[:, j], r[q], r["tol_" + q], tags)
    _check_rows("dz", _np(dz)[:, :5], r["dz"], r["tol_dz"], tags)
    want = -(r["ppo"] - CRITIC * r["vl"] + BETA * r["ent"])
    tol = r["tol_ppo"] + CRITIC * r["tol_vl"] + BETA * r["tol_ent"] + 4 * U24 * (
        np.abs(r["ppo"]) + CRITIC * np.abs(r["vl"]) + BETA * np.abs(r["ent"]))
    _check_rows("loss", _np(loss)[:, 0], want, tol, tags)


@pytest.mark.parametrize("h,pdt", [(32, torch.bfloat16), (64, torch.float32)])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 65537])
def test_urm_head_loss_block_counts(dev, table, m, h, pdt):
    """Table rows tiled to m rows: one block (m < 256), exactly one, two, and 257 blocks (m = 65 537: the
    last block's strided pass over the partials takes a second trip).  Per-row dz, sums and loss against the
    reference; two consecutive launches of the loss and of its backward bitwise equal; the ticket word back
    at 0 after each."""
    from g2048 import _lib as L
    sel = (np.arange(m) * 7 + 3) % table.n
    batch, _ = table.batch(sel)
    pooled, _ = table.features(sel, h, dtype=pdt, seed=m)
    wa, ba, wv, bv, _ = table.heads(h, seed=m + 1)
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        o = _urm_loss(L, pooled, (wa, ba, wv, bv), batch, m, h, dev, sync)
        torch.cuda.synchronize()
        assert int(sync.item()) == 0
        outs.append(o)
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k
    r = table.ref(sel, 1.0 / m)
    _check_masked(outs[0]["masked"], r["masked"])
    _check_rows("dz", _np(outs[0]["dz"])[:, :5], r["dz"], r["tol_dz"])
    _check_urm_loss(f"urm m={m}", outs[0], r, m)
    go = torch.tensor(1.0, device=dev)
    bw = []
    for _ in range(2):
        dp = torch.full((m, h), float("nan"), device=dev).to(pdt)
        grads = [torch.full(s, float("nan"), device=dev) for s in ((4, h), (4,), (1, h), (1,))]
        part = torch.empty(L.urm_head_loss_partials(m, h), device=dev)
        L.urm_head_loss_bwd(pooled, wa, wv, outs[0]["dz"], go, dp, part, sync, *grads)
        torch.cuda.synchronize()
        assert int(sync.item()) == 0
        bw.append([dp] + grads)
    for a, b in zip(*bw):
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), b.view(bits))
    dz32 = outs[0]["dz"].detach().cpu().numpy()[:, :5]
    dy = R.bf16_round(dz32)
    db_ref = dy.sum(0)
    _check_rows("db", np.concatenate([_np(bw[0][2]), _np(bw[0][4])]), db_ref, (m + 8) * U24 * np.abs(dy).sum(0))


# ----------------------------------------------------------------------------------------------- KL ----
def _kl_case(reps):
    k = R.kl_table()
    old = np.tile(k["old"], (reps, 1))
    new = np.tile(k["new"], (reps, 1))
    # the repeats differ: a bf16-exact shift of all new logits of a row leaves its KL unchanged in exact
    # arithmetic and moves the fp32 rounding
    shift = (np.arange(len(old)) // len(k["old"]) % 4).astype(np.float64)
    new = new + np.where(np.isfinite(old), 4.0 * shift[:, None], 0.0)   # (legal slots: the others do not count)
    assert R.is_bf16(new)
    kl = R.kl_row_ref(old, new)
    tol = F * R.UNITS["kl"] * R.U23 * R.kl_scale(old, new)
    return old, new, kl, tol


def _kl_bounds(kl, tol, m):
    return float(kl.sum()), float(tol.sum()) + (m - 1) * U24 * float(np.abs(kl).sum()), float(kl.max()), float(tol.max())


def _check_stats(stats, sums, kl_sum, kl_max, tol_sum, tol_max, gn, m, calls=2):
    """The nine statistics after `calls` accumulating calls against stats_ref: each entry within 4 x 2^-23
    relative (the few fp32 operations of stats_block) plus the KL budget where KL enters."""
    one = R.stats_ref(sums, kl_sum, kl_max, gn, BETA, CRITIC, m)
    want = calls * one
    want[8] = kl_max
    tol = 4 * R.U23 * calls * np.abs(one) + 1e-30
    tol[0] = 4 * R.U23 * calls * (abs(one[1]) + abs(one[2]) + abs(one[3]))   # a sum of three terms that cancel
    tol[6] += calls * tol_sum
    tol[7] += calls * tol_sum / m
    tol[8] = tol_max + 4 * R.U23 * abs(kl_max)
    got = _np(stats)
    print("stats got", got, "want", want)
    assert np.isfinite(got).all() and (np.abs(got - want) <= tol).all(), (got, want, tol)


@pytest.mark.parametrize("h,instance", [(64, "KS2_single"), (196, "KS7_single"), (300, "KS8_multi")])
def test_head_kl_and_stats(dev, h, instance):
    """g2048_ppo_head_kl (head_kl_kernel<KS, MULTI>, one-hot action head so the new logits are the KL table's
    bit for bit) sum and max against kl_row_ref, with 5 padding rows; then g2048_ppo_stats fed by it, twice."""
    from g2048 import _lib as L
    old, new, kl, tol = _kl_case(20)
    m, pad = len(old), 5
    x = np.zeros((m + pad, h))
    x[:m, :4] = new
    x[m:, :4] = [3.0, -2.0, 1.0, 0.5]
    x[:, 6::2] = R.bf16_round(np.random.default_rng(h).normal(size=x[:, 6::2].shape).astype(np.float32))
    wa = np.zeros((4, h), np.float32)
    wa[np.arange(4), np.arange(4)] = 1.0
    wa[:, 5::2] = np.random.default_rng(h + 1).normal(size=wa[:, 5::2].shape)
    oldp = np.concatenate([old, np.zeros((pad, 4), np.float32)])
    up = lambda a, dt: torch.from_numpy(a).to(dev).to(dt)  # noqa: E731
    rows = torch.tensor([m], dtype=torch.int64, device=dev)
    out = torch.empty(2, device=dev)
    L.ppo_head_kl(up(x, torch.bfloat16), up(wa, torch.float32), torch.zeros(4, device=dev), up(oldp, torch.float32),
                  torch.empty(L.ppo_head_partials(m + pad, h), device=dev), out, rows=rows)
    ks, ts, km, tm = _kl_bounds(kl, tol, m)
    got = _np(out)
    print(f"head_kl h={h}: sum {got[0]:.9g} want {ks:.9g} tol {ts:.3g}; max {got[1]:.9g} want {km:.9g} tol {tm:.3g}")
    assert abs(got[0] - ks) <= ts and abs(got[1] - km) <= tm
    sums = torch.tensor([12.5, 300.0, 80.0], device=dev)
    gn = torch.tensor(0.75, device=dev)
    stats = torch.zeros(9, device=dev)
    stats[8] = -float("inf")
    for _ in range(2):
        L.ppo_stats(sums, out, gn, torch.tensor(BETA, device=dev), CRITIC, m + pad, stats, rows=rows)
    _check_stats(stats, (12.5, 300.0, 80.0), ks, km, ts, tm, 0.75, m)


@pytest.mark.parametrize("reps", [1, 20, 40])
def test_urm_kl_stats(dev, reps):
    """g2048_urm_kl_stats (kl_row + stats_block) on the KL rows, one, two and three blocks: all nine
    statistics after two accumulating calls; the ticket word back at 0."""
    from g2048 import _lib as L
    old, new, kl, tol = _kl_case(reps)
    m = len(old)
    sums = torch.tensor([-3.5, 210.0, 55.0], device=dev)
    gn = torch.tensor(1.25, device=dev)
    stats = torch.zeros(9, device=dev)
    stats[8] = -float("inf")
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    part = torch.empty(L.urm_head_loss_partials(m, 64), device=dev)
    o, z = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev).float()
    for _ in range(2):
        L.urm_kl_stats(o, z, sums, gn, torch.tensor(BETA, device=dev), CRITIC, stats, part, sync)
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    ks, ts, km, tm = _kl_bounds(kl, tol, m)
    _check_stats(stats, (-3.5, 210.0, 55.0), ks, km, ts, tm, 1.25, m)


@pytest.mark.parametrize("h,instance", [(64, "KS2_single"), (300, "KS8_multi")])
def test_head_kl_each_row_alone(dev, h, instance):
    """Each KL row alone (m = 1): the sum and the max g2048_ppo_head_kl returns are then that row's KL, held
    to kl_row_ref at the per-row budget -- a minibatch shows only a sum and a maximum, whose fp32 summation
    bound hides one row's error."""
    from g2048 import _lib as L
    old, new, kl, tol = _kl_case(4)
    n = len(old)
    x = np.zeros((n, h))
    x[:, :4] = new
    wa = np.zeros((4, h), np.float32)
    wa[np.arange(4), np.arange(4)] = 1.0
    xt = torch.from_numpy(x).to(dev).to(torch.bfloat16)
    wat, ba, old_t = torch.from_numpy(wa).to(dev), torch.zeros(4, device=dev), torch.from_numpy(old).to(dev)
    out = torch.full((n, 2), float("nan"), device=dev)
    part = torch.empty(L.ppo_head_partials(1, h), device=dev)
    for i in range(n):
        L.ppo_head_kl(xt[i:i + 1], wat, ba, old_t[i:i + 1], part, out[i])
    got = _np(out)
    _check_rows("kl sum", got[:, 0], kl, tol)
    _check_rows("kl max", got[:, 1], kl, tol)


def test_urm_kl_each_row_alone(dev):
    """Each KL row alone through g2048_urm_kl_stats: kl_total, kl_average and kl_max of a fresh statistics
    vector are then that row's KL."""
    from g2048 import _lib as L
    old, new, kl, tol = _kl_case(4)
    n = len(old)
    old_t, new_t = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev).float()
    stats = torch.zeros(n, 12, device=dev)
    stats[:, 8] = -float("inf")
    sums, gn, beta = torch.zeros(3, device=dev), torch.tensor(0.5, device=dev), torch.tensor(BETA, device=dev)
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    part = torch.empty(L.urm_head_loss_partials(1, 64), device=dev)
    for i in range(n):
        L.urm_kl_stats(old_t[i:i + 1], new_t[i:i + 1], sums, gn, beta, CRITIC, stats[i], part, sync)
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    got = _np(stats)
    for col in (6, 7, 8):
        _check_rows(R.STAT_KEYS[col], got[:, col], kl, tol)
    assert (got[:, 4] == 0.5).all() and not got[:, 9:].any()


def _block_kl_case(dev, new, pad=0):
    """Inputs of g2048_mlp_fwd_kl (h = 196) whose logits are `new` bit for bit: a zero block weight and a zero
    LayerNorm bias make the block's branch ReLU(LN(0)) = 0, so its bf16 output is x itself; x carries the new
    logits in columns 0..3 under a one-hot action head (random x on the even columns >= 6, random head
    weights on the odd ones, zero biases)."""
    h, m = 196, len(new) + pad
    x = np.zeros((m, h))
    x[:len(new), :4] = new
    x[len(new):, :4] = [3.0, -2.0, 1.0, 0.5]
    x[:, 6::2] = R.bf16_round(np.random.default_rng(7).normal(size=x[:, 6::2].shape).astype(np.float32))
    wa = np.zeros((4, h), np.float32)
    wa[np.arange(4), np.arange(4)] = 1.0
    wa[:, 5::2] = np.random.default_rng(8).normal(size=wa[:, 5::2].shape)
    return (torch.from_numpy(x).to(dev).to(torch.bfloat16), torch.zeros(h, h, dtype=torch.bfloat16, device=dev),
            torch.ones(h, device=dev), torch.zeros(h, device=dev), torch.from_numpy(wa).to(dev),
            torch.zeros(4, device=dev))


def test_block_kl_rows(dev):
    """g2048_mlp_fwd_kl (mlp_fwd_wide_kernel<196, residual, no dropout, KL>: the last block, the action head and
    kl_row in one launch) on the KL rows: as one minibatch with 5 padding rows (sum and max), and each row
    alone (m = 1), where the sum and the max are that row's KL, at the per-row budget."""
    from g2048 import _lib as L
    old, new, kl, tol = _kl_case(20)
    m, pad = len(old), 5
    x, w, gamma, beta, wa, ba = _block_kl_case(dev, new, pad)
    old_t = torch.from_numpy(np.concatenate([old, np.zeros((pad, 4), np.float32)])).to(dev)
    rows = torch.tensor([m], dtype=torch.int64, device=dev)
    out = torch.full((2,), float("nan"), device=dev)
    L.mlp_fwd_kl(x, w, gamma, beta, None, wa, ba, old_t, torch.empty(L.ppo_head_partials(m + pad, 196), device=dev),
                 out, rows=rows)
    ks, ts, km, tm = _kl_bounds(kl, tol, m)
    got = _np(out)
    print(f"block kl: sum {got[0]:.9g} want {ks:.9g} tol {ts:.3g}; max {got[1]:.9g} want {km:.9g} tol {tm:.3g}")
    assert abs(got[0] - ks) <= ts and abs(got[1] - km) <= tm
    old, new, kl, tol = _kl_case(4)
    n = len(old)
    x, w, gamma, beta, wa, ba = _block_kl_case(dev, new)
    old_t = torch.from_numpy(old).to(dev)
    outs = torch.full((n, 2), float("nan"), device=dev)
    part = torch.empty(L.ppo_head_partials(1, 196), device=dev)
    for i in range(n):
        L.mlp_fwd_kl(x[i:i + 1], w, gamma, beta, None, wa, ba, old_t[i:i + 1], part, outs[i])
    got = _np(outs)
    _check_rows("kl sum", got[:, 0], kl, tol)
    _check_rows("kl max", got[:, 1], kl, tol)


# ---------------------------------------------------------------------------------- the fused passes ----
def _ref_from_terms(t, adv, inv_m):
    sc = R.loss_scales(t, adv, BETA, CRITIC, 1.0)
    out = {k: t[k] for k in ("ppo", "ent", "vl", "masked")}
    out["dz"] = t["dz"]
    tol = np.empty((len(adv), 5))
    tol[:, :4] = (F * R.UNITS["dz"] * R.U23 * inv_m * sc["dz"])[:, None]
    tol[:, 4] = F * R.UNITS["dv"] * R.U23 * inv_m * sc["dv"]
    out["tol_dz"] = tol
    for q in ("ppo", "ent", "vl"):
        out["tol_" + q] = F * R.UNITS[q] * R.U23 * sc[q]
    return out


@pytest.mark.parametrize("h", [64, 196])
def test_fused_passes_on_steered_columns(dev, h):
    """g2048_ppo_forward_loss, g2048_ppo_forward_kl and g2048_ppo_forward_kl_stats at m = 257 with rows = 250.
    The logits cannot be set here, so the columns are built around them: ba = [23, -23, 0.3, -0.2] with a small
    wa puts logit 0 above +20 and logit 1 below -20 wherever the legal mask admits them; the pass runs once,
    logits and value are recomputed in fp64 from its h[2] output (pinned bitwise to the layer chain by
    test_fused_train_pass_matches_layer_kernels) and old_logp / adv / ret are then set per row so that the rows
    fall into every log-ratio regime, advantage sign and value gap at the table's margins; the pass runs again.

    masked against the fp64 GEMM at rtol = atol = 1e-5 as in test_ppo_head_loss_matches_autograd: the kernel
    sums h products in fp32 in its own order.  The row reference is then evaluated at the kernel's OWN masked
    logits (so the loss math is held to the table's budget, not to 1e-5) and the fp64 value; the value the
    kernel used is not an output, so the terms that depend on it allow dv = 1e-5 (1 + |v|) of it on top."""
    from g2048 import _lib as L
    from test_gpu_ppo_fused import _pass_case
    M, m, nv = 700, 257, 250
    w, gam, bet, (wa, ba, wv, bv), data, idx, ctr = _pass_case(dev, h, M, m, 0.0, 31 * h)
    wa = (wa * 0.1).contiguous()
    ba = torch.tensor([23.0, -23.0, 0.3, -0.2], device=dev)
    rng = np.random.default_rng(h)
    pos = idx.cpu().numpy()
    assert not np.array_equal(pos, np.arange(m))
    legal_m = rng.integers(1, 16, size=m).astype(np.uint8)
    act_m = np.array([[a for a in range(4) if lm >> a & 1][rng.integers(0, bin(lm).count("1"))] for lm in legal_m],
                     np.uint8)
    legal, act = data["legal"].cpu().numpy().copy(), data["actions"].cpu().numpy().copy()
    legal[pos], act[pos] = legal_m, act_m
    data["legal"], data["actions"] = torch.from_numpy(legal).to(dev), torch.from_numpy(act).to(dev)
    rows = torch.tensor([nv], dtype=torch.int64, device=dev)
    beta = torch.tensor(BETA, device=dev)
    frag = torch.empty(L.head_split_bytes(h), dtype=torch.uint8, device=dev)
    L.head_split(wa, wv, frag)
    bf = torch.bfloat16

    def train_pass():
        batch = L.make_ppo_batch(idx, data["actions"], data["legal"], data["logp"], data["adv"], data["ret"], rows=rows)
        out = dict(h=[None, None, torch.full((m, h), float("nan"), dtype=bf, device=dev)],
                   masked=torch.full((m, 4), float("nan"), device=dev), dz=torch.full((m, 8), float("nan"), device=dev),
                   dz_bf16=torch.empty(m, 16, dtype=bf, device=dev),
                   partials=torch.empty(L.mlp_pass_partials(m, True), device=dev))
        args = L.make_mlp_pass(data["boards"], batch, m, w[0], w[1:], gam, bet, frag, ba, bv, beta_dev=beta,
                               critic=CRITIC, clip_eps=CLIP, **out)
        red = [torch.empty(k, device=dev) for k in (4, 1, 3)]
        L.ppo_forward_loss(args, *red)
        torch.cuda.synchronize()
        return out, red

    out, _ = train_pass()
    h2 = _np(out["h"][2])
    W = np.concatenate([_np(wa), _np(wv)])
    z64 = h2 @ W.T + np.concatenate([_np(ba), _np(bv)])
    lg = ((legal_m[:, None] >> np.arange(4)) & 1).astype(bool)
    assert (np.abs(np.abs(z64[:, :4][lg]) - 20.0) >= 2 * R.MARGIN_LOGIT).all()
    # ---- steer: old_logp[act] = fp32(logp_ref[act] - target), ret = fp32(v - gap) --------------------
    targets = np.array([t for ts in R.LOG_RATIO_REGIMES.values() for t in ts])
    x = np.where(lg, z64[:, :4], -np.inf)
    lp = (x - x.max(1, keepdims=True)) - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True))
    tgt = targets[rng.integers(0, len(targets), size=m)]
    advs = np.array([a for v in R.ADV_REGIMES.values() for a in v], np.float32)[rng.integers(0, 9, size=m)]
    gap = np.array(R.VALUE_GAPS)[rng.integers(0, len(R.VALUE_GAPS), size=m)]
    old = np.where(lg, lp + 0.125, -np.inf)
    old[np.arange(m), act_m] = lp[np.arange(m), act_m] - tgt
    old = old.astype(np.float32)
    ret_m = (z64[:, 4] - gap).astype(np.float32)
    for key, val in (("logp", old), ("adv", advs), ("ret", ret_m)):
        col = data[key].cpu().numpy().copy()
        col[pos] = val
        data[key] = torch.from_numpy(col).to(dev)
    out, (dba, dbv, sums) = train_pass()
    # ---- masked against the fp64 GEMM --------------------------------------------------------------
    mk = out["masked"][:nv].detach().cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isfinite(mk), lg[:nv])
    np.testing.assert_allclose(mk[lg[:nv]], z64[:nv, :4][lg[:nv]], rtol=1e-5, atol=1e-5)
    # ---- the row reference at the kernel's own logits and the fp64 value ----------------------------
    zk = np.concatenate([np.where(lg[:nv], mk, 0.0), z64[:nv, 4:5]], 1)
    inv_m = 1.0 / nv
    t = R.row_terms(zk, act_m[:nv], legal_m[:nv], old[:nv], advs[:nv], ret_m[:nv], BETA, CRITIC, R.CLIP_LO, R.CLIP_HI,
                    inv_m)
    r = _ref_from_terms(t, advs[:nv], inv_m)
    dv = 1e-5 * (1.0 + np.abs(z64[:nv, 4]))
    r["tol_dz"][:, 4] += inv_m * CRITIC * dv
    r["tol_vl"] = r["tol_vl"] + np.minimum(np.abs(t["dv0"]), 1.0) * dv + dv * dv
    # every regime is met by >= 8 rows, at the table's margins (from the reference alone)
    assert (np.abs(np.abs(t["dlt"]) - 20.0) >= R.MARGIN_LOG_RATIO - 1e-3).all()
    assert (np.abs(t["ratio"] - R.CLIP_LO) >= R.MARGIN_RATIO - 1e-3).all()
    assert (np.abs(t["ratio"] - R.CLIP_HI) >= R.MARGIN_RATIO - 1e-3).all()
    a_ = act_m[:nv]
    ar = np.arange(nv)
    counts = {"lr_below_m20": t["dlt"] < -20, "lr_low": t["in20"] & (t["ratio"] < R.CLIP_LO), "lr_in": t["inr"],
              "lr_high": t["in20"] & t["above"], "lr_above_p20": t["dlt"] > 20, "adv_pos": advs[:nv] > 0,
              "adv_neg": advs[:nv] < 0, "adv_zero": advs[:nv] == 0, "logit_hi_taken": t["hi_logit"][ar, a_],
              "logit_hi_other": t["hi_logit"].any(1) & ~t["hi_logit"][ar, a_], "logit_lo_taken": t["lo_logit"][ar, a_],
              "logit_lo_other": t["lo_logit"].any(1) & ~t["lo_logit"][ar, a_], "value_quadratic": t["quad"],
              "value_linear": ~t["quad"]}
    for g_ in R.VALUE_GAPS:
        counts["gap_%g" % g_] = np.abs(t["dv0"] - g_) < 1e-4
    for k in range(1, 5):
        counts["legal_%d" % k] = t["legal"].sum(1) == k
    short = {k: int(v.sum()) for k, v in counts.items() if v.sum() < 8}
    assert not short, short
    dz = _np(out["dz"])
    assert not dz[nv:].any() and not dz[:, 5:].any()
    _check_rows("dz", dz[:nv, :5], r["dz"], r["tol_dz"])
    _check_sums(f"fused h={h}", _np(sums), r, nv)
    db_ref = r["dz"].sum(0)
    tol_db = r["tol_dz"].sum(0) + (nv + 8) * U24 * np.abs(r["dz"]).sum(0)
    _check_rows("db", np.concatenate([_np(dba), _np(dbv)]), db_ref, tol_db)
    # ---- the KL passes: p = 0 and unchanged weights, so the new logits are the train pass's bit for bit.
    # That is asserted, not assumed: against old = the train pass's own masked logits every row's KL is then
    # (lo - lo) p = 0 exactly, so both the sum and the max come out as 0.0; one logit an ulp off would leave
    # a non-zero term.  The KL rows below can therefore be held to the KL budget alone.
    frag_kl = torch.empty(L.head_split_bytes(h), dtype=torch.uint8, device=dev)
    L.head_split(wa, None, frag_kl)
    batch = L.make_ppo_batch(idx, data["actions"], data["legal"], data["logp"], data["adv"], data["ret"], rows=rows)
    part = torch.empty(L.mlp_pass_partials(m, False), device=dev)
    same = torch.full((2,), float("nan"), device=dev)
    L.ppo_forward_kl(L.make_mlp_pass(data["boards"], batch, m, w[0], w[1:], gam, bet, frag_kl, ba,
                                     masked=out["masked"], partials=part), same)
    assert _np(same).tolist() == [0.0, 0.0], same
    kind = rng.integers(0, 3, size=m)
    oldm = np.where(lg, np.concatenate([mk, np.zeros((m - nv, 4))]), -np.inf)
    oldm = oldm + np.where(kind[:, None] == 1, R.bf16_round(rng.normal(size=(m, 4)).astype(np.float32)) * 0.5, 0.0)
    for j in np.nonzero((kind == 2) & (lg.sum(1) >= 2))[0]:   # one legal action 60 below the old maximum
        ks = np.nonzero(lg[j])[0]
        top = ks[np.argmax(oldm[j, ks])]
        oldm[j, ks[ks != top][0]] = oldm[j, top] - 60.0
    oldm = oldm.astype(np.float32)
    old_t = torch.from_numpy(oldm).to(dev)
    kl = R.kl_row_ref(oldm[:nv], zk[:, :4])
    tol = F * R.UNITS["kl"] * R.U23 * R.kl_scale(oldm[:nv], zk[:, :4])
    ks_, ts, km, tm = _kl_bounds(kl, tol, nv)
    assert (kl[kind[:nv] == 0] <= 1e-12).all() and (kind[:nv] == 0).sum() >= 8
    assert ((kind[:nv] == 2) & (lg[:nv].sum(1) >= 2)).sum() >= 8 and (kl[lg[:nv].sum(1) == 1] == 0).all()
    args = L.make_mlp_pass(data["boards"], batch, m, w[0], w[1:], gam, bet, frag_kl, ba, masked=old_t, partials=part)
    got = torch.empty(2, device=dev)
    L.ppo_forward_kl(args, got)
    g_ = _np(got)
    print(f"fused kl h={h}: sum {g_[0]:.9g} want {ks_:.9g} tol {ts:.3g}; max {g_[1]:.9g} want {km:.9g} tol {tm:.3g}")
    assert abs(g_[0] - ks_) <= ts and abs(g_[1] - km) <= tm
    stats = torch.zeros(9, device=dev)
    stats[8] = -float("inf")
    sync = torch.zeros(1, dtype=torch.int32, device=dev)
    gn = torch.tensor(0.6, device=dev)
    for _ in range(2):
        L.ppo_forward_kl_stats(args, sums, gn, beta, CRITIC, m, stats, sync, rows=rows)
    torch.cuda.synchronize()
    assert int(sync.item()) == 0
    _check_stats(stats, tuple(float(s) for s in sums), ks_, km, ts, tm, float(np.float32(0.6)), nv)
