"""The reproducible forms of the training step's gradient reductions (gsdd_set_deterministic(1): gsdd_wgrad, gsdd_colsum,
gsdd_batch_rowsum, gsdd_ln_bwd, gsdd_d3pm_embed_bwd, gsdd_adaln_bwd) against the same fp64 references and per-element bars as their
fast forms, at the shapes where the reproducible form's own index arithmetic changes: a ragged second 128-row slab and 1025 slabs in one
workgroup (wgrad), every column-group width (colsum), one launch per batch element with its own pointer offsets (batch_rowsum, AdaLN
ln_bwd: up to 656 launches, rows_per_batch not a multiple of 16), one block over 65,544 rows (plain ln_bwd), out-of-range tokens in
the embedding kernel of its own, and repeated timesteps in both instantiations of adaln_bwd.  Every bit-for-bit gradient comparison of
the whole-model tests runs in this form on both sides; a form that is wrong the same way twice passes those, and fails here.

The case bodies, references, bars and guards are those of tests/test_gpu_train_kernels.py and tests/test_gpu_gemm_family.py, called
with form="reproducible": bar gamma(n) sum |terms| + 2 U |prefill| with n the rows summed -- a fully sequential f32 sum, the worst order
any of these forms uses, stays below 0.3 of gamma(n) sum |terms| for random-sign, scaled, cancelling and all-positive terms up to
n = 300,000.  Each case also runs a second time from a fresh copy of the prefill (every output equal in bits) and once in the fast form
(the two differ by no more than the sum of their two bars), and records under its fast-form key + "[reproducible]" whether the fast form
spreads one output address over several workgroups -- only there do equal bits say what the fast form would not.

The unmarked tests at the end check the checks on the CPU: an f32 emulation of each reproducible order meets the bars, and each of eight
wrong-offset / wrong-order faults injected into it misses one."""
import contextlib

import numpy as np
import pytest
import torch

import tests.test_gpu_gemm_family as GF
import tests.test_gpu_train_kernels as TK

gpu = pytest.mark.gpu
D = TK.D
f32 = np.float32


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


@pytest.fixture
def fast_form(G):
    """The one place the process-wide switch is set: on for the test, the previous value back afterwards.  -> a context manager that
    turns it off for the fast-form comparison run inside a case"""
    prev = G.ops.set_deterministic(True)

    @contextlib.contextmanager
    def fast():
        assert G.ops.set_deterministic(False) is True
        try:
            yield
        finally:
            G.ops.set_deterministic(True)
    try:
        yield fast
        assert G.ops.set_deterministic(True) is True, "the switch was off at the end of a reproducible case"
    finally:
        G.ops.set_deterministic(prev)


# ----------------------------------------------------------------------------- GPU: the six entries in their reproducible form
@gpu
@pytest.mark.parametrize("M,N,K,with_db", [(129, 68, 68, True), (200, 12, 200, True), (70001, 200, 12, True), (131149, 68, 68, True),
                                           (40000, 12, 200, False)])
def test_wgrad_reproducible(G, fast_form, M, N, K, with_db):
    """one workgroup per 64 x 64 tile walks ceil(M / 128) slabs: a second slab of one row, 1025 slabs, db untouched without db"""
    GF.wgrad_case(G, f"wgrad[M{M}-N{N}-K{K}]", *GF.wgrad_inputs(M, N, K), with_db, form="reproducible", fast_form=fast_form,
                  slabs=-(-M // 128))


@gpu
def test_wgrad_cancellation_reproducible(G, fast_form):
    GF.wgrad_case(G, "wgrad_cancellation", *GF.wgrad_cancellation_inputs(), True, form="reproducible", fast_form=fast_form)


@gpu
@pytest.mark.parametrize("M,N", [(200, 1), (5000, 68), (262144, 4), (300000, 12), (700, 257)])
def test_colsum_reproducible(G, fast_form, M, N):
    """one block per column group takes all M rows: 1, 128, 4, 16 and 256 columns per block, M not a multiple of the row groups"""
    GF.colsum_case(G, M, N, form="reproducible", fast_form=fast_form)


@gpu
@pytest.mark.parametrize("B,L,C", [(3, 77, 12), (3, 200, 300), (3, 1000, 1), (3, 63, 68), (16, 4096, 64)])
def test_batch_rowsum_reproducible(G, fast_form, B, L, C):
    """B launches of the column-sum kernel, each on its own slice of the (sentinel-prefilled) out after the memset"""
    GF.batch_rowsum_case(G, L, C, B=B, form="reproducible", fast_form=fast_form)


@gpu
@pytest.mark.parametrize("name,M,rpb,by_batch,with_dx_in", TK.LN_BWD_CASES, ids=[c[0] for c in TK.LN_BWD_CASES])
def test_ln_bwd_reproducible(G, fast_form, name, M, rpb, by_batch, with_dx_in):
    """plain: one block over all rows; AdaLN: one single-block launch per batch element (dx of every element's last, partial 16-row
    group included), the two unused dtab slots and the guards intact"""
    TK.ln_bwd_case(G, name, M, rpb, by_batch, with_dx_in, form="reproducible", fast_form=fast_form)


@gpu
@pytest.mark.parametrize("B,L", [(3, 100), (4, 1024)])
@pytest.mark.parametrize("mask_frac", [0.0, 0.5, 1.0])
def test_embed_bwd_reproducible(G, fast_form, B, L, mask_frac):
    """the kernel of its own: out-of-range tokens clamped as the forward clamps them, rows of absent tokens untouched, dpos prefilled"""
    TK.embed_case(G, B, L, mask_frac, form="reproducible", fast_form=fast_form)


@gpu
@pytest.mark.parametrize("B,one_timestep", [(16, False), (96, False), (97, False), (128, False), (97, True)])
def test_adaln_bwd_reproducible(G, fast_form, B, one_timestep):
    """the first holder of a timestep adds every later holder's share, with and without LDS; one_timestep: one writer adds 97 shares"""
    TK.adaln_bwd_case(G, B, form="reproducible", fast_form=fast_form, one_timestep=one_timestep)


# ============================================================================= CPU self-check of the checks (no GPU)
def seq_sum(terms):
    """f32 sum along axis 0 in ascending order, starting from the first term"""
    terms = np.asarray(terms, dtype=f32)
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1:], f32)
    return np.cumsum(terms, axis=0, dtype=f32)[-1]


def grouped_sum(terms, groups):
    """rows r, r + groups, r + 2 groups, ... summed in order by 'thread' r, then the `groups` partial sums in ascending order"""
    n = terms.shape[0]
    pad = (-n) % groups
    t = np.concatenate([terms, np.zeros((pad,) + terms.shape[1:], f32)]) if pad else terms
    return seq_sum(seq_sum(t.reshape((-1, groups) + terms.shape[1:])))


def npf(t):
    return t.detach().cpu().numpy().astype(f32)


def worst(got, want, bars):
    return max(TK.ratio(torch.from_numpy(np.ascontiguousarray(got[k])), want[k], bars[k]) for k in bars)


# ---- wgrad: a sequential sum over the rows (db: rows r mod 16 per thread, then the 16 partials)
def wgrad_emul(dY, X, dW0, db0, fault=None):
    y, x = npf(dY), npf(X)
    M = y.shape[0]
    if fault == "drop_last":
        M = (M - 1) // 128 * 128                                       # the last (partial) slab never staged
    acc = seq_sum(y[:M, :, None] * x[:M, None, :])
    cs = grouped_sum(y[:M], 16)
    if fault == "overwrite":
        return {"dW": acc, "db": cs}
    return {"dW": npf(dW0) + acc, "db": npf(db0) + cs}


def wgrad_cpu(M, N=12, K=20):
    g = torch.Generator().manual_seed(M)
    dY, X, dW0, db0 = (torch.randn(*s, generator=g) for s in ((M, N), (M, K), (N, K), (N,)))
    want, bound, want_db, bound_db = GF.wgrad_ref(dY, X, dW0, db0)
    return (dY, X, dW0, db0), {"dW": want, "db": want_db}, {"dW": bound, "db": bound_db}


@pytest.mark.parametrize("M", [129, 1000, 5000])
def test_cpu_wgrad_emulation_meets_bars(M):
    args, want, bars = wgrad_cpu(M)
    assert worst(wgrad_emul(*args), want, bars) < 1


@pytest.mark.parametrize("fault", ["drop_last", "overwrite"])
@pytest.mark.parametrize("M", [129, 1000, 5000])
def test_cpu_wgrad_faults_miss_bars(M, fault):
    args, want, bars = wgrad_cpu(M)
    assert worst(wgrad_emul(*args, fault=fault), want, bars) > 1


# ---- colsum / batch_rowsum: 256 / cpb row groups per column, each strided and sequential, then the groups in order
def colsum_cpb(N):
    cpb = 256
    while cpb > 1 and cpb // 2 >= N:
        cpb //= 2
    return cpb


def colsum_emul(Y, out0, fault=None):
    y = npf(Y)
    nrg = 256 // colsum_cpb(y.shape[1])
    if fault == "drop_last":
        y = y[:(y.shape[0] - 1) // nrg * nrg]                          # the last (partial) turn of the row groups
    s = grouped_sum(y, nrg)
    return {"out": s if fault == "overwrite" else npf(out0) + s}


@pytest.mark.parametrize("M,N", [(129, 1), (1000, 68), (5000, 12), (5000, 257), (1000, 4)])
def test_cpu_colsum_emulation_meets_bars_and_faults_miss(M, N):
    g = torch.Generator().manual_seed(M + N)
    Y, out0 = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    want, bound = GF.colsum_ref(Y, out0)
    assert worst(colsum_emul(Y, out0), {"out": want}, {"out": bound}) < 1
    for fault in ("drop_last", "overwrite"):
        assert worst(colsum_emul(Y, out0, fault), {"out": want}, {"out": bound}) > 1, fault


def batch_rowsum_emul(Y, B, L, fault=None):
    out = np.zeros((B, Y.shape[1]), f32)                               # the memset
    for b in range(B):
        part = colsum_emul(Y[b * L:(b + 1) * L], torch.zeros(Y.shape[1]), "drop_last" if fault == "drop_last" else None)["out"]
        slot = 0 if fault == "slot0" else b
        out[slot] = out[slot] + part
    return {"out": out}


@pytest.mark.parametrize("B,L,C", [(3, 129, 12), (16, 1000, 64), (97, 63, 68)])
def test_cpu_batch_rowsum_emulation_meets_bars_and_faults_miss(B, L, C):
    Y = torch.randn(B * L, C, generator=torch.Generator().manual_seed(L + C))
    want, bound = GF.batch_rowsum_ref(Y, B, L)
    assert worst(batch_rowsum_emul(Y, B, L), {"out": want}, {"out": bound}) < 1
    for fault in ("drop_last", "slot0"):
        assert worst(batch_rowsum_emul(Y, B, L, fault), {"out": want}, {"out": bound}) > 1, fault


# ---- ln_bwd: per launch, 16 row lanes sum their rows of the `rit` groups in order, then the 16 lanes in order; one add onto the slot
def ln_bwd_emul(s, fault=None):
    x, dh, st, gp, pre = npf(s.x), npf(s.dh), npf(s.stats), npf(s.gp), npf(s.pre)
    din = npf(s.dx_in) if s.dx_in is not None else None
    R = s.rpb if s.by_batch else s.M
    dx = np.zeros_like(x)
    acc = pre.copy()
    for b in range(s.nslot):
        rows = slice(b * R, (b + 1) * R)
        sel = 0 if not s.by_batch else int(s.sel[0 if fault == "sel0" else b])
        gm = gp[sel * s.gstride:sel * s.gstride + D]
        xh = (x[rows] - st[rows, :1]) * st[rows, 1:]
        g = dh[rows] * gm
        m1 = g.sum(1, keepdims=True, dtype=f32) * f32(1 / 64)
        m2 = (g * xh).sum(1, keepdims=True, dtype=f32) * f32(1 / 64)
        d = st[rows, 1:] * (g - m1 - xh * m2)
        n = (R - 1) // 16 * 16 if fault == "drop_last" else R          # the last (partial) 16-row group never visited
        dx[rows][:n] = (d if din is None else din[rows] + d)[:n]
        sums = np.concatenate([grouped_sum((dh[rows] * xh)[:n], 16), grouped_sum(dh[rows][:n], 16)])
        slot = 0 if fault == "slot0" else b
        acc[slot] = sums if fault == "overwrite" else acc[slot] + sums
    return {"dx": dx, "dgamma": acc[:, :D], "dbeta": acc[:, D:]}


LN_CPU = [(129, 1, False, False), (1000, 1, False, True), (5000, 1, False, False), (1600, 100, True, True), (9700, 100, True, False),
          (970, 10, True, True)]


@pytest.mark.parametrize("M,rpb,by_batch,with_dx_in", LN_CPU)
def test_cpu_ln_bwd_emulation_meets_bars(M, rpb, by_batch, with_dx_in):
    s = TK.ln_bwd_setup(M, rpb, by_batch, with_dx_in, dev="cpu")
    assert worst(ln_bwd_emul(s), s.want, s.bars) < 1


# A plain call has one slot and no selection to get wrong.  An overwritten prefill (of size 1) is injected where the bar can resolve it:
# over 5000 rows with every ninth dh scaled by 1e3, gamma(5000) sum |dh| is about 4, so there (as at 65,544 rows on the GPU) the bar cannot
# see it; at 129 and 1000 rows and in every per-batch slot of 10 or 100 rows it can.
LN_FAULTS = ([("drop_last", c) for c in LN_CPU] + [("overwrite", c) for c in LN_CPU if c[0] != 5000]
             + [(f, c) for f in ("slot0", "sel0") for c in LN_CPU if c[2]])


@pytest.mark.parametrize("fault,case", LN_FAULTS, ids=[f"{f}-M{c[0]}-rpb{c[1]}" for f, c in LN_FAULTS])
def test_cpu_ln_bwd_faults_miss_bars(fault, case):
    M, rpb, by_batch, with_dx_in = case
    s = TK.ln_bwd_setup(M, rpb, by_batch, with_dx_in, dev="cpu")
    assert worst(ln_bwd_emul(s, fault), s.want, s.bars) > 1


# ---- embed_bwd: one thread per table cell walks the rows in ascending order
def embed_bwd_emul(s, fault=None):
    tok, dx = s.tok.view(-1).numpy(), npf(s.dx)
    acc = np.zeros((TK.NE, D), f32)
    hit = np.zeros(TK.NE, bool)
    for row in range(s.M):
        t = int(tok[row])
        if fault == "drop_oob" and not 0 <= t < TK.NE:
            continue
        t = min(max(t, 0), TK.NE - 1)
        acc[t] += dx[row]
        hit[t] = True
    demb = npf(s.pre_e)
    demb[hit] = acc[hit] if fault == "overwrite" else demb[hit] + acc[hit]
    step = s.L + 1 if fault == "dpos_stride" else s.L
    pacc = np.zeros((s.L, D), f32)
    for l in range(s.L):
        pacc[l] = seq_sum(dx[l::step])
    return {"demb": demb, "dpos": pacc if fault == "overwrite" else npf(s.pre_p) + pacc}


@pytest.mark.parametrize("B,L", [(3, 100), (16, 129), (97, 10)])
@pytest.mark.parametrize("mask_frac", [0.0, 0.5, 1.0])
def test_cpu_embed_bwd_emulation_meets_bars_and_faults_miss(B, L, mask_frac):
    s = TK.embed_setup(B, L, mask_frac, dev="cpu")
    assert worst(embed_bwd_emul(s), s.want, s.bars) < 1
    for fault in ("overwrite", "dpos_stride", "drop_oob"):
        assert worst(embed_bwd_emul(s, fault), s.want, s.bars) > 1, fault


# ---- adaln_bwd: dW, db sequential over b; demb: the first holder of a timestep adds the shares in ascending b
def adaln_bwd_emul(s, fault=None):
    t = s.t.numpy()
    e, w, dtab = npf(s.emb)[t], npf(s.w), npf(s.dtab)
    sg = f32(1) / (f32(1) + np.exp(-e))
    si, ds = e * sg, sg * (f32(1) + e * (f32(1) - sg))
    sw, sb = seq_sum(dtab[:, :, None] * si[:, None, :]), seq_sum(dtab)
    inner = dtab @ w
    demb = npf(s.pre_e)
    for b in range(s.B):
        if fault != "every_holder" and t[b] in t[:b]:
            continue
        total = inner[b] * ds[b]
        for b2 in range(b + 1, s.B):
            if t[b2] == t[b] and fault != "repeat_once":
                total = total + inner[b2] * ds[b]
        demb[t[b]] = total if fault == "overwrite" else demb[t[b]] + total
    if fault == "overwrite":
        return {"demb": demb, "dw": sw, "db": sb}
    return {"demb": demb, "dw": npf(s.pre_w) + sw, "db": npf(s.pre_b) + sb}


@pytest.mark.parametrize("B,one_timestep", [(16, False), (97, False), (97, True)])
def test_cpu_adaln_bwd_emulation_meets_bars_and_faults_miss(B, one_timestep):
    s = TK.adaln_bwd_setup(B, dev="cpu", one_timestep=one_timestep)
    assert worst(adaln_bwd_emul(s), s.want, s.bars) < 1
    for fault in ("overwrite", "repeat_once", "every_holder"):
        assert worst(adaln_bwd_emul(s, fault), s.want, s.bars) > 1, fault


def test_cpu_form_record_sees_other_bits_and_disagreement():
    """the two assertions every reproducible case adds, on made-up outputs"""
    a = {"o": torch.tensor([1.0, -0.0])}
    bars = {"o": torch.tensor([1e-6, 1e-6], dtype=torch.float64)}
    assert TK.form_record(a, None, None, bars, True) == {}
    rec = TK.form_record(a, {"o": torch.tensor([1.0, 0.0])}, {"o": torch.tensor([1.0 + 4e-6, 0.0])}, bars, False)
    assert rec["same_bits"] is False and rec["forms_agree_ratio"] > 1 and rec["fast_multi_workgroup"] is False
    with pytest.raises(AssertionError):
        TK.assert_forms(rec)
    rec = TK.form_record(a, {"o": torch.tensor([1.0, -0.0])}, {"o": torch.tensor([1.0 + 1e-6, 0.0])}, bars, True)
    assert rec["same_bits"] is True and rec["forms_agree_ratio"] <= 1
    TK.assert_forms(rec)


# ----------------------------------------------------------------------------- the switch is back off (keep this test last)
@gpu
def test_switch_is_off_after_the_reproducible_cases(G):
    assert G.ops.set_deterministic(False) is False
