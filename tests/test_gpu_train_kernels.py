"""The D3PM training step's own kernels -- LayerNorm forward / backward (plain and AdaLN), GELU2, the token + position embedding and
its backward, the condition-token linears, the AdaLN table and its backward, the training attention pair and Adam -- against a plain
fp64 evaluation of the same operation, element by element, at the training shape of config C4 (bs 16, L = 4096: M = 65,536 rows) and
at the shapes where their index arithmetic changes (rows per block, batch elements per block, LDS / no-LDS instantiations, ragged
lengths, partial tiles).  The whole-model gradient tests (test_gpu_training) check B <= 2 only; a wrong slot, row or batch offset at
the real shape shows here as an error many orders of magnitude above the bars.

The reference is computed on the device in fp64 (attention one (batch, head) pair at a time: 4096 x 4096 scores).

Bars, per output element.  U = 2^-24; gamma(k) = U (8 + 2 sqrt(k)) for a sum of k terms (as in test_gpu_gemm_family); |.| below is
of the exact (fp64) values; a "prefill" is the nonzero value an accumulating output held before the call (+= outputs: both "overwrites"
and "adds twice" are errors of the size of the prefill or of the sum).
  * ln_fwd, per row (eps = 1e-5): the mean is a 64-term sum, e_mu = gamma(64) mean|x|; d = x - mean then carries e_d = e_mu + U |d|.
    The variance q / 64 = sum d^2 / 64 moves by dv = (2 sum |d| e_d + 64 e_mu^2 + gamma(64) sum d^2) / 64 + U (var + eps); rstd
    (sqrt, reciprocal: 2 ulp) has relative error r = dv / (2 (var + eps)) + 4 U.  stats: |mean| bar e_mu, rstd bar r rstd.
    y = d rstd g + b: bar |g| rstd (e_d + r |d|) + 3 U |d rstd g| + 2 U |b|.  (Large row means beside small variances are in the
    cases: there e_mu is comparable to the spread and the bar says so.)
  * ln_bwd with the kernel's inputs (f32 stats taken as exact): xh = (x - mean) rstd has 2 U |xh|; g = dh gamma has U |g|;
    m1 = mean g and m2 = mean(g xh) are 64-term sums: e1 = gamma(64) mean|g|, e2 = (gamma(64) + 3 U) mean|g xh|.
    dx = dx_in + rstd (g - m1 - xh m2): bar rstd (5 U (|g| + |m1|) + 7 U |xh m2| + e1 + |xh| e2) + U (|dx_in| + |dx|).
    dgamma[slot] += sum dh xh, dbeta[slot] += sum dh over the N rows of the slot: bar (gamma(N) + 3 U) sum |dh xh| (resp. gamma(N)
    sum |dh|) + 2 U |prefill|.
  * gelu2 (u = a s, s = sigmoid(z), z = 1.702 a): the argument carries 2 U |z| (the rounded constant and the product) and expf up to
    2 ulp (4 U), which move s by a relative (1 - s) (2 U |z| + 4 U); the add and the division 1 ulp each (4 U):
    ds = s ((1 - s) (2 U |z| + 4 U) + 4 U).
    forward: bar |a| ds + U |u| + 2^-120: below z = -88.72 expf(-z) overflows to inf and s, u and g' are 0 in f32, while the exact
    |u| <= 52 e^z < 1.6e-37 and |g'| <= (1 + |z|) e^z < 2.6e-37, both below 2^-120 = 7.5e-37.
    backward g' = s + z s (1 - s) = s (1 + z (1 - s)) cancels twice: near saturation in 1 - s, whose absolute error is that of s (ds,
    not a relative one), and around z = -1.28, where g' = 0 and its two terms, each of size s, cancel.  Neither error is relative to g':
    the bar is (ds (1 + |z|) + 6 U |z| s (1 - s) + 2 U |g'| + 2^-120) |du| + U |du g'| + 2^-120.
  * embedding forward: one f32 add, correctly rounded: equal bit for bit to the f32 sum of the two f32 table rows.
    embedding backward: demb[v] += sum of the dx rows with clamp(tok) = v (n_v rows), dpos[l] += sum over the batch:
    gamma(n) sum |dx| + 2 U |prefill|; rows of tokens that do not occur are untouched, bit for bit.
  * small_linear: gamma(Cin) (|x| |W|^T + |b|); small_linear_bwd: dx gamma(Cout) |dy| |W|, dW gamma(R) |dy|^T |x| + 2 U |prefill|,
    db gamma(R) sum |dy| + 2 U |prefill|.
  * SiLU in f32 (e / (1 + expf(-e))): relative error (1 - s) 2 U |e| + 5 U =: ds_e;  SiLU' = s (1 + e (1 - s)) as GELU2's g'.
    adaln_table: gamma(D) (sum_k |silu_k W_jk| + |b_j|) + sum_k |silu_k W_jk| ds_e,k + U (1 + |table|).
    adaln_bwd: dW += dtab^T silu: (gamma(B) + ds_e) sum_b |dtab silu| + 2 U |prefill|;  db: gamma(B) sum |dtab| + 2 U |prefill|;
    demb[t] += silu'(e_t) (dtab W)[b] over the b with t_b = t: sum_b (gamma(2D) (|dtab| |W|) |silu'| + |dtab W| e(silu')) then
    gamma(n_t) over the repeats, + 2 U |prefill|.
  * attention (head dim 4, softmax(q k^T / 2) v, lse in the log2 domain as the kernels keep it; c = log2(e) / 2):
    scores from error-free bf16 splits and P (and dS) as bf16 hi + lo pairs (2^-17 each): unit 2^-16 + gamma(L) on every sum,
    + 8 U (1 + c max_j sum_f |q_if k_jf|) for the scores and exp2.  out: that times sum_j P_ij |v_jf|.  The default forward at
    L >= 2048 is adaptive (lo half only on tiles that can hold 2^-8 of a row's sum); its documented bound is 2e-5 of the row
    scale, i.e. 2e-5 max_j |v_jf| of the (batch, head), which is its bar; the hi + lo mode ("22") is held to the derived one.
    lse: 8 U c max_j sum_f |q k| + (2^-16 + gamma(L)) / ln 2 + 4 U (|lse| + 1).  VALU kernels (L % 32 != 0): unit gamma(L) + 8 U.
    Backward (fed the kernel's own out and lse, as the step does): P carries eP_i = ln 2 bar_lse_i, delta_i = dO_i . o_i carries
    Dd_i = sum_f |dO_if| bar_o_if; with A_ij = |dS_ij| (eP_i + unit) + P_ij (Dd_i + 4 U (|dP_ij| + |delta_i|)):
    dq bar 1/2 A |k|, dk bar 1/2 A^T |q|, dv bar (P (eP + unit))^T |dO|.
  * Adam (betas and eps as the f32 values the kernel gets; bias corrections 1 - beta^step evaluated in fp64 for the reference):
    m' carries 2 U (|b1 m| + |(1 - b1) g|), v' 3 U v'; a bias correction carries 4 U beta^step / (1 - beta^step) + U (pow in f32 or
    in double, then the subtraction).  The step dp = lr / bc1 m' / (sqrt(v' / bc2) + eps) then has
    bar (lr / bc1) e_m' / den + |dp| (e_bc1 + (e_v' / v' + e_bc2) / 2 + 8 U) and p' adds U |p'|.
Every case records its worst error / bar ratio with tests.conftest.parity_report (train_kernels::*).  The case bodies of ln_bwd, the
embedding pair and adaln_bwd are plain functions with a `form` argument: the tests here run the fast form (float atomics), those of
tests/test_gpu_train_reproducible.py the reproducible one (gsdd_set_deterministic) against the same reference, bars and guards.

Memory the kernels must not write is filled with a sentinel and checked bit for bit: rows past M (ln_fwd stats and y, embedding
rows), unused dtab slots and the gaps between accumulated outputs, demb / dW / db guard rows, the 4-float padding of Adam's m and v
and the gaps between Adam's parameters."""
import math
import types

import numpy as np
import pytest
import torch

from tests.conftest import parity_report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
D = 64
SENT = -7777.0
LN2 = math.log(2.0)
C_ATT = 0.5 / LN2


def gam(k):
    return U * (8 + 2 * np.sqrt(np.asarray(k, dtype=np.float64)))


def gamt(k):
    """gamma(k) for a tensor of term counts"""
    return U * (8 + 2 * torch.sqrt(k.double()))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def cgen(seed, dev="cuda"):
    return torch.Generator(device=dev).manual_seed(seed)


def ratio(got, want, bar):
    """worst |got - want| / bar (a non-finite result counts as infinitely wrong)"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    return float(torch.where(err == 0, 0.0, err / bar).max())


def guarded(n_before, shape, n_after, fill, dev="cuda"):
    """-> (buffer, view): a contiguous view of `shape` with n_before / n_after sentinel floats around it, the view holding `fill`"""
    n = int(np.prod(shape))
    buf = torch.full((n_before + n + n_after,), SENT, dtype=torch.float32, device=dev)
    v = buf[n_before:n_before + n].view(shape)
    v.copy_(fill)
    return buf, v


def guards_intact(buf, n_before, n, n_after):
    return bool((buf[:n_before] == SENT).all()) and bool((buf[n_before + n:] == SENT).all())


# ----------------------------------------------------------------------------- the two forms of the gradient reductions
# The case bodies of ln_bwd, embed_bwd and adaln_bwd below take form = "fast" (this file's tests: the switch is off) or "reproducible"
# (tests/test_gpu_train_reproducible.py: its fixture holds ops.set_deterministic(True) for the test and hands in `fast_form`, a context
# manager that turns the switch off for the one comparison run).  Reference, bars and guards are the same for both.
def form_key(form):
    return "" if form == "fast" else "[reproducible]"


def run_forms(run, form, fast_form=None):
    """run() -> dict of output tensors of one call from a fresh copy of the prefill.  -> (out, second run or None, fast-form run or
    None): the reproducible form runs twice, and once more in the fast form for the agreement of the two"""
    assert form in ("fast", "reproducible")
    if form == "fast":
        return run(), None, None
    with fast_form():
        fast = run()
    return run(), run(), fast


def same_bits(a, b):
    """every output of two runs equal in bits (buffers with their guards included)"""
    return all(bool(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))) for k in a)


def form_record(out, again, fast, bars, fast_multi_wg):
    """parity-report entries of a reproducible case: equal bits on the second run, the worst |reproducible - fast| / (bar + bar) over
    the outputs named in `bars` (both forms are held to the same bar), and whether the fast form spreads one output address over more
    than one workgroup (only then do equal bits say something the fast form would not)"""
    if again is None:
        return {}
    agree = max(ratio(out[k], fast[k].double(), 2 * bars[k]) for k in bars)
    return {"same_bits": same_bits(out, again), "forms_agree_ratio": agree, "fast_multi_workgroup": bool(fast_multi_wg)}


def assert_forms(rec):
    if rec:
        assert rec["same_bits"], "the reproducible form gave other bits on its second run"
        assert rec["forms_agree_ratio"] <= 1, f"fast and reproducible form differ by {rec['forms_agree_ratio']:.3g} of their two bars"


# ----------------------------------------------------------------------------- LayerNorm forward
def ln_rows(M, seed, wild=True, dev="cuda"):
    """rows of 64 with spread ~1, and (wild) large means beside small spreads"""
    g = cgen(seed, dev)
    x = torch.randn(M, D, generator=g, device=dev)
    if wild:
        r = torch.arange(M, device=dev)
        mu = torch.where(r % 5 == 0, 1e3, torch.where(r % 5 == 1, -300.0, 0.0))
        sd = torch.where(r % 7 == 0, 1e-2, torch.where(r % 7 == 1, 30.0, 1.0))
        x = x * sd[:, None] + mu[:, None]
    return x.contiguous()


def ln_fwd_ref(x, g, b):
    """fp64 (stats [M][2], y, bar_mean, bar_rstd, bar_y) for per-row affine g, b [M][64]"""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    d = xd - mu
    var = d.square().mean(1, keepdim=True)
    rs = (var + 1e-5).rsqrt()
    e_mu = gam(64) * xd.abs().mean(1, keepdim=True)
    e_d = e_mu + U * d.abs()
    dv = (2 * (d.abs() * e_d).sum(1, keepdim=True) + 64 * e_mu ** 2 + gam(64) * d.square().sum(1, keepdim=True)) / 64 + U * (var + 1e-5)
    r = dv / (2 * (var + 1e-5)) + 4 * U
    y = d * rs * g + b
    bar_y = g.abs() * rs * (e_d + r * d.abs()) + 3 * U * (d * rs * g).abs() + 2 * U * b.abs()
    return torch.cat([mu, rs], 1), y, e_mu[:, 0], (r * rs)[:, 0], bar_y


@pytest.mark.parametrize("case", ["plain_M65536", "adaln_B16_L4096", "adaln_ragged_B7_L100", "plain_ragged_M1000"])
def test_ln_fwd_matches_fp64(G, case):
    T = 100
    if case.startswith("plain"):
        B, L = 1, (65536 if case == "plain_M65536" else 1000)
    else:
        B, L = (16, 4096) if case == "adaln_B16_L4096" else (7, 100)
    M = B * L
    x = ln_rows(M, 11 + M)
    g = cgen(12)
    if case.startswith("plain"):
        gamma, beta = torch.randn(D, generator=g, device="cuda") + 1, torch.randn(D, generator=g, device="cuda")
        sel, gstride = None, 0
        gr, br = gamma.double().expand(M, D), beta.double().expand(M, D)
        gp, bp = gamma, beta
    else:
        tab = torch.randn(T, 2 * D, generator=g, device="cuda")
        tab[:, :D] += 1
        t = torch.randint(0, T, (B,), generator=g, device="cuda")
        t[0], t[-1] = 0, T - 1
        t[1] = t[2] = t[-1]                                       # duplicates
        sel, gstride = t.contiguous(), 2 * D
        bidx = torch.arange(M, device="cuda") // L
        gr, br = tab.double()[t[bidx], :D], tab.double()[t[bidx], D:]
        gp, bp = tab.view(-1), tab.view(-1)[D:]
    GUARD = 64
    sbuf = torch.full(((M + GUARD) * 2,), SENT, device="cuda")
    ybuf = torch.full(((M + GUARD) * D,), SENT, device="cuda")
    O = G.ops
    O.check(O.lib().gsdd_ln_fwd(O.ptr(x), M, D, 1e-5, O.ptr(gp), O.ptr(bp), O.ptr(sel), gstride, L, O.ptr(sbuf), O.ptr(ybuf),
                                O.stream_ptr()))
    stats, y = sbuf[:2 * M].view(M, 2), ybuf[:M * D].view(M, D)
    want_s, want_y, bm, br_, by = ln_fwd_ref(x, gr, br)
    rm = ratio(stats[:, 0], want_s[:, 0], bm)
    rr = ratio(stats[:, 1], want_s[:, 1], br_)
    ry = ratio(y, want_y, by)
    intact = bool((sbuf[2 * M:] == SENT).all()) and bool((ybuf[M * D:] == SENT).all())
    parity_report(f"train_kernels::ln_fwd[{case}]", {"M": M, "rows_per_batch": L, "mean_ratio": rm, "rstd_ratio": rr, "y_ratio": ry,
                                                    "worst_ratio": max(rm, rr, ry)})
    assert intact, "ln_fwd wrote past row M"
    assert rm <= 1 and rr <= 1 and ry <= 1, (rm, rr, ry)


# ----------------------------------------------------------------------------- LayerNorm backward
LN_BWD_CASES = [
    # (name, M, rows_per_batch, acc_by_batch, dx_in)
    ("plain_rit1_ragged", 1000, 1, False, False),
    ("plain_rit2_ragged_dxin", 20008, 1, False, True),
    ("plain_rit4_ragged", 65544, 1, False, False),
    ("plain_rit4_dxin", 65536, 1, False, True),
    ("adaln_rpb4096_B16_rit4", 65536, 4096, True, True),
    ("adaln_rpb4096_B4_rit2", 16384, 4096, True, False),
    ("adaln_rpb4096_B2_rit1", 8192, 4096, True, True),
    ("adaln_rpb16_rit1", 65536, 16, True, True),
    ("adaln_rpb32_rit2", 65536, 32, True, False),
    ("adaln_rpb48_rit1", 65568, 48, True, True),
    ("adaln_rpb100_straddle_B16", 1600, 100, True, True),
    ("adaln_rpb100_straddle_B656", 65600, 100, True, False),
    ("adaln_rpb10_straddle", 4000, 10, True, True),
]


def ln_bwd_fast_rit(M, rpb, by_batch):
    """16-row groups per block as gsdd_ln_bwd's fast form picks them"""
    rit = 4
    while rit > 1 and ((by_batch and rpb % (16 * rit) != 0) or M < 16 * rit * 512):
        rit >>= 1
    return rit


def ln_bwd_setup(M, rpb, by_batch, with_dx_in, dev="cuda"):
    """Inputs, prefill and the fp64 reference with its bars of one LayerNorm-backward case.  AdaLN cases use the trainer's dtab layout
    exactly: one [B][2D] table, dgamma = dtab, dbeta = dtab + D, gacc_stride = 2D (gamma and beta gradients interleaved row by row),
    plus two unused slots after it."""
    T = 100
    g = cgen(M + rpb, dev)
    x = ln_rows(M, M + 3 * rpb, dev=dev)
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    rs = ((xd - mu).square().mean(1, keepdim=True) + 1e-5).rsqrt()
    stats = torch.cat([mu, rs], 1).float().contiguous()
    dh = torch.randn(M, D, generator=g, device=dev)
    dh[::9] *= 1e3
    dx_in = torch.randn(M, D, generator=g, device=dev) if with_dx_in else None
    if by_batch:
        B = M // rpb
        assert B * rpb == M
        tab = torch.randn(T, 2 * D, generator=g, device=dev) + 1
        t = torch.randint(0, T, (B,), generator=g, device=dev)
        t[0], t[-1] = 0, T - 1
        if B > 3:
            t[1] = t[2] = 0
        t = t.contiguous()
        bidx = torch.arange(M, device=dev) // rpb
        gam_rows = tab.double()[t[bidx], :D]
        gp, sel, gstride = tab.view(-1), t, 2 * D
        nslot, nrows = B, torch.full((B,), rpb, device=dev)
        pre = torch.randn(B, 2 * D, generator=g, device=dev)
    else:
        gamma = torch.randn(D, generator=g, device=dev) + 1
        gam_rows = gamma.double().expand(M, D)
        gp, sel, gstride = gamma, None, 0
        bidx = torch.zeros(M, dtype=torch.long, device=dev)
        nslot, nrows = 1, torch.full((1,), M, device=dev)
        pre = torch.randn(1, 2 * D, generator=g, device=dev)
    # fp64 reference from the same f32 inputs
    sd = stats.double()
    xh = (xd - sd[:, :1]) * sd[:, 1:]
    gg = dh.double() * gam_rows
    m1, m2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    din = dx_in.double() if dx_in is not None else torch.zeros_like(xd)
    want_dx = din + sd[:, 1:] * (gg - m1 - xh * m2)
    e1, e2 = gam(64) * gg.abs().mean(1, keepdim=True), (gam(64) + 3 * U) * (gg * xh).abs().mean(1, keepdim=True)
    bar_dx = sd[:, 1:] * (5 * U * (gg.abs() + m1.abs()) + 7 * U * (xh * m2).abs() + e1 + xh.abs() * e2) + U * (din.abs() + want_dx.abs())
    z = torch.zeros(nslot, D, dtype=torch.float64, device=dev)

    def slot_sum(v):
        # (one slot: the plain fp64 column sum -- index_add of 65,544 rows onto one row is 5 s of contended fp64 atomics per case)
        return v.sum(0, keepdim=True) if nslot == 1 else z.index_add(0, bidx, v)
    sg, sb = slot_sum(dh.double() * xh), slot_sum(dh.double())
    ag, ab = slot_sum((dh.double() * xh).abs()), slot_sum(dh.double().abs())
    pd = pre.double()
    gk = gamt(nrows)[:, None]
    want = {"dx": want_dx, "dgamma": pd[:, :D] + sg, "dbeta": pd[:, D:] + sb}
    bars = {"dx": bar_dx, "dgamma": (gk + 3 * U) * ag + 2 * U * pd[:, :D].abs(), "dbeta": gk * ab + 2 * U * pd[:, D:].abs()}
    return types.SimpleNamespace(M=M, rpb=rpb, by_batch=by_batch, nslot=nslot, x=x, stats=stats, dh=dh, dx_in=dx_in, gp=gp, sel=sel,
                                 gstride=gstride, pre=pre, want=want, bars=bars)


def ln_bwd_run(G, s):
    """one call from a fresh copy of the prefill -> dx, the gradient slots [slots][64] (views of `buf`), the guarded buffer, guards"""
    if s.by_batch:
        buf, dtab = guarded(0, (s.nslot, 2 * D), 2 * 2 * D, s.pre)
        dgamma, dbeta, acc_stride = dtab, dtab.view(-1)[D:], 2 * D
        got_g, got_b = dtab[:, :D], dtab[:, D:]
    else:
        # dgamma and dbeta as the trainer hands them out (two arena views), with sentinel gaps around and between them
        buf = torch.full((16 + D + 16 + D + 16,), SENT, device="cuda")
        dgamma, dbeta = buf[16:16 + D], buf[32 + D:32 + 2 * D]
        dgamma.copy_(s.pre[0, :D])
        dbeta.copy_(s.pre[0, D:])
        acc_stride = D
        got_g, got_b = dgamma[None], dbeta[None]
    dx = G.ops.ln_bwd(s.dh, s.x, s.stats, s.gp, sel=s.sel, gstride=s.gstride, rows_per_batch=s.rpb, dx_in=s.dx_in, dgamma=dgamma,
                      dbeta=dbeta, gacc_stride=acc_stride, acc_by_batch=s.by_batch)
    if s.by_batch:
        intact = guards_intact(buf, 0, s.nslot * 2 * D, 4 * D)
    else:
        intact = bool((buf[:16] == SENT).all()) and bool((buf[16 + D:32 + D] == SENT).all()) and bool((buf[32 + 2 * D:] == SENT).all())
    return {"dx": dx, "dgamma": got_g, "dbeta": got_b, "buf": buf, "intact": torch.tensor([int(intact)], dtype=torch.int32)}


def ln_bwd_ratios(s, out):
    return tuple(ratio(out[k], s.want[k], s.bars[k]) for k in ("dx", "dgamma", "dbeta"))


def ln_bwd_case(G, name, M, rpb, by_batch, with_dx_in, form="fast", fast_form=None):
    """dx, dgamma, dbeta of the LayerNorm backward in one of its two forms"""
    s = ln_bwd_setup(M, rpb, by_batch, with_dx_in)
    out, again, fast = run_forms(lambda: ln_bwd_run(G, s), form, fast_form)
    r_dx, r_g, r_b = ln_bwd_ratios(s, out)
    rit = ln_bwd_fast_rit(M, rpb, by_batch)
    multi = (rpb % 16 != 0 or rpb > 16 * rit) if by_batch else M > 16 * rit
    rec = form_record(out, again, fast, s.bars, multi)
    parity_report(f"train_kernels::ln_bwd[{name}]{form_key(form)}", {"M": M, "rows_per_batch": rpb, "dx_ratio": r_dx, "dgamma_ratio": r_g,
                                                                     "dbeta_ratio": r_b, "worst_ratio": max(r_dx, r_g, r_b), **rec})
    assert bool(out["intact"]), "ln_bwd wrote outside its gradient slots"
    assert r_dx <= 1 and r_g <= 1 and r_b <= 1, (r_dx, r_g, r_b)
    assert_forms(rec)


@pytest.mark.parametrize("name,M,rpb,by_batch,with_dx_in", LN_BWD_CASES, ids=[c[0] for c in LN_BWD_CASES])
def test_ln_bwd_matches_fp64(G, name, M, rpb, by_batch, with_dx_in):
    """dx, dgamma, dbeta of the LayerNorm backward.  AdaLN cases use the trainer's dtab layout exactly: one [B][2D] table, dgamma =
    dtab, dbeta = dtab + D, gacc_stride = 2D (gamma and beta gradients interleaved row by row), plus two unused slots after it."""
    ln_bwd_case(G, name, M, rpb, by_batch, with_dx_in, form="fast")


# ----------------------------------------------------------------------------- GELU2
def gelu2_grid(n, seed):
    special = torch.tensor([0.0, 1e-30, -1e-30, 1e-10, -1e-10, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 20.0, -20.0, 50.0, -50.0, 52.0, -52.0,
                            60.0, -60.0, 100.0, -100.0, 88.0 / 1.702, -88.0 / 1.702, 90.0 / 1.702, -90.0 / 1.702], device="cuda")
    if n == 4:
        return torch.tensor([-100.0, 1e-30, 0.0, 100.0], device="cuda")
    g = cgen(seed)
    a = torch.randn(n, generator=g, device="cuda") * 3
    q = n // 4
    a[q:2 * q] = (torch.rand(q, generator=g, device="cuda") * 2 - 1) * 100        # out to where expf overflows
    a[2 * q:2 * q + 4096] = torch.linspace(-12, 12, 4096, device="cuda")          # the transition region, densely
    a[:special.numel()] = special
    return a.contiguous()


def gelu2_ref(a):
    ad = a.double()
    z = 1.702 * ad
    s = torch.sigmoid(z)
    ds = s * ((1 - s) * (2 * U * z.abs() + 4 * U) + 4 * U)
    u = ad * s
    gp = s * (1 + z * (1 - s))
    return u, ad.abs() * ds + U * u.abs() + 2.0 ** -120, gp, ds * (1 + z.abs()) + 6 * U * z.abs() * s * (1 - s) + 2 * U * gp.abs()


@pytest.mark.parametrize("n", [4, 65536 * 256])
def test_gelu2_forward_backward_match_fp64(G, n):
    a = gelu2_grid(n, 5)
    du = torch.randn(n, generator=cgen(6), device="cuda")
    du[:8] = 1.0
    u, bar_u, gp, bar_gp = gelu2_ref(a)
    got_u = G.ops.gelu2(a)
    got_da = G.ops.gelu2(a, du)
    dud = du.double()
    want_da = dud * gp
    r_u = ratio(got_u, u, bar_u)
    r_d = ratio(got_da, want_da, dud.abs() * (bar_gp + 2.0 ** -120) + U * want_da.abs() + 2.0 ** -120)
    parity_report(f"train_kernels::gelu2[n{n}]", {"n": n, "fwd_ratio": r_u, "bwd_ratio": r_d, "worst_ratio": max(r_u, r_d)})
    assert r_u <= 1 and r_d <= 1, (r_u, r_d)


# ----------------------------------------------------------------------------- token + position embedding
NE = 4097


def embed_setup(B, L, mask_frac, dev="cuda"):
    """Tokens (out-of-range ones included), tables, dx, prefill and the fp64 reference with its bars of one embedding case"""
    M = B * L
    g = cgen(B * 7 + int(mask_frac * 10), dev)
    tok = torch.randint(0, NE - 1, (M,), generator=g, device=dev)
    tok[torch.rand(M, generator=g, device=dev) < mask_frac] = NE - 1
    tok[5], tok[17], tok[M - 1], tok[M // 2] = -3, NE, NE + 900, -1
    tok = tok.view(B, L).contiguous()
    emb = torch.randn(NE, D, generator=g, device=dev)
    pos = torch.randn(L, D, generator=g, device=dev)
    tc = tok.view(-1).clamp(0, NE - 1)
    dx = torch.randn(M, D, generator=g, device=dev)
    dx[::13] *= 100
    pre_e = torch.randn(NE, D, generator=g, device=dev)
    pre_p = torch.randn(L, D, generator=g, device=dev)
    dd = dx.double()
    z = torch.zeros(NE, D, dtype=torch.float64, device=dev)
    cnt = torch.bincount(tc, minlength=NE)
    want = {"demb": pre_e.double() + z.index_add(0, tc, dd), "dpos": pre_p.double() + dd.view(B, L, D).sum(0)}
    bars = {"demb": gamt(cnt)[:, None] * z.index_add(0, tc, dd.abs()) + 2 * U * pre_e.double().abs(),
            "dpos": gam(B) * dd.abs().view(B, L, D).sum(0) + 2 * U * pre_p.double().abs()}
    return types.SimpleNamespace(B=B, L=L, M=M, tok=tok, tc=tc, emb=emb, pos=pos, dx=dx, pre_e=pre_e, pre_p=pre_p, cnt=cnt, want=want,
                                 bars=bars)


def embed_bwd_run(G, s):
    ebuf, demb = guarded(0, (NE, D), 4 * D, s.pre_e)
    pbuf, dpos = guarded(0, (s.L, D), 4 * D, s.pre_p)
    G.ops.d3pm_embed_bwd(s.dx, s.tok, demb, dpos)
    return {"demb": demb, "dpos": dpos, "ebuf": ebuf, "pbuf": pbuf}


def embed_case(G, B, L, mask_frac, form="fast", fast_form=None):
    """x = emb[clamp(tok)] + pos[row % L]; backward demb[clamp(tok)] += dx, dpos[row % L] += dx, the backward in one of its two forms"""
    s = embed_setup(B, L, mask_frac)
    M = s.M
    GUARD = 256
    xbuf = torch.full(((M + GUARD) * D,), SENT, device="cuda")
    O = G.ops
    O.check(O.lib().gsdd_d3pm_embed(O.ptr(s.tok), B, L, D, O.ptr(s.emb), NE, O.ptr(s.pos), 1, O.ptr(xbuf), O.stream_ptr()))
    x = xbuf[:M * D].view(M, D)
    want_x = s.emb[s.tc] + s.pos.repeat(B, 1)                     # one f32 add: correctly rounded, so equal bit for bit
    fwd_exact = bool(torch.equal(x, want_x))
    fwd_guard = bool((xbuf[M * D:] == SENT).all())
    out, again, fast = run_forms(lambda: embed_bwd_run(G, s), form, fast_form)
    r_e, r_p = ratio(out["demb"], s.want["demb"], s.bars["demb"]), ratio(out["dpos"], s.want["dpos"], s.bars["dpos"])
    untouched = bool(torch.equal(out["demb"][s.cnt == 0], s.pre_e[s.cnt == 0]))
    guards = guards_intact(out["ebuf"], 0, NE * D, 4 * D) and guards_intact(out["pbuf"], 0, L * D, 4 * D)
    # fast form: one atomic per row (per block for [MASK]) from blocks of 256 rows; with more than one block a position's B rows and the
    # [MASK] row's many come from several workgroups
    rec = form_record(out, again, fast, s.bars, M > 256)
    parity_report(f"train_kernels::embed[B{B}_L{L}_mask{mask_frac}]{form_key(form)}",
                  {"rows": M, "masked_rows": int(s.cnt[NE - 1]), "fwd_bit_exact": fwd_exact, "demb_ratio": r_e, "dpos_ratio": r_p,
                   "worst_ratio": max(r_e, r_p), **rec})
    assert fwd_exact and fwd_guard, "embedding forward"
    assert untouched and guards, "embedding backward wrote rows of tokens that do not occur, or past its tables"
    assert r_e <= 1 and r_p <= 1, (r_e, r_p)
    assert_forms(rec)


@pytest.mark.parametrize("B,L", [(16, 4096), (3, 100)])
@pytest.mark.parametrize("mask_frac", [0.0, 0.5, 1.0])
def test_embed_and_embed_bwd_match_fp64(G, B, L, mask_frac):
    """x = emb[clamp(tok)] + pos[row % L]; backward demb[clamp(tok)] += dx, dpos[row % L] += dx.  n_embed = 4097 (K = 4096 codes and
    [MASK] = 4096, the row the backward sums per block).  Tokens below 0 and at or above n_embed are clamped by the forward (to 0 and
    to [MASK]); the backward must send their gradient to the same rows."""
    embed_case(G, B, L, mask_frac, form="fast")


# ----------------------------------------------------------------------------- condition-token linears
@pytest.mark.parametrize("R", [1, 16, 128])
@pytest.mark.parametrize("Cin", [512, 64])
def test_small_linear_and_bwd_match_fp64(G, R, Cin):
    Cout = 64
    g = cgen(R * 1000 + Cin)
    x = torch.randn(R, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, Cin, generator=g, device="cuda") / math.sqrt(Cin)
    b = torch.randn(Cout, generator=g, device="cuda")
    y = G.ops.small_linear(x, w, b)
    xd, wd, bd = x.double(), w.double(), b.double()
    r_y = ratio(y, xd @ wd.t() + bd, gam(Cin) * (xd.abs() @ wd.abs().t() + bd.abs()))
    dy = torch.randn(R, Cout, generator=g, device="cuda")
    dyd = dy.double()
    res = {"y_ratio": r_y}
    for want_dx in (True, False):
        pre_w = torch.randn(Cout, Cin, generator=g, device="cuda")
        pre_b = torch.randn(Cout, generator=g, device="cuda")
        wbuf, dw = guarded(64, (Cout, Cin), 64, pre_w)
        bbuf, db = guarded(64, (Cout,), 64, pre_b)
        dx = G.ops.small_linear_bwd(dy, x, w, dw, db, want_dx=want_dx)
        if want_dx:
            res["dx_ratio"] = ratio(dx, dyd @ wd, gam(Cout) * (dyd.abs() @ wd.abs()))
        k = "" if want_dx else "_no_dx"
        res["dw_ratio" + k] = ratio(dw, pre_w.double() + dyd.t() @ xd, gam(R) * (dyd.abs().t() @ xd.abs()) + 2 * U * pre_w.double().abs())
        res["db_ratio" + k] = ratio(db, pre_b.double() + dyd.sum(0), gam(R) * dyd.abs().sum(0) + 2 * U * pre_b.double().abs())
        assert guards_intact(wbuf, 64, Cout * Cin, 64) and guards_intact(bbuf, 64, Cout, 64), "small_linear_bwd wrote outside dW / db"
    worst = max(res.values())
    parity_report(f"train_kernels::small_linear[R{R}_Cin{Cin}]", {**res, "worst_ratio": worst})
    assert worst <= 1, res


# ----------------------------------------------------------------------------- AdaLN table and its backward
def silu_parts(e):
    s = torch.sigmoid(e)
    ds_e = (1 - s) * 2 * U * e.abs() + 5 * U
    d1 = s * (1 + e * (1 - s))
    e_d1 = s * ds_e * (1 + e.abs()) + 6 * U * e.abs() * s * (1 - s) + 2 * U * d1.abs()
    return e * s, ds_e, d1, e_d1


def test_adaln_table_matches_fp64(G):
    T = 100
    g = cgen(31)
    emb = torch.randn(T, D, generator=g, device="cuda") * 3
    emb[0, :4] = torch.tensor([0.0, 60.0, -60.0, 1e-30])
    w = torch.randn(2 * D, D, generator=g, device="cuda") / 8
    b = torch.randn(2 * D, generator=g, device="cuda")
    out = G.ops.adaln_table(emb, w, b)
    si, ds_e, _, _ = silu_parts(emb.double())
    wd, bd = w.double(), b.double()
    want = si @ wd.t() + bd
    want[:, :D] += 1
    mag = si.abs() @ wd.abs().t()
    bar = gam(D) * (mag + bd.abs()) + (si.abs() * ds_e) @ wd.abs().t() + U * (1 + want.abs())
    r = ratio(out, want, bar)
    parity_report("train_kernels::adaln_table[T100_D64]", {"worst_ratio": r})
    assert r <= 1, r


def adaln_bwd_setup(B, dev="cuda", one_timestep=False):
    """Inputs, prefill and the fp64 autograd reference with its bars.  t holds repeated timesteps (several clips accumulating into one
    demb row), 0 and T - 1; one_timestep: every clip holds timestep 7"""
    T = 100
    g = cgen(40 + B, dev)
    emb = torch.randn(T, D, generator=g, device=dev) * 2
    w = torch.randn(2 * D, D, generator=g, device=dev) / 8
    t = torch.randint(0, T, (B,), generator=g, device=dev)
    t[0], t[1], t[-1] = 0, T - 1, T - 1
    t[2:6] = 7
    if one_timestep:
        t[:] = 7
    t = t.contiguous()
    dtab = torch.randn(B, 2 * D, generator=g, device=dev)
    pre_e, pre_w, pre_b = (torch.randn(*s, generator=g, device=dev) for s in ((T, D), (2 * D, D), (2 * D,)))
    # fp64 autograd of table[t] = (1 + W silu(e_t) + b | W' silu(e_t) + b')
    ed = emb.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = torch.zeros(2 * D, dtype=torch.float64, device=dev, requires_grad=True)
    tab = torch.nn.functional.silu(ed[t]) @ wd.t() + bd
    tab = torch.cat([1 + tab[:, :D], tab[:, D:]], 1)
    tab.backward(dtab.double())
    si, ds_e, d1, e_d1 = silu_parts(emb.double()[t])
    dtd = dtab.double()
    cnt = torch.bincount(t, minlength=T)
    inner = dtd @ w.double()
    inner_mag = dtd.abs() @ w.double().abs()
    per_b = gam(2 * D) * inner_mag * d1.abs() + inner.abs() * e_d1
    z = torch.zeros(T, D, dtype=torch.float64, device=dev)
    want = {"demb": pre_e.double() + ed.grad, "dw": pre_w.double() + wd.grad, "db": pre_b.double() + bd.grad}
    bars = {"demb": z.index_add(0, t, per_b) + gamt(cnt)[:, None] * z.index_add(0, t, (inner * d1).abs()) + 2 * U * pre_e.double().abs(),
            "dw": (gam(B) + ds_e.max()) * (dtd.abs().t() @ si.abs()) + 2 * U * pre_w.double().abs(),
            "db": gam(B) * dtd.abs().sum(0) + 2 * U * pre_b.double().abs()}
    return types.SimpleNamespace(B=B, T=T, emb=emb, w=w, t=t, dtab=dtab, pre_e=pre_e, pre_w=pre_w, pre_b=pre_b, cnt=cnt, want=want,
                                 bars=bars)


def adaln_bwd_run(G, s):
    dtab = s.dtab.clone()
    ebuf, demb = guarded(64, (s.T, D), 4 * D, s.pre_e)
    wbuf, dw = guarded(64, (2 * D, D), 64, s.pre_w)
    bbuf, db = guarded(64, (2 * D,), 64, s.pre_b)
    G.ops.adaln_bwd(dtab, s.t, s.emb, s.w, demb, dw, db)
    return {"demb": demb, "dw": dw, "db": db, "ebuf": ebuf, "wbuf": wbuf, "bbuf": bbuf, "dtab": dtab}


def adaln_bwd_case(G, B, form="fast", fast_form=None, one_timestep=False):
    s = adaln_bwd_setup(B, one_timestep=one_timestep)
    out, again, fast = run_forms(lambda: adaln_bwd_run(G, s), form, fast_form)
    r_e, r_w, r_b = (ratio(out[k], s.want[k], s.bars[k]) for k in ("demb", "dw", "db"))
    untouched = bool(torch.equal(out["demb"][s.cnt == 0], s.pre_e[s.cnt == 0]))
    guards = (guards_intact(out["ebuf"], 64, s.T * D, 4 * D) and guards_intact(out["wbuf"], 64, 2 * D * D, 64)
              and guards_intact(out["bbuf"], 64, 2 * D, 64))
    # fast form: the demb row of a repeated timestep gets one atomic per holder, from B D / 256 workgroups of 4 batch elements each
    rec = form_record(out, again, fast, s.bars, True)
    name = f"B{B}_one_timestep" if one_timestep else f"B{B}"
    parity_report(f"train_kernels::adaln_bwd[{name}]{form_key(form)}",
                  {"lds_instantiation": 2 * B * D * 4 <= 48 * 1024, "demb_ratio": r_e, "dw_ratio": r_w, "db_ratio": r_b,
                   "worst_ratio": max(r_e, r_w, r_b), **rec})
    assert torch.equal(out["dtab"], s.dtab), "adaln_bwd wrote its input"
    assert untouched and guards, "adaln_bwd wrote demb rows of timesteps that do not occur, or outside its outputs"
    assert r_e <= 1 and r_w <= 1 and r_b <= 1, (r_e, r_w, r_b)
    assert_forms(rec)


@pytest.mark.parametrize("B", [16, 96, 97, 128])
def test_adaln_bwd_matches_fp64_autograd(G, B):
    """B = 96 is the last batch whose 2 B D floats of SiLU / SiLU' fit the kernel's 48 KB of LDS; 97 the first that runs the
    instantiation without LDS.  t holds repeated timesteps (several clips accumulating into one demb row), 0 and T - 1."""
    adaln_bwd_case(G, B, form="fast")


# ----------------------------------------------------------------------------- training attention at the C4 shape
def attention_case(G, B, L, H, seed, fwd_mode, documented_fwd):
    """Forward (out, lse) and default backward (dq | dk | dv) against fp64, one (batch, head) pair at a time.  -> ratios dict"""
    g = cgen(seed)
    M = B * L
    mfma = L % 32 == 0
    qh = torch.randn(H, M, 4, generator=g, device="cuda") * 1.5
    kh = torch.randn(H, M, 4, generator=g, device="cuda") * 1.5
    vh = torch.randn(H, M, 4, generator=g, device="cuda")
    dO = torch.randn(M, H * 4, generator=g, device="cuda")
    GUARD = 64
    obuf = torch.full(((M + GUARD) * H * 4,), SENT, device="cuda")
    lbuf = torch.full((H * M + GUARD,), SENT, device="cuda")
    out, lse = obuf[:M * H * 4].view(M, H * 4), lbuf[:H * M]
    ws = G.ops.d3pm_attention_workspace(B, L, H, "cuda") if mfma else None
    G.ops.d3pm_attention_train(qh, kh, vh, B, L, H, out, lse, ws=ws, mode=fwd_mode)
    intact = bool((obuf[M * H * 4:] == SENT).all()) and bool((lbuf[H * M:] == SENT).all())
    bws = G.ops.d3pm_attention_bwd_workspace(B, L, H, "cuda") if mfma else None
    dqkv = G.ops.d3pm_attention_bwd(qh, kh, vh, out, dO, lse, B, L, H, ws=bws)
    torch.cuda.synchronize()
    unit = (2.0 ** -16 if mfma else 0.0) + gam(L)
    worst = {"out": 0.0, "lse": 0.0, "dq": 0.0, "dk": 0.0, "dv": 0.0}
    for b in range(B):
        rows = slice(b * L, (b + 1) * L)
        for h in range(H):
            q, k, v = (z[h, rows].double() for z in (qh, kh, vh))
            go = dO[rows, 4 * h:4 * h + 4].double()
            s = (q @ k.t()) * 0.5
            lse_n = torch.logsumexp(s, 1, keepdim=True)
            P = torch.exp(s - lse_n)
            o = P @ v
            amax = (q.abs() @ k.abs().t()).amax(1, keepdim=True)
            sc = 8 * U * (1 + C_ATT * amax)
            if documented_fwd:
                bar_o = 2e-5 * v.abs().amax(0, keepdim=True).expand_as(o)
            else:
                bar_o = (unit + sc) * (P @ v.abs())
            lse2 = lse_n / LN2
            bar_l = 8 * U * C_ATT * amax + unit / LN2 + 4 * U * (lse2.abs() + 1)
            worst["out"] = max(worst["out"], ratio(out[rows, 4 * h:4 * h + 4], o, bar_o))
            worst["lse"] = max(worst["lse"], ratio(lse[h * M + b * L:h * M + (b + 1) * L], lse2[:, 0], bar_l[:, 0]))
            dP = go @ v.t()
            delta = (go * o).sum(1, keepdim=True)
            dS = P * (dP - delta)
            eP = LN2 * bar_l
            Dd = (go.abs() * bar_o).sum(1, keepdim=True) + 4 * U * (go * o).abs().sum(1, keepdim=True)
            A = dS.abs() * (eP + unit) + P * (Dd + 4 * U * (dP.abs() + delta.abs()))
            del dP
            gr = dqkv[rows]
            worst["dq"] = max(worst["dq"], ratio(gr[:, 4 * h:4 * h + 4], 0.5 * dS @ k, 0.5 * A @ k.abs()))
            worst["dk"] = max(worst["dk"], ratio(gr[:, 64 + 4 * h:64 + 4 * h + 4], 0.5 * dS.t() @ q, 0.5 * A.t() @ q.abs()))
            worst["dv"] = max(worst["dv"], ratio(gr[:, 128 + 4 * h:128 + 4 * h + 4], P.t() @ go, (P * (eP + unit)).t() @ go.abs()))
            del s, P, dS, A
    return worst, intact


@pytest.mark.parametrize("case", ["C4_B16_L4096_default", "C4_B16_L4096_hilo", "B16_L100_valu"])
def test_training_attention_matches_fp64(G, case):
    """gsdd_d3pm_attention_train (out + lse) and gsdd_d3pm_attention_bwd (default variant: fused matrix-pipe kernel + dQ reduction)
    at the C4 training shape B = 16, L = 4096, H = 16: 16 x 16 x 4096 x 4096 = 2^32 (batch, head, query, key) products and the largest
    dq_part workspace.  The default forward is the adaptive one at this length (documented 2e-5 bound), "22" the hi + lo one (derived
    bar); B = 16 at L = 100 runs the VALU kernels (L % 32 != 0)."""
    B, H = 16, 16
    L = 100 if case == "B16_L100_valu" else 4096
    mode = "22" if case.endswith("hilo") else None
    worst, intact = attention_case(G, B, L, H, 77 + L, mode, documented_fwd=case.endswith("default"))
    parity_report(f"train_kernels::attention[{case}]", {**{k + "_ratio": v for k, v in worst.items()}, "worst_ratio": max(worst.values())})
    assert intact, "attention forward wrote past its outputs"
    assert max(worst.values()) <= 1, worst


# ----------------------------------------------------------------------------- Adam
ADAM_SIZES = [1, 3, 4095, 4096, 4097, 3 * 4096 + 5]


@pytest.mark.parametrize("dev_step", [False, True], ids=["adam_multi", "adam_multi_dev"])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_multi_matches_fp64(G, step, dev_step):
    """_optim.MultiAdam (gsdd_adam_multi / gsdd_adam_multi_dev) over parameters whose sizes straddle ADAM_CHUNK = 4096, at steps 1, 2
    and 1000 from a nonzero state: p, m, v against the fp64 update of the same f32 inputs; the 4-float padding of m and v and the gaps
    between the parameters (views of one sentinel-filled buffer) are untouched."""
    from gsdd_amd._optim import MultiAdam
    g = cgen(step * 2 + int(dev_step))
    GAP = 7
    total = sum(n + GAP for n in ADAM_SIZES) + GAP
    pbuf = torch.full((total,), SENT, device="cuda")
    params, grads, poffs, off = [], {}, [], GAP
    for i, n in enumerate(ADAM_SIZES):
        poffs.append(off)
        p = pbuf[off:off + n]
        p.copy_(torch.randn(n, generator=g, device="cuda"))
        params.append((f"p{i}", p))
        gr = torch.randn(n, generator=g, device="cuda") * 1e-2
        gr[::11] = 0.0
        grads[f"p{i}"] = gr
        off += n + GAP
    lr, b1, b2, eps = 1e-3, 0.5, 0.999, 1e-8
    opt = MultiAdam(params, lr, (b1, b2), eps)
    pad = torch.ones_like(opt.m, dtype=torch.bool)
    for (_, p), o in zip(params, opt.offs[:-1]):
        pad[int(o):int(o) + p.numel()] = False
    opt.m.copy_(torch.randn(opt.m.shape, generator=g, device="cuda") * 1e-2)
    opt.v.copy_(torch.rand(opt.v.shape, generator=g, device="cuda") * 1e-4)
    opt.m[pad] = SENT
    opt.v[pad] = SENT
    p0, m0, v0 = pbuf.clone(), opt.m.clone(), opt.v.clone()
    opt.step_count = step - 1
    if dev_step:
        opt.step(grads, step_dev=torch.tensor([step], dtype=torch.int64, device="cuda"))
    else:
        opt.step(grads)
    f32 = lambda z: float(np.float32(z))
    B1, B2, EPS = f32(b1), f32(b2), f32(eps)
    c1, c2 = 1 - B1 ** step, 1 - B2 ** step
    e_c1 = 4 * U * B1 ** step / c1 + U
    e_c2 = 4 * U * B2 ** step / c2 + U
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for (name, p), o, po in zip(params, opt.offs[:-1], poffs):
        n = p.numel()
        sl = slice(int(o), int(o) + n)
        gd, md, vd = grads[name].double(), m0[sl].double(), v0[sl].double()
        m1 = B1 * md + (1 - B1) * gd
        v1 = B2 * vd + (1 - B2) * gd * gd
        e_m = 2 * U * ((B1 * md).abs() + ((1 - B1) * gd).abs())
        e_v = 3 * U * v1
        sq = (v1 / c2).sqrt()
        den = sq + EPS
        dp = f32(lr) / c1 * m1 / den
        p1 = p0[po:po + n].double() - dp
        bar_p = f32(lr) / c1 * e_m / den + dp.abs() * (e_c1 + (e_v / v1.clamp(min=1e-300) + e_c2) / 2 * (sq / den) + 8 * U) + U * p1.abs()
        worst["m"] = max(worst["m"], ratio(opt.m[sl], m1, e_m + 2.0 ** -149))
        worst["v"] = max(worst["v"], ratio(opt.v[sl], v1, e_v + 2.0 ** -149))
        worst["p"] = max(worst["p"], ratio(p, p1, bar_p + 2.0 ** -149))
    pad_ok = bool(torch.equal(opt.m[pad], m0[pad])) and bool(torch.equal(opt.v[pad], v0[pad]))
    gap_mask = torch.ones(total, dtype=torch.bool, device="cuda")
    for po, n in zip(poffs, ADAM_SIZES):
        gap_mask[po:po + n] = False
    gaps_ok = bool(torch.equal(pbuf[gap_mask], p0[gap_mask]))
    parity_report(f"train_kernels::adam[{'dev' if dev_step else 'host'}_step{step}]",
                  {**{k + "_ratio": v for k, v in worst.items()}, "worst_ratio": max(worst.values())})
    assert pad_ok, "Adam wrote the padding of m / v"
    assert gaps_ok, "Adam wrote outside its parameters"
    assert max(worst.values()) <= 1, worst
