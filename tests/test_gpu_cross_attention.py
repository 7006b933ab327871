"""gsdd_d3pm_cross_attention -- the denoiser's general condition path (more than one condition token: one thread per (row, head), head-major
q[H][B L][4] against row-major kc / vc[B Te][4 H], softmax(q k^T / 2) v) -- against fp64 per batch element and head, and the way
Text2ImageTransformer._run_blocks_unfused strings that path together (the lazily made ln1_1 table, q2 in qkv[0:H]) against the Te = 1
fixture and against the CPU oracle.

Kernel cases (B, L, Te, H): B L H mostly no multiple of the 256-thread block, batch boundaries inside a block, Te = 1, 2, 3, 76, 77.  Keys and
values are independent per batch element; every (batch, head) has a temperature of its own, from near-uniform rows to rows that one key
dominates, and the last (batch, head) has scores of about +-60, where the maximum subtraction matters.  Bar, per output element: the one
tests/test_gpu_train_kernels.py::attention_case applies to the VALU forward, (gamma(Te) + 8 U (1 + C_ATT max_j sum_f |q_f k_jf|)) sum_j P_j
|v_jf| with that file's gam, U and C_ATT.  At Te = 1 the output is the value row bit for bit (expf(0) = 1, 1 / 1 = 1).  q, kc and vc are
views of buffers whose rows behind the valid range are NaN and out has sentinel rows behind B L: the output is finite and the sentinels
stay.  Every case records its worst error / bar ratio with tests.conftest.parity_report (cross_attention::*).

Denoiser (d3pm_L64 fixture): a condition token repeated 2 or 77 times gives a uniform softmax over identical keys, so the general path must
reproduce the fixture's Te = 1 logits within LOGIT_TOL -- on one model (the ln1_1 tables are made on the first use, with Te = 2, and reused
with Te = 77) and on a model built for each call; random conditions of 2 and 77 tokens, different per batch element and scaled so that the
attention is neither flat nor one-hot, agree with oracle.d3pm.denoiser on the same state dict within LOGIT_TOL.

The unmarked tests need no GPU: a plain f32 torch restatement of the kernel meets the bar on every case, and misses it with the head-major q
read row-major, the per-batch key offset dropped, or the maximum subtraction left out."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden, parity_report
from tests.test_gpu_parity import LOGIT_TOL, build_d3pm
from tests.test_gpu_train_kernels import C_ATT, U, gam

gpu = pytest.mark.gpu

POISON = -7777.0
PAD = 19
CASES = [(1, 1, 1, 1), (3, 37, 2, 3), (2, 300, 3, 16), (3, 37, 76, 16), (1, 256, 77, 16), (2, 64, 77, 1)]
IDS = ["B%d_L%d_Te%d_H%d" % c for c in CASES]


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def make_inputs(B, L, Te, H):
    """-> q[H][B L][4], kc[B Te][4 H], vc[B Te][4 H] (f32, CPU)"""
    g = torch.Generator().manual_seed(100000 * B + 1000 * L + 10 * Te + H)
    q = torch.randn(H, B, L, 4, generator=g)
    k = torch.randn(B, Te, H, 4, generator=g)
    v = torch.randn(B, Te, H, 4, generator=g)
    temp = torch.logspace(-0.5, 0.5, B * H).view(B, H).clone()        # largest probability of a row from about 1 / Te to about 1
    temp[B - 1, H - 1] = math.sqrt(60.0)                              # scores q.k / 2 of about +-60
    q = q * temp.t().reshape(H, B, 1, 1)
    k = k * temp.view(B, 1, H, 1)
    return q.reshape(H, B * L, 4).contiguous(), k.reshape(B * Te, 4 * H).contiguous(), v.reshape(B * Te, 4 * H).contiguous()


def reference(q, kc, vc, B, L, Te, H):
    """fp64 softmax(q k^T / 2) v per (batch, head) -> out[B L][4 H], bar[B L][4 H], the largest |score|"""
    q64 = q.double().view(H, B, L, 4).permute(1, 0, 2, 3)             # [B][H][L][4]
    k64 = kc.double().view(B, Te, H, 4).permute(0, 2, 1, 3)           # [B][H][Te][4]
    v64 = vc.double().view(B, Te, H, 4).permute(0, 2, 1, 3)
    s = (q64 @ k64.transpose(-1, -2)) * 0.5
    P = torch.softmax(s, -1)
    o = P @ v64
    amax = (q64.abs() @ k64.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    bar = (float(gam(Te)) + 8 * U * (1 + C_ATT * amax)) * (P @ v64.abs())
    rows = lambda x: x.permute(0, 2, 1, 3).reshape(B * L, 4 * H)
    return rows(o), rows(bar), float(s.abs().max())


def worst_ratio(got, want, bar):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    return float(torch.where(err == 0, 0.0, err / bar).max())


# ----------------------------------------------------------------------------- the kernel
@gpu
@pytest.mark.parametrize("B,L,Te,H", CASES, ids=IDS)
def test_cross_attention_matches_fp64(G, B, L, Te, H):
    q, kc, vc = make_inputs(B, L, Te, H)
    want, bar, smax = reference(q, kc, vc, B, L, Te, H)
    M = B * L
    qbuf = torch.full((H * M + PAD, 4), math.nan, device="cuda")
    kbuf = torch.full((B * Te + PAD, 4 * H), math.nan, device="cuda")
    vbuf = torch.full((B * Te + PAD, 4 * H), math.nan, device="cuda")
    obuf = torch.full((M + PAD, 4 * H), POISON, device="cuda")
    qbuf[:H * M] = q.view(H * M, 4).cuda()
    kbuf[:B * Te], vbuf[:B * Te] = kc.cuda(), vc.cuda()
    G.ops.d3pm_cross_attention(qbuf[:H * M].view(H, M, 4), kbuf[:B * Te], vbuf[:B * Te], B, L, Te, H, obuf[:M])
    torch.cuda.synchronize()
    got = obuf.cpu()
    r = worst_ratio(got[:M], want, bar)
    parity_report(f"cross_attention::{IDS[CASES.index((B, L, Te, H))]}", {"worst_ratio": r, "max_abs_score": smax,
                                                                        "max_err": float((got[:M].double() - want).abs().max())})
    assert torch.equal(got[M:], torch.full((PAD, 4 * H), POISON)), "rows behind B L were written"
    assert bool(torch.isfinite(got[:M]).all()), "rows behind the valid range of q, kc or vc were read"
    assert r <= 1, r
    if Te == 1:
        rep = vc.view(B, 1, 4 * H).expand(B, L, 4 * H).reshape(M, 4 * H)
        assert torch.equal(got[:M].view(torch.int32), rep.contiguous().view(torch.int32)), "Te = 1: the output is not the value row"


# ----------------------------------------------------------------------------- the denoiser's general path
def fixture():
    sd, a, cfg = load_golden("d3pm_L64")
    return sd, cfg, torch.from_numpy(a["step_xt"]), torch.from_numpy(a["step_cond"]), torch.from_numpy(a["step_t"]), torch.from_numpy(a["step_logits"])


@gpu
def test_repeated_condition_token_reproduces_one_token(G):
    sd, cfg, xt, cond, t, want = fixture()
    assert cond.shape[1] == 1
    xt, cond, t = xt.cuda(), cond.cuda(), t.cuda()
    rec = {}
    dm = build_d3pm(G, sd, cfg)
    layers = dm.transformer.packed()["layers"]
    assert all("ada2" not in lay for lay in layers)                   # made on first use of the general path
    tables = None
    for Te in (2, 77):
        got = dm.transformer(xt, cond.repeat(1, Te, 1), t).cpu()
        rec[f"one_model_Te{Te}"] = float((got - want).abs().max())
        now = [lay["ada2"] for lay in dm.transformer.packed()["layers"]]
        assert tables is None or all(x is y for x, y in zip(now, tables)), "the ln1_1 tables were made again"
        tables = now
    for Te in (77, 2):
        got = build_d3pm(G, sd, cfg).transformer(xt, cond.repeat(1, Te, 1), t).cpu()
        rec[f"fresh_model_Te{Te}"] = float((got - want).abs().max())
    one = dm.transformer(xt, cond, t).cpu()                           # the fused Te = 1 path on the model that holds the tables
    rec["one_model_Te1_after"] = float((one - want).abs().max())
    parity_report("cross_attention::denoiser_repeated_token", rec)
    assert max(rec.values()) <= LOGIT_TOL, rec


def cross_attention_pmax(tok, cond, t, sd, n_head=16):
    """largest probability of every (batch, head, position) row of block 0's cross-attention, from the oracle's own pieces"""
    from oracle import d3pm as od
    p = "transformer.blocks.0."
    x = od.content_emb(tok, sd)
    h = od.ada_layer_norm(x, t, sd, p + "ln1.")
    x = x + od.mha(h, h, sd, p + "attn1.", n_head)
    hq = od.ada_layer_norm(x, t, sd, p + "ln1_1.")
    B, Te = cond.shape[:2]
    q = F.linear(hq, sd[p + "attn2.query.weight"], sd[p + "attn2.query.bias"]).view(B, -1, n_head, 4).transpose(1, 2)
    k = F.linear(cond, sd[p + "attn2.key.weight"], sd[p + "attn2.key.bias"]).view(B, Te, n_head, 4).transpose(1, 2)
    return torch.softmax((q @ k.transpose(-2, -1)) * 0.5, -1).amax(-1)


def random_condition(Te, B, cond_dim):
    """different tokens per batch element; the scale (1 at Te = 2, 3 at Te = 77) puts the median row maximum of block 0's cross-attention
    between 0.5 and 0.95: neither flat nor one-hot (test_cpu_random_conditions_are_not_flat)"""
    g = torch.Generator().manual_seed(100 + Te)
    return (1.0 if Te == 2 else 3.0) * torch.randn(B, Te, cond_dim, generator=g)


@gpu
def test_general_path_matches_oracle(G):
    from oracle import d3pm as od
    sd, cfg, xt, cond, t, _ = fixture()
    dm = build_d3pm(G, sd, cfg)
    rec = {}
    for Te in (2, 77):
        cr = random_condition(Te, xt.shape[0], cond.shape[2])
        want = od.denoiser(xt, cr, t, sd)
        got = dm.transformer(xt.cuda(), cr.cuda(), t.cuda()).cpu()
        assert got.shape == want.shape
        rec[f"Te{Te}"] = float((got - want).abs().max())
    parity_report("cross_attention::denoiser_vs_oracle", rec)
    assert max(rec.values()) <= LOGIT_TOL, rec


# ----------------------------------------------------------------------------- no GPU
def test_cpu_random_conditions_are_not_flat():
    sd, cfg, xt, cond, t, _ = fixture()
    for Te in (2, 77):
        cr = random_condition(Te, xt.shape[0], cond.shape[2])
        assert not torch.equal(cr[0], cr[1])
        med = float(cross_attention_pmax(xt, cr, t, sd).median())
        assert 0.5 <= med <= 0.95, (Te, med)


def f32_restatement(q, kc, vc, B, L, Te, H, fault=None):
    """the kernel's arithmetic in plain f32 torch; `fault`: one of the indexing or softmax errors the kernel could make"""
    M = B * L
    if fault == "q_row_major":
        qh = q.reshape(M, H, 4).view(B, L, H, 4).permute(0, 2, 1, 3)
    else:
        qh = q.view(H, B, L, 4).permute(1, 0, 2, 3)
    kh = kc.view(B, Te, H, 4).permute(0, 2, 1, 3)
    vh = vc.view(B, Te, H, 4).permute(0, 2, 1, 3)
    if fault == "no_batch_offset":
        kh, vh = kh[:1].expand_as(kh), vh[:1].expand_as(vh)
    s = (qh @ kh.transpose(-1, -2)) * 0.5
    mx = torch.zeros_like(s[..., :1]) if fault == "no_max_subtraction" else s.amax(-1, keepdim=True)
    p = torch.exp(s - mx)
    o = (p @ vh) * (1.0 / p.sum(-1, keepdim=True))
    return o.permute(0, 2, 1, 3).reshape(M, 4 * H)


@pytest.mark.parametrize("B,L,Te,H", CASES, ids=IDS)
def test_cpu_f32_restatement_meets_bar(B, L, Te, H):
    q, kc, vc = make_inputs(B, L, Te, H)
    want, bar, smax = reference(q, kc, vc, B, L, Te, H)
    assert worst_ratio(f32_restatement(q, kc, vc, B, L, Te, H), want, bar) <= 1
    if (B, H) != (1, 1):
        assert smax > 40                                              # the large-score head is there


@pytest.mark.parametrize("fault,case", [("q_row_major", (3, 37, 2, 3)), ("q_row_major", (1, 256, 77, 16)), ("no_batch_offset", (2, 300, 3, 16)),
                                        ("no_batch_offset", (2, 64, 77, 1)), ("no_max_subtraction", (3, 37, 76, 16))])
def test_cpu_injected_fault_misses_bar(fault, case):
    q, kc, vc = make_inputs(*case)
    want, bar, _ = reference(q, kc, vc, *case)
    assert worst_ratio(f32_restatement(q, kc, vc, *case, fault=fault), want, bar) > 1
