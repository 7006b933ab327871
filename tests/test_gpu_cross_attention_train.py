"""gsdd_d3pm_cross_attention_train (out + lse) and gsdd_d3pm_cross_attention_bwd (dq, dkc, dvc) -- the cross-attention of the training
step over Te > 1 condition tokens -- against a plain fp64 evaluation on the device, element by element, in the style of
tests/test_gpu_train_kernels.py (whose U, gam, C_ATT and ratio are used here).

Layouts: q and dq head-major [H][M][4] (M = B L), kc / vc / dkc / dvc rows [B Te][4 H], out / dO rows [M][4 H], lse [H][M] in the log2
domain, scores q.k / 2.

Cases (B, L, Te, H): a cross-section of Te in {1, 2, 15, 16, 17, 22, 33, 77}, L in {1, 37, 64, 257} with B = 3 (the backward sums dkc /
dvc in chunks of 64 rows per batch element and its other kernels run 256 lanes of (row, head) pairs per block: blocks straddle batch
elements, the last chunk is partial, L = 1 has one row per batch element) and H in {1, 2, 16}; and the training shape B = 16, L = 4096,
H = 16, Te = 22 (23 M scores).

Inputs: every (batch, head) has a temperature of its own, from near-uniform rows to rows one key dominates; the last row of the last
(batch, head) is scaled so that its largest |score| is 40.5; the first row of the first (batch, head) has q = 0 (all scores equal).

Bars, per output element, derived from the kernels' arithmetic (U = 2^-24, gamma(k) = U (8 + 2 sqrt(k)); |.| of the exact values;
c = log2(e) / 2 = C_ATT).  The kernels are plain f32 on the vector ALU: q is scaled by c (1 rounding), a score is a 4-term fma chain,
the exponent is s - max (or s - lse) through exp2 (<= 2 ulp), and every sum over the Te keys of a row is a chain of Te f32 fmas.
  * unit on the sums over keys: uk = gamma(Te) + 8 U; a score and its exp2 carry sc = 8 U c max_j sum_f |q_f k_jf| relative to P.
    out: (uk + sc) sum_j P_j |v_jf|.
    lse: sc + uk / ln 2 + 4 U (|lse| + 1)  (log2f and the final add).
  * the backward is fed the kernel's own out and lse, as the step does: P = exp2(s - lse) carries eP = ln 2 bar_lse relative to P;
    delta = dO . o carries Dd = sum_f |dO_f| bar_o_f + 4 U sum_f |dO_f o_f|; dP = dO . v carries 4 U |dP|.  With
    T_ij = P_ij (Dd_i + 4 U (|dP_ij| + |delta_i|)):
      dq  = 1/2 dS k    (sum over keys):            bar 1/2 (|dS| (eP + uk) + T) |k|
      dkc = 1/2 dS^T q  (sum over the L rows):      bar 1/2 (|dS| (eP + gamma(L)) + T)^T |q|
      dvc = P^T dO      (sum over the L rows):      bar (P (eP + gamma(L)))^T |dO|
    (the row sums are taken in chunks of 64 rows and the chunks then added in order: never more roundings than the plain chain gamma(L)
    stands for.)
Every case records its worst error / bar ratio with tests.conftest.parity_report (cross_train::*).

Further checks per case: the forward's out against gsdd_d3pm_cross_attention's (the sampler's kernel) within the out bar; dq, dkc and dvc
overwrite a nonzero prefill; the floats behind every output, and behind the stated size of the workspace, keep their sentinel bit for bit;
a second run gives identical bits; (small cases) B = 3 in one launch equals three B = 1 launches bit for bit."""
import math

import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_train_kernels import C_ATT, LN2, SENT, U, gam, ratio

pytestmark = pytest.mark.gpu

GUARD = 67
PREFILL = 123.25
SMALL = [(3, 1, 1, 1), (3, 37, 2, 2), (3, 64, 15, 16), (3, 257, 16, 1), (3, 37, 17, 16), (3, 64, 22, 2), (3, 257, 33, 16), (3, 1, 77, 16),
         (3, 257, 77, 2), (3, 37, 77, 1), (3, 257, 22, 16)]
CASES = SMALL + [(16, 4096, 22, 16)]
IDS = ["B%d_L%d_Te%d_H%d" % c for c in CASES]


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def make_inputs(B, L, Te, H):
    """-> q[H][B L][4], kc[B Te][4 H], vc[B Te][4 H], dO[B L][4 H] (f32, on the device)"""
    g = torch.Generator(device="cuda").manual_seed(100000 * B + 1000 * L + 10 * Te + H)
    q = torch.randn(H, B, L, 4, generator=g, device="cuda")
    k = torch.randn(B, Te, H, 4, generator=g, device="cuda")
    v = torch.randn(B, Te, H, 4, generator=g, device="cuda")
    dO = torch.randn(B * L, 4 * H, generator=g, device="cuda")
    temp = torch.logspace(-0.5, 0.5, B * H, device="cuda").view(B, H)   # largest probability of a row from about 1 / Te to about 1
    q = q * temp.t().reshape(H, B, 1, 1)
    k = k * temp.view(B, 1, H, 1)
    s = (k[B - 1, :, H - 1].double() @ q[H - 1, B - 1, L - 1].double()) * 0.5
    q[H - 1, B - 1, L - 1] *= float(40.5 / s.abs().max())              # one row whose scores reach 40 in size
    q[0, 0, 0] = 0.0                                                    # one row whose scores are all equal
    return q.reshape(H, B * L, 4).contiguous(), k.reshape(B * Te, 4 * H).contiguous(), v.reshape(B * Te, 4 * H).contiguous(), dO


def reference(q, kc, vc, dO, B, L, Te, H):
    """fp64 values and bars, every tensor as [B][H][rows][.]"""
    q64 = q.double().view(H, B, L, 4).permute(1, 0, 2, 3)
    k64 = kc.double().view(B, Te, H, 4).permute(0, 2, 1, 3)
    v64 = vc.double().view(B, Te, H, 4).permute(0, 2, 1, 3)
    g64 = dO.double().view(B, L, H, 4).permute(0, 2, 1, 3)
    s = (q64 @ k64.transpose(-1, -2)) * 0.5
    lse_n = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - lse_n)
    o = P @ v64
    uk = float(gam(Te)) + 8 * U
    ur = float(gam(L))
    sc = 8 * U * C_ATT * (q64.abs() @ k64.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    r = {"smax": float(s.abs().max()), "out": o, "bar_out": (uk + sc) * (P @ v64.abs())}
    lse2 = lse_n / LN2
    r["lse"], r["bar_lse"] = lse2, sc + uk / LN2 + 4 * U * (lse2.abs() + 1)
    dP = g64 @ v64.transpose(-1, -2)
    delta = (g64 * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    eP = LN2 * r["bar_lse"]
    Dd = (g64.abs() * r["bar_out"]).sum(-1, keepdim=True) + 4 * U * (g64 * o).abs().sum(-1, keepdim=True)
    T = P * (Dd + 4 * U * (dP.abs() + delta.abs()))
    r["dq"], r["bar_dq"] = 0.5 * dS @ k64, 0.5 * (dS.abs() * (eP + uk) + T) @ k64.abs()
    r["dk"], r["bar_dk"] = 0.5 * dS.transpose(-1, -2) @ q64, 0.5 * (dS.abs() * (eP + ur) + T).transpose(-1, -2) @ q64.abs()
    r["dv"], r["bar_dv"] = P.transpose(-1, -2) @ g64, (P * (eP + ur)).transpose(-1, -2) @ g64.abs()
    return r


def guarded(shape, fill):
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    buf[:n] = fill
    return buf, buf[:n].view(shape)


def intact(buf, n):
    return bool((buf[n:] == SENT).all())


def bits(x):
    return x.contiguous().view(torch.int32)


def run_pair(G, q, kc, vc, dO, B, L, Te, H):
    """forward + backward on guarded, prefilled buffers -> dict of outputs and the `intact` flags"""
    M = B * L
    obuf, out = guarded((M, 4 * H), SENT)
    lbuf, lse = guarded((H * M,), SENT)
    G.ops.d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, out, lse)
    nws = G.lib().gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H)
    assert nws > 0 and nws % 4 == 0
    wbuf, ws = guarded((nws // 4,), SENT)
    qbuf, dq = guarded((H, M, 4), PREFILL)
    kbuf, dkc = guarded((B * Te, 4 * H), PREFILL)
    vbuf, dvc = guarded((B * Te, 4 * H), -PREFILL)
    G.ops.d3pm_cross_attention_bwd(q, kc, vc, out, dO, lse, B, L, Te, H, ws, dq=dq, dkc=dkc, dvc=dvc)
    torch.cuda.synchronize()
    ok = {"out": intact(obuf, out.numel()), "lse": intact(lbuf, lse.numel()), "workspace": intact(wbuf, ws.numel()),
          "dq": intact(qbuf, dq.numel()), "dkc": intact(kbuf, dkc.numel()), "dvc": intact(vbuf, dvc.numel())}
    return {"out": out, "lse": lse, "dq": dq, "dkc": dkc, "dvc": dvc}, ok


@pytest.mark.parametrize("B,L,Te,H", CASES, ids=IDS)
def test_cross_attention_train_pair_matches_fp64(G, B, L, Te, H):
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    ref = reference(q, kc, vc, dO, B, L, Te, H)
    assert ref["smax"] >= 40, ref["smax"]
    M = B * L
    got, ok = run_pair(G, q, kc, vc, dO, B, L, Te, H)
    rows = lambda x: x.view(B, L, H, 4).permute(0, 2, 1, 3)             # [M][4 H] -> [B][H][L][4]
    cond = lambda x: x.view(B, Te, H, 4).permute(0, 2, 1, 3)            # [B Te][4 H] -> [B][H][Te][4]
    worst = {
        "out": ratio(rows(got["out"]), ref["out"], ref["bar_out"]),
        "lse": ratio(got["lse"].view(H, B, L).permute(1, 0, 2).unsqueeze(-1), ref["lse"], ref["bar_lse"]),
        "dq": ratio(got["dq"].view(H, B, L, 4).permute(1, 0, 2, 3), ref["dq"], ref["bar_dq"]),
        "dk": ratio(cond(got["dkc"]), ref["dk"], ref["bar_dk"]),
        "dv": ratio(cond(got["dvc"]), ref["dv"], ref["bar_dv"]),
    }
    # the sampler's kernel on the same inputs
    plain = torch.empty((M, 4 * H), dtype=torch.float32, device="cuda")
    G.ops.d3pm_cross_attention(q, kc, vc, B, L, Te, H, plain)
    worst["out_vs_sampler_kernel"] = ratio(rows(got["out"]), rows(plain).double(), ref["bar_out"])
    name = IDS[CASES.index((B, L, Te, H))]
    print(name, worst)
    parity_report(f"cross_train::{name}", {**{k + "_ratio": v for k, v in worst.items()}, "worst_ratio": max(worst.values()),
                                           "max_abs_score": ref["smax"]})
    assert all(ok.values()), f"written outside an output or behind the workspace's stated size: {ok}"
    assert max(worst.values()) <= 1, worst
    if Te == 1:
        rep = vc.view(B, 1, 4 * H).expand(B, L, 4 * H).reshape(M, 4 * H)
        assert torch.equal(bits(got["out"]), bits(rep)), "Te = 1: the output is not the value row"
    # the same inputs give the same bits
    again, ok2 = run_pair(G, q, kc, vc, dO, B, L, Te, H)
    assert all(ok2.values()), ok2
    for k_ in got:
        assert torch.equal(bits(got[k_]), bits(again[k_])), f"{k_}: two runs differ"


@pytest.mark.parametrize("B,L,Te,H", SMALL, ids=IDS[:len(SMALL)])
def test_batch_elements_do_not_depend_on_the_launch(G, B, L, Te, H):
    """B = 3 in one launch equals three B = 1 launches, bit for bit: no sum may mix, or be ordered by, the other batch elements."""
    q, kc, vc, dO = make_inputs(B, L, Te, H)
    M = B * L
    got, _ = run_pair(G, q, kc, vc, dO, B, L, Te, H)
    for b in range(B):
        r = slice(b * L, (b + 1) * L)
        e = slice(b * Te, (b + 1) * Te)
        one, ok = run_pair(G, q[:, r].contiguous(), kc[e].contiguous(), vc[e].contiguous(), dO[r].contiguous(), 1, L, Te, H)
        assert all(ok.values()), ok
        assert torch.equal(bits(got["out"][r]), bits(one["out"])), b
        assert torch.equal(bits(got["lse"].view(H, M)[:, r]), bits(one["lse"].view(H, L))), b
        assert torch.equal(bits(got["dq"][:, r]), bits(one["dq"])), b
        assert torch.equal(bits(got["dkc"][e]), bits(one["dkc"])), b
        assert torch.equal(bits(got["dvc"][e]), bits(one["dvc"])), b
