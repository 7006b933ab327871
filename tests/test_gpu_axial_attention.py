"""gsdd_axial_attention / gsdd_axial_attention_bwd -- the VQ-VAE's axial attention: the register-resident MFMA pair (16-position lines at
head width 64 / 128, four (line, head) per block) and the LDS pair (any other line, one wave per (line, head)) -- against the written-out
fp64 forward and backward of tests/test_gpu_vqvae_training.py::_axial_reference_with_bars, element by element against its bars, at the line
lengths and head widths where the kernels' index arithmetic changes (CASES: what each one reaches).

Inputs, seeded per (case, kind): "plain" qkv = 0.7 randn, "peaked" qkv = randn with q and k scaled by 2 (scores of standard deviation 4);
datt = randn.  Every case with a 16-long axis runs both variants: "auto" (MFMA where the shape allows) and "valu" (the LDS kernels on
every axis).

GPU tests: (1) worst error / bar <= 1 on out and dqkv, an unwritten or non-finite element counts as infinite, a zero bar asks for
equality; (2) out and dqkv sit inside sentinel-guarded buffers prefilled with NaN: guards intact bit for bit, no NaN left, qkv and datt
unchanged; (3) a second run gives the same bits; (4) the call with all batch elements equals the per-element calls, and the call on the
grid with H and W exchanged equals the original, permuted back, bit for bit; (5) on an axis of length 1 out == v, dq == dk == 0 and
dv == datt bit for bit; (6) one NaN in q changes nothing outside its (line, head, axis) and makes out of its query NaN; (7) shapes
outside the contract of include/gsdd.h are refused by both entry points alike, before anything is written.

The unmarked tests need no GPU: a float32 restatement of the LDS kernels in their own order of operations (explicit line addressing, fma
chains over e and j, exp, one reciprocal per row) meets every bar at every case (the bars are not below f32's own noise); that restatement
with one fault injected at a time lands above a bar on the cases named in FAULT_CASES (the cases make each fault observable); the LDS-byte
formulas and the accepted set of the library's own rule (gsdd_axial_attention_lds_bytes) over all S <= 64.

Every run records its worst ratios with tests.conftest.parity_report (axial::<id>[kind,variant]; variant f32_restatement for the CPU one)."""
import functools
import math
import types

import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_vqvae_training import _axial_reference_with_bars

gpu = pytest.mark.gpu

SENT = -7777.0
GUARD = 256                                                  # floats on either side (a multiple of 4: the MFMA kernels store float4)
LDS_CAP = 160 * 1024


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def case(cid, dims, C, heads):
    return types.SimpleNamespace(id=cid, dims=dims, C=C, heads=heads, d=C // heads, M=dims[0] * dims[1] * dims[2] * dims[3])


CASES = {c.id: c for c in [
    case("ref_1_16_16", (1, 16, 8, 8), 256, 2),              # the reference's default grid: T on MFMA d = 128, H / W on the LDS kernels at S = 8
    case("ref_2_8_8", (1, 8, 16, 16), 256, 2),               # its generator config: T on the LDS kernels, H / W on MFMA
    case("lat32", (1, 4, 32, 32), 256, 2),                   # S = 32 at d = 128: 74,240 B in the backward
    case("s64_d32", (1, 64, 1, 2), 64, 2),                   # S = 64, 1, 2; 66,560 B in the backward
    case("s64_d8", (1, 2, 63, 64), 8, 1),                    # S = 63 and 64, one head, several softmax rows per lane
    case("s31_d128", (1, 31, 2, 1), 256, 2),                 # odd S at d = 128: 71,672 B in the backward
    case("odd", (1, 17, 33, 2), 40, 2),                      # S = 17 and 33, d = 20, T != H != W
    case("tiny", (2, 1, 3, 5), 12, 3),                       # S = 1, 3, 5; d = 4; three heads; two batch elements
    case("mfma_tail9", (1, 16, 3, 1), 192, 3),               # MFMA d = 64 with nwork = 9: the last block holds one wave
    case("mfma_tail2", (1, 16, 1, 1), 128, 2),               # MFMA d = 64 with nwork = 2
    case("n3", (3, 16, 16, 16), 128, 2),                     # MFMA d = 64, three batch elements
    case("s63_d128", (1, 63, 1, 1), 256, 2),                 # the longest line the rule admits at d = 128: 161,784 B of the 163,840
]}
KINDS = ("plain", "peaked")
HAS_16 = [cid for cid, c in CASES.items() if 16 in c.dims[1:]]
# (case, kind, valu): every case in the default variant, those with a 16-long axis also with the LDS kernels on every axis
RUNS = [(cid, kind, False) for cid in CASES for kind in KINDS] + [(cid, kind, True) for cid in HAS_16 for kind in KINDS]
RUN_IDS = [f"{cid}-{kind}-{'valu' if valu else 'auto'}" for cid, kind, valu in RUNS]


def lds_bytes(S, d, backward):
    """dynamic LDS of the LDS kernels per (line, head): q, k, v (and dO) as [S][d + 1] floats, one (two) [S][S] score images"""
    return (4 * S * (d + 1) + 2 * S * S) * 4 if backward else (3 * S * (d + 1) + S * S) * 4


def accepted(S, d):
    """the one rule of both entry points (include/gsdd.h): 1 <= S <= 64 and the backward image within a workgroup's 160 KiB"""
    return 1 <= S <= 64 and lds_bytes(S, d, True) <= LDS_CAP


@functools.lru_cache(maxsize=None)
def reference(cid, kind):
    """inputs and fp64 reference with bars of one (case, kind), made once on the CPU and shared by every test (nothing writes them)"""
    c = CASES[cid]
    g = torch.Generator().manual_seed(7919 * list(CASES).index(cid) + KINDS.index(kind))
    if kind == "plain":
        qkv = 0.7 * torch.randn(c.M, 9 * c.C, generator=g)
    else:
        qkv = torch.randn(c.M, 9 * c.C, generator=g)
        qkv.view(c.M, 3, 3, c.C)[:, :, :2, :] *= 2.0
    datt = torch.randn(c.M, 3 * c.C, generator=g)
    want_o, bar_o, want_g, bar_g, _ = _axial_reference_with_bars(qkv, datt, c.dims, c.C, c.heads)
    return types.SimpleNamespace(c=c, qkv=qkv, datt=datt, want_o=want_o, bar_o=bar_o, want_g=want_g, bar_g=bar_g)


def worst_ratio(got, want, bar):
    """max over elements of |got - want| / bar; a zero bar asks for equality; an unwritten (NaN) or non-finite element is infinite"""
    got = got.double()
    err = (got - want).abs()
    r = torch.where(bar > 0, err / bar, torch.where(err == 0, 0.0, math.inf))
    return float(torch.where(torch.isfinite(got), r, math.inf).max())


def judge(ref, out, dqkv):
    return worst_ratio(out, ref.want_o, ref.bar_o), worst_ratio(dqkv, ref.want_g, ref.bar_g)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- GPU plumbing
def guarded(M, width):
    """-> (whole buffer, its [M][width] body prefilled with NaN); GUARD sentinel floats on either side"""
    buf = torch.full((2 * GUARD + M * width,), SENT, device="cuda")
    body = buf[GUARD:GUARD + M * width].view(M, width)
    body.fill_(math.nan)
    return buf, body


def guards_intact(buf):
    want = torch.full((GUARD,), SENT, device=buf.device)
    return bits_equal(buf[:GUARD], want) and bits_equal(buf[-GUARD:], want)


def run_pair(G, qkv, datt, dims, C, heads, valu):
    """forward and backward into guarded NaN-prefilled buffers -> (out, dqkv) on the CPU, guards intact"""
    M = qkv.shape[0]
    obuf, out = guarded(M, 3 * C)
    gbuf, dqkv = guarded(M, 9 * C)
    G.ops.axial_attention(qkv, dims, C, heads, out, valu=valu)
    G.ops.axial_attention_bwd(qkv, datt, dims, C, heads, valu=valu, out=dqkv)
    torch.cuda.synchronize()
    return out.cpu(), dqkv.cpu(), guards_intact(obuf) and guards_intact(gbuf)


_gpu_runs = {}


def gpu_run(G, cid, kind, valu):
    """one (case, kind, variant) through both kernels, twice; run once and shared by tests 1 - 6 (nothing writes the results)"""
    key = (cid, kind, valu)
    if key not in _gpu_runs:
        ref = reference(cid, kind)
        c = ref.c
        qkv, datt = ref.qkv.cuda(), ref.datt.cuda()
        out, dqkv, intact = run_pair(G, qkv, datt, c.dims, c.C, c.heads, valu)
        out2, dqkv2, intact2 = run_pair(G, qkv, datt, c.dims, c.C, c.heads, valu)
        _gpu_runs[key] = types.SimpleNamespace(out=out, dqkv=dqkv, out2=out2, dqkv2=dqkv2, intact=intact and intact2,
                                               inputs_kept=bits_equal(qkv.cpu(), ref.qkv) and bits_equal(datt.cpu(), ref.datt))
    return _gpu_runs[key]


# ----------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize("cid,kind,valu", RUNS, ids=RUN_IDS)
def test_elementwise_vs_fp64(G, cid, kind, valu):
    """(1) every element of out and dqkv within its bar"""
    ref, r = reference(cid, kind), gpu_run(G, cid, kind, valu)
    r_o, r_g = judge(ref, r.out, r.dqkv)
    parity_report(f"axial::{cid}[{kind},{'valu' if valu else 'auto'}]", {"out_ratio": r_o, "dqkv_ratio": r_g, "worst_ratio": max(r_o, r_g)})
    assert r_o <= 1 and r_g <= 1, (r_o, r_g)


@gpu
@pytest.mark.parametrize("cid,kind,valu", RUNS, ids=RUN_IDS)
def test_nothing_outside_nothing_missing(G, cid, kind, valu):
    """(2) guards intact, no element of the NaN-prefilled outputs left unwritten, inputs unchanged"""
    r = gpu_run(G, cid, kind, valu)
    assert r.intact, "a guard float beside out or dqkv was written"
    assert not bool(torch.isnan(r.out).any()) and not bool(torch.isnan(r.dqkv).any()), "an element was left unwritten"
    assert r.inputs_kept, "qkv or datt changed"


@gpu
@pytest.mark.parametrize("cid,kind,valu", RUNS, ids=RUN_IDS)
def test_second_run_same_bits(G, cid, kind, valu):
    """(3) no atomics in these kernels"""
    r = gpu_run(G, cid, kind, valu)
    assert bits_equal(r.out, r.out2) and bits_equal(r.dqkv, r.dqkv2)


@gpu
@pytest.mark.parametrize("cid,valu", [("tiny", False), ("n3", False), ("n3", True)], ids=["tiny-auto", "n3-auto", "n3-valu"])
def test_batch_elements_do_not_see_each_other(G, cid, valu):
    """(4) the call with all batch elements == the per-element calls, bit for bit"""
    ref, r = reference(cid, "plain"), gpu_run(G, cid, "plain", valu)
    c = ref.c
    P = c.M // c.dims[0]
    for n in range(c.dims[0]):
        qkv, datt = ref.qkv[n * P:(n + 1) * P].cuda(), ref.datt[n * P:(n + 1) * P].cuda()
        out, dqkv, intact = run_pair(G, qkv, datt, (1,) + c.dims[1:], c.C, c.heads, valu)
        assert intact
        assert bits_equal(out, r.out[n * P:(n + 1) * P]) and bits_equal(dqkv, r.dqkv[n * P:(n + 1) * P]), n


def transpose_hw(x, dims, per_axis):
    """rows [pos][axis (w, h, t)][per_axis] of the grid (N, T, H, W) -> the same data on the grid (N, T, W, H): positions permuted and the
    w and h blocks of every row exchanged (its own inverse, with dims transposed)"""
    N, T, H, W = dims
    v = x.view(N, T, H, W, 3, per_axis).permute(0, 1, 3, 2, 4, 5)[:, :, :, :, [1, 0, 2], :]
    return v.reshape(N * T * H * W, 3 * per_axis).contiguous()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_transposed_grid_same_bits(G, kind):
    """(4) `odd` on the LDS kernels: with H and W exchanged every line runs the same arithmetic at other addresses"""
    ref = reference("odd", kind)
    c = ref.c
    N, T, H, W = c.dims
    tdims = (N, T, W, H)
    base_out, base_dqkv, intact = run_pair(G, ref.qkv.cuda(), ref.datt.cuda(), c.dims, c.C, c.heads, True)
    out, dqkv, intact_t = run_pair(G, transpose_hw(ref.qkv, c.dims, 3 * c.C).cuda(), transpose_hw(ref.datt, c.dims, c.C).cuda(), tdims, c.C,
                                   c.heads, True)
    assert intact and intact_t
    assert bits_equal(transpose_hw(out, tdims, c.C), base_out) and bits_equal(transpose_hw(dqkv, tdims, 3 * c.C), base_dqkv)


@gpu
@pytest.mark.parametrize("cid,kind", [(cid, kind) for cid in ("tiny", "s64_d32") for kind in KINDS])
def test_length_one_axis_is_exact(G, cid, kind):
    """(5) one key: the probability is exactly 1, the score gradient exactly 0"""
    ref, r = reference(cid, kind), gpu_run(G, cid, kind, False)
    c = ref.c
    axes = [a for a, S in enumerate((c.dims[3], c.dims[2], c.dims[1])) if S == 1]
    assert axes
    for a in axes:
        qkv3, dq3 = ref.qkv.view(c.M, 3, 3, c.C)[:, a], r.dqkv.view(c.M, 3, 3, c.C)[:, a]
        assert bits_equal(r.out.view(c.M, 3, c.C)[:, a], qkv3[:, 2]), "out != v"
        assert bool((dq3[:, 0] == 0).all()) and bool((dq3[:, 1] == 0).all()), "dq or dk is not zero"
        assert bits_equal(dq3[:, 2], ref.datt.view(c.M, 3, c.C)[:, a]), "dv != datt"


@gpu
def test_nan_stays_in_its_line(G):
    """(6) `odd`, plain: one NaN in q at (t, h, w) = (5, 11, 1), the h axis, head 1"""
    ref, base = reference("odd", "plain"), gpu_run(G, "odd", "plain", False)
    c = ref.c
    N, T, H, W = c.dims
    t, h, w, axis, head, e = 5, 11, 1, 1, 1, 3
    p = (t * H + h) * W + w
    qkv = ref.qkv.clone()
    qkv[p, axis * 3 * c.C + head * c.d + e] = math.nan
    out, dqkv, intact = run_pair(G, qkv.cuda(), ref.datt.cuda(), c.dims, c.C, c.heads, False)
    assert intact
    rows = torch.zeros(N, T, H, W, dtype=torch.bool)
    rows[0, t, :, w] = True                                                          # the line along h through (t, h, w)
    in_out = torch.zeros(c.M, 3, c.heads, c.d, dtype=torch.bool)
    in_out[rows.view(-1), axis, head] = True
    in_dqkv = torch.zeros(c.M, 3, 3, c.heads, c.d, dtype=torch.bool)
    in_dqkv[rows.view(-1), axis, :, head] = True
    same_o = out.view(torch.int32) == base.out.view(torch.int32)
    same_g = dqkv.view(torch.int32) == base.dqkv.view(torch.int32)
    assert bool((same_o | in_out.view(c.M, -1)).all()), "out changed outside the (line, head, axis)"
    assert bool((same_g | in_dqkv.view(c.M, -1)).all()), "dqkv changed outside the (line, head, axis)"
    assert bool(torch.isnan(out.view(c.M, 3, c.heads, c.d)[p, axis, head]).all()), "out of the NaN query is not NaN"


# dims, C, heads, variant (an int goes to the C ABI as it is), what
REFUSALS = [
    ((1, 65, 2, 2), 8, 2, False, "an axis of 65"),
    ((1, 2, 65, 2), 8, 2, True, "an axis of 65"),
    ((1, 4, 3, 2), 10, 4, False, "C % n_head != 0"),
    ((2, 1, 3, 5), 12, 3, 5, "unknown variant"),
    ((1, 64, 16, 16), 256, 2, False, "S = 64 at d = 128 behind two axes the MFMA kernels would take"),
    ((1, 64, 16, 16), 256, 2, True, "S = 64 at d = 128 behind two axes that fit"),
    ((1, 38, 2, 2), 256, 1, False, "S = 38 at d = 256 behind two axes that fit"),
]


@gpu
@pytest.mark.parametrize("dims,C,heads,variant,what", REFUSALS, ids=[f"{r[0]}x{r[1]}h{r[2]}v{int(r[3])}".replace(" ", "") for r in REFUSALS])
def test_refused_before_any_launch(G, dims, C, heads, variant, what):
    """(7) GsddError from both entry points, for the same reason, with nothing written.  (The buffers have the full size of the shape.)"""
    M = dims[0] * dims[1] * dims[2] * dims[3]
    qkv, datt = torch.zeros(M, 9 * C, device="cuda"), torch.zeros(M, 3 * C, device="cuda")
    out, dqkv = torch.full((M, 3 * C), SENT, device="cuda"), torch.full((M, 9 * C), SENT, device="cuda")
    v = variant if isinstance(variant, bool) else None
    ops, L = G.ops, G.ops.lib()
    var = ops.axial_variant(v) if v is not None else variant
    with pytest.raises(G.GsddError) as ef:
        ops.check(L.gsdd_axial_attention(ops.ptr(qkv), *dims, C, heads, ops.ptr(out), var, ops.stream_ptr(None)))
    with pytest.raises(G.GsddError) as eb:
        ops.check(L.gsdd_axial_attention_bwd(ops.ptr(qkv), ops.ptr(datt), *dims, C, heads, ops.ptr(dqkv), var, ops.stream_ptr(None)))
    torch.cuda.synchronize()
    reason_f, reason_b = (str(e.value).split(": ", 2)[2] for e in (ef, eb))          # "gsdd error N: <function>: <reason>"
    assert reason_f == reason_b, (what, str(ef.value), str(eb.value))
    assert bool((out == SENT).all()) and bool((dqkv == SENT).all()), f"{what}: an output was written before the refusal"


# ----------------------------------------------------------------------------- no GPU: f32 restatement and injected faults
def fma(a, b, c):
    """float32 fused multiply-add: the product is exact in float64, the sum is rounded there once more before float32 (a double rounding
    that differs from the fused one on ~2^-29 of the operations, far below any bar)"""
    return (a.double() * b.double() + c.double()).float()


def line_positions(dims, axis, fault=None):
    """position index [line][s] of the LDS kernels' addressing: basepos + s * stride"""
    N, T, H, W = dims
    S = (W, H, T)[axis]
    line = torch.arange(N * T * H * W // S)
    if axis == 0:
        stride, base = 1, line * W
    elif axis == 1:
        m = H if fault == "axis1_base_with_H" else W
        stride, base = W, (line // m) * H * W + line % m
    else:
        stride = W if fault == "axis2_stride_W" else H * W
        base = (0 if fault == "no_batch_offset" else (line // (H * W)) * T * H * W) + line % (H * W)
    return base[:, None] + torch.arange(S)[None, :] * stride


def f32_restatement(ref, fault=None):
    """axial_attention_kernel and axial_attention_bwd_kernel in torch float32, in the kernels' own order: rows gathered through the line
    addressing, scores and dP as fma chains over e, the row sum and delta left to right, one reciprocal per row, P.V and dQ / dK / dV as
    fma chains over j, every element scattered through the same addressing into NaN-prefilled outputs.  With `fault`, one of the errors
    the kernels could make."""
    c = ref.c
    M, C, heads, d = c.M, c.C, c.heads, c.d
    out = torch.full((M, 3, heads, d), math.nan)
    dqkv = torch.full((M, 3, 3, heads, d), math.nan)
    scale = torch.tensor(float(C if fault == "scale_by_C" else d)).sqrt().reciprocal()
    for axis in range(3):
        idx = line_positions(c.dims, axis, fault)                                    # [lines][S]
        assert int(idx.min()) >= 0 and int(idx.max()) < M
        S = idx.shape[1]
        rows = ref.qkv[idx].view(-1, S, 3, 3, heads, d)[:, :, axis]                  # [lines][S][q|k|v][head][d]
        q, k, v = (rows[:, :, j].permute(0, 2, 1, 3) for j in range(3))              # [lines][head][S][d]
        g = ref.datt[idx].view(-1, S, 3, heads, d)[:, :, axis].permute(0, 2, 1, 3)
        if fault == "wrong_head_offset":                                             # k read at another head's columns
            k = k.roll(1, dims=1)
        s = torch.zeros(q.shape[:3] + (S,))
        dp = torch.zeros_like(s)
        for e in range(d):
            s = fma(q[..., :, None, e], k[..., None, :, e], s)
            dp = fma(g[..., :, None, e], v[..., None, :, e], dp)
        s = s * scale
        p_un = torch.exp(s - s.amax(-1, keepdim=True))
        nkeys = S - 1 if fault == "drop_last_key" and S > 1 else S
        l = torch.zeros(s.shape[:3])
        for j in range(nkeys):
            l = l + p_un[..., j]
        p = p_un * (1.0 / l)[..., None]
        o = torch.zeros_like(q)
        for j in range(nkeys):
            o = fma(p[..., :, j, None], v[..., j, None, :], o)
        pd = p_un if fault == "delta_unnormalised" else p
        rs = torch.zeros_like(l)
        for j in range(S):
            rs = rs + pd[..., j] * dp[..., j]
        ds = p * (dp - rs[..., None])
        if fault != "ds_without_scale":
            ds = ds * scale
        dst = ds if fault == "dk_without_transpose" else ds.transpose(-1, -2)
        pt = p.transpose(-1, -2)
        gq, gk, gv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        for j in range(S):
            gq = fma(ds[..., :, j, None], k[..., j, None, :], gq)
            gk = fma(dst[..., :, j, None], q[..., j, None, :], gk)
            gv = fma(pt[..., :, j, None], g[..., j, None, :], gv)
        flat = idx.reshape(-1)
        out[flat, axis] = o.permute(0, 2, 1, 3).reshape(-1, heads, d)
        for j, t in enumerate((gq, gk, gv)):
            dqkv[flat, axis, j] = t.permute(0, 2, 1, 3).reshape(-1, heads, d)
    return out.view(M, 3 * C), dqkv.view(M, 9 * C)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", list(CASES))
def test_cpu_f32_restatement_meets_the_bars(cid, kind):
    """(8) the bars are not below what plain f32 arithmetic in the kernels' order gives"""
    ref = reference(cid, kind)
    r_o, r_g = judge(ref, *f32_restatement(ref))
    parity_report(f"axial::{cid}[{kind},f32_restatement]", {"out_ratio": r_o, "dqkv_ratio": r_g, "worst_ratio": max(r_o, r_g)})
    assert r_o <= 1 and r_g <= 1, (r_o, r_g)


# which case makes which fault observable
FAULT_CASES = [("scale_by_C", cid) for cid in ("tiny", "odd", "s64_d32", "mfma_tail2", "ref_1_16_16")]
FAULT_CASES += [("drop_last_key", "odd"), ("wrong_head_offset", "tiny"), ("axis1_base_with_H", "odd"), ("axis2_stride_W", "odd")]
FAULT_CASES += [(f, cid) for f in ("delta_unnormalised", "dk_without_transpose", "ds_without_scale") for cid in ("tiny", "odd", "s64_d8", "mfma_tail2")]
FAULT_CASES += [("no_batch_offset", "tiny"), ("no_batch_offset", "n3")]


@pytest.mark.parametrize("fault,cid", FAULT_CASES)
def test_cpu_injected_fault_is_caught(fault, cid):
    """(9) the restatement with one fault lands above a bar (or leaves an element unwritten) in the named case"""
    ref = reference(cid, "plain")
    r_o, r_g = judge(ref, *f32_restatement(ref, fault))
    assert max(r_o, r_g) > 1, f"{fault} stays within every bar of {cid}: {r_o}, {r_g}"


def test_cpu_lds_bytes_and_accepted_set():
    """(10) the formulas, the figures quoted for them, and the library's own rule over every S <= 64 (and just past it)"""
    import gsdd_amd
    L = gsdd_amd.lib()
    assert lds_bytes(32, 128, False) == 53632 and lds_bytes(32, 128, True) == 74240
    assert lds_bytes(31, 128, True) == 71672 and lds_bytes(64, 32, True) == 66560 and lds_bytes(64, 64, True) == 99328
    for d in (4, 8, 20, 32, 64, 128):
        for S in range(0, 67):
            ok = 1 <= S <= 64 and (d <= 64 or S <= 63)       # the accepted set, written out
            assert accepted(S, d) == ok, (S, d)
            for backward in (0, 1):
                assert L.gsdd_axial_attention_lds_bytes(S, d, backward) == (lds_bytes(S, d, bool(backward)) if ok else -1), (S, d, backward)
            if ok:
                assert lds_bytes(S, d, False) <= lds_bytes(S, d, True) <= LDS_CAP
    # what the contract promises at the least, and its edge at wider heads
    assert all(accepted(S, d) for S in range(1, 65) for d in range(1, 65)) and all(accepted(S, 128) for S in range(1, 33))
    assert max(lds_bytes(S, d, True) for S in range(1, 65) for d in range(1, 65)) == 99328
    assert accepted(63, 128) and not accepted(64, 128) and accepted(37, 256) and not accepted(38, 256)
    assert L.gsdd_axial_attention_lds_bytes(37, 256, 1) == lds_bytes(37, 256, True) and L.gsdd_axial_attention_lds_bytes(38, 256, 1) == -1


def test_cpu_cases_reach_what_they_are_listed_for():
    """every case lies inside the accepted set; the MFMA tail cases leave the last block of four (line, head) partly filled; the cases
    the backward refused at 64 KiB are above it; several softmax rows per lane (S * S > 64 lanes) and more than one row block"""
    for c in CASES.values():
        assert c.C % c.heads == 0 and all(accepted(S, c.d) for S in c.dims[1:]), c.id
    nwork = lambda c: c.M // 16 * c.heads
    assert nwork(CASES["mfma_tail9"]) == 9 and nwork(CASES["mfma_tail2"]) == 2 and nwork(CASES["n3"]) % 4 == 0
    assert all(CASES[cid].d in (64, 128) and CASES[cid].C % 4 == 0 for cid in HAS_16)
    over = {cid: max(lds_bytes(S, CASES[cid].d, True) for S in CASES[cid].dims[1:]) for cid in ("lat32", "s64_d32", "s31_d128", "s63_d128")}
    assert over == {"lat32": 74240, "s64_d32": 66560, "s31_d128": 71672, "s63_d128": 161784}
    assert sorted(HAS_16) == ["mfma_tail2", "mfma_tail9", "n3", "ref_1_16_16", "ref_2_8_8"]
