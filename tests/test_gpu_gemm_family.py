"""Every instantiation of the implicit GEMM (gsdd_gemm), the weight-gradient kernels (gsdd_conv_wgrad, gsdd_wgrad, gsdd_colsum,
gsdd_batch_rowsum) and gsdd_row_stats against a plain fp64 evaluation of the same operation, element by element.

The reference is an explicit fp64 sum over taps of shifted input rows, written here from the descriptor's definition
(include/gsdd.h), and checked against torch's fp64 conv3d / conv_transpose3d / conv3d_weight where a torch operation exists.

Error bar, per output element (not per tensor):
    |got - ref| <= gamma(K_eff) * (|pro(X)| (*) |W| + |bias| + |bvec| + |residual|),   gamma(K) = 2^-24 (8 + 2 sqrt(K))
with K_eff the contraction length (taps x Cin for the GEMM, rows for a weight gradient).  The sqrt(K) term is the random-walk
growth of K rounded f32 additions; the 8 covers the prologue / epilogue roundings and the bf16x3 products the kernels drop
(a2b3 + a3b2 + a3b3 <= 2 * 2^-24 |a||b|).  After an activation the bar is 1.2x that plus 4 * 2^-24 |out| (the activation's own
rounding; both activations have slope <= 1.1).  For the LayerNorm prologue |pro(X)| is |(x - mu) rstd gamma| + |beta|: the
prologue rounds its product before adding beta, so its error scales with the two terms, not with their (possibly cancelling)
sum.  Each case writes its worst error / bound ratio to the parity report."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import parity_report
from tests.test_gpu_train_kernels import assert_forms, form_key, form_record, run_forms

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -7777.0
BIG_M = 131072 + 77          # >= 131072 rows (the narrow / big tiles), not a multiple of 128 or 256


def gam(k_eff):
    return U * (8 + 2 * math.sqrt(k_eff))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()          # fail loudly if libgsdd.so is missing
    return gsdd_amd


def gen(seed):
    return torch.Generator().manual_seed(seed)


def same_pad_front(k, s):
    return tuple((kk - ss) // 2 + (kk - ss) % 2 for kk, ss in zip(k, s))


def conv_taps(k, s):
    pf = same_pad_front(k, s)
    return [(a - pf[0], b - pf[1], c - pf[2]) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


def pack_w(w):
    """(Cout, Cin, kt, kh, kw) -> [taps][Cout][Cin] in (kt, kh, kw) order"""
    return w.permute(2, 3, 4, 0, 1).reshape(-1, w.shape[0], w.shape[1]).contiguous()


def bn_pro(C, g):
    """BatchNorm scale / shift with a strictly positive shift: zero padding must come after BN + ReLU (relu(shift) != 0)"""
    scale = torch.randn(C, generator=g)
    shift = 0.1 + 0.5 * torch.rand(C, generator=g)
    return scale, shift


# ----------------------------------------------------------------------------- fp64 reference of the descriptor
def decode(M, grid, device):
    Do, Ho, Wo = grid
    m = torch.arange(M, device=device)
    wo = m % Wo
    q = m // Wo
    ho = q % Ho
    q = q // Ho
    return q // Do, q % Do, ho, wo


def src_rows(M, in_dims, out_grid, stride, tap, device):
    """input row of output row m under tap (dt, dh, dw), -1 where the tap falls into the zero padding"""
    N, Di, Hi, Wi = in_dims
    b, to, ho, wo = decode(M, out_grid, device)
    ti, hi, wi = to * stride[0] + tap[0], ho * stride[1] + tap[1], wo * stride[2] + tap[2]
    ok = (ti >= 0) & (ti < Di) & (hi >= 0) & (hi < Hi) & (wi >= 0) & (wi < Wi)
    return torch.where(ok, ((b * Di + ti) * Hi + hi) * Wi + wi, torch.full_like(ti, -1))


def out_rows(M, out_grid, out_dims, out_step, out_off, device):
    b, to, ho, wo = decode(M, out_grid, device)
    oD, oH, oW = out_dims
    od, oh, ow = to * out_step[0] + out_off[0], ho * out_step[1] + out_off[1], wo * out_step[2] + out_off[2]
    return b, od, oh * oW + ow, (b * oD + od) * oH * oW + oh * oW + ow


def out_addr(M, cout, out_grid, out_dims=None, out_step=(1, 1, 1), out_off=(0, 0, 0), out_pitch=None, out_mode=0, device="cpu"):
    """[M][Cout] flat index of output (m, n) in the output buffer"""
    n = torch.arange(cout, device=device)
    if out_mode == 2:
        m = torch.arange(M, device=device)
        return ((n >> 2)[None] * M + m[:, None]) * 4 + (n & 3)[None]
    od_ = out_dims if out_dims is not None else out_grid
    b, od, rem, orow = out_rows(M, out_grid, od_, out_step, out_off, device)
    if out_mode == 1:
        return ((b[:, None] * cout + n[None]) * od_[0] + od[:, None]) * (od_[1] * od_[2]) + rem[:, None]
    return orow[:, None] * (out_pitch if out_pitch is not None else cout) + n[None]


def operand(flat, src, cin, pitch, pro=None, ln=None):
    """fp64 rows pro(in[src][:cin]) and their absolute-value term; rows with src < 0 are the zero padding (applied after pro).
    Rows are read at src * pitch, so pitch < cin reads overlapping rows exactly as the kernel does."""
    ok = src >= 0
    idx = src.clamp(min=0)[:, None] * pitch + torch.arange(cin, device=flat.device)[None]
    a = flat[idx]
    if pro is not None:
        a = torch.relu(a * pro[0][None] + pro[1][None])
        aa = a
    elif ln is not None:
        mu, rs, g, bt = ln                                  # per row [M] / [M] / [M][cin] / [M][cin]
        t = (a - mu[:, None]) * rs[:, None] * g
        a, aa = t + bt, t.abs() + bt.abs()
    else:
        aa = a.abs()
    z = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.where(ok[:, None], a, z), torch.where(ok[:, None], aa, z)


def ref_gemm(x, w, M, *, in_dims=None, out_grid=None, stride=(1, 1, 1), taps=None, cin=None, pitch=None, gather=None,
             pro=None, ln=None):
    """fp64 (acc, |acc| term) [M][Cout] of sum_tap sum_c pro(in[src(m,tap)][c]) * w[tap][n][c]; a row GEMM without geometry"""
    if in_dims is None:
        in_dims, out_grid = (1, 1, 1, M), (1, 1, M)
    xf = x.double().reshape(-1)
    w64 = w.double().reshape(-1, w.shape[-2], w.shape[-1])
    cin = cin if cin is not None else w.shape[-1]
    pitch = pitch if pitch is not None else cin
    pro64 = None if pro is None else (pro[0].double().to(xf.device), pro[1].double().to(xf.device))
    acc = torch.zeros((M, w64.shape[1]), dtype=torch.float64, device=xf.device)
    ab = torch.zeros_like(acc)
    for t, tap in enumerate(taps if taps is not None else [(0, 0, 0)]):
        if gather is not None:
            src = gather.to(xf.device)
        else:
            src = src_rows(M, in_dims, out_grid, stride, tap, xf.device)
        a, aa = operand(xf, src, cin, pitch, pro64, ln)
        acc += a @ w64[t].t()
        ab += aa @ w64[t].abs().t()
    return acc, ab


def ref_rows_gpu(x, w, chunk=16384):
    """fp64 x @ w^T and |x| @ |w|^T of a large row GEMM, on the GPU in row chunks"""
    w64 = w.double()
    acc = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float64, device=x.device)
    ab = torch.empty_like(acc)
    for r in range(0, x.shape[0], chunk):
        xc = x[r:r + chunk].double()
        acc[r:r + chunk] = xc @ w64.t()
        ab[r:r + chunk] = xc.abs() @ w64.abs().t()
    return acc, ab


def act64(v, act):
    if act == 1:
        return torch.relu(v)
    if act == 2:
        return v * torch.sigmoid(1.702 * v)
    return v


def epilogue(acc, ab, k_eff, *, epi_scale=None, epi_shift=None, bvec=None, rows_per_batch=0, act=0, residual=None):
    """-> (want, bound) [M][Cout] of act(acc * scale + shift + bvec[m / rows_per_batch]) + residual"""
    dev = acc.device
    pre, mag = acc, ab
    if epi_scale is not None:
        s = epi_scale.double().to(dev)[None]
        pre, mag = pre * s, mag * s.abs()
    if epi_shift is not None:
        h = epi_shift.double().to(dev)[None]
        pre, mag = pre + h, mag + h.abs()
    if bvec is not None:
        bv = bvec.double().to(dev)[torch.arange(acc.shape[0], device=dev) // rows_per_batch]
        pre, mag = pre + bv, mag + bv.abs()
    bound = gam(k_eff) * mag
    want = act64(pre, act)
    if act:
        bound = 1.2 * bound + 4 * U * want.abs()
    if residual is not None:
        want = want + residual
        bound = bound + gam(k_eff) * residual.abs()
    return want, bound


def ratio_of(err, bound):
    inf = torch.full_like(err, float("inf"))
    return torch.where(bound > 0, err / bound, torch.where(err > 0, inf, torch.zeros_like(err)))


def check_written(name, got_buf, init_buf, addr, want, bound, **extra):
    """got_buf[addr] within bound of want (finite), every other element of got_buf bit-identical to init_buf, each address once"""
    got = got_buf.detach().reshape(-1)
    init = init_buf.detach().reshape(-1).to(got.device)
    addr = addr.reshape(-1).to(got.device)
    want, bound = want.reshape(-1).to(got.device), bound.reshape(-1).to(got.device)
    assert addr.unique().numel() == addr.numel(), "reference writes an element twice"
    g = got[addr].double()
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite outputs"
    worst = float(ratio_of((g - want).abs(), bound).max())
    written = torch.zeros(got.numel(), dtype=torch.bool, device=got.device)
    written[addr] = True
    untouched = torch.equal(got.view(torch.int32)[~written], init.view(torch.int32)[~written])
    parity_report(f"gemm_family::{name}", dict(worst_ratio=worst, n=int(addr.numel()), **extra))
    assert untouched, f"{name}: elements outside the output were written"
    assert worst <= 1.0, f"{name}: worst error / bound = {worst:.3g}"
    return worst


def check_dense(name, got, want, bound, **extra):
    g = got.detach().double().reshape(-1)
    want, bound = want.reshape(-1).to(g.device), bound.reshape(-1).to(g.device)
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite outputs"
    worst = float(ratio_of((g - want).abs(), bound).max())
    parity_report(f"gemm_family::{name}", dict(worst_ratio=worst, n=int(g.numel()), **extra))
    assert worst <= 1.0, f"{name}: worst error / bound = {worst:.3g}"
    return worst


# ----------------------------------------------------------------------------- gsdd_gemm: convolutions, every instantiation
# (id, kernel, stride, Cin, Cout, exact_f32, input dims (N, T, H, W))
CONV_CASES = [
    ("x64_f32-keff40", (1, 1, 1), (1, 1, 1), 40, 3, None, (2, 1, 10, 10)),
    ("x64_f32-flag-k3s111", (3, 3, 3), (1, 1, 1), 12, 24, True, (2, 3, 6, 7)),
    ("x64_x3-k3s122", (3, 3, 3), (1, 2, 2), 12, 24, None, (2, 4, 10, 14)),
    ("x64_x3-k4s222", (4, 4, 4), (2, 2, 2), 4, 3, None, (2, 6, 10, 12)),
    ("x128_f32-keff40", (1, 1, 1), (1, 1, 1), 40, 200, None, (2, 1, 10, 10)),
    ("x128_f32-flag-k4s222", (4, 4, 4), (2, 2, 2), 12, 136, True, (2, 6, 10, 12)),
    ("x128_x3-k3s111", (3, 3, 3), (1, 1, 1), 40, 68, None, (1, 5, 9, 11)),
    ("x128_x3-k4s122", (4, 4, 4), (1, 2, 2), 12, 200, None, (2, 3, 8, 10)),
]


@pytest.mark.parametrize("cid,k,stride,cin,cout,exact,dims", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_gemm_conv(G, cid, k, stride, cin, cout, exact, dims):
    """Same-padded conv3d with the BatchNorm + ReLU prologue (positive shift) and a bias: taps, padding and strides."""
    g = gen(zlib.crc32(cid.encode()))
    B, T, H, W = dims
    x = torch.randn(B, cin, T, H, W, generator=g)
    ntaps = k[0] * k[1] * k[2]
    w = torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * ntaps)
    bias = torch.randn(cout, generator=g)
    pro = bn_pro(cin, g)
    To, Ho, Wo = T // stride[0], H // stride[1], W // stride[2]
    M = B * To * Ho * Wo
    taps = conv_taps(k, stride)
    xr = x.permute(0, 2, 3, 4, 1).contiguous()
    acc, ab = ref_gemm(xr, pack_w(w), M, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo), stride=stride, taps=taps, pro=pro)
    # the explicit reference is the torch convolution of the prologue's output
    from oracle import vqvae as ov
    xp = torch.relu(x.double() * pro[0].double()[None, :, None, None, None] + pro[1].double()[None, :, None, None, None])
    tconv = ov.same_pad_conv3d(xp, w.double(), None, stride).permute(0, 2, 3, 4, 1).reshape(M, cout)
    assert float((tconv - acc).abs().max()) < 1e-12 * (1 + float(ab.max()))
    want, bound = epilogue(acc, ab, ntaps * cin, epi_shift=bias)
    out = torch.full((M, cout), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.gemm(xr.cuda(), pack_w(w).cuda(), out, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo), stride=stride,
               taps=G.ops.taps_tensor(taps, "cuda") if ntaps > 1 else None, ntaps=ntaps, pro=(pro[0].cuda(), pro[1].cuda()),
               epi_shift=bias.cuda(), exact_f32=exact)
    check_written(f"conv[{cid}]", out, init, out_addr(M, cout, (To, Ho, Wo)), want, bound, M=M, k_eff=ntaps * cin)


# ----------------------------------------------------------------------------- narrow / big: long row GEMMs over many rows
@pytest.mark.parametrize("cid,cout", [("narrow-rows", 24), ("big-rows", 136)])
def test_gemm_rows_large(G, cid, cout):
    cin = 1028                                     # >= 1024, a 4-channel tail in the last 32-wide chunk
    torch.manual_seed(7)
    x = torch.randn(BIG_M, cin, device="cuda")
    w = torch.randn(cout, cin, device="cuda") / math.sqrt(cin)
    bias = torch.randn(cout, device="cuda")
    acc, ab = ref_rows_gpu(x, w)
    want, bound = epilogue(acc, ab, cin, epi_shift=bias)
    del acc, ab
    out = torch.full((BIG_M, cout), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.linear(x, w, out, bias=bias)
    check_written(f"rows_large[{cid}]", out, init, out_addr(BIG_M, cout, (1, 1, BIG_M), device="cuda"), want, bound, M=BIG_M,
                  k_eff=cin)


# ----------------------------------------------------------------------------- single-term contractions (the bf16x3 split)
@pytest.mark.parametrize("cid,M,cin,cout", [("x64_x3", 200, 68, 24), ("x128_x3", 200, 68, 136), ("narrow", BIG_M, 1028, 24),
                                             ("big", BIG_M, 1028, 136)])
def test_gemm_single_term(G, cid, M, cin, cout):
    """One nonzero channel per input row: each output is one product plus the bias, which the three-piece split must carry to
    within 2^-22 (|x w| + |b|).  Budget: the dropped a2b3 + a3b2 + a3b3 are below 2^-26 |x w|; the accumulate step that adds
    a1b1 to the five small pieces costs at most one ulp (2^-23 |x w|), and the bias add half an ulp of the sum -- 3 x 2^-24 of
    the 4 x 2^-24 allowed (measured worst ratio 0.83).  A missing cross product (a1b3 or a3b1, up to 2^-17 |x w|) fails here;
    in a sum of many terms accumulation noise hides it."""
    torch.manual_seed(11)
    ch = torch.randint(0, cin, (M,), device="cuda")
    val = torch.randn(M, device="cuda") * torch.exp2(torch.randint(-12, 13, (M,), device="cuda").float())
    x = torch.zeros(M, cin, device="cuda")
    x[torch.arange(M, device="cuda"), ch] = val
    w = torch.randn(cout, cin, device="cuda")
    bias = torch.randn(cout, device="cuda") * 1e-3
    prod = val.double()[:, None] * w.double()[:, ch].t()
    want = prod + bias.double()[None]
    bound = 2.0 ** -22 * (prod.abs() + bias.double().abs()[None])
    out = torch.full((M, cout), SENTINEL, device="cuda")
    G.ops.linear(x, w, out, bias=bias)
    check_dense(f"single_term[{cid}]", out, want, bound, M=M, k_eff=cin)


# ----------------------------------------------------------------------------- transposed-conv phases
def convT_phases(k, s, pf):
    per_dim = []
    for kk, ss, p0 in zip(k, s, pf):
        per_dim.append([[(t, (p + kk - 1 - t) // ss - p0) for t in range(kk) if (p + kk - 1 - t) % ss == 0] for p in range(ss)])
    out = []
    for pt, tt in enumerate(per_dim[0]):
        for ph, th in enumerate(per_dim[1]):
            for pw, tw in enumerate(per_dim[2]):
                out.append(((pt, ph, pw), [(a[0], b[0], c[0]) for a in tt for b in th for c in tw],
                            [(a[1], b[1], c[1]) for a in tt for b in th for c in tw]))
    return out


@pytest.mark.parametrize("cid,stride,cin,cout,out_mode,dims,use_pro", [
    ("x128_x3-s222", (2, 2, 2), 40, 68, 0, (2, 3, 5, 6), True),
    ("narrow-s122-ncdhw", (1, 2, 2), 64, 3, 1, (1, 8, 127, 130), False),     # the decoder's last layer, >= 131072 rows
])
def test_gemm_convT_phases(G, cid, stride, cin, cout, out_mode, dims, use_pro):
    """A stride-s transposed conv as s^3 phase GEMMs (out_dims / out_step / out_off) into a sentinel-filled buffer: each phase
    changes exactly its own rows, together they write every element once, and the result is fp64 conv_transpose3d."""
    g = gen(5)
    k = (4, 4, 4)
    B, T, H, W = dims
    x = torch.randn(B, cin, T, H, W, generator=g)
    w = torch.randn(cin, cout, *k, generator=g) / math.sqrt(cin * 16)
    bias = torch.randn(cout, generator=g)
    pro = bn_pro(cin, g) if use_pro else None
    M = B * T * H * W
    To, Ho, Wo = T * stride[0], H * stride[1], W * stride[2]
    xr = x.permute(0, 2, 3, 4, 1).contiguous()
    xr_d = xr.cuda()
    shape = (B, cout, To, Ho, Wo) if out_mode == 1 else (B * To * Ho * Wo, cout)
    out = torch.full(shape, SENTINEL, device="cuda")
    want_all = torch.full((out.numel(),), float("nan"), dtype=torch.float64)
    worst = 0.0
    phases = convT_phases(k, stride, same_pad_front(k, stride))
    for (ph, ks, offs) in phases:
        wp = torch.stack([w[:, :, a, b, c].t() for (a, b, c) in ks]).contiguous()
        before = out.clone()
        G.ops.gemm(xr_d, wp.cuda(), out, in_dims=(B, T, H, W), out_grid=(T, H, W), taps=G.ops.taps_tensor(offs, "cuda"),
                   ntaps=len(ks), pro=None if pro is None else (pro[0].cuda(), pro[1].cuda()), epi_shift=bias.cuda(),
                   out_dims=(To, Ho, Wo), out_step=stride, out_off=ph, out_mode=out_mode)
        acc, ab = ref_gemm(xr, wp, M, in_dims=(B, T, H, W), out_grid=(T, H, W), taps=offs, pro=pro)
        want, bound = epilogue(acc, ab, len(ks) * cin, epi_shift=bias)
        addr = out_addr(M, cout, (T, H, W), (To, Ho, Wo), stride, ph, out_mode=out_mode)
        worst = max(worst, check_written(f"convT_phase[{cid}-{ph}]", out, before, addr, want, bound, k_eff=len(ks) * cin))
        want_all[addr.reshape(-1)] = want.reshape(-1)
    flat = out.reshape(-1)
    assert not bool((flat == SENTINEL).any()), "an element no phase wrote"
    assert not bool(torch.isnan(want_all).any())
    if out_mode == 0:                               # the phases assembled are the fp64 transposed convolution
        from oracle import vqvae as ov
        xp = x.double() if pro is None else torch.relu(x.double() * pro[0].double()[None, :, None, None, None] +
                                                       pro[1].double()[None, :, None, None, None])
        tconv = ov.same_pad_convT3d(xp, w.double(), bias.double(), stride).permute(0, 2, 3, 4, 1).reshape(-1)
        assert float((tconv - want_all).abs().max()) < 1e-10
    parity_report(f"gemm_family::convT_phases[{cid}]", dict(worst_ratio=worst, phases=len(phases), M=M))


# ----------------------------------------------------------------------------- masking: pitches, unread rows, tails
@pytest.mark.parametrize("cid,k,stride,cin,pitch,cout,opitch,dims", [
    ("x64_x3-1x1s222", (1, 1, 1), (2, 2, 2), 68, 76, 24, 29, (2, 4, 6, 10)),
    ("x128_x3-k3s111", (3, 3, 3), (1, 1, 1), 12, 20, 200, 205, (1, 3, 7, 9)),
])
def test_gemm_masking(G, cid, k, stride, cin, pitch, cout, opitch, dims):
    """NaN in the channels between Cin and in_pitch, in the input rows no output reads and in the weight rows past the last
    tap's Cout; a sentinel in the output columns between Cout and out_pitch.  Outputs finite and correct, sentinels intact."""
    g = gen(17)
    B, T, H, W = dims
    ntaps = k[0] * k[1] * k[2]
    To, Ho, Wo = T // stride[0], H // stride[1], W // stride[2]
    M = B * To * Ho * Wo
    taps = conv_taps(k, stride)
    Mi = B * T * H * W
    xin = torch.full((Mi, pitch), float("nan"))
    xin[:, :cin] = torch.randn(Mi, cin, generator=g)
    read = torch.zeros(Mi, dtype=torch.bool)
    for tap in taps:
        s = src_rows(M, (B, T, H, W), (To, Ho, Wo), stride, tap, "cpu")
        read[s[s >= 0]] = True
    if not bool(read.all()):
        xin[~read] = float("nan")
    wbuf = torch.full((ntaps * cout + 37, cin), float("nan"))
    wbuf[:ntaps * cout] = torch.randn(ntaps * cout, cin, generator=g) / math.sqrt(cin * ntaps)
    bias = torch.randn(cout, generator=g)
    acc, ab = ref_gemm(xin, wbuf[:ntaps * cout].view(ntaps, cout, cin), M, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo),
                       stride=stride, taps=taps, cin=cin, pitch=pitch)
    want, bound = epilogue(acc, ab, ntaps * cin, epi_shift=bias)
    out = torch.full((M, opitch), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.gemm(xin.cuda(), wbuf.cuda(), out, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo), stride=stride,
               taps=G.ops.taps_tensor(taps, "cuda") if ntaps > 1 else None, ntaps=ntaps, cin=cin, in_pitch=pitch, cout=cout,
               epi_shift=bias.cuda(), out_pitch=opitch)
    check_written(f"masking[{cid}]", out, init, out_addr(M, cout, (To, Ho, Wo), out_pitch=opitch), want, bound,
                  unread_rows=int((~read).sum()))


# ----------------------------------------------------------------------------- overlapping rows: the merged-kw stem
def stem_layout(k, s, W):
    """padw and the tap table of the merged-kw first conv (rows of 4 channels, kw window = 4 kw consecutive floats)"""
    pf = same_pad_front(k, s)
    pb = tuple(kk - ss - p for kk, ss, p in zip(k, s, pf))
    Wo = W // s[2]
    padw = max(pf[2], pb[2], (Wo - 1) * s[2] + k[2] - pf[2] - W)
    taps = [(a - pf[0], b - pf[1], padw - pf[2]) for a in range(k[0]) for b in range(k[1])]
    return padw, taps


@pytest.mark.parametrize("cid,k,stride,cout,dims,act", [
    ("x64_x3-vqvae-k4s122", (4, 4, 4), (1, 2, 2), 24, (2, 5, 12, 14), 1),
    ("x128_x3-i3d-k7s222", (7, 7, 7), (2, 2, 2), 68, (1, 6, 14, 18), 1),
])
def test_gemm_stem_overlapping_rows(G, cid, k, stride, cout, dims, act):
    """ncdhw_to_rows (checked exactly) and the conv over rows that overlap (cin = 4 kw, in_pitch = 4) against fp64 conv3d."""
    g = gen(23)
    B, T, H, W = dims
    x = torch.randn(B, 3, T, H, W, generator=g)
    padw, taps = stem_layout(k, stride, W)
    xr = G.ops.ncdhw_to_rows(x.cuda(), 4, padw)
    want_rows = torch.zeros(B, T, H, W + 2 * padw, 4)
    want_rows[:, :, :, padw:padw + W, :3] = x.permute(0, 2, 3, 4, 1)
    assert torch.equal(xr.cpu(), want_rows)
    w = torch.randn(cout, 3, *k, generator=g) / math.sqrt(3 * k[0] * k[1] * k[2])
    escale = torch.randn(cout, generator=g)
    eshift = torch.randn(cout, generator=g)
    wp = torch.zeros(cout, 4, *k)
    wp[:, :3] = w
    wm = wp.permute(2, 3, 0, 4, 1).reshape(k[0] * k[1], cout, k[2] * 4).contiguous()     # [kt*kh][Cout][kw*4]
    To, Ho, Wo = T // stride[0], H // stride[1], W // stride[2]
    M = B * To * Ho * Wo
    from oracle import vqvae as ov
    acc = ov.same_pad_conv3d(x.double(), w.double(), None, stride).permute(0, 2, 3, 4, 1).reshape(M, cout)
    ab = ov.same_pad_conv3d(x.double().abs(), w.double().abs(), None, stride).permute(0, 2, 3, 4, 1).reshape(M, cout)
    acc2, _ = ref_gemm(want_rows, wm, M, in_dims=(B, T, H, W + 2 * padw), out_grid=(To, Ho, Wo), stride=stride, taps=taps,
                       cin=4 * k[2], pitch=4)
    assert float((acc2 - acc).abs().max()) < 1e-12 * (1 + float(ab.max()))
    k_eff = k[0] * k[1] * 4 * k[2]
    want, bound = epilogue(acc, ab, k_eff, epi_scale=escale, epi_shift=eshift, act=act)
    out = torch.full((M, cout), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.gemm(xr, wm.cuda(), out, in_dims=(B, T, H, W + 2 * padw), out_grid=(To, Ho, Wo), stride=stride,
               taps=G.ops.taps_tensor(taps, "cuda"), ntaps=len(taps), cin=4 * k[2], in_pitch=4, epi_scale=escale.cuda(),
               epi_shift=eshift.cuda(), act=act)
    check_written(f"stem[{cid}]", out, init, out_addr(M, cout, (To, Ho, Wo)), want, bound, k_eff=k_eff)


# ----------------------------------------------------------------------------- epilogues
LB, NB = 77, 3            # rows per batch (not a multiple of 128) and batches


@pytest.mark.parametrize("cid", ["scale_shift_relu", "gelu2", "bvec", "residual", "residual_inplace", "head_major", "gather",
                                 "f32-bvec_residual_gelu2"])
def test_gemm_epilogues(G, cid):
    g = gen(31)
    M = LB * NB
    cin = 40 if cid.startswith("f32") else 100
    cout = 200 if cid == "head_major" else 68
    rows_in = 57 if cid == "gather" else M
    x = torch.randn(rows_in, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / math.sqrt(cin)
    bias = torch.randn(cout, generator=g)
    kw = dict(epi_shift=bias)
    gather = None
    if cid == "scale_shift_relu":
        kw.update(epi_scale=torch.randn(cout, generator=g), act=1)
    if cid in ("gelu2", "f32-bvec_residual_gelu2"):
        kw.update(act=2)
    if cid in ("bvec", "f32-bvec_residual_gelu2"):
        kw.update(bvec=torch.randn(NB, cout, generator=g), rows_per_batch=LB)
    if cid == "gather":
        gather = torch.randint(0, rows_in, (M,), generator=g)
        gather[:20] = gather[20:40].flip(0)                 # repeated, unsorted
    acc, ab = ref_gemm(x, w.view(1, cout, cin), M, gather=gather)
    res = None
    if cid in ("residual", "residual_inplace", "f32-bvec_residual_gelu2"):
        res = (torch.randn(M, cout, generator=g) * 3).double()
    want, bound = epilogue(acc, ab, cin, residual=res, **kw)
    dkw = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in kw.items()}
    if cid == "head_major":
        out = torch.full((cout // 4, M, 4), SENTINEL, device="cuda")
    elif cid == "residual_inplace":
        out = res.float().cuda()
    else:
        out = torch.full((M, cout), SENTINEL, device="cuda")
    init = out.clone()
    residual = None
    if cid == "residual":
        residual = res.float().cuda()
    elif cid == "residual_inplace":
        residual = out
    elif cid.startswith("f32"):
        residual = res.float().cuda()
    G.ops.gemm(x.cuda(), w.cuda(), out, in_dims=(1, 1, 1, rows_in), out_grid=(1, 1, M), gather=None if gather is None else gather.cuda(),
               residual=residual, out_mode=2 if cid == "head_major" else 0, **dkw)
    addr = out_addr(M, cout, (1, 1, M), out_mode=2 if cid == "head_major" else 0)
    check_written(f"epilogue[{cid}]", out, init, addr, want, bound, k_eff=cin)


# ----------------------------------------------------------------------------- LayerNorm prologue and row statistics
def ln_rows(M, C, g):
    """rows with unit-scale values, and every 5th row around a large mean (~1e3) with a small spread"""
    x = torch.randn(M, C, generator=g)
    x[::5] = 1e3 * (1 + torch.rand(M // 5 + (M % 5 > 0), 1, generator=g)) + 0.05 * torch.randn(M // 5 + (M % 5 > 0), C, generator=g)
    return x


@pytest.mark.parametrize("C", [64, 100, 1024])
def test_row_stats(G, C):
    """gsdd_row_stats (mean, 1/sqrt(biased var + eps)) against fp64 of the same f32 rows.  The mean is a sum of C terms
    (gamma(C) of the mean of |x|); the variance sums squares around the f32 mean, whose error d adds d^2 to it."""
    g = gen(C)
    M = LB * NB
    x = ln_rows(M, C, g)
    eps = 1e-5
    x64 = x.double()
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    rstd = 1 / torch.sqrt(var + eps)
    stats = torch.empty(M, 2, device="cuda")
    G.ops.row_stats(x.cuda(), stats, eps=eps)
    st = stats.cpu().double()
    dm = gam(C) * x64.abs().mean(1)
    r1 = check_dense(f"row_stats_mean[C{C}]", st[:, 0], mean, dm, C=C)
    r2 = check_dense(f"row_stats_rstd[C{C}]", st[:, 1], rstd, rstd * (gam(C) + dm ** 2 / (var + eps)), C=C)
    assert max(r1, r2) <= 1.0


@pytest.mark.parametrize("cid", ["plain-x128_x3", "adaln_sel-x128_x3", "adaln_sel-x64_f32"])
def test_gemm_ln_prologue(G, cid):
    """y = (x - mean) * rstd * gamma + beta applied while staging; with AdaLN the (gamma, beta) row is sel[batch] of a
    [T][2D] table (ln_stride = 2D, beta at +D, d3pm.py's layout), and batches select different rows."""
    g = gen(41)
    M = LB * NB
    D = 100 if "x3" in cid else 40
    cout = 136 if "x128" in cid else 24
    x = ln_rows(M, D, g)
    stats = torch.empty(M, 2, device="cuda")
    G.ops.row_stats(x.cuda(), stats)                  # inputs of the GEMM (checked on their own in test_row_stats)
    st = stats.cpu().double()
    w = torch.randn(cout, D, generator=g) / math.sqrt(D)
    bias = torch.randn(cout, generator=g)
    if cid.startswith("plain"):
        gamma_, beta_ = 1 + 0.3 * torch.randn(D, generator=g), torch.randn(D, generator=g)
        ln = (stats, gamma_.cuda(), beta_.cuda(), None, 0)
        grow, brow = gamma_.double()[None].expand(M, D), beta_.double()[None].expand(M, D)
        rpb = 0
    else:
        Tt = 5
        table = torch.randn(Tt, 2 * D, generator=g)
        sel = torch.tensor([3, 0, 4], dtype=torch.int64)
        tab = table.cuda()
        ln = (stats, tab.view(-1), tab.view(-1)[D:], sel.cuda(), 2 * D)
        rsel = sel[torch.arange(M) // LB]
        grow, brow = table.double()[rsel, :D], table.double()[rsel, D:]
        rpb = LB
    acc, ab = ref_gemm(x, w.view(1, cout, D), M, ln=(st[:, 0], st[:, 1], grow, brow))
    want, bound = epilogue(acc, ab, D, epi_shift=bias)
    out = torch.full((M, cout), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.gemm(x.cuda(), w.cuda(), out, in_dims=(1, 1, 1, M), out_grid=(1, 1, M), ln=ln, rows_per_batch=rpb,
               epi_shift=bias.cuda(), exact_f32=True if "f32" in cid else None)
    check_written(f"ln_prologue[{cid}]", out, init, out_addr(M, cout, (1, 1, M)), want, bound, k_eff=D)


# ----------------------------------------------------------------------------- dynamic range
@pytest.mark.parametrize("cid,cin,cout,exact", [("x128_x3", 100, 136, None), ("x64_f32-flag", 100, 24, True),
                                                 ("x64_x3", 100, 24, None)])
def test_gemm_dynamic_range(G, cid, cin, cout, exact):
    """Gradient-sized rows (1e-6), every 7th row scaled by 1e9 and every 5th by 1e-9: the element-wise bound still holds."""
    g = gen(53)
    M = 200
    x = torch.randn(M, cin, generator=g) * 1e-6
    x[::7] *= 1e9
    x[::5] *= 1e-9
    w = torch.randn(cout, cin, generator=g) * 0.1
    acc, ab = ref_gemm(x, w.view(1, cout, cin), M)
    want, bound = epilogue(acc, ab, cin)
    out = torch.full((M, cout), SENTINEL, device="cuda")
    init = out.clone()
    G.ops.gemm(x.cuda(), w.cuda(), out, in_dims=(1, 1, 1, M), out_grid=(1, 1, M), exact_f32=exact)
    check_written(f"dynamic_range[{cid}]", out, init, out_addr(M, cout, (1, 1, M)), want, bound, k_eff=cin)


# ----------------------------------------------------------------------------- gsdd_conv_wgrad
def conv_wgrad_slabs(M, cout, cin, ntaps, exact):
    """(kernel, rows per block in slabs) as gsdd_conv_wgrad picks them: the cases below assert the regime they claim to cover"""
    big = not exact and cout >= 128 and cin >= 128
    T = 128 if big else 64
    rows = 128 if exact else 64
    nslabs = -(-M // rows)
    per_x = -(-cout // T) * -(-cin // T) * ntaps
    gx = max(1, min(-(-(1024 if big else 2048) // per_x), nslabs))
    slabs = -(-nslabs // gx)
    slabs = (nslabs if nslabs < 8 else 8) if slabs < 8 else min(slabs, 128)
    return ("f32" if exact else "x3_128" if big else "x3_64"), slabs


def ref_conv_wgrad(x, dY, M, *, in_dims, out_grid, stride, taps, cin, pitch, pro=None, out_dims=None, out_step=(1, 1, 1),
                   out_off=(0, 0, 0), dW0):
    """fp64 dW0[tap] + sum_m dY[orow(m)] (x) pro(x[src(m,tap)]) and its absolute-value term"""
    xf = x.double().reshape(-1)
    dy = dY.double()
    _, _, _, orow = out_rows(M, out_grid, out_dims if out_dims is not None else out_grid, out_step, out_off, "cpu")
    ys = dy[orow]
    pro64 = None if pro is None else (pro[0].double(), pro[1].double())
    want, bound = [], []
    for t, tap in enumerate(taps):
        a, aa = operand(xf, src_rows(M, in_dims, out_grid, stride, tap, "cpu"), cin, pitch, pro64)
        want.append(dW0[t].double() + ys.t() @ a)
        bound.append(gam(M) * (dW0[t].double().abs() + ys.abs().t() @ aa))
    return torch.stack(want), torch.stack(bound)


# (id, kernel, stride, Cin, Cout, dims (N, T, H, W), exact, pro, expected (kernel, slabs))
CW_CASES = [
    ("f32-k3s122-pro-slabs8", (3, 3, 3), (1, 2, 2), 12, 68, (2, 6, 20, 26), True, True, ("f32", 8)),
    ("x3_64-k4s222-pro", (4, 4, 4), (2, 2, 2), 40, 24, (2, 8, 12, 18), None, True, ("x3_64", 7)),
    ("x3_128-k3s111-pro-slabs8", (3, 3, 3), (1, 1, 1), 132, 136, (1, 4, 10, 13), None, True, ("x3_128", 8)),
    ("x3_64-k3s111-slabs128", (3, 3, 3), (1, 1, 1), 12, 12, (1, 16, 200, 201), None, False, ("x3_64", 128)),
]


@pytest.mark.parametrize("cid,k,stride,cin,cout,dims,exact,use_pro,regime", CW_CASES, ids=[c[0] for c in CW_CASES])
def test_conv_wgrad(G, cid, k, stride, cin, cout, dims, exact, use_pro, regime):
    """dW (prefilled: the kernel accumulates) += sum over output rows of dY (x) pro(x) for every tap, padding and stride."""
    g = gen(61)
    B, T, H, W = dims
    To, Ho, Wo = T // stride[0], H // stride[1], W // stride[2]
    M = B * To * Ho * Wo
    ntaps = k[0] * k[1] * k[2]
    assert conv_wgrad_slabs(M, cout, cin, ntaps, exact) == regime
    taps = conv_taps(k, stride)
    x = torch.randn(B * T * H * W, cin, generator=g)
    dY = torch.randn(M, cout, generator=g)
    pro = bn_pro(cin, g) if use_pro else None
    dW0 = torch.randn(ntaps, cout, cin, generator=g)
    want, bound = ref_conv_wgrad(x, dY, M, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo), stride=stride, taps=taps, cin=cin,
                                 pitch=cin, pro=pro, dW0=dW0)
    if cid.startswith("f32"):                          # the explicit reference is torch's fp64 conv weight gradient
        xs = x.double().view(B, T, H, W, cin).permute(0, 4, 1, 2, 3)
        xs = torch.relu(xs * pro[0].double()[None, :, None, None, None] + pro[1].double()[None, :, None, None, None])
        pf = same_pad_front(k, stride)
        pads = []
        for kk, ss, p in zip(k[::-1], stride[::-1], pf[::-1]):
            pads += [p, kk - ss - p]
        tw = torch.nn.grad.conv3d_weight(F.pad(xs, pads), (cout, cin, *k), dY.double().view(B, To, Ho, Wo, cout).permute(0, 4, 1, 2, 3),
                                         stride=stride)
        assert float((pack_w(tw) + dW0.double() - want).abs().max()) < 1e-9
    dW = dW0.cuda()
    G.ops.conv_wgrad(x.cuda(), dY.cuda(), dW, in_dims=(B, T, H, W), out_grid=(To, Ho, Wo), stride=stride,
                     taps=G.ops.taps_tensor(taps, "cuda"), ntaps=ntaps, cin=cin, cout=cout,
                     pro=None if pro is None else (pro[0].cuda(), pro[1].cuda()), exact_f32=exact)
    check_dense(f"conv_wgrad[{cid}]", dW, want, bound, M=M, slabs=regime[1])


@pytest.mark.parametrize("cid,exact", [("x3_64", None), ("f32", True)])
def test_conv_wgrad_transposed_phase(G, cid, exact):
    """Weight gradient of one phase of a stride-(2,2,2) transposed conv: x on the coarse grid, dY read on the fine grid through
    out_dims / out_step / out_off (the training step's layout)."""
    g = gen(67)
    B, T, H, W, cin, cout = 2, 3, 5, 7, 40, 24
    stride = (2, 2, 2)
    k = (4, 4, 4)
    ph, ks, offs = convT_phases(k, stride, same_pad_front(k, stride))[5]
    M = B * T * H * W
    fine = (2 * T, 2 * H, 2 * W)
    x = torch.randn(M, cin, generator=g)
    dY = torch.randn(B * fine[0] * fine[1] * fine[2], cout, generator=g)
    pro = bn_pro(cin, g)
    dW0 = torch.randn(len(ks), cout, cin, generator=g)
    want, bound = ref_conv_wgrad(x, dY, M, in_dims=(B, T, H, W), out_grid=(T, H, W), stride=(1, 1, 1), taps=offs, cin=cin,
                                 pitch=cin, pro=pro, out_dims=fine, out_step=stride, out_off=ph, dW0=dW0)
    dW = dW0.cuda()
    G.ops.conv_wgrad(x.cuda(), dY.cuda(), dW, in_dims=(B, T, H, W), out_grid=(T, H, W), taps=G.ops.taps_tensor(offs, "cuda"),
                     ntaps=len(ks), cin=cin, cout=cout, pro=(pro[0].cuda(), pro[1].cuda()), out_dims=fine, out_step=stride,
                     out_off=ph, exact_f32=exact)
    check_dense(f"conv_wgrad_convT_phase[{cid}]", dW, want, bound, M=M, phase=list(ph))


@pytest.mark.parametrize("cid,exact", [("x3_64", None), ("f32", True)])
def test_conv_wgrad_merged_kw(G, cid, exact):
    """The stem's weight gradient over overlapping rows (in_pitch = 4, cin = 4 kw), checked against fp64 conv3d_weight."""
    g = gen(71)
    B, T, H, W, cout = 2, 5, 12, 14, 24
    k, stride = (4, 4, 4), (1, 2, 2)
    x = torch.randn(B, 3, T, H, W, generator=g)
    padw, taps = stem_layout(k, stride, W)
    xr = G.ops.ncdhw_to_rows(x.cuda(), 4, padw)
    To, Ho, Wo = T // stride[0], H // stride[1], W // stride[2]
    M = B * To * Ho * Wo
    dY = torch.randn(M, cout, generator=g)
    dW0 = torch.randn(len(taps), cout, 4 * k[2], generator=g)
    want, bound = ref_conv_wgrad(xr.cpu(), dY, M, in_dims=(B, T, H, W + 2 * padw), out_grid=(To, Ho, Wo), stride=stride,
                                 taps=taps, cin=4 * k[2], pitch=4, dW0=dW0)
    from oracle import vqvae as ov
    pads = ov.same_pad(k, stride)
    xp = F.pad(x.double(), [pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]])
    tw = torch.nn.grad.conv3d_weight(xp, (cout, 3, *k), dY.double().view(B, To, Ho, Wo, cout).permute(0, 4, 1, 2, 3),
                                     stride=stride)
    got_layout = (want - dW0.double()).view(k[0], k[1], cout, k[2], 4)[..., :3].permute(2, 4, 0, 1, 3)
    assert float((got_layout - tw).abs().max()) < 1e-9
    dW = dW0.cuda()
    G.ops.conv_wgrad(xr, dY.cuda(), dW, in_dims=(B, T, H, W + 2 * padw), out_grid=(To, Ho, Wo), stride=stride,
                     taps=G.ops.taps_tensor(taps, "cuda"), ntaps=len(taps), cin=4 * k[2], cout=cout, in_pitch=4, exact_f32=exact)
    check_dense(f"conv_wgrad_merged_kw[{cid}]", dW, want, bound, M=M)


@pytest.mark.parametrize("cid,cin,cout,exact", [("x3_64", 68, 24, None), ("x3_128", 132, 136, None), ("f32", 68, 24, True)])
def test_conv_wgrad_cancellation(G, cid, cin, cout, exact):
    """dY with zero column mean against x with a large positive mean (behind a train-mode BatchNorm): dW is a small difference
    of large sums; the bound is stated against |dY|^T |x|."""
    g = gen(73)
    B, T, H, W = 1, 4, 30, 31
    M = B * T * H * W
    k = (3, 3, 3)
    taps = conv_taps(k, (1, 1, 1))
    x = 40 + torch.randn(M, cin, generator=g)
    dY = torch.randn(M, cout, generator=g).double()
    dY = (dY - dY.mean(0, keepdim=True)).float()
    dW0 = torch.randn(27, cout, cin, generator=g) * 1e-3
    want, bound = ref_conv_wgrad(x, dY, M, in_dims=(B, T, H, W), out_grid=(T, H, W), stride=(1, 1, 1), taps=taps, cin=cin,
                                 pitch=cin, dW0=dW0)
    dW = dW0.cuda()
    G.ops.conv_wgrad(x.cuda(), dY.cuda(), dW, in_dims=(B, T, H, W), out_grid=(T, H, W), taps=G.ops.taps_tensor(taps, "cuda"),
                     ntaps=27, cin=cin, cout=cout, exact_f32=exact)
    check_dense(f"conv_wgrad_cancellation[{cid}]", dW, want, bound, M=M)


# ----------------------------------------------------------------------------- gsdd_wgrad / gsdd_colsum / gsdd_batch_rowsum
def wgrad_slabs(M, N, K):
    slabs, tiles = 8, -(-N // 64) * -(-K // 64)
    while slabs > 1 and -(-M // (128 * slabs)) * tiles < 512:
        slabs >>= 1
    return slabs


# The case bodies below take form = "fast" (this file's tests: the switch is off) or "reproducible" (gsdd_set_deterministic, held on
# by the fixture of tests/test_gpu_train_reproducible.py, which also hands in `fast_form`); reference and bounds are the same for both.
def guarded_out(fill):
    """-> (buffer, view): a copy of `fill` on the device with 64 sentinel floats on either side"""
    n = fill.numel()
    buf = torch.full((64 + n + 64,), SENTINEL, device="cuda")
    v = buf[64:64 + n].view(fill.shape)
    v.copy_(fill)
    return buf, v


def out_guards_intact(*bufs):
    return all(bool((b[:64] == SENTINEL).all()) and bool((b[-64:] == SENTINEL).all()) for b in bufs)


def wgrad_ref(dY, X, dW0, db0):
    """fp64 (want, bound) of dW0 + dY^T X and of db0 + colsum(dY)"""
    M = dY.shape[0]
    want = dW0.double() + dY.double().t() @ X.double()
    bound = gam(M) * (dW0.double().abs() + dY.double().abs().t() @ X.double().abs())
    return want, bound, db0.double() + dY.double().sum(0), gam(M) * (db0.double().abs() + dY.double().abs().sum(0))


def wgrad_case(G, name, dY, X, dW0, db0, with_db, form="fast", fast_form=None, **extra):
    M, N, K = dY.shape[0], dY.shape[1], X.shape[1]
    want, bound, want_db, bound_db = wgrad_ref(dY, X, dW0, db0)

    def run():
        wbuf, dW = guarded_out(dW0)
        bbuf, db = guarded_out(db0)
        G.ops.wgrad(dY, X, dW, db if with_db else None)
        return {"dW": dW, "db": db, "wbuf": wbuf, "bbuf": bbuf}
    out, again, fast = run_forms(run, form, fast_form)
    bars = {"dW": bound, "db": bound_db} if with_db else {"dW": bound}
    rec = form_record(out, again, fast, bars, -(-M // (128 * wgrad_slabs(M, N, K))) > 1)
    assert out_guards_intact(out["wbuf"], out["bbuf"]), "wgrad wrote outside dW / db"
    check_dense(f"{name}{form_key(form)}", out["dW"], want, bound, **extra, **rec)
    if with_db:
        db_name = name.replace("wgrad[", "wgrad_db[") if "[" in name else name + "_db"
        check_dense(f"{db_name}{form_key(form)}", out["db"], want_db, bound_db)
    else:
        assert torch.equal(out["db"], db0)
    assert_forms(rec)


def wgrad_inputs(M, N, K):
    torch.manual_seed(M + N)
    dY = torch.randn(M, N, device="cuda")
    X = torch.randn(M, K, device="cuda")
    dW0 = torch.randn(N, K, device="cuda")
    db0 = torch.randn(N, device="cuda")
    return dY, X, dW0, db0


@pytest.mark.parametrize("M,N,K,with_db,slabs", [(BIG_M, 68, 68, True, 8), (70001, 200, 12, True, 4), (40000, 12, 200, False, 2),
                                                  (200, 68, 68, False, 1), (200, 12, 200, True, 1)])
def test_wgrad(G, M, N, K, with_db, slabs):
    """dW[N][K] += dY^T X and db[N] += colsum(dY) (both prefilled) at row counts that take 8, 4, 2 and 1 slabs per block."""
    assert wgrad_slabs(M, N, K) == slabs
    wgrad_case(G, f"wgrad[M{M}-N{N}-K{K}]", *wgrad_inputs(M, N, K), with_db, form="fast", slabs=slabs)


def wgrad_cancellation_inputs():
    torch.manual_seed(79)
    M, N, K = 70001, 68, 200
    dY = torch.randn(M, N, device="cuda", dtype=torch.float64)
    dY = (dY - dY.mean(0, keepdim=True)).float()
    X = 40 + torch.randn(M, K, device="cuda")
    return dY, X, torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")


def test_wgrad_cancellation(G):
    """dY with zero column mean, X with a large positive mean: the bound against |dY|^T |X|."""
    wgrad_case(G, "wgrad_cancellation", *wgrad_cancellation_inputs(), True, form="fast")


def colsum_ref(Y, out0):
    M = Y.shape[0]
    return out0.double() + Y.double().sum(0), gam(M) * (out0.double().abs() + Y.double().abs().sum(0))


def colsum_case(G, M, N, form="fast", fast_form=None):
    torch.manual_seed(M + N)
    Y = torch.randn(M, N, device="cuda")
    out0 = torch.randn(N, device="cuda")
    want, bound = colsum_ref(Y, out0)

    def run():
        buf, out = guarded_out(out0)
        G.ops.colsum(Y, out)
        return {"out": out, "buf": buf}
    out, again, fast = run_forms(run, form, fast_form)
    rec = form_record(out, again, fast, {"out": bound}, M > (64 if N <= 256 and M < 262144 else 256))
    assert out_guards_intact(out["buf"]), "colsum wrote outside out"
    check_dense(f"colsum[M{M}-N{N}]{form_key(form)}", out["out"], want, bound, **rec)
    assert_forms(rec)


@pytest.mark.parametrize("M,N", [(200, 1), (1000, 3), (5000, 68), (262143, 5), (262144, 4), (300000, 12), (3000, 300),
                                 (700, 257)])
def test_colsum(G, M, N):
    """out[n] += sum_m Y[m][n] (prefilled) with 64 or 256 rows per block (M below / above 262144, N above 256)."""
    colsum_case(G, M, N, form="fast")


def batch_rowsum_ref(Y, B, L):
    Yb = Y.double().view(B, L, -1)
    return Yb.sum(1), gam(L) * Yb.abs().sum(1)


def batch_rowsum_case(G, L, C, B=3, form="fast", fast_form=None):
    torch.manual_seed(L + C)
    Y = torch.randn(B * L, C, device="cuda")
    want, bound = batch_rowsum_ref(Y, B, L)

    def run():
        buf, out = guarded_out(torch.full((B, C), SENTINEL))          # the call's own memset must clear it
        G.ops.batch_rowsum(Y, B, L, out)
        return {"out": out, "buf": buf}
    out, again, fast = run_forms(run, form, fast_form)
    rec = form_record(out, again, fast, {"out": bound}, L > 64)
    assert out_guards_intact(out["buf"]), "batch_rowsum wrote outside out"
    name = f"batch_rowsum[L{L}-C{C}]" if B == 3 else f"batch_rowsum[B{B}-L{L}-C{C}]"
    check_dense(f"{name}{form_key(form)}", out["out"], want, bound, **rec)
    assert_forms(rec)


@pytest.mark.parametrize("L,C", [(77, 12), (200, 300), (1000, 1), (63, 68)])
def test_batch_rowsum(G, L, C):
    """out[b][c] = sum_l Y[b L + l][c] over B = 3 batches, L not a multiple of 64."""
    batch_rowsum_case(G, L, C, form="fast")
