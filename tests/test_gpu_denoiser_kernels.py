"""The sampler's fused denoiser kernels -- the layer kernel (gsdd_d3pm_layer, both variants, all three instantiations), the K/V
attention images it writes, the logits kernel (gsdd_d3pm_logits) and gsdd_rows_linear -- against a plain fp64 evaluation of the same
operation, element by element, at the shapes the sampler launches.

Both fused kernels are persistent (at most 256 workgroups): a layer wave takes a second 32-row group, and a logits block a second
256-row tile, only above M = 65,536.  The two-lane sampler runs exactly M = 65,536, the one-lane sampler 131,072, so the cases below
run both, plus shapes that reach one second group only (M = 65,568), ragged batch lengths (L % 32 != 0, groups that span two batch
elements, a 4-row last group), ragged class counts (K % 64 != 0, odd chunk counts) and a partial second logits tile.

Reference: layer_ref() evaluates what LayerArgs defines (csrc/d3pm_layer.hip), in fp64 on the device, in row chunks:
    x1 = x + y Wproj^T + bproj + cvec[b]                 (b = row // L; no cvec: 0)
    x2 = x1 + W2 GELU2(W1 LN2(x1) + b1) + b2             (y = None, the q|k|v-only stage of block 0: x2 = x)
    qkv = Wqkv AdaLN(x2, ada[t2[b]]) + bqkv              (nxt = None, the last block: no q|k|v)

Error bar, per output element, carried stage by stage (U = 2^-24, gamma(K) = U (8 + 2 sqrt(K)) as in test_gpu_gemm_family):
  * a GEMM stage out = W a + bias contributes (unit + gamma(K)) (|a| (*) |W| + |bias|) + its input's bar propagated, |W| (*) e_a.
    unit is the operand format's error per product:
      h2   12 U: a and w are f16 hi + lo pairs (22 bits each, 2^-22 relative from rounding the lo piece, for each operand) and the
           lo.lo product is dropped (2^-22 of the product).  Add the loss where a lo (or hi) piece is subnormal: the matrix pipe does
           not keep subnormal f16 operands, and the kernel scales weights by 2^8 and activations by 2^4 to keep them rare, so the
           loss is below 2^-14 in the scaled operand, i.e. 2^-22 absolute per weight and 2^-18 absolute per activation:
           + 2^-18 sum_k |W| + 2^-22 sum_k |a|;
      x3p  U: three bf16 pieces keep 27 bits; the dropped products a2 b3 + a3 b2 + a3 b3 are below 2^-26 |a||w|; what is left is the
           final f32 rounding, as in gemm.hip.
  * the residual adds round once each: x1 gets 3 U (|x| + |proj term| + |cvec|), x2 gets 2 U (|x1| + |mlp term|).
  * LayerNorm / AdaLN (gamma, beta per row for AdaLN): an upstream bar e with row maximum E moves output j by at most
    rstd |gamma_j| (e_j + (1 + |xhat_j|) E) (the Jacobian's three terms; mean |xhat| <= 1); the normalisation itself adds
    rstd |gamma| gamma(64) mean|x| (the mean's rounding) + (8 U + gamma(64)) |xhat gamma| + 2 U |beta|.
  * GELU2 has slope <= 1.1, so its input's bar grows by 1.1; it runs on the bare v_exp_f32 / v_rcp_f32 (1 ulp each) with one
    rounding of the exponent argument: + 8 U |GELU2(z)| + U.
The logits kernel (exact-f32 MFMA) is held to the GEMM family's LN-prologue bar:
    gamma(64) (sum_k (|(x - mu) rstd gamma| + |beta|)_k |w_nk| + |b_n|),
and gsdd_rows_linear to gamma(K) (|x| (*) |W| + |bias| + |bvec| + |residual|).

Worst measured error / bound ratios on an MI355X (parity report, denoiser_kernels::*): layer x 0.005 (h2) / 0.018 (x3p), q|k|v 0.03
(h2) / 0.08 (x3p); the V image 0.07; key sums 0.12; attention on the images 6.5e-6 of its 2e-5 bar; rows_linear 0.17; logits 0.46,
the largest.  The layer bars are loose by two orders of magnitude (the row maximum E carried through LayerNorm and the absolute
subnormal terms dominate; an emulation of the h2 and x3p operand formats on the CPU gives 0.005 for x), and are first-order; what they
are meant to catch -- a wrong row, batch element, cvec / AdaLN row or tile -- is many orders of magnitude above them.

Besides the bars: unwritten memory is filled with a sentinel (NaN guard rows past M for x and y, so a read past M would also trip the
range screen) and checked bit for bit; the result of a row must not depend on which wave computes it (one M = 131,072 launch against
its two halves, bit for bit, including the K / V images and the per-tile key norms and sums); the layer kernel's K image, key norms and
key sums must be the bytes the attention kernel's own pre-split pass writes from the same f32 k rows, its V image must meet the v bar
(it is taken from the transposed product, whose piece products are accumulated in another order than the row path's: the values
differ from the f32 rows in the last bit, as measured; with the row path's order the bytes are identical), and the attention kernel
must read the images correctly at the one-lane batch (B2 = 32)."""
import math

import pytest
import torch

from tests.conftest import parity_report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H, D, HID, T = 16, 64, 256, 100
SENTINEL = -7777.0
UNITS = {"h2": (12 * U, 2.0 ** -18, 2.0 ** -22), "x3p": (U, 0.0, 0.0)}     # (unit per product, abs. loss per activation, per weight)
CHUNK = 16384


def gam(k):
    return U * (8 + 2 * math.sqrt(k))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()          # fail loudly if libgsdd.so is missing
    return gsdd_amd


def cgen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ----------------------------------------------------------------------------- fp64 reference of the layer descriptor
def gemm_stage(a, ea, w, b, unit, abs_a, abs_w):
    """fp64 (out, |a| (*) |W| + |b|, bar) of a W^T + b for rows a [R][K] whose own bar is ea (None: exact inputs)"""
    w = w.double()
    aw = w.abs()
    out = a @ w.t() + b.double()
    mag = a.abs() @ aw.t() + b.double().abs()
    bar = (unit + gam(w.shape[1])) * mag
    if abs_a or abs_w:
        bar = bar + abs_a * aw.sum(1) + abs_w * a.abs().sum(1, keepdim=True)
    if ea is not None:
        bar = bar + ea @ aw.t()
    return out, mag, bar


def ln_stage(v, ev, g, b):
    """fp64 LayerNorm (eps 1e-5) with per-feature or per-row affine, and its bar (module docstring)"""
    mu = v.mean(1, keepdim=True)
    d = v - mu
    rs = (d.square().mean(1, keepdim=True) + 1e-5).rsqrt()
    xh = d * rs
    t = xh * g
    ga = rs * g.abs()
    bar = ga * gam(64) * v.abs().mean(1, keepdim=True) + (8 * U + gam(64)) * t.abs() + 2 * U * b.abs()
    if ev is not None:
        bar = bar + ga * (ev + (1 + xh.abs()) * ev.amax(1, keepdim=True))
    return t + b, bar


def gelu_stage(z, ez):
    gz = z * torch.sigmoid(1.702 * z)
    return gz, 1.1 * ez + 8 * U * gz.abs() + U


def layer_ref(x, y, L, lay, cvec, nxt, t2, variant, r0, r1):
    """fp64 {'x': (want, bar) [R][64], 'qkv': (want, bar) [R][192] (feature n of row m: qkv[n >> 2][m][n & 3])} of rows r0 .. r1 of
    the layer descriptor: y = None is the q|k|v-only stage (x unchanged), nxt = None the last block (no q|k|v), cvec may be None."""
    unit, abs_a, abs_w = UNITS[variant]
    f = lambda k_, l_: l_[k_].double()
    xs = x[r0:r1].double()
    bidx = torch.arange(r0, r1, device=x.device) // L
    res = {}
    if y is not None:
        p, pmag, ep = gemm_stage(y[r0:r1].double(), None, lay["wproj"], lay["bproj"], unit, abs_a, abs_w)
        cv = cvec.double()[bidx] if cvec is not None else torch.zeros_like(xs)
        x1 = xs + p + cv
        ex1 = ep + 3 * U * (xs.abs() + pmag + cv.abs())
        hn, ehn = ln_stage(x1, ex1, f("g2", lay), f("b2", lay))
        z, _, ez = gemm_stage(hn, ehn, lay["w1"], lay["bb1"], unit, abs_a, abs_w)
        gz, egz = gelu_stage(z, ez)
        mlp, mmag, emlp = gemm_stage(gz, egz, lay["w2"], lay["bb2"], unit, abs_a, abs_w)
        x2 = x1 + mlp
        ex2 = ex1 + emlp + 2 * U * (x1.abs() + mmag)
        res["x"] = (x2, ex2)
    else:
        x2, ex2 = xs, None
    if nxt is not None:
        tab = f("ada1", nxt)[t2[bidx]]
        an, ean = ln_stage(x2, ex2, tab[:, :D], tab[:, D:])
        q, _, eq = gemm_stage(an, ean, nxt["wqkv"], nxt["bqkv"], unit, abs_a, abs_w)
        res["qkv"] = (q, eq)
    return res


def ratio_of(err, bound):
    inf = torch.full_like(err, float("inf"))
    return torch.where(bound > 0, err / bound, torch.where(err > 0, inf, torch.zeros_like(err)))


# ----------------------------------------------------------------------------- operands
def make_layer(G, seed=7):
    """trained-scale weights (as full_d3pm(scale_weights=True)): W ~ N(0, 1/fan_in), biases 0.1 N(0, 1), LayerNorm / AdaLN affine
    around (1, 0); both variants' weight images"""
    g = torch.Generator().manual_seed(seed)
    lin = lambda n, k: (torch.randn(n, k, generator=g) / math.sqrt(k), 0.1 * torch.randn(n, generator=g))
    wproj, bproj = lin(D, D)
    w1, bb1 = lin(HID, D)
    w2, bb2 = lin(D, HID)
    wqkv, bqkv = lin(3 * D, D)
    lay = dict(wproj=wproj, bproj=bproj, g2=1 + 0.3 * torch.randn(D, generator=g), b2=0.2 * torch.randn(D, generator=g),
               w1=w1, bb1=bb1, w2=w2, bb2=bb2)
    nxt = dict(ada1=torch.cat([1 + 0.3 * torch.randn(T, D, generator=g), 0.3 * torch.randn(T, D, generator=g)], 1),
               wqkv=wqkv, bqkv=bqkv)
    lay = {k: v.cuda().contiguous() for k, v in lay.items()}
    nxt = {k: v.cuda().contiguous() for k, v in nxt.items()}
    lay_h2, wqkv_h2 = G.ops.d3pm_layer_pack_h2(lay["w1"], lay["w2"], lay["wproj"], nxt["wqkv"])
    lay_x3, wqkv_x3 = G.ops.d3pm_layer_pack(lay["w2"], lay["wproj"], nxt["wqkv"])
    return ({"h2": dict(lay, lay_h2=lay_h2), "x3p": dict(lay, w2_x3=lay_x3)},
            {"h2": dict(nxt, wqkv_h2=wqkv_h2), "x3p": dict(nxt, wqkv_x3=wqkv_x3)})


@pytest.fixture(scope="module")
def P(G):
    return make_layer(G)


def make_rows(M, L, seed):
    """x, y [M][64] (y rows of mixed magnitude: 1e-3, where the f16 lo pieces go subnormal, up to ~100), cvec [B2][64] and t2 [B2],
    both different between neighbouring batch elements"""
    g = cgen(seed)
    B2 = -(-M // L)
    x = torch.randn(M, D, device="cuda", generator=g)
    scl = torch.ones(M, 1, device="cuda")
    scl[0::5] = 1e-3
    scl[3::11] = 30.0
    y = torch.randn(M, D, device="cuda", generator=g) * scl
    cvec = torch.randn(B2, D, device="cuda", generator=g) * 0.5
    t2 = (torch.arange(B2, device="cuda") * 37 + 5) % T
    return x, y, cvec, t2


def guarded(rows, fill, n_guard=64):
    """[rows][64] view at the front of a buffer whose `n_guard` following rows hold `fill`"""
    buf = torch.full((rows + n_guard, D), fill, device="cuda")
    return buf, buf[:rows]


def ws_parts(ws, M):
    """K image [16][M][8] (int32), V image [16][M / 32][256] (int32), key sums [16][M / 32][4], tile norms [16][M / 32] of an attention
    workspace for M rows of 16 heads (common.hpp: K | V | ksum | knorm)"""
    rows, nt = H * M, H * M // 32
    k = ws[:rows * 8].view(torch.int32).view(H, M, 8)
    v = ws[rows * 8:rows * 16].view(torch.int32).view(H, M // 32, 256)
    ks = ws[rows * 16:rows * 16 + 4 * nt].view(H, M // 32, 4)
    kn = ws[rows * 16 + 4 * nt:rows * 16 + 5 * nt].view(H, M // 32)
    return k, v, ks, kn


def run_layer(G, P, variant, inst, M, L, x_in, y_in, cvec, t2, kv_img=False):
    """one gsdd_d3pm_layer call on sentinel-guarded buffers; checks the guards and the range flag, returns (x, qkv, ws or None)"""
    lays, nxts = P
    xbuf, x = guarded(M, float("nan"))
    x.copy_(x_in)
    ybuf = y = None
    if inst != "qkv_only":
        ybuf, y = guarded(M, float("nan"))
        y.copy_(y_in)
    qkv = ws = wsbuf = None
    if inst != "no_qkv":
        qbuf = torch.full((3 * H * M * 4 + 4096,), SENTINEL, device="cuda")
        qkv = qbuf[:3 * H * M * 4].view(3 * H, M, 4)
        if kv_img:
            n = G.ops.d3pm_attention_workspace(M // L, L, H, "cuda").numel()
            wsbuf = torch.full((n + 1024,), SENTINEL, device="cuda")
            ws = wsbuf[:n]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    G.ops.d3pm_layer(y, x, L, None if inst == "qkv_only" else lays[variant], cvec=cvec,
                     nxt=None if inst == "no_qkv" else nxts[variant], t2=t2, qkv=qkv, kv_img=ws, range_flag=flag, variant=variant)
    torch.cuda.synchronize()
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    assert bool((xbuf[M:].view(torch.int32) == nan_bits).all()), "x written past row M"
    if ybuf is not None:
        assert bool((ybuf[M:].view(torch.int32) == nan_bits).all())
    if qkv is not None:
        assert bool((qbuf[3 * H * M * 4:] == SENTINEL).all()), "q|k|v written past its end"
        if kv_img:
            assert bool((qkv[H:] == SENTINEL).all()), "k / v rows written although images were requested"
            assert bool((wsbuf[n:] == SENTINEL).all()), "attention workspace written past its end"
    if inst == "qkv_only":
        assert torch.equal(x.view(torch.int32), x_in.view(torch.int32)), "the q|k|v-only stage changed x"
    return x, qkv, ws, int(flag.item())


def layer_worst(P, variant, inst, M, L, x_in, y_in, cvec, t2, x, qkv, skip_row=None):
    """worst error / bar ratio of x and q|k|v over all rows (skip_row: excluded), computed in row chunks"""
    lays, nxts = P
    worst = {"x": 0.0, "qkv": 0.0}
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        ref = layer_ref(x_in, None if inst == "qkv_only" else y_in, L, lays[variant], cvec, None if inst == "no_qkv" else nxts[variant],
                        t2, variant, r0, r1)
        got = {}
        if "x" in ref:
            got["x"] = x[r0:r1]
        if "qkv" in ref:
            got["qkv"] = qkv[:, r0:r1].permute(1, 0, 2).reshape(r1 - r0, 3 * D)
        for k_, (want, bar) in ref.items():
            g_ = got[k_].double()
            keep = torch.ones(r1 - r0, 1, dtype=torch.bool, device=g_.device)
            if skip_row is not None and r0 <= skip_row < r1:
                keep[skip_row - r0] = False
            assert bool((torch.isfinite(g_) | ~keep).all()), f"{k_}: non-finite outputs"
            r = torch.where(keep, ratio_of((g_ - want).abs(), bar), torch.zeros_like(bar))
            worst[k_] = max(worst[k_], float(r.max()))
    return worst


# ----------------------------------------------------------------------------- 3. every variant and instantiation at the sampler's shapes
LAYER_SHAPES = [(65536, 4096), (131072, 4096), (65568, 96), (69700, 4100)]


@pytest.mark.parametrize("M,L", LAYER_SHAPES, ids=[f"M{m}_L{l}" for m, l in LAYER_SHAPES])
@pytest.mark.parametrize("inst", ["has_qkv", "qkv_only", "no_qkv"])
@pytest.mark.parametrize("variant", ["h2", "x3p"])
def test_layer_kernel_vs_fp64(G, P, variant, inst, M, L):
    """65,536 rows (the lane shape: one group per wave), 131,072 (one lane: two groups per wave), 65,568 in batch elements of 96 (2049
    groups: block 0 wave 0 alone runs a second group, 683 distinct cvec / t2 rows) and 69,700 in batch elements of 4100 (L % 32 != 0:
    per-row cvec and AdaLN rows, groups across two batch elements, second groups and a 4-row last group)."""
    x_in, y_in, cvec, t2 = make_rows(M, L, seed=M + L)
    if inst == "no_qkv" and M == 65536:
        cvec = None                                     # (the descriptor's cvec = NULL)
    x, qkv, _, flag = run_layer(G, P, variant, inst, M, L, x_in, y_in, cvec, t2)
    worst = layer_worst(P, variant, inst, M, L, x_in, y_in, cvec, t2, x, qkv)
    parity_report(f"denoiser_kernels::layer[{variant}-{inst}-M{M}-L{L}]", dict(worst_ratio=max(worst.values()), **worst, M=M, L=L))
    assert flag == 0, "range flag raised on in-range operands"
    assert max(worst.values()) <= 1.0, worst


# ----------------------------------------------------------------------------- 4. bit identity across the grid-stride loop
def split_compare(name, full, halves, dim):
    a = torch.cat([h.contiguous() for h in halves], dim)
    assert torch.equal(full.contiguous().view(torch.int32), a.view(torch.int32)), f"{name}: a row's result depends on the wave that computes it"


@pytest.mark.parametrize("inst", ["has_qkv", "qkv_only"])
@pytest.mark.parametrize("variant", ["h2", "x3p"])
def test_layer_second_group_bit_identity(G, P, variant, inst):
    """M = 131,072 (every wave runs two groups) against its two halves as M = 65,536 launches (one group per wave), bit for bit: x, the
    q|k|v rows, and with images the K / V images, the per-tile key norms and key sums (re-indexed: row = head * M + m, tile = row / 32)."""
    M, L, half = 131072, 4096, 65536
    x_in, y_in, cvec, t2 = make_rows(M, L, seed=41)
    nb = half // L
    for kv in (False, True):
        x, qkv, ws, flag = run_layer(G, P, variant, inst, M, L, x_in, y_in, cvec, t2, kv_img=kv)
        parts = [run_layer(G, P, variant, inst, half, L, x_in[s:s + half].contiguous(), y_in[s:s + half].contiguous(),
                           cvec[s // L:s // L + nb].contiguous(), t2[s // L:s // L + nb].contiguous(), kv_img=kv)
                 for s in (0, half)]
        assert flag == 0 and all(p[3] == 0 for p in parts)
        split_compare("x", x, [p[0] for p in parts], 0)
        split_compare("q rows" if kv else "q|k|v rows", qkv[:H] if kv else qkv, [(p[1][:H] if kv else p[1]) for p in parts], 1)
        if kv:
            full = ws_parts(ws, M)
            hp = [ws_parts(p[2], half) for p in parts]
            for i, nm in enumerate(("K image", "V image", "key sums", "tile norms")):
                split_compare(nm, full[i], [h[i] for h in hp], 1)
    parity_report(f"denoiser_kernels::second_group_bit_identity[{variant}-{inst}]", dict(worst_ratio=0.0, M=M))


# ----------------------------------------------------------------------------- 5. the attention images at the production shape
def v_image_values(vimg, M):
    """V image [16][M / 32][256] int32 -> (values [16][M][4] in fp64: v1 + v2 2^-11 + v3 2^-22, constant columns [16][M][4] as f16 bits).
    Layout (common.hpp kv_image_store_v): per 32-key pair-tile, [key group g][column j] -> 8 f16 (tile th = key / 16, row r of group g:
    key = 16 th + 4 g + r)."""
    c = vimg.view(torch.float16).view(H, M // 32, 4, 16, 2, 4).permute(0, 1, 4, 2, 5, 3).reshape(H, M, 16)
    d = c.double()
    return d[..., 0:4] + d[..., 4:8] * 2.0 ** -11 + d[..., 8:12] * 2.0 ** -22, c[..., 12:16].contiguous().view(torch.int16)


def attention_sample_ref(q, k, v, B2, L, idx):
    """fp64 softmax attention (scale 1/2) of queries idx [B2][H][S] over the whole row of their (b, h); q, k, v head-major [16][M][4]"""
    hv = lambda z: z.view(H, B2, L, 4).permute(1, 0, 2, 3).double()
    qq, kk, vv = hv(q), hv(k), hv(v)
    qs = torch.gather(qq, 2, idx[..., None].expand(-1, -1, -1, 4))
    att = torch.softmax((qs @ kk.transpose(-1, -2)) * 0.5, dim=-1)
    return att @ vv                                                    # [B2][H][S][4]


@pytest.mark.parametrize("inst", ["has_qkv", "qkv_only"])
@pytest.mark.parametrize("variant", ["h2", "x3p"])
def test_layer_attention_images_production_shape(G, P, variant, inst):
    """M = 131,072, L = 4096: the layer kernel's K / V images are the bytes the attention kernel's pre-split pass writes from the same
    layer's f32 k / v rows; every tile norm bounds the stored keys from above within 1e-5; the key sums are within gamma(32) of fp64;
    and the attention kernel on those images, at B2 = 32, meets its 2e-5 bar against fp64 softmax attention for queries 0, L - 1 and
    three random ones of every (b, h)."""
    M, L = 131072, 4096
    B2 = M // L
    x_in, y_in, cvec, t2 = make_rows(M, L, seed=43)
    x_r, qkv_r, _, f1 = run_layer(G, P, variant, inst, M, L, x_in, y_in, cvec, t2)
    x_i, qkv_i, ws, f2 = run_layer(G, P, variant, inst, M, L, x_in, y_in, cvec, t2, kv_img=True)
    assert f1 == 0 and f2 == 0
    assert torch.equal(x_r.view(torch.int32), x_i.view(torch.int32)) and torch.equal(qkv_r[:H], qkv_i[:H])
    q, k, v = qkv_r[:H].contiguous(), qkv_r[H:2 * H].contiguous(), qkv_r[2 * H:].contiguous()
    ws_ref = G.ops.d3pm_attention_workspace(B2, L, H, "cuda")
    out_ref = torch.empty(M, D, device="cuda")
    G.ops.d3pm_attention(q, k, v, B2, L, H, out_ref, ws=ws_ref)      # the pre-split pass writes ws_ref from the f32 rows
    out = torch.empty(M, D, device="cuda")
    G.ops.d3pm_attention(q, None, None, B2, L, H, out, ws=ws)         # premade images
    torch.cuda.synchronize()
    mine, ref = ws_parts(ws, M), ws_parts(ws_ref, M)
    diff = {nm: int((a != b).sum()) for nm, a, b in zip(("k_image", "v_image", "ksum", "knorm"), mine, ref)}
    # tile norms and key sums against fp64 of the stored keys
    kt = k.double().view(H, M // 32, 32, 4)
    true_max = kt.norm(dim=-1).amax(dim=2)
    kn = mine[3].double()
    norm_ok = bool((kn >= true_max).all()) and bool((kn <= true_max * (1 + 1e-5) + 1e-30).all())
    ks_ratio = float(ratio_of((mine[2].double() - kt.sum(2)).abs(), gam(32) * kt.abs().sum(2)).max())
    # attention on the images vs fp64, sampled queries of every (b, h)
    g = cgen(47)
    idx = torch.cat([torch.zeros(B2, H, 1, dtype=torch.int64, device="cuda"), torch.full((B2, H, 1), L - 1, device="cuda"),
                     torch.randint(1, L - 1, (B2, H, 3), device="cuda", generator=g)], 2)
    want = attention_sample_ref(q, k, v, B2, L, idx)
    rows = torch.arange(B2, device="cuda")[:, None, None] * L + idx                          # [B2][H][S]
    cols = torch.arange(H, device="cuda")[None, :, None, None] * 4 + torch.arange(4, device="cuda")
    got = out[rows[..., None], cols].double()                                             # [B2][H][S][4]
    att_err = float((got - want).abs().max())
    # V: the image holds the layer's v from the product taken the other way round (activations as the A operand, so that a lane
    # holds eight rows of one column), whose piece products reach the f32 accumulator in another order than the row path's: its
    # values may differ from the f32 rows' in the last bits.  So the V image is held to the layer's fp64 bar (the q|k|v bar of the
    # v features) and its constant columns must be the pre-split pass's.
    v_img, cst_img = v_image_values(mine[1], M)
    v_pre, cst_pre = v_image_values(ref[1], M)
    v_rows = v.double()
    v_ratio = 0.0
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        lays, nxts = P
        want_v, bar_v = layer_ref(x_in, None if inst == "qkv_only" else y_in, L, lays[variant], cvec, nxts[variant], t2, variant,
                                  r0, r1)["qkv"]
        want_v = want_v[:, 2 * D:].reshape(r1 - r0, H, 4).permute(1, 0, 2)
        bar_v = bar_v[:, 2 * D:].reshape(r1 - r0, H, 4).permute(1, 0, 2)
        v_ratio = max(v_ratio, float(ratio_of((v_img[:, r0:r1] - want_v).abs(), bar_v).max()))
    v_pre_exact = bool((v_pre == v_rows).all())
    v_dev = float((v_img - v_rows).abs().max())
    parity_report(f"denoiser_kernels::attention_images[{variant}-{inst}]",
                  dict(worst_ratio=max(att_err / 2e-5, ks_ratio, v_ratio), attn_err=att_err, ksum_ratio=ks_ratio, v_ratio=v_ratio,
                       v_max_dev_from_rows=v_dev, v_values_differing=int((v_img != v_rows).sum()), differing_words=diff))
    assert diff["k_image"] == 0, diff
    assert norm_ok, "a tile norm is below the largest stored key norm, or more than 1e-5 above it"
    assert ks_ratio <= 1.0 and diff["ksum"] == 0 and diff["knorm"] == 0, (ks_ratio, diff)
    assert att_err < 2e-5, att_err
    assert torch.equal(cst_img, cst_pre), "V image: constant columns differ from the pre-split pass's"
    assert v_pre_exact, "the pre-split pass's V image does not decode to the f32 rows"
    assert v_ratio <= 1.0, (v_ratio, v_dev)


# ----------------------------------------------------------------------------- 6. the range screen inside the grid-stride loop
@pytest.mark.parametrize("M,L,row", [(131072, 4096, 65536 + 4097), (69700, 4100, 69698)], ids=["second_group", "ragged_last_group"])
def test_layer_range_screen_second_group(G, P, M, L, row):
    """One row of y at 1e4 (16 a overflows f16) in a wave's second group / in the 4-row last group: the flag is set, every other row
    still meets its bar (the overflow does not leak), and the NaN guard rows past M (run_layer) never set it on their own."""
    x_in, y_in, cvec, t2 = make_rows(M, L, seed=53)
    y_in[row] = 1e4
    x, qkv, _, flag = run_layer(G, P, "h2", "has_qkv", M, L, x_in, y_in, cvec, t2)
    worst = layer_worst(P, "h2", "has_qkv", M, L, x_in, y_in, cvec, t2, x, qkv, skip_row=row)
    parity_report(f"denoiser_kernels::range_screen[M{M}-row{row}]", dict(worst_ratio=max(worst.values()), **worst, flag=flag))
    assert flag == 1, "the range screen missed an overflowing row"
    assert max(worst.values()) <= 1.0, worst


# ----------------------------------------------------------------------------- 7. the logits kernel
def logits_operands(M, K, seed):
    g = cgen(seed)
    xbuf, x = guarded(M, float("nan"))
    x.copy_(torch.randn(M, D, device="cuda", generator=g) * (0.5 + torch.rand(M, 1, device="cuda", generator=g) * 4)
            + torch.randn(M, 1, device="cuda", generator=g))
    lg = 1 + 0.3 * torch.randn(D, device="cuda", generator=g)
    lb = 0.2 * torch.randn(D, device="cuda", generator=g)
    w = torch.randn(K, D, device="cuda", generator=g) / 8
    bias = 0.1 * torch.randn(K, device="cuda", generator=g)
    return x, lg, lb, w, bias


def run_logits(G, x, lg, lb, w, bias):
    M, K = x.shape[0], w.shape[0]
    obuf = torch.full(((M + 40) * K,), SENTINEL, device="cuda")
    out = obuf[:M * K].view(M, K)
    G.ops.d3pm_logits(x, lg, lb, w, bias, out)
    torch.cuda.synchronize()
    assert bool((obuf[M * K:] == SENTINEL).all()), "logits written past row M"
    return out


LOGIT_CASES = [(m, k) for m in (131072, 65736) for k in (4096, 1028, 4160, 32)]


@pytest.mark.parametrize("M,K", LOGIT_CASES, ids=[f"M{m}_K{k}" for m, k in LOGIT_CASES])
def test_logits_kernel_vs_fp64(G, M, K):
    """K = 4096 (production), 1028 (5 chunks, a last chunk of 4 classes on the masked store path), 4160 (17 chunks, a partial last
    chunk on the full-tile path), 32 (narrower than a sub-chunk); M = 131,072 (every block runs two tiles) and 65,736 (257 tiles:
    block 0's second tile is partial, one wave partly and one wholly past M)."""
    x, lg, lb, w, bias = logits_operands(M, K, seed=M + K)
    out = run_logits(G, x, lg, lb, w, bias)
    w64, b64 = w.double(), bias.double()
    worst = 0.0
    step = max(1024, (1 << 24) // K)
    for r0 in range(0, M, step):
        xs = x[r0:r0 + step].double()
        mu = xs.mean(1, keepdim=True)
        t = (xs - mu) * (xs.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() * lg.double()
        a, aa = t + lb.double(), t.abs() + lb.double().abs()
        want = a @ w64.t() + b64
        bar = gam(D) * (aa @ w64.abs().t() + b64.abs())
        g_ = out[r0:r0 + step].double()
        assert bool(torch.isfinite(g_).all()), "non-finite logits"
        worst = max(worst, float(ratio_of((g_ - want).abs(), bar).max()))
    parity_report(f"denoiser_kernels::logits[M{M}-K{K}]", dict(worst_ratio=worst, M=M, K=K))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("K", [4096, 1028])
def test_logits_second_tile_bit_identity(G, K):
    """M = 131,072 (two tiles per block) against its halves (one tile per block), bit for bit"""
    M, half = 131072, 65536
    x, lg, lb, w, bias = logits_operands(M, K, seed=59 + K)
    full = run_logits(G, x, lg, lb, w, bias)
    halves = [run_logits(G, x[s:s + half].contiguous(), lg, lb, w, bias) for s in (0, half)]
    split_compare("logits", full, halves, 0)
    parity_report(f"denoiser_kernels::logits_second_tile_bit_identity[K{K}]", dict(worst_ratio=0.0, M=M, K=K))


# ----------------------------------------------------------------------------- 8. gsdd_rows_linear: a second, partial group per wave
@pytest.mark.parametrize("n_in,n_out", [(64, 192), (256, 64)], ids=["KC1", "NB1"])
def test_rows_linear_second_group(G, n_in, n_out):
    """M = 65,536 + 120: the grid-stride loop of both kernel shape classes (KC = 1, NB = 1) runs a second group, partly past M, with the
    per-batch vector and residual epilogue; each element against gamma(K) of its magnitude, rows past M untouched."""
    import numpy as np
    ops = G.ops
    M, Bn = 65536 + 120, 8
    Lb = M // Bn
    g = cgen(n_in + n_out)
    x = torch.randn(M, n_in, device="cuda", generator=g) * (0.1 + 3 * torch.rand(M, 1, device="cuda", generator=g))
    w = torch.randn(n_out, n_in, device="cuda", generator=g) / math.sqrt(n_in)
    bias = torch.randn(n_out, device="cuda", generator=g)
    bvec = torch.randn(Bn, n_out, device="cuda", generator=g)
    res = torch.randn(M, n_out, device="cuda", generator=g)
    img = torch.empty((ops.rows_linear_image_bytes(n_out, n_in),), dtype=torch.uint8, device="cuda")
    table = np.array([(w.data_ptr(), n_out, n_in, n_in, 0, img.data_ptr())],
                     dtype=np.dtype([("w", "<u8"), ("n_out", "<i4"), ("n_in", "<i4"), ("ld", "<i4"), ("transpose", "<i4"), ("img", "<u8")]))
    ops.rows_linear_pack_many(torch.from_numpy(table.view(np.uint8).copy()).cuda(), 1, n_out, n_in)
    obuf = torch.full(((M + 64) * n_out,), SENTINEL, device="cuda")
    out = obuf[:M * n_out].view(M, n_out)
    ops.rows_linear(x, img, n_out, out, bias=bias, bvec=bvec, rows_per_batch=Lb, residual=res)
    torch.cuda.synchronize()
    assert bool((obuf[M * n_out:] == SENTINEL).all()), "rows_linear wrote past row M"
    bv = bvec.double()[torch.arange(M, device="cuda") // Lb]
    want = x.double() @ w.double().t() + bias.double() + bv + res.double()
    bar = gam(n_in) * (x.double().abs() @ w.double().abs().t() + bias.double().abs() + bv.abs() + res.double().abs())
    assert bool(torch.isfinite(out).all())
    worst = float(ratio_of((out.double() - want).abs(), bar).max())
    parity_report(f"denoiser_kernels::rows_linear_second_group[{n_in}x{n_out}]", dict(worst_ratio=worst, M=M))
    assert worst <= 1.0, worst
