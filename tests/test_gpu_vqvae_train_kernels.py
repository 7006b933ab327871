"""The VQ-VAE training step's own kernels -- train-mode BatchNorm statistics (bn_train), the BatchNorm + ReLU backward (bn_relu_bwd),
relu_mask, lincomb, the mean-squared-error reduction and the codebook EMA statistics / update / perplexity -- against a plain fp64
evaluation of the same operation, element by element, at the batch-64 shapes of config C2 (M = 64 x 16 x 16 x 16 = 262,144 latent rows of
256 or 128 channels, 50,331,648 reconstruction elements, 2^30 elements of the largest saved decoder activation, K = 4096 codes of E = 128)
and at the shapes where their index arithmetic changes (M = 1, 63, 64, 65 and 64 x 256 + 37 rows: one slab, a ragged slab, more than 256
stage-1 blocks; C = 4, 48, 260, 512: the channel loop past 256 threads; E = 4, 12, 128).  The whole-model tests (test_gpu_vqvae_training,
test_gpu_fullsize_training) reach these kernels at batch 1-3 with a flat relative bar, or assert only that the loss falls.

The references are computed in fp64 on the device the inputs live on.  The unmarked tests at the end need no GPU: a plain-torch emulation of
each kernel's arithmetic (f32 where the kernel rounds to f32, fp64 where it uses double) must meet the same bars on the small shapes, and
must miss them with one fault injected at a time -- the bars are neither unreachable nor vacuous.

Bars, per output element.  U = 2^-24, u = 2^-53; gamma(k) = U (8 + 2 sqrt(k)) for an f32 sum of k terms (as in test_gpu_gemm_family); |.|
is of the exact (fp64) values; a "prefill" is the nonzero value an accumulating output held before the call; sqrtf, division, logf and expf
are taken at 2 ulp (4 U relative), every other f32 operation as correctly rounded (U).
  * Two-stage fp64 reductions (bn_train, bn_relu_bwd): 64 rows serially per slab, ceil(nblk / 256) slabs serially per thread, a 64-lane
    butterfly (6) and 3 adds over the waves: depth dep = 64 + ceil(nblk / 256) + 9, so a sum S = sum t carries dep u sum |t|.
  * bn_train: s = sum x and q = sum x^2 (x^2 exact in fp64) carry dep u sum |x| and dep u q.  mean = s / M: e_mean = U |mean| + dep u
    mean|x| after the cast to f32.  The one-pass variance q / M - mean^2 rounds q / M, mean^2 (twice the relative error of mean) and the
    difference, all of size q / M (|mean| mean|x| <= q / M): dv64 = c u q / M with c = 3 dep + 8 -- relative to var this is the
    cancellation term c u (q / M) / var, the whole cost of the one-pass formula.  The cast to f32 and the addition of eps add 2 U (var +
    eps); sqrtf and the division 4 U: r = (dv64 + 2 U (var + eps)) / (2 (var + eps)) + 4 U is the relative bar of rstd and of scale = w
    rstd.  shift = b - mean scale: |scale| e_mean + |mean scale| (r + U) + U |shift|.
    running_mean' = (1 - m) rm + m mean: U |(1 - m) rm| + m e_mean + U |m mean| + U |rm'| (m and 1 - m as the f32 values the kernel
    forms); running_var' likewise with unb = var M / max(M - 1, 1) carrying dv64 M / max(M - 1, 1) + U unb.  M = 1 has var = unb = 0.
    Beside the bars each case records the kernel's worst relative rstd error next to that of torch's own f32 batch_norm on the same
    device tensor (both against fp64); in the input families (spread O(1), |mean| / std = 0, 10, 100, mixed scales, and a hard one with
    mean^2 / var = 4e8) the kernel must be within 2 x of torch's: two independent f32 evaluations differ by about that much.
  * bn_relu_bwd with the kernel's inputs (the f32 mean_rstd of bn_train taken as exact): xh = (x - mu) rs carries 2 U |xh|.
    y = g xh + b decides the mask.  Evaluated as the backward does (g ((x - mu) rs) + b) it carries 3 U |g xh| + U |y|; as the GEMM
    prologue does (fma(x, scale, shift), scale = w / sqrtf(var + eps) against g rs: two divisions, 4 U; shift = b - fl(mu scale)) it
    carries 4 U |g xh| + U |mu g rs| + U |b - mu g rs| + U |y|.  e_y is the larger (the second), times 1 + 8 U for the second-order terms.
    An element with |y| <= e_y is *undecided*: dx there must match the masked or the unmasked candidate, and the sums of its channel
    widen by A1 = sum |da|, A2 = sum |da xh| over the channel's undecided elements.  The share of undecided elements must be <= 1e-4.
    S1 = sum dy (exact f32 terms, fp64 sum, cast): e_1 = dep u sum |dy| + U |S1| + A1; S2 = sum dy xh (f32 products of the rounded xh:
    3 U per term): e_2 = (3 U + dep u) sum |dy xh| + U |S2| + A2.  dbeta += S1: e_1 + U |S1| + 2 U |prefill|; dgamma += S2 likewise.
    dx = dx_in + g rs (dy - S1 / M - xh S2 / M) in f32 with invM = 1.f / (float)M (U) and the f32-rounded sums: m1 = S1 invM carries
    e_1 / M + 2 U |m1|, xh S2 invM carries |xh| e_2 / M + 5 U |xh m2|; the two subtractions U (|dy| + |m1|) + U (|dy| + |m1| + |xh m2|);
    g rs and its product with the bracket 2 U of the result; the final add U |dx|:
    bar |g rs| (6 U (|dy| + |m1|) + 8 U |xh m2| + e_1 / M + |xh| e_2 / M) + U |dx|.
  * relu_mask: a select; equal bit for bit to torch.where(out > 0, dout, 0).
  * lincomb, out = a + alpha (b - c): U |alpha| |b - c| + U |alpha (b - c)| + U |out| (one rounding less with fma contraction).
  * mse: d = a - b carries U |d|, d d then 3 U d^2; fp64 sums; scale / n in fp64; one cast: 3 U sum d^2 scale / n + U |result|.
  * codebook statistics: n_total = bincount exactly (float atomics of 1.0 below 2^24); encode_sum[k] within gamma(n_k) sum |z| over
    the rows of code k; rows of codes that do not occur exactly zero.
  * codebook update (d = 0.99f, 1 - d exact in f32; n_total and encode_sum taken as exact inputs): N' = N d + (1 - d) n_total: b_N = U (|N
    d| + |(1 - d) n_total| + |N'|); z_avg' likewise.  n = sum N' (fp64 sum of the f32 values, cast): b_n = sum b_N + U n.
    w = (N' + 1e-7f) / (n + K 1e-7f) n: r_w = b_N / (N' + 1e-7) + 2 b_n / n + 8 U; emb = z_avg' / w: b_za / w + |emb| (r_w + 4 U).
    usage = [N' >= 1] is decided in fp64 for every code at least 4 ulp (of 1) from the threshold (b_N < 2 ulp there); one more code
    is given an (N, n_total) pair that every evaluation order of the f32 expression, fused or not, puts on 1.0f exactly: kept.  A
    restarted code has embeddings[k] = z[perm[k]] bit for bit while z_avg[k] carries the EMA value.
  * perplexity exp(-sum p log(p + 1e-10f)), p = n_k / M: p carries 2 U p, the argument of logf then 3 U relative, logf 4 U |L|, the product U:
    per term p (3 U + 7 U |L|); fp64 sum h, cast (U |h|), expf (4 U): bar perp (sum p (3 U + 7 U |L|) + U |h| + 4 U).
Every GPU case records its worst error / bar ratio with tests.conftest.parity_report (vqvae_train_kernels::*).

Memory the kernels must not write is filled with a sentinel and checked bit for bit: around every output, and around every workspace,
which is given exactly the number of bytes the *_workspace_bytes function returns (8192 for mse)."""
import math
import types

import numpy as np
import pytest
import torch

from tests.conftest import parity_report

gpu = pytest.mark.gpu

U = 2.0 ** -24
U64 = 2.0 ** -53
SENT = -7777.0
FULL_M = 64 * 16 * 16 * 16
RAGGED_M = 64 * 256 + 37


def gam(k):
    return U * (8 + 2 * np.sqrt(np.asarray(k, dtype=np.float64)))


def gamt(k):
    """gamma(k) for a tensor of term counts"""
    return U * (8 + 2 * torch.sqrt(k.double()))


def f32(v):
    return float(np.float32(v))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ratio(got, want, bar, alt=None):
    """worst |got - want| / bar (a non-finite result counts as infinitely wrong); with `alt`, the nearer of the two candidates counts"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    if alt is not None:
        err = torch.minimum(err, (got - alt).abs())
    if err.numel() == 0:
        return 0.0
    return float(torch.where(err == 0, 0.0, err / bar).max())


def guarded(n_before, shape, n_after, fill, dev="cuda", dtype=torch.float32):
    """-> (buffer, view): a contiguous view of `shape` with n_before / n_after sentinel elements around it, the view holding `fill`"""
    n = int(np.prod(shape))
    buf = torch.full((n_before + n + n_after,), SENT, dtype=dtype, device=dev)
    v = buf[n_before:n_before + n].view(shape)
    if fill is not None:
        v.copy_(fill) if torch.is_tensor(fill) else v.fill_(fill)
    return buf, v


def guards_intact(buf, n_before, n, n_after):
    return bool((buf[:n_before] == SENT).all()) and bool((buf[n_before + n:] == SENT).all())


def depth(M):
    nblk = (M + 63) // 64
    return 64 + (nblk + 255) // 256 + 9


# ----------------------------------------------------------------------------- inputs of the BatchNorm pair
BN_FAMILIES = ["unit", "m10", "m100", "mixed", "hard"]


def bn_family(name, M, C, seed, dev):
    """rows x[M][C] as the res-stack feeds BatchNorm: spread O(1) with |mean| / std = 0, 10, 100 per channel, mixed spreads 1e-2 .. 1e2
    with |mean| / std up to 100, and the hard family: mean +-1000 beside std 0.05 (mean^2 / var = 4e8).  Channel 0 is constant (var = 0),
    channel 1 all zero."""
    g = gen(seed, dev)
    x = torch.randn(M, C, generator=g, device=dev)
    ch = torch.arange(C, device=dev)
    sign = torch.where(ch % 2 == 0, 1.0, -1.0)
    if name == "unit":
        sd, mu = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    elif name == "m10":
        sd = torch.ones(C, device=dev)
        mu = 10.0 * sign
    elif name == "m100":
        sd = 0.5 + (ch % 7).float() / 4
        mu = 100.0 * sd * sign
    elif name == "mixed":
        sd = 10.0 ** ((ch % 5).float() - 2)
        mu = sd * (ch % 11).float() * 10.0 * sign
    else:
        sd = torch.full((C,), 0.05, device=dev)
        mu = 1000.0 * sign
    x = x * sd + mu
    x[:, 0] = 3.25
    x[:, 1] = 0.0
    return x.contiguous()


def bn_params(C, seed, dev):
    """-> weight, bias, running_mean, running_var (bias +-0.5 on the constant and the all-zero channel: their mask is the bias's sign)"""
    g = gen(seed, dev)
    w = (0.5 + torch.rand(C, generator=g, device=dev)) * torch.where(torch.rand(C, generator=g, device=dev) < 0.25, -1.0, 1.0)
    b = torch.randn(C, generator=g, device=dev) * 0.5
    b[0], b[1] = 0.5, -0.5
    rm = torch.randn(C, generator=g, device=dev)
    rv = torch.rand(C, generator=g, device=dev) + 0.5
    return w, b, rm, rv


def bn_train_ref(x, w, b, rm, rv, eps=1e-5, mom=0.1):
    """fp64 two-pass reference of bn_train and its bars -> {name: (want, bar)}"""
    M = x.shape[0]
    xd = x.double()
    mean = xd.mean(0)
    var = (xd - mean).square().mean(0)
    q = xd.square().mean(0)
    dep = depth(M)
    e_mean = U * mean.abs() + dep * U64 * xd.abs().mean(0)
    dv64 = (3 * dep + 8) * U64 * q
    epsf, momf, omm = f32(eps), f32(mom), f32(np.float32(1) - np.float32(mom))
    ve = var + epsf
    r = (dv64 + 2 * U * ve) / (2 * ve) + 4 * U
    rstd = ve.rsqrt()
    scale = w.double() * rstd
    shift = b.double() - mean * scale
    fac = M / max(M - 1, 1)
    unb = var * fac
    rm1 = omm * rm.double() + momf * mean
    rv1 = omm * rv.double() + momf * unb
    return {
        "mean": (mean, e_mean),
        "rstd": (rstd, r * rstd),
        "scale": (scale, r * scale.abs()),
        "shift": (shift, scale.abs() * e_mean + (mean * scale).abs() * (r + U) + U * shift.abs()),
        "running_mean": (rm1, U * (omm * rm.double()).abs() + momf * e_mean + U * (momf * mean).abs() + U * rm1.abs()),
        "running_var": (rv1, U * (omm * rv.double()).abs() + momf * (dv64 * fac + U * unb) + U * momf * unb + U * rv1.abs()),
    }


def slab_sums(t, fault=None):
    """fp64 per-channel sum of t[M][C] the way the two-stage kernels form it: 64-row slabs, then over the slabs"""
    M, C = t.shape
    nblk = (M + 63) // 64
    p = torch.zeros(nblk * 64, C, dtype=torch.float64, device=t.device)
    p[:M] = t.double()
    p = p.view(nblk, 64, C).sum(1)
    if fault == "drop_last_slab":
        p = p[:-1]
    return p.sum(0)


def bn_train_emul(x, w, b, rm, rv, eps=1e-5, mom=0.1, fault=None):
    """channel_stats_partial_kernel + bn_train_finalize_kernel in plain torch: fp64 one-pass sums, then the f32 bookkeeping"""
    M = x.shape[0]
    one = torch.tensor(1.0, dtype=torch.float32, device=x.device)
    s = slab_sums(x, fault)
    q = slab_sums(x.double().square(), fault)
    mean = s / M
    var = (q / M - mean * mean).clamp(min=0)
    fac = M / max(M - 1, 1)
    meanf = mean.float()
    varf = (var * fac if fault == "unbiased_scale" else var).float()
    den = torch.sqrt(varf + one * eps)
    sc = w / den
    sh = b - meanf * sc
    mr = torch.stack([meanf, one / den], 1)
    if fault == "swap_mean_rstd":
        mr = torch.stack([one / den, meanf], 1)
    unb = (var * fac).float()
    m = one * mom
    return {"scale": sc, "shift": sh, "mean": mr[:, 0], "rstd": mr[:, 1], "running_mean": (one - m) * rm + m * meanf,
            "running_var": (one - m) * rv + m * unb, "mean_rstd": mr.contiguous()}


def bn_train_ratios(got, ref):
    return {k + "_ratio": ratio(got[k], *ref[k]) for k in ref if k in got}


# ----------------------------------------------------------------------------- BatchNorm + ReLU backward: reference and emulation
def bn_bwd_ref(da, x, mr, g, bt, dx_in, pre_g, pre_b):
    """fp64 reference of bn_relu_bwd from the same f32 inputs -> dict (see the module docstring for every bar)"""
    M = x.shape[0]
    xd, dad = x.double(), da.double()
    mu, rs, gd, bd = mr[:, 0].double(), mr[:, 1].double(), g.double(), bt.double()
    xh = (xd - mu) * rs
    del xd
    gx = gd * xh
    y = gx + bd
    mgr = mu * gd * rs
    e_y = (4 * U * gx.abs() + U * (mgr.abs() + (bd - mgr).abs()) + U * y.abs()) * (1 + 8 * U)
    del gx
    und = y.abs() <= e_y
    mask = y > 0
    del e_y
    dy = dad * mask
    dyx = dy * xh
    a1 = (dad.abs() * und).sum(0)
    a2 = ((dad * xh).abs() * und).sum(0)
    S1, S2 = dy.sum(0), dyx.sum(0)
    dep = depth(M)
    e1 = dep * U64 * dy.abs().sum(0) + U * S1.abs() + a1
    e2 = (3 * U + dep * U64) * dyx.abs().sum(0) + U * S2.abs() + a2
    del dyx
    m1, m2 = S1 / M, S2 / M
    din = dx_in.double() if dx_in is not None else 0.0
    grs = gd * rs
    dx_a = din + grs * (dy - m1 - xh * m2)
    dx_b = din + grs * (dad * (mask ^ und) - m1 - xh * m2)
    dyabs = torch.where(und, dad.abs(), dy.abs())
    bar_dx = grs.abs() * (6 * U * (dyabs + m1.abs()) + 8 * U * (xh * m2).abs() + e1 / M + xh.abs() * e2 / M) \
        + U * torch.maximum(dx_a.abs(), dx_b.abs())
    return {"dx": (dx_a, bar_dx, dx_b), "dbeta": (pre_b.double() + S1, e1 + U * S1.abs() + 2 * U * pre_b.double().abs()),
            "dgamma": (pre_g.double() + S2, e2 + U * S2.abs() + 2 * U * pre_g.double().abs()),
            "und": und, "y": y, "m1": m1, "m2": m2, "xh": xh, "grs": grs}


def bn_bwd_emul(da, x, mr, g, bt, dx_in, pre_g, pre_b, fault=None, pro=None):
    """bn_relu_bwd partial / reduce / apply in plain torch f32 (fp64 sums).  pro = (scale, shift): decide the mask as the GEMM prologue
    does, fmaxf(fmaf(x, scale, shift), 0) > 0, instead of the backward's own expression (both must meet the bars)"""
    M = x.shape[0]
    mu, rs = mr[:, 0], mr[:, 1]
    xh = (x - mu) * rs
    if pro is None:
        y = g * xh + bt
    else:
        y = (x.double() * pro[0].double() + pro[1].double()).float()          # one rounding: the fma
    dy = torch.where(y > 0, da, torch.zeros_like(da))
    s1f, s2f = slab_sums(dy, fault).float(), slab_sums(dy * xh, fault).float()
    inv_m = torch.tensor(1.0, dtype=torch.float32, device=x.device) / torch.tensor(float(M), dtype=torch.float32, device=x.device)
    res = g * rs * (dy - s1f * inv_m - xh * s2f * inv_m)
    dx = res if dx_in is None or fault == "assign_dx" else dx_in + res
    if fault == "assign_acc":
        return {"dx": dx, "dbeta": s1f, "dgamma": s2f}
    return {"dx": dx, "dbeta": pre_b + s1f, "dgamma": pre_g + s2f}


def bn_bwd_ratios(got, ref):
    return {"dx_ratio": ratio(got["dx"], ref["dx"][0], ref["dx"][1], alt=ref["dx"][2]),
            "dgamma_ratio": ratio(got["dgamma"], *ref["dgamma"]), "dbeta_ratio": ratio(got["dbeta"], *ref["dbeta"])}


def bn_bwd_inputs(M, C, seed, dev, with_dx_in):
    g = gen(seed, dev)
    da = torch.randn(M, C, generator=g, device=dev)
    da[::9] *= 1e3
    dx_in = torch.randn(M, C, generator=g, device=dev) if with_dx_in else None
    pre_g = torch.randn(C, generator=g, device=dev) * 3
    pre_b = torch.randn(C, generator=g, device=dev) * 3
    return da, dx_in, pre_g, pre_b


UND_CAP = 1e-4
BWD_FAMILIES = ["unit", "m10", "m100", "mixed"]        # the hard family's e_y (|mu| rs = 2e4) leaves 2e-3 of it undecided: forward only


# ----------------------------------------------------------------------------- lincomb, mse: reference and emulation
def lincomb_ref(a, b, c, alpha):
    al = f32(alpha)
    d = b.double() - c.double()
    out = (a.double() if a is not None else 0.0) + al * d
    return out, U * abs(al) * d.abs() + U * (al * d).abs() + U * out.abs()


def lincomb_emul(a, b, c, alpha, fault=None):
    p = torch.tensor(alpha, dtype=torch.float32, device=b.device) * (b - c)
    return p if a is None or fault == "ignore_a" else a + p


def mse_ref(a, b, scale):
    d2 = (a.double() - b.double()).square().sum()
    want = d2 * f32(scale) / a.numel()
    return want, 3 * U * want + U * want.abs()


def mse_emul(a, b, scale, fault=None):
    n = a.numel()
    d = a.view(-1) - b.view(-1)
    sq = (d * d).double()
    if fault == "no_grid_stride":
        sq = sq[:min((n + 255) // 256, 1024) * 256]
    return (sq.sum() * (float(np.float32(scale)) / n)).float()


# ----------------------------------------------------------------------------- codebook: reference and emulation
def cb_indices(M, K, seed, dev):
    """idx[M] with, for M >= 16384: codes that never occur (1, K/2, K-2), codes that occur once (2, K/2+1), a hot code (3) that takes
    more than 10,000 rows, and the codes 0 and K-1 present"""
    g = gen(seed, dev)
    idx = torch.randint(0, K, (M,), generator=g, device=dev)
    if M >= 16384:
        hot, never, once = 3, [1, K // 2, K - 2], [2, K // 2 + 1]
        idx[:12000] = hot
        for k in never + once:
            idx[idx == k] = hot
        idx[12000], idx[M - 2] = once[0], once[1]
        idx[12001], idx[M - 1] = 0, K - 1
    return idx.contiguous()


def cb_stats_ref(z, idx, K):
    E = z.shape[1]
    cnt = torch.bincount(idx, minlength=K)
    zero = torch.zeros(K, E, dtype=torch.float64, device=z.device)
    want = zero.index_add(0, idx, z.double())
    bar = gamt(cnt)[:, None] * zero.index_add(0, idx, z.double().abs())
    return cnt, want, bar


def exact_threshold_pair(decay=0.99):
    """(N, n): an f32 N and a count n for which N d + (1 - d) n is 1.0f exactly however the f32 expression is evaluated: both products
    rounded, or either product fused into the addition (its exact value, from fp64, strictly inside 1.0f's rounding interval)"""
    d = np.float32(decay)
    omd = np.float32(1) - d
    for n in range(1, 100):
        t = omd * np.float32(n)
        c = np.float32((1.0 - float(t)) / float(d))
        for _ in range(8):
            c = np.nextafter(c, np.float32(0))
        for _ in range(17):
            fused = (float(c) * float(d) + float(t), float(np.float32(c * d)) + float(omd) * n)
            if np.float32(c * d) + t == np.float32(1) and all(1 - 0.9 * 2.0 ** -25 < v < 1 + 0.9 * 2.0 ** -24 for v in fused):
                return float(c), n
            c = np.nextafter(c, np.float32(2))
    raise AssertionError("no (N, n) lands on 1.0f")


def cb_state(K, E, n_total, seed, dev, on_code, decay=0.99):
    """N, z_avg, embeddings before the update.  N is set so that N' = N d + (1 - d) n_total lands 16 ulp below 1 (k % 4 == 0), 16 ulp
    above (k % 4 == 1), anywhere in [0, 3) (k % 4 == 2) or far above; `on_code` gets the N of exact_threshold_pair (its n_total is set by the caller)."""
    g = gen(seed, dev)
    d = f32(decay)
    omd = f32(np.float32(1) - np.float32(decay))
    k = torch.arange(K, device=dev)
    nt = n_total.double()
    target = torch.where(k % 4 == 0, 1 - 16 * 2.0 ** -24, 1 + 16 * 2.0 ** -23)
    n0 = (target - omd * nt) / d
    generic = torch.rand(K, generator=g, device=dev, dtype=torch.float64) * 3
    n0 = torch.where((k % 4 >= 2) | (n0 < 0), generic, n0)
    n0 = torch.where(k % 4 == 3, n0 * 40 + 2, n0)
    n0[on_code] = exact_threshold_pair(decay)[0]
    za = torch.randn(K, E, generator=g, device=dev) * (1 + n0.float()[:, None])
    emb = torch.randn(K, E, generator=g, device=dev)
    return n0.float().contiguous(), za.contiguous(), emb.contiguous()


def perplexity_ref(counts, m):
    """exp(-sum p log(p + 1e-10f)), p = counts / m, in fp64 -> (value, bar)"""
    p = counts.double() / m
    L = torch.log(p + f32(1e-10))
    h = (p * L).sum()
    e_h = (p * (3 * U + 7 * U * L.abs())).sum() + U * h.abs()
    perp = torch.exp(-h)
    return perp, perp * (e_h + 4 * U)


def cb_update_ref(z, perm, n0, za0, n_total, es, m_rows, on_code, decay=0.99, n_local=None, m_local=None):
    """fp64 restatement of videogpt_vq_vae.py:199-219 (the EMA branch after the statistics) and its bars"""
    K, E = za0.shape
    d, omd, tiny = f32(decay), f32(np.float32(1) - np.float32(decay)), f32(1e-7)
    nd, ntd = n0.double(), n_total.double()
    N1 = nd * d + omd * ntd
    b_N = U * ((nd * d).abs() + (omd * ntd).abs() + N1.abs())
    za1 = za0.double() * d + omd * es.double()
    b_za = U * ((za0.double() * d).abs() + (omd * es.double()).abs() + za1.abs())
    n = N1.sum()
    b_n = b_N.sum() + U * n
    w = (N1 + tiny) / (n + K * tiny) * n
    r_w = b_N / (N1 + tiny) + 2 * b_n / n + 8 * U
    emb_ema = za1 / w[:, None]
    bar_emb = b_za / w[:, None] + emb_ema.abs() * (r_w[:, None] + 4 * U)
    # usage: fp64 decides every code at least 4 ulp from 1 (and twice its own b_N); the only other code may be on_code, which every
    # evaluation order of the f32 expression puts on 1.0f exactly (exact_threshold_pair): kept
    far = (N1 - 1).abs() >= 4 * 2.0 ** -23
    assert bool((b_N[far] < (N1 - 1).abs()[far] / 2).all())
    near = torch.nonzero(~far).view(-1).tolist()
    near_ok = near == [on_code] and (float(n0[on_code]), int(n_total[on_code])) == exact_threshold_pair(decay)
    usage = torch.where(far, N1 >= 1, torch.ones_like(far))
    restart = z[perm]
    p_tot, bar_tot = perplexity_ref(n_total, m_rows)
    out = {"N": (N1, b_N), "z_avg": (za1, b_za), "emb_ema": (emb_ema, bar_emb), "usage": usage, "restart": restart,
           "n_sum": (n, b_n), "near_ok": near_ok, "n_near": int((~far).sum()), "perplexity": (p_tot, bar_tot)}
    if n_local is not None:
        out["perplexity"] = perplexity_ref(n_local, m_local)
    return out


def cb_update_emul(z, perm, n0, za0, n_total, es, m_rows, decay=0.99, n_local=None, m_local=None, fault=None):
    """codebook_ema_n_kernel + codebook_ema_emb_kernel (+ code_perplexity_kernel) in plain torch f32"""
    K, E = za0.shape
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=n0.device)
    d = t(decay)
    N1 = n0 * d + (t(1.0) - d) * n_total
    za1 = za0 * d + (t(1.0) - d) * es
    n = N1.double().sum().float()
    w = (N1 + t(1e-7)) / (n + t(float(K)) * t(1e-7)) * n
    usage = ((N1 > 1) if fault == "gt_instead_of_ge" else (N1 >= 1)).float()[:, None]
    emb = (za1 / w[:, None]) * usage + z[perm] * (1 - usage)
    if fault == "restart_overwrites_z_avg":
        za1 = torch.where(usage > 0, za1, z[perm])

    def perp(counts, m):
        p = counts / t(float(m))
        return torch.exp(-(p * torch.log(p + t(1e-10))).double().sum().float())
    if n_local is not None and fault != "n_total_for_local_perplexity":
        pp = perp(n_local, m_local)
    else:
        pp = perp(n_total, m_local if n_local is not None else m_rows)
    return {"N": N1, "z_avg": za1, "emb": emb, "n_sum": n, "perplexity": pp}


def cb_update_ratios(got, ref):
    """-> ratios dict; restarted rows of the embeddings must equal the restart rows bit for bit (else infinitely wrong)"""
    use = ref["usage"]
    r = {"N_ratio": ratio(got["N"], *ref["N"]), "z_avg_ratio": ratio(got["z_avg"], *ref["z_avg"]),
         "n_sum_ratio": ratio(got["n_sum"], *ref["n_sum"]), "perplexity_ratio": ratio(got["perplexity"], *ref["perplexity"]),
         "emb_ratio": ratio(got["emb"][use], ref["emb_ema"][0][use], ref["emb_ema"][1][use])}
    r["restart_bit_exact"] = bool(torch.equal(got["emb"][~use], ref["restart"][~use]))
    if not r["restart_bit_exact"]:
        r["emb_ratio"] = math.inf
    return r


def cb_update_inputs(M, E, K, seed, dev):
    """everything the update takes, as the two-rank step passes it: n_total = n_local + the other rank's counts, m_local != rows of z"""
    g = gen(seed, dev)
    idx = cb_indices(M, K, seed, dev)
    n_local = torch.bincount(idx, minlength=K).float()
    other = torch.bincount(torch.randint(0, K, (M // 4,), generator=g, device=dev), minlength=K).float()
    other[n_local == 0] = 0                                   # codes that never occur stay at n_total = 0
    on_code = K // 2 + 2
    n_local[on_code], other[on_code] = exact_threshold_pair()[1], 0          # phase 1 does not read idx: the counts are free
    n_total = (n_local + other).contiguous()
    es = torch.randn(K, E, generator=g, device=dev) * n_total[:, None].sqrt()
    rows = max(M, K) + 5                                     # the restart candidates (tiled when there are fewer latents than codes)
    z = torch.randn(rows, E, generator=g, device=dev)
    perm = torch.randperm(rows, generator=g, device=dev)[:K].contiguous()
    n0, za0, emb0 = cb_state(K, E, n_total, seed + 1, dev, on_code)
    return dict(idx=idx, n_local=n_local.contiguous(), n_total=n_total, es=es.contiguous(), z=z.contiguous(), perm=perm, n0=n0, za0=za0,
                emb0=emb0, on_code=on_code, rows=rows)


# ============================================================================= GPU tests
BN_TRAIN_CASES = [
    # (name, family, M, C, want_stats, update_running)
    *[(f"C2_M262144_C256_{f}", f, FULL_M, 256, True, True) for f in BN_FAMILIES],
    ("C2_M262144_C128_mixed", "mixed", FULL_M, 128, True, True),
    ("M1_C256", "mixed", 1, 256, True, True),
    ("M1_C260_norunning", "m10", 1, 260, True, False),
    ("M63_C48", "m100", 63, 48, True, True),
    ("M64_C4", "unit", 64, 4, True, True),
    ("M65_C260", "mixed", 65, 260, True, True),
    ("M65_C512_nostats", "m10", 65, 512, False, True),
    ("M16421_C512", "mixed", RAGGED_M, 512, True, True),
    ("M16421_C260_hard", "hard", RAGGED_M, 260, True, True),
    ("M16421_C256_nostats_norunning", "m100", RAGGED_M, 256, False, False),
    ("M16421_C48", "hard", RAGGED_M, 48, True, True),
    ("M16421_C4", "m100", RAGGED_M, 4, True, True),
]


def run_bn_train_guarded(G, x, w, b, rm, rv, want_stats, update_running, eps=1e-5, mom=0.1):
    """gsdd_bn_train with every output and the exactly-sized workspace between sentinels -> (outputs dict, guards intact)"""
    O = G.ops
    M, C = x.shape
    GD = 64
    nws = O.lib().gsdd_bn_train_workspace_bytes(M, C)
    assert nws == ((M + 63) // 64) * C * 16
    wbuf, ws = guarded(GD, (nws // 8,), GD, None, dtype=torch.float64)
    bufs = {k: guarded(GD, s, GD, f) for k, s, f in (("scale", (C,), 0.0), ("shift", (C,), 0.0), ("mr", (C, 2), 0.0),
                                                      ("rm", (C,), rm), ("rv", (C,), rv))}
    v = {k: bufs[k][1] for k in bufs}
    O.check(O.lib().gsdd_bn_train(O.ptr(x), M, C, O.ptr(w), O.ptr(b), eps, mom, O.ptr(v["rm"] if update_running else None),
                                  O.ptr(v["rv"] if update_running else None), O.ptr(v["scale"]), O.ptr(v["shift"]),
                                  O.ptr(v["mr"] if want_stats else None), O.ptr(ws), nws, O.stream_ptr()))
    torch.cuda.synchronize()
    intact = guards_intact(wbuf, GD, nws // 8, GD) and all(guards_intact(bufs[k][0], GD, v[k].numel(), GD) for k in bufs)
    return {"scale": v["scale"], "shift": v["shift"], "mean": v["mr"][:, 0], "rstd": v["mr"][:, 1], "mean_rstd": v["mr"],
            "running_mean": v["rm"], "running_var": v["rv"]}, intact


def make_bn(w, b, rm, rv):
    return types.SimpleNamespace(weight=w, bias=b, running_mean=rm.clone(), running_var=rv.clone(), eps=1e-5,
                                 num_batches_tracked=torch.zeros((), dtype=torch.int64, device=w.device))


@gpu
@pytest.mark.parametrize("name,family,M,C,want_stats,update_running", BN_TRAIN_CASES, ids=[c[0] for c in BN_TRAIN_CASES])
def test_bn_train_matches_fp64(G, name, family, M, C, want_stats, update_running):
    """scale, shift, mean_rstd and the running statistics of gsdd_bn_train against the fp64 two-pass statistics; the ops.bn_train wrapper
    must give the same bits, count the batch, and leave the running buffers alone when told to.  Records the kernel's worst relative rstd
    error beside torch's own f32 batch_norm; in the C2-shape family cases the kernel must be within 2 x of torch's."""
    x = bn_family(family, M, C, 100 + C + M % 997, "cuda")
    w, b, rm, rv = bn_params(C, C + 1, "cuda")
    got, intact = run_bn_train_guarded(G, x, w, b, rm, rv, want_stats, update_running)
    ref = bn_train_ref(x, w, b, rm, rv)
    keys = ["scale", "shift"] + (["mean", "rstd"] if want_stats else []) + (["running_mean", "running_var"] if update_running else [])
    res = {k + "_ratio": ratio(got[k], *ref[k]) for k in keys}
    untouched = True
    if not update_running:
        untouched = bool(torch.equal(got["running_mean"], rm)) and bool(torch.equal(got["running_var"], rv))
    if not want_stats:
        untouched = untouched and bool((got["mean_rstd"] == 0).all())
    # the wrapper: same bits, batch counted, running buffers as asked
    bn = make_bn(w, b, rm, rv)
    r = G.ops.bn_train(x, bn, update_running=update_running, want_stats=want_stats)
    (sc, sh), mr = r if want_stats else (r, None)
    same = bool(torch.equal(sc, got["scale"])) and bool(torch.equal(sh, got["shift"])) and (mr is None or bool(torch.equal(mr, got["mean_rstd"])))
    same = same and bool(torch.equal(bn.running_mean, got["running_mean"])) and bool(torch.equal(bn.running_var, got["running_var"]))
    counted = int(bn.num_batches_tracked) == (1 if update_running else 0)
    # rstd beside torch's f32 batch_norm (save_invstd), both against fp64
    rec = {"M": M, "C": C, "family": family}
    if want_stats and M > 1:
        _, _, t_rstd = torch.native_batch_norm(x, w, b, rm.clone(), rv.clone(), True, 0.1, 1e-5)
        want_rstd = ref["rstd"][0]
        rec["rstd_relerr_kernel"] = float(((got["rstd"].double() - want_rstd).abs() / want_rstd).max())
        rec["rstd_relerr_torch_f32"] = float(((t_rstd.double() - want_rstd).abs() / want_rstd).max())
    worst = max(res.values())
    parity_report(f"vqvae_train_kernels::bn_train[{name}]", {**rec, **res, "worst_ratio": worst})
    assert intact, "bn_train wrote outside its outputs or its workspace"
    assert untouched, "bn_train wrote running statistics / mean_rstd it was told to leave"
    assert same and counted, "ops.bn_train differs from the direct call, or did not count the batch"
    assert worst <= 1, res
    if name.startswith("C2_M262144_C256"):
        assert rec["rstd_relerr_kernel"] <= 2 * rec["rstd_relerr_torch_f32"], rec


BN_BWD_CASES = [
    # (name, family, M, C, dx_in)
    ("C2_M262144_C256_m100_dxin", "m100", FULL_M, 256, True),
    ("C2_M262144_C256_mixed", "mixed", FULL_M, 256, False),
    ("C2_M262144_C128_m10_dxin", "m10", FULL_M, 128, True),
    ("C2_M262144_C128_unit", "unit", FULL_M, 128, False),
    ("M1_C256_dxin", "unit", 1, 256, True),
    ("M1_C4", "unit", 1, 4, False),
    ("M63_C48_dxin", "m100", 63, 48, True),
    ("M64_C260", "m10", 64, 260, False),
    ("M65_C512_dxin", "mixed", 65, 512, True),
    ("M65_C4", "m100", 65, 4, False),
    ("M16421_C260_dxin", "mixed", RAGGED_M, 260, True),
    ("M16421_C512", "m100", RAGGED_M, 512, False),
    ("M16421_C48_dxin", "unit", RAGGED_M, 48, True),
    ("M16421_C4", "m10", RAGGED_M, 4, False),
]


def run_bn_bwd_guarded(G, da, x, mr, g, bt, dx_in, pre_g, pre_b):
    O = G.ops
    M, C = x.shape
    GD = 64
    nws = O.lib().gsdd_bn_relu_bwd_workspace_bytes(M, C)
    assert nws == ((M + 63) // 64) * C * 16 + C * 8
    wbuf, ws = guarded(GD, (nws // 8,), GD, None, dtype=torch.float64)
    xbuf, dx = guarded(GD, (M, C), GD, None)
    gbuf, dgamma = guarded(GD, (C,), GD, pre_g)
    bbuf, dbeta = guarded(GD, (C,), GD, pre_b)
    O.check(O.lib().gsdd_bn_relu_bwd(O.ptr(da), O.ptr(x), M, C, O.ptr(mr), O.ptr(g), O.ptr(bt), O.ptr(dx_in), O.ptr(dx), O.ptr(dgamma),
                                     O.ptr(dbeta), O.ptr(ws), nws, O.stream_ptr()))
    torch.cuda.synchronize()
    intact = guards_intact(wbuf, GD, nws // 8, GD) and guards_intact(xbuf, GD, M * C, GD) and guards_intact(gbuf, GD, C, GD) \
        and guards_intact(bbuf, GD, C, GD)
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}, intact


@gpu
@pytest.mark.parametrize("name,family,M,C,with_dx_in", BN_BWD_CASES, ids=[c[0] for c in BN_BWD_CASES])
def test_bn_relu_bwd_matches_fp64(G, name, family, M, C, with_dx_in):
    """dx, dgamma += and dbeta += of gsdd_bn_relu_bwd, fed bn_train's own f32 mean_rstd as the trainer feeds it (taken as exact
    inputs), from nonzero accumulators; the ops.bn_relu_bwd wrapper must give the same bits."""
    x = bn_family(family, M, C, 300 + C + M % 997, "cuda")
    w, b, rm, rv = bn_params(C, C + 2, "cuda")
    bn = make_bn(w, b, rm, rv)
    _, mr = G.ops.bn_train(x, bn, want_stats=True)
    da, dx_in, pre_g, pre_b = bn_bwd_inputs(M, C, M + C, "cuda", with_dx_in)
    got, intact = run_bn_bwd_guarded(G, da, x, mr, w, b, dx_in, pre_g, pre_b)
    ref = bn_bwd_ref(da, x, mr, w, b, dx_in, pre_g, pre_b)
    res = bn_bwd_ratios(got, ref)
    n_und = int(ref["und"].sum())
    dg2, db2 = pre_g.clone(), pre_b.clone()
    dx2 = G.ops.bn_relu_bwd(da, x, mr, bn, dg2, db2, dx_in=dx_in)
    same = bool(torch.equal(dx2, got["dx"])) and bool(torch.equal(dg2, got["dgamma"])) and bool(torch.equal(db2, got["dbeta"]))
    worst = max(res.values())
    parity_report(f"vqvae_train_kernels::bn_relu_bwd[{name}]", {"M": M, "C": C, "family": family, "undecided": n_und,
                                                               "undecided_share": n_und / (M * C), **res, "worst_ratio": worst})
    assert intact, "bn_relu_bwd wrote outside its outputs or its workspace"
    assert same, "ops.bn_relu_bwd differs from the direct call"
    assert n_und <= UND_CAP * M * C, (n_und, M * C)
    assert worst <= 1, res


@gpu
def test_bn_relu_mask_forward_backward_consistency(G):
    """The forward decides the ReLU mask in the GEMM prologue, fmaxf(fmaf(x, scale, shift), 0); the backward re-derives it from g ((x -
    mu) rs) + b.  At the C2 shape (|mean| / std = 100 family): the forward mask from a 1-tap identity GEMM in the exact-f32 mode
    (out = relu(fma(x, scale, shift)): within half an ulp of the fp64 value, which a separate multiply and add are not), the backward's from dx with |da| in [1, 2] (dy = dx / (g rs) + m1 + xh m2 is da or 0).
    Counts the elements where they disagree; every one of them must be an undecided element (|y| <= e_y)."""
    M, C = FULL_M, 256
    x = bn_family("m100", M, C, 71, "cuda")
    w, b, rm, rv = bn_params(C, 72, "cuda")
    bn = make_bn(w, b, rm, rv)
    (scale, shift), mr = G.ops.bn_train(x, bn, want_stats=True)
    g = gen(73, "cuda")
    da = (1 + torch.rand(M, C, generator=g, device="cuda")) * torch.where(torch.rand(M, C, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    eye = torch.eye(C, device="cuda").view(1, C, C).contiguous()
    out = G.ops.gemm(x, eye, torch.empty(M, C, device="cuda"), in_dims=(1, 1, 1, M), out_grid=(1, 1, M), pro=(scale, shift), exact_f32=True)
    y_fma = x.double() * scale.double() + shift.double()                     # the product is exact in fp64: one rounding, as the fma
    prologue_exact = bool(((out.double() - y_fma.clamp(min=0)).abs() <= U * y_fma.abs() + 2.0 ** -150).all())
    del y_fma
    zeros = torch.zeros(C, device="cuda")
    dx = G.ops.bn_relu_bwd(da, x, mr, bn, zeros.clone(), zeros.clone())
    ref = bn_bwd_ref(da, x, mr, w, b, None, zeros, zeros)
    dy_implied = dx.double() / ref["grs"] + ref["m1"] + ref["xh"] * ref["m2"]
    bwd_mask = dy_implied.abs() > 0.5 * da.double().abs()
    recovered = bool((torch.minimum(dy_implied.abs(), (dy_implied - da.double()).abs()) < 1e-2).all())
    disagree = (out > 0) != bwd_mask
    n_dis, n_und = int(disagree.sum()), int(ref["und"].sum())
    n_bad = int((disagree & ~ref["und"]).sum())
    fwd_vs_fp64 = int((((out > 0) != (ref["y"] > 0)) & ~ref["und"]).sum())
    parity_report("vqvae_train_kernels::bn_relu_mask_consistency[C2_M262144_C256_m100]",
                  {"elements": M * C, "mask_disagreements": n_dis, "undecided": n_und, "disagreements_on_decided": n_bad,
                   "forward_mask_wrong_on_decided": fwd_vs_fp64, "prologue_is_exact_fma": prologue_exact,
                   "worst_ratio": 0.0 if n_bad == 0 and fwd_vs_fp64 == 0 else math.inf})
    assert prologue_exact, "the identity GEMM did not return relu(fma(x, scale, shift))"
    assert recovered, "dx does not determine the backward's mask"
    assert n_und <= UND_CAP * M * C
    assert n_bad == 0 and fwd_vs_fp64 == 0, (n_dis, n_bad, fwd_vs_fp64)


def relu_specials(dev):
    out = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, math.inf, -math.inf, 1.0, -1.0,
                        1.17549435e-38, 3e38, -3e38, 5e-324], device=dev)
    return out, torch.tensor([-0.0] * 8 + [2.5, -0.0, -0.0, -0.0, 7.0, -0.0, 1.0, -0.0], device=dev)


@gpu
@pytest.mark.parametrize("n", [4, 16, 1028, 64 * 16 * 64 * 64 * 256], ids=["n4", "n16", "n1028", "C2_decoder_64x16x64x64x256"])
def test_relu_mask_bit_exact(G, n):
    """dpre = dout [out > 0], bit for bit, with +-0, denormals and +-inf in `out` and -0.0 in `dout`; the largest case is the input of
    the last transposed convolution at batch 64 (2^30 elements), the largest saved activation the trainer passes."""
    g = gen(n % 1009, "cuda")
    out = torch.randn(n, generator=g, device="cuda")
    dout = torch.randn(n, generator=g, device="cuda")
    so, sd = relu_specials("cuda")
    k = min(n, so.numel())
    for at in {0, (n // 2) // 4 * 4, n - k}:
        m = min(k, n - at)
        out[at:at + m] = so[:m]
        dout[at:at + m] = sd[:m]
    GD = 256
    pbuf, dpre = guarded(GD, (n,), GD, None)
    O = G.ops
    O.check(O.lib().gsdd_relu_mask(O.ptr(dout), O.ptr(out), O.ptr(dpre), n, O.stream_ptr()))
    torch.cuda.synchronize()
    want = torch.where(out > 0, dout, torch.zeros((), device="cuda"))
    exact = bool(torch.equal(dpre.view(torch.int32), want.view(torch.int32)))
    intact = guards_intact(pbuf, GD, n, GD)
    del want
    wrapper = n > 2 ** 20 or bool(torch.equal(O.relu_mask(dout, out).view(torch.int32), dpre.view(torch.int32)))
    parity_report(f"vqvae_train_kernels::relu_mask[n{n}]", {"n": n, "bit_exact": exact, "worst_ratio": 0.0 if exact else math.inf})
    assert intact, "relu_mask wrote outside dpre"
    assert exact and wrapper


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 1026])
def test_relu_mask_refuses_lengths_not_multiple_of_4(G, n):
    O = G.ops
    out, dout = torch.randn(n + 4, device="cuda"), torch.randn(n + 4, device="cuda")
    pbuf, dpre = guarded(64, (n + 4,), 64, None)
    with pytest.raises(G.ops.GsddError):
        O.check(O.lib().gsdd_relu_mask(O.ptr(dout), O.ptr(out), O.ptr(dpre), n, O.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((pbuf == SENT).all()), "a refused relu_mask call wrote"


C2_RECON = 64 * 3 * 16 * 128 * 128
C2_LATENT = FULL_M * 128


@gpu
@pytest.mark.parametrize("with_a", [True, False], ids=["a", "a_none"])
@pytest.mark.parametrize("n", [1, 255, 1000, C2_LATENT, C2_RECON])
def test_lincomb_matches_fp64(G, n, with_a):
    """out = a + alpha (b - c) with the trainer's two alphas at the real element counts: 2 / (0.06 numel) (d loss / d x_recon) and 0.25 x
    2 / numel (the commitment term added to the decoder's gradient)."""
    g = gen(n % 1013 + int(with_a), "cuda")
    b, c = torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda")
    a = torch.randn(n, generator=g, device="cuda") * 1e-6 if with_a else None
    res = {}
    O = G.ops
    for tag, alpha in (("recon", 2.0 / (0.06 * C2_RECON)), ("commit", 0.25 * 2.0 / C2_LATENT)):
        obuf, out = guarded(256, (n,), 256, None)
        O.check(O.lib().gsdd_lincomb(O.ptr(a), O.ptr(b), O.ptr(c), alpha, O.ptr(out), n, O.stream_ptr()))
        torch.cuda.synchronize()
        assert guards_intact(obuf, 256, n, 256), "lincomb wrote outside out"
        assert torch.equal(O.lincomb(a, b, c, alpha), out), "ops.lincomb differs from the direct call"
        res[tag + "_ratio"] = ratio(out, *lincomb_ref(a, b, c, alpha))
    worst = max(res.values())
    parity_report(f"vqvae_train_kernels::lincomb[n{n}_{'a' if with_a else 'a_none'}]", {"n": n, **res, "worst_ratio": worst})
    assert worst <= 1, res


@gpu
@pytest.mark.parametrize("n,scale", [(1, 1.0), (255, 0.25), (256 * 1024, 1.0 / 0.06), (256 * 1024 + 1, 0.25), (C2_LATENT, 0.25),
                                     (C2_RECON, 1.0 / 0.06)])
def test_mse_matches_fp64(G, n, scale):
    """scale / n sum (a - b)^2: one trip per thread up to 256 x 1024 elements, the grid-stride loop from 256 x 1024 + 1 on (192 trips
    at the reconstruction loss); twice, bit-identical; the workspace is exactly 8192 bytes between sentinels."""
    g = gen(n % 1019, "cuda")
    a = torch.randn(n, generator=g, device="cuda")
    b = a + torch.randn(n, generator=g, device="cuda") * 0.3
    b[-1] = a[-1] + 5.0                                    # the last element (the only one of the second trip at 256 x 1024 + 1) counts
    O = G.ops
    outs = []
    for _ in range(2):
        wbuf, ws = guarded(16, (1024,), 16, None, dtype=torch.float64)
        obuf, out = guarded(16, (1,), 16, None)
        O.check(O.lib().gsdd_mse(O.ptr(a), O.ptr(b), n, scale, O.ptr(out), O.ptr(ws), 8192, O.stream_ptr()))
        torch.cuda.synchronize()
        assert guards_intact(wbuf, 16, 1024, 16) and guards_intact(obuf, 16, 1, 16), "mse wrote outside its output or workspace"
        outs.append(out.clone())
    want, bar = mse_ref(a, b, scale)
    r = ratio(outs[0], want, bar)
    repeat = bool(torch.equal(outs[0], outs[1])) and bool(torch.equal(O.mse(a, b, scale).view(1), outs[0]))
    parity_report(f"vqvae_train_kernels::mse[n{n}]", {"n": n, "repeatable": repeat, "worst_ratio": r})
    assert repeat, "mse is documented as deterministic"
    assert r <= 1, r


CB_SHAPES = [(1, 4, 16), (63, 12, 16), (64, 4, 64), (65, 12, 64), (RAGGED_M, 128, 256), (RAGGED_M, 12, 4096), (FULL_M, 128, 4096)]
CB_IDS = [f"M{m}_E{e}_K{k}" for m, e, k in CB_SHAPES]


@gpu
@pytest.mark.parametrize("M,E,K", CB_SHAPES, ids=CB_IDS)
def test_codebook_ema_stats_match_fp64(G, M, E, K):
    """n_total == bincount exactly, encode_sum within gamma(n_k) sum |z|, rows of absent codes exactly zero; at M >= 16384 the index
    vector holds absent codes, codes that occur once, a code with more than 10,000 rows and the codes 0 and K - 1 all at once."""
    idx = cb_indices(M, K, M + E, "cuda")
    z = torch.randn(M, E, generator=gen(M + K, "cuda"), device="cuda")
    z[::5] *= 30
    O = G.ops
    nbuf, n_total = guarded(64, (K,), 64, None)
    ebuf, es = guarded(64, (K, E), 64, None)
    dummy = torch.empty(2, device="cuda")
    O.check(O.lib().gsdd_codebook_ema(O.ptr(z), O.ptr(idx), M, E, K, 0.99, None, O.ptr(n_total), O.ptr(n_total), O.ptr(n_total),
                                      O.ptr(n_total), O.ptr(es), O.ptr(dummy), 0, O.stream_ptr()))
    torch.cuda.synchronize()
    cnt, want, bar = cb_stats_ref(z, idx, K)
    if M >= 16384:
        assert int((cnt == 0).sum()) >= 3 and int((cnt == 1).sum()) >= 2 and int(cnt.max()) > 10000 and int(cnt[0]) > 0 and int(cnt[K - 1]) > 0
    counts_exact = bool(torch.equal(n_total, cnt.float()))
    absent_zero = bool((es[cnt == 0] == 0).all())
    r = ratio(es, want, bar)
    intact = guards_intact(nbuf, 64, K, 64) and guards_intact(ebuf, 64, K * E, 64)
    w_n, w_es = O.codebook_ema_stats(z, idx, K)
    wrapper = bool(torch.equal(w_n, n_total)) and ratio(w_es, want, bar) <= 1
    parity_report(f"vqvae_train_kernels::codebook_stats[M{M}_E{E}_K{K}]",
                  {"absent_codes": int((cnt == 0).sum()), "single_row_codes": int((cnt == 1).sum()), "largest_code_rows": int(cnt.max()),
                   "counts_exact": counts_exact, "encode_sum_ratio": r, "worst_ratio": r if counts_exact and absent_zero else math.inf})
    assert intact, "codebook statistics wrote outside n_total / encode_sum"
    assert counts_exact and absent_zero and wrapper
    assert r <= 1, r


@gpu
@pytest.mark.parametrize("local", [True, False], ids=["n_local", "no_n_local"])
@pytest.mark.parametrize("M,E,K", CB_SHAPES, ids=CB_IDS)
def test_codebook_ema_update_matches_fp64(G, M, E, K, local):
    """N, z_avg, embeddings, n_sum and the perplexity of the update against the fp64 restatement of the reference's EMA branch, with N set
    to land below, on and above the restart threshold; restarted codes take z[perm[k]] bit for bit while z_avg keeps the EMA value.
    With n_local (the two-rank step: n_total all-reduced, m_local != rows of z) scalars[1] is the local perplexity."""
    c = cb_update_inputs(M, E, K, M + 3 * E + K, "cuda")
    m_local = M
    O = G.ops
    GD = 64
    Nb, N = guarded(GD, (K,), GD, c["n0"])
    zb, za = guarded(GD, (K, E), GD, c["za0"])
    eb, emb = guarded(GD, (K, E), GD, c["emb0"])
    sb, scal = guarded(GD, (2,), GD, None)
    nt0, es0, z0 = c["n_total"].clone(), c["es"].clone(), c["z"].clone()
    O.check(O.lib().gsdd_codebook_ema(O.ptr(c["z"]), O.ptr(c["idx"]), c["rows"], E, K, 0.99, O.ptr(c["perm"]), O.ptr(N), O.ptr(za), O.ptr(emb),
                                      O.ptr(c["n_total"]), O.ptr(c["es"]), O.ptr(scal), 1, O.stream_ptr()))
    if local:
        O.check(O.lib().gsdd_code_perplexity(O.ptr(c["n_local"]), K, m_local, O.ptr(scal[1:]), O.stream_ptr()))
    torch.cuda.synchronize()
    kw = dict(n_local=c["n_local"], m_local=m_local) if local else {}
    ref = cb_update_ref(c["z"], c["perm"], c["n0"], c["za0"], c["n_total"], c["es"], c["rows"], c["on_code"], **kw)
    got = {"N": N, "z_avg": za, "emb": emb, "n_sum": scal[0], "perplexity": scal[1]}
    res = cb_update_ratios(got, ref)
    intact = all(guards_intact(bf, GD, v.numel(), GD) for bf, v in ((Nb, N), (zb, za), (eb, emb), (sb, scal)))
    inputs_kept = bool(torch.equal(c["n_total"], nt0)) and bool(torch.equal(c["es"], es0)) and bool(torch.equal(c["z"], z0))
    # the wrapper on a copy of the state
    N2, za2, emb2 = c["n0"].clone(), c["za0"].clone(), c["emb0"].clone()
    s2 = O.codebook_ema_update(c["z"], c["idx"], c["perm"], N2, za2, emb2, c["n_total"], c["es"], **kw)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(p, q)) for p, q in ((N2, N), (za2, za), (emb2, emb), (s2, scal)))
    use = ref["usage"]
    nums = {k: v for k, v in res.items() if k.endswith("_ratio")}
    worst = max(nums.values())
    parity_report(f"vqvae_train_kernels::codebook_update[M{M}_E{E}_K{K}_{'n_local' if local else 'no_n_local'}]",
                  {"restarted_codes": int((~use).sum()), "kept_codes": int(use.sum()), "codes_within_4ulp_of_threshold": ref["n_near"],
                   "on_threshold_code_N": float(N[c["on_code"]]), **res, "worst_ratio": worst})
    assert ref["near_ok"], "the codes within 4 ulp of the restart threshold are not exactly the constructed one: the inputs are wrong"
    assert int((~use).sum()) > 0 and int(use.sum()) > 0
    assert float(N[c["on_code"]]) == 1.0, "the constructed code did not land on 1.0f"
    assert intact, "the codebook update wrote outside N / z_avg / embeddings / scalars"
    assert inputs_kept, "the codebook update wrote its inputs"
    assert same, "ops.codebook_ema_update differs from the direct calls"
    assert res["restart_bit_exact"], "a restarted code is not z[perm[k]]"
    assert worst <= 1, res


@gpu
@pytest.mark.parametrize("E", [1, 6, 130])
def test_codebook_ema_refuses_E_not_multiple_of_4(G, E):
    O = G.ops
    M, K = 64, 16
    z = torch.randn(M, E, device="cuda")
    idx = torch.randint(0, K, (M,), device="cuda")
    perm = torch.arange(K, device="cuda")
    bufs = [guarded(64, s, 64, 1.0) for s in ((K,), (K, E), (K, E), (K,), (K, E), (2,))]
    N, za, emb, n_total, es, scal = (v for _, v in bufs)
    for phase in (0, 1):
        with pytest.raises(G.ops.GsddError):
            O.check(O.lib().gsdd_codebook_ema(O.ptr(z), O.ptr(idx), M, E, K, 0.99, O.ptr(perm), O.ptr(N), O.ptr(za), O.ptr(emb),
                                              O.ptr(n_total), O.ptr(es), O.ptr(scal), phase, O.stream_ptr()))
    torch.cuda.synchronize()
    for bf, v in bufs:
        assert guards_intact(bf, 64, v.numel(), 64) and bool((v == 1.0).all()), "a refused codebook call wrote"


# ============================================================================= CPU self-check of the bars (no GPU)
SMALL_BN = [("unit", 64, 4), ("m10", 1, 260), ("m100", 63, 48), ("mixed", 65, 260), ("hard", 65, 48), ("mixed", 1000, 512),
            ("m100", RAGGED_M, 48), ("hard", RAGGED_M, 4)]


@pytest.mark.parametrize("family,M,C", SMALL_BN)
def test_cpu_bn_train_emulation_meets_bars(family, M, C):
    x = bn_family(family, M, C, 7 + M + C, "cpu")
    w, b, rm, rv = bn_params(C, 8, "cpu")
    res = bn_train_ratios(bn_train_emul(x, w, b, rm, rv), bn_train_ref(x, w, b, rm, rv))
    assert len(res) == 6 and max(res.values()) < 1, res


@pytest.mark.parametrize("fault", ["drop_last_slab", "swap_mean_rstd", "unbiased_scale"])
@pytest.mark.parametrize("family,M,C", [("unit", 65, 4), ("m10", RAGGED_M, 48), ("mixed", 1000, 260)])
def test_cpu_bn_train_faults_miss_bars(family, M, C, fault):
    x = bn_family(family, M, C, 9 + M + C, "cpu")
    w, b, rm, rv = bn_params(C, 10, "cpu")
    res = bn_train_ratios(bn_train_emul(x, w, b, rm, rv, fault=fault), bn_train_ref(x, w, b, rm, rv))
    assert max(res.values()) > 1, res


SMALL_BWD = [("unit", 1, 4, False), ("m10", 63, 48, True), ("m100", 64, 260, False), ("mixed", 65, 512, True), ("mixed", 1000, 48, False),
             ("m100", RAGGED_M, 48, True)]


def cpu_bwd_setup(family, M, C, with_dx_in, seed):
    x = bn_family(family, M, C, seed + M + C, "cpu")
    w, b, rm, rv = bn_params(C, seed + 1, "cpu")
    fwd = bn_train_emul(x, w, b, rm, rv)
    da, dx_in, pre_g, pre_b = bn_bwd_inputs(M, C, seed + 2, "cpu", with_dx_in)
    return (da, x, fwd["mean_rstd"], w, b, dx_in, pre_g, pre_b), (fwd["scale"], fwd["shift"])


@pytest.mark.parametrize("mask", ["backward", "prologue"])
@pytest.mark.parametrize("family,M,C,with_dx_in", SMALL_BWD)
def test_cpu_bn_relu_bwd_emulation_meets_bars(family, M, C, with_dx_in, mask):
    """with the mask decided either way: the backward's own expression, or the forward prologue's fma(x, scale, shift)"""
    args, pro = cpu_bwd_setup(family, M, C, with_dx_in, 20)
    ref = bn_bwd_ref(*args)
    res = bn_bwd_ratios(bn_bwd_emul(*args, pro=pro if mask == "prologue" else None), ref)
    assert int(ref["und"].sum()) <= UND_CAP * M * C
    assert max(res.values()) < 1, res


@pytest.mark.parametrize("fault", ["drop_last_slab", "assign_acc", "assign_dx"])
@pytest.mark.parametrize("family,M,C", [("unit", 65, 4), ("m100", RAGGED_M, 48), ("mixed", 1000, 260)])
def test_cpu_bn_relu_bwd_faults_miss_bars(family, M, C, fault):
    args, _ = cpu_bwd_setup(family, M, C, True, 30)
    res = bn_bwd_ratios(bn_bwd_emul(*args, fault=fault), bn_bwd_ref(*args))
    assert max(res.values()) > 1, res


def test_cpu_bn_relu_bwd_swapped_stats_miss_bars():
    """mean and rstd swapped in mean_rstd (the fault injected into bn_train's emulation) as the backward sees it"""
    args, _ = cpu_bwd_setup("m10", 1000, 48, True, 40)
    good = bn_bwd_ref(*args)
    bad = list(args)
    bad[2] = args[2].flip(1).contiguous()
    res = bn_bwd_ratios(bn_bwd_emul(*bad), good)
    assert max(res.values()) > 1, res


@pytest.mark.parametrize("family", BWD_FAMILIES)
def test_cpu_undecided_share_of_the_input_families(family):
    """the share of elements whose mask the fp64 reference cannot decide (|y| <= e_y) is <= 1e-4 in every family the GPU cases use"""
    M, C = RAGGED_M, 256
    args, _ = cpu_bwd_setup(family, M, C, False, 50)
    und = bn_bwd_ref(*args)["und"]
    assert int(und.sum()) <= UND_CAP * M * C, int(und.sum())


def test_cpu_hard_family_is_left_to_the_forward():
    """the hard family (|mean| rstd = 2e4) leaves more than 1e-4 of its elements undecided: it is a bn_train family only"""
    M, C = RAGGED_M, 256
    args, _ = cpu_bwd_setup("hard", M, C, False, 60)
    assert int(bn_bwd_ref(*args)["und"].sum()) > UND_CAP * M * C


def test_cpu_relu_mask_specials():
    out, dout = relu_specials("cpu")
    want = torch.where(out > 0, dout, torch.zeros(()))
    pos = [2, 4, 6, 8, 10, 12, 13]                          # denormals, the smallest normal, +inf and ordinary positives pass dout
    assert [i for i in range(16) if out[i] > 0] == pos
    assert torch.equal(want.view(torch.int32)[pos], dout.view(torch.int32)[pos])
    assert bool((want.view(torch.int32)[[i for i in range(16) if i not in pos]] == 0).all())      # +0.0, never -0.0


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("n", [1, 255, 1000, 70001])
def test_cpu_lincomb_emulation_meets_bars_and_fault_misses(n, with_a):
    g = gen(n, "cpu")
    b, c = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a = torch.randn(n, generator=g) * 1e-6 if with_a else None
    for alpha in (2.0 / (0.06 * C2_RECON), 0.25 * 2.0 / C2_LATENT):
        want, bar = lincomb_ref(a, b, c, alpha)
        assert ratio(lincomb_emul(a, b, c, alpha), want, bar) < 1
        fused = ((a.double() if with_a else 0.0) + f32(alpha) * (b - c).double()).float()          # fma contraction: one rounding less
        assert ratio(fused, want, bar) < 1
        if with_a:
            assert ratio(lincomb_emul(a, b, c, alpha, fault="ignore_a"), want, bar) > 1


@pytest.mark.parametrize("n", [1, 255, 256 * 1024, 256 * 1024 + 1])
def test_cpu_mse_emulation_meets_bars_and_fault_misses(n):
    g = gen(n, "cpu")
    a = torch.randn(n, generator=g)
    b = a + torch.randn(n, generator=g) * 0.3
    b[-1] = a[-1] + 5.0
    want, bar = mse_ref(a, b, 1.0 / 0.06)
    assert ratio(mse_emul(a, b, 1.0 / 0.06), want, bar) < 1
    if n > 256 * 1024:
        assert ratio(mse_emul(a, b, 1.0 / 0.06, fault="no_grid_stride"), want, bar) > 1


@pytest.mark.parametrize("M,E,K", [(65, 12, 64), (RAGGED_M, 12, 256), (RAGGED_M, 4, 4096)])
def test_cpu_codebook_stats_reference_is_the_one_hot_product(M, E, K):
    """the index_add reference equals the reference module's one_hot formulation (n_total = onehot.sum(0), encode_sum = flat^T onehot)"""
    idx = cb_indices(M, K, M + E, "cpu")
    z = torch.randn(M, E, generator=gen(M, "cpu"))
    cnt, want, bar = cb_stats_ref(z, idx, K)
    onehot = torch.nn.functional.one_hot(idx, K).double()
    assert torch.equal(cnt.double(), onehot.sum(0))
    assert ratio((z.double().t() @ onehot).t(), want, bar + 1e-300) < 1e-3
    f32_sum = torch.zeros(K, E).index_add(0, idx, z)                       # an f32 accumulation in another order meets gamma(n_k)
    assert ratio(f32_sum, want, bar) < 1


@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("M,E,K", [(1, 4, 16), (65, 12, 64), (RAGGED_M, 12, 256), (RAGGED_M, 4, 4096)])
def test_cpu_codebook_update_emulation_meets_bars(M, E, K, local):
    c = cb_update_inputs(M, E, K, M + 3 * E + K, "cpu")
    kw = dict(n_local=c["n_local"], m_local=M) if local else {}
    ref = cb_update_ref(c["z"], c["perm"], c["n0"], c["za0"], c["n_total"], c["es"], c["rows"], c["on_code"], **kw)
    res = cb_update_ratios(cb_update_emul(c["z"], c["perm"], c["n0"], c["za0"], c["n_total"], c["es"], c["rows"], **kw), ref)
    assert ref["near_ok"] and int((~ref["usage"]).sum()) > 0 and int(ref["usage"].sum()) > 0
    assert res["restart_bit_exact"] and max(v for k, v in res.items() if k.endswith("_ratio")) < 1, res


@pytest.mark.parametrize("fault", ["gt_instead_of_ge", "restart_overwrites_z_avg", "n_total_for_local_perplexity"])
@pytest.mark.parametrize("M,E,K", [(65, 12, 64), (RAGGED_M, 4, 4096)])
def test_cpu_codebook_update_faults_miss_bars(M, E, K, fault):
    c = cb_update_inputs(M, E, K, M + 3 * E + K, "cpu")
    kw = dict(n_local=c["n_local"], m_local=M)
    ref = cb_update_ref(c["z"], c["perm"], c["n0"], c["za0"], c["n_total"], c["es"], c["rows"], c["on_code"], **kw)
    res = cb_update_ratios(cb_update_emul(c["z"], c["perm"], c["n0"], c["za0"], c["n_total"], c["es"], c["rows"], fault=fault, **kw), ref)
    assert max(v for k, v in res.items() if k.endswith("_ratio")) > 1, res
