"""numpy fp64 restatement of the paired video metrics (csrc/paired_metrics.hip, gsdd_amd.metrics.paired_frame_metrics; the rule:
include/gsdd.h): the squared error of two clips' uint8 levels per (clip, frame, channel) plane, and the SSIM of Wang et al. 2004 on
them -- 11 x 11 Gaussian window of sigma 1.5, valid positions, data range 255, second moments ABOUT the window's means.  Plain module (not
a conftest), on top of tests/gif_ref.py's uint8 rule.  Next to the rule it holds what the tests judge it and the kernel by: two fp32
restatements (one that centres first, whose own error against fp64 sets the GPU tolerance, and the naive one-pass form that must fail
it), the rule with a fault switched in (wrong border, window, sigma or constant), and the case list the host and GPU tests share."""
import numpy as np

import gif_ref

TAPS = 11
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2


def gaussian(sigma=1.5):
    """g[i] ~ exp(-(i - 5)^2 / (2 sigma^2)), normalised in fp64, then rounded to fp32: the eleven values the kernel holds"""
    i = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * sigma ** 2))
    return (g / g.sum()).astype(np.float32)


G32 = gaussian()


def levels(x):
    """an operand in either form -> (B, T, H, W, 3) uint8: float32 (B, 3, T, H, W) through the uint8 rule, uint8 (B, T, H, W, 3) as is"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        assert x.ndim == 5 and x.shape[-1] == 3
        return x
    assert x.dtype == np.float32 and x.ndim == 5 and x.shape[1] == 3
    return gif_ref.levels_of(x)


def planes(lv):
    """(B, T, H, W, 3) -> (B, T, 3, H, W) fp64"""
    return np.moveaxis(np.asarray(lv), -1, 2).astype(np.float64)


def sse(a, b):
    """-> (B, T, 3) int64"""
    d = levels(a).astype(np.int64) - levels(b).astype(np.int64)
    return (d * d).sum(axis=(2, 3))


def psnr(sse_btc, H, W):
    """(B, T, 3) -> (B, T) fp64: 10 log10(255^2 3 H W / sum_c sse), inf for no error"""
    total = np.asarray(sse_btc).sum(axis=-1).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(total == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * 3 * H * W / np.maximum(total, 1.0)))


def _windows(p, pad=False):
    """(..., H, W) -> (..., H', W', 121): every window's taps in row-major order, copied out so that a weighted sum over a window is
    one matrix-vector product; pad: zero-padded "same" windows (the FAULT), else valid ones"""
    if pad:
        p = np.pad(p, [(0, 0)] * (p.ndim - 2) + [(5, 5), (5, 5)])
    v = np.lib.stride_tricks.sliding_window_view(p, (TAPS, TAPS), axis=(-2, -1))
    return np.ascontiguousarray(v).reshape(v.shape[:-2] + (TAPS * TAPS,))


def _score(mu_a, mu_b, var_a, var_b, cov, c1, c2, two):
    return (two * mu_a * mu_b + c1) * (two * cov + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))


def ssim_map(a, b, window=None, c2=C2, pad=False):
    """THE RULE, in fp64: a, b (..., H, W) levels -> s (..., H - 10, W - 10) of every valid window.  window (11, 11), c2 and pad
    switch a fault in."""
    w = np.multiply.outer(G32.astype(np.float64), G32.astype(np.float64)) if window is None else np.asarray(window, dtype=np.float64)
    w = w.reshape(-1)
    wa, wb = _windows(np.asarray(a, dtype=np.float64), pad), _windows(np.asarray(b, dtype=np.float64), pad)
    mu_a, mu_b = wa @ w, wb @ w
    wa -= mu_a[..., None]                                       # the moments ABOUT the means
    wb -= mu_b[..., None]
    return _score(mu_a, mu_b, (wa * wa) @ w, (wb * wb) @ w, (wa * wb) @ w, C1, c2, 2.0)


def ssim(a, b, **fault):
    """two operands in either form -> (B, T, 3) fp64: the mean of s over each plane's windows"""
    return ssim_map(planes(levels(a)), planes(levels(b)), **fault).mean(axis=(-2, -1))


def frame_metrics(a, b):
    """what gsdd_amd.metrics.paired_frame_metrics returns, restated"""
    lv = levels(a)
    e = sse(a, b)
    return {"psnr": psnr(e, lv.shape[2], lv.shape[3]), "ssim": ssim(a, b).mean(axis=-1), "sse": e}


def _w32():
    return (G32[:, None] * G32[None, :]).astype(np.float32).reshape(-1)


def ssim_fp32(a, b):
    """fp32 throughout, with the mean taken FIRST: mu per window, then the moments of x - mu, 121 taps each.
    -> s (..., H - 10, W - 10) float32"""
    f = np.float32
    w = _w32()
    wa, wb = _windows(np.asarray(a, dtype=f)), _windows(np.asarray(b, dtype=f))
    mu_a, mu_b = wa @ w, wb @ w
    wa -= mu_a[..., None]
    wb -= mu_b[..., None]
    s = _score(mu_a, mu_b, (wa * wa) @ w, (wb * wb) @ w, (wa * wb) @ w, f(C1), f(C2), f(2))
    assert s.dtype == f
    return s


def ssim_naive_fp32(a, b):
    """fp32 throughout in ONE pass, E[x x] - mu mu: the form the contract rules out.  -> s float32"""
    f = np.float32
    w = _w32()
    wa, wb = _windows(np.asarray(a, dtype=f)), _windows(np.asarray(b, dtype=f))
    mu_a, mu_b = wa @ w, wb @ w
    s = _score(mu_a, mu_b, (wa * wa) @ w - mu_a * mu_a, (wb * wb) @ w - mu_b * mu_b, (wa * wb) @ w - mu_a * mu_b, f(C1), f(C2), f(2))
    assert s.dtype == f
    return s


# the faults of the rule that the tolerance has to tell from the rule: keyword arguments of ssim_map / ssim
FAULTS = {
    "same_padding": dict(pad=True),
    "uniform_window": dict(window=np.full((TAPS, TAPS), 1.0 / (TAPS * TAPS))),
    "sigma_1.0": dict(window=np.multiply.outer(gaussian(1.0).astype(np.float64), gaussian(1.0).astype(np.float64))),
    "c2_of_range_1": dict(c2=0.03 ** 2),
}

# ----------------------------------------------------------------------------- the case list
SHAPES = [(2, 3, 11, 11), (2, 3, 12, 16), (2, 3, 11, 75), (2, 3, 75, 11), (2, 3, 43, 37), (2, 3, 64, 64), (2, 3, 97, 61), (1, 1, 128, 128)]
CONTENTS = ("random", "noise10", "flat250", "ramp", "step", "identical", "black_white")


def content(kind, shape, seed=0):
    """-> (a, b) levels (B, T, H, W, 3) uint8"""
    B, T, H, W = shape
    full = (B, T, H, W, 3)
    rng = np.random.default_rng([seed, CONTENTS.index(kind), H, W])
    u8 = lambda v: np.clip(v, 0, 255).astype(np.uint8)          # noqa: E731
    if kind == "random":
        return u8(rng.integers(0, 256, full)), u8(rng.integers(0, 256, full))
    if kind == "noise10":
        a = rng.integers(0, 256, full)
        return u8(a), u8(np.rint(a + rng.normal(0.0, 10.0, full)))
    if kind == "flat250":
        return u8(250 + rng.integers(0, 3, full)), u8(250 + rng.integers(0, 3, full))
    if kind == "ramp":
        base = np.rint(np.arange(W) * (255.0 / max(W - 1, 1))).astype(np.int64)[None, None, None, :, None]
        return u8(base + rng.integers(-2, 3, full)), u8(base + rng.integers(-2, 3, full))
    if kind == "step":
        base = np.where(np.arange(W) < W // 2, 0, 255)[None, None, None, :, None]
        return u8(base + rng.integers(-2, 3, full)), u8(base + rng.integers(-2, 3, full))
    if kind == "identical":
        a = u8(rng.integers(0, 256, full))
        return a, a.copy()
    if kind == "black_white":
        return np.zeros(full, dtype=np.uint8), np.full(full, 255, dtype=np.uint8)
    raise ValueError(kind)


def cases():
    """-> [(name, a levels, b levels)]: every plane size with every content"""
    return [(f"{kind}_{s[2]}x{s[3]}", *content(kind, s)) for s in SHAPES for kind in CONTENTS]


def float_operand(lv, inject=False, seed=0):
    """levels -> float32 clips (B, 3, T, H, W) with exactly these levels; inject: also values that de-normalise below 0 and above 1,
    infinities and NaNs scattered in (the levels then follow from gif_ref.levels_of)"""
    x = gif_ref.clips_from_levels(lv)
    if inject:
        flat = x.reshape(-1)
        rng = np.random.default_rng(seed)
        for value in (-4.0, 6.0, np.nan, np.inf, -np.inf):
            flat[rng.integers(0, flat.size, max(2, flat.size // 50))] = value
    return x


def window_error(case_list):
    """e_win: the worst |fp32 - fp64| of one window's s by the form that centres first, over the cases
    -> (e_win, {case: its worst}, {case: the rule's ssim (B, T, 3) fp64}); the rule is evaluated once for both"""
    per_case, means = {}, {}
    for name, a, b in case_list:
        pa, pb = planes(a), planes(b)
        rule = ssim_map(pa, pb)
        per_case[name] = float(np.abs(ssim_fp32(pa, pb).astype(np.float64) - rule).max())
        means[name] = rule.mean(axis=(-2, -1))
    return max(per_case.values()), per_case, means
