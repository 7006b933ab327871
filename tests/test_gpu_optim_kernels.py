"""The optimiser stage's kernels (csrc/optim.hip: gsdd_grad_sqnorm, gsdd_grad_norm_finalize, gsdd_adamw_ema_multi, gsdd_swap_multi)
through _optim.MultiAdam, against an fp64 restatement -- torch.nn.utils.clip_grad_norm_ -> torch.optim.AdamW -> the running average
with its warm-up decay -- of the same f32 inputs, in the layout of test_adam_multi_matches_fp64: tensors of 1, 3, 4095, 4096, 4097 and
3 * 4096 + 5 elements as views of one sentinel-filled buffer with gaps of 7 floats (so most parameters and gradients are NOT 16-byte
aligned: the element-by-element path; the "aligned16" cases put every view on a 16-byte boundary: the four-wide path), a nonzero state
with sentinel-filled padding.  Gaps and padding must come back bit for bit.

Bars, per element, U = 2^-24, |.| of the exact values (no fitted constants):
  * norm: the partial sums are exact to ~1e-16 n, so the f32 result is the rounding of the fp64 norm: one f32 ulp.  The coefficient
    min(1, max_norm / (norm + 1e-6)) is formed in double on the device and rounded once: one ulp.
  * g' = coef g: e_g = 2 U (the coefficient's rounding, the product) when clipping is on, else 0 (coef = 1 exactly).
  * m' = b1 m + (1 - b1) g': 2 U (|b1 m| + |(1 - b1) g'|) + e_g |(1 - b1) g'|.
  * v' = b2 v + (1 - b2) g'^2: three roundings in the second term, one in the first, one in the sum, and g'^2 carries 2 e_g:
    (4 U + 2 e_g) v'.
  * decay p_d = p (1 - lr wd): the factor carries 2 U, the product U: 3 U |p_d| on tensors that decay, 0 (bit-equal) on the others.
  * the step dp = (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)), bias corrections in double on the device (4 U beta^s / (1 - beta^s)
    + U each, as in test_adam_multi_matches_fp64): (lr / bc1) e_m' / den + |dp| (e_bc1 + (e_v' / v' + e_bc2) / 2 (sq / den) + 8 U).
    p' = p_d - dp adds U |p'|.
  * e' = d e + (1 - d) p', d = min(ema_decay, (1 + s) / (10 + s)) formed in double and rounded to f32 (U d absolute, which is also the
    absolute error of 1 - d: the subtraction is exact for d >= 1/2 and rounds once below): 2 U |d e| + (U d + 2 U (1 - d)) |p'|
    + (1 - d) bar_p' + U |e'|."""
import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import parity_report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149
SENT = -7777.0
GAP = 7
SIZES = [1, 3, 4095, 4096, 4097, 3 * 4096 + 5]
LR, B1, B2, EPS, WD, EMA = 1e-3, 0.5, 0.999, 1e-8, 0.05, 0.999
f32 = lambda z: float(np.float32(z))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def ratio(got, want, bar):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    return float(torch.where(err == 0, 0.0, err / bar).max())


class Layout:
    """parameters as gapped views of one sentinel-filled buffer, gradients, and a MultiAdam over them with a nonzero state"""

    def __init__(self, seed, sizes=SIZES, align=False, **opts):
        from gsdd_amd._optim import MultiAdam
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.sizes = list(sizes)
        total = sum(n + GAP + 3 for n in sizes) + GAP
        self.pbuf = torch.full((total,), SENT, device="cuda")
        self.gbuf = torch.full((total,), SENT, device="cuda")
        self.params, self.grads, self.poffs, off = [], {}, [], GAP
        for i, n in enumerate(sizes):
            if align:                                   # every view on a 16-byte boundary: the four-wide path of p and g
                off = (off + 3) & ~3
            self.poffs.append(off)
            p = self.pbuf[off:off + n]
            p.copy_(torch.randn(n, generator=g, device="cuda"))
            self.params.append((f"p{i}", p))
            gr = self.gbuf[off:off + n]
            gr.copy_(torch.randn(n, generator=g, device="cuda") * 1e-2)
            gr[::11] = 0.0
            self.grads[f"p{i}"] = gr
            off += n + GAP
        self.opt = opt = MultiAdam(self.params, LR, (B1, B2), EPS, **opts)
        self.pad = torch.ones_like(opt.m, dtype=torch.bool)
        for (_, p), o in zip(self.params, opt.offs[:-1]):
            self.pad[int(o):int(o) + p.numel()] = False
        opt.m.copy_(torch.randn(opt.m.shape, generator=g, device="cuda") * 1e-2)
        opt.v.copy_(torch.rand(opt.v.shape, generator=g, device="cuda") * 1e-4)
        opt.m[self.pad] = SENT
        opt.v[self.pad] = SENT
        if opt.ema is not None:
            opt.ema.copy_(torch.randn(opt.ema.shape, generator=g, device="cuda"))
            opt.ema[self.pad] = SENT
        self.gap_mask = torch.ones(total, dtype=torch.bool, device="cuda")
        for po, n in zip(self.poffs, sizes):
            self.gap_mask[po:po + n] = False
        self.snapshot()

    def snapshot(self):
        o = self.opt
        self.p0, self.g0, self.m0, self.v0 = self.pbuf.clone(), self.gbuf.clone(), o.m.clone(), o.v.clone()
        self.e0 = None if o.ema is None else o.ema.clone()

    def slices(self):
        for (name, p), o, po in zip(self.params, self.opt.offs[:-1], self.poffs):
            yield name, p, slice(int(o), int(o) + p.numel()), slice(po, po + p.numel())

    def untouched(self):
        """gaps of the parameter buffer, the whole gradient buffer (gradients are never rewritten), the padding of m, v and ema"""
        o = self.opt
        ok = bool(torch.equal(self.pbuf[self.gap_mask], self.p0[self.gap_mask])) and bool(torch.equal(self.gbuf, self.g0))
        ok = ok and bool(torch.equal(o.m[self.pad], self.m0[self.pad])) and bool(torch.equal(o.v[self.pad], self.v0[self.pad]))
        return ok and (o.ema is None or bool(torch.equal(o.ema[self.pad], self.e0[self.pad])))

    def state_equal(self):
        o = self.opt
        return (bool(torch.equal(self.pbuf, self.p0)) and bool(torch.equal(o.m, self.m0)) and bool(torch.equal(o.v, self.v0))
                and (o.ema is None or bool(torch.equal(o.ema, self.e0))))

    def norm64(self):
        return math.sqrt(sum(float((g.double() ** 2).sum()) for g in self.grads.values()))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ----------------------------------------------------------------------------- norm, coefficient
@pytest.mark.parametrize("sizes", [SIZES, SIZES + [257 * 4096 + 1]], ids=["six_tensors", "more_partials_than_lanes"])
def test_norm_and_clip_coefficient(G, sizes):
    from gsdd_amd import ops
    L = Layout(3, sizes, max_grad_norm=1.0)
    opt = L.opt
    table = torch.from_numpy(opt._build_table(L.grads)).cuda()
    assert table.shape == (opt.n_blocks, 7) and (opt.n_blocks > 256) == (len(sizes) > len(SIZES))
    want = L.norm64()
    got = {}
    for name, max_norm in (("above", 2.0 * want), ("below", 0.25 * want), ("again", 0.25 * want)):
        opt.partials.fill_(-1.0)
        ops.grad_sqnorm(table, opt.partials)
        ops.grad_norm_finalize(opt.partials, opt.n_blocks, max_norm, True, opt.words)
        got[name] = (opt.words.clone(), opt.partials.clone())
        norm, coef = float(opt.grad_norm), float(opt.clip_coef)
        c64 = min(1.0, f32(max_norm) / (want + 1e-6))
        rec = {"norm_err_ulp": abs(norm - want) / ulp32(want), "coef_err_ulp": abs(coef - c64) / ulp32(c64)}
        parity_report(f"optim_kernels::norm[{len(sizes)}_{name}]", rec)
        assert abs(norm - want) <= ulp32(want), (norm, want)
        assert abs(coef - c64) <= ulp32(c64), (coef, c64)
        assert (coef == 1.0) == (name == "above")
        assert int(opt.words[7]) == 1 and opt.skipped_steps == 0
    assert torch.equal(got["below"][0], got["again"][0]) and torch.equal(got["below"][1], got["again"][1])     # the same bits
    # the partials are the blocks' own sums
    first = float((L.grads["p0"].double() ** 2).sum())
    assert abs(float(got["below"][1][0]) - first) <= 1e-15 * first
    assert L.state_equal() and L.untouched()


# ----------------------------------------------------------------------------- the update
CONFIGS = {
    "clip": dict(max_grad_norm="below"),
    "decay": dict(weight_decay=WD, decay_mask="alternate"),
    "ema": dict(ema_decay=EMA),
    "all": dict(max_grad_norm="below", weight_decay=WD, decay_mask="alternate", ema_decay=EMA),
}


def build(seed, cfg, align=False):
    cfg = dict(cfg, align=align)
    if cfg.get("decay_mask") == "alternate":
        cfg["decay_mask"] = {f"p{i}": i % 2 == 0 for i in range(len(SIZES))}        # every second tensor is exempt
    below = cfg.get("max_grad_norm") == "below"
    if below:
        cfg["max_grad_norm"] = 1.0
    L = Layout(seed, **cfg)
    if below:
        L.opt.max_grad_norm = 0.37 * L.norm64()
    return L


def tensor_reference(pd, g, md, vd, ed, *, step, lr, wd, dec, coef, eg, d, b1=None, b2=None, eps=None):
    """One tensor, fp64 (the module docstring's restatement and bars): p, g (unclipped), m, v, e (or None) ->
    (p1, bar_p, m1, bar_m, v1, bar_v, e1, bar_e).  coef: the clip coefficient in fp64, eg its error (2 U, or 0 without clipping);
    d: the average's effective decay or None."""
    b1, b2, eps = f32(B1 if b1 is None else b1), f32(B2 if b2 is None else b2), f32(EPS if eps is None else eps)
    c1, c2 = 1 - b1 ** step, 1 - b2 ** step
    e_c1 = 4 * U * b1 ** step / c1 + U
    e_c2 = 4 * U * b2 ** step / c2 + U
    gd = g * coef
    m1 = b1 * md + (1 - b1) * gd
    v1 = b2 * vd + (1 - b2) * gd * gd
    e_m = 2 * U * ((b1 * md).abs() + ((1 - b1) * gd).abs()) + eg * ((1 - b1) * gd).abs()
    e_v = (4 * U + 2 * eg) * v1
    pdec = pd * (1 - lr * wd) if dec else pd
    e_pd = 3 * U * pdec.abs() if dec else torch.zeros_like(pd)
    sq = (v1 / c2).sqrt()
    den = sq + eps
    dp = lr / c1 * m1 / den
    p1 = pdec - dp
    bar_p = e_pd + lr / c1 * e_m / den + dp.abs() * (e_c1 + (e_v / v1.clamp(min=1e-300) + e_c2) / 2 * (sq / den) + 8 * U) + U * p1.abs()
    e1 = bar_e = None
    if d is not None:
        e1 = d * ed + (1 - d) * p1
        bar_e = 2 * U * (d * ed).abs() + (U * d + 2 * U * (1 - d)) * p1.abs() + (1 - d) * bar_p + U * e1.abs() + TINY
    return p1, bar_p + TINY, m1, e_m + TINY, v1, e_v + TINY, e1, bar_e


def reference_and_bars(L, step, ema_d=None):
    """fp64 restatement of one step from L's snapshot -> {name: tensor_reference(...)}"""
    opt = L.opt
    coef, eg = 1.0, 0.0
    if opt.max_grad_norm is not None:
        coef, eg = min(1.0, f32(opt.max_grad_norm) / (L.norm64() + 1e-6)), 2 * U
    d = None
    if opt.ema is not None:
        d = min(f32(opt.ema_decay), (1.0 + step) / (10.0 + step)) if ema_d is None else ema_d
    out = {}
    for (name, p, sl, psl), dec in zip(L.slices(), opt.decays):
        out[name] = tensor_reference(L.p0[psl].double(), L.grads[name].double(), L.m0[sl].double(), L.v0[sl].double(),
                                     None if d is None else L.e0[sl].double(), step=step, lr=f32(opt.lr), wd=f32(opt.weight_decay),
                                     dec=dec, coef=coef, eg=eg, d=d)
    return out


@pytest.mark.parametrize("align", [False, True], ids=["gap7", "aligned16"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_update_matches_fp64(G, step, cfg, align):
    L = build(10 * step + len(cfg), CONFIGS[cfg], align)
    opt = L.opt
    if align:
        assert all(p.data_ptr() % 16 == 0 and L.grads[nm].data_ptr() % 16 == 0 for nm, p in L.params)
    else:
        assert sum(p.data_ptr() % 16 != 0 for _, p in L.params) >= 4
    opt.step_count = step - 1
    opt.step(L.grads)
    ref = reference_and_bars(L, step)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "e": 0.0}
    for name, p, sl, _ in L.slices():
        p1, bar_p, m1, bar_m, v1, bar_v, e1, bar_e = ref[name]
        worst["p"] = max(worst["p"], ratio(p, p1, bar_p))
        worst["m"] = max(worst["m"], ratio(opt.m[sl], m1, bar_m))
        worst["v"] = max(worst["v"], ratio(opt.v[sl], v1, bar_v))
        if e1 is not None:
            worst["e"] = max(worst["e"], ratio(opt.ema[sl], e1, bar_e))
    parity_report(f"optim_kernels::update[{cfg}_step{step}_{'aligned16' if align else 'gap7'}]", {**{k + "_ratio": v for k, v in worst.items()}, "worst_ratio": max(worst.values())})
    assert L.untouched(), "the update wrote a gap, a gradient or the padding of m / v / ema"
    assert max(worst.values()) <= 1, worst
    if opt.max_grad_norm is not None:
        assert float(opt.clip_coef) < 1.0
    if opt.ema is not None and step == 1:
        # the warm-up: the effective decay at step 1 is 2 / 11, not 0.999 -- against the 0.999 restatement the result is far outside
        assert min(f32(EMA), 2.0 / 11.0) == 2.0 / 11.0
        far = reference_and_bars(L, step, ema_d=f32(EMA))
        name, _, sl, _ = list(L.slices())[-1]
        assert ratio(opt.ema[sl], far[name][6], far[name][7]) > 1e3
    if "decay_mask" in CONFIGS[cfg]:
        # exempt tensors: bit for bit what the same optimiser gives without weight decay
        plain = dict(CONFIGS[cfg], weight_decay=0.0, device_lr=True)          # (device_lr: the stage's kernel with nothing else on)
        plain.pop("decay_mask")
        L2 = build(10 * step + len(cfg), plain, align)
        assert torch.equal(L2.p0, L.p0) and torch.equal(L2.m0, L.m0)
        L2.opt.step_count = step - 1
        L2.opt.step(L2.grads)
        for i, ((name, p, sl, _), (_, p2, _, _)) in enumerate(zip(L.slices(), L2.slices())):
            assert opt.decays[i] == (i % 2 == 0)
            assert torch.equal(p, p2) != opt.decays[i], name
            assert torch.equal(opt.m[sl], L2.opt.m[sl]) and torch.equal(opt.v[sl], L2.opt.v[sl])


# ----------------------------------------------------------------------------- the non-finite guard
@pytest.mark.parametrize("case", ["nan_in_4097", "inf_in_1"])
def test_nonfinite_gradient_skips_the_update(G, case):
    L = build(77, dict(CONFIGS["all"], skip_nonfinite=True))
    opt = L.opt
    name, idx, bad = ("p4", 2049, float("nan")) if case == "nan_in_4097" else ("p0", 0, float("inf"))
    assert L.grads[name].numel() == (4097 if name == "p4" else 1)
    keep = L.grads[name][idx].clone()
    L.grads[name][idx] = bad
    L.snapshot()
    opt.step_count = 4
    opt.step(L.grads)
    assert L.state_equal(), "a skipped step wrote p, m, v or the average"
    assert opt.skipped_steps == 1 and int(opt.words[7]) == 0 and not math.isfinite(float(opt.grad_norm))
    assert opt.step_count == 5                       # the count advances all the same
    L.grads[name][idx] = keep
    L.snapshot()
    opt.max_grad_norm = 0.37 * L.norm64()
    opt.step(L.grads)
    ref = reference_and_bars(L, 6)
    worst = 0.0
    for nm, p, sl, _ in L.slices():
        p1, bar_p, m1, bar_m, v1, bar_v, e1, bar_e = ref[nm]
        worst = max(worst, ratio(p, p1, bar_p), ratio(opt.m[sl], m1, bar_m), ratio(opt.v[sl], v1, bar_v), ratio(opt.ema[sl], e1, bar_e))
    assert worst <= 1, worst
    assert not L.state_equal() and opt.skipped_steps == 1 and int(opt.words[7]) == 1 and L.untouched()


def test_nonfinite_without_the_guard_is_not_counted(G):
    """skip_nonfinite off: the flag stays 1 and nothing is counted (the NaN goes through, as with clip_grad_norm_ + AdamW)"""
    L = build(78, CONFIGS["clip"])
    L.grads["p4"][7] = float("nan")
    L.opt.step(L.grads)
    assert int(L.opt.words[7]) == 1 and L.opt.skipped_steps == 0 and bool(torch.isnan(L.params[1][1]).all())


# ----------------------------------------------------------------------------- swap
@pytest.mark.parametrize("align", [False, True], ids=["gap7", "aligned16"])
def test_swap_exchanges_parameters_and_average_exactly(G, align):
    L = build(5, CONFIGS["ema"], align)
    opt = L.opt
    opt.swap_ema()
    for _, p, sl, psl in L.slices():
        assert torch.equal(p, L.e0[sl]) and torch.equal(opt.ema[sl], L.p0[psl])
    assert L.untouched() and torch.equal(opt.m, L.m0) and torch.equal(opt.v, L.v0)
    opt.swap_ema()
    assert L.state_equal()


# ----------------------------------------------------------------------------- defaults: the parent's path
@pytest.mark.parametrize("step", [1, 1000])
def test_defaults_are_the_plain_adam_launch(G, step):
    """every new option at its default: MultiAdam.step is gsdd_adam_multi on the table it always built -- the same bits as a direct call"""
    from gsdd_amd._lib import lib, ptr, stream_ptr, check
    A, Bq = Layout(9), Layout(9)
    assert not A.opt.staged and A.opt.words is None and A.opt.ema is None and torch.equal(A.p0, Bq.p0)
    A.opt.step_count = step - 1
    A.opt.step(A.grads)
    assert A.opt._table.shape[1] == 5
    rows = []
    for name, p, sl, _ in Bq.slices():
        for s in range(0, p.numel(), 4096):
            rows.append([p.data_ptr() + 4 * s, Bq.grads[name].data_ptr() + 4 * s, Bq.opt.m.data_ptr() + 4 * (sl.start + s),
                         Bq.opt.v.data_ptr() + 4 * (sl.start + s), min(4096, p.numel() - s)])
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    check(lib().gsdd_adam_multi(ptr(table), table.shape[0], LR, B1, B2, EPS, step, stream_ptr()))
    assert torch.equal(A.pbuf, Bq.pbuf) and torch.equal(A.opt.m, Bq.opt.m) and torch.equal(A.opt.v, Bq.opt.v)
    assert not torch.equal(A.pbuf, A.p0)


# ----------------------------------------------------------------------------- the stage with nothing on: plain Adam, the recorded bits
def ordered(words):
    """f32 bit patterns -> integers whose differences count ulps"""
    a = words.view(np.int32).astype(np.int64)
    return np.where(a < 0, -(a & 0x7FFFFFFF), a)


@pytest.mark.parametrize("align", [False, True], ids=["gap7", "aligned16"])
def test_stage_with_nothing_on_gives_the_recorded_plain_adam_bits(G, align):
    """gsdd_adamw_ema_multi with clip coefficient 1, no decay and no average (device_lr: the stage's kernel with nothing else on) is plain
    Adam.  tests/golden/adam_plain_bits.npz holds the p, m and v words that gsdd_adam_multi_dev, the captured training step's plain Adam
    kernel, wrote on the MI355X for the fixture's inputs at steps 1, 2 and 1000 (tests/golden/make_golden_adam_plain.py).  The stage's
    kernel must give the same words on the element-wise path (gap7: every p and g misaligned) and on the four-wide one (aligned16): the
    arithmetic does not depend on the load width.  No tolerance: a differing word is a finding about the kernel, reported as a count and
    the largest distance in ulps."""
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_plain_bits.npz"), allow_pickle=False)
    sizes = [int(n) for n in fx["sizes"]]
    assert sizes == [1, 3, 4095, 4097] and tuple(fx["hyper"]) == (LR, B1, B2, EPS) and [int(s) for s in fx["steps"]] == [1, 2, 1000]
    L = Layout(9, sizes, align, device_lr=True)
    opt = L.opt
    assert opt.staged and opt.ema is None and opt.decays == [False] * 4
    assert all((p.data_ptr() % 16 == 0 and L.grads[nm].data_ptr() % 16 == 0) == align for nm, p in L.params)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for (name, p, sl, _), s in zip(L.slices(), starts):
        for dst, key in ((p, "p"), (L.grads[name], "g"), (opt.m[sl], "m"), (opt.v[sl], "v")):
            dst.copy_(torch.from_numpy(fx[key][s:s + p.numel()]))
    assert all(float(L.grads[nm][0]) == 0.0 for nm, _ in L.params)           # (every 11th gradient is exactly zero)
    L.snapshot()
    bad = {}
    for step in (1, 2, 1000):
        L.pbuf.copy_(L.p0)
        opt.m.copy_(L.m0)
        opt.v.copy_(L.v0)
        opt.step_count = step - 1
        opt.step(L.grads)
        assert opt._table.shape[1] == 7
        for which in "pmv":
            got = np.concatenate([(p if which == "p" else getattr(opt, which)[sl]).cpu().numpy() for _, p, sl, _ in L.slices()])
            got, want = got.view(np.uint32), fx[f"{which}_step{step}"]
            assert got.shape == want.shape == (sum(sizes),)
            n_bad = int((got != want).sum())
            if n_bad:
                bad[f"{which}_step{step}"] = (n_bad, int(np.abs(ordered(got) - ordered(want)).max()))
        assert L.untouched(), "the update wrote a gap, a gradient or the padding of m / v"
        assert not L.state_equal() and opt.ema is None
        words = opt.words.cpu().numpy()
        assert int(opt.words.view(torch.int64)[0]) == step and words.view(np.float32)[4] == np.float32(LR)
        assert words.view(np.float32)[5] == 0.0 and words.view(np.float32)[6] == 1.0 and words[7] == 1 and opt.skipped_steps == 0
    parity_report(f"optim_kernels::plain_adam_bits[{'aligned16' if align else 'gap7'}]",
                  {"words_compared": 9 * sum(sizes), "words_differing": sum(n for n, _ in bad.values()),
                   "max_ulps": max([u for _, u in bad.values()], default=0)})
    assert not bad, f"(words differing, largest distance in ulps) from the recorded plain Adam bits: {bad}"
