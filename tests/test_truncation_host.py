"""Top-r truncated sampling's host side (no GPU): the rule itself, restated in numpy and checked against the literal upstream
formulation (VQ-Diffusion's predict_start_with_truncation: sort, cumsum, shift, gather); the rejections at both levels; that
truncation_rate = None adds nothing to what reaches ops; the config key; the register budget of the truncated kernels.

The restatement here (mass_above, truncate_rows, boundary_margin) is the yardstick the GPU tests and the fixture generator import."""
import ctypes
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ----------------------------------------------------------------------------- the rule
def mass_above(x):
    """x: (B, C, L) log-probabilities, classes on axis 1 -> fp64 (B, C, L): sum_{j : x_j > x_k} exp(x_j) for every k.  Stated on
    values: exactly equal entries get the same mass."""
    x = np.asarray(x)
    xs = np.moveaxis(x, 1, -1).astype(np.float64)                       # (B, L, C)
    order = np.argsort(-xs, axis=-1, kind="stable")
    srt = np.take_along_axis(xs, order, -1)
    p = np.exp(srt)
    excl = np.cumsum(p, -1) - p                                          # mass of the entries sorted before this one
    # an entry that ties with its predecessor takes the mass of the first entry of its run
    first = np.concatenate([np.ones(srt.shape[:-1] + (1,), bool), srt[..., 1:] != srt[..., :-1]], -1)
    idx = np.where(first, np.arange(srt.shape[-1]), 0)
    idx = np.maximum.accumulate(idx, axis=-1)
    excl = np.take_along_axis(excl, idx, -1)
    out = np.empty_like(excl)
    np.put_along_axis(out, order, excl, -1)
    return np.moveaxis(out, -1, 1)


def truncate_rows(x, r):
    """The truncated row: class k is kept iff mass_above(k) < r, every other entry becomes -70; no renormalisation.  x is what
    cf_predict_start returns, (B, K + 1, L) with the [MASK] row at -70 (which stays -70 either way)."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(mass_above(x) < r, x, np.float32(-70)).astype(np.float32)


def boundary_margin(x, r):
    """(B, L): min_k |mass_above(k) - r|, how far the row's decision is from flipping for some class."""
    return np.abs(mass_above(x) - r).min(axis=1)


def upstream_truncate(out, truncation_r):
    """predict_start_with_truncation's 'r' wrapper body, literally (VQ-Diffusion, inference_VQ_Diffusion.py)."""
    temp, indices = torch.sort(out, 1, descending=True)
    temp1 = torch.exp(temp)
    temp2 = temp1.cumsum(dim=1)
    temp3 = temp2 < truncation_r
    new_temp = torch.full_like(temp3[:, 0:1, :], True)
    temp6 = torch.cat((new_temp, temp3), dim=1)
    temp3 = temp6[:, :-1, :]
    temp4 = temp3.gather(1, indices.argsort(1))
    temp5 = temp4.float() * out + (1 - temp4.float()) * (-70)
    return temp5


def random_rows(B, K, L, sigma, seed):
    """Rows shaped like cf_predict_start's output: log_softmax of N(0, sigma^2) logits clamped to [-70, 0], plus the [MASK] row."""
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, K, L, generator=g, dtype=torch.float64) * sigma, dim=1).float().clamp(-70, 0)
    return torch.cat([lp, torch.full((B, 1, L), -70.0)], dim=1)


@pytest.mark.parametrize("K,sigma,r", [(32, 2.0, 0.86), (512, 3.0, 0.86), (4096, 2.0, 0.86), (4096, 4.0, 0.5), (64, 1.0, 0.999)])
def test_restatement_agrees_with_the_upstream_formulation(K, sigma, r):
    x = random_rows(3, K, 16, sigma, seed=K + int(100 * r))
    xn = x.numpy()
    # rows without ties among the entries above the clamp (entries at -70 do not change whichever way they fall)
    srt = np.sort(xn[:, :-1], axis=1)
    tie_free = ~((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] > -70)).any(axis=1)
    assert tie_free.sum() >= 16                        # (at K = 4096 about half of the fp32 rows hold two equal entries somewhere)
    got = truncate_rows(xn, r)
    want64 = upstream_truncate(x.double(), r).float().numpy()
    sel = np.broadcast_to(tie_free[:, None, :], xn.shape)
    assert np.array_equal(got[sel], want64[sel])
    # upstream's own fp32 cumulative sum can only disagree within rounding of the boundary
    want32 = upstream_truncate(x, r).numpy()
    far_rows = tie_free & (boundary_margin(xn, r) > 1e-5)
    far = np.broadcast_to(far_rows[:, None, :], xn.shape)
    assert far_rows.sum() >= 8 and np.array_equal(got[far], want32[far])
    # properties: the maximum is always kept, kept entries are untouched, cut ones are exactly -70, the [MASK] row stays -70
    kept = got != -70
    assert kept[:, :-1].any(axis=1).all() and np.array_equal(got[kept], xn[kept]) and (got[:, -1] == -70).all()
    assert np.take_along_axis(kept, xn.argmax(axis=1)[:, None, :], 1).all()
    m = mass_above(xn)
    assert (m[kept] < r).all() and (m[~kept & (xn > -70)] >= r).all()


def test_equal_entries_are_kept_or_cut_together():
    lp = np.log(np.array([0.4, 0.2, 0.2, 0.1, 0.05, 0.05], dtype=np.float64)).astype(np.float32)
    x = np.concatenate([lp, [-70]]).astype(np.float32).reshape(1, 7, 1)
    keep = lambda r: (truncate_rows(x, r)[0, :, 0] != -70).tolist()
    assert keep(0.3) == [True, False, False, False, False, False, False]         # the first is always kept
    assert keep(0.5) == [True, True, True, False, False, False, False]           # mass above both 0.2 entries is 0.4 < 0.5
    assert keep(0.85) == [True, True, True, True, False, False, False]
    assert keep(0.95) == [True, True, True, True, True, True, False]
    m = mass_above(x)[0, :, 0]
    assert m[1] == m[2] and m[4] == m[5] and m[0] == 0


# ----------------------------------------------------------------------------- validation
@pytest.fixture(scope="module")
def tiny_dm():
    """The d3pm_L64 fixture's architecture on the CPU: argument checking only, nothing is computed."""
    import gsdd_amd
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=32, spatial_size=[8, 8], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=64, block_activate="GELU2",
                                        content_spatial_size=[8, 8], condition_dim=512, diffusion_step=100)
    return gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2,
                                         content_seq_len=64)


BAD_RATES = [0, 1, 1.0, -0.1, 1.5, True, False, "0.86", float("nan"), float("inf"), 1e-60, 1 - 1e-12, [0.5]]


def test_truncation_rate_rejections(tiny_dm):
    import gsdd_amd
    from gsdd_amd.d3pm import check_truncation_rate
    dm = tiny_dm
    assert dm.truncation_rate is None
    assert check_truncation_rate(None) is None and check_truncation_rate(0.86) == 0.86 and check_truncation_rate(np.float32(0.5)) == 0.5
    cond = torch.zeros(2, 1, 512)
    text = lambda texts: torch.zeros(len(texts), 512)
    try:
        for bad in BAD_RATES:
            dm.truncation_rate = bad
            # raised at the top of the call: before the device check (this model sits on the CPU) and before any other argument's
            with pytest.raises(gsdd_amd.GsddError, match="truncation_rate"):
                dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0)
            with pytest.raises(gsdd_amd.GsddError, match="truncation_rate"):
                dm.sample_fast(["a"] * 2, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=cond)
            dm.prior_rule = 2
            with pytest.raises(gsdd_amd.GsddError, match="truncation_rate"):
                dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0)
            dm.prior_rule = 0
            with pytest.raises(gsdd_amd.GsddError, match="truncation_rate"):
                dm.p_sample_tokens(torch.zeros(2, 64, dtype=torch.long), cond, cond, torch.zeros(2, dtype=torch.long), 0, truncation_rate=bad)
            with pytest.raises(gsdd_amd.GsddError, match="sample_truncation_rate"):
                gsdd_amd.DiscreteDiffusion(text, dm, sample_truncation_rate=bad)
    finally:
        dm.truncation_rate, dm.prior_rule = None, 0
    # r = 1: the message says why and points to None
    with pytest.raises(gsdd_amd.GsddError, match=r"rounding.*None"):
        check_truncation_rate(1)


def test_none_adds_nothing_to_what_reaches_ops(tiny_dm, monkeypatch):
    """truncation_rate = None: the sampler passes no truncation keyword on, and ops fills the descriptor it filled before (trunc_rate
    0 = off, every other byte equal)."""
    import gsdd_amd
    from gsdd_amd import ops
    from gsdd_amd.d3pm import DiffusionTransformer, _trunc_kwargs
    assert _trunc_kwargs(None) == {} and _trunc_kwargs(0.86) == {"trunc_rate": 0.86}
    seen = []
    monkeypatch.setattr(DiffusionTransformer, "_sample_once",
                        lambda self, plan, *a, **kw: seen.append(kw.get("truncation_rate", "absent")) or {"content_token": None})
    monkeypatch.setattr(DiffusionTransformer, "_range_flags", [], raising=False)
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    try:
        for rate in (None, 0.86):
            dm.truncation_rate = rate
            dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0)
            dm.sample_fast(["a"] * 2, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=cond)
            dm.prior_rule = 2
            dm.n_sample = [1] + [0] * 35 + [1] * 64
            dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0)
            dm.prior_rule = 0
    finally:
        dm.truncation_rate, dm.prior_rule = None, 0
        dm.update_n_sample()
    assert seen == [None] * 3 + [0.86] * 3

    # the descriptors
    class FakeLib:
        def __init__(self):
            self.descs = []

        def _take(self, ref, stream):
            d = ref._obj
            self.descs.append((type(d), bytes(memoryview(d).cast("B")), d.trunc_rate))
            return 0
        gsdd_d3pm_step = gsdd_d3pm_purity_step = _take

    fake = FakeLib()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    B, L, K = 2, 4, 8
    lc, tok, sid = torch.zeros(B * L, K), torch.zeros(B, L, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    sched = [torch.zeros(101)] * 8
    f, t, smax = torch.zeros(B, L), torch.zeros(B, dtype=torch.long), torch.zeros(B)
    for kw in ({}, {"trunc_rate": None}, {"trunc_rate": 0.86}):
        ops.d3pm_step(lc, lc, tok, tok, sched, t, sid, K=K, T=100, guidance=2.0, seed=1, post_skip=1, **kw)
        ops.d3pm_purity_step(lc, lc, f, smax, tok, sid, K=K, guidance=2.0, prior_rule=2, prior_weight=1.0, seed=1, **kw)
    (s0, p0, s1, p1, s2, p2) = fake.descs
    assert s0[0] is gsdd_amd._lib.StepDesc and p0[0] is gsdd_amd._lib.PurityDesc
    assert s0 == s1 and p0 == p1 and s0[2] == 0.0 and p0[2] == 0.0
    assert s2[2] == p2[2] == ctypes.c_float(0.86).value and s2[1] != s0[1] and p2[1] != p0[1]


def test_config_key_reaches_the_model(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.sample_truncation_rate is None
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.sample_truncation_rate=0.86"]).model.generator
    assert gen.sample_truncation_rate == 0.86
    text = lambda texts: torch.zeros(len(texts), 512)
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm).sample_truncation_rate is None
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_truncation_rate=gen.sample_truncation_rate, sample_skip_step=1)
    assert dd.sample_truncation_rate == 0.86

    # sample_videos hands it to the diffusion model before it samples (and leaves it alone when the key is null)
    class Auto:
        device = torch.device("cpu")
        latent_shape = (64,)
        decode = staticmethod(lambda tok: tok)
    seen = []

    def fake_sample_fast(*a, **kw):
        seen.append(tiny_dm.truncation_rate)
        return {"content_token": torch.zeros(2, 64, dtype=torch.long)}
    monkeypatch.setattr(tiny_dm, "sample_fast", fake_sample_fast, raising=False)
    try:
        dd.sample_videos(["a", "b"], Auto())
        tiny_dm.truncation_rate = 0.5
        gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_skip_step=1).sample_videos(["a", "b"], Auto())
    finally:
        tiny_dm.truncation_rate = None
    assert seen == [0.86, 0.5]


def test_abi_carries_the_truncation_rate():
    import gsdd_amd
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    assert header.count("float trunc_rate;") == 2
    L = gsdd_amd.lib()                                   # (lib() checks both descriptors' sizes against gsdd_abi_sizeof)
    assert L.gsdd_version() >= 102
    for cls in (gsdd_amd._lib.StepDesc, gsdd_amd._lib.PurityDesc):
        assert cls._fields_[-1] == ("trunc_rate", ctypes.c_float)


# ----------------------------------------------------------------------------- the kernels' registers
@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_truncated_production_kernels_have_no_scratch():
    """K = 4096 without test hooks: d3pm_step_trunc_kernel<16, true, false> and d3pm_purity_trunc_kernel<16, true, {0, 2}, false> keep
    the row and its exponentials in registers, no scratch at two waves per SIMD; the tool lists both source files."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_step.hip" in mod.SOURCES and "d3pm_purity.hip" in mod.SOURCES
    rows = mod.collect(["d3pm_step.hip", "d3pm_purity.hip"])
    for name in ("d3pm_step_trunc_kernel<16, true, false>", "d3pm_purity_trunc_kernel<16, true, 0, false>",
                 "d3pm_purity_trunc_kernel<16, true, 2, false>"):
        r = [r for r in rows if r["kernel"].startswith(name)]
        assert len(r) == 1, (name, [x["kernel"] for x in rows])
        assert r[0]["scratch_bytes_per_lane"] == 0 and r[0]["vgprs"] <= 256 and r[0]["occupancy_waves_per_simd"] >= 2, r[0]
