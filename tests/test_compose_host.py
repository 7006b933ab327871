"""Composed guidance, host side (no GPU): the algebra of the restatement (tests/compose_ref.py), the committed inputs' leave-out share
on the reference alone, that an f32 emulation of the restatement meets every bar of test_gpu_compose.py on every case (the bars are
not below fp32's own noise), that each injected fault comes out above a bar or as a token mismatch, the sampler's and the glue's
GsddError cases, the config keys, and the C ABI's argument refusals (each returns before anything is launched)."""
import ctypes
import os

import pytest
import torch

from tests import compose_ref as cr
from tests.test_cond_dropout_host import tiny_dm
from tests.test_gpu_objective_kernels import LOW_MARGIN_CAP
from tests.test_gpu_sampler_widths import B, GUIDANCE, L, case, recon
from tests.test_gpu_truncation import GAP_FLOOR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGEBRA_K = [260, 1020]


# ----------------------------------------------------------------------------- (a) algebra on the restatement
@pytest.mark.parametrize("K", ALGEBRA_K)
def test_weights_s_and_1_minus_s_are_the_two_way_mix_with_the_second_condition_as_cf(K):
    c = case(K, True)
    g = torch.Generator().manual_seed(5)
    neg, null = c["lc"] + torch.randn(c["lc"].shape, generator=g), c["lu"]
    s = GUIDANCE
    w = torch.tensor([[s, 1 - s]]).expand(B, 2)
    e = cr.compose([c["lc"], neg, null], w, torch.float64)
    lsm = lambda x: torch.log_softmax(x.double(), 1).clamp(-70, 0)
    assert float((e - (lsm(neg) + s * (lsm(c["lc"]) - lsm(neg)))).abs().max()) < 1e-11          # x_u cancels
    assert float((recon(e, None, torch.float64) - recon(c["lc"], neg, torch.float64)).abs().max()) < 1e-11


@pytest.mark.parametrize("K", ALGEBRA_K)
def test_one_condition_at_weight_s_is_the_guided_row(K):
    c = case(K, True)
    e = cr.compose([c["lc"], c["lu"]], torch.full((B, 1), GUIDANCE), torch.float64)
    assert float((recon(e, None, torch.float64) - recon(c["lc"], c["lu"], torch.float64)).abs().max()) < 1e-11


@pytest.mark.parametrize("K", ALGEBRA_K)
def test_a_zero_weight_removes_its_condition(K):
    I = cr.inputs(K, "w1_0.75_-0.25")
    w = I["w"].clone()
    w[:, 1] = 0
    with_it = cr.compose(I["blocks"], w, torch.float64)
    without = cr.compose([I["blocks"][0], I["blocks"][2], I["blocks"][3]], w[:, [0, 2]], torch.float64)
    assert torch.equal(with_it, without)
    # ... and all weights zero leave the unconditional row, bit for bit, in both precisions (what test_gpu_compose holds the kernel's
    # log-softmax against the step's with)
    for dt in (torch.float64, torch.float32):
        xu = torch.log_softmax(I["blocks"][-1].double(), 1).to(dt).clamp(-70, 0)
        assert torch.equal(cr.compose(I["blocks"], torch.zeros_like(w), dt), xu)


# ----------------------------------------------------------------------------- (b) - (e) inputs, leave-out share, emulation
def test_the_cases_are_the_issues():
    assert cr.KS == [4, 252, 256, 260, 512, 1024, 2048, 4092, 4100, 8192, 4096, 1020, 2044] and (B, L) == (3, 37)
    sets = {n: cr.weights_of(n) for n in cr.WEIGHT_SETS}
    assert [w.shape[1] for w in sets.values()] == [1, 2, 3, 4, 3] and all(w.shape[0] == B for w in sets.values())
    assert sets["w2"][0].tolist() == [2] and sets["w1.5_-0.5"][0].tolist() == [1.5, -0.5]
    assert sets["w1_0.75_-0.25"][0].tolist() == [1, 0.75, -0.25] and sets["w1.5_0.75_-0.5_-0.25"][0].tolist() == [1.5, 0.75, -0.5, -0.25]
    m = sets["matrix"]
    assert int((m == 0).sum()) >= 1 and len({tuple(r.tolist()) for r in m}) == B
    I = cr.inputs(4100, "w1.5_0.75_-0.5_-0.25")
    assert len(I["blocks"]) == 5 and I["blocks"][0] is case(4100, True)["lc"] and I["blocks"][-1] is case(4100, True)["lu"]
    assert all(b.shape == (B, 4100, L) for b in I["blocks"])


@pytest.mark.parametrize("K,name", cr.CASES, ids=cr.CASE_IDS)
def test_reference_leave_out_share_and_f32_emulation(K, name):
    """(d) on the reference alone: positions whose fp64 top-two Gumbel gap is below GAP_FLOOR are at most LOW_MARGIN_CAP (1 %) of the
    case.  (e) the restatement in plain f32 arithmetic meets every bar."""
    R = cr.reference(K, name)
    left_out = int((R["gap"] < GAP_FLOOR).sum())
    assert left_out <= LOW_MARGIN_CAP == 1, left_out
    assert R["e"].shape == (B, K, L) and bool(torch.isfinite(R["e"]).all())
    E = cr.restate(K, name, torch.float32)
    rec = cr.check(E, R)
    print(K, name, rec)
    assert not cr.failures(rec), rec


# ----------------------------------------------------------------------------- (f) injected faults
@pytest.mark.parametrize("fault", cr.FAULTS)
def test_injected_fault_is_caught(fault):
    """mix_not_in_log_softmax_space: the raw logits mixed; xu_dropped: sum_i w_i x_i (equal to the contract exactly where the weights
    sum to 1: caught in every other case); weights_of_sample_0: row 0 of the weights for every sample (the matrix cases);
    last_quad_dropped: the last four classes never written; null_block_first: block 0 read as the null condition."""
    caught = {}
    for (K, name), cid in zip(cr.CASES, cr.CASE_IDS):
        if K not in (4, 260, 1020, 4096, 4100):
            continue
        if fault == "weights_of_sample_0" and name != "matrix":
            continue
        if fault == "xu_dropped" and abs(float(cr.weights_of(name)[0].sum()) - 1) < 1e-6 and name != "matrix":
            continue
        caught[cid] = cr.failures(cr.check(cr.restate(K, name, torch.float32, fault), cr.reference(K, name)))
    assert caught and all(caught.values()), [n for n, v in caught.items() if not v]


# ----------------------------------------------------------------------------- (g) refusals
def test_check_compose_refusals():
    import gsdd_amd
    from gsdd_amd.d3pm import Compose, check_compose
    cond = torch.zeros(4, 3, 8)
    ok = [torch.ones(4, 3, 8)]
    assert check_compose(None, None, None, cond, 4) is None
    c = check_compose(ok, [2.0, -1.0], None, cond, 4)
    assert isinstance(c, Compose) and c.weights.shape == (4, 2) and c.weights.dtype == torch.float32 and c.lens is None
    assert c.weights[3].tolist() == [2.0, -1.0]
    c = check_compose(ok * 3, torch.arange(16.0).view(4, 4), [[1, 2, 3, 3]] * 3, cond, 4)
    assert c.weights[1].tolist() == [4, 5, 6, 7] and len(c.lens) == 3 and c.lens[0].dtype == torch.int32
    bad = [
        (dict(e=None, w=[1.0, 1.0]), "need compose_embeds"),
        (dict(e=[], w=[1.0]), "list of 1"),
        (dict(e=ok * 4, w=[1.0] * 5), "at most 4"),
        (dict(e=[torch.ones(4, 2, 8)], w=[1.0, 1.0]), "like condition_embed"),
        (dict(e=[torch.ones(4, 3, 8, device="meta")], w=[1.0, 1.0]), "like condition_embed"),
        (dict(e=ok, w=None), "needs compose_weights"),
        (dict(e=ok, w=[1.0]), "compose_weights must be"),
        (dict(e=ok, w=torch.ones(3, 2)), "compose_weights must be"),
        (dict(e=ok, w=[1.0, float("nan")]), "finite"),
        (dict(e=ok, w=[float("inf"), 1.0]), "finite"),
        (dict(e=ok, w=[1.0, 1.0], n=[[1, 2, 3, 3]] * 2), "one"),
        (dict(e=ok, w=[1.0, 1.0], n=[[1, 2, 3, 4]]), "outside"),
    ]
    for kw, text in bad:
        with pytest.raises(gsdd_amd.GsddError, match=text):
            check_compose(kw["e"], kw["w"], kw.get("n"), cond, 4)
    with pytest.raises(gsdd_amd.GsddError, match="B, Te, cond_dim"):
        check_compose([torch.ones(4, 8)], [1.0, 1.0], None, torch.zeros(4, 8), 4)


def test_sampler_refusals_before_any_launch():
    """sample / sample_fast / sample_long refuse a malformed composed call, and one without an unconditional condition also when
    guidance_scale is 1, on the host (the model sits on the CPU: nothing could have been launched)."""
    import gsdd_amd
    dm = tiny_dm(cond_dim=8)
    cond, cf = torch.zeros(4, 1, 8), torch.zeros(4, 1, 8)
    extra = [torch.ones(4, 1, 8)]
    for call in (lambda **kw: dm.sample(["a"] * 4, None, cond, cf, filter_ratio=0, **kw),
                 lambda **kw: dm.sample_fast(["a"] * 4, None, cond, filter_ratio=0, cf_condition_embed=cf, **kw),
                 lambda **kw: dm.sample_long(["a"] * 4, None, cond, cf, latent_shape=(2, 2, 4), n_frames=4, overlap=1, **kw),
                 lambda **kw: dm.sample_long(["a"] * 4, None, cond, cf, latent_shape=(2, 2, 4), n_frames=2, overlap=1, **kw)):
        with pytest.raises(gsdd_amd.GsddError, match="needs compose_weights"):
            call(compose_embeds=extra)
        with pytest.raises(gsdd_amd.GsddError, match="finite"):
            call(compose_embeds=extra, compose_weights=[1.0, float("nan")])
        with pytest.raises(gsdd_amd.GsddError, match="at most 4"):
            call(compose_embeds=extra * 4, compose_weights=[1.0] * 5)
        with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):          # a well-formed composed call gets as far as the device check
            call(compose_embeds=extra, compose_weights=[1.0, -1.0])
    for scale in (2.0, 1.0):
        dm.guidance_scale = scale
        with pytest.raises(gsdd_amd.GsddError, match="needs the unconditional condition"):
            dm.sample(["a"] * 4, None, cond, None, filter_ratio=0, compose_embeds=extra, compose_weights=[1.0, -1.0])
        with pytest.raises(gsdd_amd.GsddError, match="needs the unconditional condition"):
            dm.sample_fast(["a"] * 4, None, cond, filter_ratio=0, compose_embeds=extra, compose_weights=[1.0, -1.0])
    # learnable_cf: the learned null rows serve, the call gets as far as the device check
    dml = tiny_dm(learnable_cf=True)
    dml.guidance_scale = 1.0
    with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):
        dml.sample(["a"] * 4, None, torch.zeros(4, 1, 512), None, filter_ratio=0, compose_embeds=[torch.ones(4, 1, 512)],
                   compose_weights=[1.0, -1.0])


def test_glue_validates_and_hands_the_conditions_on(monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.sample_compose is None and gen.sample_compose_caption_weight is None
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.zero_text_emb=false",       # (README.md's line)
                                                              "model.generator.sample_compose=[{text: 'blurry, static camera', weight: -1.0}]"]).model.generator
    assert gsdd_amd.d3pm.check_compose_entries(gen.sample_compose) == (("blurry, static camera", -1.0),) and gen.zero_text_emb is False
    dm = tiny_dm()
    # the stand-in provider: a caption's embedding is its length in every channel
    text = lambda texts: torch.tensor([float(len(t)) for t in texts])[:, None].expand(len(texts), 512).contiguous()
    entries = [{"text": "blurry, static camera", "weight": -1.0}, {"text": "sunny", "weight": 0.5}]
    for bad in ("x", [], [{}] * 4, [{"text": "a"}], [{"text": "a", "weight": 1, "more": 2}], [{"text": 3, "weight": 1.0}],
                [{"text": "a", "weight": "1"}], [{"text": "a", "weight": float("nan")}], [{"text": "a", "weight": True}], [("a", 1.0)]):
        with pytest.raises(gsdd_amd.GsddError, match="sample_compose"):
            gsdd_amd.DiscreteDiffusion(text, dm, zero_text_emb=False, sample_compose=bad)
    with pytest.raises(gsdd_amd.GsddError, match="zero_text_emb"):
        gsdd_amd.DiscreteDiffusion(text, dm, sample_compose=entries)                 # (zero_text_emb defaults to true)
    for bad in ("2", float("inf"), True):
        with pytest.raises(gsdd_amd.GsddError, match="sample_compose_caption_weight"):
            gsdd_amd.DiscreteDiffusion(text, dm, zero_text_emb=False, sample_compose=entries, sample_compose_caption_weight=bad)
    assert gsdd_amd.DiscreteDiffusion(text, dm).sample_compose is None

    class Auto:
        device = torch.device("cpu")
        latent_shape = (16,)
        decode = staticmethod(lambda tok: tok)
    seen = []

    def fake_sample(*a, **kw):
        seen.append(kw)
        return {"content_token": torch.zeros(2, 16, dtype=torch.long)}
    monkeypatch.setattr(dm, "sample", fake_sample, raising=False)
    dd = gsdd_amd.DiscreteDiffusion(text, dm, zero_text_emb=False, sample_compose=entries)
    dd.sample_videos(["a", "bb"], Auto())
    kw = seen[-1]
    assert kw["compose_weights"] == [2.0, -1.0, 0.5]                                 # (the caption at guidance_scale = 2)
    assert [tuple(e.shape) for e in kw["compose_embeds"]] == [(2, 1, 512)] * 2 and "compose_lens" not in kw
    assert float(kw["compose_embeds"][0][0, 0, 0]) == len("blurry, static camera") and float(kw["compose_embeds"][1][1, 0, 0]) == 5
    dd = gsdd_amd.DiscreteDiffusion(text, dm, zero_text_emb=False, sample_compose=entries, sample_compose_caption_weight=1.5)
    dd.sample_videos(["a", "bb"], Auto(), compose=[{"text": "night", "weight": 0.25}])      # the call's own list wins
    assert seen[-1]["compose_weights"] == [1.5, 0.25] and len(seen[-1]["compose_embeds"]) == 1
    gsdd_amd.DiscreteDiffusion(text, dm, zero_text_emb=False).sample_videos(["a", "bb"], Auto())
    assert not any(k.startswith("compose") for k in seen[-1])                        # no list: the call as it was
    with pytest.raises(gsdd_amd.GsddError, match="zero_text_emb"):
        gsdd_amd.DiscreteDiffusion(text, dm).sample_videos(["a", "bb"], Auto(), compose=entries)


def test_ops_and_descriptor_refusals():
    """ops.d3pm_compose's own checks, then the C ABI's through the raw descriptor: each refusal returns GSDD_E_ARG with a message before
    anything is launched, so made-up addresses will do."""
    import gsdd_amd
    from gsdd_amd._lib import ComposeDesc
    lib = gsdd_amd.lib()
    assert "gsdd_d3pm_compose" in gsdd_amd.EXPORTS and lib.gsdd_version() >= 118
    assert lib.gsdd_abi_sizeof(10) == ctypes.sizeof(ComposeDesc) == 40 and lib.gsdd_abi_sizeof(9) == -1 and lib.gsdd_abi_sizeof(6) == -1
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    assert "gsdd_compose_desc" in header and "#define GSDD_COMPOSE_MAX_COND 4" in header and gsdd_amd._lib.COMPOSE_MAX_COND == 4
    logits, w = torch.zeros(3 * 6, 8), torch.zeros(2, 2)
    for kw, text in ((dict(n_cond=0), "n_cond"), (dict(n_cond=5), "n_cond"), (dict(n_cond=True), "n_cond"),
                     (dict(logits=logits.double()), "logits must be"), (dict(logits=logits[:-1]), "logits must be"),
                     (dict(logits=torch.zeros(8, 18).t()), "logits must be"),
                     (dict(weights=w.double()), "weights must be"), (dict(weights=torch.zeros(2, 3)), "weights must be"),
                     (dict(weights=torch.zeros(2, 2, device="meta")), "live on"),
                     (dict(out=torch.zeros(6, 4)), "out must be"), (dict(out=torch.zeros(6, 8, dtype=torch.float64)), "out must be")):
        a = dict(dict(logits=logits, weights=w, n_cond=2, out=None), **kw)
        with pytest.raises(gsdd_amd.GsddError, match=text):
            gsdd_amd.ops.d3pm_compose(a["logits"], a["weights"], n_cond=a["n_cond"], B=2, L=3, K=8, out=a["out"])
    for sizes in (dict(B=2.0), dict(L=True), dict(K=0), dict(B=-2)):
        with pytest.raises(gsdd_amd.GsddError, match="positive ints"):
            gsdd_amd.ops.d3pm_compose(logits, w, n_cond=2, **dict(dict(B=2, L=3, K=8), **sizes))
    with pytest.raises(gsdd_amd.GsddError, match="must be a tensor"):
        gsdd_amd.ops.d3pm_compose([0.0] * 144, w, n_cond=2, B=2, L=3, K=8)
    with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):                      # well-formed on the CPU: no CPU fallback
        gsdd_amd.ops.d3pm_compose(logits, w, n_cond=2, B=2, L=3, K=8)

    base, blk = 0x100000, 2 * 3 * 8 * 4

    def rc(**kw):
        d = ComposeDesc()
        d.logits, d.weights, d.out, d.n_cond, d.B, d.L, d.K = base, 0x800000, base, 2, 2, 3, 8
        for k, v in kw.items():
            setattr(d, k, v)
        code = lib.gsdd_d3pm_compose(ctypes.byref(d), None)
        return code, lib.gsdd_last_error().decode()
    assert lib.gsdd_d3pm_compose(None, None) == -1
    for kw, text in ((dict(logits=None), "null pointer"), (dict(weights=None), "null pointer"), (dict(out=None), "null pointer"),
                     (dict(n_cond=0), "n_cond"), (dict(n_cond=5), "n_cond"), (dict(B=0), "bad sizes"), (dict(L=-1), "bad sizes"),
                     (dict(K=0), "multiple of 4"), (dict(K=6), "multiple of 4"), (dict(K=8196), "multiple of 4"),
                     (dict(logits=base + 4), "aligned"), (dict(out=0x900004), "aligned"),
                     (dict(out=base + blk), "overlap"), (dict(out=base + 2 * blk), "overlap"), (dict(out=base + 16), "overlap"),
                     (dict(out=base - 16), "overlap"), (dict(out=base + 3 * blk - 16), "overlap")):
        code, msg = rc(**kw)
        assert code == -1 and text in msg and msg.startswith("gsdd_d3pm_compose"), (kw, code, msg)
