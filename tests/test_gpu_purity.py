"""Purity-prior sampling (DiffusionTransformer.sample with prior_rule 1 / 2; diffusion_transformer.py:304-346, :621-626) on the MI355X.

The pin is tests/golden/purity_L64.npz: the reference's own sample() on the d3pm_L64 model with torch.rand_like / torch.multinomial
replaced by Philox draws (tests/golden/make_golden_purity.py), for rule 1, rule 2 and rule 2 with prior_weight 1.  Every decision of
those chains is at least 1e-3 away from a tie (asserted by the generator, re-checked here), 50 times the 2e-5 allowed between device
and reference log-probabilities, so tokens and selected sets are compared exactly."""
import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_parity import build_d3pm

pytestmark = pytest.mark.gpu

RUNS = {"r1w0": (1, 0.0), "r2w0": (2, 0.0), "r2w1": (2, 1.0)}


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def dev(x):
    return torch.as_tensor(x).cuda()


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def rows(x):
    """(B, K, L) logits -> the denoiser's [B*L][K] rows on the device"""
    x = x.numpy() if isinstance(x, torch.Tensor) else x
    B, K, L = x.shape
    return dev(np.ascontiguousarray(x.transpose(0, 2, 1))).view(B * L, K)


def keys_numpy(w, u):
    with np.errstate(divide="ignore"):
        return (np.log(w.astype(np.float32)) - np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30))).astype(np.float32)


def select_numpy(key, masked, n):
    """The n largest keys among the masked positions, ties to the lower index (stable sort)."""
    key = np.where(masked, key, -np.inf)
    return np.argsort(-key, kind="stable")[:min(n, int(masked.sum()))]


def purity_buffers(B, L, K, dbg=False):
    f = dict(dtype=torch.float32, device="cuda")
    out = {"score": torch.empty((B, L), **f), "smax": torch.empty((B,), **f), "cand": torch.empty((B, L), dtype=torch.int64, device="cuda")}
    if dbg:
        out.update(recon_dbg=torch.empty((B, K + 1, L), **f), prob_dbg=torch.empty((B, K + 1, L), **f), score_dbg=torch.empty((B, L), **f))
    return out


# ----------------------------------------------------------------------------- the purity step kernel
@pytest.mark.parametrize("run", list(RUNS))
def test_purity_kernel_on_the_fixture_logits(G, golden, run):
    """The first call of each fixture chain: log_x_recon, prob and the normalised scores within 2e-5 of the reference's; the candidate
    tokens and the revealed set exact."""
    from oracle import d3pm as od
    _, a, cfg = golden("purity_L64")
    rule, weight = RUNS[run]
    B, K, L = a["first_logits"].shape
    seed, stream = cfg["noise_seed"], 0
    buf = purity_buffers(B, L, K, dbg=True)
    sid = i64([stream])
    G.ops.d3pm_purity_step(rows(a["first_logits"]), rows(a["first_logits_uncond"]), buf["score"], buf["smax"], buf["cand"], sid, K=K,
                           guidance=2.0, prior_rule=rule, prior_weight=weight, seed=seed, recon_dbg=buf["recon_dbg"],
                           prob_dbg=buf["prob_dbg"], score_dbg=buf["score_dbg"])
    err = {k: float(np.abs(buf[k + "_dbg"].cpu().numpy() - a[f"{run}_{k}"]).max()) for k in ("recon", "prob", "score")}
    print(run, "max abs errors", err)
    want_cand = od.gumbel_argmax(torch.from_numpy(a[f"{run}_prob"]), seed, stream)
    # the instantiation without hooks must give the hooked one's tokens and scores
    plain = purity_buffers(B, L, K)
    G.ops.d3pm_purity_step(rows(a["first_logits"]), rows(a["first_logits_uncond"]), plain["score"], plain["smax"], plain["cand"], sid, K=K,
                           guidance=2.0, prior_rule=rule, prior_weight=weight, seed=seed)
    n = int(a["calls"][0][1])
    tok = torch.full((B, L), K, dtype=torch.int64, device="cuda")
    out = torch.empty_like(tok)
    G.ops.d3pm_purity_select(tok, out, plain["cand"], plain["score"], plain["smax"], i64([n]), sid, K=K, prior_rule=rule, seed=seed,
                             stream_add=1)
    parity_report(f"purity_kernel_{run}", {**err, "cand_mismatches": int((buf["cand"].cpu() != want_cand).sum()),
                                           "min_key_gap": float(a[f"{run}_key_gap"].min()), "min_cand_gap": float(a[f"{run}_cand_gap"].min())})
    assert a[f"{run}_key_gap"].min() >= 1e-3 and a[f"{run}_cand_gap"].min() >= 1e-3           # the fixture's floor
    assert max(err.values()) <= 2e-5, err
    assert torch.equal(buf["cand"].cpu(), want_cand)
    assert torch.equal(plain["cand"], buf["cand"]) and torch.equal(plain["score"], buf["score"])
    assert np.array_equal(out.cpu().numpy(), a[f"{run}_trace"][0].astype(np.int64))
    assert int((out != K).sum()) == n * B


def restate(lc, lu, rule, weight, seed, stream):
    """prob, the normalised score and the candidate tokens from oracle pieces (diffusion_transformer.py:313-326)."""
    from oracle import d3pm as od
    rec = od.cf_mix(od.predict_start_from_logits(lc)[:, :-1], od.predict_start_from_logits(lu)[:, :-1], 2.0) if lu is not None \
        else od.predict_start_from_logits(lc)
    if rule == 1:
        score = torch.ones(rec.shape[0], rec.shape[2])
    else:
        score = torch.exp(rec).max(dim=1).values.clamp(0, 1)
        score = score / (score.max(dim=1, keepdim=True).values + 1e-10)
    if rule != 1 and weight > 0:
        prob = ((1 + score * weight).unsqueeze(1) * rec).softmax(dim=1).log().clamp(-70, 0)
    else:
        prob = rec
    return prob, score, od.gumbel_argmax(prob, seed, stream)


@pytest.mark.parametrize("rule,weight", [(1, 0.0), (2, 0.0), (2, 1.0)])
def test_purity_kernel_production_instantiation(G, rule, weight):
    """K = 4096 without debug buffers (d3pm_purity_kernel<16, true, *, false, 2>), guided, masked and unmasked inputs: candidate
    tokens and the revealed positions exact against the restatement."""
    from oracle import philox
    K, B, L, seed, stream = 4096, 5, 8, 4321, 7
    g = torch.Generator().manual_seed(K + rule)
    lc = torch.randn(B, K, L, generator=g) * 3.0
    lu = lc + torch.randn(B, K, L, generator=g)
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    xt[1] = K                                                                            # one sample all [MASK]
    _, score, want_cand = restate(lc, lu, rule, weight, seed, stream)
    buf = purity_buffers(B, L, K)
    sid = i64([stream])
    G.ops.d3pm_purity_step(rows(lc), rows(lu), buf["score"], buf["smax"], buf["cand"], sid, K=K, guidance=2.0, prior_rule=rule,
                           prior_weight=weight, seed=seed)
    mism = int((buf["cand"].cpu() != want_cand).sum())
    n = 2
    out = torch.empty_like(xt).cuda()
    G.ops.d3pm_purity_select(dev(xt), out, buf["cand"], buf["score"], buf["smax"], i64([n]), sid, K=K, prior_rule=rule, seed=seed, stream_add=1)
    u = philox.uniform_rows(seed, stream + 1, B, L)
    want = xt.clone()
    for b in range(B):
        sel = select_numpy(keys_numpy(score[b].numpy(), u[b]), (xt[b] == K).numpy(), n)
        want[b, sel] = want_cand[b, sel]
    parity_report(f"purity_k4096_rule{rule}_w{weight:g}", {"cand_mismatches": mism, "positions": B * L,
                                                           "token_mismatches": int((out.cpu() != want).sum())})
    assert mism == 0
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out.cpu()[xt != K], xt[xt != K])


# ----------------------------------------------------------------------------- the selection kernel alone
@pytest.mark.parametrize("L", [4096, 1000])
def test_selection_kernel(G, L):
    """Against a stable numpy sort of the kernel's own keys (which are the fp32 formula's to a few ulp): exactly n [MASK] positions per
    sample change, to their candidates; every other token is bit-identical; n = 0 changes nothing."""
    from oracle import philox
    K, B, seed, stream = 4096, 3, 97, 12
    g = torch.Generator().manual_seed(L)
    tok = torch.randint(0, K, (B, L), generator=g)
    tok[torch.rand(B, L, generator=g) < 0.6] = K
    tok[2, : L // 2] = K
    cand = torch.randint(0, K, (B, L), generator=g)
    score = (torch.rand(B, L, generator=g) * 0.99 + 0.01).float()
    smax = score.max(dim=1).values
    u = philox.uniform_rows(seed, stream + 1, B, L, row0=5)
    masked = (tok == K).numpy()
    d_tok, d_cand, d_score, d_smax, sid = dev(tok), dev(cand), dev(score), dev(smax), i64([stream])
    for rule in (2, 1):
        w = (score / (smax[:, None] + 1e-10)).numpy() if rule == 2 else np.ones((B, L), dtype=np.float32)
        want_keys = keys_numpy(w, u)
        for n in (0, 1, 11, 1024, int(masked.sum(1).min())):
            n = min(n, int(masked.sum(1).min()))
            out = torch.full_like(d_tok, -1)
            keys = torch.empty((B, L), dtype=torch.float32, device="cuda")
            G.ops.d3pm_purity_select(d_tok, out, d_cand, d_score, d_smax, i64([n]), sid, K=K, prior_rule=rule, seed=seed, stream_add=1,
                                     row0=5 * L, key_dbg=keys)
            keys, out = keys.cpu().numpy(), out.cpu()
            # a few ulp of fp32 at |key| <= ~20 (log of a weight >= 0.01 plus a Gumbel value)
            assert np.allclose(keys, want_keys, rtol=2e-6, atol=1e-5), float(np.abs(keys - want_keys).max())
            want = tok.clone()
            for b in range(B):
                sel = select_numpy(keys[b], masked[b], n)
                assert len(sel) == n
                want[b, sel] = cand[b, sel]
            changed = out != tok
            assert torch.equal(out, want), (L, rule, n, int((out != want).sum()))
            assert changed.sum(1).tolist() == [n] * B and bool((tok[changed] == K).all())
            assert torch.equal(out[~changed], tok[~changed])
    # in place (tok_out = tok_in) gives the same tokens
    inplace = d_tok.clone()
    G.ops.d3pm_purity_select(inplace, inplace, d_cand, d_score, d_smax, i64([11]), sid, K=K, prior_rule=1, seed=seed, stream_add=1, row0=5 * L)
    out = torch.empty_like(d_tok)
    G.ops.d3pm_purity_select(d_tok, out, d_cand, d_score, d_smax, i64([11]), sid, K=K, prior_rule=1, seed=seed, stream_add=1, row0=5 * L)
    assert torch.equal(inplace, out)


def test_selection_kernel_rejects_long_sequences(G):
    B, L, K = 1, 4097, 32
    tok = torch.full((B, L), K, dtype=torch.int64, device="cuda")
    z = torch.ones((B, L), device="cuda")
    with pytest.raises(G.GsddError, match="4096"):
        G.ops.d3pm_purity_select(tok, tok.clone(), tok, z, z[:, 0].contiguous(), i64([1]), i64([0]), K=K, prior_rule=2, seed=1)


def test_advance_plan(G):
    plan_t, plan_n = i64([90, 90, 40, 0]), i64([4, 3, 9, 0])
    step, t, n, sid = i64([0]), i64([90] * 6), i64([4]), i64([10])
    seen = []
    for _ in range(5):
        G.ops.advance_plan(step, plan_t, plan_n, t, n, sid, 2)
        seen.append((int(step), t.tolist(), int(n), int(sid)))
    assert seen == [(1, [90] * 6, 3, 12), (2, [40] * 6, 9, 14), (3, [0] * 6, 0, 16), (4, [0] * 6, 0, 18), (5, [0] * 6, 0, 20)]


# ----------------------------------------------------------------------------- the whole chain
def purity_dm(G, golden, run=None):
    sd, a, cfg = golden("d3pm_L64")
    _, p, pcfg = golden("purity_L64")
    dm = build_d3pm(G, sd, cfg)
    if run is not None:
        dm.prior_rule, dm.prior_weight = RUNS[run]
        dm.prior_ps, dm.n_sample = pcfg["prior_ps"], p["n_sample"].tolist()
    return dm, a, cfg, p, pcfg


@pytest.mark.parametrize("run", list(RUNS))
def test_purity_chain_matches_the_reference(G, golden, run):
    dm, a, cfg, p, pcfg = purity_dm(G, golden, run)
    B = cfg["B"]
    cond = dev(a["step_cond"])
    want_trace, want = p[f"{run}_trace"].astype(np.int64), p[f"{run}_tokens"].astype(np.int64)
    n_calls = len(p["calls"])
    dm.set_noise(pcfg["noise_seed"])
    trace = []
    got = dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0, trace=trace)["content_token"].cpu().numpy()
    assert len(trace) == n_calls == 42
    bad = [i for i in range(n_calls) if not np.array_equal(trace[i].cpu().numpy(), want_trace[i])]
    assert not bad, f"{run}: token trace diverges at call {bad[0]} {p['calls'][bad[0]].tolist()} of {n_calls}"
    assert np.array_equal(got, want) and int((got == cfg["K"]).sum()) == 0
    assert dm.noise_stream == 2 * (n_calls - 1) + 1 == dm._last_draws
    dm.set_noise(pcfg["noise_seed"], stream=0)
    got_g = dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0, use_graph=True)["content_token"].cpu().numpy()
    assert np.array_equal(got_g, want), f"{run} captured: {(got_g != want).sum()} tokens differ"
    assert dm.noise_stream == 2 * (n_calls - 1) + 1 and len(dm._last_plan.calls) == n_calls - 1 and dm._last_plan.final
    parity_report(f"purity_chain_{run}", {"calls": n_calls, "mismatches": 0, "streams": dm.noise_stream})


def test_purity_lanes_and_shards(G, golden):
    """B = 8 in two lanes equals one lane; a shard keyed at its global rows equals the matching rows of the full batch."""
    sd, a, cfg = golden("d3pm_L64")
    B = 8
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    toks = {}
    for lanes in (1, 2):
        dm, _, _, p, pcfg = purity_dm(G, golden, "r2w1")
        dm.set_noise(77, stream=2)
        toks[lanes] = dm.sample(["x"] * B, None, cond, cf, filter_ratio=0, lanes=lanes)["content_token"].cpu()
        assert dm._last_lanes == lanes and dm.noise_stream == 2 + 83
    assert torch.equal(toks[1], toks[2]) and int((toks[1] == cfg["K"]).sum()) == 0
    dm.set_noise(77, stream=2, row_offset=4)
    shard = dm.sample(["x"] * 4, None, cond[4:], cf[4:], filter_ratio=0)["content_token"].cpu()
    assert torch.equal(shard, toks[1][4:])


def test_prior_rule_zero_after_a_purity_run_is_plain_sampling(G, golden):
    dm, a, cfg, p, pcfg = purity_dm(G, golden, "r2w0")
    B, T = cfg["B"], cfg["T"]
    cond = dev(a["step_cond"])
    dm.set_noise(pcfg["noise_seed"])
    dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0)
    dm.prior_rule = 0                                           # n_sample / prior_ps stay as the purity run left them
    dm.set_noise(cfg["noise_seed"])
    tok = dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0)["content_token"].cpu().numpy()
    assert np.array_equal(tok, a["loop_tokens"]) and dm.noise_stream == T
    plain = build_d3pm(G, golden("d3pm_L64")[0], cfg)
    plain.set_noise(31, stream=9)
    dm.set_noise(31, stream=9)
    want = plain.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0)["content_token"]
    assert torch.equal(dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0)["content_token"], want)
    assert dm.noise_stream == plain.noise_stream == 9 + T


# ----------------------------------------------------------------------------- the eval entry point
def test_eval_entry_point_prior_rule(G, tmp_path, monkeypatch):
    """`python src/eval.py model.generator.sample_prior_rule=2 model.generator.sample_prior_scale_schedule=true` at the toy sizes of
    test_gpu_entrypoints, with diffusion_step = 10 (the smallest T the reference has a reveal list for; rescaled from 1024 to the toy
    model's 64 tokens it reveals 60 over t >= 1, the step at t = 0 decides the rest): the sampler runs the purity plan and leaves no
    [MASK] token."""
    from tests.test_gpu_entrypoints import STAGE2, finite
    from gsdd_amd.d3pm import DiffusionTransformer, PurityPlan, purity_plan, reference_n_sample, scaled_n_sample
    from src.eval import main
    seen = []
    orig = DiffusionTransformer._sample_once

    def spy(self, plan, *args, **kw):
        out = orig(self, plan, *args, **kw)
        seen.append((plan, out["content_token"].cpu()))
        return out
    monkeypatch.setattr(DiffusionTransformer, "_sample_once", spy)
    extra = ["model.do_evaluation=true", "model.evaluator.videoencoder._target_=src.utils.evaluator.MeanPoolEncoder",
             "model.generator.diffusion_model.diffusion_step=10", "model.generator.sample_prior_rule=2",
             "model.generator.sample_prior_weight=1", "model.generator.sample_prior_scale_schedule=true"]
    metrics = main(STAGE2 + extra + [f"paths.output_dir={tmp_path}"])
    finite(metrics, ["total/test", "l/dummy/test", "Metrics/fvd-test"])
    ns = scaled_n_sample(reference_n_sample(10), 64)
    calls = purity_plan(ns, 1024, 10)
    assert sum(ns[1:]) == 60 and len(calls) == 10
    assert seen
    for plan, tok in seen:
        assert isinstance(plan, PurityPlan) and plan.rule == 2 and plan.weight == 1.0 and plan.final
        assert list(plan.calls) == calls[:-1]
        assert int((tok == 32).sum()) == 0 and int(tok.min()) >= 0
