"""DiffusionTransformer.sample_fast (diffusion_transformer.py:648-713, VQ-Diffusion's skip-step sampler) on the MI355X.

The reference's own sample_fast cannot run: it calls cf_predict_start with three of its four arguments. As for
sample(filter_ratio > 0), the pin is a restatement of what the method is written to do, built from oracle pieces that are themselves
pinned to the reference (cf_predict_start, q_posterior, Gumbel arg-max): the denoiser at t = T-1, T-1-(1+s), ..., 0, the posterior at
t - s for t > s (else at t), from the all-[MASK] start with its true -inf rows; step i draws Philox stream noise_stream + i."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_parity import build_d3pm

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def dev(x):
    return torch.as_tensor(x).cuda()


def oracle_sample_fast(B, L, cond, cf_cond, sd, scale, seed, skip_step, stream0=0, row0=0):
    """-> (tokens, per-step token trace).  diffusion_transformer.py:686-713 with the unconditional embedding handed to
    cf_predict_start."""
    from oracle import d3pm as od
    T = sd["log_at"].shape[0]
    K1 = sd["transformer.content_emb.emb.weight"].shape[0]
    diffusion_list = [index for index in range(T - 1, -1, -1 - skip_step)]
    if diffusion_list[-1] != 0:
        diffusion_list.append(0)
    log_z = torch.full((B, K1, L), float("-inf"))
    log_z[:, -1] = 0
    trace = []
    with torch.no_grad():
        for i, index in enumerate(diffusion_list):
            t = torch.full((B,), index, dtype=torch.long)
            rec = od.cf_predict_start(log_z, cond, cf_cond, t, sd, scale)
            post = od.q_posterior(rec, log_z, t - skip_step if index > skip_step else t, sd)
            tok = od.gumbel_argmax(post, seed, stream0 + i, row0=row0)
            log_z = od.index_to_log_onehot(tok, K1)
            trace.append(tok)
    return tok, trace


_ORACLE = {}


def oracle_cached(golden, s):
    if s not in _ORACLE:
        sd, a, cfg = golden("d3pm_L64")
        cond = torch.from_numpy(a["step_cond"])
        _ORACLE[s] = oracle_sample_fast(cfg["B"], cfg["L"], cond, torch.zeros_like(cond), sd, cfg["guidance"], cfg["noise_seed"], s,
                                        stream0=5)
    return _ORACLE[s]


# ----------------------------------------------------------------------------- the step kernel alone
@pytest.mark.parametrize("post_skip", [1, 3])
def test_step_kernel_post_skip_matches_oracle(G, golden, post_skip):
    """The reference fixture's logits through the hooked instantiation: posterior values at t' within 2e-5, tokens bit-exact."""
    from oracle import d3pm as od
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    B, L, K = cfg["B"], cfg["L"], cfg["K"]
    lc = dev(np.ascontiguousarray(a["step_logits"].transpose(0, 2, 1))).view(B * L, K)
    lu = dev(np.ascontiguousarray(a["step_logits_uncond"].transpose(0, 2, 1))).view(B * L, K)
    xt = dev(a["step_xt"])
    stream = int(a["step_stream"])
    sid = torch.tensor([stream], dtype=torch.int64, device="cuda")
    # the fixture's own timesteps plus the boundary t = post_skip (posterior at t) and t = post_skip + 1 (posterior at 1)
    for t_host in (torch.from_numpy(a["step_t"]).long(), torch.tensor([post_skip, post_skip + 1] * (B // 2) + [0] * (B % 2))):
        tp = torch.where(t_host > post_skip, t_host - post_skip, t_host)
        out = torch.empty_like(xt)
        post = torch.empty((B, K + 1, L), device="cuda")
        G.ops.d3pm_step(lc, lu, xt, out, dm._sched(), dev(t_host), sid, K=K, T=cfg["T"], guidance=2.0, seed=cfg["noise_seed"],
                        post_dbg=post, post_skip=post_skip)
        log_xt = od.index_to_log_onehot(torch.from_numpy(a["step_xt"]), K + 1)
        rec = od.cf_mix(od.predict_start_from_logits(torch.from_numpy(a["step_logits"]))[:, :-1],
                        od.predict_start_from_logits(torch.from_numpy(a["step_logits_uncond"]))[:, :-1], 2.0)
        want_post = od.q_posterior(rec, log_xt, tp, sd)
        torch.testing.assert_close(post.cpu(), want_post, atol=2e-5, rtol=0)
        assert torch.equal(out.cpu(), od.gumbel_argmax(want_post, cfg["noise_seed"], stream)), t_host
        # p_sample_tokens' hook runs the same kernel through the denoiser
        got = dm.p_sample_tokens(xt, dev(a["step_cond"]), torch.zeros_like(dev(a["step_cond"])), dev(t_host), stream, post_skip=post_skip)
        assert got.shape == xt.shape and int(got.max()) <= K


@pytest.mark.parametrize("post_skip", [1, 3])
def test_step_kernel_post_skip_production_instantiation(G, post_skip):
    """K = 4096 without debug buffers: the instantiation the sampler runs at the bench shape (d3pm_step_kernel<16, true, false, 2>).
    Tokens bit-exact against the oracle's posterior at t', guided, masked and unmasked x_t, t = 0 and both sides of t = post_skip."""
    from oracle import d3pm as od
    from gsdd_amd.d3pm import SCHED_ORDER
    K, B, L, T, seed, stream = 4096, 5, 8, 100, 4321, 7
    g = torch.Generator().manual_seed(K + post_skip)
    lc = torch.randn(B, K, L, generator=g) * 3.0
    lu = lc + torch.randn(B, K, L, generator=g)
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    t = torch.tensor([57, 0, 99, post_skip, post_skip + 1])
    tp = torch.where(t > post_skip, t - post_skip, t)
    sd = od.schedule_buffers(T, K)
    sched = [dev(sd[n]) for n in SCHED_ORDER]
    rows = lambda x: dev(np.ascontiguousarray(x.numpy().transpose(0, 2, 1))).view(B * L, K)
    rec = od.cf_mix(od.predict_start_from_logits(lc)[:, :-1], od.predict_start_from_logits(lu)[:, :-1], 2.0)
    want_tok = od.gumbel_argmax(od.q_posterior(rec, od.index_to_log_onehot(xt, K + 1), tp, sd), seed, stream)
    plain = torch.empty_like(xt).cuda()
    G.ops.d3pm_step(rows(lc), rows(lu), dev(xt), plain, sched, dev(t), torch.tensor([stream], dtype=torch.int64, device="cuda"),
                    K=K, T=T, guidance=2.0, seed=seed, post_skip=post_skip)
    mism = int((plain.cpu() != want_tok).sum())
    parity_report(f"sample_fast_step_k4096_s{post_skip}", {"mismatches": mism, "positions": B * L})
    assert mism == 0


# ----------------------------------------------------------------------------- the whole chain
@pytest.mark.parametrize("s", [1, 3, 7, 98, 99, 250])
def test_sample_fast_chain_matches_restatement(G, golden, s):
    from gsdd_amd.d3pm import sample_plan
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    B, T = cfg["B"], cfg["T"]
    want, want_trace = oracle_cached(golden, s)
    n = sample_plan(T, skip_step=s).n_steps
    assert len(want_trace) == n
    cond = dev(a["step_cond"])
    dm.set_noise(cfg["noise_seed"], stream=5)
    trace = []
    got = dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=s, cf_condition_embed=torch.zeros_like(cond),
                         trace=trace)["content_token"].cpu()
    assert len(trace) == n
    bad = [i for i, (x, y) in enumerate(zip(trace, want_trace)) if not torch.equal(x.cpu(), y)]
    assert not bad, f"s={s}: token trace diverges at step {bad[0]} of {n}"
    assert torch.equal(got, want) and dm.noise_stream == 5 + n
    dm.set_noise(cfg["noise_seed"], stream=5)
    got_g = dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=s, cf_condition_embed=torch.zeros_like(cond),
                           use_graph=True)["content_token"].cpu()
    assert torch.equal(got_g, want), f"s={s} captured: {(got_g != want).sum().item()} tokens differ"
    assert dm.noise_stream == 5 + n and dm._last_plan.n_steps == n
    parity_report(f"sample_fast_chain_s{s}", {"steps": n, "mismatches": 0, "max_token": int(got.max())})


def test_skip_step_zero_is_sample(G, golden):
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    B, T = cfg["B"], cfg["T"]
    cond = dev(a["step_cond"])
    dm.set_noise(cfg["noise_seed"], stream=3)
    ref = dm.sample(["a"] * B, None, cond, torch.zeros_like(cond), filter_ratio=0)["content_token"].cpu()
    assert dm.noise_stream == 3 + T
    dm.set_noise(cfg["noise_seed"], stream=3)
    fast = dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=0, cf_condition_embed=torch.zeros_like(cond))["content_token"].cpu()
    assert torch.equal(fast, ref) and dm.noise_stream == 3 + T
    dm.set_noise(cfg["noise_seed"])
    fast = dm.sample_fast(["a"] * B, None, cond, None, 0, skip_step=0, cf_condition_embed=torch.zeros_like(cond))["content_token"].cpu()
    assert np.array_equal(fast.numpy(), a["loop_tokens"]) and dm.noise_stream == T


# ----------------------------------------------------------------------------- what sample() has, sample_fast has
def test_sample_fast_two_lanes_equal_one(G, golden):
    sd, a, cfg = golden("d3pm_L64")
    B = 8
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    toks = {}
    for lanes in (1, 2):
        dm = build_d3pm(G, sd, cfg)
        dm.set_noise(77, stream=2)
        toks[lanes] = dm.sample_fast(["x"] * B, None, cond, filter_ratio=0, skip_step=3, cf_condition_embed=cf,
                                     lanes=lanes)["content_token"].cpu()
        assert dm._last_lanes == lanes and dm.noise_stream == 2 + 26
    assert torch.equal(toks[1], toks[2])


def test_sample_fast_identical_embeddings_dedupe(G, golden, monkeypatch):
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    B = cfg["B"]
    zero = torch.zeros_like(dev(a["step_cond"]))
    toks = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GSDD_CFG_DEDUPE", mode)
        dm.set_noise(cfg["noise_seed"])
        toks[mode] = dm.sample_fast(["a"] * B, None, zero, filter_ratio=0, skip_step=3, cf_condition_embed=zero.clone())["content_token"].cpu()
        assert dm._last_cfg_dedupe == (mode == "1")
    assert torch.equal(toks["1"], toks["0"])
    want, _ = oracle_sample_fast(B, cfg["L"], zero.cpu(), zero.cpu(), sd, cfg["guidance"], cfg["noise_seed"], 3)
    assert torch.equal(toks["1"], want)


def test_sample_fast_range_demotion(G, golden, monkeypatch):
    """An mlp bias of 6000 trips the f16 layer kernel's range screen: the call is repeated on the bf16x3 kernel with the noise stream
    rewound, so the tokens are those of an x3p-only run and the stream advances once."""
    sd, a, cfg = golden("d3pm_L64")
    sd = {k_: v_.clone() for k_, v_ in sd.items()}
    sd["transformer.blocks.1.mlp.0.bias"][7] = 6000.0
    B = cfg["B"]
    cond = dev(a["step_cond"])
    dm = build_d3pm(G, sd, cfg)
    dm.set_noise(cfg["noise_seed"])
    tok = dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=3, cf_condition_embed=torch.zeros_like(cond))["content_token"].cpu()
    assert dm.transformer.range_demotions == 1 and dm.noise_stream == 26
    monkeypatch.setenv("GSDD_LAYER", "x3p")
    dm3 = build_d3pm(G, sd, cfg)
    dm3.set_noise(cfg["noise_seed"])
    tok3 = dm3.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=3, cf_condition_embed=torch.zeros_like(cond))["content_token"].cpu()
    assert getattr(dm3.transformer, "range_demotions", 0) == 0
    assert torch.equal(tok, tok3) and int(tok.max()) < cfg["K"]


def test_sample_fast_row_offset_shard(G, golden):
    """A shard keyed at its global rows (row_offset) draws the noise of those rows: its tokens are the full batch's rows."""
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    B = 4
    g = torch.Generator().manual_seed(9)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.zeros_like(cond)
    dm.set_noise(11, stream=4)
    full = dm.sample_fast(["x"] * B, None, cond, filter_ratio=0, skip_step=7, cf_condition_embed=cf)["content_token"].cpu()
    dm.set_noise(11, stream=4, row_offset=2)
    shard = dm.sample_fast(["x"] * 2, None, cond[2:], filter_ratio=0, skip_step=7, cf_condition_embed=cf[2:])["content_token"].cpu()
    assert torch.equal(shard, full[2:])


# ----------------------------------------------------------------------------- bench shape and the eval entry point
def test_sample_fast_bench_shape(G):
    sys.path.insert(0, REPO)
    import bench
    args = argparse.Namespace(grid=[16, 16, 16], codes=4096, layers=19, diffusion_steps=100)
    dm, vq, L = bench.build_models(args, torch.device("cuda"))
    B = 16
    g = torch.Generator().manual_seed(100)
    cond = torch.randn(B, 1, 512, generator=g).cuda()
    dm.set_noise(1234, 0)
    tok = dm.sample_fast(["synthetic"] * B, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=torch.zeros_like(cond))["content_token"]
    assert dm._last_lanes == 2 and dm.noise_stream == 51 and dm._last_plan.n_steps == 51
    assert tuple(tok.shape) == (B, L) and int(tok.min()) >= 0 and int(tok.max()) < 4096


@pytest.mark.parametrize("skip,steps", [(None, 20), (9, 3)])
def test_eval_entry_point_skip_step(G, tmp_path, monkeypatch, skip, steps):
    """`python src/eval.py model.generator.sample_skip_step=9` at the toy sizes of test_gpu_entrypoints (T = 20): the sampler runs the
    plan's 3 steps [19, 9, 0]; the default null runs all 20."""
    from tests.test_gpu_entrypoints import STAGE2, finite
    from gsdd_amd.d3pm import DiffusionTransformer
    from src.eval import main
    seen = []
    orig = DiffusionTransformer._sample_once

    def spy(self, plan, *args, **kw):
        seen.append(plan)
        return orig(self, plan, *args, **kw)
    monkeypatch.setattr(DiffusionTransformer, "_sample_once", spy)
    # (eval samples only with do_evaluation; the I3D features have no weights offline: the stand-in pooling encoder takes the clips)
    extra = ["model.do_evaluation=true", "model.evaluator.videoencoder._target_=src.utils.evaluator.MeanPoolEncoder"]
    extra += [] if skip is None else [f"model.generator.sample_skip_step={skip}"]
    metrics = main(STAGE2 + extra + [f"paths.output_dir={tmp_path}"])
    finite(metrics, ["total/test", "l/dummy/test", "Metrics/fvd-test"])
    assert seen and all(p.n_steps == steps and p.post_skip == (skip or 0) for p in seen), seen
