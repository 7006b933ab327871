"""Known-token conditioned sampling (known_mask / known_mode; frame prediction, interpolation, inpainting) on the MI355X.

The pin is tests/golden/known_L64.npz: the reference's own sample() on the d3pm_L64 model with its p_pred / p_sample wrapped by the
rule as tests/golden/make_golden_known.py states it, and torch.rand_like replaced by Philox draws.  A known position's token is a
Gumbel arg-max over three distinct log-probabilities, so the fixture records per step and position the gap between the two best
values of the draw the position used; tokens are compared exactly wherever that gap is at least 1e-3 (50 x the 2e-5 allowed between
device and reference log-probabilities), and the positions left out must stay under 5 %, which every test asserts for its own inputs.
Positions that are not known must equal the launch without a mask bit for bit: they run the same code on the same uniforms."""
import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_parity import build_d3pm
from tests.test_known_host import (FREQ, MODES, WIDTHS, compared, known_only, post_timestep, production_inputs, schedule,
                                   width_inputs)

pytestmark = pytest.mark.gpu

MODE_CODE = {"renoise": 0, "hold": 1}


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


def poisoned(r, known):
    """The rows of the known positions filled with NaN: a kernel that reads them cannot return the expected tokens."""
    r = r.clone()
    r[dev(known).view(-1)] = float("nan")
    return r


def device_sched(T, K):
    from gsdd_amd.d3pm import SCHED_ORDER
    sd = schedule(T, K)
    return sd, [dev(sd[n]) for n in SCHED_ORDER]


def fixture_inputs(golden):
    _, a, kcfg = golden("known_L64")
    known = torch.from_numpy(a["known"])
    return a, kcfg, known, torch.from_numpy(a["x_known"].astype(np.int64))


def step_pair(G, lc, lu, xt, sched, t, stream, known, x_known, mode, *, K, T, seed, guidance, **kw):
    """The masked launch on NaN-poisoned known rows and the plain launch on the clean rows, same stream -> (masked, plain) tokens."""
    got, plain = torch.empty_like(xt), torch.empty_like(xt)
    G.ops.d3pm_step(poisoned(lc, known), None if lu is None else poisoned(lu, known), xt, got, sched, t, i64([stream]), K=K, T=T,
                    guidance=guidance, seed=seed, known=dev(known).to(torch.uint8), x_known=dev(x_known), known_mode=MODE_CODE[mode], **kw)
    G.ops.d3pm_step(lc, lu, xt, plain, sched, t, i64([stream]), K=K, T=T, guidance=guidance, seed=seed, **kw)
    return got.cpu(), plain.cpu()


# ----------------------------------------------------------------------------- 1 / 2. single calls of the fixture's chain
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("call", ["first", "mid"])
def test_fixture_call(G, golden, call, mode):
    sd, _, cfg = golden("d3pm_L64")
    a, kcfg, known, x_known = fixture_inputs(golden)
    dm = build_d3pm(G, sd, cfg)
    B, K, L = a["first_logits"].shape
    T = cfg["T"]
    if call == "first":
        step, xt, lc, lu = 0, torch.full((B, L), K, dtype=torch.int64), a["first_logits"], a["first_logits_uncond"]
    else:
        step, xt = kcfg["mid_step"], torch.from_numpy(a[f"mid_xt_{mode}"].astype(np.int64))
        lc, lu = a[f"mid_logits_{mode}"], a[f"mid_logits_uncond_{mode}"]
        assert int(a["mid_t"]) == T - 1 - step
    got, plain = step_pair(G, rows(lc), rows(lu), dev(xt), dm._sched(), i64([T - 1 - step] * B), step, known, x_known, mode, K=K, T=T,
                           seed=kcfg["noise_seed"], guidance=float(cfg["guidance"]))
    ok, left_out = compared(a[f"gap_{mode}"][step])
    want = a[f"trace_{mode}"][step].astype(np.int64)
    mism = int((got.numpy() != want)[ok].sum())
    rec = {"mismatches": mism, "left_out_share": left_out, "known_positions": int(known.sum()),
           "known_at_mask": int((got[known] == K).sum()), "known_at_token": int((got[known] == x_known[known]).sum())}
    print(rec)
    parity_report(f"known_fixture_{call}_{mode}", rec)
    assert mism == 0
    assert torch.equal(got[~known], plain[~known])                          # bit-equal to the launch without a mask
    if mode == "hold" or call == "mid":                                     # (at t = T - 1 a re-noised position is [MASK] like the rest)
        assert not torch.equal(got[known], plain[known])                    # the mask matters on these inputs
    if mode == "hold":
        assert torch.equal(got[known], x_known[known])


# ----------------------------------------------------------------------------- 3. the fixture's chain, teacher-forced
@pytest.mark.parametrize("mode", MODES)
def test_teacher_forced_chain_reproduces_the_fixture(G, golden, mode):
    """Step i from the fixture's trace[i-1] at stream i must give trace[i], at every position whose decision the reference itself
    made at least the floor away from a flip."""
    from gsdd_amd.d3pm import check_known
    sd, b, cfg = golden("d3pm_L64")
    a, kcfg, known, x_known = fixture_inputs(golden)
    dm = build_d3pm(G, sd, cfg)
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    cond = dev(b["step_cond"])
    cf = torch.zeros_like(cond)
    dm.set_noise(kcfg["noise_seed"])
    kn = check_known(known, x_known, mode, B=B, L=L, K=K)
    kn = (kn[0].cuda(), kn[1].cuda(), kn[2])
    trace = a[f"trace_{mode}"].astype(np.int64)
    ok, left_out = compared(a[f"gap_{mode}"])
    bad = []
    for i in range(T):
        prev = torch.full((B, L), K, dtype=torch.int64, device="cuda") if i == 0 else dev(trace[i - 1])
        got = dm.p_sample_tokens(prev, cond, cf, i64([T - 1 - i] * B), i, known=kn).cpu().numpy()
        n = int((got != trace[i])[ok[i]].sum())
        if n:
            bad.append((i, n))
    rec = {"steps": T, "positions": int(ok.size), "left_out_share": left_out, "mismatches": int(sum(n for _, n in bad))}
    print(rec)
    parity_report(f"known_teacher_forced_{mode}", rec)
    assert not bad, f"(step, mismatching positions): {bad[:10]}"


# ----------------------------------------------------------------------------- 4. the production instantiations
@pytest.mark.parametrize("trunc", [None, 0.86])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("post_skip", [0, 3])
def test_production_instantiation(G, post_skip, mode, trunc):
    """K = 4096 (d3pm_step_known_kernel<16, true> / d3pm_step_known_trunc_kernel<16, true>), guided, 2 x 37 positions: the last
    workgroup is partial and the mask's runs cross workgroups.  The known rows of both logit tensors are NaN."""
    K, T, seed, stream = 4096, 100, 4321, 7
    lc, lu, xt, known, x_known, t = production_inputs()
    sd, sched = device_sched(T, K)
    kw = {} if trunc is None else {"trunc_rate": trunc}
    got, plain = step_pair(G, rows(lc), rows(lu), dev(xt), sched, dev(t), stream, known, x_known, mode, K=K, T=T, seed=seed,
                           guidance=2.0, post_skip=post_skip, **kw)
    want, gap = known_only(x_known, post_timestep(t, post_skip), sd, K, mode, seed, stream)
    ok, left_out = compared(gap.numpy(), known.numpy())
    mism = int((got != want).numpy()[ok].sum())
    rec = {"mismatches": mism, "known_positions": int(known.sum()), "left_out_share": left_out,
           "known_kept": int((got[known] == x_known[known]).sum()), "known_masked": int((got[known] == K).sum())}
    print(rec)
    parity_report(f"known_k4096_s{post_skip}_{mode}_{'trunc' if trunc else 'plain'}", rec)
    assert mism == 0
    assert torch.equal(got[~known], plain[~known])
    assert int(got.min()) >= 0 and int(got.max()) <= K
    if mode == "renoise":                           # t' - 1 = 56 / 53 and 2: sample 0 is partly [MASK], sample 1 (gamma-bar 0.02) keeps its tokens
        assert 0 < int((got[0][known[0]] == K).sum()) < int(known[0].sum())


# ----------------------------------------------------------------------------- 5. every class width
@pytest.mark.parametrize("K", WIDTHS)
def test_every_class_width(G, K):
    """Each J of both families, the partial widths and the [MASK] class on its lane (K / 4) % 64; t = 50 and t = 0, where the level is
    index T and the known output is x_known itself.  Plain and truncated, both modes."""
    T, seed, stream = 100, 99, 5
    sd, sched = device_sched(T, K)
    rec = {}
    for t in (50, 0):
        lc, lu, xt, known, x_known, tt = width_inputs(K, t)
        for mode in MODES:
            want, gap = known_only(x_known, tt, sd, K, mode, seed, stream)
            ok, left_out = compared(gap.numpy(), known.numpy())
            for trunc in (None, 0.86):
                kw = {} if trunc is None else {"trunc_rate": trunc}
                got, plain = step_pair(G, rows(lc), rows(lu), dev(xt), sched, dev(tt), stream, known, x_known, mode, K=K, T=T,
                                       seed=seed, guidance=2.0, **kw)
                key = f"t{t}_{mode}_{'trunc' if trunc else 'plain'}"
                rec[key] = int((got != want).numpy()[ok].sum())
                assert torch.equal(got[~known], plain[~known]), key
                if t == 0 or mode == "hold":
                    assert torch.equal(got[known], x_known[known]), key
            rec[f"t{t}_{mode}_left_out"] = left_out
    print(K, rec)
    parity_report(f"known_width_{K}", rec)
    assert all(v == 0 for k, v in rec.items() if not k.endswith("left_out")), rec


# ----------------------------------------------------------------------------- 6. the level of the draw
def test_mask_share_is_that_of_level_t_minus_1(G):
    """8192 known positions at t = 50: the [MASK] share is within 5 binomial standard deviations of gamma-bar_49 = 0.495 (the band's
    edges are 0.495 +- 0.028; a draw at level t would centre on gamma-bar_50 = 0.505), every other token is x_known."""
    K, N, t, T = FREQ["K"], FREQ["N"], FREQ["t"], 100
    sd, sched = device_sched(T, K)
    x_known = torch.randint(0, K, (1, N), generator=torch.Generator().manual_seed(FREQ["seed"]))
    nan = torch.full((N, K), float("nan"), device="cuda")
    got = torch.empty((1, N), dtype=torch.int64, device="cuda")
    G.ops.d3pm_step(nan, nan, torch.full((1, N), K, dtype=torch.int64, device="cuda"), got, sched, i64([t]), i64([FREQ["stream"]]), K=K, T=T,
                    guidance=2.0, seed=FREQ["seed"], known=torch.ones((1, N), dtype=torch.uint8, device="cuda"), x_known=dev(x_known),
                    known_mode=0)
    got = got.cpu()
    g_prev = float(sd["log_cumprod_ct"][t - 1].exp())
    share = float((got == K).float().mean())
    sigma = (g_prev * (1 - g_prev) / N) ** 0.5
    want, gap = known_only(x_known, torch.tensor([t]), sd, K, "renoise", FREQ["seed"], FREQ["stream"])
    ok, left_out = compared(gap.numpy())
    rec = {"mask_share": share, "gamma_bar_t_minus_1": g_prev, "band": 5 * sigma, "left_out_share": left_out,
           "mismatches": int((got != want).numpy()[ok].sum()), "other_tokens": int(((got != K) & (got != x_known)).sum())}
    print(rec)
    parity_report("known_mask_share", rec)
    assert abs(share - g_prev) <= 5 * sigma
    assert rec["mismatches"] == 0
    # alpha-bar_49 K beta-bar_49 ~ 1e-5 each: a uniform resample among 8192 draws is rare, and nothing else can come out
    assert rec["other_tokens"] <= 3


# ----------------------------------------------------------------------------- 7. free-running properties
def run(dm, sampler, cond, cf, **kw):
    B = cond.shape[0]
    if sampler == "sample_fast":
        return dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=cf, **kw)["content_token"]
    return dm.sample(["a"] * B, None, cond, cf, filter_ratio=0, **kw)["content_token"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sampler", ["sample", "sample_fast"])
def test_free_running_properties(G, golden, sampler, mode):
    sd, a, cfg = golden("d3pm_L64")
    K, L, B = cfg["K"], cfg["L"], 8
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    content = torch.randint(0, K, (B, L), generator=g)
    mask = torch.rand(B, L, generator=g) < 0.4
    mask[:, :16] = True                                                     # the first frame of the 4 x 4 x 4 grid
    dm = build_d3pm(G, sd, cfg)

    def go(stream=4, **kw):
        dm.set_noise(31, stream=stream)
        out = run(dm, sampler, cond, cf, **kw)
        return out.cpu(), dm.noise_stream - stream, dm._last_lanes
    plain, draws, lanes = go()
    assert lanes == 2
    kw = dict(content_token=content.cuda(), known_mask=mask.cuda(), known_mode=mode)
    toks, n, lanes = go(**kw)
    assert n == draws and lanes == 2                                        # the stream advances as in the plain call
    assert torch.equal(toks[mask], content[mask])                           # the known positions end on their tokens
    assert int((toks == K).sum()) == 0 and not torch.equal(toks[~mask], plain[~mask])
    # one lane, two lanes, and the eager chain give the same tokens; mask and tokens may come from the host
    one, n1, lanes1 = go(**kw, lanes=1)
    trace = []
    eager, n2, _ = go(content_token=content, known_mask=mask, known_mode=mode, trace=trace)
    assert lanes1 == 1 and n1 == n2 == draws
    assert torch.equal(one, toks) and torch.equal(eager, toks) and torch.equal(trace[-1].cpu(), toks) and len(trace) == draws
    held = [bool(torch.equal(t.cpu()[mask], content[mask])) for t in trace]
    if mode == "hold":
        assert all(held)
    else:                                                                   # re-noised: [MASK] at first, the tokens at the end
        assert not held[0] and held[-1] and float((trace[0].cpu()[mask] == K).float().mean()) > 0.9
    # an all-False mask is the plain call bit for bit, an all-True one returns content_token
    none, n3, _ = go(content_token=content.cuda(), known_mask=torch.zeros(B, L, dtype=torch.bool), known_mode=mode)
    every, n4, _ = go(content_token=content.cuda(), known_mask=torch.ones(L, dtype=torch.bool), known_mode=mode)
    assert torch.equal(none, plain) and torch.equal(every, content) and n3 == n4 == draws
    # and no mask at all still is
    again, _, _ = go()
    assert torch.equal(again, plain)


# ----------------------------------------------------------------------------- 8. the generator glue
@pytest.mark.parametrize("skip", [None, 1])
def test_glue_conditions_on_the_first_frame(G, golden, skip):
    from tests.test_gpu_glue import build
    gen, vq, batch, a, cfg, cfgd = build(G, golden)
    gen = G.DiscreteDiffusion(gen.textencoder, gen.diffusion_model, sample_condition_frames=1, sample_skip_step=skip)
    dm = gen.diffusion_model.eval()
    dm.set_noise(cfg["noise_seed"], stream=int(cfg["stream"]))
    with torch.no_grad():
        quant = vq.encode(batch["video"])
        out = gen(batch, vq, None, do_inference=True)
        pred = out["pred_data"]
    B = quant.shape[0]
    per_frame = quant[0, 0].numel()
    tok = gen.last_content_token
    assert tok.shape == (B, quant[0].numel())
    assert torch.equal(tok[:, :per_frame], quant.view(B, -1)[:, :per_frame])             # the first latent frame carries the input's codes
    assert not torch.equal(tok[:, per_frame:], quant.view(B, -1)[:, per_frame:]) and int((tok == cfgd["K"]).sum()) == 0
    assert pred.shape == batch["video"].shape and bool(torch.isfinite(pred).all())
    with torch.no_grad():
        torch.testing.assert_close(pred, vq.decode(tok.view(quant.shape)), atol=0, rtol=0)
