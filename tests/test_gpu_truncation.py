"""Top-r truncated sampling (DiffusionTransformer.truncation_rate; VQ-Diffusion's predict_start_with_truncation, "top0.86r") on the
MI355X.

The pin is tests/golden/truncation_L64.npz: the reference's own sample() on the d3pm_L64 model with its cf_predict_start wrapped by
the rule as tests/test_truncation_host.py restates it, and torch.rand_like replaced by Philox draws
(tests/golden/make_golden_truncation.py).  Truncation is a threshold decision, so the fixture records per step and position how close
the reference's own row was to the boundary (min_k |mass_above(k) - r|) and the gap between the two best Gumbel values.  Tokens are
compared exactly wherever the margin is at least 1e-4 -- 5 x the cumulative-mass error that the 2e-5 allowed between device and
reference log-probabilities can cause, the mass being at most 1 -- and the gap at least 1e-3; the positions left out must stay under
5 % of all positions, which every test asserts for its own inputs."""
import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_parity import build_d3pm
from tests.test_truncation_host import boundary_margin, mass_above, truncate_rows

pytestmark = pytest.mark.gpu

RATE = 0.86
MARGIN_FLOOR, GAP_FLOOR, MAX_LEFT_OUT = 1e-4, 1e-3, 0.05


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


def top2_gap(logp, seed, stream, row0=0):
    """(B, L): the gap between the two best Gumbel + log-probability values of the (B, K+1, L) draw at `stream`."""
    from oracle import philox
    B, K1, L = logp.shape
    u = philox.uniform_bkl(seed, stream, B, K1, L, row0=row0)
    v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + np.asarray(logp, dtype=np.float32)).astype(np.float32), axis=1)
    return v[:, -1, :] - v[:, -2, :]


def truncated(rec, rate=RATE):
    return torch.from_numpy(truncate_rows(rec.numpy(), rate))


def compared(margin, gap):
    """The positions a token comparison covers, after asserting that the ones left out are at most 5 %."""
    out = (np.asarray(margin) < MARGIN_FLOOR) | (np.asarray(gap) < GAP_FLOOR)
    assert out.mean() <= MAX_LEFT_OUT, f"{out.mean():.3%} of the positions are within the floors: the inputs are too close to the boundary"
    return ~out, float(out.mean())


# ----------------------------------------------------------------------------- 1. the kernel against the fixture's rows
def test_step_kernel_truncated_rows_match_the_fixture(G, golden):
    sd, _, cfg = golden("d3pm_L64")
    _, a, tcfg = golden("truncation_L64")
    dm = build_d3pm(G, sd, cfg)
    B, K, L = a["first_logits"].shape
    T = cfg["T"]
    xt = torch.full((B, L), K, dtype=torch.int64, device="cuda")
    x0 = torch.empty((B, K + 1, L), device="cuda")
    out = torch.empty_like(xt)
    G.ops.d3pm_step(rows(a["first_logits"]), rows(a["first_logits_uncond"]), xt, out, dm._sched(), i64([T - 1] * B), i64([0]), K=K, T=T,
                    guidance=float(cfg["guidance"]), seed=tcfg["noise_seed"], x0_dbg=x0, trunc_rate=tcfg["rate"])
    got, want = x0.cpu().numpy(), a["first_rows"]
    kept_got, kept_want = got != -70, want != -70
    err = float(np.abs(got - want)[kept_want & kept_got].max())
    rec = {"kept_set_mismatches": int((kept_got != kept_want).sum()), "max_abs_err_kept": err, "kept_per_row_mean": float(kept_want.sum(1).mean()),
           "min_margin": float(a["margin"][0].min())}
    print(rec)
    parity_report("truncation_step_rows", rec)
    assert a["margin"][0].min() >= MARGIN_FLOOR                 # no row of the first call is near the boundary: the sets must be equal
    assert np.array_equal(kept_got, kept_want)
    assert err <= 2e-5
    assert (got[~kept_want] == -70).all() and (got[:, -1] == -70).all()
    assert kept_want[:, :-1].sum(1).min() >= 1 and kept_want[:, :-1].sum(1).max() < K          # something was cut, something kept
    # the hook-free instantiation draws the hooked one's tokens, and those of the fixture's first step where it is decided
    plain = torch.empty_like(xt)
    G.ops.d3pm_step(rows(a["first_logits"]), rows(a["first_logits_uncond"]), xt, plain, dm._sched(), i64([T - 1] * B), i64([0]), K=K, T=T,
                    guidance=float(cfg["guidance"]), seed=tcfg["noise_seed"], trunc_rate=tcfg["rate"])
    assert torch.equal(plain, out)
    ok, _ = compared(a["margin"][0], a["gap"][0])
    assert np.array_equal(out.cpu().numpy()[ok], a["trace"][0].astype(np.int64)[ok])
    # without truncation the same launch leaves classes the truncated row has cut
    G.ops.d3pm_step(rows(a["first_logits"]), rows(a["first_logits_uncond"]), xt, plain, dm._sched(), i64([T - 1] * B), i64([0]), K=K, T=T,
                    guidance=float(cfg["guidance"]), seed=tcfg["noise_seed"], x0_dbg=x0)
    assert int(((x0.cpu().numpy() != -70) & ~kept_want).sum()) > 0


# ----------------------------------------------------------------------------- 2. the fixture's chain, teacher-forced
def test_teacher_forced_chain_reproduces_the_fixture(G, golden):
    """Step i from the fixture's trace[i-1] at stream i must give trace[i], at every position whose decision the reference itself
    made at least the floors away from a flip."""
    sd, b, cfg = golden("d3pm_L64")
    _, a, tcfg = golden("truncation_L64")
    dm = build_d3pm(G, sd, cfg)
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    cond = dev(b["step_cond"])
    cf = torch.zeros_like(cond)
    dm.set_noise(tcfg["noise_seed"])
    trace = a["trace"].astype(np.int64)
    ok, left_out = compared(a["margin"], a["gap"])
    assert trace.shape == (T, B, L)
    bad = []
    for i in range(T):
        prev = torch.full((B, L), K, dtype=torch.int64, device="cuda") if i == 0 else dev(trace[i - 1])
        got = dm.p_sample_tokens(prev, cond, cf, i64([T - 1 - i] * B), i, truncation_rate=tcfg["rate"]).cpu().numpy()
        n = int((got != trace[i])[ok[i]].sum())
        if n:
            bad.append((i, n))
    rec = {"steps": T, "positions": int(ok.size), "left_out_share": left_out, "mismatches": int(sum(n for _, n in bad))}
    print(rec)
    parity_report("truncation_teacher_forced", rec)
    assert not bad, f"(step, mismatching positions): {bad[:10]}"


# ----------------------------------------------------------------------------- 3. the production instantiations
def production_inputs(K, B, L, seed, guided):
    """Logits of sigma 5.  A row's margin is at most half the probability of the class at the r = 0.86 boundary, so the share of rows
    within 1e-4 is about 2e-4 over that probability.  Measured on the restatement alone, 512 rows of 4096 classes each, guided /
    unguided: sigma 2: 76 % / 93 % of the rows within 1e-4 (the boundary class carries ~2e-4; ~500-700 classes kept), sigma 3: 20 % / 28 %,
    sigma 4: 4.1 % / 5.7 %, sigma 5: 1.0 % / 1.2 % (~10 classes kept), sigma 6: 0.2 % / 0 %.  Sigma 5 is the smallest that keeps the
    reference itself well inside the 5 % cap."""
    g = torch.Generator().manual_seed(seed)
    lc = torch.randn(B, K, L, generator=g) * 5.0
    lu = lc + torch.randn(B, K, L, generator=g) if guided else None
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    xt[1] = K                                                                            # one sample all [MASK]
    return lc, lu, xt


def recon_rows(lc, lu):
    from oracle import d3pm as od
    if lu is None:
        return od.predict_start_from_logits(lc)
    return od.cf_mix(od.predict_start_from_logits(lc)[:, :-1], od.predict_start_from_logits(lu)[:, :-1], 2.0)


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("post_skip", [0, 3])
def test_step_kernel_truncated_production_instantiation(G, guided, post_skip):
    """K = 4096 without debug buffers (d3pm_step_trunc_kernel<16, true, false>), masked and unmasked x_t, t on both sides of post_skip:
    tokens exact against the restatement (oracle pieces + truncate_rows) on the rows that pass the floors."""
    from oracle import d3pm as od
    from gsdd_amd.d3pm import SCHED_ORDER
    K, B, L, T, seed, stream = 4096, 6, 32, 100, 4321, 7
    lc, lu, xt = production_inputs(K, B, L, K + post_skip + (10 if guided else 0), guided)
    t = torch.tensor([57, 0, 99, 3, 4, 30])
    tp = torch.where(t > post_skip, t - post_skip, t)
    sd = od.schedule_buffers(T, K)
    sched = [dev(sd[n]) for n in SCHED_ORDER]
    rec = recon_rows(lc, lu)
    post = od.q_posterior(truncated(rec), od.index_to_log_onehot(xt, K + 1), tp, sd)
    want = od.gumbel_argmax(post, seed, stream)
    ok, left_out = compared(boundary_margin(rec.numpy(), RATE), top2_gap(post.numpy(), seed, stream))
    got = torch.empty_like(xt).cuda()
    G.ops.d3pm_step(rows(lc), rows(lu) if guided else None, dev(xt), got, sched, dev(t), i64([stream]), K=K, T=T, guidance=2.0 if guided else 1.0,
                    seed=seed, post_skip=post_skip, trunc_rate=RATE)
    mism = int((got.cpu() != want).numpy()[ok].sum())
    # the truncation must matter on these inputs: the untruncated posterior draws other tokens somewhere
    plain = od.gumbel_argmax(od.q_posterior(rec, od.index_to_log_onehot(xt, K + 1), tp, sd), seed, stream)
    rec_ = {"mismatches": mism, "positions": B * L, "left_out_share": left_out, "tokens_truncation_changes": int((plain != want).sum())}
    print(rec_)
    parity_report(f"truncation_step_k4096_{'guided' if guided else 'plain'}_s{post_skip}", rec_)
    assert mism == 0
    assert int((plain != want).sum()) > 0


def purity_restate(rec, rule, weight, seed, stream):
    """prob and the candidate tokens of a purity call on an already truncated log_x_recon (diffusion_transformer.py:313-326)."""
    from oracle import d3pm as od
    score = torch.exp(rec).max(dim=1).values.clamp(0, 1)
    score = score / (score.max(dim=1, keepdim=True).values + 1e-10)
    prob = ((1 + score * weight).unsqueeze(1) * rec).softmax(dim=1).log().clamp(-70, 0) if rule != 1 and weight > 0 else rec
    return prob, score, od.gumbel_argmax(prob, seed, stream)


def purity_buffers(B, L, K, dbg=False):
    f = dict(dtype=torch.float32, device="cuda")
    out = {"score": torch.empty((B, L), **f), "smax": torch.empty((B,), **f), "cand": torch.empty((B, L), dtype=torch.int64, device="cuda")}
    if dbg:
        out.update(recon_dbg=torch.empty((B, K + 1, L), **f), prob_dbg=torch.empty((B, K + 1, L), **f), score_dbg=torch.empty((B, L), **f))
    return out


@pytest.mark.parametrize("weight", [0.0, 1.0])
def test_purity_kernel_truncated_rows_match_the_fixture(G, golden, weight):
    """Rule 2 on the fixture's first logits (K = 32, hooked instantiation): recon_dbg is the fixture's truncated row, prob_dbg the
    re-weighted truncated row, the score is the untruncated call's (the row maximum is always kept)."""
    _, a, tcfg = golden("truncation_L64")
    B, K, L = a["first_logits"].shape
    seed, stream = tcfg["noise_seed"], 0
    lc, lu, sid = rows(a["first_logits"]), rows(a["first_logits_uncond"]), i64([stream])
    buf = purity_buffers(B, L, K, dbg=True)
    G.ops.d3pm_purity_step(lc, lu, buf["score"], buf["smax"], buf["cand"], sid, K=K, guidance=2.0, prior_rule=2, prior_weight=weight, seed=seed,
                           recon_dbg=buf["recon_dbg"], prob_dbg=buf["prob_dbg"], score_dbg=buf["score_dbg"], trunc_rate=tcfg["rate"])
    want_rec = a["first_rows"]
    prob, score, want_cand = purity_restate(torch.from_numpy(want_rec), 2, weight, seed, stream)
    got_rec, got_prob = buf["recon_dbg"].cpu().numpy(), buf["prob_dbg"].cpu().numpy()
    kept = want_rec != -70
    assert np.array_equal(got_rec != -70, kept) and (got_rec[~kept] == -70).all()
    err = {"recon": float(np.abs(got_rec - want_rec).max()), "prob": float(np.abs(got_prob - prob.numpy()).max()),
           "score": float(np.abs(buf["score_dbg"].cpu().numpy() - score.numpy()).max())}
    print(weight, err)
    assert max(err.values()) <= 2e-5, err
    ok, left_out = compared(a["margin"][0], top2_gap(prob.numpy(), seed, stream))
    assert np.array_equal(buf["cand"].cpu().numpy()[ok], want_cand.numpy()[ok])
    # hook-free instantiation: same candidates; untruncated call: same scores
    plain, off = purity_buffers(B, L, K), purity_buffers(B, L, K)
    G.ops.d3pm_purity_step(lc, lu, plain["score"], plain["smax"], plain["cand"], sid, K=K, guidance=2.0, prior_rule=2, prior_weight=weight,
                           seed=seed, trunc_rate=tcfg["rate"])
    G.ops.d3pm_purity_step(lc, lu, off["score"], off["smax"], off["cand"], sid, K=K, guidance=2.0, prior_rule=2, prior_weight=weight, seed=seed)
    assert torch.equal(plain["cand"], buf["cand"]) and torch.equal(plain["score"], off["score"]) and torch.equal(plain["smax"], off["smax"])
    parity_report(f"truncation_purity_rows_w{weight:g}", {**err, "left_out_share": left_out})


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("weight", [0.0, 1.0])
def test_purity_kernel_truncated_production_instantiation(G, weight, guided):
    """K = 4096 without debug buffers (d3pm_purity_trunc_kernel<16, true, 0 / 2, false>), rule 2: candidates exact against the
    restatement on the rows that pass the floors."""
    K, B, L, seed, stream = 4096, 6, 32, 4321, 7
    lc, lu, _ = production_inputs(K, B, L, K + 77 + int(weight) + (10 if guided else 0), guided)
    rec = recon_rows(lc, lu)
    prob, _, want = purity_restate(truncated(rec), 2, weight, seed, stream)
    ok, left_out = compared(boundary_margin(rec.numpy(), RATE), top2_gap(prob.numpy(), seed, stream))
    buf = purity_buffers(B, L, K)
    G.ops.d3pm_purity_step(rows(lc), rows(lu) if guided else None, buf["score"], buf["smax"], buf["cand"], i64([stream]), K=K,
                           guidance=2.0 if guided else 1.0, prior_rule=2, prior_weight=weight, seed=seed, trunc_rate=RATE)
    mism = int((buf["cand"].cpu() != want).numpy()[ok].sum())
    _, _, untruncated = purity_restate(rec, 2, weight, seed, stream)
    rec_ = {"mismatches": mism, "positions": B * L, "left_out_share": left_out, "tokens_truncation_changes": int((untruncated != want).sum())}
    print(rec_)
    parity_report(f"truncation_purity_k4096_{'guided' if guided else 'plain'}_w{weight:g}", rec_)
    assert mism == 0
    assert int((untruncated != want).sum()) > 0


# ----------------------------------------------------------------------------- 4. free-running properties
SAMPLERS = ["sample", "sample_fast", "purity"]


def make_dm(G, golden, sampler):
    sd, a, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    if sampler == "purity":
        _, p, pcfg = golden("purity_L64")
        dm.prior_rule, dm.prior_weight, dm.prior_ps, dm.n_sample = 2, 1.0, pcfg["prior_ps"], p["n_sample"].tolist()
    return dm


def run(dm, sampler, cond, cf, **kw):
    B = cond.shape[0]
    if sampler == "sample_fast":
        return dm.sample_fast(["a"] * B, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=cf, **kw)["content_token"]
    return dm.sample(["a"] * B, None, cond, cf, filter_ratio=0, **kw)["content_token"]


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_free_running_properties(G, golden, sampler):
    sd, a, cfg = golden("d3pm_L64")
    K = cfg["K"]
    g = torch.Generator().manual_seed(11)
    cond8 = torch.randn(8, 1, cfg["cond_dim"], generator=g).cuda()
    cf8 = torch.randn(8, 1, cfg["cond_dim"], generator=g).cuda()
    cond, cf = cond8[:2].contiguous(), cf8[:2].contiguous()
    # captured graph == eager trace run, token for token
    dm = make_dm(G, golden, sampler)
    dm.truncation_rate = RATE
    dm.set_noise(31, stream=4)
    trace = []
    eager = run(dm, sampler, cond, cf, trace=trace)
    draws = dm.noise_stream - 4
    dm.set_noise(31, stream=4)
    graph = run(dm, sampler, cond, cf, use_graph=True)
    assert torch.equal(eager, graph) and torch.equal(trace[-1], eager) and dm.noise_stream - 4 == draws
    # truncation changes the tokens of this chain; None is the run without the attribute, bit for bit
    toks = {}
    for name in ("default", "none", "deleted"):
        dm = make_dm(G, golden, sampler)
        if name == "none":
            dm.truncation_rate = None
        elif name == "deleted":
            del dm.truncation_rate
        dm.set_noise(31, stream=4)
        toks[name] = run(dm, sampler, cond, cf)
        assert dm.noise_stream - 4 == draws
    assert torch.equal(toks["default"], toks["none"]) and torch.equal(toks["default"], toks["deleted"])
    assert not torch.equal(toks["default"], eager)
    # a batch of 8 equals two batches of 4 keyed at their global rows
    dm = make_dm(G, golden, sampler)
    dm.truncation_rate = RATE
    dm.set_noise(77, stream=2)
    full = run(dm, sampler, cond8, cf8)
    for half in (0, 1):
        dm.set_noise(77, stream=2, row_offset=4 * half)
        part = run(dm, sampler, cond8[4 * half:4 * half + 4].contiguous(), cf8[4 * half:4 * half + 4].contiguous())
        assert torch.equal(part, full[4 * half:4 * half + 4]), half


def test_changed_tokens_lie_in_the_kept_set(G, golden):
    """An eager plain chain: every token that changed at step i lies in the restatement's kept set of its row, widened by the classes
    within the 1e-4 margin; the restatement runs the oracle denoiser on the device's own trace[i-1]."""
    from oracle import d3pm as od
    sd, a, cfg = golden("d3pm_L64")
    dm = make_dm(G, golden, "sample")
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    cond = torch.from_numpy(a["step_cond"])
    cf = torch.zeros_like(cond)
    dm.truncation_rate = RATE
    dm.set_noise(5)
    trace = []
    run(dm, "sample", cond.cuda(), cf.cuda(), trace=trace)
    trace = [t.cpu() for t in trace]
    assert len(trace) == T
    changed = outside = 0
    kept_sizes = []
    with torch.no_grad():
        for i in range(T):
            prev = torch.full((B, L), K, dtype=torch.long) if i == 0 else trace[i - 1]
            if i == 0:
                log_z = torch.full((B, K + 1, L), float("-inf"))
                log_z[:, -1] = 0
            else:
                log_z = od.index_to_log_onehot(prev, K + 1)
            rec = od.cf_predict_start(log_z, cond, cf, torch.full((B,), T - 1 - i, dtype=torch.long), sd, cfg["guidance"]).numpy()
            wide = mass_above(rec) < RATE + MARGIN_FLOOR                                  # (B, K+1, L)
            kept_sizes.append(wide[:, :-1].sum(1).mean())
            moved = (trace[i] != prev).numpy()
            tok = trace[i].numpy()
            inside = np.take_along_axis(wide, tok[:, None, :], 1)[:, 0, :]
            changed += int(moved.sum())
            outside += int((moved & ~inside).sum())
    rec_ = {"changed_tokens": changed, "outside_kept_set": outside, "mean_kept_classes": float(np.mean(kept_sizes))}
    print(rec_)
    parity_report("truncation_changed_tokens", rec_)
    assert changed >= B * L and np.mean(kept_sizes) < K - 1
    assert outside == 0
