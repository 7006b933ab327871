"""Composed guidance on the MI355X: gsdd_d3pm_compose (csrc/d3pm_compose.hip) against the fp64 restatement of tests/compose_ref.py at
every class width, and the sampler's composed calls on the two-layer golden model.

WIDTHS.  K = 4, 252, 256, 260, 512, 1024, 2048, 4092, 4096, 4100, 8192, 1020, 2044 (J = 1, 2, 4, 8, 16 in one pass, J = 32 in two, the
FULL instantiation of K = 4096), N = 1 ... 4 with the weight sets of compose_ref.WEIGHT_SETS, 111 positions at row0 = 1000.  Bars (all
from compose_ref): e within 2e-5 + 2^-22 |e_fp64|; the step run on e, through its x0_dbg hook, within the flat 2e-5 of fp64; tokens of
the hooked and of the hook-free step equal to the reference's wherever the fp64 top-two Gumbel gap is at least 1e-3, at most 1 % of
a case left out.  The CPU's f32 emulation of the restatement gave at most 1.2e-5 on x0 and a ratio of at most 0.39 on e
(test_compose_host.py prints them); the achieved values go to the parity report (MI355X: 1.18e-5 on x0 and a ratio of 0.39 on e
at worst, the emulation's own figures; no token mismatch, at most one position of 111 left out).  In place (out = block 0) gives the bits of a
separate out; sentinels around out and the weights stay intact.
The kernel's log-softmax is the step's, bit for bit: with all weights zero e is x_u exactly (x_u + 0 (x_i - x_u)), held against the
x0_dbg rows of the unguided step on the null block, at every width -- the two-pass J = 32 included.  The FULL and the partly empty
J = 16 instantiations agree bit for bit on a K = 4096 row whose last quad is -inf, which is what a K = 4092 row is to its kernel.

SPECIAL CASES.  Weights (s, 1 - s) against the two-way d3pm_step(lc, l_neg, guidance = s), and N = 1, w = 2 against the guided step, both
through x0_dbg within twice the bar (each side is within the bar of the same fp64 row).

CHAIN (tests.test_gpu_parity.build_d3pm, L = 64, 8 clips; Te = 1: the fused path, Te = 3 with lengths: the unfused one; N = 2 with a
per-clip weight sweep, N = 4).  A graphed two-lane call, a graphed one-lane call and an eager traced call give the same tokens bit for
bit; the trace equals a manual loop of tr.run(rep = N + 1) -> ops.d3pm_compose -> ops.d3pm_step(logits_u = None), launch for launch;
compose_embeds = None is the parent's call.  Once each with skip_step = 1, truncation_rate = 0.86, prior_rule = 2, a known-frame mask and
sample_long over two windows.  The stacked pass itself, rep = 3, 4, 5: every block equals the rep = 1 pass on its condition.  Weights (1, 0, ...) reproduce the unguided step's tokens outside near ties."""
import math

import pytest
import torch

from tests import compose_ref as cr
from tests.conftest import parity_report
from tests.test_gpu_objective_kernels import SCHED_ORDER, STEP_ROW0, T, guarded, intact, step_rows
from tests.test_gpu_parity import LOGIT_TOL, build_d3pm
from tests.test_gpu_sampler_widths import B, BAR, GUIDANCE, L, STEP_STREAM, case, maxerr
from tests.test_gpu_truncation import GAP_FLOOR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def stacked(blocks, K):
    """(N + 1) blocks of [B L][K] rows, as the denoiser leaves them"""
    return torch.cat([step_rows(b, K) for b in blocks], 0).contiguous()


def bkl(rows, K):
    """[B L][K] rows -> (B, K, L) on the CPU"""
    return rows.view(B, L, K).permute(0, 2, 1).contiguous().cpu()


def run_compose(G, blocks, w, K, in_place=False):
    """-> (e rows [B L][K] on the device, guards intact)"""
    N = len(blocks) - 1
    ew = guarded((B, N), torch.float32, 16, 16, fill=w.cuda())
    if in_place:
        el = guarded(((N + 1) * B * L, K), torch.float32, 64, 64, fill=stacked(blocks, K))
        out = G.ops.d3pm_compose(el[1], ew[1], n_cond=N, B=B, L=L, K=K)
        torch.cuda.synchronize()
        assert out.data_ptr() == el[1].data_ptr() and torch.equal(el[1][B * L:], stacked(blocks, K)[B * L:]), "a block other than 0 changed"
        return out, intact(el) and intact(ew)
    eo = guarded((B * L, K), torch.float32, 64, 64)
    logits = stacked(blocks, K)
    before = logits.clone()
    G.ops.d3pm_compose(logits, ew[1], n_cond=N, B=B, L=L, K=K, out=eo[1])
    torch.cuda.synchronize()
    assert torch.equal(logits, before), "the logits changed under a separate out"
    return eo[1], intact(eo) and intact(ew) and torch.equal(ew[1].cpu(), w)


def run_step(G, c, rows_c, rows_u=None, hooked=True, guidance=GUIDANCE):
    """d3pm_step on [B L][K] rows -> (x0 (B, K + 1, L) or None, tokens), CPU"""
    K = c["K"]
    x0 = torch.empty((B, K + 1, L), device="cuda") if hooked else None
    tok = torch.empty((B, L), dtype=torch.int64, device="cuda")
    G.ops.d3pm_step(rows_c, rows_u, c["xt"].cuda(), tok, [c["sd"][n].cuda() for n in SCHED_ORDER], c["t"].cuda(), i64([STEP_STREAM]), K=K, T=T,
                    guidance=guidance, seed=c["seed"], row0=STEP_ROW0, x0_dbg=x0)
    torch.cuda.synchronize()
    return None if x0 is None else x0.cpu(), tok.cpu()


# ----------------------------------------------------------------------------- every class width
@pytest.mark.parametrize("K,name", cr.CASES, ids=cr.CASE_IDS)
def test_compose_at_every_class_width(G, K, name):
    I, R = cr.inputs(K, name), cr.reference(K, name)
    c = I["c"]
    e, ok = run_compose(G, I["blocks"], I["w"], K)
    assert ok, "d3pm_compose wrote outside out or into the weights"
    e_in, ok_in = run_compose(G, I["blocks"], I["w"], K, in_place=True)
    assert ok_in, "d3pm_compose (in place) wrote outside the logits or into the weights"
    in_place_differs = int((e_in.view(torch.int32) != e.view(torch.int32)).sum())
    x0, tok = run_step(G, c, e.contiguous())
    _, tok_plain = run_step(G, c, e.contiguous(), hooked=False)
    rec = cr.check(dict(e=bkl(e, K), x0=x0, tok=tok), R)
    rec.update(in_place_differs=in_place_differs, plain_differs_from_hooked=int((tok_plain != tok).sum()), positions=B * L)
    parity_report(f"compose::widths[K{K}_{name}]", rec)
    assert not cr.failures(rec) and in_place_differs == 0 and rec["plain_differs_from_hooked"] == 0, rec


@pytest.mark.parametrize("K", cr.KS)
def test_zero_weights_leave_the_steps_own_log_softmax(G, K):
    """e = x_u + 0 (x_i - x_u) = x_u exactly: the kernel's clamp(log_softmax) against the unguided step's x0_dbg rows, bit for bit, in the
    one-pass widths and in the two-pass J = 32."""
    I = cr.inputs(K, "w1_0.75_-0.25")
    c = I["c"]
    e, ok = run_compose(G, I["blocks"], torch.zeros(B, 3), K)
    x0, _ = run_step(G, c, step_rows(I["blocks"][-1], K))
    assert ok and torch.equal(bkl(e, K), x0[:, :K].contiguous())          # (equal as floats: no NaN, and 0 is 0 whatever its sign)


def test_full_and_partly_empty_instantiations_agree(G):
    """K = 4096 with -inf in the last quad (FULL, every slot loaded) against the same rows at K = 4092 (the last slot of lane 63 filled
    with -inf by the kernel): the first 4092 classes bit for bit, the -inf classes at the clamp."""
    I = cr.inputs(4096, "w1.5_0.75_-0.5_-0.25")
    blocks = [b.clone() for b in I["blocks"]]
    for b in blocks:
        b[:, -4:] = -math.inf
    full, ok = run_compose(G, blocks, I["w"], 4096)
    part, ok2 = run_compose(G, [b[:, :-4].contiguous() for b in blocks], I["w"], 4092)
    assert ok and ok2
    assert torch.equal(full[:, :4092].contiguous().view(torch.int32), part.contiguous().view(torch.int32)) and bool((full[:, 4092:] == -70).all())


# ----------------------------------------------------------------------------- special cases against the existing two-way step
@pytest.mark.parametrize("K", [260, 4096, 8192])
def test_two_way_special_cases_against_the_guided_step(G, K):
    c = case(K, True)
    g = torch.Generator().manual_seed(5)
    neg = c["lc"] + torch.randn(c["lc"].shape, generator=g)
    s = GUIDANCE
    # (s, 1 - s) on (caption, negative caption): x_u cancels, the row is the guided step's with the negative caption as cf
    e, ok = run_compose(G, [c["lc"], neg, c["lu"]], torch.tensor([[s, 1 - s]]).expand(B, 2).contiguous(), K)
    x0_c, _ = run_step(G, c, e.contiguous())
    x0_g, _ = run_step(G, c, step_rows(c["lc"], K), step_rows(neg, K), guidance=s)
    neg_err = maxerr(x0_c, x0_g.double())
    # N = 1, w = s: the guided step itself
    e1, ok1 = run_compose(G, [c["lc"], c["lu"]], torch.full((B, 1), s), K)
    x0_1, _ = run_step(G, c, e1.contiguous())
    x0_2, _ = run_step(G, c, step_rows(c["lc"], K), step_rows(c["lu"], K), guidance=s)
    one_err = maxerr(x0_1, x0_2.double())
    parity_report(f"compose::two_way[K{K}]", {"negative_prompt_max_err": neg_err, "one_condition_max_err": one_err,
                                              "worst_ratio": max(neg_err, one_err) / (2 * BAR)})
    assert ok and ok1 and neg_err <= 2 * BAR and one_err <= 2 * BAR, (neg_err, one_err)


# ----------------------------------------------------------------------------- the chain on the golden model
NB, SEED = 8, 9127
SHAPE = (4, 4, 4)
LENS = {0: [1, 3, 2, 3, 1, 2, 3, 3], 1: [3, 1, 2, 2, 3, 3, 1, 2], 2: [2, 2, 3, 1, 1, 3, 2, 3], 3: [3, 3, 1, 2, 2, 1, 3, 1]}


def chain_inputs(cfg, Te, N):
    g = torch.Generator().manual_seed(300 + 10 * Te + N)
    C = cfg["cond_dim"]
    cond = torch.randn(NB, Te, C, generator=g).cuda()
    extra = [torch.randn(NB, Te, C, generator=g).cuda() for _ in range(N - 1)]
    cf = torch.zeros(NB, Te, C).cuda()
    if N == 2:                                   # a per-clip sweep between two captions: clip b at (s (1 - a_b), s a_b)
        a = torch.linspace(0, 1, NB)
        w = torch.stack([2.0 * (1 - a), 2.0 * a], 1)
    else:
        w = torch.tensor([1.5, 0.75, -0.5, -0.25])
    kw = dict(compose_embeds=extra, compose_weights=w)
    if Te > 1:
        kw.update(condition_len=LENS[0], compose_lens=[LENS[i] for i in range(1, N)])
    return cond, cf, kw


@pytest.fixture(scope="module")
def model(G, golden):
    sd, _, cfg = golden("d3pm_L64")
    return build_d3pm(G, sd, cfg), cfg


def sample(dm, cond, cf, fast=None, **kw):
    dm.set_noise(SEED, stream=2)
    texts = ["a"] * NB
    if fast is not None:
        return dm.sample_fast(texts, None, cond, filter_ratio=0, skip_step=fast, cf_condition_embed=cf, **kw)["content_token"].cpu()
    return dm.sample(texts, None, cond, cf, filter_ratio=0, **kw)["content_token"].cpu()


def manual_chain(G, dm, cond, cf, kw):
    """the composed chain launch for launch: tr.run(rep = N + 1) -> d3pm_compose -> d3pm_step(logits_u = None) -> advance"""
    tr, Lq, K, Tq = dm.transformer, dm.shape, dm.num_classes - 1, dm.num_timesteps
    extra, w = kw["compose_embeds"], torch.as_tensor(kw["compose_weights"]).float()
    N, Te = len(extra) + 1, cond.shape[1]
    w = (w[None].expand(NB, N) if w.dim() == 1 else w).contiguous().cuda()
    lens = None
    if "condition_len" in kw:
        lens = torch.tensor(kw["condition_len"] + sum(kw["compose_lens"], []) + [Te] * NB, dtype=torch.int32).cuda()
    tr.packed(); tr.fragment_images()
    condv = tr.cond_vectors(torch.cat([cond, *extra, cf], 0).contiguous())
    ws = tr.workspace((N + 1) * NB, Lq, "cuda", rep=N + 1)
    t2, sid = torch.full(((N + 1) * NB,), Tq - 1, dtype=torch.int64, device="cuda"), i64([2])
    tok = torch.full((NB, Lq), K, dtype=torch.int64, device="cuda")
    sched = dm._sched()
    trace = []
    for _ in range(Tq):
        logits = tr.run(tok, condv, Te, t2, ws, rep=N + 1, cond_len=lens)
        mix = G.ops.d3pm_compose(logits, w, n_cond=N, B=NB, L=Lq, K=K)
        G.ops.d3pm_step(mix, None, tok, tok, sched, t2, sid, K=K, T=Tq, guidance=float(dm.guidance_scale), seed=SEED, row0=0)
        G.ops.advance(t2, -1, sid, 1)
        trace.append(tok.clone().cpu())
    return trace


@pytest.mark.parametrize("Te,N", [(1, 2), (1, 4), (3, 2), (3, 4)])
def test_composed_chain_graphed_eager_and_manual(G, model, Te, N):
    dm, cfg = model
    cond, cf, kw = chain_inputs(cfg, Te, N)
    two = sample(dm, cond, cf, **kw)
    assert dm._last_lanes == 2 and not dm._last_cfg_dedupe and dm.noise_stream == 2 + dm.num_timesteps
    one = sample(dm, cond, cf, lanes=1, **kw)
    assert dm._last_lanes == 1
    trace = []
    eager = sample(dm, cond, cf, trace=trace, **kw)
    assert len(trace) == dm.num_timesteps and int(two.min()) >= 0 and int(two.max()) < cfg["K"]
    assert torch.equal(two, one), "two lanes != one lane"
    assert torch.equal(two, eager), "captured chain != eager trace"
    manual = manual_chain(G, dm, cond, cf, kw)
    bad = [i for i in range(len(trace)) if not torch.equal(trace[i].cpu(), manual[i])]
    assert not bad, f"the trace leaves the manual loop at step {bad[0]}"
    guided = sample(dm, cond, cf)
    assert not torch.equal(guided, two), "the composed conditions change no token"
    # compose_embeds = None is the call without the keywords
    assert torch.equal(sample(dm, cond, cf, compose_embeds=None, compose_weights=None, compose_lens=None), guided)
    # the weights are the scales: guidance_scale plays no part
    scale = dm.guidance_scale
    try:
        dm.guidance_scale = 1.0
        assert torch.equal(sample(dm, cond, cf, **kw), two)
    finally:
        dm.guidance_scale = scale
    parity_report(f"compose::chain[Te{Te}_N{N}]", {"steps": len(trace), "mismatches": 0,
                                                   "tokens_changed_by_composing": int((guided != two).sum()), "tokens": int(two.numel())})


@pytest.mark.parametrize("variant", ["skip_step", "truncation", "purity", "known", "long"])
def test_every_plan_takes_composed_conditions(G, model, golden, variant):
    dm, cfg = model
    cond, cf, kw = chain_inputs(cfg, 1, 4)
    Lq, K = dm.shape, cfg["K"]
    call = lambda **more: sample(dm, cond, cf, **kw, **more)
    plain = lambda **more: sample(dm, cond, cf, **more)
    names = ("truncation_rate", "prior_rule", "prior_weight", "prior_ps", "n_sample")      # the model is shared: left as it was found
    before = {n: getattr(dm, n, None) for n in names}
    try:
        if variant == "skip_step":
            call, plain = (lambda **more: sample(dm, cond, cf, fast=1, **kw, **more)), (lambda **more: sample(dm, cond, cf, fast=1, **more))
        elif variant == "truncation":
            dm.truncation_rate = 0.86
        elif variant == "purity":
            _, p, pcfg = golden("purity_L64")
            dm.prior_rule, dm.prior_weight, dm.prior_ps, dm.n_sample = 2, 1.0, pcfg["prior_ps"], p["n_sample"].tolist()
        elif variant == "known":
            g = torch.Generator().manual_seed(3)
            known = torch.zeros(Lq, dtype=torch.bool)
            known[:16] = True
            more = dict(content_token=torch.randint(0, K, (NB, Lq), generator=g).cuda(), known_mask=known)
            call, plain = (lambda **m: sample(dm, cond, cf, **kw, **more, **m)), (lambda **m: sample(dm, cond, cf, **more, **m))
        elif variant == "long":
            def long(extra, **m):
                dm.set_noise(SEED, stream=2)
                out = dm.sample_long(["a"] * NB, None, cond, cf, latent_shape=SHAPE, n_frames=6, overlap=2, **extra, **m)
                assert out["windows"] == 2
                return out["content_token"].cpu()
            call, plain = (lambda **m: long(kw, **m)), (lambda **m: long({}, **m))
        graphed = call()
        assert dm._last_lanes == 2
        eager = call(use_graph=False)
        assert torch.equal(graphed, eager), "captured chain != eager chain"
        assert int(graphed.min()) >= 0 and int(graphed.max()) < K
        assert not torch.equal(plain(), graphed), "the composed conditions change no token"
    finally:
        for n, v in before.items():
            setattr(dm, n, v)


@pytest.mark.parametrize("Te,N", [(1, 2), (1, 3), (1, 4), (3, 4)])
def test_stacked_copies_are_the_single_passes(G, model, Te, N):
    """Text2ImageTransformer.run at rep = N + 1 = 3, 4, 5 (workspace(rep=), and on the fused path, Te = 1, block 0's shared q|k|v and
    the copy of its attention output to every copy) against rep = 1 passes of its own: block i of the stacked logits is the pass on
    condition i alone -- bit for bit on the fused path, within the logit bar on the unfused one (Te = 3, with lengths) -- independently of
    the sampler, which stacks the same way."""
    dm, cfg = model
    cond, cf, kw = chain_inputs(cfg, Te, N)
    tr, Lq, K = dm.transformer, dm.shape, cfg["K"]
    conds = [cond, *kw["compose_embeds"], cf]
    lens = None if Te == 1 else [LENS[i] for i in range(N)] + [[Te] * NB]
    tr.packed(); tr.fragment_images()
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, K, (NB, Lq), generator=g)
    tok[:, ::2] = K
    tok = tok.cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    rep = N + 1
    ws = tr.workspace(rep * NB, Lq, "cuda", rep=rep)
    assert ("qkv0" in ws) and ws["qkv0"].shape[1] == NB * Lq and ws["logits"].shape == (rep * NB * Lq, K)
    t2 = torch.full((rep * NB,), 40, dtype=torch.int64, device="cuda")
    stacked_logits = tr.run(tok, tr.cond_vectors(torch.cat(conds, 0).contiguous()), Te, t2, ws, rep=rep,
                            cond_len=None if lens is None else i32(sum(lens, []))).clone()
    assert int(ws["range"].item()) == 0
    ws1 = tr.workspace(NB, Lq, "cuda")
    differ, worst = [], 0.0
    for i, c in enumerate(conds):
        one = tr.run(tok, tr.cond_vectors(c.contiguous()), Te, t2[:NB].contiguous(), ws1, cond_len=None if lens is None else i32(lens[i]))
        block = stacked_logits[i * NB * Lq:(i + 1) * NB * Lq]
        differ.append(int((one.view(torch.int32) != block.view(torch.int32)).sum()))
        worst = max(worst, float((one - block).abs().max()))
    parity_report(f"compose::stacked_copies[Te{Te}_N{N}]", {"differing_logits_per_block": differ, "max_abs_diff": worst})
    if Te == 1:
        assert differ == [0] * rep, differ
    else:
        # The unfused path's generic GEMM picks its tile by the row count, which a stacked pass multiplies by rep: a sum may run in
        # another order there, so the blocks are held to the project's logit bar (test_gpu_parity.LOGIT_TOL), not to the bit.
        assert worst <= LOGIT_TOL, (worst, differ)
    assert not torch.equal(stacked_logits[:NB * Lq], stacked_logits[NB * Lq:2 * NB * Lq]), "the conditions change no logit"


def test_unit_weight_on_the_caption_is_the_unguided_step(G, model):
    """Weights (1, 0, 0, 0) with cf given: e = x_u + 1 (x_0 - x_u), the caption's own row up to a rounding, so a single step's tokens
    are the unguided step's wherever the unguided posterior's top-two Gumbel gap (fp64, from its post_dbg) is at least GAP_FLOOR."""
    from oracle import philox
    dm, cfg = model
    cond, cf, kw = chain_inputs(cfg, 1, 4)
    tr, Lq, K, Tq = dm.transformer, dm.shape, cfg["K"], dm.num_timesteps
    N = 4
    tr.packed(); tr.fragment_images()
    condv = tr.cond_vectors(torch.cat([cond, *kw["compose_embeds"], cf], 0).contiguous())
    ws = tr.workspace((N + 1) * NB, Lq, "cuda", rep=N + 1)
    g = torch.Generator().manual_seed(8)
    tok = torch.randint(0, K, (NB, Lq), generator=g)
    tok[:, ::2] = K
    tok = tok.cuda()
    t2 = torch.full(((N + 1) * NB,), 40, dtype=torch.int64, device="cuda")
    logits = tr.run(tok, condv, 1, t2, ws, rep=N + 1).clone()
    step = lambda rows, **hook: G.ops.d3pm_step(rows, None, tok, torch.empty_like(tok), dm._sched(), t2, i64([5]), K=K, T=Tq, guidance=1.0,
                                                 seed=SEED, row0=0, **hook).cpu()
    post = torch.empty((NB, K + 1, Lq), device="cuda")
    want = step(logits[:NB * Lq].contiguous(), post_dbg=post)
    w = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(NB, N).contiguous().cuda()
    got = step(G.ops.d3pm_compose(logits, w, n_cond=N, B=NB, L=Lq, K=K))
    u = torch.from_numpy(philox.uniform_bkl(SEED, 5, NB, K + 1, Lq, row0=0))
    top = (-torch.log(-torch.log(u + 1e-30) + 1e-30) + post.cpu().double()).topk(2, 1).values
    ok = (top[:, 0] - top[:, 1]) >= GAP_FLOOR
    left_out = int((~ok).sum())
    parity_report("compose::unit_weight", {"positions": NB * Lq, "left_out": left_out, "mismatches": int(((got != want) & ok).sum()),
                                           "mismatches_anywhere": int((got != want).sum())})
    assert int(((got != want) & ok).sum()) == 0 and left_out <= 0.01 * NB * Lq, left_out


# ----------------------------------------------------------------------------- glue
def test_generator_composes_captions(G, golden):
    """DiscreteDiffusion(sample_compose=[...]) with the hash stand-in text encoder and zero_text_emb=False: sample() gets the embeddings of
    the listed texts and the weights (the caption at guidance_scale), the tokens are those of that call, and they decode."""
    from src.models.text_models.clip_text_embedding import CLIPTextEmbedding
    from tests.test_gpu_glue import build
    gen0, vq, batch, a, cfg, cfgd = build(G, golden, zero_text_emb=False)
    dm = gen0.diffusion_model.eval()
    provider = CLIPTextEmbedding(clip_dim=cfgd["cond_dim"]).cuda()
    entries = [{"text": "blurry, static camera", "weight": -1.0}, {"text": "bright colours", "weight": 0.5}]
    gen = G.DiscreteDiffusion(provider, dm, zero_text_emb=False, sample_compose=entries)
    texts = batch["text"]
    nB = len(texts)
    seen = {}
    real = dm.sample

    def spy(*a_, **kw):
        seen.update(kw)
        return real(*a_, **kw)
    dm.sample = spy
    try:
        dm.set_noise(5, stream=1)
        with torch.no_grad():
            clips = gen.sample_videos(texts, vq)
    finally:
        del dm.sample
    emb = lambda t: gen._text([t] * nB, "cuda")
    assert seen["compose_weights"] == [float(dm.guidance_scale), -1.0, 0.5] and len(seen["compose_embeds"]) == 2
    assert torch.equal(seen["compose_embeds"][0], emb("blurry, static camera")) and torch.equal(seen["compose_embeds"][1], emb("bright colours"))
    tok = gen.last_content_token.cpu()
    assert tuple(clips.shape[:2]) == (nB, 3) and bool(torch.isfinite(clips).all()) and int(tok.max()) < cfgd["K"]
    dm.set_noise(5, stream=1)
    want = dm.sample(texts, None, gen._text(texts, "cuda"), gen._text([""] * nB, "cuda"), filter_ratio=0,
                     compose_embeds=[emb("blurry, static camera"), emb("bright colours")],
                     compose_weights=[float(dm.guidance_scale), -1.0, 0.5])["content_token"].cpu()
    assert torch.equal(tok, want)
    plain = G.DiscreteDiffusion(provider, dm, zero_text_emb=False)
    dm.set_noise(5, stream=1)
    with torch.no_grad():
        plain.sample_videos(texts, vq)
    assert not torch.equal(plain.last_content_token.cpu(), tok), "the composed captions change no token"
