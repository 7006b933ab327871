"""Per-sample condition lengths (caption padding masked in cross-attention) through the denoiser, the sampler, the trainer and the
generator glue, at the smallest model: L = 64, K = 32, two layers, n_embd 64, 16 heads (the trained-like weights of
tests/test_gpu_training_cond_tokens.py::make_model, so that cross-attention is not flat), Te = 22, B = 8 with lengths
[2, 22, 7, 3, 22, 5, 11, 4] -- two sampler lanes of 4.

Denoiser: NaN in every padded condition row gives the bits of zeros there; the mask takes effect (> 1e-3 somewhere against the unmasked
call on zero padding); row b agrees with a B = 1 unmasked call on cond[b, :len[b]] within the project's logit gate of 1e-4 (DESIGN.md
section 2; the achieved difference is recorded, not asserted to be 0: small_linear's bit-stability across row counts is unmeasured).

Sampler (guided, 100 steps): captured = eager trace; two lanes = one lane; NaN padding = zero padding; condition_len None and
condition_len = Te everywhere are the call without the keyword; sample_fast(skip_step=3) and a known_mask run, captured = eager;
a cf_condition_len shorter than Te changes the tokens.

Trainer: loss and gradients against torch.autograd of oracle.d3pm.train_loss with a -inf key mask added to its cross-attention (the
restatement and the bars of tests/test_gpu_training_cond_tokens.py: loss rtol 2e-5, every tensor to 2e-3 of max(its largest entry,
1e-3 of the model's largest gradient)); finite garbage (+-1e3) in the padded condition rows gives torch.equal loss and gradients; with a
drop mask and a learned null embedding the dropped samples are full length and the null gradient is within the same bar; the captured
step reproduces the eager one bit for bit while the lengths change from step to step (at learning rate 0: see the test).  The
bit-for-bit comparisons of gradients run with D3PMTrainer(deterministic=True) on both sides, as tests/test_gpu_cond_dropout.py does and
explains: the fast backward adds workgroup partials with float atomics, and two identical calls differ in their last bits.

Glue: DiscreteDiffusion(mask_text_padding=True) on the byte-level provider of tests/test_gpu_text_tokens.py."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import parity_report
from tests.test_gpu_training_cond_tokens import K, NOISE_SEED, T, make_model

pytestmark = pytest.mark.gpu

B, L, Te, SPATIAL = 8, 64, 22, (8, 8)
LENS = [2, 22, 7, 3, 22, 5, 11, 4]
TVALS = (0, 61, 37, 99, 5, 80, 12, 50)
DROP = (True, False, True, False, False, True, False, False)


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def bits(x):
    return x.contiguous().view(torch.int32)


def inputs():
    g = torch.Generator().manual_seed(1000 * L + Te + 3)
    return torch.randint(0, K, (B, L), generator=g), torch.randn(B, Te, 512, generator=g), torch.randn(B, Te, 512, generator=g)


def pad(cond, lens, value):
    """cond with the rows at and behind every sample's length filled with `value` (a number, or a tensor of cond's shape)"""
    out = cond.clone()
    for b, n in enumerate(lens):
        out[b, n:] = value if not torch.is_tensor(value) else value[b, n:]
    return out


# ----------------------------------------------------------------------------- denoiser
def test_denoiser_never_reads_the_padding(G):
    tok, cond, _ = inputs()
    tr = make_model(SPATIAL)[0].cuda().eval().transformer
    tok, t = tok.cuda(), torch.tensor(TVALS).cuda()
    lens = torch.tensor(LENS)
    zero, nan = pad(cond, LENS, 0.0).cuda(), pad(cond, LENS, float("nan")).cuda()
    masked = tr.forward(tok, zero, t, lens).clone()
    masked_nan = tr.forward(tok, nan, t, lens).clone()
    unmasked = tr.forward(tok, zero, t).clone()
    assert bool(torch.isfinite(masked).all())
    assert torch.equal(bits(masked), bits(masked_nan)), "the padded condition rows are read"
    effect = float((masked - unmasked).abs().max())
    assert effect > 1e-3, f"the mask has no effect on the logits: {effect}"
    worst = 0.0
    for b, n in enumerate(LENS):
        if n == 1:
            continue
        one = tr.forward(tok[b:b + 1], cond[b:b + 1, :n].cuda().contiguous(), t[b:b + 1])
        worst = max(worst, float((one[0] - masked[b]).abs().max()))
    parity_report("condition_len::denoiser", {"row_vs_truncated_B1_max_abs": worst, "mask_effect_max_abs": effect, "gate": 1e-4})
    assert worst <= 1e-4, worst
    # full lengths are the call without lengths; lengths are validated on the host; one token takes all-ones only
    full = tr.forward(tok, zero, t, torch.full((B,), Te))
    assert torch.equal(bits(full), bits(unmasked))
    with pytest.raises(G.GsddError, match=r"cond_len\[1\] = 23"):
        tr.forward(tok, zero, t, [2, 23, 7, 3, 22, 5, 11, 4])
    one_tok = zero[:, :1].contiguous()
    assert torch.equal(bits(tr.forward(tok, one_tok, t, torch.ones(B, dtype=torch.long))), bits(tr.forward(tok, one_tok, t)))
    with pytest.raises(G.GsddError):
        tr.forward(tok, one_tok, t, lens)


# ----------------------------------------------------------------------------- sampler
@pytest.fixture(scope="module")
def sampler(G):
    """-> call(kind, cond, cf, **kw) -> tokens (CPU) of a guided chain from the same noise; kind 'sample' / 'fast' / 'known'"""
    dm = make_model(SPATIAL)[0].cuda().eval()
    tok, _, _ = inputs()
    known = torch.zeros(L, dtype=torch.bool)
    known[:16] = True

    def call(kind, cond, cf, **kw):
        dm.set_noise(NOISE_SEED, stream=2)
        texts = ["a"] * B
        if kind == "sample":
            out = dm.sample(texts, None, cond, cf, filter_ratio=0, **kw)
        elif kind == "fast":
            out = dm.sample_fast(texts, None, cond, filter_ratio=0, skip_step=3, cf_condition_embed=cf, **kw)
        else:
            out = dm.sample(texts, None, cond, cf, content_token=tok.cuda(), filter_ratio=0, known_mask=known, **kw)
        return out["content_token"].cpu()
    call.dm = dm
    return call


def test_sampler_with_lengths(G, sampler):
    _, cond, cf = inputs()
    zero, nan, cf = pad(cond, LENS, 0.0).cuda(), pad(cond, LENS, float("nan")).cuda(), cf.cuda()
    lens = torch.tensor(LENS)
    captured = sampler("sample", zero, cf, condition_len=lens)
    assert sampler.dm._last_lanes == 2 and not sampler.dm._last_cfg_dedupe
    trace = []
    eager = sampler("sample", zero, cf, condition_len=lens, trace=trace)
    assert len(trace) == T and int(captured.min()) >= 0 and int(captured.max()) < K
    assert torch.equal(captured, eager), "captured chain != eager trace"
    assert torch.equal(sampler("sample", zero, cf, condition_len=lens, lanes=1), captured), "two lanes != one lane"
    assert sampler.dm._last_lanes == 1
    assert torch.equal(sampler("sample", nan, cf, condition_len=lens), captured), "NaN padding != zero padding"
    assert torch.equal(sampler("sample", nan, cf, condition_len=LENS, use_graph=False), captured)
    plain = sampler("sample", zero, cf)
    assert not torch.equal(plain, captured), "the lengths change no token"
    parity_report("condition_len::sampler", {"tokens_changed_by_the_mask": int((plain != captured).sum()), "tokens": int(plain.numel())})


def test_sampler_without_lengths_is_todays_call(G, sampler):
    _, cond, cf = inputs()
    cond, cf = cond.cuda(), cf.cuda()
    today = sampler("sample", cond, cf)
    assert torch.equal(sampler("sample", cond, cf, condition_len=None, cf_condition_len=None), today)
    assert torch.equal(sampler("sample", cond, cf, condition_len=torch.full((B,), Te)), today)
    assert torch.equal(sampler("sample", cond, cf, condition_len=[Te] * B, cf_condition_len=[Te] * B, use_graph=False), today)
    # the unconditional copy's lengths are honoured; equal conditions with different lengths are not deduplicated
    short = sampler("sample", cond, cf, cf_condition_len=[3] * B)
    assert not torch.equal(short, today), "cf_condition_len changes no token"
    assert torch.equal(sampler("sample", cond, cf, cf_condition_len=[3] * B, use_graph=False), short)
    same = sampler("sample", cond, cond)
    assert sampler.dm._last_cfg_dedupe
    assert torch.equal(sampler("sample", cond, cond, condition_len=[Te] * B), same) and sampler.dm._last_cfg_dedupe
    sampler("sample", cond, cond, condition_len=LENS)
    assert not sampler.dm._last_cfg_dedupe
    for bad in ([0] + LENS[1:], LENS[:-1], [float(v) for v in LENS]):
        with pytest.raises(G.GsddError, match="condition_len"):
            sampler("sample", cond, cf, condition_len=bad)


@pytest.mark.parametrize("kind", ["fast", "known"])
def test_other_programs_take_lengths(G, sampler, kind):
    _, cond, cf = inputs()
    zero, nan, cf = pad(cond, LENS, 0.0).cuda(), pad(cond, LENS, float("nan")).cuda(), cf.cuda()
    captured = sampler(kind, nan, cf, condition_len=LENS)
    eager = sampler(kind, zero, cf, condition_len=LENS, use_graph=False)
    assert torch.equal(captured, eager)
    assert not torch.equal(sampler(kind, zero, cf), captured)


def test_p_sample_tokens_takes_lengths(G, sampler):
    tok, cond, cf = inputs()
    dm = sampler.dm
    dm.set_noise(NOISE_SEED, stream=2)
    t = torch.full((B,), 40).cuda()
    zero, nan = pad(cond, LENS, 0.0).cuda(), pad(cond, LENS, float("nan")).cuda()
    a = dm.p_sample_tokens(tok.cuda(), zero, cf.cuda(), t, 5, condition_len=LENS)
    b = dm.p_sample_tokens(tok.cuda(), nan, cf.cuda(), t, 5, condition_len=LENS)
    assert torch.equal(a, b) and int(a.max()) <= K


# ----------------------------------------------------------------------------- trainer
def masked_oracle(sd, x0, cond, lens, t, pt, null=None, drop=None):
    """torch.autograd of oracle.d3pm.train_loss with a -inf key mask on its cross-attention (attn2): sample b attends to keys
    < lens[b]; a dropped sample takes the null rows and all Te keys.  -> (loss, transformer gradients, gradient of the null rows)"""
    from oracle import d3pm as od
    lens = torch.as_tensor(lens)
    if drop is not None:
        cond = torch.where(drop[:, None, None], null[None], cond)
        lens = torch.where(drop, torch.full_like(lens, cond.shape[1]), lens)
    dead = torch.arange(cond.shape[1])[None, :] >= lens[:, None]                   # (B, Te)
    plain = od.mha

    def mha(xq, xkv, sd_, p, n_head):
        if not p.endswith("attn2."):
            return plain(xq, xkv, sd_, p, n_head)
        Bq, Tq, C = xq.shape
        hs = C // n_head
        k = F.linear(xkv, sd_[p + "key.weight"], sd_[p + "key.bias"]).view(Bq, -1, n_head, hs).transpose(1, 2)
        q = F.linear(xq, sd_[p + "query.weight"], sd_[p + "query.bias"]).view(Bq, Tq, n_head, hs).transpose(1, 2)
        v = F.linear(xkv, sd_[p + "value.weight"], sd_[p + "value.bias"]).view(Bq, -1, n_head, hs).transpose(1, 2)
        s = (q @ k.transpose(-2, -1)) * (1.0 / hs ** 0.5)
        att = F.softmax(s.masked_fill(dead[:, None, None, :], float("-inf")), dim=-1)
        y = (att @ v).transpose(1, 2).contiguous().view(Bq, Tq, C)
        return F.linear(y, sd_[p + "proj.weight"], sd_[p + "proj.bias"])
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith("transformer.") and v.dtype.is_floating_point else v) for k, v in sd.items()}
    od.mha = mha
    try:
        loss, _, _, _ = od.train_loss(x0, cond, t, pt, leaf, NOISE_SEED, 0)
    finally:
        od.mha = plain
    loss.backward()
    grads = {k[len("transformer."):]: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()
             if k.startswith("transformer.") and v.dtype.is_floating_point}
    return loss.item(), grads, (None if null is None else null.grad.detach().clone())


def train_args():
    return torch.tensor(TVALS, dtype=torch.long), torch.ones(B) / T


def compare(got, want, gmax):
    return {k: (got[k].cpu() - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax) for k, w in want.items()}


def test_gradients_match_autograd_with_a_key_mask(G):
    from gsdd_amd.d3pm_train import D3PMTrainer
    x0, cond, _ = inputs()
    t, pt = train_args()
    dm, sd = make_model(SPATIAL)
    want_loss, want, _ = masked_oracle(sd, x0, cond, LENS, t, pt)                  # (CPU, before any device call)
    loss_unmasked, _, _ = masked_oracle(sd, x0, cond, [Te] * B, t, pt)
    assert abs(loss_unmasked - want_loss) > 1e-4 * abs(want_loss), "the mask does not move the loss: the check would see nothing"
    gmax = max(w.abs().max().item() for w in want.values())
    dm = dm.cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm)
    loss, got = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=t.cuda(), pt=pt.cuda(), cond_len=torch.tensor(LENS))
    errs = compare(got, want, gmax)
    worst = max(errs, key=errs.get)
    rec = {"worst_relative_error": errs[worst], "worst_parameter": worst, "loss": loss.item(), "oracle_loss": want_loss,
           "oracle_loss_unmasked": loss_unmasked, "worst_ratio": errs[worst] / 2e-3}
    print(rec)
    parity_report("condition_len::training", rec)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=2e-5)
    assert set(got) == set(want)
    for k, e in errs.items():
        assert e < 2e-3, f"{k}: relative max error {e:.3e}"


def test_finite_garbage_in_the_padding_changes_nothing(G):
    """+-1e3 in the padded condition rows: torch.equal loss and gradients (both calls with the reproducible reductions); a condition
    that comes on the host with inf / NaN in it is refused."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    x0, cond, other = inputs()
    t, pt = train_args()
    garbage = pad(cond, LENS, 1e3 * torch.sign(other))
    runs = []
    for c in (pad(cond, LENS, 0.0), garbage):
        dm = make_model(SPATIAL)[0].cuda()
        dm.set_noise(NOISE_SEED, stream=0)
        loss, g = D3PMTrainer(dm, deterministic=True).loss_and_grads(x0.cuda(), c.cuda(), t=t.cuda(), pt=pt.cuda(), cond_len=LENS)
        runs.append((loss.clone(), {k: v.clone() for k, v in g.items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k
    with pytest.raises(G.GsddError, match="finite"):
        D3PMTrainer(dm).loss_and_grads(x0.cuda(), pad(cond, LENS, float("nan")), t=t.cuda(), pt=pt.cuda(), cond_len=LENS)


def test_dropped_samples_are_full_length(G):
    from gsdd_amd.d3pm_train import D3PMTrainer
    x0, cond, _ = inputs()
    t, pt = train_args()
    drop = torch.tensor(DROP)
    dm, sd = make_model(SPATIAL)
    dm.learnable_cf = True
    dm.empty_text_embed.data = torch.randn(77, 512, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    null = dm.empty_text_embed.detach()[:Te].float().clone().requires_grad_(True)
    want_loss, want, want_null = masked_oracle(sd, x0, cond, LENS, t, pt, null=null, drop=drop)
    gmax = max(w.abs().max().item() for w in want.values())
    assert want_null.abs().max().item() > 1e-3 * gmax, "the bar would not see the null gradient"
    dm = dm.cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm)
    loss, got = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=t.cuda(), pt=pt.cuda(), drop=drop.cuda(), cond_len=LENS)
    assert torch.equal(tr.last_drop.cpu().bool(), drop)
    errs = compare(got, want, gmax)
    gn = got["empty_text_embed"]
    errs["empty_text_embed"] = (gn[:Te].cpu() - want_null).abs().max().item() / max(want_null.abs().max().item(), 1e-3 * gmax)
    worst = max(errs, key=errs.get)
    rec = {"worst_relative_error": errs[worst], "worst_parameter": worst, "null_relative_error": errs["empty_text_embed"],
           "loss": loss.item(), "oracle_loss": want_loss, "worst_ratio": errs[worst] / 2e-3}
    print(rec)
    parity_report("condition_len::training_dropout", rec)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=2e-5)
    for k, e in errs.items():
        assert e < 2e-3, f"{k}: relative max error {e:.3e}"
    assert not bool(gn[Te:].any())


def test_captured_step_refreshes_the_lengths(G, monkeypatch):
    """Four steps whose lengths differ from step to step (two eager ones, the capture's replay, one more replay) against the same
    steps launch by launch: every loss, Adam's first and second moments (which accumulate every step's gradients) and the parameters
    bit for bit, both modes with the reproducible reductions.
    The learning rate is 0, so that every step starts from the same parameters in both modes and what is compared is the step -- q_sample,
    forward, loss, backward, the moments.  With a learning rate the two modes part after the first replay for a reason that has nothing
    to do with lengths: the launch-by-launch Adam evaluates its bias corrections 1 - beta^step on the host in f32 (powf), the captured
    one on the device in f64 (the step count is a device word there), so the updates differ in their last bits.  Measured with lr = 1e-3:
    losses 1 to 3 bit-equal (3 is the first replay), loss 4 = 5.4899 five ulps apart (bits 1085255017 / 1085255022)."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    g = torch.Generator().manual_seed(43)
    batches = [(torch.randint(0, K, (B, L), generator=g).cuda(), torch.randn(B, Te, 512, generator=g).cuda(),
                torch.randint(0, T, (B,), generator=g).cuda(), torch.full((B,), 1.0 / T).cuda(),
                torch.randint(1, Te + 1, (B,), generator=g)) for _ in range(4)]
    assert not torch.equal(batches[2][4], batches[3][4])
    runs = {}
    for mode in ("0", "1", "stale"):
        monkeypatch.setenv("GSDD_TRAIN_GRAPH", "0" if mode == "stale" else mode)
        dm = make_model(SPATIAL)[0].cuda().train()
        start = {k: v.detach().cpu().clone() for k, v in dm.transformer.state_dict().items()}
        dm.set_noise(NOISE_SEED, stream=3)
        tr = D3PMTrainer(dm, lr=0.0, deterministic=True)
        # ("stale": the last step with the lengths of the step before it -- what a buffer that is not refreshed would compute)
        losses = [tr.step(x0, cond, t=t, pt=pt, cond_len=batches[2][4] if (mode == "stale" and i == 3) else n).cpu()
                  for i, (x0, cond, t, pt, n) in enumerate(batches)]
        took_graph = getattr(tr, "_graph", None) is not None
        opt = tr.optimizer_state()
        runs[mode] = (losses, {k: v.detach().cpu() for k, v in dm.transformer.state_dict().items()}, opt["m"].detach().cpu().clone(),
                      opt["v"].detach().cpu().clone())
        # the captured graph is released before any comparison (a CUDAGraph freed by the cyclic collector during a
        # later test's stream capture aborts the process)
        del tr, dm, opt
        gc.collect()
        torch.cuda.synchronize()
        assert took_graph == (mode == "1"), "the step with lengths did not take the graph path"
    eager, captured, stale = runs["0"], runs["1"], runs["stale"]
    parity_report("condition_len::captured", {"losses": [float(v[0]) for v in captured[0]], "eager_losses": [float(v[0]) for v in eager[0]],
                                              "stale_last_loss": float(stale[0][3][0])})
    assert not torch.equal(bits(stale[0][3]), bits(eager[0][3])), "the lengths of the last step do not move its loss: the check sees nothing"
    for a, b in zip(eager[0], captured[0]):
        assert torch.equal(bits(a), bits(b)), (eager[0], captured[0])
    assert torch.equal(bits(eager[2]), bits(captured[2])) and torch.equal(bits(eager[3]), bits(captured[3])), "Adam's moments differ"
    assert bool(eager[2].any()) and not torch.equal(bits(stale[2]), bits(eager[2]))
    for k, w in eager[1].items():
        assert torch.equal(bits(w), bits(captured[1][k])) and torch.equal(bits(w), bits(start[k])), k


# ----------------------------------------------------------------------------- glue
def test_generator_masks_text_padding(G, tmp_path, golden):
    from tests.test_gpu_glue import build, pin_time
    from tests.test_gpu_text_tokens import byte_level_provider
    gen0, vq, batch, a, cfg, cfgd = build(G, golden, zero_text_emb=False)
    C = cfgd["cond_dim"]
    provider = byte_level_provider(tmp_path, C, C // 16, per_token=True).cuda()
    texts = ["a", "a b c d e f g h"]
    batch = dict(batch, video=batch["video"][:2].contiguous(), text=texts)
    dm = gen0.diffusion_model.eval()
    emb, lens = provider(texts, return_lengths=True)
    assert lens.tolist() == [3, 10] and tuple(emb.shape) == (2, 22, C)
    masked = G.DiscreteDiffusion(provider, dm, zero_text_emb=False, mask_text_padding=True)
    plain = G.DiscreteDiffusion(provider, dm, zero_text_emb=False)
    t_fix = torch.tensor([37, 80]).cuda()
    dm.sample_time = lambda b, device, method="uniform": (t_fix, torch.ones(b, device="cuda") / cfgd["T"])

    def run(gen, **kw):
        dm.set_noise(5, stream=0)
        with torch.no_grad():
            if kw:
                gen.sample_videos(texts, vq, **kw)
                return None, gen.last_content_token.cpu()
            out = gen(batch, vq, None, do_inference=True)
            return out["losses"].clone(), gen.last_content_token.cpu()
    loss_m, tok_m = run(masked)
    loss_p, tok_p = run(plain)
    assert bool(torch.isfinite(loss_m)) and tuple(tok_m.shape) == (2, 64)
    # the objective saw the lengths: the same forward with the provider's own outputs handed to the diffusion model
    quant = vq.encode(batch["video"]).view(2, -1)
    for want, extra in ((loss_m, {"condition_len": lens}), (loss_p, {})):
        dm.set_noise(5, stream=0)
        with torch.no_grad():
            got = dm({"condition_embed_token": emb, "content_token": quant, **extra}, return_loss=True, return_logits=False)["loss"]
        assert torch.equal(bits(got), bits(want))
    # sample_videos(text_emb, text_len) with the provider's outputs; the sampler of forward(do_inference=True) drew after one objective
    dm.set_noise(5, stream=1)
    with torch.no_grad():
        masked.sample_videos(texts, vq, text_emb=emb, text_len=lens)
    assert torch.equal(masked.last_content_token.cpu(), tok_m)
    dm.set_noise(5, stream=1)
    with torch.no_grad():
        plain.sample_videos(texts, vq, text_emb=emb)
    assert torch.equal(plain.last_content_token.cpu(), tok_p), "mask_text_padding=False is not today's output"
    dm.set_noise(5, stream=1)
    with torch.no_grad():
        plain.sample_videos(texts, vq)
    assert torch.equal(plain.last_content_token.cpu(), tok_p)
    # the training forward with autograd takes the lengths through the bridge
    dm.train()
    dm.set_noise(5, stream=0)
    out = masked(batch, vq, None, do_inference=False)
    out["losses"].backward()
    assert bool(torch.isfinite(out["losses"])) and all(bool(torch.isfinite(p.grad).all()) for p in dm.transformer.parameters())
    zeroed = G.DiscreteDiffusion(provider, dm, zero_text_emb=True, mask_text_padding=True)
    assert zeroed._text(texts, "cuda", return_lengths=True)[1] is None
    parity_report("condition_len::glue", {"tokens_changed_by_the_mask": int((tok_m != tok_p).sum()), "loss_masked": float(loss_m),
                                          "loss_plain": float(loss_p)})
