"""Classifier-free training on the MI355X: condition dropout (gsdd_cond_dropout), the gradient of the learned null embedding
(gsdd_cond_null_grad), and both through D3PMTrainer (eager, captured), the autograd bridge and the sampler.

Kernels.  The drop flags equal the numpy restatement of the Philox rule (gsdd_amd.cond_drop_rows, itself pinned to oracle/philox.py in
tests/test_cond_dropout_host.py) and every output row is bit-equal to its source or to the null row.  The null gradient is held, element
by element, to (B + 2 D + 4) 2^-24 (sum |terms| + |dnull_in|) against fp64: the kernel adds B samples, then D products for the keys and D
for the values, one add joins them and one adds onto dnull; each rounds by at most 2^-24 of a partial sum that the sum of absolute terms
bounds.

Whole model.  Model, weights and bar of tests/test_gpu_training_cond_tokens.py (two layers, K = 32; the loss to rtol 2e-5, every tensor
to 2e-3 of max(its own largest entry, 1e-3 of the model's largest gradient)), B = 4, t = (0, 61, 37, 99), mask [T, F, T, F],
learnable_cf.  Reference: torch.autograd through oracle.d3pm.train_loss on where(drop, null, cond) with the null rows as a leaf.
Precondition, on the CPU before any device call: the null gradient's largest entry exceeds 1e-3 of the model's largest gradient
(below that the bar would not see it); on the oracle the ratio is 0.019 ... 0.080 over the cases.

Bit-equality of gradients.  The issue sets: the loss and every transformer gradient of the masked call are bit-equal to a plain call on
the pre-substituted condition, and a call that drops nothing is today's call bit for bit.  In the backward's fast form that cannot be
observed: gsdd_wgrad, gsdd_ln_bwd, gsdd_colsum, gsdd_batch_rowsum, gsdd_d3pm_embed_bwd and gsdd_adaln_bwd add workgroup partials with
float atomics, and two IDENTICAL plain calls on fresh models differ in 19 ... 40 of the 63 gradient tensors by up to 2.2e-7 of the
tensor's scale (masked against substituted: 13 ... 32 of 63, up to 3.1e-7; the losses are bit-equal).  Those comparisons therefore run
with D3PMTrainer(deterministic=True) on both sides -- the reductions' reproducible form (gsdd_set_deterministic: one workgroup per output
address, fixed order), in which a difference between the two calls can only come from what they compute -- and
test_deterministic_backward holds that form to the oracle's bar and to bit-equality between two identical calls.  In the fast form the
same noise reaches test_captured_step_equals_the_eager_steps through Adam, which turns the noise of a near-zero gradient entry into a
visible update (two EAGER runs of its three steps were seen 4.0e-5 apart in one entry of blocks.1.ln1_1.emb.weight against atol 2e-6, all
else within the tolerances); that test runs both modes with deterministic=True as well, so that what it compares is the captured graph
against the launches and not two draws of the noise.

A mask without a dropped sample keeps "empty_text_embed" in the gradient dict, all zeros (the decision is device data: the host does not
read it); with cond_drop_prob = 0 and no mask the key is absent and the call is today's, bit for bit."""
import functools
import gc

import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_training_cond_tokens import K, NOISE_SEED, T, make_model

pytestmark = pytest.mark.gpu

B = 4
TVALS = (0, 61, 37, 99)
MASK = (True, False, True, False)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def bits(x):
    return x.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- 1. the dropout kernel
@pytest.mark.parametrize("shape", [(37, 22, 512, 1000), (5, 77, 512, 0), (1, 1, 4, 2 ** 33 + 5), (3, 3, 20, 7)], ids=str)
def test_dropout_kernel(G, shape):
    Bk, Te, C, row0 = shape
    g = torch.Generator().manual_seed(Bk * 1000 + Te)
    cond, null = torch.randn(Bk, Te, C, generator=g).cuda(), torch.randn(Te, C, generator=g).cuda()
    stream = 3
    sid = torch.tensor([stream], dtype=torch.int64, device="cuda")
    for seed in (NOISE_SEED, (5 << 32) | 77):
        for p in (0.0, 0.1, 0.5, 1.0):
            out, flags = G.ops.cond_dropout(cond, null, p, seed=seed, sid=sid, row0=row0)
            want = G.cond_drop_rows(seed, stream, Bk, row0, p)
            assert np.array_equal(flags.cpu().numpy().astype(bool), want), (seed, p)
            src = torch.where(torch.from_numpy(want).cuda()[:, None, None], null[None], cond)
            assert torch.equal(bits(out), bits(src)), (seed, p)
    mask = torch.rand(Bk, generator=g) < 0.5
    if Bk > 1:
        mask[0], mask[1] = True, False
    for m in (mask, mask.to(torch.uint8)):
        out, flags = G.ops.cond_dropout(cond, null, 0.0, seed=NOISE_SEED, sid=None, row0=row0, drop=m.cuda())
        assert torch.equal(flags.cpu().bool(), mask)                              # the mask is obeyed (p = 0 would drop nothing) and echoed
        assert torch.equal(bits(out), bits(torch.where(mask.cuda()[:, None, None], null[None], cond)))
    with pytest.raises(G.GsddError):
        G.ops.cond_dropout(cond, null, 0.1, seed=NOISE_SEED, sid=sid, row0=row0, out=cond)           # out == cond: nothing launched


def test_dropout_counts(G):
    cond, null = torch.zeros(8192, 1, 4).cuda(), torch.ones(1, 4).cuda()
    sid = torch.tensor([3], dtype=torch.int64, device="cuda")
    counts = {}
    for p in (0.1, 0.5):
        out, flags = G.ops.cond_dropout(cond, null, p, seed=NOISE_SEED, sid=sid, row0=1000)
        counts[p] = int(flags.sum())
        assert int(out[:, 0, 0].sum()) == counts[p]
    parity_report("cond_dropout::counts_8192", {"p0.1": counts[0.1], "p0.5": counts[0.5]})
    assert counts == {0.1: 839, 0.5: 4034}


# ----------------------------------------------------------------------------- 2. the null-gradient kernel against fp64
@pytest.mark.parametrize("shape", [(1, 1, 64, 512), (5, 3, 64, 512), (16, 22, 64, 512), (4, 77, 64, 512), (3, 2, 8, 20)], ids=str)
def test_null_grad_kernel(G, shape):
    Bk, Te, D, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    dk, dv = torch.randn(Bk, Te, D, generator=g), torch.randn(Bk, Te, D, generator=g)
    wk, wv = torch.randn(D, C, generator=g) / D ** 0.5, torch.randn(D, C, generator=g) / D ** 0.5
    dnull0 = torch.randn(Te, C, generator=g)
    mixed = torch.arange(Bk) % 2 == 0
    worst = 0.0
    for name, mask in (("none", torch.zeros(Bk, dtype=torch.bool)), ("all", torch.ones(Bk, dtype=torch.bool)), ("mixed", mixed)):
        for keys in (True, False):
            m = mask.double()[:, None, None]
            want = dnull0.double() + (dv.double() * m).sum(0) @ wv.double()
            mag = dnull0.double().abs() + (dv.double().abs() * m).sum(0) @ wv.double().abs()
            if keys:
                want = want + (dk.double() * m).sum(0) @ wk.double()
                mag = mag + (dk.double().abs() * m).sum(0) @ wk.double().abs()
            bar = (Bk + 2 * D + 4) * U * mag
            runs = []
            for _ in range(2):
                dnull = dnull0.clone().cuda()
                G.ops.cond_null_grad(dk.cuda() if keys else None, dv.cuda(), mask.to(torch.uint8).cuda(), wk.cuda() if keys else None,
                                     wv.cuda(), Bk, Te, dnull)
                runs.append(dnull.cpu())
            assert torch.equal(bits(runs[0]), bits(runs[1])), (name, keys)                      # no atomics, a fixed order
            if not mask.any():
                assert torch.equal(bits(runs[0]), bits(dnull0)), (name, keys)                   # nothing dropped: dnull keeps its bits
            err = (runs[0].double() - want).abs()
            ratio = float((err / bar).max())
            worst = max(worst, ratio)
            print(f"null_grad {shape} mask={name} keys={keys}: worst error / bar {ratio:.3f}, max |error| {float(err.max()):.3e}")
            assert bool((err <= bar).all()), f"{shape} mask={name} keys={keys}: worst error / bar {ratio:.3f}"
    parity_report(f"cond_null_grad::B{Bk}_Te{Te}_D{D}_C{C}", {"worst_error_over_bar": worst})


# ----------------------------------------------------------------------------- the whole model
def build(spatial):
    """the model of tests/test_gpu_training_cond_tokens.py with learnable_cf and a seeded null embedding (CPU)"""
    dm, sd = make_model(spatial)
    dm.learnable_cf = True
    dm.empty_text_embed.data = torch.randn(77, 512, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    sd["empty_text_embed"] = dm.empty_text_embed.detach().clone()
    return dm, sd


def batch4(L, Te):
    g = torch.Generator().manual_seed(1000 * L + Te + 7)
    return torch.randint(0, K, (B, L), generator=g), torch.randn(B, Te, 512, generator=g)


def args4():
    return torch.tensor(TVALS, dtype=torch.long), torch.ones(B) / T, torch.tensor(MASK)


@functools.lru_cache(maxsize=None)
def oracle_case(spatial, Te):
    """(loss, transformer gradients by name, gradient of the null rows (Te, 512)): torch.autograd of the oracle on where(drop, null, cond);
    CPU only, computed once per case and left unchanged"""
    from oracle import d3pm as od
    _, sd = build(spatial)
    x0, cond = batch4(spatial[0] * spatial[1], Te)
    t, pt, mask = args4()
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith("transformer.") and v.dtype.is_floating_point else v) for k, v in sd.items()}
    null = sd["empty_text_embed"][:Te].float().requires_grad_(True)
    loss, _, _, _ = od.train_loss(x0, torch.where(mask[:, None, None], null[None], cond), t, pt, leaf, NOISE_SEED, 0)
    loss.backward()
    grads = {k[len("transformer."):]: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()
             if k.startswith("transformer.") and v.dtype.is_floating_point}
    return loss.item(), grads, null.grad.detach().clone()


def precondition(spatial, Te):
    """CPU, before any device call: the bar must be able to see the null gradient"""
    want_loss, want, want_null = oracle_case(spatial, Te)
    gmax = max(w.abs().max().item() for w in want.values())
    ratio = want_null.abs().max().item() / gmax
    assert ratio > 1e-3, f"the null gradient is {ratio:.2e} of the model's largest gradient: the bar would not see it"
    return want_loss, want, want_null, gmax, ratio


def masked_call(G, spatial, Te, deterministic=False):
    """-> (trainer, loss, cloned gradient dict) of loss_and_grads with the mask on a fresh model"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    x0, cond = batch4(spatial[0] * spatial[1], Te)
    t, pt, mask = args4()
    dm = build(spatial)[0].cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm, deterministic=deterministic)
    loss, got = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=t.cuda(), pt=pt.cuda(), drop=mask.cuda())
    return tr, loss.clone(), {k: v.clone() for k, v in got.items()}


@pytest.mark.parametrize("Te", [1, 3, 22])
@pytest.mark.parametrize("spatial", [(12, 8), (8, 5)], ids=["L96", "L40"])
def test_model_gradients_match_autograd_of_oracle(G, spatial, Te):
    from gsdd_amd.d3pm_train import D3PMTrainer
    want_loss, want, want_null, gmax, ratio = precondition(spatial, Te)              # (CPU, before any device call)
    L = spatial[0] * spatial[1]
    tr, loss, got = masked_call(G, spatial, Te)
    assert torch.equal(tr.last_drop.cpu().bool(), torch.tensor(MASK))
    gn = got["empty_text_embed"]
    assert tuple(gn.shape) == (77, 512) and gn.dtype == torch.float32
    errs = {k: (got[k].cpu() - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax) for k, w in want.items() if k in got}
    errs["empty_text_embed"] = (gn[:Te].cpu() - want_null).abs().max().item() / max(want_null.abs().max().item(), 1e-3 * gmax)
    worst = max(errs, key=errs.get)
    rec = {"worst_relative_error": errs[worst], "worst_parameter": worst, "null_relative_error": errs["empty_text_embed"],
           "null_over_largest_gradient": ratio, "loss": loss.item(), "oracle_loss": want_loss, "worst_ratio": errs[worst] / 2e-3}
    print(rec)
    parity_report(f"cond_dropout_model::L{L}_Te{Te}", rec)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=2e-5)
    assert set(got) == set(want) | {"empty_text_embed"}, set(got) ^ set(want)
    for k, e in errs.items():
        assert e < 2e-3, f"{k}: relative max error {e:.3e}"
    assert not bool(gn[Te:].any()), "rows >= Te of the null gradient must be exactly zero"



def bit_differences(a, b):
    """(number of tensors of `a` that differ in bits from `b`'s, the worst difference relative to the tensor's scale, its name)"""
    gmax = max(v.abs().max().item() for v in a.values())
    n, worst, name = 0, 0.0, ""
    for k, v in a.items():
        if not torch.equal(bits(v), bits(b[k])):
            n += 1
            e = (v - b[k]).abs().max().item() / max(v.abs().max().item(), 1e-3 * gmax)
            worst, name = (e, k) if e >= worst else (worst, name)
    return n, worst, name


@pytest.mark.parametrize("Te", [1, 3, 22])
@pytest.mark.parametrize("spatial", [(12, 8), (8, 5)], ids=["L96", "L40"])
def test_masked_call_is_the_plain_call_on_the_substituted_condition(G, spatial, Te):
    """the loss and every transformer gradient bit-equal, as the issue sets it; both calls with the backward's reductions in their
    reproducible form (see the module docstring)"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    L = spatial[0] * spatial[1]
    _, loss, got = masked_call(G, spatial, Te, deterministic=True)
    x0, cond = batch4(L, Te)
    t, pt, mask = args4()
    dm = build(spatial)[0].cuda()
    sub = torch.where(mask[:, None, None], dm.empty_text_embed.detach()[:Te].float().cpu()[None], cond)
    dm.set_noise(NOISE_SEED, stream=0)
    loss_p, plain = D3PMTrainer(dm, deterministic=True).loss_and_grads(x0.cuda(), sub.cuda(), t=t.cuda(), pt=pt.cuda())
    n, worst, name = bit_differences(plain, got)
    rec = {"loss_bit_equal": bool(torch.equal(bits(loss_p), bits(loss))), "gradient_tensors_differing": n, "gradient_tensors": len(plain),
           "worst_relative_difference": worst, "worst_parameter": name}
    print(rec)
    parity_report(f"cond_dropout_substituted::L{L}_Te{Te}", rec)
    assert "empty_text_embed" not in plain and torch.equal(bits(loss_p), bits(loss))
    for k, v in plain.items():
        assert torch.equal(bits(v), bits(got[k])), k


def test_no_dropped_sample_is_todays_call(G):
    """an all-False mask and cond_drop_prob = 0 against the call without the feature: the loss and every transformer gradient bit-equal,
    as the issue sets it; every call with the backward's reductions in their reproducible form (see the module docstring)"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial, Te = (12, 8), 3
    x0, cond = batch4(96, Te)
    t, pt, _ = args4()

    def call(learnable, **kw):
        dm = build(spatial)[0].cuda()
        dm.learnable_cf = learnable
        dm.set_noise(NOISE_SEED, stream=0)
        tr = D3PMTrainer(dm, deterministic=True)
        loss, g = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=t.cuda(), pt=pt.cuda(), **kw)
        return tr, loss.clone(), {k: v.clone() for k, v in g.items()}, dm
    _, loss0, today, _ = call(False)
    tr1, loss1, p0, dm1 = call(True)                                       # learnable_cf alone changes nothing: cond_drop_prob is 0
    assert dm1.cond_drop_prob == 0.0 and tr1.last_drop is None and "empty_text_embed" not in p0 and set(p0) == set(today)
    tr2, loss2, none, _ = call(True, drop=torch.zeros(B, dtype=torch.bool).cuda())
    assert not bool(tr2.last_drop.any()) and not bool(none.pop("empty_text_embed").any())
    for name, g in (("cond_drop_prob 0", p0), ("all-False mask", none)):
        print(name, "against the call without the feature: (tensors differing in bits, worst relative difference, where) =", bit_differences(today, g))
    for loss, g in ((loss1, p0), (loss2, none)):
        assert torch.equal(bits(loss), bits(loss0)) and set(g) == set(today)
        for k, v in today.items():
            assert torch.equal(bits(g[k]), bits(v)), k


@pytest.mark.parametrize("spatial,Te", [((12, 8), 3), ((8, 5), 22), ((12, 8), 1)], ids=["L96-3", "L40-22", "L96-1"])
def test_deterministic_backward(G, spatial, Te):
    """D3PMTrainer(deterministic=True): the same gradients to the oracle's bar, the same bits from two identical calls, and the
    process-wide switch back off afterwards"""
    want_loss, want, want_null, gmax, _ = precondition(spatial, Te)
    _, loss1, g1 = masked_call(G, spatial, Te, deterministic=True)
    _, loss2, g2 = masked_call(G, spatial, Te, deterministic=True)
    assert G.ops.set_deterministic(False) is False
    np.testing.assert_allclose(loss1.item(), want_loss, rtol=2e-5)
    errs = {k: (g1[k].cpu() - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax) for k, w in want.items()}
    errs["empty_text_embed"] = (g1["empty_text_embed"][:Te].cpu() - want_null).abs().max().item() / max(want_null.abs().max().item(), 1e-3 * gmax)
    worst = max(errs, key=errs.get)
    n, d, name = bit_differences(g1, g2)
    parity_report(f"cond_dropout_deterministic::L{spatial[0] * spatial[1]}_Te{Te}",
                  {"worst_relative_error": errs[worst], "worst_parameter": worst, "tensors_differing_between_two_calls": n, "worst_difference": d})
    assert set(g1) == set(want) | {"empty_text_embed"}
    for k, e in errs.items():
        assert e < 2e-3, f"{k}: relative max error {e:.3e}"
    assert torch.equal(bits(loss1), bits(loss2))
    for k, v in g1.items():
        assert torch.equal(bits(v), bits(g2[k])), k


# ----------------------------------------------------------------------------- 4. the optimiser
def test_adam_step_moves_the_null_embedding_as_torch(G):
    """one native step against torch.optim.Adam on the oracle's gradient: tolerances and `big` filter of test_adam_step_matches_torch"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial, Te = (12, 8), 3
    _, want, want_null, gmax, _ = precondition(spatial, Te)
    dm, sd = build(spatial)
    start = sd["empty_text_embed"][:Te].float()                           # the f32 copy the step updates
    prm = torch.nn.Parameter(start.clone())
    opt = torch.optim.Adam([prm], lr=1e-4, betas=(0.5, 0.999))
    prm.grad = want_null
    opt.step()
    x0, cond = batch4(96, Te)
    t, pt, mask = args4()
    dm = dm.cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm, lr=1e-4, betas=(0.5, 0.999))
    tr.step(x0.cuda(), cond.cuda(), t=t.cuda(), pt=pt.cuda(), drop=mask.cuda())
    after = dm.empty_text_embed.detach().cpu()
    assert after.dtype == torch.float64 and tuple(after.shape) == (77, 512)
    assert torch.equal(after[Te:], sd["empty_text_embed"][Te:]), "rows >= Te must keep their fp64 values"
    d_ref = prm.detach() - start
    d_got = (after[:Te] - start.double()).float()
    big = want_null.abs() > 1e-3 * want_null.abs().max().clamp(min=1e-12)      # ignore sign flips of ~zero gradients
    assert int(big.sum()) > 0.9 * big.numel()
    parity_report("cond_dropout_adam::L96_Te3", {"max_update_error": float((d_got - d_ref)[big].abs().max()), "compared": int(big.sum())})
    assert torch.allclose(d_got[big], d_ref[big], atol=2e-6, rtol=2e-2)
    # the transformer moved as well, through the same launch
    k = "blocks.0.attn2.value.weight"
    assert not torch.equal(dict(dm.transformer.named_parameters())[k].detach().cpu(), sd["transformer." + k])
    st = tr.optimizer_state()
    assert st["m"].numel() == tr._adam.m.numel() and tr._adam.params[-1][0] == "empty_text_embed" and st["step"] == 1


# ----------------------------------------------------------------------------- 5. captured = eager
def test_captured_step_equals_the_eager_steps(G, monkeypatch):
    """three steps, p = 0.5, the draw on the device: tolerances of test_captured_step_equals_the_eager_steps; empty_text_embed compared.
    Both modes with the reproducible reductions (see the module docstring)."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial, Te = (12, 8), 3
    for s in (3, 4, 5):                                                    # (CPU) every step drops two of the four samples
        assert int(G.cond_drop_rows(NOISE_SEED, s, B, 0, 0.5).sum()) == 2
    g = torch.Generator().manual_seed(43)
    batches = [(torch.randint(0, K, (B, 96), generator=g).cuda(), torch.randn(B, Te, 512, generator=g).cuda(),
                torch.randint(0, T, (B,), generator=g).cuda(), torch.full((B,), 1.0 / T).cuda()) for _ in range(3)]
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GSDD_TRAIN_GRAPH", mode)
        dm = build(spatial)[0].cuda().train()
        dm.cond_drop_prob = 0.5
        dm.set_noise(NOISE_SEED, stream=3)
        tr = D3PMTrainer(dm, lr=1e-3, deterministic=True)
        losses = []
        for i, (x0, cond, t, pt) in enumerate(batches):
            losses.append(tr.step(x0, cond, t=t, pt=pt)[0].item())
            if mode == "0":
                assert np.array_equal(tr.last_drop.cpu().numpy().astype(bool), G.cond_drop_rows(NOISE_SEED, 3 + i, B, 0, 0.5))
        took_graph, stream_after, adam_steps = getattr(tr, "_graph", None) is not None, dm.noise_stream, tr._adam.step_count
        params = {k: v.detach().cpu() for k, v in dm.transformer.state_dict().items()}
        params["empty_text_embed"] = dm.empty_text_embed.detach().cpu()
        runs[mode] = (losses, params)
        # the captured graph is released here, before any comparison: a failing assertion keeps this frame's locals alive in its
        # traceback's reference cycle, and a CUDAGraph that the cyclic collector frees during a later test's stream capture aborts the process
        del tr, dm
        gc.collect()
        torch.cuda.synchronize()
        assert took_graph == (mode == "1"), "the step with dropout did not take the graph path"
        assert stream_after == 6 and adam_steps == len(batches)
    np.testing.assert_allclose(runs["1"][0], runs["0"][0], rtol=2e-5)
    start = build(spatial)[1]["empty_text_embed"]
    assert not torch.equal(runs["0"][1]["empty_text_embed"][:Te], start[:Te]) and torch.equal(runs["0"][1]["empty_text_embed"][Te:], start[Te:])
    worst, outside = 0.0, []
    for k, w in runs["0"][1].items():
        if k.endswith(("attn1.key.bias", "attn2.key.bias")):
            continue
        d = (runs["1"][1][k] - w).abs()
        worst = max(worst, float(d.max()))
        if bool((d > 2e-6 + 1e-5 * w.abs()).any()):
            outside.append((k, int((d > 2e-6 + 1e-5 * w.abs()).sum()), float(d.max())))
    print("captured against eager: largest parameter difference", worst, "; (tensor, entries outside the tolerances, largest) =", outside)
    parity_report("cond_dropout_captured::L96_Te3", {"max_parameter_difference": worst, "losses": runs["1"][0], "outside_tolerance": outside})
    for k, w in runs["0"][1].items():
        if k.endswith(("attn1.key.bias", "attn2.key.bias")):     # softmax is shift invariant: these gradients are mathematically zero, what
            continue                                             # arrives is rounding noise, and Adam normalises noise to full-size updates
        torch.testing.assert_close(runs["1"][1][k], w, atol=2e-6, rtol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


# ----------------------------------------------------------------------------- 6. the autograd bridge
def test_autograd_bridge_fills_the_null_embedding_s_grad(G):
    spatial, Te = (12, 8), 3
    x0, cond = batch4(96, Te)
    _, _, mask = args4()
    dm = build(spatial)[0].cuda().train()
    dm.set_noise(NOISE_SEED, stream=0)
    torch.manual_seed(5)                                                   # (forward draws its own timesteps)
    out = dm({"content_token": x0.cuda(), "condition_embed_token": cond.cuda(), "condition_drop": mask.cuda()}, return_loss=True,
             return_logits=False)
    out["loss"].backward()
    grad = dm.empty_text_embed.grad
    assert grad is not None and grad.dtype == torch.float64 and tuple(grad.shape) == (77, 512)
    assert not bool(grad[Te:].any()) and bool(grad[:Te].any())
    assert dict(dm.transformer.named_parameters())["blocks.0.attn2.value.weight"].grad is not None
    t_used = dm.last_train_stats["t"].clone()
    from gsdd_amd.d3pm_train import D3PMTrainer
    dm2 = build(spatial)[0].cuda()
    dm2.set_noise(NOISE_SEED, stream=0)
    loss, got = D3PMTrainer(dm2).loss_and_grads(x0.cuda(), cond.cuda(), t=t_used, pt=torch.full((B,), 1.0 / T).cuda(), drop=mask.cuda())
    assert torch.equal(bits(loss[0]), bits(out["loss"].detach()))
    assert torch.equal(grad, got["empty_text_embed"].double())
    # torch's Adam over the module's parameters then updates the fp64 parameter like any other
    before = dm.empty_text_embed.detach().clone()
    torch.optim.Adam(dm.parameters(), lr=1e-4, betas=(0.5, 0.999)).step()
    assert not torch.equal(dm.empty_text_embed.detach()[:Te], before[:Te]) and torch.equal(dm.empty_text_embed.detach()[Te:], before[Te:])


# ----------------------------------------------------------------------------- 7. the sampler
def test_sampler_uses_the_learned_null_rows(G):
    """learnable_cf and cf_condition_embed = None: the tokens of the call with the null rows passed explicitly, eager and captured,
    sample and sample_fast(skip_step=1); an explicit embedding still wins"""
    Bs, Te = 2, 3
    dm = build((8, 8))[0].cuda().eval()
    cond = torch.randn(Bs, Te, 512, generator=torch.Generator().manual_seed(3)).cuda()
    null = dm.empty_text_embed.detach()[:Te].float()[None].expand(Bs, Te, 512).contiguous()
    toks = {}
    for name, call in (("sample", lambda cf, graph: dm.sample(["a"] * Bs, None, cond, cf, filter_ratio=0, use_graph=graph)),
                       ("sample_fast", lambda cf, graph: dm.sample_fast(["a"] * Bs, None, cond, filter_ratio=0, skip_step=1,
                                                                        cf_condition_embed=cf, use_graph=graph))):
        for graph in (False, True):
            dm.set_noise(NOISE_SEED, stream=2)
            want = call(null, graph)["content_token"].cpu()
            dm.set_noise(NOISE_SEED, stream=2)
            got = call(None, graph)["content_token"].cpu()
            assert torch.equal(got, want), (name, graph)
            assert int(want.max()) <= K and int(want.min()) >= 0
            toks[(name, graph)] = want
        assert torch.equal(toks[(name, False)], toks[(name, True)])
    dm.set_noise(NOISE_SEED, stream=2)
    other = dm.sample(["a"] * Bs, None, cond, torch.zeros_like(cond), filter_ratio=0)["content_token"].cpu()
    assert not torch.equal(other, toks[("sample", True)])                  # an explicit cf_condition_embed is what the chain guides with
    dm.learnable_cf = False
    with pytest.raises(G.GsddError, match="needs cf_condition_embed"):
        dm.sample(["a"] * Bs, None, cond, None, filter_ratio=0)
    parity_report("cond_dropout_sampler::L64_Te3", {"mismatches": 0, "calls": 8})
