"""D3PMTrainer's optimiser stage end to end on small models: one step against torch's clip_grad_norm_ + AdamW in fp64, a learning-rate
warm-up on the captured path (one graph for the whole schedule), the averaged weights swapped in and out around sampling, exact
resume, and the non-finite guard.  Bars of the one-step comparison are the derived ones of tests/test_gpu_optim_kernels.py."""
import gc
import math

import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_optim_kernels import U, f32, ratio, tensor_reference
from tests.test_gpu_training import build as build_l64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def release(*objs):
    """captured graphs are released before any comparison (a CUDAGraph freed by the cyclic collector during a
    later test's stream capture aborts the process)"""
    for o in objs:
        if hasattr(o, "_graphs"):
            o._graph, o._graphs = None, {}
    gc.collect()
    torch.cuda.synchronize()


def l64_batches(cfg, n, seed=41):
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, K, (B, L), generator=g).cuda(), torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda(),
             torch.randint(0, T, (B,), generator=g).cuda(), torch.full((B,), 1.0 / T).cuda()) for _ in range(n)]


def expected_decaying(names):
    """by module type: the weight matrices of the attention, MLP and logit-head Linear layers -- nothing of a norm, no embedding"""
    lin = ("attn1.query", "attn1.key", "attn1.value", "attn1.proj", "attn2.query", "attn2.key", "attn2.value", "attn2.proj",
           "mlp.0", "mlp.2")
    return {n for n in names if n == "to_logits.1.weight" or (n.endswith(".weight") and n.startswith("blocks.")
                                                               and n.split(".", 2)[2][:-len(".weight")] in lin)}


# ----------------------------------------------------------------------------- one step against torch
def test_one_step_matches_clip_and_adamw_in_fp64(G, golden):
    from gsdd_amd.d3pm_train import D3PMTrainer, default_decay_mask
    sd, a, cfg = golden("d3pm_L64")
    (x0, cond, t, pt), = l64_batches(cfg, 1)
    lr, wd, ema, betas = 1e-3, 0.05, 0.999, (0.9, 0.96)

    def fresh(**kw):
        dm = build_l64(G, sd, cfg).train()
        dm.set_noise(cfg["noise_seed"], stream=3)
        return dm, D3PMTrainer(dm, lr=lr, betas=betas, deterministic=True, **kw)

    dm0, tr0 = fresh()
    _, g = tr0.loss_and_grads(x0, cond, t=t, pt=pt)                       # the device gradients of this batch (reproducible form)
    grads = {k: v.detach().double().cpu() for k, v in g.items()}
    norm = math.sqrt(sum(float((v ** 2).sum()) for v in grads.values()))
    max_norm = 0.5 * norm
    dm, tr = fresh(max_grad_norm=max_norm, weight_decay=wd, ema_decay=ema)
    names = [n for n, _ in dm.transformer.named_parameters()]
    mask = default_decay_mask(dm.transformer, ("empty_text_embed",))
    assert {n for n in names if mask[n]} == expected_decaying(names) and len(expected_decaying(names)) == 10 * cfg["n_layer"] + 1
    assert not mask["empty_text_embed"] and not mask["content_emb.emb.weight"] and not mask["blocks.0.ln1.linear.weight"]
    start = {n: p.detach().double().cpu() for n, p in dm.transformer.named_parameters()}
    tr.step(x0, cond, t=t, pt=pt)
    assert tr._adam.decays == [mask[n] for n in names]
    got = {n: p.detach().cpu() for n, p in dm.transformer.named_parameters()}
    avg = tr.ema_state_dict()
    # torch: clip_grad_norm_ + AdamW on fp64 CPU copies, the same mask (the f32 values of lr, betas, eps the kernel gets)
    prm = {n: torch.nn.Parameter(v.clone()) for n, v in start.items()}
    for n in names:
        prm[n].grad = grads[n].clone()
    total = torch.nn.utils.clip_grad_norm_(list(prm.values()), f32(max_norm))
    opt = torch.optim.AdamW([{"params": [prm[n] for n in names if mask[n]], "weight_decay": f32(wd)},
                             {"params": [prm[n] for n in names if not mask[n]], "weight_decay": 0.0}],
                            lr=f32(lr), betas=(f32(betas[0]), f32(betas[1])), eps=f32(1e-8))
    opt.step()
    assert abs(float(tr.last_grad_norm) - float(total)) <= float(np.spacing(np.float32(total)))
    coef = min(1.0, f32(max_norm) / (norm + 1e-6))
    d = min(f32(ema), 2.0 / 11.0)
    worst = {"p": 0.0, "e": 0.0, "restatement": 0.0}
    for n in names:
        if n.endswith("attn1.key.bias"):              # mathematically zero gradient: rounding noise that Adam normalises to full-size steps
            continue
        zero = torch.zeros_like(start[n])
        p1, bar_p, _, _, _, _, e1, bar_e = tensor_reference(start[n], grads[n], zero, zero, start[n], step=1, lr=f32(lr), wd=f32(wd),
                                                            dec=mask[n], coef=coef, eg=2 * U, d=d, b1=betas[0], b2=betas[1])
        worst["restatement"] = max(worst["restatement"], float((p1 - prm[n].detach()).abs().max()))
        worst["p"] = max(worst["p"], ratio(got[n], prm[n].detach(), bar_p))
        worst["e"] = max(worst["e"], ratio(avg[n], d * start[n] + (1 - d) * prm[n].detach(), bar_e))
    parity_report("train_optim::one_step[L64]", worst)
    release(tr, tr0)
    assert worst["restatement"] <= 1e-12              # the bars' restatement IS torch's clip + AdamW
    assert worst["p"] <= 1 and worst["e"] <= 1, worst


# ----------------------------------------------------------------------------- warm-up on the captured path
def test_warmup_replays_one_captured_graph(G, golden, monkeypatch):
    """seven steps of linear_warmup(1e-3, 5) on changing batches with clip + decay + average + guard: the trainer captures ONCE and the
    graph of step 3 serves every later learning rate; losses, weights, average and skip count are those of the launch-by-launch run
    (tolerances of test_captured_training_step_equals_the_eager_steps)"""
    from gsdd_amd.d3pm_train import D3PMTrainer, linear_warmup
    sd, a, cfg = golden("d3pm_L64")
    batches = l64_batches(cfg, 7)
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GSDD_TRAIN_GRAPH", mode)
        dm = build_l64(G, sd, cfg).train()
        dm.set_noise(cfg["noise_seed"], stream=3)
        tr = D3PMTrainer(dm, lr=1e-3, lr_schedule=linear_warmup(1e-3, 5), max_grad_norm=1.0, weight_decay=0.01, ema_decay=0.99,
                         skip_nonfinite=True)
        losses, lrs, graphs = [], [], []
        for x0, cond, t, pt in batches:
            losses.append(tr.step(x0, cond, t=t, pt=pt)[0].item())
            lrs.append(tr.lr)
            graphs.append(tr._graph)
        facts = dict(captures=tr.captures, n_graphs=len(tr._graphs), same=all(g is graphs[2] for g in graphs[2:]),
                     took=graphs[2] is not None, steps=tr._adam.step_count, skipped=tr.skipped_steps,
                     lr_word=float(tr._adam.words.view(torch.float32)[4]), step_word=int(tr._adam.words.view(torch.int64)[0]))
        runs[mode] = (losses, {k: v.detach().cpu() for k, v in dm.transformer.state_dict().items()}, tr.ema_state_dict(), facts, lrs)
        release(tr)
        del tr, dm
    monkeypatch.delenv("GSDD_TRAIN_GRAPH")
    want_lrs = [1e-3 * min(1.0, s / 5) for s in range(1, 8)]
    for mode in ("0", "1"):
        f = runs[mode][3]
        assert runs[mode][4] == want_lrs and f["lr_word"] == f32(1e-3) and f["step_word"] == 7 and f["steps"] == 7 and f["skipped"] == 0
    f = runs["1"][3]
    assert f["took"] and f["captures"] == 1 and f["n_graphs"] == 1 and f["same"], f       # the learning rate is not baked in
    assert runs["0"][3]["captures"] == 0
    np.testing.assert_allclose(runs["1"][0], runs["0"][0], rtol=2e-5)
    for which in (1, 2):
        for k, w in runs["0"][which].items():
            if k.endswith("attn1.key.bias"):
                continue
            torch.testing.assert_close(runs["1"][which][k], w, atol=2e-6, rtol=1e-5, msg=lambda m, k=k: f"{('weights', 'average')[which - 1]} {k}: {m}")


# ----------------------------------------------------------------------------- the averaged weights around sampling
def test_ema_weights_swap_in_and_out_around_sampling(G):
    from gsdd_amd.d3pm_train import D3PMTrainer
    from tests.test_gpu_cond_dropout import build as build_cf
    from tests.test_gpu_training_cond_tokens import K, NOISE_SEED, T
    spatial, Te, B = (8, 8), 3, 4
    g = torch.Generator().manual_seed(43)
    dm = build_cf(spatial)[0].cuda().train()
    dm.cond_drop_prob = 0.5
    dm.set_noise(NOISE_SEED, stream=3)
    tr = D3PMTrainer(dm, lr=1e-3, ema_decay=0.9, deterministic=True)
    for _ in range(3):
        tr.step(torch.randint(0, K, (B, 64), generator=g).cuda(), torch.randn(B, Te, 512, generator=g).cuda(),
                t=torch.randint(0, T, (B,), generator=g).cuda(), pt=torch.full((B,), 1.0 / T).cuda())
    assert tr._adam.params[-1][0] == "empty_text_embed"
    dm.eval()
    cond = torch.randn(2, Te, 512, generator=g).cuda()

    def sample(model):
        model.set_noise(NOISE_SEED, stream=2)
        return model.sample(["a"] * 2, None, cond, None, filter_ratio=0)["content_token"].cpu()

    null_live = dm.empty_text_embed.detach().clone()
    live = {k: v.detach().clone() for k, v in dm.transformer.state_dict().items()}
    before = sample(dm)
    # a second model built from the averaged state
    dm2 = build_cf(spatial)[0].cuda().eval()
    dm2.transformer.load_state_dict(tr.ema_state_dict())
    dm2.empty_text_embed.data.copy_(tr.ema_null_embedding())
    want = sample(dm2)
    with tr.ema_weights():
        inside = sample(dm)
        null_inside = dm.empty_text_embed.detach().clone()
        with pytest.raises(G.GsddError):
            with tr.ema_weights():
                pass
        with pytest.raises(G.GsddError):
            tr.step(torch.zeros(B, 64, dtype=torch.long).cuda(), torch.zeros(B, Te, 512).cuda())
    after = sample(dm)
    null_after = dm.empty_text_embed.detach().clone()
    same_weights = all(torch.equal(v, live[k]) for k, v in dm.transformer.state_dict().items())
    release(tr)
    assert torch.equal(inside, want), "inside ema_weights() the sampler did not run on the averaged weights"
    assert not torch.equal(want, before), "the averaged model samples the live model's tokens: the case shows nothing"
    assert torch.equal(after, before) and same_weights
    assert torch.equal(null_after, null_live), "empty_text_embed was not restored bit for bit"
    assert torch.equal(null_inside[:Te], tr.ema_null_embedding()[:Te].cuda()) and not torch.equal(null_inside[:Te], null_live[:Te])


# ----------------------------------------------------------------------------- resume
def test_resume_is_bit_exact(G, golden, monkeypatch):
    """deterministic=True, launch by launch: three steps, optimizer_state() + state_dict into a fresh model and trainer, two more steps
    == five uninterrupted steps in parameters, m, v, average and step count, bit for bit"""
    from gsdd_amd.d3pm_train import D3PMTrainer, linear_warmup
    monkeypatch.setenv("GSDD_TRAIN_GRAPH", "0")
    sd, a, cfg = golden("d3pm_L64")
    batches = l64_batches(cfg, 5, seed=7)
    kw = dict(lr=1e-3, lr_schedule=linear_warmup(1e-3, 4), max_grad_norm=1.0, weight_decay=0.01, ema_decay=0.99, skip_nonfinite=True,
              deterministic=True)

    def fresh(state_dict):
        dm = build_l64(G, state_dict, cfg).train()
        return dm, D3PMTrainer(dm, **kw)

    dm, tr = fresh(sd)
    dm.set_noise(cfg["noise_seed"], stream=3)
    for x0, cond, t, pt in batches:
        tr.step(x0, cond, t=t, pt=pt)
    full = ({k: v.detach().cpu() for k, v in dm.state_dict().items()}, tr.optimizer_state())
    dm1, tr1 = fresh(sd)
    dm1.set_noise(cfg["noise_seed"], stream=3)
    for x0, cond, t, pt in batches[:3]:
        tr1.step(x0, cond, t=t, pt=pt)
    dm2, tr2 = fresh({k: v.detach().cpu() for k, v in dm1.state_dict().items()})
    dm2.set_noise(cfg["noise_seed"], stream=dm1.noise_stream)
    tr2.load_optimizer_state(tr1.optimizer_state())
    for x0, cond, t, pt in batches[3:]:
        tr2.step(x0, cond, t=t, pt=pt)
    assert tr2.lr == 1e-3 and tr.lr == 1e-3
    got = ({k: v.detach().cpu() for k, v in dm2.state_dict().items()}, tr2.optimizer_state())
    release(tr, tr1, tr2)
    assert got[1]["step"] == full[1]["step"] == 5 and got[1]["skipped_steps"] == full[1]["skipped_steps"] == 0
    for k in ("m", "v", "ema"):
        assert torch.equal(got[1][k], full[1][k]), k
    assert len(full[0]) > 10
    for k, v in full[0].items():
        if k != "empty_text_embed":        # (not in the fixture: every constructed model draws its own, and this run never reads it)
            assert torch.equal(got[0][k], v), k


# ----------------------------------------------------------------------------- the non-finite guard end to end
def test_nan_gradient_skips_one_step_and_training_goes_on(G, golden, monkeypatch):
    """a NaN written into the logit head's gradient between loss_and_grads and the optimiser (launch-by-launch path): the weights, the
    moments and the average are unchanged, the skip is counted, the step count advances, and the next step trains"""
    from gsdd_amd.d3pm_train import D3PMTrainer
    monkeypatch.setenv("GSDD_TRAIN_GRAPH", "0")
    sd, a, cfg = golden("d3pm_L64")
    batches = l64_batches(cfg, 3, seed=11)
    dm = build_l64(G, sd, cfg).train()
    dm.set_noise(cfg["noise_seed"], stream=3)
    tr = D3PMTrainer(dm, lr=1e-3, ema_decay=0.99, skip_nonfinite=True)
    poison = {"on": False}
    inner = tr.loss_and_grads

    def loss_and_grads(*args, **kw):
        loss, grads = inner(*args, **kw)
        if poison["on"]:
            grads["to_logits.1.weight"][0, 0] = float("nan")
        return loss, grads

    tr.loss_and_grads = loss_and_grads
    snap = lambda: ({k: v.detach().clone() for k, v in dm.transformer.state_dict().items()}, tr._adam.m.clone(), tr._adam.v.clone(),
                    tr._adam.ema.clone())
    same = lambda x, y: all(torch.equal(x[0][k], y[0][k]) for k in x[0]) and all(torch.equal(p, q) for p, q in zip(x[1:], y[1:]))
    x0, cond, t, pt = batches[0]
    tr.step(x0, cond, t=t, pt=pt)
    s1 = snap()
    norm1 = float(tr.last_grad_norm)
    poison["on"] = True
    x0, cond, t, pt = batches[1]
    tr.step(x0, cond, t=t, pt=pt)
    s2, skipped2, norm2 = snap(), tr.skipped_steps, float(tr.last_grad_norm)
    poison["on"] = False
    x0, cond, t, pt = batches[2]
    loss3 = float(tr.step(x0, cond, t=t, pt=pt)[0])
    s3, skipped3, steps = snap(), tr.skipped_steps, tr._adam.step_count
    finite3 = all(bool(torch.isfinite(v).all()) for v in s3[0].values() if v.dtype.is_floating_point)
    release(tr)
    assert math.isfinite(norm1) and math.isnan(norm2)
    assert same(s1, s2), "the poisoned step changed a weight, a moment or the average"
    assert skipped2 == 1 and skipped3 == 1 and steps == 3
    assert not same(s2, s3) and finite3 and math.isfinite(loss3)
