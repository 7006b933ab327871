"""The D3PM training step with per-token text conditioning (cond of shape (B, Te > 1, cond_dim)): every parameter gradient of the whole
model against torch.autograd of oracle.d3pm.train_loss (which handles any Te), one Adam step against torch.optim.Adam, and the captured
step against the eager one.  With Te > 1 the cross-attention softmax runs over several keys, so attn2.query, attn2.key and ln1_1 --
exactly zero with one token -- carry real gradients.

Model: two layers, K = 32, B = 2, seeded trained-like weights (scaled as in tests/test_gpu_training.py::random_model).  L = 96 (spatial
[12, 8]: matrix-pipe self-attention, and the row GEMMs on the fragment images) and L = 40 (L % 32 != 0: the vector self-attention
kernels); Te in {3, 22}; t = [0, 61] and [37, 99]; each once more with GSDD_TRAIN_LINEAR=gemm (the generic row GEMM branch).

Bar (the project's gradient bar, tests/test_gpu_training.py): the loss to rtol 2e-5; every tensor to 2e-3 of max(its own largest entry,
1e-3 of the model's largest gradient).

Precondition, on the oracle alone and on the CPU, before any device call: the median over (layer, batch, head, row) of the largest
cross-attention probability lies in [1.5 / Te, 0.9] -- neither flat (where dq and dk vanish) nor one-hot.  Discrimination: the largest
entries of the attn2.query.weight, attn2.key.weight and ln1_1.linear.weight gradients are above 1e-3 of the model's largest gradient in
every layer; below that the bar would not see them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import parity_report

pytestmark = pytest.mark.gpu

K, B, T, SEED, NOISE_SEED = 32, 2, 100, 8, 21
ZERO_WITH_ONE_TOKEN = ("attn2.query.weight", "attn2.query.bias", "attn2.key.weight", "attn2.key.bias", "ln1_1.emb.weight",
                       "ln1_1.linear.weight", "ln1_1.linear.bias")


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def make_model(spatial):
    """-> (DiffusionTransformer on the CPU, its state dict): two layers, weights of a trained-like magnitude"""
    import gsdd_amd as G
    L = spatial[0] * spatial[1]
    d = G.DalleMaskImageEmbedding(num_embed=K, spatial_size=list(spatial), embed_dim=64)
    tr = G.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                 content_spatial_size=list(spatial), condition_dim=512, diffusion_step=T)
    g = torch.Generator().manual_seed(SEED)
    for mod in tr.modules():
        if isinstance(mod, torch.nn.Linear):
            mod.weight.data = torch.randn(mod.weight.shape, generator=g) * (1.0 / mod.in_features ** 0.5)
            mod.bias.data = 0.1 * torch.randn(mod.bias.shape, generator=g)
        elif isinstance(mod, torch.nn.Embedding):
            mod.weight.data = torch.randn(mod.weight.shape, generator=g) * 0.5
    dm = G.DiffusionTransformer(transformer=tr, diffusion_step=T, alpha_init_type="alpha1", auxiliary_loss_weight=5e-4,
                                adaptive_auxiliary_loss=True, guidance_scale=2, content_seq_len=L)
    return dm, {k: v.detach().clone() for k, v in dm.state_dict().items()}


def batch(L, Te):
    g = torch.Generator().manual_seed(1000 * L + Te)
    return torch.randint(0, K, (B, L), generator=g), torch.randn(B, Te, 512, generator=g)


def cross_attention_pmax(x0, cond, t, sd, n_head=16):
    """largest probability of every cross-attention row of every block, from the oracle's own pieces, on the x_t the loss draws"""
    from oracle import d3pm as od
    xt = od.gumbel_argmax(od.q_pred(od.index_to_log_onehot(x0, sd["transformer.content_emb.emb.weight"].shape[0]), t, sd), NOISE_SEED, 0)
    x, out = od.content_emb(xt, sd), []
    Te = cond.shape[1]
    for i in range(od.n_layers(sd)):
        p = f"transformer.blocks.{i}."
        h = od.ada_layer_norm(x, t, sd, p + "ln1.")
        hq = od.ada_layer_norm(x + od.mha(h, h, sd, p + "attn1.", n_head), t, sd, p + "ln1_1.")
        q = F.linear(hq, sd[p + "attn2.query.weight"], sd[p + "attn2.query.bias"]).view(B, -1, n_head, 4).transpose(1, 2)
        k = F.linear(cond, sd[p + "attn2.key.weight"], sd[p + "attn2.key.bias"]).view(B, Te, n_head, 4).transpose(1, 2)
        out.append(torch.softmax((q @ k.transpose(-2, -1)) * 0.5, -1).amax(-1).reshape(-1))
        x = od.block(x, cond, t, sd, p, n_head)
    return torch.cat(out)


@functools.lru_cache(maxsize=None)
def oracle_case(spatial, Te, tvals):
    """(loss, gradients by parameter name, median largest cross-attention probability): CPU only, computed once per case"""
    from oracle import d3pm as od
    _, sd = make_model(spatial)
    x0, cond = batch(spatial[0] * spatial[1], Te)
    t = torch.tensor(tvals, dtype=torch.long)
    with torch.no_grad():
        med = float(cross_attention_pmax(x0, cond, t, sd).median())
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith("transformer.") and v.dtype.is_floating_point else v) for k, v in sd.items()}
    loss, _, _, _ = od.train_loss(x0, cond, t, torch.ones(B) / T, leaf, NOISE_SEED, 0)
    loss.backward()
    grads = {k[len("transformer."):]: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()
             if k.startswith("transformer.") and v.dtype.is_floating_point}
    return loss.item(), grads, med


def check_preconditions(Te, want, med):
    assert 1.5 / Te <= med <= 0.9, f"cross-attention rows are flat or one-hot: median largest probability {med}"
    gmax = max(w.abs().max().item() for w in want.values())
    for i in range(2):
        for n in ("attn2.query.weight", "attn2.key.weight", "ln1_1.linear.weight"):
            assert want[f"blocks.{i}.{n}"].abs().max().item() > 1e-3 * gmax, (i, n)
    return gmax


@pytest.mark.parametrize("linear", ["images", "gemm"])
@pytest.mark.parametrize("tvals", [(0, 61), (37, 99)])
@pytest.mark.parametrize("Te", [3, 22])
@pytest.mark.parametrize("spatial", [(12, 8), (8, 5)], ids=["L96", "L40"])
def test_loss_gradients_match_autograd_of_oracle(G, monkeypatch, spatial, Te, tvals, linear):
    from gsdd_amd.d3pm_train import D3PMTrainer
    want_loss, want, med = oracle_case(spatial, Te, tvals)
    gmax = check_preconditions(Te, want, med)                      # (CPU, before any device call)
    if linear == "gemm":
        monkeypatch.setenv("GSDD_TRAIN_LINEAR", "gemm")
    L = spatial[0] * spatial[1]
    x0, cond = batch(L, Te)
    dm = make_model(spatial)[0].cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm)
    loss, got = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=torch.tensor(tvals).cuda(), pt=(torch.ones(B) / T).cuda())
    assert (tr._images is not None) == (linear == "images")
    worst = ("", 0.0)
    for k, w in want.items():
        scale = max(w.abs().max().item(), 1e-3 * gmax)
        err = (got[k].cpu() - w).abs().max().item() / scale
        if err > worst[1]:
            worst = (k, err)
    rec = {"worst_relative_error": worst[1], "worst_parameter": worst[0], "loss": loss.item(), "oracle_loss": want_loss,
           "median_largest_probability": med, "worst_ratio": worst[1] / 2e-3}
    print(rec)
    parity_report(f"training_cond_tokens::L{L}_Te{Te}_t{tvals[0]}_{tvals[1]}_{linear}", rec)
    np.testing.assert_allclose(loss.item(), want_loss, rtol=2e-5)
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        assert got[k].shape == w.shape, k
        scale = max(w.abs().max().item(), 1e-3 * gmax)
        err = (got[k].cpu() - w).abs().max().item() / scale
        assert err < 2e-3, f"{k}: relative max error {err:.3e} (|g|max {scale:.3e})"


def test_adam_step_matches_torch(G):
    """One D3PMTrainer.step equals torch.optim.Adam on the oracle's gradients (as tests/test_gpu_training.py::test_adam_step_matches_torch)."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial, Te, tvals = (12, 8), 3, (37, 99)
    _, want_g, med = oracle_case(spatial, Te, tvals)
    check_preconditions(Te, want_g, med)
    dm, sd = make_model(spatial)
    ref = {k[len("transformer."):]: v.clone() for k, v in sd.items() if k.startswith("transformer.") and v.dtype.is_floating_point}
    params = [torch.nn.Parameter(v) for v in ref.values()]
    opt = torch.optim.Adam(params, lr=1e-4, betas=(0.5, 0.999))
    for prm, k in zip(params, ref):
        prm.grad = want_g[k]
    opt.step()
    dm = dm.cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    x0, cond = batch(96, Te)
    D3PMTrainer(dm, lr=1e-4, betas=(0.5, 0.999)).step(x0.cuda(), cond.cuda(), t=torch.tensor(tvals).cuda(), pt=(torch.ones(B) / T).cuda())
    got = dict(dm.transformer.named_parameters())
    gmax = max(v.abs().max().item() for v in want_g.values())
    compared = set()
    for prm, k in zip(params, ref):
        if want_g[k].abs().max().item() < 1e-4 * gmax:
            continue        # mathematically zero gradient (rounding noise): Adam turns noise into +-lr steps, not comparable
        d_ref = prm.detach() - sd["transformer." + k]
        d_got = got[k].detach().cpu() - sd["transformer." + k]
        big = want_g[k].abs() > 1e-3 * want_g[k].abs().max().clamp(min=1e-12)      # ignore sign flips of ~zero gradients
        assert torch.allclose(d_got[big], d_ref[big], atol=2e-6, rtol=2e-2), k
        compared.add(k)
    assert {f"blocks.{i}.{n}" for i in range(2) for n in ("attn2.query.weight", "attn2.key.weight", "ln1_1.linear.weight")} <= compared
    assert dm.transformer._packed is None


def test_captured_step_equals_the_eager_steps(G, monkeypatch):
    """Te = 3 at L = 96: three steps give the same losses and final parameters as a captured graph (the third step is the replay) and
    launch by launch (GSDD_TRAIN_GRAPH=0); tolerances of tests/test_gpu_training.py::test_captured_training_step_equals_the_eager_steps."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial, Te = (12, 8), 3
    g = torch.Generator().manual_seed(43)
    batches = [(torch.randint(0, K, (B, 96), generator=g).cuda(), torch.randn(B, Te, 512, generator=g).cuda(),
                torch.randint(0, T, (B,), generator=g).cuda(), torch.full((B,), 1.0 / T).cuda()) for _ in range(3)]
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GSDD_TRAIN_GRAPH", mode)
        dm = make_model(spatial)[0].cuda().train()
        dm.set_noise(NOISE_SEED, stream=3)
        tr = D3PMTrainer(dm, lr=1e-3)
        losses = [tr.step(x0, cond, t=t, pt=pt)[0].item() for x0, cond, t, pt in batches]
        assert (getattr(tr, "_graph", None) is not None) == (mode == "1"), "the Te > 1 step did not take the graph path"
        assert dm.noise_stream == 3 + len(batches) and tr._adam.step_count == len(batches)
        runs[mode] = (losses, {k: v.detach().clone() for k, v in dm.transformer.state_dict().items()})
    np.testing.assert_allclose(runs["1"][0], runs["0"][0], rtol=2e-5)
    for k, w in runs["0"][1].items():
        if k.endswith(("attn1.key.bias", "attn2.key.bias")):     # softmax is shift invariant: these gradients are mathematically zero, what
            continue                                             # arrives is rounding noise, and Adam normalises noise to full-size updates
        torch.testing.assert_close(runs["1"][1][k], w, atol=2e-6, rtol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_one_token_keeps_its_exact_zeros_and_the_graph_path(G):
    """Te = 1: attn2.query, attn2.key and ln1_1 get exactly zero gradient, the attn2 images are never packed, and the step is captured."""
    from gsdd_amd.d3pm_train import D3PMTrainer
    spatial = (12, 8)
    x0, cond = batch(96, 1)
    dm = make_model(spatial)[0].cuda()
    dm.set_noise(NOISE_SEED, stream=0)
    tr = D3PMTrainer(dm)
    t, pt = torch.tensor([37, 99]).cuda(), (torch.ones(B) / T).cuda()
    _, got = tr.loss_and_grads(x0.cuda(), cond.cuda(), t=t, pt=pt)
    for i in range(2):
        for n in ZERO_WITH_ONE_TOKEN:
            assert not bool(got[f"blocks.{i}.{n}"].any()), (i, n)
        assert bool(got[f"blocks.{i}.attn2.value.weight"].any()) and bool(got[f"blocks.{i}.attn2.proj.weight"].any())
    assert tr._images is not None and not tr._images.cross and "q2" not in tr._images.images[0]
    for _ in range(3):
        tr.step(x0.cuda(), cond.cuda(), t=t, pt=pt)
    assert getattr(tr, "_graph", None) is not None
