"""Classifier-free training, host side (no GPU): the drop rule's numpy restatement against the oracle's Philox, the validation of
cond_drop_prob / train_cond_drop_prob and of the null condition, the unchanged state dict, the config key and the C ABI's symbols."""
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 21


def oracle_flags(seed, stream, B, row0, p):
    """the rule as the issue states it, on oracle.philox.philox4x32_10: key = seed, counter = (row lo, row hi, stream, 1), word 0"""
    from oracle.philox import philox4x32_10
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    w = philox4x32_10((rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32),
                      np.full(B, stream, dtype=np.uint32), np.ones(B, dtype=np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) < np.float32(p)


def tiny_dm(learnable_cf=False, cond_dim=512, spatial=(4, 4)):
    import gsdd_amd as G
    L = spatial[0] * spatial[1]
    d = G.DalleMaskImageEmbedding(num_embed=32, spatial_size=list(spatial), embed_dim=64)
    tr = G.Text2ImageTransformer(dalle=d, n_layer=1, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                 content_spatial_size=list(spatial), condition_dim=cond_dim, diffusion_step=100)
    return G.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2, content_seq_len=L,
                                  learnable_cf=learnable_cf)


def test_restatement_is_the_philox_rule():
    import gsdd_amd
    f = gsdd_amd.cond_drop_rows
    assert int(f(SEED, 3, 8192, 1000, 0.1).sum()) == 839 and int(f(SEED, 3, 8192, 1000, 0.5).sum()) == 4034
    for stream, want in ((3, [0, 1, 0, 1]), (4, [0, 1, 1, 0]), (5, [0, 0, 1, 1])):
        assert f(SEED, stream, 4, 0, 0.5).astype(int).tolist() == want
    for seed, stream, B, row0, p in ((SEED, 3, 8192, 1000, 0.1), (SEED, 3, 8192, 1000, 0.5), (SEED, 7, 9, 2 ** 33 + 5, 0.5),
                                     ((5 << 32) | 77, 2 ** 31 + 3, 64, 0, 0.3)):
        got = f(seed, stream, B, row0, p)
        assert got.dtype == np.bool_ and got.shape == (B,)
        assert np.array_equal(got, oracle_flags(seed, stream, B, row0, p)), (seed, stream, B, row0, p)


def test_a_shard_draws_the_rows_of_the_full_batch():
    import gsdd_amd
    f = gsdd_amd.cond_drop_rows
    full = f(SEED, 3, 64, 1000, 0.5)
    assert np.array_equal(f(SEED, 3, 8, 1000 + 16, 0.5), full[16:24])
    assert 0 < full.sum() < 64


def test_p_zero_drops_nothing_p_one_everything():
    import gsdd_amd
    f = gsdd_amd.cond_drop_rows
    assert not f(SEED, 3, 8192, 1000, 0.0).any() and f(SEED, 3, 8192, 1000, 1.0).all()


def test_discrete_diffusion_validates_train_cond_drop_prob():
    import gsdd_amd
    text = lambda texts: torch.zeros(len(texts), 512)
    dm = tiny_dm()
    assert dm.cond_drop_prob == 0.0
    assert gsdd_amd.DiscreteDiffusion(text, dm).diffusion_model.cond_drop_prob == 0.0        # null leaves the attribute alone
    for bad in (-0.1, 1.5, "0.1", True, float("nan"), [0.1]):
        with pytest.raises(gsdd_amd.GsddError, match="train_cond_drop_prob"):
            gsdd_amd.DiscreteDiffusion(text, dm, train_cond_drop_prob=bad)
    assert dm.cond_drop_prob == 0.0
    for ok in (0, 0.1, 1, 1.0):
        assert gsdd_amd.DiscreteDiffusion(text, dm, train_cond_drop_prob=ok).diffusion_model.cond_drop_prob == float(ok)
    # the null condition handed to the denoiser: the provider's "" embedding without learnable_cf, nothing with it or without dropout
    dd = gsdd_amd.DiscreteDiffusion(lambda texts: torch.ones(len(texts), 22, 512), dm, zero_text_emb=False, train_cond_drop_prob=0.1)
    n = dd.null_condition("cpu")
    assert tuple(n.shape) == (1, 22, 512) and dd.null_condition("cpu") is n
    dm.cond_drop_prob = 0.0
    assert dd.null_condition("cpu") is None
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm(learnable_cf=True), train_cond_drop_prob=0.1).null_condition("cpu") is None


def test_learned_null_embedding_needs_its_shape():
    import gsdd_amd
    from gsdd_amd.d3pm_train import D3PMTrainer
    dm = tiny_dm(learnable_cf=True)
    dm.cond_drop_prob = 0.1
    x0 = torch.zeros(2, 16, dtype=torch.long)
    with pytest.raises(gsdd_amd.GsddError, match="learnable_cf"):
        D3PMTrainer(dm).loss_and_grads(x0, torch.zeros(2, 78, 512))
    with pytest.raises(gsdd_amd.GsddError, match="learnable_cf"):
        dm.null_condition(78, 512)
    dm = tiny_dm(learnable_cf=True, cond_dim=256)
    dm.cond_drop_prob = 0.1
    with pytest.raises(gsdd_amd.GsddError, match="learnable_cf"):
        D3PMTrainer(dm).loss_and_grads(x0, torch.zeros(2, 3, 256))
    with pytest.raises(gsdd_amd.GsddError, match="learnable_cf"):          # an explicit mask asks for the null rows as well
        D3PMTrainer(dm).loss_and_grads(x0, torch.zeros(2, 3, 256), drop=torch.tensor([True, False]))
    dm = tiny_dm(learnable_cf=True)
    rows = dm.null_condition(3, 512)
    assert rows.dtype == torch.float32 and torch.equal(rows, dm.empty_text_embed.detach()[:3].float())


def test_dropout_without_a_null_condition_is_an_error():
    import gsdd_amd
    from gsdd_amd.d3pm_train import D3PMTrainer
    dm = tiny_dm()
    x0, cond = torch.zeros(2, 16, dtype=torch.long), torch.zeros(2, 3, 512)
    dm.cond_drop_prob = 0.1
    with pytest.raises(gsdd_amd.GsddError, match="needs a null condition"):
        D3PMTrainer(dm).loss_and_grads(x0, cond)
    with pytest.raises(gsdd_amd.GsddError, match="needs a null condition"):
        D3PMTrainer(dm).step(x0, cond)
    dm.cond_drop_prob = 0.0
    with pytest.raises(gsdd_amd.GsddError, match="needs a null condition"):
        D3PMTrainer(dm).loss_and_grads(x0, cond, drop=torch.tensor([True, False]))
    with pytest.raises(gsdd_amd.GsddError, match="null condition must be"):
        dm.null_condition(3, 512, torch.zeros(4, 512))
    assert tuple(dm.null_condition(3, 512, torch.zeros(1, 3, 512)).shape) == (3, 512)
    with pytest.raises(gsdd_amd.GsddError, match="drop mask"):
        D3PMTrainer(dm).loss_and_grads(x0, cond, null_cond=torch.zeros(3, 512), drop=torch.tensor([1.0, 0.0]))
    for bad in (-0.5, 2, "x"):
        dm.cond_drop_prob = bad
        with pytest.raises(gsdd_amd.GsddError, match="cond_drop_prob"):
            D3PMTrainer(dm).loss_and_grads(x0, cond, null_cond=torch.zeros(3, 512))
    # without dropout the call goes on as before: the first thing it misses on this machine is the device
    dm.cond_drop_prob = 0.0
    with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):
        D3PMTrainer(dm).loss_and_grads(x0, cond)


def test_guided_sampling_without_an_unconditional_embedding():
    import gsdd_amd
    dm = tiny_dm()
    cond = torch.zeros(2, 3, 512)
    with pytest.raises(gsdd_amd.GsddError, match="needs cf_condition_embed"):
        dm.sample_fast(["a", "b"], None, cond, filter_ratio=0)
    dm = tiny_dm(learnable_cf=True)
    cf = dm._cf_embed(cond, None)
    assert tuple(cf.shape) == (2, 3, 512) and torch.equal(cf[1], dm.empty_text_embed.detach()[:3].float())
    given = torch.ones(2, 3, 512)
    assert dm._cf_embed(cond, given) is given                              # an explicit embedding still wins
    dm.guidance_scale = 1
    assert dm._cf_embed(cond, None) is None


def test_state_dict_is_unchanged():
    for learnable in (False, True):
        dm = tiny_dm(learnable_cf=learnable)
        sd = dm.state_dict()
        assert "empty_text_embed" in sd and tuple(sd["empty_text_embed"].shape) == (77, 512) and sd["empty_text_embed"].dtype == torch.float64
        assert not any("cond_drop" in k or "null" in k for k in sd)
        assert set(sd) == {"empty_text_embed", "log_at", "log_bt", "log_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct",
                           "log_1_min_ct", "log_1_min_cumprod_ct", "Lt_history", "Lt_count"} | {"transformer." + k for k in dm.transformer.state_dict()}
        assert [n for n, _ in dm.named_parameters() if not n.startswith("transformer.")] == ["empty_text_embed"]


def test_config_composes_with_the_new_key(monkeypatch):
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.train_cond_drop_prob is None
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.train_cond_drop_prob=0.1"]).model.generator
    assert gen.train_cond_drop_prob == 0.1


def test_abi_symbols():
    import gsdd_amd
    with open(os.path.join(REPO, "include", "gsdd.h")) as f:
        header = f.read()
    for sym in ("gsdd_cond_dropout", "gsdd_cond_null_grad", "gsdd_set_deterministic"):
        assert sym in gsdd_amd.EXPORTS and header.count(f"int {sym}(") == 1, sym
    if os.path.exists(gsdd_amd.LIB_PATH):
        L = gsdd_amd.lib()
        assert L.gsdd_version() >= 108 and hasattr(L, "gsdd_cond_dropout") and hasattr(L, "gsdd_cond_null_grad")
        assert L.gsdd_set_deterministic(1) == 0 and L.gsdd_set_deterministic(0) == 1 and L.gsdd_set_deterministic(0) == 0      # returns the previous setting
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "gsdd_cond_dropout" in doc and "gsdd_cond_null_grad" in doc and "gsdd_set_deterministic" in doc


def test_trainer_deterministic_switch(monkeypatch):
    from gsdd_amd.d3pm_train import D3PMTrainer
    dm = tiny_dm()
    assert D3PMTrainer(dm).deterministic is False and D3PMTrainer(dm, deterministic=True).deterministic is True
    monkeypatch.setenv("GSDD_TRAIN_DETERMINISTIC", "1")
    assert D3PMTrainer(dm).deterministic is True and D3PMTrainer(dm, deterministic=False).deterministic is False
