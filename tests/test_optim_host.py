"""Host side of the optimiser stage (no GPU): the warm-up schedule, the decay mask from module types, MultiAdam's state round trip
with and without averaged weights, the new config keys and their guard, the ema_weights() context's misuse errors, and the ABI's
declarations."""
import ctypes
import os
import warnings

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("gsdd_grad_sqnorm", "gsdd_grad_norm_finalize", "gsdd_adamw_ema_multi", "gsdd_swap_multi")


def tiny_model(n_layer=2):
    import gsdd_amd as G
    d = G.DalleMaskImageEmbedding(num_embed=32, spatial_size=[4, 8], embed_dim=64)
    tr = G.Text2ImageTransformer(dalle=d, n_layer=n_layer, n_embd=64, n_head=16, content_seq_len=32, block_activate="GELU2",
                                 content_spatial_size=[4, 8], condition_dim=512, diffusion_step=100)
    return G.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", auxiliary_loss_weight=5e-4,
                                  adaptive_auxiliary_loss=True, guidance_scale=2, content_seq_len=32)


def test_linear_warmup_values():
    from gsdd_amd.d3pm_train import linear_warmup
    f = linear_warmup(1e-3, 5)
    assert f(1) == 1e-3 * (1 / 5) and f(3) == 1e-3 * (3 / 5) and f(5) == 1e-3 and f(6) == 1e-3 and f(10 ** 6) == 1e-3
    assert linear_warmup(2e-4, 1)(1) == 2e-4
    for bad in (0, -3):
        with pytest.raises(ValueError):
            linear_warmup(1e-3, bad)


def test_default_decay_mask_follows_module_types():
    from gsdd_amd.d3pm_train import D3PMTrainer, default_decay_mask
    dm = tiny_model()
    tr = dm.transformer
    mask = default_decay_mask(tr, (D3PMTrainer.NULL_NAME,))
    names = [n for n, _ in tr.named_parameters()]
    assert set(mask) == set(names) | {"empty_text_embed"} and mask["empty_text_embed"] is False
    mods = dict(tr.named_modules())
    from gsdd_amd.d3pm import AdaLayerNorm
    for n in names:
        owner, leaf = n.rsplit(".", 1)
        chain = [mods[".".join(owner.split(".")[:i])] for i in range(1, owner.count(".") + 2)]
        in_norm = any(isinstance(m, (torch.nn.LayerNorm, AdaLayerNorm)) for m in chain)
        want = isinstance(mods[owner], torch.nn.Linear) and leaf == "weight" and not in_norm
        assert mask[n] == want, n
    decays = {n for n in names if mask[n]}
    assert "to_logits.1.weight" in decays and "blocks.0.attn1.query.weight" in decays and "blocks.1.mlp.2.weight" in decays
    assert "blocks.0.attn2.value.weight" in decays and len(decays) == 10 * 2 + 1
    for n in ("to_logits.1.bias", "to_logits.0.weight", "blocks.0.ln1.linear.weight", "blocks.0.ln1.emb.weight", "blocks.0.ln1_1.linear.weight",
              "blocks.0.ln2.weight", "content_emb.emb.weight", "content_emb.height_emb.weight", "blocks.1.mlp.0.bias"):
        assert n in mask and not mask[n], n


def test_multi_adam_state_round_trip():
    from gsdd_amd._optim import MultiAdam, unflatten
    g = torch.Generator().manual_seed(1)
    params = [("a", torch.randn(5, generator=g)), ("b", torch.randn(3, 7, generator=g)), ("c", torch.randn(4096 + 2, generator=g))]
    opt = MultiAdam(params, 1e-3, (0.9, 0.96), 1e-8, max_grad_norm=1.0, weight_decay=0.01, decay_mask={"a": False}, ema_decay=0.999,
                    skip_nonfinite=True)
    assert opt.staged and opt.n_blocks == 4 and opt.decays == [False, True, True] and list(opt.offs) == [0, 8, 32, 32 + 4100]
    words = opt.words.numpy()
    assert words.view("float32")[6] == 1.0 and words[7] == 1 and opt.skipped_steps == 0          # clip_coef 1, finite 1
    # the average starts from the parameters, padding zero
    avg = unflatten(opt.ema, [(n, p.shape) for n, p in params])
    assert all(torch.equal(avg[n], p) for n, p in params) and float(opt.ema[5:8].abs().sum()) == 0
    opt.m.copy_(torch.randn(opt.m.shape, generator=g))
    opt.v.copy_(torch.rand(opt.v.shape, generator=g))
    opt.ema.copy_(torch.randn(opt.ema.shape, generator=g))
    opt.step_count = 12
    opt.words.view(torch.int64)[1] = 3
    st = opt.state()
    assert set(st) == {"m", "v", "step", "ema", "skipped_steps"} and st["step"] == 12 and st["skipped_steps"] == 3
    other = MultiAdam(params, 1e-3, (0.9, 0.96), 1e-8, ema_decay=0.999)
    other.load_state(st)
    assert all(torch.equal(getattr(other, k), getattr(opt, k)) for k in ("m", "v", "ema")) and other.step_count == 12 and other.skipped_steps == 3
    # a state from before the average existed: loads with a warning, the average starts from the current parameters
    legacy = {k: st[k] for k in ("m", "v", "step")}
    other.ema.fill_(7.0)
    with pytest.warns(UserWarning, match="no averaged weights"):
        other.load_state(legacy)
    assert all(torch.equal(unflatten(other.ema, [(n, p.shape) for n, p in params])[n], p) for n, p in params) and other.skipped_steps == 0
    # defaults: exactly the state and the table of before
    plain = MultiAdam(params, 1e-3, (0.5, 0.999), 1e-8)
    assert not plain.staged and plain.ema is None and plain.words is None and set(plain.state()) == {"m", "v", "step"}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain.load_state(legacy)                      # no average wanted: no warning
    t = plain._build_table({n: torch.zeros_like(p) for n, p in params})
    assert t.shape == (4, 5) and list(t[:, 4]) == [5, 21, 4096, 2]
    wide = opt._build_table({n: torch.zeros_like(p) for n, p in params})
    assert wide.shape == (4, 7) and list(wide[:, 6]) == [0, 1, 1, 1] and wide[3, 5] == opt.ema.data_ptr() + 4 * (32 + 4096)
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(weight_decay=-0.1), dict(ema_decay=1.0), dict(ema_decay=-0.5)):
        with pytest.raises(ValueError):
            MultiAdam(params, 1e-3, (0.5, 0.999), 1e-8, **kw)
    with pytest.raises(ValueError):
        other.load_state({**st, "ema": torch.zeros(3)})


def test_trainer_arguments_and_ema_context_misuse():
    import gsdd_amd
    from gsdd_amd.d3pm_train import D3PMTrainer, linear_warmup
    dm = tiny_model(1)
    plain = D3PMTrainer(dm)
    assert not plain._staged and not plain.has_ema and plain.last_grad_norm is None and plain.skipped_steps == 0
    with pytest.raises(gsdd_amd.GsddError, match="no averaged weights"):
        with plain.ema_weights():
            pass
    for kw in (dict(max_grad_norm=0), dict(weight_decay=-1.0), dict(ema_decay=1.0)):
        with pytest.raises(ValueError):
            D3PMTrainer(dm, **kw)
    tr = D3PMTrainer(dm, ema_decay=0.999, lr_schedule=linear_warmup(1e-3, 10))
    assert tr._staged and tr.has_ema and tr._next_step() == 1
    before = {k: v.clone() for k, v in dm.transformer.state_dict().items()}
    with tr.ema_weights():                            # before the first step the average is the parameters: nothing is exchanged
        with pytest.raises(gsdd_amd.GsddError, match="does not nest"):
            with tr.ema_weights():
                pass
        with pytest.raises(gsdd_amd.GsddError, match="inside ema_weights"):
            tr.step(torch.zeros(1, 32, dtype=torch.long), torch.zeros(1, 1, 512))
        with pytest.raises(gsdd_amd.GsddError):
            tr.optimizer_state()
    with tr.ema_weights():                            # the flag is cleared on the way out, errors inside included
        pass
    assert all(torch.equal(v, before[k]) for k, v in dm.transformer.state_dict().items())
    sd = tr.ema_state_dict()
    assert set(sd) == set(before) and all(torch.equal(sd[k], before[k]) and not sd[k].is_cuda for k in sd)
    # a pending state moves the schedule's step
    tr.load_optimizer_state({"m": torch.zeros(1), "v": torch.zeros(1), "step": 41, "skipped_steps": 2})
    assert tr._next_step() == 42 and tr.skipped_steps == 2
    assert D3PMTrainer(dm, skip_nonfinite=True)._staged and D3PMTrainer(dm, weight_decay=0.01)._staged


def test_config_keys_and_the_native_step_guard(monkeypatch):
    from gsdd_amd.hydra_lite import compose
    from src.models.multistage_text_motion_model import NATIVE_OPTIM_DEFAULTS, check_native_optim
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    for top, flags in (("train.yaml", ["model=discrete_diffusion"]), ("eval.yaml", [])):
        m = compose(os.path.join(REPO, "configs"), top, flags).model
        assert dict(m.native_optim) == NATIVE_OPTIM_DEFAULTS and m.sample_with_ema is True and m.use_ema is False and m.native_step is False
    m = compose(os.path.join(REPO, "configs"), "train.yaml",
                ["model=discrete_diffusion", "model.native_step=true", "model.native_optim.max_grad_norm=1.0", "model.native_optim.weight_decay=0.045",
                 "model.native_optim.betas=[0.9,0.96]", "model.native_optim.ema_decay=0.99", "model.native_optim.skip_nonfinite=true",
                 "model.native_optim.warmup_steps=5000", "model.sample_with_ema=false"]).model
    got = check_native_optim(dict(m.native_optim), m.native_step)
    assert got == {"max_grad_norm": 1.0, "weight_decay": 0.045, "betas": [0.9, 0.96], "ema_decay": 0.99, "skip_nonfinite": True,
                   "warmup_steps": 5000} and m.sample_with_ema is False
    assert check_native_optim(None, False) == NATIVE_OPTIM_DEFAULTS == check_native_optim(dict(NATIVE_OPTIM_DEFAULTS), False)
    for key, val in (("max_grad_norm", 1.0), ("weight_decay", 0.01), ("betas", [0.9, 0.96]), ("ema_decay", 0.99), ("skip_nonfinite", True),
                     ("warmup_steps", 10)):
        with pytest.raises(ValueError, match=f"native_optim.{key} is set but native_step is false"):
            check_native_optim({key: val}, False)
        assert check_native_optim({key: val}, True)[key] == val
    with pytest.raises(ValueError, match="unknown keys"):
        check_native_optim({"clip": 1.0}, True)


def test_use_ema_names_the_missing_key():
    from src.models.multistage_text_motion_model import MultistageTextMotionModel

    class Gen(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.diffusion_model = tiny_model(1)

    gen = Gen()
    model = MultistageTextMotionModel(generator=gen, autoencoder=torch.nn.Identity(), generator_losses=False, use_ema=True)
    with pytest.raises(KeyError, match=r'checkpoint\["gsdd"\]\["native_adam"\]\["ema"\]'):
        model.load_ema_weights({"gsdd": {"native_adam": {"m": torch.zeros(1), "v": torch.zeros(1), "step": 1}}})
    with pytest.raises(KeyError, match="native_adam"):
        model.load_ema_weights({})
    # a checkpoint that has them: the averaged values land in the transformer
    from gsdd_amd._optim import flat_offsets
    tr = gen.diffusion_model.transformer
    n = int(flat_offsets([p.numel() for p in tr.parameters()])[-1])
    flat = torch.arange(n, dtype=torch.float32) * 1e-6
    model.load_ema_weights({"gsdd": {"native_adam": {"ema": flat}}})
    first = next(iter(tr.parameters()))
    assert torch.equal(first.detach().reshape(-1), flat[:first.numel()])
    with pytest.raises(ValueError, match="native_optim.ema_decay is set but native_step is false"):
        MultistageTextMotionModel(generator=gen, autoencoder=torch.nn.Identity(), generator_losses=False, native_optim={"ema_decay": 0.99})


def test_symbols_are_declared_exported_and_bound():
    import gsdd_amd
    with open(os.path.join(REPO, "include", "gsdd.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert s in gsdd_amd.EXPORTS and header.count(f"int {s}(") == 1, s
    assert header.count("} gsdd_optim_state;") == 1 and "never rewritten" in header.lower()
    S = gsdd_amd._lib.OptimState
    assert [n for n, _ in S._fields_] == ["step", "skipped_steps", "lr", "grad_norm", "clip_coef", "finite"] and ctypes.sizeof(S) == 32
    assert (S.lr.offset, S.grad_norm.offset, S.clip_coef.offset, S.finite.offset) == (16, 20, 24, 28)
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    assert all(s in doc for s in SYMBOLS)
    if os.path.exists(gsdd_amd.LIB_PATH):
        L = gsdd_amd.lib()                              # (lib() checks sizeof(gsdd_optim_state) against gsdd_abi_sizeof(8))
        assert L.gsdd_version() >= 110 and L.gsdd_abi_sizeof(8) == 32 and L.gsdd_abi_sizeof(6) == -1
        assert all(hasattr(L, s) for s in SYMBOLS)
        # argument errors come back before any device call
        for rc in (L.gsdd_grad_sqnorm(None, 4, None, None), L.gsdd_swap_multi(None, 1, None),
                   L.gsdd_grad_norm_finalize(ctypes.c_void_p(256), 4, 0.0, 1, ctypes.c_void_p(512), None),
                   L.gsdd_adamw_ema_multi(ctypes.c_void_p(256), 0, 0.9, 0.96, 1e-8, 0.0, 0.0, ctypes.c_void_p(512), None),
                   L.gsdd_adamw_ema_multi(ctypes.c_void_p(256), 4, 0.9, 0.96, 1e-8, -1.0, 0.0, ctypes.c_void_p(512), None),
                   L.gsdd_adamw_ema_multi(ctypes.c_void_p(256), 4, 0.9, 0.96, 1e-8, 0.0, 1.0, ctypes.c_void_p(512), None)):
            assert rc == -1 and L.gsdd_last_error()
