"""Host side of the native CLIP image tower (gsdd_amd.vision.ClipVisionTower) and of CLIPSIM: the fp64 restatement the GPU tests use as
their reference reproduces the fixture and the library, its preprocessing is torch's bicubic, the two weight layouts give identical
operands, the checkpoint helper picks exactly the image tower, the metric agrees with numpy, the evaluator without a scorer is the old
one, the contract errors are raised, and every fault the GPU tests are there to catch moves the outputs they check by at least 10 x
the bound that guards it (the figures are quoted in tests/golden/make_golden_clip_vision.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gsdd_amd
from gsdd_amd.checkpoint import extract_clip_text_tower, extract_clip_vision_tower
from gsdd_amd.metrics import clip_similarity
from gsdd_amd.vision import ClipVisionTower, hf_to_openai_vision_state_dict
from clip_vision_ref import (attention_inputs, attention_ref, bicubic_matrix, frame_patches_ref, make_clips, preprocess_ref, preprocess_torch, quantised_levels,
                             tower_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsdd_clip_frame_patches", "gsdd_clip_vision_embed", "gsdd_clip_attention")
PATCH_CASES = [(8, 8, 8), (16, 56, 8), (56, 56, 8), (128, 224, 32), (37, 64, 32)]          # (H, R, P) of the GPU test


def _fixture(golden):
    sd, a, cfg = golden("clip_vision_small")
    pixels = torch.from_numpy(a["pixels_x32"]).float() / 32
    return sd, pixels, torch.from_numpy(a["want"]), 4.0 * float(a["ref_fp32_err"]), cfg


def test_restatement_reproduces_the_fixture(golden):
    sd, pixels, want, bound, cfg = _fixture(golden)
    assert pixels.shape == (6, 3, 56, 56) and want.shape == (6, 32) and want.dtype == torch.float64 and 0 < bound < 1e-4
    assert cfg["image_size"] == 56 and cfg["patch_size"] == 8 and sd["vision_model.embeddings.position_embedding.weight"].shape == (50, 128)
    assert (tower_ref(sd, pixels, cfg["n_head"]) - want).abs().max().item() <= 1e-12
    # a frame alone gives the same row
    assert (tower_ref(sd, pixels[4:5], cfg["n_head"]) - want[4:5]).abs().max().item() <= 1e-12


def test_restatement_matches_a_fresh_library_tower():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPVisionConfig(hidden_size=64, intermediate_size=96, projection_dim=24, num_hidden_layers=3, num_attention_heads=2,
                                        image_size=24, patch_size=4, hidden_act="quick_gelu")
    torch.manual_seed(3)
    m = transformers.CLIPVisionModelWithProjection(cfg).eval().double()
    px = torch.randn((3, 3, 24, 24), dtype=torch.float64)
    with torch.no_grad():
        want = m(pixel_values=px).image_embeds
    assert (tower_ref(m.state_dict(), px, 2) - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("H,R,P", PATCH_CASES)
def test_preprocessing_is_torchs_bicubic(H, R, P):
    clips = make_clips(2, 3, H, seed=H + R)
    lv = quantised_levels(clips)
    assert lv.dtype == torch.float32 and torch.equal(lv, lv.round()) and lv.min() == 0 and lv.max() == 255
    raw = clips * torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1, 1) + torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1, 1)
    assert (raw < 0).float().mean() > 0.02 and (raw > 1).float().mean() > 0.02             # the quantiser's clamp is exercised both ways
    got = preprocess_ref(clips, R)
    want = preprocess_torch(clips, R, dtype=torch.float64)
    assert got.shape == (6, 3, R, R) and (got - want).abs().max().item() <= 1e-12
    unclamped = bicubic_matrix(H, R) @ (lv[0, :, 0].double() / 255 @ bicubic_matrix(H, R).t())
    if H < R:                                                                              # the checkerboard overshoots and is clamped
        assert unclamped.min() < -0.01 and unclamped.max() > 1.01
    else:                                                                                  # every fraction is 0: the quantised frame itself
        assert torch.equal(preprocess_ref(clips, R, normalise=False), (lv.double() / 255).permute(0, 2, 1, 3, 4).reshape(6, 3, H, H))
    rows = frame_patches_ref(clips, R, P)
    G = R // P
    assert rows.shape == (6 * G * G, 3 * P * P)
    # row (n, gy, gx), element (c, py, px)
    n, gy, gx, c, py, px = 4, G - 1, 0, 2, P - 1, 1
    assert rows[(n * G + gy) * G + gx, (c * P + py) * P + px] == got[n, c, gy * P + py, gx * P + px]
    # the patch embedding as a linear over these rows is the convolution
    w = torch.randn((5, 3, P, P), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    conv = F.conv2d(got, w, stride=P).flatten(2).transpose(1, 2).reshape(6 * G * G, 5)
    assert (rows @ w.reshape(5, -1).t() - conv).abs().max().item() <= 1e-11


def _operands(t):
    out = {k: getattr(t, k) for k in ClipVisionTower._VECTORS}
    for i, lay in enumerate(t.layers):
        out.update({f"{i}.{k}": v for k, v in lay.items()})
    return out


def test_both_weight_layouts_give_identical_operands(golden):
    sd, pixels, want, bound, cfg = _fixture(golden)
    hf = ClipVisionTower.from_hf_state_dict(sd, cfg["n_head"])
    oa_sd = hf_to_openai_vision_state_dict(sd)
    assert oa_sd["visual.proj"].shape == (128, 32) and oa_sd["visual.transformer.resblocks.1.attn.in_proj_weight"].shape == (384, 128)
    assert oa_sd["visual.conv1.weight"].shape == (128, 3, 8, 8) and all(k.startswith("visual.") for k in oa_sd)
    # the text tower and the scalars travel in the same dict and are ignored
    oa_sd.update({"token_embedding.weight": torch.zeros(4, 4), "transformer.resblocks.0.ln_1.weight": torch.ones(4), "logit_scale": torch.tensor(1.0)})
    oa = ClipVisionTower.from_openai_state_dict(oa_sd)
    assert oa.n_head == hf.n_head == 2 and len(oa.layers) == len(hf.layers) == 2
    assert (hf.patch, hf.grid, hf.seq, hf.resolution, hf.width) == (8, 7, 50, 56, 128)
    ho, oo = _operands(hf), _operands(oa)
    assert set(ho) == set(oo)
    for k in ho:
        assert ho[k].dtype == torch.float32 and ho[k].is_contiguous() and oo[k].is_contiguous() and torch.equal(ho[k], oo[k]), k
    assert hf.patch_w.shape == (128, 192) and torch.equal(hf.patch_w, sd["vision_model.embeddings.patch_embedding.weight"].reshape(128, 192))
    assert torch.equal(hf.layers[0]["wqkv"][128:256], sd["vision_model.encoder.layers.0.self_attn.k_proj.weight"])
    assert hf.proj.shape == (32, 128)
    # fp16 storage (the clip package's default) is widened: the operands are the fp32 images of the halves
    half = ClipVisionTower.from_openai_state_dict({k: v.half() for k, v in oa_sd.items()})
    for k, v in _operands(half).items():
        assert v.dtype == torch.float32, k
    assert torch.equal(half.proj, oa_sd["visual.proj"].half().float().t())
    assert torch.equal(half.layers[1]["wqkv"], oa_sd["visual.transformer.resblocks.1.attn.in_proj_weight"].half().float())


def test_extract_clip_vision_tower_picks_exactly_the_visual_keys(golden):
    sd, pixels, want, bound, cfg = _fixture(golden)
    oa_sd = hf_to_openai_vision_state_dict(sd)
    state = {"textencoder.clip_model." + k: v for k, v in oa_sd.items()}
    state.update({"generator.transformer.blocks.0.ln1.weight": torch.ones(4), "textencoder.clip_model.token_embedding.weight": torch.ones(2, 2),
                  "textencoder.clip_model.transformer.resblocks.0.ln_1.weight": torch.ones(4), "textencoder.clip_model.logit_scale": torch.tensor(1.0),
                  "textencoder.clip_model.text_projection": torch.ones(4, 4), "textencoder.embed_text.weight": torch.ones(4, 4)})
    for wrapped in (state, {"state_dict": state, "epoch": 3}):
        got = extract_clip_vision_tower(wrapped)
        assert set(got) == set(oa_sd) and all(torch.equal(got[k], oa_sd[k]) for k in oa_sd)
    assert set(extract_clip_vision_tower({"generator." + k: v for k, v in state.items()})) == set(oa_sd)
    assert extract_clip_vision_tower({k: v for k, v in state.items() if ".visual." not in k}) is None
    assert extract_clip_vision_tower({"generator.x": torch.ones(1)}) is None
    # the text helper keeps leaving the image tower out, and the checkpoint loader keeps dropping both
    assert not any(k.startswith("visual.") for k in extract_clip_text_tower(state))
    t = ClipVisionTower.from_openai_state_dict(extract_clip_vision_tower(state))
    assert torch.equal(t.proj, sd["visual_projection.weight"])
    from gsdd_amd.checkpoint import _is_dead
    assert all(_is_dead(k) for k in state if k.startswith("textencoder."))


def test_clip_similarity_agrees_with_numpy():
    rng = np.random.default_rng(0)
    t, f = rng.standard_normal((5, 16)), rng.standard_normal((5, 7, 16)) * 3.0
    f[2] = t[2][None] * 4.0                                        # every frame parallel to the caption: 1
    f[3] = -t[3][None]                                             # antiparallel: -1
    want = np.mean(np.einsum("bte,be->bt", f, t) / (np.linalg.norm(f, axis=-1) * np.linalg.norm(t, axis=-1)[:, None]), axis=1)
    got = clip_similarity(torch.from_numpy(t).float(), torch.from_numpy(f).float())
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,)
    want32 = np.mean(np.einsum("bte,be->bt", f.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64))
                     / (np.linalg.norm(f.astype(np.float32).astype(np.float64), axis=-1)
                        * np.linalg.norm(t.astype(np.float32).astype(np.float64), axis=-1)[:, None]), axis=1)
    assert np.abs(got.numpy() - want32).max() <= 1e-14
    assert np.abs(clip_similarity(t, f).numpy() - want).max() <= 1e-14
    assert abs(got[2].item() - 1.0) <= 1e-7 and abs(got[3].item() + 1.0) <= 1e-7 and got.abs().max() <= 1 + 1e-12
    with pytest.raises(ValueError):
        clip_similarity(torch.zeros(5, 16), torch.zeros(4, 7, 16))
    assert "100" in clip_similarity.__doc__ and "[-1, 1]" in clip_similarity.__doc__


def test_evaluator_without_a_scorer_returns_the_old_dict(monkeypatch):
    import src  # noqa: F401
    from src.utils.evaluator import ClipSimScorer, Evaluator, MeanPoolEncoder
    # (the FVD side's resize is a HIP kernel; on the host the features are taken from the clips as they are)
    monkeypatch.setattr(Evaluator, "_prepare", lambda self, clips: clips.float())
    g = torch.Generator().manual_seed(0)
    batches = [({"video": torch.randn((4, 3, 4, 16, 16), generator=g), "text": [f"caption {i}" for i in range(4)]},
                torch.randn((4, 3, 4, 16, 16), generator=g)) for _ in range(3)]
    ev = Evaluator("cpu", MeanPoolEncoder(grid=2), target_resolution=32)
    assert ev.clip_scorer is None
    for i, (batch, out) in enumerate(batches):
        ev.push_vals(batch, i, out)
    plain = ev.evaluate_metrics()
    assert set(plain) == {"fvd"} and ev.all_clip_scores == []

    # a scorer made of stand-ins (the metric and the plumbing run on the host; the native tower itself needs a GPU)
    seen = []

    def text_embedder(texts):
        seen.append(list(texts))
        return torch.ones((len(texts), 6))

    def vision_tower(clips):
        return clips.float().mean(dim=(3, 4)).permute(0, 2, 1).repeat(1, 1, 2)             # (B, T, 6)

    ev2 = Evaluator("cpu", MeanPoolEncoder(grid=2), target_resolution=32, clip_scorer=ClipSimScorer(text_embedder, vision_tower))
    for i, (batch, out) in enumerate(batches):
        ev2.push_vals(batch, i, out)
    both = ev2.evaluate_metrics()
    assert set(both) == {"fvd", "clipsim"} and both["fvd"] == plain["fvd"] and seen == [b["text"] for b, _ in batches]
    want = torch.cat([clip_similarity(torch.ones((4, 6)), vision_tower(out)) for _, out in batches]).mean().item()
    assert both["clipsim"] == want and -1 <= want <= 1
    ev2.reset()
    assert ev2.all_clip_scores == [] and ev2.all_video_embeds_gt == []


def test_scorer_helper_builds_both_towers_from_one_local_directory(tmp_path):
    transformers = pytest.importorskip("transformers")
    import src  # noqa: F401
    from src.utils.evaluator import ClipSimScorer, clip_scorer_from_pretrained
    chars = [chr(c) for c in range(ord("a"), ord("z") + 1)]
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 26 + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 52, 53
    transformers.CLIPTokenizer(vocab=vocab, merges=[]).save_pretrained(tmp_path)
    tc = dict(vocab_size=54, hidden_size=64, intermediate_size=64, projection_dim=16, num_hidden_layers=1, num_attention_heads=2,
              max_position_embeddings=77, bos_token_id=52, eos_token_id=53, pad_token_id=0)
    vc = dict(hidden_size=64, intermediate_size=64, projection_dim=16, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8)
    torch.manual_seed(0)
    m = transformers.CLIPModel(transformers.CLIPConfig(text_config=tc, vision_config=vc, projection_dim=16)).eval()
    m.save_pretrained(tmp_path)
    s = clip_scorer_from_pretrained(str(tmp_path), device="cpu")
    assert isinstance(s, ClipSimScorer) and isinstance(s.vision_tower, ClipVisionTower)
    t = s.vision_tower
    assert (t.patch, t.seq, t.resolution, t.n_head, len(t.layers)) == (8, 17, 32, 2, 2)
    assert torch.equal(t.proj, m.visual_projection.weight.detach()) and torch.equal(t.class_emb, m.vision_model.embeddings.class_embedding.detach())
    text = s.text_embedder(["ab", "c"])                                                    # the text side answers on the host as PyTorch
    assert tuple(text.shape) == (2, 16)
    with pytest.raises(gsdd_amd.GsddError, match="no CPU fallback"):                       # the image side has no host path
        s(["ab", "c"], torch.zeros((2, 3, 2, 16, 16)))
    with pytest.raises(FileNotFoundError):
        clip_scorer_from_pretrained(str(tmp_path / "missing"))


def test_contract_errors(golden):
    sd, pixels, want, bound, cfg = _fixture(golden)
    tower = ClipVisionTower.from_hf_state_dict(sd, cfg["n_head"])
    with pytest.raises(gsdd_amd.GsddError, match="square"):
        tower.forward(torch.zeros((1, 3, 2, 16, 24)))                                      # H != W
    with pytest.raises(gsdd_amd.GsddError, match="larger than the tower's resolution 56"):
        tower.forward(torch.zeros((1, 3, 2, 64, 64)))                                      # H > R
    with pytest.raises(gsdd_amd.GsddError):
        tower.forward(torch.zeros((1, 4, 2, 16, 16)))
    with pytest.raises(gsdd_amd.GsddError, match="no CPU fallback"):                       # a tower on the host cannot run
        tower.forward(torch.zeros((1, 3, 2, 16, 16)))
    with pytest.raises(gsdd_amd.GsddError, match="no CPU fallback"):
        tower.forward_pixels(pixels)
    with pytest.raises(gsdd_amd.GsddError, match="pixel_values"):
        tower.forward_pixels(torch.zeros((1, 3, 48, 48)))
    # a sequence above 77: ViT-B/16's 14 x 14 + 1 = 197 positions; 9 x 9 + 1 = 82 is the smallest square grid that does not fit
    for grid in (9, 14):
        big = dict(sd)
        big["vision_model.embeddings.position_embedding.weight"] = torch.zeros((grid * grid + 1, 128))
        with pytest.raises(gsdd_amd.GsddError, match="at most 77"):
            ClipVisionTower.from_hf_state_dict(big, cfg["n_head"])
    fits = dict(sd)
    fits["vision_model.embeddings.position_embedding.weight"] = torch.zeros((8 * 8 + 1, 128))                # 65 positions
    assert ClipVisionTower.from_hf_state_dict(fits, cfg["n_head"]).resolution == 64
    with pytest.raises(gsdd_amd.GsddError, match="QuickGELU"):
        ClipVisionTower.from_hf_state_dict(sd, cfg["n_head"], hidden_act="gelu")
    with pytest.raises(gsdd_amd.GsddError, match="head dimension"):
        ClipVisionTower.from_hf_state_dict(sd, 1)                                          # d = 128
    # the wrappers refuse the same shapes before anything reaches the library
    with pytest.raises(gsdd_amd.GsddError, match="H == W <= R"):
        gsdd_amd.ops.clip_frame_patches(torch.zeros((1, 3, 1, 16, 16)), 56, 16)            # R % P != 0


def test_injected_faults_move_the_fixture_rows(golden):
    """Every fault the whole-tower GPU test is there to catch moves EVERY frame's outputs by at least 10 x its bound (4 x ref_fp32_err)."""
    sd, pixels, want, bound, cfg = _fixture(golden)
    moved = {}
    for fault in ("tail_unmasked", "tail_off_by_one", "causal", "class_last", "patch_order", "no_pre_ln"):
        d = (tower_ref(sd, pixels, cfg["n_head"], fault=fault) - want).abs().amax(dim=1)
        moved[fault] = d.min().item()
        print(f"[fault] {fault}: moves the frames' outputs by {d.min().item():.3e} .. {d.max().item():.3e}, {d.min().item() / bound:.0f} x the bound {bound:.3e}")
    assert min(moved.values()) >= 10 * bound, (moved, bound)


@pytest.mark.parametrize("S", [17, 33, 50, 65, 77])
def test_injected_attention_faults_move_the_attention_tests_outputs(S):
    """The attention-alone GPU test's inputs (clip_vision_ref.attention_inputs): a kernel that leaves the tail of its last key
    tile unmasked, masks one key too many or keeps the causal mask misses that test's bound by at least 10 x."""
    for n_head, d in ((2, 64), (2, 16)):
        for hot in ("last", "first"):
            q, k, v = attention_inputs(3, S, n_head, d, hot)
            want = attention_ref(q, k, v, d ** -0.5)
            bound = 4.0 * (attention_ref(q, k, v, d ** -0.5, dtype=torch.float32).double() - want).abs().max().item()
            for fault in ("tail_unmasked", "tail_off_by_one", "causal"):
                moved = (attention_ref(q, k, v, d ** -0.5, fault=fault) - want).abs().max().item()
                assert moved >= 10 * bound, (S, n_head, d, hot, fault, moved, bound)


def test_a_half_resize_moves_the_patch_rows():
    """PIL's a = -0.5 in place of torch's -0.75 moves the patch rows of every upscaling case by at least 10 x that case's bound (4 x the
    error of torch's fp32 composite against fp64)."""
    for H, R, P in PATCH_CASES:
        clips = make_clips(2, 3, H, seed=H + R)
        want = frame_patches_ref(clips, R, P)
        bound = 4.0 * (preprocess_torch(clips, R).double() - preprocess_ref(clips, R)).abs().max().item()
        moved = (frame_patches_ref(clips, R, P, fault="a_half") - want).abs().max().item()
        print(f"[fault] a_half H={H} R={R}: moved {moved:.3e}, bound {bound:.3e}")
        if H < R:
            assert moved >= 10 * bound, (H, R, moved, bound)
        else:
            assert moved == 0.0                                    # nothing is interpolated at H == R (the GPU test asks for exactness)


def test_entry_points_are_declared_and_exported():
    with open(os.path.join(REPO, "include", "gsdd.h")) as f:
        header = f.read()
    L = gsdd_amd.lib()
    for sym in SYMBOLS:
        assert sym in gsdd_amd.EXPORTS and f"int {sym}(" in header, sym
        assert hasattr(L, sym), sym
    assert "a = -0.75" in header and "NOT PIL's" in header
    for name in ("clip_frame_patches", "clip_vision_embed", "clip_attention"):
        assert callable(getattr(gsdd_amd.ops, name))
    assert gsdd_amd.ClipVisionTower is ClipVisionTower
