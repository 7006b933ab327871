"""Host side of the native CLIP text tower (gsdd_amd.text.ClipTextTower): the fp64 restatement the GPU tests use as their reference
reproduces the fixture and the library, the two weight layouts give identical fused operands, the checkpoint helper picks exactly the
text tower, and the ABI declares and exports the new entry points."""
import os

import pytest
import torch

import gsdd_amd
from gsdd_amd.checkpoint import extract_clip_text_tower
from gsdd_amd.text import ClipTextTower, hf_to_openai_state_dict
from text_tower_ref import tower_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsdd_text_embed", "gsdd_text_attention", "gsdd_text_pool")


def test_restatement_reproduces_the_fixture(golden):
    sd, a, cfg = golden("clip_text_small")
    ids, want = torch.from_numpy(a["ids"]), torch.from_numpy(a["want"])
    assert ids.shape == (8, 77) and want.dtype == torch.float64 and 0 < float(a["ref_fp32_err"]) < 1e-4
    got = tower_ref(sd, ids, cfg["n_head"])
    assert (got - want).abs().max().item() <= 1e-12
    # context trimming changes nothing: rows 0..4 end before position 32
    assert (tower_ref(sd, ids[:5, :32], cfg["n_head"]) - want[:5]).abs().max().item() <= 1e-12


def test_restatement_matches_a_fresh_library_tower():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPTextConfig(vocab_size=50, hidden_size=64, intermediate_size=96, projection_dim=24, num_hidden_layers=3,
                                      num_attention_heads=2, max_position_embeddings=40, hidden_act="quick_gelu", bos_token_id=48,
                                      eos_token_id=49, pad_token_id=0)
    torch.manual_seed(3)
    m = transformers.CLIPTextModelWithProjection(cfg).eval().double()
    ids = torch.zeros((4, 40), dtype=torch.int64)
    for r, n in enumerate((2, 9, 17, 40)):
        ids[r, :n] = torch.cat([torch.tensor([48]), torch.randint(1, 48, (n - 2,)), torch.tensor([49])])
    with torch.no_grad():
        want = m(input_ids=ids).text_embeds
    got = tower_ref(m.state_dict(), ids, 2)
    assert (got - want).abs().max().item() <= 1e-12


def _operands(t):
    out = {k: getattr(t, k) for k in ("tok_emb", "pos_emb", "gf", "bf", "proj")}
    for i, lay in enumerate(t.layers):
        out.update({f"{i}.{k}": v for k, v in lay.items()})
    return out


def test_both_weight_layouts_give_identical_operands(golden):
    sd, a, cfg = golden("clip_text_small")
    hf = ClipTextTower.from_hf_state_dict(sd, cfg["n_head"])
    oa_sd = hf_to_openai_state_dict(sd)
    assert oa_sd["text_projection"].shape == (128, 32) and oa_sd["transformer.resblocks.1.attn.in_proj_weight"].shape == (384, 128)
    assert "positional_embedding" in oa_sd and not any(k.startswith("text_model.") for k in oa_sd)
    # the clip package's visual tower and scalars travel in the same dict and are ignored
    oa_sd.update({"visual.conv1.weight": torch.zeros(4, 3, 2, 2), "visual.transformer.resblocks.0.ln_1.weight": torch.ones(4),
                  "logit_scale": torch.tensor(1.0)})
    oa = ClipTextTower.from_openai_state_dict(oa_sd)
    assert oa.n_head == hf.n_head == 2 and len(oa.layers) == len(hf.layers) == 2
    ho, oo = _operands(hf), _operands(oa)
    assert set(ho) == set(oo)
    for k in ho:
        assert ho[k].dtype == torch.float32 and ho[k].is_contiguous() and oo[k].is_contiguous() and torch.equal(ho[k], oo[k]), k
    assert hf.layers[0]["wqkv"].shape == (384, 128) and torch.equal(hf.layers[0]["wqkv"][128:256],
                                                                    sd["text_model.encoder.layers.0.self_attn.k_proj.weight"])
    assert hf.proj.shape == (32, 128)
    # fp16 storage (the clip package's default) is widened: the operands are the fp32 images of the halves
    half = ClipTextTower.from_openai_state_dict({k: v.half() for k, v in oa_sd.items()})
    for k, v in _operands(half).items():
        assert v.dtype == torch.float32, k
    assert torch.equal(half.proj, oa_sd["text_projection"].half().float().t())
    assert torch.equal(half.layers[1]["wqkv"], oa_sd["transformer.resblocks.1.attn.in_proj_weight"].half().float())


def test_extract_clip_text_tower_picks_exactly_the_text_keys(golden):
    sd, a, cfg = golden("clip_text_small")
    oa_sd = hf_to_openai_state_dict(sd)
    state = {"textencoder.clip_model." + k: v for k, v in oa_sd.items()}
    state.update({"generator.transformer.blocks.0.ln1.weight": torch.ones(4), "generator.content_emb.emb.weight": torch.ones(2, 2),
                  "textencoder.clip_model.visual.conv1.weight": torch.zeros(4, 3, 2, 2),
                  "textencoder.clip_model.visual.transformer.resblocks.0.ln_1.weight": torch.ones(4),
                  "textencoder.clip_model.visual.proj": torch.ones(4, 4), "textencoder.clip_model.logit_scale": torch.tensor(1.0),
                  "textencoder.embed_text.weight": torch.ones(4, 4), "textencoder.embed_text.bias": torch.ones(4)})
    for wrapped in (state, {"state_dict": state, "epoch": 3}):
        got = extract_clip_text_tower(wrapped)
        assert set(got) == set(oa_sd)
        assert all(torch.equal(got[k], oa_sd[k]) for k in oa_sd)
    # the same tower as the reference's whole-model files carry it, under the generator
    nested = extract_clip_text_tower({"generator." + k: v for k, v in state.items()})
    assert set(nested) == set(oa_sd)
    assert extract_clip_text_tower({k: v for k, v in state.items() if not k.startswith("textencoder.clip_model.")}) is None
    assert extract_clip_text_tower({"generator.x": torch.ones(1)}) is None
    t = ClipTextTower.from_openai_state_dict(extract_clip_text_tower(state))
    assert torch.equal(t.proj, sd["text_projection.weight"])


def test_native_on_a_cpu_module_raises(tmp_path, golden):
    transformers = pytest.importorskip("transformers")
    import src  # noqa: F401
    from src.models.text_models.clip_text_embedding import CLIPTextEmbedding
    chars = [chr(c) for c in range(ord("a"), ord("z") + 1)]
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 26 + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 52, 53
    transformers.CLIPTokenizer(vocab=vocab, merges=[]).save_pretrained(tmp_path)
    cfg = transformers.CLIPTextConfig(vocab_size=54, hidden_size=64, intermediate_size=64, projection_dim=16, num_hidden_layers=1,
                                      num_attention_heads=2, max_position_embeddings=77, bos_token_id=52, eos_token_id=53, pad_token_id=0)
    torch.manual_seed(0)
    transformers.CLIPTextModelWithProjection(cfg).save_pretrained(tmp_path)
    with pytest.raises(gsdd_amd.GsddError):
        CLIPTextEmbedding(clip_dim=16, weights=str(tmp_path), native=True)(["ab"])
    p = CLIPTextEmbedding(clip_dim=16, weights=str(tmp_path))
    with pytest.raises(gsdd_amd.GsddError):
        p(["ab"], native=True)
    assert tuple(p(["ab", "c"]).shape) == (2, 16) and tuple(p(["ab"], native=False).shape) == (1, 16)     # the CPU path is untouched
    # a tower on the host cannot run either: there is no CPU fallback
    sd, a, gcfg = golden("clip_text_small")
    with pytest.raises(gsdd_amd.GsddError):
        ClipTextTower.from_hf_state_dict(sd, gcfg["n_head"]).forward(torch.from_numpy(a["ids"]))


def test_entry_points_are_declared_and_exported():
    with open(os.path.join(REPO, "include", "gsdd.h")) as f:
        header = f.read()
    L = gsdd_amd.lib()
    for sym in SYMBOLS:
        assert sym in gsdd_amd.EXPORTS and f"int {sym}(" in header, sym
        assert hasattr(L, sym), sym
    assert "clip.model.CLIP.encode_text" in header and "clip_text_embedding.py:56-65" in header
    for name in ("text_embed", "text_attention", "text_pool"):
        assert callable(getattr(gsdd_amd.ops, name))
