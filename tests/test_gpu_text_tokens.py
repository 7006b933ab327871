"""Per-token text conditioning from the native CLIP text tower: ClipTextTower.forward(tokens=True), CLIPTextEmbedding(per_token=True)
and the generator glue that carries a (B, Te, C) condition through one training forward and the sampler.

Tower: the seeded tower of tests/golden/clip_text_small.npz (tests/golden/make_golden_clip_text.py) rebuilt as a `transformers` module;
tokens=True returns the final-LayerNorm row of every position that ran -- `last_hidden_state[:, :S]`, no pooling, no projection.
Reference: that module in fp64.  Bound: 4 x the error of the same module in fp32 against fp64 on the same rows, measured here (as
`ref_fp32_err` is for the pooled output: another summation order plus the dropped terms of the bf16 x 3 split in the linears)."""
import pytest
import torch
import transformers

import gsdd_amd
from gsdd_amd.text import ClipTextTower
from conftest import load_golden, parity_report

pytestmark = pytest.mark.gpu

CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=128, projection_dim=32, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=77, hidden_act="quick_gelu", bos_token_id=62, eos_token_id=63, pad_token_id=0)


@pytest.fixture(scope="module")
def fixture_tower():
    sd, a, cfg = load_golden("clip_text_small")
    ids = torch.from_numpy(a["ids"])
    m = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**CFG)).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        h32 = m.text_model(input_ids=ids, attention_mask=None).last_hidden_state.double()
        h64 = m.double().text_model(input_ids=ids, attention_mask=None).last_hidden_state
    tower = ClipTextTower.from_hf_state_dict(sd, cfg["n_head"]).cuda()
    return {"ids": ids, "want": h64, "ref32": h32, "tower": tower, "pooled_want": torch.from_numpy(a["want"]),
            "pooled_bound": 4.0 * float(a["ref_fp32_err"])}


@pytest.mark.parametrize("rows,width", [(8, 77), (5, 32), (2, 8)], ids=["S77", "S22", "S3"])
def test_token_features_match_transformers_fp64(fixture_tower, rows, width):
    f = fixture_tower
    ids = f["ids"][:rows, :width].contiguous()
    S = int(ids.argmax(dim=1).max()) + 1                            # the positions the tower runs (trimmed to the longest caption)
    before = f["tower"](ids)
    got = f["tower"](ids, tokens=True)
    after = f["tower"](ids)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (rows, S, 128)
    want = f["want"][:rows, :S]
    ref_err = (f["ref32"][:rows, :S] - want).abs().max().item()
    bound = 4.0 * ref_err
    err = (got.cpu().double() - want).abs().max().item()
    untrimmed = f["tower"](ids, tokens=True, trim=False)
    assert tuple(untrimmed.shape) == (rows, width, 128)
    err_untrimmed = (untrimmed.cpu().double() - f["want"][:rows, :width]).abs().max().item()
    bound_untrimmed = 4.0 * (f["ref32"][:rows, :width] - f["want"][:rows, :width]).abs().max().item()
    parity_report(f"text_tokens_S{S}", {"err": err, "bound": bound, "ref_fp32_err": ref_err, "max_abs_want": want.abs().max().item(),
                                        "err_untrimmed": err_untrimmed, "bound_untrimmed": bound_untrimmed})
    assert 0 < ref_err and err <= bound, (err, bound)
    assert err_untrimmed <= bound_untrimmed, (err_untrimmed, bound_untrimmed)
    # the default call is what it was: the same bits before and after a tokens=True call, inside the pooled output's own bound
    assert torch.equal(before, after)
    assert (before.cpu().double() - f["pooled_want"][:rows]).abs().max().item() <= f["pooled_bound"]


def byte_level_provider(tmp_path, hidden, heads, **kw):
    """A CLIPTextEmbedding on a small seeded tower with a byte-level vocabulary, saved to and loaded from tmp_path (nothing is fetched)."""
    import src  # noqa: F401
    from src.models.text_models.clip_text_embedding import CLIPTextEmbedding
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b); cs.append(256 + n); n += 1
    chars = [chr(c) for c in cs]
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 256 + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 512, 513
    transformers.CLIPTokenizer(vocab=vocab, merges=[]).save_pretrained(tmp_path)
    cfg = transformers.CLIPTextConfig(vocab_size=514, hidden_size=hidden, intermediate_size=2 * hidden, projection_dim=hidden,
                                      num_hidden_layers=2, num_attention_heads=heads, max_position_embeddings=77, bos_token_id=512,
                                      eos_token_id=513, pad_token_id=0)
    torch.manual_seed(0)
    transformers.CLIPTextModelWithProjection(cfg).save_pretrained(tmp_path)
    return CLIPTextEmbedding(clip_dim=hidden, weights=str(tmp_path), **kw)


TEXTS = ["a dog runs", "x" * 40, "", "two people dance in a kitchen", "b", "the quick brown fox", "jumps over", "lazy dogs"]


def test_provider_returns_22_token_rows(tmp_path):
    p = byte_level_provider(tmp_path, 32, 2, per_token=True)
    ids = p.tokenize(TEXTS)
    with torch.no_grad():
        h32 = p.clip_model.text_model(input_ids=ids, attention_mask=None).last_hidden_state[:, :22].double()
        cpu = p(TEXTS)                                              # the PyTorch path where the module lives
        want = p.clip_model.double().text_model(input_ids=ids, attention_mask=None).last_hidden_state[:, :22]
        p.clip_model.float()
    assert tuple(cpu.shape) == (8, 22, 32) and torch.equal(cpu.double(), h32)
    ref_err = (h32 - want).abs().max().item()
    bound = 4.0 * ref_err
    p = p.cuda()
    got = p(TEXTS)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (8, 22, 32)
    assert max(p._tower._buffers)[1] == 22                          # untrimmed: always the recipe's 22 positions
    err = (got.cpu().double() - want).abs().max().item()
    # a caption's rows do not depend on which other captions share the batch (nor on their lengths): every call runs the same 22
    # positions, so each row is computed from the same operands in the same order -- bit for bit
    singles = [p([t])[0] for t in TEXTS]
    other = p([TEXTS[4], TEXTS[1]])
    alone = max((s_ - got[i]).abs().max().item() for i, s_ in enumerate(singles))
    pair = (other[0] - got[4]).abs().max().item()
    assert tuple(p(["b"]).shape) == (1, 22, 32)
    parity_report("text_tokens_provider", {"err": err, "bound": bound, "ref_fp32_err": ref_err, "diff_caption_alone_vs_batch": alone,
                                           "diff_caption_in_another_batch": pair})
    assert 0 < ref_err and err <= bound, (err, bound)
    assert all(torch.equal(s_, got[i]) for i, s_ in enumerate(singles)), alone
    assert torch.equal(other[0], got[4]) and torch.equal(other[1], got[1]), pair
    # the pooled provider on the same tower is unchanged by the flag's existence
    pooled = byte_level_provider(tmp_path, 32, 2).cuda()(TEXTS)
    assert tuple(pooled.shape) == (8, 32)
    with pytest.raises(gsdd_amd.GsddError):
        from src.models.text_models.clip_text_embedding import CLIPTextEmbedding
        CLIPTextEmbedding(clip_dim=32, per_token=True)(TEXTS)       # the hash embedding has no tokens


def test_generator_trains_and_samples_on_token_conditions(tmp_path, golden):
    """DiscreteDiffusion with a per-token provider and zero_text_emb=False at L = 64: one training forward (+ backward through the
    bridge) and sample_videos run on a (B, 22, cond_dim) condition; losses, gradients and clips are finite."""
    from tests.test_gpu_glue import build
    gen, vq, batch, a, cfg, cfgd = build(gsdd_amd, golden, zero_text_emb=False)
    C = cfgd["cond_dim"]
    assert cfgd["L"] == 64 and C % 32 == 0
    provider = byte_level_provider(tmp_path, C, C // 16, per_token=True).cuda()
    gen = gsdd_amd.DiscreteDiffusion(provider, gen.diffusion_model, zero_text_emb=False)
    B = batch["video"].shape[0]
    batch = dict(batch, text=TEXTS[:B])
    emb = gen.get_text_embeddings(batch["text"])
    assert tuple(emb.shape) == (B, 22, C) and float(emb.abs().max()) > 0
    dm = gen.diffusion_model.train()
    dm.set_noise(5, stream=0)
    out = gen(batch, vq, None, do_inference=False)
    assert out["losses"].ndim == 0 and bool(torch.isfinite(out["losses"]))
    out["losses"].backward()
    grads = {n: p.grad for n, p in dm.transformer.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(grads[f"blocks.0.{n}"].abs().max()) > 0 for n in ("attn2.query.weight", "attn2.key.weight", "ln1_1.linear.weight"))
    dm.eval()
    with torch.no_grad():
        clips = gen.sample_videos(batch["text"], vq)
    tok = gen.last_content_token
    assert tuple(tok.shape) == (B, 64) and int(tok.min()) >= 0
    assert clips.shape == batch["video"].shape and bool(torch.isfinite(clips).all())
