"""The native CLIP text tower on the GPU (csrc/text_tower.hip, gsdd_amd.text.ClipTextTower) against fp64.

Bounds.  Attention alone: 4 x the error of the same computation in fp32 with torch on the CPU against the same fp64 reference,
measured in the test (a different summation order may not cost more than that).  The whole tower: 4 x `ref_fp32_err` of the fixture
(tests/golden/make_golden_clip_text.py: the library's own fp32 error on these rows), read from the fixture; the factor covers another
summation order plus the dropped terms of the bf16 x 3 split in the linears."""
import numpy as np
import pytest
import torch

import gsdd_amd
from gsdd_amd import ops
from gsdd_amd.text import ClipTextTower, hf_to_openai_state_dict
from conftest import parity_report
from text_tower_ref import attention_ref, tower_ref

pytestmark = pytest.mark.gpu

S_LIST = [1, 2, 15, 16, 17, 22, 32, 33, 64, 77]
HEADS = [(1, 64), (2, 64), (8, 64), (2, 32)]
POISON = -777.0


@pytest.fixture(scope="module")
def fixture_tower():
    from conftest import load_golden
    sd, a, cfg = load_golden("clip_text_small")
    ids, want = torch.from_numpy(a["ids"]), torch.from_numpy(a["want"])
    bound = 4.0 * float(a["ref_fp32_err"])
    tower = ClipTextTower.from_hf_state_dict(sd, cfg["n_head"]).cuda()
    full = tower(ids).cpu().double()
    return {"sd": sd, "cfg": cfg, "ids": ids, "want": want, "bound": bound, "tower": tower, "full": full}


@pytest.mark.parametrize("n_head,d", HEADS)
@pytest.mark.parametrize("S", S_LIST)
def test_text_attention_against_fp64(S, n_head, d):
    B, C = 3, n_head * d
    g = torch.Generator().manual_seed(1000 * S + 10 * n_head + d)
    q, k, v = (torch.randn((B, S, n_head, d), generator=g) for _ in range(3))
    # per (batch, head) temperature: from near-uniform rows to rows dominated by one key (largest probability from ~0.1 to ~1)
    temp = torch.logspace(-0.5, 0.5, B * n_head).view(B, 1, n_head, 1)
    q, k = q * temp, k * temp
    scale = d ** -0.5
    qh, kh, vh = (t.transpose(1, 2) for t in (q, k, v))
    want = attention_ref(qh, kh, vh, scale)                                       # (B, H, S, d) fp64
    ref32 = attention_ref(qh, kh, vh, scale, dtype=torch.float32).double()
    bound = 4.0 * (ref32 - want).abs().max().item()
    pmax = torch.softmax((qh.double() * scale) @ kh.double().transpose(-1, -2)
                         + torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1), -1)[..., -1, :].amax(-1)
    pad = 16
    qkv = torch.full((B * S + pad, 3 * C), float("nan"))
    qkv[:B * S] = torch.cat([q.reshape(B * S, C), k.reshape(B * S, C), v.reshape(B * S, C)], dim=1)
    qkv = qkv.cuda()
    out = torch.full((B * S + pad, C), POISON, device="cuda")
    ops.text_attention(qkv[:B * S], B, S, n_head, out[:B * S], scale=scale)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[B * S:], torch.full((pad, C), POISON)), "rows behind B*S were written"
    got = got[:B * S].double().view(B, S, n_head, d).transpose(1, 2)
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    print(f"[text_attention] S={S} heads={n_head} d={d}: err {err:.3e} bound {bound:.3e} last-row pmax {pmax.min():.2f}..{pmax.max():.2f}")
    if (S, n_head, d) in ((77, 8, 64), (77, 2, 32), (22, 8, 64)):
        parity_report(f"text_attention_S{S}_h{n_head}_d{d}", {"err": err, "bound": bound, "ref_fp32_err": bound / 4})
    assert err <= bound, (err, bound)


def test_text_attention_rejects_bad_arguments():
    qkv = torch.zeros((78, 192), device="cuda")
    out = torch.full((78, 64), POISON, device="cuda")
    with pytest.raises(gsdd_amd.GsddError):
        ops.text_attention(qkv, 1, 78, 1, out)                     # S > 77
    with pytest.raises(gsdd_amd.GsddError):
        ops.text_attention(qkv[:8], 1, 8, 8, out[:8])              # head dimension 8
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((78, 64), POISON))


def test_text_embed_and_pool_are_exact():
    g = torch.Generator().manual_seed(7)
    B, S, pitch, C, vocab = 5, 19, 23, 72, 41                      # C no multiple of 64, S < pitch
    tok, pos = torch.randn((vocab, C), generator=g), torch.randn((S + 3, C), generator=g)
    ids = torch.randint(0, vocab, (B, pitch), generator=g)
    ids[0, 0], ids[1, 1] = 0, vocab - 1
    x = torch.full((B * S + 4, C), POISON, device="cuda")
    ops.text_embed(ids.cuda(), tok.cuda(), pos.cuda(), x[:B * S], S, ids_host=ids)
    want = (tok[ids[:, :S]] + pos[:S]).reshape(B * S, C)
    got = x.cpu()
    assert torch.equal(got[:B * S], want) and torch.equal(got[B * S:], torch.full((4, C), POISON))
    eot = torch.tensor([0, S - 1, 3, 7, S - 1])
    pooled = torch.full((B + 1, C), POISON, device="cuda")
    ops.text_pool(x[:B * S], eot.cuda(), B, S, pooled[:B], eot_host=eot)
    got = pooled.cpu()
    assert torch.equal(got[:B], want.view(B, S, C)[torch.arange(B), eot]) and torch.equal(got[B], torch.full((C,), POISON))


def test_text_embed_and_pool_reject_out_of_range_before_any_launch():
    B, S, C, vocab = 2, 6, 16, 10
    tok, pos = torch.ones((vocab, C), device="cuda"), torch.ones((S, C), device="cuda")
    for bad in (vocab, -1, 2 ** 40):
        ids = torch.zeros((B, S), dtype=torch.int64)
        ids[1, 4] = bad
        x = torch.full((B * S, C), POISON, device="cuda")
        with pytest.raises(gsdd_amd.GsddError, match="vocabulary"):
            ops.text_embed(ids.cuda(), tok, pos, x, S, ids_host=ids)
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), torch.full((B * S, C), POISON))        # nothing was launched
    x = torch.ones((B * S, C), device="cuda")
    for bad in (S, -1):
        eot = torch.tensor([1, bad])
        pooled = torch.full((B, C), POISON, device="cuda")
        with pytest.raises(gsdd_amd.GsddError, match="outside"):
            ops.text_pool(x, eot.cuda(), B, S, pooled, eot_host=eot)
        torch.cuda.synchronize()
        assert torch.equal(pooled.cpu(), torch.full((B, C), POISON))
    with pytest.raises(gsdd_amd.GsddError):                                # more positions than the position table has
        ops.text_embed(torch.zeros((B, S + 1), dtype=torch.int64, device="cuda"), tok, pos, torch.empty((B * (S + 1), C), device="cuda"), S + 1)
    # the tower checks the ids it is given the same way
    with pytest.raises(gsdd_amd.GsddError):
        ops.text_embed(torch.zeros((B, S), dtype=torch.int32, device="cuda"), tok, pos, x, S)


def test_text_kernels_guard_ids_they_cannot_check_on_the_host():
    """Without the host copy the entry points cannot see the values; the kernels then read nothing out of range and mark the row."""
    B, S, C, vocab = 2, 4, 8, 5
    tok = torch.arange(vocab * C, dtype=torch.float32).view(vocab, C)
    pos = torch.zeros((S, C))
    ids = torch.tensor([[0, 1, 2, 3], [4, 99, -3, 0]])
    x = torch.empty((B * S, C), device="cuda")
    ops.text_embed(ids.cuda(), tok.cuda(), pos.cuda(), x, S)
    got = x.cpu().view(B, S, C)
    bad = torch.zeros((B, S), dtype=torch.bool)
    bad[1, 1] = bad[1, 2] = True
    assert torch.isnan(got[bad]).all() and torch.equal(got[~bad], tok[ids[~bad]])
    pooled = torch.empty((B, C), device="cuda")
    ops.text_pool(x, torch.tensor([3, S + 2]).cuda(), B, S, pooled)
    got = pooled.cpu()
    assert torch.equal(got[0], tok[3]) and torch.isnan(got[1]).all()


def test_tower_on_the_fixture(fixture_tower):
    f = fixture_tower
    err = (f["full"] - f["want"]).abs().max().item()
    ref = tower_ref(f["sd"], f["ids"], f["cfg"]["n_head"])
    assert (ref - f["want"]).abs().max().item() <= 1e-12
    # the clip package's key layout gives the same operands, hence the same bits
    oa = ClipTextTower.from_openai_state_dict(hf_to_openai_state_dict(f["sd"])).cuda()
    same = torch.equal(oa(f["ids"]).cpu().double(), f["full"])
    untrimmed = (f["tower"](f["ids"][:5], trim=False).cpu().double() - f["want"][:5]).abs().max().item()
    parity_report("text_tower_fixture", {"err": err, "bound": f["bound"], "ref_fp32_err": f["bound"] / 4, "max_abs_want": f["want"].abs().max().item(),
                                         "openai_layout_identical": same, "err_rows0_5_untrimmed": untrimmed})
    assert err <= f["bound"], (err, f["bound"])
    assert same
    assert untrimmed <= f["bound"]


def test_tower_context_trimming_changes_nothing(fixture_tower):
    f = fixture_tower
    narrow = f["tower"](f["ids"][:5, :32].contiguous()).cpu().double()         # S_eff = 22 instead of 77
    d_narrow = (narrow - f["full"][:5]).abs().max().item()
    e_narrow = (narrow - f["want"][:5]).abs().max().item()
    d_alone = e_alone = 0.0
    for r in range(f["ids"].shape[0]):
        one = f["tower"](f["ids"][r:r + 1]).cpu().double()
        d_alone = max(d_alone, (one - f["full"][r:r + 1]).abs().max().item())
        e_alone = max(e_alone, (one - f["want"][r:r + 1]).abs().max().item())
    # an explicit eot equal to the default changes nothing either, whether it lives on the host or on the device
    eot = f["ids"].argmax(dim=1)
    assert torch.equal(f["tower"](f["ids"].cuda(), eot=eot.cuda()).cpu().double(), f["full"])
    parity_report("text_tower_trimming", {"diff_32_wide_vs_77_wide": d_narrow, "diff_row_alone_vs_batch": d_alone, "err_32_wide": e_narrow,
                                          "err_row_alone": e_alone, "bound": f["bound"]})
    assert max(d_narrow, d_alone, e_narrow, e_alone) <= f["bound"]
    with pytest.raises(gsdd_amd.GsddError):
        f["tower"](f["ids"], eot=torch.full((8,), 77))
    bad = f["ids"].clone()
    bad[2, 5] = 64                                                             # the vocabulary has 64 entries
    with pytest.raises(gsdd_amd.GsddError, match="vocabulary"):
        f["tower"](bad, eot=eot)


def test_provider_runs_the_native_tower_on_the_gpu(tmp_path):
    transformers = pytest.importorskip("transformers")
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
    cfg = transformers.CLIPTextConfig(vocab_size=514, hidden_size=32, intermediate_size=64, projection_dim=16, num_hidden_layers=2,
                                      num_attention_heads=2, max_position_embeddings=77, bos_token_id=512, eos_token_id=513, pad_token_id=0)
    torch.manual_seed(0)
    transformers.CLIPTextModelWithProjection(cfg).save_pretrained(tmp_path)
    texts = ["a dog runs", "x" * 40, "", "two people dance in a kitchen", "b", "the quick brown fox", "jumps over", "lazy dogs"]
    p = CLIPTextEmbedding(clip_dim=16, weights=str(tmp_path))
    cpu = p(texts).double()
    ids = p.tokenize(texts)
    eot = (ids == 513).int().argmax(dim=1)
    want = tower_ref(p.clip_model.state_dict(), ids, 2, eot=eot)
    bound = 4.0 * (cpu - want).abs().max().item()                              # 4 x the fp32 CPU module's own error against fp64
    p = p.cuda()
    got = p(texts)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (8, 16)
    assert p._tower is not None and p._tower.device.type == "cuda" and max(p._tower._buffers)[1] == 22      # trimmed to 22 positions
    err = (got.cpu().double() - want).abs().max().item()
    torch_path = p(texts, native=False)                                        # the PyTorch path still runs where the module lives
    err_torch = (torch_path.cpu().double() - want).abs().max().item()
    assert torch.equal(p(texts, native=True), got)
    parity_report("text_provider_byte_tower", {"err_native": err, "err_torch_gpu": err_torch, "bound": bound, "ref_fp32_err": bound / 4})
    assert err <= bound, (err, bound)
    assert torch_path.is_cuda and err_torch <= 1e-4
    # moving the module rebuilds the tower; back on the CPU the PyTorch path answers and native=True is an error
    p = p.cpu()
    assert torch.equal(p(texts).double(), cpu)
    with pytest.raises(gsdd_amd.GsddError):
        p(texts, native=True)
