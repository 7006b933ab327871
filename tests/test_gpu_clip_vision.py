"""The native CLIP image tower on the GPU (csrc/clip_vision.hip, gsdd_amd.vision.ClipVisionTower) and CLIPSIM against fp64.

Bounds.  Attention alone: 4 x the error of the same computation in fp32 with torch on the CPU against the same fp64 reference,
measured in the test (the convention of tests/test_gpu_text_tower.py: another summation order may not cost more than that).  Frame
patches: 4 x the error of torch's own fp32 composite (levels / 255, F.interpolate bicubic, clamp, normalise) against the fp64
restatement; that yardstick is loose because torch forms the source coordinate and the weights in fp32, and the kernel takes the
coordinate's floor and fraction in integers -- the achieved error and its ratio to the bound are recorded, the bar is not tightened.
Patch GEMM: the element-wise bar of tests/test_gpu_gemm_family.py, gamma(K) (|X| |W|^T), gamma(K) = 2^-24 (8 + 2 sqrt(K)).  The whole
tower: 4 x `ref_fp32_err` of the fixture (tests/golden/make_golden_clip_vision.py: the library's own fp32 error on these frames).
CLIPSIM: that bound carried through the cosine (derived in the test)."""
import math

import pytest
import torch

import gsdd_amd
from gsdd_amd import ops
from gsdd_amd.metrics import clip_similarity
from gsdd_amd.vision import ClipVisionTower, hf_to_openai_vision_state_dict
from conftest import parity_report
from clip_vision_ref import (attention_inputs, attention_ref, frame_patches_ref, frames_ref, make_clips, patch_rows, preprocess_ref,
                             preprocess_torch, quantised_levels, tower_ref)

pytestmark = pytest.mark.gpu

S_LIST = [1, 2, 15, 16, 17, 31, 32, 33, 50, 64, 65, 77]
HEADS = [(1, 64), (2, 64), (12, 64), (2, 32), (2, 16)]
PATCH_CASES = [(8, 8, 8), (16, 56, 8), (56, 56, 8), (128, 224, 32), (37, 64, 32)]          # (H, R, P)
NAN = float("nan")
POISON = -777.0


@pytest.fixture(scope="module")
def fixture_tower():
    from conftest import load_golden
    sd, a, cfg = load_golden("clip_vision_small")
    pixels, want = torch.from_numpy(a["pixels_x32"]).float() / 32, torch.from_numpy(a["want"])
    bound = 4.0 * float(a["ref_fp32_err"])
    tower = ClipVisionTower.from_hf_state_dict(sd, cfg["n_head"]).cuda()
    full = tower.forward_pixels(pixels).cpu().double()
    return {"sd": sd, "cfg": cfg, "pixels": pixels, "want": want, "bound": bound, "tower": tower, "full": full}


def _fused(q, k, v):
    """(B, H, S, d) x 3 -> fused rows [B*S][3C]"""
    B, H, S, d = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B * S, H * d) for t in (q, k, v)], dim=1).contiguous()


@pytest.mark.parametrize("hot", ["last", "first"])
@pytest.mark.parametrize("n_head,d", HEADS)
@pytest.mark.parametrize("S", S_LIST)
def test_clip_attention_against_fp64(S, n_head, d, hot):
    B, C = 3, n_head * d
    q, k, v = attention_inputs(B, S, n_head, d, hot)
    scale = d ** -0.5
    want = attention_ref(q, k, v, scale)                                           # (B, H, S, d) fp64
    ref32 = attention_ref(q, k, v, scale, dtype=torch.float32).double()
    bound = 4.0 * (ref32 - want).abs().max().item()
    prob = torch.softmax((q.double() * scale) @ k.double().transpose(-1, -2), -1)
    p_hot = prob[..., S - 1 if hot == "last" else 0]
    pad = 16
    qkv = torch.full((B * S + pad, 3 * C), NAN)
    qkv[:B * S] = _fused(q, k, v)
    qkv = qkv.cuda()
    out = torch.full((B * S + pad, C), NAN, device="cuda")
    out[B * S:] = POISON
    ops.clip_attention(qkv[:B * S], B, S, n_head, out[:B * S], scale=scale)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[B * S:], torch.full((pad, C), POISON)), "rows behind B*S were written"
    assert torch.isfinite(got[:B * S]).all(), "an output element was not written (out was pre-filled with NaN) or is not finite"
    got64 = got[:B * S].double().view(B, S, n_head, d).transpose(1, 2)
    err = (got64 - want).abs().max().item()
    print(f"[clip_attention] S={S} heads={n_head} d={d} hot={hot}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.2f} "
          f"p(hot key) {p_hot.min():.2f}..{p_hot.max():.2f}")
    if (S, n_head, d) in ((50, 12, 64), (77, 12, 64), (50, 2, 16), (17, 2, 32)):
        parity_report(f"clip_attention_S{S}_h{n_head}_d{d}_{hot}", {"err": err, "bound": bound, "ref_fp32_err": bound / 4})
    assert err <= bound, (err, bound)
    # row b of the batch equals the same row launched alone, bit for bit
    for b in range(B):
        one = torch.full((S, C), NAN, device="cuda")
        ops.clip_attention(qkv[b * S:(b + 1) * S], 1, S, n_head, one, scale=scale)
        assert torch.equal(one.cpu(), got[b * S:(b + 1) * S]), f"row {b} alone differs from row {b} of the batch"


def test_clip_attention_rejects_bad_arguments():
    qkv = torch.zeros((78, 192), device="cuda")
    out = torch.full((78, 64), POISON, device="cuda")
    with pytest.raises(gsdd_amd.GsddError):
        ops.clip_attention(qkv, 1, 78, 1, out)                     # S > 77
    with pytest.raises(gsdd_amd.GsddError):
        ops.clip_attention(qkv[:8], 1, 8, 8, out[:8])              # head dimension 8
    with pytest.raises(gsdd_amd.GsddError):
        ops.clip_attention(torch.zeros((8, 384), device="cuda"), 1, 8, 1, torch.zeros((8, 128), device="cuda"))      # head dimension 128
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((78, 64), POISON))


@pytest.mark.parametrize("H,R,P", PATCH_CASES)
def test_frame_patches_against_fp64(H, R, P):
    B, T, G = 2, 3, R // P
    clips = make_clips(B, T, H, seed=H + R)
    want = frame_patches_ref(clips, R, P)                                          # [B*T*G*G][3*P*P] fp64
    yard = patch_rows(preprocess_torch(clips, R), P).double()                      # torch's fp32 composite
    bound = 4.0 * (yard - want).abs().max().item()
    pad = 8
    out = torch.full((B * T * G * G + pad, 3 * P * P), NAN, device="cuda")
    out[B * T * G * G:] = POISON
    ops.clip_frame_patches(clips.cuda(), R, P, out=out[:B * T * G * G])
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[B * T * G * G:], torch.full((pad, 3 * P * P), POISON)), "rows behind the last patch were written"
    assert torch.isfinite(got[:B * T * G * G]).all(), "a patch element was not written"
    err = (got[:B * T * G * G].double() - want).abs().max().item()
    lo, hi = want.min().item(), want.max().item()
    rec = {"err": err, "bound": bound, "torch_fp32_err": bound / 4, "ratio": err / bound if bound else 0.0, "want_min": lo, "want_max": hi}
    if H == R:
        # every fraction is 0 and the weights are exactly (0, 1, 0, 0): the quantised frame, normalised with the same fp32 operations
        lv = (quantised_levels(clips) / 255.0).permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, H)
        mean, std = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in ((0.48145466, 0.4578275, 0.40821073),
                                                                                     (0.26862954, 0.26130258, 0.27577711)))
        exact = patch_rows((lv - mean) / std, P)
        rec["identical_to_the_quantised_frame"] = bool(torch.equal(got[:B * T * G * G], exact))
    parity_report(f"clip_frame_patches_H{H}_R{R}_P{P}", rec)
    assert err <= bound, (err, bound)
    # the clamp to [0, 1] holds everywhere (the checkerboard's overshoot would leave it)
    assert lo >= (0 - 0.48145466) / 0.26130258 - 1e-6 and got[:B * T * G * G].min().item() >= (0 - 0.48145466) / 0.26130258 - 1e-6
    if H == R:
        assert rec["identical_to_the_quantised_frame"]


def test_frame_patches_rejects_bad_shapes():
    out = torch.full((49, 192), POISON, device="cuda")
    L = gsdd_amd.lib()
    clips = torch.zeros((1, 3, 1, 16, 24), device="cuda")
    st = gsdd_amd._lib.stream_ptr()
    p = gsdd_amd._lib.ptr
    assert L.gsdd_clip_frame_patches(p(clips), 1, 1, 16, 24, 56, 8, p(out), st) != 0       # H != W
    assert L.gsdd_clip_frame_patches(p(clips), 1, 1, 64, 64, 56, 8, p(out), st) != 0       # H > R
    assert L.gsdd_clip_frame_patches(p(clips), 1, 1, 16, 16, 56, 16, p(out), st) != 0      # R % P != 0
    with pytest.raises(gsdd_amd.GsddError):
        ops.clip_frame_patches(clips, 56, 8)
    with pytest.raises(gsdd_amd.GsddError):
        ops.clip_vision_embed(torch.zeros((77, 16), device="cuda"), torch.zeros(16, device="cuda"), torch.zeros((78, 16), device="cuda"), 1, 78,
                              torch.zeros((78, 16), device="cuda"))                        # S > 77
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((49, 192), POISON))


def test_vision_embed_is_exact():
    g = torch.Generator().manual_seed(11)
    N, S, C = 3, 10, 72                                            # C no multiple of 64
    pe, cls, pos = torch.randn((N * (S - 1), C), generator=g), torch.randn((C,), generator=g), torch.randn((S + 2, C), generator=g)
    x = torch.full((N * S + 3, C), POISON, device="cuda")
    ops.clip_vision_embed(pe.cuda(), cls.cuda(), pos.cuda(), N, S, x[:N * S])
    want = (torch.cat([cls.view(1, 1, C).expand(N, 1, C), pe.view(N, S - 1, C)], dim=1) + pos[:S]).reshape(N * S, C)
    got = x.cpu()
    assert torch.equal(got[:N * S], want) and torch.equal(got[N * S:], torch.full((3, C), POISON))
    two = torch.full((2 * 2, C), POISON, device="cuda")            # S = 2: one patch per frame
    ops.clip_vision_embed(pe[:2].cuda(), cls.cuda(), pos.cuda(), 2, 2, two)
    assert torch.equal(two.cpu(), torch.stack([cls + pos[0], pe[0] + pos[1], cls + pos[0], pe[1] + pos[1]]))


def test_patch_gemm_at_vit_b32s_contraction_length():
    """The patch embedding of ViT-B/32 as one linear: 3 * 32 * 32 = 3072 terms per output, no bias."""
    g = torch.Generator().manual_seed(5)
    M, K, Cout = 2 * 49, 3 * 32 * 32, 96
    x = torch.randn((M, K), generator=g) * 1.2                                     # CLIP-normalised pixels: about unit scale
    w = torch.randn((Cout, K), generator=g) * 0.02
    out = torch.full((M, Cout), NAN, device="cuda")
    ops.linear(x.cuda(), w.cuda(), out)
    torch.cuda.synchronize()
    want = x.double() @ w.double().t()
    bound = 2.0 ** -24 * (8 + 2 * math.sqrt(K)) * (x.double().abs() @ w.double().abs().t())
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    worst = ((got - want).abs() / bound).max().item()
    parity_report("clip_patch_gemm_K3072", {"worst_err_over_bound": worst, "err": (got - want).abs().max().item(), "M": M, "K": K})
    assert worst <= 1.0, worst


def test_tower_on_the_fixture(fixture_tower):
    f = fixture_tower
    err = (f["full"] - f["want"]).abs().max().item()
    ref = tower_ref(f["sd"], f["pixels"], f["cfg"]["n_head"])
    assert (ref - f["want"]).abs().max().item() <= 1e-12
    # the clip package's key layout gives the same operands, hence the same bits
    oa = ClipVisionTower.from_openai_state_dict(hf_to_openai_vision_state_dict(f["sd"])).cuda()
    same = torch.equal(oa.forward_pixels(f["pixels"]).cpu().double(), f["full"])
    # six frames in one call against the six run one at a time
    d_alone = e_alone = 0.0
    for r in range(f["pixels"].shape[0]):
        one = f["tower"].forward_pixels(f["pixels"][r:r + 1]).cpu().double()
        d_alone = max(d_alone, (one - f["full"][r:r + 1]).abs().max().item())
        e_alone = max(e_alone, (one - f["want"][r:r + 1]).abs().max().item())
    parity_report("clip_vision_fixture", {"err": err, "bound": f["bound"], "ref_fp32_err": f["bound"] / 4, "max_abs_want": f["want"].abs().max().item(),
                                          "openai_layout_identical": same, "diff_frame_alone_vs_batch": d_alone, "err_frame_alone": e_alone})
    assert err <= f["bound"], (err, f["bound"])
    assert same
    assert d_alone == 0.0 and e_alone <= f["bound"], (d_alone, e_alone, f["bound"])        # a frame's bits do not depend on its neighbours
    assert f["tower"].forward_pixels(f["pixels"].cuda()).is_cuda and set(f["tower"]._buffers) == {(6, 50), (1, 50)}


def test_clipsim_end_to_end(fixture_tower):
    """ClipSimScorer with the fixture's tower and a stub text embedder on (2, 3, 4, 16, 16) clips at R = 56, against the fp64
    restatement.  Bound: the image features are within b = the tower's bound of the reference's, element-wise, so a frame's feature f
    moves by at most e = b sqrt(E) in length; the cosine's gradient with respect to f has length sqrt(1 - cos^2) / |f| <= 1 / |f|, and
    along the segment |f| >= |f| - e, so a frame's cosine moves by at most e / (|f| - e) and the score by the mean of that over frames."""
    import src  # noqa: F401
    from src.utils.evaluator import ClipSimScorer, Evaluator, MeanPoolEncoder
    f = fixture_tower
    B, T, E = 2, 4, 32
    clips = make_clips(B, T, 16, seed=77)
    texts = ["a checkerboard flickers", "noise"]
    g = torch.Generator().manual_seed(3)
    table = {t: torch.randn((E,), generator=g) for t in texts}
    embed = lambda ts: torch.stack([table[t] for t in ts])
    scorer = ClipSimScorer(embed, f["tower"])
    got = scorer(texts, clips)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
    frames = frames_ref(f["sd"], clips, f["cfg"]["n_head"], 56)                    # (B, T, E) fp64
    want = clip_similarity(embed(texts), frames)
    e = f["bound"] * math.sqrt(E)
    norms = frames.norm(dim=-1)
    assert norms.min().item() > 100 * e
    bound = (e / (norms - e)).mean(dim=1)
    err = (got - want).abs()
    feat_err = (f["tower"](clips).cpu().double() - frames).abs().max().item()
    parity_report("clipsim_end_to_end", {"err": err.tolist(), "bound": bound.tolist(), "score": want.tolist(), "feature_err": feat_err,
                                         "feature_bound": f["bound"], "min_feature_norm": norms.min().item()})
    assert feat_err <= f["bound"], (feat_err, f["bound"])
    assert bool((err <= bound).all()), (err, bound)
    assert float(want.abs().max()) <= 1.0
    # the evaluator with the scorer returns both keys, and the FVD is the one it returns without
    batch = {"video": make_clips(4, T, 16, seed=78), "text": texts * 2}
    outputs = torch.cat([clips, clips.flip(0)])
    enc = MeanPoolEncoder(grid=2)
    ev, ev0 = Evaluator("cuda", enc, target_resolution=32, clip_scorer=scorer), Evaluator("cuda", enc, target_resolution=32)
    for x in (ev, ev0):
        x.push_vals(batch, 0, outputs)
        x.push_vals(batch, 1, outputs.flip(2))
    m, m0 = ev.evaluate_metrics(), ev0.evaluate_metrics()
    assert set(m) == {"fvd", "clipsim"} and set(m0) == {"fvd"} and m["fvd"] == m0["fvd"]
    # frames reversed in time score the same; clips swapped between the captions score as the restatement says
    swapped = clip_similarity(embed(texts), frames.flip(0))
    want_mean = torch.cat([want, swapped, want, swapped]).mean().item()
    assert abs(m["clipsim"] - want_mean) <= float(bound.max())
