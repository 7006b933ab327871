"""fp64 restatement of the CLIP image tower (`clip.model.VisionTransformer` / transformers.CLIPVisionModelWithProjection) on a state
dict with the transformers key names -- patch rows in the conv weight's element order [c][py][px], the class token in FRONT of the
patches, position embedding, pre-LayerNorm, pre-LN blocks with q scaled by d^-0.5, NO mask and QuickGELU, the class-token row, the
final LayerNorm, the bias-free projection -- and of the frame preprocessing in front of it (gsdd_clip_frame_patches).  Plain module
(not a conftest): the host tests check it against the fixture and the library, the GPU tests use it as the reference.

Every piece takes a `fault` naming one deliberate mistake, so that the host tests can record how far each moves the checked outputs:
"tail_unmasked" (the zero-filled keys of the last 16-key tile take part in the softmax), "tail_off_by_one" (key S - 1 masked too),
"causal" (the text tower's mask left on), "class_last" (class token behind the patches), "patch_order" (patch elements [py][px][c]),
"no_pre_ln", and for the preprocessing "a_half" (Keys' a = -0.5, PIL's, instead of torch's -0.75)."""
import torch
import torch.nn.functional as F

IM_MEAN, IM_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def attention_ref(q, k, v, scale, dtype=torch.float64, fault=None):
    """softmax(scale q k^T) v on (B, H, S, d) tensors in `dtype`, with torch's own operations."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    S = q.shape[-2]
    if fault == "tail_unmasked":                                   # what a kernel does that leaves the zero K rows of its last tile in
        pad = (-S) % 16
        k, v = F.pad(k, (0, 0, 0, pad)), F.pad(v, (0, 0, 0, pad))
    s = (q * scale) @ k.transpose(-1, -2)
    if fault == "tail_off_by_one":
        s[..., S - 1] = float("-inf")
    if fault == "causal":
        s = s + torch.full((S, S), float("-inf"), dtype=dtype).triu(1)
    return torch.softmax(s, dim=-1) @ v


def attention_inputs(B, S, n_head, d, hot):
    """q, k, v (B, H, S, d) fp32 of the attention-alone tests.  A per-(row, head) temperature takes the rows from near-uniform to
    dominated by one key (score spread 0.1 .. 10); on top, every query and ONE key share a component worth +6 in that key's score: the
    key in the LAST valid position (hot="last": a kernel that drops or mis-masks the tail of its last tile loses the bulk of the cooler
    rows) or the key in position 0 (hot="first")."""
    g = torch.Generator().manual_seed(1000 * S + 10 * n_head + d + (1 if hot == "last" else 0))
    q, k, v = (torch.randn((B, n_head, S, d), generator=g) for _ in range(3))
    temp = torch.logspace(-0.5, 0.5, B * n_head).view(B, n_head, 1, 1)
    q, k = q * temp, k * temp
    u = torch.randn((d,), generator=g)
    u = u / u.norm() * (6.0 ** 0.5) * d ** 0.25
    q = q + u
    pos = S - 1 if hot == "last" else 0
    k[:, :, pos] = k[:, :, pos] + u
    return q.contiguous(), k.contiguous(), v.contiguous()


def patch_rows(pixels, P, fault=None):
    """(N, 3, R, R) -> [N*G*G][3*P*P], row n*G*G + gy*G + gx, element order [c][py][px]."""
    N, _, R, _ = pixels.shape
    G = R // P
    x = pixels.reshape(N, 3, G, P, G, P)
    x = x.permute(0, 2, 4, 3, 5, 1) if fault == "patch_order" else x.permute(0, 2, 4, 1, 3, 5)
    return x.reshape(N * G * G, 3 * P * P)


def tower_ref(sd, pixels, n_head, eps=1e-5, dtype=torch.float64, fault=None):
    """-> (N, E) in `dtype`.  sd: transformers-layout state dict, pixels: (N, 3, R, R) CLIP-normalised."""
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    e = "vision_model.embeddings."
    conv = w[e + "patch_embedding.weight"]
    C, P = conv.shape[0], conv.shape[2]
    N = pixels.shape[0]
    pe = (patch_rows(pixels.to(dtype), P, fault) @ conv.reshape(C, -1).t()).view(N, -1, C)
    cls = w[e + "class_embedding"].view(1, 1, C).expand(N, 1, C)
    x = torch.cat([pe, cls] if fault == "class_last" else [cls, pe], dim=1) + w[e + "position_embedding.weight"]
    S, d = x.shape[1], C // n_head
    if fault != "no_pre_ln":
        x = F.layer_norm(x, (C,), w["vision_model.pre_layrnorm.weight"], w["vision_model.pre_layrnorm.bias"], eps)
    n = 0
    while f"vision_model.encoder.layers.{n}.layer_norm1.weight" in w:
        p = f"vision_model.encoder.layers.{n}."
        h = F.layer_norm(x, (C,), w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
        q, k, v = (F.linear(h, w[p + f"self_attn.{a}_proj.weight"], w[p + f"self_attn.{a}_proj.bias"])
                   .view(N, S, n_head, d).transpose(1, 2) for a in "qkv")
        a = attention_ref(q, k, v, d ** -0.5, dtype, fault).transpose(1, 2).reshape(N, S, C)
        x = x + F.linear(a, w[p + "self_attn.out_proj.weight"], w[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (C,), w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps)
        h = F.linear(h, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"])
        n += 1
    pooled = x[:, S - 1 if fault == "class_last" else 0]
    pooled = F.layer_norm(pooled, (C,), w["vision_model.post_layernorm.weight"], w["vision_model.post_layernorm.bias"], eps)
    return F.linear(pooled, w["visual_projection.weight"])


# ------------------------------------------------------------------ frame preprocessing
def make_clips(B, T, H, seed):
    """ImageNet-normalised test clips (B, 3, T, H, H) float32: N(0, 1.5) noise, which de-normalises below 0 and above 1 in about a
    tenth of the pixels each (the quantiser's clamp), smooth ramps in the last frame of clip 0, and a 0 / 1 checkerboard of 2 x 2
    cells in frame 0 of clip 0, whose bicubic overshoot the clamp to [0, 1] must cut."""
    g = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn((B, 3, T, H, H), generator=g)
    mean, std = (torch.tensor(v).view(3, 1, 1) for v in (IM_MEAN, IM_STD))
    i = torch.arange(H)
    board = (((i[:, None] // 2) + (i[None, :] // 2)) % 2).float().expand(3, H, H)
    x[0, :, 0] = (board - mean) / std
    ramp = ((i[:, None] + i[None, :]).float() / max(2 * H - 2, 1)).expand(3, H, H)
    x[0, :, T - 1] = (ramp - mean) / std
    return x


def quantised_levels(clips):
    """ImageNet-normalised float32 clips (B, 3, T, H, W) -> the uint8 levels 0..255 as float32, computed in fp32 exactly as the
    evaluator's _prepare computes them (x * std + mean, x 255, truncated; clamped where a uint8 cast would wrap).  The levels are
    integers and DEFINED by that fp32 arithmetic, so the fp64 reference starts from them and not from an fp64 de-normalisation (which
    would land one level away wherever x * 255 falls within a rounding of an integer)."""
    x = clips.to(torch.float32)
    std, mean = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1, 1) for v in (IM_STD, IM_MEAN))
    return torch.nan_to_num(torch.trunc((x * std + mean) * 255), nan=0.0).clamp(0, 255)


def _cubic_weights(t, a):
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    c1 = lambda x: ((a + 2) * x - (a + 3)) * x * x + 1
    c2 = lambda x: ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return torch.stack([c2(x0), c1(x1), c1(x2), c2(x3)], dim=-1)


def bicubic_matrix(H, R, a=-0.75, dtype=torch.float64):
    """[R][H] matrix of torch's bicubic resize along one axis (align_corners=False, no antialias, border indices clamped): output o
    reads the taps i0 - 1 .. i0 + 2 around the source coordinate (o + 0.5) H / R - 0.5 = ((2 o + 1) H - R) / (2 R), whose floor and
    fraction are taken in integers."""
    o = torch.arange(R, dtype=torch.int64)
    num, den = (2 * o + 1) * H - R, 2 * R
    i0 = torch.div(num, den, rounding_mode="floor")
    t = (num - i0 * den).to(dtype) / den
    wts = _cubic_weights(t, a)
    m = torch.zeros((R, H), dtype=dtype)
    for j in range(4):
        m.index_put_((o, (i0 - 1 + j).clamp(0, H - 1)), wts[:, j], accumulate=True)
    return m


def preprocess_ref(clips, R, dtype=torch.float64, fault=None, normalise=True):
    """ImageNet-normalised clips (B, 3, T, H, H) -> (B*T, 3, R, R) in `dtype`: quantised levels / 255, bicubic resize, clamp to
    [0, 1], CLIP's normalisation (normalise=False stops after the clamp)."""
    B, _, T, H, W = clips.shape
    assert H == W <= R
    x = (quantised_levels(clips).to(dtype) / 255).permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, H)
    m = bicubic_matrix(H, R, a=-0.5 if fault == "a_half" else -0.75, dtype=dtype)
    x = (m @ (x @ m.t())).clamp(0, 1)                              # rows first (over x), then the column, as torch does
    if not normalise:
        return x
    mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    return (x - mean) / std


def preprocess_torch(clips, R, dtype=torch.float32, normalise=True):
    """The same composite with torch's own resize in `dtype`: levels / 255, F.interpolate(mode="bicubic", align_corners=False), clamp,
    CLIP's normalisation.  In fp32 it is the yardstick of the kernel's tolerance (torch forms the source coordinate and the weights in
    fp32); in fp64 it is what the restatement must equal."""
    B, _, T, H, W = clips.shape
    x = (quantised_levels(clips).to(dtype) / 255).permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, W)
    x = F.interpolate(x, size=(R, R), mode="bicubic", align_corners=False).clamp(0, 1)
    if not normalise:
        return x
    mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    return (x - mean) / std


def frame_patches_ref(clips, R, P, dtype=torch.float64, fault=None):
    """What gsdd_clip_frame_patches writes: [B*T*G*G][3*P*P]."""
    return patch_rows(preprocess_ref(clips, R, dtype, fault), P)


def frames_ref(sd, clips, n_head, R, dtype=torch.float64):
    """ClipVisionTower.forward in `dtype`: (B, 3, T, H, H) -> (B, T, E)."""
    B, T = clips.shape[0], clips.shape[2]
    return tower_ref(sd, preprocess_ref(clips, R, dtype), n_head, dtype=dtype).view(B, T, -1)
