"""The CLIP image tower on the HIP path: `clip.model.VisionTransformer` / transformers.CLIPVisionModelWithProjection (patch embedding,
class token + position embedding, pre-LayerNorm, pre-LN transformer with QuickGELU and NO attention mask, the class-token row, the
final LayerNorm, the bias-free projection).  It is the image half of CLIPSIM (gsdd_amd.metrics.clip_similarity): the cosine between a
caption's CLIP text feature (gsdd_amd.text.ClipTextTower) and the CLIP image feature of every generated frame.

Every computation is a kernel of libgsdd.so: gsdd_clip_frame_patches / gsdd_clip_vision_embed (csrc/clip_vision.hip),
gsdd_clip_attention (csrc/clip_attention.hip), gsdd_text_pool with every position 0 (the class-token row), and gsdd_row_stats /
gsdd_ln_apply / gsdd_gemm for the LayerNorms and the linears -- the patch embedding, a Conv2d(3, C, P, stride P, bias=False), is one
plain linear over patch rows.  The residual blocks and the tower base are _clip.py's, shared with the text tower; here they run with
the non-causal attention.  fp32 throughout; the reference's `clip` package runs the tower in fp16.

Frames reach `forward` as the decoder returns them (ImageNet-normalised floats) and are quantised to uint8 levels as the evaluator
does, resized with TORCH's bicubic and normalised with CLIP's statistics; the `clip` package resizes with PIL's (another kernel,
antialiasing), so scores on real weights are close to, not equal to, that pipeline's.  `forward_pixels` takes frames that are
already at the tower's resolution and CLIP-normalised.

The attention kernel holds a sequence of at most 77 positions, so ViT-B/32 at 224 (7 x 7 patches + 1 = 50) fits and ViT-B/16 (197)
and ViT-L/14 (257) do not."""
import torch

from . import ops
from ._clip import LN_EPS, MAX_POSITIONS, ClipTower, _f32, hf_layers_to_openai, layers_from_hf, layers_from_openai, run_resblocks
from ._lib import GsddError

MAX_SEQUENCE = MAX_POSITIONS


def hf_to_openai_vision_state_dict(sd):
    """Keys of transformers.CLIPVisionModelWithProjection -> the `clip` package's `visual.*` keys (q|k|v concatenated into in_proj,
    visual_projection transposed to [C][E]).  The inverse of what from_openai_state_dict undoes; used by tests and by exporters."""
    e = "vision_model.embeddings."
    return {"visual.conv1.weight": sd[e + "patch_embedding.weight"], "visual.class_embedding": sd[e + "class_embedding"],
            "visual.positional_embedding": sd[e + "position_embedding.weight"],
            "visual.ln_pre.weight": sd["vision_model.pre_layrnorm.weight"], "visual.ln_pre.bias": sd["vision_model.pre_layrnorm.bias"],
            "visual.ln_post.weight": sd["vision_model.post_layernorm.weight"], "visual.ln_post.bias": sd["vision_model.post_layernorm.bias"],
            "visual.proj": sd["visual_projection.weight"].t().contiguous(),
            **hf_layers_to_openai(sd, "vision_model.encoder.layers.", "visual.transformer.resblocks.")}


class ClipVisionTower(ClipTower):
    """Frozen fp32 device weights of a CLIP image tower and its forward pass on the HIP kernels.

    Operands: `patch_w` [C][3*P*P] (the conv weight flattened, element order [c][py][px]), `class_emb` [C], `pos_emb` [S][C],
    `g_pre` / `b_pre` and `g_post` / `b_post` (the LayerNorms in front of and behind the transformer), `proj` [E][C] (applied as
    x @ proj.T, no bias), and per layer the text tower's: `wqkv` / `bqkv`, `wo` / `bo`, `w1` / `b1`, `w2` / `b2`, `g1` / `be1`,
    `g2` / `be2`."""

    _VECTORS = ("patch_w", "class_emb", "pos_emb", "g_pre", "b_pre", "g_post", "b_post", "proj")

    def __init__(self, patch_w, class_emb, pos_emb, g_pre, b_pre, layers, g_post, b_post, proj, n_head, eps=LN_EPS, hidden_act="quick_gelu"):
        if hidden_act != "quick_gelu":
            raise GsddError(f"ClipVisionTower implements CLIP's QuickGELU (x sigmoid(1.702 x)); the supplied tower uses {hidden_act!r}")
        if patch_w.dim() != 4 or patch_w.shape[1] != 3 or patch_w.shape[2] != patch_w.shape[3]:
            raise GsddError(f"ClipVisionTower: the patch embedding must be a [C][3][P][P] weight, got {tuple(patch_w.shape)}")
        self.patch = int(patch_w.shape[2])
        self.patch_w = _f32(patch_w).reshape(patch_w.shape[0], -1).contiguous()
        self.class_emb, self.pos_emb, self.proj = _f32(class_emb).reshape(-1), _f32(pos_emb), _f32(proj)
        self.g_pre, self.b_pre, self.g_post, self.b_post = _f32(g_pre), _f32(b_pre), _f32(g_post), _f32(b_post)
        self.width = self.patch_w.shape[0]
        self.seq = int(self.pos_emb.shape[0])
        self.grid = int(round((self.seq - 1) ** 0.5))
        self.resolution = self.grid * self.patch
        self._set_layers(layers, n_head, eps)
        if self.grid * self.grid + 1 != self.seq:
            raise GsddError(f"ClipVisionTower: {self.seq} position embeddings are not a square grid of patches plus the class token")
        if self.seq > MAX_SEQUENCE:
            raise GsddError(f"ClipVisionTower: a sequence of {self.seq} positions ({self.grid} x {self.grid} patches + the class token); "
                            f"the attention kernel holds at most {MAX_SEQUENCE} (ViT-B/32 at 224 has 50; ViT-B/16 and ViT-L/14 do not fit)")
        self._check_shapes(self.proj.shape[1] == self.width and self.pos_emb.shape[1] == self.width and self.class_emb.shape[0] == self.width)

    # ------------------------------------------------------------------ weight import
    @classmethod
    def from_hf_state_dict(cls, sd, n_head, eps=LN_EPS, hidden_act="quick_gelu"):
        """sd: state dict of transformers.CLIPVisionModelWithProjection (vision_model.embeddings.*, vision_model.pre_layrnorm.* -- the
        library's spelling --, vision_model.encoder.layers.N.*, vision_model.post_layernorm.*, visual_projection.weight).  The head
        count is not recoverable from the tensors."""
        layers = layers_from_hf(sd, "vision_model.encoder.layers.")
        e = "vision_model.embeddings."
        return cls(sd[e + "patch_embedding.weight"], sd[e + "class_embedding"], sd[e + "position_embedding.weight"],
                   sd["vision_model.pre_layrnorm.weight"], sd["vision_model.pre_layrnorm.bias"], layers,
                   sd["vision_model.post_layernorm.weight"], sd["vision_model.post_layernorm.bias"], sd["visual_projection.weight"],
                   n_head, eps, hidden_act)

    @classmethod
    def from_openai_state_dict(cls, sd, eps=LN_EPS):
        """sd: the `clip` package's keys (what the reference's Lightning checkpoints carry under `textencoder.clip_model.`, see
        checkpoint.extract_clip_vision_tower): fp16 tensors are widened, `visual.proj` ([C][E], applied as x @ P) is transposed,
        heads = width / 64 (clip.model.CLIP: vision_heads = vision_width // 64), the text tower's keys are ignored."""
        layers = layers_from_openai(sd, "visual.transformer.resblocks.")
        width = sd["visual.conv1.weight"].shape[0]
        if width % 64:
            raise GsddError(f"ClipVisionTower: the clip package uses width / 64 heads; width {width} is not a multiple of 64")
        return cls(sd["visual.conv1.weight"], sd["visual.class_embedding"], sd["visual.positional_embedding"], sd["visual.ln_pre.weight"],
                   sd["visual.ln_pre.bias"], layers, sd["visual.ln_post.weight"], sd["visual.ln_post.bias"], _f32(sd["visual.proj"]).t(),
                   width // 64, eps)

    # ------------------------------------------------------------------ forward
    def _extra_buffers(self, N, S, f):
        return {"pe": torch.empty((N * (S - 1), self.width), **f), "first": torch.zeros((N,), dtype=torch.int64, device=self.device),
                "first_host": torch.zeros((N,), dtype=torch.int64)}

    def _run(self, rows, N):
        """rows: patch rows [N*G*G][3*P*P] on the device -> (N, E)."""
        S = self.seq
        buf = self._get_buffers(N, S)
        x, y, stats = buf["x"], buf["y"], buf["stats"]
        ops.linear(rows, self.patch_w, buf["pe"])
        ops.clip_vision_embed(buf["pe"], self.class_emb, self.pos_emb, N, S, y)
        ops.row_stats(y, stats, eps=self.eps)
        ops.ln_apply(y, stats, self.g_pre, self.b_pre, out=x)
        run_resblocks(self.layers, ops.clip_attention, buf, N, S, self.n_head, self.eps)
        return self._pool_project(buf, buf["first"], buf["first_host"], N, S, self.g_post, self.b_post)      # the class-token row of every frame

    @torch.no_grad()
    def forward(self, clips):
        """clips: float (B, 3, T, H, W), ImageNet-normalised as the decoder returns them, H == W <= the tower's resolution -> (B, T, E)
        fp32 on the tower's device: the image feature of every frame (not normalised to unit length)."""
        if clips.dim() != 5 or clips.shape[1] != 3:
            raise GsddError(f"ClipVisionTower.forward: clips must be (B, 3, T, H, W), got {tuple(clips.shape)}")
        B, _, T, H, W = clips.shape
        if H != W:
            raise GsddError(f"ClipVisionTower.forward: frames of {H} x {W}; only square frames are supported (no crop is applied)")
        if H > self.resolution:
            raise GsddError(f"ClipVisionTower.forward: frames of {H} x {W} are larger than the tower's resolution {self.resolution}; "
                            "shrinking needs an antialiased resize, which is not supported")
        self._need_device("forward")
        clips = clips.detach().to(device=self.device, dtype=torch.float32).contiguous()
        rows = ops.clip_frame_patches(clips, self.resolution, self.patch)
        return self._run(rows, B * T).view(B, T, -1)

    @torch.no_grad()
    def forward_pixels(self, pixel_values):
        """pixel_values: float (N, 3, R, R) at the tower's resolution, already CLIP-normalised (what the library's image processor
        yields) -> (N, E) fp32.  No resize: the patch rows are a reshape of the frames."""
        R, P, G = self.resolution, self.patch, self.grid
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, R, R):
            raise GsddError(f"ClipVisionTower.forward_pixels: pixel_values must be (N, 3, {R}, {R}), got {tuple(pixel_values.shape)}")
        self._need_device("forward_pixels")
        N = pixel_values.shape[0]
        px = pixel_values.detach().to(device=self.device, dtype=torch.float32)
        rows = px.reshape(N, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(N * G * G, 3 * P * P).contiguous()
        return self._run(rows, N)

    __call__ = forward
