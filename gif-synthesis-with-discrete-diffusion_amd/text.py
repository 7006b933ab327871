"""The CLIP text tower on the HIP path: `clip.model.CLIP.encode_text` (token + position embedding, pre-LN causal transformer with
QuickGELU, final LayerNorm, the row at the end-of-text token, the text projection), which the reference calls at
src/models/text_models/clip_text_embedding.py:56-65.

Every computation is a kernel of libgsdd.so: gsdd_text_embed / gsdd_text_pool (csrc/text_tower.hip), gsdd_text_attention
(csrc/clip_attention.hip) and, for the linears with their LayerNorm prologue, bias, QuickGELU (activation 2) and residual,
gsdd_row_stats + gsdd_gemm.  What the two CLIP towers share lives in _clip.py.  The arithmetic is fp32 throughout; the reference runs
the same tower in fp16 (`clip.model.convert_weights`).

Context trimming: under the causal mask nothing behind a row's end-of-text position reaches it, so only the first
S_eff = max(eot) + 1 positions of the batch are run (at the reference's recipe, start + 20 + end, at most 22 of 77).  `eot` is taken
from the ids on the host, where the tokenizer has just produced them, so choosing S_eff costs no device synchronisation."""
import torch

from . import ops
from ._clip import LN_EPS, MAX_POSITIONS, ClipTower, _f32, hf_layers_to_openai, layers_from_hf, layers_from_openai, run_resblocks
from ._lib import GsddError

MAX_CONTEXT = MAX_POSITIONS


def hf_to_openai_state_dict(sd):
    """Keys of transformers.CLIPTextModelWithProjection -> the `clip` package's text-tower keys (q|k|v concatenated into in_proj,
    text_projection transposed to [C][P]).  The inverse of what from_openai_state_dict undoes; used by tests and by exporters."""
    return {"token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
            "positional_embedding": sd["text_model.embeddings.position_embedding.weight"],
            "ln_final.weight": sd["text_model.final_layer_norm.weight"], "ln_final.bias": sd["text_model.final_layer_norm.bias"],
            "text_projection": sd["text_projection.weight"].t().contiguous(),
            **hf_layers_to_openai(sd, "text_model.encoder.layers.", "transformer.resblocks.")}


class ClipTextTower(ClipTower):
    """Frozen fp32 device weights of a CLIP text tower and its forward pass on the HIP kernels.

    Operands per layer: `wqkv` [3C][C] / `bqkv` [3C] (q | k | v fused), `wo` / `bo`, `w1` / `b1` (fc1, [I][C]), `w2` / `b2`
    (fc2, [C][I]), `g1` / `be1` and `g2` / `be2` (the two LayerNorms); `tok_emb` [vocab][C], `pos_emb` [n_pos][C], `gf` / `bf` (final
    LayerNorm), `proj` [P][C] (applied as x @ proj.T, no bias)."""

    _VECTORS = ("tok_emb", "pos_emb", "gf", "bf", "proj")

    def __init__(self, tok_emb, pos_emb, layers, gf, bf, proj, n_head, eps=LN_EPS):
        self.tok_emb, self.pos_emb, self.gf, self.bf, self.proj = _f32(tok_emb), _f32(pos_emb), _f32(gf), _f32(bf), _f32(proj)
        self.width = self.tok_emb.shape[1]
        self._set_layers(layers, n_head, eps)
        self._check_shapes(self.proj.shape[1] == self.width and self.pos_emb.shape[1] == self.width)

    # ------------------------------------------------------------------ weight import
    @classmethod
    def from_hf_state_dict(cls, sd, n_head, eps=LN_EPS):
        """sd: state dict of transformers.CLIPTextModelWithProjection (text_model.embeddings.*, text_model.encoder.layers.N.*,
        text_model.final_layer_norm.*, text_projection.weight).  The head count is not recoverable from the tensors."""
        layers = layers_from_hf(sd, "text_model.encoder.layers.")
        return cls(sd["text_model.embeddings.token_embedding.weight"], sd["text_model.embeddings.position_embedding.weight"], layers,
                   sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"], sd["text_projection.weight"],
                   n_head, eps)

    @classmethod
    def from_openai_state_dict(cls, sd, eps=LN_EPS):
        """sd: the `clip` package's keys (what the reference's Lightning checkpoints carry under `textencoder.clip_model.`, see
        checkpoint.extract_clip_text_tower): fp16 tensors are widened, `text_projection` ([C][P], applied as x @ P) is transposed,
        heads = width / 64 (clip.model.CLIP: transformer_heads = transformer_width // 64), `visual.*` keys are ignored."""
        layers = layers_from_openai(sd, "transformer.resblocks.")
        width = sd["token_embedding.weight"].shape[1]
        if width % 64:
            raise GsddError(f"ClipTextTower: the clip package uses width / 64 heads; width {width} is not a multiple of 64")
        return cls(sd["token_embedding.weight"], sd["positional_embedding"], layers, sd["ln_final.weight"], sd["ln_final.bias"],
                   _f32(sd["text_projection"]).t(), width // 64, eps)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, ids, eot=None, trim=True, tokens=False):
        """ids: int64 (B, S <= 77), on the host or on the tower's device; eot: int64 (B,) end-of-text positions, default the first
        position holding the row's largest id (`text.argmax(dim=-1)` of encode_text) -> (B, P) fp32 on the tower's device.
        trim=False runs the whole width of `ids` instead of the first max(eot) + 1 positions (the result does not depend on it).
        tokens=True: the per-token features instead -- the final LayerNorm of every position that ran, (B, S, width) fp32, no projection
        and no pooling (upstream VQ-Diffusion's condition; a position sees only the ones before it, so a row does not depend on S)."""
        self._need_device("forward")
        if ids.dim() != 2 or ids.dtype != torch.int64:
            raise GsddError(f"ClipTextTower.forward: ids must be an int64 (B, S) matrix, got {ids.dtype} {tuple(ids.shape)}")
        B, width = ids.shape
        if not 1 <= width <= MAX_CONTEXT:
            raise GsddError(f"ClipTextTower.forward: context of {width} positions, 1 .. {MAX_CONTEXT} supported")
        ids_host = ids.detach().cpu().contiguous()               # (a copy only if the caller's ids live on the device)
        eot_host = ids_host.argmax(dim=1) if eot is None else torch.as_tensor(eot).detach().cpu().to(torch.int64).contiguous()
        if tuple(eot_host.shape) != (B,) or int(eot_host.min()) < 0 or int(eot_host.max()) >= width:
            raise GsddError(f"ClipTextTower.forward: eot must hold {B} positions inside [0, {width})")
        S = int(eot_host.max()) + 1 if trim else width
        if S > self.pos_emb.shape[0]:
            raise GsddError(f"ClipTextTower.forward: {S} positions, the tower has {self.pos_emb.shape[0]} position embeddings")
        dev = self.device
        ids_dev = ids.contiguous() if ids.device == dev else ids_host.to(dev)
        eot_dev = eot_host.to(dev)
        buf = self._get_buffers(B, S)
        x, stats = buf["x"], buf["stats"]
        ops.text_embed(ids_dev, self.tok_emb, self.pos_emb, x, S, ids_host=ids_host)
        run_resblocks(self.layers, ops.text_attention, buf, B, S, self.n_head, self.eps)
        if tokens:
            ops.row_stats(x, stats, eps=self.eps)
            return ops.ln_apply(x, stats, self.gf, self.bf).view(B, S, self.width)
        return self._pool_project(buf, eot_dev, eot_host, B, S, self.gf, self.bf)

    __call__ = forward
