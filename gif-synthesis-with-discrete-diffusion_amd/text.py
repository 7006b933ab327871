"""The CLIP text tower on the HIP path: `clip.model.CLIP.encode_text` (token + position embedding, pre-LN causal transformer with
QuickGELU, final LayerNorm, the row at the end-of-text token, the text projection), which the reference calls at
src/models/text_models/clip_text_embedding.py:56-65.

Every computation is a kernel of libgsdd.so: gsdd_text_embed / gsdd_text_attention / gsdd_text_pool (csrc/text_tower.hip) and, for
the linears with their LayerNorm prologue, bias, QuickGELU (activation 2) and residual, gsdd_row_stats + gsdd_gemm.  The arithmetic
is fp32 throughout; the reference runs the same tower in fp16 (`clip.model.convert_weights`).

Context trimming: under the causal mask nothing behind a row's end-of-text position reaches it, so only the first
S_eff = max(eot) + 1 positions of the batch are run (at the reference's recipe, start + 20 + end, at most 22 of 77).  `eot` is taken
from the ids on the host, where the tokenizer has just produced them, so choosing S_eff costs no device synchronisation."""
import re

import torch

from . import ops
from ._lib import GsddError

MAX_CONTEXT = 77
LN_EPS = 1e-5


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def hf_to_openai_state_dict(sd):
    """Keys of transformers.CLIPTextModelWithProjection -> the `clip` package's text-tower keys (q|k|v concatenated into in_proj,
    text_projection transposed to [C][P]).  The inverse of what from_openai_state_dict undoes; used by tests and by exporters."""
    out = {"token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
           "positional_embedding": sd["text_model.embeddings.position_embedding.weight"],
           "ln_final.weight": sd["text_model.final_layer_norm.weight"], "ln_final.bias": sd["text_model.final_layer_norm.bias"],
           "text_projection": sd["text_projection.weight"].t().contiguous()}
    n = 0
    while f"text_model.encoder.layers.{n}.layer_norm1.weight" in sd:
        s, d = f"text_model.encoder.layers.{n}.", f"transformer.resblocks.{n}."
        for wb in ("weight", "bias"):
            out[d + "attn.in_proj_" + wb] = torch.cat([sd[s + f"self_attn.{x}_proj.{wb}"] for x in "qkv"], dim=0)
            for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"),
                         ("mlp.fc1", "mlp.c_fc"), ("mlp.fc2", "mlp.c_proj")):
                out[d + f"{b}.{wb}"] = sd[s + f"{a}.{wb}"]
        n += 1
    return out


def run_resblocks(layers, attention, buf, B, S, n_head, eps):
    """CLIP's pre-LN residual blocks over the rows in buf["x"] ([B*S][C], updated in place; y / qkv / att / h / stats are scratch):
    LayerNorm folded into the q|k|v linear, `attention` (ops.text_attention: causal, the text tower; ops.clip_attention: every key, the
    image tower), output linear + residual, LayerNorm folded into fc1 with QuickGELU, fc2 + residual.  Shared by both towers."""
    x, y, qkv, att, h, stats = (buf[k] for k in ("x", "y", "qkv", "att", "h", "stats"))
    for lay in layers:
        ops.row_stats(x, stats, eps=eps)
        ops.linear(x, lay["wqkv"], qkv, bias=lay["bqkv"], ln=(stats, lay["g1"], lay["be1"], None, 0))
        attention(qkv, B, S, n_head, att)
        ops.linear(att, lay["wo"], y, bias=lay["bo"], residual=x)
        ops.row_stats(y, stats, eps=eps)
        ops.linear(y, lay["w1"], h, bias=lay["b1"], ln=(stats, lay["g2"], lay["be2"], None, 0), act=ops.ACT_GELU2)
        ops.linear(h, lay["w2"], x, bias=lay["b2"], residual=y)
    return x


class ClipTextTower:
    """Frozen fp32 device weights of a CLIP text tower and its forward pass on the HIP kernels.

    Operands per layer: `wqkv` [3C][C] / `bqkv` [3C] (q | k | v fused), `wo` / `bo`, `w1` / `b1` (fc1, [I][C]), `w2` / `b2`
    (fc2, [C][I]), `g1` / `be1` and `g2` / `be2` (the two LayerNorms); `tok_emb` [vocab][C], `pos_emb` [n_pos][C], `gf` / `bf` (final
    LayerNorm), `proj` [P][C] (applied as x @ proj.T, no bias)."""

    def __init__(self, tok_emb, pos_emb, layers, gf, bf, proj, n_head, eps=LN_EPS):
        self.tok_emb, self.pos_emb, self.gf, self.bf, self.proj = _f32(tok_emb), _f32(pos_emb), _f32(gf), _f32(bf), _f32(proj)
        self.layers = [{k: _f32(v) for k, v in lay.items()} for lay in layers]
        self.n_head, self.eps = int(n_head), float(eps)
        self.width = self.tok_emb.shape[1]
        if not self.layers:
            raise GsddError("ClipTextTower: no transformer layers found in the state dict")
        if self.width % self.n_head or self.width // self.n_head not in (64, 32, 16):
            raise GsddError(f"ClipTextTower: width {self.width} over {self.n_head} heads gives a head dimension other than 64, 32 or 16")
        if self.proj.shape[1] != self.width or self.pos_emb.shape[1] != self.width:
            raise GsddError("ClipTextTower: embedding / projection widths do not match")
        for lay in self.layers:
            if tuple(lay["wqkv"].shape) != (3 * self.width, self.width) or lay["w2"].shape[1] != lay["w1"].shape[0] \
                    or lay["w1"].shape[0] != self.layers[0]["w1"].shape[0]:
                raise GsddError("ClipTextTower: layer operand shapes do not match the tower's width")
        self._buffers = {}

    # ------------------------------------------------------------------ weight import
    @classmethod
    def from_hf_state_dict(cls, sd, n_head, eps=LN_EPS):
        """sd: state dict of transformers.CLIPTextModelWithProjection (text_model.embeddings.*, text_model.encoder.layers.N.*,
        text_model.final_layer_norm.*, text_projection.weight).  The head count is not recoverable from the tensors."""
        layers, n = [], 0
        while f"text_model.encoder.layers.{n}.layer_norm1.weight" in sd:
            p = f"text_model.encoder.layers.{n}."
            layers.append({
                "wqkv": torch.cat([_f32(sd[p + f"self_attn.{x}_proj.weight"]) for x in "qkv"], dim=0),
                "bqkv": torch.cat([_f32(sd[p + f"self_attn.{x}_proj.bias"]) for x in "qkv"], dim=0),
                "wo": sd[p + "self_attn.out_proj.weight"], "bo": sd[p + "self_attn.out_proj.bias"],
                "g1": sd[p + "layer_norm1.weight"], "be1": sd[p + "layer_norm1.bias"],
                "g2": sd[p + "layer_norm2.weight"], "be2": sd[p + "layer_norm2.bias"],
                "w1": sd[p + "mlp.fc1.weight"], "b1": sd[p + "mlp.fc1.bias"],
                "w2": sd[p + "mlp.fc2.weight"], "b2": sd[p + "mlp.fc2.bias"]})
            n += 1
        return cls(sd["text_model.embeddings.token_embedding.weight"], sd["text_model.embeddings.position_embedding.weight"], layers,
                   sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"], sd["text_projection.weight"],
                   n_head, eps)

    @classmethod
    def from_openai_state_dict(cls, sd, eps=LN_EPS):
        """sd: the `clip` package's keys (what the reference's Lightning checkpoints carry under `textencoder.clip_model.`, see
        checkpoint.extract_clip_text_tower): fp16 tensors are widened, `text_projection` ([C][P], applied as x @ P) is transposed,
        heads = width / 64 (clip.model.CLIP: transformer_heads = transformer_width // 64), `visual.*` keys are ignored."""
        pat = re.compile(r"^transformer\.resblocks\.(\d+)\.ln_1\.weight$")
        n_layer = 1 + max((int(m.group(1)) for m in map(pat.match, sd) if m), default=-1)
        layers = []
        for n in range(n_layer):
            p = f"transformer.resblocks.{n}."
            layers.append({
                "wqkv": sd[p + "attn.in_proj_weight"], "bqkv": sd[p + "attn.in_proj_bias"],
                "wo": sd[p + "attn.out_proj.weight"], "bo": sd[p + "attn.out_proj.bias"],
                "g1": sd[p + "ln_1.weight"], "be1": sd[p + "ln_1.bias"], "g2": sd[p + "ln_2.weight"], "be2": sd[p + "ln_2.bias"],
                "w1": sd[p + "mlp.c_fc.weight"], "b1": sd[p + "mlp.c_fc.bias"],
                "w2": sd[p + "mlp.c_proj.weight"], "b2": sd[p + "mlp.c_proj.bias"]})
        width = sd["token_embedding.weight"].shape[1]
        if width % 64:
            raise GsddError(f"ClipTextTower: the clip package uses width / 64 heads; width {width} is not a multiple of 64")
        return cls(sd["token_embedding.weight"], sd["positional_embedding"], layers, sd["ln_final.weight"], sd["ln_final.bias"],
                   _f32(sd["text_projection"]).t(), width // 64, eps)

    def to(self, device):
        dev = torch.device(device)
        for k in ("tok_emb", "pos_emb", "gf", "bf", "proj"):
            setattr(self, k, getattr(self, k).to(dev))
        self.layers = [{k: v.to(dev) for k, v in lay.items()} for lay in self.layers]
        self._buffers = {}
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    @property
    def device(self):
        return self.tok_emb.device

    # ------------------------------------------------------------------ forward
    def _get_buffers(self, B, S):
        buf = self._buffers.get((B, S))
        if buf is None:
            f = dict(dtype=torch.float32, device=self.device)
            Cw, M, inner = self.width, B * S, self.layers[0]["w1"].shape[0]
            buf = {"x": torch.empty((M, Cw), **f), "y": torch.empty((M, Cw), **f), "qkv": torch.empty((M, 3 * Cw), **f),
                   "att": torch.empty((M, Cw), **f), "h": torch.empty((M, inner), **f), "stats": torch.empty((M, 2), **f),
                   "pooled": torch.empty((B, Cw), **f), "pstats": torch.empty((B, 2), **f)}
            self._buffers[(B, S)] = buf
        return buf

    @torch.no_grad()
    def forward(self, ids, eot=None, trim=True, tokens=False):
        """ids: int64 (B, S <= 77), on the host or on the tower's device; eot: int64 (B,) end-of-text positions, default the first
        position holding the row's largest id (`text.argmax(dim=-1)` of encode_text) -> (B, P) fp32 on the tower's device.
        trim=False runs the whole width of `ids` instead of the first max(eot) + 1 positions (the result does not depend on it).
        tokens=True: the per-token features instead -- the final LayerNorm of every position that ran, (B, S, width) fp32, no projection
        and no pooling (upstream VQ-Diffusion's condition; a position sees only the ones before it, so a row does not depend on S)."""
        if not self.device.type == "cuda":
            raise GsddError("ClipTextTower.forward needs the weights on a ROCm device (no CPU fallback): call .to(device) first")
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
        ops.text_pool(x, eot_dev, B, S, buf["pooled"], eot_host=eot_host)
        ops.row_stats(buf["pooled"], buf["pstats"], eps=self.eps)
        out = torch.empty((B, self.proj.shape[0]), dtype=torch.float32, device=dev)
        ops.linear(buf["pooled"], self.proj, out, ln=(buf["pstats"], self.gf, self.bf, None, 0))
        return out

    __call__ = forward
