"""What the two CLIP towers (text.py, vision.py) share: the per-layer operands and their import from both checkpoint layouts, the pre-LN
residual blocks, and a base class with the validation, the device moves, the scratch buffers and the "one row per sequence, final
LayerNorm, projection" tail.  Each tower keeps its own ends: embedding, context trimming or frame preprocessing, and `forward`."""
import re

import torch

from . import ops
from ._lib import GsddError

MAX_POSITIONS = 77                        # the rows the attention kernel's LDS images hold (csrc/clip_attention.hip)
LN_EPS = 1e-5

# per-layer operands other than the fused q|k|v: (weight, bias, module in the `transformers` layout, module in the `clip` package's)
_LAYER_MODULES = (("wo", "bo", "self_attn.out_proj", "attn.out_proj"), ("g1", "be1", "layer_norm1", "ln_1"), ("g2", "be2", "layer_norm2", "ln_2"),
                  ("w1", "b1", "mlp.fc1", "mlp.c_fc"), ("w2", "b2", "mlp.fc2", "mlp.c_proj"))


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def hf_layers_to_openai(sd, src, dst):
    """The layers `src`N.* of a `transformers` CLIP state dict under the `clip` package's keys `dst`N.* (q | k | v concatenated into
    in_proj); src / dst: e.g. "text_model.encoder.layers." / "transformer.resblocks."."""
    out, n = {}, 0
    while f"{src}{n}.layer_norm1.weight" in sd:
        s, d = f"{src}{n}.", f"{dst}{n}."
        for wb in ("weight", "bias"):
            out[d + "attn.in_proj_" + wb] = torch.cat([sd[s + f"self_attn.{x}_proj.{wb}"] for x in "qkv"], dim=0)
            for _, _, a, b in _LAYER_MODULES:
                out[d + f"{b}.{wb}"] = sd[s + f"{a}.{wb}"]
        n += 1
    return out


def layers_from_openai(sd, prefix):
    """Per-layer operand dicts from the `clip` package's keys `prefix`N.* ("transformer.resblocks." / "visual.transformer.resblocks.")."""
    pat = re.compile("^" + re.escape(prefix) + r"(\d+)\.ln_1\.weight$")
    n_layer = 1 + max((int(m.group(1)) for m in map(pat.match, sd) if m), default=-1)
    layers = []
    for n in range(n_layer):
        p = f"{prefix}{n}."
        lay = {"wqkv": sd[p + "attn.in_proj_weight"], "bqkv": sd[p + "attn.in_proj_bias"]}
        for w, b, _, mod in _LAYER_MODULES:
            lay[w], lay[b] = sd[p + mod + ".weight"], sd[p + mod + ".bias"]
        layers.append(lay)
    return layers


def layers_from_hf(sd, prefix):
    """Per-layer operand dicts from the `transformers` keys `prefix`N.* ("text_model.encoder.layers." / "vision_model.encoder.layers.")."""
    return layers_from_openai(hf_layers_to_openai(sd, prefix, ""), "")


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


class ClipTower:
    """The frozen fp32 transformer of a CLIP tower.  A subclass sets its own tensors (named in `_VECTORS`, the first one deciding
    `device`, `proj` [P][C] among them) and `width`, then calls `_set_layers` and `_check_shapes`."""

    _VECTORS = ()

    def _set_layers(self, layers, n_head, eps):
        self.layers = [{k: _f32(v) for k, v in lay.items()} for lay in layers]
        self.n_head, self.eps = int(n_head), float(eps)
        self._buffers = {}
        if not self.layers:
            raise GsddError(f"{type(self).__name__}: no transformer layers found in the state dict")

    def _check_shapes(self, widths_match):
        name = type(self).__name__
        if self.width % self.n_head or self.width // self.n_head not in (64, 32, 16):
            raise GsddError(f"{name}: width {self.width} over {self.n_head} heads gives a head dimension other than 64, 32 or 16")
        if not widths_match:
            raise GsddError(f"{name}: embedding / projection widths do not match")
        for lay in self.layers:
            if tuple(lay["wqkv"].shape) != (3 * self.width, self.width) or lay["w2"].shape[1] != lay["w1"].shape[0] \
                    or lay["w1"].shape[0] != self.layers[0]["w1"].shape[0]:
                raise GsddError(f"{name}: layer operand shapes do not match the tower's width")

    def to(self, device):
        dev = torch.device(device)
        for k in self._VECTORS:
            setattr(self, k, getattr(self, k).to(dev))
        self.layers = [{k: v.to(dev) for k, v in lay.items()} for lay in self.layers]
        self._buffers = {}
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    @property
    def device(self):
        return getattr(self, self._VECTORS[0]).device

    def _need_device(self, what):
        if not self.device.type == "cuda":
            raise GsddError(f"{type(self).__name__}.{what} needs the weights on a ROCm device (no CPU fallback): call .to(device) first")

    def _extra_buffers(self, B, S, f):
        return {}

    def _get_buffers(self, B, S):
        """Scratch for B sequences of S positions, kept per (B, S)."""
        buf = self._buffers.get((B, S))
        if buf is None:
            f = dict(dtype=torch.float32, device=self.device)
            Cw, M, inner = self.width, B * S, self.layers[0]["w1"].shape[0]
            buf = {"x": torch.empty((M, Cw), **f), "y": torch.empty((M, Cw), **f), "qkv": torch.empty((M, 3 * Cw), **f),
                   "att": torch.empty((M, Cw), **f), "h": torch.empty((M, inner), **f), "stats": torch.empty((M, 2), **f),
                   "pooled": torch.empty((B, Cw), **f), "pstats": torch.empty((B, 2), **f), **self._extra_buffers(B, S, f)}
            self._buffers[(B, S)] = buf
        return buf

    def _pool_project(self, buf, pos, pos_host, B, S, gamma, beta):
        """Row pos[b] of every sequence in buf["x"], its LayerNorm (per row, so it runs on these B rows only) and the projection -> (B, P)."""
        ops.text_pool(buf["x"], pos, B, S, buf["pooled"], eot_host=pos_host)
        ops.row_stats(buf["pooled"], buf["pstats"], eps=self.eps)
        out = torch.empty((B, self.proj.shape[0]), dtype=torch.float32, device=self.device)
        ops.linear(buf["pooled"], self.proj, out, ln=(buf["pstats"], gamma, beta, None, 0))
        return out
