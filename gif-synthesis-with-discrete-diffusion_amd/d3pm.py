"""D3PM denoiser + discrete-diffusion shells with the reference's constructors, method names and
state_dict keys, computing on gfx950 through the C ABI.

Reference: src/models/motionencoder/{dalle_mask_image_embedding,transformer_utils,diffusion_transformer}.py and
src/models/networks/discrete_diffusion.py.  The nn.Module tree only owns parameters under the
reference's names.  A sampling chain is a program: the tuple of op kinds a plan lists in order of
execution ("step", "jump", "reveal", "final", and "slide" between two windows of a long rollout).  Every op of a kind is the same launch sequence driven by device counters (the
timestep, the Philox stream id), so `issue_schedule` has each lane run a kind eagerly once, capture it into a hipGraph if it
recurs, and replay it from then on; `DiffusionTransformer._sample_once` walks that schedule.
"""
import collections
import collections.abc
import contextlib
import ctypes
import math
import numbers
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import GsddError, _is_int


@contextlib.contextmanager
def _timed(ws, name, stream):
    """bench.py's in-situ timing: with ws["events"] = {} present, a HIP event pair on the launch stream brackets the launches made
    inside the block and is appended to ws["events"][name]; otherwise (always, in the product path) nothing happens."""
    ev = ws.get("events") if name is not None else None
    if ev is None:
        yield
        return
    pair = (ops.Event(), ops.Event())
    pair[0].record(stream)
    yield
    pair[1].record(stream)
    ev.setdefault(name, []).append(pair)


# ----------------------------------------------------------------------------- parameter containers
class DalleMaskImageEmbedding(nn.Module):
    """dalle_mask_image_embedding.py:27-57 (num_embed+1 rows, last = [MASK])."""

    def __init__(self, num_embed=8192, spatial_size=[32, 32], embed_dim=3968, trainable=True,
                 pos_emb_type="embedding"):
        super().__init__()
        if isinstance(spatial_size, int):
            spatial_size = [spatial_size, spatial_size]
        if pos_emb_type != "embedding":
            raise NotImplementedError("only pos_emb_type='embedding' is used by the reference configs")
        self.spatial_size = list(spatial_size)
        self.num_embed = num_embed + 1
        self.embed_dim = embed_dim
        self.trainable = trainable
        self.pos_emb_type = pos_emb_type
        self.emb = nn.Embedding(self.num_embed, embed_dim)
        self.height_emb = nn.Embedding(self.spatial_size[0], embed_dim)
        self.width_emb = nn.Embedding(self.spatial_size[1], embed_dim)
        if not trainable:
            for p in self.parameters():
                p.requires_grad = False

    def pos_table(self, L):
        """(height_emb[p // W] + width_emb[p % W])[:L]  (dalle_mask_image_embedding.py:70-77)"""
        Hs, Ws = self.spatial_size
        if Hs * Ws < L:
            raise GsddError(f"spatial_size {self.spatial_size} has fewer than content_seq_len={L} positions")
        pos = (self.height_emb.weight.unsqueeze(1) + self.width_emb.weight.unsqueeze(0)).view(Hs * Ws, -1)
        return pos[:L].contiguous()


class AdaLayerNorm(nn.Module):
    """transformer_utils.py:138-149 (timestep_type='adalayernorm' -> nn.Embedding)."""

    def __init__(self, n_embd, diffusion_step, emb_type="adalayernorm"):
        super().__init__()
        if "abs" in emb_type:
            raise NotImplementedError("sinusoidal timestep embedding is not used by the reference configs")
        self.emb = nn.Embedding(diffusion_step, n_embd)
        self.linear = nn.Linear(n_embd, n_embd * 2)
        self.diff_step = diffusion_step


class _Attention(nn.Module):
    def __init__(self, n_embd, kv_dim):
        super().__init__()
        self.key = nn.Linear(kv_dim, n_embd)
        self.query = nn.Linear(n_embd, n_embd)
        self.value = nn.Linear(kv_dim, n_embd)
        self.proj = nn.Linear(n_embd, n_embd)


class Block(nn.Module):
    """transformer_utils.py:178-264, attn_type='selfcross'."""

    def __init__(self, n_embd, n_head, condition_dim, diffusion_step, timestep_type, mlp_hidden_times):
        super().__init__()
        self.ln1 = AdaLayerNorm(n_embd, diffusion_step, timestep_type)
        self.ln2 = nn.LayerNorm(n_embd)
        self.attn1 = _Attention(n_embd, n_embd)
        self.attn2 = _Attention(n_embd, condition_dim)
        self.ln1_1 = AdaLayerNorm(n_embd, diffusion_step, timestep_type)
        self.mlp = nn.Sequential(nn.Linear(n_embd, mlp_hidden_times * n_embd), nn.Identity(),
                                 nn.Linear(mlp_hidden_times * n_embd, n_embd), nn.Identity())


class Text2ImageTransformer(nn.Module):
    """Drop-in for transformer_utils.py:299-444.  forward(input, cond_emb, t) -> logits (B, K, L)."""

    def __init__(self, dalle, condition_seq_len=77, n_layer=14, n_embd=1024, n_head=16, content_seq_len=1024,
                 attn_pdrop=0, resid_pdrop=0, mlp_hidden_times=4, block_activate=None, attn_type="selfcross",
                 content_spatial_size=[32, 32], condition_dim=512, diffusion_step=1000, timestep_type="adalayernorm",
                 mlp_type="fc", checkpoint=False):
        super().__init__()
        if attn_type != "selfcross" or mlp_type != "fc" or block_activate != "GELU2":
            raise NotImplementedError("only attn_type='selfcross', mlp_type='fc', block_activate='GELU2' "
                                      "(the reference configs) are built")
        if n_embd % n_head != 0 or n_embd // n_head != 4:
            raise NotImplementedError("the HIP attention kernel is specialised for head dim 4 (n_embd 64, 16 heads)")
        if attn_pdrop != 0 or resid_pdrop != 0:
            raise NotImplementedError("dropout > 0 is not used by the reference configs")
        self.content_emb = dalle
        self.n_layer, self.n_embd, self.n_head = n_layer, n_embd, n_head
        self.blocks = nn.Sequential(*[Block(n_embd, n_head, condition_dim, diffusion_step, timestep_type,
                                            mlp_hidden_times) for _ in range(n_layer)])
        out_cls = self.content_emb.num_embed - 1
        self.to_logits = nn.Sequential(nn.LayerNorm(n_embd), nn.Linear(n_embd, out_cls))
        self.condition_seq_len, self.content_seq_len = condition_seq_len, content_seq_len
        self.condition_dim, self.diffusion_step = condition_dim, diffusion_step
        self.apply(self._init_weights)
        self._packed, self._packed_key = None, None
        # how the softmax probabilities enter P.V in the self-attention kernel (include/gsdd.h, GSDD_ATTN_*): None = the library's
        # default (adaptive lo half for L >= 2048, f16 hi + lo below), or 'a8' | '22' | '11' | 'a12'.  '11' (f16 hi only everywhere) is
        # the fastest and data-independent: within the 1e-4 logits contract on every pinned case, not within the kernel's own 2e-5 bar
        # on peaked rows.  The environment variable GSDD_ATTN_P overrides None.
        self.attention_mode = None
        # set by demote_to_x3p (an activation left the f16 operand range of the default layer kernel): this model keeps the bf16x3 layer
        # kernel across re-packs -- every optimizer step re-packs -- until a state dict is loaded into it
        self._range_demoted = False
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_range_demoted", False))

    @staticmethod
    def _init_weights(module):                       # transformer_utils.py:363-371
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if isinstance(module, nn.Linear) and module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm) and module.elementwise_affine:
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    # ------------------------------------------------------------------ packed weights
    def packed(self):
        key = tuple((t.data_ptr(), t._version) for t in self.parameters())
        if self._packed is None or key != self._packed_key:
            with torch.no_grad():
                self._packed = self._pack()
            self._packed_key = key
        return self._packed

    def _pack(self):
        p = {"pos": self.content_emb.pos_table(self.content_seq_len), "emb": self.content_emb.emb.weight.contiguous(),
             "layers": []}
        for blk in self.blocks:
            a1, a2 = blk.attn1, blk.attn2
            lay = dict(
                ada1=ops.adaln_table(blk.ln1.emb.weight.contiguous(), blk.ln1.linear.weight.contiguous(),
                                     blk.ln1.linear.bias.contiguous()),
                wqkv=torch.cat([a1.query.weight, a1.key.weight, a1.value.weight], 0).contiguous(),
                bqkv=torch.cat([a1.query.bias, a1.key.bias, a1.value.bias], 0).contiguous(),
                wproj=a1.proj.weight.contiguous(), bproj=a1.proj.bias.contiguous(),
                wq2=a2.query.weight.contiguous(), bq2=a2.query.bias.contiguous(),
                wk2=a2.key.weight.contiguous(), bk2=a2.key.bias.contiguous(),
                wv2=a2.value.weight.contiguous(), bv2=a2.value.bias.contiguous(),
                wproj2=a2.proj.weight.contiguous(), bproj2=a2.proj.bias.contiguous(),
                g2=blk.ln2.weight.contiguous(), b2=blk.ln2.bias.contiguous(),
                w1=blk.mlp[0].weight.contiguous(), bb1=blk.mlp[0].bias.contiguous(),
                w2=blk.mlp[2].weight.contiguous(), bb2=blk.mlp[2].bias.contiguous())
            p["layers"].append(lay)
        p["gf"], p["bf"] = self.to_logits[0].weight.contiguous(), self.to_logits[0].bias.contiguous()
        p["wl"], p["bl"] = self.to_logits[1].weight.contiguous(), self.to_logits[1].bias.contiguous()
        return p

    def _ada2(self, li):
        """AdaLN table of block li's cross-attention norm (ln1_1).  Only the general path (more than one condition token) reads it --
        with one token the cross-attention collapses to a vector and ln1_1 drops out -- so it is made on first use, not at every re-pack
        (the training step re-packs after every update)."""
        lay = self.packed()["layers"][li]
        if "ada2" not in lay:
            blk = self.blocks[li]
            with torch.no_grad():
                lay["ada2"] = ops.adaln_table(blk.ln1_1.emb.weight.contiguous(), blk.ln1_1.linear.weight.contiguous(),
                                              blk.ln1_1.linear.bias.contiguous())
        return lay["ada2"]

    def fragment_images(self, stream=None):
        """Weight fragment images of the fused layer kernel, made on the sampler's first use after the weights changed (the training
        step re-packs every iteration and never needs them): f16 hi + lo images by default, the bf16x3 images when GSDD_LAYER=x3p
        asks for that kernel (A/B).  Enqueued on `stream`: every stream that reads them must be ordered after it (sample() builds
        them on the caller's stream before its lanes fork)."""
        layers = self.packed()["layers"]
        if not (self.n_embd == 64 and layers and layers[0]["w1"].shape[0] == 256):
            return
        want = os.environ.get("GSDD_LAYER", "h2")
        if want not in ("h2", "x3p"):
            raise GsddError(f"GSDD_LAYER={want!r}: the fused layer kernels are 'h2' (f16 hi + lo images) and 'x3p' (bf16x3 images)")
        if want == "h2" and self._range_demoted:
            want = "x3p"
        if want == "h2" and "lay_h2" not in layers[0] and "w2_x3" not in layers[0]:
            # the f16 images hold 2^8 w: a weight of 255 or more would overflow them (checked once per weight set; such a model takes
            # the bf16x3 kernel, which has f32's range)
            wmax = max(float(lay[k].abs().max()) for lay in layers for k in ("w1", "w2", "wproj", "wqkv"))
            if not wmax < 255.0:
                want = "x3p"
        elif want == "h2" and "w2_x3" in layers[0]:
            want = "x3p"
        if want == "x3p":
            if "w2_x3" not in layers[0]:
                for lay in layers:
                    lay["w2_x3"], lay["wqkv_x3"] = ops.d3pm_layer_pack(lay["w2"], lay["wproj"], lay["wqkv"], stream=stream)
        elif "lay_h2" not in layers[0]:
            for lay in layers:
                lay["lay_h2"], lay["wqkv_h2"] = ops.d3pm_layer_pack_h2(lay["w1"], lay["w2"], lay["wproj"], lay["wqkv"], stream=stream)

    def demote_to_x3p(self, stream=None):
        """The f16 hi + lo layer kernel carries activations as 16 a in f16: |a| >= 4094 (an outlier LN / GELU2 / attention output of a
        trained checkpoint) overflows.  The kernel flags that (LayerDesc.range_flag) and the caller lands here: this weight set takes the
        bf16x3 kernel, which has f32's range, until a state dict is loaded (the decision survives re-packs: a training loop's validation
        pass would otherwise try the f16 images again after every optimizer step and run everything twice).  -> True if anything changed."""
        self._range_demoted = True
        layers = self.packed()["layers"]
        if not layers or "lay_h2" not in layers[0]:
            return False
        for lay in layers:
            lay.pop("lay_h2", None), lay.pop("wqkv_h2", None)
            lay["w2_x3"], lay["wqkv_x3"] = ops.d3pm_layer_pack(lay["w2"], lay["wproj"], lay["wqkv"], stream=stream)
        self.range_demotions = getattr(self, "range_demotions", 0) + 1
        return True

    def run_checked(self, tok, condv, Te, t2, ws, rep=1, stream=None, cond_len=None):
        """run() + the range screen of the f16 hi + lo layer kernel (one 4-byte read back: eager callers only -- forward(),
        p_sample_tokens, the no-grad objective; sample() checks once per call, after its captured loop, and the gradient path
        (d3pm_train.py) does not use the fused layer kernel at all).  The read is a host synchronisation, kept because the caller
        gets these logits: a demoted model (see demote_to_x3p) pays it without ever re-running."""
        logits = self.run(tok, condv, Te, t2, ws, rep=rep, stream=stream, cond_len=cond_len)
        if int(ws["range"].item()) != 0:
            ws["range"].zero_()
            if not self.demote_to_x3p(stream):
                raise GsddError("non-finite activations in the denoiser (inf / NaN in the inputs or weights?)")
            logits = self.run(tok, condv, Te, t2, ws, rep=rep, stream=stream, cond_len=cond_len)
        return logits

    # ------------------------------------------------------------------ one denoiser pass on the HIP path
    def cond_vectors(self, cond):
        """Per-layer cross-attention operands of the condition tokens (B2, Te, cond_dim).
        Te == 1: softmax over one key is exactly 1, so attn2 adds proj(value(cond)) to every position
        (transformer_utils.py:95-113) -> [n_layer] tensors (B2, D).  Te > 1: (keys, values) rows."""
        p = self.packed()
        B2, Te, cd = cond.shape
        flat = cond.reshape(B2 * Te, cd).contiguous().float()
        out = []
        for lay in p["layers"]:
            v = ops.small_linear(flat, lay["wv2"], lay["bv2"])
            if Te == 1:
                out.append(ops.small_linear(v, lay["wproj2"], lay["bproj2"]))
            else:
                out.append((ops.small_linear(flat, lay["wk2"], lay["bk2"]), v))
        return out

    def run(self, tok, condv, Te, t2, ws, rep=1, stream=None, cond_len=None):
        """tok (B,L) int64; the pass runs on `rep` stacked copies of the batch (B2 = rep*B rows of cond).
        t2: int64 [B2] timesteps on device.  ws: workspace dict from `workspace()`.  -> logits [B2*L][K].
        cond_len: None, or int32 [B2] on the device with Te > 1 -- row b's cross-attention runs over its first cond_len[b] condition
        tokens only and never reads the others (the kernels clamp a value outside [1, Te]; callers with a host copy check it first,
        see check_condition_len)."""
        p = self.packed()
        B, L = tok.shape
        B2, D, H = rep * B, self.n_embd, self.n_head
        if cond_len is not None:
            if Te == 1:
                raise GsddError("cond_len needs more than one condition token: with Te = 1 pass None (forward() checks it is all ones)")
            if cond_len.dtype != torch.int32 or tuple(cond_len.shape) != (B2,) or not cond_len.is_cuda:
                raise GsddError(f"cond_len must be an int32 device tensor of shape ({B2},), got {cond_len.dtype} {tuple(cond_len.shape)}")
        M = B2 * L
        x, stats, qkv, y, hbuf, logits = ws["x"], ws["stats"], ws["qkv"], ws["y"], ws["h"], ws["logits"]
        ops.d3pm_embed(tok, p["emb"], p["pos"], x, rep=rep, stream=stream)
        layers = p["layers"]
        if Te == 1 and D == 64 and hbuf.shape[1] == 256:
            self.fragment_images(stream)
            # fused path: [AdaLN+qkv] for block 0, then per block attention + one fused kernel that also emits the
            # next block's q|k|v
            # The `rep` stacked copies (classifier-free guidance: conditional + unconditional) share tokens and timesteps, so
            # block 0's q|k|v and self-attention output are identical in every copy: computed once, then copied.
            M1 = B * L
            share0 = rep > 1 and "qkv0" in ws
            # The fused layer kernel writes k and v straight into the attention workspace as the matrix-pipe kernel's pre-split
            # images (no f32 k|v rows, no pre-split pass); block 0 runs its q|k|v stage alone on the embedding
            attn_ws = ws.get("attn")
            amode = ops.attn_mode(self.attention_mode)
            img = (attn_ws is not None and L % 32 == 0
                   and all(("lay_h2" in l and "wqkv_h2" in l) or ("w2_x3" in l and "wqkv_x3" in l) for l in layers)
                   and amode != ops.abi.ATTN_F32PV)
            x0, q0 = (x[:M1], ws["qkv0"]) if share0 else (x, qkv)
            if img:
                ops.d3pm_layer(None, x0, L, None, nxt=layers[0], t2=t2, qkv=q0, kv_img=attn_ws, range_flag=ws.get("range"), stream=stream)
            else:
                ops.row_stats(x0, stats, stream=stream)
                ops.linear(x0, layers[0]["wqkv"], q0, bias=layers[0]["bqkv"],
                           ln=(stats, layers[0]["ada1"].view(-1), layers[0]["ada1"].view(-1)[D:], t2, 2 * D),
                           rows_per_batch=L, out_mode=2, stream=stream)
            for li, lay in enumerate(layers):
                if li == 0 and share0:
                    if img:
                        ops.d3pm_attention(q0[0:H], None, None, B, L, H, y, ws=attn_ws, redo=ws.get("redo"), mode=amode, stream=stream)
                    else:
                        ops.d3pm_attention(q0[0:H], q0[H:2 * H], q0[2 * H:3 * H], B, L, H, y, ws=attn_ws, redo=ws.get("redo"), mode=amode, stream=stream)
                    with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else contextlib.nullcontext():
                        for r in range(1, rep):
                            y[r * M1:(r + 1) * M1].copy_(y[:M1])
                else:
                    with _timed(ws, "attention", stream):      # bench.py: HIP events around the dominant kernel, in situ
                        if img:
                            ops.d3pm_attention(qkv[0:H], None, None, B2, L, H, y, ws=attn_ws, redo=ws.get("redo"), mode=amode, stream=stream)
                        else:
                            ops.d3pm_attention(qkv[0:H], qkv[H:2 * H], qkv[2 * H:3 * H], B2, L, H, y, ws=attn_ws, redo=ws.get("redo"), mode=amode, stream=stream)
                nxt = layers[li + 1] if li + 1 < len(layers) else None
                with _timed(ws, "layer" if nxt is not None else None, stream):
                    ops.d3pm_layer(y, x, L, lay, cvec=condv[li], nxt=nxt, t2=t2, qkv=qkv, kv_img=attn_ws if img else None,
                                   range_flag=ws.get("range"), stream=stream)
        else:
            self._run_blocks_unfused(layers, condv, Te, t2, ws, B2, L, stream, cond_len)
        if D == 64 and p["wl"].shape[0] % 4 == 0:
            with _timed(ws, "logits", stream):
                ops.d3pm_logits(x, p["gf"], p["bf"], p["wl"], p["bl"], logits, stream=stream)
        else:
            ops.row_stats(x, stats, stream=stream)
            ops.linear(x, p["wl"], logits, bias=p["bl"], ln=(stats, p["gf"], p["bf"], None, 0), stream=stream)
        return logits

    def _run_blocks_unfused(self, layers, condv, Te, t2, ws, B2, L, stream, cond_len=None):
        """General path (any T_E): one launch per operator (transformer_utils.py:266-282 in order)."""
        D, H = self.n_embd, self.n_head
        x, stats, qkv, y, hbuf = ws["x"], ws["stats"], ws["qkv"], ws["y"], ws["h"]
        for li, lay in enumerate(layers):
            ops.row_stats(x, stats, stream=stream)
            ops.linear(x, lay["wqkv"], qkv, bias=lay["bqkv"],
                       ln=(stats, lay["ada1"].view(-1), lay["ada1"].view(-1)[D:], t2, 2 * D),
                       rows_per_batch=L, out_mode=2, stream=stream)
            ops.d3pm_attention(qkv[0:H], qkv[H:2 * H], qkv[2 * H:3 * H], B2, L, H, y, ws=ws.get("attn"), redo=ws.get("redo"),
                               mode=ops.attn_mode(self.attention_mode), stream=stream)
            if Te == 1:
                ops.linear(y, lay["wproj"], x, bias=lay["bproj"], bvec=condv[li], rows_per_batch=L, residual=x,
                           stream=stream)
            else:
                ops.linear(y, lay["wproj"], x, bias=lay["bproj"], residual=x, stream=stream)
                ops.row_stats(x, stats, stream=stream)
                q2 = qkv[0:H]
                ada2 = self._ada2(li)
                ops.linear(x, lay["wq2"], q2, bias=lay["bq2"],
                           ln=(stats, ada2.view(-1), ada2.view(-1)[D:], t2, 2 * D),
                           rows_per_batch=L, out_mode=2, stream=stream)
                ops.d3pm_cross_attention(q2, condv[li][0], condv[li][1], B2, L, Te, H, y, stream=stream, cond_len=cond_len)
                ops.linear(y, lay["wproj2"], x, bias=lay["bproj2"], residual=x, stream=stream)
            ops.row_stats(x, stats, stream=stream)
            ops.linear(x, lay["w1"], hbuf, bias=lay["bb1"], ln=(stats, lay["g2"], lay["b2"], None, 0),
                       act=ops.ACT_GELU2, stream=stream)
            ops.linear(hbuf, lay["w2"], x, bias=lay["bb2"], residual=x, stream=stream)

    def workspace(self, B2, L, device, rep=1):
        D, H = self.n_embd, self.n_head
        M = B2 * L
        K = self.content_emb.num_embed - 1
        f = dict(dtype=torch.float32, device=device)
        ws = {"x": torch.empty((M, D), **f), "stats": torch.empty((M, 2), **f),
              "qkv": torch.empty((3 * H, M, 4), **f), "y": torch.empty((M, D), **f),
              "h": torch.empty((M, self.blocks[0].mlp[0].out_features), **f),
              "logits": torch.empty((M, K), **f), "attn": ops.d3pm_attention_workspace(B2, L, H, device),
              # chunk-redo events of the attention kernel since this workspace was made (a device counter the caller owns)
              "redo": torch.zeros((1,), dtype=torch.int64, device=device),
              # set by the f16 hi + lo layer kernel when an activation left its operand range (checked by the callers of run())
              "range": torch.zeros((1,), dtype=torch.int32, device=device)}
        if rep > 1:                                  # block 0's q|k|v of one copy (the copies share it, see run())
            ws["qkv0"] = torch.empty((3 * H, M // rep, 4), **f)
        return ws

    @torch.no_grad()
    def forward(self, input, cond_emb, t, cond_len=None):
        """(B,L) int64 tokens, (B,Te,cond_dim), (B,) int64 -> logits (B, K, L) (view of [B][L][K] rows,
        like the reference's rearrange 'b l c -> b c l', transformer_utils.py:442-443).
        cond_len: None, or (B,) integers in [1, Te] -- sample b is conditioned on its first cond_len[b] tokens only; the rows of
        cond_emb behind them are never read (Te = 1: must be all ones)."""
        if not input.is_cuda:
            raise GsddError("the denoiser runs on the HIP path only: move module and inputs to a ROCm device")
        B, L = input.shape
        ws = self.workspace(B, L, input.device)
        cond_emb = cond_emb.float()
        condv = self.cond_vectors(cond_emb)
        Te = cond_emb.shape[1]
        if cond_len is not None:
            cond_len = check_condition_len(cond_len, B, Te, "cond_len")
            cond_len = cond_len.to(input.device) if Te > 1 else None          # (one token: the whole length, nothing to mask)
        logits = self.run_checked(input.contiguous(), condv, Te, t.to(input.device).long().contiguous(), ws, cond_len=cond_len)
        return logits.view(B, L, -1).transpose(1, 2)


# ----------------------------------------------------------------------------- diffusion
def alpha_schedule(time_step, N=100, att_1=0.99999, att_T=0.000009, ctt_1=0.000009, ctt_T=0.99999):
    """Linear schedule in fp64 numpy (host, init only).  Reference: diffusion_transformer.py:56-69."""
    att = np.arange(0, time_step) / (time_step - 1) * (att_T - att_1) + att_1
    att = np.concatenate(([1], att))
    at = att[1:] / att[:-1]
    ctt = np.arange(0, time_step) / (time_step - 1) * (ctt_T - ctt_1) + ctt_1
    ctt = np.concatenate(([0], ctt))
    one_minus_ctt = 1 - ctt
    ct = 1 - one_minus_ctt[1:] / one_minus_ctt[:-1]
    bt = (1 - at - ct) / N
    att = np.concatenate((att[1:], [1]))
    ctt = np.concatenate((ctt[1:], [0]))
    btt = (1 - att - ctt) / N
    return at, bt, ct, att, btt, ctt


class SamplePlan(collections.namedtuple("SamplePlan", "t0 n_steps dt post_skip q_sample")):
    """A reverse chain: the denoiser's first timestep t0, the number of steps, how far t moves per step (t <- max(t - dt, 0)),
    the posterior's skip s (it runs at t - s for t > s, else at t) and whether the start is a q_sample draw of given tokens."""
    __slots__ = ()

    @property
    def draws(self):
        """Noise streams a run spends: one per step, one more for the q_sample start."""
        return self.n_steps + (1 if self.q_sample else 0)

    @property
    def program(self):
        return ("step",) * self.n_steps


def sample_plan(T, skip_step=0, start_step=0):
    """The chain sample() / sample_fast() run, host-side and pure.
    start_step > 0: sample(filter_ratio > 0) -- q_sample at start_step - 1, then t = start_step - 1 ... 0.
    Otherwise from all-[MASK]: t = T-1, T-1-(1+s), ... down to the last value >= 0, then 0 if the list does not end there
    (diffusion_transformer.py:692-694); skip_step = 0 is sample(filter_ratio=0)."""
    if start_step:
        return SamplePlan(start_step - 1, start_step, 1, 0, True)
    n = (T - 1) // (1 + skip_step) + 1 + (1 if (T - 1) % (1 + skip_step) else 0)
    return SamplePlan(T - 1, n, 1 + skip_step, skip_step, False)


def plan_timesteps(plan):
    """-> [(t, t')]: the denoiser's and the posterior's timestep of every step of `plan`."""
    out, t = [], plan.t0
    for _ in range(plan.n_steps):
        out.append((t, t - plan.post_skip if t > plan.post_skip else t))
        t = max(t - plan.dt, 0)
    return out


class ResamplePlan(collections.namedtuple("ResamplePlan", "T jump times ops")):
    """A known-token chain with RePaint's resampling jumps: `ops` is the order of execution, ("step", t) -- the ordinary reverse step
    with the denoiser at t, which leaves the state at level t - 1 -- and ("jump", a) -- the whole state diffused forward from level a to
    a + jump.  t0, n_steps, q_sample, draws and program read like SamplePlan's; every step is the plain one (dt 1, post_skip 0)."""
    __slots__ = ()
    q_sample, dt, post_skip = False, 1, 0

    @property
    def t0(self):
        return self.T - 1

    @property
    def n_steps(self):
        return sum(1 for kind, _ in self.ops if kind == "step")

    @property
    def n_jumps(self):
        return len(self.ops) - self.n_steps

    @property
    def draws(self):
        """Noise streams a run spends: one per step and one per jump, in order of execution."""
        return len(self.ops)

    @property
    def program(self):
        return tuple(kind for kind, _ in self.ops)


def resample_plan(T, jump, times):
    """The chain sample(resample_jump=jump, resample_times=times) runs, host-side and pure (RePaint, Algorithm 1, on the levels of this
    sampler).  The landing levels T-1-m*jump (m = 1 .. (T-1)//jump, all >= 0) are each left upwards times - 1 times: whenever the
    chain arrives at one that has visits left, the state jumps forward by `jump` levels and the steps in between run again.
    T + (times-1) * jump * ((T-1)//jump) steps and (times-1) * ((T-1)//jump) jumps; never a jump from the clean level -1, the last
    op is the step at t = 0, and times = 1 is sample_plan(T)'s chain."""
    left = {T - 1 - m * jump: times - 1 for m in range(1, (T - 1) // jump + 1)}
    ops, t = [], T - 1
    while t >= 0:
        ops.append(("step", t))
        t -= 1
        if left.get(t, 0) > 0:
            left[t] -= 1
            ops.append(("jump", t))
            t += jump
    return ResamplePlan(T, jump, times, tuple(ops))


def jump_table(T, K, jump):
    """-> f32 (T + 1, 3): log(alpha~ + beta~), log(beta~), log(gamma~) of the forward move from level a to a + jump (the product of
    the one-step matrices a + 1 ... a + jump in closed form), row a mod (T + 1) -- row T is the clean level -1.  With abar / gbar the
    cumulative arrays of alpha_schedule (index T: 1 / 0): alpha~ = abar_b / abar_a, gamma~ = (gbar_b - gbar_a) / (1 - gbar_a),
    beta~ = (1 - alpha~ - gamma~) / K, all in fp64 (beta~ is a difference of numbers of size 1e-5 at the top of the schedule).  Rows
    whose target a + jump lies above T - 1 are NaN: the chain never asks for them.  What gsdd_d3pm_forward_jump reads."""
    _, _, _, att, _, ctt = alpha_schedule(T, N=K)
    out = np.full((T + 1, 3), np.nan, dtype=np.float64)
    for row in range(T + 1):
        a = -1 if row == T else row
        b = a + jump
        if b > T - 1:
            continue
        al = att[b] / att[row]
        ga = (ctt[b] - ctt[row]) / (1.0 - ctt[row])
        be = (1.0 - al - ga) / K
        out[row] = np.log(al + be), np.log(be), np.log(ga)
    return torch.from_numpy(out.astype(np.float32))


def check_resample(jump, times, T, known_mask):
    """Validates sample()'s resample_jump / resample_times.  -> None (the plain chain) or (jump, times) with times >= 2."""
    if not _is_int(times) or times < 1:
        raise GsddError(f"resample_times must be an int >= 1, got {times!r}")
    if jump is None:
        if times != 1:
            raise GsddError(f"resample_times = {times} needs resample_jump (how many levels every resampling jumps back up)")
        return None
    if not _is_int(jump) or not 1 <= jump <= T - 1:
        raise GsddError(f"resample_jump must be None or an int in [1, {T - 1}] (num_timesteps - 1), got {jump!r}")
    if known_mask is None:
        raise GsddError("resample_jump needs known_mask: resampling harmonises sampled positions with given ones")
    return (int(jump), int(times)) if times > 1 else None


class PurityPlan(collections.namedtuple("PurityPlan", "calls final rule weight")):
    """A purity-prior chain (sample() with prior_rule 1 / 2): the (t, n) of every p_sample call at t > 0 -- denoiser at t, reveal n
    [MASK] positions per sample -- whether a plain reverse step at t = 0 closes it, the rule and the prior weight r.
    n_steps, t0, q_sample, draws and program read like SamplePlan's: what the sampling loop asks of either plan."""
    __slots__ = ()
    q_sample = False                                # from all-[MASK] only

    @property
    def n_steps(self):
        return len(self.calls)

    @property
    def t0(self):
        return self.calls[0][0] if self.calls else 0

    @property
    def draws(self):
        """Two noise streams per call (candidates, selection), one more for the closing plain step."""
        return 2 * len(self.calls) + (1 if self.final else 0)

    @property
    def program(self):
        return ("reveal",) * len(self.calls) + (("final",) if self.final else ())


def window_count(window_frames, n_frames, overlap):
    """Validates the geometry of a sliding-window rollout and -> W, the number of windows: F = window_frames latent frames per window,
    consecutive windows share k = overlap of them (stride s = F - k), n = n_frames long frames: W = 1 + ceil(max(n - F, 0) / s)."""
    for name, v in (("window_frames", window_frames), ("n_frames", n_frames), ("overlap", overlap)):
        if not _is_int(v):
            raise GsddError(f"{name} must be an int, got {v!r}")
    if window_frames < 2:
        raise GsddError(f"window_frames = {window_frames}: a window needs at least 2 latent frames (one known, one to sample)")
    if not 1 <= overlap <= window_frames - 1:
        raise GsddError(f"overlap must lie in [1, {window_frames - 1}] (window_frames - 1: at least one frame is left to sample), got {overlap}")
    if n_frames < window_frames:
        raise GsddError(f"n_frames = {n_frames} is below window_frames = {window_frames}: a long clip holds at least one window")
    s = window_frames - overlap
    return 1 + (max(n_frames - window_frames, 0) + s - 1) // s


class LongPlan(collections.namedtuple("LongPlan", "window_frames n_frames overlap window windows")):
    """A sliding-window rollout (made by `long_plan`, which validates the geometry and counts the windows once): `windows` runs of the
    plan `window` (a SamplePlan or a ResamplePlan from all-[MASK]) with a "slide"
    between two of them.  Window w covers long frames [w s, w s + F), s = F - k; from window 1 on the first k frames are known -- the
    last k of the window before.  Long frame f takes its tokens from the first window that sampled it (`owned`).  t0, dt, post_skip,
    q_sample and jump read like the window plan's: every window is the same chain, so the lanes' step / jump graphs serve all of them."""
    __slots__ = ()
    q_sample = False

    @property
    def stride(self):
        return self.window_frames - self.overlap

    @property
    def program(self):
        return self.window.program + (("slide",) + self.window.program) * (self.windows - 1)

    @property
    def draws(self):
        """The sum of the windows' draws: a slide spends no noise stream."""
        return self.windows * self.window.draws

    @property
    def n_steps(self):
        return self.windows * self.window.n_steps

    t0 = property(lambda self: self.window.t0)
    dt = property(lambda self: self.window.dt)
    post_skip = property(lambda self: self.window.post_skip)
    jump = property(lambda self: self.window.jump)

    def owned(self, w):
        """-> range of the long frames window w contributes: [0, F) for window 0, [w s + k, min(w s + F, n)) for w >= 1."""
        if not 0 <= w < self.windows:
            raise GsddError(f"window {w} of a rollout with {self.windows}")
        lo = 0 if w == 0 else w * self.stride + self.overlap
        return range(lo, min(w * self.stride + self.window_frames, self.n_frames))

    def frame_map(self):
        """-> [(window, frame within the window)] for every long frame."""
        out = [None] * self.n_frames
        for w in range(self.windows):
            for f in self.owned(w):
                out[f] = (w, f - w * self.stride)
        return out


def long_plan(window_frames, n_frames, overlap, window_plan):
    """The rollout sample_long() runs, host-side and pure: `window_plan` is what sample() / sample_fast() would run for one window
    (sample_plan(T), sample_plan(T, skip_step) or resample_plan(T, jump, times)).  A purity-prior plan is refused -- its reveal schedule
    counts [MASK] positions, as check_known says -- and so is a partially noised start (filter_ratio > 0), which re-noises the known
    frames."""
    windows = window_count(window_frames, n_frames, overlap)
    if isinstance(window_plan, PurityPlan):
        raise GsddError("long_plan: no rollout for the purity prior (prior_rule 1 / 2): the overlap frames are known tokens and the "
                        "purity prior's reveal schedule counts [MASK] positions")
    if not isinstance(window_plan, (SamplePlan, ResamplePlan)):
        raise GsddError(f"long_plan: window_plan must be a SamplePlan or a ResamplePlan, got {type(window_plan).__name__}")
    if window_plan.q_sample:
        raise GsddError("long_plan: filter_ratio > 0 (a partially noised start) is refused: a window samples from all-[MASK] only")
    return LongPlan(int(window_frames), int(n_frames), int(overlap), window_plan, windows)


def issue_schedule(program, lanes, graphed):
    """-> [(lane, kind, action)] in host issue order for a plan's `program` (its op kinds in order of execution), pure.  Op-major,
    lane-minor, so that the lanes' queues are fed alternately.  Not graphed: every op is "eager".  Graphed: a lane runs the first op
    of a kind "eager" (arguments are validated outside capture) and, if the kind occurs again, records it right after ("capture":
    recorded, not executed); every later op of the kind is a "replay" of that graph."""
    left, seen, out = collections.Counter(program), set(), []
    for kind in program:
        left[kind] -= 1
        for ln in range(lanes):
            if graphed and kind in seen:
                out.append((ln, kind, "replay"))
                continue
            out.append((ln, kind, "eager"))
            if graphed and left[kind]:
                out.append((ln, kind, "capture"))
        seen.add(kind)
    return out


def reference_n_sample(T, prior_ps=1024):
    """The reveal schedules DiffusionTransformer.update_n_sample carries (diffusion_transformer.py:166-179), written for 1024 tokens;
    None for a T it has no list for."""
    if T == 100:
        return [1, 6] + [11, 10, 10] * 32 + [11, 15] if prior_ps <= 10 else [1, 10] + [11, 10, 10] * 32 + [11, 11]
    if T == 50:
        return [10] + [21, 20] * 24 + [30]
    if T == 25:
        return [21] + [41] * 23 + [60]
    if T == 10:
        return [69] + [102] * 8 + [139]
    if T == 200:
        return [1, 3] + [6, 6, 4, 4] * 49 + [6, 9]
    return None


def purity_plan(n_sample, prior_ps, T):
    """-> [(t, n)]: the p_sample calls of the reference's loop (diffusion_transformer.py:621-626 with :336-340) for a reveal schedule,
    host-side and pure.  At t >= 1 a call reveals n = min(n_sample[t] - sampled, prior_ps) positions, a single left-over one folded
    into it, until n_sample[t] are revealed; a timestep with n_sample[t] == 0 makes no call (and runs no denoiser pass).  `sampled`
    grows by exactly n per call: a candidate token is never [MASK] (its row is -70, out of a 24-bit uniform's Gumbel reach).  The
    last entry is (0, n_sample[0]) when n_sample[0] > 0: the ordinary reverse step at t = 0, which resamples every position."""
    calls = []
    for t in range(T - 1, 0, -1):
        sampled = 0
        while sampled < n_sample[t]:
            n = min(n_sample[t] - sampled, prior_ps)
            if n_sample[t] - sampled - n == 1:
                n = n_sample[t] - sampled
            calls.append((t, n))
            sampled += n
    if n_sample[0] > 0:
        calls.append((0, n_sample[0]))
    return calls


def scaled_n_sample(n_sample, L, L_ref=1024):
    """A reveal schedule written for L_ref tokens, rescaled to L by cumulative rounding over t = T-1 ... 1 (the order the chain runs
    in): same length, entry 0 kept, sum over t >= 1 equal to round(sum * L / L_ref), the identity at L == L_ref."""
    out = list(n_sample)
    acc = done = 0
    for t in range(len(n_sample) - 1, 0, -1):
        acc += n_sample[t]
        upto = (2 * acc * L + L_ref) // (2 * L_ref)          # round half up, in integers
        out[t] = upto - done
        done = upto
    return out


def check_truncation_rate(rate, name="truncation_rate"):
    """-> None (no truncation) or the rate as a float.  Top-r truncated sampling (VQ-Diffusion's predict_start_with_truncation,
    "top0.86r") keeps, per position, the classes whose probability mass strictly above them is below r and drops the rest to -70 before
    the posterior / the purity draw.  r must be a real number with 0 < r < 1 as the kernel's fp32 sees it."""
    if rate is None:
        return None
    ok = not isinstance(rate, bool) and isinstance(rate, numbers.Real) and 0 < rate < 1
    if ok:
        ok = 0 < ctypes.c_float(float(rate)).value < 1
    if not ok:
        raise GsddError(f"{name} must be None or a real number in (0, 1), got {rate!r}; 1 is rejected because whether the last class "
                        f"survives would then depend on rounding -- use None to sample without truncation")
    return float(rate)


def check_cond_drop_prob(p, name="cond_drop_prob"):
    """-> the probability as a float; None is 0 (no condition dropout).  Anything but a real number in [0, 1] raises."""
    if p is None:
        return 0.0
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:
        raise GsddError(f"{name} must be null or a real number in [0, 1], got {p!r}")
    return float(p)


def cond_drop_rows(seed, stream, B, row0, p):
    """The drop flags gsdd_cond_dropout draws for global sample rows row0 .. row0 + B - 1 (numpy restatement): row r is dropped iff
    u < float32(p), u = (w >> 8) * 2^-24, w = word 0 of Philox4x32-10 with key `seed` and counter (r [64 bit], stream, 1).  `stream` is
    the stream id of the step's q_sample draw; every other draw has 0 in counter word 3.  -> bool (B,)"""
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    c0, c1 = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    c2, c3 = np.full(B, int(stream) & 0xFFFFFFFF, dtype=np.uint64), np.ones(B, dtype=np.uint64)
    c0, c1 = c0.astype(np.uint64), c1.astype(np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF))
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    u = (c0.astype(np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(p)


def _trunc_kwargs(rate):
    """The keyword a truncated launch adds to ops.d3pm_step / ops.d3pm_purity_step; nothing at all without truncation."""
    return {} if rate is None else {"trunc_rate": float(rate)}


KNOWN_MODES = {"renoise": 0, "hold": 1}      # gsdd_step_desc.known_mode


def frame_mask(latent_shape, frames):
    """-> (L,) bool, true at the positions of the latent frames listed.  latent_shape is (t, h, w), flattened t-major as
    quant.view(B, -1) flattens the encoder's codes; frames is an int k (the first k frames: clip continuation) or an iterable of frame
    indices (first + last frame: interpolation).  Negative indices count from the end."""
    shape = tuple(latent_shape)
    if len(shape) != 3 or not all(_is_int(v) and v >= 1 for v in shape):
        raise GsddError(f"frame_mask: latent_shape must be three positive ints (t, h, w), got {latent_shape!r}")
    nt = int(shape[0])
    if _is_int(frames):
        if not 0 <= frames <= nt:
            raise GsddError(f"frame_mask: the first {frames} frames of a latent with {nt}")
        idx = list(range(int(frames)))
    else:
        try:
            idx = list(frames)
        except TypeError:
            raise GsddError(f"frame_mask: frames must be an int or an iterable of frame indices, got {frames!r}") from None
        if not all(_is_int(i) and -nt <= i < nt for i in idx):
            raise GsddError(f"frame_mask: frame indices {idx!r} outside a latent with {nt} frames")
    m = torch.zeros(shape, dtype=torch.bool)
    m[[int(i) for i in idx]] = True
    return m.reshape(-1)


def check_known(known_mask, content_token, known_mode, *, B, L, K, start_step=0, prior_rule=0):
    """Validates the arguments of known-token conditioned sampling.  -> None (no mask: the plain call) or (mask (B, L) bool,
    tokens (B, L) int64, gsdd_step_desc.known_mode), on the devices the arguments came on.  known_mask is (B, L) or (L,) (the same
    positions in every clip, what frame_mask returns); the tokens at its positions are content_token's and must be codes in [0, K)
    -- [MASK] is no clean token.  One host check per call, as content_token is checked for filter_ratio > 0."""
    if known_mask is None:
        return None
    if not isinstance(known_mode, str) or known_mode not in KNOWN_MODES:
        raise GsddError(f"known_mode must be one of {sorted(KNOWN_MODES)}, got {known_mode!r}")
    if content_token is None:
        raise GsddError("known_mask needs content_token (the tokens at the known positions)")
    if start_step != 0:
        raise GsddError(f"known_mask samples from all-[MASK] only: int(num_timesteps * filter_ratio) = {start_step}, must be 0 "
                        "(a partially noised start re-noises every position, the known ones included)")
    if prior_rule != 0:
        raise GsddError("known_mask cannot be combined with prior_rule > 0: the purity prior's reveal schedule counts [MASK] positions")
    mask, tok = torch.as_tensor(known_mask), torch.as_tensor(content_token)
    if mask.dtype != torch.bool:
        raise GsddError(f"known_mask must be a bool tensor, got {mask.dtype}")
    if mask.dim() == 1 and mask.shape[0] == L:
        mask = mask.unsqueeze(0).expand(B, L)
    if tuple(mask.shape) != (B, L):
        raise GsddError(f"known_mask must have shape {(B, L)} or {(L,)}, got {tuple(mask.shape)}")
    if tok.numel() != B * L or tok.is_floating_point() or tok.dtype == torch.bool:
        raise GsddError(f"content_token must hold {B} x {L} integer tokens, got {tuple(tok.shape)} {tok.dtype}")
    tok = tok.long().reshape(B, L)
    mask = mask.to(tok.device)
    at = tok[mask]
    if at.numel() and (int(at.min()) < 0 or int(at.max()) >= K):
        raise GsddError(f"content_token at known positions must lie in [0, {K}): found {int(at.min())} .. {int(at.max())} "
                        f"([MASK] = {K} is not a clean token)")
    return mask.contiguous(), tok.contiguous(), KNOWN_MODES[known_mode]


def check_condition_len(condition_len, B, Te, what="condition_len"):
    """Validates per-sample condition lengths: (B,) integers in [1, Te] -- sample b is conditioned on its first condition_len[b] tokens
    (a tokenizer's eot + 1); the condition rows behind them are caption padding the cross-attention never reads.  -> a contiguous int32
    CPU tensor (one host read per call if the lengths came on a device; a list or a numpy array will do)."""
    n = torch.as_tensor(condition_len)
    if n.is_floating_point() or n.is_complex() or n.dtype == torch.bool:
        raise GsddError(f"{what} must hold integers, got {n.dtype}")
    if tuple(n.shape) != (B,):
        raise GsddError(f"{what} must have shape ({B},), one length per sample, got {tuple(n.shape)}")
    n = n.detach().cpu().to(torch.int64)
    bad = ((n < 1) | (n > Te)).nonzero()
    if bad.numel():
        b = int(bad[0])
        raise GsddError(f"{what}[{b}] = {int(n[b])} is outside [1, {Te}] (Te condition tokens)")
    return n.to(torch.int32).contiguous()


def _guidance_lens(condition_len, cf_condition_len, B, Te, guided):
    """The lengths of a sampling call's conditional and unconditional copies -> None (no lengths: the plain call) or
    (len, cf_len or None), int32 CPU (B,).  cf_condition_len defaults to Te: the null embedding is full length."""
    if condition_len is None and (cf_condition_len is None or not guided):
        return None
    full = torch.full((B,), Te, dtype=torch.int32)
    len_c = full if condition_len is None else check_condition_len(condition_len, B, Te)
    if not guided:
        return (len_c, None) if Te > 1 else None
    len_u = full if cf_condition_len is None else check_condition_len(cf_condition_len, B, Te, "cf_condition_len")
    return (len_c, len_u) if Te > 1 else None          # (one token, checked to be all ones: nothing to mask)


def _len_kwargs(condition_len, cf_condition_len):
    """sample()'s length keywords as `_sample_once` takes them; nothing at all without lengths."""
    if condition_len is None and cf_condition_len is None:
        return {}
    return {"condition_len": condition_len, "cf_condition_len": cf_condition_len}


COMPOSE_MAX_COND = ops.abi.COMPOSE_MAX_COND     # conditions of a composed call, the call's own condition_embed included

Compose = collections.namedtuple("Compose", "embeds weights lens")
Compose.__doc__ = """A composed call's extra conditions (`check_compose`): embeds, the 1 ... 3 tensors shaped like condition_embed;
weights, f32 CPU (B, N) over all N = 1 + len(embeds) conditions, the call's own first; lens, None or one (B,) int32 CPU length vector
per extra condition."""


def check_compose(compose_embeds, compose_weights, compose_lens, condition_embed, B):
    """Validates sample()'s compose_embeds / compose_weights / compose_lens.  -> None (the plain call) or a `Compose`.
    The step of a composed call reads e = x_u + sum_i w_i (x_i - x_u) over the N conditions (gsdd_d3pm_compose, include/gsdd.h):
    the weights are the scales and guidance_scale plays no part."""
    if compose_embeds is None:
        if compose_weights is not None or compose_lens is not None:
            raise GsddError("compose_weights / compose_lens need compose_embeds (the extra conditions they belong to)")
        return None
    embeds = list(compose_embeds) if isinstance(compose_embeds, (list, tuple)) else None
    if not embeds or not all(torch.is_tensor(e) for e in embeds):
        raise GsddError(f"compose_embeds must be a list of 1 ... {COMPOSE_MAX_COND - 1} tensors shaped like condition_embed")
    N = 1 + len(embeds)
    if N > COMPOSE_MAX_COND:
        raise GsddError(f"a composed call takes at most {COMPOSE_MAX_COND} conditions, condition_embed included: got {N}")
    if condition_embed.dim() != 3:
        raise GsddError(f"a composed call needs condition_embed (B, Te, cond_dim), got {tuple(condition_embed.shape)}")
    for i, e in enumerate(embeds):
        if e.shape != condition_embed.shape or e.device != condition_embed.device:
            raise GsddError(f"compose_embeds[{i}] is {tuple(e.shape)} on {e.device}: must be {tuple(condition_embed.shape)} on "
                            f"{condition_embed.device}, like condition_embed")
    if compose_weights is None:
        raise GsddError(f"compose_embeds needs compose_weights: ({N},) or ({B}, {N}) weights, condition_embed's first")
    w = torch.as_tensor(compose_weights)
    if w.is_complex() or w.dtype == torch.bool or tuple(w.shape) not in ((N,), (B, N)):
        raise GsddError(f"compose_weights must be ({N},) or ({B}, {N}) numbers, got {w.dtype} {tuple(w.shape)}")
    w = w.detach().cpu().to(torch.float32)
    if not bool(torch.isfinite(w).all()):
        raise GsddError("compose_weights must be finite")
    w = (w.unsqueeze(0).expand(B, N) if w.dim() == 1 else w).contiguous()
    lens = None
    if compose_lens is not None:
        lens = list(compose_lens) if isinstance(compose_lens, (list, tuple)) else None
        if lens is None or len(lens) != len(embeds):
            raise GsddError(f"compose_lens must list one ({B},) length vector per extra condition ({len(embeds)})")
        lens = [check_condition_len(n, B, condition_embed.shape[1], f"compose_lens[{i}]") for i, n in enumerate(lens)]
    return Compose(tuple(embeds), w, lens)


def check_compose_entries(entries, what="compose"):
    """Validates the glue's list of extra captions: None, or at most COMPOSE_MAX_COND - 1 mappings {text: str, weight: finite number}
    (nothing else in them).  -> None or a tuple of (text, weight)."""
    if entries is None:
        return None
    if isinstance(entries, (str, bytes)) or not isinstance(entries, collections.abc.Sequence) or not 1 <= len(entries) <= COMPOSE_MAX_COND - 1:
        raise GsddError(f"{what} must be null or a list of 1 ... {COMPOSE_MAX_COND - 1} {{text, weight}} entries, got {entries!r}")
    out = []
    for i, e in enumerate(entries):
        if not isinstance(e, collections.abc.Mapping) or set(e.keys()) != {"text", "weight"}:
            raise GsddError(f"{what}[{i}] must be a mapping with exactly the keys text and weight, got {e!r}")
        text, w = e["text"], e["weight"]
        if not isinstance(text, str):
            raise GsddError(f"{what}[{i}].text must be a string, got {text!r}")
        if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(w):
            raise GsddError(f"{what}[{i}].weight must be a finite number, got {w!r}")
        out.append((text, float(w)))
    return tuple(out)


def _compose_kwargs(compose):
    """check_compose's result as `_sample_once` takes it; nothing at all for a plain call."""
    return {} if compose is None else {"compose": compose}


def _known_kwargs(known, dev, sl=slice(None)):
    """check_known's result -> the known / x_known / known_mode keywords of ops.d3pm_step for the clips `sl` of the batch, on `dev`;
    nothing at all without a mask."""
    if known is None:
        return {}
    mask, tok, mode = known
    return {"known": mask[sl].to(dev).to(torch.uint8).contiguous(), "x_known": tok[sl].to(dev).contiguous(), "known_mode": mode}


SCHED_ORDER = ("log_at", "log_bt", "log_ct", "log_1_min_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct",
               "log_1_min_cumprod_ct")


class _Lane:
    """One sub-batch of a sampling call (clips `sl` of the batch) and the ops of its chain.  Independent sub-batches run their reverse
    chains concurrently on separate HIP streams: every clip's chain depends only on its own tokens, condition and noise rows (the noise
    key is the global row index), so the tokens are those of the single-lane run, and workgroups of one lane fill the tail of the
    other lane's kernels.  Holds the stream st, tokens tok, condition vectors condv (Te condition tokens, `rep` stacked guidance
    copies), timesteps t2, workspace ws, noise-stream counter sid, M = Bs L positions from global row row0, the known-position
    keywords, the graph of every op kind captured so far and what only some programs need: the jump's table and held positions, the
    reveal's plan arrays, counters and candidate buffers.  Built on `st`, after st waits for the caller's stream."""

    def __init__(self, dm, plan, st, sl, conds, rep, x0, known, trunc_kw, cond_len=None, long_tok=None, compose_w=None):
        dev, L, K, Bs, tr = dm.device, dm.shape, dm.num_classes - 1, sl.stop - sl.start, dm.transformer
        self.tr, self.plan, self.st, self.rep, self.guided, self.graphs = tr, plan, st, rep, dm._guided, {}
        # a composed lane (rep = N + 1 copies: the N conditions, then the null condition): its clips' (Bs, N) weights, a device buffer
        # every captured op reads
        self.compose_w, self.Bs, self.L = None if compose_w is None else compose_w.to(dev).contiguous(), Bs, L
        self.trunc_kw = trunc_kw                    # a launch constant of both step kernels: a captured graph records it
        self.sched, self.K, self.T = dm._sched(), K, dm.num_timesteps
        self.guidance, self.seed = float(dm.guidance_scale), dm.noise_seed
        self.Te, self.M, self.row0 = conds.shape[1], Bs * L, (dm.row_offset + sl.start) * L
        self.condv = tr.cond_vectors(conds.contiguous())
        # condition lengths of the lane's rep * Bs rows ([len | cf_len]), or None: lane set-up, a device buffer every captured op reads
        self.cond_len = None if cond_len is None else cond_len.to(dev).contiguous()
        self.ws = tr.workspace(rep * Bs, L, dev, rep=rep)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.t2 = torch.full((rep * Bs,), plan.t0, dtype=torch.int64, device=dev)
        self.sid = i64([dm.noise_stream + (1 if plan.q_sample else 0)])      # the partially noised start spends one draw on q_sample
        if x0 is None:
            self.tok = torch.full((Bs, L), K, dtype=torch.int64, device=dev)          # all [MASK] (:613-618)
        else:                                                                        # q_sample at t = start_step - 1 (:628-630)
            self.tok = torch.empty((Bs, L), dtype=torch.int64, device=dev)
            ops.d3pm_q_sample(x0[sl].contiguous(), self.tok, self.sched, self.t2[:Bs].contiguous(), i64([dm.noise_stream]), K=K,
                              T=self.T, seed=self.seed, row0=self.row0, stream=st)
        # known positions (check_known): this lane's slices of mask and tokens, made once, here, outside graph capture -- they are
        # constants of the chain; nothing at all without a mask
        if long_tok is None:
            self.known_kw = _known_kwargs(known, dev, sl)
        else:
            # a rollout (LongPlan): every window runs the step with known positions on buffers of the lane's own, which the slide
            # rewrites between two windows -- so the graphs of the first windows serve all later ones.  `known` is (mask or None,
            # tokens or None, mode): window 0 carries the caller's mask, or none at all (all zero: the plain step, bit for bit)
            mask, xk, mode = known
            self.known_kw = {"known": torch.zeros((Bs, L), dtype=torch.uint8, device=dev),
                             "x_known": torch.zeros((Bs, L), dtype=torch.int64, device=dev), "known_mode": mode}
            if mask is not None:
                self.known_kw["known"].copy_(mask[sl])
                self.known_kw["x_known"].copy_(xk[sl])
            self.long_rows = long_tok[sl]           # this lane's rows of the (B, n h w) long buffer
            self.win_state = i64([0, 0])            # the finished window's index, the slide kernel's arrival counter
            self.bad = torch.zeros((1,), dtype=torch.int32, device=dev)      # tokens outside [0, K) that a slide made known
        if "jump" in plan.program:              # the jump's table and, in hold mode, the positions it copies through
            self.jump_table = dm._jump_table(plan.jump, dev)
            self.jump_hold = self.known_kw["known"] if self.known_kw["known_mode"] == KNOWN_MODES["hold"] else None
        if "reveal" in plan.program:
            # (t, n) of every call plus a (0, 0) sentinel: after the last reveal the counter leaves t = 0 for the final step
            self.plan_t, self.plan_n = i64([t for t, _ in plan.calls] + [0]), i64([n for _, n in plan.calls] + [0])
            self.step_dev, self.n_dev = i64([0]), i64([plan.calls[0][1]])
            self.score = torch.empty((Bs, L), dtype=torch.float32, device=dev)
            self.smax = torch.empty((Bs,), dtype=torch.float32, device=dev)
            self.cand = torch.empty((Bs, L), dtype=torch.int64, device=dev)

    def denoise(self):                          # -> the conditional and the unconditional logits of the lane's tokens at t2
        logits = self.tr.run(self.tok, self.condv, self.Te, self.t2, self.ws, rep=self.rep, stream=self.st, cond_len=self.cond_len)
        if self.compose_w is not None:          # the composed row, into block 0 of the logits: the step reads it alone
            return ops.d3pm_compose(logits, self.compose_w, n_cond=self.rep - 1, B=self.Bs, L=self.L, K=self.K, stream=self.st), None
        return logits[:self.M], (logits[self.M:] if self.rep == 2 else logits[:self.M]) if self.guided else None

    def plain_step(self, post_skip):
        ops.d3pm_step(*self.denoise(), self.tok, self.tok, self.sched, self.t2, self.sid, K=self.K, T=self.T, guidance=self.guidance,
                      seed=self.seed, row0=self.row0, post_skip=post_skip, stream=self.st, **self.trunc_kw, **self.known_kw)

    def step(self):                             # the reverse step at t2, then t2 and sid move on
        self.plain_step(self.plan.post_skip)
        if self.plan.dt == 1:
            ops.advance(self.t2, -1, self.sid, 1, stream=self.st)
        else:                                   # skip-step chain: t moves by -(1 + s) and stops at 0 (the appended last step)
            ops.advance_floor(self.t2, -self.plan.dt, 0, self.sid, 1, stream=self.st)

    def jump(self):                             # the state at level t2 moves forward to t2 + jump; one noise stream, like a step
        ops.d3pm_forward_jump(self.tok, self.tok, self.jump_table, self.t2, self.sid, K=self.K, T=self.T, jump=self.plan.jump,
                              seed=self.seed, row0=self.row0, hold=self.jump_hold, stream=self.st)
        ops.advance(self.t2, self.plan.jump, self.sid, 1, stream=self.st)

    def reveal(self):                           # a purity call: candidates, the n_dev most trusted [MASK] positions, the next (t, n)
        plan = self.plan
        ops.d3pm_purity_step(*self.denoise(), self.score, self.smax, self.cand, self.sid, K=self.K, guidance=self.guidance,
                             prior_rule=plan.rule, prior_weight=plan.weight, seed=self.seed, row0=self.row0, stream=self.st,
                             **self.trunc_kw)
        ops.d3pm_purity_select(self.tok, self.tok, self.cand, self.score, self.smax, self.n_dev, self.sid, K=self.K,
                               prior_rule=plan.rule, seed=self.seed, stream_add=1, row0=self.row0, stream=self.st)
        ops.advance_plan(self.step_dev, self.plan_t, self.plan_n, self.t2, self.n_dev, self.sid, 2, stream=self.st)

    def final(self):                            # the purity chain's ordinary reverse step at t = 0
        self.plain_step(0)

    def slide(self, final=False):               # between two windows: frames out, the overlap in as known tokens, [MASK], t2 = t0
        p, kw = self.plan, self.known_kw
        ops.d3pm_window_slide(self.tok, self.long_rows, kw["x_known"], kw["known"], self.t2, self.win_state, self.bad,
                              F=p.window_frames, k=p.overlap, n=p.n_frames, K=self.K, t0=p.t0, final=final, stream=self.st)

    OPS = {"step": step, "jump": jump, "reveal": reveal, "final": final, "slide": slide}

    def issue(self, kind, action, trace=None):
        """One entry of `issue_schedule`; an eager op of a traced call appends the lane's tokens to `trace`."""
        if action == "replay":
            self.graphs[kind].launch(self.st)
            return
        with torch.cuda.stream(self.st):
            if action == "capture":
                g = self.graphs[kind] = ops.Graph()
                g.begin(self.st)
                try:
                    self.OPS[kind](self)        # recorded, not executed; the graph keeps every tensor the op hands to the C ABI
                finally:
                    g.end(self.st)
            else:
                self.OPS[kind](self)
                if trace is not None:
                    trace.append(self.tok.clone())


class DiffusionTransformer(nn.Module):
    """Drop-in for diffusion_transformer.py:71-645 (sample, forward/_train_loss surface)."""

    def __init__(self, *, condition_emb_config=None, transformer=None, diffusion_step=100, alpha_init_type="cos",
                 auxiliary_loss_weight=0, adaptive_auxiliary_loss=False, mask_weight=[1, 1], learnable_cf=False,
                 guidance_scale=5, content_seq_len=1024):
        super().__init__()
        if alpha_init_type != "alpha1":
            raise ValueError("alpha_init_type must be 'alpha1' (the reference crashes on anything else, "
                             "diffusion_transformer.py:115-118)")
        self.condition_emb = None
        self.transformer = transformer
        self.content_seq_len = content_seq_len
        self.num_classes = self.transformer.content_emb.num_embed
        self.shape = content_seq_len
        self.num_timesteps = diffusion_step
        self.auxiliary_loss_weight = auxiliary_loss_weight
        self.adaptive_auxiliary_loss = adaptive_auxiliary_loss
        self.mask_weight = mask_weight
        at, bt, ct, att, btt, ctt = (torch.tensor(a.astype("float64"))
                                     for a in alpha_schedule(self.num_timesteps, N=self.num_classes - 1))
        l1m = lambda a: torch.log(1 - a.exp() + 1e-40)
        log_ct, log_cct = torch.log(ct), torch.log(ctt)
        self.register_buffer("log_at", torch.log(at).float())
        self.register_buffer("log_bt", torch.log(bt).float())
        self.register_buffer("log_ct", log_ct.float())
        self.register_buffer("log_cumprod_at", torch.log(att).float())
        self.register_buffer("log_cumprod_bt", torch.log(btt).float())
        self.register_buffer("log_cumprod_ct", log_cct.float())
        self.register_buffer("log_1_min_ct", l1m(log_ct).float())
        self.register_buffer("log_1_min_cumprod_ct", l1m(log_cct).float())
        self.register_buffer("Lt_history", torch.zeros(self.num_timesteps))
        self.register_buffer("Lt_count", torch.zeros(self.num_timesteps))
        self.empty_text_embed = nn.Parameter(torch.randn(size=(77, 512), dtype=torch.float64))
        self.prior_rule = 0          # 0: plain sampling; 1: high-quality inference only; 2: purity prior (diffusion_transformer.py:157-161)
        self.prior_ps = 1024         # most positions one call reveals
        self.prior_weight = 0        # r of Eq. 11, Improved VQ-Diffusion
        self.n_sample = None         # reveals per timestep (update_n_sample; None: the reference has no list for this T)
        self.update_n_sample()
        self.truncation_rate = None  # None: no truncation; 0 < r < 1: top-r truncated sampling (upstream's "top0.86r" is 0.86)
        self.learnable_cf = learnable_cf
        self.cond_drop_prob = 0.0    # training: probability that a sample's condition is replaced by the null condition (classifier-free
                                     # training; the null condition is empty_text_embed[:Te] with learnable_cf, else the caller's)
        self.guidance_scale = guidance_scale
        self.noise_seed = 0          # Philox key; the stream id advances with every draw
        self.noise_stream = 0
        self.row_offset = 0          # global row of this rank's first sample (multi-GPU batch sharding)
        self.sample_lanes = None     # concurrent sub-batches of sample() (see there): None = two when the batch allows it;
                                     # `bench.py --lanes N` / GSDD_SAMPLE_LANES override it

    @property
    def device(self):
        return self.transformer.to_logits[-1].weight.device

    @property
    def _guided(self):
        """Whether a reverse step mixes conditional and unconditional logits (guidance_scale != 1)."""
        return abs(self.guidance_scale - 1) >= 1e-3

    def set_noise(self, seed, stream=0, row_offset=0):
        self.noise_seed, self.noise_stream, self.row_offset = int(seed), int(stream), int(row_offset)

    def _sched(self):
        return [getattr(self, n) for n in SCHED_ORDER]

    def check_learned_null(self, Te, cond_dim):
        rows, width = self.empty_text_embed.shape
        if Te > rows or cond_dim != width:
            raise GsddError(f"learnable_cf: the learned null embedding is ({rows}, {width}); the condition has Te = {Te} tokens of "
                            f"width {cond_dim} (needs Te <= {rows} and cond_dim == {width})")

    def null_condition(self, Te, cond_dim, null_cond=None):
        """-> the (Te, cond_dim) f32 null condition of classifier-free training and guidance: with learnable_cf rows [:Te] of
        empty_text_embed rounded to f32 (Improved VQ-Diffusion's learned null embedding; diffusion_transformer.py:541-543), else the
        caller's `null_cond`, (Te, cond_dim) or (1, Te, cond_dim)."""
        if self.learnable_cf:
            self.check_learned_null(Te, cond_dim)
            return self.empty_text_embed.detach()[:Te].float().contiguous()
        if Te > 77:
            raise GsddError(f"the null condition holds up to 77 condition tokens, got Te = {Te}")
        if null_cond is None:
            raise GsddError("condition dropout without learnable_cf needs a null condition (null_cond / "
                            "input['null_condition_embed_token']): the (Te, cond_dim) embedding that stands for 'no caption'")
        n = null_cond[0] if (null_cond.dim() == 3 and null_cond.shape[0] == 1) else null_cond
        if tuple(n.shape) != (Te, cond_dim):
            raise GsddError(f"the null condition must be (Te, cond_dim) = {(Te, cond_dim)} or (1, Te, cond_dim), got {tuple(null_cond.shape)}")
        return n.detach().float().contiguous()

    def _cf_embed(self, condition_embed, cf_condition_embed, composed=False):
        """The unconditional condition of a guided or composed sampling call: the caller's, else (learnable_cf) the learned null rows
        repeated over the batch."""
        if cf_condition_embed is not None or not (self._guided or composed):
            return cf_condition_embed
        if not self.learnable_cf:
            raise GsddError("a composed call (compose_embeds) needs the unconditional condition: cf_condition_embed, or a model with "
                            "learnable_cf" if composed else "guided sampling (guidance_scale != 1) needs cf_condition_embed")
        cond = condition_embed if condition_embed.dim() == 3 else condition_embed.unsqueeze(1)
        B, Te, cd = cond.shape
        return self.null_condition(Te, cd).to(cond.device).unsqueeze(0).expand(B, Te, cd).contiguous()

    def _jump_table(self, jump, dev):
        """The device copy of jump_table(T, K, jump), made once per jump (and device)."""
        cache = self.__dict__.setdefault("_jump_tables", {})
        key = (int(jump), str(dev))
        if key not in cache:
            cache[key] = jump_table(self.num_timesteps, self.num_classes - 1, int(jump)).to(dev).contiguous()
        return cache[key]

    def update_n_sample(self):
        """diffusion_transformer.py:166-179: the reference's list for this num_timesteps / prior_ps (unchanged for any other T)."""
        ns = reference_n_sample(self.num_timesteps, self.prior_ps)
        if ns is not None:
            self.n_sample = ns

    def _purity_plan(self, start_step):
        """Validates the prior attributes and returns the PurityPlan sample() runs (prior_rule 1 / 2)."""
        T, L = self.num_timesteps, self.shape
        if start_step != 0:
            raise GsddError("prior_rule > 0 samples from all-[MASK] only: filter_ratio must give start_step 0 (the reference's "
                            "filter_ratio > 0 loop raises with any prior_rule, diffusion_transformer.py:636)")
        if not _is_int(self.prior_ps) or self.prior_ps < 1:
            raise GsddError(f"prior_ps must be an int >= 1, got {self.prior_ps!r}")
        if isinstance(self.prior_weight, bool) or not isinstance(self.prior_weight, numbers.Real) or not self.prior_weight >= 0:
            raise GsddError(f"prior_weight must be a number >= 0, got {self.prior_weight!r}")
        ns = self.n_sample
        if ns is None or len(ns) != T:
            raise GsddError(f"n_sample must list one reveal count per timestep: len(n_sample) = {None if ns is None else len(ns)}, "
                            f"num_timesteps = {T}")
        if not all(_is_int(v) for v in ns):
            raise GsddError("n_sample entries must be ints")
        if min(ns) < 0:
            raise GsddError(f"negative entry in n_sample: {min(ns)}")
        if ns[0] > 1024:
            raise GsddError(f"n_sample[0] = {ns[0]} > 1024: the reference's loop never ends there (diffusion_transformer.py:350, :625)")
        if sum(ns[1:]) > L:
            raise GsddError(f"n_sample reveals {sum(ns[1:])} positions over t >= 1 but the sequence has {L}: over-subscribed schedule "
                            "(the reference then overwrites decoded tokens); rescale it with scaled_n_sample")
        if L > 4096:
            raise GsddError(f"prior_rule > 0 needs content_seq_len <= 4096 (the selection kernel's limit), got {L}")
        calls = purity_plan([int(v) for v in ns], int(self.prior_ps), T)
        final = bool(calls) and calls[-1][0] == 0
        return PurityPlan(tuple(calls[:-1] if final else calls), final, int(self.prior_rule), float(self.prior_weight))

    @staticmethod
    def _batch_of(condition_token, kwargs):
        return len(condition_token) if condition_token is not None else kwargs["batch_size"]

    # ------------------------------------------------------------------ sampling (diffusion_transformer.py:568-713)
    @torch.no_grad()
    def sample(self, condition_token, condition_mask, condition_embed, cf_condition_embed, content_token=None,
               filter_ratio=0.5, temperature=1.0, return_att_weight=False, return_logits=False, content_logits=None,
               print_log=True, use_graph=True, trace=None, *, known_mask=None, known_mode="renoise", resample_jump=None,
               resample_times=1, condition_len=None, cf_condition_len=None, compose_embeds=None, compose_weights=None,
               compose_lens=None, **kwargs):
        """diffusion_transformer.py:568-644.  The arguments pick a plan (`sample_plan`, `resample_plan`, `_purity_plan`); `_sample_once`
        executes the plan's program -- its op kinds in order -- as `issue_schedule` lays it out over the lanes (a lane runs a kind
        eagerly once, captures it into a hipGraph if it recurs and replays it from then on; use_graph=False or a `trace` list: every
        op eagerly in one lane, one trace entry per op); `_sample_checked` repeats the call on the bf16x3 layer kernel if an
        activation left the f16 operand range.
        filter_ratio > 0: start from content_token noised to t = start_step - 1 and run start_step reverse steps
        (diffusion_transformer.py:590-592, :626-634; the reference's own loop there passes p_sample four of its six positional
        parameters and raises TypeError -- this is the behaviour that branch is written for, one p_sample per step).
        prior_rule 1 / 2 (attributes, as in the reference): the purity-prior chain of `purity_plan` -- every call at t > 0 runs the
        denoiser, draws a candidate per position and reveals the n most trusted [MASK] positions (two noise streams per call);
        the step at t = 0 is the ordinary one.
        known_mask (bool, (B, L) or (L,)): the positions whose clean tokens are given, in content_token (frame prediction,
        interpolation, inpainting; `frame_mask`).  From all-[MASK], prior_rule 0.  Those positions skip the learned reverse step:
        known_mode "renoise" draws them from the forward marginal q(x_{t-1} | x_0) at every step (RePaint's construction for the
        absorbing chain; x_0 itself at t = 0), "hold" writes x_0 at every step.  Every other position is sampled as without the mask
        and sees the known ones through self-attention.  None launches exactly the plain chain.
        resample_jump / resample_times (with known_mask): RePaint's resampling -- `resample_plan`: after every `resample_jump` reverse
        steps the whole state is diffused forward by that many levels (gsdd_d3pm_forward_jump; "hold" copies the known positions
        through, "renoise" moves them like every other position) and denoised again, `resample_times` times over, so that the sampled
        positions see the known content more than once per level.  Every step and every jump spends one noise stream.  None or
        resample_times = 1: the call without them, launch for launch.
        condition_len / cf_condition_len ((B,) integers in [1, Te], `check_condition_len`; more than one condition token): clip b is
        conditioned on the first condition_len[b] rows of condition_embed[b] only -- the rows behind them are caption padding, which
        the cross-attention never reads -- and its unconditional copy on the first cf_condition_len[b] rows of cf_condition_embed[b]
        (default Te: the null embedding is full length).  They work with every plan.  The positional condition_mask stays ignored.
        None: the call without them, launch for launch.
        compose_embeds / compose_weights / compose_lens: composed guidance (`check_compose`) -- compose_embeds lists 1 ... 3 further
        conditions shaped like condition_embed, compose_weights the (N,) or (B, N) weights of all N = 1 + len(compose_embeds)
        conditions, condition_embed's first (any finite number: a negative weight is a negative prompt), compose_lens one (B,) length
        vector per extra condition (default: full length).  Every denoiser pass then runs N + 1 stacked copies and one launch
        (gsdd_d3pm_compose) folds their rows into e = x_u + sum_i w_i (x_i - x_u), which the step reads without a second row.  The
        weights are the scales: guidance_scale plays no part, the unconditional condition is always needed, and the copies are never
        deduplicated.  They work with every plan.  None: the call without them, launch for launch."""
        kwargs = dict(kwargs, **_len_kwargs(condition_len, cf_condition_len))
        compose = check_compose(compose_embeds, compose_weights, compose_lens, condition_embed, self._batch_of(condition_token, kwargs))
        kwargs.update(_compose_kwargs(compose))
        trunc = check_truncation_rate(getattr(self, "truncation_rate", None))
        start_step = int(self.num_timesteps * filter_ratio)
        cf_condition_embed = self._cf_embed(condition_embed, cf_condition_embed, compose is not None)      # (None + learnable_cf: the learned null rows)
        if isinstance(self.prior_rule, bool) or self.prior_rule not in (0, 1, 2):
            raise GsddError(f"prior_rule must be 0, 1 or 2, got {self.prior_rule!r}")
        known = None if known_mask is None else check_known(known_mask, content_token, known_mode, B=self._batch_of(condition_token, kwargs),
                                                            L=self.shape, K=self.num_classes - 1, start_step=start_step,
                                                            prior_rule=self.prior_rule)
        resample = check_resample(resample_jump, resample_times, self.num_timesteps, known_mask)
        if known is not None:
            plan = sample_plan(self.num_timesteps) if resample is None else resample_plan(self.num_timesteps, *resample)
            return self._sample_checked(plan, condition_token, condition_embed, cf_condition_embed,
                                        return_logits=return_logits, use_graph=use_graph, trace=trace, truncation_rate=trunc,
                                        known=known, **kwargs)
        if self.prior_rule != 0:        # purity-prior inference (:304-346): reveal n_sample[t] trusted positions per timestep
            return self._sample_checked(self._purity_plan(start_step), condition_token, condition_embed, cf_condition_embed,
                                        return_logits=return_logits, use_graph=use_graph, trace=trace, truncation_rate=trunc, **kwargs)
        if start_step != 0 and content_token is None:
            raise GsddError("filter_ratio > 0 needs content_token (the tokens to start from)")
        return self._sample_checked(sample_plan(self.num_timesteps, start_step=start_step), condition_token, condition_embed,
                                    cf_condition_embed, content_token=content_token, return_logits=return_logits,
                                    use_graph=use_graph, trace=trace, truncation_rate=trunc, **kwargs)

    @torch.no_grad()
    def sample_fast(self, condition_token, condition_mask, condition_embed, content_token=None, filter_ratio=0.5,
                    temperature=1.0, return_att_weight=False, return_logits=False, content_logits=None, print_log=True,
                    skip_step=1, *, cf_condition_embed=None, use_graph=True, trace=None, known_mask=None, known_mode="renoise",
                    condition_len=None, cf_condition_len=None, compose_embeds=None, compose_weights=None, compose_lens=None, **kwargs):
        """VQ-Diffusion's skip-step sampler (diffusion_transformer.py:648-713): the denoiser runs at t = T-1, T-1-(1+s), ..., then 0
        (`sample_plan`), and each step's posterior jumps to t - s (for t > s) across the skipped levels.  From all-[MASK] only, as the
        reference asserts.  The reference passes cf_predict_start three of its four arguments; the
        unconditional embedding is the keyword cf_condition_embed here.  skip_step = 0 is sample(filter_ratio=0), bit for bit.
        known_mask / known_mode: as in sample(); a known position is re-noised to the level the step's posterior jumps to.
        condition_len / cf_condition_len, compose_embeds / compose_weights / compose_lens: as in sample()."""
        T = self.num_timesteps
        kwargs = dict(kwargs, **_len_kwargs(condition_len, cf_condition_len))
        compose = check_compose(compose_embeds, compose_weights, compose_lens, condition_embed, self._batch_of(condition_token, kwargs))
        kwargs.update(_compose_kwargs(compose))
        if "resample_jump" in kwargs or "resample_times" in kwargs:
            raise GsddError("sample_fast takes no resample_jump / resample_times: the skip-step chain has no resampling jumps (use sample)")
        trunc = check_truncation_rate(getattr(self, "truncation_rate", None))
        known = None if known_mask is None else check_known(known_mask, content_token, known_mode, B=self._batch_of(condition_token, kwargs),
                                                            L=self.shape, K=self.num_classes - 1, start_step=int(T * filter_ratio))
        known_kw = {} if known is None else {"known": known}
        if int(T * filter_ratio) != 0:
            raise GsddError(f"sample_fast starts from all-[MASK] only: int(num_timesteps * filter_ratio) = {int(T * filter_ratio)}, "
                            "must be 0 (diffusion_transformer.py:686)")
        if not _is_int(skip_step) or skip_step < 0:
            raise GsddError(f"skip_step must be a non-negative int, got {skip_step!r}")
        cf_condition_embed = self._cf_embed(condition_embed, cf_condition_embed, compose is not None)      # (None + learnable_cf: the learned null rows)
        if return_logits:
            raise NotImplementedError("return_logits is unused by the reference call sites")
        return self._sample_checked(sample_plan(T, skip_step=int(skip_step)), condition_token, condition_embed, cf_condition_embed,
                                    use_graph=use_graph, trace=trace, truncation_rate=trunc, **known_kw, **kwargs)

    @torch.no_grad()
    def sample_long(self, condition_token, condition_mask, condition_embed, cf_condition_embed, *, latent_shape, n_frames, overlap,
                    content_token=None, known_mask=None, known_mode="renoise", skip_step=None, resample_jump=None, resample_times=1,
                    condition_len=None, cf_condition_len=None, compose_embeds=None, compose_weights=None, compose_lens=None,
                    use_graph=True, trace=None, filter_ratio=0, **kwargs):
        """A clip of n_frames latent frames, longer than the model's window of F = latent_shape[0]: the sliding-window rollout of
        `long_plan` as one program of the executor.  Window 0 is the call sample() -- or, with skip_step, sample_fast() -- would make
        (content_token / known_mask apply to it alone: continuing a real clip); every later window keeps the last `overlap` frames
        of the window before as known tokens (frame_mask(latent_shape, overlap), known_mode, the resampling jumps) and samples the
        rest.  Between two windows one launch per lane (gsdd_d3pm_window_slide) moves the finished frames to the long buffer, makes
        the overlap the next window's known tokens and resets tokens and timesteps, all on the lane's fixed buffers: no host round
        trip, and the step / jump graphs captured in the first windows replay in every later one.  One condition per clip serves all
        windows.  The tokens are those of the manual chain of those calls under the same set_noise, and noise_stream ends where the
        chain leaves it.  A [MASK] in an overlap raises after the call (one read of device counters, with the range flags; after a
        repeat on the bf16x3 kernel they are the repeat's counters).  On that error path alone the call differs from the chain: the
        whole rollout has run and noise_stream has advanced by all its draws, where the chain's check_known would have stopped before
        the next window.
        compose_embeds / compose_weights / compose_lens: as in sample(); the composed conditions serve all windows.
        n_frames == F is sample() / sample_fast() itself.  Not with prior_rule > 0, filter_ratio > 0, or skip_step together with
        resampling jumps.  -> {"content_token": (B, n_frames h w) int64, "windows": W}"""
        T, K = self.num_timesteps, self.num_classes - 1
        shape = tuple(latent_shape)
        if len(shape) != 3 or not all(_is_int(v) and v >= 1 for v in shape) or shape[0] * shape[1] * shape[2] != self.shape:
            raise GsddError(f"latent_shape must be three positive ints (t, h, w) with t h w = content_seq_len = {self.shape}, got {latent_shape!r}")
        if isinstance(self.prior_rule, bool) or self.prior_rule not in (0, 1, 2):
            raise GsddError(f"prior_rule must be 0, 1 or 2, got {self.prior_rule!r}")
        if self.prior_rule != 0:
            raise GsddError("sample_long cannot be combined with prior_rule > 0: the overlap frames are known tokens and the purity "
                            "prior's reveal schedule counts [MASK] positions")
        if int(T * filter_ratio) != 0:
            raise GsddError(f"sample_long samples every window from all-[MASK]: int(num_timesteps * filter_ratio) = {int(T * filter_ratio)}, "
                            "must be 0")
        if skip_step is not None:
            if not _is_int(skip_step) or skip_step < 0:
                raise GsddError(f"skip_step must be None or a non-negative int, got {skip_step!r}")
            if resample_jump is not None or resample_times != 1:
                raise GsddError("skip_step cannot be combined with resample_jump / resample_times: the skip-step chain has no resampling jumps")
        if not isinstance(known_mode, str) or known_mode not in KNOWN_MODES:
            raise GsddError(f"known_mode must be one of {sorted(KNOWN_MODES)}, got {known_mode!r}")
        resample = check_resample(resample_jump, resample_times, T, True)       # (every window from the second on has known frames)
        window = sample_plan(T, skip_step=int(skip_step)) if skip_step is not None else (
            sample_plan(T) if resample is None else resample_plan(T, *resample))
        plan = long_plan(shape[0], n_frames, overlap, window)
        B, L, hw = self._batch_of(condition_token, kwargs), self.shape, shape[1] * shape[2]
        lens = _len_kwargs(condition_len, cf_condition_len)
        if plan.windows == 1:                       # one window: the existing call, launch for launch
            if resample is not None and known_mask is None:      # (window 0 of a resampled rollout: the jumps with nothing known)
                content_token, known_mask = torch.zeros((B, L), dtype=torch.int64), torch.zeros((L,), dtype=torch.bool)
            known_kw = {} if known_mask is None else {"known_mask": known_mask, "known_mode": known_mode}
            # the composed keywords as they came, nothing at all without them: the call below validates them
            compose_kw = {k: v for k, v in (("compose_embeds", compose_embeds), ("compose_weights", compose_weights),
                                            ("compose_lens", compose_lens)) if v is not None}
            if skip_step is not None:
                out = self.sample_fast(condition_token, condition_mask, condition_embed, content_token=content_token, filter_ratio=0,
                                       skip_step=int(skip_step), cf_condition_embed=cf_condition_embed, use_graph=use_graph, trace=trace,
                                       **known_kw, **lens, **compose_kw, **kwargs)
            else:
                if resample is not None:
                    known_kw.update(resample_jump=resample_jump, resample_times=resample_times)
                out = self.sample(condition_token, condition_mask, condition_embed, cf_condition_embed, content_token=content_token,
                                  filter_ratio=0, use_graph=use_graph, trace=trace, **known_kw, **lens, **compose_kw, **kwargs)
            return {"content_token": out["content_token"], "windows": 1}
        compose = check_compose(compose_embeds, compose_weights, compose_lens, condition_embed, B)
        trunc = check_truncation_rate(getattr(self, "truncation_rate", None))
        cf_condition_embed = self._cf_embed(condition_embed, cf_condition_embed, compose is not None)
        known = (None, None, KNOWN_MODES[known_mode])
        if known_mask is not None:
            known = check_known(known_mask, content_token, known_mode, B=B, L=L, K=K)
        # the long buffer: made once, on the caller's stream, before the lanes fork; every lane writes its own rows
        long_tok = torch.full((B, plan.n_frames * hw), K, dtype=torch.int64, device=self.device)
        out = self._sample_checked(plan, condition_token, condition_embed, cf_condition_embed, use_graph=use_graph, trace=trace,
                                   truncation_rate=trunc, known=known, long_tok=long_tok, **lens, **_compose_kwargs(compose), **kwargs)
        bad = sum(int(c.item()) for c in self._bad_counters)      # (the lanes of the run that counted: _sample_checked's last)
        if bad:
            raise GsddError(f"sample_long: {bad} token(s) outside [0, {K}) in the overlap frames of a finished window ([MASK] = {K} is "
                            "no clean token: the window's chain did not resolve every position)")
        return {"content_token": out["content_token"], "windows": plan.windows}

    def _sample_checked(self, plan, *args, trace=None, **kw):
        """`_sample_once`, then one read of the layer kernel's range flags after the loop (outside graph capture): if an activation left
        the f16 operand range the call is repeated on the bf16x3 layer kernel (Text2ImageTransformer.demote_to_x3p) -- same noise
        stream, so the tokens are those of an x3p run."""
        mark = len(trace) if trace is not None else 0
        out = self._sample_once(plan, *args, trace=trace, **kw)
        if any(int(f.item()) != 0 for f in self._range_flags):
            if not self.transformer.demote_to_x3p():
                raise GsddError("non-finite activations in the denoiser (inf / NaN in the inputs or weights?)")
            if trace is not None:
                del trace[mark:]
            self.noise_stream -= self._last_draws
            out = self._sample_once(plan, *args, trace=trace, **kw)
        return out

    def _sample_once(self, plan, condition_token, condition_embed, cf_condition_embed, content_token=None, return_logits=False,
                     use_graph=True, trace=None, truncation_rate=None, known=None, condition_len=None, cf_condition_len=None,
                     long_tok=None, compose=None, **kwargs):
        """Runs plan.program once: resolves the guidance copies and the lane count, builds the lanes, issues `issue_schedule`'s
        entries and joins the lanes' streams."""
        dev = self.device
        if dev.type != "cuda":
            raise GsddError("sampling runs on the HIP path only: move the module to a ROCm device")
        B, L, K = self._batch_of(condition_token, kwargs), self.shape, self.num_classes - 1
        cond = condition_embed.to(dev).float()
        cf = cf_condition_embed.to(dev).float().type_as(cond) if (self._guided or compose is not None) else None
        # Identical conditional and unconditional embeddings -- the reference's shipped inference path: DiscreteDiffusion.forward zeroes
        # both (discrete_diffusion.py:25, :49) -- make the two guidance copies the same computation on the same inputs, bit for bit.
        # Then one copy runs and the step kernel reads its logits on both sides of log p_u + s (log p_c - log p_u): the same values
        # through the same arithmetic as the stacked pass, at half the denoiser work.  (One host comparison per sample() call;
        # GSDD_CFG_DEDUPE=0 keeps the two copies.)
        # (With condition lengths the copies must also attend to the same rows: equal lengths.)
        lens = None
        if condition_len is not None or cf_condition_len is not None:
            if cond.dim() != 3:
                raise GsddError(f"condition_len needs condition_embed (B, Te, cond_dim), got {tuple(cond.shape)}")
            lens = _guidance_lens(condition_len, cf_condition_len, B, cond.shape[1], self._guided or compose is not None)
        same_cond = (compose is None and self._guided and os.environ.get("GSDD_CFG_DEDUPE", "1") != "0" and cf.shape == cond.shape
                     and bool(torch.equal(cond, cf)) and (lens is None or bool(torch.equal(lens[0], lens[1]))))
        rep = 2 if (self._guided and not same_cond) else 1
        if compose is not None:
            # A composed call: rep = N + 1 copies, cat([c_0, ..., c_{N-1}, u]), never deduplicated; the lengths stack the same way
            # (an extra condition's default is full length, as the unconditional copy's)
            if cf.shape != cond.shape:
                raise GsddError(f"a composed call needs cf_condition_embed shaped like condition_embed {tuple(cond.shape)}, got {tuple(cf.shape)}")
            extra = [e.to(dev).float() for e in compose.embeds]
            same_cond, rep, Te = False, len(extra) + 2, cond.shape[1]
            if (lens is not None or compose.lens is not None) and Te > 1:
                full = torch.full((B,), Te, dtype=torch.int32)
                len_c, len_u = (full, full) if lens is None else (lens[0], full if lens[1] is None else lens[1])
                lens = [len_c, *(compose.lens if compose.lens is not None else [full] * len(extra)), len_u]
            else:
                lens = None
        x0 = None
        if plan.q_sample:
            x0 = content_token.to(dev).long().reshape(B, L).contiguous()
            if int(x0.min()) < 0 or int(x0.max()) > K:
                raise GsddError("content_token outside [0, num_embed]")
        # Two lanes by default (measured +8.5 % at bs 16: BENCH_r02 extra.two_lanes); a lane keeps at least 4 clips.  An eager or
        # traced call runs in one.
        graphed = use_graph and trace is None
        lanes = kwargs.get("lanes", os.environ.get("GSDD_SAMPLE_LANES", self.sample_lanes))
        lanes = 2 if lanes is None else int(lanes)
        lanes = lanes if (graphed and lanes > 1 and B % lanes == 0 and B // lanes >= 4) else 1
        # hipGraph capture is not allowed on the legacy default stream: the lanes run on side streams
        if getattr(self, "_streams", None) is None or len(self._streams) < lanes:
            self._streams = [torch.cuda.Stream(device=dev) for _ in range(lanes)]
        cur = torch.cuda.current_stream()
        self.transformer.packed()                   # packed weights, AdaLN tables and the fragment images are (re)built HERE, on the
        self.transformer.fragment_images()          # caller's stream: each lane's wait_stream(cur) below then orders its reads after them
        lane_list = []

        def lane(ln):
            # Lanes are set up on first use, in order: lane 0's first op is on the GPU while the host sets up lane 1 (setting every
            # lane up before the first op measured 0.08 % slower at the headline shape)
            while len(lane_list) <= ln:
                st = self._streams[len(lane_list)]
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    sl = slice(len(lane_list) * (B // lanes), (len(lane_list) + 1) * (B // lanes))
                    if compose is not None:
                        conds = torch.cat([cond[sl], *(e[sl] for e in extra), cf[sl]], 0)
                        lane_len = None if lens is None else torch.cat([n[sl] for n in lens])
                        lane_list.append(_Lane(self, plan, st, sl, conds, rep, x0, known, _trunc_kwargs(truncation_rate), lane_len, long_tok,
                                               compose_w=compose.weights[sl]))
                        continue
                    conds = torch.cat([cond[sl], cf[sl]], 0) if rep == 2 else cond[sl]
                    lane_len = None if lens is None else (torch.cat([lens[0][sl], lens[1][sl]]) if rep == 2 else lens[0][sl])
                    lane_list.append(_Lane(self, plan, st, sl, conds, rep, x0, known, _trunc_kwargs(truncation_rate), lane_len, long_tok))
            return lane_list[ln]
        for ln, kind, action in issue_schedule(plan.program, lanes, graphed):
            lane(ln).issue(kind, action, trace)
        lane(lanes - 1)                             # (an empty program: the all-[MASK] start is the result)
        if long_tok is not None:                    # a rollout: the last window's frames join the long buffer (no slide follows it)
            for lane in lane_list:
                lane.slide(final=True)
        for lane in lane_list:
            cur.wait_stream(lane.st)
            lane.tok.record_stream(cur)
        self._redo_counters = [lane.ws["redo"] for lane in lane_list]      # attention chunk-redo events of this call, per lane
        self._range_flags = [lane.ws["range"] for lane in lane_list]
        self._bad_counters = [lane.bad for lane in lane_list] if long_tok is not None else []
        # the graphs live until the next call: their replays may still be in flight when this one returns
        self._last_graphs = [lane.graphs for lane in lane_list]
        self._last_jump_graphs = [lane.graphs.get("jump") for lane in lane_list] if graphed and "jump" in plan.program else []
        self._last_lanes, self._last_plan, self._last_cfg_dedupe, self._last_draws = lanes, plan, same_cond, plan.draws
        self.noise_stream += plan.draws
        if return_logits:
            raise NotImplementedError("return_logits is unused by the reference call sites")
        if long_tok is not None:
            return {"content_token": long_tok}
        return {"content_token": lane_list[0].tok if lanes == 1 else torch.cat([lane.tok for lane in lane_list], 0)}

    def attention_redo_events(self):
        """Chunk-redo events of the attention kernel during the last sample() call (synchronises: reads device counters)."""
        return int(sum(int(c.item()) for c in getattr(self, "_redo_counters", [])))

    # ------------------------------------------------------------------ single-step pieces (parity tests, training glue)
    @torch.no_grad()
    def p_sample_tokens(self, tok, cond, cf_cond, t, stream_id, post_dbg=None, x0_dbg=None, post_skip=0, truncation_rate=None,
                        known=None, condition_len=None, cf_condition_len=None):
        """One reverse step on tokens (p_sample, diffusion_transformer.py:304-352, prior_rule 0); post_skip > 0: the posterior at
        t - post_skip for t > post_skip (a sample_fast step, :700-704); truncation_rate: top-r truncation of the guided row;
        known: what `check_known` returns (mask, clean tokens, mode) -- those positions skip the learned step as in sample();
        condition_len / cf_condition_len: as in sample()."""
        trunc_kw = _trunc_kwargs(check_truncation_rate(truncation_rate))
        dev = tok.device
        known_kw = _known_kwargs(known, dev)
        B, L = tok.shape
        K, T = self.num_classes - 1, self.num_timesteps
        guided = self._guided
        rep = 2 if guided else 1
        conds = torch.cat([cond, cf_cond], 0).float().contiguous() if guided else cond.float().contiguous()
        tr = self.transformer
        ws = tr.workspace(rep * B, L, dev, rep=rep)
        condv = tr.cond_vectors(conds)
        t2 = torch.cat([t, t]).contiguous() if guided else t.contiguous()
        lens = None
        if condition_len is not None or cf_condition_len is not None:
            lens = _guidance_lens(condition_len, cf_condition_len, B, conds.shape[1], guided)
        cond_len = None if lens is None else (torch.cat(lens) if guided else lens[0]).to(dev)
        logits = tr.run_checked(tok.contiguous(), condv, conds.shape[1], t2.long(), ws, rep=rep, cond_len=cond_len)
        sid = torch.tensor([stream_id], dtype=torch.int64, device=dev)
        out = torch.empty_like(tok)
        M = B * L
        ops.d3pm_step(logits[:M], logits[M:] if guided else None, tok, out, self._sched(), t2, sid, K=K, T=T,
                      guidance=float(self.guidance_scale), seed=self.noise_seed, row0=self.row_offset * L,
                      post_dbg=post_dbg, x0_dbg=x0_dbg, post_skip=post_skip, **trunc_kw, **known_kw)
        return out

    # ------------------------------------------------------------------ training objective (forward value)
    def sample_time(self, b, device, method="uniform"):
        """diffusion_transformer.py:368-389 (host-side control flow; importance sampling once every Lt_count > 10)."""
        if method == "importance":
            if not (self.Lt_count > 10).all():
                return self.sample_time(b, device, method="uniform")
            Lt_sqrt = torch.sqrt(self.Lt_history + 1e-10) + 0.0001
            Lt_sqrt[0] = Lt_sqrt[1]
            pt_all = Lt_sqrt / Lt_sqrt.sum()
            t = torch.multinomial(pt_all, num_samples=b, replacement=True)
            return t, pt_all.gather(dim=0, index=t)
        if method == "uniform":
            t = torch.randint(0, self.num_timesteps, (b,), device=device).long()
            return t, torch.ones_like(t).float() / self.num_timesteps
        raise ValueError(method)

    @torch.no_grad()
    def _train_loss(self, x, cond_emb, is_train=True, want_probs=True, cond_len=None):
        """_train_loss (diffusion_transformer.py:391-457) as HIP kernels: q_sample -> denoiser -> fused KL/NLL/aux
        reduction (forward value; the gradient path is d3pm_train.py, reached through forward() when autograd is enabled)."""
        dev = x.device
        B, L = x.shape
        K, T = self.num_classes - 1, self.num_timesteps
        t, pt = self.sample_time(B, dev, "importance")
        t = t.to(dev).long().contiguous()
        pt = pt.to(dev).float().contiguous()
        sid = torch.tensor([self.noise_stream], dtype=torch.int64, device=dev)
        self.noise_stream += 1
        sched = self._sched()
        x0 = x.contiguous().long()
        xt = torch.empty_like(x0)
        ops.d3pm_q_sample(x0, xt, sched, t, sid, K=K, T=T, seed=self.noise_seed, row0=self.row_offset * L)
        tr = self.transformer
        ws = tr.workspace(B, L, dev)
        cond = cond_emb.float().contiguous()
        if cond_len is not None:      # (B,) condition lengths: validated on the host; one token -> nothing to mask
            cond_len = check_condition_len(cond_len, B, cond.shape[1], "condition_len")
            cond_len = cond_len.to(dev) if cond.shape[1] > 1 else None
        logits = tr.run_checked(xt, tr.cond_vectors(cond), cond.shape[1], t, ws, cond_len=cond_len)
        aux_w = self.auxiliary_loss_weight if is_train else 0.0
        out = ops.d3pm_train_loss(logits, x0, xt, t, pt, sched, self.Lt_history, self.Lt_count, K=K, T=T,
                                  mask_weight=self.mask_weight, aux_weight=aux_w,
                                  adaptive_aux=self.adaptive_auxiliary_loss, want_probs=want_probs)
        out["t"], out["xt"] = t, xt
        return out

    def forward(self, input, return_loss=False, return_logits=True, return_att_weight=False, is_train=True, **kwargs):
        """diffusion_transformer.py:520-565 -> {'logits': exp(log_model_prob) (B,K+1,L), 'loss', 'pred_data' (B,L)}.
        input["condition_len"] (optional, (B,) integers in [1, Te]): sample b is conditioned on the first condition_len[b] rows of
        condition_embed_token[b] only (caption padding behind them; the rows must still be finite when training)."""
        tok = input["content_token"]
        if not tok.is_cuda:
            raise GsddError("the HIP path needs tensors on a ROCm device (no CPU fallback)")
        cond = input.get("condition_embed_token")
        if cond is None:
            raise NotImplementedError("cond_emb=None is not used by the reference call sites")
        if torch.is_grad_enabled() and is_train and self.training and any(p.requires_grad for p in self.transformer.parameters()):
            # the loss carries a grad_fn into the HIP backward (d3pm_train.py): loss.backward() fills the transformer's .grad
            # (condition dropout -- cond_drop_prob, or the explicit input["condition_drop"] (B,) bool mask -- applies here only: the
            # no-grad objective below and the sampler never drop a condition)
            from .d3pm_train import train_forward
            loss, r = train_forward(self, tok, cond.float(), want_probs=return_logits, null_cond=input.get("null_condition_embed_token"),
                                    drop=input.get("condition_drop"), cond_len=input.get("condition_len"))
            out = {"pred_data": r["x0_recon"]}
            if return_logits:
                out["logits"] = r["probs"]
            if return_loss:
                out["loss"] = loss
            self.last_train_stats = r
            return out
        out = {}
        if is_train:
            r = self._train_loss(tok, cond.float(), is_train=True, want_probs=return_logits, cond_len=input.get("condition_len"))
            if return_logits:
                out["logits"] = r["probs"]
            if return_loss:
                out["loss"] = r["loss"][0]
            out["pred_data"] = r["x0_recon"]
            self.last_train_stats = r
        return out


def _instantiate(cfg):
    """discrete_diffusion.py:11-12: plain dicts (hydra_lite's composition) or DictConfigs (real hydra, when installed)."""
    if isinstance(cfg, dict):
        from .hydra_lite import instantiate
    else:
        from hydra.utils import instantiate
    return instantiate(cfg)


class Deferred:
    """A value of LazyOutputs that is computed when somebody asks for it."""

    def __init__(self, fn):
        self.fn = fn


class LazyOutputs(collections.abc.MutableMapping):
    """The generator's output dict with its two pure, unconditionally computed by-products deferred: `pred_data` (training: the decode
    of the single-step prediction) / `pred_single_step` (inference) and `test` (the decode of the input's own codes) are full VQ-VAE
    decodes -- 2 x 30 ms at bs 16 beside a 57 ms denoiser step -- that the reference's stage-2 training step computes and never reads
    (its loss is `outputs['losses']`: metrics/loss_func.py:10-14, multistage_text_motion_model.py:170-190).  They are deterministic
    functions of tokens and frozen weights, so computing them on first access gives every reader the same tensors; readers that copy the
    mapping (`dict.update`, `dict(...)`) trigger them, as do `items()` / `values()`.  `pending()` lists what has not been computed."""

    def __init__(self, **items):
        self._d = dict(items)

    def __getitem__(self, k):
        v = self._d[k]
        if isinstance(v, Deferred):
            with torch.no_grad():
                v = v.fn()
            self._d[k] = v
        return v

    def __setitem__(self, k, v):
        self._d[k] = v

    def __delitem__(self, k):
        del self._d[k]

    def __iter__(self):
        return iter(self._d)

    def __len__(self):
        return len(self._d)

    def __contains__(self, k):                  # (the Mapping default would go through __getitem__ and compute the value)
        return k in self._d

    def pending(self):
        return sorted(k for k, v in self._d.items() if isinstance(v, Deferred))


class DiscreteDiffusion(nn.Module):
    """Drop-in for src/models/networks/discrete_diffusion.py:8-83 (generator glue).  `textencoder` and
    `diffusion_model` may be already-built modules or (with hydra present) configs to instantiate.

    zero_text_emb=True is the reference as written: both text embeddings are replaced by zeros (discrete_diffusion.py:25, :49).
    False lets the captions condition the denoiser.
    sample_skip_step=None samples with DiffusionTransformer.sample (every timestep); an int s samples with sample_fast(skip_step=s).
    sample_prior_rule / sample_prior_weight / sample_prior_ps: when not None, set the diffusion model's prior_rule / prior_weight /
    prior_ps before sampling (purity-prior inference; prior_ps also reloads the reference's n_sample list);
    sample_prior_scale_schedule=True rescales that list from 1024 tokens to the model's content_seq_len (scaled_n_sample).
    sample_truncation_rate: when not None, sets the diffusion model's truncation_rate before sampling (top-r truncated sampling,
    0 < r < 1; VQ-Diffusion's inference uses 0.86).
    sample_condition_frames: null, an int k in [1, t_latent) or a list of latent frame indices: forward(do_inference=True) then keeps
    those latent frames of the input clip (its own codes) and samples the rest (frame prediction / interpolation; `frame_mask`);
    sample_known_mode "renoise" / "hold" is the sampler's known_mode.  Not with sample_prior_rule > 0.
    sample_resample_jump / sample_resample_times: the sampler's resample_jump / resample_times (RePaint's resampling jumps), handed to
    sample() when a mask is in use; null leaves the plain known chain.  Not with sample_skip_step (sample_fast has no jumps).
    train_cond_drop_prob: null, or the probability in [0, 1] with which a training sample's text condition is replaced by the null
    condition (classifier-free training; sets the diffusion model's cond_drop_prob).  The null condition is the learned
    empty_text_embed when the diffusion model has learnable_cf, else the provider's embedding of "" -- the unconditional branch the
    sampler guides with.
    mask_text_padding: true asks a per-token provider for each caption's length (end-of-text position + 1) and hands it to the training
    objective and the sampler as condition lengths: the cross-attention then runs over a caption's own tokens and never reads the
    padding behind them, so a sample does not depend on how wide the batch was padded.  The unconditional copy and a dropped training
    sample stay full length.  Dropped with zero_text_emb (condition and null condition are the same zeros there).
    sample_long_frames: null, or the number of latent frames of a long clip (at least the model's window): the render path
    (src/models/base.py) and sample_videos(long_frames=) then sample it with DiffusionTransformer.sample_long -- windows that share
    sample_long_overlap latent frames -- and decode it with VQVAE.decode_long, sample_long_blend "linear" / "keep" / "replace" across
    the overlaps.  forward(do_inference=True) keeps sampling one window.  Not with sample_prior_rule > 0.
    sample_compose: null, or a list of at most three {text, weight} entries shared by every clip of a batch: composed guidance
    (DiffusionTransformer.sample's compose_embeds / compose_weights) -- a clip is sampled under x_u + w_0 (x_caption - x_u) +
    sum_i weight_i (x_text_i - x_u) in log-probability space, a negative weight pushing away from its text (a negative prompt).
    sample_compose_caption_weight is w_0; null takes the diffusion model's guidance_scale.  Not with zero_text_emb: true."""

    def __init__(self, textencoder, diffusion_model, zero_text_emb=True, sample_skip_step=None, sample_prior_rule=None,
                 sample_prior_weight=None, sample_prior_ps=None, sample_prior_scale_schedule=False, sample_truncation_rate=None,
                 sample_condition_frames=None, sample_known_mode="renoise", sample_resample_jump=None, sample_resample_times=None,
                 sample_long_frames=None, sample_long_overlap=4, sample_long_blend="linear",
                 sample_compose=None, sample_compose_caption_weight=None,
                 train_cond_drop_prob=None, mask_text_padding=False, **kwargs):
        super().__init__()
        self.sample_compose = check_compose_entries(sample_compose, "sample_compose")
        if self.sample_compose is not None and zero_text_emb:
            raise GsddError("sample_compose cannot be combined with zero_text_emb: true -- every caption would be the same zero vectors; "
                            "set zero_text_emb: false")
        w = sample_compose_caption_weight
        if w is not None and (isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(w)):
            raise GsddError(f"sample_compose_caption_weight must be null or a finite number, got {w!r}")
        self.sample_compose_caption_weight = None if w is None else float(w)
        if sample_long_frames is not None and not (_is_int(sample_long_frames) and sample_long_frames >= 2):
            raise GsddError(f"sample_long_frames must be null or an int >= 2 (latent frames of the long clip), got {sample_long_frames!r}")
        if not (_is_int(sample_long_overlap) and sample_long_overlap >= 1):
            raise GsddError(f"sample_long_overlap must be an int >= 1 (latent frames two windows share), got {sample_long_overlap!r}")
        if not isinstance(sample_long_blend, str) or sample_long_blend not in ops.BLEND_MODES:
            raise GsddError(f"sample_long_blend must be one of {sorted(ops.BLEND_MODES)}, got {sample_long_blend!r}")
        if sample_long_frames is not None and sample_prior_rule:
            raise GsddError("sample_long_frames and sample_prior_rule > 0 cannot be combined: the overlap frames are known tokens and the "
                            "purity prior's reveal schedule counts [MASK] positions")
        self.sample_long_frames = None if sample_long_frames is None else int(sample_long_frames)
        self.sample_long_overlap, self.sample_long_blend = int(sample_long_overlap), sample_long_blend
        if not isinstance(mask_text_padding, bool):
            raise GsddError(f"mask_text_padding must be true or false, got {mask_text_padding!r}")
        self.mask_text_padding = mask_text_padding
        p_drop = None if train_cond_drop_prob is None else check_cond_drop_prob(train_cond_drop_prob, "train_cond_drop_prob")
        if not isinstance(textencoder, nn.Module) and not callable(textencoder):
            textencoder = _instantiate(textencoder)
        if not isinstance(diffusion_model, nn.Module):
            diffusion_model = _instantiate(diffusion_model)
        self.textencoder = textencoder
        self.diffusion_model = diffusion_model
        if p_drop is not None:
            diffusion_model.cond_drop_prob = p_drop
        self._null_text = None         # the provider's embedding of "" (1, Te, C): the null condition without learnable_cf
        self.zero_text_emb = bool(zero_text_emb)
        if sample_skip_step is not None and (isinstance(sample_skip_step, bool) or not isinstance(sample_skip_step, numbers.Integral)
                                             or sample_skip_step < 0):
            raise GsddError(f"sample_skip_step must be null or a non-negative int, got {sample_skip_step!r}")
        self.sample_skip_step = None if sample_skip_step is None else int(sample_skip_step)
        if sample_prior_rule is not None and not (_is_int(sample_prior_rule) and sample_prior_rule in (0, 1, 2)):
            raise GsddError(f"sample_prior_rule must be null, 0, 1 or 2, got {sample_prior_rule!r}")
        if sample_prior_weight is not None and (isinstance(sample_prior_weight, bool) or not isinstance(sample_prior_weight, numbers.Real)
                                                or not sample_prior_weight >= 0):
            raise GsddError(f"sample_prior_weight must be null or a number >= 0, got {sample_prior_weight!r}")
        if sample_prior_ps is not None and not (_is_int(sample_prior_ps) and sample_prior_ps >= 1):
            raise GsddError(f"sample_prior_ps must be null or an int >= 1, got {sample_prior_ps!r}")
        if not isinstance(sample_prior_scale_schedule, bool):
            raise GsddError(f"sample_prior_scale_schedule must be true or false, got {sample_prior_scale_schedule!r}")
        if sample_prior_rule and self.sample_skip_step is not None:
            raise GsddError("sample_prior_rule > 0 and sample_skip_step cannot be combined: sample_fast has no purity prior "
                            "(diffusion_transformer.py:648-713)")
        self.sample_prior_rule = None if sample_prior_rule is None else int(sample_prior_rule)
        self.sample_prior_weight = None if sample_prior_weight is None else float(sample_prior_weight)
        self.sample_prior_ps = None if sample_prior_ps is None else int(sample_prior_ps)
        self.sample_prior_scale_schedule = sample_prior_scale_schedule
        self.sample_truncation_rate = check_truncation_rate(sample_truncation_rate, "sample_truncation_rate")
        if sample_condition_frames is not None:
            frames = sample_condition_frames
            if _is_int(frames):
                if frames < 1:
                    raise GsddError(f"sample_condition_frames must be null, an int >= 1 or a list of frame indices, got {frames!r}")
                frames = int(frames)
            else:
                try:
                    frames = [v for v in frames] if not isinstance(frames, (str, bytes)) else None
                except TypeError:
                    frames = None
                if not frames or not all(_is_int(v) for v in frames):
                    raise GsddError("sample_condition_frames must be null, an int >= 1 or a non-empty list of frame indices, "
                                    f"got {sample_condition_frames!r}")
                frames = [int(v) for v in frames]
            if sample_prior_rule:
                raise GsddError("sample_condition_frames and sample_prior_rule > 0 cannot be combined: the purity prior's reveal "
                                "schedule counts [MASK] positions")
            sample_condition_frames = frames
        if not isinstance(sample_known_mode, str) or sample_known_mode not in KNOWN_MODES:
            raise GsddError(f"sample_known_mode must be one of {sorted(KNOWN_MODES)}, got {sample_known_mode!r}")
        self.sample_condition_frames = sample_condition_frames
        self.sample_known_mode = sample_known_mode
        for name, v, lo in (("sample_resample_jump", sample_resample_jump, 1), ("sample_resample_times", sample_resample_times, 1)):
            if v is not None and not (_is_int(v) and v >= lo):
                raise GsddError(f"{name} must be null or an int >= {lo}, got {v!r}")
        if sample_resample_times is not None and sample_resample_times > 1 and sample_resample_jump is None:
            raise GsddError(f"sample_resample_times = {sample_resample_times} needs sample_resample_jump")
        if sample_resample_jump is not None and self.sample_skip_step is not None:
            raise GsddError("sample_resample_jump and sample_skip_step cannot be combined: sample_fast has no resampling jumps")
        self.sample_resample_jump = None if sample_resample_jump is None else int(sample_resample_jump)
        self.sample_resample_times = None if sample_resample_times is None else int(sample_resample_times)

    def condition_frame_mask(self, latent_shape):
        """-> None or the (L,) bool mask of sample_condition_frames on this latent grid (validated here, at sampling time)."""
        frames = self.sample_condition_frames
        if frames is None:
            return None
        if isinstance(frames, int) and not 1 <= frames < latent_shape[0]:
            raise GsddError(f"sample_condition_frames = {frames} must lie in [1, {latent_shape[0]}): the latent has {latent_shape[0]} "
                            "frames and at least one must be left to sample")
        return frame_mask(latent_shape, frames)

    def _text(self, texts, dev, return_lengths=False):
        """-> the (B, Te, C) condition of `texts`; return_lengths: (condition, the captions' int32 (B,) host lengths, or None when
        mask_text_padding is off or the embedding is zeroed)."""
        want = return_lengths and self.mask_text_padding and not self.zero_text_emb
        emb, lens = self.textencoder(texts, return_lengths=True) if want else (self.textencoder(texts), None)
        emb = (emb.unsqueeze(1) if emb.dim() == 2 else emb).to(dev)   # (B, C) pooled, or (B, Te, C) from a per-token provider
        emb = torch.zeros_like(emb) if self.zero_text_emb else emb.float()
        return (emb, lens) if return_lengths else emb

    def null_condition(self, dev):
        """The null condition a training step with condition dropout needs from the caller: None when nothing is dropped or the
        diffusion model learns its own (learnable_cf), else the provider's embedding of "" (1, Te, C), computed once."""
        dm = self.diffusion_model
        if not getattr(dm, "cond_drop_prob", 0.0) or dm.learnable_cf:
            return None
        if self._null_text is None or self._null_text.device != torch.device(dev):
            with torch.no_grad():
                self._null_text = self._text([""], dev)
        return self._null_text

    def forward(self, batch, autoencoder, length_estimator=None, do_inference=False):
        """discrete_diffusion.py:16-83: encode -> diffusion objective -> [sample] -> decode; same output-dict keys.
        `losses` carries the HIP backward's grad_fn when autograd is enabled and the denoiser is in train mode, so the caller's
        `manual_backward(loss)` (multistage_text_motion_model.py:186-197) fills the transformer's .grad.  Encode, both decodes
        and the sampler are not differentiable in the reference either (arg-min / arg-max cut the graph) and run under no_grad."""
        dev = autoencoder.device
        x = batch["video"].to(dev)
        from .parallel import broadcast_buffers, set_rank_noise_rows
        set_rank_noise_rows(self.diffusion_model, x.shape[0])          # data parallel: the ranks draw different noise rows
        if self.diffusion_model.training:
            broadcast_buffers(self.diffusion_model)                    # DDP's per-forward buffer broadcast (Lt_history / Lt_count)
        with torch.no_grad():
            quant = autoencoder.encode(x)
        quant_flat = quant.view(x.shape[0], -1)
        with torch.no_grad():
            text_emb, text_len = self._text(batch["text"], dev, return_lengths=True)
        diffusion_out = self.diffusion_model({"condition_embed_token": text_emb, "content_token": quant_flat,
                                              "null_condition_embed_token": self.null_condition(dev), "condition_len": text_len},
                                             return_loss=True, return_logits=False)   # (`logits` = exp(log_model_prob), a (B, K+1, L)
        # tensor the reference computes here and never reads (discrete_diffusion.py:38-41, :66-81): not asked for, so the loss and its gradient take the one-pass kernel)
        # arg-max over K+1 classes can only return [MASK] when every code row sits at the -70 clamp; the reference would
        # then fail inside F.embedding, we decode code K-1 instead
        pred_tokens = diffusion_out["pred_data"].view(quant.shape).clamp(max=autoencoder.n_codes - 1)
        # the two decodes nobody may ever read (LazyOutputs): deferred while the VQ-VAE is frozen in eval mode (a train-mode decode
        # would update BatchNorm statistics: then it happens here, as in the reference); GSDD_EAGER_OUTPUTS=1 computes them here too
        lazy = (not autoencoder.training) and os.environ.get("GSDD_EAGER_OUTPUTS") is None
        # a deferred decode must be the decode the eager call would have made: it is refused if the VQ-VAE's weights have been replaced or
        # updated (through torch) since this forward (the reference decodes here, under the weights of this moment)
        weights_now = lambda: tuple((p.data_ptr(), p._version) for p in autoencoder.parameters())
        weights_then = weights_now() if lazy else None

        def deferred_decode(tokens):
            def fn():
                if weights_then is not None and weights_now() != weights_then:
                    raise GsddError("the VQ-VAE's weights changed between DiscreteDiffusion.forward and the first read of a deferred output "
                                    "(pred_data / pred_single_step / test): read it before updating the autoencoder, or set "
                                    "GSDD_EAGER_OUTPUTS=1 to decode inside forward as the reference does")
                return autoencoder.decode(tokens)
            return Deferred(fn)
        single_step_out = deferred_decode(pred_tokens)
        test = deferred_decode(quant)
        with torch.no_grad():
            if do_inference:                # (the sampler draws from the noise stream: always at this point of the call)
                shape = tuple(quant.shape[1:])
                mask = self.condition_frame_mask(shape)     # the conditioned latent frames keep the input clip's own codes
                known_kw = {} if mask is None else {"known_tokens": quant_flat, "known_mask": mask}
                inference_out = self.sample_videos(batch["text"], autoencoder, latent_shape=shape, text_emb=text_emb, text_len=text_len,
                                                   **known_kw)
        if do_inference:
            out = LazyOutputs(pred_data=inference_out, pred_single_step=single_step_out, gt_data=x, losses=diffusion_out["loss"], test=test)
        else:
            out = LazyOutputs(pred_data=single_step_out, gt_data=x, losses=diffusion_out["loss"], test=test)
        if not lazy:
            for k in list(out):
                out[k]
        return out

    @torch.no_grad()
    def sample_videos(self, texts, autoencoder, latent_shape=None, text_emb=None, known_tokens=None, known_mask=None, text_len=None,
                      long_frames=None, compose=None):
        """The inference branch of forward (discrete_diffusion.py:44-62): text -> tokens -> decoded clips.
        known_tokens (B, L) / known_mask ((B, L) or (L,) bool): clean tokens to keep at the mask's positions (the sampler's
        content_token / known_mask, with sample_known_mode); without a mask the call is the plain one.
        text_len goes with text_emb: the captions' (B,) condition lengths (the sampler's condition_len), None for none; without
        text_emb both come from the provider.
        long_frames: None, or the latent frames n of a long clip: sample_long with sample_long_overlap (the mask, if any, applies to
        its first window), then decode_long with sample_long_blend -> (B, 3, n d_t, H, W); last_content_token is the long grid.
        compose: None (then sample_compose), or that list for this call: every clip is sampled under its own caption at
        sample_compose_caption_weight (null: the diffusion model's guidance_scale) composed with the listed texts at their weights
        (the sampler's compose_embeds / compose_weights, with the texts' lengths under mask_text_padding)."""
        dev = autoencoder.device
        B = len(texts)
        compose = self.sample_compose if compose is None else check_compose_entries(compose)
        if compose is not None and self.zero_text_emb:
            raise GsddError("compose cannot be combined with zero_text_emb: every caption would be the same zero vectors")
        if text_emb is None:
            text_emb, text_len = self._text(texts, dev, return_lengths=True)
        if self.zero_text_emb:
            text_len = None
        dm = self.diffusion_model
        if dm.learnable_cf:                     # the learned null embedding is the unconditional condition (diffusion_transformer.py:541-543)
            cf_emb = dm._cf_embed(text_emb, None)
        else:
            cf_emb = self._text([""] * B, dev)                                          # :46-49
        if self.sample_prior_rule is not None:
            dm.prior_rule = self.sample_prior_rule
        if self.sample_prior_weight is not None:
            dm.prior_weight = self.sample_prior_weight
        if self.sample_prior_ps is not None:
            dm.prior_ps = self.sample_prior_ps
            dm.update_n_sample()
        if self.sample_truncation_rate is not None:
            dm.truncation_rate = self.sample_truncation_rate
        if self.sample_prior_scale_schedule and self.sample_skip_step is None and dm.prior_rule:
            ref = reference_n_sample(dm.num_timesteps, dm.prior_ps)
            if ref is None:
                raise GsddError(f"sample_prior_scale_schedule: the reference has no n_sample list for num_timesteps = {dm.num_timesteps}")
            dm.n_sample = scaled_n_sample(ref, dm.shape)
        if known_mask is None:
            content, known_kw = None, {}
        else:
            content, known_kw = known_tokens, {"known_mask": known_mask, "known_mode": self.sample_known_mode}
            if self.sample_resample_jump is not None:
                known_kw.update(resample_jump=self.sample_resample_jump,
                                resample_times=1 if self.sample_resample_times is None else self.sample_resample_times)
        if text_len is not None:
            known_kw = dict(known_kw, condition_len=text_len)          # (the unconditional copy stays full length)
        if compose is not None:
            w0 = dm.guidance_scale if self.sample_compose_caption_weight is None else self.sample_compose_caption_weight
            extra = [self._text([text] * B, dev, return_lengths=True) for text, _ in compose]
            known_kw = dict(known_kw, compose_embeds=[e for e, _ in extra], compose_weights=[float(w0)] + [w for _, w in compose])
            if text_len is not None and all(n is not None for _, n in extra):
                known_kw["compose_lens"] = [n for _, n in extra]
        shape = tuple(latent_shape if latent_shape is not None else autoencoder.latent_shape)
        if long_frames is not None:
            long_kw = dict({"known_mode": self.sample_known_mode}, **known_kw)
            if self.sample_resample_jump is not None:          # (every window from the second on has known frames to harmonise with)
                long_kw.update(resample_jump=self.sample_resample_jump,
                               resample_times=1 if self.sample_resample_times is None else self.sample_resample_times)
            out = dm.sample_long(texts, None, text_emb, cf_emb, latent_shape=shape, n_frames=long_frames, overlap=self.sample_long_overlap,
                                 content_token=content, skip_step=self.sample_skip_step, **long_kw)
            self.last_content_token = out["content_token"]
            return autoencoder.decode_long(out["content_token"].view(B, long_frames, *shape[1:]), self.sample_long_overlap,
                                           blend=self.sample_long_blend)
        if self.sample_skip_step is None:
            out = self.diffusion_model.sample(texts, None, text_emb, cf_emb, content_token=content, filter_ratio=0, **known_kw)
        else:
            out = self.diffusion_model.sample_fast(texts, None, text_emb, content_token=content, filter_ratio=0,
                                                   skip_step=self.sample_skip_step, cf_condition_embed=cf_emb, **known_kw)
        self.last_content_token = out["content_token"]
        return autoencoder.decode(out["content_token"].view(B, *shape))

    def get_text_embeddings(self, features):                                           # discrete_diffusion.py:91-94
        emb = self.textencoder(features)
        return emb.unsqueeze(1) if emb.dim() == 2 else emb
