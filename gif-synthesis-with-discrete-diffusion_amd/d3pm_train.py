"""D3PM training step on the HIP path: forward with saved activations, analytic backward, Adam, data-parallel gradient
all-reduce.  Correctness-first (one launch per operator, f32 MFMA GEMMs, VALU attention backward): parity-tested against
torch.autograd of the CPU oracle; the sampling path does not depend on anything here.

Reference: MultistageTextMotionModel.allsplit_step (src/models/multistage_text_motion_model.py:170-206: zero_grad ->
manual_backward -> Adam(lr 1e-4, betas (0.5, 0.999))) around DiffusionTransformer._train_loss
(src/models/motionencoder/diffusion_transformer.py:391-457); DDP gradient averaging = configs/trainer/default.yaml:8."""
import contextlib
import itertools
import os
import warnings

import numpy as np
import torch

from . import ops
from ._optim import GradArena, GradBook, MultiAdam, check_stage_args, linear_warmup          # noqa: F401  (linear_warmup: the shipped lr_schedule)
from ._lib import GsddError
from .parallel import GradReducer, broadcast_module, world_size

BUCKET_LAYERS = 5          # blocks per gradient bucket: 19 blocks + head + embeddings -> 5 all-reduces of ~2.7 MB each


class _LinearImages:
    """bf16x3 fragment images (gsdd_rows_linear) of every block's weight matrices and of their transposes (the data-gradient
    operands), all refreshed by ONE launch per optimiser step.  The descriptor table points at the parameters themselves (the
    optimisers update them in place); `refresh` rebuilds it if a parameter has moved."""
    NAMES = ("qkv", "qkv_t", "proj", "proj_t", "w1", "w1_t", "w2", "w2_t")
    CROSS_NAMES = ("q2", "q2_t", "proj2", "proj2_t")      # attn2.query / attn2.proj: from the first step with more than one condition token

    def __init__(self, tr):
        self.tr = tr
        self.ptrs = None
        self.cross = False

    def _pieces(self, blk):
        a, m = blk.attn1, blk.mlp
        q, k, v = a.query.weight, a.key.weight, a.value.weight
        # name -> (n_out, n_in, [(weight, rows of the image matrix it fills, columns, transpose, fragment offset)])
        pieces = {
            "qkv": (192, 64, [(w, 64, 64, 0, 8 * j) for j, w in enumerate((q, k, v))]),
            "qkv_t": (64, 192, [(w, 64, 64, 1, 8 * j) for j, w in enumerate((q, k, v))]),
            "proj": (64, 64, [(a.proj.weight, 64, 64, 0, 0)]),
            "proj_t": (64, 64, [(a.proj.weight, 64, 64, 1, 0)]),
            "w1": (256, 64, [(m[0].weight, 256, 64, 0, 0)]),
            "w1_t": (64, 256, [(m[0].weight, 64, 256, 1, 0)]),
            "w2": (64, 256, [(m[2].weight, 64, 256, 0, 0)]),
            "w2_t": (256, 64, [(m[2].weight, 256, 64, 1, 0)]),
        }
        if self.cross:
            a2 = blk.attn2
            pieces.update({
                "q2": (64, 64, [(a2.query.weight, 64, 64, 0, 0)]),
                "q2_t": (64, 64, [(a2.query.weight, 64, 64, 1, 0)]),
                "proj2": (64, 64, [(a2.proj.weight, 64, 64, 0, 0)]),
                "proj2_t": (64, 64, [(a2.proj.weight, 64, 64, 1, 0)]),
            })
        return pieces

    def _build(self):
        dev = self.tr.blocks[0].mlp[0].weight.device
        per_block = sum(ops.rows_linear_image_bytes(no, ni) for no, ni, _ in self._pieces(self.tr.blocks[0]).values())
        self.buf = torch.empty((len(self.tr.blocks) * per_block,), dtype=torch.uint8, device=dev)
        rows, self.images, off = [], [], 0
        for blk in self.tr.blocks:
            imgs = {}
            for name, (no, ni, pieces) in self._pieces(blk).items():
                nbytes = ops.rows_linear_image_bytes(no, ni)
                imgs[name] = self.buf[off:off + nbytes]
                for w, po, pi, tr_, frag in pieces:
                    assert w.is_contiguous() and w.dtype == torch.float32
                    rows.append((w.data_ptr(), po, pi, w.shape[1], tr_, self.buf.data_ptr() + off + frag * 3 * 1024))
                off += nbytes
            self.images.append(imgs)
        table = np.array(rows, dtype=np.dtype([("w", "<u8"), ("n_out", "<i4"), ("n_in", "<i4"), ("ld", "<i4"), ("transpose", "<i4"),
                                               ("img", "<u8")]))
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self.n_desc = len(rows)
        self.ptrs = [r[0] for r in rows]

    def _current_ptrs(self):
        return [w.data_ptr() for blk in self.tr.blocks for _, _, pieces in self._pieces(blk).values() for w, *_ in pieces]

    def refresh(self, cross=False):
        """cross: the step needs the attn2.query / attn2.proj images too.  Once asked for they stay in the table (a one-token step
        that follows does not rebuild it); a trainer that only ever sees one token never packs them."""
        if cross and not self.cross:
            # A step captured before this one replays the pack launch on the old table and images: its graph pins them
            # (D3PMTrainer._pins), so they are simply replaced here.
            self.cross, self.ptrs = True, None
        if self.ptrs is None or self.ptrs != self._current_ptrs():
            self._build()
        ops.rows_linear_pack_many(self.table, self.n_desc, 256, 256)
        return self.images


class _RowGemm:
    """The block's row GEMMs on the branch the step takes, decided once per step: gsdd_rows_linear on the fragment images `imgs` (one
    dict per block, `_LinearImages.refresh`) when the block has the north-star widths, else (imgs None) the generic GEMM on the weight.
    `lin(i, x, name, w, n_out, ...)` is block i's matrix `name`, `lin.t(i, dy, name, w, n_out)` its transpose (the data gradient)."""

    def __init__(self, imgs, device):
        self.imgs, self.f = imgs, dict(dtype=torch.float32, device=device)

    def __call__(self, i, x, name, w, n_out, head_major=False, bias=None, residual=None, bvec=None, rows_per_batch=0):
        out = torch.empty((n_out // 4, x.shape[0], 4) if head_major else (x.shape[0], n_out), **self.f)
        if self.imgs is not None:
            return ops.rows_linear(x, self.imgs[i][name], n_out, out, bias=bias, bvec=bvec, rows_per_batch=rows_per_batch,
                                   residual=residual, head_major=head_major)
        return ops.linear(x, w, out, bias=bias, rows_per_batch=rows_per_batch, residual=residual, bvec=bvec,
                          out_mode=2 if head_major else 0)

    def t(self, i, dy, name, w, n_out):
        out = torch.empty((dy.shape[0], n_out), **self.f)
        if self.imgs is not None:
            return ops.rows_linear(dy, self.imgs[i][name + "_t"], n_out, out)
        return ops.linear(dy, w.t().contiguous(), out)


def default_decay_mask(transformer, extra_no_decay=()):
    """name -> bool over the transformer's parameters, by module type: the weight matrices of nn.Linear layers decay; biases, every
    LayerNorm / AdaLayerNorm parameter (its embedding and its linear layer included) and every nn.Embedding table do not.  Names in
    `extra_no_decay` (the learned null embedding) are added as non-decaying."""
    from .d3pm import AdaLayerNorm
    mask = {}

    def walk(mod, prefix, in_norm):
        in_norm = in_norm or isinstance(mod, (torch.nn.LayerNorm, AdaLayerNorm))
        for nm, _ in mod.named_parameters(recurse=False):
            mask[prefix + nm] = bool(isinstance(mod, torch.nn.Linear) and nm == "weight" and not in_norm)
        for cn, child in mod.named_children():
            walk(child, prefix + cn + ".", in_norm)

    walk(transformer, "", False)
    for nm in extra_no_decay:
        mask[nm] = False
    return mask


class D3PMTrainer:
    NULL_NAME = "empty_text_embed"       # the learned null embedding in the gradient dict and the optimiser's parameter list

    def __init__(self, dm, lr=1e-4, betas=(0.5, 0.999), eps=1e-8, deterministic=None, max_grad_norm=None, weight_decay=0.0,
                 ema_decay=None, skip_nonfinite=False, lr_schedule=None, decay_mask=None):
        """max_grad_norm / weight_decay / ema_decay / skip_nonfinite / lr_schedule: the optimiser stage (_optim.MultiAdam): global-norm
        clipping (torch's clip_grad_norm_), decoupled weight decay (torch.optim.AdamW; `decay_mask`, name -> bool, defaults to
        `default_decay_mask`), an exponential moving average of the weights with the warm-up decay min(ema_decay, (1 + step) /
        (10 + step)), a guard that skips the update when the gradient norm is inf / NaN, and a learning-rate schedule (a callable
        step -> lr, the step counted from 1, evaluated on the host before each step; `linear_warmup`).  With any of them set the
        learning rate, the step count, the norm and the clip coefficient are device words: the captured step is keyed without the
        learning rate and one graph serves every step of a schedule.  `last_grad_norm` is the norm as a device scalar (reading it
        waits for the step; not reading it costs nothing), `skipped_steps` reads the guard's count from the device.  A skipped step
        still advances the step count (the bias corrections and the EMA warm-up see it), which keeps the host's and the device's
        counts equal without a read-back.  With all of them at their defaults the step is plain Adam, exactly as before.
        Data-parallel runs need nothing extra: the gradients are all-reduced before the optimiser, so every rank clips by the norm of
        the same mean gradient, takes the same decision in the guard and keeps the same average.
        deterministic: True runs the backward's reductions in their reproducible form (ops.set_deterministic: one workgroup per
        output address instead of float atomics) -- two calls on the same inputs then give the same gradient bits, at a cost in step
        time; None reads GSDD_TRAIN_DETERMINISTIC=1.  The default (False) is the fast form, whose gradients differ from run to run in
        their last bits."""
        self.dm, self.lr, self.betas, self.eps = dm, lr, betas, eps
        self.lr_schedule = lr_schedule
        self._optim_kw = dict(max_grad_norm=max_grad_norm, weight_decay=weight_decay, ema_decay=ema_decay,
                              skip_nonfinite=bool(skip_nonfinite), device_lr=lr_schedule is not None)
        self._decay_mask = decay_mask
        check_stage_args(max_grad_norm, weight_decay, ema_decay)           # now, not at the first step
        self._staged = bool(max_grad_norm is not None or float(weight_decay) > 0 or ema_decay is not None or skip_nonfinite
                            or lr_schedule is not None)
        self._in_ema = False                # inside ema_weights(): the transformer holds the averaged weights
        self.deterministic = (os.environ.get("GSDD_TRAIN_DETERMINISTIC") == "1") if deterministic is None else bool(deterministic)
        self.step_count = 0
        self.state = {}
        self.reducer = GradReducer()
        self._synced = False
        self._images = None                 # _LinearImages, from the first step on the fragment-image branch
        self._arena = None                  # GradArena, from the first loss_and_grads
        self._null32 = None                 # f32 copy of dm.empty_text_embed, from the first step that drops with learnable_cf
        self.last_fwd = self.last_drop = None
        self._adam, self._pending_adam = None, None         # MultiAdam from the first step; a state loaded before it exists
        self._graph, self._graphs = None, {}                # the captured step in use; the two most recent by key
        self._eager_steps, self._graph_failed = 0, False
        self.captures = 0                                   # how many times a step was captured (a schedule must not re-capture)

    def _sync_start(self):
        """Once, before the first data-parallel step: every rank takes rank 0's parameters and buffers (what DDP does at wrap time)."""
        if not self._synced and world_size() > 1:
            broadcast_module(self.dm)
        self._synced = True

    # ------------------------------------------------------------------ forward with saved activations
    def _forward(self, xt, cond, t, cond_len=None):
        tr = self.dm.transformer
        p = tr.packed()
        B, L = xt.shape
        D = tr.n_embd
        cond = cond.float().contiguous()
        if cond.dim() != 3 or cond.shape[0] != B:
            raise GsddError(f"the condition must be (B, Te, cond_dim) with B = {B}, got {tuple(cond.shape)}")
        Te = cond.shape[1]
        sv = {"xt": xt, "t": t, "cond": cond.reshape(B * Te, -1).contiguous(), "Te": Te, "p": p, "layers": [],     # cond: rows [B Te][cond_dim]
              "cond_len": cond_len,              # None, or int32 [B] on the device: the condition tokens each sample attends to
              "dims": (B, L, D, tr.n_head), "blocks": list(tr.blocks)}
        x = torch.empty((B * L, D), dtype=torch.float32, device=xt.device)
        ops.d3pm_embed(xt, p["emb"], p["pos"], x)
        aws = ops.d3pm_attention_workspace(B, L, tr.n_head, xt.device) if L % 32 == 0 else None     # pre-split K/V images (matrix-pipe forward)
        # the row GEMMs run on gsdd_rows_linear (weights as fragment images, refreshed once per step) when the block has the
        # north-star widths; other widths take the generic GEMM
        imgs = None
        if D == 64 and p["layers"] and p["layers"][0]["w1"].shape[0] == 256 and os.environ.get("GSDD_TRAIN_LINEAR") != "gemm":
            if self._images is None:
                self._images = _LinearImages(tr)
            imgs = self._images.refresh(cross=Te > 1)
        sv["lin"] = _RowGemm(imgs, xt.device)
        for i in range(len(p["layers"])):
            s, x = self._block_forward(i, x, sv, aws)
            sv["layers"].append(s)
        sv["x_out"] = x
        sv["statsf"], sv["hf"] = ops.ln_fwd(x, p["gf"], p["bf"])
        sv["logits"] = ops.linear(sv["hf"], p["wl"], torch.empty((B * L, p["wl"].shape[0]), dtype=torch.float32, device=xt.device),
                                  bias=p["bl"])
        return sv

    def _block_forward(self, i, x, sv, aws):
        """-> (the activations block i's backward reads, the block's output).  With more than one condition token the middle is the
        general block (transformer_utils.py:266-282): x1a = x + proj(attn1); x1 = x1a + proj2(attn2(ln1_1(x1a), cond)).  With one
        token the cross-attention softmax runs over a single key and the block adds the vector proj2(value(cond)) to every position:
        it is folded into attn1's projection (bvec), and x1a, ln1_1, q2 and k2 are neither computed nor kept."""
        lay, lin, t, flat, Te = sv["p"]["layers"][i], sv["lin"], sv["t"], sv["cond"], sv["Te"]
        (B, L, D, H), M = sv["dims"], x.shape[0]
        f = dict(dtype=torch.float32, device=x.device)
        s = {"x_in": x}
        s["stats1"], s["hn"] = ops.ln_fwd(x, lay["ada1"].view(-1), lay["ada1"].view(-1)[D:], sel=t, gstride=2 * D,
                                          rows_per_batch=L)          # AdaLayerNorm: statistics + normalised rows in one pass
        s["qkv"] = lin(i, s["hn"], "qkv", lay["wqkv"], 3 * D, head_major=True, bias=lay["bqkv"])
        s["y"], s["lse"] = torch.empty((M, D), **f), torch.empty((H * M,), **f)
        ops.d3pm_attention_train(s["qkv"][0:H], s["qkv"][H:2 * H], s["qkv"][2 * H:], B, L, H, s["y"], s["lse"], ws=aws)
        if Te > 1:
            s["x1a"] = lin(i, s["y"], "proj", lay["wproj"], D, bias=lay["bproj"], residual=x)
            ada2 = self.dm.transformer._ada2(i).view(-1)
            s["stats11"], s["hq"] = ops.ln_fwd(s["x1a"], ada2, ada2[D:], sel=t, gstride=2 * D, rows_per_batch=L)
            s["q2"] = lin(i, s["hq"], "q2", lay["wq2"], D, head_major=True, bias=lay["bq2"])
            s["k2"] = ops.small_linear(flat, lay["wk2"], lay["bk2"])
            s["v2"] = ops.small_linear(flat, lay["wv2"], lay["bv2"])
            s["y2"], s["lse2"] = torch.empty((M, D), **f), torch.empty((H * M,), **f)
            ops.d3pm_cross_attention_train(s["q2"], s["k2"], s["v2"], B, L, Te, H, s["y2"], s["lse2"], cond_len=sv["cond_len"])
            s["x1"] = lin(i, s["y2"], "proj2", lay["wproj2"], D, bias=lay["bproj2"], residual=s["x1a"])
        else:
            s["v2"] = ops.small_linear(flat, lay["wv2"], lay["bv2"])
            cvec = ops.small_linear(s["v2"], lay["wproj2"], lay["bproj2"])
            s["x1"] = lin(i, s["y"], "proj", lay["wproj"], D, bias=lay["bproj"], bvec=cvec, rows_per_batch=L, residual=x)
        s["stats2"], s["h2"] = ops.ln_fwd(s["x1"], lay["g2"], lay["b2"])
        s["a"] = lin(i, s["h2"], "w1", lay["w1"], lay["w1"].shape[0], bias=lay["bb1"])
        s["u"] = ops.gelu2(s["a"])
        return s, lin(i, s["u"], "w2", lay["w2"], D, bias=lay["bb2"], residual=s["x1"])

    # ------------------------------------------------------------------ classifier-free training: condition dropout
    def _dropout_plan(self, cond, null_cond, drop):
        """Validates the step's condition dropout on the host (no device call) -> None when the step drops nothing (cond_drop_prob == 0
        and no mask: the step then launches exactly what it launches without the feature), else (p, learnable)."""
        dm = self.dm
        from .d3pm import check_cond_drop_prob
        p = check_cond_drop_prob(getattr(dm, "cond_drop_prob", 0.0))
        if p == 0.0 and drop is None:
            return None
        if cond.dim() != 3:
            raise GsddError(f"the condition must be (B, Te, cond_dim), got {tuple(cond.shape)}")
        B, Te, cd = cond.shape
        if drop is not None and (drop.dtype not in (torch.bool, torch.uint8) or tuple(drop.shape) != (B,)):
            raise GsddError(f"the drop mask must be a bool (B,) = {(B,)} tensor, got {tuple(drop.shape)} {drop.dtype}")
        if cd % 4 != 0:
            raise GsddError(f"condition dropout needs cond_dim % 4 == 0, got {cd}")
        learnable = bool(dm.learnable_cf)
        if learnable:
            dm.check_learned_null(Te, cd)
        elif null_cond is None or Te > 77:
            dm.null_condition(Te, cd, None)                        # (raises: no null condition, or more tokens than the kernel takes)
        return p, learnable

    def _drop_condition(self, cond, plan, null_cond, drop, sid):
        """-> (condition with the dropped samples' rows replaced by the null rows, the uint8 (B,) decisions).  With learnable_cf the null
        rows are the first Te of an f32 copy of dm.empty_text_embed made here, every step: the fp64 parameter stays the single source of
        truth (load_state_dict, a torch optimiser and a resumed run need no bookkeeping)."""
        dm = self.dm
        p, learnable = plan
        B, Te, cd = cond.shape
        dev = cond.device
        if learnable:
            if self._null32 is None or self._null32.device != dev:
                self._null32 = torch.empty(tuple(dm.empty_text_embed.shape), dtype=torch.float32, device=dev)
            self._null32.copy_(dm.empty_text_embed.detach())                   # fp64 -> f32, one copy node
            rows = self._null32[:Te]
        else:
            rows = dm.null_condition(Te, cd, null_cond).to(dev)
        if drop is not None:
            drop = drop.to(dev)
            drop = (drop if drop.dtype == torch.uint8 else drop.to(torch.uint8)).contiguous()
        return ops.cond_dropout(cond, rows, p, seed=dm.noise_seed, sid=sid, row0=dm.row_offset, drop=drop)

    # ------------------------------------------------------------------ loss + gradients
    def loss_and_grads(self, *args, **kwargs):
        """`_loss_and_grads` (see there), bracketed by the reproducible-reductions switch when the trainer is `deterministic`."""
        if not self.deterministic:
            return self._loss_and_grads(*args, **kwargs)
        prev = ops.set_deterministic(True)
        try:
            return self._loss_and_grads(*args, **kwargs)
        finally:
            ops.set_deterministic(prev)

    @torch.no_grad()
    def _loss_and_grads(self, x0, cond, t=None, pt=None, want_probs=False, reduce=False, sid=None, null_cond=None, drop=None,
                        cond_len=None):
        """-> (loss tensor [1], {state_dict name: gradient}) for the transformer's parameters.  The gradients are views of one
        arena that the next call re-uses; `self.last_fwd` keeps the forward's dict (x0_recon, per_sample, probs if asked).
        reduce=True: the gradients come back averaged over the data-parallel group; the all-reduce runs in buckets of
        BUCKET_LAYERS blocks issued while the backward of the earlier blocks is still being enqueued.
        sid: int64[1] device tensor holding the Philox stream id of this step's q_sample draw (the captured step keeps it on the device);
        None: made from dm.noise_stream.
        Condition dropout (classifier-free training): with dm.cond_drop_prob = p > 0 sample b's (Te, cond_dim) condition rows are
        replaced by the null condition iff u_b < p, u_b drawn on the device from (noise_seed, global sample row, this step's stream id)
        -- `cond_drop_rows` restates it; the draw shares no counter with q_sample's, so x_t is that of the step without dropout.
        `drop`, a (B,) bool mask, overrides the draw.  The null condition is dm.empty_text_embed[:Te] with dm.learnable_cf -- the
        gradient dict then carries its gradient under "empty_text_embed", (77, 512) with rows >= Te exactly zero -- else `null_cond`,
        (Te, cond_dim) or (1, Te, cond_dim).  `self.last_drop` keeps the uint8 (B,) decisions (None: no dropout in this step).
        cond_len ((B,) integers in [1, Te]; more than one condition token): sample b's cross-attention runs over its first cond_len[b]
        condition tokens only; the rows behind them are caption padding, never read by the attention, and the attention's key / value
        gradients there are exact zeros.  Those zeros are multiplied by the padding rows in the key / value weight gradients, so the
        condition rows must be FINITE in training, padding included (a condition that comes on the host is checked).  Lengths on the
        host (a CPU tensor, a list) are validated here; an int32 tensor on the device is taken as it is, without a read back -- the
        kernels clamp it into [1, Te].  A dropped sample takes the null rows and length Te: the null condition is full length."""
        cond_len = self._check_lengths(cond, cond_len)
        plan = self._dropout_plan(cond, null_cond, drop)
        self._sync_start()
        if not x0.is_cuda:
            raise GsddError("the HIP path needs tensors on a ROCm device (no CPU fallback)")
        tr = self.dm.transformer
        x0, xt, cond, t, pt, cond_len = self._prepare(x0, cond, t, pt, sid, plan, null_cond, drop, cond_len)
        sv = self._forward(xt, cond, t, cond_len)
        fwd, dlogits = self._loss(sv, x0, pt, want_probs)
        if self._arena is None:
            self._arena = GradArena(x0.device)
        book = GradBook(self._arena, self.reducer if (reduce and self.reducer.active()) else None)
        dx = self._head_backward(sv, dlogits, book)
        del dlogits
        B, L = x0.shape
        bws = ops.d3pm_attention_bwd_workspace(B, L, tr.n_head, dx.device) if L % 32 == 0 else None     # operand images (matrix-pipe backward)
        cws = ops.d3pm_cross_attention_bwd_workspace(B, L, sv["Te"], tr.n_head, dx.device) if sv["Te"] > 1 else None  # delta + the dK / dV partials
        # the learned null embedding's gradient: every block leaves its (dk2, dv2, Wk2, Wv2) here; the sums over the dropped samples
        # are formed after the last block, into the arena's last gradient (a bucket that is already out must not be written again)
        null_terms = [] if (plan is not None and plan[1]) else None
        n = len(sv["layers"])
        for i in reversed(range(n)):
            dx = self._block_backward(i, sv, dx, book, bws, cws, null_terms)
            if (n - i) % BUCKET_LAYERS == 0:
                book.bucket()
        self._embed_backward(sv, dx, book)
        names = (nm for nm, _ in tr.named_parameters())           # (a generator: the walk over the parameters is paid only with a reducer)
        if null_terms is not None:
            # (77, 512) f32, one gsdd_cond_null_grad call per block onto rows [:Te] in the backward's block order (a fixed order: the
            # same bits every run); rows >= Te keep the arena's zero fill
            gnull = book.zeros(self.NULL_NAME, self._null32)
            for dk2, dv2, wk2, wv2 in null_terms:
                ops.cond_null_grad(dk2, dv2, self.last_drop, wk2, wv2, B, sv["Te"], gnull[:sv["Te"]])
            names = itertools.chain(names, [self.NULL_NAME])
        return fwd["loss"], book.finish(names)

    def _check_lengths(self, cond, cond_len):
        """The step's condition lengths -> None (no lengths, or one condition token: nothing to mask) or an int32 (B,) tensor, on the
        device as given or validated on the host (`check_condition_len`)."""
        if cond_len is None:
            return None
        if cond.dim() != 3:
            raise GsddError(f"the condition must be (B, Te, cond_dim), got {tuple(cond.shape)}")
        B, Te = cond.shape[:2]
        if not cond.is_cuda and not bool(torch.isfinite(cond).all()):
            raise GsddError("cond_len: the condition holds inf / NaN; in training every condition row must be finite, padding included "
                            "(the zero key / value gradients of the padding are multiplied by those rows)")
        if torch.is_tensor(cond_len) and cond_len.is_cuda and cond_len.dtype == torch.int32 and tuple(cond_len.shape) == (B,) and Te > 1:
            return cond_len.contiguous()
        from .d3pm import check_condition_len
        cond_len = check_condition_len(cond_len, B, Te, "cond_len")
        return cond_len if Te > 1 else None

    def _prepare(self, x0, cond, t, pt, sid, plan, null_cond, drop, cond_len=None):
        """-> (x0, x_t, condition, t, p(t), condition lengths) on the device: the weights re-packed if they changed, timesteps drawn if
        none were given, x_t drawn by q_sample on this step's Philox stream, the condition with its dropped samples substituted (and
        their lengths set to Te)."""
        dm = self.dm
        dm.transformer.packed()
        B, L = x0.shape
        K, T = dm.num_classes - 1, dm.num_timesteps
        dev = x0.device
        if t is None:
            t, pt = dm.sample_time(B, dev, "importance")
        t, pt = t.to(dev).long().contiguous(), pt.to(dev).float().contiguous()
        if sid is None:
            sid = torch.tensor([dm.noise_stream], dtype=torch.int64, device=dev)
        dm.noise_stream += 1
        x0 = x0.contiguous().long()
        xt = torch.empty_like(x0)
        ops.d3pm_q_sample(x0, xt, dm._sched(), t, sid, K=K, T=T, seed=dm.noise_seed, row0=dm.row_offset * L)
        self.last_drop = None
        if plan is not None:          # the substituted condition is what the forward, every saved activation and every gradient see
            cond, self.last_drop = self._drop_condition(cond.to(dev).float().contiguous(), plan, null_cond, drop, sid)
        if cond_len is not None:
            cond_len = cond_len.to(dev)
            if plan is not None:      # a dropped sample attends to all Te null rows (formed on the device: the decisions live there)
                cond_len = torch.where(self.last_drop != 0, torch.full_like(cond_len, cond.shape[1]), cond_len)
        return x0, xt, cond, t, pt, cond_len

    def _loss(self, sv, x0, pt, want_probs):
        """-> (the forward's dict, kept as `self.last_fwd`; d loss / d logits)"""
        dm, xt, t, sched = self.dm, sv["xt"], sv["t"], self.dm._sched()
        kw = dict(K=dm.num_classes - 1, T=dm.num_timesteps, mask_weight=dm.mask_weight, aux_weight=dm.auxiliary_loss_weight,
                  adaptive_aux=dm.adaptive_auxiliary_loss)
        if want_probs or os.environ.get("GSDD_TRAIN_LOSS_SPLIT"):      # (the switch: A/B and the equality test of the two paths)
            fwd = ops.d3pm_train_loss(sv["logits"], x0, xt, t, pt, sched, dm.Lt_history, dm.Lt_count, want_probs=want_probs, **kw)
            dlogits = ops.d3pm_train_loss_bwd(sv["logits"], x0, xt, t, pt, sched, **kw)
        else:                                                          # one pass over the logits for the loss and its gradient
            fwd, dlogits = ops.d3pm_train_loss_grad(sv["logits"], x0, xt, t, pt, sched, dm.Lt_history, dm.Lt_count, **kw)
        fwd["t"], fwd["xt"] = t, xt
        self.last_fwd = fwd
        return fwd, dlogits

    def _head_backward(self, sv, dlogits, book):
        """to_logits (final LayerNorm + the class projection) -> d loss / d (the last block's output); the head's gradients are the
        first bucket"""
        p, z = sv["p"], book.zeros
        D = self.dm.transformer.n_embd
        ops.wgrad(dlogits, sv["hf"], z("to_logits.1.weight", p["wl"]), z("to_logits.1.bias", p["bl"]))
        dhf = ops.linear(dlogits, p["wl"].t().contiguous(), torch.empty((dlogits.shape[0], D), dtype=torch.float32, device=dlogits.device))
        dx = ops.ln_bwd(dhf, sv["x_out"], sv["statsf"], p["gf"], dgamma=z("to_logits.0.weight", p["gf"]),
                        dbeta=z("to_logits.0.bias", p["bf"]), gacc_stride=D)
        book.bucket()
        return dx

    def _block_backward(self, i, sv, dx, book, bws, cws, null_terms):
        """d loss / d (block i's output) -> d loss / d (its input); the block's gradients go into the book"""
        lay, s, blk, lin, t = sv["p"]["layers"][i], sv["layers"][i], sv["blocks"][i], sv["lin"], sv["t"]
        B, L, D, H = sv["dims"]
        pre, z = f"blocks.{i}.", book.zeros
        # ---- MLP
        ops.wgrad(dx, s["u"], z(pre + "mlp.2.weight", lay["w2"]), z(pre + "mlp.2.bias", lay["bb2"]))
        du = lin.t(i, dx, "w2", lay["w2"], s["u"].shape[1])
        da = ops.gelu2(s["a"], du)
        ops.wgrad(da, s["h2"], z(pre + "mlp.0.weight", lay["w1"]), z(pre + "mlp.0.bias", lay["bb1"]))
        dh2 = lin.t(i, da, "w1", lay["w1"], D)
        dx1 = ops.ln_bwd(dh2, s["x1"], s["stats2"], lay["g2"], dx_in=dx, dgamma=z(pre + "ln2.weight", lay["g2"]),
                         dbeta=z(pre + "ln2.bias", lay["b2"]), gacc_stride=D)
        # ---- the condition: cross-attention over its tokens, or the broadcast vector; attn1's output projection
        if sv["Te"] > 1:
            dx1 = self._cross_attention_backward(i, sv, dx1, book, cws, null_terms)
        else:
            self._condition_vector_backward(i, sv, dx1, book, null_terms)
        dy = lin.t(i, dx1, "proj", lay["wproj"], D)
        # ---- self-attention
        qkv = s["qkv"]
        dqkv = ops.d3pm_attention_bwd(qkv[0:H], qkv[H:2 * H], qkv[2 * H:], s["y"], dy, s["lse"], B, L, H, ws=bws)
        wq, bq = book.scratch(lay["wqkv"].shape), book.scratch(lay["bqkv"].shape)
        ops.wgrad(dqkv, s["hn"], wq, bq)
        for j, nm in enumerate(("query", "key", "value")):        # row blocks of the fused gradient: views, already contiguous
            book.g[pre + f"attn1.{nm}.weight"] = wq[j * D:(j + 1) * D]
            book.g[pre + f"attn1.{nm}.bias"] = bq[j * D:(j + 1) * D]
        dhn = lin.t(i, dqkv, "qkv", lay["wqkv"], D)
        dtab = torch.zeros((B, 2 * D), dtype=torch.float32, device=dx.device)      # (not in the arena: the arena's size must not depend on the batch size)
        dx = ops.ln_bwd(dhn, s["x_in"], s["stats1"], lay["ada1"].view(-1), sel=t, gstride=2 * D, rows_per_batch=L,
                        dx_in=dx1, dgamma=dtab, dbeta=dtab.view(-1)[D:], gacc_stride=2 * D, acc_by_batch=True)
        ops.adaln_bwd(dtab, t, blk.ln1.emb.weight.contiguous(), blk.ln1.linear.weight.contiguous(),
                      z(pre + "ln1.emb.weight", blk.ln1.emb.weight), z(pre + "ln1.linear.weight", blk.ln1.linear.weight),
                      z(pre + "ln1.linear.bias", blk.ln1.linear.bias))
        return dx

    def _cross_attention_backward(self, i, sv, dx1, book, cws, null_terms):
        """More than one condition token: attn2's projection, the attention, its query, ln1_1; keys / values against the condition
        rows; attn1.proj's weight gradient -> d loss / d x1a"""
        lay, s, blk, lin, t = sv["p"]["layers"][i], sv["layers"][i], sv["blocks"][i], sv["lin"], sv["t"]
        (B, L, D, H), Te = sv["dims"], sv["Te"]
        pre, z = f"blocks.{i}.", book.zeros
        ops.wgrad(dx1, s["y2"], z(pre + "attn2.proj.weight", lay["wproj2"]), z(pre + "attn2.proj.bias", lay["bproj2"]))
        dy2 = lin.t(i, dx1, "proj2", lay["wproj2"], D)
        # (with condition lengths the dk2 / dv2 rows of the padding are exact zeros: they add nothing to the key / value weight gradients
        # below as long as the condition rows there are finite)
        dq2, dk2, dv2 = ops.d3pm_cross_attention_bwd(s["q2"], s["k2"], s["v2"], s["y2"], dy2, s["lse2"], B, L, Te, H, cws,
                                                     cond_len=sv["cond_len"])
        dq2 = dq2.permute(1, 0, 2).reshape(B * L, D).contiguous()          # head-major -> rows, the layout wgrad and the row GEMMs take
        ops.wgrad(dq2, s["hq"], z(pre + "attn2.query.weight", lay["wq2"]), z(pre + "attn2.query.bias", lay["bq2"]))
        dhq = lin.t(i, dq2, "q2", lay["wq2"], D)
        ada2 = self.dm.transformer._ada2(i).view(-1)
        dtab2 = torch.zeros((B, 2 * D), dtype=torch.float32, device=dx1.device)
        dx1 = ops.ln_bwd(dhq, s["x1a"], s["stats11"], ada2, sel=t, gstride=2 * D, rows_per_batch=L, dx_in=dx1, dgamma=dtab2,
                         dbeta=dtab2.view(-1)[D:], gacc_stride=2 * D, acc_by_batch=True)
        ops.adaln_bwd(dtab2, t, blk.ln1_1.emb.weight.contiguous(), blk.ln1_1.linear.weight.contiguous(),
                      z(pre + "ln1_1.emb.weight", blk.ln1_1.emb.weight), z(pre + "ln1_1.linear.weight", blk.ln1_1.linear.weight),
                      z(pre + "ln1_1.linear.bias", blk.ln1_1.linear.bias))
        ops.small_linear_bwd(dk2, sv["cond"], lay["wk2"], z(pre + "attn2.key.weight", lay["wk2"]),
                             z(pre + "attn2.key.bias", lay["bk2"]), want_dx=False)
        ops.small_linear_bwd(dv2, sv["cond"], lay["wv2"], z(pre + "attn2.value.weight", lay["wv2"]),
                             z(pre + "attn2.value.bias", lay["bv2"]), want_dx=False)
        if null_terms is not None:
            null_terms.append((dk2, dv2, lay["wk2"], lay["wv2"]))
        ops.wgrad(dx1, s["y"], z(pre + "attn1.proj.weight", lay["wproj"]), z(pre + "attn1.proj.bias", lay["bproj"]))
        return dx1

    def _condition_vector_backward(self, i, sv, dx1, book, null_terms):
        """One condition token: attn1.proj's weight gradient, then the broadcast vector proj2(value(cond)) -- the sum of dx1 over a
        sample's rows through attn2.proj and attn2.value.  The softmax over a single key gives attn2.query, attn2.key and ln1_1
        exactly zero gradient: they are requested and left at the arena's fill."""
        lay, s, blk = sv["p"]["layers"][i], sv["layers"][i], sv["blocks"][i]
        pre, z = f"blocks.{i}.", book.zeros
        ops.wgrad(dx1, s["y"], z(pre + "attn1.proj.weight", lay["wproj"]), z(pre + "attn1.proj.bias", lay["bproj"]))
        dcvec = ops.batch_rowsum(dx1, *sv["dims"][:2])
        dv2 = ops.small_linear_bwd(dcvec, s["v2"], lay["wproj2"], z(pre + "attn2.proj.weight", lay["wproj2"]),
                                   z(pre + "attn2.proj.bias", lay["bproj2"]))
        ops.small_linear_bwd(dv2, sv["cond"], lay["wv2"], z(pre + "attn2.value.weight", lay["wv2"]),
                             z(pre + "attn2.value.bias", lay["bv2"]), want_dx=False)
        if null_terms is not None:          # no key term
            null_terms.append((None, dv2, None, lay["wv2"]))
        for nm, ref in (("attn2.key.weight", lay["wk2"]), ("attn2.key.bias", lay["bk2"]),
                        ("attn2.query.weight", lay["wq2"]), ("attn2.query.bias", lay["bq2"]),
                        ("ln1_1.emb.weight", blk.ln1_1.emb.weight), ("ln1_1.linear.weight", blk.ln1_1.linear.weight),
                        ("ln1_1.linear.bias", blk.ln1_1.linear.bias)):
            z(pre + nm, ref)

    def _embed_backward(self, sv, dx, book):
        """token and position embeddings; the (Hs Ws, D) position gradient and the width sum are arena scratch"""
        ce = self.dm.transformer.content_emb
        Hs, Ws = ce.spatial_size
        D = dx.shape[1]
        dpos = book.scratch((Hs * Ws, D))
        ops.d3pm_embed_bwd(dx, sv["xt"], book.zeros("content_emb.emb.weight", ce.emb.weight), dpos)
        ops.batch_rowsum(dpos, Hs, Ws, out=book.zeros("content_emb.height_emb.weight", ce.height_emb.weight))
        dw_ = book.scratch((Ws * D,))
        ops.colsum(dpos.view(Hs, Ws * D), dw_)
        book.g["content_emb.width_emb.weight"] = dw_.view(Ws, D)

    # ------------------------------------------------------------------ the step as one captured graph
    def _graph_usable(self, x0, cond):
        """Single-process steps only: with a data-parallel group the bucketed all-reduces run between the backward's launches through
        torch.distributed, outside any capture (the eager path; its launch gaps are covered by the collectives' own latency)."""
        return (os.environ.get("GSDD_TRAIN_GRAPH", "1") != "0" and not self._graph_failed and x0.is_cuda
                and not self.reducer.active() and world_size() == 1 and x0.shape[1] % 32 == 0)

    def _capture(self, x0, cond, null_cond=None, drop=None, cond_len=None):
        """Everything of a step that runs on the device -- re-pack of the weight images and AdaLN tables, q_sample, forward, loss +
        gradient, backward, Adam -- recorded once into a hipGraph and replayed: ~1000 small dependent launches leave ~2 ms of gaps per
        step when they are enqueued one by one.  Nothing step-dependent is baked in: x_0, condition, t, p(t) live in static buffers,
        the Philox stream id and Adam's step count are device words the host sets before each replay; the timesteps are drawn
        by DiffusionTransformer.sample_time before each replay, exactly as the eager step draws them.  torch's graph-private
        allocator pool keeps every activation of the captured step at its address (torch.cuda.graph is the plumbing; every node of
        the graph is a libgsdd kernel or a fill / copy).
        Condition dropout: the f32 copy of the learned null embedding, the dropout kernel (its draw reads the stream id's device word),
        the null gradient and the copy of the updated rows back into the fp64 parameter are nodes too; an explicit mask and a caller's
        null condition live in static buffers like x_0.
        Condition lengths live in a static int32 (B,) buffer that every replay refreshes; the dropped samples' length Te is formed
        from the dropout decisions inside the graph."""
        dm, dev = self.dm, x0.device
        B = x0.shape[0]
        st = {"shape": (tuple(x0.shape), tuple(cond.shape)), "lr": None if self._staged else self.lr,      # (staged: lr is a device word)
              "x0": x0.clone().long().contiguous(), "cond": cond.clone().float().contiguous(),
              "t": torch.zeros((B,), dtype=torch.int64, device=dev), "pt": torch.full((B,), 1.0 / dm.num_timesteps, dtype=torch.float32, device=dev),
              "sid": torch.tensor([dm.noise_stream], dtype=torch.int64, device=dev),
              "adam_step": torch.tensor([self._adam.step_count + 1], dtype=torch.int64, device=dev),
              "drop": None if drop is None else drop.to(dev).to(torch.uint8).contiguous().clone(),
              "null": None if null_cond is None else null_cond.to(dev).float().contiguous().clone(),
              "len": None if cond_len is None else cond_len.to(dev).to(torch.int32).contiguous().clone()}
        tr = dm.transformer
        keep = (dm.noise_stream, self._adam.step_count)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tr._packed = None                                    # the re-pack is part of the graph: every replay sees the current weights
            loss, grads = self.loss_and_grads(st["x0"], st["cond"], st["t"], st["pt"], reduce=False, sid=st["sid"], null_cond=st["null"],
                                              drop=st["drop"], cond_len=st["len"])
            self._adam.lr = self.lr
            # (staged: step and lr are words of the optimiser's state block, written before each replay; the stage's launches are
            # the same nodes here as in the launch-by-launch step)
            self._adam.step(grads, step_dev=st["adam_step"], write_words=False)
            self._write_back_null(grads, cond.shape[1])
        dm.noise_stream, self._adam.step_count = keep             # capture executed nothing
        self.captures += 1
        st["graph"], st["loss"], st["packed"] = graph, loss, tr._packed
        st["pins"] = self._pins()
        tr._packed = None
        return st

    def _pins(self):
        """name -> tensor: everything outside a captured step's own pool that its graph replays on and that the trainer reaches only
        through an attribute it may re-assign -- the gradient arena, Adam's address table, moments, averages, state block and partial
        sums, the weight images with their descriptor table, the f32 null embedding.  Taken right after the capture and kept in the
        graph's `st`: a later step that outgrows the arena, rebuilds a table or adds the cross-attention images then replaces the
        trainer's attribute only, and the graph goes on replaying on buffers it owns.  (The parameters and the schedule buffers belong
        to the module.)"""
        a, im = self._adam, self._images
        pins = {"arena.buf": self._arena.buf, "adam.table": a._table, "adam.m": a.m, "adam.v": a.v, "adam.ema": a.ema,
                "adam.words": a.words, "adam.partials": a.partials, "null32": self._null32}
        if im is not None and im.ptrs is not None:
            pins["images.buf"], pins["images.table"] = im.buf, im.table
        return {k: v for k, v in pins.items() if v is not None}

    @torch.no_grad()
    def step(self, x0, cond, t=None, pt=None, null_cond=None, drop=None, cond_len=None):
        """One optimiser step.  null_cond / drop: the null condition and the explicit drop mask of condition dropout (loss_and_grads);
        cond_len: the per-sample condition lengths (loss_and_grads).
        With dm.learnable_cf the learned null embedding is updated with the transformer's parameters: its f32 copy and its gradient go
        through the same Adam launch, and rows [:Te] of the updated copy are written back into the fp64 parameter."""
        if self._in_ema:
            raise GsddError("D3PMTrainer.step inside ema_weights(): the transformer holds the averaged weights")
        if self.lr_schedule is not None:
            self.lr = float(self.lr_schedule(self._next_step()))
        self._sync_start()
        cond_len = self._check_lengths(cond, cond_len)
        if self._graph_usable(x0, cond):
            return self._step_graphed(x0, cond, t, pt, null_cond, drop, cond_len)
        return self._step_eager(x0, cond, t, pt, null_cond, drop, cond_len)

    def _write_back_null(self, grads, Te):
        """After Adam: rows [:Te] of the updated f32 copy go back into dm.empty_text_embed (f32 -> fp64, one copy node).  The rows
        beyond Te have an exactly zero gradient and keep their fp64 values."""
        if self.NULL_NAME in grads:
            self.dm.empty_text_embed.data[:Te].copy_(self._null32[:Te])

    def _step_graphed(self, x0, cond, t, pt, null_cond=None, drop=None, cond_len=None):
        """Two eager steps first (arenas, images and tables reach their final addresses), then capture, then replays."""
        # one captured graph per (batch shape, learning rate), the two most recent kept: an epoch's short last batch must not make
        # every epoch capture twice (each graph owns its activations' pool: ~7 GB at bs 16, L = 4096)
        graphs = self._graphs
        # ... and per condition-dropout setting: the probability is a launch constant of the dropout kernel, and the learned null
        # embedding, a mask and a caller's null condition each change the graph's nodes
        # (with the optimiser stage the learning rate is a device word and not part of the key: one graph serves a whole schedule)
        key = (tuple(x0.shape), tuple(cond.shape), None if self._staged else float(self.lr), float(getattr(self.dm, "cond_drop_prob", 0.0) or 0.0),
               bool(self.dm.learnable_cf), drop is not None, null_cond is not None, self.deterministic, cond_len is not None)
        st = self._graph = graphs.get(key)
        if st is None and self._eager_steps < 2:
            self._eager_steps += 1
            return self._step_eager(x0, cond, t, pt, null_cond, drop, cond_len)
        dm = self.dm
        if st is None:
            keep = (dm.noise_stream, self._adam.step_count)
            try:
                st = self._graph = self._capture(x0, cond, null_cond, drop, cond_len)
                while len(graphs) >= 2:
                    graphs.pop(next(iter(graphs)))
                graphs[key] = st
            except Exception as e:                                # noqa: BLE001  (a capture that cannot be made must not cost the step)
                warnings.warn(f"D3PMTrainer: the training step could not be captured as a graph ({type(e).__name__}: {e}); running launch by launch")
                dm.noise_stream, self._adam.step_count = keep
                self._graph_failed = True
                dm.transformer._packed = None
                torch.cuda.synchronize()
                return self._step_eager(x0, cond, t, pt, null_cond, drop, cond_len)
        if t is None:
            # the reference's own timestep sampler (importance sampling once every Lt_count exceeds 10: its check reads device memory,
            # i.e. waits for the previous step -- one host round trip per step, ~0.1 ms beside a 54 ms replay)
            t, pt = dm.sample_time(x0.shape[0], x0.device, "importance")
        st["x0"].copy_(x0, non_blocking=True)
        st["cond"].copy_(cond, non_blocking=True)
        st["t"].copy_(t, non_blocking=True)
        st["pt"].copy_(pt, non_blocking=True)
        if drop is not None:
            st["drop"].copy_(drop, non_blocking=True)
        if null_cond is not None:
            st["null"].copy_(null_cond.reshape(st["null"].shape), non_blocking=True)
        if cond_len is not None:
            st["len"].copy_(cond_len, non_blocking=True)
        # the two device words are set from the host's counts before every replay (two fills): whoever else draws from the noise stream
        # between steps -- the validation loop's _train_loss, set_noise, a resumed checkpoint -- moves dm.noise_stream, and the replay
        # must use the stream id the eager step would
        st["sid"].fill_(dm.noise_stream)
        st["adam_step"].fill_(self._adam.step_count + 1)
        if self._staged:
            self._adam.write_step_words(self._adam.step_count + 1, self.lr)
        st["graph"].replay()
        dm.noise_stream += 1
        self._adam.step_count += 1
        self.step_count += 1
        dm.transformer._packed = None                            # the packed views any eager caller holds predate this update
        self.last_fwd = None
        return st["loss"].clone()

    def _step_eager(self, x0, cond, t=None, pt=None, null_cond=None, drop=None, cond_len=None):
        loss, grads = self.loss_and_grads(x0, cond, t, pt, reduce=True, null_cond=null_cond, drop=drop, cond_len=cond_len)
        tr = self.dm.transformer
        params = dict(tr.named_parameters())
        self.step_count += 1
        learned = self.NULL_NAME in grads
        if self._adam is None:
            # the learned null embedding joins the parameter list (last) as its f32 copy: one Adam launch updates everything, and
            # optimizer_state() / load_optimizer_state() carry its moments with the rest
            plist = list(params.items()) + ([(self.NULL_NAME, self._null32)] if learned else [])
            kw = {}
            if self._staged:
                mask = self._decay_mask if self._decay_mask is not None else default_decay_mask(tr, (self.NULL_NAME,))
                kw = dict(self._optim_kw, decay_mask=mask)
            self._adam = MultiAdam(plist, self.lr, self.betas, self.eps, **kw)
            self._adam.load_state(self._pending_adam)
            self._pending_adam = None
        if learned != (self._adam.params[-1][0] == self.NULL_NAME):
            raise GsddError("this trainer's optimiser state was laid out " + ("without" if learned else "with") + " the learned null "
                            "embedding: condition dropout with learnable_cf must be on for every step of a trainer or for none "
                            "(make a new D3PMTrainer to change it)")
        self._adam.lr = self.lr
        self._adam.step(grads)                  # all parameters in one launch
        self._write_back_null(grads, cond.shape[1])
        tr._packed = None                       # parameters changed in place through raw pointers
        return loss

    # ------------------------------------------------------------------ the optimiser stage's accessors; the averaged weights
    def _next_step(self):
        """the count (from 1) of the coming optimiser step, a resumed state's steps included"""
        if self._adam is not None:
            return self._adam.step_count + 1
        return int((self._pending_adam or {}).get("step", 0)) + 1

    @property
    def last_grad_norm(self):
        """The last step's global gradient norm (before clipping) as a device scalar; None before the first step or when neither
        clipping nor the non-finite guard is on.  Reading its value waits for the step; not reading it costs nothing."""
        if self._adam is None or not (self._optim_kw["max_grad_norm"] is not None or self._optim_kw["skip_nonfinite"]):
            return None
        return self._adam.grad_norm

    @property
    def skipped_steps(self):
        """how many updates the non-finite guard has skipped, read from the device on request"""
        if self._adam is None:
            return int((self._pending_adam or {}).get("skipped_steps", 0))
        return self._adam.skipped_steps

    @property
    def has_ema(self):
        return self._optim_kw["ema_decay"] is not None

    def _drop_weight_caches(self):
        """everything derived from the transformer's weights that does not notice a write through raw pointers: the packed views with
        their AdaLN tables and the sampler's fragment images (all inside `_packed`).  The trainer's `_LinearImages` are re-packed by
        every forward, a captured step re-packs inside its graph."""
        self.dm.transformer._packed = None
        self.last_fwd = None

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the transformer (and, with a learned null embedding, dm.empty_text_embed) holds the averaged weights:
        one gsdd_swap_multi exchanges parameters and averages in place, a second one on exit puts both back, bit for bit.  Before the
        first optimiser step the average IS the parameters and nothing is exchanged.  Nesting, or a training step inside the
        context, raises GsddError."""
        if not self.has_ema:
            raise GsddError("ema_weights(): this trainer keeps no averaged weights (ema_decay is None)")
        if self._in_ema:
            raise GsddError("ema_weights() is already active: the context does not nest")
        adam = self._adam if (self._adam is not None and self._adam.ema is not None) else None
        null_live = None
        self._in_ema = True
        try:
            if adam is not None:
                learned = adam.params[-1][0] == self.NULL_NAME
                if learned:            # the f32 copy is exchanged with the rest; the fp64 parameter takes the averaged rows for the duration
                    null_live = self.dm.empty_text_embed.data.clone()
                adam.swap_ema()
                if learned:
                    self.dm.empty_text_embed.data.copy_(self._null32)
                self._drop_weight_caches()
            yield self
        finally:
            if adam is not None:
                adam.swap_ema()
                if null_live is not None:
                    self.dm.empty_text_embed.data.copy_(null_live)
                self._drop_weight_caches()
            self._in_ema = False

    def ema_state_dict(self):
        """The averaged weights under the transformer's state_dict keys, CPU tensors (buffers, if any, as they are):
        transformer.load_state_dict and load_reference_checkpoint take them.  Before the first step: the current weights."""
        if not self.has_ema:
            raise GsddError("ema_state_dict(): this trainer keeps no averaged weights (ema_decay is None)")
        tr = self.dm.transformer
        sd = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
        if self._adam is not None and self._adam.ema is not None:
            if self._in_ema:
                raise GsddError("ema_state_dict() inside ema_weights(): the average and the weights are exchanged")
            for name, t in self._adam.ema_tensors().items():
                if name != self.NULL_NAME:
                    sd[name] = t.cpu()
        return sd

    def ema_null_embedding(self):
        """the averaged learned null embedding, (77, 512) fp64 on the CPU (rows the training never reached keep the parameter's
        values), or None when the optimiser does not carry it"""
        a = self._adam
        if a is None or a.ema is None or a.params[-1][0] != self.NULL_NAME:
            return None
        return a.ema_tensors()[self.NULL_NAME].double().cpu()

    # ------------------------------------------------------------------ optimiser state for checkpoints (exact resume)
    def optimizer_state(self):
        """m, v, the step count and -- with the optimiser stage -- the averaged weights (`ema`) and the guard's `skipped_steps`"""
        if self._in_ema:
            raise GsddError("optimizer_state() inside ema_weights(): the average and the weights are exchanged")
        return self._adam.state() if self._adam is not None else self._pending_adam

    def load_optimizer_state(self, state):
        self._graph, self._graphs = None, {}                    # (captured steps bake the addresses of the Adam state they were made with)
        if state is None:
            return
        if self._adam is not None:
            self._adam.load_state(state)
        else:
            self._pending_adam = state


class _TrainForward(torch.autograd.Function):
    """Bridges the HIP training objective into torch.autograd so that the reference's stage-2 loop (zero_grad, manual_backward(loss),
    optimizer.step(): multistage_text_motion_model.py:186-197) runs unchanged: forward evaluates loss and gradients on the HIP path
    (one fused pass: the activations never outlive it), backward hands each transformer parameter its gradient scaled by the
    incoming d(loss)."""

    @staticmethod
    def forward(ctx, trainer, x0, cond, want_probs, null_cond, drop, cond_len, *params):
        loss, grads = trainer.loss_and_grads(x0, cond, want_probs=want_probs, reduce=True, null_cond=null_cond, drop=drop,
                                             cond_len=cond_len)    # DDP semantics: .grad = group mean
        names = [n for n, _ in trainer.dm.transformer.named_parameters()]
        ctx.grads = [grads[n].clone() for n in names]          # the arena is re-used by the next forward
        if len(params) > len(names):                           # dm.empty_text_embed, the last input: its gradient widened to the parameter's fp64
            ctx.grads.append(grads[trainer.NULL_NAME].double())
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g_loss):
        out = tuple(g * g_loss for g in ctx.grads)
        ctx.grads = None
        return (None, None, None, None, None, None, None) + out


def train_forward(dm, x0, cond, want_probs=False, null_cond=None, drop=None, cond_len=None):
    """DiffusionTransformer.forward in train mode with autograd enabled -> (loss with grad_fn, forward dict).  With condition dropout
    and dm.learnable_cf, dm.empty_text_embed is an input of the autograd node too: backward leaves its (77, 512) fp64 gradient in .grad,
    and the caller's optimiser over generator.parameters() updates it like any other parameter.  cond_len: the per-sample condition
    lengths (D3PMTrainer.loss_and_grads)."""
    tr = getattr(dm, "_hip_trainer", None)
    if tr is None:
        tr = D3PMTrainer(dm)
        object.__setattr__(dm, "_hip_trainer", tr)
    params = [p for _, p in dm.transformer.named_parameters()]
    if dm.learnable_cf and tr._dropout_plan(cond, null_cond, drop) is not None:
        params.append(dm.empty_text_embed)
    loss = _TrainForward.apply(tr, x0, cond, want_probs, null_cond, drop, cond_len, *params)
    return loss, tr.last_fwd
