"""Tensor-level wrappers over the C ABI (include/gsdd.h).  torch is used only to own device memory
and streams; every computation below is a HIP kernel in libgsdd.so."""
import ctypes as C
import os

import torch

from . import _lib as abi
from ._lib import ComposeDesc, GemmDesc, GsddError, JumpDesc, LayerDesc, PurityDesc, PuritySelectDesc, StepDesc, TrainDesc, _is_int, check, lib, ptr, stream_ptr

ACT_NONE, ACT_RELU, ACT_GELU2 = 0, 1, 2


# ----------------------------------------------------------------------------- variant / precision selection
# The C ABI takes the arithmetic mode / kernel variant as an argument of each call (include/gsdd.h); libgsdd.so reads no environment.
# The debugging switches the tests and the A/B tools have always used are environment variables: they are translated HERE, per call, into
# those arguments (an explicit keyword argument of the wrapper wins over the environment).
_ATTN_MODES = {"auto": abi.ATTN_AUTO, "22": abi.ATTN_P22, "11": abi.ATTN_P11, "a8": abi.ATTN_A8, "a12": abi.ATTN_A12,
               "f32pv": abi.ATTN_F32PV, "kc256": abi.ATTN_KC256}
_LAYER_VARIANTS = {"auto": abi.LAYER_AUTO, "h2": abi.LAYER_H2, "x3p": abi.LAYER_X3P}
_ATTN_BWD_VARIANTS = {"auto": abi.ATTN_BWD_AUTO, "valu": abi.ATTN_BWD_VALU, "split": abi.ATTN_BWD_SPLIT, "fqc64": abi.ATTN_BWD_FQC64,
                      "fqc128": abi.ATTN_BWD_FQC128, "nw8": abi.ATTN_BWD_NW8, "dbg1": abi.ATTN_BWD_DBG1, "dbg2": abi.ATTN_BWD_DBG2}


def _pick(table, value, what):
    if isinstance(value, int):
        return value
    try:
        return table[str(value).lower()]
    except KeyError:
        raise GsddError(f"{what}: {value!r} is not one of {sorted(table)}") from None


def attn_mode(mode=None):
    """GSDD_ATTN_P = 22 | 11 | a8 | a12 (the sampler's P format), GSDD_ATTN_V3=1 (exact-f32 P.V kernel), GSDD_ATTN_KC=256."""
    if mode is not None:
        return _pick(_ATTN_MODES, mode, "attention mode")
    if os.environ.get("GSDD_ATTN_V3"):
        return abi.ATTN_F32PV
    if os.environ.get("GSDD_ATTN_KC") == "256":
        return abi.ATTN_KC256
    return _pick(_ATTN_MODES, os.environ.get("GSDD_ATTN_P", "auto"), "GSDD_ATTN_P")


def attn_train_mode(mode=None):
    """GSDD_ATTN_TRAIN_P = 22 | a8 (explicit values only; anything else is an error)."""
    v = mode if mode is not None else os.environ.get("GSDD_ATTN_TRAIN_P", "auto")
    m = _pick(_ATTN_MODES, v, "GSDD_ATTN_TRAIN_P")
    if m not in (abi.ATTN_AUTO, abi.ATTN_P22, abi.ATTN_A8):
        raise GsddError(f"GSDD_ATTN_TRAIN_P: {v!r} is not one of '22', 'a8'")
    return m


def attn_lean_flag():
    """GSDD_ATTN_LEAN=0: every wave of the adaptive attention kernels takes the general chunk loop (OR-ed into the mode argument)."""
    v = os.environ.get("GSDD_ATTN_LEAN", "1")
    if v not in ("0", "1"):
        raise GsddError(f"GSDD_ATTN_LEAN: {v!r} is not one of '0', '1'")
    return abi.ATTN_NOLEAN if v == "0" else 0


def attn_bwd_variant(variant=None):
    """GSDD_ATTN_BWD = valu | split | fqc64 | fqc128 | nw8 | dbg1 | dbg2 (development variants of the attention backward)."""
    return _pick(_ATTN_BWD_VARIANTS, variant if variant is not None else os.environ.get("GSDD_ATTN_BWD", "auto"), "GSDD_ATTN_BWD")


def layer_variant(variant=None):
    """GSDD_LAYER = h2 | x3p."""
    return _pick(_LAYER_VARIANTS, variant if variant is not None else os.environ.get("GSDD_LAYER", "auto"), "GSDD_LAYER")


def gemm_flags(exact_f32=None):
    """GSDD_GEMM_F32=1: the exact-f32 MFMA instead of the bf16x3 matrix pipe."""
    if exact_f32 is None:
        exact_f32 = bool(os.environ.get("GSDD_GEMM_F32"))
    return abi.GEMM_EXACT_F32 if exact_f32 else 0


def axial_variant(valu=None):
    """GSDD_AXIAL_VALU=1: the LDS / vector kernel for every axis."""
    if valu is None:
        valu = bool(os.environ.get("GSDD_AXIAL_VALU"))
    return abi.AXIAL_VALU if valu else abi.AXIAL_AUTO


def taps_tensor(taps, device):
    """int32 device table [(dt,dh,dw), ...]"""
    return torch.tensor(taps, dtype=torch.int32, device=device).contiguous()


def gemm(inp, w, out, *, in_dims, out_grid, stride=(1, 1, 1), taps=None, ntaps=1, cin=None, in_pitch=None,
         gather=None, pro=None, ln=None, epi_scale=None, epi_shift=None, bvec=None, rows_per_batch=0, act=ACT_NONE,
         residual=None, out_dims=None, out_step=(1, 1, 1), out_off=(0, 0, 0), out_pitch=None, out_mode=0, cout=None,
         exact_f32=None, stream=None, _desc_only=False):
    """out[orow(m)][n] = epi(sum_tap sum_c pro(in[src(m,tap)][c]) * w[tap][n][c]).

    in_dims = (N, Di, Hi, Wi); out_grid = (Do, Ho, Wo); w: [ntaps][Cout][Cin];
    pro = (scale, shift) per input channel with ReLU; ln = (stats, gamma, beta, sel, stride)."""
    d = GemmDesc()
    N, Di, Hi, Wi = in_dims
    d.in_ = ptr(inp)
    d.N, d.Di, d.Hi, d.Wi = N, Di, Hi, Wi
    d.Cin = cin if cin is not None else w.shape[-1]
    d.in_pitch = in_pitch if in_pitch is not None else d.Cin
    d.Do, d.Ho, d.Wo = out_grid
    d.sd, d.sh, d.sw = stride
    d.ntaps = ntaps
    d.taps = ptr(taps)
    d.gather = ptr(gather)
    d.w = ptr(w)
    d.Cout = cout if cout is not None else w.shape[-2]
    if pro is not None:
        d.pro_scale, d.pro_shift = ptr(pro[0]), ptr(pro[1])
    if ln is not None:
        stats, gamma, beta, sel, ln_stride = ln
        d.ln_stats, d.ln_gamma, d.ln_beta, d.ln_sel, d.ln_stride = ptr(stats), ptr(gamma), ptr(beta), ptr(sel), ln_stride
    d.rows_per_batch = rows_per_batch
    d.epi_scale, d.epi_shift, d.bvec = ptr(epi_scale), ptr(epi_shift), ptr(bvec)
    d.act = act
    d.residual = ptr(residual)
    d.out = ptr(out)
    od = out_dims if out_dims is not None else out_grid
    d.oD, d.oH, d.oW = od
    d.osd, d.osh, d.osw = out_step
    d.ood, d.ooh, d.oow = out_off
    d.out_pitch = out_pitch if out_pitch is not None else d.Cout
    d.out_mode = out_mode
    d.flags = gemm_flags(exact_f32)
    if _desc_only:
        return d
    check(lib().gsdd_gemm(C.byref(d), stream_ptr(stream)))
    return out


def linear(x, w, out, *, bias=None, ln=None, rows_per_batch=0, act=ACT_NONE, residual=None, bvec=None, out_mode=0,
           stream=None):
    """Row GEMM: out[m][:] = act(pro(x[m]) @ w.T + bias [+ bvec[batch]]) [+ residual].  x: [M][Cin], w: [Cout][Cin]."""
    M = x.shape[0]
    return gemm(x, w, out, in_dims=(1, 1, 1, M), out_grid=(1, 1, M), ln=ln, epi_shift=bias, bvec=bvec,
                rows_per_batch=rows_per_batch, act=act, residual=residual, out_mode=out_mode, stream=stream)


def row_stats(x, stats, eps=1e-5, stream=None):
    check(lib().gsdd_row_stats(ptr(x), x.shape[0], x.shape[1], eps, ptr(stats), stream_ptr(stream)))
    return stats


def ln_apply(x, stats, gamma, beta, out=None, stream=None):
    """LayerNorm rows of any width from row_stats' statistics (gsdd_ln_apply) -> out [M][C]."""
    if out is None:
        out = torch.empty_like(x)
    check(lib().gsdd_ln_apply(ptr(x), ptr(stats), ptr(gamma), ptr(beta), x.shape[0], x.shape[1], ptr(out), stream_ptr(stream)))
    return out


def ncdhw_to_rows(x, cpad, padw, out=None, stream=None):
    N, Cc, D, H, W = x.shape
    if out is None:
        out = torch.empty((N, D, H, W + 2 * padw, cpad), dtype=torch.float32, device=x.device)
    check(lib().gsdd_ncdhw_to_rows(ptr(x), N, Cc, D, H, W, cpad, padw, ptr(out), stream_ptr(stream)))
    return out


def axial_attention(qkv, dims, C_, n_head, out, valu=None, stream=None):
    N, T, H, W = dims
    check(lib().gsdd_axial_attention(ptr(qkv), N, T, H, W, C_, n_head, ptr(out), axial_variant(valu), stream_ptr(stream)))
    return out


def pool3d(x, dims, C_, kernel, stride, pad_front, out_grid, out, *, mode="max", in_pitch=None, out_pitch=None, stream=None):
    """Channels-last 3-D pooling (gsdd_pool3d).  x: rows [N*Di*Hi*Wi][in_pitch] (C_ pooled channels), out: rows of out_pitch floats
    (may be a channel slice view's flat tail of a wider buffer)."""
    N, Di, Hi, Wi = dims
    k, s_, p = (C.c_int * 3)(*kernel), (C.c_int * 3)(*stride), (C.c_int * 3)(*pad_front)
    check(lib().gsdd_pool3d(ptr(x), N, Di, Hi, Wi, C_, in_pitch if in_pitch is not None else C_, k, s_, p, out_grid[0], out_grid[1],
                            out_grid[2], 0 if mode == "max" else 1, ptr(out), out_pitch if out_pitch is not None else C_,
                            stream_ptr(stream)))
    return out


def nearest_code(z, cb, idx, zq=None, stream=None, matrix=True):
    """matrix=False: no workspace -> the register-tiled vector kernel whatever the shape (tests compare the two)."""
    ws = None
    if matrix and not os.environ.get("GSDD_NEAREST_VALU"):
        ws = torch.empty((lib().gsdd_nearest_code_workspace_bytes(cb.shape[0]) // 4,), dtype=torch.float32, device=z.device)
    check(lib().gsdd_nearest_code(ptr(z), z.shape[0], z.shape[1], ptr(cb), cb.shape[0], ptr(idx), ptr(zq), ptr(ws),
                                  0 if ws is None else ws.numel() * 4, stream_ptr(stream)))
    return idx


def bn_train(x, bn, momentum=0.1, update_running=True, want_stats=False, stream=None):
    """Batch statistics of rows x[M][C] -> (scale, shift) for the consuming GEMM's prologue; updates bn's running stats.
    want_stats: also return the per-channel (mean, rstd) pairs the backward needs."""
    M, C_ = x.shape
    n = lib().gsdd_bn_train_workspace_bytes(M, C_)
    ws = torch.empty((n // 8,), dtype=torch.float64, device=x.device)
    scale = torch.empty((C_,), dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    rm, rv = (bn.running_mean, bn.running_var) if update_running else (None, None)
    mr = torch.empty((C_, 2), dtype=torch.float32, device=x.device) if want_stats else None
    check(lib().gsdd_bn_train(ptr(x), M, C_, ptr(bn.weight.detach()), ptr(bn.bias.detach()), bn.eps, momentum, ptr(rm), ptr(rv),
                              ptr(scale), ptr(shift), ptr(mr), ptr(ws), n, stream_ptr(stream)))
    if update_running:
        bn.num_batches_tracked += 1
    if want_stats:
        return (scale, shift), mr
    return scale, shift


def codebook_ema_stats(z, idx, K, stream=None):
    M, E = z.shape
    n_total = torch.empty((K,), dtype=torch.float32, device=z.device)
    encode_sum = torch.empty((K, E), dtype=torch.float32, device=z.device)
    dummy = torch.empty((2,), dtype=torch.float32, device=z.device)
    check(lib().gsdd_codebook_ema(ptr(z), ptr(idx), M, E, K, 0.99, None, ptr(n_total), ptr(n_total), ptr(n_total),
                                  ptr(n_total), ptr(encode_sum), ptr(dummy), 0, stream_ptr(stream)))
    return n_total, encode_sum


def codebook_ema_update(z, idx, perm, N, z_avg, emb, n_total, encode_sum, decay=0.99, n_local=None, m_local=None, stream=None):
    """z: the restart-candidate rows (tiled / broadcast).  scalars[1] = perplexity of the local one-hot mean: pass this rank's
    own counts `n_local` over its `m_local` latents whenever n_total was all-reduced or z was tiled."""
    M, E = z.shape
    scalars = torch.empty((2,), dtype=torch.float32, device=z.device)
    check(lib().gsdd_codebook_ema(ptr(z), ptr(idx), M, E, emb.shape[0], decay, ptr(perm), ptr(N), ptr(z_avg), ptr(emb),
                                  ptr(n_total), ptr(encode_sum), ptr(scalars), 1, stream_ptr(stream)))
    if n_local is not None:
        check(lib().gsdd_code_perplexity(ptr(n_local), emb.shape[0], m_local, ptr(scalars[1:]), stream_ptr(stream)))
    return scalars


def mse(a, b, scale=1.0, stream=None):
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    ws = torch.empty((1024,), dtype=torch.float64, device=a.device)
    check(lib().gsdd_mse(ptr(a), ptr(b), a.numel(), scale, ptr(out), ptr(ws), 8192, stream_ptr(stream)))
    return out[0]


def d3pm_embed(tok, emb, pos, x, rep=1, stream=None):
    B, L = tok.shape
    check(lib().gsdd_d3pm_embed(ptr(tok), B, L, emb.shape[1], ptr(emb), emb.shape[0], ptr(pos), rep, ptr(x),
                                stream_ptr(stream)))
    return x


def adaln_table(emb_w, lin_w, lin_b, out=None, stream=None):
    T, D = emb_w.shape
    if out is None:
        out = torch.empty((T, 2 * D), dtype=torch.float32, device=emb_w.device)
    check(lib().gsdd_adaln_table(ptr(emb_w), T, D, ptr(lin_w), ptr(lin_b), ptr(out), stream_ptr(stream)))
    return out


def small_linear(x, w, b, out=None, stream=None):
    R, Cin = x.shape
    if out is None:
        out = torch.empty((R, w.shape[0]), dtype=torch.float32, device=x.device)
    check(lib().gsdd_small_linear(ptr(x), R, Cin, ptr(w), ptr(b), w.shape[0], ptr(out), stream_ptr(stream)))
    return out


def d3pm_attention_workspace(B, L, H, device):
    n = lib().gsdd_d3pm_attention_workspace_bytes(B, L, H)
    return torch.empty(((n + 3) // 4,), dtype=torch.float32, device=device)


def d3pm_attention(q, k, v, B, L, H, out, ws=None, redo=None, mode=None, stream=None):
    """ws: scratch from d3pm_attention_workspace (matrix-pipe kernel); None -> workspace-free exact-f32 P.V kernel.
    redo: optional int64[1] device counter of the kernel's chunk-redo events (caller-owned; see include/gsdd.h).
    mode: 'auto' | '22' | '11' | 'a8' | 'a12' | 'f32pv' | 'kc256' (GSDD_ATTN_* of include/gsdd.h); None -> the environment, else auto."""
    nbytes = 0 if ws is None else ws.numel() * 4
    check(lib().gsdd_d3pm_attention(ptr(q), ptr(k), ptr(v), B, L, H, ptr(out), ptr(ws), nbytes, ptr(redo), attn_mode(mode) | attn_lean_flag(),
                                    stream_ptr(stream)))
    return out


def d3pm_layer(y, x, L, lay, cvec=None, nxt=None, t2=None, qkv=None, kv_img=None, range_flag=None, variant=None, stream=None):
    """Fused post-attention half of a block (+ the next block's AdaLN/qkv when `nxt` is given).
    y = lay = None: only the next-block stage on x as it is (block 0, whose input is the embedding)."""
    d = LayerDesc()
    d.y, d.x, d.M, d.L, d.n_embd, d.hidden = ptr(y), ptr(x), x.shape[0], L, x.shape[1], 256
    d.cvec = ptr(cvec)
    if lay is not None:
        d.hidden = lay["w1"].shape[0]
        d.wproj, d.bproj, d.ln2_g, d.ln2_b = ptr(lay["wproj"]), ptr(lay["bproj"]), ptr(lay["g2"]), ptr(lay["b2"])
        d.w1, d.b1, d.w2, d.b2 = ptr(lay["w1"]), ptr(lay["bb1"]), ptr(lay["w2"]), ptr(lay["bb2"])
        d.w2_x3 = ptr(lay.get("w2_x3"))
        d.layer_h2 = ptr(lay.get("lay_h2"))
    if nxt is not None:
        d.ada, d.t2, d.wqkv, d.bqkv, d.qkv = ptr(nxt["ada1"]), ptr(t2), ptr(nxt["wqkv"]), ptr(nxt["bqkv"]), ptr(qkv)
        d.wqkv_x3 = ptr(nxt.get("wqkv_x3"))
        d.wqkv_h2 = ptr(nxt.get("wqkv_h2"))
        d.kv_img = ptr(kv_img)
        d.kv_img_bytes = 0 if kv_img is None else kv_img.numel() * kv_img.element_size()
    d.range_flag = ptr(range_flag)
    d.variant = layer_variant(variant)
    check(lib().gsdd_d3pm_layer(C.byref(d), stream_ptr(stream)))


LAYER_X3_BYTES, WQKV_X3_BYTES = 40 * 3 * 1024, 24 * 3 * 1024


def d3pm_layer_pack(w2, wproj, wqkv, stream=None):
    """bf16x3 fragment images for the fused layer kernel: (w2 + wproj of a block, wqkv of a block); valid until the weights change."""
    lay_x3 = torch.empty((LAYER_X3_BYTES,), dtype=torch.uint8, device=w2.device)
    wqkv_x3 = torch.empty((WQKV_X3_BYTES,), dtype=torch.uint8, device=w2.device)
    check(lib().gsdd_d3pm_layer_pack(ptr(w2), ptr(wproj), ptr(wqkv), ptr(lay_x3), ptr(wqkv_x3), stream_ptr(stream)))
    return lay_x3, wqkv_x3


LAYER_H2_BYTES, WQKV_H2_BYTES = 72 * 2 * 1024, 24 * 2 * 1024


def d3pm_layer_pack_h2(w1, w2, wproj, wqkv, stream=None):
    """f16 hi + lo fragment images for the fused layer kernel: (w1 + w2 + wproj of a block, wqkv of a block)."""
    lay_h2 = torch.empty((LAYER_H2_BYTES,), dtype=torch.uint8, device=w2.device)
    wqkv_h2 = torch.empty((WQKV_H2_BYTES,), dtype=torch.uint8, device=w2.device)
    check(lib().gsdd_d3pm_layer_pack_h2(ptr(w1), ptr(w2), ptr(wproj), ptr(wqkv), ptr(lay_h2), ptr(wqkv_h2), stream_ptr(stream)))
    return lay_h2, wqkv_h2


def rows_linear_image_bytes(n_out, n_in):
    return (n_out // 64) * (n_in // 64) * 8 * 3 * 1024


def rows_linear_pack_many(table, n_desc, max_out, max_in, stream=None):
    """table: device bytes holding n_desc descriptors {w ptr, n_out, n_in, ld, transpose, image ptr} (include/gsdd.h)."""
    check(lib().gsdd_rows_linear_pack_many(ptr(table), n_desc, max_out, max_in, stream_ptr(stream)))


def rows_linear(x, image, n_out, out, *, bias=None, bvec=None, rows_per_batch=0, residual=None, head_major=False, stream=None):
    """out[m][:] = x[m] W'^T + bias [+ bvec[batch]] [+ residual[m]] with W' as a gsdd_rows_linear_pack_many image (training step)."""
    check(lib().gsdd_rows_linear(ptr(x), x.shape[0], x.shape[1], ptr(image), n_out, ptr(bias), ptr(bvec), rows_per_batch,
                                 ptr(residual), ptr(out), int(head_major), stream_ptr(stream)))
    return out


def d3pm_logits(x, g, b, w, bias, out, stream=None):
    check(lib().gsdd_d3pm_logits(ptr(x), x.shape[0], x.shape[1], ptr(g), ptr(b), ptr(w), ptr(bias), w.shape[0], ptr(out),
                                 stream_ptr(stream)))
    return out


def _cond_len_args(cond_len, cond_len_host, B, what):
    """(device pointer, host pointer or NULL) of a condition-length pair: int32 (B,) on the device, its optional host copy int32 (B,)."""
    if not torch.is_tensor(cond_len) or cond_len.dtype != torch.int32 or tuple(cond_len.shape) != (B,) or not cond_len.is_contiguous():
        raise GsddError(f"{what}: cond_len must be a contiguous int32 tensor of shape ({B},)")
    if cond_len_host is None:
        return ptr(cond_len), None
    h = cond_len_host
    if not torch.is_tensor(h) or h.is_cuda or h.dtype != torch.int32 or tuple(h.shape) != (B,) or not h.is_contiguous():
        raise GsddError(f"{what}: cond_len_host must be a contiguous int32 CPU tensor of shape ({B},)")
    return ptr(cond_len), C.c_void_p(h.data_ptr())


def d3pm_cross_attention(q, kc, vc, B, L, Te, H, out, stream=None, cond_len=None, cond_len_host=None):
    """cond_len: None, or int32 (B,) on the device -- batch element b attends to its first cond_len[b] keys only
    (gsdd_d3pm_cross_attention_len); cond_len_host: its host copy, range-checked before the launch."""
    if cond_len is None:
        check(lib().gsdd_d3pm_cross_attention(ptr(q), ptr(kc), ptr(vc), B, L, Te, H, ptr(out), stream_ptr(stream)))
    else:
        ln, lh = _cond_len_args(cond_len, cond_len_host, B, "d3pm_cross_attention")
        check(lib().gsdd_d3pm_cross_attention_len(ptr(q), ptr(kc), ptr(vc), ln, lh, B, L, Te, H, ptr(out), stream_ptr(stream)))
    return out


def d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, out, lse, stream=None, cond_len=None, cond_len_host=None):
    """Training forward of the general cross-attention: out rows [M][4 H] and lse [H][M] (log2 domain).  cond_len / cond_len_host as
    d3pm_cross_attention."""
    if cond_len is None:
        check(lib().gsdd_d3pm_cross_attention_train(ptr(q), ptr(kc), ptr(vc), B, L, Te, H, ptr(out), ptr(lse), stream_ptr(stream)))
    else:
        ln, lh = _cond_len_args(cond_len, cond_len_host, B, "d3pm_cross_attention_train")
        check(lib().gsdd_d3pm_cross_attention_train_len(ptr(q), ptr(kc), ptr(vc), ln, lh, B, L, Te, H, ptr(out), ptr(lse),
                                                        stream_ptr(stream)))
    return out


def d3pm_cross_attention_bwd_workspace(B, L, Te, H, device):
    n = lib().gsdd_d3pm_cross_attention_bwd_workspace_bytes(B, L, Te, H)
    return torch.empty(((n + 3) // 4,), dtype=torch.float32, device=device)


def d3pm_cross_attention_bwd(q, kc, vc, o, dO, lse, B, L, Te, H, ws, dq=None, dkc=None, dvc=None, stream=None, cond_len=None,
                             cond_len_host=None):
    """-> (dq head-major [H][M][4], dkc, dvc rows [B Te][4 H]), all overwritten; ws from d3pm_cross_attention_bwd_workspace.
    cond_len / cond_len_host as d3pm_cross_attention: the dkc / dvc rows at and behind a batch element's length are exact zeros."""
    f = dict(dtype=torch.float32, device=q.device)
    dq = torch.empty((H, B * L, 4), **f) if dq is None else dq
    dkc = torch.empty((B * Te, 4 * H), **f) if dkc is None else dkc
    dvc = torch.empty((B * Te, 4 * H), **f) if dvc is None else dvc
    nws = 0 if ws is None else ws.numel() * ws.element_size()
    if cond_len is None:
        check(lib().gsdd_d3pm_cross_attention_bwd(ptr(q), ptr(kc), ptr(vc), ptr(o), ptr(dO), ptr(lse), B, L, Te, H, ptr(dq), ptr(dkc),
                                                  ptr(dvc), ptr(ws), nws, stream_ptr(stream)))
    else:
        ln, lh = _cond_len_args(cond_len, cond_len_host, B, "d3pm_cross_attention_bwd")
        check(lib().gsdd_d3pm_cross_attention_bwd_len(ptr(q), ptr(kc), ptr(vc), ptr(o), ptr(dO), ptr(lse), ln, lh, B, L, Te, H, ptr(dq),
                                                      ptr(dkc), ptr(dvc), ptr(ws), nws, stream_ptr(stream)))
    return dq, dkc, dvc


def d3pm_step(logits_c, logits_u, tok_in, tok_out, sched, t_dev, stream_dev, *, K, T, guidance, seed, row0=0,
              post_dbg=None, x0_dbg=None, post_skip=0, trunc_rate=None, known=None, x_known=None, known_mode=0, stream=None):
    """trunc_rate: None (off) or 0 < r < 1, top-r truncation of the guided row before the posterior (gsdd_step_desc.trunc_rate).
    known: None (off) or a (B, L) uint8 / bool tensor, non-zero where the clean token x_known (B, L) int64 is given; known_mode 0
    re-noises x_known to the step's level, 1 holds it (gsdd_step_desc.known / x_known / known_mode)."""
    B, L = tok_in.shape
    d = StepDesc()
    if known is not None:
        if x_known is None:
            raise GsddError("d3pm_step: known needs x_known")
        if known.dtype not in (torch.uint8, torch.bool) or x_known.dtype != torch.int64:
            raise GsddError(f"d3pm_step: known must be uint8 / bool and x_known int64, got {known.dtype} / {x_known.dtype}")
        if tuple(known.shape) != (B, L) or tuple(x_known.shape) != (B, L) or not known.is_contiguous() or not x_known.is_contiguous():
            raise GsddError(f"d3pm_step: known and x_known must be contiguous {(B, L)} tensors, got {tuple(known.shape)} / {tuple(x_known.shape)}")
        d.known, d.x_known, d.known_mode = ptr(known), ptr(x_known), int(known_mode)
    d.post_skip = int(post_skip)
    d.trunc_rate = 0.0 if trunc_rate is None else float(trunc_rate)
    d.occupancy = int(os.environ.get("GSDD_STEP_OCC", "0"))
    d.logits_c, d.logits_u = ptr(logits_c), ptr(logits_u)
    d.tok_in, d.tok_out = ptr(tok_in), ptr(tok_out)
    d.B, d.L, d.K, d.T = B, L, K, T
    d.guidance = guidance
    for i in range(8):
        d.sched[i] = ptr(sched[i])
    d.t_dev, d.seed, d.stream_dev, d.row0 = ptr(t_dev), seed, ptr(stream_dev), row0
    d.post_dbg, d.x0_dbg = ptr(post_dbg), ptr(x0_dbg)
    check(lib().gsdd_d3pm_step(C.byref(d), stream_ptr(stream)))
    return tok_out


def d3pm_q_sample(x0, xt, sched, t_dev, stream_dev, *, K, T, seed, row0=0, stream=None):
    B, L = x0.shape
    arr = (C.c_void_p * 8)(*[ptr(s) for s in sched])
    check(lib().gsdd_d3pm_q_sample(ptr(x0), ptr(xt), B, L, K, T, arr, ptr(t_dev), seed, ptr(stream_dev), row0,
                                   stream_ptr(stream)))
    return xt


def d3pm_forward_jump(tok_in, tok_out, table, t_dev, stream_dev, *, K, T, jump, seed, row0=0, hold=None, stream=None):
    """tok_out ~ q(x_{a + jump} | x_a = tok_in) per position (gsdd_d3pm_forward_jump; tok_out may be tok_in).  table: the device f32
    [(T + 1), 3] log-probabilities of this jump (d3pm.jump_table), t_dev: int64 [B] from-levels a (-1 / T: clean), hold: None or a
    (B, L) uint8 / bool tensor, non-zero where the token is copied through."""
    B, L = tok_in.shape
    d = JumpDesc()
    if table.dtype != torch.float32 or table.numel() != (T + 1) * 3:
        raise GsddError(f"d3pm_forward_jump: table must hold {(T + 1) * 3} float32 values, got {tuple(table.shape)} {table.dtype}")
    if tok_in.dtype != torch.int64 or tok_out.dtype != torch.int64 or tuple(tok_out.shape) != (B, L) or t_dev.dtype != torch.int64 or t_dev.numel() < B:
        raise GsddError("d3pm_forward_jump: tok_in / tok_out must be int64 (B, L) tensors and t_dev int64 with at least B entries")
    if not (tok_in.is_contiguous() and tok_out.is_contiguous() and t_dev.is_contiguous() and table.is_contiguous()):
        raise GsddError("d3pm_forward_jump: tok_in, tok_out, t_dev and table must be contiguous")
    if hold is not None:
        if hold.dtype not in (torch.uint8, torch.bool) or tuple(hold.shape) != (B, L) or not hold.is_contiguous():
            raise GsddError(f"d3pm_forward_jump: hold must be a contiguous uint8 / bool {(B, L)} tensor, got {tuple(hold.shape)} {hold.dtype}")
        d.hold = ptr(hold)
    d.tok_in, d.tok_out = ptr(tok_in), ptr(tok_out)
    d.B, d.L, d.K, d.T = B, L, K, T
    d.table, d.jump = ptr(table), int(jump)
    d.t_dev, d.seed, d.stream_dev, d.row0 = ptr(t_dev), seed, ptr(stream_dev), row0
    check(lib().gsdd_d3pm_forward_jump(C.byref(d), stream_ptr(stream)))
    return tok_out


def d3pm_compose(logits, weights, *, n_cond, B, L, K, out=None, stream=None):
    """out = x_u + sum_i weights[b][i] (x_i - x_u) per position, x = clamp(log_softmax(.), -70, 0) (gsdd_d3pm_compose, include/gsdd.h):
    what a reverse step then reads as logits_c with logits_u = None.  logits: the denoiser's stacked f32 output, n_cond + 1 blocks of
    B L rows of K, the conditions first and the null condition last; weights: device f32 (B, n_cond); out: None (block 0 of logits,
    in place) or a (B L, K) f32 tensor clear of logits.  -> out, (B L, K)."""
    if not _is_int(n_cond) or not 1 <= n_cond <= abi.COMPOSE_MAX_COND:
        raise GsddError(f"d3pm_compose: n_cond must be an int in [1, {abi.COMPOSE_MAX_COND}], got {n_cond!r}")
    if not all(_is_int(v) and v >= 1 for v in (B, L, K)):
        raise GsddError(f"d3pm_compose: B, L and K must be positive ints, got {B!r}, {L!r}, {K!r}")
    rows = B * L
    if not torch.is_tensor(logits):
        raise GsddError(f"d3pm_compose: logits must be a tensor, got {type(logits).__name__}")
    if logits.dtype != torch.float32 or logits.numel() != (n_cond + 1) * rows * K or not logits.is_contiguous():
        raise GsddError(f"d3pm_compose: logits must be a contiguous float32 tensor of {n_cond + 1} blocks of {(rows, K)}, got "
                        f"{tuple(logits.shape)} {logits.dtype}")
    if not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) != (B, n_cond) or not weights.is_contiguous():
        raise GsddError(f"d3pm_compose: weights must be a contiguous float32 {(B, n_cond)} tensor")
    if weights.device != logits.device:
        raise GsddError(f"d3pm_compose: weights live on {weights.device}, logits on {logits.device}")
    if out is None:
        out = logits.view(n_cond + 1, rows, K)[0]
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, K) or not out.is_contiguous() or out.device != logits.device:
        raise GsddError(f"d3pm_compose: out must be a contiguous float32 {(rows, K)} tensor on {logits.device}, got {tuple(out.shape)} {out.dtype}")
    d = ComposeDesc()
    d.logits, d.weights, d.out = ptr(logits), ptr(weights), ptr(out)
    d.n_cond, d.B, d.L, d.K = n_cond, B, L, K
    check(lib().gsdd_d3pm_compose(C.byref(d), stream_ptr(stream)))
    return out


def _train_desc(logits, x0, xt, t_dev, pt, sched, K, T, mask_weight, aux_weight, adaptive_aux):
    """gsdd_train_desc with its inputs filled; the output pointers stay null (what gsdd_d3pm_train_loss_bwd takes)."""
    d = TrainDesc()
    d.logits, d.x0, d.xt, d.t_dev, d.pt = ptr(logits), ptr(x0), ptr(xt), ptr(t_dev), ptr(pt)
    (d.B, d.L), d.K, d.T = x0.shape, K, T
    for i in range(8):
        d.sched[i] = ptr(sched[i])
    d.mask_weight[0], d.mask_weight[1] = float(mask_weight[0]), float(mask_weight[1])
    d.aux_weight, d.adaptive_aux = float(aux_weight), int(bool(adaptive_aux))
    return d


def _train_outputs(d, x0, Lt_history, Lt_count, probs_classes=None):
    """Allocates the forward results and points d at them -> (the result dict, the per-position scratch: the caller holds it until its
    launch is enqueued)."""
    B, L = x0.shape
    dev = x0.device
    f = dict(dtype=torch.float32, device=dev)
    out = {"loss": torch.empty((1,), **f), "per_sample": torch.empty((B, 4), **f),
           "x0_recon": torch.empty((B, L), dtype=torch.int64, device=dev),
           "xt1_recon": torch.empty((B, L), dtype=torch.int64, device=dev),
           "probs": torch.empty((B, probs_classes, L), **f) if probs_classes else None}
    scratch = torch.empty((3, B * L), **f)
    d.kl, d.nll, d.aux = ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2])
    d.x0_recon, d.xt1_recon = ptr(out["x0_recon"]), ptr(out["xt1_recon"])
    d.Lt_history, d.Lt_count = ptr(Lt_history), ptr(Lt_count)
    d.loss, d.per_sample, d.probs = ptr(out["loss"]), ptr(out["per_sample"]), ptr(out["probs"])
    return out, scratch


def d3pm_train_loss(logits, x0, xt, t_dev, pt, sched, Lt_history, Lt_count, *, K, T, mask_weight, aux_weight, adaptive_aux,
                    want_probs=True, stream=None):
    """-> dict(loss [1], per_sample [B][4], x0_recon (B,L), xt1_recon (B,L), probs (B,K+1,L) or None)"""
    d = _train_desc(logits, x0, xt, t_dev, pt, sched, K, T, mask_weight, aux_weight, adaptive_aux)
    out, scratch = _train_outputs(d, x0, Lt_history, Lt_count, probs_classes=K + 1 if want_probs else None)
    check(lib().gsdd_d3pm_train_loss(C.byref(d), stream_ptr(stream)))
    return out


def d3pm_train_loss_grad(logits, x0, xt, t_dev, pt, sched, Lt_history, Lt_count, *, K, T, mask_weight, aux_weight, adaptive_aux,
                         stream=None):
    """d3pm_train_loss (without probs) and d3pm_train_loss_bwd in one pass over the logits -> (forward dict, dlogits)."""
    d = _train_desc(logits, x0, xt, t_dev, pt, sched, K, T, mask_weight, aux_weight, adaptive_aux)
    out, scratch = _train_outputs(d, x0, Lt_history, Lt_count)
    dlogits = torch.empty_like(logits)
    check(lib().gsdd_d3pm_train_loss_grad(C.byref(d), ptr(dlogits), stream_ptr(stream)))
    return out, dlogits


def advance(t_dev, dt, stream_dev, ds, stream=None):
    B = 0 if t_dev is None else t_dev.numel()
    check(lib().gsdd_advance(ptr(t_dev), B, dt, ptr(stream_dev), ds, stream_ptr(stream)))


def advance_floor(t_dev, dt, t_min, stream_dev, ds, stream=None):
    """t = max(t + dt, t_min), stream += ds on the device (the skip-step sampler's loop counter)."""
    B = 0 if t_dev is None else t_dev.numel()
    check(lib().gsdd_advance_floor(ptr(t_dev), B, dt, t_min, ptr(stream_dev), ds, stream_ptr(stream)))


def d3pm_purity_step(logits_c, logits_u, score, smax, cand, stream_dev, *, K, guidance, prior_rule, prior_weight, seed, row0=0,
                     recon_dbg=None, prob_dbg=None, score_dbg=None, trunc_rate=None, stream=None):
    """First half of a purity-prior call (gsdd_d3pm_purity_step): raw scores (B, L), their per-sample maximum (B,) and the candidate
    tokens (B, L) from the denoiser's logits.  trunc_rate: None (off) or 0 < r < 1, top-r truncation of log_x_recon."""
    B, L = cand.shape
    d = PurityDesc()
    d.logits_c, d.logits_u = ptr(logits_c), ptr(logits_u)
    d.B, d.L, d.K = B, L, K
    d.guidance, d.prior_rule, d.prior_weight = guidance, int(prior_rule), float(prior_weight)
    d.seed, d.stream_dev, d.row0 = seed, ptr(stream_dev), row0
    d.score, d.smax, d.cand = ptr(score), ptr(smax), ptr(cand)
    d.recon_dbg, d.prob_dbg, d.score_dbg = ptr(recon_dbg), ptr(prob_dbg), ptr(score_dbg)
    d.trunc_rate = 0.0 if trunc_rate is None else float(trunc_rate)
    check(lib().gsdd_d3pm_purity_step(C.byref(d), stream_ptr(stream)))
    return cand


def d3pm_purity_select(tok_in, tok_out, cand, score, smax, n_dev, stream_dev, *, K, prior_rule, seed, stream_add=0, row0=0,
                       key_dbg=None, stream=None):
    """Second half (gsdd_d3pm_purity_select): reveal n_dev[0] of each sample's [MASK] positions, Gumbel-top-n on the (B, L) draw at
    stream stream_dev[0] + stream_add."""
    B, L = tok_in.shape
    d = PuritySelectDesc()
    d.tok_in, d.tok_out, d.cand, d.score, d.smax = ptr(tok_in), ptr(tok_out), ptr(cand), ptr(score), ptr(smax)
    d.B, d.L, d.K, d.prior_rule = B, L, K, int(prior_rule)
    d.n_dev, d.seed, d.stream_dev, d.stream_add, d.row0 = ptr(n_dev), seed, ptr(stream_dev), int(stream_add), row0
    d.key_dbg = ptr(key_dbg)
    check(lib().gsdd_d3pm_purity_select(C.byref(d), stream_ptr(stream)))
    return tok_out


def advance_plan(step_dev, plan_t, plan_n, t_dev, n_dev, stream_dev, ds, stream=None):
    """step += 1; t[:] = plan_t[min(step, len - 1)], n = plan_n[...]; stream += ds -- on the device (the purity chain's counter)."""
    check(lib().gsdd_advance_plan(ptr(step_dev), ptr(plan_t), ptr(plan_n), plan_t.numel(), ptr(t_dev), t_dev.numel(), ptr(n_dev),
                                  ptr(stream_dev), ds, stream_ptr(stream)))


# ----------------------------------------------------------------------------- long clips (d3pm.long_plan, VQVAE.decode_long)
def d3pm_window_slide(tok, long_tok, x_known, known, t2, state, bad, *, F, k, n, K, t0, final=False, stream=None):
    """The op between two windows of a sliding-window rollout (gsdd_d3pm_window_slide): the finished window tok (Bs, F hw) int64,
    whose index is state[0], contributes its frames to long_tok (Bs, n hw) -- the lane's rows of the long buffer --, its last k
    frames become x_known[:, :k hw] (a token outside [0, K) there adds one to bad, int32 (1,)), known (Bs, F hw) uint8 becomes 1 on
    the first k hw positions and 0 elsewhere, tok all [MASK] = K, t2 (int64, its rows) t0 and state (int64 (2,)) moves to the next
    window.  final: only the copy to long_tok (the launch behind the last window); x_known, known, t2 and bad may be None."""
    if tok.dim() != 2 or tok.dtype != torch.int64 or not all(_is_int(v) for v in (F, k, n, K, t0)) or F < 1 or tok.shape[1] % F:
        raise GsddError(f"d3pm_window_slide: tok must be int64 (Bs, F hw) and F, k, n, K, t0 ints, got {tuple(tok.shape)} {tok.dtype}, F = {F!r}")
    Bs, Lw = tok.shape
    hw = Lw // F
    if long_tok.dtype != torch.int64 or tuple(long_tok.shape) != (Bs, n * hw):
        raise GsddError(f"d3pm_window_slide: long_tok must be int64 {(Bs, n * hw)}, got {tuple(long_tok.shape)} {long_tok.dtype}")
    if state.dtype != torch.int64 or state.numel() != 2:
        raise GsddError("d3pm_window_slide: state must hold two int64 words (the finished window's index, 0)")
    n_t2 = 0
    if not final:
        if x_known is None or known is None or t2 is None or bad is None:
            raise GsddError("d3pm_window_slide: x_known, known, t2 and bad are needed unless final")
        if x_known.dtype != torch.int64 or tuple(x_known.shape) != (Bs, Lw) or known.dtype != torch.uint8 or tuple(known.shape) != (Bs, Lw):
            raise GsddError(f"d3pm_window_slide: x_known must be int64 and known uint8, both {(Bs, Lw)}, got {tuple(x_known.shape)} "
                            f"{x_known.dtype} / {tuple(known.shape)} {known.dtype}")
        if t2.dtype != torch.int64 or bad.dtype != torch.int32 or bad.numel() != 1:
            raise GsddError("d3pm_window_slide: t2 must be int64 and bad one int32 word")
        n_t2 = t2.numel()
    check(lib().gsdd_d3pm_window_slide(ptr(tok), ptr(long_tok), ptr(x_known), ptr(known), ptr(t2), ptr(state), ptr(bad), Bs, F, hw, k, n,
                                       K, t0, n_t2, 1 if final else 0, stream_ptr(stream)))


BLEND_MODES = {"linear": abi.BLEND_LINEAR, "keep": abi.BLEND_KEEP, "replace": abi.BLEND_REPLACE}


def clip_window_blend(win, out, f0, n_ov, blend="linear", stream=None):
    """One decoded window win (B, C, Fw, H, W) float32 merged into the long clip out (B, C, Fo, H, W) at output frame f0
    (gsdd_clip_window_blend): its first n_ov frames overlap frames already in `out` -- crossfaded ("linear", weight (j + 1) /
    (n_ov + 1) for the window), left alone ("keep") or overwritten ("replace") --, the others are copied; frames behind Fo are
    dropped."""
    if not isinstance(blend, str) or blend not in BLEND_MODES:
        raise GsddError(f"clip_window_blend: blend must be one of {sorted(BLEND_MODES)}, got {blend!r}")
    if win.dim() != 5 or out.dim() != 5 or win.dtype != torch.float32 or out.dtype != torch.float32:
        raise GsddError(f"clip_window_blend: win and out must be float32 (B, C, frames, H, W), got {tuple(win.shape)} {win.dtype} / "
                        f"{tuple(out.shape)} {out.dtype}")
    B, C_, Fw, H, W = win.shape
    if tuple(out.shape[:2]) != (B, C_) or tuple(out.shape[3:]) != (H, W):
        raise GsddError(f"clip_window_blend: out {tuple(out.shape)} does not match win {tuple(win.shape)} outside the frame axis")
    if not _is_int(f0) or not _is_int(n_ov):
        raise GsddError(f"clip_window_blend: f0 and n_ov must be ints, got {f0!r}, {n_ov!r}")
    check(lib().gsdd_clip_window_blend(ptr(win), ptr(out), B * C_, Fw, H * W, out.shape[2], f0, n_ov, BLEND_MODES[blend],
                                       stream_ptr(stream)))
    return out


# ----------------------------------------------------------------------------- CLIP text tower (text.py)
def _host_ptr(t, what):
    """Pointer of a HOST int64 tensor (the optional host copy the text entry points range-check before they launch); None -> NULL."""
    if t is None:
        return None
    if t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
        raise GsddError(f"{what} must be a contiguous int64 CPU tensor")
    return C.c_void_p(t.data_ptr())


def text_embed(ids, tok_emb, pos_emb, x, S, ids_host=None, stream=None):
    """x[b*S + s] = tok_emb[ids[b][s]] + pos_emb[s], s < S (gsdd_text_embed).  ids: int64 (B, pitch >= S) on the device; ids_host: the
    same matrix on the host, checked against the vocabulary before the launch."""
    B, pitch = ids.shape
    if ids.dtype != torch.int64:
        raise GsddError(f"text_embed: ids must be int64, got {ids.dtype}")
    if ids_host is not None and tuple(ids_host.shape) != (B, pitch):
        raise GsddError(f"text_embed: ids_host has shape {tuple(ids_host.shape)}, ids {(B, pitch)}")
    check(lib().gsdd_text_embed(ptr(ids), _host_ptr(ids_host, "ids_host"), B, S, pitch, tok_emb.shape[1], ptr(tok_emb), tok_emb.shape[0],
                                ptr(pos_emb), pos_emb.shape[0], ptr(x), stream_ptr(stream)))
    return x


def _clip_attention(name, entry, qkv, B, S, n_head, out, scale, stream):
    """The two attention entry points of the CLIP towers (csrc/clip_attention.hip): `entry` is gsdd_<name>; scale defaults to d^-0.5."""
    C_ = qkv.shape[1] // 3
    if qkv.shape[0] != B * S or qkv.shape[1] != 3 * C_ or tuple(out.shape) != (B * S, C_):
        raise GsddError(f"{name}: qkv {tuple(qkv.shape)} / out {tuple(out.shape)} do not match B = {B}, S = {S}")
    if scale is None:
        scale = float(C_ // n_head) ** -0.5
    check(entry(ptr(qkv), B, S, C_, n_head, scale, ptr(out), stream_ptr(stream)))
    return out


def text_attention(qkv, B, S, n_head, out, scale=None, stream=None):
    """Causal self-attention over fused q|k|v rows [B*S][3C] -> out [B*S][C] (gsdd_text_attention); scale defaults to d^-0.5."""
    return _clip_attention("text_attention", lib().gsdd_text_attention, qkv, B, S, n_head, out, scale, stream)


def text_pool(x, eot, B, S, out, eot_host=None, stream=None):
    """out[b] = x[b*S + eot[b]] (gsdd_text_pool).  eot: int64 (B,) on the device; eot_host: its host copy, checked before the launch."""
    if eot.dtype != torch.int64 or tuple(eot.shape) != (B,) or (eot_host is not None and tuple(eot_host.shape) != (B,)):
        raise GsddError("text_pool: eot (and eot_host) must be int64 of shape (B,)")
    if x.shape[0] != B * S or tuple(out.shape) != (B, x.shape[1]):
        raise GsddError(f"text_pool: x {tuple(x.shape)} / out {tuple(out.shape)} do not match B = {B}, S = {S}")
    check(lib().gsdd_text_pool(ptr(x), ptr(eot), _host_ptr(eot_host, "eot_host"), B, S, x.shape[1], ptr(out), stream_ptr(stream)))
    return out


# ----------------------------------------------------------------------------- CLIP image tower (vision.py)
def clip_frame_patches(clips, R, P, out=None, stream=None):
    """ImageNet-normalised clips (B, 3, T, H, W) -> CLIP-normalised patch rows [B*T*G*G][3*P*P], G = R / P (gsdd_clip_frame_patches:
    de-normalise, quantise to uint8 levels, torch's bicubic resize to R x R, clamp, CLIP's normalisation).  H == W <= R, R % P == 0."""
    if clips.dim() != 5 or clips.shape[1] != 3 or clips.dtype != torch.float32:
        raise GsddError(f"clip_frame_patches: clips must be float32 (B, 3, T, H, W), got {clips.dtype} {tuple(clips.shape)}")
    B, _, T, H, W = clips.shape
    if H != W or H > R or P <= 0 or R % P:
        raise GsddError(f"clip_frame_patches: frames of {H} x {W} to resolution {R} in patches of {P}: H == W <= R and R % P == 0 "
                        "are required (non-square or shrunk frames are not supported)")
    G = R // P
    if out is None:
        out = torch.empty((B * T * G * G, 3 * P * P), dtype=torch.float32, device=clips.device)
    elif tuple(out.shape) != (B * T * G * G, 3 * P * P):
        raise GsddError(f"clip_frame_patches: out {tuple(out.shape)} is not {(B * T * G * G, 3 * P * P)}")
    check(lib().gsdd_clip_frame_patches(ptr(clips), B, T, H, W, R, P, ptr(out), stream_ptr(stream)))
    return out


def clip_vision_embed(patches, class_emb, pos_emb, N, S, x, stream=None):
    """x[n*S] = class_emb + pos_emb[0], x[n*S + 1 + p] = patches[n*(S-1) + p] + pos_emb[1 + p] (gsdd_clip_vision_embed)."""
    C_ = patches.shape[1]
    if patches.shape[0] != N * (S - 1) or tuple(x.shape) != (N * S, C_) or tuple(class_emb.shape) != (C_,) \
            or pos_emb.shape[0] < S or pos_emb.shape[1] != C_:
        raise GsddError(f"clip_vision_embed: patches {tuple(patches.shape)} / class {tuple(class_emb.shape)} / positions "
                        f"{tuple(pos_emb.shape)} / x {tuple(x.shape)} do not match N = {N}, S = {S}")
    check(lib().gsdd_clip_vision_embed(ptr(patches), ptr(class_emb), ptr(pos_emb), N, S, C_, ptr(x), stream_ptr(stream)))
    return x


def clip_attention(qkv, B, S, n_head, out, scale=None, stream=None):
    """Non-causal self-attention over fused q|k|v rows [B*S][3C] -> out [B*S][C] (gsdd_clip_attention); scale defaults to d^-0.5."""
    return _clip_attention("clip_attention", lib().gsdd_clip_attention, qkv, B, S, n_head, out, scale, stream)


# ----------------------------------------------------------------------------- GIF export (gif.py)
GIF_BINS = 32768


def _gif_clips(what, clips, per_frame):
    """-> (B, T, H, W, G) of ImageNet-normalised float32 clips (B, 3, T, H, W) on the device"""
    if not torch.is_tensor(clips) or clips.dim() != 5 or clips.shape[1] != 3 or clips.dtype != torch.float32:
        got = f"{clips.dtype} {tuple(clips.shape)}" if torch.is_tensor(clips) else type(clips).__name__
        raise GsddError(f"{what}: clips must be float32 (B, 3, T, H, W), got {got}")
    if not clips.is_cuda:
        raise GsddError(f"{what}: clips must live on a ROCm device (no CPU fallback)")
    B, _, T, H, W = clips.shape
    return B, T, H, W, (B * T if per_frame else B)


def _gif_words(what, t, shape, device):
    """a 32-bit integer tensor of `shape` on `device` (torch has no arithmetic on uint32: the kernels' uint32 words travel as int32)"""
    if t is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise GsddError(f"{what}: out must be int32 {tuple(shape)} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def gif_histogram(clips, per_frame=False, out=None, stream=None):
    """-> hist (G, 32768) int32 holding uint32 counts: pixels per 15-bit colour bin of every group (gsdd_gif_histogram); G = B, or
    B*T with per_frame."""
    B, T, H, W, G = _gif_clips("gif_histogram", clips, per_frame)
    out = _gif_words("gif_histogram", out, (G, GIF_BINS), clips.device)
    check(lib().gsdd_gif_histogram(ptr(clips), B, T, H, W, int(bool(per_frame)), ptr(out), stream_ptr(stream)))
    return out


def gif_box_sums(clips, box_of_bin, per_frame=False, out=None, stream=None):
    """box_of_bin (G, 32768) uint8 on the device -> sums (G, 256, 4) int32 holding uint32 (count, R, G, B sums) per box
    (gsdd_gif_box_sums)."""
    B, T, H, W, G = _gif_clips("gif_box_sums", clips, per_frame)
    if not torch.is_tensor(box_of_bin) or box_of_bin.dtype != torch.uint8 or tuple(box_of_bin.shape) != (G, GIF_BINS):
        raise GsddError(f"gif_box_sums: box_of_bin must be uint8 {(G, GIF_BINS)}")
    out = _gif_words("gif_box_sums", out, (G, 256, 4), clips.device)
    check(lib().gsdd_gif_box_sums(ptr(clips), B, T, H, W, int(bool(per_frame)), ptr(box_of_bin), ptr(out), stream_ptr(stream)))
    return out


def gif_map(clips, palette, n_colors, per_frame=False, dither=0, out=None, stream=None):
    """palette (G, 256, 4) uint8 (R, G, B, unused), n_colors (G,) int32, both on the device -> indices (B, T, H, W) uint8: the nearest of
    the first n_colors entries, lowest index on ties; dither: ordered-dither amplitude 0 .. 64 (gsdd_gif_map)."""
    if not isinstance(dither, int) or isinstance(dither, bool) or not 0 <= dither <= 64:
        raise GsddError(f"gif_map: dither is an integer amplitude in 0 .. 64, got {dither!r}")
    B, T, H, W, G = _gif_clips("gif_map", clips, per_frame)
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (G, 256, 4):
        raise GsddError(f"gif_map: palette must be uint8 {(G, 256, 4)}")
    if not torch.is_tensor(n_colors) or n_colors.dtype != torch.int32 or tuple(n_colors.shape) != (G,):
        raise GsddError(f"gif_map: n_colors must be int32 {(G,)}")
    if out is None:
        out = torch.empty((B, T, H, W), dtype=torch.uint8, device=clips.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, T, H, W):
        raise GsddError(f"gif_map: out must be uint8 {(B, T, H, W)}")
    check(lib().gsdd_gif_map(ptr(clips), B, T, H, W, int(bool(per_frame)), ptr(palette), ptr(n_colors), dither, ptr(out),
                             stream_ptr(stream)))
    return out


def _gif_palette(what, palette, n_colors, G):
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (G, 256, 4) or not palette.is_contiguous():
        raise GsddError(f"{what}: palette must be contiguous uint8 {(G, 256, 4)}")
    if not torch.is_tensor(n_colors) or n_colors.dtype != torch.int32 or tuple(n_colors.shape) != (G,) or not n_colors.is_contiguous():
        raise GsddError(f"{what}: n_colors must be int32 {(G,)}")
    if not palette.is_cuda or not n_colors.is_cuda:
        raise GsddError(f"{what}: palette and n_colors must live on a ROCm device (no CPU fallback)")


def gif_palette_sums(clips, palette, n_colors, per_frame=False, out=None, sse_out=None, stream=None):
    """One Lloyd assignment pass: palette (G, 256, 4) uint8, n_colors (G,) int32 on the device -> (sums (G, 256, 4) int32 holding
    uint32 (count, R, G, B sums) of the pixels nearest to each of the first n_colors entries, lowest index on ties, sse (G,) int64: the
    group's total squared distance) (gsdd_gif_palette_sums).  Both are zeroed by the call."""
    B, T, H, W, G = _gif_clips("gif_palette_sums", clips, per_frame)
    _gif_palette("gif_palette_sums", palette, n_colors, G)
    out = _gif_words("gif_palette_sums", out, (G, 256, 4), clips.device)
    if sse_out is None:
        sse_out = torch.empty((G,), dtype=torch.int64, device=clips.device)
    elif sse_out.dtype != torch.int64 or tuple(sse_out.shape) != (G,) or sse_out.device != clips.device or not sse_out.is_contiguous():
        raise GsddError(f"gif_palette_sums: sse_out must be contiguous int64 {(G,)} on {clips.device}")
    check(lib().gsdd_gif_palette_sums(ptr(clips), B, T, H, W, int(bool(per_frame)), ptr(palette), ptr(n_colors), ptr(out), ptr(sse_out),
                                      stream_ptr(stream)))
    return out, sse_out


def gif_diffuse(clips, palette, n_colors, per_frame=False, out=None, stream=None):
    """palette (G, 256, 4) uint8, n_colors (G,) int32 on the device -> indices (B, T, H, W) uint8 by Floyd-Steinberg error diffusion,
    every frame on its own, left to right and top to bottom (gsdd_gif_diffuse; the rule in full: include/gsdd.h)."""
    B, T, H, W, G = _gif_clips("gif_diffuse", clips, per_frame)
    _gif_palette("gif_diffuse", palette, n_colors, G)
    if out is None:
        out = torch.empty((B, T, H, W), dtype=torch.uint8, device=clips.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, T, H, W) or out.device != clips.device or not out.is_contiguous():
        raise GsddError(f"gif_diffuse: out must be contiguous uint8 {(B, T, H, W)} on {clips.device}")
    check(lib().gsdd_gif_diffuse(ptr(clips), B, T, H, W, int(bool(per_frame)), ptr(palette), ptr(n_colors), ptr(out), stream_ptr(stream)))
    return out


GIF_MAX_TOLERANCE = 3 * 255 * 255


def gif_delta(clips, indices, palette, n_colors, per_frame=False, tolerance=0, out=None, rects=None, changed=None, stream=None):
    """The delta stage: indices (B, T, H, W) uint8 of gif_map / gif_diffuse, palette (G, 256, 4) uint8, n_colors (G,) int32 on the
    device -> (out (B, T, H, W) uint8: the group's transparent index n_colors[g] wherever the pixel keeps the colour it shows (or, with
    tolerance > 0, shows one within that squared RGB distance of its level), rects (B, T, 4) int32: x0, y0, x1, y1 of the changed
    pixels, (W, H, -1, -1) for none, changed (B, T) int32 holding uint32 counts) (gsdd_gif_delta; the rule in full: include/gsdd.h).
    rects and changed are initialised by the call."""
    if not isinstance(tolerance, int) or isinstance(tolerance, bool) or not 0 <= tolerance <= GIF_MAX_TOLERANCE:
        raise GsddError(f"gif_delta: tolerance is an integer squared RGB distance in 0 .. {GIF_MAX_TOLERANCE}, got {tolerance!r}")
    B, T, H, W, G = _gif_clips("gif_delta", clips, per_frame)
    _gif_palette("gif_delta", palette, n_colors, G)
    dev = clips.device

    def buffer(name, t, dtype, shape):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise GsddError(f"gif_delta: {name} must be contiguous {dtype} {shape} on {dev}")
        return t
    if not torch.is_tensor(indices) or indices.dtype != torch.uint8 or tuple(indices.shape) != (B, T, H, W) or indices.device != dev \
            or not indices.is_contiguous():
        raise GsddError(f"gif_delta: indices must be contiguous uint8 {(B, T, H, W)} on {dev}")
    if not clips.is_contiguous():
        raise GsddError("gif_delta: clips must be contiguous")
    out = buffer("out", out, torch.uint8, (B, T, H, W))
    if out.data_ptr() == indices.data_ptr():
        raise GsddError("gif_delta: out must not be indices")
    rects = buffer("rects", rects, torch.int32, (B, T, 4))
    changed = buffer("changed", changed, torch.int32, (B, T))
    check(lib().gsdd_gif_delta(ptr(clips), ptr(indices), B, T, H, W, int(bool(per_frame)), ptr(palette), ptr(n_colors), tolerance, ptr(out),
                               ptr(rects), ptr(changed), stream_ptr(stream)))
    return out, rects, changed


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def gif_median_cut(hist, colors=256):
    """Host: hist (32768,) uint32 numpy -> (box_of_bin (32768,) uint8 numpy, number of boxes) (gsdd_gif_median_cut)."""
    import numpy as np
    if not isinstance(hist, np.ndarray) or hist.dtype != np.uint32 or hist.shape != (GIF_BINS,):
        raise GsddError("gif_median_cut: hist must be a uint32 numpy array of 32768 bins")
    if not isinstance(colors, int) or isinstance(colors, bool) or not 2 <= colors <= 256:
        raise GsddError(f"gif_median_cut: colors is an integer in 2 .. 256, got {colors!r}")
    hist = np.ascontiguousarray(hist)
    box = np.empty(GIF_BINS, dtype=np.uint8)
    n = C.c_int(0)
    check(lib().gsdd_gif_median_cut(_np_ptr(hist), colors, _np_ptr(box), C.byref(n)))
    return box, n.value


def gif_encode(indices, palettes, n_colors, delay_cs, loop=0, cap=None):
    """Host: indices (T, H, W) uint8, palettes (1 or T, 256, 3) uint8, n_colors (1 or T,) int32, all numpy -> (the GIF89a file as
    bytes, the clear codes its LZW streams hold) (gsdd_gif_encode).  cap: the output buffer's size (default: gsdd_gif_encode_bound)."""
    import numpy as np
    if not isinstance(indices, np.ndarray) or indices.dtype != np.uint8 or indices.ndim != 3:
        raise GsddError("gif_encode: indices must be a uint8 numpy array (T, H, W)")
    T, H, W = indices.shape
    if not isinstance(palettes, np.ndarray) or palettes.dtype != np.uint8 or palettes.ndim != 3 or palettes.shape[1:] != (256, 3) \
            or palettes.shape[0] not in (1, T):
        raise GsddError(f"gif_encode: palettes must be uint8 (1 or {T}, 256, 3)")
    n_colors = np.ascontiguousarray(n_colors, dtype=np.int32).reshape(-1)
    if n_colors.shape[0] != palettes.shape[0]:
        raise GsddError("gif_encode: one colour count per palette")
    indices, palettes = np.ascontiguousarray(indices), np.ascontiguousarray(palettes)
    L = lib()
    if cap is None:
        cap = L.gsdd_gif_encode_bound(T, H, W)
        if cap < 0:
            check(int(cap))
    buf = np.empty(cap + 1, dtype=np.uint8)
    buf[cap] = 0xA5                                            # a guard byte behind the buffer
    clears = C.c_int64(0)
    n = L.gsdd_gif_encode(_np_ptr(indices), T, H, W, _np_ptr(palettes), _np_ptr(n_colors), palettes.shape[0], int(delay_cs), int(loop),
                          _np_ptr(buf), cap, C.byref(clears))
    if buf[cap] != 0xA5:
        raise GsddError("gif_encode: the encoder wrote behind its buffer")
    if n < 0:
        check(int(n))
    return buf[:n].tobytes(), clears.value


def gif_encode_delta(indices, palettes, n_colors, rects, transparent, delay_cs, loop=0, cap=None):
    """Host: gif_encode for delta frames -- indices (T, H, W) uint8 (gif_delta's out), rects (T, 4) int32 = x0, y0, x1, y1 of each
    frame's sub-image ((W, H, -1, -1): none, written as 1 x 1), transparent (1 or T,) int32: each table's transparent index, -1 = none;
    all numpy -> (the GIF89a file as bytes, the clear codes its LZW streams hold) (gsdd_gif_encode_delta)."""
    import numpy as np
    if not isinstance(indices, np.ndarray) or indices.dtype != np.uint8 or indices.ndim != 3:
        raise GsddError("gif_encode_delta: indices must be a uint8 numpy array (T, H, W)")
    T, H, W = indices.shape
    if not isinstance(palettes, np.ndarray) or palettes.dtype != np.uint8 or palettes.ndim != 3 or palettes.shape[1:] != (256, 3) \
            or palettes.shape[0] not in (1, T):
        raise GsddError(f"gif_encode_delta: palettes must be uint8 (1 or {T}, 256, 3)")
    n_colors = np.ascontiguousarray(n_colors, dtype=np.int32).reshape(-1)
    transparent = np.ascontiguousarray(transparent, dtype=np.int32).reshape(-1)
    if n_colors.shape[0] != palettes.shape[0] or transparent.shape[0] != palettes.shape[0]:
        raise GsddError("gif_encode_delta: one colour count and one transparent index per palette")
    rects = np.ascontiguousarray(rects, dtype=np.int32)
    if rects.shape != (T, 4):
        raise GsddError(f"gif_encode_delta: rects must be int32 {(T, 4)}")
    indices, palettes = np.ascontiguousarray(indices), np.ascontiguousarray(palettes)
    L = lib()
    if cap is None:
        cap = L.gsdd_gif_encode_bound(T, H, W)
        if cap < 0:
            check(int(cap))
    buf = np.empty(cap + 1, dtype=np.uint8)
    buf[cap] = 0xA5                                            # a guard byte behind the buffer
    clears = C.c_int64(0)
    n = L.gsdd_gif_encode_delta(_np_ptr(indices), T, H, W, _np_ptr(palettes), _np_ptr(n_colors), palettes.shape[0], _np_ptr(rects),
                                _np_ptr(transparent), int(delay_cs), int(loop), _np_ptr(buf), cap, C.byref(clears))
    if buf[cap] != 0xA5:
        raise GsddError("gif_encode_delta: the encoder wrote behind its buffer")
    if n < 0:
        check(int(n))
    return buf[:n].tobytes(), clears.value


# ----------------------------------------------------------------------------- paired video metrics (metrics.py)
def _paired_operand(name, x):
    """-> (form, (B, T, H, W)) of one operand: 0 = float32 (B, 3, T, H, W), 1 = uint8 (B, T, H, W, 3)"""
    if torch.is_tensor(x) and x.dim() == 5 and x.dtype == torch.float32 and x.shape[1] == 3:
        form, shape = 0, (x.shape[0], x.shape[2], x.shape[3], x.shape[4])
    elif torch.is_tensor(x) and x.dim() == 5 and x.dtype == torch.uint8 and x.shape[4] == 3:
        form, shape = 1, tuple(x.shape[:4])
    else:
        got = f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__
        raise GsddError(f"paired_metrics: {name} must be float32 (B, 3, T, H, W) or uint8 (B, T, H, W, 3), got {got}")
    if not x.is_cuda:
        raise GsddError(f"paired_metrics: {name} must live on a ROCm device (no CPU fallback)")
    if not x.is_contiguous():
        raise GsddError(f"paired_metrics: {name} must be contiguous")
    return form, tuple(int(v) for v in shape)


def paired_metrics_tiles(H, W):
    """the tiles a plane of H x W is cut into: the length of the partials' tile axis (gsdd_paired_metrics_tiles)"""
    n = lib().gsdd_paired_metrics_tiles(int(H), int(W))
    if n < 0:
        check(int(n))
    return int(n)


def paired_metrics(a, b, want_ssim=True, partials=None, stream=None):
    """Two clips, each float32 (B, 3, T, H, W) ImageNet-normalised (its levels by the uint8 rule) or uint8 (B, T, H, W, 3), of the same
    B, T, H, W -> (sse (B, T, 3) int64: the squared error of the levels per frame and channel, exact; ssim (B, T, 3) float64: the mean
    SSIM of the plane's 11 x 11 Gaussian windows, or None without want_ssim, which then takes any H, W instead of >= 11)
    (gsdd_paired_metrics; the rule in full: include/gsdd.h).  partials: the kernel's per-tile results, int32
    (B*T*3, paired_metrics_tiles(H, W), 2); every word is written by the call.  The finish is a sum over the tile axis."""
    form_a, shape = _paired_operand("a", a)
    form_b, shape_b = _paired_operand("b", b)
    if shape != shape_b or a.device != b.device:
        raise GsddError(f"paired_metrics: a is (B, T, H, W) = {shape} on {a.device}, b {shape_b} on {b.device}")
    B, T, H, W = shape
    if min(shape) < 1:
        raise GsddError(f"paired_metrics: empty operands {shape}")
    want_ssim = bool(want_ssim)
    if want_ssim and (H < 11 or W < 11):
        raise GsddError(f"paired_metrics: SSIM needs H and W of at least 11, got {H} x {W} (want_ssim=False gives the squared error alone)")
    planes, tiles = B * T * 3, paired_metrics_tiles(H, W)
    if partials is None:
        partials = torch.zeros((planes, tiles, 2), dtype=torch.int32, device=a.device)
    elif not torch.is_tensor(partials) or partials.dtype != torch.int32 or tuple(partials.shape) != (planes, tiles, 2) \
            or partials.device != a.device or not partials.is_contiguous():
        raise GsddError(f"paired_metrics: partials must be contiguous int32 {(planes, tiles, 2)} on {a.device}")
    check(lib().gsdd_paired_metrics(ptr(a), form_a, ptr(b), form_b, B, T, H, W, int(want_ssim), ptr(partials), stream_ptr(stream)))
    sse = partials[:, :, 0].sum(dim=1, dtype=torch.int64).view(B, T, 3)
    if not want_ssim:
        return sse, None
    # (a DEVICE divisor: torch divides by a host scalar as a multiplication by its reciprocal, and n * (1 / n) is not always 1)
    windows = torch.full((), float((H - 10) * (W - 10)), dtype=torch.float64, device=a.device)
    ssim = partials.view(torch.float32)[:, :, 1].sum(dim=1, dtype=torch.float64) / windows
    return sse, ssim.view(B, T, 3)


# ----------------------------------------------------------------------------- LPIPS (lpips.py)
def lpips_stem_rows(x, table, padw, frame0=0, n=None, out=None, stream=None):
    """Frames frame0 .. frame0 + n - 1 (frame = b T + t; all of them by default) of a clip in either of paired_metrics' operand forms ->
    float32 (n, H, W + 2 padw, 4): per pixel the three values table[c][level] and 0, the padw columns in front of and behind every row 0
    -- the first convolution's operand with kw merged into the contraction (gsdd_lpips_stem_rows; the rule: include/gsdd.h).  table:
    float32 (3, 256) on the device (lpips.stem_table()).  Every float of `out` is written."""
    form, (B, T, H, W) = _paired_operand("x", x)
    n = B * T - frame0 if n is None else n
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (3, 256) or table.device != x.device \
            or not table.is_contiguous():
        raise GsddError(f"lpips_stem_rows: table must be contiguous float32 (3, 256) on {x.device}")
    shape = (int(n), H, W + 2 * int(padw), 4)
    if min(shape) < 1 or padw < 0:
        raise GsddError(f"lpips_stem_rows: nothing to write for n = {n}, padw = {padw} on frames of {H} x {W}")
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=x.device)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != x.device \
            or not out.is_contiguous():
        raise GsddError(f"lpips_stem_rows: out must be contiguous float32 {shape} on {x.device}")
    check(lib().gsdd_lpips_stem_rows(ptr(x), form, B, T, H, W, int(frame0), int(n), int(padw), ptr(table), ptr(out), stream_ptr(stream)))
    return out


def lpips_distance_slots(P, C_):
    """the workgroups one frame pair's P positions of C_ channels are cut into: the partials' slot axis (gsdd_lpips_distance_slots)"""
    s = lib().gsdd_lpips_distance_slots(int(P), int(C_))
    if s < 0:
        check(int(s))
    return int(s)


def lpips_layer_distance(feat, w, n, partials=None, stream=None):
    """feat: float32 rows (2 n P, C) of one tap, channels last, the n pred frames first and then the n target frames; w: float32 (C,)
    -> (n,) float64 on the device: the mean over the P positions of sum_c w_c (a^_c - b^_c)^2 with a^ = a / (sqrt(sum a^2) + 1e-10)
    (gsdd_lpips_layer_distance; the rule: include/gsdd.h).  partials: the kernel's per-workgroup sums, float64
    (n, lpips_distance_slots(P, C)); every word is written by the call.  The finish is a sum over the slot axis and a division by P."""
    if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 2 or not feat.is_cuda or not feat.is_contiguous():
        raise GsddError("lpips_layer_distance: feat must be contiguous float32 rows (2 n P, C) on a ROCm device (no CPU fallback)")
    rows, C_ = int(feat.shape[0]), int(feat.shape[1])
    n = int(n)
    if n < 1 or rows < 1 or rows % (2 * n) != 0:
        raise GsddError(f"lpips_layer_distance: {rows} rows do not hold 2 x {n} frames of equally many positions")
    if C_ % 4 != 0 or not 4 <= C_ <= 512:
        raise GsddError(f"lpips_layer_distance: C = {C_} is not a multiple of 4 in 4 .. 512")
    if not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (C_,) or w.device != feat.device or not w.is_contiguous():
        raise GsddError(f"lpips_layer_distance: w must be contiguous float32 ({C_},) on {feat.device}")
    P = rows // (2 * n)
    slots = lpips_distance_slots(P, C_)
    if partials is None:
        partials = torch.zeros((n, slots), dtype=torch.float64, device=feat.device)
    elif not torch.is_tensor(partials) or partials.dtype != torch.float64 or tuple(partials.shape) != (n, slots) \
            or partials.device != feat.device or not partials.is_contiguous():
        raise GsddError(f"lpips_layer_distance: partials must be contiguous float64 {(n, slots)} on {feat.device}")
    check(lib().gsdd_lpips_layer_distance(ptr(feat), ptr(w), n, P, C_, ptr(partials), stream_ptr(stream)))
    # (a DEVICE divisor, as in paired_metrics)
    return partials.sum(dim=1) / torch.full((), float(P), dtype=torch.float64, device=feat.device)


# ----------------------------------------------------------------------------- GIF import (gif.py)
GIF_INFO = ("width", "height", "frames", "palettes", "raster_bytes", "loop", "global_table", "version")


def _gif_bytes(what, data):
    import numpy as np
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(data, dtype=np.uint8)
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.ndim != 1:
        raise GsddError(f"{what}: the file is bytes or a one-dimensional uint8 numpy array")
    return np.ascontiguousarray(data)


def gif_probe(data):
    """Host: the bytes of a GIF -> dict of width, height, frames, palettes (colour tables, global + local), raster_bytes (the sum of
    w*h over the frames), loop (-1: none), global_table (0 / 1), version (87 / 89); block structure only, no LZW (gsdd_gif_probe)."""
    import numpy as np
    data = _gif_bytes("gif_probe", data)
    info = np.zeros(8, dtype=np.int64)
    check(lib().gsdd_gif_probe(_np_ptr(data), data.size, _np_ptr(info)))
    return dict(zip(GIF_INFO, (int(v) for v in info)))


def gif_decode(data, raster_cap=None):
    """Host: the bytes of a GIF -> (frames (F, 8) int32 [x, y, w, h, raster offset, palette row, transparent index or -1, disposal],
    delays (F,) int32 centiseconds, palettes (P, 256, 4) uint8, raster (raster_bytes,) uint8 in display order, info of gif_probe)
    (gsdd_gif_decode).  raster_cap: the raster buffer's size (default: the probe's raster_bytes)."""
    import numpy as np
    data = _gif_bytes("gif_decode", data)
    info = gif_probe(data)
    F, P = info["frames"], info["palettes"]
    cap = info["raster_bytes"] if raster_cap is None else int(raster_cap)
    if cap < 0:
        raise GsddError("gif_decode: raster_cap is not negative")
    frames = np.zeros((F, 8), dtype=np.int32)
    delays = np.zeros(F, dtype=np.int32)
    palettes = np.zeros((P, 256, 4), dtype=np.uint8)
    raster = np.zeros(cap + 1, dtype=np.uint8)
    raster[cap] = 0xA5                                         # a guard byte behind the buffer
    rc = lib().gsdd_gif_decode(_np_ptr(data), data.size, _np_ptr(frames), _np_ptr(delays), _np_ptr(palettes), _np_ptr(raster), cap)
    if raster[cap] != 0xA5:
        raise GsddError("gif_decode: the decoder wrote behind its buffer")
    check(rc)
    return frames, delays, palettes, raster[:cap], info


def gif_compose(raster, frames, palettes, W, H, select, matte=(0, 0, 0), out=None, stream=None, select_dev=None):
    """raster uint8 (n,), frames int32 (F, 8), palettes uint8 (P, 256, 4) on the device as gif_decode returned them; select: a list of
    frame numbers, non-decreasing in 0 .. F-1 -> out (T_out, H, W, 3) uint8: the composited canvas behind each selected frame
    (gsdd_gif_compose).  select_dev: `select` as an int32 tensor on the device, if the caller has copied it already (else it is
    copied here).  One launch, no synchronisation."""
    import contextlib

    import numpy as np
    if not (torch.is_tensor(raster) and raster.dtype == torch.uint8 and raster.dim() == 1):
        raise GsddError("gif_compose: raster must be a one-dimensional uint8 tensor")
    if not (torch.is_tensor(frames) and frames.dtype == torch.int32 and frames.dim() == 2 and frames.shape[1] == 8):
        raise GsddError("gif_compose: frames must be int32 (F, 8)")
    if not (torch.is_tensor(palettes) and palettes.dtype == torch.uint8 and palettes.dim() == 3 and tuple(palettes.shape[1:]) == (256, 4)):
        raise GsddError("gif_compose: palettes must be uint8 (P, 256, 4)")
    if not raster.is_cuda:
        raise GsddError("gif_compose: the tables must live on a ROCm device (no CPU fallback)")
    try:
        sel = np.ascontiguousarray(np.asarray(select, dtype=np.int64).reshape(-1).astype(np.int32))
        matte = tuple(int(c) for c in matte)
    except (TypeError, ValueError, OverflowError):
        raise GsddError("gif_compose: select is a list of frame numbers, matte an (R, G, B) of 0 .. 255")
    if len(matte) != 3 or not all(0 <= c <= 255 for c in matte):
        raise GsddError(f"gif_compose: matte is an (R, G, B) of 0 .. 255, got {matte!r}")
    T_out, W, H = int(sel.size), int(W), int(H)
    shape = (T_out, H, W, 3)
    if out is None:
        if T_out < 1 or not (1 <= W <= 65535 and 1 <= H <= 65535):
            shape = (1, 1, 1, 3)                               # (the library reports the bad sizes)
        out = torch.empty(shape, dtype=torch.uint8, device=raster.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape:
        raise GsddError(f"gif_compose: out must be uint8 {shape}")
    if select_dev is None:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            select_dev = torch.from_numpy(sel if T_out else np.zeros(1, dtype=np.int32)).to(raster.device)
    elif not (torch.is_tensor(select_dev) and select_dev.dtype == torch.int32 and tuple(select_dev.shape) == (T_out,)):
        raise GsddError(f"gif_compose: select_dev must be int32 {(T_out,)}")
    sel_dev = select_dev
    check(lib().gsdd_gif_compose(ptr(raster), ptr(frames), ptr(palettes), frames.shape[0], W, H, ptr(sel_dev), _np_ptr(sel), T_out,
                                 (matte[0] << 16) | (matte[1] << 8) | matte[2], ptr(out), stream_ptr(stream)))
    return out


def philox_uniform(seed, stream_id, n_rows, n_cols, device, row0=0):
    out = torch.empty((n_rows, n_cols), dtype=torch.float32, device=device)
    check(lib().gsdd_philox_uniform(seed, stream_id, row0, n_rows, n_cols, ptr(out), stream_ptr()))
    return out


class Graph:
    """A captured hipGraph of one reverse step (gsdd_graph_* in include/gsdd.h).  The capture is a bare stream capture, with no
    allocator pool of its own: `kept` holds every tensor handed to `ptr()` between `begin` and `end` (the temporaries an op's wrapper
    allocates included), so that no address the graph replays on returns to the allocator before the graph is gone."""

    def __init__(self):
        self.handle = C.c_void_p()
        self.kept = []

    def begin(self, stream):
        check(lib().gsdd_graph_begin(stream_ptr(stream)))
        abi._keeper = self.kept

    def end(self, stream):
        abi._keeper = None
        check(lib().gsdd_graph_end(stream_ptr(stream), C.byref(self.handle)))

    def launch(self, stream):
        check(lib().gsdd_graph_launch(self.handle, stream_ptr(stream)))

    def __del__(self):
        try:
            if self.handle:
                lib().gsdd_graph_destroy(self.handle)
        except Exception:
            pass


class Event:
    """hipEvent recorded on an explicit stream (torch.cuda.Event only sees torch's current stream)."""

    def __init__(self):
        self.h = C.c_void_p()
        check(lib().gsdd_event_create(C.byref(self.h)))

    def record(self, stream=None):
        check(lib().gsdd_event_record(self.h, stream_ptr(stream)))

    def elapsed_ms(self, stop):
        ms = C.c_float()
        check(lib().gsdd_event_elapsed_ms(self.h, stop.h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            lib().gsdd_event_destroy(self.h)
        except Exception:
            pass


# ----------------------------------------------------------------------------- training-step building blocks
def d3pm_train_loss_bwd(logits, x0, xt, t_dev, pt, sched, *, K, T, mask_weight, aux_weight, adaptive_aux, stream=None):
    d = _train_desc(logits, x0, xt, t_dev, pt, sched, K, T, mask_weight, aux_weight, adaptive_aux)
    dlogits = torch.empty_like(logits)
    check(lib().gsdd_d3pm_train_loss_bwd(C.byref(d), ptr(dlogits), stream_ptr(stream)))
    return dlogits


def gelu2(a, du=None, stream=None):
    out = torch.empty_like(a)
    check(lib().gsdd_gelu2(ptr(a), ptr(du), ptr(out), a.numel(), 0 if du is None else 1, stream_ptr(stream)))
    return out


def ln_fwd(x, gamma, beta, *, sel=None, gstride=0, rows_per_batch=1, eps=1e-5, stream=None):
    """-> (stats [M][2], y [M][64]): LayerNorm statistics and the normalised, scaled rows in one pass."""
    stats = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    check(lib().gsdd_ln_fwd(ptr(x), x.shape[0], x.shape[1], eps, ptr(gamma), ptr(beta), ptr(sel), gstride, rows_per_batch,
                            ptr(stats), ptr(y), stream_ptr(stream)))
    return stats, y


def ln_bwd(dh, x, stats, gamma, *, sel=None, gstride=0, rows_per_batch=1, dx_in=None, dgamma=None, dbeta=None,
           gacc_stride=0, acc_by_batch=False, stream=None):
    dx = torch.empty_like(x)
    check(lib().gsdd_ln_bwd(ptr(dh), ptr(x), ptr(stats), ptr(gamma), ptr(sel), gstride, rows_per_batch, x.shape[0], x.shape[1],
                            ptr(dx_in), ptr(dx), ptr(dgamma), ptr(dbeta), gacc_stride, int(acc_by_batch), stream_ptr(stream)))
    return dx


def wgrad(dY, X, dW, db=None, stream=None):
    """dW[N][K] += dY^T X ; db[N] += colsum(dY)"""
    check(lib().gsdd_wgrad(ptr(dY), dY.shape[1], ptr(X), X.shape[1], dY.shape[0], dY.shape[1], X.shape[1], ptr(dW), ptr(db),
                           stream_ptr(stream)))


def colsum(Y, out, stream=None):
    check(lib().gsdd_colsum(ptr(Y), Y.shape[1], Y.shape[0], Y.shape[1], ptr(out), stream_ptr(stream)))


def batch_rowsum(Y, B, L, out=None, stream=None):
    if out is None:
        out = torch.empty((B, Y.shape[1]), dtype=torch.float32, device=Y.device)
    check(lib().gsdd_batch_rowsum(ptr(Y), B, L, Y.shape[1], ptr(out), stream_ptr(stream)))
    return out


def d3pm_attention_train(q, k, v, B, L, H, out, lse, ws=None, mode=None, stream=None):
    check(lib().gsdd_d3pm_attention_train(ptr(q), ptr(k), ptr(v), B, L, H, ptr(out), ptr(lse), ptr(ws),
                                          0 if ws is None else ws.numel() * ws.element_size(), attn_train_mode(mode) | attn_lean_flag(), stream_ptr(stream)))


def d3pm_attention_bwd_workspace(B, L, H, device):
    n = lib().gsdd_d3pm_attention_bwd_workspace_bytes(B, L, H)
    return torch.empty((n // 4,), dtype=torch.float32, device=device)


def d3pm_attention_bwd(q, k, v, o, dO, lse, B, L, H, ws=None, variant=None, stream=None):
    dqkv = torch.empty((B * L, 3 * H * 4), dtype=torch.float32, device=q.device)
    scratch = torch.empty((H * B * L,), dtype=torch.float32, device=q.device)
    check(lib().gsdd_d3pm_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(dO), ptr(lse), B, L, H, ptr(dqkv), ptr(scratch), ptr(ws),
                                        0 if ws is None else ws.numel() * ws.element_size(), attn_bwd_variant(variant), stream_ptr(stream)))
    return dqkv


def d3pm_embed_bwd(dx, tok, demb, dpos, stream=None):
    B, L = tok.shape
    check(lib().gsdd_d3pm_embed_bwd(ptr(dx), ptr(tok), B, L, dx.shape[1], demb.shape[0], ptr(demb), ptr(dpos), stream_ptr(stream)))


def small_linear_bwd(dy, x, w, dw, db=None, want_dx=True, stream=None):
    R, Cin = x.shape
    dx = torch.empty_like(x) if want_dx else None
    check(lib().gsdd_small_linear_bwd(ptr(dy), ptr(x), ptr(w), R, Cin, w.shape[0], ptr(dx), ptr(dw), ptr(db), stream_ptr(stream)))
    return dx


def adaln_bwd(dtab, t, emb, w, demb, dw, db, stream=None):
    check(lib().gsdd_adaln_bwd(ptr(dtab), ptr(t), dtab.shape[0], emb.shape[1], ptr(emb), ptr(w), ptr(demb), ptr(dw), ptr(db),
                               stream_ptr(stream)))


# ----------------------------------------------------------------------------- optimiser stage (gsdd_optim_state; _optim.MultiAdam)
def grad_sqnorm(table, partials, stream=None):
    """partials[b] (float64) = sum of g^2 over block b of the wide table (int64 (n_blocks, 7))"""
    check(lib().gsdd_grad_sqnorm(ptr(table), table.shape[0], ptr(partials), stream_ptr(stream)))


def grad_norm_finalize(partials, n_blocks, max_norm, skip_nonfinite, state, stream=None):
    """norm, clip coefficient, finite flag and skip count into the device state block; max_norm None: no clipping"""
    check(lib().gsdd_grad_norm_finalize(ptr(partials), n_blocks, float("inf") if max_norm is None else max_norm,
                                        1 if skip_nonfinite else 0, ptr(state), stream_ptr(stream)))


def adamw_ema_multi(table, beta1, beta2, eps, weight_decay, ema_decay, state, stream=None):
    check(lib().gsdd_adamw_ema_multi(ptr(table), table.shape[0], beta1, beta2, eps, weight_decay, ema_decay or 0.0, ptr(state),
                                     stream_ptr(stream)))


def swap_multi(table, stream=None):
    """exchanges every block's parameter and running average, exactly"""
    check(lib().gsdd_swap_multi(ptr(table), table.shape[0], stream_ptr(stream)))


def set_deterministic(on):
    """Switches the training step's gradient reductions to their reproducible form (gsdd_set_deterministic; process-wide) -> the
    previous setting.  D3PMTrainer(deterministic=True) brackets its calls with it."""
    return bool(lib().gsdd_set_deterministic(1 if on else 0))


# ----------------------------------------------------------------------------- classifier-free training: condition dropout
def cond_dropout(cond, null_rows, p, *, seed, sid, row0=0, drop=None, out=None, drop_out=None, stream=None):
    """-> (out, drop_out): out[b] = the null rows where sample b is dropped, else cond[b] (gsdd_cond_dropout).  cond (B, Te, C) f32,
    null_rows (Te, C) f32; the decision is the Philox draw keyed by (seed, row0 + b, sid[0]) against p, or `drop` (B,) bool / uint8
    when given; sid: int64[1] device tensor (the stream id of the step's q_sample draw)."""
    if cond.dim() != 3 or cond.dtype != torch.float32 or null_rows.dtype != torch.float32:
        raise GsddError(f"cond_dropout: cond must be a float32 (B, Te, C) tensor and null_rows float32, got {tuple(cond.shape)} {cond.dtype}")
    B, Te, Cd = cond.shape
    if null_rows.numel() != Te * Cd:
        raise GsddError(f"cond_dropout: null_rows must hold (Te, C) = {(Te, Cd)} values, got {tuple(null_rows.shape)}")
    if drop is not None:
        if drop.dtype not in (torch.uint8, torch.bool) or tuple(drop.shape) != (B,):
            raise GsddError(f"cond_dropout: drop must be a bool / uint8 {(B,)} tensor, got {tuple(drop.shape)} {drop.dtype}")
    elif sid is None or sid.dtype != torch.int64:
        raise GsddError("cond_dropout: the draw needs sid, an int64[1] device tensor")
    out = torch.empty_like(cond) if out is None else out
    drop_out = torch.empty((B,), dtype=torch.uint8, device=cond.device) if drop_out is None else drop_out
    if out.dtype != torch.float32 or out.shape != cond.shape or drop_out.dtype != torch.uint8 or drop_out.numel() != B:
        raise GsddError("cond_dropout: out must be float32 of cond's shape and drop_out uint8 (B,)")
    check(lib().gsdd_cond_dropout(ptr(cond), ptr(null_rows), B, Te, Cd, float(p), int(seed), ptr(sid), int(row0), ptr(drop), ptr(out),
                                  ptr(drop_out), stream_ptr(stream)))
    return out, drop_out


def cond_null_grad(dk, dv, drop, wk, wv, B, Te, dnull, stream=None):
    """dnull (Te, C) += sum over the dropped samples of dk[b] Wk + dv[b] Wv (gsdd_cond_null_grad); dk / dv hold (B, Te, D) values,
    wk / wv are (D, C); dk and wk are both None on the one-token path.  drop: uint8 (B,), what cond_dropout wrote."""
    D, Cd = wv.shape
    if dv.numel() != B * Te * D or (dk is not None and dk.numel() != B * Te * D) or dnull.numel() != Te * Cd:
        raise GsddError(f"cond_null_grad: dk / dv must hold (B, Te, D) = {(B, Te, D)} values and dnull (Te, C) = {(Te, Cd)}")
    if drop.dtype not in (torch.uint8, torch.bool) or drop.numel() != B or (wk is not None and wk.shape != wv.shape):
        raise GsddError("cond_null_grad: drop must be bool / uint8 (B,) and wk of wv's shape")
    if any(x is not None and x.dtype != torch.float32 for x in (dk, dv, wk, wv, dnull)):
        raise GsddError("cond_null_grad: float32 tensors only")
    check(lib().gsdd_cond_null_grad(ptr(dk), ptr(dv), ptr(drop), ptr(wk), ptr(wv), B, Te, D, Cd, ptr(dnull), stream_ptr(stream)))
    return dnull


# ----------------------------------------------------------------------------- VQ-VAE training-step building blocks
def conv_wgrad(x, dY, dW, *, in_dims, out_grid, stride=(1, 1, 1), taps=None, ntaps=1, cin, cout, in_pitch=None, pro=None,
               out_dims=None, out_step=(1, 1, 1), out_off=(0, 0, 0), exact_f32=None, stream=None):
    """dW[tap][cout][cin] += sum_m dY[orow(m)] (x) pro(x[src(m,tap)])  (same geometry arguments as the forward gemm)."""
    d = gemm(x, dW, dW, in_dims=in_dims, out_grid=out_grid, stride=stride, taps=taps, ntaps=ntaps, cin=cin, in_pitch=in_pitch,
             pro=pro, out_dims=out_dims, out_step=out_step, out_off=out_off, cout=cout, exact_f32=exact_f32, _desc_only=True)
    check(lib().gsdd_conv_wgrad(C.byref(d), ptr(dY), dY.shape[-1], ptr(dW), stream_ptr(stream)))


def bn_relu_bwd(da, x, mean_rstd, bn, dgamma, dbeta, dx_in=None, stream=None):
    M, C_ = x.shape
    n = lib().gsdd_bn_relu_bwd_workspace_bytes(M, C_)
    ws = torch.empty(((n + 7) // 8,), dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    check(lib().gsdd_bn_relu_bwd(ptr(da), ptr(x), M, C_, ptr(mean_rstd), ptr(bn.weight.detach()), ptr(bn.bias.detach()),
                                 ptr(dx_in), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), n, stream_ptr(stream)))
    return dx


def relu_mask(dout, out, stream=None):
    dpre = torch.empty_like(dout)
    check(lib().gsdd_relu_mask(ptr(dout), ptr(out), ptr(dpre), dout.numel(), stream_ptr(stream)))
    return dpre


def lincomb(a, b, c, alpha, stream=None):
    out = torch.empty_like(b)
    check(lib().gsdd_lincomb(ptr(a), ptr(b), ptr(c), alpha, ptr(out), b.numel(), stream_ptr(stream)))
    return out


def axial_attention_bwd(qkv, datt, dims, C_, n_head, valu=None, stream=None, out=None):
    N, T, H, W = dims
    dqkv = out if out is not None else torch.empty_like(qkv)
    check(lib().gsdd_axial_attention_bwd(ptr(qkv), ptr(datt), N, T, H, W, C_, n_head, ptr(dqkv), axial_variant(valu), stream_ptr(stream)))
    return dqkv
