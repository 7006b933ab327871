"""No output of the library depends on what uninitialised memory held.

Every tests/test_gpu_*.py file runs its calls once, on buffers a fresh process has just obtained -- memory that usually reads as zero.
A kernel that accumulates into, reduces over, or reads a tail of a buffer it never wrote passes all of them and goes wrong in a real
loop, where torch's caching allocator hands back blocks that held logits, NaNs or indices a moment ago.  Here every case runs under
tests/stale_memory.py's `stale(byte)`: whatever torch.empty / empty_like / empty_strided / new_empty returns -- in the package's
wrappers and modules, and for the outputs the case itself allocates -- holds `byte` in every byte of its storage.

The scheme, the same for every case (`CASES`: id -> builder): the builder makes the inputs once, outside the context, and returns
`run()`, which allocates every workspace through the project's own functions and every caller-side output with torch.empty, makes the
calls and returns the outputs by name.  `run()` is called twice under 0x00 (the precondition: the entry is reproducible at all; the
cases marked `deterministic` hold ops.set_deterministic(True) for it) and once under each other byte of BYTES; every output is compared
bit for bit on an integer view, so that NaN equals NaN.  The helper must have filled at least once, and the case must have reached
every call site tests/stale_memory.py's ledger (SITES) gives it.

Where an entry point documents that it accumulates into, or leaves untouched, part of a caller's buffer (wgrad / colsum / conv_wgrad,
the gradient slots of ln_bwd / small_linear_bwd / adaln_bwd / embed_bwd / bn_relu_bwd / cond_null_grad, demb rows of absent
timesteps, the columns outside a pool3d / gemm out_pitch slice), the case initialises that part explicitly, as the entry's own test
does.  Fragment images with unused bytes (d3pm_layer_pack*, rows_linear_pack_many) are compared through their consumer's output.

Scratch that holds integers later used as addresses, read in the source before the first run:
  * nearest-code keys (small_ops.hip, gsdd_nearest_code): the caller's idx doubles as the 64-bit key array; nearest_code_keys_init_kernel
    writes every m < M before the matrix kernel's atomicMin, the finish kernel maps an untouched key to code 0 and any other to its low
    word, a code < K that nc_key packed; the norm workspace's K floats are all written by code_norm_kernel.
  * purity candidates (d3pm_purity.hip): the draw kernel stores cand[pos] for every position, purity_smax_kernel overwrites smax[b] from a
    block reduction over score[b][:] (every score written by the same launch); the selection copies cand into tok_out as a value only.
  * token outputs (d3pm_step / purity_select / q_sample / forward_jump) are written for every (b, l); the consumer that indexes with a
    token, the embedding kernel, clamps it into [0, n_embed - 1].
The GPU run confirms this reading; it is not a way to look for a fault."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

from tests import stale_memory as sm
from tests.stale_memory import BYTES, SITES

pytestmark = pytest.mark.gpu

CASES = {}
U8 = torch.uint8


def case(cid, deterministic=False):
    def deco(build):
        assert cid not in CASES, cid
        CASES[cid] = (build, deterministic)
        return build
    return deco


# ----------------------------------------------------------------------------- the harness
def run_case(cid, deterministic=None):
    """-> what stale_memory.sweep returns for the case: [(byte, {name: host bits}, Stale)] for 0x00, 0x00, 0xFF, 0x7F, 0xFE"""
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    build, det = CASES[cid]
    det = det if deterministic is None else deterministic
    prev = gsdd_amd.ops.set_deterministic(True) if det else None
    try:
        return sm.sweep(build(gsdd_amd))
    finally:
        if det:
            gsdd_amd.ops.set_deterministic(prev)


def assert_clean(cid, results):
    unstable, by_byte, reached = sm.verdict(results)
    fills = [st.fills for _, _, st in results]
    print(f"[stale] {cid}: fills {fills[0]}, package sites {sorted(s for s in reached if s[0].startswith(sm.PACKAGE))}")
    assert results[0][1] and all(h.numel() for h in results[0][1].values()), f"{cid}: an empty output compares nothing"
    assert not unstable, f"{cid}: two runs under 0x00 differ in {unstable}: the entry is not reproducible, nothing can be concluded"
    assert not by_byte, f"{cid}: outputs depend on what uninitialised memory held: " + str({f"0x{b:02X}": v for b, v in by_byte.items()})
    assert min(fills) >= 1, f"{cid}: the helper filled nothing"
    want = {site for site, ids in SITES.items() if cid in ids}
    assert want <= reached, f"{cid}: the ledger gives this case {sorted(want - reached)}, which it did not reach"


# ----------------------------------------------------------------------------- small helpers of the cases
def E(*shape, dtype=torch.float32):
    """a caller-side output: torch.empty, so that it is stale inside the context"""
    return torch.empty(shape, dtype=dtype, device="cuda")


def pre(t):
    """a caller-side buffer an entry accumulates into: obtained uninitialised, then initialised explicitly with `t`"""
    out = torch.empty(tuple(t.shape), dtype=t.dtype, device="cuda")
    out.copy_(t)
    return out


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ----------------------------------------------------------------------------- sampler attention
def _attention(L):
    def build(G):
        B, H = 2, 16
        g = gen(100 + L)
        q, k, v = (rn(g, H, B * L, 4, scale=1.5) for _ in range(3))

        def run():
            out = {}
            for mode in (None, "22", "a8", "11"):
                ws = G.ops.d3pm_attention_workspace(B, L, H, "cuda")
                redo = torch.zeros((1,), dtype=torch.int64, device="cuda")
                y = E(B * L, 4 * H)
                G.ops.d3pm_attention(q, k, v, B, L, H, y, ws=ws, redo=redo, mode=mode)
                out[f"out[{mode}]"], out[f"redo[{mode}]"] = y, redo
            return out
        return run
    return build


for _L in (32, 96, 288, 48, 40):          # matrix pipe (K/V images, key sums, norm bounds, statistics) | L % 16 == 0 only | VALU
    case(f"attention[L{_L}]")(_attention(_L))


# ----------------------------------------------------------------------------- training attention
def _attention_train(B, L, variant, with_ws):
    def build(G):
        H = 16
        g = gen(7 * L + B)
        q, k, v = (rn(g, H, B * L, 4, scale=1.5) for _ in range(3))
        dO = rn(g, B * L, 4 * H)

        def run():
            y, lse = E(B * L, 4 * H), E(H * B * L)
            ws = G.ops.d3pm_attention_workspace(B, L, H, "cuda") if with_ws else None
            G.ops.d3pm_attention_train(q, k, v, B, L, H, y, lse, ws=ws)
            bws = G.ops.d3pm_attention_bwd_workspace(B, L, H, "cuda") if with_ws else None
            dqkv = G.ops.d3pm_attention_bwd(q, k, v, y, dO, lse, B, L, H, ws=bws, variant=variant)
            return {"out": y, "lse": lse, "dqkv": dqkv}
        return run
    return build


for _B, _L in ((2, 64), (2, 96), (1, 320)):
    for _v in (None, "split"):
        case(f"attention_train[B{_B}-L{_L}-{_v or 'default'}]")(_attention_train(_B, _L, _v, True))
case("attention_train[B2-L40-no_workspace]")(_attention_train(2, 40, None, False))


# ----------------------------------------------------------------------------- cross-attention: sampler forward, training forward, backward
def _cross(B, L, Te, H, with_len):
    def build(G):
        from tests.test_gpu_cross_attention_train import make_inputs
        q, kc, vc, dO = make_inputs(B, L, Te, H)
        lens_host = torch.tensor([1, Te, max(1, Te // 2)][:B], dtype=torch.int32) if with_len else None
        lens = None if lens_host is None else lens_host.cuda()
        kw = dict(cond_len=lens, cond_len_host=lens_host)

        def run():
            O = G.ops
            y = O.d3pm_cross_attention(q, kc, vc, B, L, Te, H, E(B * L, 4 * H), **kw)
            yt, lse = E(B * L, 4 * H), E(H * B * L)
            O.d3pm_cross_attention_train(q, kc, vc, B, L, Te, H, yt, lse, **kw)
            ws = O.d3pm_cross_attention_bwd_workspace(B, L, Te, H, "cuda")
            dq, dkc, dvc = O.d3pm_cross_attention_bwd(q, kc, vc, yt, dO, lse, B, L, Te, H, ws, **kw)
            return {"out": y, "out_train": yt, "lse": lse, "dq": dq, "dkc": dkc, "dvc": dvc}
        return run
    return build


for _s in ((3, 37, 2, 3), (2, 64, 77, 1)):
    for _wl in (False, True):
        case("cross_attention[B%d-L%d-Te%d-H%d%s]" % (*_s, "-len" if _wl else ""))(_cross(*_s, _wl))


# ----------------------------------------------------------------------------- nearest code
def _nearest(kernel, E_, K, M):
    def build(G):
        from tests.test_gpu_nearest_code import case as nc_case, make_inputs
        z, cb = (t.cuda() for t in make_inputs(nc_case(kernel, E_, K, M))[:2])

        def run():
            out = {}
            for with_zq in (True, False):
                idx = E(M, dtype=torch.int64)
                zq = E(M, E_) if with_zq else None
                G.ops.nearest_code(z, cb, idx, zq, matrix=kernel == "matrix")
                out[f"idx[zq={with_zq}]"] = idx
                if with_zq:
                    out["zq"] = zq
            return out
        return run
    return build


for _c in (("matrix", 128, 64, 257), ("matrix", 128, 96, 257), ("matrix", 128, 64, 1), ("vector", 64, 65, 63), ("vector", 128, 96, 257)):
    case("nearest_code[%s-E%d-K%d-M%d]" % _c)(_nearest(*_c))


# ----------------------------------------------------------------------------- VQ-VAE training kernels
@case("bn_train")
def _bn_train(G):
    from tests.test_gpu_vqvae_train_kernels import bn_family, bn_params, make_bn
    shapes = [("mixed", 65, 260), ("m100", 63, 48), ("m10", 1, 260)]
    inputs = [(bn_family(f, M, C, 300 + C, "cuda"), bn_params(C, C + 2, "cuda")) for f, M, C in shapes]

    def run():
        out = {}
        for i, (x, (w, b, rm, rv)) in enumerate(inputs):
            bn = make_bn(w, b, rm, rv)
            (sc, sh), mr = G.ops.bn_train(x, bn, want_stats=True)
            sc2, sh2 = G.ops.bn_train(x, make_bn(w, b, rm, rv), update_running=False)
            out.update({f"scale{i}": sc, f"shift{i}": sh, f"mean_rstd{i}": mr, f"running_mean{i}": bn.running_mean,
                        f"running_var{i}": bn.running_var, f"scale_nostats{i}": sc2, f"shift_nostats{i}": sh2})
        return out
    return run


@case("bn_relu_bwd")
def _bn_relu_bwd(G):
    from tests.test_gpu_vqvae_train_kernels import bn_bwd_inputs, bn_family, bn_params, make_bn
    inputs = []
    for f, M, C, with_dx_in in (("mixed", 65, 260, True), ("m10", 63, 48, False)):
        x = bn_family(f, M, C, 300 + C + M, "cuda")
        w, b, rm, rv = bn_params(C, C + 2, "cuda")
        _, mr = G.ops.bn_train(x, make_bn(w, b, rm, rv), want_stats=True)
        inputs.append((x, (w, b, rm, rv), mr.clone(), bn_bwd_inputs(M, C, M + C, "cuda", with_dx_in)))

    def run():
        out = {}
        for i, (x, (w, b, rm, rv), mr, (da, dx_in, pre_g, pre_b)) in enumerate(inputs):
            dg, db = pre(pre_g), pre(pre_b)                              # gradient slots: the kernel accumulates
            out[f"dx{i}"] = G.ops.bn_relu_bwd(da, x, mr, make_bn(w, b, rm, rv), dg, db, dx_in=dx_in)
            out[f"dgamma{i}"], out[f"dbeta{i}"] = dg, db
        return out
    return run


@case("mse")
def _mse(G):
    g = gen(5)
    pairs = []
    for n in (5, 256 * 1024 + 1):                                        # one partial | the grid-stride loop and every partial
        a = rn(g, n)
        pairs.append((a, a + rn(g, n, scale=0.3)))

    def run():
        return {f"mse[n{a.numel()}]": G.ops.mse(a, b, 0.25).reshape(1) for a, b in pairs}
    return run


@case("codebook_ema")
def _codebook(G):
    from tests.test_gpu_vqvae_train_kernels import cb_update_inputs
    M, E_, K = 65, 12, 64
    c = cb_update_inputs(M, E_, K, M + 3 * E_ + K, "cuda")
    g = gen(M + K)
    z = rn(g, M, E_)
    # encode_sum is a sum by float atomics, with no reproducible form: here no code takes more than two rows (0 + a + b has one rounding
    # in either order), 24 codes take none (rows the call's own clearing must leave at zero)
    idx = (torch.randperm(M, generator=g) % 40).cuda()
    assert int(torch.bincount(idx, minlength=K).max()) == 2

    def run():
        n_total, es = G.ops.codebook_ema_stats(z, idx, K)
        N, za, emb = c["n0"].clone(), c["za0"].clone(), c["emb0"].clone()          # the codebook's state: updated in place
        s1 = G.ops.codebook_ema_update(c["z"], c["idx"], c["perm"], N, za, emb, c["n_total"], c["es"])
        N2, za2, emb2 = c["n0"].clone(), c["za0"].clone(), c["emb0"].clone()
        s2 = G.ops.codebook_ema_update(c["z"], c["idx"], c["perm"], N2, za2, emb2, c["n_total"], c["es"], n_local=c["n_local"], m_local=M)
        return {"n_total": n_total, "encode_sum": es, "N": N, "z_avg": za, "emb": emb, "scalars": s1, "N_local": N2, "z_avg_local": za2,
                "emb_local": emb2, "scalars_local": s2}
    return run


def _conv_wgrad(index):
    def build(G):
        from tests.test_gpu_gemm_family import CW_CASES, bn_pro, conv_taps, gen as ggen
        cid, k, stride, cin, cout, dims, exact, use_pro, regime = CW_CASES[index]
        g = ggen(61)
        B, T, H, W = dims
        grid = (T // stride[0], H // stride[1], W // stride[2])
        M = B * grid[0] * grid[1] * grid[2]
        ntaps = k[0] * k[1] * k[2]
        x = torch.randn(B * T * H * W, cin, generator=g).cuda()
        dY = torch.randn(M, cout, generator=g).cuda()
        pro = tuple(p.cuda() for p in bn_pro(cin, g)) if use_pro else None
        # The kernel adds one partial per block of row slabs onto dW with float atomics.  The x3_64 case has one such block per tile:
        # any prefill gives the same bits.  The f32 case has two: its prefill is zero, so that the sum 0 + a + b has one rounding in
        # either order (what the training step hands in: the gradient arena's zero fill).
        dW0 = torch.randn(ntaps, cout, cin, generator=g) if index == 1 else torch.zeros(ntaps, cout, cin)
        assert -(-M // ((128 if exact else 64) * regime[1])) == (1 if index == 1 else 2)
        taps = G.ops.taps_tensor(conv_taps(k, stride), "cuda")

        def run():
            dW = pre(dW0)                                                # the kernel accumulates
            G.ops.conv_wgrad(x, dY, dW, in_dims=dims, out_grid=grid, stride=stride, taps=taps, ntaps=ntaps, cin=cin, cout=cout, pro=pro,
                             exact_f32=exact)
            return {"dW": dW}
        return run
    return build


case("conv_wgrad[f32]")(_conv_wgrad(0))
case("conv_wgrad[x3_64]")(_conv_wgrad(1))


def _axial(dims, C_):
    def build(G):
        N, T, H, W = dims
        g = gen(C_ + T)
        qkv = rn(g, N * T * H * W, 9 * C_, scale=0.7)
        datt = rn(g, N * T * H * W, 3 * C_)

        def run():
            out = E(*datt.shape)
            G.ops.axial_attention(qkv, dims, C_, 2, out)
            return {"out": out, "dqkv": G.ops.axial_attention_bwd(qkv, datt, dims, C_, 2)}
        return run
    return build


case("axial_attention[1x4x16x16-C64]")(_axial((1, 4, 16, 16), 64))
case("axial_attention[1x16x8x4-C256]")(_axial((1, 16, 8, 4), 256))


@case("relu_mask_lincomb")
def _relu_lincomb(G):
    g = gen(9)
    dout, o = rn(g, 1028), torch.relu(rn(g, 1028))
    a, b, c = rn(g, 1000), rn(g, 1000), rn(g, 1000)

    def run():
        return {"relu_mask": G.ops.relu_mask(dout, o), "lincomb": G.ops.lincomb(a, b, c, 0.25), "lincomb_no_a": G.ops.lincomb(None, b, c, 0.25)}
    return run


# ----------------------------------------------------------------------------- D3PM training kernels
@case("ln_fwd")
def _ln_fwd(G):
    from tests.test_gpu_train_kernels import D, ln_rows
    g = gen(12)
    x1, x2 = ln_rows(1000, 1011), ln_rows(700, 711)
    gamma, beta = rn(g, D) + 1, rn(g, D)
    tab = rn(g, 100, 2 * D)
    t = torch.tensor([0, 99, 99, 5, 17, 63, 99], dtype=torch.int64, device="cuda")

    def run():
        s1, y1 = G.ops.ln_fwd(x1, gamma, beta)
        s2, y2 = G.ops.ln_fwd(x2, tab.view(-1), tab.view(-1)[D:], sel=t, gstride=2 * D, rows_per_batch=100)
        return {"stats_plain": s1, "y_plain": y1, "stats_adaln": s2, "y_adaln": y2}
    return run


@case("ln_bwd", deterministic=True)
def _ln_bwd(G):
    from tests.test_gpu_train_kernels import ln_bwd_run, ln_bwd_setup
    setups = [ln_bwd_setup(1000, 1, False, False), ln_bwd_setup(1600, 100, True, True)]       # plain ragged | AdaLN, straddling blocks

    def run():
        out = {}
        for i, s in enumerate(setups):
            r = ln_bwd_run(G, s)                                         # (its gradient slots are prefilled, between sentinels)
            out.update({f"dx{i}": r["dx"], f"buf{i}": r["buf"]})
        return out
    return run


@case("wgrad_colsum_rowsum", deterministic=True)
def _wgrad(G):
    from tests.test_gpu_gemm_family import wgrad_inputs
    dY, X, dW0, db0 = wgrad_inputs(129, 68, 68)
    torch.manual_seed(3)
    Ys = [torch.randn(200, 1, device="cuda"), torch.randn(700, 257, device="cuda")]
    outs0 = [torch.randn(1, device="cuda"), torch.randn(257, device="cuda")]
    Yb = torch.randn(3 * 77, 12, device="cuda")

    def run():
        dW, db = pre(dW0), pre(db0)                                      # += outputs
        G.ops.wgrad(dY, X, dW, db)
        out = {"dW": dW, "db": db}
        for i, (Y, o0) in enumerate(zip(Ys, outs0)):
            o = pre(o0)
            G.ops.colsum(Y, o)
            out[f"colsum{i}"] = o
        out["batch_rowsum"] = G.ops.batch_rowsum(Yb, 3, 77)             # overwritten: the call clears it
        out["batch_rowsum_out"] = G.ops.batch_rowsum(Yb, 3, 77, out=E(3, 12))
        return out
    return run


@case("embed", deterministic=True)
def _embed(G):
    from tests.test_gpu_train_kernels import D, embed_bwd_run, embed_setup
    s = embed_setup(3, 100, 0.5)

    def run():
        x = E(s.M, D)
        G.ops.d3pm_embed(s.tok, s.emb, s.pos, x)
        r = embed_bwd_run(G, s)                                          # (demb / dpos prefilled: rows of absent tokens stay)
        return {"x": x, "ebuf": r["ebuf"], "pbuf": r["pbuf"]}
    return run


@case("small_linear")
def _small_linear(G):
    g = gen(16512)
    R, Cin, Cout = 16, 512, 64
    x, w, b, dy = rn(g, R, Cin), rn(g, Cout, Cin, scale=Cin ** -0.5), rn(g, Cout), rn(g, R, Cout)
    pre_w, pre_b = rn(g, Cout, Cin), rn(g, Cout)

    def run():
        out = {"y": G.ops.small_linear(x, w, b), "y_out": G.ops.small_linear(x, w, b, out=E(R, Cout))}
        for want_dx in (True, False):
            dw, db = pre(pre_w), pre(pre_b)
            dx = G.ops.small_linear_bwd(dy, x, w, dw, db, want_dx=want_dx)
            out.update({f"dw[{want_dx}]": dw, f"db[{want_dx}]": db})
            if want_dx:
                out["dx"] = dx
        return out
    return run


@case("adaln", deterministic=True)
def _adaln(G):
    from tests.test_gpu_train_kernels import D, adaln_bwd_run, adaln_bwd_setup
    g = gen(31)
    emb, w, b = rn(g, 100, D, scale=3.0), rn(g, 2 * D, D, scale=0.125), rn(g, 2 * D)
    setups = [adaln_bwd_setup(16), adaln_bwd_setup(97)]                  # the LDS instantiation | the first batch without it

    def run():
        out = {"table": G.ops.adaln_table(emb, w, b), "table_out": G.ops.adaln_table(emb, w, b, out=E(100, 2 * D))}
        for s in setups:
            r = adaln_bwd_run(G, s)                                      # (prefilled gradients between sentinels)
            out.update({f"ebuf[B{s.B}]": r["ebuf"], f"wbuf[B{s.B}]": r["wbuf"], f"bbuf[B{s.B}]": r["bbuf"]})
        return out
    return run


@case("gelu2")
def _gelu2(G):
    g = gen(6)
    a, du = rn(g, 1028, scale=3.0), rn(g, 1028)

    def run():
        return {"u": G.ops.gelu2(a), "da": G.ops.gelu2(a, du)}
    return run


def _small_dm(G, K, spatial=(8, 5), T=100):
    L = spatial[0] * spatial[1]
    d = G.DalleMaskImageEmbedding(num_embed=K, spatial_size=list(spatial), embed_dim=64)
    tr = G.Text2ImageTransformer(dalle=d, n_layer=1, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                 content_spatial_size=list(spatial), diffusion_step=T)
    return G.DiffusionTransformer(transformer=tr, diffusion_step=T, alpha_init_type="alpha1", auxiliary_loss_weight=5e-4,
                                  adaptive_auxiliary_loss=True, guidance_scale=2, content_seq_len=L).cuda()


def _train_loss(K):
    def build(G):
        B, L, T = 3, 40, 100
        sched = _small_dm(G, K)._sched()
        g = gen(K)
        logits = rn(g, B * L, K, scale=3.0)
        x0 = torch.randint(0, K, (B, L), generator=g).cuda()
        xt = x0.clone()
        xt[(torch.rand(B, L, generator=g) < 0.5).cuda()] = K
        xt[0, :5] = torch.randint(0, K, (5,), generator=g).cuda()
        t, pt = i64([0, 37, 99]), torch.tensor([0.01, 0.02, 0.005]).cuda()
        h0, c0 = torch.rand(T, generator=g).cuda(), torch.randint(0, 20, (T,), generator=g).float().cuda()
        kw = dict(K=K, T=T, mask_weight=[1.0, 0.7], aux_weight=5e-4, adaptive_aux=True)

        def run():
            O = G.ops
            ha, ca, hb, cb = h0.clone(), c0.clone(), h0.clone(), c0.clone()          # Lt_history / Lt_count: updated in place
            fa = O.d3pm_train_loss(logits, x0, xt, t, pt, sched, ha, ca, want_probs=True, **kw)
            ga = O.d3pm_train_loss_bwd(logits, x0, xt, t, pt, sched, **kw)
            fb, gb = O.d3pm_train_loss_grad(logits, x0, xt, t, pt, sched, hb, cb, **kw)
            out = {"bwd": ga, "grad": gb, "Lt_history": ha, "Lt_count": ca, "Lt_history_fused": hb, "Lt_count_fused": cb}
            out.update({f"loss.{k}": v for k, v in fa.items() if v is not None})
            out.update({f"fused.{k}": v for k, v in fb.items() if v is not None})
            return out
        return run
    return build


case("train_loss[K32]")(_train_loss(32))
case("train_loss[K4096]")(_train_loss(4096))


# ----------------------------------------------------------------------------- sampler row kernels
def _rows(K):
    def build(G):
        B, L, T = 2, 37, 100
        dm = _small_dm(G, K)
        sched = dm._sched()
        g = gen(K + 1)
        lc, lu = rn(g, B * L, K, scale=3.0), rn(g, B * L, K, scale=3.0)
        tok = torch.randint(0, K, (B, L), generator=g)
        tok[:, ::3] = K
        tok = tok.cuda()
        x0 = torch.randint(0, K, (B, L), generator=g).cuda()
        known = (torch.rand(B, L, generator=g) < 0.3).to(U8).cuda()
        t, sid = i64([37, 99]), i64([3])
        levels = i64([20, -1])
        table = dm._jump_table(7, torch.device("cuda"))
        kw = dict(K=K, T=T, guidance=2.0, seed=11, row0=5 * L)
        cond, null = rn(g, 4, 3, 64), rn(g, 3, 64)
        dk, dv, wk, wv = rn(g, 4, 3, 64), rn(g, 4, 3, 64), rn(g, 64, 64), rn(g, 64, 64)
        dnull0 = rn(g, 3, 64)

        def run():
            O = G.ops
            out = {}
            for name, extra in (("plain", {}), ("truncated", dict(trunc_rate=0.86)), ("skip", dict(post_skip=3)),
                                ("known_renoise", dict(known=known, x_known=x0, known_mode=0)),
                                ("known_hold", dict(known=known, x_known=x0, known_mode=1, trunc_rate=0.86))):
                out[f"step[{name}]"] = O.d3pm_step(lc, lu, tok, E(B, L, dtype=torch.int64), sched, t, sid, **kw, **extra)
            out["step[unguided]"] = O.d3pm_step(lc, None, tok, E(B, L, dtype=torch.int64), sched, t, sid, **kw)
            for rule, weight, trunc in ((1, 0.0, None), (2, 1.0, None), (2, 1.0, 0.86)):
                score, smax, cand = E(B, L), E(B), E(B, L, dtype=torch.int64)
                O.d3pm_purity_step(lc, lu, score, smax, cand, sid, K=K, guidance=2.0, prior_rule=rule, prior_weight=weight, seed=11,
                                   row0=5 * L, trunc_rate=trunc)
                sel = O.d3pm_purity_select(tok, E(B, L, dtype=torch.int64), cand, score, smax, i64([2]), sid, K=K, prior_rule=rule, seed=11,
                                           stream_add=1, row0=5 * L)
                tag = f"{rule}-{weight}-{trunc}"
                out.update({f"score[{tag}]": score, f"smax[{tag}]": smax, f"cand[{tag}]": cand, f"select[{tag}]": sel})
            out["q_sample"] = O.d3pm_q_sample(x0, E(B, L, dtype=torch.int64), sched, t, sid, K=K, T=T, seed=11, row0=5 * L)
            out["jump"] = O.d3pm_forward_jump(tok, E(B, L, dtype=torch.int64), table, levels, sid, K=K, T=T, jump=7, seed=11, row0=5 * L)
            out["jump_hold"] = O.d3pm_forward_jump(tok, E(B, L, dtype=torch.int64), table, levels, sid, K=K, T=T, jump=7, seed=11, row0=5 * L,
                                                   hold=known)
            dropped, drop = O.cond_dropout(cond, null, 0.5, seed=11, sid=sid, row0=2)
            out["cond_dropout"], out["drop"] = dropped, drop
            out["dnull"] = O.cond_null_grad(dk, dv, drop, wk, wv, 4, 3, pre(dnull0))           # += output
            out["philox"] = O.philox_uniform(11, 3, 5, 37, "cuda", row0=2)
            return out
        return run
    return build


case("sampler_rows[K32]")(_rows(32))
case("sampler_rows[K4096]")(_rows(4096))


# ----------------------------------------------------------------------------- the optimiser stage
@case("multi_adam")
def _multi_adam(G):
    from gsdd_amd._optim import MultiAdam
    g = gen(21)
    sizes = [1, 4097, 3 * 4096 + 5]
    p0 = [rn(g, n) for n in sizes]
    g0 = [[rn(g, n, scale=1e-2) for n in sizes] for _ in range(2)]

    def run():
        params = [(f"p{i}", p.clone()) for i, p in enumerate(p0)]
        opt = MultiAdam(params, 1e-3, (0.9, 0.96), 1e-8, max_grad_norm=0.05, weight_decay=0.05, ema_decay=0.999)
        for step in range(2):
            opt.step({f"p{i}": pre(gr) for i, gr in enumerate(g0[step])})
        out = {name: p for name, p in params}
        out.update({"m": opt.m, "v": opt.v, "ema": opt.ema, "partials": opt.partials, "grad_norm": opt.grad_norm.reshape(1),
                    "clip_coef": opt.clip_coef.reshape(1)})
        return out
    return run


# ----------------------------------------------------------------------------- CLIP kernels
@case("clip_kernels")
def _clip(G):
    from clip_vision_ref import make_clips
    g = gen(33)
    B = 3
    att = {(S, h, d): rn(g, B * S, 3 * h * d) for S in (17, 50) for h, d in ((2, 64), (2, 16))}
    clips = make_clips(2, 3, 37, seed=101).cuda()
    N, S, C = 3, 10, 72
    pe, cls, pos = rn(g, N * (S - 1), C), rn(g, C), rn(g, S + 2, C)
    Bt, St, pitch, vocab = 5, 19, 23, 41
    tok_emb, pos_emb = rn(g, vocab, C), rn(g, St + 3, C)
    ids = torch.randint(0, vocab, (Bt, pitch), generator=g)
    eot = torch.tensor([0, St - 1, 3, 7, St - 1])
    ids_d, eot_d = ids.cuda(), eot.cuda()

    def run():
        O = G.ops
        out = {}
        for (S_, h, d), qkv in att.items():
            out[f"text_attention[S{S_}-d{d}]"] = O.text_attention(qkv, B, S_, h, E(B * S_, h * d))
            out[f"clip_attention[S{S_}-d{d}]"] = O.clip_attention(qkv, B, S_, h, E(B * S_, h * d))
        out["patches"] = O.clip_frame_patches(clips, 64, 32)
        out["vision_embed"] = O.clip_vision_embed(pe, cls, pos, N, S, E(N * S, C))
        x = O.text_embed(ids_d, tok_emb, pos_emb, E(Bt * St, C), St, ids_host=ids)
        out["text_embed"] = x
        out["text_pool"] = O.text_pool(x, eot_d, Bt, St, E(Bt, C), eot_host=eot)
        return out
    return run


# ----------------------------------------------------------------------------- GIF kernels
def _gif(per_frame):
    def build(G):
        import gif_ref
        from tests.test_gpu_gif_read import scene
        rng = np.random.default_rng(17)
        colours = rng.integers(0, 256, (40, 3))
        shape = (2, 3, 9, 11)
        levels = np.clip(colours[rng.integers(0, 40, shape)] + rng.integers(-3, 4, shape + (3,)), 0, 255).astype(np.uint8)
        for t in (1, 2):                                                 # frames that keep most of their predecessor: deltas with a rectangle
            keep = rng.random(shape[2:]) < 0.7
            levels[:, t][:, keep] = levels[:, t - 1][:, keep]
        clips = torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda()
        hist = gif_ref.histogram(levels, per_frame)
        cuts = [gif_ref.median_cut(h, 16) for h in hist]
        box = torch.from_numpy(np.stack([c[0] for c in cuts])).cuda()
        n = torch.from_numpy(np.array([c[1] for c in cuts], dtype=np.int32)).cuda()
        pal = gif_ref.palette_of(gif_ref.box_sums(levels, np.stack([c[0] for c in cuts]), per_frame))
        pal4 = torch.from_numpy(np.concatenate([pal, np.zeros(pal.shape[:2] + (1,), dtype=np.uint8)], axis=-1)).cuda()
        s = scene(20, 14, 7, seed=30)
        raster, frames, palettes = (torch.from_numpy(s[k]).cuda() for k in ("raster", "frames", "palettes"))

        def run():
            O = G.ops
            out = {"hist": O.gif_histogram(clips, per_frame), "box_sums": O.gif_box_sums(clips, box, per_frame)}
            for dither in (0, 32):
                out[f"map[{dither}]"] = O.gif_map(clips, pal4, n, per_frame, dither)
            out["palette_sums"], out["sse"] = O.gif_palette_sums(clips, pal4, n, per_frame)
            out["diffuse"] = O.gif_diffuse(clips, pal4, n, per_frame)
            for tol in (0, 48):
                for stage in ("map[0]", "diffuse"):
                    d, rects, changed = O.gif_delta(clips, out[stage], pal4, n, per_frame, tolerance=tol)
                    out.update({f"delta[{stage}-{tol}]": d, f"rects[{stage}-{tol}]": rects, f"changed[{stage}-{tol}]": changed})
            out["compose"] = O.gif_compose(raster, frames, palettes, s["W"], s["H"], [0, 2, 3, 6, 6], matte=(9, 8, 7))
            return out
        return run
    return build


case("gif_kernels[per_clip]")(_gif(False))
case("gif_kernels[per_frame]")(_gif(True))


# ----------------------------------------------------------------------------- pooling, preprocessing, row kernels, the ln= prologue
@case("pool_preprocess_rows")
def _others(G):
    from gsdd_amd.data import preprocess
    g = gen(44)
    xin = rn(g, 2, 24, 5, 9, 11)
    rows = xin.permute(0, 2, 3, 4, 1).contiguous().view(-1, 24)
    video = torch.randint(0, 256, (2, 3, 30, 44, 3), generator=g).to(U8).cuda()
    x5 = rn(g, 2, 3, 5, 12, 14)
    M, C, Cout = 37, 72, 40
    x, gamma, beta, w, bias = rn(g, M, C), rn(g, C) + 1, rn(g, C), rn(g, Cout, C, scale=C ** -0.5), rn(g, Cout)

    def run():
        O = G.ops
        out = {}
        k, s_, p = (3, 3, 3), (1, 2, 2), (1, 1, 1)
        grid = (5, 5, 6)
        wide = E(2 * 5 * 5 * 6, 32)
        wide.fill_(7.0)                                                  # the columns outside the slice are the caller's
        O.pool3d(rows, (2, 5, 9, 11), 24, k, s_, p, grid, wide.view(-1)[4:], mode="max", out_pitch=32)
        out["pool_max"] = wide
        mgrid = (4, 3, 5)
        out["pool_mean"] = O.pool3d(rows, (2, 5, 9, 11), 24, (2, 7, 7), (1, 1, 1), (0, 0, 0), mgrid, E(2 * 4 * 3 * 5, 24), mode="mean")
        out["preprocess"] = preprocess(video, 16)
        out["ncdhw_to_rows"] = O.ncdhw_to_rows(x5, 4, 1)
        stats = O.row_stats(x, E(M, 2))
        out["row_stats"] = stats
        out["ln_apply"] = O.ln_apply(x, stats, gamma, beta)
        out["linear_ln"] = O.linear(x, w, E(M, Cout), bias=bias, ln=(stats, gamma, beta, None, 0))
        return out
    return run


# ----------------------------------------------------------------------------- composite: the sampler on d3pm_L64
def _l64(G):
    from tests.conftest import load_golden
    from tests.test_gpu_training import build
    sd, a, cfg = load_golden("d3pm_L64")
    return build(G, sd, cfg).eval(), cfg


def _sampler(kind):
    def build(G):
        B = 8
        dm0, cfg = _l64(G)
        L, K = cfg["L"], cfg["K"]
        g = gen(64)
        cond = rn(g, B, 1, cfg["cond_dim"])
        cf = torch.zeros_like(cond)
        tok = torch.randint(0, K, (B, L), generator=g).cuda()
        known = torch.zeros(L, dtype=torch.bool)
        known[:16] = True
        texts = ["a"] * B

        def run():
            dm = dm0
            dm.transformer._packed = None                # packed weights, AdaLN tables and fragment images are made again, in stale memory
            dm.prior_rule, dm.prior_weight = 0, 0
            dm.set_noise(cfg["noise_seed"], stream=2)
            kw = dict(filter_ratio=0, use_graph=False)
            if kind == "sample":
                out = dm.sample(texts, None, cond, cf, **kw)
            elif kind == "x3p":
                with environ(GSDD_LAYER="x3p"):
                    out = dm.sample(texts, None, cond, cf, **kw)
            elif kind == "fast":
                out = dm.sample_fast(texts, None, cond, skip_step=3, cf_condition_embed=cf, **kw)
            elif kind == "prior2":
                ns = [0] * cfg["T"]
                ns[0], ns[40:61] = 1, [3] * 21          # 21 reveals of three positions, then the ordinary step at t = 0
                dm.prior_rule, dm.prior_weight, dm.n_sample, dm.prior_ps = 2, 1, ns, 64
                out = dm.sample(texts, None, cond, cf, **kw)
            elif kind == "known_resample":
                out = dm.sample(texts, None, cond, cf, content_token=tok, known_mask=known, resample_jump=10, resample_times=2, **kw)
            elif kind == "partial":
                out = dm.sample(texts, None, cond, cf, content_token=tok, filter_ratio=0.5, use_graph=False)
            else:
                t = torch.full((B,), 40, dtype=torch.int64, device="cuda")
                res = {"p_sample_tokens": dm.p_sample_tokens(tok, cond, cf, t, 5)}
                torch.manual_seed(0)                     # (_train_loss draws its timesteps from torch's generator)
                dm.Lt_history.zero_()
                dm.Lt_count.zero_()
                fwd = dm._train_loss(tok, cond, want_probs=True)
                res.update({f"train_loss.{k}": v for k, v in fwd.items() if torch.is_tensor(v)})
                return res
            return {"tokens": out["content_token"]}
        return run
    return build


for _k in ("sample", "x3p", "fast", "prior2", "known_resample", "partial", "single_calls"):
    case(f"sampler[{_k}]")(_sampler(_k))


@case("sampler[Te22-cond_len]")
def _sampler_len(G):
    from tests.test_gpu_condition_len import LENS, SPATIAL
    from tests.test_gpu_training_cond_tokens import NOISE_SEED, make_model
    dm = make_model(SPATIAL)[0].cuda().eval()
    B, Te = len(LENS), 22
    g = gen(22)
    cond, cf = rn(g, B, Te, 512), rn(g, B, Te, 512)

    def run():
        dm.transformer._packed = None
        dm.set_noise(NOISE_SEED, stream=2)
        out = dm.sample(["a"] * B, None, cond, cf, filter_ratio=0, use_graph=False, condition_len=LENS)
        return {"tokens": out["content_token"]}
    return run


# ----------------------------------------------------------------------------- composite: two trainer steps on d3pm_L64
def _trainer(Te):
    def build(G):
        from gsdd_amd.d3pm_train import D3PMTrainer
        dm0, cfg = _l64(G)
        dm0 = dm0.train()
        B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
        g = gen(41 + Te)
        batches = [(torch.randint(0, K, (B, L), generator=g).cuda(), rn(g, B, Te, cfg["cond_dim"]),
                    torch.randint(0, T, (B,), generator=g).cuda(), torch.full((B,), 1.0 / T).cuda()) for _ in range(2)]
        null = torch.randn(77, cfg["cond_dim"], generator=g, dtype=torch.float64)

        def run():
            dm = copy.deepcopy(dm0)
            dm.transformer._packed = None
            if Te > 1:                                   # classifier-free training: the draw on the device against p = 0.5, a learned null row
                dm.learnable_cf, dm.cond_drop_prob = True, 0.5
                dm.empty_text_embed.data = null.clone().to(dm.empty_text_embed.device)
            dm.set_noise(cfg["noise_seed"], stream=3)
            with environ(GSDD_TRAIN_GRAPH="0"):
                tr = D3PMTrainer(dm, lr=1e-3, betas=(0.9, 0.96), deterministic=True, max_grad_norm=0.5, weight_decay=0.05, ema_decay=0.999)
                x0, cond, t, pt = batches[0]
                loss, grads = tr.loss_and_grads(x0, cond, t=t, pt=pt)
                out = {"loss": loss.clone()}
                out.update({f"grad.{k}": v.clone() for k, v in grads.items()})
                dm.set_noise(cfg["noise_seed"], stream=3)
                for x0, cond, t, pt in batches:          # the second step reuses what the first freed
                    tr.step(x0, cond, t=t, pt=pt)
                out.update({f"weight.{n}": p.detach() for n, p in dm.transformer.named_parameters()})
                out.update({f"ema.{n}": v for n, v in tr.ema_state_dict().items()})
                out["grad_norm"] = tr.last_grad_norm.reshape(1)
                if Te > 1:
                    out["null"] = dm.empty_text_embed.detach()
            return out
        return run
    return build


case("trainer[Te1]")(_trainer(1))                   # (the trainer holds the switch itself: deterministic=True)
case("trainer[Te3-dropout]")(_trainer(3))


# ----------------------------------------------------------------------------- composite: VQ-VAE
@case("vqvae[eval]")
def _vqvae_eval(G):
    from tests.conftest import load_golden
    sd, a, cfg = load_golden("vqvae_ds188")
    m = G.VQVAE(None, cfg["embedding_dim"], cfg["n_codes"], cfg["n_hiddens"], cfg["n_res_layers"], cfg["downsample"], cfg["sequence_length"],
                cfg["resolution"])
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = torch.from_numpy(a["x"]).cuda()
    codes = torch.from_numpy(a["encodings"]).cuda()

    def run():
        m._packed = None
        enc, emb = m.encode(x, include_embeddings=True)
        fwd = m({"video": x})
        return {"encode": enc, "encode_plain": m.encode(x), "embeddings": emb, "decode": m.decode(codes), "pred": fwd["pred_data"],
                "recon_loss": fwd["losses"]["recon_loss"].reshape(1), "commitment_loss": fwd["losses"]["commitment_loss"].reshape(1)}
    return run


# Outputs of the VQ-VAE step that have no reproducible form (their two 0x00 runs differ, with and without ops.set_deterministic): the
# weight gradients of the stem and of the last transposed convolution (gsdd_conv_wgrad adds more than two row-block partials per dW
# element with float atomics) and what follows from encode_sum (gsdd_codebook_ema: float atomics per code): the codebook's z_avg and
# embeddings.  They are left out by name, not compared with a tolerance; the kernels themselves are in conv_wgrad[*] and codebook_ema.
VQVAE_NOT_REPRODUCIBLE = ("encoder.convs.0.conv.weight", "decoder.convts.2.convt.weight", "embeddings", "z_avg")


@case("vqvae[train]", deterministic=True)
def _vqvae_train(G):
    from gsdd_amd.vqvae_trainer import VQVAETrainer
    from tests.test_gpu_vqvae_training import build_vqvae, case as vq_case
    x, sd, cfg, perm = vq_case(G, None, "train_ds188")
    x = x.cuda()
    pt = torch.from_numpy(np.asarray(perm))
    m0 = build_vqvae(G, sd, cfg)

    def fresh():
        m = copy.deepcopy(m0)
        m._packed = None
        m.perm_source = lambda n: pt
        return m

    def run():
        m = fresh()
        trainer = VQVAETrainer(m, lr=4e-4, betas=(0.5, 0.999))
        sv, losses = trainer.forward(x)
        grads = trainer.backward(sv)
        out = {f"grad.{k}": v.clone() for k, v in grads.items()}
        out.update({"idx": sv["idx"], "recon_loss": losses["recon_loss"].reshape(1), "commitment_loss": losses["commitment_loss"].reshape(1),
                    "embeddings": m.codebook.embeddings.detach(), "N": m.codebook.N.detach(), "z_avg": m.codebook.z_avg.detach()})
        m2 = fresh()
        VQVAETrainer(m2, lr=4e-4, betas=(0.5, 0.999)).step(x)
        out.update({f"stepped.{k}": v.detach() for k, v in m2.state_dict().items()})
        m3 = fresh()
        with torch.no_grad():                            # the train-mode forward value: BatchNorm on batch statistics, the codebook update
            fwd = m3({"video": x})
        out.update({"nograd.pred": fwd["pred_data"], "nograd.recon": fwd["losses"]["recon_loss"].reshape(1),
                    "nograd.encode": m3.encode(x), "nograd.embeddings": m3.codebook.embeddings.detach()})
        return {k: v for k, v in out.items() if not k.endswith(VQVAE_NOT_REPRODUCIBLE)}
    return run


# ----------------------------------------------------------------------------- composite: CLIP towers, I3D
@case("clip_towers")
def _towers(G):
    from gsdd_amd.text import ClipTextTower
    from gsdd_amd.vision import ClipVisionTower
    from tests.conftest import load_golden
    sd, a, cfg = load_golden("clip_text_small")
    text, ids = ClipTextTower.from_hf_state_dict(sd, cfg["n_head"]).cuda(), torch.from_numpy(a["ids"])
    sd, a, cfg = load_golden("clip_vision_small")
    vision, pixels = ClipVisionTower.from_hf_state_dict(sd, cfg["n_head"]).cuda(), (torch.from_numpy(a["pixels_x32"]).float() / 32).cuda()
    clips = rn(gen(8), 2, 3, 2, 16, 16)

    def run():
        text._buffers, vision._buffers = {}, {}          # the towers' scratch is made again, in stale memory
        return {"text": text(ids), "text_untrimmed": text(ids[:5], trim=False), "vision_pixels": vision.forward_pixels(pixels),
                "vision_clips": vision(clips)}
    return run


@case("i3d")
def _i3d(G):
    from tests.test_oracle_golden import i3d_fixture
    z, sd = i3d_fixture()
    m = G.InceptionI3d()
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = rn(gen(5), 1, 3, 16, 224, 224)                   # the smallest clip the average pool accepts

    def run():
        m._packed = None
        return {"logits": m(x)}
    return run


# ----------------------------------------------------------------------------- composite: GIF export and reading
@case("gif_files")
def _gif_files(G):
    import tempfile

    import gif_ref
    from src.datamodules.gif_folder_datamodule import GifFolderDataModule
    levels = np.concatenate([gif_ref.synthetic_levels(False), gif_ref.synthetic_levels(True)])
    clips = torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda()

    def run():
        out = {}
        with tempfile.TemporaryDirectory() as tmp:
            paths = [os.path.join(tmp, "data", "test", "synthetic", f"{name}.gif") for name in ("clean", "noisy")]
            idx, pal, n = G.gif.write_gifs(clips, paths, fps=8, refine=2, dither="fs", optimize=True, tolerance=48)
            out.update({"indices": idx, "palette": pal, "n_colors": n})
            for name, path in zip(("clean", "noisy"), paths):
                with open(path, "rb") as f:
                    out[f"file[{name}]"] = f.read()
            dm = GifFolderDataModule(os.path.join(tmp, "data"), sequence_length=4, resolution=16, batch_size=2, frames_between_clips=4,
                                     device="cuda")
            for b, batch in enumerate(dm.test_dataloader()):
                out[f"video[{b}]"] = batch["video"]
        return out
    return run


# ----------------------------------------------------------------------------- the tests (below the cases: CASES is complete here)
@pytest.mark.parametrize("cid", sorted(CASES))
def test_no_output_depends_on_stale_memory(cid):
    assert_clean(cid, run_case(cid))


def test_the_harness_sees_a_stale_read_on_the_device():
    """the fill reaches device memory before the first kernel reads it: a sum into uncleared scratch, a maximum and a count over a partly
    written buffer, in plain torch on the device, are exposed by the bytes tests/test_stale_memory_host.py derives"""
    x = torch.tensor([0.5, 2.0, 1.25, 3.0, 0.75], device="cuda")

    def run():
        acc, buf, count = E(1), E(8), E(3, dtype=torch.int32)
        acc += x.sum()
        buf[:5] = x
        count += 1
        clean = E(8)
        clean[:5] = x
        clean[5:] = 0
        return {"sum": acc, "max": torch.fmax(buf[:4], buf[4:]).amax(), "count": count, "clean": clean.sum()}
    unstable, by_byte, _ = sm.verdict(sm.sweep(run))
    assert unstable == [] and by_byte == {0xFF: ["count", "sum"], 0x7F: ["count", "max", "sum"], 0xFE: ["count", "sum"]}


def test_every_ledger_case_exists():
    ids = {i for v in SITES.values() for i in v}
    assert ids <= set(CASES), sorted(ids - set(CASES))


def test_the_deterministic_switch_is_off_after_the_cases():
    import gsdd_amd
    assert gsdd_amd.ops.set_deterministic(False) is False
