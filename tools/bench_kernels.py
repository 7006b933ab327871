#!/usr/bin/env python3
"""Micro-benchmarks of the hot kernels at the C3 workload shapes (HIP events on the launch stream)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsdd_amd  # noqa: E402
from gsdd_amd import ops  # noqa: E402


def timeit(fn, iters=10, warm=2):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    e0, e1 = ops.Event(), ops.Event()
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    return e0.elapsed_ms(e1) / iters


def main():
    which = sys.argv[1:] or ["attn", "gemm", "layer", "logits", "step"]
    dev = "cuda"
    # the first measurement of a process otherwise runs at the idle clock: the power state takes far longer than timeit's two warm
    # calls to ramp up (measured: the same kernel 1.14 ms as the first case of a run, 0.98 ms as the third)
    wa = torch.randn((8192, 8192), device=dev)
    for _ in range(60):
        wa = (wa @ wa).clamp_(-1, 1)
    torch.cuda.synchronize()
    del wa
    B2, L, H, D, K = 32, 4096, 16, 64, 4096
    M = B2 * L
    if "attn" in which:
        q = torch.randn((3 * H, M, 4), device=dev)
        out = torch.empty((M, H * 4), device=dev)
        aws = ops.d3pm_attention_workspace(B2, L, H, dev)
        fl = 16.0 * L * L * H * B2
        for scale in [float(v) for v in os.environ.get("GSDD_BENCH_SCALES", "0.05,1,2,3").split(",")]:      # 0.05: flat softmax rows (the N(0, 0.02) init); 1: trained-like; 2, 3: peaky
            qs = q * scale
            ops.d3pm_attention(qs[0:H], qs[H:2 * H], qs[2 * H:], B2, L, H, out, ws=aws)      # pre-split images made once
            for pbits in os.environ.get("GSDD_BENCH_PMODES", "22,11,a8,a12").split(","):
                os.environ["GSDD_ATTN_P"] = pbits
                ms = timeit(lambda: ops.d3pm_attention(qs[0:H], None, None, B2, L, H, out, ws=aws))
                print(f"attention  B2={B2} L={L} q,k x{scale:g} P{pbits}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s ({fl / ms / 1e9 / 157.3 * 100:.1f}% of f32 MFMA peak)")
        os.environ.pop("GSDD_ATTN_P", None)
    if "attnbwd" in which:
        Bt = 16
        Mt = Bt * L
        qkv = torch.randn((3 * H, Mt, 4), device=dev)
        o = torch.empty((Mt, H * 4), device=dev)
        lse = torch.empty((H * Mt,), device=dev)
        dO = torch.randn((Mt, H * 4), device=dev)
        ops.d3pm_attention_train(qkv[0:H], qkv[H:2 * H], qkv[2 * H:], Bt, L, H, o, lse, ws=ops.d3pm_attention_workspace(Bt, L, H, dev))
        ws = ops.d3pm_attention_bwd_workspace(Bt, L, H, dev)
        fl = 40.0 * L * L * H * Bt
        variants = (("fused", None), ("fused no-LDS-acc", "dbg1"), ("fused no-dQ", "dbg2"), ("split", "split"))
        if os.environ.get("GSDD_BENCH_BWD_VARIANTS"):      # e.g. "fused": the counter passes want the shipped variant alone
            keep = os.environ["GSDD_BENCH_BWD_VARIANTS"].split(",")
            variants = tuple(v for v in variants if v[0] in keep)
        for name, variant in variants:
            ms = timeit(lambda: ops.d3pm_attention_bwd(qkv[0:H], qkv[H:2 * H], qkv[2 * H:], o, dO, lse, Bt, L, H, ws=ws, variant=variant), iters=5)
            print(f"attention bwd B={Bt} L={L} {name}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s")
    if "wgrad" in which:
        Mt = 16 * L
        for (n, k) in [(64, 64), (192, 64), (256, 64), (64, 256), (4096, 64)]:
            dY = torch.randn((Mt, n), device=dev); X = torch.randn((Mt, k), device=dev)
            dW = torch.zeros((n, k), device=dev); db = torch.zeros((n,), device=dev)
            ms = timeit(lambda: ops.wgrad(dY, X, dW, db))
            dW3 = torch.zeros((1, n, k), device=dev)
            ms2 = timeit(lambda: ops.conv_wgrad(X, dY, dW3, in_dims=(1, 1, 1, Mt), out_grid=(1, 1, Mt), cin=k, cout=n))
            fl = 2.0 * Mt * n * k
            print(f"wgrad M={Mt} N={n} K={k}: f32 kernel {ms * 1e3:.1f} us ({fl / ms / 1e9:.1f} TFLOP/s)   conv_wgrad (bf16x3) {ms2 * 1e3:.1f} us "
                  f"({fl / ms2 / 1e9:.1f} TFLOP/s)")
    if "gemm" in which:
        x = torch.randn((M, D), device=dev)
        stats = torch.empty((M, 2), device=dev)
        g = torch.randn((100, 2 * D), device=dev)
        t2 = torch.full((B2,), 50, dtype=torch.int64, device=dev)
        for (name, cin, cout, ln, act, mode, res) in [("qkv", 64, 192, True, 0, 2, False), ("proj", 64, 64, False, 0, 0, True),
                                                      ("mlp1", 64, 256, True, 2, 0, False), ("mlp2", 256, 64, False, 0, 0, True),
                                                      ("logits", 64, K, True, 0, 0, False)]:
            w = torch.randn((cout, cin), device=dev) * 0.05
            b = torch.randn((cout,), device=dev)
            a = torch.randn((M, cin), device=dev)
            o = torch.empty((M, cout), device=dev)
            r = torch.randn((M, cout), device=dev) if res else None
            lnarg = (stats, g.view(-1), g.view(-1)[D:], t2, 2 * D) if ln else None
            ops.row_stats(x, stats)
            ms = timeit(lambda: ops.linear(a, w, o, bias=b, ln=lnarg, rows_per_batch=L, act=act, residual=r, out_mode=mode))
            fl = 2.0 * M * cin * cout
            by = 4.0 * M * (cin + cout * (2 if res else 1))
            print(f"gemm {name:7s} {cin}->{cout}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s  {by / ms / 1e6:.0f} GB/s")
        ms = timeit(lambda: ops.row_stats(x, stats))
        print(f"row_stats: {ms:.3f} ms  {4.0 * M * D / ms / 1e6:.0f} GB/s")
    if "layer" in which:
        d = gsdd_amd.DalleMaskImageEmbedding(num_embed=K, spatial_size=[64, 64], embed_dim=64)
        tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                            content_spatial_size=[64, 64], diffusion_step=100).cuda()
        p = tr.packed()
        for lay in p["layers"]:               # weight fragment images (the sampler makes them on first use): f16 hi + lo, or GSDD_LAYER=x3p
            if os.environ.get("GSDD_LAYER") == "x3p":
                lay["w2_x3"], lay["wqkv_x3"] = ops.d3pm_layer_pack(lay["w2"], lay["wproj"], lay["wqkv"])
            else:
                lay["lay_h2"], lay["wqkv_h2"] = ops.d3pm_layer_pack_h2(lay["w1"], lay["w2"], lay["wproj"], lay["wqkv"])
        # the full batch (2B = 32 rows of L) and one sampler lane's half of it (M = 65536)
        for B2l in [int(v) for v in os.environ.get("GSDD_LAYER_B2", f"{B2},{B2 // 2}").split(",")]:
            Ml = B2l * L
            x = torch.randn((Ml, D), device=dev); y = torch.randn((Ml, D), device=dev)
            qkv = torch.empty((3 * H, Ml, 4), device=dev)
            cv = torch.randn((B2l, D), device=dev)
            t2 = torch.full((B2l,), 50, dtype=torch.int64, device=dev)
            ms = timeit(lambda: ops.d3pm_layer(y, x, L, p["layers"][0], cvec=cv, nxt=p["layers"][1], t2=t2, qkv=qkv))
            fl = 2.0 * Ml * (64 * 64 + 2 * 64 * 256 + 64 * 192)
            print(f"M={Ml} fused layer (proj+mlp+next qkv): {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s")
            aws = ops.d3pm_attention_workspace(B2l, L, H, dev)
            ms = timeit(lambda: ops.d3pm_layer(y, x, L, p["layers"][0], cvec=cv, nxt=p["layers"][1], t2=t2, qkv=qkv, kv_img=aws))
            print(f"M={Ml} fused layer (proj+mlp+next q, K/V images): {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s")
            ms = timeit(lambda: ops.d3pm_layer(y, x, L, p["layers"][0], cvec=cv))
            fl = 2.0 * Ml * (64 * 64 + 2 * 64 * 256)
            print(f"M={Ml} fused layer (proj+mlp, last):    {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s")
    if "logits" in which:
        x = torch.randn((M, D), device=dev)
        w = torch.randn((K, D), device=dev) * 0.05
        b = torch.randn((K,), device=dev); g = torch.randn((D,), device=dev); bt = torch.randn((D,), device=dev)
        o = torch.empty((M, K), device=dev)
        ms = timeit(lambda: ops.d3pm_logits(x, g, bt, w, b, o))
        print(f"logits kernel 64->{K}: {ms:.3f} ms  {2.0 * M * D * K / ms / 1e9:.1f} TFLOP/s  {4.0 * M * K / ms / 1e6:.0f} GB/s written")
    if "conv" in which:
        # VQ-VAE shapes at C2 (C = 256), batch 8
        from gsdd_amd.vqvae import conv_taps, convT_phases
        Bc, C_ = 8, 256
        f = dict(dtype=torch.float32, device=dev)

        def report(name, ms, fl):
            print(f"{name:34s}: {ms:8.3f} ms  {fl / ms / 1e9:6.1f} TFLOP/s ({fl / ms / 1e9 / 157.3 * 100:.1f}% of f32 MFMA peak)", flush=True)
        Mrows = Bc * 16 * 32 * 32
        a = torch.randn((Mrows, 4096), **f); w = torch.randn((1, C_, 4096), **f) * 0.02; o = torch.empty((Mrows, C_), **f)
        ms = timeit(lambda: ops.gemm(a, w, o, in_dims=(1, 1, 1, Mrows), out_grid=(1, 1, Mrows)), iters=5)
        report("plain gemm M=131072 K=4096 N=256", ms, 2.0 * Mrows * 4096 * C_)
        del a
        # conv1: (16,64,64)x256 -> (16,32,32)x256, k4 s(1,2,2)
        x = torch.randn((Bc * 16 * 64 * 64, C_), **f)
        taps = ops.taps_tensor(conv_taps((4, 4, 4), (1, 2, 2), (2, 1, 1)), dev)
        w = torch.randn((64, C_, C_), **f) * 0.02
        o = torch.empty((Mrows, C_), **f)
        bias = torch.randn((C_,), **f)
        ms = timeit(lambda: ops.gemm(x, w, o, in_dims=(Bc, 16, 64, 64), out_grid=(16, 32, 32), stride=(1, 2, 2), taps=taps, ntaps=64,
                                     epi_shift=bias, act=ops.ACT_RELU), iters=5)
        report("conv1 k4 s(1,2,2) 256->256", ms, 2.0 * Mrows * 64 * C_ * C_)
        dW = torch.zeros_like(w)
        dY = torch.randn((Mrows, C_), **f)
        ms = timeit(lambda: ops.conv_wgrad(x, dY, dW, in_dims=(Bc, 16, 64, 64), out_grid=(16, 32, 32), stride=(1, 2, 2), taps=taps,
                                           ntaps=64, cin=C_, cout=C_), iters=5)
        report("conv1 wgrad", ms, 2.0 * Mrows * 64 * C_ * C_)
        del x, dY
        # res-block conv3: 27 taps 256 -> 128 with BN+ReLU prologue on the latent grid
        Ml = Bc * 16 * 16 * 16
        h = torch.randn((Ml, C_), **f)
        w3 = torch.randn((27, C_ // 2, C_), **f) * 0.02
        t3 = ops.taps_tensor(conv_taps((3, 3, 3), (1, 1, 1), (1, 1, 1)), dev)
        pro = (torch.rand((C_,), **f) + 0.5, torch.randn((C_,), **f) * 0.1)
        o3 = torch.empty((Ml, C_ // 2), **f)
        ms = timeit(lambda: ops.gemm(h, w3, o3, in_dims=(Bc, 16, 16, 16), out_grid=(16, 16, 16), taps=t3, ntaps=27, pro=pro))
        report("res conv3 27 taps 256->128 (pro)", ms, 2.0 * Ml * 27 * C_ * C_ // 2)
        wq = torch.randn((1, 9 * C_, C_), **f) * 0.02
        oq = torch.empty((Ml, 9 * C_), **f)
        ms = timeit(lambda: ops.gemm(h, wq, oq, in_dims=(Bc, 16, 16, 16), out_grid=(16, 16, 16), pro=pro))
        report("res qkv 1x1 256->2304 (pro)", ms, 2.0 * Ml * 9 * C_ * C_)
        # convT1 phases: (16,32,32) -> (16,64,64), 4 phases x 16 taps
        xin = torch.randn((Mrows, C_), **f)
        out = torch.empty((Bc * 16 * 64 * 64, C_), **f)
        phases = convT_phases((4, 4, 4), (1, 2, 2), (2, 1, 1))
        pw = [(ph, torch.randn((len(ks), C_, C_), **f) * 0.02, ops.taps_tensor(offs, dev)) for ph, ks, offs in phases]

        def convT():
            for ph, wph, tp in pw:
                ops.gemm(xin, wph, out, in_dims=(Bc, 16, 32, 32), out_grid=(16, 32, 32), taps=tp, ntaps=wph.shape[0], epi_shift=bias,
                         act=ops.ACT_RELU, out_dims=(16, 64, 64), out_step=(1, 2, 2), out_off=ph)
        ms = timeit(convT, iters=5)
        report("convT1 (4 phases x 16 taps)", ms, 2.0 * Mrows * 64 * C_ * C_)
        # last convT: 256 -> 3, NCDHW output
        xin2 = out
        out3 = torch.empty((Bc, 3, 16, 128, 128), **f)
        pw3 = [(ph, torch.randn((len(ks), 3, C_), **f) * 0.02, ops.taps_tensor(offs, dev)) for ph, ks, offs in phases]
        b3 = torch.randn((3,), **f)

        def convT3():
            for ph, wph, tp in pw3:
                ops.gemm(xin2, wph, out3, in_dims=(Bc, 16, 64, 64), out_grid=(16, 64, 64), taps=tp, ntaps=wph.shape[0], epi_shift=b3,
                         out_dims=(16, 128, 128), out_step=(1, 2, 2), out_off=ph, out_mode=1)
        ms = timeit(convT3, iters=5)
        report("convT2 256->3 (4 phases x 16 taps)", ms, 2.0 * Bc * 16 * 64 * 64 * 64 * C_ * 3)
        zz = torch.randn((Ml, 128), **f); cb = torch.randn((4096, 128), **f)
        idx = torch.empty((Ml,), dtype=torch.int64, device=dev)
        ms = timeit(lambda: ops.nearest_code(zz, cb, idx))
        report("nearest_code 32768 x 4096 x 128", ms, 2.0 * Ml * 4096 * 128)
    if "step" in which:
        Bs = B2 // 2
        for Ks in [int(v) for v in os.environ.get("GSDD_STEP_K", str(K)).split(",")]:
            Mh = Bs * L
            logits = torch.randn((2 * Mh, Ks), device=dev)
            tok = torch.randint(0, Ks + 1, (Bs, L), device=dev)
            t = torch.full((B2,), 50, dtype=torch.int64, device=dev)
            sid = torch.zeros(1, dtype=torch.int64, device=dev)
            d = gsdd_amd.DalleMaskImageEmbedding(num_embed=Ks, spatial_size=[64, 64], embed_dim=64)
            tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=1, n_embd=64, n_head=16, content_seq_len=L, block_activate="GELU2",
                                                content_spatial_size=[64, 64], diffusion_step=100)
            dm = gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2,
                                               content_seq_len=L).cuda()
            ms = timeit(lambda: ops.d3pm_step(logits[:Mh], logits[Mh:], tok, tok, dm._sched(), t, sid, K=Ks, T=100, guidance=2.0, seed=1))
            by = 2.0 * Mh * Ks * 4
            print(f"d3pm_step B={Bs} K={Ks}: {ms:.3f} ms  {by / ms / 1e6:.0f} GB/s algorithmic  {ms * 1e6 / (Mh * Ks) * 1e3:.2f} ps/element")
            del logits

    if "nearest" in which:
        for Mn in [int(v) for v in os.environ.get("GSDD_NEAREST_M", "32768,262144").split(",")]:    # C2 at bs 8 and at bs 64
            z = torch.randn((Mn, 128), device=dev)
            cb = torch.randn((4096, 128), device=dev)
            idx = torch.empty((Mn,), dtype=torch.int64, device=dev)
            fl = 2.0 * Mn * 4096 * 128
            for name, mat in (("matrix cores", True), ("vector kernel", False)):
                ms = timeit(lambda: ops.nearest_code(z, cb, idx, None, matrix=mat))
                print(f"nearest_code M={Mn} K=4096 E=128 {name}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s ({fl / ms / 1e9 / 157.3 * 100:.1f}% of f32 MFMA peak)")


if __name__ == "__main__":
    main()
