#!/usr/bin/env python3
"""Generate tests/golden/known_L64.npz: the REFERENCE's sample() with positions whose clean tokens are given (frame prediction /
interpolation / inpainting) on the d3pm_L64 construction (K 32, L 64, T 100, B 2, the same weights: they are not stored again).

Runs only where the reference checkout is (see make_golden.py, whose stubs and build_d3pm are used); the reference is imported
read-only, bytecode writing off.  This file states the rule once, with the reference's own functions:

  * x_known (B, L) codes in [0, K) and known (B, L) bool.  Row 0 of the mask is the first 16 positions (the first frame of a 4 x 4 x 4
    grid), row 1 a seeded Bernoulli(0.5) scatter.
  * the chain is the reference's own sample() from all-[MASK], t = T-1 ... 0, one (B, K+1, L) uniform draw per step.
  * unknown positions: nothing changes.
  * known positions, "renoise": the reference's p_pred is wrapped so that model_log_prob there is the reference's own
    q_pred(log_onehot(x_known), t - 1) -- with its mod (T + 1) wrap, so the level at t = 0 is index T (alpha-bar 1, gamma-bar 0) and the
    draw returns x_known -- and log_sample_categorical draws from it with the same uniforms of that position.
  * known positions, "hold": the p_sample result is overwritten there with x_known.

torch.rand_like is replaced by the (B, K+1, L) Philox draw of oracle/philox.py uniform_bkl, one stream per step, which a device can
regenerate.  Per step and position the file records the gap between the two best Gumbel + log-probability values of the draw the
position actually used (inf where none was made: hold).  A device test leaves out positions whose gap is under GAP_FLOOR; this
generator asserts that those are at most MAX_LEFT_OUT of all positions.

Besides the two traces: the denoiser's two logit tensors of the first call (all [MASK], t = T - 1: the same in both modes) and one
mid-chain call at step index 50 per mode (x_t = trace[49], t = 49, both logit tensors; the expected tokens are trace[50]).

Usage:  python tests/golden/make_golden_known.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg
from oracle import philox

K, L, T, B = 32, 64, 100, 2
NOISE_SEED = 1234
MASK_SEED = 77          # x_known and the scatter row of the mask
MID_STEP = 50
GAP_FLOOR = 1e-3        # 50 x the 2e-5 the step-kernel tests allow between device and oracle log-probabilities
MAX_LEFT_OUT = 0.05
MODES = ("renoise", "hold")


def known_inputs():
    g = torch.Generator().manual_seed(MASK_SEED)
    x_known = torch.randint(0, K, (B, L), generator=g)
    known = torch.zeros(B, L, dtype=torch.bool)
    known[0, :16] = True
    known[1] = torch.rand(L, generator=g) < 0.5
    return x_known, known


def run_chain(dm, dt_mod, mode, x_known, known, cond, cf_cond):
    state = {"stream": 0}
    rec = {"gap": [], "trace": []}
    orig_p_pred, orig_lsc, orig_p_sample = dm.p_pred, dm.log_sample_categorical, dm.p_sample
    kn = known[:, None, :]
    log_x_known = dt_mod.index_to_log_onehot(x_known, K + 1)

    def p_pred(log_x, cond_emb, cf_cond_emb, t):
        model_log_prob, log_x_recon = orig_p_pred(log_x, cond_emb, cf_cond_emb, t)
        if mode == "renoise":
            model_log_prob = torch.where(kn, dm.q_pred(log_x_known, t - 1), model_log_prob)
        return model_log_prob, log_x_recon

    def rand_like(x, **kw):
        Bx, K1, Lx = x.shape
        u = philox.uniform_bkl(NOISE_SEED, state["stream"], Bx, K1, Lx)
        state["stream"] += 1
        return torch.from_numpy(u).to(x.dtype)

    def lsc(logits):
        u = philox.uniform_bkl(NOISE_SEED, state["stream"], *logits.shape)
        v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + logits.numpy()).astype(np.float32), axis=1)
        gap = v[:, -1, :] - v[:, -2, :]
        if mode == "hold":
            gap = np.where(known.numpy(), np.float32(np.inf), gap)
        rec["gap"].append(gap.astype(np.float32))
        return orig_lsc(logits)

    def p_sample(*a, **k):
        out, sampled = orig_p_sample(*a, **k)
        idx = dt_mod.log_onehot_to_index(out)
        if mode == "hold":
            idx = torch.where(known, x_known, idx)
            out = dt_mod.index_to_log_onehot(idx, K + 1)
        rec["trace"].append(idx.numpy().astype(np.int8))
        return out, sampled

    dm.p_pred, dm.log_sample_categorical, dm.p_sample = p_pred, lsc, p_sample
    keep = torch.rand_like
    torch.rand_like = rand_like
    try:
        with torch.no_grad():
            res = dm.sample(["a"] * B, None, cond, cf_cond, content_token=None, filter_ratio=0)
    finally:
        torch.rand_like = keep
        dm.p_pred, dm.log_sample_categorical, dm.p_sample = orig_p_pred, orig_lsc, orig_p_sample
    tokens = res["content_token"].numpy()
    trace, gap = np.stack(rec["trace"]), np.stack(rec["gap"])
    assert trace.shape == gap.shape == (T, B, L) and state["stream"] == T
    assert np.array_equal(trace[-1], tokens) and int((tokens == K).sum()) == 0
    return trace, gap, tokens


def main():
    mg.install_stubs()
    import src.models.motionencoder.diffusion_transformer as dt_mod

    base = np.load(os.path.join(mg.OUT, "d3pm_L64.npz"))
    assert (int(base["cfg_K"]), int(base["cfg_L"]), int(base["cfg_T"]), int(base["cfg_B"])) == (K, L, T, B)
    dm = mg.build_d3pm(K, L, [8, 8], int(base["cfg_n_layer"]), int(base["cfg_cond_dim"]), T, seed=21)
    for k, v in dm.state_dict().items():
        if "sd/" + k in base.files and not k.startswith("Lt_"):       # (the fixture's training step has updated Lt_history / Lt_count)
            assert np.array_equal(v.numpy(), base["sd/" + k]), k          # the weights of d3pm_L64.npz
    cond = torch.from_numpy(base["step_cond"])
    cf_cond = torch.zeros_like(cond)
    dm.prior_rule = 0
    x_known, known = known_inputs()
    assert int(x_known.min()) >= 0 and int(x_known.max()) < K

    out = {"x_known": x_known.numpy().astype(np.int8), "known": known.numpy()}
    shares = {}
    for mode in MODES:
        trace, gap, tokens = run_chain(dm, dt_mod, mode, x_known, known, cond, cf_cond)
        kn = known.numpy()
        assert np.array_equal(tokens[kn], x_known.numpy()[kn])            # both modes end on the clean tokens
        left_out = gap < GAP_FLOOR
        shares[mode] = float(left_out.mean())
        print("%s: left out %.3f %% of %d positions (known: %d of %d draws); [MASK] share of the known positions at steps 0 / 50 / 98: "
              "%.2f / %.2f / %.2f" % (mode, 100 * shares[mode], left_out.size, int(left_out[:, kn].sum()), int(kn.sum()) * T,
                                      (trace[0][kn] == K).mean(), (trace[50][kn] == K).mean(), (trace[98][kn] == K).mean()))
        assert shares[mode] <= MAX_LEFT_OUT, shares[mode]
        out.update({f"trace_{mode}": trace, f"gap_{mode}": gap, f"tokens_{mode}": tokens.astype(np.int8)})
        # the mid-chain call: the denoiser's logits on the chain's own x_t
        with torch.no_grad():
            xt = torch.from_numpy(trace[MID_STEP - 1].astype(np.int64))
            tm = torch.full((B,), T - 1 - MID_STEP, dtype=torch.long)
            out[f"mid_xt_{mode}"] = trace[MID_STEP - 1]
            out[f"mid_logits_{mode}"] = dm.transformer(xt.clone(), cond, tm).numpy()             # (B, K, L)
            out[f"mid_logits_uncond_{mode}"] = dm.transformer(xt.clone(), cf_cond, tm).numpy()
            out[f"mid_tokens_{mode}"] = trace[MID_STEP]
    assert not np.array_equal(out["trace_renoise"], out["trace_hold"])
    out["mid_t"] = np.int64(T - 1 - MID_STEP)
    # the denoiser's logits of the first call (all [MASK], t = T - 1): the step kernel's input, the same in both modes
    with torch.no_grad():
        xt0, t0 = torch.full((B, L), K, dtype=torch.long), torch.full((B,), T - 1, dtype=torch.long)
        out["first_logits"] = dm.transformer(xt0.clone(), cond, t0).numpy()
        out["first_logits_uncond"] = dm.transformer(xt0.clone(), cf_cond, t0).numpy()
    out.update({"cfg_noise_seed": NOISE_SEED, "cfg_mask_seed": MASK_SEED, "cfg_mid_step": MID_STEP, "cfg_gap_floor": GAP_FLOOR,
                "cfg_max_left_out": MAX_LEFT_OUT, "cfg_left_out_renoise": shares["renoise"], "cfg_left_out_hold": shares["hold"],
                "cfg_base": "d3pm_L64"})
    path = os.path.join(mg.OUT, "known_L64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
