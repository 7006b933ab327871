#!/usr/bin/env python3
"""Generate tests/golden/truncation_L64.npz: the REFERENCE's sample() with top-r truncated sampling (VQ-Diffusion's
predict_start_with_truncation, "top0.86r") on the d3pm_L64 construction (K 32, L 64, T 100, B 2, the same weights: they are not stored
again).

Runs only where the reference checkout is (see make_golden.py, whose stubs and build_d3pm are used); the reference is imported
read-only, bytecode writing off.  The reference fork dropped upstream's wrapper but kept what it wraps: here its own cf_predict_start is
wrapped with the rule as tests/test_truncation_host.py restates it (class k kept iff the mass strictly above it is below r, cut entries
-70, no renormalisation) and its own sample() runs the 100 steps.  torch.rand_like is replaced by the (B, K+1, L) Philox draw of
oracle/philox.py uniform_bkl, one stream per step, which a device can regenerate.

Per step and position the file records how close the reference's own decision was to flipping: the boundary margin
min_k |mass_above(k) - r| of the row that was truncated and the gap between the two best Gumbel + log-probability values of the draw.
A device test leaves out positions whose margin is under MARGIN_FLOOR or whose gap is under GAP_FLOOR; this generator asserts that
those are at most MAX_LEFT_OUT of all positions.

Usage:  python tests/golden/make_golden_truncation.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg
from oracle import philox

_spec = importlib.util.spec_from_file_location("truncation_rule", os.path.join(os.path.dirname(HERE), "test_truncation_host.py"))
_rule = importlib.util.module_from_spec(_spec)      # (by path: the reference checkout has a `tests` package of its own)
_spec.loader.exec_module(_rule)
boundary_margin, truncate_rows = _rule.boundary_margin, _rule.truncate_rows

K, L, T, B = 32, 64, 100, 2
RATE = 0.86
NOISE_SEED = 1234
MARGIN_FLOOR = 1e-4     # 5 x the cumulative-mass error a 2e-5 log-probability error can cause (the mass is at most 1)
GAP_FLOOR = 1e-3        # 50 x the 2e-5 the step-kernel tests allow between device and oracle log-probabilities
MAX_LEFT_OUT = 0.05


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

    state = {"stream": 0}
    rec = {"rows": [], "margin": [], "gap": [], "trace": []}
    orig_cf, orig_lsc, orig_p_sample = dm.cf_predict_start, dm.log_sample_categorical, dm.p_sample

    def cf_predict_start(*a, **k):                      # upstream: predict_start_with_truncation(self.cf_predict_start, "top0.86r")
        out = orig_cf(*a, **k).numpy()
        rec["margin"].append(boundary_margin(out, RATE).astype(np.float32))
        cut = truncate_rows(out, RATE)
        rec["rows"].append(cut)
        return torch.from_numpy(cut)

    def rand_like(x, **kw):
        Bx, K1, Lx = x.shape
        u = philox.uniform_bkl(NOISE_SEED, state["stream"], Bx, K1, Lx)
        state["stream"] += 1
        return torch.from_numpy(u).to(x.dtype)

    def lsc(logits):
        u = philox.uniform_bkl(NOISE_SEED, state["stream"], *logits.shape)
        v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + logits.numpy()).astype(np.float32), axis=1)
        rec["gap"].append(v[:, -1, :] - v[:, -2, :])
        return orig_lsc(logits)

    def p_sample(*a, **k):
        r = orig_p_sample(*a, **k)
        rec["trace"].append(dt_mod.log_onehot_to_index(r[0]).numpy().astype(np.int8))
        return r

    dm.cf_predict_start, dm.log_sample_categorical, dm.p_sample = cf_predict_start, lsc, p_sample
    keep = torch.rand_like
    torch.rand_like = rand_like
    try:
        with torch.no_grad():
            res = dm.sample(["a"] * B, None, cond, cf_cond, content_token=None, filter_ratio=0)
    finally:
        torch.rand_like = keep
        dm.cf_predict_start, dm.log_sample_categorical, dm.p_sample = orig_cf, orig_lsc, orig_p_sample
    tokens = res["content_token"].numpy()
    trace, margin, gap = np.stack(rec["trace"]), np.stack(rec["margin"]), np.stack(rec["gap"]).astype(np.float32)
    assert trace.shape == margin.shape == gap.shape == (T, B, L) and state["stream"] == T
    assert np.array_equal(trace[-1], tokens) and int((tokens == K).sum()) == 0
    left_out = (margin < MARGIN_FLOOR) | (gap < GAP_FLOOR)
    share = float(left_out.mean())
    print("left out: %.3f %% of %d positions (margin < %g: %d, gap < %g: %d); first call: min margin %.3g, %d of %d rows within 1e-3"
          % (100 * share, left_out.size, MARGIN_FLOOR, int((margin < MARGIN_FLOOR).sum()), GAP_FLOOR, int((gap < GAP_FLOOR).sum()),
             margin[0].min(), int((margin[0] < 1e-3).sum()), margin[0].size))
    assert share <= MAX_LEFT_OUT, share
    assert margin[0].min() >= MARGIN_FLOOR              # the first call's rows are compared whole (kept sets must be equal)

    out = {"first_rows": rec["rows"][0].astype(np.float32), "trace": trace, "tokens": tokens.astype(np.int8), "margin": margin, "gap": gap}
    # the denoiser's logits of the first call (all [MASK], t = T - 1): the step kernel's input
    with torch.no_grad():
        xt0, t0 = torch.full((B, L), K, dtype=torch.long), torch.full((B,), T - 1, dtype=torch.long)
        out["first_logits"] = dm.transformer(xt0.clone(), cond, t0).numpy()                 # (B, K, L)
        out["first_logits_uncond"] = dm.transformer(xt0.clone(), cf_cond, t0).numpy()
    kept = out["first_rows"][:, :-1] > -70
    print("first call: classes kept per row min %d / mean %.1f / max %d of %d" % (kept.sum(1).min(), kept.sum(1).mean(), kept.sum(1).max(), K))
    out.update({"cfg_rate": RATE, "cfg_noise_seed": NOISE_SEED, "cfg_margin_floor": MARGIN_FLOOR, "cfg_gap_floor": GAP_FLOOR,
                "cfg_max_left_out": MAX_LEFT_OUT, "cfg_left_out": share, "cfg_base": "d3pm_L64"})
    path = os.path.join(mg.OUT, "truncation_L64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
