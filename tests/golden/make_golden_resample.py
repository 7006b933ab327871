#!/usr/bin/env python3
"""Generate tests/golden/resample_L64.npz: known-token conditioned sampling with RePaint's resampling jumps, computed by the REFERENCE's
own functions on the d3pm_L64 construction (K 32, L 64, T 100, B 2, the same weights: they are not stored again) with the known
positions of make_golden_known.py.

Runs only where the reference checkout is (see make_golden.py, whose stubs and build_d3pm are used); the reference is imported
read-only, bytecode writing off.  The chain is `resample_plan(T, jump, times)`:

  * ("step", t): the reference's own p_sample at t from the current log-one-hot state, with the known-position wrapping of
    make_golden_known.py ("renoise": model_log_prob at a known position is the reference's q_pred(log_onehot(x_known), t - 1);
    "hold": the result is overwritten there with x_known).
  * ("jump", a): every position moves forward from level a to b = a + jump by the rule stated here once, in fp64, from the cumulative
    arrays of the reference's alpha_schedule (index -1 = T: abar 1, gbar 0):
        alpha~ = abar_b / abar_a,  gamma~ = (gbar_b - gbar_a) / (1 - gbar_a),  beta~ = (1 - alpha~ - gamma~) / K;
        [MASK] stays [MASK]; a code i goes to [MASK] with gamma~, stays i with alpha~ + beta~, to any other code with beta~ each.
    The log-probabilities are cast to f32 and drawn by the reference's log_sample_categorical.  A [MASK] input has one class of
    probability 1 (no draw is recorded for it); in "hold" mode the known positions are copied through, in "renoise" mode they jump
    like every other position.
  * every op draws from its own (B, K+1, L) Philox stream, in order of execution (torch.rand_like replaced by oracle/philox.py
    uniform_bkl, which a device can regenerate).

Two chains: "renoise" with jump 10, times 2 (190 steps, 9 jumps) and "hold" with jump 30, times 3 (280 steps, 6 jumps).  Per op the
file stores the tokens after it (int8) and the gap between the two best Gumbel + log-probability values of the draw each position used
(inf where none was made: hold positions, [MASK] inputs of a jump).  A device test leaves out positions whose gap is under GAP_FLOOR;
the noise seed is the first one, counting up from 1234, for which those are at most MAX_LEFT_OUT of all positions in both chains.

Usage:  python tests/golden/make_golden_resample.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg
import make_golden_known as mk
from oracle import philox

K, L, T, B = mk.K, mk.L, mk.T, mk.B
GAP_FLOOR, MAX_LEFT_OUT = mk.GAP_FLOOR, mk.MAX_LEFT_OUT
FIRST_SEED = 1234
CHAINS = {"renoise": (10, 2), "hold": (30, 3)}      # mode -> (jump, times)


def load_plan():
    """resample_plan from the package's d3pm.py without importing the package (the reference's `src` is on the path here)."""
    import importlib.util
    pkg = os.path.join(mg.REPO, "gif-synthesis-with-discrete-diffusion_amd")
    spec = importlib.util.spec_from_file_location("gsdd_pkg", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gsdd_pkg"] = mod
    spec.loader.exec_module(mod)
    return mod.d3pm.resample_plan


def jump_logp(tok, a, jump, att, ctt):
    """(B, K+1, L) f32 log q(x_{a+jump} | x_a = tok) by the fp64 rule; att / ctt: the reference's cumulative arrays (index T = level -1)."""
    ia, b = (a + T + 1) % (T + 1), a + jump
    assert 0 <= b <= T - 1
    al = att[b] / att[ia]
    ga = (ctt[b] - ctt[ia]) / (1.0 - ctt[ia])
    be = (1.0 - al - ga) / K
    tok = tok.numpy()
    lp = np.full((B, K + 1, L), np.log(be), dtype=np.float64)
    lp[:, K, :] = np.log(ga)
    bi, li = np.nonzero(tok < K)
    lp[bi, tok[bi, li], li] = np.log(al + be)
    bm, lm = np.nonzero(tok == K)
    lp[bm, :, lm] = -np.inf
    lp[bm, K, lm] = 0.0
    return torch.from_numpy(lp.astype(np.float32))


def run_chain(dm, dt_mod, mode, plan, seed, x_known, known, cond, cf_cond, att, ctt):
    state = {"stream": 0}
    rec = {"gap": [], "trace": []}
    orig_p_pred, orig_lsc = dm.p_pred, dm.log_sample_categorical
    kn = known[:, None, :]
    log_x_known = dt_mod.index_to_log_onehot(x_known, K + 1)

    def p_pred(log_x, cond_emb, cf_cond_emb, t):
        model_log_prob, log_x_recon = orig_p_pred(log_x, cond_emb, cf_cond_emb, t)
        if mode == "renoise":
            model_log_prob = torch.where(kn, dm.q_pred(log_x_known, t - 1), model_log_prob)
        return model_log_prob, log_x_recon

    def rand_like(x, **kw):
        Bx, K1, Lx = x.shape
        u = philox.uniform_bkl(seed, state["stream"], Bx, K1, Lx)
        state["stream"] += 1
        return torch.from_numpy(u).to(x.dtype)

    def lsc(logits):
        u = philox.uniform_bkl(seed, state["stream"], *logits.shape)
        v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + logits.numpy()).astype(np.float32), axis=1)
        state["gap"] = (v[:, -1, :] - v[:, -2, :]).astype(np.float32)
        return orig_lsc(logits)

    dm.p_pred, dm.log_sample_categorical = p_pred, lsc
    keep = torch.rand_like
    torch.rand_like = rand_like
    try:
        with torch.no_grad():
            log_z = torch.full((B, K + 1, L), float("-inf"))        # all [MASK], as sample() starts
            log_z[:, K] = 0
            for kind, lvl in plan.ops:
                if kind == "step":
                    t = torch.full((B,), lvl, dtype=torch.long)
                    log_z, _ = dm.p_sample(log_z, cond, cf_cond, t, [0] * B, dm.n_sample[lvl])
                    idx, gap = dt_mod.log_onehot_to_index(log_z), state["gap"]
                    if mode == "hold":
                        idx = torch.where(known, x_known, idx)
                        gap = np.where(known.numpy(), np.float32(np.inf), gap)
                else:
                    prev = dt_mod.log_onehot_to_index(log_z)
                    idx = dt_mod.log_onehot_to_index(dm.log_sample_categorical(jump_logp(prev, lvl, plan.jump, att, ctt)))
                    gap = np.where(prev.numpy() == K, np.float32(np.inf), state["gap"])
                    assert bool((idx[prev == K] == K).all())
                    if mode == "hold":
                        idx = torch.where(known, prev, idx)
                        gap = np.where(known.numpy(), np.float32(np.inf), gap)
                log_z = dt_mod.index_to_log_onehot(idx, K + 1)
                rec["trace"].append(idx.numpy().astype(np.int8))
                rec["gap"].append(gap.astype(np.float32))
    finally:
        torch.rand_like = keep
        dm.p_pred, dm.log_sample_categorical = orig_p_pred, orig_lsc
    trace, gap = np.stack(rec["trace"]), np.stack(rec["gap"])
    assert trace.shape == gap.shape == (plan.draws, B, L) and state["stream"] == plan.draws
    assert int((trace[-1] == K).sum()) == 0
    return trace, gap


def main():
    resample_plan = load_plan()
    mg.install_stubs()
    import src.models.motionencoder.diffusion_transformer as dt_mod

    base = np.load(os.path.join(mg.OUT, "d3pm_L64.npz"))
    assert (int(base["cfg_K"]), int(base["cfg_L"]), int(base["cfg_T"]), int(base["cfg_B"])) == (K, L, T, B)
    dm = mg.build_d3pm(K, L, [8, 8], int(base["cfg_n_layer"]), int(base["cfg_cond_dim"]), T, seed=21)
    for k, v in dm.state_dict().items():
        if "sd/" + k in base.files and not k.startswith("Lt_"):
            assert np.array_equal(v.numpy(), base["sd/" + k]), k          # the weights of d3pm_L64.npz
    cond = torch.from_numpy(base["step_cond"])
    cf_cond = torch.zeros_like(cond)
    dm.prior_rule = 0
    x_known, known = mk.known_inputs()
    _, _, _, att, _, ctt = dt_mod.alpha_schedule(T, N=K)
    att, ctt = np.asarray(att, dtype=np.float64), np.asarray(ctt, dtype=np.float64)
    assert att[T] == 1 and ctt[T] == 0
    plans = {mode: resample_plan(T, *jt) for mode, jt in CHAINS.items()}
    assert (plans["renoise"].n_steps, plans["renoise"].n_jumps) == (190, 9) and (plans["hold"].n_steps, plans["hold"].n_jumps) == (280, 6)

    kn = known.numpy()
    for seed in range(FIRST_SEED, FIRST_SEED + 50):
        out, shares = {}, {}
        for mode, plan in plans.items():
            trace, gap = run_chain(dm, dt_mod, mode, plan, seed, x_known, known, cond, cf_cond, att, ctt)
            shares[mode] = float((gap < GAP_FLOOR).mean())
            out.update({f"trace_{mode}": trace, f"gap_{mode}": gap, f"ops_{mode}": np.array([(k == "jump", v) for k, v in plan.ops], dtype=np.int16)})
        print("seed %d: left out %s" % (seed, {m: "%.3f %%" % (100 * s) for m, s in shares.items()}))
        if max(shares.values()) <= MAX_LEFT_OUT:
            break
    else:
        raise SystemExit("no seed keeps the reference inside the cap")
    for mode, plan in plans.items():
        trace = out[f"trace_{mode}"]
        assert np.array_equal(trace[-1][kn], x_known.numpy()[kn])         # both chains end on the clean tokens
        jumps = [i for i, (k, _) in enumerate(plan.ops) if k == "jump"]
        print("%s: jump %d times %d, %d ops; [MASK] share before / after the first and the last jump: %.2f -> %.2f, %.2f -> %.2f" % (
            mode, plan.jump, plan.times, plan.draws, (trace[jumps[0] - 1] == K).mean(), (trace[jumps[0]] == K).mean(),
            (trace[jumps[-1] - 1] == K).mean(), (trace[jumps[-1]] == K).mean()))
    assert shares["renoise"] <= MAX_LEFT_OUT and shares["hold"] <= MAX_LEFT_OUT
    out.update({"x_known": x_known.numpy().astype(np.int8), "known": kn,
                "cfg_noise_seed": seed, "cfg_mask_seed": mk.MASK_SEED, "cfg_gap_floor": GAP_FLOOR, "cfg_max_left_out": MAX_LEFT_OUT,
                "cfg_left_out_renoise": shares["renoise"], "cfg_left_out_hold": shares["hold"], "cfg_base": "d3pm_L64",
                "cfg_jump_renoise": CHAINS["renoise"][0], "cfg_times_renoise": CHAINS["renoise"][1],
                "cfg_jump_hold": CHAINS["hold"][0], "cfg_times_hold": CHAINS["hold"][1]})
    path = os.path.join(mg.OUT, "resample_L64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(mg.OUT, "d3pm_L2048.npz"))


if __name__ == "__main__":
    main()
