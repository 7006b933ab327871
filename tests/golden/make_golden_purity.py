#!/usr/bin/env python3
"""Generate tests/golden/purity_L64.npz: the REFERENCE's purity-prior sampling (DiffusionTransformer.sample with prior_rule 1 / 2,
diffusion_transformer.py:304-346, :621-626) on the d3pm_L64 construction (K 32, L 64, T 100, B 2, the same weights: they are not
stored again).

Runs only where the reference checkout is (see make_golden.py, whose stubs and build_d3pm are used); the reference is imported
read-only, bytecode writing off.  The two sources of randomness are replaced by Philox draws a device can regenerate:
  * torch.rand_like  -> the (B, K+1, L) draw of oracle/philox.py uniform_bkl            (the candidate tokens)
  * torch.multinomial(w, n) -> Gumbel-top-n over ONE (B, L) draw (uniform_rows) per call: key_l = log w_l - log(-log(u_l + 1e-30) + 1e-30)
    on the positions with w_l > 0, the n largest keys, ties to the lower index -- sampling without replacement from w.
A purity call spends two streams (candidates s, selection s + 1), the plain step at t = 0 one.

The noise seed is searched so that no decision of the three chains is closer than MIN_GAP to a tie: the gap between the n-th and
(n+1)-th selection key of every call, and the gap between the two best candidates (Gumbel + log-probability) at every selected position.

Usage:  python tests/golden/make_golden_purity.py
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

MIN_GAP = 1e-3          # 50 x the 2e-5 the step-kernel tests allow between device and oracle log-probabilities
K, L, T, B = 32, 64, 100, 2
PRIOR_PS = 4
RUNS = {"r1w0": (1, 0.0), "r2w0": (2, 0.0), "r2w1": (2, 1.0)}


def schedule():
    """100 reveal counts for 64 tokens: 66 zero entries, single reveals every third timestep, and timesteps that PRIOR_PS = 4 folds
    (5 -> one call of 5), splits in two (7 -> 4 + 3; 9 -> 4 + 5) and in three (10 -> 4 + 4 + 2).  64 reveals over t >= 1."""
    ns = [0] * T
    for t in range(99, 0, -3):
        ns[t] = 1
    ns[98], ns[50], ns[2], ns[1], ns[0] = 5, 7, 9, 10, 1
    assert sum(ns[1:]) == L
    return ns


class Noise:
    """State shared by the patched torch.rand_like / torch.multinomial and the p_sample wrapper."""

    def __init__(self, seed):
        self.seed, self.stream, self.purity, self.sel_stream, self.i = seed, 0, False, None, 0
        self.key_gap, self.cand_gap = np.inf, np.inf
        self.top2 = None            # (B, L) gap between the two best candidates of the current call
        self.weights = []           # the multinomial weight rows of the current call

    def rand_like(self, x, **kw):
        Bx, K1, Lx = x.shape
        u = philox.uniform_bkl(self.seed, self.stream, Bx, K1, Lx)
        self.sel_stream = self.stream + 1
        self.stream += 2 if self.purity else 1
        return torch.from_numpy(u).to(x.dtype)

    def multinomial(self, w, n, *a, **k):
        w = w.detach().numpy().astype(np.float32)
        u = philox.uniform_rows(self.seed, self.sel_stream, B, w.shape[0])[self.i]
        with np.errstate(divide="ignore"):
            key = np.log(w) - np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30))
        key = np.where(w > 0, key, -np.inf).astype(np.float32)
        order = np.argsort(-key, kind="stable")
        assert n <= int((w > 0).sum()), "over-subscribed schedule"
        sel = order[:n]
        if n < int((w > 0).sum()):
            self.key_gap = min(self.key_gap, float(key[order[n - 1]] - key[order[n]]))
        self.cand_gap = min(self.cand_gap, float(self.top2[self.i][sel].min()))
        self.weights.append(w)
        self.i += 1
        return torch.from_numpy(sel.astype(np.int64))


def run_chain(dm, dt_mod, cond, cf_cond, rule, weight, seed, ns, stop_below=None):
    """-> dict of the chain's records, or None as soon as a gap falls under stop_below."""
    noise = Noise(seed)
    dm.prior_rule, dm.prior_weight, dm.prior_ps, dm.n_sample = rule, weight, PRIOR_PS, list(ns)
    rec = {"calls": [], "trace": [], "key_gap": [], "cand_gap": []}
    orig_p_sample, orig_lsc, orig_p_pred = dm.p_sample, dm.log_sample_categorical, dm.p_pred
    first = {}

    class Stop(Exception):
        pass

    def p_pred(*a, **k):
        r = orig_p_pred(*a, **k)
        first.setdefault("recon", r[1].numpy().copy())
        return r

    def lsc(logits):
        if noise.purity:
            first.setdefault("prob", logits.numpy().copy())
        stream = noise.stream
        out = orig_lsc(logits)
        u = philox.uniform_bkl(noise.seed, stream, *logits.shape)
        v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + logits.numpy()).astype(np.float32), axis=1)
        noise.top2 = v[:, -1, :] - v[:, -2, :]
        return out

    def p_sample(log_x, cond_emb, cf_cond_emb, t, sampled, to_sample):
        noise.purity = bool(t[0] > 0)
        noise.i, noise.key_gap, noise.cand_gap, noise.weights = 0, np.inf, np.inf, []
        before = list(sampled)
        r = orig_p_sample(log_x, cond_emb, cf_cond_emb, t, sampled, to_sample)
        tok = dt_mod.log_onehot_to_index(r[0]).numpy()
        if noise.purity:
            n = r[1][0] - before[0]
            assert all(s - b0 == n for s, b0 in zip(r[1], before))
            first.setdefault("score", np.stack(noise.weights))
        else:
            n, noise.cand_gap = to_sample, float(noise.top2.min())          # the plain step decides every position
        rec["calls"].append((int(t[0]), int(n)))
        rec["trace"].append(tok.astype(np.int8))
        rec["key_gap"].append(noise.key_gap)
        rec["cand_gap"].append(noise.cand_gap)
        if stop_below is not None and min(noise.key_gap, noise.cand_gap) < stop_below:
            raise Stop
        return r

    dm.p_sample, dm.log_sample_categorical, dm.p_pred = p_sample, lsc, p_pred
    keep = torch.rand_like, torch.multinomial
    torch.rand_like, torch.multinomial = noise.rand_like, noise.multinomial
    try:
        with torch.no_grad():
            res = dm.sample(["a"] * B, None, cond, cf_cond, content_token=None, filter_ratio=0)
    except Stop:
        return None
    finally:
        torch.rand_like, torch.multinomial = keep
        dm.p_sample, dm.log_sample_categorical, dm.p_pred = orig_p_sample, orig_lsc, orig_p_pred
    rec.update(first, tokens=res["content_token"].numpy(), streams=noise.stream)
    return rec


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
    ns = schedule()

    out = {}
    # the reference's own lists (update_n_sample), by T and prior_ps
    for name, (Tn, ps) in {"T10": (10, 1024), "T25": (25, 1024), "T50": (50, 1024), "T100_ps10": (100, 10), "T100": (100, 1024),
                           "T200": (200, 1024)}.items():
        dm.num_timesteps, dm.prior_ps = Tn, ps
        dm.update_n_sample()
        out["ref_n_sample_" + name] = np.array(dm.n_sample, dtype=np.int64)
    dm.num_timesteps = T

    for seed in range(1234, 1234 + 2000):
        recs = {}
        for name, (rule, weight) in RUNS.items():
            r = run_chain(dm, dt_mod, cond, cf_cond, rule, weight, seed, ns, stop_below=MIN_GAP)
            if r is None:
                break
            recs[name] = r
        if len(recs) == len(RUNS):
            break
    else:
        raise SystemExit("no seed with every gap >= MIN_GAP")
    calls = recs["r1w0"]["calls"]
    # the denoiser's logits of the first call (all [MASK], t = calls[0][0]; the same in the three chains): the purity kernel's input
    with torch.no_grad():
        xt0, t0 = torch.full((B, L), K, dtype=torch.long), torch.full((B,), calls[0][0], dtype=torch.long)
        out["first_logits"] = dm.transformer(xt0.clone(), cond, t0).numpy()                 # (B, K, L)
        out["first_logits_uncond"] = dm.transformer(xt0.clone(), cf_cond, t0).numpy()
    for name, r in recs.items():
        assert r["calls"] == calls and r["streams"] == 2 * (len(calls) - 1) + 1
        assert min(r["key_gap"]) >= MIN_GAP and min(r["cand_gap"]) >= MIN_GAP
        assert int((r["tokens"] == K).sum()) == 0                         # every token revealed
        out.update({f"{name}_trace": np.stack(r["trace"]), f"{name}_tokens": r["tokens"].astype(np.int8),
                    f"{name}_recon": r["recon"].astype(np.float32), f"{name}_prob": r["prob"].astype(np.float32),
                    f"{name}_score": r["score"].astype(np.float32),
                    f"{name}_key_gap": np.array(r["key_gap"], dtype=np.float32), f"{name}_cand_gap": np.array(r["cand_gap"], dtype=np.float32)})
        print(name, "min key gap %.3g" % min(r["key_gap"]), "min candidate gap %.3g" % min(r["cand_gap"]),
              "tokens unique:", len(np.unique(r["tokens"])))
    out.update({"n_sample": np.array(ns, dtype=np.int64), "calls": np.array(calls, dtype=np.int64),
                "cfg_prior_ps": PRIOR_PS, "cfg_noise_seed": seed, "cfg_min_gap": MIN_GAP, "cfg_base": "d3pm_L64",
                "cfg_rules": np.array([v[0] for v in RUNS.values()]), "cfg_weights": np.array([v[1] for v in RUNS.values()])})
    path = os.path.join(mg.OUT, "purity_L64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; noise seed", seed, "calls", len(calls))


if __name__ == "__main__":
    main()
