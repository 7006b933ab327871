"""Composed guidance (gsdd_d3pm_compose, include/gsdd.h) restated: one statement, runnable in two precisions, as
test_gpu_sampler_widths.recon is.  float64 is the reference, float32 the emulation that the injected faults go into.  Shared by
test_compose_host.py (the machinery, on the CPU) and test_gpu_compose.py (the kernel).

REFERENCE.  x = clamp(log_softmax(logits), -70, 0) per block (the log-softmax sum in fp64 in both precisions, as the kernel's),
e = x_u + sum_i w_i (x_i - x_u) accumulated in the order i = 0, 1, ..., then the step's own predict_start on e with no second row:
test_gpu_sampler_widths.recon(e, None, dt), and its posterior and draw as that file's restate makes them.

INPUTS.  test_gpu_sampler_widths.case(K, guided=True): B = 3, L = 37 (111 positions, no multiple of a workgroup's four), row0 = 1000,
mixed sigma rows, the row maximum in the last quad, one exact tie.  Block 0 is its lc, the null block its lu (= lc + randn), every extra
condition lc + randn from the seed 12000 + K.  The weight sets are the issue's: [2]; [1.5, -0.5]; [1, 0.75, -0.25];
[1.5, 0.75, -0.5, -0.25]; and one (B, N) matrix with a zero entry and a different row per sample.

BARS.  e within 2e-5 + 2^-22 |e_fp64|: the project's row bar, plus the stored value's own rounding at magnitudes up to a few hundred
(x_u is down to -70 and the weights' absolute sum is up to 3).  The step's x0 on e within the project's flat 2e-5.  Tokens equal
wherever the fp64 top-two Gumbel gap is at least GAP_FLOOR = 1e-3, at most LOW_MARGIN_CAP (1 %) of a case left out."""
import functools
import math

import torch

from tests.test_gpu_objective_kernels import LOW_MARGIN_CAP, gumbel_margin
from tests.test_gpu_sampler_widths import B, BAR, L, PARTIAL_4_8, STEP_STREAM, WIDTHS, case, draw, maxerr, recon
from tests.test_gpu_truncation import GAP_FLOOR

KS = WIDTHS + PARTIAL_4_8
WEIGHT_SETS = {
    "w2": [2.0],
    "w1.5_-0.5": [1.5, -0.5],
    "w1_0.75_-0.25": [1.0, 0.75, -0.25],
    "w1.5_0.75_-0.5_-0.25": [1.5, 0.75, -0.5, -0.25],
    "matrix": [[1.5, 0.0, -0.5], [1.0, 0.5, 0.25], [2.0, -0.75, 0.5]],
}
CASES = [(K, name) for K in KS for name in WEIGHT_SETS]
CASE_IDS = [f"K{K}_{name}" for K, name in CASES]
FAULTS = ["mix_not_in_log_softmax_space", "xu_dropped", "weights_of_sample_0", "last_quad_dropped", "null_block_first"]
E_REL = 2.0 ** -22


def weights_of(name):
    """-> f32 (B, N)"""
    w = torch.tensor(WEIGHT_SETS[name], dtype=torch.float32)
    return (w[None].expand(B, -1) if w.dim() == 1 else w).contiguous()


def compose(blocks, w, dt, fault=None):
    """blocks: N + 1 logits tensors (B, K, L), the conditions first and the null condition last; w: (B, N).  -> e (B, K, L) in dt"""
    lsm = (lambda x: x.to(dt)) if fault == "mix_not_in_log_softmax_space" else (lambda x: torch.log_softmax(x.double(), 1).to(dt).clamp(-70, 0))
    if fault == "null_block_first":             # block 0 read as the null condition, blocks 1 ... N as the conditions
        xu, conds = lsm(blocks[0]), blocks[1:]
    else:
        xu, conds = lsm(blocks[-1]), blocks[:-1]
    w = w.to(dt)
    if fault == "weights_of_sample_0":
        w = w[:1].expand_as(w)
    e = None
    for i, blk in enumerate(conds):
        if fault == "xu_dropped":               # sum_i w_i x_i: x_u's own share, 1 - sum_i w_i, is what is missing
            term = w[:, i, None, None] * lsm(blk)
            e = term if e is None else e + term
            continue
        term = w[:, i, None, None] * (lsm(blk) - xu)
        e = xu + term if e is None else e + term
    if fault == "last_quad_dropped":
        e = e.clone()
        e[:, -4:] = blocks[0].to(dt)[:, -4:]        # block 0's logits stay where the composed row belongs
    return e


@functools.lru_cache(maxsize=None)
def inputs(K, name):
    """-> dict(c: the sampler-widths case, blocks, w)"""
    c = case(K, True)
    w = weights_of(name)
    g = torch.Generator().manual_seed(12000 + K)
    extra = [c["lc"] + torch.randn(c["lc"].shape, generator=g) for _ in range(3)][:w.shape[1] - 1]
    return dict(c=c, blocks=[c["lc"], *extra, c["lu"]], w=w)


def restate(K, name, dt, fault=None):
    """-> dict(e, x0 (B, K + 1, L), post, tok, gap) of a composed step in dtype dt"""
    from oracle import d3pm as od
    I = inputs(K, name)
    c = I["c"]
    e = compose(I["blocks"], I["w"], dt, fault)
    x0 = recon(e, None, dt)
    sd = {k: v.to(dt) for k, v in c["sd"].items()}
    post = od.q_posterior(x0, od.index_to_log_onehot(c["xt"], K + 1).to(dt), c["t"], sd)
    if dt == torch.float64 and fault is None:
        tok, gap = gumbel_margin(post, c["seed"], STEP_STREAM)
    else:
        tok, gap = draw(post, c["seed"], STEP_STREAM, K)
    return dict(e=e, x0=x0, post=post, tok=tok, gap=gap)


@functools.lru_cache(maxsize=None)
def reference(K, name):
    return restate(K, name, torch.float64)


def check(got, R):
    """got: e (B, K, L), x0 (B, K + 1, L), tok (B, L) -> record; worst_ratio <= 1 and no mismatch is a pass"""
    err = (got["e"].double() - R["e"]).abs()
    e_ratio = float((err / (BAR + E_REL * R["e"].abs())).max()) if bool(torch.isfinite(err).all()) else math.inf
    ok = R["gap"] >= GAP_FLOOR
    rec = {"e_max_err": float(err.max()), "e_ratio": e_ratio, "e_abs_max": float(R["e"].abs().max()),
           "x0_max_err": maxerr(got["x0"], R["x0"]), "tok_mismatches": int(((got["tok"] != R["tok"]) & ok).sum()),
           "tok_left_out": int((~ok).sum())}
    rec["worst_ratio"] = max(e_ratio, rec["x0_max_err"] / BAR)
    return rec


def failures(rec):
    bad = [k for k in ("tok_mismatches",) if rec[k] != 0]
    bad += ["tok_left_out"] if rec["tok_left_out"] > LOW_MARGIN_CAP else []
    return bad + (["worst_ratio"] if not rec["worst_ratio"] <= 1 else [])
