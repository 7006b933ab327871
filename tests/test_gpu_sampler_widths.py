"""The sampler's row kernels that hold a position's class row in registers -- the top-r truncated reverse step
(d3pm_step_trunc_kernel), the purity-prior kernels (d3pm_purity_kernel, d3pm_purity_trunc_kernel) and, beside them, the plain step
(d3pm_step_kernel) -- against an fp64 restatement at every register-grid width J = ceil(K / 256) the host tables dispatch on:
K = 4, 252, 256, 260, 512, 1024, 2048, 4092, 4096, 4100, 8192 (J = 1, 2, 4, 8, 16, 32 and the FULL instantiations of K = 4096), plus
K = 1020 and 2044, the partly empty J = 4 and J = 8 that the plain step's table tells from the full ones and no other width reaches;
3 x 37 = 111 positions (no multiple of the four positions of a workgroup: a wave of the last workgroup leaves at `pos >= B L`),
row0 = 1000, guided (guidance 2, lu = lc + randn) and unguided.  The selection kernel (purity_select_kernel) runs at L = 1, 3, 37,
1025, 2049 with n below, at and above the [MASK] count.

REFERENCE (`restate` with dtype float64, on the CPU).  Written out here from the kernels' header comments, not taken from the oracle's
fp32 functions: rec = log-softmax clamped to [-70, 0]; guided: xu + g (xc - xu) minus its log-sum-exp over the K classes, clamped again;
the -70 [MASK] row appended.  Truncation at rate 0.86: class k is kept iff mass_above(k) < rate on the fp64 values
(test_truncation_host.mass_above), cut classes become -70, [MASK] stays -70.  Posterior: oracle.d3pm.q_posterior, which is
dtype-agnostic (its only constants are the f32 LOG_ZERO the kernel also uses), on the fp64 row with the eight f32 schedule buffers cast
to double.  Score: exp(max_k rec) for rule 2, 1 for rule 1; smax its maximum over L; w = score / (smax + f32(1e-10)).  prob: for
rule 2 with weight r > 0 the log-softmax of (1 + w r) rec over all K + 1 rows, clamped; rec otherwise.  Tokens and candidates: the
Gumbel arg-max on the Philox uniforms (oracle.philox; seed 4321 + K, streams 7 / 11, keyed at row0) of the fp64 row, the top-two gap
from test_gpu_objective_kernels.gumbel_margin.

BARS.  The project's own contract numbers, none new: log-probability rows (kept values of a truncated row, untruncated rows, prob,
posterior), score, smax and the normalised score within 2e-5 of fp64 (test_step_kernel_full_width_matches_oracle's bar); cut classes
and the [MASK] row exactly -70; a row's kept set equal to the reference's wherever the reference's own boundary margin
min_k |mass_above(k) - rate| is at least MARGIN_FLOOR = 1e-4; tokens equal wherever that holds and the reference's top-two Gumbel gap
is at least GAP_FLOOR = 1e-3 (test_gpu_truncation's floors), at most MAX_LEFT_OUT = 5 % of a case left out; untruncated candidates and
tokens equal wherever the gap passes, at most 1 % left out (LOW_MARGIN_CAP).  Hook-free and hooked instantiations agree bit for bit,
and a truncated purity call's score and smax are the untruncated call's bit for bit (the row maximum is always kept).
One output cannot meet the flat number in f32 and is held in another form (reweighted_bar has the derivation): prob of an untruncated
call with rule 2 and weight > 0.  Its factor a = 1 + w r carries the error of the score, one number per position, into every class
multiplied by the class's depth |rec|: the f32 emulation is off by 2.3e-5 at rec = -21 ... -33 in one row of K = 4092 guided, the MI355X
by 2.2e-5 to 2.3e-5 at K = 2044, 4100, 8192 on such classes, both by 3e-5 below -60.  So that output is held to the flat 2e-5 after
one common slope per position, bounded by the derived error of a, is taken out (wider, up to 3e-5, only where the class's own roundings
exceed 2e-5: under 0.5 % of the entries, all below -28); classes at the top of a row get nothing from the slope.  Measured on the
MI355X: worst residual / bar 0.60, worst slope / bound 0.77; the plain error / 2e-5 is recorded as prob_flat_ratio (up to 1.57).  The
truncated calls' prob keeps the plain flat 2e-5 (worst 4.3e-6), as does every other output (worst 1.05e-5, the untruncated posterior).
The [MASK] class is drawn on lane (K >> 2) & 63.  A purity call cannot show that draw: its [MASK] row is -70 and never wins.  The step
can, where x_t = [MASK] and t is small, so the truncated hook-free step runs once more per case at t = (2, 3, 5), where a [MASK]
position stays [MASK] with probability 0.50, 0.67, 0.80: in every case [MASK] wins and loses at several of the 39 such positions.

INPUTS are chosen on the reference alone.  Each case's rows are a mixture: the positions l = 1 (mod 3) are wide rows of sigma 2.5 / 3
(3.25 / 3.75 at K = 8192; tens to hundreds of kept classes: every lane and several slot indices), the others sigma 5 (4-13 kept).
A drawn row whose fp64 boundary margin is below 2e-4 is replaced by the next row of the same seeded generator (sigma-3 rows of 4096+
classes would otherwise put a fifth to a half of a case within 1e-4 of the boundary), so the 5 % cap binds through the draw gap only.
Row l = 10 of every sample holds two exactly equal logits (second and third largest: a tie in every precision).  A permutation of a row's classes leaves
its margin unchanged and is used to put, in every sample, into the last quad k >= K - 4 -- the only occupant of the last slot when
K = 256 (J - 1) + 4 -- (a) the row maximum (row 6), (b) the smallest kept class of a row that keeps several, (c) the largest cut class
of a row.  x_t is [MASK] at every third position, with K - 1, K - 2 and 0 among the unmasked ones; t = (0, 1, T - 1).

The CPU part (not marked gpu) tests this file's own machinery on the reference: leave-out shares, non-empty cases, that truncation
changes tokens and candidates, the edge rows, a wide row over >= 2 slot indices and >= 32 lanes for K >= 1024; that an f32 emulation
of the restatement meets every bar on every case (the bars are not below fp32's own noise); and that each of six injected faults
comes out above a bar or as a kept-set / token mismatch at a compared position.

INSTANTIATIONS (DESIGN.md section 2 has the table).  With hooks a purity call runs MODE 1 + 2, as does rule 2 with weight > 0 without
hooks; rule 1 and rule 2 with weight 0 without hooks run MODE 0: all three passes, hooked and plain, truncated and not, at every width."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_objective_kernels import (LOW_MARGIN_CAP, SCHED_ORDER, STEP_B, STEP_K, STEP_L, STEP_ROW0, T, guarded, gumbel_margin,
                                              intact, step_rows)
from tests.test_gpu_purity import keys_numpy, select_numpy
from tests.test_gpu_truncation import GAP_FLOOR, MARGIN_FLOOR, MAX_LEFT_OUT
from tests.test_truncation_host import boundary_margin, mass_above, truncate_rows

gpu = pytest.mark.gpu

B, L, ROW0 = STEP_B, STEP_L, STEP_ROW0
WIDTHS = STEP_K + [4096]
PARTIAL_4_8 = [1020, 2044]                 # J = 4 and 8 with an empty last lane: d3pm_step_kernel<4 | 8, false, *> run at no width of STEP_K
RATE = 0.86
DRAW_MARGIN = 2e-4                         # rejection threshold of the input draw: twice MARGIN_FLOOR
BAR = 2e-5
GUIDANCE = 2.0
STEP_STREAM, PURITY_STREAM, MASK_STREAM = 7, 11, 8
T_MASK = (2, 3, 5)                         # the extra step call: P(x_{t-1} = [MASK] | x_t = [MASK]) = 0.50, 0.67, 0.80
MAX_L, TIE_L = 6, 10                       # the rows of every sample that hold edge (a) and the tie
E10 = float(np.float32(1e-10))
PURITY_RUNS = [(1, 0.0), (2, 0.0), (2, 1.0)]
PURITY_TRUNC_RUNS = [(2, 0.0), (2, 1.0), (1, 0.0)]
FAULTS = ["tail_quad_dropped", "inclusive_mass", "cut_is_strict", "mix_not_renormalised", "weight_unnormalised", "mask_draw_wrong_lane"]
# the calls a fault can reach (restate's arguments); the others would only be recomputed unchanged
FAULT_PARTS = {"tail_quad_dropped": dict(truncs=(True,)), "inclusive_mass": dict(truncs=(True,)), "cut_is_strict": dict(truncs=(True,)),
               "mix_not_renormalised": dict(truncs=(False,), runs=[(2, 0.0)]), "mask_draw_wrong_lane": dict(runs=[]),
               "weight_unnormalised": dict(runs=[(2, 1.0)], steps=False)}
CASES = [(K, guided) for K in WIDTHS + PARTIAL_4_8 for guided in (True, False)]
CASE_IDS = [f"K{K}_{'guided' if g else 'unguided'}" for K, g in CASES]


def slots(K):
    return (K + 255) // 256


# ----------------------------------------------------------------------------- the restatement: one statement, two precisions
def recon(lc, lu, dt, fault=None):
    """log p(x0 | x_t) rows (B, K + 1, L) of dtype dt from logits (B, K, L); the log-softmax sum is fp64 in both precisions"""
    lsm = lambda x: torch.log_softmax(x.double(), 1).to(dt).clamp(-70, 0)
    a = lsm(lc)
    if lu is not None:
        u = lsm(lu)
        m = u + GUIDANCE * (a - u)
        if fault != "mix_not_renormalised":
            m = m - torch.logsumexp(m, 1, keepdim=True)
        a = m.clamp(-70, 0)
    return torch.cat([a, torch.full_like(a[:, :1], -70.0)], 1)


def truncate(rec, K, fault=None):
    """class k kept iff mass_above(k) < RATE (fp64 mass of the row's own values); everything else -70"""
    x = rec.numpy()
    xm = x.astype(np.float64)
    tail = slice(256 * (slots(K) - 1), K)
    if fault == "tail_quad_dropped":
        xm[:, tail] = -np.inf
    m = mass_above(xm)
    if fault == "inclusive_mass":
        m = m + np.exp(xm)
    keep = m < RATE
    if fault == "cut_is_strict":
        cut = np.where(keep, xm, np.inf).min(axis=1, keepdims=True)
        keep &= xm > cut
    if fault == "tail_quad_dropped":
        keep[:, tail] = False
    return torch.from_numpy(np.where(keep, x, x.dtype.type(-70)))


@functools.lru_cache(maxsize=None)
def gumbels(seed, stream, K):
    """f32 Gumbel values (B, K + 1, L) of the draw at `stream`, as gumbel_margin and the kernels form them"""
    from oracle import philox
    u = torch.from_numpy(philox.uniform_bkl(seed, stream, B, K + 1, L, row0=ROW0))
    return -torch.log(-torch.log(u + 1e-30) + 1e-30)


def draw(logp, seed, stream, K, fault=None):
    """-> (tokens (B, L), top-two gap)"""
    g = gumbels(seed, stream, K)
    if fault == "mask_draw_wrong_lane":
        g = g.clone()
        g[:, K] = g[:, 0]
    v = g + logp
    if fault == "tail_quad_dropped":
        v[:, 256 * (slots(K) - 1):K] = -math.inf
    top = v.topk(2, 1).values
    return v.argmax(1), top[:, 0] - top[:, 1]


def purity(rec, rule, weight, dt, fault=None):
    """score (raw), smax, the normalised score and prob of a purity call on the (truncated or plain) row"""
    score = torch.exp(rec.max(1).values) if rule == 2 else torch.ones(B, L, dtype=dt)
    smax = score.max(1).values
    w = score / (smax[:, None] + E10)
    prob = rec
    if rule == 2 and weight > 0:
        a = 1 + (score if fault == "weight_unnormalised" else w) * weight
        y = a[:, None, :] * rec
        prob = (y - torch.logsumexp(y, 1, keepdim=True)).clamp(-70, 0)
    return dict(score=score, smax=smax, score_dbg=w if rule == 2 else torch.ones(B, L, dtype=dt), prob=prob)


@functools.lru_cache(maxsize=None)
def f32_rows(K, guided):
    """the emulation's untruncated row: what every fault but mix_not_renormalised starts from"""
    c = case(K, guided)
    return recon(c["lc"], c["lu"], torch.float32)


def restate(c, dt, fault=None, truncs=(False, True), runs=PURITY_RUNS, steps=True):
    """Every output of the step and purity calls of a case, in dtype dt: float64 without a fault is the reference (tokens and gaps
    from gumbel_margin), float32 the emulation that the injected faults go into.  truncs / runs / steps restrict it to the calls a
    fault can reach."""
    from oracle import d3pm as od
    K, seed = c["K"], c["seed"]
    ref = dt == torch.float64 and fault is None
    sd = {k: v.to(dt) for k, v in c["sd"].items()}
    lxt = od.index_to_log_onehot(c["xt"], K + 1).to(dt)
    pick = (lambda p, s: gumbel_margin(p, seed, s)) if ref else (lambda p, s: draw(p, seed, s, K, fault))
    R = {"rec": recon(c["lc"], c["lu"], dt, fault) if ref or fault == "mix_not_renormalised" else f32_rows(c["K"], c["guided"])}
    for trunc in truncs:
        key = "_t" if trunc else ""
        if trunc:
            R["rec_t"] = truncate(R["rec"], K, fault)
        row = R["rec" + key]
        if steps:
            post = od.q_posterior(row, lxt, c["t"], sd)
            assert post.dtype == dt and post.shape == (B, K + 1, L)
            R["post" + key] = post
            R["tok" + key], R["gap" + key] = pick(post, STEP_STREAM)
        if steps and trunc:                                  # the [MASK] class in play: masked x_t at small t
            R["tok_m"], R["gap_m"] = pick(od.q_posterior(row, lxt, torch.tensor(T_MASK), sd), MASK_STREAM)
        for rule, weight in runs:
            P = purity(row, rule, weight, dt, fault)
            P["cand"], P["gap"] = pick(P["prob"], PURITY_STREAM)
            R[(rule, weight, key == "_t")] = P
    if ref:
        R["margin"] = torch.from_numpy(boundary_margin(R["rec"].numpy(), RATE))
    return R


# ----------------------------------------------------------------------------- inputs
def draw_rows(K, guided, g):
    """(N, K) logit rows lc, lu: sigma 2.5 / 3 at l = 1 (mod 3), sigma 5 elsewhere, row TIE_L with its second and third largest
    logits equal; a row whose fp64 boundary margin is below DRAW_MARGIN is replaced by the next row of the generator.  K = 8192: the
    wide rows are sigma 3.25 / 3.75 -- a sigma-3 row of 8192 classes carries about 4e-4 at the boundary class and passes the draw
    about once in a thousand (measured: 40,000 candidates for 36 rows), which selects freak rows and takes half a minute."""
    l = torch.arange(B * L) % L
    lo, hi = (2.5, 3.0) if K < 8192 else (3.25, 3.75)
    sigma = torch.where(l % 3 == 1, torch.where((l // 3) % 2 == 0, lo, hi), 5.0)
    lc, lu = torch.empty(B * L, K), torch.empty(B * L, K)
    todo = torch.arange(B * L)
    while todo.numel():
        slot = todo.repeat_interleave(max(1, 64 // todo.numel()))      # several candidates per open row: the first that passes is taken
        c = torch.randn(slot.numel(), K, generator=g) * sigma[slot, None]
        du = torch.randn(slot.numel(), K, generator=g)
        tie = (l[slot] == TIE_L).nonzero()[:, 0]
        if tie.numel():
            top = c[tie].topk(3, 1).indices
            c[tie, top[:, 2]] = c[tie, top[:, 1]]
            du[tie, top[:, 2]] = du[tie, top[:, 1]]
        u = c + du
        rec = recon(c[:, :, None], u[:, :, None] if guided else None, torch.float64)
        ok = boundary_margin(rec.numpy(), RATE)[:, 0] >= DRAW_MARGIN
        first = {}
        for i in np.flatnonzero(ok):
            first.setdefault(int(slot[i]), int(i))
        for r, i in first.items():
            lc[r], lu[r] = c[i], u[i]
        todo = torch.tensor([int(r) for r in todo if int(r) not in first], dtype=torch.int64)
    return lc, lu


def place_edges(lc, lu, K, guided):
    """Permute classes (the same two of lc and lu) so that in every sample the last quad holds (a) the maximum of row MAX_L, (b) the
    smallest kept class of the first other row that keeps at least two, (c) the largest cut class of the next row that cuts one."""
    rec = recon(lc[:, :, None], lu[:, :, None] if guided else None, torch.float64).numpy()
    x = rec[:, :K, 0]
    keep = (mass_above(rec) < RATE)[:, :K, 0]

    def swap(r, i, j):
        for a in (lc, lu):
            a[r, i], a[r, j] = a[r, j].clone(), a[r, i].clone()
    for b in range(B):
        swap(b * L + MAX_L, int(x[b * L + MAX_L].argmax()), K - 1)
        used = {MAX_L, TIE_L}
        for l in range(L):
            r = b * L + l
            if l not in used and keep[r].sum() >= 2:
                swap(r, int(np.where(keep[r], x[r], np.inf).argmin()), K - 2)
                used.add(l)
                break
        for l in range(L):
            r = b * L + l
            cut = ~keep[r] & (x[r] > -70)
            if l not in used and cut.any():
                swap(r, int(np.where(cut, x[r], -np.inf).argmax()), K - 3)
                break


@functools.lru_cache(maxsize=None)
def case(K, guided):
    """committed inputs: everything comes from the seed 11000 + K"""
    from oracle import d3pm as od
    g = torch.Generator().manual_seed(11000 + K)
    lc, lu = draw_rows(K, guided, g)
    place_edges(lc, lu, K, guided)
    rows = lambda a: a.view(B, L, K).permute(0, 2, 1).contiguous()
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    xt[:, 1], xt[:, 4], xt[0, 5] = K - 1, K - 2, 0
    return dict(K=K, guided=guided, lc=rows(lc), lu=rows(lu) if guided else None, xt=xt, t=torch.tensor([0, 1, T - 1]),
                sd=od.schedule_buffers(T, K), seed=4321 + K)


@functools.lru_cache(maxsize=None)
def reference(K, guided):
    c = case(K, guided)
    R = restate(c, torch.float64)
    R["bars"] = {w: reweighted_bar(c, R, w) for _, w in PURITY_RUNS if w > 0}
    R["K"], R["xt_masked"] = K, c["xt"] == K
    return R


# ----------------------------------------------------------------------------- the comparisons (GPU results and the emulation alike)
def half_ulp(x):
    """half a unit in the last place of the f32 binade that holds x: the most one rounding to f32 moves a value of that size"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126))) - 24)


U = 2.0 ** -24
CE = 1.7e-7 + U                            # exp_term's relative error per unit of its argument (as in test_gpu_objective_kernels)


def lse_err(v, K):
    """(B, 1, L): error of the kernels' f32 wave_logsumexp of the rows v (B, C, L): exp_term's documented error on every term,
    weighted by the term's share (the largest term is exp(0) = 1 exactly); the 4 J + 5 additions of a sum in [1, 2) and above
    -- the lane's 4 J terms in slot order, the 6-step butterfly -- as a random walk of roundings of at most U each; the log, the
    final add and the rounding of the maximum's difference: 3 U"""
    d = (v - v.max(1, keepdim=True).values).abs()
    return (torch.softmax(v, 1) * CE * d).sum(1, keepdim=True) + U * (3 + math.sqrt(4 * slots(K) + 5))


def reweighted_bar(c, R, weight):
    """prob = clamp(a rec - lse(a rec)), a = 1 + w weight, of an untruncated call with rule 2 and weight > 0: the one output that plain
    f32 cannot hold to the flat 2e-5 below a moderate depth.  -> dict(r, e_a, fit).  Its error has three parts (hu(x) = half an ulp of
    x's f32 binade, the most one rounding moves a value of that size):
      own     the roundings that belong to the class alone:
              a [g hu(xc) + |1 - g| hu(xu) + g hu(xc - xu) + hu(m) + hu(rec)] + hu(a rec) + hu(prob)     (unguided: a hu(rec) + ...),
              xc, xu the clamped log-softmaxes, m their guidance mix.  Below 1.4e-5 above -32; from -32 down the binade [32, 64) makes
              the row's chain 5 x 1.9e-6 and the product lands in [32, 128): up to 2.6e-5 (a = 2).
      shared  a lse_err(m) + lse_err(a rec): what the two f32 log-sum-exps add to every class alike, about 2e-6.
      rec d_a the error d_a of the factor a, ONE number per position, which every class takes multiplied by its own depth.
              a = 1 + weight score / (smax + 1e-10) and score = exp(max_k rec): the absolute error of the row's maximum -- for a
              guided row that of the f32 log-sum-exp of the mix over K classes -- is the relative error of score, and of smax alike:
              |d_a| <= e_a = weight w (e_max + max_l e_max + 5 U) + 2 U  (exp_le0 2 ulp twice, the quotient; the product and the sum).
              Guided, K = 4092: 1.8e-6 on a peaked row, up to 4e-6 on a wide one; unguided (the maximum comes from the fp64 log-softmax): 4e-7.
    The third part is what breaks the flat number, in f32 as such: the f32 emulation is off by 2.3e-5 at rec = -21 ... -33 in one row
    of K = 4092 guided whose a is off by 4.8e-7 (score +2.7e-7, smax -1.7e-7; the row's mean error is -1.2e-5), and the MI355X by
    2.2e-5 to 2.3e-5 at K = 2044, 4100 and 8192 on classes whose own roundings stay below 2e-5; both reach 3e-5 below -60.
    Held (reweighted_check): for every position there is ONE d_a with |d_a| <= e_a such that every class of the row satisfies
        |prob_kernel - prob_fp64 - rec_k d_a| <= r_k,     r_k = max(2e-5, own_k + shared),
    i.e. the flat 2e-5 after the row's common slope is taken out, wider only where the class's own roundings exceed it (under 0.5 % of the
    entries, all below -28).  A class at the top of its row (rec near 0) gets nothing from the slope and is held to 2e-5 as it stands.
    Classes at the -70 clamp are held to r_k directly.  A truncated call keeps the plain flat 2e-5: its kept classes lie above -20."""
    hu = half_ulp
    K = c["K"]
    lsm = lambda x: torch.log_softmax(x.double(), 1).clamp(-70, 0)
    rec, P = R["rec"], R[(2, weight, False)]
    xc = lsm(c["lc"])
    own = hu(rec[:, :K])
    e_lse_m = torch.zeros(B, 1, L, dtype=torch.float64)
    if c["lu"] is not None:
        xu = lsm(c["lu"])
        m = xu + GUIDANCE * (xc - xu)
        own = GUIDANCE * hu(xc) + abs(1 - GUIDANCE) * hu(xu) + GUIDANCE * hu(xc - xu) + hu(m) + own
        e_lse_m = lse_err(m, K)
    own = torch.cat([own, torch.zeros_like(own[:, :1])], 1)
    e_max = (own.gather(1, rec.argmax(1, keepdim=True)) + e_lse_m)[:, 0]               # (B, L): of the row maximum
    w = P["score_dbg"]
    av = (1 + w * weight)[:, None, :]
    e_a = weight * w * (e_max + e_max.max(1, keepdim=True).values + 5 * U) + 2 * U
    y = av * rec
    r = (av * own + hu(y) + hu(P["prob"]) + av * e_lse_m + lse_err(y, K)).clamp(min=BAR)
    return dict(r=r, e_a=e_a, fit=(P["prob"] > -70) & (rec < 0))


def reweighted_check(got, want, rec, bar):
    """-> (worst |residual| / r over all classes after each position's best common slope within +- e_a, worst |slope| / e_a)"""
    err = got.double() - want
    if not bool(torch.isfinite(err).all()):
        return math.inf, math.inf
    r, e_a, fit = bar["r"], bar["e_a"][:, None, :], bar["fit"]
    inf = torch.full_like(err, math.inf)
    lo = torch.where(fit, (err + r) / rec, -inf).max(1, keepdim=True).values           # rec < 0: the division turns the bounds round
    hi = torch.where(fit, (err - r) / rec, inf).min(1, keepdim=True).values
    slope = torch.maximum(torch.minimum((lo + hi) / 2, e_a), -e_a)
    slope = torch.where(torch.isfinite(slope), slope, torch.zeros_like(slope))
    resid = torch.where(fit, err - rec * slope, err).abs() / r
    return float(resid.max()), float((slope.abs() / e_a).max())


def maxerr(got, want, sel=None):
    """max |got - want| over sel; a non-finite result counts as infinitely wrong"""
    d = (got.double() - want).abs()
    d = d if sel is None else d[sel.expand_as(d)]
    if d.numel() == 0:
        return 0.0
    return float(d.max()) if bool(torch.isfinite(d).all()) else math.inf


def row_check(got, R, trunc):
    """a hooked row (x0_dbg / recon_dbg) against the reference's -> record; truncated: kept set, kept values, exact -70 elsewhere"""
    if not trunc:
        return {"row_max_err": maxerr(got, R["rec"]), "mask_row_not_m70": int((got[:, -1] != -70).sum())}
    ok = (R["margin"] >= MARGIN_FLOOR)[:, None, :]
    kw, kg = R["rec_t"] != -70, got != -70
    return {"kept_set_mismatches": int(((kw != kg) & ok).sum()), "mask_row_not_m70": int((got[:, -1] != -70).sum()),
            "row_max_err": maxerr(got, R["rec_t"], kw & kg & ok), "kept_per_row_mean": float(kw.sum(1).double().mean())}


def token_check(got, want, gap, R, trunc, name):
    ok = gap >= GAP_FLOOR
    if trunc:
        ok = ok & (R["margin"] >= MARGIN_FLOOR)
    return {name + "_mismatches": int(((got != want) & ok).sum()), name + "_left_out_share": float((~ok).double().mean())}


def check_step(got, R, trunc):
    """got: x0, post, tok (hooked), tok_plain"""
    k = "_t" if trunc else ""
    ok = (R["margin"] >= MARGIN_FLOOR)[:, None, :] if trunc else None
    rec = row_check(got["x0"], R, trunc)
    rec["post_max_err"] = maxerr(got["post"], R["post" + k], ok)
    rec.update(token_check(got["tok"], R["tok" + k], R["gap" + k], R, trunc, "tok"))
    rec["plain_differs_from_hooked"] = int((got["tok_plain"] != got["tok"]).sum())
    rec["worst_ratio"] = max(rec["row_max_err"], rec["post_max_err"]) / BAR
    return rec


def check_purity(got, R, rule, weight, trunc):
    """got: score, smax, cand (hooked call), recon, prob, score_dbg, and the hook-free call's cand_plain, score_plain, smax_plain"""
    P = R[(rule, weight, trunc)]
    ok = (R["margin"] >= MARGIN_FLOOR)[:, None, :] if trunc else None
    rec = row_check(got["recon"], R, trunc)
    rec.update(score_max_err=maxerr(got["score"], P["score"]), smax_max_err=maxerr(got["smax"], P["smax"]),
               score_dbg_max_err=maxerr(got["score_dbg"], P["score_dbg"]), prob_max_err=maxerr(got["prob"], P["prob"], ok))
    rec.update(token_check(got["cand"], P["cand"], P["gap"], R, trunc, "cand"))
    rec["plain_differs_from_hooked"] = sum(int((got[k + "_plain"] != got[k]).sum()) for k in ("cand", "score", "smax"))
    if rule == 2 and weight > 0 and not trunc:                 # the re-weighted row: 2e-5 after the row's common slope (reweighted_bar)
        bar = R["bars"][weight]
        rec["prob_flat_ratio"] = rec.pop("prob_max_err") / BAR                          # recorded, not asserted: f32 itself exceeds 1
        rec["prob_resid_ratio"], rec["prob_slope_ratio"] = reweighted_check(got["prob"], P["prob"], R["rec"], bar)
        rec["prob_r_above_2e-5_share"], rec["prob_r_max"] = float((bar["r"] > BAR).double().mean()), float(bar["r"].max())
    rec["worst_ratio"] = max([v for k, v in rec.items() if k.endswith("_max_err")]) / BAR
    rec["worst_ratio"] = max(rec["worst_ratio"], rec.get("prob_resid_ratio", 0.0))
    return rec


def check_mask_step(tok, R):
    """the truncated step at t = T_MASK, hook-free: tokens where margin and gap pass the floors"""
    masked = R["xt_masked"]
    rec = token_check(tok, R["tok_m"], R["gap_m"], R, True, "tok")
    rec.update(mask_kept=int(((R["tok_m"] == R["K"]) & masked).sum()), mask_revealed=int(((R["tok_m"] != R["K"]) & masked).sum()),
               worst_ratio=math.inf if rec["tok_mismatches"] else 0.0)
    return rec


def failures(rec, trunc):
    """the keys of a record that miss the contract"""
    cap = MAX_LEFT_OUT if trunc else LOW_MARGIN_CAP / (B * L)
    bad = [k for k, v in rec.items() if (k.endswith("_mismatches") or k in ("mask_row_not_m70", "plain_differs_from_hooked",
                                                                              "score_differs_from_untruncated")) and v != 0]
    bad += [k for k, v in rec.items() if k.endswith("_left_out_share") and v > cap]
    return bad + (["worst_ratio"] if not rec["worst_ratio"] <= 1 else [])


def emulated(E, key, rule=None, weight=None):
    """the emulation's results of one call in the shape check_step / check_purity take"""
    k = "_t" if key else ""
    if rule is None:
        return dict(x0=E["rec" + k], post=E["post" + k], tok=E["tok" + k], tok_plain=E["tok" + k])
    P = E[(rule, weight, key)]
    return dict(recon=E["rec" + k], prob=P["prob"], score=P["score"], smax=P["smax"], score_dbg=P["score_dbg"], cand=P["cand"],
                cand_plain=P["cand"], score_plain=P["score"], smax_plain=P["smax"])


def check_all(E, R):
    """every comparison the GPU tests make, on a restate() result -> {call: failing keys}"""
    out = {}
    for trunc in (False, True):
        if "tok" + ("_t" if trunc else "") in E:
            out[f"step{'_trunc' if trunc else ''}"] = failures(check_step(emulated(E, trunc), R, trunc), trunc)
        for rule, weight in PURITY_RUNS:
            if (rule, weight, trunc) in E:
                rec = check_purity(emulated(E, trunc, rule, weight), R, rule, weight, trunc)
                out[f"purity{'_trunc' if trunc else ''}_r{rule}w{weight:g}"] = failures(rec, trunc)
    if "tok_m" in E:
        out["mask_step"] = failures(check_mask_step(E["tok_m"], R), True)
    return out


# ----------------------------------------------------------------------------- CPU: the test's own machinery
@pytest.mark.parametrize("K,guided", CASES, ids=CASE_IDS)
def test_inputs_leave_out_shares_and_edge_rows(K, guided):
    """On the reference alone: the shares left out are within the caps and no case is empty; truncation changes a token and a candidate
    of every call; the last quad holds the row maximum, a kept class that is not the maximum and the largest cut class in compared
    rows; for K >= 1024 a wide row keeps classes in two slot indices and 32 lanes; the tie row is a tie."""
    c, R = case(K, guided), reference(K, guided)
    assert (B * L) % 4 != 0 and c["lc"].shape == (B, K, L)
    rows_ok = R["margin"] >= MARGIN_FLOOR
    assert bool(rows_ok.all()), "the rejection draw leaves no row within the margin floor"
    for key, tok, gap, cap in (("", R["tok"], R["gap"], LOW_MARGIN_CAP / (B * L)), ("_t", R["tok_t"], R["gap_t"], MAX_LEFT_OUT)):
        out = (gap < GAP_FLOOR) | (~rows_ok if key else torch.zeros_like(rows_ok))
        assert float(out.double().mean()) <= cap and int((~out).sum()) > 0, (key, int(out.sum()))
    assert int((R["tok"] != R["tok_t"]).sum()) > 0, "truncation changes no token of the step"
    changed_cands = 0
    for rule, weight in PURITY_RUNS:
        P, Pt = R[(rule, weight, False)], R[(rule, weight, True)]
        assert int((P["gap"] < GAP_FLOOR).sum()) <= LOW_MARGIN_CAP
        assert float(((Pt["gap"] < GAP_FLOOR) | ~rows_ok).double().mean()) <= MAX_LEFT_OUT
        changed_cands += int((P["cand"] != Pt["cand"]).sum())
        assert torch.equal(P["score"], Pt["score"]) and torch.equal(P["smax"], Pt["smax"])
    assert changed_cands > 0, "truncation changes no candidate"
    # the extra step call: at the [MASK] positions the [MASK] class both wins and loses, and the shares hold
    m = check_mask_step(R["tok_m"], R)
    assert m["mask_kept"] >= 5 and m["mask_revealed"] >= 5 and m["tok_left_out_share"] <= MAX_LEFT_OUT, m
    for bar in R["bars"].values():                           # r is the flat 2e-5 but for the deep classes of peaked rows
        x = R["rec"].expand_as(bar["r"])
        wide = bar["r"] > BAR
        assert float(wide.double().mean()) <= 0.005 and float(bar["r"].max()) <= 3.2e-5 and (not wide.any() or float(x[wide].max()) < -28)
        assert float(bar["e_a"].max()) <= (5e-6 if guided else 1e-6)
    # x_t: [MASK] at every third position, K - 1, K - 2 and 0 among the others
    assert bool((c["xt"][:, ::3] == K).all()) and all(int((c["xt"] == v).sum()) > 0 for v in (K - 1, K - 2, 0))
    # the edges
    x, xt_ = R["rec"][:, :K], R["rec_t"][:, :K]
    kept = xt_ != -70
    last = torch.arange(K) >= K - 4
    top = x.argmax(1)                                                                      # (B, L)
    not_top = torch.arange(K)[None, :, None] != top[:, None, :]
    cut_max = torch.where(~kept & (x > -70), x, torch.full_like(x, -math.inf))
    assert int(((top >= K - 4) & rows_ok).sum()) >= B, "(a) the row maximum in the last quad"
    assert int(((kept & not_top & last[None, :, None]).any(1) & rows_ok).sum()) >= B, "(b) a kept class, not the maximum, in the last quad"
    assert int(((cut_max.argmax(1) >= K - 4) & cut_max.isfinite().any(1) & rows_ok).sum()) >= B, "(c) the largest cut class in the last quad"
    assert int(kept.sum(1).min()) >= 1 and int((~kept & (x > -70)).sum()) > 0
    if K >= 1024:
        k_idx = torch.arange(K)[None, :, None]
        n_slots = torch.stack([(kept & (k_idx >> 8 == j)).any(1) for j in range(slots(K))]).sum(0)
        n_lanes = torch.stack([(kept & ((k_idx >> 2) & 63 == ln)).any(1) for ln in range(64)]).sum(0)
        assert bool(((n_slots >= 2) & (n_lanes >= 32) & rows_ok).any()), (int(n_slots.max()), int(n_lanes.max()))
    # the tie row: two exactly equal entries that are kept or cut together
    v = x[:, :, TIE_L].sort(1, descending=True).values
    assert bool(((v[:, :-1] == v[:, 1:]) & (v[:, 1:] > -70)).any(1).all())
    # this file's draw and truncation are the imported ones
    assert torch.equal(draw(R["post_t"], c["seed"], STEP_STREAM, K)[0], R["tok_t"])
    r32 = R["rec"].float()
    assert np.array_equal(truncate(r32, K).numpy(), truncate_rows(r32.numpy(), RATE))


@pytest.mark.parametrize("K,guided", CASES, ids=CASE_IDS)
def test_f32_emulation_meets_every_bar(K, guided):
    """The bars are not below fp32's own noise: the restatement in plain f32 arithmetic passes every comparison of every call."""
    res = check_all(restate(case(K, guided), torch.float32), reference(K, guided))
    assert not any(res.values()), {k: v for k, v in res.items() if v}


@pytest.mark.parametrize("fault", FAULTS)
def test_injected_fault_is_caught(fault):
    """tail_quad_dropped: classes >= 256 (J - 1) absent from the mass and the draw; inclusive_mass: a class's own probability counted
    in the mass above it (upstream's cumsum off by one); cut_is_strict: a class equal to the cut value dropped; mix_not_renormalised:
    the guided row without its log-sum-exp; weight_unnormalised: a = 1 + score r without / smax; mask_draw_wrong_lane: the [MASK]
    class drawn with the uniform of quad 0 (visible in the step only, and there in every case through the t = (2, 3, 5) call).  Each
    fails a comparison of every case it applies to; weight_unnormalised of at least one (it needs smax well below 1).  A fault is put
    into the calls it can reach only (FAULT_PARTS)."""
    caught = {}
    for (K, guided), name in zip(CASES, CASE_IDS):
        if fault == "mix_not_renormalised" and not guided:
            continue
        res = check_all(restate(case(K, guided), torch.float32, fault, **FAULT_PARTS.get(fault, {})), reference(K, guided))
        caught[name] = {k: v for k, v in res.items() if v}
    print(fault, {n: sorted(v) for n, v in caught.items() if v})
    assert any(caught.values()), f"{fault}: no comparison of any case fails"
    if fault == "tail_quad_dropped":
        assert all(caught[n] for n in ("K260_guided", "K260_unguided", "K4100_guided", "K4100_unguided"))
    if fault != "weight_unnormalised":
        assert all(caught.values()), [n for n, v in caught.items() if not v]
    if fault == "mask_draw_wrong_lane":
        assert all("mask_step" in v for v in caught.values())


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    assert tuple(gsdd_amd.d3pm.SCHED_ORDER) == SCHED_ORDER
    return gsdd_amd


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def dev_rows(c):
    return step_rows(c["lc"], c["K"]), None if c["lu"] is None else step_rows(c["lu"], c["K"])


def collect(E):
    torch.cuda.synchronize()
    return {k: e[1].cpu() for k, e in E.items()}, all(intact(e) for e in E.values())


def run_step(G, c, hooked, trunc, t=None, stream=STEP_STREAM):
    """one d3pm_step call, every output a view into a sentinel-filled buffer -> (outputs on the CPU, guards intact)"""
    t = c["t"] if t is None else torch.tensor(t)
    K = c["K"]
    E = {"tok": guarded((B, L), torch.int64, 16, 16)}
    if hooked:
        E["post"] = guarded((B, K + 1, L), torch.float32, 64, (K + 1) * L + 64)      # a position past B L lands in "sample B"
        E["x0"] = guarded((B, K + 1, L), torch.float32, 64, (K + 1) * L + 64)
    lc, lu = dev_rows(c)
    G.ops.d3pm_step(lc, lu, c["xt"].cuda(), E["tok"][1], [c["sd"][n].cuda() for n in SCHED_ORDER], t.cuda(), i64([stream]), K=K, T=T,
                    guidance=GUIDANCE, seed=c["seed"], row0=ROW0, post_dbg=E["post"][1] if hooked else None,
                    x0_dbg=E["x0"][1] if hooked else None, trunc_rate=RATE if trunc else None)
    return collect(E)


def run_purity(G, c, rule, weight, hooked, trunc):
    K = c["K"]
    f = torch.float32
    E = {"score": guarded((B, L), f, 64, 64), "smax": guarded((B,), f, 16, 16), "cand": guarded((B, L), torch.int64, 16, 16)}
    if hooked:
        E["recon"] = guarded((B, K + 1, L), f, 64, (K + 1) * L + 64)
        E["prob"] = guarded((B, K + 1, L), f, 64, (K + 1) * L + 64)
        E["score_dbg"] = guarded((B, L), f, 64, 64)
    lc, lu = dev_rows(c)
    hook = lambda k: E[k][1] if hooked else None
    G.ops.d3pm_purity_step(lc, lu, E["score"][1], E["smax"][1], E["cand"][1], i64([PURITY_STREAM]), K=K, guidance=GUIDANCE, prior_rule=rule,
                           prior_weight=weight, seed=c["seed"], row0=ROW0, recon_dbg=hook("recon"), prob_dbg=hook("prob"),
                           score_dbg=hook("score_dbg"), trunc_rate=RATE if trunc else None)
    return collect(E)


def tag(K, guided):
    return f"K{K}_{'guided' if guided else 'unguided'}"


@gpu
@pytest.mark.parametrize("K,guided", CASES, ids=CASE_IDS)
def test_truncated_step_at_every_class_width(G, K, guided, monkeypatch):
    """d3pm_step_trunc_kernel<J, FULL, hooked / plain> (and, untruncated, d3pm_step_kernel's) at every width: the hooked row's kept set
    equals the reference's, kept values and the posterior within 2e-5 of fp64, cut classes and [MASK] exactly -70; the plain
    instantiation's tokens equal the hooked one's bit for bit and the reference's wherever margin and gap pass the floors."""
    c, R = case(K, guided), reference(K, guided)
    bad = {}
    for trunc in (True, False):
        h, ok_h = run_step(G, c, True, trunc)
        p, ok_p = run_step(G, c, False, trunc)
        assert ok_h and ok_p, "d3pm_step wrote outside an output"
        rec = check_step(dict(x0=h["x0"], post=h["post"], tok=h["tok"], tok_plain=p["tok"]), R, trunc)
        if K == 4096 and not trunc:                          # the three-waves-per-SIMD instantiation of the production shape
            monkeypatch.setenv("GSDD_STEP_OCC", "3")
            o3, ok_3 = run_step(G, c, False, False)
            monkeypatch.delenv("GSDD_STEP_OCC")
            assert ok_3
            rec["plain_differs_from_hooked"] += int((o3["tok"] != h["tok"]).sum())
        parity_report(f"sampler_widths::{'trunc_step' if trunc else 'step'}[{tag(K, guided)}]", {"positions": B * L, **rec})
        bad[trunc] = failures(rec, trunc)
    m, ok_m = run_step(G, c, False, True, t=T_MASK, stream=MASK_STREAM)      # [MASK] in play: drawn on lane (K >> 2) & 63
    assert ok_m
    rec = check_mask_step(m["tok"], R)
    parity_report(f"sampler_widths::mask_step[{tag(K, guided)}]", {"positions": B * L, **rec})
    bad["mask"] = failures(rec, True)
    assert not any(bad.values()), bad


def purity_case(G, c, R, rule, weight, trunc, untruncated=None):
    h, ok_h = run_purity(G, c, rule, weight, True, trunc)
    p, ok_p = run_purity(G, c, rule, weight, False, trunc)
    assert ok_h and ok_p, "d3pm_purity_step wrote outside an output"
    got = dict(h, cand_plain=p["cand"], score_plain=p["score"], smax_plain=p["smax"])
    rec = check_purity(got, R, rule, weight, trunc)
    if untruncated is not None:
        rec["score_differs_from_untruncated"] = sum(int((p[k] != untruncated[k]).sum()) for k in ("score", "smax"))
    name = f"sampler_widths::{'purity_trunc' if trunc else 'purity'}[{tag(c['K'], c['guided'])}_r{rule}w{weight:g}]"
    parity_report(name, {"positions": B * L, **rec})
    return failures(rec, trunc), p


@gpu
@pytest.mark.parametrize("K,guided", CASES, ids=CASE_IDS)
def test_purity_step_at_every_class_width(G, K, guided):
    """d3pm_purity_kernel<J, FULL, 0 / 1 / 2, hooked / plain>: score, smax, recon_dbg, prob_dbg and score_dbg within 2e-5 of fp64, the
    candidates equal to the reference's wherever the gap passes the floor; the hook-free call (MODE 0, or MODE 1 + 2 for rule 2 with
    weight 1) writes the hooked call's (MODE 1 + 2) cand, score and smax bit for bit."""
    c, R = case(K, guided), reference(K, guided)
    bad = {(rule, weight): purity_case(G, c, R, rule, weight, False)[0] for rule, weight in PURITY_RUNS}
    assert not any(bad.values()), bad


@gpu
@pytest.mark.parametrize("K,guided", CASES, ids=CASE_IDS)
def test_truncated_purity_step_at_every_class_width(G, K, guided):
    """d3pm_purity_trunc_kernel<J, FULL, 0 / 2, hooked / plain>: recon_dbg's kept set and values and prob_dbg as the truncated step's
    row, candidates with the truncation floors, score and smax bit-equal to the untruncated call's."""
    c, R = case(K, guided), reference(K, guided)
    bad = {}
    for rule, weight in PURITY_TRUNC_RUNS:
        plain, ok = run_purity(G, c, rule, weight, False, False)
        assert ok
        bad[(rule, weight)] = purity_case(G, c, R, rule, weight, True, untruncated=plain)[0]
    assert not any(bad.values()), bad


@gpu
@pytest.mark.parametrize("L_", [1, 3, 37, 1025, 2049])
def test_selection_kernel_at_small_and_odd_lengths(G, L_):
    """purity_select_kernel where the sort is padded to a power of two, the last Philox quad is cut short and L lies on either side of
    the 1024 threads; n = 0, 1, sample 0's [MASK] count, that + 3, L + 5 and -2 (the kernel's own clamps and its "fewer [MASK]
    positions than n" branch).  Against the stable numpy sort of the kernel's own keys, which are held to the fp32 formula: exactly
    min(max(n, 0), masked) [MASK] positions of a sample change, to their candidates, every other token is bit-identical, also in place."""
    from oracle import philox
    K, Bs, seed, stream = 4096, 3, 97, 12
    g = torch.Generator().manual_seed(500 + L_)
    tok = torch.randint(0, K, (Bs, L_), generator=g)
    tok[torch.rand(Bs, L_, generator=g) < 0.6] = K
    tok[0, 0], tok[2] = K, K                                # sample 2 is all [MASK]
    tok[1] = tok[1].clamp(max=K - 1)                        # sample 1 has fewer [MASK] positions than sample 0: none, or five at L >= 37
    tok[1, 3:36:7] = K
    cand = torch.randint(0, K, (Bs, L_), generator=g)
    score = (torch.rand(Bs, L_, generator=g) * 0.99 + 0.01).float()
    smax = score.max(dim=1).values
    u = philox.uniform_rows(seed, stream + 1, Bs, L_, row0=5)
    masked = (tok == K).numpy()
    count = masked.sum(1)
    m0 = int(count[0])
    ns = [0, 1, m0, m0 + 3, L_ + 5, -2]
    assert count[1] < m0 <= L_ and count[2] == L_          # n = m0 exceeds sample 1's count, n = L + 5 everyone's
    d_tok, d_cand, d_score, d_smax, sid = tok.cuda(), cand.cuda(), score.cuda(), smax.cuda(), i64([stream])
    worst_key, key_ratio, mism, bad = 0.0, 0.0, 0, []
    for rule in (2, 1):
        w = (score / (smax[:, None] + 1e-10)).numpy() if rule == 2 else np.ones((Bs, L_), dtype=np.float32)
        want_keys = keys_numpy(w, u)
        for n in ns:
            for inplace in (False, True):
                e_out = guarded((Bs, L_), torch.int64, 16, 16, fill=d_tok if inplace else None)
                e_key = guarded((Bs, L_), torch.float32, 16, 16)
                G.ops.d3pm_purity_select(e_out[1] if inplace else d_tok, e_out[1], d_cand, d_score, d_smax, i64([n]), sid, K=K,
                                         prior_rule=rule, seed=seed, stream_add=1, row0=5 * L_, key_dbg=e_key[1])
                torch.cuda.synchronize()
                assert intact(e_out) and intact(e_key), "d3pm_purity_select wrote outside an output"
                keys, out = e_key[1].cpu().numpy(), e_out[1].cpu()
                worst_key = max(worst_key, float(np.abs(keys - want_keys).max()))
                key_ratio = max(key_ratio, float((np.abs(keys - want_keys) / (1e-5 + 2e-6 * np.abs(want_keys))).max()))
                want = tok.clone()
                for b in range(Bs):
                    sel = select_numpy(keys[b], masked[b], max(n, 0))
                    assert len(sel) == min(max(n, 0), int(count[b]))
                    want[b, sel] = cand[b, sel]
                changed = out != tok
                mism += int((out != want).sum())
                if not (torch.equal(out, want) and int((changed & (tok != K)).sum()) == 0
                        and changed.sum(1).tolist() == np.minimum(max(n, 0), count).tolist()):
                    bad.append((rule, n, inplace, int((out != want).sum())))
    parity_report(f"sampler_widths::select[L{L_}]", {"masked_per_sample": count.tolist(), "n": ns, "key_max_err": worst_key,
                                                     "token_mismatches": mism, "worst_ratio": math.inf if mism else 0.0})
    assert key_ratio <= 1, worst_key                          # keys: test_selection_kernel's rtol 2e-6, atol 1e-5
    assert not bad, f"(rule, n, in place, mismatching tokens): {bad}"
