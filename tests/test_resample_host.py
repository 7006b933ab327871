"""RePaint's resampling jumps, host side (no GPU): the plan, the fp64 table, the argument checks, the rule restated over the oracle's
pieces and checked against the reference-generated fixture, and the inputs and comparison the GPU tests use.

The rule (tests/golden/make_golden_resample.py states it with the reference's own functions): a forward jump moves every position
from level a to b = a + jump independently.  With abar / gbar the cumulative arrays of alpha_schedule (index -1 = T: 1 / 0),
alpha~ = abar_b / abar_a, gamma~ = (gbar_b - gbar_a) / (1 - gbar_a), beta~ = (1 - alpha~ - gamma~) / K: a [MASK] stays [MASK] without a
draw, a code i goes to [MASK] with gamma~, stays with alpha~ + beta~, to any other code with beta~ each; the draw is the Gumbel arg-max on
the position's own uniforms of the op's (B, K + 1, L) Philox stream.  Hold positions are copied through.

The restatement here (jump_probs64, jump_logp, jump_tokens, the input constructions, verdict) is the yardstick tests/test_gpu_resample.py
imports."""
import os

import numpy as np
import pytest
import torch

from tests.test_known_host import GAP_FLOOR, MAX_LEFT_OUT, chain_posterior, compared, known_tokens, schedule, tiny_dm, top2_gap  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [(100, 10, 2), (100, 30, 3), (100, 99, 2), (100, 1, 2), (100, 11, 2), (7, 3, 3)]


# ----------------------------------------------------------------------------- the rule, fp64
def cumulative64(T, K):
    from oracle import d3pm as od
    at, bt, ct, att, btt, ctt = od.alpha_schedule(T, N=K)
    return at, bt, ct, att, ctt


def jump_probs64(T, K, a, jump):
    """(alpha~ + beta~, beta~, gamma~) of the move from level a (-1: clean) to a + jump, closed form in fp64."""
    _, _, _, att, ctt = cumulative64(T, K)
    ia, b = (a + T + 1) % (T + 1), a + jump
    assert -1 <= a and 0 <= b <= T - 1, (a, jump)
    al = att[b] / att[ia]
    ga = (ctt[b] - ctt[ia]) / (1.0 - ctt[ia])
    be = (1.0 - al - ga) / K
    return al + be, be, ga


def jump_matrix64(T, K, a, jump):
    """The same move as the product of the one-step (K + 1) x (K + 1) matrices of levels a + 1 ... a + jump built from at, bt, ct."""
    at, bt, ct, _, _ = cumulative64(T, K)
    P = np.eye(K + 1)
    for s in range(a + 1, a + jump + 1):
        Q = np.full((K + 1, K + 1), bt[s])
        Q[np.arange(K), np.arange(K)] += at[s]
        Q[:, K] = ct[s]
        Q[K, :] = 0.0
        Q[K, K] = 1.0
        P = P @ Q
    return P


def jump_logp(tok, levels, jump, T, K):
    """(B, K + 1, L) f32: log q(x_{a_b + jump} | x_{a_b} = tok[b]) per batch row b at from-level levels[b]; a [MASK] input has the one
    class [MASK] (probability 1)."""
    tok = np.asarray(tok)
    B, L = tok.shape
    lp = np.empty((B, K + 1, L), dtype=np.float64)
    for b in range(B):
        hit, miss, mval = jump_probs64(T, K, int(levels[b]), jump)
        lp[b] = np.log(miss)
        lp[b, K] = np.log(mval)
        code = np.nonzero(tok[b] < K)[0]
        lp[b, tok[b, code], code] = np.log(hit)
        m = np.nonzero(tok[b] == K)[0]
        lp[b][:, m] = -np.inf
        lp[b, K, m] = 0.0
    return torch.from_numpy(lp.astype(np.float32))


def jump_tokens(tok, levels, jump, T, K, seed, stream, row0=0, hold=None):
    """One forward jump by the rule -> (tokens (B, L), gap (B, L) of the draw each position used; inf where none was made: [MASK]
    inputs and hold positions)."""
    from oracle import d3pm as od
    tok = torch.as_tensor(tok)
    lp = jump_logp(tok.numpy(), levels, jump, T, K)
    out = od.gumbel_argmax(lp, seed, stream, row0=row0)
    gap = torch.from_numpy(top2_gap(lp.numpy(), seed, stream, row0))
    skip = tok == K
    if hold is not None:
        skip = skip | torch.as_tensor(hold).bool()
    return torch.where(skip, tok, out), torch.where(skip, torch.full_like(gap, float("inf")), gap)


def verdict(got, want, gap, tok_in, hold, K):
    """The comparison of the GPU test: token mismatches where the fp64 draw's gap is at least the floor, positions left out, and the
    positions that must be exact whatever the gap ([MASK] inputs and hold positions: the input itself)."""
    got, want, gap, tok_in = (np.asarray(v) for v in (got, want, gap, tok_in))
    hold = np.zeros(tok_in.shape, bool) if hold is None else np.asarray(hold).astype(bool)
    through = hold | (tok_in == K)
    out = gap < GAP_FLOOR
    return {"mismatches": int((got != want)[~out].sum()), "left_out": int(out.sum()),
            "through_changed": int((got != tok_in)[through].sum()), "out_of_range": int(((got < 0) | (got > K)).sum())}


# ----------------------------------------------------------------------------- the kernel's arithmetic in numpy, with faults to inject
def emulate_kernel(tok, table, levels, K, T, jump, seed, stream, row0=0, hold=None, fault=None):
    """What gsdd_d3pm_forward_jump computes, from the f32 table the device reads: per batch row the table row of the wrapped
    from-level, the [MASK] / hold shortcuts, Gumbel arg-max with the first index on ties.  fault: None, "row_at_b" (the table row of
    the target level), "mask_redrawn" (no [MASK] shortcut) or "hold_drawn" (the hold mask ignored)."""
    from oracle import philox
    tok = np.asarray(tok)
    table = np.asarray(table, dtype=np.float32)
    B, L = tok.shape
    lp = np.empty((B, K + 1, L), dtype=np.float32)
    for b in range(B):
        lvl = int(levels[b]) + (jump if fault == "row_at_b" else 0)
        hit, miss, mval = table[(lvl % (T + 1) + T + 1) % (T + 1)]
        lp[b] = miss
        lp[b, K] = mval
        code = np.nonzero(tok[b] < K)[0]
        lp[b, tok[b, code], code] = hit
    u = philox.uniform_bkl(seed, stream, B, K + 1, L, row0=row0)
    g = -np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30))
    with np.errstate(invalid="ignore"):
        v = (g + lp).astype(np.float32)
    out = np.where(np.isnan(v).any(axis=1), 0, np.argmax(np.where(np.isnan(v), -np.inf, v), axis=1))   # a NaN row never beats "best": class 0
    skip = np.zeros(tok.shape, bool) if fault == "mask_redrawn" else tok == K
    if hold is not None and fault != "hold_drawn":
        skip = skip | np.asarray(hold).astype(bool)
    return np.where(skip, tok, out)


# ----------------------------------------------------------------------------- inputs shared with tests/test_gpu_resample.py
WIDTHS = [4, 252, 256, 260, 1020, 1024, 2044, 2048, 4092, 4096, 4100, 8192]
JUMPS = [1, 10, 60]
CASE = {"B": 3, "L": 37, "T": 100, "row0": 1000, "seed": 4321, "stream": 7, "max_left_out": 2}


def case_levels(jump, T=100):
    """The batch rows' from-levels: clean, mid-schedule, and the highest one this jump may leave (three different ones for jump 1 and
    10; at jump 60 the highest level is 39 itself)."""
    return [-1, 39, T - 1 - jump]


def case_inputs(K, jump, input_seed):
    """3 x 37 tokens (the last workgroup of 111 positions has one wave that exits): about a third [MASK], codes 0 and K - 1 among the
    rest, and a hold mask on about a fifth of the positions, [MASK] and code inputs alike."""
    g = torch.Generator().manual_seed(input_seed)
    B, L = CASE["B"], CASE["L"]
    tok = torch.randint(0, K, (B, L), generator=g)
    tok[torch.rand(B, L, generator=g) < 1 / 3] = K
    tok[0, 1], tok[1, 2], tok[2, 3], tok[2, 36] = 0, K - 1, 0, K - 1
    hold = torch.rand(B, L, generator=g) < 0.2
    hold[0, 1] = hold[1, 2] = False
    return tok, hold


def case_seed(K, jump):
    """The first input seed, counting up from 1000 + K + jump, for which the fp64 restatement leaves at most 2 of the 111 positions
    under the gap floor.  -> (seed, tokens, hold, want, gap)"""
    for s in range(1000 + K + jump, 1000 + K + jump + 50):
        tok, hold = case_inputs(K, jump, s)
        want, gap = jump_tokens(tok, case_levels(jump), jump, CASE["T"], K, CASE["seed"], CASE["stream"], row0=CASE["row0"], hold=hold)
        if int((gap < GAP_FLOOR).sum()) <= CASE["max_left_out"]:
            return s, tok, hold, want, gap
    raise AssertionError(f"no input seed for K = {K}, jump = {jump}")


def all_mask_case(K):
    """Redrawing a [MASK] input hardly shows in tokens: [MASK] is by far the likeliest class of such a draw (K beta~ << gamma~)
    everywhere but at the bottom of the schedule.  From the clean level with jump 1, gamma~ = 9e-6 against K beta~ = 1e-6: one redrawn
    [MASK] in ten would come out as a code.  So: 111 [MASK] inputs at level -1, jump 1, which must all come back as [MASK]."""
    B, L = CASE["B"], CASE["L"]
    tok = torch.full((B, L), K, dtype=torch.int64)
    return tok, [-1] * B, 1, tok.clone(), torch.full((B, L), float("inf"))


# the seeds case_seed finds, recorded (test_case_inputs_stay_within_the_cap checks them): every case takes its first candidate except
# the ones listed
CASE_SEED_EXCEPTIONS = {}

FREQ = {"K": 32, "N": 8192, "level": 39, "jump": 10, "seed": 2026, "T": 100}


def freq_inputs(stream):
    tok = torch.randint(0, FREQ["K"], (1, FREQ["N"]), generator=torch.Generator().manual_seed(FREQ["seed"]))
    want, gap = jump_tokens(tok, [FREQ["level"]], FREQ["jump"], FREQ["T"], FREQ["K"], FREQ["seed"], stream)
    return tok, want, gap


def freq_bands():
    hit, miss, mval = jump_probs64(FREQ["T"], FREQ["K"], FREQ["level"], FREQ["jump"])
    sig = lambda p: (p * (1 - p) / FREQ["N"]) ** 0.5
    return (mval, sig(mval)), (hit, sig(hit))


def freq_stream():
    """The first Philox stream, counting up from 3, on which the fp64 draw's own [MASK] and kept shares are inside 3 sigma."""
    (pm, sm), (ph, sh) = freq_bands()
    for stream in range(3, 40):
        tok, want, _ = freq_inputs(stream)
        if abs(float((want == FREQ["K"]).float().mean()) - pm) <= 3 * sm and abs(float((want == tok).float().mean()) - ph) <= 3 * sh:
            return stream
    raise AssertionError("no stream")


FREQ_STREAM = 3      # what freq_stream() finds (checked below)


# ----------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("T,jump,times", PLANS)
def test_plan_counts_and_order(T, jump, times):
    from gsdd_amd.d3pm import resample_plan
    plan = resample_plan(T, jump, times)
    n_land = (T - 1) // jump
    assert plan.n_steps == T + (times - 1) * jump * n_land and plan.n_jumps == (times - 1) * n_land
    assert plan.draws == plan.n_steps + plan.n_jumps == len(plan.ops)
    assert (plan.t0, plan.q_sample, plan.dt, plan.post_skip) == (T - 1, False, 1, 0)
    level = T - 1                                   # the level of the state: the all-[MASK] start is what the denoiser sees at T - 1
    visits = {}
    for kind, v in plan.ops:
        assert 0 <= level <= T - 1
        assert v == level, (kind, v, level)         # a step runs the denoiser at the state's level, a jump starts where the step left it
        if kind == "step":
            level -= 1
            visits[v] = visits.get(v, 0) + 1
        else:
            assert kind == "jump" and v >= 0 and v + jump <= T - 1          # never from the clean level, never above T - 1
            level += jump
    assert plan.ops[-1] == ("step", 0) and level == -1
    # every level below the topmost stretch is denoised `times` times, the remainder at the top once
    top = T - 1 - n_land * jump
    assert all(visits[t] == (times if t > top else 1) for t in range(T)), visits
    assert all(a[0] == "step" or b[0] == "step" for a, b in zip(plan.ops, plan.ops[1:]))          # no two jumps in a row


def test_plan_figures_of_the_issue():
    from gsdd_amd.d3pm import resample_plan
    assert (resample_plan(100, 10, 2).n_steps, resample_plan(100, 10, 2).n_jumps) == (190, 9)
    assert (resample_plan(100, 30, 3).n_steps, resample_plan(100, 30, 3).n_jumps) == (280, 6)


@pytest.mark.parametrize("T,jump", [(100, 10), (100, 99), (7, 3)])
def test_times_one_is_the_plain_chain(T, jump):
    from gsdd_amd.d3pm import plan_timesteps, resample_plan, sample_plan
    plan = resample_plan(T, jump, 1)
    assert plan.n_jumps == 0 and [t for _, t in plan.ops] == [t for t, _ in plan_timesteps(sample_plan(T))]
    assert plan.draws == sample_plan(T).draws


# ----------------------------------------------------------------------------- the table
@pytest.mark.parametrize("jump", [1, 2, 10, 50])
def test_jump_table_is_the_product_of_the_one_step_matrices(jump):
    from gsdd_amd.d3pm import jump_table
    T, K = 100, 32
    tab = jump_table(T, K, jump)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (T + 1, 3)
    tab = tab.numpy().astype(np.float64)
    worst = 0.0
    for a in (-1, 0, 5, 49, 89, 97):
        if a + jump > T - 1:
            continue
        P = jump_matrix64(T, K, a, jump)
        want = np.log([P[3, 3], P[3, 4], P[3, K]])
        assert np.allclose(P[K], np.eye(K + 1)[K]) and abs(P[3].sum() - 1) < 1e-12 and np.allclose(P[3, :K][np.arange(K) != 3], P[3, 4], rtol=1e-12)
        closed = np.log(jump_probs64(T, K, a, jump))
        assert np.abs(closed - want).max() <= 1e-9 * np.abs(want).max() + 1e-13            # the closed form is the product
        err = np.abs(tab[(a + T + 1) % (T + 1)] - want) / np.abs(want)
        worst = max(worst, float(err.max()))
    print(jump, {"worst_relative_error_of_the_logs": worst})
    assert worst <= 1e-6


@pytest.mark.parametrize("K", [32, 4096])
@pytest.mark.parametrize("jump", [1, 10, 60, 99])
def test_jump_table_nan_rows_and_the_clean_row(jump, K):
    from gsdd_amd.d3pm import jump_table
    from oracle import d3pm as od
    T = 100
    tab = jump_table(T, K, jump).numpy()
    for row in range(T + 1):
        a = -1 if row == T else row
        assert bool(np.isnan(tab[row]).all()) == (a + jump > T - 1) and bool(np.isnan(tab[row]).any()) == (a + jump > T - 1), row
    fin = tab[~np.isnan(tab).any(1)]
    assert (fin <= 0).all() and (fin[:, 0] > fin[:, 1]).all()
    assert np.allclose(np.exp(fin[:, 0].astype(np.float64)) + (K - 1) * np.exp(fin[:, 1].astype(np.float64))
                       + np.exp(fin[:, 2].astype(np.float64)), 1.0, atol=1e-6)
    # from the clean level the move is q(x_b | x_0): the oracle's q_pred at level b = jump - 1, up to a few f32 roundings of its
    # log_add_exp at magnitudes up to 20 (4 x 20 x 6e-8 = 5e-6)
    sd = schedule(T, K)
    q = od.q_pred(od.index_to_log_onehot(torch.tensor([[3]]), K + 1), torch.tensor([jump - 1]), sd)[0, :, 0].numpy()
    assert np.abs(tab[T] - np.array([q[3], q[4], q[K]])).max() <= 1e-5


# ----------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("mode", ["renoise", "hold"])
def test_restatement_reproduces_the_fixture(golden, mode):
    """Teacher-forced over the reference's own trace: op i from trace[i-1] on stream i gives trace[i] -- exactly, at every position:
    steps by the known-token restatement of test_known_host, jumps by jump_tokens."""
    from gsdd_amd.d3pm import resample_plan
    sd, b, cfg = golden("d3pm_L64")
    _, a, rcfg = golden("resample_L64")
    _, ka, _ = golden("known_L64")
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    assert rcfg["gap_floor"] == GAP_FLOOR and rcfg["max_left_out"] == MAX_LEFT_OUT and rcfg["base"] == "d3pm_L64"
    assert np.array_equal(a["known"], ka["known"]) and np.array_equal(a["x_known"], ka["x_known"])       # the masks of the known fixture
    assert (rcfg["jump_renoise"], rcfg["times_renoise"], rcfg["jump_hold"], rcfg["times_hold"]) == (10, 2, 30, 3)
    plan = resample_plan(T, rcfg[f"jump_{mode}"], rcfg[f"times_{mode}"])
    known, x_known = torch.from_numpy(a["known"]), torch.from_numpy(a["x_known"].astype(np.int64))
    trace, gap = a[f"trace_{mode}"].astype(np.int64), a[f"gap_{mode}"]
    assert trace.shape == gap.shape == (plan.draws, B, L)
    assert [(bool(j), int(v)) for j, v in a[f"ops_{mode}"]] == [(k == "jump", v) for k, v in plan.ops]
    ok, left_out = compared(gap)
    assert left_out == pytest.approx(rcfg[f"left_out_{mode}"])
    cond = torch.from_numpy(b["step_cond"])
    cf = torch.zeros_like(cond)
    seed, bad, gap_err = rcfg["noise_seed"], [], 0.0
    hold = known if mode == "hold" else None
    with torch.no_grad():
        for i, (kind, lvl) in enumerate(plan.ops):
            prev = None if i == 0 else torch.from_numpy(trace[i - 1])
            if kind == "step":
                post, t = chain_posterior(prev, T - 1 - lvl, cond, cf, sd, cfg)
                tok, g = known_tokens(post, x_known, known, t, sd, mode, seed, i)
            else:
                tok, g = jump_tokens(prev, [lvl] * B, plan.jump, T, K, seed, i, hold=hold)
                assert np.isinf(g.numpy()[trace[i - 1] == K]).all()
            if not np.array_equal(tok.numpy(), trace[i]):
                bad.append((i, kind, int((tok.numpy() != trace[i]).sum())))
            fin = np.isfinite(gap[i])
            assert np.array_equal(fin, np.isfinite(g.numpy())), (i, kind)
            gap_err = max(gap_err, float(np.abs(g.numpy()[fin] - gap[i][fin]).max()))
    print(mode, {"ops": plan.draws, "left_out_share": left_out, "mismatches": bad, "max_gap_err": gap_err})
    assert not bad, bad
    assert gap_err <= 1e-4
    kn = a["known"]
    assert np.array_equal(trace[-1][kn], a["x_known"].astype(np.int64)[kn]) and int((trace[-1] == K).sum()) == 0
    jumps = [i for i, (k, _) in enumerate(plan.ops) if k == "jump"]
    for i in jumps:                                 # a jump only ever adds [MASK] among the positions that were [MASK]; hold positions stay
        assert (trace[i][trace[i - 1] == K] == K).all()
        if mode == "hold":
            assert np.array_equal(trace[i][kn], trace[i - 1][kn])
    assert (trace[jumps[0]] == K).mean() > (trace[jumps[0] - 1] == K).mean()


def test_fixture_is_small():
    size = lambda n: os.path.getsize(os.path.join(REPO, "tests", "golden", n))
    assert size("resample_L64.npz") < size("d3pm_L2048.npz") and size("resample_L64.npz") < 1 << 20


# ----------------------------------------------------------------------------- argument errors
def test_sampler_rejections(tiny_dm):
    """Raised at the top of sample(), before the device check (this model sits on the CPU)."""
    import gsdd_amd
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    tok = torch.randint(0, 32, (2, 64), generator=torch.Generator().manual_seed(1))
    mask = torch.zeros(2, 64, dtype=torch.bool)
    mask[:, :16] = True
    base = dict(known_mask=mask, content_token=tok, filter_ratio=0)
    call = lambda **kw: dm.sample(["a"] * 2, None, cond, cond, **{**base, **kw})
    for match, kw in [("resample_jump must be", dict(resample_jump=0, resample_times=2)),
                      ("resample_jump must be", dict(resample_jump=100, resample_times=2)),
                      ("resample_jump must be", dict(resample_jump=-3, resample_times=2)),
                      ("resample_jump must be", dict(resample_jump=2.0, resample_times=2)),
                      ("resample_jump must be", dict(resample_jump=True, resample_times=2)),
                      ("resample_jump must be", dict(resample_jump="10", resample_times=2)),
                      ("resample_times must be", dict(resample_jump=10, resample_times=0)),
                      ("resample_times must be", dict(resample_jump=10, resample_times=1.5)),
                      ("resample_times must be", dict(resample_jump=10, resample_times=None)),
                      ("resample_times must be", dict(resample_jump=10, resample_times=True)),
                      ("needs resample_jump", dict(resample_times=2)),
                      ("needs known_mask", dict(resample_jump=10, resample_times=2, known_mask=None)),
                      ("needs known_mask", dict(resample_jump=10, known_mask=None)),
                      ("all-\\[MASK\\] only", dict(resample_jump=10, resample_times=2, filter_ratio=0.5))]:
        with pytest.raises(gsdd_amd.GsddError, match=match):
            call(**kw)
    for kw in (dict(resample_jump=10, resample_times=2), dict(resample_jump=99, resample_times=3, known_mode="hold"),
               dict(resample_jump=1, resample_times=1), dict()):
        with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):           # valid: stops at the device check
            call(**kw)
    try:
        dm.prior_rule = 2
        with pytest.raises(gsdd_amd.GsddError, match="prior_rule > 0"):
            call(resample_jump=10, resample_times=2)
    finally:
        dm.prior_rule = 0
    for kw in (dict(resample_jump=10), dict(resample_times=2), dict(resample_jump=None)):          # sample_fast does not take them
        with pytest.raises(gsdd_amd.GsddError, match="sample_fast takes no resample_jump"):
            dm.sample_fast(["a"] * 2, None, cond, cf_condition_embed=cond, **kw, **base)


def test_plans_reach_the_loop(tiny_dm, monkeypatch):
    """None or times = 1 hands the loop sample_plan(T) itself; otherwise resample_plan."""
    from gsdd_amd.d3pm import DiffusionTransformer, resample_plan, sample_plan
    seen = []
    monkeypatch.setattr(DiffusionTransformer, "_sample_once", lambda self, plan, *a, **kw: seen.append((plan, kw)) or {"content_token": None})
    monkeypatch.setattr(DiffusionTransformer, "_range_flags", [], raising=False)
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    mask = torch.zeros(64, dtype=torch.bool)
    mask[:16] = True
    base = dict(known_mask=mask, content_token=torch.zeros(2, 64, dtype=torch.long), filter_ratio=0)
    dm.sample(["a"] * 2, None, cond, cond, **base)
    dm.sample(["a"] * 2, None, cond, cond, resample_jump=10, resample_times=1, **base)
    dm.sample(["a"] * 2, None, cond, cond, resample_jump=10, resample_times=2, known_mode="hold", **base)
    assert seen[0][0] == seen[1][0] == sample_plan(100) and type(seen[1][0]) is type(sample_plan(100))
    assert seen[2][0] == resample_plan(100, 10, 2) and seen[2][1]["known"][2] == 1
    assert all("resample_jump" not in kw and "resample_times" not in kw for _, kw in seen)


def test_discrete_diffusion_keys(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    text = lambda texts: torch.zeros(len(texts), 512)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm)
    assert dd.sample_resample_jump is None and dd.sample_resample_times is None
    for kw in (dict(sample_resample_jump=0), dict(sample_resample_jump=1.5), dict(sample_resample_jump=True),
               dict(sample_resample_jump=10, sample_resample_times=0), dict(sample_resample_jump=10, sample_resample_times="2")):
        with pytest.raises(gsdd_amd.GsddError, match="sample_resample_"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, **kw)
    with pytest.raises(gsdd_amd.GsddError, match="needs sample_resample_jump"):
        gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_resample_times=2)
    with pytest.raises(gsdd_amd.GsddError, match="sample_skip_step"):
        gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_resample_jump=10, sample_skip_step=1)
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.sample_resample_jump is None and gen.sample_resample_times is None
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.sample_resample_jump=10",
                                                               "model.generator.sample_resample_times=2"]).model.generator
    assert gen.sample_resample_jump == 10 and gen.sample_resample_times == 2

    class Auto:
        device = torch.device("cpu")
        latent_shape = (4, 4, 4)
        decode = staticmethod(lambda tok: tok)
    seen = []
    monkeypatch.setattr(tiny_dm, "sample", lambda *a, **kw: seen.append(kw) or {"content_token": torch.zeros(2, 64, dtype=torch.long)}, raising=False)
    tok = torch.ones(2, 64, dtype=torch.long)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_resample_jump=10, sample_resample_times=2)
    mask = dd.condition_frame_mask((4, 4, 4))
    dd.sample_videos(["a", "b"], Auto(), known_tokens=tok, known_mask=mask)
    dd.sample_videos(["a", "b"], Auto())                                               # no mask: the plain call, no resampling keys
    gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_resample_jump=5).sample_videos(
        ["a", "b"], Auto(), known_tokens=tok, known_mask=mask)
    gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1).sample_videos(["a", "b"], Auto(), known_tokens=tok, known_mask=mask)
    assert (seen[0]["resample_jump"], seen[0]["resample_times"]) == (10, 2) and seen[0]["known_mask"] is mask
    assert "resample_jump" not in seen[1] and "resample_times" not in seen[1]
    assert (seen[2]["resample_jump"], seen[2]["resample_times"]) == (5, 1)
    assert "resample_jump" not in seen[3]


def test_ops_wrapper_refuses_what_the_kernel_would_misread():
    """Dense int64 (B, L) tokens, a whole table: checked before anything reaches the library (these tensors sit on the CPU)."""
    import gsdd_amd
    from gsdd_amd import ops
    tok, wide = torch.zeros(4, 6, dtype=torch.long), torch.zeros(4, 12, dtype=torch.long)
    t, sid, table = torch.zeros(4, dtype=torch.long), torch.zeros(1, dtype=torch.long), torch.zeros(101, 3)
    kw = dict(K=8, T=100, jump=1, seed=1)
    for match, args, extra in [("contiguous", (wide[:, ::2], tok, table, t, sid), {}), ("contiguous", (tok, wide[:, ::2], table, t, sid), {}),
                               ("contiguous", (tok, tok, torch.zeros(101, 6)[:, ::2], t, sid), {}),
                               ("table must hold", (tok, tok, table[:50], t, sid), {}), ("table must hold", (tok, tok, table.double(), t, sid), {}),
                               ("must be int64", (tok.int(), tok, table, t, sid), {}), ("must be int64", (tok, tok[:2], table, t, sid), {}),
                               ("must be int64", (tok, tok, table, t[:3], sid), {}),
                               ("hold must be", (tok, tok, table, t, sid), {"hold": torch.zeros(4, 6)}),
                               ("hold must be", (tok, tok, table, t, sid), {"hold": torch.zeros(4, 12, dtype=torch.uint8)[:, ::2]})]:
        with pytest.raises(gsdd_amd.GsddError, match=match):
            ops.d3pm_forward_jump(*args, **kw, **extra)
    with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):           # a valid call stops at the device check
        ops.d3pm_forward_jump(tok, tok, table, t, sid, **kw)


def test_abi_carries_the_jump():
    import ctypes
    import gsdd_amd
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    assert header.count("} gsdd_jump_desc;") == 1 and header.count("int gsdd_d3pm_forward_jump(const gsdd_jump_desc* d, void* stream);") == 1
    L = gsdd_amd.lib()                               # (lib() checks the descriptor's size against gsdd_abi_sizeof)
    assert L.gsdd_version() >= 104 and "gsdd_d3pm_forward_jump" in gsdd_amd.EXPORTS
    S = gsdd_amd._lib.JumpDesc
    assert [n for n, _ in S._fields_] == ["tok_in", "tok_out", "B", "L", "K", "T", "table", "jump", "t_dev", "hold", "seed", "stream_dev", "row0"]
    assert L.gsdd_abi_sizeof(7) == ctypes.sizeof(S) == S.row0.offset + 8 and S.table.offset == 32 and S.t_dev.offset == S.jump.offset + 8


# ----------------------------------------------------------------------------- the GPU tests' inputs, on the restatement alone
def test_case_inputs_stay_within_the_cap():
    taken = {}
    for K in WIDTHS:
        for jump in JUMPS:
            s, tok, hold, want, gap = case_seed(K, jump)
            taken[K, jump] = s
            assert tok.shape == (3, 37) and 20 <= int((tok == K).sum()) <= 55 and int((tok == 0).sum()) >= 1 and int((tok == K - 1).sum()) >= 1
            assert 8 <= int(hold.sum()) <= 40 and bool((hold & (tok == K)).any()) and bool((hold & (tok < K)).any())
            lv = case_levels(jump)
            assert len(set(lv)) == (2 if jump == 60 else 3) and lv[0] == -1 and lv[2] + jump == CASE["T"] - 1
            assert torch.equal(want[hold | (tok == K)], tok[hold | (tok == K)])
    want_seeds = {k: CASE_SEED_EXCEPTIONS.get(k, 1000 + k[0] + k[1]) for k in taken}
    print({k: v for k, v in taken.items() if v != 1000 + k[0] + k[1]})
    assert taken == want_seeds


def test_frequency_inputs():
    (pm, sm), (ph, sh) = freq_bands()
    assert 0.1 < pm < 0.3 and ph == pytest.approx(1 - pm, abs=1e-3)          # gamma~ of 39 -> 49; a surviving code almost surely stays
    assert freq_stream() == FREQ_STREAM
    tok, want, gap = freq_inputs(FREQ_STREAM)
    assert int((tok == FREQ["K"]).sum()) == 0 and float((gap < GAP_FLOOR).float().mean()) <= MAX_LEFT_OUT


# ----------------------------------------------------------------------------- the comparison catches the faults it is there for
@pytest.mark.parametrize("K,jump", [(32, 10), (4096, 1), (260, 60)])
def test_comparison_catches_injected_faults(K, jump):
    from gsdd_amd.d3pm import jump_table
    T = CASE["T"]
    _, tok, hold, want, gap = case_seed(K, jump)
    table = jump_table(T, K, jump)
    args = (tok.numpy(), table.numpy(), case_levels(jump), K, T, jump, CASE["seed"], CASE["stream"])
    clean = verdict(emulate_kernel(*args, row0=CASE["row0"], hold=hold.numpy()), want, gap, tok, hold, K)
    assert clean == {"mismatches": 0, "left_out": clean["left_out"], "through_changed": 0, "out_of_range": 0} and clean["left_out"] <= 2
    seen = {}
    for fault in ("row_at_b", "hold_drawn"):
        seen[fault] = verdict(emulate_kernel(*args, row0=CASE["row0"], hold=hold.numpy(), fault=fault), want, gap, tok, hold, K)
    assert seen["row_at_b"]["mismatches"] > 0 and seen["hold_drawn"]["through_changed"] > 0, seen
    # a redrawn [MASK]: on the all-[MASK] call every width's GPU case makes next to this one
    mtok, mlev, mjump, mwant, mgap = all_mask_case(K)
    margs = (mtok.numpy(), jump_table(T, K, mjump).numpy(), mlev, K, T, mjump, CASE["seed"], CASE["stream"])
    assert verdict(emulate_kernel(*margs, row0=CASE["row0"]), mwant, mgap, mtok, None, K)["through_changed"] == 0
    seen["mask_redrawn"] = verdict(emulate_kernel(*margs, row0=CASE["row0"], fault="mask_redrawn"), mwant, mgap, mtok, None, K)
    assert seen["mask_redrawn"]["through_changed"] > 0, seen
    wrong_rows = verdict(emulate_kernel(*args, row0=0, hold=hold.numpy()), want, gap, tok, hold, K)           # and the row offset
    assert wrong_rows["mismatches"] > 0
    print(K, jump, seen)
