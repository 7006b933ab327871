"""Known-token conditioned sampling's host side (no GPU): the rule restated over the oracle's pieces and checked against the
reference-generated fixture; frame_mask; the rejections at every level; the config keys; that no mask adds nothing to what reaches the
library; the inputs the GPU tests use.

The rule (tests/golden/make_golden_known.py states it with the reference's own functions): a position whose clean token x_known is
given skips the learned reverse step.  With known_mode "renoise" its token after a step whose posterior runs at t' is
argmax_k(gumbel(u) + q_pred(log_onehot(x_known), t' - 1)) on the position's own uniforms of that step's (B, K + 1, L) draw; with
"hold" it is x_known.  Every other position is the plain step's.

The restatement here (known_logp, known_tokens, top2_gap, the input constructions) is the yardstick the GPU tests and the fixture
generator import."""
import ctypes
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_FLOOR, MAX_LEFT_OUT = 1e-3, 0.05        # 50 x the 2e-5 allowed between device and oracle log-probabilities; the share a test may leave out
MODES = ("renoise", "hold")


# ----------------------------------------------------------------------------- the rule
def known_logp(x_known, t_post, sd, K):
    """(B, K + 1, L): q(x_{t'-1} | x_0 = x_known) = q_pred(log_onehot(x_known), t' - 1), the level wrapped modulo T + 1."""
    from oracle import d3pm as od
    return od.q_pred(od.index_to_log_onehot(x_known, K + 1), t_post - 1, sd)


def top2_gap(logp, seed, stream, row0=0):
    """(B, L): the gap between the two best Gumbel + log-probability values of the (B, K + 1, L) draw at `stream`."""
    from oracle import philox
    B, K1, L = logp.shape
    u = philox.uniform_bkl(seed, stream, B, K1, L, row0=row0)
    v = np.sort((-np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30)) + np.asarray(logp, dtype=np.float32)).astype(np.float32), axis=1)
    return v[:, -1, :] - v[:, -2, :]


def known_tokens(post, x_known, known, t_post, sd, mode, seed, stream, row0=0):
    """One step of the rule.  post: the plain step's (B, K + 1, L) posterior.  -> (tokens (B, L), gap (B, L) of the draw each
    position used; inf where no draw was made)."""
    from oracle import d3pm as od
    K = post.shape[1] - 1
    kn = known[:, None, :]
    if mode == "renoise":
        logp = torch.where(kn, known_logp(x_known, t_post, sd, K), post)
        return od.gumbel_argmax(logp, seed, stream, row0=row0), torch.from_numpy(top2_gap(logp.numpy(), seed, stream, row0))
    assert mode == "hold", mode
    tok = torch.where(known, x_known, od.gumbel_argmax(post, seed, stream, row0=row0))
    gap = torch.from_numpy(top2_gap(post.numpy(), seed, stream, row0))
    return tok, torch.where(known, torch.full_like(gap, float("inf")), gap)


def known_only(x_known, t_post, sd, K, mode, seed, stream, row0=0):
    """The rule at positions that are all known: (tokens, gap)."""
    from oracle import d3pm as od
    if mode == "hold":
        return x_known.clone(), torch.full(x_known.shape, float("inf"))
    logp = known_logp(x_known, t_post, sd, K)
    return od.gumbel_argmax(logp, seed, stream, row0=row0), torch.from_numpy(top2_gap(logp.numpy(), seed, stream, row0))


def compared(gap, where=None):
    """The positions a token comparison covers (of `where`), after asserting that the ones left out are at most 5 %."""
    gap = np.asarray(gap)
    where = np.ones(gap.shape, bool) if where is None else np.asarray(where)
    out = (gap < GAP_FLOOR) & where
    share = float(out.sum()) / max(int(where.sum()), 1)
    assert share <= MAX_LEFT_OUT, f"{share:.3%} of the positions are within the gap floor"
    return where & ~out, share


# ----------------------------------------------------------------------------- inputs shared with tests/test_gpu_known.py
def production_inputs(K=4096, B=2, L=37, seed=97):
    """Guided logits of sigma 5 (what the truncation tests settled on), x_t with [MASK] and codes, a Bernoulli(0.5) mask whose runs
    cross the 4-position workgroups (the last workgroup of 2 x 37 positions is partial), clean tokens, t on both sides of post_skip 3."""
    g = torch.Generator().manual_seed(seed)
    lc = torch.randn(B, K, L, generator=g) * 5.0
    lu = lc + torch.randn(B, K, L, generator=g)
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::3] = K
    known = torch.rand(B, L, generator=g) < 0.5
    x_known = torch.randint(0, K, (B, L), generator=g)
    t = torch.tensor([57, 3])
    return lc, lu, xt, known, x_known, t


def post_timestep(t, post_skip):
    return torch.where(t > post_skip, t - post_skip, t)


WIDTHS = [4, 252, 260, 1020, 4092, 4096, 4100, 8192]


def width_inputs(K, t, B=2, L=9):
    """2 x 9 positions, half of them known (alternating, so every workgroup mixes both kinds), the clean tokens spread over the
    width with its first and last class among them."""
    g = torch.Generator().manual_seed(1000 + K + t)
    lc = torch.randn(B, K, L, generator=g) * 2.0
    lu = lc + torch.randn(B, K, L, generator=g)
    xt = torch.randint(0, K, (B, L), generator=g)
    xt[:, ::2] = K
    known = torch.zeros(B, L, dtype=torch.bool)
    known.view(-1)[::2] = True
    x_known = torch.randint(0, K, (B, L), generator=g)
    x_known[0, 0], x_known[1, 1] = 0, K - 1
    return lc, lu, xt, known, x_known, torch.full((B,), t, dtype=torch.long)


FREQ = {"K": 256, "N": 8192, "t": 50, "seed": 2025, "stream": 3}


def schedule(T, K):
    from oracle import d3pm as od
    return od.schedule_buffers(T, K)


# ----------------------------------------------------------------------------- the fixture
def chain_posterior(prev, i, cond, cf, sd, cfg):
    """The plain posterior of reverse step i (t = T - 1 - i) from the tokens `prev` (None: the all-[MASK] start, true -inf rows)."""
    from oracle import d3pm as od
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    if prev is None:
        log_z = torch.full((B, K + 1, L), float("-inf"))
        log_z[:, -1] = 0
    else:
        log_z = od.index_to_log_onehot(prev, K + 1)
    t = torch.full((B,), T - 1 - i, dtype=torch.long)
    rec = od.cf_predict_start(log_z, cond, cf, t, sd, cfg["guidance"])
    return od.q_posterior(rec, log_z, t, sd), t


@pytest.mark.parametrize("mode", MODES)
def test_restatement_reproduces_the_fixture(golden, mode):
    """Teacher-forced over the reference's own trace: step i from trace[i-1] on stream i gives trace[i] wherever the reference's own
    decision was at least the floor away from a flip; the recorded gaps are the restatement's."""
    sd, b, cfg = golden("d3pm_L64")
    _, a, kcfg = golden("known_L64")
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    assert kcfg["gap_floor"] == GAP_FLOOR and kcfg["max_left_out"] == MAX_LEFT_OUT and kcfg["base"] == "d3pm_L64"
    known, x_known = torch.from_numpy(a["known"]), torch.from_numpy(a["x_known"].astype(np.int64))
    assert known.shape == (B, L) and known[0, :16].all() and not known[0, 16:].any() and 8 < int(known[1].sum()) < L - 8
    assert int(x_known.min()) >= 0 and int(x_known.max()) < K
    trace, gap = a[f"trace_{mode}"].astype(np.int64), a[f"gap_{mode}"]
    assert trace.shape == gap.shape == (T, B, L) and np.array_equal(trace[-1], a[f"tokens_{mode}"])
    ok, left_out = compared(gap)
    cond = torch.from_numpy(b["step_cond"])
    cf = torch.zeros_like(cond)
    bad, gap_err = [], 0.0
    with torch.no_grad():
        for i in range(T):
            post, t = chain_posterior(None if i == 0 else torch.from_numpy(trace[i - 1]), i, cond, cf, sd, cfg)
            tok, g = known_tokens(post, x_known, known, t, sd, mode, kcfg["noise_seed"], i)
            n = int((tok.numpy() != trace[i])[ok[i]].sum())
            if n:
                bad.append((i, n))
            fin = np.isfinite(gap[i])
            assert np.array_equal(fin, np.isfinite(g.numpy()))
            gap_err = max(gap_err, float(np.abs(g.numpy()[fin] - gap[i][fin]).max()))
    print(mode, {"left_out_share": left_out, "mismatches": bad, "max_gap_err": gap_err})
    assert not bad, bad
    assert gap_err <= 1e-4
    # the known positions end on their clean tokens (level -1 = index T: alpha-bar 1, gamma-bar 0), in both modes
    assert np.array_equal(trace[-1][a["known"]], a["x_known"].astype(np.int64)[a["known"]])
    if mode == "hold":
        assert all(np.array_equal(trace[i][a["known"]], trace[-1][a["known"]]) for i in range(T)) and np.isinf(gap[:, a["known"]]).all()
    else:                       # re-noised: early in the chain the known positions are mostly [MASK], late mostly their tokens
        assert (trace[0][a["known"]] == K).mean() > 0.9 and (trace[T // 2][a["known"]] == K).mean() < 0.9


def test_fixture_single_calls_are_the_trace(golden):
    _, a, kcfg = golden("known_L64")
    T = a["trace_renoise"].shape[0]
    assert kcfg["mid_step"] == 50 and int(a["mid_t"]) == T - 1 - 50
    for mode in MODES:
        assert np.array_equal(a[f"mid_xt_{mode}"], a[f"trace_{mode}"][49]) and np.array_equal(a[f"mid_tokens_{mode}"], a[f"trace_{mode}"][50])
        assert a[f"mid_logits_{mode}"].shape == a["first_logits"].shape == a[f"mid_logits_uncond_{mode}"].shape


# ----------------------------------------------------------------------------- frame_mask
def test_frame_mask():
    import gsdd_amd
    from gsdd_amd.d3pm import frame_mask
    m = frame_mask((4, 4, 4), 1)
    assert m.dtype == torch.bool and m.shape == (64,) and m[:16].all() and not m[16:].any()
    assert torch.equal(frame_mask((4, 2, 3), 2), torch.arange(24) < 12)
    both = frame_mask((4, 2, 2), [0, 3])                                    # interpolation: first + last frame
    assert both.tolist() == [True] * 4 + [False] * 8 + [True] * 4
    assert torch.equal(frame_mask((4, 2, 2), (0, -1)), both) and torch.equal(frame_mask((4, 2, 2), iter([3, 0])), both)
    assert not frame_mask((4, 2, 2), 0).any() and frame_mask((4, 2, 2), 4).all() and not frame_mask((4, 2, 2), []).any()
    # t-major, as quant.view(B, -1) flattens a (B, t, h, w) code tensor
    q = torch.arange(2 * 3 * 2 * 2).view(2, 3, 2, 2)
    assert torch.equal(q.view(2, -1)[:, frame_mask((3, 2, 2), [1])], q[:, 1].reshape(2, -1))
    for shape, frames in [((4, 4), 1), ((4, 0, 4), 1), ((4, 4, 4), 5), ((4, 4, 4), -1), ((4, 4, 4), [4]), ((4, 4, 4), [0.5]),
                          ((4, 4, 4), True), ((4, 4, 4), None), ((4, 4, 4), [-5])]:
        with pytest.raises(gsdd_amd.GsddError, match="frame_mask"):
            frame_mask(shape, frames)


# ----------------------------------------------------------------------------- validation
@pytest.fixture(scope="module")
def tiny_dm():
    """The d3pm_L64 fixture's architecture on the CPU: argument checking only, nothing is computed."""
    import gsdd_amd
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=32, spatial_size=[8, 8], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=64, block_activate="GELU2",
                                        content_spatial_size=[8, 8], condition_dim=512, diffusion_step=100)
    return gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2,
                                         content_seq_len=64)


def rejections(B=2, L=64, K=32):
    """(match, keyword changes) of every call the sampler must refuse; the base call is valid."""
    tok = torch.randint(0, K, (B, L), generator=torch.Generator().manual_seed(1))
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[:, :16] = True
    high, low, masked = tok.clone(), tok.clone(), tok.clone()
    high[1, 3], low[0, 0], masked[0, 15] = K + 1, -1, K
    base = dict(known_mask=mask, content_token=tok, known_mode="renoise", filter_ratio=0)
    return base, [
        ("needs content_token", dict(content_token=None)),
        ("shape", dict(known_mask=mask[:, :32])),
        ("shape", dict(known_mask=mask[:1])),
        ("shape", dict(known_mask=mask.view(-1))),
        ("bool tensor", dict(known_mask=mask.long())),
        ("integer tokens", dict(content_token=tok[:, :32])),
        ("integer tokens", dict(content_token=tok.float())),
        (r"must lie in \[0, 32\)", dict(content_token=high)),
        (r"must lie in \[0, 32\)", dict(content_token=low)),
        (r"\[MASK\] = 32 is not a clean token", dict(content_token=masked)),
        ("all-\\[MASK\\] only", dict(filter_ratio=0.5)),
        ("known_mode", dict(known_mode="keep")),
        ("known_mode", dict(known_mode=1)),
        ("known_mode", dict(known_mode=None)),
    ]


def test_sampler_rejections(tiny_dm):
    """Every refusal is raised at the top of sample / sample_fast: before the device check (this model sits on the CPU)."""
    import gsdd_amd
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    base, cases = rejections()

    def call(fast, kw):
        kw = dict(kw)
        if fast:
            return dm.sample_fast(["a"] * 2, None, cond, skip_step=1, cf_condition_embed=cond, **kw)
        return dm.sample(["a"] * 2, None, cond, cond, **kw)
    for fast in (False, True):
        for match, change in cases:
            with pytest.raises(gsdd_amd.GsddError, match=match):
                call(fast, {**base, **change})
        # the valid call passes the argument checks and stops at the device check
        with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):
            call(fast, base)
        with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):
            call(fast, {**base, "known_mask": base["known_mask"][0], "known_mode": "hold"})        # (L,): the same positions in every clip
    # a token outside [0, K) at a position that is NOT known is none of the mask's business
    tok = base["content_token"].clone()
    tok[0, 40] = 32
    with pytest.raises(gsdd_amd.GsddError, match="HIP path only"):
        call(False, {**base, "content_token": tok})
    try:
        for rule in (1, 2):
            dm.prior_rule = rule
            with pytest.raises(gsdd_amd.GsddError, match="prior_rule > 0"):
                call(False, base)
    finally:
        dm.prior_rule = 0


def test_check_known_returns_what_the_launch_needs():
    from gsdd_amd.d3pm import KNOWN_MODES, check_known
    assert KNOWN_MODES == {"renoise": 0, "hold": 1}
    base, _ = rejections()
    assert check_known(None, None, "whatever", B=2, L=64, K=32) is None                   # no mask: nothing is looked at
    for mode, code in KNOWN_MODES.items():
        m, tok, c = check_known(base["known_mask"][0], base["content_token"].view(2, 4, 4, 4).int(), mode, B=2, L=64, K=32)
        assert c == code and m.shape == tok.shape == (2, 64) and m.dtype == torch.bool and tok.dtype == torch.int64
        assert m.is_contiguous() and tok.is_contiguous() and torch.equal(m, base["known_mask"]) and torch.equal(tok, base["content_token"])


def test_discrete_diffusion_validation(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    text = lambda texts: torch.zeros(len(texts), 512)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm)
    assert dd.sample_condition_frames is None and dd.sample_known_mode == "renoise" and dd.condition_frame_mask((4, 4, 4)) is None
    for bad in (0, -1, True, 1.5, "2", [], [1.5], [True], ["0"]):
        with pytest.raises(gsdd_amd.GsddError, match="sample_condition_frames"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=bad)
    for bad in ("keep", 0, None):
        with pytest.raises(gsdd_amd.GsddError, match="sample_known_mode"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_known_mode=bad)
    for rule in (1, 2):
        with pytest.raises(gsdd_amd.GsddError, match="sample_prior_rule > 0"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_prior_rule=rule)
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=1, sample_prior_rule=0).sample_condition_frames == 1
    # validated against the latent grid at sampling time
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=2, sample_known_mode="hold", sample_skip_step=1)
    assert torch.equal(dd.condition_frame_mask((4, 4, 4)), torch.arange(64) < 32)
    for nt in (1, 2):
        with pytest.raises(gsdd_amd.GsddError, match="sample_condition_frames = 2"):
            dd.condition_frame_mask((nt, 4, 4))
    dl = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_condition_frames=[0, 3])
    assert dl.condition_frame_mask((4, 4, 4)).view(4, 16).all(1).tolist() == [True, False, False, True]
    with pytest.raises(gsdd_amd.GsddError, match="frame_mask"):
        dl.condition_frame_mask((3, 4, 4))
    # the config keys
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.sample_condition_frames is None and gen.sample_known_mode == "renoise"
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.sample_condition_frames=4",
                                                               "model.generator.sample_known_mode=hold"]).model.generator
    assert gen.sample_condition_frames == 4 and gen.sample_known_mode == "hold"

    # sample_videos hands tokens, mask and mode to the sampler; without a mask the call is the plain one
    class Auto:
        device = torch.device("cpu")
        latent_shape = (4, 4, 4)
        decode = staticmethod(lambda tok: tok)
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        return {"content_token": torch.zeros(2, 64, dtype=torch.long)}
    monkeypatch.setattr(tiny_dm, "sample_fast", fake, raising=False)
    monkeypatch.setattr(tiny_dm, "sample", fake, raising=False)
    tok = torch.ones(2, 64, dtype=torch.long)
    mask = dd.condition_frame_mask((4, 4, 4))
    dd.sample_videos(["a", "b"], Auto(), known_tokens=tok, known_mask=mask)
    dd.sample_videos(["a", "b"], Auto())
    dl.sample_videos(["a", "b"], Auto(), known_tokens=tok, known_mask=mask)
    assert seen[0]["content_token"] is tok and seen[0]["known_mask"] is mask and seen[0]["known_mode"] == "hold" and seen[0]["skip_step"] == 1
    assert seen[1]["content_token"] is None and "known_mask" not in seen[1] and "known_mode" not in seen[1]
    assert seen[2]["known_mode"] == "renoise" and "skip_step" not in seen[2]


def test_no_mask_adds_nothing_to_what_reaches_the_library(tiny_dm, monkeypatch):
    """known_mask = None: the sampler passes no `known` on, and ops fills the descriptor of a call without the keywords (NULL
    pointers, mode 0); with a mask the three fields carry the tensors."""
    import gsdd_amd
    from gsdd_amd import ops
    from gsdd_amd.d3pm import DiffusionTransformer
    seen = []
    monkeypatch.setattr(DiffusionTransformer, "_sample_once", lambda self, plan, *a, **kw: seen.append((plan, kw)) or {"content_token": None})
    monkeypatch.setattr(DiffusionTransformer, "_range_flags", [], raising=False)
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    base, _ = rejections()
    base.pop("filter_ratio")
    dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0)
    dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0, known_mask=None, known_mode="nonsense is not looked at")
    dm.sample_fast(["a"] * 2, None, cond, filter_ratio=0, skip_step=2, cf_condition_embed=cond)
    dm.sample(["a"] * 2, None, cond, cond, filter_ratio=0, **base)
    dm.sample_fast(["a"] * 2, None, cond, filter_ratio=0, skip_step=2, cf_condition_embed=cond, **{**base, "known_mode": "hold"})
    assert all("known" not in kw for _, kw in seen[:3])
    assert seen[3][1]["known"][2] == 0 and seen[4][1]["known"][2] == 1 and torch.equal(seen[3][1]["known"][1], base["content_token"])
    assert seen[3][0] == seen[0][0] and seen[4][0] == seen[2][0]                          # the chains' plans are the plain calls'

    class FakeLib:
        def __init__(self):
            self.descs = []

        def gsdd_d3pm_step(self, ref, stream):
            d = ref._obj
            self.descs.append((bytes(memoryview(d).cast("B")), d.known, d.x_known, d.known_mode))
            return 0
    fake = FakeLib()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(ops, "stream_ptr", lambda s=None: None)
    B, L, K = 2, 4, 8
    lc, tok, sid = torch.zeros(B * L, K), torch.zeros(B, L, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    sched, t = [torch.zeros(101)] * 8, torch.zeros(B, dtype=torch.long)
    kn, xk = torch.ones(B, L, dtype=torch.uint8), torch.ones(B, L, dtype=torch.long)
    for kw in ({}, {"known": None, "x_known": xk, "known_mode": 1}, {"known": kn, "x_known": xk, "known_mode": 1},
               {"known": kn.bool(), "x_known": xk}):
        ops.d3pm_step(lc, lc, tok, tok, sched, t, sid, K=K, T=100, guidance=2.0, seed=1, post_skip=1, **kw)
    d0, d1, d2, d3 = fake.descs
    assert d0 == d1 and d0[1:] == (None, None, 0)
    assert d2[1:] == (kn.data_ptr(), xk.data_ptr(), 1) and d3[2:] == (xk.data_ptr(), 0) and d2[0] != d0[0]
    for kw in ({"known": kn}, {"known": kn.long(), "x_known": xk}, {"known": kn, "x_known": xk.int()}, {"known": kn[:1], "x_known": xk},
               {"known": kn, "x_known": xk.t().contiguous().t()}):
        with pytest.raises(gsdd_amd.GsddError, match="d3pm_step: known"):
            ops.d3pm_step(lc, lc, tok, tok, sched, t, sid, K=K, T=100, guidance=2.0, seed=1, **kw)


def test_abi_carries_the_known_fields():
    import gsdd_amd
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for decl in ("const uint8_t* known;", "const int64_t* x_known;", "int known_mode;"):
        assert header.count(decl) == 1, decl
    L = gsdd_amd.lib()                                   # (lib() checks the descriptor's size against gsdd_abi_sizeof)
    assert L.gsdd_version() >= 103
    S = gsdd_amd._lib.StepDesc
    names = [n for n, _ in S._fields_]
    assert names[-5:] == ["post_skip", "known", "x_known", "known_mode", "trunc_rate"]
    # the header's order, no padding between them: two pointers after an even number of ints, then int + float
    assert S.known.offset == S.post_skip.offset + 4 and S.known.offset % 8 == 0 and S.x_known.offset == S.known.offset + 8
    assert S.known_mode.offset == S.x_known.offset + 8 and S.trunc_rate.offset == S.known_mode.offset + 4
    assert ctypes.sizeof(S) == S.trunc_rate.offset + 4


# ----------------------------------------------------------------------------- the GPU tests' inputs, on the restatement alone
@pytest.mark.parametrize("post_skip", [0, 3])
def test_production_inputs_stay_within_the_cap(post_skip):
    K, T, seed, stream = 4096, 100, 4321, 7
    lc, lu, xt, known, x_known, t = production_inputs()
    assert lc.shape == (2, K, 37) and float(lc.std()) == pytest.approx(5.0, rel=0.02)
    assert 10 <= int(known.sum()) <= 64 and int(x_known.min()) >= 0 and int(x_known.max()) < K
    kw = known.view(-1)
    n = kw.numel()
    groups = [kw[i:i + 4] for i in range(0, n, 4)]
    assert n % 4 != 0 and any(g.any() and not g.all() for g in groups)                   # partial last workgroup, mixed workgroups
    tp = post_timestep(t, post_skip)
    assert tp.tolist() == ([57, 3] if post_skip == 0 else [54, 3])
    tok, gap = known_only(x_known, tp, schedule(T, K), K, "renoise", seed, stream)
    _, share = compared(gap.numpy(), known.numpy())
    print(post_skip, {"left_out_share": share, "kept_share": float((tok == x_known)[known].float().mean())})
    assert share <= MAX_LEFT_OUT


def test_width_inputs_stay_within_the_cap():
    T, seed, stream = 100, 99, 5
    shares = {}
    for K in WIDTHS:
        for t in (50, 0):
            lc, lu, xt, known, x_known, tt = width_inputs(K, t)
            assert int(known.sum()) == 9 and int(x_known.max()) < K
            tok, gap = known_only(x_known, tt, schedule(T, K), K, "renoise", seed, stream)
            _, shares[K, t] = compared(gap.numpy(), known.numpy())
            if t == 0:
                assert torch.equal(tok, x_known) and float(gap.min()) > 30              # level -1: the draw returns x_known, far from a flip
    print(shares)
    assert max(shares.values()) <= MAX_LEFT_OUT


def test_frequency_test_timestep_sits_mid_schedule():
    """gamma-bar of the level the known draw uses at the frequency test's t: within 0.45 - 0.55, where a draw at level t instead of
    t - 1 moves the [MASK] share by a full percentage point (5 binomial standard deviations of 8192 draws are 2.8 points)."""
    sd = schedule(100, FREQ["K"])
    t = FREQ["t"]
    g_prev, g_t = float(sd["log_cumprod_ct"][t - 1].exp()), float(sd["log_cumprod_ct"][t].exp())
    assert 0.45 <= g_prev <= 0.55
    assert g_prev == pytest.approx(0.495, abs=1e-3) and g_t == pytest.approx(0.505, abs=1e-3)
    # the restatement's own [MASK] share on the test's tokens and stream is inside the band
    x_known = torch.randint(0, FREQ["K"], (1, FREQ["N"]), generator=torch.Generator().manual_seed(FREQ["seed"]))
    tok, _ = known_only(x_known, torch.tensor([t]), sd, FREQ["K"], "renoise", FREQ["seed"], FREQ["stream"])
    share = float((tok == FREQ["K"]).float().mean())
    sigma = (g_prev * (1 - g_prev) / FREQ["N"]) ** 0.5
    print({"gamma_bar_t_minus_1": g_prev, "mask_share": share, "band": 5 * sigma})
    assert abs(share - g_prev) <= 5 * sigma
