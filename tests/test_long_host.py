"""Long clips without a GPU: d3pm.long_plan against the restatement of tests/long_ref.py (window count, frame map, program, draws),
every refusal of the plan, of sample_long and of the generator's three keys, the two entry points' argument checks, the header and
the command-line override."""
import ctypes
import os
import re

import pytest
import torch

from tests import long_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 100


def geometries():
    for F in (2, 4, 16):
        for k in range(1, F):
            s = F - k
            for n in sorted({F, F + 1, F + s - 1, F + s, F + s + 1, F + 3 * s}):
                yield F, k, n


def window_plans():
    from gsdd_amd import d3pm
    return [d3pm.sample_plan(T), d3pm.sample_plan(T, 1), d3pm.resample_plan(T, 10, 2)]


def test_long_plan_geometry_program_and_draws():
    from gsdd_amd import d3pm
    seen = set()
    for F, k, n in geometries():
        s = F - k
        for wp in window_plans():
            plan = d3pm.long_plan(F, n, k, wp)
            W = plan.windows
            assert W == ref.windows(F, n, k) == 1 + -(-max(n - F, 0) // s), (F, k, n)
            assert plan.stride == s and plan.window is wp and (plan.t0, plan.dt, plan.post_skip) == (wp.t0, wp.dt, wp.post_skip)
            assert plan.frame_map() == ref.frame_map(F, n, k), (F, k, n)
            # every long frame is owned by exactly one window, the union is [0, n), window 0 owns [0, F), a later one at most s frames
            owned = [list(plan.owned(w)) for w in range(W)]
            flat = [f for fr in owned for f in fr]
            assert sorted(flat) == list(range(n)) and len(set(flat)) == n
            assert owned[0] == list(range(F)) and all(1 <= len(fr) <= s for fr in owned[1:]), (F, k, n)
            assert all(fr == list(range(w * s + k, min(w * s + F, n))) for w, fr in enumerate(owned) if w)
            want = list(wp.program)
            for _ in range(W - 1):
                want += ["slide"] + list(wp.program)
            assert list(plan.program) == want and plan.program.count("slide") == W - 1
            assert plan.draws == W * wp.draws and plan.n_steps == W * wp.n_steps and not plan.q_sample
            if n == F:
                assert W == 1 and plan.program == wp.program and plan.draws == wp.draws
            seen.add(W)
            with pytest.raises(d3pm.GsddError):
                plan.owned(W)
    assert {1, 2, 3, 4} <= seen
    # the schedule's "captured iff it recurs" rule covers the slide: one eager slide with two windows, a captured one with three
    sched = lambda W: [a for _, kind, a in d3pm.issue_schedule(d3pm.long_plan(4, 4 + 2 * (W - 1), 2, d3pm.sample_plan(T)).program, 1, True)
                       if kind == "slide"]
    assert sched(1) == [] and sched(2) == ["eager"] and sched(3) == ["eager", "capture", "replay"]
    assert sched(4) == ["eager", "capture", "replay", "replay"]
    assert "slide" in d3pm._Lane.OPS


def test_long_plan_refusals_name_the_argument():
    from gsdd_amd import d3pm
    E, wp = d3pm.GsddError, d3pm.sample_plan(T)
    for k in (0, -1, 4, 5):
        with pytest.raises(E, match="overlap"):
            d3pm.long_plan(4, 8, k, wp)
    for n in (3, 0, -4):
        with pytest.raises(E, match="n_frames"):
            d3pm.long_plan(4, n, 1, wp)
    for bad in (1.0, True, "4", None):
        with pytest.raises(E, match="window_frames"):
            d3pm.long_plan(bad, 8, 1, wp)
        with pytest.raises(E, match="n_frames"):
            d3pm.long_plan(4, bad, 1, wp)
        with pytest.raises(E, match="overlap"):
            d3pm.long_plan(4, 8, bad, wp)
    with pytest.raises(E, match="window_frames"):
        d3pm.long_plan(1, 8, 1, wp)
    with pytest.raises(E, match="prior_rule"):
        d3pm.long_plan(4, 8, 1, d3pm.PurityPlan(((99, 3),), True, 2, 0.0))
    with pytest.raises(E, match="filter_ratio"):
        d3pm.long_plan(4, 8, 1, d3pm.sample_plan(T, start_step=50))
    with pytest.raises(E, match="window_plan"):
        d3pm.long_plan(4, 8, 1, None)


@pytest.fixture(scope="module")
def tiny_dm():
    """The d3pm_L64 fixture's architecture on the CPU: argument checking only, nothing is computed."""
    import gsdd_amd
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=32, spatial_size=[8, 8], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=64, block_activate="GELU2",
                                        content_spatial_size=[8, 8], condition_dim=512, diffusion_step=T)
    return gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=T, alpha_init_type="alpha1", guidance_scale=2, content_seq_len=64)


def test_sample_long_refusals(tiny_dm):
    import gsdd_amd
    E, dm = gsdd_amd.GsddError, tiny_dm
    cond = torch.zeros(2, 1, 512)
    call = lambda **kw: dm.sample_long(["a", "b"], None, cond, cond, **dict(dict(latent_shape=(4, 4, 4), n_frames=8, overlap=2), **kw))
    for kw, what in (({"overlap": 0}, "overlap"), ({"overlap": 4}, "overlap"), ({"n_frames": 3}, "n_frames"), ({"n_frames": 8.0}, "n_frames"),
                     ({"overlap": True}, "overlap"), ({"latent_shape": (4, 4, 5)}, "latent_shape"), ({"latent_shape": (64,)}, "latent_shape"),
                     ({"filter_ratio": 0.5}, "filter_ratio"), ({"skip_step": -1}, "skip_step"), ({"skip_step": 1.5}, "skip_step"),
                     ({"skip_step": 1, "resample_jump": 10, "resample_times": 2}, "skip_step"), ({"skip_step": 1, "resample_times": 2}, "skip_step"),
                     ({"known_mode": "keep"}, "known_mode"), ({"resample_times": 2}, "resample_jump"), ({"resample_jump": 100}, "resample_jump")):
        with pytest.raises(E, match=what):
            call(**kw)
    for rule in (1, 2):
        dm.prior_rule = rule
        try:
            with pytest.raises(E, match="prior_rule"):
                call()
        finally:
            dm.prior_rule = 0
    with pytest.raises(E, match="ROCm device"):          # valid arguments: refused only because the module is on the CPU
        call()
    mask = gsdd_amd.d3pm.frame_mask((4, 4, 4), 1)
    with pytest.raises(E, match="content_token"):        # a caller's mask for window 0 goes through check_known
        call(known_mask=mask)
    with pytest.raises(E, match=r"\[MASK\]"):
        call(known_mask=mask, content_token=torch.full((2, 64), 32))


def test_discrete_diffusion_long_keys(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    E = gsdd_amd.GsddError
    text = lambda texts: torch.zeros(len(texts), 512)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm)
    assert dd.sample_long_frames is None and dd.sample_long_overlap == 4 and dd.sample_long_blend == "linear"
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_frames=40, sample_long_overlap=2, sample_long_blend="keep")
    assert (dd.sample_long_frames, dd.sample_long_overlap, dd.sample_long_blend) == (40, 2, "keep")
    for bad in (0, 1, -3, True, 2.5, "40"):
        with pytest.raises(E, match="sample_long_frames"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_frames=bad)
    for bad in (0, -1, True, 1.5, None, "4"):
        with pytest.raises(E, match="sample_long_overlap"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_overlap=bad)
    for bad in ("fade", 0, None, True):
        with pytest.raises(E, match="sample_long_blend"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_blend=bad)
    for rule in (1, 2):
        with pytest.raises(E, match="sample_prior_rule > 0"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_frames=40, sample_prior_rule=rule)
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_long_frames=40, sample_prior_rule=0).sample_long_frames == 40
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_prior_rule=2).sample_long_frames is None      # the default overlap alone is fine
    # the command line: with the key absent from a config ("+") and present in the shipped one
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert gen.get("sample_long_frames") is None
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["+model.generator.sample_long_frames=40"]).model.generator
    assert gen.sample_long_frames == 40 and isinstance(gen.sample_long_frames, int)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.sample_long_frames=24", "model.generator.sample_long_overlap=2",
                                                                "model.generator.sample_long_blend=replace"]).model.generator
    assert (gen.sample_long_frames, gen.sample_long_overlap, gen.sample_long_blend) == (24, 2, "replace")


def test_entries_reject_bad_arguments_before_any_launch():
    import gsdd_amd
    L = gsdd_amd.lib()
    assert L.gsdd_version() >= 117 and L.gsdd_abi_sizeof(9) == -1            # plain scalar arguments: no new descriptor
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for name in ("gsdd_d3pm_window_slide", "gsdd_clip_window_blend"):
        assert gsdd_amd.EXPORTS.count(name) == 1 and hasattr(L, name)
        assert len(re.findall(r"\bint " + name + r"\s*\(", header)) == 1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                   # never read: every call below returns from its checks
    # tok, long_tok, x_known, known, t2, state, bad, Bs, F, hw, k, n, K, t0, n_t2, final
    ok = [p, p, p, p, p, p, p, 2, 4, 16, 2, 8, 32, 99, 4, 0]
    for j, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, 0), (7, -2), (8, 0), (9, 0), (9, -16),
                   (10, 0), (10, 4), (10, 5), (10, -1), (11, 3), (11, 0), (11, -8), (12, 0), (13, -1), (14, -1), (14, 2 * 4 * 16 + 1), (15, 2),
                   (15, -1), (7, 1 << 26)):
        args = ok[:j] + [bad] + ok[j + 1:]
        assert L.gsdd_d3pm_window_slide(*args, None) == -1, (j, bad)
        assert b"gsdd_d3pm_window_slide" in L.gsdd_last_error()
    for j in (0, 1, 5):                                         # the final copy still needs the tokens, the long buffer and the state
        args = [p, p, None, None, None, p, None, 2, 4, 16, 2, 8, 32, 99, 0, 1]
        args[j] = None
        assert L.gsdd_d3pm_window_slide(*args, None) == -1
    # win, out, BC, Fw, HW, Fo, f0, n_ov, mode
    ok = [p, p, 6, 4, 35, 10, 2, 1, 0]
    for j, bad in ((0, None), (1, None), (2, 0), (2, -6), (2, 65536), (3, 0), (3, -4), (4, 0), (4, -35), (5, 3), (5, 0), (5, -10), (6, -1),
                   (6, 10), (7, -1), (7, 4), (7, 5), (8, 3), (8, -1), (0, p + 2), (1, p + 1)):
        args = ok[:j] + [bad] + ok[j + 1:]
        assert L.gsdd_clip_window_blend(*args, None) == -1, (j, bad)
        assert b"gsdd_clip_window_blend" in L.gsdd_last_error()
    assert L.gsdd_clip_window_blend(p, p, 6, 4, 35, 10, 0, 1, 0, None) == -1         # an overlapped window cannot be the first
    E = gsdd_amd.GsddError
    with pytest.raises(E, match="ROCm device"):
        gsdd_amd.ops.clip_window_blend(torch.zeros((1, 3, 4, 5, 7)), torch.zeros((1, 3, 8, 5, 7)), 2, 1)
    with pytest.raises(E, match="blend"):
        gsdd_amd.ops.clip_window_blend(torch.zeros((1, 3, 4, 5, 7)), torch.zeros((1, 3, 8, 5, 7)), 2, 1, blend="fade")
    with pytest.raises(E, match="does not match"):
        gsdd_amd.ops.clip_window_blend(torch.zeros((1, 3, 4, 5, 7)), torch.zeros((1, 3, 8, 5, 8)), 2, 1)
    z = lambda *s, dt=torch.int64: torch.zeros(s, dtype=dt)
    with pytest.raises(E, match="ROCm device"):
        gsdd_amd.ops.d3pm_window_slide(z(2, 64), z(2, 128), z(2, 64), z(2, 64, dt=torch.uint8), z(2), z(2), z(1, dt=torch.int32),
                                       F=4, k=2, n=8, K=32, t0=99)
    with pytest.raises(E, match="long_tok"):
        gsdd_amd.ops.d3pm_window_slide(z(2, 64), z(2, 127), z(2, 64), z(2, 64, dt=torch.uint8), z(2), z(2), z(1, dt=torch.int32),
                                       F=4, k=2, n=8, K=32, t0=99)


def test_decode_long_refusals():
    import gsdd_amd
    m = gsdd_amd.VQVAE(None, 8, 16, 8, 1, [2, 4, 4], 8, 16)
    assert m.latent_shape == (4, 4, 4)
    tok = torch.zeros((1, 6, 4, 4), dtype=torch.int64)
    m.train()
    with pytest.raises(gsdd_amd.GsddError, match="eval mode"):
        m.decode_long(tok, 2)
    m.eval()
    for kw, what in ((dict(overlap=0), "overlap"), (dict(overlap=4), "overlap"), (dict(overlap=2, blend="fade"), "blend")):
        with pytest.raises(gsdd_amd.GsddError, match=what):
            m.decode_long(tok, **kw)
    with pytest.raises(gsdd_amd.GsddError, match="n_frames"):
        m.decode_long(tok[:, :3], 2)
    with pytest.raises(gsdd_amd.GsddError, match="tokens"):
        m.decode_long(tok[0], 2)


def test_documents_name_the_feature():
    for doc, words in (("README.md", ("sample_long_frames",)),
                       ("DESIGN.md", ("gsdd_d3pm_window_slide", "gsdd_clip_window_blend", "sample_long", "decode_long", "caption per window")),
                       ("INTEGRATION.md", ("gsdd_d3pm_window_slide", "gsdd_clip_window_blend"))):
        text = open(os.path.join(REPO, doc)).read()
        for word in words:
            assert word in text, (doc, word)
