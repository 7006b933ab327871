"""Purity-prior sampling's host side (no GPU): the call plan against the reference's recorded calls and a literal count of its loop,
the reveal schedules, every rejection raised before device work, the schedule rescaling, the config keys, the register budget of the
production purity kernels, and the selection rule (Gumbel-top-n on Philox draws) as a draw without replacement."""
import importlib.util
import itertools
import os
import shutil

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def reference_calls(n_sample, prior_ps, T, B=2):
    """diffusion_transformer.py:621-626 with the bookkeeping of p_sample (:335-344, :350) restated literally: every sample reveals
    exactly n_sample positions per call."""
    calls = []
    for diffusion_index in range(T - 1, -1, -1):
        sampled = [0] * B
        while min(sampled) < n_sample[diffusion_index]:
            to_sample = n_sample[diffusion_index]
            if diffusion_index > 0:
                for i in range(B):
                    n = min(to_sample - sampled[i], prior_ps)
                    if to_sample - sampled[i] - n == 1:
                        n = to_sample - sampled[i]
                    if n <= 0:
                        continue
                    sampled[i] += n
                    n_call = n
                calls.append((diffusion_index, n_call))
            else:
                sampled = [1024] * B
                calls.append((0, to_sample))
    return calls


def test_plan_reproduces_the_fixture_calls():
    from gsdd_amd.d3pm import purity_plan
    _, a, cfg = load_golden("purity_L64")
    ns = a["n_sample"].tolist()
    calls = purity_plan(ns, cfg["prior_ps"], len(ns))
    assert calls == [tuple(c) for c in a["calls"].tolist()]
    assert len(calls) == 42 and calls[-1] == (0, 1)
    assert sum(1 for t, _ in calls if t == 50) == 2 and sum(1 for t, _ in calls if t == 1) == 3        # split timesteps
    assert (98, 5) in calls                                                                            # the folded left-over
    assert sum(n for t, n in calls if t > 0) == 64


def test_plan_matches_a_literal_count_of_the_reference_loop():
    from gsdd_amd.d3pm import purity_plan
    T = 4
    for ns_t, ps in itertools.product(range(0, 14), range(1, 9)):
        for ns0 in (0, 1, 7):
            ns = [ns0, ns_t, 0, (ns_t * 2) % 5]
            assert purity_plan(ns, ps, T) == reference_calls(ns, ps, T), (ns, ps)
    assert purity_plan([0, 3], 2, 2) == [(1, 3)]                                    # one left over is folded in
    assert purity_plan([0, 4], 2, 2) == [(1, 2), (1, 2)]
    assert purity_plan([2, 0, 0], 5, 3) == [(0, 2)]                                 # no call at n_sample[t] == 0
    # 21 non-zero entries at t >= 1 with prior_ps above them: 21 purity calls and the plain step
    ns = [1] + [3, 0, 0, 0] * 21
    assert len(purity_plan(ns, 1024, len(ns))) == 22


def test_update_n_sample_lists_equal_the_reference(tiny_dm):
    from gsdd_amd.d3pm import reference_n_sample
    _, a, _ = load_golden("purity_L64")
    for name, (T, ps) in {"T10": (10, 1024), "T25": (25, 1024), "T50": (50, 1024), "T100_ps10": (100, 10), "T100": (100, 1024),
                          "T200": (200, 1024)}.items():
        want = a["ref_n_sample_" + name].tolist()
        assert reference_n_sample(T, ps) == want and len(want) == T, name
    assert reference_n_sample(20) is None
    assert sum(reference_n_sample(100)[1:]) == 1024                                 # the default list reveals 1024 tokens over t >= 1
    dm = tiny_dm
    assert (dm.prior_rule, dm.prior_ps, dm.prior_weight) == (0, 1024, 0)
    assert dm.n_sample == a["ref_n_sample_T100"].tolist()
    dm.prior_ps = 10
    dm.update_n_sample()
    assert dm.n_sample == a["ref_n_sample_T100_ps10"].tolist()
    dm.prior_ps = 1024
    dm.update_n_sample()


@pytest.fixture(scope="module")
def tiny_dm():
    """The d3pm_L64 fixture's architecture on the CPU: argument checking only, nothing is computed."""
    import gsdd_amd
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=32, spatial_size=[8, 8], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=64, block_activate="GELU2",
                                        content_spatial_size=[8, 8], condition_dim=512, diffusion_step=100)
    return gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2,
                                         content_seq_len=64)


def test_purity_rejections(tiny_dm):
    import gsdd_amd
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    good = [1] + [0] * 35 + [1] * 64                                             # 64 reveals over t >= 1
    go = lambda **kw: dm.sample(["a", "b"], None, cond, torch.zeros_like(cond), filter_ratio=kw.pop("filter_ratio", 0), **kw)

    def expect(match, **attrs):
        keep = {k: getattr(dm, k) for k in ("prior_rule", "prior_ps", "prior_weight", "n_sample")}
        dm.prior_rule, dm.n_sample = 2, list(good)
        fr = attrs.pop("filter_ratio", 0)
        for k, v in attrs.items():
            setattr(dm, k, v)
        try:
            with pytest.raises(gsdd_amd.GsddError, match=match):
                go(filter_ratio=fr)
        finally:
            for k, v in keep.items():
                setattr(dm, k, v)

    for bad in (3, -1, "2", 1.5, True):
        expect("prior_rule", prior_rule=bad)
    expect("filter_ratio", filter_ratio=0.5)
    expect("len\\(n_sample\\)", n_sample=good[:-1])
    expect("len\\(n_sample\\)", n_sample=None)
    expect("negative", n_sample=[1, -1] + good[2:])
    expect("prior_ps", prior_ps=0)
    expect("prior_ps", prior_ps=2.0)
    expect("prior_weight", prior_weight=-0.5)
    expect("n_sample\\[0\\]", n_sample=[1025] + good[1:])
    expect("over-subscribed", n_sample=[1] + [0] * 34 + [1] * 65)                   # 65 reveals for 64 tokens
    expect("over-subscribed", n_sample=dm.n_sample)                               # the reference's list for 1024 tokens at L = 64
    # a valid schedule gets as far as the device check (this module lives on the CPU); nothing was drawn
    expect("ROCm device")
    expect("ROCm device", prior_rule=1, prior_ps=3, prior_weight=2.5)
    assert dm.noise_stream == 0 and dm.prior_rule == 0
    # prior_rule = 0 ignores the other attributes (today's path), and sample_fast ignores all of them
    dm.n_sample, dm.prior_ps = None, -3
    try:
        with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):
            go()
        dm.prior_rule = 2
        with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):
            dm.sample_fast(["a", "b"], None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=torch.zeros_like(cond))
    finally:
        dm.prior_rule, dm.prior_ps = 0, 1024
        dm.update_n_sample()


def test_scaled_n_sample_properties():
    from gsdd_amd.d3pm import reference_n_sample, scaled_n_sample
    for T, ps in ((10, 1024), (25, 1024), (50, 1024), (100, 10), (100, 1024), (200, 1024)):
        ns = reference_n_sample(T, ps)
        total = sum(ns[1:])
        assert scaled_n_sample(ns, 1024) == ns                                   # the identity at L = L_ref
        for L in (64, 100, 777, 1024, 2048, 4096):
            out = scaled_n_sample(ns, L)
            assert len(out) == len(ns) and out[0] == ns[0] and min(out) >= 0
            assert sum(out[1:]) == int(np.floor(total * L / 1024 + 0.5)), (T, L)
            # cumulative rounding: every prefix (in chain order, t = T-1 downwards) is within half a token of the exact scaling
            acc_in, acc_out = np.cumsum(ns[:0:-1]), np.cumsum(out[:0:-1])
            assert np.all(np.abs(acc_out - acc_in * L / 1024) <= 0.5)
    assert sum(scaled_n_sample(reference_n_sample(100), 4096)[1:]) == 4096           # the lists reveal 1024 over t >= 1
    assert scaled_n_sample([3, 10, 10], 512, L_ref=1024) == [3, 5, 5]


def test_config_keys_reach_discrete_diffusion(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml", []).model.generator
    assert (gen.sample_prior_rule, gen.sample_prior_weight, gen.sample_prior_ps, gen.sample_prior_scale_schedule) == (None, None, None, False)
    gen = compose(os.path.join(REPO, "configs"), "eval.yaml",
                  ["model.generator.sample_prior_rule=2", "model.generator.sample_prior_weight=1.5", "model.generator.sample_prior_ps=8",
                   "model.generator.sample_prior_scale_schedule=true"]).model.generator
    assert (gen.sample_prior_rule, gen.sample_prior_weight, gen.sample_prior_ps, gen.sample_prior_scale_schedule) == (2, 1.5, 8, True)
    text = lambda texts: torch.zeros(len(texts), 512)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm)
    assert (dd.sample_prior_rule, dd.sample_prior_weight, dd.sample_prior_ps, dd.sample_prior_scale_schedule) == (None, None, None, False)
    dd = gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_prior_rule=gen.sample_prior_rule, sample_prior_weight=gen.sample_prior_weight,
                                    sample_prior_ps=gen.sample_prior_ps, sample_prior_scale_schedule=gen.sample_prior_scale_schedule)
    assert (dd.sample_prior_rule, dd.sample_prior_weight, dd.sample_prior_ps, dd.sample_prior_scale_schedule) == (2, 1.5, 8, True)
    for kw, match in (({"sample_prior_rule": 3}, "sample_prior_rule"), ({"sample_prior_rule": True}, "sample_prior_rule"),
                      ({"sample_prior_weight": -1}, "sample_prior_weight"), ({"sample_prior_ps": 0}, "sample_prior_ps"),
                      ({"sample_prior_ps": 1.5}, "sample_prior_ps"), ({"sample_prior_scale_schedule": 1}, "sample_prior_scale_schedule"),
                      ({"sample_prior_rule": 2, "sample_skip_step": 1}, "sample_skip_step")):
        with pytest.raises(gsdd_amd.GsddError, match=match):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, **kw)
    gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_prior_rule=0, sample_skip_step=1)       # rule 0 is plain sampling: allowed


def test_library_exports_the_purity_entry_points():
    import gsdd_amd
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for sym in ("gsdd_d3pm_purity_step", "gsdd_d3pm_purity_select", "gsdd_advance_plan"):
        assert sym in gsdd_amd.EXPORTS and f"int {sym}(" in header
    L = gsdd_amd.lib()                                   # (also checks both new descriptors against gsdd_abi_sizeof codes 4 and 5)
    assert L.gsdd_abi_sizeof(4) > 0 and L.gsdd_abi_sizeof(5) > 0 and L.gsdd_abi_sizeof(6) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_production_purity_kernel_registers():
    """d3pm_purity_kernel<16, true, MODE, false, 2> (K = 4096, no test hooks), the fused pass, the score pass and the draw pass: no
    scratch at two waves per SIMD, like the step kernel; the selection kernel's sort buffer is the 32 KB of 4096 (key, index) pairs."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "d3pm_purity.hip" in mod.SOURCES
    rows = mod.collect(["d3pm_purity.hip"])
    for mode in (0, 1, 2):
        r = [r for r in rows if r["kernel"].startswith(f"d3pm_purity_kernel<16, true, {mode}, false, 2>")]
        assert len(r) == 1, (mode, [x["kernel"] for x in rows])
        assert r[0]["scratch_bytes_per_lane"] == 0 and r[0]["vgprs"] <= 256 and r[0]["occupancy_waves_per_simd"] >= 2, r[0]
    sel = [r for r in rows if r["kernel"].startswith("purity_select_kernel")]
    assert len(sel) == 1 and sel[0]["scratch_bytes_per_lane"] == 0 and sel[0]["static_lds_bytes"] == 4096 * 8, sel


def select_numpy(w, u, n):
    """The selection kernel's rule in numpy: keys in fp32, the n largest, ties to the lower index (stable sort of the negated keys);
    positions of weight 0 are excluded."""
    w, u = np.asarray(w, dtype=np.float32), np.asarray(u, dtype=np.float32)
    with np.errstate(divide="ignore"):
        key = np.log(w) - np.log(-np.log(u + np.float32(1e-30)) + np.float32(1e-30))
    key = np.where(w > 0, key, -np.inf).astype(np.float32)
    return np.argsort(-key, kind="stable")[:n]


def test_selection_rule_is_a_draw_without_replacement():
    """4 weights, n = 2, 20 000 Philox streams: the frequency of every ordered pair (first pick, second pick) within 5 binomial standard
    deviations of its Plackett-Luce probability w_i / W * w_j / (W - w_i)."""
    from oracle import philox
    w = np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32)
    N = 20000
    counts = np.zeros((4, 4))
    for stream in range(N):
        i, j = select_numpy(w, philox.uniform_rows(99, stream, 1, 4)[0], 2)
        counts[i, j] += 1
    assert counts.sum() == N and np.all(np.diag(counts) == 0)
    W = float(w.sum())
    for i in range(4):
        for j in range(4):
            if i != j:
                p = float(w[i]) / W * float(w[j]) / (W - float(w[i]))
                sd = np.sqrt(N * p * (1 - p))
                assert abs(counts[i, j] - N * p) <= 5 * sd, (i, j, counts[i, j], N * p, sd)
    # ties go to the lower index; zero weights are never drawn
    assert select_numpy([1, 1, 1], [0.5, 0.5, 0.5], 2).tolist() == [0, 1]
    assert set(select_numpy([0, 1, 0, 1], [0.9, 0.1, 0.9, 0.2], 2).tolist()) == {1, 3}


def test_both_plans_answer_what_the_sampling_loop_asks():
    """n_steps, t0, q_sample and draws of SamplePlan and PurityPlan: the step count, the denoiser's first timestep, whether the chain
    starts from a q_sample draw, and the noise streams a run spends -- one per step plus the q_sample draw for a SamplePlan, two per
    call plus the closing plain step for a PurityPlan."""
    from gsdd_amd.d3pm import PurityPlan, SamplePlan, sample_plan
    read = lambda p: (p.n_steps, p.t0, bool(p.q_sample), p.draws)
    assert read(sample_plan(100)) == (100, 99, False, 100)
    assert read(sample_plan(100, start_step=50)) == (50, 49, True, 51)
    assert read(sample_plan(100, skip_step=3)) == (26, 99, False, 26)
    calls = ((99, 11), (99, 4), (97, 10))
    assert read(PurityPlan(calls, True, 2, 1.0)) == (3, 99, False, 7)
    assert read(PurityPlan(calls, False, 1, 0.0)) == (3, 99, False, 6)
    assert read(PurityPlan((), True, 1, 0.0)) == (0, 0, False, 1)
    assert read(PurityPlan((), False, 1, 0.0)) == (0, 0, False, 0)
    for p in (sample_plan(100), sample_plan(100, start_step=50), sample_plan(100, skip_step=3)):
        assert p.draws == p.n_steps + p.q_sample
    for p in (PurityPlan(calls, True, 2, 1.0), PurityPlan(calls, False, 1, 0.0), PurityPlan((), True, 1, 0.0)):
        assert p.draws == 2 * len(p.calls) + p.final
    # still the tuples they were
    assert SamplePlan._fields == ("t0", "n_steps", "dt", "post_skip", "q_sample") and PurityPlan._fields == ("calls", "final", "rule", "weight")
    assert sample_plan(100) == (99, 100, 1, 0, False) and PurityPlan(calls, True, 2, 1.0) == (calls, True, 2, 1.0)
