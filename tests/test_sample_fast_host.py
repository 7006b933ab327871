"""sample_fast's host side (no GPU): the step plan against the reference's own timestep list, the argument errors raised before any
device work, the config switch, and the register budget of the production step kernel that now also reads `post_skip`."""
import importlib.util
import os
import shutil

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def reference_schedule(T, skip_step):
    """diffusion_transformer.py:692-704, restated literally: the denoiser's timesteps and the posterior's."""
    start_step = T
    diffusion_list = [index for index in range(start_step - 1, -1, -1 - skip_step)]
    if diffusion_list[-1] != 0:
        diffusion_list.append(0)
    post = [index - skip_step if index > skip_step else index for index in diffusion_list]
    return diffusion_list, post


@pytest.mark.parametrize("T", [2, 20, 25, 50, 100])
def test_plan_matches_the_reference_timestep_list(T):
    from gsdd_amd.d3pm import plan_timesteps, sample_plan
    for s in range(0, T + 3):
        plan = sample_plan(T, skip_step=s)
        want_t, want_post = reference_schedule(T, s)
        got = plan_timesteps(plan)
        assert [t for t, _ in got] == want_t, (T, s)
        assert [tp for _, tp in got] == want_post, (T, s)
        assert plan.n_steps == len(want_t) and plan.t0 == T - 1 and plan.dt == 1 + s and plan.post_skip == s
        assert not plan.q_sample
        assert all(0 <= tp <= t < T for t, tp in got)


def test_plan_step_counts_at_T100():
    from gsdd_amd.d3pm import sample_plan
    want = {1: 51, 2: 34, 3: 26, 4: 21, 9: 11, 98: 2, 99: 2, 250: 2}
    assert {s: sample_plan(100, skip_step=s).n_steps for s in want} == want
    # skip_step = 0 is sample(filter_ratio=0); start_step > 0 is sample(filter_ratio > 0)
    assert sample_plan(100) == sample_plan(100, skip_step=0) == (99, 100, 1, 0, False)
    assert sample_plan(100, start_step=30) == (29, 30, 1, 0, True)


@pytest.fixture(scope="module")
def tiny_dm():
    """The d3pm_L64 fixture's architecture on the CPU: argument checking only, nothing is computed."""
    import gsdd_amd
    d = gsdd_amd.DalleMaskImageEmbedding(num_embed=32, spatial_size=[8, 8], embed_dim=64)
    tr = gsdd_amd.Text2ImageTransformer(dalle=d, n_layer=2, n_embd=64, n_head=16, content_seq_len=64, block_activate="GELU2",
                                        content_spatial_size=[8, 8], condition_dim=512, diffusion_step=100)
    return gsdd_amd.DiffusionTransformer(transformer=tr, diffusion_step=100, alpha_init_type="alpha1", guidance_scale=2,
                                         content_seq_len=64)


def test_sample_fast_argument_errors(tiny_dm):
    import gsdd_amd
    dm = tiny_dm
    cond = torch.zeros(2, 1, 512)
    kw = dict(cf_condition_embed=torch.zeros(2, 1, 512))
    with pytest.raises(gsdd_amd.GsddError, match="filter_ratio"):
        dm.sample_fast(["a", "b"], None, cond, **kw)                                 # the default 0.5, as upstream's assert
    with pytest.raises(gsdd_amd.GsddError, match="filter_ratio"):
        dm.sample_fast(["a", "b"], None, cond, filter_ratio=0.01, **kw)              # int(100 * 0.01) = 1
    for bad in (-1, 1.0, "1", True, False, None):
        with pytest.raises(gsdd_amd.GsddError, match="skip_step"):
            dm.sample_fast(["a", "b"], None, cond, filter_ratio=0, skip_step=bad, **kw)
    with pytest.raises(gsdd_amd.GsddError, match="cf_condition_embed"):
        dm.sample_fast(["a", "b"], None, cond, filter_ratio=0, skip_step=1)
    with pytest.raises(NotImplementedError):
        dm.sample_fast(["a", "b"], None, cond, filter_ratio=0, skip_step=1, return_logits=True, **kw)
    # valid arguments get as far as the device check (this module lives on the CPU)
    with pytest.raises(gsdd_amd.GsddError, match="ROCm device"):
        dm.sample_fast(["a", "b"], None, cond, filter_ratio=0, skip_step=1, **kw)
    assert dm.noise_stream == 0


def test_discrete_diffusion_skip_step_switch(tiny_dm, monkeypatch):
    import gsdd_amd
    from gsdd_amd.hydra_lite import compose
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", [])
    assert cfg.model.generator.sample_skip_step is None
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", ["model.generator.sample_skip_step=1"])
    assert cfg.model.generator.sample_skip_step == 1
    text = lambda texts: torch.zeros(len(texts), 512)
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm).sample_skip_step is None
    assert gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_skip_step=3).sample_skip_step == 3
    for bad in (-1, 1.5, True):
        with pytest.raises(gsdd_amd.GsddError, match="sample_skip_step"):
            gsdd_amd.DiscreteDiffusion(text, tiny_dm, sample_skip_step=bad)


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_production_step_kernel_registers():
    """d3pm_step_kernel<16, true, false, 2> (K = 4096, no test hooks): the posterior's t' is one more scalar; the kernel must stay
    without scratch at two waves per SIMD."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = [r for r in mod.collect(["d3pm_step.hip"]) if r["kernel"].startswith("d3pm_step_kernel<16, true, false, 2>")]
    assert len(rows) == 1, rows
    r = rows[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgprs"] <= 256 and r["occupancy_waves_per_simd"] >= 2, r
