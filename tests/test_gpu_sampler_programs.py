"""The smallest op programs at which "a kind is captured iff it recurs" can go wrong, on the MI355X: a purity chain of one reveal,
of one reveal plus the final step, of the final step alone, and a resample chain with a single jump.  Each runs graphed in two lanes,
graphed in one, eager and traced; the four must agree on the tokens, the noise streams spent and the trace's length.  d3pm_L64 golden
model at B = 8 (two lanes of 4)."""
import pytest
import torch

from tests.test_gpu_parity import build_d3pm

pytestmark = pytest.mark.gpu

B = 8


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def purity_case(reveal, final):
    def setup(dm, cfg):
        ns = [0] * cfg["T"]
        if reveal:
            ns[50] = 64
        if final:
            ns[0] = 1
        dm.n_sample, dm.prior_ps, dm.prior_rule = ns, 64, 2
        return {}, ("reveal",) * reveal + ("final",) * final
    return setup


def single_jump_case(dm, cfg):
    g = torch.Generator().manual_seed(11)
    content = torch.randint(0, cfg["K"], (B, cfg["L"]), generator=g)
    mask = torch.rand(B, cfg["L"], generator=g) < 0.4
    kw = dict(content_token=content.cuda(), known_mask=mask.cuda(), known_mode="hold", resample_jump=99, resample_times=2)
    return kw, ("step",) * 99 + ("jump",) + ("step",) * 100


CASES = {"one_reveal": purity_case(1, 0), "one_reveal_and_final": purity_case(1, 1), "final_only": purity_case(0, 1),
         "single_jump": single_jump_case}


@pytest.mark.parametrize("case", list(CASES))
def test_program_runs_the_same_in_every_mode(G, golden, case):
    sd, _, cfg = golden("d3pm_L64")
    assert cfg["T"] == 100 and cfg["L"] == 64
    dm = build_d3pm(G, sd, cfg)
    call_kw, program = CASES[case](dm, cfg)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    trace = []
    modes = {"graph": {}, "one_lane": {"lanes": 1}, "eager": {"use_graph": False}, "trace": {"trace": trace}}
    toks = {}
    for name, kw in modes.items():
        dm.set_noise(77, stream=3)
        toks[name] = dm.sample(["x"] * B, None, cond, cf, filter_ratio=0, **call_kw, **kw)["content_token"].cpu()
        plan = dm._last_plan
        assert plan.program == program
        assert dm.noise_stream - 3 == plan.draws == dm._last_draws, (name, dm.noise_stream, plan.draws)
        assert dm._last_lanes == (2 if name == "graph" else 1)
        if case == "single_jump":
            assert dm._last_jump_graphs == ([None] * dm._last_lanes if name in ("graph", "one_lane") else [])
        else:
            assert dm._last_jump_graphs == []
    assert len(trace) == len(program)
    for name in ("one_lane", "eager", "trace"):
        assert torch.equal(toks[name], toks["graph"]), (case, name, int((toks[name] != toks["graph"]).sum()))
    assert torch.equal(trace[-1].cpu(), toks["graph"])
    if case == "single_jump":
        assert int((toks["graph"] == cfg["K"]).sum()) == 0
    elif case == "one_reveal":                      # all 64 positions revealed by the one call
        assert int((toks["graph"] == cfg["K"]).sum()) == 0
