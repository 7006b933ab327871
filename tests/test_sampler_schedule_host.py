"""The sampler's issue schedule (gsdd_amd.d3pm.issue_schedule) against a transcription of the three host loops it replaced.

Before the sampler ran every plan as an op program it issued a chain through three code paths: a replay loop for plain, skip-step and
purity chains (plus a `finals` loop for the purity chain's closing step), a second loop for resample chains with a lazily captured jump
graph per lane, and eager loops.  `oracle` below writes those three paths down as explicit loops, with the two differences of DESIGN.md
applied: (a) an op kind that occurs once in the program is run eagerly and not captured, (b) a lane's first op is an entry of the
schedule like every later one instead of a part of the lane set-up loop (when the executor sets a lane up is its own business: the
list of issues is the same).  No GPU, no torch."""
import pytest

from gsdd_amd.d3pm import PurityPlan, issue_schedule, resample_plan, sample_plan

PLANS = {
    "plain_T1": sample_plan(1), "plain_T2": sample_plan(2), "plain_T5": sample_plan(5),
    "skip_1": sample_plan(5, skip_step=1), "skip_3": sample_plan(5, skip_step=3), "start_3": sample_plan(5, start_step=3),
    "resample_7_2_2": resample_plan(7, 2, 2), "resample_7_2_3": resample_plan(7, 2, 3), "resample_one_jump": resample_plan(5, 4, 2),
    "purity_empty": PurityPlan((), False, 2, 0.0), "purity_final_only": PurityPlan((), True, 2, 0.0),
    "purity_one_call": PurityPlan(((3, 4),), False, 2, 0.0),
    "purity_three_calls_final": PurityPlan(((4, 2), (4, 1), (2, 3)), True, 1, 0.0),
}
MODES = [(1, True), (2, True), (1, False)]          # (lanes, graphed): an eager or traced call runs in one lane


def first_op(lane, kind, recurs):
    """A lane's first op of a kind: eager (arguments are validated outside capture), then recorded if anything will replay it."""
    return [(lane, kind, "eager")] + ([(lane, kind, "capture")] if recurs else [])


def oracle(plan, lanes, graphed):
    """The (lane, kind, action) triples of the three former issue paths."""
    out = []
    if not graphed:                                 # 3. eager: one lane, every op in order, the purity chain's closing step last
        if hasattr(plan, "ops"):
            for kind, _ in plan.ops:
                out.append((0, kind, "eager"))
        else:
            kind = "reveal" if hasattr(plan, "calls") else "step"
            for _ in range(plan.n_steps):
                out.append((0, kind, "eager"))
            if getattr(plan, "final", False):
                out.append((0, "final", "eager"))
        return out
    if hasattr(plan, "ops"):                        # 2. resample: the step graph and a lazily captured jump graph per lane
        if plan.n_steps:
            for ln in range(lanes):                 # (b): issued from the lane-setup loop before
                out += first_op(ln, "step", plan.n_steps > 1)
        jump_seen = [False] * lanes
        for kind, _ in plan.ops[1:]:
            for ln in range(lanes):
                if kind == "step":
                    out.append((ln, "step", "replay"))
                elif not jump_seen[ln]:
                    out += first_op(ln, "jump", plan.n_jumps > 1)       # (a): a single jump is not captured
                    jump_seen[ln] = True
                else:
                    out.append((ln, "jump", "replay"))
        return out
    kind = "reveal" if hasattr(plan, "calls") else "step"               # 1. plain / skip / purity: replays, then the finals
    if plan.n_steps:
        for ln in range(lanes):
            out += first_op(ln, kind, plan.n_steps > 1)                 # (a): a single step / reveal is not captured
    for _ in range(plan.n_steps - 1):
        for ln in range(lanes):
            out.append((ln, kind, "replay"))
    if getattr(plan, "final", False):
        for ln in range(lanes):
            out.append((ln, "final", "eager"))
    return out


def test_programs():
    assert sample_plan(5).program == ("step",) * 5 and sample_plan(5, skip_step=3).program == ("step",) * 2
    assert sample_plan(5, start_step=3).program == ("step",) * 3 and sample_plan(1).program == ("step",)
    assert resample_plan(5, 4, 2).program == ("step",) * 4 + ("jump",) + ("step",) * 5
    for name in ("resample_7_2_2", "resample_7_2_3"):
        assert PLANS[name].program == tuple(kind for kind, _ in PLANS[name].ops)
    assert PLANS["purity_empty"].program == () and PLANS["purity_final_only"].program == ("final",)
    assert PLANS["purity_one_call"].program == ("reveal",)
    assert PLANS["purity_three_calls_final"].program == ("reveal", "reveal", "reveal", "final")


@pytest.mark.parametrize("lanes,graphed", MODES)
@pytest.mark.parametrize("name", list(PLANS))
def test_schedule_is_what_the_three_loops_issued(name, lanes, graphed):
    plan = PLANS[name]
    got = issue_schedule(plan.program, lanes, graphed)
    assert got == oracle(plan, lanes, graphed)
    for ln in range(lanes):
        mine = [(kind, action) for lane, kind, action in got if lane == ln]
        ran = [kind for kind, action in mine if action != "capture"]
        assert tuple(ran) == plan.program           # eager + replay entries: one per op, in program order
        captured = [kind for kind, action in mine if action == "capture"]
        assert len(captured) == len(set(captured))  # at most once per lane and kind
        for i, (kind, action) in enumerate(mine):
            if action == "capture":
                assert i > 0 and mine[i - 1] == (kind, "eager")
                assert plan.program.count(kind) > 1                     # a kind that occurs once is never captured
            if action == "replay":
                assert graphed and (kind, "capture") in mine[:i]
    if not graphed:
        assert all(action == "eager" for _, _, action in got)


def test_schedule_does_not_touch_torch():
    import inspect
    src = inspect.getsource(issue_schedule)
    assert "torch" not in src and "ops." not in src


def test_comparison_rejects_two_lanes_swapped_in_one_round():
    plan = PLANS["resample_7_2_2"]
    want = oracle(plan, 2, True)
    i = next(i for i, e in enumerate(want) if e == (0, "step", "replay"))
    assert want[i + 1] == (1, "step", "replay")
    wrong = want[:i] + [want[i + 1], want[i]] + want[i + 2:]
    assert wrong != want and sorted(wrong) == sorted(want)
    assert issue_schedule(plan.program, 2, True) != wrong
