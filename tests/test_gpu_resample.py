"""RePaint's resampling jumps (sample(..., resample_jump, resample_times); gsdd_d3pm_forward_jump) on the MI355X.

The kernel is compared with the fp64 restatement of tests/test_resample_host.py: a forward jump's token is a Gumbel arg-max over three
distinct log-probabilities, so tokens are compared exactly wherever the gap between the two best values of the fp64 draw is at least
1e-3 (the project's floor: 50 x the 2e-5 allowed between device and reference log-probabilities; here the device reads the same fp64-made
values rounded to f32, so the floor is generous), [MASK] inputs and hold positions always.  The chain is pinned by
tests/golden/resample_L64.npz (the reference's own functions driven through resample_plan, tests/golden/make_golden_resample.py),
teacher-forced op by op."""
import numpy as np
import pytest
import torch

from tests.conftest import parity_report
from tests.test_gpu_parity import build_d3pm
from tests.test_known_host import compared
from tests.test_resample_host import (CASE, FREQ, FREQ_STREAM, JUMPS, WIDTHS, all_mask_case, case_levels, case_seed, freq_bands,
                                      freq_inputs, verdict)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def dev(x):
    return torch.as_tensor(x).cuda()


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def jump(G, tok, levels, jmp, *, K, T, seed, stream, row0=0, hold=None, in_place=False):
    from gsdd_amd.d3pm import jump_table
    tin = dev(tok).clone()
    out = tin if in_place else torch.full_like(tin, -7)
    G.ops.d3pm_forward_jump(tin, out, jump_table(T, K, jmp).cuda(), i64(list(levels)), i64([stream]), K=K, T=T, jump=jmp, seed=seed,
                            row0=row0, hold=None if hold is None else dev(hold).to(torch.uint8))
    return out.cpu()


# ----------------------------------------------------------------------------- 1. the kernel at every class width
@pytest.mark.parametrize("jmp", JUMPS)
@pytest.mark.parametrize("K", WIDTHS)
def test_kernel_against_fp64_at_every_class_width(G, K, jmp):
    """3 x 37 positions from global row 1000, the rows at from-levels (-1, 39, T - 1 - jump), a third [MASK] inputs, codes 0 and K - 1,
    a hold mask; then 111 [MASK] inputs from the clean level, where a redrawn [MASK] would show."""
    T = CASE["T"]
    s, tok, hold, want, gap = case_seed(K, jmp)
    kw = dict(K=K, T=T, seed=CASE["seed"], stream=CASE["stream"], row0=CASE["row0"])
    got = jump(G, tok, case_levels(jmp), jmp, hold=hold, **kw)
    same = jump(G, tok, case_levels(jmp), jmp, hold=hold, in_place=True, **kw)
    rec = verdict(got, want, gap, tok, hold, K)
    rec.update(input_seed=s, in_place_differs=int((same != got).sum()), to_mask=int(((got == K) & (tok != K)).sum()),
               kept=int(((got == tok) & (tok != K) & ~hold).sum()), other=int(((got != tok) & (got != K)).sum()))
    mtok, mlev, mjump, mwant, mgap = all_mask_case(K)
    rec["all_mask_changed"] = verdict(jump(G, mtok, mlev, mjump, **kw), mwant, mgap, mtok, None, K)["through_changed"]
    print(K, jmp, rec)
    parity_report(f"resample_width_{K}_j{jmp}", rec)
    assert rec["left_out"] <= CASE["max_left_out"]
    assert rec["mismatches"] == 0 and rec["through_changed"] == 0 and rec["out_of_range"] == 0
    assert rec["in_place_differs"] == 0 and rec["all_mask_changed"] == 0
    assert rec["to_mask"] > 0                        # the row that lands on level T - 1 is all [MASK] (gamma-bar there is 0.99999)
    no_hold = jump(G, tok, case_levels(jmp), jmp, **kw)
    assert torch.equal(no_hold[~hold], got[~hold])  # the hold mask changes nothing anywhere else


# ----------------------------------------------------------------------------- 2. the level of the draw
def test_shares_are_those_of_the_jump(G):
    """8192 code positions at K = 32, level 39, jump 10: the [MASK] share within 5 binomial standard deviations of gamma~ and the kept
    share within 5 of alpha~ + beta~ (a table row taken at 49 would give gamma~ = 0.20 instead of 0.17: 7 sigma away)."""
    tok, want, gap = freq_inputs(FREQ_STREAM)
    (pm, sm), (ph, sh) = freq_bands()
    got = jump(G, tok, [FREQ["level"]], FREQ["jump"], K=FREQ["K"], T=FREQ["T"], seed=FREQ["seed"], stream=FREQ_STREAM)
    ok, left_out = compared(gap.numpy())
    rec = {"mask_share": float((got == FREQ["K"]).float().mean()), "gamma": pm, "mask_band": 5 * sm,
           "kept_share": float((got == tok).float().mean()), "alpha_plus_beta": ph, "kept_band": 5 * sh,
           "left_out_share": left_out, "mismatches": int((got != want).numpy()[ok].sum())}
    print(rec)
    parity_report("resample_shares", rec)
    assert abs(rec["mask_share"] - pm) <= 5 * sm and abs(rec["kept_share"] - ph) <= 5 * sh
    assert rec["mismatches"] == 0


# ----------------------------------------------------------------------------- 3. the fixture's chains, teacher-forced
@pytest.mark.parametrize("mode", ["renoise", "hold"])
def test_teacher_forced_chain_reproduces_the_fixture(G, golden, mode):
    """Op i from the fixture's trace[i-1] at stream i must give trace[i], steps and jumps alike, at every position whose decision the
    reference itself made at least the floor away from a flip."""
    from gsdd_amd.d3pm import check_known, jump_table, resample_plan
    sd, b, cfg = golden("d3pm_L64")
    _, a, rcfg = golden("resample_L64")
    dm = build_d3pm(G, sd, cfg)
    B, L, K, T = cfg["B"], cfg["L"], cfg["K"], cfg["T"]
    plan = resample_plan(T, rcfg[f"jump_{mode}"], rcfg[f"times_{mode}"])
    known, x_known = torch.from_numpy(a["known"]), torch.from_numpy(a["x_known"].astype(np.int64))
    cond = dev(b["step_cond"])
    cf = torch.zeros_like(cond)
    seed = rcfg["noise_seed"]
    dm.set_noise(seed)
    kn = check_known(known, x_known, mode, B=B, L=L, K=K)
    kn = (kn[0].cuda(), kn[1].cuda(), kn[2])
    hold = kn[0].to(torch.uint8).contiguous() if mode == "hold" else None
    table = jump_table(T, K, plan.jump).cuda()
    trace = a[f"trace_{mode}"].astype(np.int64)
    ok, left_out = compared(a[f"gap_{mode}"])
    bad = []
    for i, (kind, lvl) in enumerate(plan.ops):
        prev = torch.full((B, L), K, dtype=torch.int64, device="cuda") if i == 0 else dev(trace[i - 1])
        if kind == "step":
            got = dm.p_sample_tokens(prev, cond, cf, i64([lvl] * B), i, known=kn)
        else:
            got = G.ops.d3pm_forward_jump(prev, torch.empty_like(prev), table, i64([lvl] * B), i64([i]), K=K, T=T, jump=plan.jump,
                                          seed=seed, hold=hold)
        n = int((got.cpu().numpy() != trace[i])[ok[i]].sum())
        if n:
            bad.append((i, kind, n))
    rec = {"ops": plan.draws, "jumps": plan.n_jumps, "positions": int(ok.size), "left_out_share": left_out,
           "mismatches": int(sum(n for _, _, n in bad))}
    print(rec)
    parity_report(f"resample_teacher_forced_{mode}", rec)
    assert not bad, f"(op, kind, mismatching positions): {bad[:10]}"


# ----------------------------------------------------------------------------- 4. free-running properties
@pytest.mark.parametrize("mode,jmp,times", [("renoise", 10, 2), ("hold", 30, 3)])
def test_free_running_properties(G, golden, mode, jmp, times):
    from gsdd_amd.d3pm import resample_plan
    sd, a, cfg = golden("d3pm_L64")
    K, L, T, B = cfg["K"], cfg["L"], cfg["T"], 8
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    cf = torch.randn(B, 1, cfg["cond_dim"], generator=g).cuda()
    content = torch.randint(0, K, (B, L), generator=g)
    mask = torch.rand(B, L, generator=g) < 0.4
    mask[:, :16] = True                                                     # the first frame of the 4 x 4 x 4 grid
    dm = build_d3pm(G, sd, cfg)
    plan = resample_plan(T, jmp, times)

    def go(stream=4, rows=slice(None), row_offset=0, **kw):
        dm.set_noise(31, stream=stream, row_offset=row_offset)
        n = content[rows].shape[0]
        out = dm.sample(["a"] * n, None, cond[rows], cf[rows], filter_ratio=0, content_token=content[rows].cuda(),
                        known_mask=mask[rows].cuda(), known_mode=mode, **kw)["content_token"]
        return out.cpu(), dm.noise_stream - stream, dm._last_lanes
    known_plain, draws_plain, _ = go()
    rs = dict(resample_jump=jmp, resample_times=times)
    toks, n, lanes = go(**rs)
    assert lanes == 2 and n == plan.draws == dm._last_plan.draws and dm._last_plan == plan      # one stream per step and per jump
    assert len(dm._last_jump_graphs) == 2 and all(gr is not None for gr in dm._last_jump_graphs)
    assert torch.equal(toks[mask], content[mask])                           # the known positions end on their tokens
    assert int((toks == K).sum()) == 0 and not torch.equal(toks[~mask], known_plain[~mask])
    # one lane, two lanes and the eager chain: the same tokens and the same stream count
    one, n1, lanes1 = go(**rs, lanes=1)
    trace = []
    eager, n2, _ = go(**rs, trace=trace)
    unc, n3, _ = go(**rs, use_graph=False)
    assert lanes1 == 1 and n1 == n2 == n3 == plan.draws and len(trace) == plan.draws
    assert torch.equal(one, toks) and torch.equal(eager, toks) and torch.equal(unc, toks) and torch.equal(trace[-1].cpu(), toks)
    # the trace has one entry per op: a jump only adds [MASK], the first one adds some, and hold keeps the known positions throughout
    for i, (kind, _) in enumerate(plan.ops):
        if kind == "jump":
            before, after = trace[i - 1].cpu(), trace[i].cpu()
            assert bool((after[before == K] == K).all())
            if mode == "hold":
                assert torch.equal(after[mask], content[mask])
    first = [i for i, (kind, _) in enumerate(plan.ops) if kind == "jump"][0]
    assert int((trace[first].cpu() == K).sum()) > int((trace[first - 1].cpu() == K).sum())
    # times = 1 (and no jump at all) is the plain known call bit for bit, stream count included
    t1, n4, _ = go(resample_jump=jmp, resample_times=1)
    assert torch.equal(t1, known_plain) and n4 == draws_plain == T
    # a shard of the batch at its row offset equals the full batch's rows
    shard, n5, _ = go(rows=slice(4, 8), row_offset=4, **rs)
    assert torch.equal(shard, toks[4:8]) and n5 == plan.draws
    # and the plain known call after all of this still is what it was
    again, _, _ = go()
    assert torch.equal(again, known_plain) and dm._last_jump_graphs == []                 # (and it holds no jump graph of an earlier call)


# ----------------------------------------------------------------------------- 5. the generator glue
def test_glue_resamples_with_the_first_frame_given(G, golden):
    from tests.test_gpu_glue import build
    gen, vq, batch, a, cfg, cfgd = build(G, golden)
    gen = G.DiscreteDiffusion(gen.textencoder, gen.diffusion_model, sample_condition_frames=1, sample_resample_jump=10,
                              sample_resample_times=2)
    dm = gen.diffusion_model.eval()
    dm.set_noise(cfg["noise_seed"], stream=int(cfg["stream"]))
    with torch.no_grad():
        quant = vq.encode(batch["video"])
        out = gen(batch, vq, None, do_inference=True)
        pred = out["pred_data"]
    B = quant.shape[0]
    per_frame = quant[0, 0].numel()
    tok = gen.last_content_token
    assert dm._last_plan.n_jumps == 9 and dm._last_plan.n_steps == 190
    assert torch.equal(tok[:, :per_frame], quant.view(B, -1)[:, :per_frame])             # the first latent frame carries the input's codes
    assert not torch.equal(tok[:, per_frame:], quant.view(B, -1)[:, per_frame:]) and int((tok == cfgd["K"]).sum()) == 0
    assert pred.shape == batch["video"].shape and bool(torch.isfinite(pred).all())
    with torch.no_grad():
        torch.testing.assert_close(pred, vq.decode(tok.view(quant.shape)), atol=0, rtol=0)
