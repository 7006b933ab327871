"""Paired video metrics on the GPU (csrc/paired_metrics.hip, gsdd_amd.ops.paired_metrics, gsdd_amd.metrics.paired_frame_metrics, the
evaluator) against the fp64 restatement (tests/paired_ref.py).  The squared error is an integer: equality.  SSIM per plane is held to
4 e_win, e_win the worst per-window error against fp64 of an fp32 restatement that centres first, measured on the same case list
(tests/test_paired_host.py shows what that bound keeps out).  A workgroup owns a 16 x 16 tile of window positions: 11 x 11 is one
window, 12 x 16 less than a tile, 11 x 75 and 75 x 11 a row and a column of ragged tiles, 43 x 37 ragged both ways, 64 x 64 and 97 x 61
several tiles with the last ones ragged, 128 x 128 the workload's plane.  Measured on one MI355X: 0 of 3612 squared errors differ; the
worst plane's SSIM is 3.9e-8 from the restatement, 0.022 of the bound 4 e_win = 1.8e-6 (profiles/rV_parity_report.json)."""
import numpy as np
import pytest
import torch

import gif_ref
import paired_ref as ref
import stale_memory
from conftest import parity_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


@pytest.fixture(scope="module")
def yardstick(cases):
    """computed once for the module: (e_win, {case: ...}, {case: the rule's ssim (B, T, 3)})"""
    return ref.window_error(cases)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _operands(lv):
    """levels -> (form 0 on the device, form 1 on the device)"""
    return _dev(gif_ref.clips_from_levels(lv)), _dev(lv)


# ---------------------------------------------------------------------------------------------- the case list
def test_case_list_in_every_form_pairing(G, cases, yardstick):
    e_win, _, means = yardstick
    bound = 4.0 * e_win
    worst, worst_case, mism, compared = 0.0, None, 0, 0
    for name, a, b in cases:
        want_sse, want = ref.sse(a, b), means[name]
        first = None
        for fa, xa in enumerate(_operands(a)):
            for fb, xb in enumerate(_operands(b)):
                sse, ssim = G.ops.paired_metrics(xa, xb)
                assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and tuple(sse.shape) == tuple(ssim.shape) == a.shape[:2] + (3,)
                sse, ssim = sse.cpu().numpy(), ssim.cpu().numpy()
                mism += int(np.count_nonzero(sse != want_sse))
                compared += want_sse.size
                err = float(np.abs(ssim - want).max())
                if err > worst:
                    worst, worst_case = err, f"{name}_forms{fa}{fb}"
                if first is None:
                    first = ssim
                assert np.array_equal(ssim.view(np.int64), first.view(np.int64)), (name, fa, fb)         # the form changes no bit
                only = G.ops.paired_metrics(xa, xb, want_ssim=False)
                assert only[1] is None and np.array_equal(only[0].cpu().numpy(), want_sse), (name, fa, fb)
    print(f"sse: {mism} mismatches of {compared}; ssim: worst |kernel - fp64| = {worst:.3e} ({worst_case}), bound 4 e_win = {bound:.3e}")
    parity_report("paired_metrics", {"sse_mismatches": mism, "sse_compared": compared, "ssim_worst_abs_err": worst,
                                     "ssim_worst_case": worst_case, "e_win": e_win, "ssim_bound": bound,
                                     "ssim_err_over_bound": worst / bound, "cases": len(cases), "form_pairings": 4})
    assert mism == 0
    assert worst <= bound, (worst, worst_case)


def test_out_of_range_values_and_nan_in_the_float_form(G, cases, yardstick):
    bound = 4.0 * yardstick[0]
    for name, a, b in cases:
        if not name.endswith(("_12x16", "_43x37", "_97x61")) or not name.startswith(("noise10", "flat250", "step")):
            continue
        xa, xb = ref.float_operand(a, inject=True, seed=1), ref.float_operand(b, inject=True, seed=2)
        la, lb = ref.levels(xa), ref.levels(xb)
        assert not np.array_equal(la, a) and la.min() == 0 and la.max() == 255
        want = ref.frame_metrics(la, lb)
        for pa, pb in ((_dev(xa), _dev(xb)), (_dev(xa), _dev(lb)), (_dev(la), _dev(xb))):
            got = G.metrics.paired_frame_metrics(pa, pb)
            assert np.array_equal(got["sse"].numpy(), want["sse"]), name
            assert np.abs(got["ssim"].numpy() - want["ssim"]).max() <= bound, name
            assert np.allclose(got["psnr"].numpy(), want["psnr"], rtol=1e-12, atol=0), name


# ---------------------------------------------------------------------------------------------- exact properties
def test_identical_operands_score_exactly_one(G, cases):
    for name, a, _ in cases:
        if not name.startswith(("random", "flat250", "step")):
            continue
        f0, f1 = _operands(a)
        for xa, xb in ((f0, f0), (f1, f1.clone()), (f0, f1)):
            got = G.metrics.paired_frame_metrics(xa, xb)
            assert torch.all(got["ssim"] == 1.0) and torch.all(got["sse"] == 0) and torch.all(torch.isinf(got["psnr"])), name
            assert torch.all(G.ops.paired_metrics(xa, xb)[1] == 1.0), name


def test_a_sample_alone_and_a_second_call_give_the_same_bits(G, cases):
    for name, a, b in cases:
        if not name.startswith(("noise10", "ramp")) or a.shape[0] < 2:
            continue
        xa, xb = _operands(a)[0], _operands(b)[1]
        sse, ssim = G.ops.paired_metrics(xa, xb)
        sse2, ssim2 = G.ops.paired_metrics(xa, xb)
        assert stale_memory.same_bits(sse, sse2) and stale_memory.same_bits(ssim, ssim2), name
        for i in range(a.shape[0]):
            one = G.ops.paired_metrics(xa[i:i + 1].contiguous(), xb[i:i + 1].contiguous())
            assert stale_memory.same_bits(one[0], sse[i:i + 1]) and stale_memory.same_bits(one[1], ssim[i:i + 1]), (name, i)


# ---------------------------------------------------------------------------------------------- stale memory
def test_results_do_not_depend_on_what_the_partials_held(G, cases):
    by_name = {n: (a, b) for n, a, b in cases}
    for name in ("noise10_43x37", "step_97x61", "random_11x11"):
        a, b = by_name[name]
        xa, xb = _operands(a)[0], _operands(b)[1]
        H, W = a.shape[2:4]
        shape = (a.shape[0] * a.shape[1] * 3, G.ops.paired_metrics_tiles(H, W), 2)
        for want_ssim in (True, False):
            results = []
            for byte in stale_memory.BYTES:
                partials = torch.full(shape, byte * 0x01010101 - (1 << 32 if byte >= 0x80 else 0), dtype=torch.int32, device="cuda")
                assert partials.view(torch.uint8).eq(byte).all()
                sse, ssim = G.ops.paired_metrics(xa, xb, want_ssim=want_ssim, partials=partials)
                results.append(stale_memory.host_bits({"sse": sse, "partials": partials, **({"ssim": ssim} if want_ssim else {})}))
            fresh = G.ops.paired_metrics(xa, xb, want_ssim=want_ssim)
            assert stale_memory.same_bits(fresh[0], sse) and (not want_ssim or stale_memory.same_bits(fresh[1], ssim))
            for byte, r in zip(stale_memory.BYTES[1:], results[1:]):
                assert stale_memory.differing(results[0], r) == [], (name, want_ssim, hex(byte))
    # the call itself obtains no uninitialised memory: nothing of the package is filled under stale()
    a, b = by_name["noise10_43x37"]
    xa, xb = _operands(a)[0], _operands(b)[1]
    with stale_memory.stale(0xFF) as st:
        got = G.metrics.paired_frame_metrics(xa, xb)
        G.metrics.psnr(xa, xb)
    assert st.reached(stale_memory.P) == set() and np.array_equal(got["sse"].numpy(), ref.sse(a, b))


# ---------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_raise_before_anything_is_written(G):
    E = G.GsddError
    ok = torch.zeros((1, 3, 2, 16, 16), device="cuda")
    ok8 = torch.zeros((1, 2, 16, 16, 3), dtype=torch.uint8, device="cuda")
    partials = torch.full((6, 1, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    small = torch.zeros((1, 3, 2, 10, 16), device="cuda")
    calls = [lambda: G.ops.paired_metrics(small, small, partials=partials),                       # H = 10 with SSIM wanted
             lambda: G.ops.paired_metrics(ok, torch.zeros((1, 3, 2, 16, 17), device="cuda"), partials=partials),
             lambda: G.ops.paired_metrics(ok, ok8[:, :1].contiguous(), partials=partials),
             lambda: G.ops.paired_metrics(ok.double(), ok, partials=partials),                      # wrong dtype for either form
             lambda: G.ops.paired_metrics(ok, ok8.to(torch.int8), partials=partials),
             lambda: G.ops.paired_metrics(ok, torch.zeros((1, 2, 3, 16, 16), dtype=torch.uint8, device="cuda"), partials=partials),
             lambda: G.ops.paired_metrics(ok.transpose(3, 4), ok, partials=partials),               # not contiguous
             lambda: G.ops.paired_metrics(ok, ok8.transpose(2, 3), partials=partials),
             lambda: G.ops.paired_metrics(ok.cpu(), ok, partials=partials),                         # a CPU tensor
             lambda: G.ops.paired_metrics(ok, ok8.cpu(), partials=partials),
             lambda: G.ops.paired_metrics(ok, ok8, partials=partials.cpu()),
             lambda: G.ops.paired_metrics(ok, ok8, partials=partials.long()),
             lambda: G.ops.paired_metrics(ok, ok8, partials=partials[:, :, :1]),
             lambda: G.metrics.paired_frame_metrics(small, small)]
    for i, call in enumerate(calls):
        with pytest.raises(E):
            call()
        assert partials.eq(0x5A5A5A5A).all(), i
    # the squared error alone takes any plane
    for hw in ((1, 1), (5, 3), (10, 16)):
        lv = np.random.default_rng(hw[0]).integers(0, 256, (2, 3) + hw + (3,)).astype(np.uint8)
        lw = np.random.default_rng(hw[1] + 100).integers(0, 256, (2, 3) + hw + (3,)).astype(np.uint8)
        want = ref.sse(lv, lw)
        for xa in _operands(lv):
            sse, none = G.ops.paired_metrics(xa, _dev(lw), want_ssim=False)
            assert none is None and np.array_equal(sse.cpu().numpy(), want), hw
            got = G.metrics.psnr(xa, _dev(lw))
            assert got.dtype == torch.float64 and np.allclose(got.numpy(), ref.psnr(want, *hw), rtol=1e-12, atol=0), hw
        with pytest.raises(E):
            G.ops.paired_metrics(_dev(lv), _dev(lw))


# ---------------------------------------------------------------------------------------------- end to end
def test_written_gif_read_back_scores_as_its_palette_indices(G, tmp_path, yardstick):
    levels = np.concatenate([gif_ref.synthetic_levels(noise=True), gif_ref.synthetic_levels()])          # (2, 4, 32, 32, 3)
    clips = gif_ref.clips_from_levels(levels)
    dev = _dev(clips)
    paths = [str(tmp_path / f"{b}.gif") for b in range(2)]
    idx, pal, n = G.gif.write_gifs(dev, paths, fps=8, colors=64)
    shown = gif_ref.reconstruct(idx.cpu().numpy(), pal.cpu().numpy())                                # palette[indices]
    frames = torch.stack([G.gif.read_gif(p, "cuda")[0] for p in paths])
    assert frames.dtype == torch.uint8 and np.array_equal(frames.cpu().numpy(), shown)
    got = G.metrics.paired_frame_metrics(frames.contiguous(), dev)
    want = ref.frame_metrics(shown, clips)
    assert np.array_equal(got["sse"].numpy(), want["sse"]) and want["sse"].sum() > 0
    assert np.allclose(got["psnr"].numpy(), want["psnr"], rtol=1e-12, atol=0)
    assert np.abs(got["ssim"].numpy() - want["ssim"]).max() <= 4.0 * yardstick[0]
    # the whole clip's PSNR that the GIF tools print, from the same integers
    assert G.gif.psnr_from_sse(int(got["sse"].sum()), levels.size) == pytest.approx(gif_ref.psnr(shown, levels), rel=1e-12)


def test_evaluator_returns_the_means_of_the_direct_calls(G):
    import src  # noqa: F401
    from src.utils.evaluator import Evaluator, MeanPoolEncoder
    rng = np.random.default_rng(7)
    batches = []
    for i in range(2):
        target = rng.integers(0, 256, (3, 4, 32, 32, 3))
        pred = np.clip(np.rint(target + rng.normal(0, 6.0 * (i + 1), target.shape)), 0, 255)
        pred[:, :2] = target[:, :2]                             # two given frames, as a prediction run has them
        batches.append(({"video": torch.from_numpy(gif_ref.clips_from_levels(target.astype(np.uint8))), "text": ["x"] * 3},
                        _dev(gif_ref.clips_from_levels(pred.astype(np.uint8)))))
    plain = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32)
    ev = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True, paired_from_frame=2)
    whole = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True)
    for i, (batch, out) in enumerate(batches):
        for e in (plain, ev, whole):
            e.push_vals(batch, i, out)
    old, got = plain.evaluate_metrics(), ev.evaluate_metrics()
    assert set(old) == {"fvd"} and set(got) == {"fvd", "psnr", "ssim"} and got["fvd"] == old["fvd"]
    direct = [G.metrics.paired_frame_metrics(out, batch["video"].cuda()) for batch, out in batches]
    psnr, ssim = torch.cat([d["psnr"] for d in direct]), torch.cat([d["ssim"] for d in direct])
    assert got["psnr"] == float(psnr[:, 2:].mean()) and got["ssim"] == float(ssim[:, 2:].mean()) and np.isfinite(got["psnr"])
    assert torch.equal(ev.frame_curves()["psnr"], psnr.mean(dim=0)) and torch.equal(ev.frame_curves()["ssim"], ssim.mean(dim=0))
    assert torch.isinf(ev.frame_curves()["psnr"]).tolist() == [True, True, False, False]
    assert whole.evaluate_metrics()["psnr"] == float("inf") and whole.evaluate_metrics()["ssim"] == float(ssim.mean())
    want = [ref.frame_metrics(gif_ref.levels_of(out.cpu().numpy()), gif_ref.levels_of(batch["video"].numpy())) for batch, out in batches]
    assert np.array_equal(torch.cat([d["sse"] for d in direct]).numpy(), np.concatenate([w["sse"] for w in want]))
    ev.reset()
    assert ev.all_frame_psnr == [] and ev.all_frame_ssim == []
