"""Paired video metrics, the part that needs no GPU: the restatement of the rule (tests/paired_ref.py) against an independent
formulation, the yardstick the GPU test judges the kernel by and the conditions that keep it honest, the entry's argument checks (they
return before anything is launched), the evaluator's plumbing on a stub, the config, and the documents."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gif_ref
import paired_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


@pytest.fixture(scope="module")
def yardstick(cases):
    """(e_win, {case: worst window error of the centred fp32 form}, {case: the rule's plane means})"""
    return ref.window_error(cases)


# ---------------------------------------------------------------------------------------------- the definition
def _conv_ssim(a, b):
    """the rule once more, in torch fp64 through conv2d: raw second moments, and the window's weight sum where the rule needs it --
    sum w (a - mu_a)(b - mu_b) = sum w a b - (2 - sum w) mu_a mu_b"""
    g = torch.from_numpy(ref.G32.astype(np.float64))
    w = torch.outer(g, g)[None, None]
    k = 2.0 - float(w.sum())
    pa = torch.from_numpy(ref.planes(a)).flatten(0, 2)[:, None]
    pb = torch.from_numpy(ref.planes(b)).flatten(0, 2)[:, None]
    conv = lambda x: torch.nn.functional.conv2d(x, w)[:, 0]     # noqa: E731
    mu_a, mu_b = conv(pa), conv(pb)
    var_a, var_b, cov = conv(pa * pa) - k * mu_a * mu_a, conv(pb * pb) - k * mu_b * mu_b, conv(pa * pb) - k * mu_a * mu_b
    s = (2 * mu_a * mu_b + ref.C1) * (2 * cov + ref.C2) / ((mu_a ** 2 + mu_b ** 2 + ref.C1) * (var_a + var_b + ref.C2))
    return s.mean(dim=(-2, -1)).reshape(a.shape[0], a.shape[1], 3).numpy()


def test_restatement_agrees_with_a_conv2d_formulation(cases, yardstick):
    worst = 0.0
    for name, a, b in cases:
        got = yardstick[2][name]
        assert got.shape == a.shape[:2] + (3,) and got.dtype == np.float64
        worst = max(worst, float(np.abs(got - _conv_ssim(a, b)).max()))
    print(f"restatement against conv2d, worst plane mean: {worst:.3e}")
    assert worst <= 1e-12
    # the weights: eleven fp32 values, symmetric, that sum to 1 - 1.4e-9 -- the header prints the first six
    assert ref.G32.dtype == np.float32 and np.array_equal(ref.G32, ref.G32[::-1])
    assert [float(v).hex() for v in ref.G32[:6]] == ["0x1.0d956c0000000p-10", "0x1.f1fe020000000p-8", "0x1.26eb180000000p-5",
                                                     "0x1.bff0fe0000000p-4", "0x1.b43c400000000p-3", "0x1.1065600000000p-2"]
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    kernel = open(os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc", "paired_metrics.hip")).read()
    for v in ref.G32[:6]:
        mantissa, exponent = float(v).hex().split("p")
        short = mantissa.rstrip("0") + "p" + exponent           # 0x1.0d956c0000000p-10 -> 0x1.0d956cp-10
        assert short in header and short + "f" in kernel, short


def test_known_values_of_the_rule(cases):
    by_name = {n: (a, b) for n, a, b in cases}
    a, b = by_name["identical_43x37"]
    assert np.all(ref.ssim(a, b) == 1.0) and np.all(ref.sse(a, b) == 0) and np.all(np.isinf(ref.frame_metrics(a, b)["psnr"]))
    a, b = by_name["black_white_12x16"]
    # mu_a = 0, every moment of a is 0: s = C1 C2 / ((mu_b^2 + C1) C2)
    mu = 255.0 * float(ref.G32.astype(np.float64).sum()) ** 2
    assert np.abs(ref.ssim(a, b) - ref.C1 / (mu * mu + ref.C1)).max() <= 1e-15
    assert np.all(ref.sse(a, b) == 255 * 255 * 12 * 16) and np.all(ref.frame_metrics(a, b)["psnr"] == 0.0)
    # either form of an operand has the same levels; injected values clamp
    a, b = by_name["noise10_12x16"]
    assert np.array_equal(ref.levels(ref.float_operand(a)), a)
    x = ref.float_operand(a, inject=True)
    assert np.isnan(x).any() and np.isinf(x).any() and not np.array_equal(ref.levels(x), a)
    assert np.array_equal(ref.sse(x, b), ref.sse(ref.levels(x), b))


def test_psnr_is_gif_refs_on_the_levels(cases):
    for name, a, b in cases:
        got = {"sse": ref.sse(a, b)}
        got["psnr"] = ref.psnr(got["sse"], a.shape[2], a.shape[3])
        for bi in range(a.shape[0]):
            for t in range(a.shape[1]):
                want = gif_ref.psnr(a[bi, t], b[bi, t])
                assert got["psnr"][bi, t] == want or abs(got["psnr"][bi, t] - want) <= 1e-12 * abs(want), (name, bi, t)
        assert np.array_equal(got["sse"].sum(axis=-1), ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(axis=(2, 3, 4)))


def test_library_psnr_helper_agrees(cases):
    """gsdd_amd.metrics forms the PSNR on the host from the kernel's integers: the same numbers as the restatement's"""
    from gsdd_amd.metrics import _frame_psnr
    for name, a, b in cases[:14]:
        e = ref.sse(a, b)
        got = _frame_psnr(torch.from_numpy(e), 3 * a.shape[2] * a.shape[3]).numpy()
        want = ref.psnr(e, a.shape[2], a.shape[3])
        assert got.dtype == np.float64 and np.array_equal(np.isinf(got), np.isinf(want)), name
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max(initial=0.0) <= 1e-12, name


# ---------------------------------------------------------------------------------------------- the yardstick
def test_yardstick_and_the_conditions_that_keep_it_honest(cases, yardstick):
    """The GPU bound on a plane's SSIM is 4 e_win, e_win the worst per-window error against fp64 of an fp32 form that centres first
    (measured here: 4.5e-7 on the case list, bound 1.8e-6).  It is only worth something if it tells the rule from what it must not be:
    the naive one-pass fp32 form on flat bright and step content (seen: 2.0e-4 and 3.9e-5 on a plane mean), and the rule with a fault
    -- zero-padded windows (0.49), a uniform window (0.30), sigma 1.0 (0.23), C2 of a data range of 1 (1.2)."""
    e_win, per_case, means = yardstick
    bound = 4.0 * e_win
    print(f"e_win = {e_win:.3e} (worst case {max(per_case, key=per_case.get)}), bound = {bound:.3e}")
    assert 0.0 < e_win < 2e-6                                   # an fp32 form that centres first: a few ulps of 1
    for kind in ("flat250", "step"):
        worst = 0.0
        for name, a, b in cases:
            if name.startswith(kind):
                naive = ref.ssim_naive_fp32(ref.planes(a), ref.planes(b)).astype(np.float64).mean(axis=(-2, -1))
                worst = max(worst, float(np.abs(naive - means[name]).max()))
        print(f"naive one-pass fp32 on {kind}: {worst:.3e} = {worst / bound:.1f} bounds")
        assert worst > bound, kind
    for fault, kwargs in ref.FAULTS.items():
        small = [c for c in cases if c[1].shape[2] * c[1].shape[3] <= 43 * 37]           # one case has to show it: the small planes do
        worst = max(float(np.abs(ref.ssim(a, b, **kwargs) - means[name]).max()) for name, a, b in small)
        print(f"fault {fault}: {worst:.3e} = {worst / bound:.0f} bounds")
        assert worst >= 10.0 * bound, fault


# ---------------------------------------------------------------------------------------------- the entry's argument checks
def test_entry_rejects_bad_arguments_before_any_launch():
    import gsdd_amd
    L = gsdd_amd.lib()
    assert L.gsdd_version() >= 115
    assert [L.gsdd_paired_metrics_tiles(h, w) for h, w in ((1, 1), (11, 11), (26, 26), (27, 26), (43, 37), (128, 128), (5, 3))] == \
        [1, 1, 1, 2, 6, 64, 1]
    assert L.gsdd_paired_metrics_tiles(0, 5) == -1 and L.gsdd_paired_metrics_tiles(5, -1) == -1
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)                                   # never read: every call below returns from its checks
    ok = [p, 0, p, 1, 2, 3, 16, 16, 1, p]
    for j, bad in ((0, None), (2, None), (9, None), (1, 2), (1, -1), (3, 2), (4, 0), (5, 0), (6, 0), (7, -3), (8, 2), (8, -1),
                   (6, 10), (7, 10),                            # SSIM needs an 11 x 11 window
                   (0, p + 2), (9, p + 1),                      # a float operand and the partials are 4-byte aligned
                   (6, 65536), (4, 1 << 30)):                   # 2^31 pixels in a plane; 2^31 planes
        args = ok[:j] + [bad] + ok[j + 1:]
        if (j, bad) == (6, 65536):
            args[7] = 32768
        assert L.gsdd_paired_metrics(*args, None) == -1, (j, bad)
        assert b"gsdd_paired_metrics" in L.gsdd_last_error()
    assert L.gsdd_paired_metrics(p, 0, p, 0, 1 << 16, 1 << 8, 128, 128, 0, p, None) == -1         # 3 * 2^24 planes of 64 tiles
    assert b"too many workgroups" in L.gsdd_last_error()
    assert L.gsdd_paired_metrics(p, 0, p, 0, 1, 1, 10, 10, 1, p, None) == -1 and b"11" in L.gsdd_last_error()
    E = gsdd_amd.GsddError
    x = torch.zeros((1, 3, 2, 16, 16))
    with pytest.raises(E, match="ROCm device"):
        gsdd_amd.ops.paired_metrics(x, x)
    with pytest.raises(E, match="float32 .* or uint8"):
        gsdd_amd.ops.paired_metrics(x.double(), x)
    with pytest.raises(E, match="float32 .* or uint8"):
        gsdd_amd.ops.paired_metrics(torch.zeros((1, 2, 16, 16, 4), dtype=torch.uint8), x)
    with pytest.raises(E):
        gsdd_amd.metrics.paired_frame_metrics(x, x)
    with pytest.raises(E):
        gsdd_amd.metrics.psnr(x, x)


# ---------------------------------------------------------------------------------------------- the evaluator
def _stub(pred, target):
    """stands in for metrics.paired_frame_metrics on the host: per frame, numbers that depend on the frame and the sample"""
    d = (pred.double() - target.double()).abs().mean(dim=(1, 3, 4))                # (B, T)
    return {"psnr": 40.0 - d, "ssim": 1.0 / (1.0 + d), "sse": torch.zeros(d.shape + (3,), dtype=torch.int64)}


def _batches():
    g = torch.Generator().manual_seed(1)
    return [({"video": torch.randn((4, 3, 6, 16, 16), generator=g), "text": ["a"] * 4}, torch.randn((4, 3, 6, 16, 16), generator=g))
            for _ in range(3)]


def test_evaluator_scores_pairs_only_when_asked(monkeypatch):
    import src  # noqa: F401
    import src.utils.evaluator as E
    monkeypatch.setattr(E.Evaluator, "_prepare", lambda self, clips: clips.float())
    calls = []
    monkeypatch.setattr(E, "paired_frame_metrics", lambda p, t: calls.append((p, t)) or _stub(p, t))
    batches = _batches()
    plain = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32)
    assert plain.paired_metrics is False and plain.paired_from_frame == 0
    for i, (batch, out) in enumerate(batches):
        plain.push_vals(batch, i, out)
    old = plain.evaluate_metrics()
    assert set(old) == {"fvd"} and calls == [] and plain.all_frame_psnr == []
    with pytest.raises(ValueError, match="paired_metrics"):
        plain.frame_curves()

    per_frame = [_stub(out, batch["video"]) for batch, out in batches]
    psnr, ssim = torch.cat([m["psnr"] for m in per_frame]), torch.cat([m["ssim"] for m in per_frame])     # (12, 6)
    for start in (0, 4, 5):
        ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True, paired_from_frame=start)
        del calls[:]
        for i, (batch, out) in enumerate(batches):
            ev.push_vals(batch, i, out)
        assert len(calls) == 3 and all(p.dtype == torch.float32 and p.is_contiguous() and t.is_contiguous() for p, t in calls)
        assert torch.equal(calls[1][0], batches[1][1]) and torch.equal(calls[1][1], batches[1][0]["video"])      # (pred, target)
        got = ev.evaluate_metrics()
        assert set(got) == {"fvd", "psnr", "ssim"} and got["fvd"] == old["fvd"]
        assert got["psnr"] == float(psnr[:, start:].mean()) and got["ssim"] == float(ssim[:, start:].mean())
        curves = ev.frame_curves()                              # all frames, whatever the scalar leaves out
        assert set(curves) == {"psnr", "ssim"} and tuple(curves["psnr"].shape) == (6,) and curves["psnr"].dtype == torch.float64
        assert torch.equal(curves["psnr"], psnr.mean(dim=0)) and torch.equal(curves["ssim"], ssim.mean(dim=0))
        ev.reset()
        assert ev.all_frame_psnr == [] and ev.all_frame_ssim == [] and ev.all_video_embeds_gt == []
    assert float(psnr[:, 4:].mean()) != float(psnr.mean())      # the scalar does depend on the first frame
    # a frame equal to its target: inf in the scalar that contains it, and at its place in the curve
    ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True, paired_from_frame=2)
    monkeypatch.setattr(E, "paired_frame_metrics", lambda p, t: {**_stub(p, t), "psnr": torch.where(
        torch.arange(6)[None] == 3, torch.tensor(float("inf"), dtype=torch.float64), _stub(p, t)["psnr"])})
    ev.push_vals(*[(b, 0, o) for b, o in batches][0])
    assert ev.evaluate_metrics()["psnr"] == float("inf") and np.isfinite(ev.evaluate_metrics()["ssim"])
    assert torch.isinf(ev.frame_curves()["psnr"]).tolist() == [False, False, False, True, False, False]
    # no frame left, or a frame number that is none
    ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True, paired_from_frame=6)
    ev.push_vals(batches[0][0], 0, batches[0][1])
    with pytest.raises(ValueError, match="paired_from_frame"):
        ev.evaluate_metrics()
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="paired_from_frame"):
            E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), paired_metrics=True, paired_from_frame=bad)
    assert "inf" in E.__doc__ and "paired_from_frame" in E.__doc__


def test_config_reaches_the_constructor(monkeypatch):
    import src  # noqa: F401
    from gsdd_amd.hydra_lite import compose, instantiate
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    stand_in = ["model.evaluator.videoencoder._target_=src.utils.evaluator.MeanPoolEncoder"]
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", stand_in)
    assert cfg.model.evaluator.paired_metrics is False and cfg.model.evaluator.paired_from_frame == 0
    ev = instantiate(cfg.model.evaluator, device="cpu", _recursive_=False)
    assert ev.paired_metrics is False and ev.paired_from_frame == 0 and ev.clip_scorer is None
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", stand_in + ["model.evaluator.paired_metrics=true",
                                                                            "model.evaluator.paired_from_frame=4",
                                                                            "model.generator.sample_condition_frames=4"])
    ev = instantiate(cfg.model.evaluator, device="cpu", _recursive_=False)
    assert ev.paired_metrics is True and ev.paired_from_frame == 4 and cfg.model.generator.sample_condition_frames == 4
    text = open(os.path.join(REPO, "configs", "model", "evaluator.yaml")).read()
    assert "paired_metrics: false" in text and "paired_from_frame: 0" in text


# ---------------------------------------------------------------------------------------------- the documents
def test_documents_name_the_entry():
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    assert "int gsdd_paired_metrics(" in header and "int64_t gsdd_paired_metrics_tiles(" in header
    for word in ("SSIM", "C1 = (0.01 * 255)^2", "C2 = (0.03 * 255)^2", "H - 11", "form 0", "form 1", "want_ssim"):
        assert word in header, word
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "gsdd_paired_metrics" in integration and "paired_frame_metrics" in integration
    assert "paired_metrics=true" in open(os.path.join(REPO, "README.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "gsdd_paired_metrics" in design and "MS-SSIM" in design and "LPIPS" in design
