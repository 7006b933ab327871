"""LPIPS, the part that needs no GPU: the restatement of the rule (tests/lpips_ref.py) against an independent formulation, the input
table against its expression, the weight loaders on state dicts in the published layouts, the yardstick the GPU test judges the
kernels by and the faults that keep it honest, the entries' argument checks (they return before anything is launched), the
evaluator's plumbing on a stub scorer, the config, and the documents."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lpips_ref as ref
import paired_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("alex", "vgg")


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("net", NETS)
def test_restatement_agrees_with_an_im2col_formulation(net):
    rho, want, _ = ref.yardstick(net)
    weights = ref.seeded_weights(net)
    worst = 0.0
    for name, a, b, _ in ref.cases(net):
        assert want[name].dtype == torch.float64 and tuple(want[name].shape) == a.shape[:2] + (5,)
        assert bool((want[name] >= 0).all())
        worst = max(worst, float((ref.lpips_im2col(net, a, b, weights) - want[name]).abs().max()))
    print(f"{net}: restatement against im2col, worst layer distance: {worst:.3e}")
    assert worst <= 1e-12


def test_stem_table_is_its_expression():
    from gsdd_amd import lpips
    t = lpips.stem_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256) and np.array_equal(t.numpy(), ref.table())
    assert lpips.SHIFT == ref.SHIFT == (-0.030, -0.088, -0.188) and lpips.SCALE == ref.SCALE == (0.458, 0.448, 0.450)
    for c in range(3):
        for level in (0, 1, 127, 128, 254, 255):
            want = np.float32((level / 127.5 - 1.0 - ref.SHIFT[c]) / ref.SCALE[c])            # python floats: fp64, rounded once
            assert t[c, level].item() == want
    assert float(t.min()) < -2.0 and not bool((t == 0).any())                                  # no level maps to the padding's 0
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    assert "(level / 127.5 - 1.0 - shift[c]) / scale[c]" in header and "(-0.030, -0.088, -0.188)" in header
    assert "(0.458, 0.448, 0.450)" in header and "1e-10" in header


@pytest.mark.parametrize("net", NETS)
def test_layer_table_is_the_published_one(net):
    from gsdd_amd import lpips
    assert lpips.conv_keys(net) == list(zip(ref.FEATURE_INDEX[net], ref.SLICE[net]))
    assert lpips.tap_channels(net) == ref.TAP_CHANNELS[net]
    flat = tuple((lay["op"], lay["cin"], lay["cout"], lay["k"], lay["stride"], lay["pad"], lay["tap"]) if lay["op"] == "conv" else
                 (lay["op"], lay["k"], lay["stride"]) for lay in lpips.NETS[net]["layers"])
    assert flat == ref.LAYERS[net] and lpips.NETS[net]["backbone"] == ref.BACKBONE[net]
    m = ref.MIN_SIDE[net]
    assert lpips.NETS[net]["min_side"] == m and lpips.feature_sizes(net, m, m)[-1] == (1, 1)
    for H, W in ((m - 1, m), (m, m - 1), (1, 1)):
        with pytest.raises(lpips.GsddError, match="smallest side"):
            lpips.feature_sizes(net, H, W)
    # the sizes are torch's
    x = torch.zeros((1, 3, 47, 35), dtype=torch.float64)
    maps = ref.taps(net, x, ref.seeded_weights(net)[0])
    sizes = [s for s, lay in zip(lpips.feature_sizes(net, 47, 35), lpips.NETS[net]["layers"]) if lay["op"] == "conv" and lay["tap"]]
    assert sizes == [tuple(t.shape[2:]) for t in maps]


# ---------------------------------------------------------------------------------------------- the loaders
@pytest.mark.parametrize("net", NETS)
def test_loaders_take_the_published_layouts(net, tmp_path):
    from gsdd_amd.lpips import GsddError, Lpips
    convs, lins = ref.seeded_weights(net)
    direct = Lpips(net, convs, lins)
    full = ref.lpips_state_dict(net, convs, lins)
    assert any(k.startswith("lins.") for k in full) and "scaling_layer.shift" in full           # the keys a loader has to ignore
    backbone, lin = ref.backbone_state_dict(net, convs), ref.lin_state_dict(lins)
    torch.save(full, tmp_path / "full.pth")
    os.makedirs(tmp_path / "parts")
    torch.save(backbone, tmp_path / "parts" / (ref.BACKBONE[net] + ".pth"))
    torch.save(lin, tmp_path / "parts" / (net + ".pth"))
    loaded = [Lpips.from_lpips_state_dict(full), Lpips.from_lpips_state_dict(full, net), Lpips.from_state_dicts(backbone, lin, net),
              Lpips.from_pretrained(str(tmp_path / "full.pth"), net), Lpips.from_pretrained(str(tmp_path / "parts"), net)]
    for got in loaded:
        assert got.net == net and len(got.w) == len(convs) and len(got.lin) == 5
        assert all(torch.equal(x, y) for x, y in zip(got.w + got.b + got.lin, direct.w + direct.b + direct.lin))
    # the packing: the first convolution with kw in the contraction over 4-float pixels, the others [taps][Cout][Cin]
    k = convs[0][0].shape[2]
    assert tuple(direct.w[0].shape) == (k, 64, 4 * k) and torch.equal(direct.w[0][2, :, 4 * 1 + 2], convs[0][0][:, 2, 2, 1])
    assert bool((direct.w[0].view(k, 64, k, 4)[..., 3] == 0).all())
    assert tuple(direct.w[1].shape) == (convs[1][0].shape[2] ** 2,) + tuple(convs[1][0].shape[:2])
    assert all(v.dim() == 1 and bool((v >= 0).all()) for v in direct.lin)
    # a missing key and a wrong shape are named
    i, s = ref.FEATURE_INDEX[net][1], ref.SLICE[net][1]
    for sd, key, load in ((full, f"net.slice{s}.{i}.bias", Lpips.from_lpips_state_dict), (full, "lin3.model.1.weight", Lpips.from_lpips_state_dict),
                          (backbone, f"features.{i}.weight", lambda d: Lpips.from_state_dicts(d, lin, net)),
                          (lin, "lin0.model.1.weight", lambda d: Lpips.from_state_dicts(backbone, d, net))):
        with pytest.raises(GsddError, match=key.replace(".", r"\.")):
            load({k: v for k, v in sd.items() if k != key})
    bad = dict(full)
    bad[f"net.slice{s}.{i}.weight"] = full[f"net.slice{s}.{i}.weight"][:, :-1]
    with pytest.raises(GsddError, match="convolution 1 must be"):
        Lpips.from_lpips_state_dict(bad)
    bad = dict(full)
    bad["lin2.model.1.weight"] = full["lin2.model.1.weight"][:, :-4]
    with pytest.raises(GsddError, match="lin2 must be"):
        Lpips.from_lpips_state_dict(bad)
    with pytest.raises(GsddError, match="not one of"):
        Lpips("squeeze", convs, lins)
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        Lpips.from_pretrained(str(tmp_path / "absent.pth"), net)
    # no CPU fallback
    x = torch.zeros((1, 3, 1, 32, 32))
    with pytest.raises(GsddError, match="no CPU fallback"):
        direct(x, x)


# ---------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("net", NETS)
def test_yardstick_and_the_faults_that_keep_it_honest(net):
    """The GPU bound on a frame's LPIPS is 4 rho sqrt(want), rho the worst |fp32 restatement - fp64| / sqrt(fp64) over the case list
    (measured here on the seeded weights: 1.8e-7 for alex, 1.3e-7 for vgg).  It is only worth something if it tells the rule from the
    rule with a fault: each fault must move EVERY frame of the random and noise10 cases by at least 10 bounds.  Seen: padding in level
    space >= 2.0e3, no scaling layer >= 196, spatial sum >= 4e6, a skipped tap >= 1.3e4, BGR order >= 282, a tap before its ReLU
    >= 676 bounds.  Ceil-mode pools are the identity wherever every pooled side fits its windows exactly -- alex at 31, 32, 64 and 128,
    vgg at even sides -- and cannot be told there by anything; on the other sizes (31x45 and 47x35, 17x23) they move every frame by
    >= 9e3 bounds.  Moving eps inside the root changes results by 1e-12 and is not pinned; dropping it is, by the dead-position case."""
    rho, want, per_case = ref.yardstick(net)
    print(f"{net}: rho = {rho:.3e} (worst case {max(per_case, key=per_case.get)})")
    assert 0.0 < rho < 2e-6                                      # an fp32 evaluation: a few ulps of the features
    weights = ref.seeded_weights(net)
    shown = [c for c in ref.cases(net) if c[0].startswith(("random", "noise10"))]
    assert len(shown) == 2 * len(ref.SHAPES[net])
    for fault in ref.FAULTS:
        if fault == "no_eps":
            continue
        ratios = {}
        for name, a, b, _ in shown:
            v = want[name].sum(dim=-1)
            moved = (ref.lpips(net, a, b, weights, fault=fault).sum(dim=-1) - v).abs()
            ratios[name] = float((moved / (4.0 * rho * v.sqrt())).min())
        print(f"{net}: fault {fault}: least move {min(ratios.values()):.3g} bounds ({min(ratios, key=ratios.get)})")
        if fault == "ceil_mode_pools":
            for name, a, _, _ in shown:
                x = torch.zeros((1, 3) + a.shape[2:4], dtype=torch.float64)
                same = [t.shape for t in ref.taps(net, x, weights[0])] == [t.shape for t in ref.taps(net, x, weights[0], ceil_pools=True)]
                assert (ratios[name] == 0.0) if same else (ratios[name] >= 10.0), (name, ratios[name])
            assert any(r >= 10.0 for r in ratios.values())
        else:
            assert min(ratios.values()) >= 10.0, (fault, ratios)
    # a layer whose every position is dead (all-zero feature vectors in both operands): 0 from that layer by the rule, NaN without eps
    name, a, b, _ = shown[0]
    compared = [i for i, lay in enumerate(x for x in ref.LAYERS[net] if x[0] == "conv") if lay[6]]
    for tap, dead in ((0, compared[0]), (4, compared[-1])):
        w = ref.seeded_weights(net, dead_layer=dead)
        d = ref.lpips(net, a, b, w)
        assert bool(torch.isfinite(d).all()) and bool((d[..., tap] == 0).all())
        assert bool(torch.isnan(ref.lpips(net, a, b, w, fault="no_eps")[..., tap]).all())


# ---------------------------------------------------------------------------------------------- the entries' argument checks
def test_entries_reject_bad_arguments_before_any_launch():
    import gsdd_amd
    L = gsdd_amd.lib()
    assert L.gsdd_version() >= 116
    for name in ("gsdd_lpips_stem_rows", "gsdd_lpips_distance_slots", "gsdd_lpips_layer_distance"):
        assert name in gsdd_amd.EXPORTS and hasattr(L, name)
    # 32 * 64 / G positions a workgroup, G the power of two at or above C / 4, 64 at the most
    assert [L.gsdd_lpips_distance_slots(p, c) for p, c in ((1, 4), (2048, 4), (2049, 4), (128, 64), (129, 64), (961, 64), (32, 512),
                                                           (33, 512), (32, 192), (33, 384), (64, 128), (65, 128))] == \
        [1, 1, 2, 1, 2, 8, 1, 2, 1, 2, 1, 2]
    for p, c in ((0, 64), (5, 0), (5, 6), (5, 516), (-1, 4)):
        assert L.gsdd_lpips_distance_slots(p, c) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                   # never read: every call below returns from its checks
    assert p % 16 == 0
    ok = [p, 0, 2, 3, 31, 31, 0, 6, 2, p, p]                    # x, form, B, T, H, W, frame0, n, padw, table, out
    for j, bad in ((0, None), (9, None), (10, None), (1, 2), (1, -1), (2, 0), (3, 0), (4, 0), (5, -3), (6, -1), (6, 1), (7, 0), (7, 7),
                   (8, -1), (8, 65), (0, p + 2), (9, p + 1), (10, p + 4)):
        args = ok[:j] + [bad] + ok[j + 1:]
        assert L.gsdd_lpips_stem_rows(*args, None) == -1, (j, bad)
        assert b"gsdd_lpips_stem_rows" in L.gsdd_last_error()
    ok = [p, p, 3, 49, 64, p]                                   # feat, w, n, P, C, partials
    for j, bad in ((0, None), (1, None), (5, None), (2, 0), (3, 0), (4, 0), (4, 6), (4, 516), (4, -4), (0, p + 4), (1, p + 8), (5, p + 4),
                   (3, 1 << 31), (2, 1 << 30)):
        args = ok[:j] + [bad] + ok[j + 1:]
        assert L.gsdd_lpips_layer_distance(*args, None) == -1, (j, bad)
        assert b"gsdd_lpips_layer_distance" in L.gsdd_last_error()
    E = gsdd_amd.GsddError
    x = torch.zeros((1, 3, 2, 31, 31))
    with pytest.raises(E, match="ROCm device"):
        gsdd_amd.ops.lpips_stem_rows(x, torch.zeros((3, 256)), 2)
    with pytest.raises(E, match="ROCm device"):
        gsdd_amd.ops.lpips_layer_distance(torch.zeros((98, 64)), torch.zeros((64,)), 1)


# ---------------------------------------------------------------------------------------------- the evaluator
class _StubScorer:
    """stands in for gsdd_amd.lpips.Lpips on the host: per frame, a number that depends on the frame and the sample"""

    def __init__(self):
        self.calls = []

    def __call__(self, pred, target):
        self.calls.append((pred, target))
        d = (pred.double() - target.double()).abs().mean(dim=(1, 3, 4))                # (B, T)
        return {"lpips": d / (1.0 + d), "layers": d[..., None].expand(*d.shape, 5) / 5.0}


def _batches():
    g = torch.Generator().manual_seed(2)
    return [({"video": torch.randn((4, 3, 6, 16, 16), generator=g), "text": ["a"] * 4}, torch.randn((4, 3, 6, 16, 16), generator=g))
            for _ in range(3)]


def test_evaluator_scores_lpips_only_when_asked(monkeypatch):
    import src  # noqa: F401
    import src.utils.evaluator as E
    monkeypatch.setattr(E.Evaluator, "_prepare", lambda self, clips: clips.float())
    batches = _batches()
    plain = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32)
    assert plain.lpips_scorer is None
    for i, (batch, out) in enumerate(batches):
        plain.push_vals(batch, i, out)
    old = plain.evaluate_metrics()
    assert set(old) == {"fvd"} and plain.all_frame_lpips == []
    with pytest.raises(ValueError, match="paired_metrics"):
        plain.frame_curves()

    want = torch.cat([_StubScorer()(out, batch["video"])["lpips"] for batch, out in batches])               # (12, 6)
    for start in (0, 4, 5):
        stub = _StubScorer()
        ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, lpips_scorer=stub, paired_from_frame=start)
        for i, (batch, out) in enumerate(batches):
            ev.push_vals(batch, i, out)
        assert len(stub.calls) == 3 and all(p.dtype == torch.float32 and p.is_contiguous() and t.is_contiguous() for p, t in stub.calls)
        assert torch.equal(stub.calls[1][0], batches[1][1]) and torch.equal(stub.calls[1][1], batches[1][0]["video"])   # (pred, target)
        got = ev.evaluate_metrics()
        assert set(got) == {"fvd", "lpips"} and got["fvd"] == old["fvd"] and got["lpips"] == float(want[:, start:].mean())
        curves = ev.frame_curves()                              # all frames, whatever the scalar leaves out; no PSNR without paired_metrics
        assert set(curves) == {"lpips"} and curves["lpips"].dtype == torch.float64 and torch.equal(curves["lpips"], want.mean(dim=0))
        ev.reset()
        assert ev.all_frame_lpips == []
    assert float(want[:, 4:].mean()) != float(want.mean())
    # next to the paired metrics: three keys more, every one over the same frames
    monkeypatch.setattr(E, "paired_frame_metrics", lambda p, t: {"psnr": torch.full(p.shape[:1] + p.shape[2:3], 30.0, dtype=torch.float64),
                                                                 "ssim": torch.full(p.shape[:1] + p.shape[2:3], 0.5, dtype=torch.float64)})
    ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, lpips_scorer=_StubScorer(), paired_metrics=True,
                     paired_from_frame=2)
    for i, (batch, out) in enumerate(batches):
        ev.push_vals(batch, i, out)
    got = ev.evaluate_metrics()
    assert set(got) == {"fvd", "psnr", "ssim", "lpips"} and got["lpips"] == float(want[:, 2:].mean()) and got["psnr"] == 30.0
    assert set(ev.frame_curves()) == {"psnr", "ssim", "lpips"}
    # no frame left
    ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), target_resolution=32, lpips_scorer=_StubScorer(), paired_from_frame=6)
    ev.push_vals(batches[0][0], 0, batches[0][1])
    with pytest.raises(ValueError, match="paired_from_frame"):
        ev.evaluate_metrics()
    # a scorer named in a config is instantiated, like clip_scorer
    ev = E.Evaluator("cpu", E.MeanPoolEncoder(grid=2), lpips_scorer={"_target_": "test_lpips_host._StubScorer"})
    assert type(ev.lpips_scorer).__name__ == "_StubScorer"
    assert "LPIPS" in E.__doc__ and "lpips_scorer" in E.__doc__


def test_paired_frame_metrics_default_is_unchanged(monkeypatch):
    """without a scorer the dict holds today's three entries and nothing of LPIPS is touched; with one, "lpips" is the scorer's"""
    import gsdd_amd
    from gsdd_amd import metrics
    B, T = 2, 3
    monkeypatch.setattr(gsdd_amd.ops, "paired_metrics", lambda a, b, want_ssim=True: (torch.ones((B, T, 3), dtype=torch.int64),
                                                                                       torch.full((B, T, 3), 0.25, dtype=torch.float64)))
    x = torch.zeros((B, 3, T, 12, 12))
    got = metrics.paired_frame_metrics(x, x)
    assert set(got) == {"psnr", "ssim", "sse"}
    stub = _StubScorer()
    more = metrics.paired_frame_metrics(x, x + 1.0, lpips=stub)
    assert set(more) == {"psnr", "ssim", "sse", "lpips"} and len(stub.calls) == 1 and tuple(more["lpips"].shape) == (B, T)
    assert all(torch.equal(got[k], more[k]) for k in got)


def test_config_reaches_the_constructor(monkeypatch, tmp_path):
    import src  # noqa: F401
    from gsdd_amd.hydra_lite import compose, instantiate
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    stand_in = ["model.evaluator.videoencoder._target_=src.utils.evaluator.MeanPoolEncoder"]
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", stand_in)
    assert cfg.model.evaluator.lpips_scorer is None
    ev = instantiate(cfg.model.evaluator, device="cpu", _recursive_=False)
    assert ev.lpips_scorer is None and ev.paired_metrics is False and ev.clip_scorer is None
    # the commented example: lpips_from_pretrained as a _target_, on weights in the published layout
    convs, lins = ref.seeded_weights("alex")
    torch.save(ref.lpips_state_dict("alex", convs, lins), tmp_path / "alex_full.pth")
    cfg = compose(os.path.join(REPO, "configs"), "eval.yaml", stand_in + [
        "model.evaluator.lpips_scorer={_target_: src.utils.evaluator.lpips_from_pretrained, weights: " + str(tmp_path / "alex_full.pth") +
        ", net: alex, device: cpu}"])
    ev = instantiate(cfg.model.evaluator, device="cpu", _recursive_=False)
    assert type(ev.lpips_scorer).__name__ == "Lpips" and ev.lpips_scorer.net == "alex" and ev.lpips_scorer.device.type == "cpu"
    text = open(os.path.join(REPO, "configs", "model", "evaluator.yaml")).read()
    assert "lpips_scorer: null" in text and "src.utils.evaluator.lpips_from_pretrained" in text


# ---------------------------------------------------------------------------------------------- the documents
def test_documents_name_the_entries():
    header = open(os.path.join(REPO, "include", "gsdd.h")).read()
    for word in ("int gsdd_lpips_stem_rows(", "int gsdd_lpips_layer_distance(", "int64_t gsdd_lpips_distance_slots(", "Zhang et al. 2018",
                 "k11 s4 p2", "relu1_2", "ZERO IN THE SCALED SPACE", "eps OUTSIDE the root"):
        assert word in header, word
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for word in ("gsdd_lpips_stem_rows", "gsdd_lpips_layer_distance", "lpips_from_pretrained", "Lpips"):
        assert word in integration, word
    assert "lpips_scorer" in open(os.path.join(REPO, "README.md")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for word in ("gsdd_lpips_layer_distance", "gsdd_lpips_stem_rows", "ceil-mode", "MS-SSIM", "LPIPS", "rW_lpips.csv"):
        assert word in design, word
