"""LPIPS on the GPU (csrc/lpips.hip, gsdd_amd.ops.lpips_stem_rows / lpips_layer_distance, gsdd_amd.lpips.Lpips, the evaluator) against
the fp64 restatement (tests/lpips_ref.py) on seeded weights.  The stem operand is a table look-up: equality, bit for bit.  The distance
head alone is held to 4 x the worst relative error of the same expression in torch's fp32 on the CPU.  A frame's LPIPS through the whole
net is held to 4 rho sqrt(want), rho the worst |fp32 restatement - fp64| / sqrt(fp64) over the same case list (tests/test_lpips_host.py
shows what that bound keeps out).  Sizes: 31 and 16 are the nets' smallest frames (1 x 1 maps at the end), 31 x 45, 47 x 35 and 17 x 23
leave ragged pools, 64 x 64 and one 128 x 128 pair reach several workgroups a frame in the distance head.  Measured on one MI355X
(profiles/rW_lpips_parity_report.json), the towers' contractions in gsdd_gemm's default bf16-split mode: the distance head's worst
relative error 3.8e-7 at (n, C, P) = (3, 4, 1), 0.64 of the bound; alex's worst frame at 0.25 of its bound (rho 1.8e-7, 105 frames),
vgg's at 0.40 (rho 1.3e-7, 40 frames)."""
import numpy as np
import pytest
import torch

import gif_ref
import lpips_ref as ref
import paired_ref
import stale_memory
from conftest import parity_report

pytestmark = pytest.mark.gpu
NETS = ("alex", "vgg")


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


@pytest.fixture(scope="module")
def scorers(G):
    from gsdd_amd.lpips import Lpips
    return {net: Lpips(net, *ref.seeded_weights(net)).cuda() for net in NETS}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _operand(lv, form):
    return _dev(gif_ref.clips_from_levels(lv)) if form == "float" else _dev(lv)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---------------------------------------------------------------------------------------------- the stem operand
def _stem_want(lv, padw):
    """levels (B, T, H, W, 3) -> float32 (B T, H, W + 2 padw, 4) by the table rule"""
    B, T, H, W, _ = lv.shape
    t = ref.table()
    out = np.zeros((B * T, H, W + 2 * padw, 4), dtype=np.float32)
    flat = lv.reshape(B * T, H, W, 3)
    for c in range(3):
        out[:, :, padw:padw + W, c] = t[c][flat[..., c]]
    return out


@pytest.mark.parametrize("hw", [(1, 1), (5, 3), (31, 31), (31, 45), (64, 64)])
def test_stem_rows_is_the_table_rule_bit_for_bit(G, hw):
    from gsdd_amd.lpips import stem_table
    table = stem_table().cuda()
    assert np.array_equal(table.cpu().numpy(), ref.table())
    rng = np.random.default_rng(hw)
    lv = rng.integers(0, 256, (2, 3) + hw + (3,)).astype(np.uint8)
    x = paired_ref.float_operand(lv, inject=True, seed=3)                          # NaN, infinities, values beyond both ends
    lx = paired_ref.levels(x)
    assert np.isnan(x).any() and np.isinf(x).any()
    for padw in (2, 1, 0):                                                         # alex's, vgg's, none
        for operand, levels in ((_dev(lv), lv), (_dev(gif_ref.clips_from_levels(lv)), lv), (_dev(x), lx)):
            want = _stem_want(levels, padw)
            got = G.ops.lpips_stem_rows(operand, table, padw)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (hw, padw)
            if padw:
                pads = torch.cat([got[:, :, :padw], got[:, :, -padw:]], dim=2)
                assert bool((pads.view(torch.int32) == 0).all())                   # +0.0, every bit
            # a chunk of the frames into a caller's buffer that held something else: the same floats, every one written
            for byte in (0xFF, 0x7F):
                out = torch.full((3,) + want.shape[1:], byte * 0x01010101 - (1 << 32 if byte >= 0x80 else 0), dtype=torch.int32,
                                 device="cuda").view(torch.float32)
                back = G.ops.lpips_stem_rows(operand, table, padw, frame0=2, n=3, out=out)
                assert back is out and np.array_equal(out.cpu().numpy().view(np.int32), want[2:5].view(np.int32)), (hw, padw, byte)


# ---------------------------------------------------------------------------------------------- the distance head alone
def _head_case(n, C, P, seed):
    """features as a tower leaves them (ReLU outputs, a third of the elements 0), some positions all zero in one or both operands"""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn((2 * n, P, C), generator=g) + 0.4)
    f[0, 0] = 0.0                                                                  # position 0 of frame 0: zero in pred alone ...
    if P > 2:
        f[n, 1] = 0.0                                                              # ... position 1 in target alone ...
        f[0, 2] = 0.0
        f[n, 2] = 0.0                                                              # ... position 2 in both
    w = torch.rand((C,), generator=g)
    return f, w


def _head_ref(f, w, n, dtype):
    x = f.to(dtype).permute(0, 2, 1)[..., None]                                    # (2 n, C, P, 1)
    return ref.layer_distance(x[:n], x[n:], w.to(dtype))


def test_layer_distance_alone_within_four_times_torch_fp32(G):
    """bound: 4 x the worst relative error, over this grid, of the same expression evaluated by torch in fp32 on the CPU"""
    rows = []
    for n in (1, 3):
        for C in (4, 64, 192, 256, 384, 512):
            for P in (1, 9, 49, 63, 961, 1025):
                f, w = _head_case(n, C, P, seed=1000 * n + C + P)
                want = _head_ref(f, w, n, torch.float64)
                e32 = float(((_head_ref(f, w, n, torch.float32).double() - want).abs() / want).max())
                got = G.ops.lpips_layer_distance(f.reshape(2 * n * P, C).cuda(), w.cuda(), n)
                assert got.dtype == torch.float64 and tuple(got.shape) == (n,) and bool(torch.isfinite(got).all())
                rows.append(((n, C, P), e32, float(((got.cpu() - want).abs() / want).max())))
                # equal halves: exactly 0; all-zero feature vectors everywhere: exactly 0, not NaN
                same = torch.cat([f[:n], f[:n]]).reshape(2 * n * P, C).cuda()
                assert bool((G.ops.lpips_layer_distance(same, w.cuda(), n) == 0.0).all()), (n, C, P)
                assert bool((G.ops.lpips_layer_distance(torch.zeros_like(same), w.cuda(), n) == 0.0).all()), (n, C, P)
    e32 = max(r[1] for r in rows)
    worst = max(rows, key=lambda r: r[2])
    print(f"distance head: torch fp32 worst relative error {e32:.3e}, kernel worst {worst[2]:.3e} at (n, C, P) = {worst[0]}")
    parity_report("lpips_layer_distance", {"torch_fp32_worst_rel_err": e32, "kernel_worst_rel_err": worst[2], "kernel_worst_case": worst[0],
                                           "bound_rel": 4.0 * e32, "err_over_bound": worst[2] / (4.0 * e32), "cases": len(rows)})
    assert 0.0 < e32 < 1e-5
    for case, _, err in rows:
        assert err <= 4.0 * e32, (case, err)


def test_zero_vectors_contribute_nothing(G):
    """a position that is all zero in BOTH operands adds 0 to the sum: the result times P does not change when such positions are added"""
    n, C, P = 2, 64, 130
    f, w = _head_case(n, C, P, seed=5)
    got = G.ops.lpips_layer_distance(f.reshape(-1, C).cuda(), w.cuda(), n)
    padded = torch.cat([f, torch.zeros((2 * n, 70, C))], dim=1)
    more = G.ops.lpips_layer_distance(padded.reshape(-1, C).cuda(), w.cuda(), n)
    assert float(((more * 200.0 - got * 130.0).abs() / (got * 130.0)).max()) <= 1e-14          # (slots regroup the fp64 sum, no more)


# ---------------------------------------------------------------------------------------------- the whole net
@pytest.mark.parametrize("net", NETS)
def test_case_list_within_the_yardstick(G, scorers, net):
    rho, want, _ = ref.yardstick(net)
    worst, worst_case, frames = 0.0, None, 0
    layer_worst = 0.0
    for name, a, b, (fa, fb) in ref.cases(net):
        got = scorers[net](_operand(a, fa), _operand(b, fb))
        assert got["lpips"].dtype == torch.float64 and tuple(got["lpips"].shape) == a.shape[:2] and not got["lpips"].is_cuda
        assert tuple(got["layers"].shape) == a.shape[:2] + (5,) and torch.equal(got["lpips"], got["layers"].sum(dim=-1))
        v = want[name].sum(dim=-1)
        ratio = (got["lpips"] - v).abs() / (4.0 * rho * v.sqrt())
        frames += ratio.numel()
        layer_worst = max(layer_worst, float(((got["layers"] - want[name]).abs() / (4.0 * rho * want[name].sqrt())).max()))
        if float(ratio.max()) > worst:
            worst, worst_case = float(ratio.max()), f"{name}_{fa}_{fb}"
    print(f"{net}: rho = {rho:.3e}; worst |kernel - fp64| / (4 rho sqrt(want)) = {worst:.3f} ({worst_case}) over {frames} frames; "
          f"per layer {layer_worst:.3f}")
    parity_report(f"lpips_{net}", {"rho": rho, "worst_err_over_bound": worst, "worst_case": worst_case, "frames": frames,
                                   "worst_layer_err_over_its_bound": layer_worst, "gemm_mode": "bf16x3 (default)"})
    assert worst <= 1.0, (worst, worst_case)


@pytest.mark.parametrize("net", NETS)
def test_dead_positions_stay_finite(G, net):
    from gsdd_amd.lpips import Lpips
    rho = ref.yardstick(net)[0]
    name, a, b, _ = ref.cases(net)[1]
    compared = [i for i, lay in enumerate(x for x in ref.LAYERS[net] if x[0] == "conv") if lay[6]]
    for dead in (compared[0], compared[-1]):
        w = ref.seeded_weights(net, dead_layer=dead)
        got = Lpips(net, *w).cuda()(_dev(a), _operand(b, "float"))
        want = ref.lpips(net, a, b, w)
        assert bool(torch.isfinite(got["layers"]).all())
        assert bool((got["layers"][..., 0 if dead == compared[0] else 4] == 0.0).all())
        v = want.sum(dim=-1)
        assert bool(((got["lpips"] - v).abs() <= 4.0 * rho * v.sqrt()).all()), (net, dead)


# ---------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("net", NETS)
def test_equal_frames_score_exactly_zero_and_the_bits_do_not_depend_on_the_batch(G, scorers, net):
    s = scorers[net]
    by_name = {c[0]: c for c in ref.cases(net)}
    side = "47x35" if net == "alex" else "17x23"
    _, a, b, _ = by_name[f"noise10_{side}"]
    f0, f1 = _operand(a, "float"), _operand(a, "uint8")
    for xa, xb in ((f0, f0), (f1, f1.clone()), (f0, f1)):
        got = s(xa, xb)
        assert bool((got["lpips"] == 0.0).all()) and bool((got["layers"] == 0.0).all())
    xa, xb = _operand(a, "float"), _operand(b, "uint8")
    whole = s(xa, xb)
    again = s(xa, xb)
    assert stale_memory.same_bits(whole["layers"], again["layers"]) and bool((whole["lpips"] > 0).all())
    # every chunking, down to one frame pair a pass
    for chunk in (1, 2, 3, 1000):
        assert stale_memory.same_bits(s(xa, xb, chunk=chunk)["layers"], whole["layers"]), chunk
    # a clip alone, and a frame alone
    for i in range(a.shape[0]):
        one = s(xa[i:i + 1].contiguous(), xb[i:i + 1].contiguous())
        assert stale_memory.same_bits(one["layers"], whole["layers"][i:i + 1]), i
    one = s(xa[-1:, :, -1:].contiguous(), xb[-1:, -1:].contiguous())
    assert stale_memory.same_bits(one["layers"], whole["layers"][-1:, -1:])
    # a small budget chunks by itself
    from gsdd_amd.lpips import Lpips
    tight = Lpips(net, *ref.seeded_weights(net), budget_bytes=1).cuda()
    assert tight.chunk_frames(*a.shape[2:4]) == 1 and s.chunk_frames(*a.shape[2:4]) > a.shape[0] * a.shape[1]
    assert stale_memory.same_bits(tight(xa, xb)["layers"], whole["layers"])


def test_results_do_not_depend_on_what_the_partials_held(G):
    n, C, P = 3, 192, 300
    f, w = _head_case(n, C, P, seed=9)
    feat, w = f.reshape(-1, C).cuda(), w.cuda()
    slots = G.ops.lpips_distance_slots(P, C)
    assert slots == 10
    results = []
    for byte in stale_memory.BYTES:
        partials = torch.full((n, slots * 2), byte * 0x01010101 - (1 << 32 if byte >= 0x80 else 0), dtype=torch.int32,
                              device="cuda").view(torch.float64)
        assert tuple(partials.shape) == (n, slots) and bool(partials.view(torch.uint8).eq(byte).all())
        d = G.ops.lpips_layer_distance(feat, w, n, partials=partials)
        results.append(stale_memory.host_bits({"d": d, "partials": partials}))
    fresh = G.ops.lpips_layer_distance(feat, w, n)
    assert stale_memory.same_bits(fresh, d)
    for byte, r in zip(stale_memory.BYTES[1:], results[1:]):
        assert stale_memory.differing(results[0], r) == [], hex(byte)


# ---------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_raise_before_anything_is_written(G, scorers):
    E = G.GsddError
    from gsdd_amd.lpips import stem_table
    table = stem_table().cuda()
    ok = torch.zeros((1, 3, 2, 31, 31), device="cuda")
    ok8 = torch.zeros((1, 2, 31, 31, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((2, 31, 35, 4), 3.5, device="cuda")
    calls = [lambda: G.ops.lpips_stem_rows(ok.double(), table, 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok.cpu(), table, 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok.transpose(3, 4), table, 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok, table.cpu(), 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok, table[:, :255], 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok, table.double(), 2, out=out),
             lambda: G.ops.lpips_stem_rows(ok, table, 1, out=out),                                  # out is sized for padw = 2
             lambda: G.ops.lpips_stem_rows(ok, table, 2, frame0=1, n=2, out=out),                   # frames 1 .. 2 of 2
             lambda: G.ops.lpips_stem_rows(ok, table, 2, frame0=-1, n=2, out=out),
             lambda: G.ops.lpips_stem_rows(ok8, table, 2, frame0=0, n=3, out=torch.full((3, 31, 35, 4), 3.5, device="cuda")),
             lambda: G.ops.lpips_stem_rows(ok, table, 65, out=torch.full((2, 31, 161, 4), 3.5, device="cuda")),
             lambda: G.ops.lpips_stem_rows(ok, table, 2, out=out.cpu()),
             lambda: G.ops.lpips_stem_rows(ok, table, 2, out=out[:, :, :, :3])]
    for i, call in enumerate(calls):
        with pytest.raises(E):
            call()
        assert bool(out.eq(3.5).all()), i
    feat, w = torch.ones((2 * 2 * 49, 64), device="cuda"), torch.ones((64,), device="cuda")
    partials = torch.full((2, 1), 3.5, dtype=torch.float64, device="cuda")
    calls = [lambda: G.ops.lpips_layer_distance(feat, w, 3, partials=partials),                    # 196 rows are not 2 x 3 frames
             lambda: G.ops.lpips_layer_distance(feat, w, 0, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat[:, :62].contiguous(), w[:62].contiguous(), 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(torch.ones((196, 516), device="cuda"), torch.ones((516,), device="cuda"), 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat, w[:60].contiguous(), 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat.double(), w, 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat.cpu(), w, 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat, w.cpu(), 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat.t(), w, 2, partials=partials),
             lambda: G.ops.lpips_layer_distance(feat, w, 2, partials=partials.float()),
             lambda: G.ops.lpips_layer_distance(feat, w, 2, partials=partials.cpu()),
             lambda: G.ops.lpips_layer_distance(feat, w, 2, partials=torch.full((2, 2), 3.5, dtype=torch.float64, device="cuda"))]
    for i, call in enumerate(calls):
        with pytest.raises(E):
            call()
        assert bool(partials.eq(3.5).all()), i
    # the scorer: frames below the net's smallest side, mismatched operands, tensors that are not on the device
    for net, small in (("alex", 30), ("vgg", 15)):
        s = scorers[net]
        x = torch.zeros((1, 3, 2, small, 40), device="cuda")
        with pytest.raises(E, match="smallest side"):
            s(x, x)
        with pytest.raises(E, match="smallest side"):
            G.metrics.paired_frame_metrics(x, x, lpips=s)
        assert set(G.metrics.paired_frame_metrics(x, x)) == {"psnr", "ssim", "sse"}                # legal without a scorer
        big = torch.zeros((1, 3, 2, 40, 40), device="cuda")
        for bad in (torch.zeros((1, 3, 2, 40, 41), device="cuda"), torch.zeros((1, 3, 40, 40, 3), dtype=torch.uint8, device="cuda"),
                    torch.zeros((2, 3, 2, 40, 40), device="cuda"), big.cpu(), big.double()):
            with pytest.raises(E):
                s(big, bad)
        with pytest.raises(E):
            s(big, big, chunk=0)


# ---------------------------------------------------------------------------------------------- the evaluator
def test_evaluator_returns_the_means_of_the_direct_calls(G, scorers, monkeypatch):
    import src  # noqa: F401
    from src.utils.evaluator import Evaluator, MeanPoolEncoder
    rng = np.random.default_rng(11)
    batches = []
    for i in range(2):
        target = rng.integers(0, 256, (3, 4, 32, 32, 3))
        pred = np.clip(np.rint(target + rng.normal(0, 6.0 * (i + 1), target.shape)), 0, 255)
        pred[:, :2] = target[:, :2]                             # two given frames, as a prediction run has them
        batches.append(({"video": torch.from_numpy(gif_ref.clips_from_levels(target.astype(np.uint8))), "text": ["x"] * 3},
                        _dev(gif_ref.clips_from_levels(pred.astype(np.uint8)))))
    launches = {"stem": 0, "distance": 0}
    real_stem, real_distance = G.ops.lpips_stem_rows, G.ops.lpips_layer_distance
    monkeypatch.setattr(G.ops, "lpips_stem_rows", lambda *a, **k: launches.__setitem__("stem", launches["stem"] + 1) or real_stem(*a, **k))
    monkeypatch.setattr(G.ops, "lpips_layer_distance",
                        lambda *a, **k: launches.__setitem__("distance", launches["distance"] + 1) or real_distance(*a, **k))
    s = scorers["alex"]
    plain = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32, paired_metrics=True)
    for i, (batch, out) in enumerate(batches):
        plain.push_vals(batch, i, out)
    old = plain.evaluate_metrics()
    assert set(old) == {"fvd", "psnr", "ssim"} and launches == {"stem": 0, "distance": 0} and plain.all_frame_lpips == []
    ev = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32, lpips_scorer=s, paired_from_frame=2)
    both = Evaluator("cuda", MeanPoolEncoder(grid=2), target_resolution=32, lpips_scorer=s, paired_metrics=True)
    for i, (batch, out) in enumerate(batches):
        ev.push_vals(batch, i, out)
        both.push_vals(batch, i, out)
    assert launches == {"stem": 2 * 4, "distance": 5 * 4}
    got = ev.evaluate_metrics()
    assert set(got) == {"fvd", "lpips"} and got["fvd"] == old["fvd"]
    direct = torch.cat([s(out, batch["video"].cuda())["lpips"] for batch, out in batches])                 # (6, 4)
    assert got["lpips"] == float(direct[:, 2:].mean()) and got["lpips"] > 0
    assert torch.equal(ev.frame_curves()["lpips"], direct.mean(dim=0)) and ev.frame_curves()["lpips"][:2].tolist() == [0.0, 0.0]
    more = both.evaluate_metrics()
    assert set(more) == {"fvd", "psnr", "ssim", "lpips"} and more["lpips"] == float(direct.mean())
    assert more["ssim"] == old["ssim"] and more["psnr"] == old["psnr"]
    want = torch.cat([ref.lpips("alex", gif_ref.levels_of(out.cpu().numpy()), gif_ref.levels_of(batch["video"].numpy()),
                                ref.seeded_weights("alex")).sum(dim=-1) for batch, out in batches])
    rho = ref.yardstick("alex")[0]
    assert bool(((direct - want).abs() <= 4.0 * rho * want.sqrt()).all())
    through = G.metrics.paired_frame_metrics(batches[0][1], batches[0][0]["video"].cuda(), lpips=s)
    assert set(through) == {"psnr", "ssim", "sse", "lpips"} and torch.equal(through["lpips"], direct[:3])
