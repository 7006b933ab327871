"""Long clips on the MI355X: the slide between two windows and the window blend against the restatement of tests/long_ref.py, the
rollout DiffusionTransformer.sample_long against the manual chain of public calls it is defined by (d3pm_L64 model), the stitched
decode and the generator / render glue (the models of tests.test_gpu_glue.build), and a sweep over what fresh memory holds.

The manual chain: window 0 is sample() -- sample_fast() with skip_step --, with the caller's mask if there is one; every later window
is the same call with content_token = the window before's last k frames in front, known_mask = frame_mask(latent_shape, k); the
long grid takes each frame from the first window that sampled it.  A window plan with resampling jumps runs the jumps in window 0 as
well (long_plan: every window is the same program), which the chain spells as an all-False mask.

The long buffer's rows have the fixed pitch n h w, so "nothing behind a row's end" shows as: every word of the lane's rows that the
window does not own, the rows' neighbours included, keeps its canary, as do the margins in front of the first and behind the last row."""
import numpy as np
import pytest
import torch

from tests import long_ref as ref
from tests import stale_memory as sm
from tests.test_gpu_parity import build_d3pm

pytestmark = pytest.mark.gpu

CANARY = -7
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gsdd_amd.lib()
    return gsdd_amd


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- the slide alone
def slide_cases():
    for Bs in (1, 3):
        for F, hw, k in ((4, 16, 1), (4, 16, 3), (3, 5, 2), (16, 256, 4)):
            s = F - k
            for rep in (1, 2):
                # window 1 contributes [F, F + s): all of it, a partial range (s >= 2), a single frame; window 0 all F; a later window
                for w, n in {(1, F + s + 1), (1, F + max(s - 1, 1)), (1, F + 1), (0, F + 1), (2, F + 2 * s)}:
                    yield Bs, F, hw, k, rep, w, n


@pytest.mark.parametrize("Bs,F,hw,k,rep,w,n", sorted(slide_cases()))
def test_window_slide_equals_the_restatement(G, Bs, F, hw, k, rep, w, n):
    K, t0, Lw, s = 32, 99, F * hw, F - k
    g = gen(Bs * 1000 + F * 100 + k * 10 + rep + w + n)
    margin, row = 3 * hw + 5, n * hw
    tok = torch.randint(0, K, (Bs, Lw), generator=g)
    x_known = torch.randint(0, K, (Bs, Lw), generator=g)
    known = torch.randint(0, 2, (Bs, Lw), generator=g).to(torch.uint8)
    t2 = torch.randint(-1, 99, (rep * Bs,), generator=g)
    for plant in ("none", "overlap", "outside", "final"):
        tk = tok.clone()
        if plant == "overlap":
            tk[Bs - 1, s * hw + (k * hw) // 2] = K                   # [MASK] at a position that becomes known
            tk[0, Lw - 1] = K
        elif plant == "outside":
            tk[Bs - 1, s * hw - 1] = K                                # the last position in front of the overlap
            tk[0, 0] = K
        flat = torch.full((margin + Bs * row + margin,), CANARY, dtype=torch.int64)
        d = {name: t.clone().cuda() for name, t in (("tok", tk), ("flat", flat), ("x_known", x_known), ("known", known), ("t2", t2))}
        rows = d["flat"][margin:margin + Bs * row].view(Bs, row)
        state = torch.tensor([w, 0], dtype=torch.int64, device="cuda")
        bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
        final = plant == "final"
        G.ops.d3pm_window_slide(d["tok"], rows, d["x_known"], d["known"], d["t2"], state, bad, F=F, k=k, n=n, K=K, t0=t0, final=final)
        want = ref.slide(tk.numpy(), flat[margin:margin + Bs * row].view(Bs, row).numpy(), x_known.numpy(), known.numpy(), t2.numpy(), w,
                         F=F, k=k, n=n, K=K, t0=t0, final=final)
        got_flat = d["flat"].cpu()
        assert bool((got_flat[:margin] == CANARY).all()) and bool((got_flat[margin + Bs * row:] == CANARY).all()), plant
        for name, got, exp in (("tok", d["tok"], want[0]), ("long", rows, want[1]), ("x_known", d["x_known"], want[2]),
                               ("known", d["known"], want[3]), ("t2", d["t2"], want[4])):
            assert np.array_equal(got.cpu().numpy(), exp), (plant, name)
        assert state.tolist() == [want[5], 0] and int(bad.item()) == want[6], plant
        assert (int(bad.item()) > 0) == (plant == "overlap")
        written = int((rows.cpu() != CANARY).sum())
        assert written == Bs * hw * len([f for f in range(0 if w == 0 else k, F) if w * s + f < n]) > 0


def test_window_slide_ignores_an_index_outside_the_clip(G):
    """A window index the rollout never produces writes nothing to the long buffer (the bound that keeps a stale state harmless)."""
    F, hw, k, n, K = 4, 16, 2, 8, 32
    for w in (-1, 9, 1 << 62, -(1 << 62)):
        tok = torch.randint(0, K, (2, F * hw), generator=gen(3)).cuda()
        flat = torch.full((64 + 2 * n * hw + 64,), CANARY, dtype=torch.int64, device="cuda")
        state = torch.tensor([w, 0], dtype=torch.int64, device="cuda")
        G.ops.d3pm_window_slide(tok, flat[64:64 + 2 * n * hw].view(2, n * hw), torch.zeros_like(tok), torch.zeros_like(tok, dtype=torch.uint8),
                                torch.zeros(2, dtype=torch.int64, device="cuda"), state, torch.zeros(1, dtype=torch.int32, device="cuda"),
                                F=F, k=k, n=n, K=K, t0=99)
        assert bool((flat == CANARY).all()) and bool((tok == K).all()) and state.tolist() == [w + 1, 0]


# ----------------------------------------------------------------------------- the blend alone
@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 7), (1, 3, 16, 16, 16)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("mode", ["linear", "keep", "replace"])
def test_window_blend_equals_the_restatement(G, shape, k, mode):
    B, C, Fw, H, W = shape
    g = gen(Fw * 10 + k)
    for Fo, f0 in ((Fw + (Fw - k), Fw - k), (Fw + 1, Fw - k), (Fw + (Fw - k) - 1, Fw - k), (2 * Fw, 3)):      # full, truncated last windows, odd offset
        if f0 + k > Fo or f0 < 1:
            continue
        win = torch.randn(shape, generator=g) * 3
        numel = B * C * Fo * H * W
        flat = torch.randn((numel + 64,), generator=g)
        flat[numel:] = 1234.5
        out0 = flat[:numel].view(B, C, Fo, H, W).clone()
        dflat = flat.cuda()
        dout = dflat[:numel].view(B, C, Fo, H, W)
        G.ops.clip_window_blend(win.cuda(), dout, f0, k, mode)
        got = dout.cpu()
        assert bool((dflat[numel:].cpu() == 1234.5).all())                               # nothing behind the output
        want = ref.blend(win.numpy().astype(np.float64), out0.numpy().astype(np.float64), f0, k, mode)
        last = min(f0 + Fw, Fo)
        assert torch.equal(got[:, :, :f0], out0[:, :, :f0]) and torch.equal(got[:, :, last:], out0[:, :, last:])      # frames outside the window
        assert torch.equal(got[:, :, f0 + k:last], win[:, :, k:last - f0])               # copied frames: bitwise
        ov_got, ov_old, ov_win = got[:, :, f0:f0 + k], out0[:, :, f0:f0 + k], win[:, :, :k]
        if mode == "keep":
            assert torch.equal(ov_got, ov_old)
        elif mode == "replace":
            assert torch.equal(ov_got, ov_win)
        else:
            # three roundings in a (win - out) -- a, the difference, the product -- and one in the sum, rounded up
            bound = 4 * EPS * (ov_win.abs() + ov_old.abs()).double().numpy()
            err = np.abs(ov_got.double().numpy() - want[:, :, f0:f0 + k])
            print(f"blend {shape} k={k} Fo={Fo}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
            assert not torch.equal(ov_got, ov_old) and not torch.equal(ov_got, ov_win)
    # window 0: no overlap, a plain copy
    win = torch.randn(shape, generator=g)
    dout = torch.full((B, C, Fw + 2, H, W), 5.0, device="cuda")
    G.ops.clip_window_blend(win.cuda(), dout, 0, 0, mode)
    assert torch.equal(dout[:, :, :Fw].cpu(), win) and bool((dout[:, :, Fw:] == 5.0).all())


def test_window_blend_unaligned_views(G):
    """Planes that do not start on a 16-byte boundary take the element path: same results."""
    win = torch.randn((1, 3, 3, 5, 7), generator=gen(9))           # 105 floats per plane: planes 1 and 2 are off 16 bytes
    base = torch.randn((3 * 7 * 35 + 1,), generator=gen(10))
    for off in (0, 1):
        out0 = base[off:off + 3 * 7 * 35].view(1, 3, 7, 5, 7)
        dbase = base.cuda()
        dout = dbase[off:off + 3 * 7 * 35].view(1, 3, 7, 5, 7)
        G.ops.clip_window_blend(win.cuda(), dout, 2, 1, "linear")
        want = ref.blend(win.numpy().astype(np.float64), out0.numpy().astype(np.float64), 2, 1, "linear")
        bound = 4 * EPS * (np.abs(win.numpy()[:, :, :1]) + np.abs(out0.numpy()[:, :, 2:3])).astype(np.float64)
        got = dout.cpu().double().numpy()
        assert bool((np.abs(got[:, :, 2:3] - want[:, :, 2:3]) <= bound).all())
        assert np.array_equal(got[:, :, 3:5], win.double().numpy()[:, :, 1:]) and np.array_equal(got[:, :, :2], out0.double().numpy()[:, :, :2])
        assert np.array_equal(got[:, :, 5:], out0.double().numpy()[:, :, 5:])


# ----------------------------------------------------------------------------- the contract
SHAPE = (4, 4, 4)
B = 8
SEED = 4711


def conds(cfg):
    cond = torch.randn(B, 1, cfg["cond_dim"], generator=gen(5)).cuda()
    return cond, torch.zeros_like(cond)


def manual_chain(G, dm, cfg, n, k, *, mode="renoise", skip=None, jump=None, times=1, mask=None, content=None, traces=None):
    """The chain of existing public calls sample_long is defined by -> (long tokens (B, n hw) on the host, the windows' tokens)."""
    F, hw = SHAPE[0], SHAPE[1] * SHAPE[2]
    s, L = F - k, cfg["L"]
    cond, cf = conds(cfg)
    texts = ["x"] * B
    dm.set_noise(SEED)
    windows = []
    for w in range(ref.windows(F, n, k)):
        if w:
            content = torch.cat([windows[-1][:, s * hw:], torch.zeros((B, s * hw), dtype=torch.int64, device="cuda")], 1)
            mask = G.d3pm.frame_mask(SHAPE, k)
        elif jump is not None and mask is None:                   # the jumps with nothing known
            content, mask = torch.zeros((B, L), dtype=torch.int64), torch.zeros((L,), dtype=torch.bool)
        kw = {} if mask is None else {"known_mask": mask, "known_mode": mode}
        tr = None
        if traces is not None:
            tr = []
            traces.append(tr)
        if skip is not None:
            out = dm.sample_fast(texts, None, cond, content_token=content, filter_ratio=0, skip_step=skip, cf_condition_embed=cf, trace=tr, **kw)
        else:
            if jump is not None:
                kw.update(resample_jump=jump, resample_times=times)
            out = dm.sample(texts, None, cond, cf, content_token=content, filter_ratio=0, trace=tr, **kw)
        windows.append(out["content_token"].clone())
    grid = torch.stack([windows[w][:, f * hw:(f + 1) * hw] for w, f in ref.frame_map(F, n, k)], 1).reshape(B, n * hw)
    return grid.cpu(), [w.cpu() for w in windows], dm.noise_stream


@pytest.fixture(scope="module")
def chains(G, golden):
    """The manual chain of every (k, n), computed once and shared."""
    sd, _, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    cache = {}

    def get(k, n, **kw):
        key = (k, n, tuple(sorted((a, str(b)) for a, b in kw.items())))
        if key not in cache:
            cache[key] = manual_chain(G, dm, cfg, n, k, **kw)
        return cache[key]
    return get


def run_long(G, golden, n, k, **kw):
    sd, _, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    cond, cf = conds(cfg)
    dm.set_noise(SEED)
    out = dm.sample_long(["x"] * B, None, cond, cf, latent_shape=SHAPE, n_frames=n, overlap=k, **kw)
    return dm, out


@pytest.mark.parametrize("k,n,W", [(1, 4, 1), (1, 5, 2), (2, 8, 3), (3, 7, 4), (2, 10, 4)])
@pytest.mark.parametrize("mode", ["lanes2", "lanes1", "eager", "trace"])
def test_sample_long_equals_the_manual_chain(G, golden, chains, k, n, W, mode):
    want, windows, stream_after = chains(k, n)
    trace = [] if mode == "trace" else None
    kw = {"lanes2": {}, "lanes1": {"lanes": 1}, "eager": {"use_graph": False}, "trace": {"trace": trace}}[mode]
    dm, out = run_long(G, golden, n, k, **kw)
    K, hw, s, F = dm.num_classes - 1, 16, SHAPE[0] - k, SHAPE[0]
    tok = out["content_token"]
    assert out["windows"] == W == len(windows) and tuple(tok.shape) == (B, n * hw) and tok.dtype == torch.int64
    assert torch.equal(tok.cpu(), want), f"{int((tok.cpu() != want).sum())} tokens differ from the manual chain"
    assert int((tok == K).sum()) == 0 and int(tok.min()) >= 0
    plan = dm._last_plan
    assert plan.draws == dm._last_draws == W * 100 and dm.noise_stream == stream_after == W * 100
    assert dm._last_lanes == (2 if mode == "lanes2" else 1)
    if W > 1:
        assert plan.windows == W and plan.program.count("slide") == W - 1
    for graphs in dm._last_graphs:                                     # at most one graph per op kind and lane
        assert set(graphs) == ({"step", "slide"} if W >= 3 else {"step"}) if mode in ("lanes2", "lanes1") else graphs == {}
    assert len(dm._last_graphs) == dm._last_lanes
    if mode == "trace":
        assert len(trace) == len(plan.program)
        ends = [i - 1 for i, kind in enumerate(plan.program) if kind == "slide"] + [len(trace) - 1]
        got = [trace[i].cpu() for i in ends]
        assert len(got) == W and all(torch.equal(a, b) for a, b in zip(got, windows))
        for a, b in zip(got, got[1:]):                                 # the overlap carries identical tokens
            assert torch.equal(a[:, s * hw:], b[:, :k * hw])
        for i, kind in enumerate(plan.program):
            if kind == "slide":
                assert bool((trace[i] == K).all())                     # the next window starts from all [MASK]


def test_one_window_is_sample_itself(G, golden):
    sd, _, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    cond, cf = conds(cfg)
    dm.set_noise(SEED)
    want = dm.sample(["x"] * B, None, cond, cf, filter_ratio=0)["content_token"].cpu()
    plain = dm._last_plan
    dm2, out = run_long(G, golden, 4, 1)
    assert torch.equal(out["content_token"].cpu(), want) and dm2._last_plan == plain and dm2.noise_stream == dm.noise_stream
    dm.set_noise(SEED)
    want = dm.sample_fast(["x"] * B, None, cond, filter_ratio=0, skip_step=1, cf_condition_embed=cf)["content_token"].cpu()
    dm3, out = run_long(G, golden, 4, 3, skip_step=1)
    assert torch.equal(out["content_token"].cpu(), want) and dm3._last_plan == dm._last_plan


@pytest.mark.parametrize("case", ["hold", "skip", "resample", "mask"])
def test_sample_long_variants_equal_the_manual_chain(G, golden, chains, case):
    k, n = 2, 8
    g = gen(17)
    mask = torch.zeros((B, 64), dtype=torch.bool)
    mask[:, :16] = True                                                # the caller's first frame ...
    mask[::2, 40:44] = True                                            # ... and a few positions of its own in every other clip
    content = torch.randint(0, 32, (B, 64), generator=g)
    chain_kw, long_kw = {"hold": ({"mode": "hold"}, {"known_mode": "hold"}),
                         "skip": ({"skip": 1}, {"skip_step": 1}),
                         "resample": ({"jump": 10, "times": 2}, {"resample_jump": 10, "resample_times": 2}),
                         "mask": ({"mask": mask, "content": content}, {"known_mask": mask, "content_token": content})}[case]
    if case == "mask":
        want, windows, stream_after = manual_chain(G, build_d3pm(G, *golden("d3pm_L64")[::2]), golden("d3pm_L64")[2], n, k, **chain_kw)
    else:
        want, windows, stream_after = chains(k, n, **chain_kw)
    dm, out = run_long(G, golden, n, k, **long_kw)
    assert out["windows"] == 3 and torch.equal(out["content_token"].cpu(), want), case
    assert dm.noise_stream == stream_after == dm._last_draws and int((out["content_token"] == 32).sum()) == 0
    kinds = {"step", "slide"} | ({"jump"} if case == "resample" else set())
    assert all(set(g_) == kinds for g_ in dm._last_graphs) and dm._last_lanes == 2
    if case == "mask":                                                 # window 0 kept the caller's tokens, the caller's tensors are untouched
        assert torch.equal(out["content_token"].cpu()[:, :64][mask], content[mask])
        assert int(mask.sum()) == 8 * 16 + 4 * 4 and int(content.max()) < 32
    if case == "skip":
        assert dm._last_draws == 3 * 51
    # a different known_mode / plan is a different chain on these inputs: the comparison above can fail
    plain = chains(k, n)[0]
    if case != "mask":
        assert not torch.equal(want[:, 64:], plain[:, 64:]), case


def test_mask_in_an_overlap_raises(G, golden, monkeypatch):
    """A window that leaves [MASK] in its last k frames: counted by the slide, raised after the call."""
    sd, _, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    cond, cf = conds(cfg)
    real = G.ops.d3pm_window_slide

    def planted(tok, *a, **kw):
        if not kw.get("final"):
            tok[:, -1] = 32                                            # (on the lane's stream: the executor issues under it)
        return real(tok, *a, **kw)
    monkeypatch.setattr(G.ops, "d3pm_window_slide", planted)
    with pytest.raises(G.GsddError, match=r"\[MASK\]"):
        dm.sample_long(["x"] * B, None, cond, cf, latent_shape=SHAPE, n_frames=6, overlap=2, use_graph=False)


# ----------------------------------------------------------------------------- decode_long and the glue
def windows_of(vq, tokens, k):
    """per-window decodes at the windows of the plan; a last window past the grid's end is filled with the last frame"""
    n, F = tokens.shape[1], vq.latent_shape[0]
    s = F - k
    out = []
    for w in range(ref.windows(F, n, k)):
        idx = torch.clamp(torch.arange(w * s, w * s + F), max=n - 1).cuda()
        out.append(vq.decode(tokens[:, idx]).cpu())
    return out


@pytest.mark.parametrize("blend", ["linear", "keep", "replace"])
def test_decode_long(G, golden, blend):
    from tests.test_gpu_glue import build
    gen_, vq, batch, a, cfg, cfgd = build(G, golden)
    F, h, w = vq.latent_shape
    dt = vq.downsample[0]
    k = max(1, min(2, F // 2))                                         # k <= s: every output frame is blended at most once
    s = F - k
    for n in sorted({F, F + s, F + s + 1, F + 2 * s + 1}):              # one window; two; a last window of one frame, twice over
        tokens = torch.randint(0, vq.n_codes, (2, n, h, w), generator=gen(n)).cuda()
        got = vq.decode_long(tokens, k, blend=blend)
        if n == F:
            assert torch.equal(got, vq.decode(tokens))                 # bit for bit
            continue
        wins = windows_of(vq, tokens, k)
        assert tuple(got.shape) == (2, 3, n * dt) + tuple(wins[0].shape[3:]) and bool(torch.isfinite(got).all())
        want = np.zeros(tuple(got.shape), dtype=np.float64)
        bound = np.zeros(tuple(got.shape), dtype=np.float64)
        for wi, win in enumerate(wins):
            f0, n_ov = wi * s * dt, (k * dt if wi else 0)
            if n_ov and blend == "linear":
                bound[:, :, f0:f0 + n_ov] = 4 * EPS * (np.abs(win.numpy()[:, :, :n_ov]) + np.abs(want[:, :, f0:f0 + n_ov]))
            want = ref.blend(win.numpy().astype(np.float64), want, f0, n_ov, blend)
        err = np.abs(got.cpu().double().numpy() - want)
        print(f"decode_long {blend} n={n}: {len(wins)} windows, max err {err.max():.3e}, max bound {bound.max():.3e}")
        assert bool((err <= bound).all())                              # copies, keep and replace: bound 0, bitwise
    vq.train()
    with pytest.raises(G.GsddError, match="eval mode"):
        vq.decode_long(tokens, k)
    vq.eval()


def test_generator_and_render_glue(G, golden, tmp_path):
    import src  # noqa: F401
    from src.models.multistage_text_motion_model import MultistageTextMotionModel
    from tests.test_gpu_glue import build
    gen_, vq, batch, a, cfg, cfgd = build(G, golden)
    F, h, w = vq.latent_shape
    dt, k = vq.downsample[0], 1
    n = F + (F - k) + 1                                                # three windows, the last one truncated
    gen_.sample_long_overlap, nb = k, len(batch["text"])
    dm = gen_.diffusion_model.eval()
    dm.set_noise(11)
    clips = gen_.sample_videos(batch["text"], vq, long_frames=n)
    H = batch["video"].shape[-1]
    assert tuple(clips.shape) == (nb, 3, n * dt, H, H) and bool(torch.isfinite(clips).all())
    grid = gen_.last_content_token
    assert tuple(grid.shape) == (nb, n * h * w) and dm._last_plan.windows == 3 and int((grid == dm.num_classes - 1).sum()) == 0
    assert torch.equal(clips, vq.decode_long(grid.view(nb, n, h, w), k, blend="linear"))
    # forward(do_inference=True) keeps sampling one window, whatever sample_long_frames says
    gen_.sample_long_frames = n
    with torch.no_grad():
        out = gen_(batch, vq, None, do_inference=True)
    assert out["pred_data"].shape == out["gt_data"].shape == batch["video"].shape and tuple(gen_.last_content_token.shape) == (nb, F * h * w)
    # the render path writes the long clip, sampled by itself; the evaluation's sample is not used
    model = MultistageTextMotionModel(generator=gen_, autoencoder=vq, lr_args={"gen_lr": 1e-4, "auto_lr": 1e-6}, devices=[0],
                                      render_dir=str(tmp_path), render_max=2).cuda().eval()
    sentinel = {"pred_data": torch.zeros_like(batch["video"])}
    model.render_test_batch(batch, 0, sentinel)
    files = sorted(p.name for p in (tmp_path / "test").iterdir())
    assert files == [f"0_{i}.gif" for i in range(min(nb, 2))] + ["captions.txt"]
    for name in files[:-1]:
        info = G.gif.probe_gif(str(tmp_path / "test" / name))
        assert info["frames"] == n * dt and (info["width"], info["height"]) == (H, H)
        frames, delays, _ = G.gif.read_gif(str(tmp_path / "test" / name), "cuda")
        assert frames.shape[0] == n * dt and int(frames.max()) > 0                 # not the sentinel's black frames
    assert bool((sentinel["pred_data"] == 0).all())


# ----------------------------------------------------------------------------- what fresh memory holds
def test_results_do_not_depend_on_uninitialised_memory(G, golden):
    from tests.test_gpu_glue import build
    sd, _, cfg = golden("d3pm_L64")
    dm = build_d3pm(G, sd, cfg)
    cond, cf = conds(cfg)
    _, vq, _, _, _, _ = build(G, golden)
    F, h, w = vq.latent_shape
    n = F + (F - 1) + 1                                                # overlap 1: three windows, the last truncated

    def run():
        dm.set_noise(SEED)
        out = dm.sample_long(["x"] * B, None, cond, cf, latent_shape=SHAPE, n_frames=7, overlap=2)        # W = 3, one frame in the last
        tokens = torch.randint(0, vq.n_codes, (2, n, h, w), generator=gen(1)).cuda()
        return {"tokens": out["content_token"], "clip": vq.decode_long(tokens, 1)}
    unstable, by_byte, reached = sm.verdict(sm.sweep(run))
    assert unstable == [] and by_byte == {}, (unstable, by_byte)
