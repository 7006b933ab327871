"""The delta stage of the GIF export on the GPU (csrc/gif_delta.hip, gsdd_amd.gif.delta_frames / write_gifs(optimize=True)) against its
numpy restatement (tests/gif_delta_ref.py, on top of tests/gif_ref.py).  Integer arithmetic behind the uint8 rule, so EVERY comparison is
equality.  A workgroup covers 1024 pixels of a canvas, a thread four: 1 x 1, 5 x 3 (H W odd: every other frame's slot is off the dword
boundary), 63 x 1 (one ragged thread), 64 x 64 (four whole workgroups) and 97 x 61 = 5917 (six, the last ragged, odd); the LDS table of
rectangles holds 256 frames, so T = 300 takes two chunks.  Every call gets stale output buffers: the call initialises them itself."""
import numpy as np
import pytest
import torch

import gif_delta_ref as ref
import gif_read_ref
import gif_ref
from conftest import parity_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def _pal4(pal):
    return torch.from_numpy(np.concatenate([pal[..., :3], np.full(pal.shape[:2] + (1,), 0x5A, dtype=np.uint8)], axis=-1)).cuda()


def _report(name, got, want, **extra):
    mism = int(np.count_nonzero(np.asarray(got) != np.asarray(want)))
    parity_report(name, {"mismatches": mism, "compared": int(np.asarray(want).size), **extra})
    assert mism == 0, name


def _scene(shape, seed, noise=1, n=40):
    """(B, T, H, W): a still background of a few colours, a 5 x 5 block that moves two pixels right and one down a frame, +-noise levels
    on every value -> (levels (B, T, H, W, 3) uint8, base palette (256, 3) whose first entries are the scene's colours)"""
    B, T, H, W = shape
    rng = np.random.default_rng(seed)
    colours = rng.permutation(1 << 24)[:256]
    base = np.stack([colours & 255, (colours >> 8) & 255, colours >> 16], axis=1).astype(np.uint8)
    cid = np.broadcast_to(rng.integers(1, max(2, min(n, 12)), (B, 1, H, W)), shape).copy()
    for t in range(T):
        cid[:, t, (t % H):(t % H) + 5, (2 * t) % W:(2 * t) % W + 5] = 0
    v = base[cid].astype(np.int64) + rng.integers(-noise, noise + 1, shape + (3,))
    return np.clip(v, 0, 255).astype(np.uint8), base


def _palettes(base, groups, n, per_frame):
    """one table per group with n_colors = n: the base's first n entries, rotated by the group's number when frames are groups -- equal
    colours behind different indices"""
    pal = np.zeros((groups, 256, 3), dtype=np.uint8)
    for g in range(groups):
        pal[g, :n] = np.roll(base[:n], g if per_frame else 0, axis=0)
    return pal, np.full(groups, n, dtype=np.int32)


def _delta(G, tag, levels, idx, pal, n, per_frame, tolerance, clips=None):
    """the kernel into stale buffers against the restatement; -> the restatement's (out, rects, changed, transparent, displayed)"""
    want = ref.delta(levels, idx, pal, n, per_frame, tolerance)
    clips = gif_ref.clips_from_levels(levels) if clips is None else clips
    out = torch.full(idx.shape, 0xEE, dtype=torch.uint8, device="cuda")
    rects = torch.full(idx.shape[:2] + (4,), 12345, dtype=torch.int32, device="cuda")
    changed = torch.full(idx.shape[:2], -7, dtype=torch.int32, device="cuda")
    dev = (torch.from_numpy(clips).cuda(), torch.from_numpy(idx).cuda(), _pal4(pal), torch.from_numpy(np.asarray(n, dtype=np.int32)).cuda())
    for call in range(2):                                       # the second call finds the first one's results in the buffers
        got = G.ops.gif_delta(*dev, bool(per_frame), tolerance, out=out, rects=rects, changed=changed)
        assert got[0] is out and got[1] is rects and got[2] is changed
        full = f"{tag}_pf{int(per_frame)}_tol{tolerance}_call{call}"
        _report(full + "_out", out.cpu().numpy(), want[0], kept=int(want[0].size - want[2].sum()))
        _report(full + "_rects", rects.cpu().numpy(), want[1])
        _report(full + "_changed", changed.cpu().numpy().view(np.uint32), want[2])
    return want


def _mapped(levels, base, n, per_frame):
    B, T = levels.shape[:2]
    pal, nc = _palettes(base, B * T if per_frame else B, n, per_frame)
    return gif_ref.map_indices(levels, pal, nc, per_frame), pal, nc


# ---------------------------------------------------------------------------------------------- canvases and clip lengths
@pytest.mark.parametrize("T", [1, 2, 7, 16])
@pytest.mark.parametrize("hw", [(1, 1), (5, 3), (63, 1), (64, 64), (97, 61)])
def test_canvases_and_lengths(G, hw, T):
    levels, base = _scene((2, T) + hw, hw[0] * 7 + hw[1] + T)
    for per_frame in (False, True):
        idx, pal, n = _mapped(levels, base, 40, per_frame)
        for tolerance in (0, 48):
            want = _delta(G, f"gif_delta_{hw[0]}x{hw[1]}_T{T}", levels, idx, pal, n, per_frame, tolerance)
            assert want[1][:, 0].tolist() == [[0, 0, hw[1] - 1, hw[0] - 1]] * 2 and want[2][:, 0].tolist() == [hw[0] * hw[1]] * 2
    assert T == 1 or hw[0] * hw[1] < 64 or 0 < want[2][:, 1:].sum() < 2 * (T - 1) * hw[0] * hw[1]     # something is kept, something changes


@pytest.mark.parametrize("tolerance", [0, 48])
def test_more_frames_than_the_lds_table_holds(G, tolerance):
    levels, base = _scene((2, 300, 5, 3), 300)
    idx, pal, n = _mapped(levels, base, 16, False)
    want = _delta(G, "gif_delta_5x3_T300", levels, idx, pal, n, False, tolerance)
    assert want[2][:, 256:].any()                                                # frames of the second chunk do change


# ---------------------------------------------------------------------------------------------- colour counts and tolerances
@pytest.mark.parametrize("tolerance", [0, 1, 48, 195075])
@pytest.mark.parametrize("n", [1, 2, 255, 256])
def test_colour_counts_and_tolerances(G, n, tolerance):
    levels, base = _scene((2, 7, 17, 13), n, noise=2, n=n)
    for per_frame in (False, True):
        idx, pal, nc = _mapped(levels, base, n, per_frame)
        out, rects, changed, transparent, displayed = _delta(G, f"gif_delta_n{n}", levels, idx, pal, nc, per_frame, tolerance)
        assert set(transparent.tolist()) == ({-1} if n == 256 else {n})
        if n == 256:                                            # no free index: cropping only, and no tolerance
            assert np.array_equal(out, idx) and np.array_equal(displayed, gif_ref.reconstruct(idx, pal, per_frame))
        elif tolerance == 195075:                               # everything is within it: frame 0 stays for good
            assert not changed[:, 1:].any() and np.all(out[:, 1:] == n) and np.all(rects[:, 1:] == (13, 17, -1, -1))
        if tolerance == 0:
            assert np.array_equal(displayed, gif_ref.reconstruct(idx, pal, per_frame))


def test_duplicated_palette_entries_compare_as_colours(G):
    """every colour twice in the table, and the frames alternate between the two copies: not one pixel changes behind frame 0"""
    levels, base = _scene((1, 6, 17, 13), 3, noise=0)
    levels[:, 1:] = levels[:, :1]
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, 0:80:2] = pal[0, 1:80:2] = base[:40]
    n = np.array([80], dtype=np.int32)
    idx = gif_ref.map_indices(levels, pal, n)
    idx[:, 1::2] += 1                                           # the odd copy in every other frame
    assert np.array_equal(gif_ref.reconstruct(idx, pal)[:, 1], levels[:, 0])
    for tolerance in (0, 48):
        out, rects, changed, _, _ = _delta(G, "gif_delta_duplicates", levels, idx, pal, n, False, tolerance)
        assert not changed[:, 1:].any() and np.all(out[:, 1:] == 80)


def test_change_and_back_drift_and_identical_frames(G):
    # one pixel goes A -> B -> A: repainted twice; the frame between two identical ones is empty
    levels = np.full((1, 5, 5, 3, 3), (10, 200, 90), dtype=np.uint8)
    levels[0, 1, 2, 1] = levels[0, 3, 2, 1] = (200, 10, 90)
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, :2] = ((10, 200, 90), (200, 10, 90))
    n = np.array([2], dtype=np.int32)
    idx = gif_ref.map_indices(levels, pal, n)
    for tolerance in (0, 48):
        _, rects, changed, _, _ = _delta(G, "gif_delta_back_and_forth", levels, idx, pal, n, False, tolerance)
        assert changed[0].tolist() == [15, 1, 1, 1, 1] and rects[0, 1:].tolist() == [[1, 2, 1, 2]] * 4
    same = np.broadcast_to(levels[:, 1:2], levels.shape).copy()
    _, rects, changed, _, _ = _delta(G, "gif_delta_identical_frames", same, gif_ref.map_indices(same, pal, n), pal, n, False, 0)
    assert changed[0].tolist() == [15, 0, 0, 0, 0] and rects[0, 1:].tolist() == [[3, 5, -1, -1]] * 4
    # a drift of one level a frame, every level in the table: 7^2 = 49 > 48, so frames 7 and 14 repaint what frames 1 .. 6 kept --
    # the tolerance is against what is displayed, not against the frame before
    T = 16
    drift = np.full((1, T, 5, 3, 3), 40, dtype=np.uint8)
    drift[0, :, :, :, 0] = 100 + np.arange(T)[:, None, None]
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, :T] = 40
    pal[0, :T, 0] = 100 + np.arange(T)
    n = np.array([T], dtype=np.int32)
    idx = gif_ref.map_indices(drift, pal, n)
    assert idx[0, :, 0, 0].tolist() == list(range(T))
    _, _, changed, _, displayed = _delta(G, "gif_delta_drift", drift, idx, pal, n, False, 48)
    assert changed[0].tolist() == [15 if t % 7 == 0 else 0 for t in range(T)]
    assert displayed[0, :, 0, 0, 0].tolist() == [100 + 7 * (t // 7) for t in range(T)]
    _, _, changed, _, _ = _delta(G, "gif_delta_drift", drift, idx, pal, n, False, 0)
    assert changed[0].tolist() == [15] * T


def test_nan_and_out_of_range_values(G):
    levels, base = _scene((2, 4, 17, 13), 11)
    clips = gif_ref.clips_from_levels(levels)
    flat = clips.reshape(-1)
    flat[3::7] = -4.0                                           # de-normalised below 0
    flat[5::11] = 6.0                                           # above 1
    flat[100::97] = np.nan
    flat[101], flat[102] = np.inf, -np.inf
    levels = gif_ref.levels_of(clips)
    assert levels.min() == 0 and levels.max() == 255
    for per_frame in (False, True):
        idx, pal, n = _mapped(levels, base, 40, per_frame)
        for tolerance in (0, 48, 30000):
            _delta(G, "gif_delta_clamp", levels, idx, pal, n, per_frame, tolerance, clips=clips)


@pytest.mark.parametrize("stage", ["map_dither32", "diffuse"])
def test_indices_of_the_dithering_stages(G, stage):
    """the indices come with a dither, the tolerance compares the level WITHOUT one"""
    levels, base = _scene((2, 5, 33, 31), 5, noise=3)
    clips = gif_ref.clips_from_levels(levels)
    for per_frame in (False, True):
        pal, n = _palettes(base, 10 if per_frame else 2, 6, per_frame)            # half of the scene's colours: there is error to diffuse
        args = (torch.from_numpy(clips).cuda(), _pal4(pal), torch.from_numpy(n).cuda(), per_frame)
        idx = (G.ops.gif_map(*args, 32) if stage == "map_dither32" else G.ops.gif_diffuse(*args)).cpu().numpy()
        assert np.any(idx != gif_ref.map_indices(levels, pal, n, per_frame))
        for tolerance in (0, 48, 768):
            _delta(G, f"gif_delta_{stage}", levels, idx, pal, n, per_frame, tolerance)


# ---------------------------------------------------------------------------------------------- write_gifs, the hooks
def _two_squares():
    levels = np.concatenate([ref.moving_square_levels(noise=2, seed=1), ref.moving_square_levels(noise=2, seed=2)[:, ::-1]])
    return np.ascontiguousarray(levels), gif_ref.clips_from_levels(levels)


@pytest.mark.parametrize("palette", ["clip", "frame"])
@pytest.mark.parametrize("colors", [255, 256])
def test_write_gifs_optimize_reads_back(G, tmp_path, palette, colors, monkeypatch):
    levels, clips = _two_squares()
    dev = torch.from_numpy(clips).cuda()
    per_frame = palette == "frame"
    calls = []
    real = G.ops.gif_delta
    monkeypatch.setattr(G.ops, "gif_delta", lambda *a, **k: calls.append(a[5]) or real(*a, **k))
    sizes = {}
    for tolerance in (None, 0, 48):
        paths = [str(tmp_path / f"{tolerance}_{b}.gif") for b in range(2)]
        kwargs = {} if tolerance is None else {"optimize": True, "tolerance": tolerance}
        idx, pal, n = G.gif.write_gifs(dev, paths, fps=8, colors=colors, palette=palette, **kwargs)
        want_idx, want_pal, want_n = gif_ref.quantize(clips, colors, palette)      # still the unoptimised 3-tuple
        _report(f"gif_delta_write_{palette}_c{colors}_tol{tolerance}_indices", idx.cpu().numpy(), want_idx)
        assert np.array_equal(pal.cpu().numpy(), want_pal) and np.array_equal(n.cpu().numpy(), want_n)
        shown = ref.delta(levels, want_idx, want_pal, want_n, per_frame, tolerance or 0)[4]
        if not tolerance:
            assert np.array_equal(shown, gif_ref.reconstruct(want_idx, want_pal, per_frame))
        for b, path in enumerate(paths):
            frames, delays, info = G.gif.read_gif(path, "cuda")
            assert delays == [12] * 8 and info["frames"] == 8
            _report(f"gif_delta_write_{palette}_c{colors}_tol{tolerance}_read_back_{b}", frames.cpu().numpy(), shown[b])
        sizes[tolerance] = sum((tmp_path / f"{tolerance}_{b}.gif").stat().st_size for b in range(2))
    assert calls == [0, 48]                                     # one launch per optimised call, none for the plain one
    # +-2 levels of noise: the exact delta keeps a scatter of pixels, which LZW likes less than the noise itself (the file grows); the
    # tolerance keeps the whole still background
    assert sizes[48] < sizes[None] and sizes[48] < sizes[0]
    parity_report(f"gif_delta_write_{palette}_c{colors}_bytes", {"plain": sizes[None], "optimize": sizes[0], "tolerance_48": sizes[48]})


def test_write_gifs_defaults_write_what_they_wrote(G, tmp_path, monkeypatch):
    """no option: the file is gsdd_gif_encode's of the quantiser's indices (the reader tests' builder restates that container byte for
    byte), and neither new entry is called"""
    def never(*a, **k):
        raise AssertionError("called by a default write_gifs")
    monkeypatch.setattr(G.ops, "gif_delta", never)
    monkeypatch.setattr(G.ops, "gif_encode_delta", never)
    levels, clips = _two_squares()
    for kwargs in ({}, {"optimize": False, "tolerance": 0}, {"colors": 16, "palette": "frame"}):
        paths = [str(tmp_path / f"{len(kwargs)}_{b}.gif") for b in range(2)]
        G.gif.write_gifs(torch.from_numpy(clips).cuda(), paths, **kwargs)
        idx, pal, n = gif_ref.quantize(clips, kwargs.get("colors", 256), kwargs.get("palette", "clip"))
        for b, path in enumerate(paths):
            if kwargs.get("palette") == "frame":
                frames = [dict(indices=idx[b, t], disposal=1, delay=20, palette=pal[b * 8 + t, :n[b * 8 + t]]) for t in range(8)]
                want = gif_read_ref.build_gif(32, 32, frames, None, loop=0)
            else:
                want = gif_read_ref.build_gif(32, 32, [dict(indices=idx[b, t], disposal=1, delay=20) for t in range(8)], pal[b, :n[b]], loop=0)
            with open(path, "rb") as f:
                assert f.read() == want, (kwargs, b)
    with pytest.raises(G.GsddError, match="tolerance needs optimize"):
        G.gif.write_gifs(torch.from_numpy(clips).cuda(), paths, tolerance=48)


def _wrapper(kind, **flags):
    import src  # noqa: F401
    levels, clips = _two_squares()
    clips = torch.from_numpy(clips).cuda()
    batch = {"video": clips.flip(0).cpu(), "text": ["a square", "another square"], "length": [8, 8]}
    if kind == "stage2":
        from src.models.multistage_text_motion_model import MultistageTextMotionModel
        model = MultistageTextMotionModel(generator=torch.nn.Linear(1, 1), autoencoder=torch.nn.Identity(), generator_losses=False, **flags)
    else:
        from src.models.text_motion_model import TextMotionModel
        model = TextMotionModel(generator=torch.nn.Linear(1, 1), **flags)
    model.sample_generator_step = lambda b: {"pred_data": clips[:len(b["text"])], "length": b["length"]}
    return model, batch, clips


@pytest.mark.parametrize("kind", ["stage1", "stage2"])
def test_model_hook_forwards_optimize_and_tolerance(G, tmp_path, kind):
    files = {}
    cases = (("default", {}, {}), ("optimize", {"render_optimize": True}, {"optimize": True, "colors": 255}),
             ("tolerance", {"render_optimize": True, "render_tolerance": 48}, {"optimize": True, "tolerance": 48, "colors": 255}))
    for name, flags, _ in cases:
        model, batch, clips = _wrapper(kind, render_dir=str(tmp_path / name), **flags)
        assert (model.render_optimize, model.render_tolerance) == (flags.get("render_optimize", False), flags.get("render_tolerance", 0))
        model.render_test_batch(batch, 0, None)
        files[name] = [(tmp_path / name / "test" / f"0_{i}.gif").read_bytes() for i in range(2)]
    for name, _, kwargs in cases:                               # the bytes of write_gifs with the same keywords
        paths = [str(tmp_path / "direct" / name / f"{i}.gif") for i in range(2)]
        G.gif.write_gifs(clips, paths, fps=5, **kwargs)
        for i, p in enumerate(paths):
            with open(p, "rb") as f:
                assert f.read() == files[name][i], (name, i)
    assert all(len(files["tolerance"][i]) < len(files["default"][i]) and files["optimize"][i] != files["default"][i] for i in range(2))


def test_eval_entry_point_takes_the_options(G, tmp_path):
    """`python src/eval.py model.render_dir=<dir> model.render_optimize=true model.render_tolerance=48` at the toy sizes of
    test_gpu_gif.py"""
    from src.eval import main
    small = ["model=discrete_diffusion", "datamodule.resolution=32", "datamodule.sequence_length=4", "batch_size=2", "datamodule.n_batches=1",
             "model.autoencoder.n_hiddens=16", "model.autoencoder.n_codes=32", "model.autoencoder.embedding_dim=8",
             "model.autoencoder.n_res_layers=1", "model.generator.diffusion_model.content_seq_len=64",
             "model.generator.diffusion_model.diffusion_step=20", "model.generator.diffusion_model.transformer.content_seq_len=64",
             "model.generator.diffusion_model.transformer.n_layer=2",
             "model.generator.diffusion_model.transformer.content_spatial_size=[8,8]",
             "model.generator.diffusion_model.transformer.dalle.num_embed=32",
             "model.generator.diffusion_model.transformer.dalle.spatial_size=[8,8]"]
    seen, launched = [], []
    real, real_delta = G.gif.quantize_clips, G.ops.gif_delta

    def spy(clips, **kwargs):
        seen.append(kwargs)
        return real(clips, **kwargs)

    def spy_delta(*args, **kwargs):
        launched.append(args[5])
        return real_delta(*args, **kwargs)
    G.gif.quantize_clips, G.ops.gif_delta = spy, spy_delta
    try:
        main(small + [f"paths.output_dir={tmp_path}", f"model.render_dir={tmp_path / 'gifs'}", "model.render_max=2",
                      "model.render_optimize=true", "model.render_tolerance=48"])
    finally:
        G.gif.quantize_clips, G.ops.gif_delta = real, real_delta
    assert seen == [{"refine": 0, "dither": 0, "colors": 255}] and launched == [48]
    for name in ("0_0.gif", "0_1.gif"):
        assert G.gif.read_gif(str(tmp_path / "gifs" / "test" / name), "cuda")[0].shape == (4, 32, 32, 3)


# ---------------------------------------------------------------------------------------------- bad arguments
def test_entry_rejects_bad_arguments(G):
    L = G.lib()
    clips = torch.zeros((1, 3, 2, 8, 8), device="cuda")
    idx = torch.zeros((1, 2, 8, 8), dtype=torch.uint8, device="cuda")
    pal = torch.zeros((2, 256, 4), dtype=torch.uint8, device="cuda")
    n = torch.ones(2, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(idx)
    rects = torch.zeros((1, 2, 4), dtype=torch.int32, device="cuda")
    changed = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    c, i, p, k, o, r, h = (t.data_ptr() for t in (clips, idx, pal, n, out, rects, changed))
    ok = (c, i, 1, 2, 8, 8, 0, p, k, 0, o, r, h)
    assert L.gsdd_gif_delta(*ok, None) == 0
    for j in (0, 1, 7, 8, 10, 11, 12):                          # each pointer null in turn
        assert L.gsdd_gif_delta(*ok[:j], None, *ok[j + 1:], None) == -1, j
    for j, bad in ((7, p + 2), (11, r + 2), (12, h + 1), (9, -1), (9, 195076), (10, i), (6, 2), (2, 0), (3, -1), (4, 65536), (5, 65536)):
        assert L.gsdd_gif_delta(*ok[:j], bad, *ok[j + 1:], None) == -1, (j, bad)
    assert L.gsdd_gif_delta(c, i, 1, 2, 4096, 4096, 0, p, k, 0, o, r, h, None) == -1          # 2^25 pixels in a clip
    assert L.gsdd_gif_delta(c, i, 1, 1, 4097, 4096, 1, p, k, 0, o, r, h, None) == -1          # more than 2^24 in a frame
    torch.cuda.synchronize()
    E = G.GsddError
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx, pal[:1, :, :3], n[:1])
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx, pal, n, per_frame=False)                    # two palettes for one clip
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx[:, :1], pal[:1], n[:1])
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx, pal[:1], n[:1], out=idx)
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx, pal[:1], n[:1], rects=rects.long())
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx, pal[:1], n[:1], changed=changed[:, :1])
    with pytest.raises(E):
        G.ops.gif_delta(clips, idx.cpu(), pal[:1], n[:1])
    got = G.gif.delta_frames(clips, idx, pal[:, :, :3], n, palette_mode="frame", tolerance=3)
    assert [tuple(t.shape) for t in got] == [(1, 2, 8, 8), (1, 2, 4), (1, 2), (2,)] and got[3].tolist() == [1, 1]
