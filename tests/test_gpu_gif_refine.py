"""The palette refinement and the error diffusion of the GIF export on the GPU (csrc/gif_refine.hip, gsdd_amd.gif) against their numpy
restatement (tests/gif_refine_ref.py, on top of tests/gif_ref.py).  Integer arithmetic behind the uint8 rule, so EVERY comparison is
equality.  Shapes are the smallest that take every path: for the assignment pass one workgroup per group and two with a ragged tail
(its chunk is 4096 pixels; 4097 and 4160 pixels here), clips and frames as groups; for the diffusion every number of lanes a row is given (16, 8, 4, 2, 1), frames
of one row and one column, frames of more rows than the workgroup's 1024 threads (bands, the band row in LDS) and rows longer than twice
the rows at a time.  Not here: a frame of more than 1024 rows AND more than 2047 columns, where the bands start W + 1 rather than 2048 steps
apart -- two million pixels cost the restatement a minute; that arithmetic is the same expression at any size."""
import types

import numpy as np
import pytest
import torch

import gif_ref
import gif_refine_ref as ref
from conftest import parity_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _pal4(pal):
    return torch.from_numpy(np.concatenate([pal[..., :3], np.zeros(pal.shape[:2] + (1,), dtype=np.uint8)], axis=-1)).cuda()


def _report(name, got, want, **extra):
    mism = int(np.count_nonzero(np.asarray(got) != np.asarray(want)))
    parity_report(name, {"mismatches": mism, "compared": int(np.asarray(want).size), **extra})
    assert mism == 0, name


def _coloured(shape, seed):
    """forty colours with a little jitter, as tests/test_gpu_gif.py draws them: shared and neighbouring bins"""
    rng = np.random.default_rng(seed)
    colours = rng.integers(0, 256, (40, 3))
    return np.clip(colours[rng.integers(0, 40, shape)] + rng.integers(-3, 4, shape + (3,)), 0, 255).astype(np.uint8)


_CACHE = {}


def sums_case(name):
    """-> (clips float32 numpy, levels uint8 (B, T, H, W, 3)), computed once"""
    if name not in _CACHE:
        if name == "one_colour":
            levels = np.full((1, 2, 16, 16, 3), (200, 17, 96), dtype=np.uint8)
        else:
            shape = (2, 3, 8, 8) if name == "clamp" else tuple(int(v) for v in name.split("x"))
            levels = _coloured(shape, sum(shape) + 3)
        clips = gif_ref.clips_from_levels(levels)
        if name == "clamp":
            flat = clips.reshape(-1)
            flat[3::7] = -4.0                                    # de-normalised below 0
            flat[5::11] = 6.0                                    # above 1
            flat[100] = np.nan
            flat[101], flat[102] = np.inf, -np.inf
            levels = gif_ref.levels_of(clips)
            assert levels.min() == 0 and levels.max() == 255
        else:
            assert np.array_equal(gif_ref.levels_of(clips), levels)
        _CACHE[name] = (clips, levels)
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------- gsdd_gif_palette_sums
# 8 x 8 x 3 and 17 x 23 x 2: one workgroup a group; 1 x 17 x 241 = 4097 pixels a clip, 2 x 64 x 65 = 4160 a frame: two, the second ragged
@pytest.mark.parametrize("colors", [16, 256])
@pytest.mark.parametrize("per_frame", [0, 1])
@pytest.mark.parametrize("name", ["2x3x8x8", "1x2x17x23", "1x1x17x241", "1x2x64x65", "one_colour", "clamp"])
def test_palette_sums(G, name, per_frame, colors):
    clips, levels = sums_case(name)
    _, pal, n = gif_ref.quantize(clips, colors, "frame" if per_frame else "clip")
    want, want_sse = ref.palette_sums(levels, pal, n, bool(per_frame))
    # stale contents, and two calls into the same buffers: the call zeroes both outputs itself
    out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")
    sse = torch.full(want_sse.shape, 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(clips).cuda()
    for call in range(2):
        got, got_sse = G.ops.gif_palette_sums(dev, _pal4(pal), torch.from_numpy(n).cuda(), bool(per_frame), out=out, sse_out=sse)
        assert got is out and got_sse is sse
        tag = f"gif_palette_sums_{name}_pf{per_frame}_c{colors}_call{call}"
        _report(tag, _u32(got), want, n_colors=n.tolist())
        _report(tag + "_sse", _u64(got_sse), want_sse, sse=want_sse.tolist())
    assert want[..., 0].sum(axis=1).tolist() == [levels[0].size // 3 // (levels.shape[1] if per_frame else 1)] * want.shape[0]


@pytest.mark.parametrize("n_colors", [0, 1, 2, 255, 256])
def test_palette_sums_ties_and_colour_counts(G, n_colors):
    """a palette with duplicated entries and pixels exactly between two entries: the lowest index takes them, the higher of two equal
    entries comes out empty, and only entries in front of n_colors take part (none at all with n_colors = 0: zeros)"""
    rng = np.random.default_rng(n_colors)
    pal = rng.integers(0, 256, (1, 256, 3)).astype(np.uint8)
    pal[0, 0] = (10, 10, 10)
    pal[0, 1] = (20, 10, 10)                                    # (15, 10, 10) is 25 from both
    pal[0, 3:256:2] = pal[0, 2:255:2]                           # every pair behind them duplicated: the odd entry is the copy
    levels = rng.integers(0, 256, (1, 2, 17, 23, 3)).astype(np.uint8)
    levels[0, 0, 0, :8] = (15, 10, 10)
    levels[0, 1, :4, :4] = pal[0, 2:18].reshape(4, 4, 3)        # pixels that ARE duplicated entries
    n = np.array([n_colors], dtype=np.int32)
    want, want_sse = ref.palette_sums(levels, pal, n)
    assert not want[0, 3:256:2].any() and (n_colors < 2 or want[0, 0, 0] >= 8) and (n_colors > 0 or not want.any())
    got, got_sse = G.ops.gif_palette_sums(torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda(), _pal4(pal), torch.from_numpy(n).cuda())
    _report(f"gif_palette_sums_ties_n{n_colors}", _u32(got), want)
    _report(f"gif_palette_sums_ties_n{n_colors}_sse", _u64(got_sse), want_sse, sse=want_sse.tolist())


def test_palette_sums_error_beyond_32_bits(G):
    """a 160 x 160 white frame against the one-entry palette (0, 0, 0): 25,600 * 195,075 > 2^32; a second group keeps a small error"""
    levels = np.full((2, 1, 160, 160, 3), 255, dtype=np.uint8)
    levels[1] = 1
    pal = np.zeros((2, 256, 3), dtype=np.uint8)
    n = np.array([1, 1], dtype=np.int32)
    want, want_sse = ref.palette_sums(levels, pal, n)
    assert want_sse.tolist() == [25600 * 195075, 25600 * 3] and want_sse[0] > 2 ** 32
    got, got_sse = G.ops.gif_palette_sums(torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda(), _pal4(pal), torch.from_numpy(n).cuda())
    _report("gif_palette_sums_wide_sse", _u64(got_sse), want_sse, sse=want_sse.tolist())
    _report("gif_palette_sums_wide", _u32(got), want)


# ---------------------------------------------------------------------------------------------- gsdd_gif_diffuse
def _smooth(shape, seed):
    """a colour ramp with noise: what error diffusion is for (most pixels sit between palette entries)"""
    B, T, H, W = shape
    rng = np.random.default_rng(seed)
    b, t, y, x = np.meshgrid(np.arange(B), np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    v = np.stack([(5 * x + 40 * t + 90 * b) % 256, (7 * y + 3 * x) % 256, (2 * (x + y) + 60 * t) % 256], axis=-1)
    return np.clip(v + rng.integers(-6, 7, v.shape), 0, 255).astype(np.uint8)


def _random_palette(G_, seed):
    return np.random.default_rng(seed).integers(0, 256, (G_, 256, 3)).astype(np.uint8)


def _diffuse(G, tag, levels, pal, n, per_frame=False):
    want = ref.diffuse(levels, pal, n, per_frame)
    clips = gif_ref.clips_from_levels(levels)
    out = torch.full(want.shape, 0xEE, dtype=torch.uint8, device="cuda")
    got = G.ops.gif_diffuse(torch.from_numpy(clips).cuda(), _pal4(pal), torch.from_numpy(np.asarray(n, dtype=np.int32)).cuda(), per_frame, out=out)
    plain = gif_ref.map_indices(levels, pal, n, per_frame)
    _report(tag, got.cpu().numpy(), want, differs_from_plain_map=int(np.count_nonzero(want != plain)))
    return want, plain


# lanes a row: 16 up to 64 rows (64 x 64 fills the workgroup), 8 at 65, 4 at 130, 2 at 300, 1 at 600; 1030 and 2049 rows: two and three
# bands of 1024; 1 x 3000 and 3 x 150: rows longer than twice the rows at a time
@pytest.mark.parametrize("hw,n_colors", [((1, 1), 8), ((1, 7), 8), ((7, 1), 8), ((5, 3), 8), ((17, 13), 256), ((64, 64), 256), ((65, 9), 16),
                                         ((130, 5), 8), ((300, 3), 7), ((600, 2), 8), ((1030, 3), 8), ((2049, 2), 4), ((1, 3000), 2),
                                         ((3, 150), 8)])
def test_diffuse_frame_sizes(G, hw, n_colors):
    levels = _smooth((1, 1) + hw, hw[0] * 31 + hw[1])
    want, plain = _diffuse(G, f"gif_diffuse_{hw[0]}x{hw[1]}_n{n_colors}", levels, _random_palette(1, hw[1]), [n_colors])
    assert hw[0] * hw[1] < 64 or np.any(want != plain)          # the larger cases do diffuse something


@pytest.mark.parametrize("per_frame", [0, 1])
def test_diffuse_clips_and_frames_as_groups(G, per_frame):
    """T > 1: every frame starts without error, and takes the palette of its clip or its own"""
    levels = _smooth((2, 3, 17, 13), 5)
    groups = 6 if per_frame else 2
    n = [256, 2, 16, 1, 8, 256][:groups]
    want, _ = _diffuse(G, f"gif_diffuse_groups_pf{per_frame}", levels, _random_palette(groups, 9 + per_frame), n, bool(per_frame))
    same = levels.copy()
    same[:, 1:] = same[:, :1]                                   # equal frames under one palette give equal indices: nothing is carried over
    pal = _random_palette(2, 4)
    want, _ = _diffuse(G, f"gif_diffuse_equal_frames_pf{per_frame}", same, pal[[0, 0, 0, 1, 1, 1]] if per_frame else pal,
                       [8] * groups, bool(per_frame))
    assert np.array_equal(want[:, 0], want[:, 1]) and np.array_equal(want[:, 0], want[:, 2])


@pytest.mark.parametrize("n_colors", [0, 1, 2, 256])
def test_diffuse_colour_counts(G, n_colors):
    """entries behind n_colors are not searched; n_colors = 0 writes index 0 as gsdd_gif_map does; duplicated entries: the lowest index"""
    pal = _random_palette(1, 21)
    pal[0, 3:256:2] = pal[0, 2:255:2]
    want, _ = _diffuse(G, f"gif_diffuse_n{n_colors}", _smooth((1, 2, 17, 13), 8), pal, [n_colors])
    assert want.max() < max(n_colors, 1) and not (want[want > 1] & 1).any()


def test_diffuse_saturates_the_clamp(G):
    """black and white only, on mid-grey: errors of +-127 accumulate to targets beyond [0, 255] and are clamped"""
    levels = np.full((1, 1, 17, 13, 3), 127, dtype=np.uint8)
    levels[0, 0, 5:9] = (250, 3, 128)
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, 1] = 255
    want, _ = _diffuse(G, "gif_diffuse_black_white", levels, pal, [2])
    assert 0.3 < want.mean() < 0.7                              # a checkerboard-like mixture, not one colour


# ---------------------------------------------------------------------------------------------- quantize_clips
def _two_clips():
    levels = np.concatenate([gif_ref.synthetic_levels(False), gif_ref.synthetic_levels(True)])
    return levels, gif_ref.clips_from_levels(levels)


def _refined(colors, palette, passes):
    """the restatement of quantize_clips(refine=passes) in front of the index stage, computed once"""
    key = ("refined", colors, palette, passes)
    if key not in _CACHE:
        levels, clips = _two_clips()
        _, pal0, n = gif_ref.quantize(clips, colors, palette)
        pal, errors = ref.refine(levels, pal0, n, passes, palette == "frame")
        _CACHE[key] = types.SimpleNamespace(levels=levels, clips=clips, pal0=pal0, n=n, pal=pal, errors=errors)
    return _CACHE[key]


@pytest.mark.parametrize("colors,palette,passes,dither", [(64, "clip", 1, 0), (64, "clip", 3, 16), (64, "clip", 8, "fs"), (16, "frame", 3, "fs"),
                                                          (256, "clip", 8, 0)])
def test_quantize_clips_refined(G, colors, palette, passes, dither):
    r = _refined(colors, palette, passes)
    per_frame = palette == "frame"
    dev = torch.from_numpy(r.clips).cuda()
    idx, pal, n = G.gif.quantize_clips(dev, colors=colors, palette=palette, dither=dither, refine=passes)
    again = G.gif.quantize_clips(dev, colors=colors, palette=palette, dither=dither, refine=passes)
    assert all(torch.equal(a, b) for a, b in zip((idx, pal, n), again))                       # two runs are bit-identical
    tag = f"gif_refine_c{colors}_{palette}_N{passes}_d{dither}"
    _report(tag + "_palette", pal.cpu().numpy(), r.pal, n_colors=r.n.tolist())
    assert np.array_equal(n.cpu().numpy(), r.n) and pal.shape == r.pal.shape and pal.dtype == torch.uint8
    want_idx = ref.diffuse(r.levels, r.pal, r.n, per_frame) if dither == "fs" else gif_ref.map_indices(r.levels, r.pal, r.n, per_frame, dither)
    _report(tag + "_indices", idx.cpu().numpy(), want_idx)
    # the N + 1 errors of p_0 .. p_N, from the median cut's palette
    got_pal4, errors = G.gif.refine_palette(dev, _pal4(r.pal0), n, passes, per_frame)
    _report(tag + "_errors", _u64(errors), r.errors, errors=r.errors.tolist())
    assert torch.equal(got_pal4[..., :3], pal) and errors.shape == (passes + 1, r.n.size) and errors.dtype == torch.int64
    # never worse than the median cut, by construction -- and strictly better on these clips (tests/test_gif_refine_host.py)
    before = G.gif.palette_error(dev, torch.from_numpy(r.pal0).cuda(), n, palette)
    after = G.gif.palette_error(dev, pal, n, palette)
    assert before.dtype == torch.int64 and before.is_cuda and bool((after <= before).all())
    assert _u64(before).tolist() == r.errors[0].tolist() and _u64(after).tolist() == r.errors.min(axis=0).tolist()
    values = r.levels[0].size // (4 if per_frame else 1)
    assert G.gif.psnr_from_sse(int(after[0]), values) >= G.gif.psnr_from_sse(int(before[0]), values)


def test_quantize_clips_defaults_are_unchanged(G, monkeypatch):
    """refine = 0 with an integer dither: the 3-tuple of the quantiser as it was (its restatement, tests/gif_ref.py), and neither new
    entry is launched"""
    def never(*a, **k):
        raise AssertionError("launched by a default call")
    monkeypatch.setattr(G.ops, "gif_palette_sums", never)
    monkeypatch.setattr(G.ops, "gif_diffuse", never)
    levels, clips = _two_clips()
    dev = torch.from_numpy(clips).cuda()
    for kwargs in ({}, {"refine": 0, "dither": 0}, {"colors": 16, "dither": 32, "palette": "frame"}):
        got = G.gif.quantize_clips(dev, **kwargs)
        want = gif_ref.quantize(clips, kwargs.get("colors", 256), kwargs.get("palette", "clip"), kwargs.get("dither", 0))
        assert len(got) == 3
        for part, g, w in zip(("indices", "palette", "n_colors"), got, want):
            _report(f"gif_defaults_{len(kwargs)}_{part}", g.cpu().numpy(), w)


# ---------------------------------------------------------------------------------------------- write_gifs and the hooks
def test_write_gifs_refined_and_diffused_reads_back(G, tmp_path):
    levels, clips = _two_clips()
    paths = [str(tmp_path / "clean.gif"), str(tmp_path / "noisy.gif")]
    idx, pal, n = G.gif.write_gifs(torch.from_numpy(clips).cuda(), paths, fps=8, colors=64, refine=8, dither="fs")
    r = _refined(64, "clip", 8)
    _report("gif_write_refined_palette", pal.cpu().numpy(), r.pal)
    shown = gif_ref.reconstruct(idx.cpu().numpy(), pal.cpu().numpy())
    for b, path in enumerate(paths):
        frames, delays, info = G.gif.read_gif(path, "cuda")
        assert delays == [12] * 4 and info["frames"] == 4
        _report(f"gif_write_refined_read_back_{b}", frames.cpu().numpy(), shown[b])


def _wrapper(kind, **flags):
    import src  # noqa: F401
    levels, clips = _two_clips()
    clips = torch.from_numpy(clips).cuda()
    batch = {"video": clips.flip(0).cpu(), "text": ["a clean ramp", "a noisy ramp"], "length": [4, 4]}
    if kind == "stage2":
        from src.models.multistage_text_motion_model import MultistageTextMotionModel
        model = MultistageTextMotionModel(generator=torch.nn.Linear(1, 1), autoencoder=torch.nn.Identity(), generator_losses=False, **flags)
    else:
        from src.models.text_motion_model import TextMotionModel
        model = TextMotionModel(generator=torch.nn.Linear(1, 1), **flags)
    model.sample_generator_step = lambda b: {"pred_data": clips[:len(b["text"])], "length": b["length"]}
    return model, batch, clips


@pytest.mark.parametrize("kind", ["stage1", "stage2"])
def test_model_hook_forwards_refine_and_dither(G, tmp_path, kind):
    files = {}
    for name, flags in (("default", {}), ("refine", {"render_refine": 8}), ("fs", {"render_dither": "fs"}), ("both", {"render_refine": 8, "render_dither": "fs"})):
        model, batch, clips = _wrapper(kind, render_dir=str(tmp_path / name), **flags)
        assert (model.render_refine, model.render_dither) == (flags.get("render_refine", 0), flags.get("render_dither", 0))
        model.render_test_batch(batch, 0, None)
        files[name] = [(tmp_path / name / "test" / f"0_{i}.gif").read_bytes() for i in range(2)]
    # not set: the bytes of a plain write_gifs call; set: the bytes of write_gifs with the same keywords
    for name, kwargs in (("default", {}), ("refine", {"refine": 8}), ("fs", {"dither": "fs"}), ("both", {"refine": 8, "dither": "fs"})):
        paths = [str(tmp_path / "direct" / name / f"{i}.gif") for i in range(2)]
        G.gif.write_gifs(clips, paths, fps=5, **kwargs)
        for i, p in enumerate(paths):
            with open(p, "rb") as f:
                assert f.read() == files[name][i], (name, i)
    for name in ("refine", "fs", "both"):
        assert all(files[name][i] != files["default"][i] for i in range(2)), name
    assert files["both"] != files["refine"] and files["both"] != files["fs"]


def test_eval_entry_point_takes_the_options(G, tmp_path):
    """`python src/eval.py model.render_dir=<dir> model.render_refine=8 model.render_dither=fs` at the toy sizes of test_gpu_gif.py"""
    from src.eval import main
    small = ["model=discrete_diffusion", "datamodule.resolution=32", "datamodule.sequence_length=4", "batch_size=2", "datamodule.n_batches=1",
             "model.autoencoder.n_hiddens=16", "model.autoencoder.n_codes=32", "model.autoencoder.embedding_dim=8",
             "model.autoencoder.n_res_layers=1", "model.generator.diffusion_model.content_seq_len=64",
             "model.generator.diffusion_model.diffusion_step=20", "model.generator.diffusion_model.transformer.content_seq_len=64",
             "model.generator.diffusion_model.transformer.n_layer=2",
             "model.generator.diffusion_model.transformer.content_spatial_size=[8,8]",
             "model.generator.diffusion_model.transformer.dalle.num_embed=32",
             "model.generator.diffusion_model.transformer.dalle.spatial_size=[8,8]"]
    seen = []
    real = G.gif.quantize_clips

    def spy(clips, **kwargs):
        seen.append(kwargs)
        return real(clips, **kwargs)
    G.gif.quantize_clips = spy
    try:
        main(small + [f"paths.output_dir={tmp_path}", f"model.render_dir={tmp_path / 'gifs'}", "model.render_max=2", "model.render_refine=8",
                      "model.render_dither=fs"])
    finally:
        G.gif.quantize_clips = real
    assert seen == [{"refine": 8, "dither": "fs"}]
    for name in ("0_0.gif", "0_1.gif"):
        assert G.gif.read_gif(str(tmp_path / "gifs" / "test" / name), "cuda")[0].shape == (4, 32, 32, 3)


# ---------------------------------------------------------------------------------------------- bad arguments
def test_entries_reject_bad_arguments(G):
    L = G.lib()
    clips = torch.zeros((1, 3, 1, 8, 8), device="cuda")
    pal = torch.zeros((2, 256, 4), dtype=torch.uint8, device="cuda")
    n = torch.ones(1, dtype=torch.int32, device="cuda")
    sums = torch.zeros((1, 256, 4), dtype=torch.int32, device="cuda")
    sse = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device="cuda")
    c, p, k, s, e, o = (t.data_ptr() for t in (clips, pal, n, sums, sse, out))
    ok = (c, 1, 1, 8, 8, 0, p, k, s, e)
    assert L.gsdd_gif_palette_sums(*ok, None) == 0
    for i in (0, 6, 7, 8, 9):                                   # each pointer null in turn
        assert L.gsdd_gif_palette_sums(*ok[:i], None, *ok[i + 1:], None) == -1, i
    assert L.gsdd_gif_palette_sums(c, 1, 1, 8, 8, 0, p + 1, k, s, e, None) == -1              # a misaligned palette
    assert L.gsdd_gif_palette_sums(c, 1, 1, 8, 8, 0, p, k, s, e + 4, None) == -1              # a misaligned error word
    assert L.gsdd_gif_palette_sums(c, 1, 2, 4096, 4096, 0, p, k, s, e, None) == -1            # 2^25 pixels in a group
    assert L.gsdd_gif_palette_sums(c, 1, 1, 8, 65536, 0, p, k, s, e, None) == -1
    ok = (c, 1, 1, 8, 8, 0, p, k, o)
    assert L.gsdd_gif_diffuse(*ok, None) == 0
    for i in (0, 6, 7, 8):
        assert L.gsdd_gif_diffuse(*ok[:i], None, *ok[i + 1:], None) == -1, i
    assert L.gsdd_gif_diffuse(c, 1, 1, 8, 8, 0, p + 2, k, o, None) == -1
    assert L.gsdd_gif_diffuse(c, 1, 1, 4097, 4096, 1, p, k, o, None) == -1                   # more than 2^24 pixels in a frame
    assert L.gsdd_gif_diffuse(c, 1, 1, 8, 8, 3, p, k, o, None) == -1
    torch.cuda.synchronize()
    with pytest.raises(G.GsddError):
        G.ops.gif_palette_sums(clips, pal[:1, :, :3], n)
    with pytest.raises(G.GsddError):
        G.ops.gif_diffuse(clips, pal[:1], n.long())
    with pytest.raises(G.GsddError):
        G.ops.gif_palette_sums(clips, pal[:1], n, sse_out=torch.zeros(1, dtype=torch.int32, device="cuda"))
