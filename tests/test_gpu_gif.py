"""The GIF export on the GPU (csrc/gif.hip, gsdd_amd.gif) against its numpy restatement (tests/gif_ref.py).  Everything behind the
uint8 rule is integer arithmetic, so EVERY comparison is equality: histograms, box sums, indices, palettes, and the pixels PIL decodes
from the written files.  Inputs are built from uint8 levels at the middle of each level's interval (no value on a truncation
boundary); one case adds values below 0, above 1 and a NaN for the clamp.  Shapes: the smallest that take every path -- one workgroup
and several per group, with a ragged tail, for each kernel's chunk (16384 / 4096 / 1024 pixels), clips and frames as groups."""
import io
import types

import numpy as np
import pytest
import torch
from PIL import Image

import gif_ref
from conftest import parity_report

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 8, 8), (1, 2, 17, 23), (3, 1, 16, 16), (1, 2, 96, 100)]     # the last: 19200 pixels a clip, 9600 a frame
CASES = [f"{b}x{t}x{h}x{w}" for b, t, h, w in SHAPES] + ["one_colour", "bins4096", "clamp"]


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def _levels(name):
    if name == "one_colour":                                    # every lane of every wave on one bin
        return np.full((1, 1, 64, 64, 3), (200, 17, 96), dtype=np.uint8)
    if name == "bins4096":                                      # 4096 pixels, 4096 distinct bins
        i = np.arange(4096)
        return (np.stack([i & 15, (i >> 4) & 15, (i >> 8) & 15], axis=-1) * 8 + 3).astype(np.uint8).reshape(1, 1, 64, 64, 3)
    shape = SHAPES[0] if name == "clamp" else tuple(int(v) for v in name.split("x"))
    rng = np.random.default_rng(sum(shape) + 7)
    colours = rng.integers(0, 256, (40, 3))                     # forty colours with a little jitter: shared and neighbouring bins
    pick = rng.integers(0, 40, shape)
    return np.clip(colours[pick] + rng.integers(-3, 4, shape + (3,)), 0, 255).astype(np.uint8)


_CACHE = {}


def case(name):
    """-> (clips float32 numpy, levels uint8 (B, T, H, W, 3)), computed once"""
    if name not in _CACHE:
        levels = _levels(name)
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


def _ref(name, per_frame, colors):
    key = (name, per_frame, colors)
    if key not in _CACHE:
        _, levels = case(name)
        hist = gif_ref.histogram(levels, per_frame)
        cuts = [gif_ref.median_cut(h, colors) for h in hist]
        box = np.stack([c[0] for c in cuts])
        n = np.array([c[1] for c in cuts], dtype=np.int32)
        sums = gif_ref.box_sums(levels, box, per_frame)
        _CACHE[key] = (hist, box, n, sums, gif_ref.palette_of(sums))
    return _CACHE[key]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _report(name, got, want, **extra):
    mism = int(np.count_nonzero(np.asarray(got) != np.asarray(want)))
    parity_report(name, {"mismatches": mism, "compared": int(np.asarray(want).size), **extra})
    assert mism == 0, name


@pytest.mark.parametrize("per_frame", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_histogram(G, name, per_frame):
    clips, levels = case(name)
    want = gif_ref.histogram(levels, bool(per_frame))
    out = torch.full((want.shape[0], 32768), 0x5A5A5A5A, dtype=torch.int32, device="cuda")       # stale contents: the call zeroes
    got = _u32(G.ops.gif_histogram(torch.from_numpy(clips).cuda(), bool(per_frame), out=out))
    assert got.sum(axis=1).tolist() == [levels[0].size // 3 // (levels.shape[1] if per_frame else 1)] * want.shape[0]
    _report(f"gif_histogram_{name}_pf{per_frame}", got, want, occupied_bins=int(np.count_nonzero(want)))


@pytest.mark.parametrize("colors", [16, 256])
@pytest.mark.parametrize("per_frame", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_box_sums(G, name, per_frame, colors):
    clips, levels = case(name)
    _, box, n, want, _ = _ref(name, bool(per_frame), colors)
    out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")
    got = _u32(G.ops.gif_box_sums(torch.from_numpy(clips).cuda(), torch.from_numpy(box).cuda(), bool(per_frame), out=out))
    _report(f"gif_box_sums_{name}_pf{per_frame}_c{colors}", got, want, boxes=n.tolist())


def _pal4(pal):
    return torch.from_numpy(np.concatenate([pal, np.zeros(pal.shape[:2] + (1,), dtype=np.uint8)], axis=-1)).cuda()


@pytest.mark.parametrize("dither", [0, 1, 32, 64])
@pytest.mark.parametrize("per_frame", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_map(G, name, per_frame, dither):
    clips, levels = case(name)
    _, _, n, _, pal = _ref(name, bool(per_frame), 256 if dither in (0, 64) else 16)
    want = gif_ref.map_indices(levels, pal, n, bool(per_frame), dither)
    got = G.ops.gif_map(torch.from_numpy(clips).cuda(), _pal4(pal), torch.from_numpy(n).cuda(), bool(per_frame), dither).cpu().numpy()
    _report(f"gif_map_{name}_pf{per_frame}_d{dither}", got, want)


@pytest.mark.parametrize("n_colors", [1, 2, 255, 256])
def test_map_ties_and_colour_counts(G, n_colors):
    """a palette with duplicated entries and pixels exactly between two entries: the lowest index wins, and only entries in front
    of n_colors are searched (entries behind it are nearer to most pixels here)"""
    rng = np.random.default_rng(n_colors)
    pal = rng.integers(0, 256, (1, 256, 3)).astype(np.uint8)
    pal[0, 0] = (10, 10, 10)
    pal[0, 1] = (20, 10, 10)                                    # (15, 10, 10) is 25 from both
    pal[0, 2:256:2] = pal[0, 3:256:2]                           # every pair behind them duplicated
    pal[0, 254] = pal[0, 0]
    levels = rng.integers(0, 256, (1, 2, 17, 23, 3)).astype(np.uint8)
    levels[0, 0, 0, :8] = (15, 10, 10)
    levels[0, 0, 1, :8] = (10, 15, 10)                          # nearer to entry 0
    levels[0, 1, :4, :4] = pal[0, 2:18].reshape(4, 4, 3)        # pixels that ARE duplicated entries
    n = np.array([n_colors], dtype=np.int32)
    want = gif_ref.map_indices(levels, pal, n)
    assert want.max() < n_colors and (want[0, 0, 0, :8] == 0).all()
    got = G.ops.gif_map(torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda(), _pal4(pal), torch.from_numpy(n).cuda()).cpu().numpy()
    _report(f"gif_map_ties_n{n_colors}", got, want)


def _decode(path_or_bytes):
    im = Image.open(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else path_or_bytes)
    frames = []
    for t in range(getattr(im, "n_frames", 1)):
        im.seek(t)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return im, np.stack(frames)


@pytest.mark.parametrize("palette,colors,dither", [("clip", 256, 0), ("clip", 16, 32), ("frame", 64, 0)])
def test_write_gifs_end_to_end(G, tmp_path, palette, colors, dither):
    levels = np.concatenate([gif_ref.synthetic_levels(False), gif_ref.synthetic_levels(True)])
    clips = gif_ref.clips_from_levels(levels)
    paths = [str(tmp_path / "a" / "clean.gif"), str(tmp_path / "noisy.gif")]
    idx, pal, n = G.gif.write_gifs(torch.from_numpy(clips).cuda(), paths, fps=8, colors=colors, palette=palette, dither=dither)
    idx, pal, n = idx.cpu().numpy(), pal.cpu().numpy(), n.cpu().numpy()
    want_idx, want_pal, want_n = gif_ref.quantize(clips, colors, palette, dither)
    tag = f"gif_e2e_{palette}_c{colors}_d{dither}"
    _report(tag + "_indices", idx, want_idx)
    _report(tag + "_palette", pal, want_pal, n_colors=n.tolist())
    assert np.array_equal(n, want_n) and idx.dtype == np.uint8 and pal.shape == (2 * (4 if palette == "frame" else 1), 256, 3)
    shown = gif_ref.reconstruct(idx, pal, palette == "frame")
    for b, path in enumerate(paths):
        im, frames = _decode(path)
        assert im.size == (32, 32) and im.n_frames == 4 and im.info["loop"] == 0 and im.info["duration"] == 120     # round(100 / 8) = 12 cs
        _report(f"{tag}_decoded_{b}", frames, shown[b])
        # the quality PIL's median cut was measured against (tests/test_gif_host.py) is inherited: the same figure, to the bit
        assert gif_ref.psnr(frames, levels[b]) == gif_ref.psnr(gif_ref.reconstruct(want_idx, want_pal, palette == "frame")[b], levels[b])
    if not dither and palette == "clip":
        direct = G.gif.encode_gif(torch.from_numpy(idx[1]).cuda(), torch.from_numpy(pal[1]).cuda(), int(n[1]), fps=8)
        with open(paths[1], "rb") as f:
            assert f.read() == direct


def test_quantize_clips_is_reproducible_and_checks_arguments(G):
    clips = torch.from_numpy(case("1x2x96x100")[0]).cuda()
    a = G.gif.quantize_clips(clips, colors=64, dither=16)
    b = G.gif.quantize_clips(clips, colors=64, dither=16)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(G.GsddError):
        G.ops.gif_histogram(clips.double())
    with pytest.raises(G.GsddError):
        G.ops.gif_map(clips, torch.zeros((1, 256, 4), dtype=torch.uint8, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"), dither=65)
    with pytest.raises(G.GsddError):
        G.ops.gif_box_sums(clips, torch.zeros((2, 32768), dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------- the model wrappers' hook
def _wrapper(tmp_path, kind, **flags):
    import src  # noqa: F401
    levels = np.concatenate([gif_ref.synthetic_levels(False), gif_ref.synthetic_levels(True)])
    clips = torch.from_numpy(gif_ref.clips_from_levels(levels)).cuda()
    batch = {"video": clips.flip(0).cpu(), "text": ["a clean  ramp", "a noisy\nramp"], "length": [4, 4]}
    if kind == "stage2":
        from src.models.multistage_text_motion_model import MultistageTextMotionModel
        model = MultistageTextMotionModel(generator=torch.nn.Linear(1, 1), autoencoder=torch.nn.Identity(), generator_losses=False, **flags)
    else:
        from src.models.text_motion_model import TextMotionModel
        model = TextMotionModel(generator=torch.nn.Linear(1, 1), **flags)
    calls = []

    def sample(b):                                              # the stubbed sampler: the "sampled" clips of the batch's items
        calls.append(len(b["text"]))
        return {"pred_data": clips[:len(b["text"])], "length": b["length"]}
    model.sample_generator_step = sample
    model.trainer = types.SimpleNamespace(current_epoch=20, callback_metrics={},
                                          datamodule=types.SimpleNamespace(val_dataloader=lambda: [batch]))
    return model, batch, clips, calls


@pytest.mark.parametrize("kind", ["stage1", "stage2"])
def test_model_hook_writes_gifs(G, tmp_path, kind):
    out = tmp_path / "render"
    model, batch, clips, calls = _wrapper(tmp_path, kind, render_animations=True, render_dir=str(out), render_fps=10, render_max=3)
    model.render_sample_results()
    assert calls == [1] and torch.equal(model.last_sample["pred_data"], clips[:1])
    d = out / "epoch_20"
    assert sorted(p.name for p in d.iterdir()) == ["captions.txt", "gt.gif", "pred.gif"]
    assert (d / "captions.txt").read_text() == "pred.gif\ta clean ramp\ngt.gif\ta clean ramp\n"
    for name, src in (("pred.gif", clips[:1]), ("gt.gif", batch["video"][:1].cuda())):
        im, frames = _decode(str(d / name))
        idx, pal, _ = G.gif.quantize_clips(src)
        assert im.n_frames == 4 and im.info["duration"] == 100
        assert np.array_equal(frames, gif_ref.reconstruct(idx.cpu().numpy(), pal.cpu().numpy())[0]), name
    # the test split: the evaluation's sample is reused; without one the hook samples; render_max caps the files
    model.render_test_batch(batch, 0, {"pred_data": clips})
    assert calls == [1]
    model.render_test_batch(batch, 1, None)
    assert calls == [1, 2]
    model.render_test_batch(batch, 2, None)
    assert calls == [1, 2]                                      # the cap was reached: not even sampled
    t = out / "test"
    assert sorted(p.name for p in t.iterdir()) == ["0_0.gif", "0_1.gif", "1_0.gif", "captions.txt"]
    assert (t / "captions.txt").read_text() == "0_0.gif\ta clean ramp\n0_1.gif\ta noisy ramp\n1_0.gif\ta clean ramp\n"
    assert _decode(str(t / "0_1.gif"))[1].shape == (4, 32, 32, 3)


def test_eval_entry_point_leaves_gifs(G, tmp_path):
    """`python src/eval.py model.render_dir=<dir>` at the toy sizes of test_gpu_entrypoints: the test split samples each batch and
    writes its clips, render_max in all, each a file PIL opens"""
    from src.eval import main
    small = ["model=discrete_diffusion", "datamodule.resolution=32", "datamodule.sequence_length=4", "batch_size=2", "datamodule.n_batches=3",
             "model.autoencoder.n_hiddens=16", "model.autoencoder.n_codes=32", "model.autoencoder.embedding_dim=8",
             "model.autoencoder.n_res_layers=1", "model.generator.diffusion_model.content_seq_len=64",
             "model.generator.diffusion_model.diffusion_step=20", "model.generator.diffusion_model.transformer.content_seq_len=64",
             "model.generator.diffusion_model.transformer.n_layer=2",
             "model.generator.diffusion_model.transformer.content_spatial_size=[8,8]",
             "model.generator.diffusion_model.transformer.dalle.num_embed=32",
             "model.generator.diffusion_model.transformer.dalle.spatial_size=[8,8]"]
    out = tmp_path / "gifs"
    metrics = main(small + [f"paths.output_dir={tmp_path}", f"model.render_dir={out}", "model.render_max=3", "model.render_fps=4"])
    assert "total/test" in metrics
    assert sorted(p.name for p in (out / "test").iterdir()) == ["0_0.gif", "0_1.gif", "1_0.gif", "captions.txt"]
    assert len((out / "test" / "captions.txt").read_text().splitlines()) == 3
    for name in ("0_0.gif", "0_1.gif", "1_0.gif"):
        im, frames = _decode(str(out / "test" / name))
        assert frames.shape == (4, 32, 32, 3) and im.info["duration"] == 250 and im.info["loop"] == 0


@pytest.mark.parametrize("kind", ["stage1", "stage2"])
def test_model_hook_is_off_by_default(G, tmp_path, kind, monkeypatch):
    monkeypatch.chdir(tmp_path)
    model, batch, clips, calls = _wrapper(tmp_path, kind, render_animations=True)
    assert model.render_dir is None
    model.render_sample_results()
    model.render_test_batch(batch, 0, None)
    assert calls == [1] and torch.equal(model.last_sample["pred_data"], clips[:1]) and list(tmp_path.iterdir()) == []
    off, _, _, calls_off = _wrapper(tmp_path, kind, render_animations=False, render_dir=str(tmp_path / "r"))
    off.render_sample_results()
    assert calls_off == [] and not hasattr(off, "last_sample") and list(tmp_path.iterdir()) == []
