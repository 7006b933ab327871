"""The palette refinement and the error diffusion of the GIF export without a GPU: what the numpy restatement (tests/gif_refine_ref.py)
gains on the two 4 x 32 x 32 test clips -- the yardsticks the device stages inherit, since the GPU tests pin them to the restatement by
equality --, the selection rule on a hand-made error sequence, and the argument checks that run before any device call."""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import gif_ref
import gif_refine_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(noise, colors) for noise in (False, True) for colors in (256, 64, 16)]
_CACHE = {}


def case(noise, colors):
    """-> levels, n_colors, the median cut's palette, the refined palette (8 passes), the 9 errors; computed once"""
    if (noise, colors) not in _CACHE:
        levels = gif_ref.synthetic_levels(noise)
        _, pal, n = gif_ref.quantize(gif_ref.clips_from_levels(levels), colors)
        refined, errors = ref.refine(levels, pal, n, 8)
        _CACHE[(noise, colors)] = types.SimpleNamespace(levels=levels, n=n, pal=pal, refined=refined, errors=errors)
    return _CACHE[(noise, colors)]


@pytest.fixture(scope="module")
def gsdd():
    import gsdd_amd
    if "GSDD_LIB_PATH" not in os.environ:                 # incremental: a no-op when the library is newer than its sources
        subprocess.check_call(["bash", os.path.join(REPO, "build.sh")], cwd=REPO, stdout=subprocess.DEVNULL)
    gsdd_amd.lib()
    return gsdd_amd


@pytest.mark.parametrize("noise,colors", CASES)
def test_refinement_lowers_the_error(noise, colors):
    c = case(noise, colors)
    before, after = int(c.errors[0, 0]), int(c.errors[:, 0].min())
    print(f"noise={noise} colors={colors}: squared error {before} -> {after}, "
          f"PSNR {10 * np.log10(255.0 ** 2 * c.levels.size / before):.2f} -> {10 * np.log10(255.0 ** 2 * c.levels.size / after):.2f} dB")
    assert after < before
    # the error the refinement reports is the error of the palette it returns, and of the image that palette gives
    sums, sse = ref.palette_sums(c.levels, c.refined, c.n)
    assert int(sse[0]) == after and int(sums[0, :, 0].sum()) == c.levels.size // 3
    shown = gif_ref.reconstruct(gif_ref.map_indices(c.levels, c.refined, c.n), c.refined)
    assert int(((shown.astype(np.int64) - c.levels.astype(np.int64)) ** 2).sum()) == after
    assert not c.refined[0, int(c.n[0]):].any()             # entries behind n_colors stay zeros


def test_refinement_of_the_clean_clip_at_256_colours_is_the_recorded_one():
    c = case(False, 256)
    assert (int(c.errors[0, 0]), int(c.errors[:, 0].min())) == (1010596, 883007)


@pytest.mark.parametrize("noise,colors", CASES)
def test_error_diffusion_beats_no_dither_and_bayer(noise, colors):
    c = case(noise, colors)
    rms = {}
    for name, idx in (("none", gif_ref.map_indices(c.levels, c.refined, c.n)), ("bayer32", gif_ref.map_indices(c.levels, c.refined, c.n, dither=32)),
                      ("fs", ref.diffuse(c.levels, c.refined, c.n))):
        assert idx.max() < int(c.n[0])
        rms[name] = ref.block_mean_rms(gif_ref.reconstruct(idx, c.refined), c.levels)
    print(f"noise={noise} colors={colors}: RMS error of 4 x 4 block means " + ", ".join(f"{k} {v:.3f}" for k, v in rms.items()))
    assert rms["fs"] < rms["none"] and rms["fs"] < rms["bayer32"]


def test_diffuse_by_hand():
    """two pixels, black and white: mid-grey 127 goes to black and leaves +127, of which 7/16 reaches the right neighbour:
    (7*127 + 8) >> 4 = 56, 127 + 56 = 183 -> white, error -72; the row below gets 5 and 3 sixteenths of those"""
    levels = np.full((1, 1, 2, 2, 3), 127, dtype=np.uint8)
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, 1] = 255
    got = ref.diffuse(levels, pal, np.array([2]))[0, 0]
    # (1, 0): acc = 3*(-72) + 5*127 = 419, (419 + 8) >> 4 = 26, 153 -> white, e = -102;
    # (1, 1): acc = 7*(-102) + 5*(-72) + 127 = -947, (-947 + 8) >> 4 = -59 (arithmetic), 68 -> black
    assert got.tolist() == [[0, 1], [1, 0]]
    assert ref.diffuse(levels, pal, np.array([0])).tolist() == [[[[0, 0], [0, 0]]]]


def test_selection_keeps_the_earliest_minimum(gsdd):
    rising = np.array([[5, 7], [6, 7], [9, 3], [9, 3]], dtype=np.uint64)      # group 0 only rises: p_0; group 1: the first 3
    assert ref.select(rising).tolist() == [0, 2]
    pals = [torch.full((2, 256, 4), k, dtype=torch.uint8) for k in range(4)]
    best = gsdd.gif.select_palette(pals, [torch.from_numpy(r.astype(np.int64)) for r in rising])
    assert best[0].unique().tolist() == [0] and best[1].unique().tolist() == [2]


def test_arguments_are_checked_before_any_device_call(gsdd):
    E = gsdd.GsddError
    clips = torch.zeros((1, 3, 2, 8, 8))                      # a CPU tensor: a device call would fail with another message
    for bad in (-1, 33, True, 1.5):
        with pytest.raises(E, match="refine"):
            gsdd.gif.quantize_clips(clips, refine=bad)
        with pytest.raises(E, match="refine"):
            gsdd.gif.write_gifs(clips, ["x.gif"], refine=bad)
    for bad in ("floyd", "FS", 65, True):
        with pytest.raises(E, match="dither"):
            gsdd.gif.quantize_clips(clips, dither=bad)
    with pytest.raises(E, match="ROCm device"):
        gsdd.gif.quantize_clips(clips, refine=8, dither="fs")
    pal, n = torch.zeros((1, 256, 4), dtype=torch.uint8), torch.ones(1, dtype=torch.int32)
    for call in (lambda c: gsdd.ops.gif_palette_sums(c, pal, n), lambda c: gsdd.ops.gif_diffuse(c, pal, n),
                 lambda c: gsdd.gif.palette_error(c, pal[..., :3], n)):
        for c in (clips, clips.double(), clips[0]):
            with pytest.raises(E):
                call(c)
    with pytest.raises(E, match="palette_mode"):
        gsdd.gif.palette_error(clips, pal, n, palette_mode="video")
    assert gsdd.gif.psnr_from_sse(0, 12) == float("inf") and abs(gsdd.gif.psnr_from_sse(1010596, 12288) - 28.98) < 0.005


def test_symbols_version_and_documentation(gsdd):
    L = gsdd.lib()
    assert L.gsdd_version() >= 113
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    with open(os.path.join(REPO, "include", "gsdd.h")) as f:
        header = f.read()
    for name in ("gsdd_gif_palette_sums", "gsdd_gif_diffuse"):
        assert hasattr(L, name) and name in gsdd.EXPORTS and name in doc and header.count(f"int {name}(") == 1, name
    # bad arguments are rejected before any launch (no GPU is touched)
    one, odd = 0x1000, 0x1002
    for args in ((None, 1, 1, 8, 8, 0, one, one, one, one), (one, 1, 1, 8, 8, 0, None, one, one, one), (one, 1, 1, 8, 8, 0, one, None, one, one),
                 (one, 1, 1, 8, 8, 0, one, one, None, one), (one, 1, 1, 8, 8, 0, one, one, one, None), (one, 1, 1, 8, 8, 0, odd, one, one, one),
                 (one, 1, 1, 8, 8, 0, one, one, one, 0x1004), (one, 1, 2, 4096, 4096, 0, one, one, one, one),
                 (one, 1, 1, 8, 65536, 0, one, one, one, one), (one, 1, 1, 8, 8, 2, one, one, one, one)):
        assert L.gsdd_gif_palette_sums(*args, None) == -1, args
    for args in ((None, 1, 1, 8, 8, 0, one, one, one), (one, 1, 1, 8, 8, 0, None, one, one), (one, 1, 1, 8, 8, 0, one, None, one),
                 (one, 1, 1, 8, 8, 0, one, one, None), (one, 1, 1, 8, 8, 0, odd, one, one), (one, 1, 1, 4097, 4096, 1, one, one, one),
                 (one, 1, 1, 65536, 8, 0, one, one, one), (one, 0, 1, 8, 8, 0, one, one, one)):
        assert L.gsdd_gif_diffuse(*args, None) == -1, args
