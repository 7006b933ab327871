"""Host half of the GIF export (csrc/gif_host.hpp behind gsdd_gif_median_cut / gsdd_gif_encode, gsdd_amd.gif), without a GPU:
the library's median cut against the numpy restatement (tests/gif_ref.py), the GIF89a / LZW writer through PIL as the independent
decoder, the restatement's quality against PIL's own median cut, and the wrappers' argument checks."""
import io
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import gif_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gsdd():
    import gsdd_amd
    if "GSDD_LIB_PATH" not in os.environ:                 # incremental: a no-op when the library is newer than its sources
        subprocess.check_call(["bash", os.path.join(REPO, "build.sh")], cwd=REPO, stdout=subprocess.DEVNULL)
    gsdd_amd.lib()
    return gsdd_amd


# ---------------------------------------------------------------------------------------------- median cut
def _histograms():
    rng = np.random.default_rng(1)
    out = {"synthetic": gif_ref.histogram(gif_ref.synthetic_levels())[0],
           "synthetic_noise": gif_ref.histogram(gif_ref.synthetic_levels(noise=True))[0]}
    one = np.zeros(gif_ref.BINS, dtype=np.uint32)
    one[12345] = 4096
    out["one_bin"] = one
    h256 = np.zeros(gif_ref.BINS, dtype=np.uint32)
    h256[rng.choice(gif_ref.BINS, 256, replace=False)] = rng.integers(1, 1000, 256).astype(np.uint32)
    out["256_bins"] = h256
    h300 = np.zeros(gif_ref.BINS, dtype=np.uint32)
    h300[rng.choice(gif_ref.BINS, 300, replace=False)] = 7            # equal counts: the tie rules decide
    out["300_equal_bins"] = h300
    return out


HISTOGRAMS = _histograms()


@pytest.mark.parametrize("colors", [2, 16, 255, 256])
@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_median_cut_equals_restatement(gsdd, name, colors):
    hist = HISTOGRAMS[name]
    box, n = gsdd.ops.gif_median_cut(hist, colors)
    want, n_want = gif_ref.median_cut(hist, colors)
    assert n == n_want == min(colors, int(np.count_nonzero(hist)))
    assert np.array_equal(box, want)
    assert np.all(box[hist == 0] == 255) and set(box[hist != 0].tolist()) == set(range(n))


def test_median_cut_rejects_bad_colors(gsdd):
    hist = HISTOGRAMS["256_bins"]
    for bad in (1, 0, 257, -3):
        with pytest.raises(gsdd.GsddError):
            gsdd.ops.gif_median_cut(hist, bad)
    L = gsdd.lib()
    box = np.zeros(gif_ref.BINS, dtype=np.uint8)
    import ctypes as C
    n = C.c_int(0)
    for bad in (1, 257):
        assert L.gsdd_gif_median_cut(C.c_void_p(hist.ctypes.data), bad, C.c_void_p(box.ctypes.data), C.byref(n)) == -1
    assert L.gsdd_gif_median_cut(None, 16, C.c_void_p(box.ctypes.data), C.byref(n)) == -1


# ---------------------------------------------------------------------------------------------- encoder
def _random_palette(rng, n):
    pal = np.zeros((256, 3), dtype=np.uint8)
    colours = rng.permutation(1 << 24)[:n]                              # distinct colours: a decoded pixel names its index
    pal[:n] = np.stack([colours & 255, (colours >> 8) & 255, colours >> 16], axis=1)
    return pal


def _decode(data):
    im = Image.open(io.BytesIO(data))
    frames = []
    for t in range(getattr(im, "n_frames", 1)):
        im.seek(t)
        frames.append((np.asarray(im.convert("RGB")).copy(), im.info.get("duration")))
    return im, frames


def _check_round_trip(gsdd, idx, pal, n, delay=7, loop=3):
    data, clears = gsdd.ops.gif_encode(idx, pal, n, delay, loop)
    assert data[:6] == b"GIF89a" and data[-1:] == b";"
    im, frames = _decode(data)
    T, H, W = idx.shape
    assert len(frames) == T and im.size == (W, H) and im.info["loop"] == loop
    for t, (rgb, duration) in enumerate(frames):
        assert duration == 10 * delay
        assert np.array_equal(rgb, pal[t if pal.shape[0] > 1 else 0][idx[t]]), f"frame {t}"
    return data, clears


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 8, 8), (2, 17, 23)])
def test_encoder_round_trip_shapes(gsdd, shape):
    rng = np.random.default_rng(sum(shape))
    pal = _random_palette(rng, 37)[None]
    idx = rng.integers(0, 37, shape).astype(np.uint8)
    _check_round_trip(gsdd, idx, pal, np.array([37], dtype=np.int32))


def test_encoder_single_colour_frame_is_small(gsdd):
    pal = _random_palette(np.random.default_rng(2), 1)[None]
    idx = np.zeros((1, 64, 64), dtype=np.uint8)
    data, clears = _check_round_trip(gsdd, idx, pal, np.array([1], dtype=np.int32))
    assert len(data) < 256 and clears == 1                  # ~60 bytes of container and ~90 codes of at most 9 bits


def test_encoder_emits_a_mid_stream_clear(gsdd):
    rng = np.random.default_rng(3)
    pal = _random_palette(rng, 256)[None]
    idx = rng.integers(0, 256, (1, 96, 96)).astype(np.uint8)   # ~9216 codes: the 4096-entry table fills at least once
    _, clears = _check_round_trip(gsdd, idx, pal, np.array([256], dtype=np.int32))
    assert clears >= 2


def test_encoder_local_tables(gsdd):
    rng = np.random.default_rng(4)
    counts = np.array([2, 5, 256], dtype=np.int32)
    pal = np.stack([_random_palette(rng, int(c)) for c in counts])
    idx = np.stack([rng.integers(0, int(c), (19, 21)) for c in counts]).astype(np.uint8)
    _check_round_trip(gsdd, idx, pal, counts)


def test_encoder_respects_cap(gsdd):
    rng = np.random.default_rng(5)
    pal = _random_palette(rng, 200)[None]
    idx = rng.integers(0, 200, (2, 17, 23)).astype(np.uint8)
    n = np.array([200], dtype=np.int32)
    data, _ = gsdd.ops.gif_encode(idx, pal, n, 20, 0)
    again, _ = gsdd.ops.gif_encode(idx, pal, n, 20, 0, cap=len(data))       # exactly enough
    assert again == data
    assert len(data) <= gsdd.lib().gsdd_gif_encode_bound(2, 17, 23)
    # one byte short: the error code, and the byte behind the buffer (and every byte of a canary tail) untouched
    import ctypes as C
    cap = len(data) - 1
    buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)                              # noqa: E731
    rc = gsdd.lib().gsdd_gif_encode(p(idx), 2, 17, 23, p(pal), p(n), 1, 20, 0, p(buf), cap, None)
    assert rc == -4 and np.all(buf[cap:] == 0xA5)
    assert bytes(buf[:cap]) == data[:cap]
    with pytest.raises(gsdd.GsddError):
        gsdd.ops.gif_encode(idx, pal, n, 20, 0, cap=cap)
    # an index outside its table, a colour count outside 1 .. 256, a palette count that is neither 1 nor T
    with pytest.raises(gsdd.GsddError):
        gsdd.ops.gif_encode(idx, pal, np.array([100], dtype=np.int32), 20, 0)
    for bad in (0, 257):
        with pytest.raises(gsdd.GsddError):
            gsdd.ops.gif_encode(np.zeros_like(idx), pal, np.array([bad], dtype=np.int32), 20, 0)
    with pytest.raises(gsdd.GsddError):
        gsdd.ops.gif_encode(np.zeros((3, 4, 4), dtype=np.uint8), np.zeros((2, 256, 3), dtype=np.uint8), np.array([2, 2], dtype=np.int32), 20)


def test_encode_gif_delay_rounding(gsdd):
    idx = np.zeros((2, 4, 4), dtype=np.uint8)
    pal = _random_palette(np.random.default_rng(6), 2)
    for fps, delay in ((5, 20), (8, 12), (30, 3), (1000 / 15, 2)):
        assert gsdd.gif.delay_centiseconds(fps) == delay
        _, frames = _decode(gsdd.gif.encode_gif(torch.from_numpy(idx), torch.from_numpy(pal), 2, fps=fps))
        assert [d for _, d in frames] == [10 * delay] * 2
    for bad in (250, 0, -1):                                 # 100 / 250 rounds to 0
        with pytest.raises(gsdd.GsddError):
            gsdd.gif.encode_gif(idx, pal, 2, fps=bad)


# ---------------------------------------------------------------------------------------------- the restatement against PIL's median cut
@pytest.mark.parametrize("colors", [256, 64, 16])
@pytest.mark.parametrize("noise", [False, True])
def test_restatement_is_no_worse_than_pil_median_cut(noise, colors):
    levels = gif_ref.synthetic_levels(noise)
    idx, pal, n = gif_ref.quantize(gif_ref.clips_from_levels(levels), colors)
    assert np.array_equal(gif_ref.levels_of(gif_ref.clips_from_levels(levels)), levels)
    assert 1 <= n[0] <= colors and idx.max() < n[0]
    ours = gif_ref.psnr(gif_ref.reconstruct(idx, pal), levels)
    tall = Image.fromarray(levels[0].reshape(4 * 32, 32, 3), "RGB")                 # the clip as one tall image
    q = tall.quantize(colors, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
    pil = gif_ref.psnr(np.asarray(q.convert("RGB")).reshape(levels[0].shape), levels[0])
    print(f"[gif] noise={noise} colors={colors}: restatement {ours:.2f} dB, PIL median cut {pil:.2f} dB")
    assert ours >= pil


def test_bayer_matrix_is_a_permutation():
    y, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    m = gif_ref.bayer(x, y)
    assert sorted(m.ravel().tolist()) == list(range(64)) and m[0, 0] == 0
    off = gif_ref.dither_offsets(16, 24, 64)
    assert off.min() == -32 and off.max() == 31 and np.array_equal(off[:8, :8], off[8:, 16:])
    assert not gif_ref.dither_offsets(8, 8, 0).any()


# ---------------------------------------------------------------------------------------------- wrappers
def test_wrappers_fail_loudly(gsdd):
    ops, E = gsdd.ops, gsdd.GsddError
    clips = torch.zeros((1, 3, 2, 8, 8))
    pal = torch.zeros((1, 256, 4), dtype=torch.uint8)
    n = torch.ones(1, dtype=torch.int32)
    box = torch.zeros((1, 32768), dtype=torch.uint8)
    for call in (lambda c: ops.gif_histogram(c), lambda c: ops.gif_box_sums(c, box), lambda c: ops.gif_map(c, pal, n),
                 lambda c: gsdd.gif.quantize_clips(c), lambda c: gsdd.gif.write_gifs(c, ["x.gif"])):
        with pytest.raises(E):
            call(clips)                                                         # a CPU tensor
        with pytest.raises(E):
            call(clips.double())                                                # not fp32
        with pytest.raises(E):
            call(clips[0])                                                      # 4-D
    with pytest.raises(E, match="dither"):
        ops.gif_map(clips, pal, n, dither=65)                                   # (checked ahead of the device check)
    with pytest.raises(E, match="dither"):
        gsdd.gif.quantize_clips(clips, dither=65)
    with pytest.raises(E, match="colors"):
        gsdd.gif.quantize_clips(clips, colors=1)
    with pytest.raises(E, match="palette"):
        gsdd.gif.quantize_clips(clips, palette="video")


def test_symbols_version_and_documentation(gsdd):
    L = gsdd.lib()
    names = ["gsdd_gif_histogram", "gsdd_gif_box_sums", "gsdd_gif_map", "gsdd_gif_median_cut", "gsdd_gif_encode_bound", "gsdd_gif_encode"]
    assert L.gsdd_version() >= 111
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in names:
        assert hasattr(L, name) and name in gsdd.EXPORTS and name in doc, name
    assert L.gsdd_abi_sizeof(6) == -1 and L.gsdd_abi_sizeof(9) == -1             # no descriptor struct was added
    # device entries reject bad arguments before any launch (no GPU is touched)
    one = 0x1000
    assert L.gsdd_gif_histogram(None, 1, 1, 8, 8, 0, one, None) == -1
    assert L.gsdd_gif_histogram(one, 1, 1, 8, 65536, 0, one, None) == -1
    assert L.gsdd_gif_histogram(one, 0, 1, 8, 8, 0, one, None) == -1
    assert L.gsdd_gif_histogram(one, 1, 2, 4096, 4096, 0, one, None) == -1          # 2^25 pixels in a group
    assert L.gsdd_gif_box_sums(one, 1, 1, 8, 8, 0, None, one, None) == -1
    assert L.gsdd_gif_map(one, 1, 1, 8, 8, 0, one, one, 65, one, None) == -1
    assert L.gsdd_gif_map(one, 1, 1, 8, 8, 0, one, one, -1, one, None) == -1
    assert L.gsdd_gif_map(one, 1, 1, 8, 8, 2, one, one, 0, one, None) == -1
