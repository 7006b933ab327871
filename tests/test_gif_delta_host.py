"""Host half of the GIF export's delta stage (gif::encode_delta of csrc/gif_host.hpp behind gsdd_gif_encode_delta), without a GPU: the
delta of the numpy restatement (tests/gif_delta_ref.py) goes into the library's encoder and the file is decoded three ways -- by PIL, by
the reader's restatement (gif_read_ref.decode + compose) and by the library's own decoder (gsdd_gif_decode, then compose) -- which must
all show the restatement's displayed frames.  Every comparison is an equality."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import gif_delta_ref as ref
import gif_read_ref
import gif_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gsdd():
    import gsdd_amd
    if "GSDD_LIB_PATH" not in os.environ:                 # incremental: a no-op when the library is newer than its sources
        subprocess.check_call(["bash", os.path.join(REPO, "build.sh")], cwd=REPO, stdout=subprocess.DEVNULL)
    gsdd_amd.lib()
    return gsdd_amd


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _three_ways(gsdd, data):
    """-> the frames (T, H, W, 3) PIL shows, the reader's restatement shows, and the library's decoder + the restatement's compositor"""
    im = Image.open(io.BytesIO(data))
    pil = []
    for t in range(getattr(im, "n_frames", 1)):
        im.seek(t)
        pil.append(np.asarray(im.convert("RGB")).copy())
    d = gif_read_ref.decode(data)
    F = len(d["frames"])
    restated = gif_read_ref.compose(d["raster"], d["frames"], d["palettes"], d["width"], d["height"], list(range(F)))
    table, _, palettes, raster, info = gsdd.ops.gif_decode(data)
    assert np.array_equal(table, d["frames"]) and np.array_equal(raster, d["raster"]) and np.array_equal(palettes, d["palettes"])
    own = gif_read_ref.compose(raster, table, palettes, info["width"], info["height"], list(range(info["frames"])))
    return np.stack(pil), restated, own


def _clip(T_frames, H, W, n, local, seed):
    """colour ids with structure: frame 1 repeats frame 0 (nothing changes), frames 2 .. 5 change one corner each (top left, top right,
    bottom left, bottom right), frame 6 changes a random third of the pixels -> (indices (T, H, W), palettes (1 or T, 256, 3), n_colors).
    With local tables every frame's table is another permutation of the same colours: equal colours behind different indices."""
    rng = np.random.default_rng(seed)
    colours = rng.permutation(1 << 24)[:n]
    colours = np.stack([colours & 255, (colours >> 8) & 255, colours >> 16], axis=1).astype(np.uint8)
    cid = np.empty((T_frames, H, W), dtype=np.int64)
    cid[0] = rng.integers(0, n, (H, W))
    cid[1] = cid[0]
    for t, (y, x) in zip(range(2, 6), ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        cid[t] = cid[t - 1]
        cid[t, y, x] = (cid[t, y, x] + 1) % n
    cid[6] = np.where(rng.random((H, W)) < 1 / 3, rng.integers(0, n, (H, W)), cid[5])
    if not local:
        pal = np.zeros((1, 256, 3), dtype=np.uint8)
        pal[0, :n] = colours
        return cid.astype(np.uint8), pal, np.array([n], dtype=np.int32)
    pal = np.zeros((T_frames, 256, 3), dtype=np.uint8)
    idx = np.empty_like(cid)
    for t in range(T_frames):
        perm = rng.permutation(n)
        pal[t, perm] = colours
        idx[t] = perm[cid[t]]
    return idx.astype(np.uint8), pal, np.full(T_frames, n, dtype=np.int32)


@pytest.mark.parametrize("hw", [(1, 1), (5, 3), (32, 32)])
@pytest.mark.parametrize("n", [1, 2, 255, 256])
@pytest.mark.parametrize("local", [False, True])
def test_delta_file_decodes_to_the_displayed_frames(gsdd, local, n, hw):
    H, W = hw
    idx, pal, nc = _clip(7, H, W, n, local, seed=H * 1000 + n + local)
    want = gif_ref.reconstruct(idx[None], pal, per_frame=local)[0]                      # palette[indices]
    out, rects, changed, transparent, displayed = ref.delta(want[None], idx[None], pal, nc, per_frame=local, tolerance=0)
    assert np.array_equal(displayed[0], want)                                           # tolerance 0: the unoptimised frames
    assert np.array_equal(ref.decode_displayed(out[0], rects[0], pal, transparent, local), want)
    assert rects[0, 0].tolist() == [0, 0, W - 1, H - 1] and changed[0, 0] == H * W
    assert rects[0, 1].tolist() == [W, H, -1, -1] and changed[0, 1] == 0                # the all-unchanged frame
    if n > 1:
        corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        assert [tuple(r[:2]) for r in rects[0, 2:6].tolist()] == corners and changed[0, 2:6].tolist() == [1] * 4
    assert transparent.tolist() == ([-1] if n == 256 else [n]) * len(nc)
    assert n == 256 or np.count_nonzero(out[0] == n) == int(H * W * 7 - changed[0].sum())
    data, clears = gsdd.ops.gif_encode_delta(out[0], pal, nc, rects[0], transparent, 7, 3)
    assert data[:6] == b"GIF89a" and data[-1:] == b";" and clears == 7
    assert len(data) <= gsdd.lib().gsdd_gif_encode_bound(7, H, W)
    for name, got in zip(("PIL", "gif_read_ref", "gsdd_gif_decode"), _three_ways(gsdd, data)):
        assert got.shape == want.shape and np.array_equal(got, want), name
    # the container: every image descriptor carries its rectangle, every control extension the transparent index, disposal 1
    d = gif_read_ref.decode(data)
    boxes = np.where(rects[0][:, 2:3] < 0, np.array([[0, 0, 1, 1]]), np.concatenate([rects[0][:, :2], rects[0][:, 2:] - rects[0][:, :2] + 1], 1))
    assert np.array_equal(d["frames"][:, :4], boxes) and d["frames"][:, 7].tolist() == [1] * 7 and d["delays"].tolist() == [7] * 7
    assert d["frames"][:, 6].tolist() == [int(transparent[t if local else 0]) for t in range(7)] and d["loop"] == 3
    again = gsdd.gif.encode_gif(torch.from_numpy(out[0]), torch.from_numpy(pal if local else pal[0]), torch.from_numpy(nc),
                                fps=100 / 7, loop=3, rects=torch.from_numpy(rects[0]), transparent=torch.from_numpy(transparent))
    assert again == data


def _square(noise, colors=255):
    levels = ref.moving_square_levels(noise=noise)
    clips = gif_ref.clips_from_levels(levels)
    assert np.array_equal(gif_ref.levels_of(clips), levels)
    idx, pal, n = gif_ref.quantize(clips, colors)
    return levels, idx, pal, n


def test_moving_square_file_is_smaller(gsdd):
    levels, idx, pal, n = _square(0)
    plain, _ = gsdd.ops.gif_encode(idx[0], pal, n, 20, 0)
    out, rects, changed, transparent, displayed = ref.delta(levels, idx, pal, n)
    data, _ = gsdd.ops.gif_encode_delta(out[0], pal, n, rects[0], transparent, 20, 0)
    print(f"[gif delta] 8 x 32 x 32, moving 8 x 8 square: {len(plain)} -> {len(data)} bytes, ratio {len(data) / len(plain):.3f}")
    assert len(data) < len(plain)
    assert all(np.array_equal(got, displayed[0]) for got in _three_ways(gsdd, data))
    assert np.array_equal(displayed, gif_ref.reconstruct(idx, pal))


@pytest.mark.parametrize("tolerance", [1, 48, 768])
def test_tolerance_keeps_every_pixel_within_it(gsdd, tolerance):
    levels, idx, pal, n = _square(2)
    exact = gif_ref.reconstruct(idx, pal)
    out, rects, changed, transparent, displayed = ref.delta(levels, idx, pal, n, tolerance=tolerance)
    d2 = ((displayed.astype(np.int64) - levels.astype(np.int64)) ** 2).sum(-1)
    assert np.all(np.all(displayed == exact, axis=-1) | (d2 <= tolerance))
    none = ref.delta(levels, idx, pal, n)[2]
    # two noisy levels of the still background are at most 4 apart a channel, 48 in all: from there on the tolerance keeps pixels
    # the exact form repaints
    assert tolerance < 48 or changed.sum() < none.sum()
    data, _ = gsdd.ops.gif_encode_delta(out[0], pal, n, rects[0], transparent, 20, 0)
    print(f"[gif delta] tolerance {tolerance}: {int(changed.sum())} of {int(none.sum())} changed pixels, {len(data)} bytes")
    for name, got in zip(("PIL", "gif_read_ref", "gsdd_gif_decode"), _three_ways(gsdd, data)):
        assert np.array_equal(got, displayed[0]), name


def test_whole_frames_without_transparency_are_encode_s_bytes(gsdd):
    """gsdd_gif_encode writes what it wrote (the reader tests' builder restates its container byte for byte), and gsdd_gif_encode_delta
    with whole-frame rectangles and no transparent index writes the same"""
    for local in (False, True):
        idx, pal, nc = _clip(7, 17, 23, 37, local, seed=5)
        data, _ = gsdd.ops.gif_encode(idx, pal, nc, 20, 2)
        frames = [dict(indices=idx[t], disposal=1, delay=20, palette=pal[t, :37] if local else None) for t in range(7)]
        assert data == gif_read_ref.build_gif(23, 17, frames, None if local else pal[0, :37], loop=2)
        whole = np.tile(np.array([0, 0, 22, 16], dtype=np.int32), (7, 1))
        assert gsdd.ops.gif_encode_delta(idx, pal, nc, whole, np.full(len(nc), -1, dtype=np.int32), 20, 2)[0] == data


def test_encoder_respects_cap_and_rejects_bad_arguments(gsdd):
    L = gsdd.lib()
    levels, idx, pal, n = _square(0, colors=16)
    out, rects, _, transparent, _ = ref.delta(levels, idx, pal, n)
    out, rects = np.ascontiguousarray(out[0]), np.ascontiguousarray(rects[0])
    T, H, W = out.shape
    data, _ = gsdd.ops.gif_encode_delta(out, pal, n, rects, transparent, 20, 0)
    assert gsdd.ops.gif_encode_delta(out, pal, n, rects, transparent, 20, 0, cap=len(data))[0] == data
    cap = len(data) - 1
    buf = np.full(cap + 64, 0xA5, dtype=np.uint8)

    def call(indices=out, T=T, pal=pal, n=n, npal=1, rects=rects, tr=transparent, delay=20, loop=0, out_buf=buf, cap=cap):
        ptr = lambda a: None if a is None else _p(a)                                    # noqa: E731
        return L.gsdd_gif_encode_delta(ptr(indices), T, H, W, ptr(pal), ptr(n), npal, ptr(rects), ptr(tr), delay, loop, ptr(out_buf), cap, None)
    assert call() == -4 and np.all(buf[cap:] == 0xA5) and bytes(buf[:cap]) == data[:cap]
    assert call(cap=0) == -4 and np.all(buf[cap:] == 0xA5)
    assert call(cap=len(data)) == len(data) and bytes(buf[:len(data)]) == data
    with pytest.raises(gsdd.GsddError):
        gsdd.ops.gif_encode_delta(out, pal, n, rects, transparent, 20, 0, cap=cap)
    big = np.empty(L.gsdd_gif_encode_bound(T, H, W), dtype=np.uint8)

    def rect(t, *r):
        bad = rects.copy()
        bad[t] = r
        return bad
    i32 = lambda *v: np.array(v, dtype=np.int32)                                        # noqa: E731
    for name, kwargs in (("leaves the canvas right", dict(rects=rect(1, 0, 0, W, 0))), ("leaves the canvas below", dict(rects=rect(1, 0, 0, 0, H))),
                         ("negative corner", dict(rects=rect(2, -1, 0, 3, 3))), ("inverted x", dict(rects=rect(2, 5, 0, 4, 3))),
                         ("inverted y", dict(rects=rect(2, 0, 5, 3, 4))), ("half an empty marker", dict(rects=rect(3, W, H, -1, 0))),
                         ("transparent 256", dict(tr=i32(256))), ("transparent -2", dict(tr=i32(-2))),
                         ("an index beyond its table", dict(n=i32(int(n[0]) - 1), tr=i32(255))),
                         ("n_colors 0", dict(n=i32(0))), ("n_colors 257", dict(n=i32(257))), ("two palettes", dict(npal=2)),
                         ("delay", dict(delay=65536)), ("loop", dict(loop=-1)), ("no frames", dict(T=0)), ("negative cap", dict(cap=-1)),
                         ("null indices", dict(indices=None)), ("null palettes", dict(pal=None)), ("null n_colors", dict(n=None)),
                         ("null rects", dict(rects=None)), ("null transparent", dict(tr=None)), ("null out", dict(out_buf=None))):
        kwargs.setdefault("out_buf", big)
        kwargs.setdefault("cap", big.size)
        assert call(**kwargs) == -1, name
        assert "gsdd_gif_encode_delta" in L.gsdd_last_error().decode()
    # an index beyond the table OUTSIDE its frame's rectangle is not read, let alone written
    stray = out.copy()
    assert rects[1].tolist() != [0, 0, W - 1, H - 1]
    stray[1, H - 1, W - 1] = 200
    assert call(indices=stray, out_buf=big, cap=big.size) == len(data) and bytes(big[:len(data)]) == data
    for bad in (dict(rects=rects[:3]), dict(transparent=np.array([1, 2], dtype=np.int32))):
        args = dict(rects=rects, transparent=transparent)
        args.update(bad)
        with pytest.raises(gsdd.GsddError):
            gsdd.ops.gif_encode_delta(out, pal, n, args["rects"], args["transparent"], 20, 0)
    with pytest.raises(gsdd.GsddError, match="rects and transparent"):
        gsdd.gif.encode_gif(out, pal[0], n, rects=rects)


def test_wrappers_fail_loudly(gsdd):
    E = gsdd.GsddError
    clips = torch.zeros((1, 3, 2, 8, 8))
    idx = torch.zeros((1, 2, 8, 8), dtype=torch.uint8)
    pal = torch.zeros((1, 256, 4), dtype=torch.uint8)
    n = torch.ones(1, dtype=torch.int32)
    for call in (lambda c: gsdd.ops.gif_delta(c, idx, pal, n), lambda c: gsdd.gif.delta_frames(c, idx, pal[..., :3], n),
                 lambda c: gsdd.gif.write_gifs(c, ["x.gif"], optimize=True)):
        with pytest.raises(E):
            call(clips)                                                         # a CPU tensor: no CPU fallback
        with pytest.raises(E):
            call(clips.double())
    for bad in (-1, 195076, 1.5, True):
        with pytest.raises(E, match="tolerance"):
            gsdd.ops.gif_delta(clips, idx, pal, n, tolerance=bad)               # (checked ahead of the device check)
    with pytest.raises(E, match="tolerance needs optimize"):
        gsdd.gif.write_gifs(clips, ["x.gif"], tolerance=48)
    with pytest.raises(E, match="palette_mode"):
        gsdd.gif.delta_frames(clips, idx, pal, n, palette_mode="video")


def test_symbols_version_and_documentation(gsdd):
    L = gsdd.lib()
    assert L.gsdd_version() >= 114
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in ("gsdd_gif_delta", "gsdd_gif_encode_delta"):
        assert hasattr(L, name) and name in gsdd.EXPORTS and name in doc, name
    # the device entry rejects bad arguments before any launch (no GPU is touched)
    one = 0x1000
    ok = [one, one, 1, 1, 8, 8, 0, one, one, 0, one + 64, one, one, None]
    for i, bad in ((0, None), (1, None), (7, None), (8, None), (10, None), (11, None), (12, None), (7, one + 2), (9, -1), (9, 195076),
                   (10, one), (6, 2), (2, 0), (4, 65536), (5, 65536)):
        args = list(ok)
        args[i] = bad
        assert L.gsdd_gif_delta(*args) == -1, (i, bad)
    assert L.gsdd_gif_delta(one, one, 1, 2, 4096, 4096, 0, one, one, 0, one + 64, one, one, None) == -1      # 2^25 pixels in a group
