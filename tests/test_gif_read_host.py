"""Host half of the GIF import (csrc/gif_read_host.hpp behind gsdd_gif_probe / gsdd_gif_decode), without a GPU: the library's decoder
against the numpy restatement (tests/gif_read_ref.py) on builder-made files, on the project's own writer's output and on PIL-written
files; every malformed case; every prefix of a small file; the raster capacity.  Every comparison is an equality."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import gif_read_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAP = -1, -4


@pytest.fixture(scope="module")
def gsdd():
    import gsdd_amd
    if "GSDD_LIB_PATH" not in os.environ:                 # incremental: a no-op when the library is newer than its sources
        subprocess.check_call(["bash", os.path.join(REPO, "build.sh")], cwd=REPO, stdout=subprocess.DEVNULL)
    gsdd_amd.lib()
    return gsdd_amd


def _palette(rng, n):
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _files():
    rng = np.random.default_rng(5)
    out = {}
    for m in range(1, 9):                                  # every minimum code size, with a table of 2^m entries
        out[f"min_code_{m}"] = ref.build_gif(13, 11, [dict(indices=rng.integers(0, 1 << m, (11, 13)), min_code=m)],
                                             global_palette=_palette(rng, 1 << m))
    out["one_colour_64x64"] = ref.build_gif(64, 64, [dict(indices=np.full((64, 64), 3))], global_palette=_palette(rng, 5))
    noise = rng.integers(0, 256, (96, 96))
    pal256 = _palette(rng, 256)
    for mode in ("full", "deferred"):
        out[f"noise_96x96_clear_{mode}"] = ref.build_gif(96, 96, [dict(indices=noise, clear=mode)], global_palette=pal256)
    small = rng.integers(0, 7, (30, 40))
    for n in (1, 255, (3, 200, 1, 17)):
        out[f"sub_blocks_{n}"] = ref.build_gif(40, 30, [dict(indices=small, sub_block=n)], global_palette=_palette(rng, 7))
    for h in (1, 2, 3, 4, 5, 8, 9, 17):
        out[f"interlaced_h{h}"] = ref.build_gif(9, 20, [dict(indices=rng.integers(0, 16, (h, 7)), x=2, y=1, interlace=True)],
                                                global_palette=_palette(rng, 16))
    out["canvas_1x1"] = ref.build_gif(1, 1, [dict(indices=[[1]])], global_palette=_palette(rng, 2))
    out["local_2_beside_global_256"] = ref.build_gif(
        8, 6, [dict(indices=rng.integers(0, 256, (6, 8))), dict(indices=rng.integers(0, 2, (3, 4)), x=4, y=3, palette=_palette(rng, 2)),
               dict(indices=rng.integers(0, 256, (2, 2)), x=1, y=1, delay=7)], global_palette=pal256, loop=3)
    out["no_trailer"] = ref.build_gif(6, 5, [dict(indices=rng.integers(0, 4, (5, 6)), delay=2)], global_palette=_palette(rng, 4),
                                      trailer=False)
    out["local_tables_only_87a"] = ref.build_gif(5, 4, [dict(indices=rng.integers(0, 3, (4, 5)), palette=_palette(rng, 3)),
                                                        dict(indices=rng.integers(0, 9, (2, 3)), x=2, y=2, palette=_palette(rng, 9))],
                                                 version=b"87a")
    out["animation"] = ref.build_gif(
        12, 10, [dict(indices=rng.integers(0, 8, (10, 12)), disposal=1, delay=10),
                 dict(indices=rng.integers(0, 8, (4, 5)), x=7, y=6, disposal=2, transparent=3, delay=65535),
                 dict(indices=rng.integers(0, 8, (3, 3)), x=0, y=0, disposal=3, delay=0, interlace=True),
                 dict(indices=rng.integers(0, 8, (1, 12)), x=0, y=9, disposal=5, transparent=0)],       # (disposal 5 is stored as 0)
        global_palette=_palette(rng, 8), loop=0)
    return out


FILES = _files()


def _same(got, want):
    frames, delays, palettes, raster, info = got
    assert np.array_equal(frames, want["frames"]) and frames.dtype == np.int32
    assert np.array_equal(delays, want["delays"])
    assert np.array_equal(palettes, want["palettes"])
    assert np.array_equal(raster, want["raster"])
    assert (info["width"], info["height"], info["loop"], info["global_table"]) == \
        (want["width"], want["height"], want["loop"], want["global_table"])
    # the probe (what `info` is) agrees with the decode
    assert info["frames"] == len(frames) and info["palettes"] == len(palettes) and info["raster_bytes"] == raster.size
    assert info["raster_bytes"] == int((frames[:, 2].astype(np.int64) * frames[:, 3]).sum())


@pytest.mark.parametrize("name", sorted(FILES))
def test_decode_equals_restatement(gsdd, name):
    _same(gsdd.ops.gif_decode(FILES[name]), ref.decode(FILES[name]))


def test_builder_files_are_what_they_claim():
    """the deferred-clear file really holds a full table without a second clear code, the other one a second clear code; the version,
    the stored disposal and the loop count come through"""
    assert FILES["noise_96x96_clear_full"] != FILES["noise_96x96_clear_deferred"]
    px = np.random.default_rng(5).integers(0, 256, 9216)
    full, deferred = {}, {}
    ref.lzw_encode(px, 8, "full", full), ref.lzw_encode(px, 8, "deferred", deferred)
    assert full["clears"] >= 2 and full["codes_at_full_table"] == 0
    assert deferred["clears"] == 1 and deferred["codes_at_full_table"] > 1000
    a = ref.decode(FILES["animation"])
    assert a["frames"][:, 7].tolist() == [1, 2, 3, 0] and a["frames"][:, 6].tolist() == [-1, 3, -1, 0] and a["loop"] == 0
    assert a["delays"].tolist() == [10, 65535, 0, 0]
    assert ref.decode(FILES["no_trailer"])["loop"] == -1 and FILES["no_trailer"][-1] == 0


def test_probe_fields(gsdd):
    info = gsdd.gif.probe_gif(FILES["local_2_beside_global_256"])
    assert info == dict(width=8, height=6, frames=3, palettes=2, raster_bytes=48 + 12 + 4, loop=3, global_table=1, version=89)
    info = gsdd.gif.probe_gif(FILES["local_tables_only_87a"])
    assert info["version"] == 87 and info["global_table"] == 0 and info["palettes"] == 2 and info["loop"] == -1


@pytest.mark.parametrize("palette", ["clip", "frame"])
def test_own_writer_decodes_to_what_went_in(gsdd, palette):
    rng = np.random.default_rng(11)
    T, H, W = 3, 21, 34
    n = np.array([200] if palette == "clip" else [2, 37, 256], dtype=np.int32)
    pal = np.zeros((len(n), 256, 3), dtype=np.uint8)
    for p, c in enumerate(n):
        pal[p, :c] = rng.integers(0, 256, (c, 3))
    idx = np.stack([rng.integers(0, n[t if palette == "frame" else 0], (H, W)) for t in range(T)]).astype(np.uint8)
    data, _ = gsdd.ops.gif_encode(idx, pal, n, delay_cs=20, loop=0)
    frames, delays, palettes, raster, info = gsdd.ops.gif_decode(data)
    assert np.array_equal(raster.reshape(T, H, W), idx)
    assert np.array_equal(palettes[:, :, :3], pal) and not palettes[:, :, 3].any()
    assert frames.tolist() == [[0, 0, W, H, t * H * W, t if palette == "frame" else 0, -1, 1] for t in range(T)]
    assert delays.tolist() == [20] * T and info["loop"] == 0 and info["global_table"] == (palette == "clip")
    _same((frames, delays, palettes, raster, info), ref.decode(data))


def _pil_rasters(data):
    """per frame the rectangle and the raw indices as PIL's own LZW decoder gives them.  Written against PIL 12.2: `im.tile` entries
    (codec, extents, offset, (bits, interlace, transparency)), `Image._getdecoder` and `decoder.setimage` are PIL internals, so a
    failure in here after a PIL upgrade is this helper's, not the library's."""
    im = Image.open(io.BytesIO(data))
    out = []
    for f in range(im.n_frames):
        im.seek(f)
        _, (x0, y0, x1, y1), offset, (bits, interlace, _) = im.tile[0]
        plane = Image.new("P", im.size, 0)
        decoder = Image._getdecoder("P", "gif", (bits, interlace, -1))
        decoder.setimage(plane.im, (x0, y0, x1, y1))
        decoder.decode(data[offset:])
        out.append(((x0, y0, x1 - x0, y1 - y0), np.asarray(plane)[y0:y1, x0:x1]))
        im.load()
    return out


def _pil_clip(seed, T=6, H=32, W=40):
    """palette images that share one palette: a static textured background with a small moving square, so that optimize=True crops
    every later frame to the rectangle that changed"""
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, (72, 3)).astype(np.uint8)
    clip = np.repeat(rng.integers(0, 64, (1, H, W)), T, axis=0).astype(np.uint8)
    for t in range(T):
        clip[t, 3 + 2 * t:9 + 2 * t, 5 + 4 * t:12 + 4 * t] = 64 + t
    imgs = []
    for f in clip:
        im = Image.fromarray(f, "P")
        im.putpalette(palette.tobytes())
        imgs.append(im)
    return imgs


def _pil_file(seed, **kw):
    imgs = _pil_clip(seed)
    buf = io.BytesIO()
    imgs[0].save(buf, format="GIF", save_all=True, append_images=imgs[1:], optimize=True, duration=40, loop=0, **kw)
    return buf.getvalue(), len(imgs)


@pytest.mark.parametrize("seed", [1, 2])
def test_pil_written_files_decode_to_pils_rasters(gsdd, seed):
    data, T = _pil_file(seed)
    frames, delays, palettes, raster, info = gsdd.ops.gif_decode(data)
    want = _pil_rasters(data)
    assert info["frames"] == len(want) == T
    assert any(tuple(f[2:4]) != (info["width"], info["height"]) for f in frames.tolist())       # sub-rectangles do occur
    for f, (rect, idx) in zip(frames.tolist(), want):
        assert tuple(f[:4]) == rect
        assert np.array_equal(raster[f[4]:f[4] + f[2] * f[3]].reshape(f[3], f[2]), idx)
    assert delays.tolist() == [4] * T
    _same((frames, delays, palettes, raster, info), ref.decode(data))


# ---------------------------------------------------------------------------------------------- malformed input
def _codes(codes, width):
    acc = nbits = 0
    out = bytearray()
    for c in codes:
        acc |= c << nbits
        nbits += width
    while nbits > 0:
        out.append(acc & 255)
        acc >>= 8
        nbits -= 8
    return bytes(out)


def _with_stream(codes, w=3, h=2):
    """a 3 x 2 image whose LZW stream is the given 3-bit codes (minimum code size 2: clear = 4, end = 5, first free entry 6)"""
    head = ref.build_gif(w, h, [], global_palette=np.zeros((4, 3)), trailer=False)
    return head + b"\x2C" + bytes([0, 0, 0, 0, w, 0, h, 0, 0, 2]) + ref.sub_blocks(_codes(codes, 3)) + b"\x3B"


BASE = ref.build_gif(3, 2, [dict(indices=[[0, 1, 2], [3, 2, 1]])], global_palette=np.arange(12).reshape(4, 3))
DESC = 13 + 12                                              # the image descriptor's 0x2C: behind the header and a 4-entry table


def _patched(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


MALFORMED = {
    "bad_signature": b"GIX89a" + BASE[6:],
    "not_a_gif": b"\x89PNG\r\n\x1a\n" + bytes(32),
    "empty": b"",
    "rectangle_leaves_canvas_x": _patched(BASE, DESC + 1, 1),
    "rectangle_leaves_canvas_y": _patched(BASE, DESC + 3, 1),
    "zero_width": _patched(BASE, DESC + 5, 0),
    "zero_height": _patched(BASE, DESC + 7, 0),
    "no_frames_trailer": BASE[:DESC] + b"\x3B",
    "no_frames_no_trailer": BASE[:DESC],
    "no_frames_only_extensions": BASE[:DESC] + b"\x21\xF9\x04\x00\x00\x00\x00\x00" + b"\x3B",
    "min_code_0": _patched(BASE, DESC + 10, 0),
    "min_code_9": _patched(BASE, DESC + 10, 9),
    "code_above_next_free": _with_stream([4, 0, 7, 5]),
    "first_code_not_a_literal": _with_stream([4, 6, 5]),
    "first_code_after_second_clear_not_a_literal": _with_stream([4, 0, 4, 7, 5]),
    "ends_before_all_pixels_end_code": _with_stream([4, 0, 1, 5]),
    "ends_before_all_pixels_chain": _with_stream([4, 0, 1]),
    "chain_cut_in_block": BASE[:-4],
    "chain_cut_before_terminator": BASE[:-2],
    "extension_cut": BASE[:DESC] + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01",
    "unknown_block": BASE[:DESC] + b"\x07" + BASE[DESC:],
    "no_colour_table": b"GIF89a\x03\x00\x02\x00\x70\x00\x00" + BASE[DESC:],
}


def test_malformed_cases_are_what_they_claim():
    assert ref.decode(BASE)["raster"].tolist() == [0, 1, 2, 3, 2, 1] and BASE[DESC] == 0x2C and BASE[DESC + 10] == 2
    # (3-bit codes throughout: a clear code before the table's eighth entry would widen them)
    assert ref.decode(_with_stream([4, 0, 1, 4, 2, 3, 4, 2, 1, 5]))["raster"].tolist() == [0, 1, 2, 3, 2, 1]
    assert ref.decode(_with_stream([4, 0, 6, 7, 5]))["raster"].tolist() == [0, 0, 0, 0, 0, 0]        # KwKwK twice: 1 + 2 + 3 pixels
    assert ref.decode(_with_stream([4, 0, 6, 7, 5], w=5, h=1))["raster"].tolist() == [0, 0, 0, 0, 0]  # ... a pixel too many: dropped
    for name, data in MALFORMED.items():
        with pytest.raises(ref.GifError):
            ref.decode(data)


@pytest.mark.parametrize("codes,w,h", [([4, 0, 1, 4, 2, 3, 4, 2, 1, 5], 3, 2), ([4, 0, 6, 7, 5], 3, 2), ([4, 0, 6, 7, 5], 5, 1),
                                       ([4, 0, 6, 7], 3, 2), ([4, 4, 3, 4, 4, 2, 5], 2, 1)],
                         ids=["clears", "kwkwk_twice", "a_pixel_too_many", "no_end_code", "repeated_clears"])
def test_hand_packed_streams(gsdd, codes, w, h):
    data = _with_stream(codes, w, h)
    _same(gsdd.ops.gif_decode(data), ref.decode(data))


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_input_is_an_argument_error(gsdd, name):
    data = np.frombuffer(MALFORMED[name], dtype=np.uint8).copy()          # an exact-size copy
    L = gsdd.lib()
    info = np.zeros(8, dtype=np.int64)
    frames, delays = np.zeros((8, 8), dtype=np.int32), np.zeros(8, dtype=np.int32)
    palettes, raster = np.zeros((8, 256, 4), dtype=np.uint8), np.zeros(4096, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc_probe = L.gsdd_gif_probe(p(data), data.size, p(info))
    rc = L.gsdd_gif_decode(p(data), data.size, p(frames), p(delays), p(palettes), p(raster), raster.size)
    assert rc == E_ARG and rc_probe in (0, E_ARG)
    assert b"gsdd_gif_decode" in L.gsdd_last_error() and b" at byte " in L.gsdd_last_error()
    lzw_only = name in ("code_above_next_free", "first_code_not_a_literal", "first_code_after_second_clear_not_a_literal",
                        "ends_before_all_pixels_end_code", "ends_before_all_pixels_chain")
    assert rc_probe == (0 if lzw_only else E_ARG)                         # the probe walks the blocks only
    with pytest.raises(gsdd.GsddError, match="at byte"):
        gsdd.ops.gif_decode(MALFORMED[name])
    if not lzw_only:
        with pytest.raises(gsdd.GsddError, match="probe_gif: <bytes>: .* at byte"):
            gsdd.gif.probe_gif(MALFORMED[name])


def test_error_names_the_offset(gsdd):
    with pytest.raises(gsdd.GsddError, match=r"bad signature\) at byte 0$"):
        gsdd.ops.gif_probe(MALFORMED["bad_signature"])
    with pytest.raises(gsdd.GsddError, match=rf"leaves the canvas at byte {DESC}$"):
        gsdd.ops.gif_probe(MALFORMED["rectangle_leaves_canvas_x"])
    with pytest.raises(gsdd.GsddError, match=rf"minimum code size outside 1 \.\. 8 at byte {DESC + 10}$"):
        gsdd.ops.gif_probe(MALFORMED["min_code_9"])
    with pytest.raises(gsdd.GsddError, match=r"no frames at byte 25$"):
        gsdd.ops.gif_probe(MALFORMED["no_frames_no_trailer"])
    L = gsdd.lib()
    assert L.gsdd_gif_probe(None, 0, None) == E_ARG
    assert L.gsdd_gif_decode(None, 0, None, None, None, None, 0) == E_ARG


@pytest.mark.parametrize("name", ["animation", "local_2_beside_global_256", "min_code_1"])
def test_every_prefix_is_an_error_or_a_valid_shorter_result(gsdd, name):
    """... and exactly the restatement's verdict and result, at every length"""
    data = FILES[name]
    valid = 0
    for n in range(len(data) + 1):
        prefix = np.frombuffer(data[:n], dtype=np.uint8).copy()
        try:
            want = ref.decode(data[:n])
        except ref.GifError:
            want = None
        try:
            got = gsdd.ops.gif_decode(prefix)
        except gsdd.GsddError as e:
            assert "gsdd error -1" in str(e), (n, e)
            got = None
        assert (got is None) == (want is None), n
        if got is not None:
            _same(got, want)
            valid += 1
    assert valid >= 2                                       # with and without the trailer, at the least


def test_raster_capacity(gsdd):
    data = FILES["local_2_beside_global_256"]
    total = gsdd.ops.gif_probe(data)["raster_bytes"]
    for cap in (total - 1, 48, 47, 0):                      # (ops.gif_decode checks its guard byte behind the buffer)
        with pytest.raises(gsdd.GsddError, match="gsdd error -4"):
            gsdd.ops.gif_decode(data, raster_cap=cap)
    L = gsdd.lib()
    d = np.frombuffer(data, dtype=np.uint8).copy()
    frames, delays = np.zeros((3, 8), dtype=np.int32), np.zeros(3, dtype=np.int32)
    palettes, raster = np.zeros((2, 256, 4), dtype=np.uint8), np.full(total + 8, 0xA5, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.gsdd_gif_decode(p(d), d.size, p(frames), p(delays), p(palettes), p(raster), total - 1) == E_CAP
    assert np.all(raster[total - 1:] == 0xA5)
    assert L.gsdd_gif_decode(p(d), d.size, p(frames), p(delays), p(palettes), p(raster), total) == 0
    assert np.all(raster[total:] == 0xA5) and np.array_equal(raster[:total], ref.decode(data)["raster"])


def test_abi(gsdd):
    L = gsdd.lib()
    assert L.gsdd_version() >= 112
    assert {"gsdd_gif_probe", "gsdd_gif_decode", "gsdd_gif_compose"} <= set(gsdd.EXPORTS)
    assert L.gsdd_abi_sizeof(6) == -1                       # plain integer tables: no new struct


def test_read_gif_needs_a_device(gsdd):
    with pytest.raises(gsdd.GsddError, match="no CPU fallback"):
        gsdd.gif.read_gif(FILES["animation"], "cpu")
    with pytest.raises(gsdd.GsddError, match="cannot read"):
        gsdd.gif.probe_gif(os.path.join(REPO, "tests", "no_such_file.gif"))
