"""The GIF import on the GPU (csrc/gif_read.hip, gsdd_amd.gif.read_gif, src/datamodules/gif_folder_datamodule.py) against its numpy
restatement (tests/gif_read_ref.py).  Compositing is integer selection, so EVERY comparison is byte-for-byte equality.  Canvases: the
smallest that take every path of the kernel -- one pixel, fewer pixels than a thread owns, one row, a multiple of the four pixels a
thread owns (64 x 64: dword stores in every slot), and 97 x 61 = 5917 pixels: odd, so every other output slot starts off a dword
boundary and is written bytewise, one pixel in the ragged tail, and 1480 threads = six workgroups of 256."""
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageSequence

import gif_read_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
CANVASES = [(1, 1), (5, 3), (63, 1), (64, 64), (97, 61)]            # (W, H)
KINDS = ["full", "one", "left", "top", "right", "bottom", "overlap", "disjoint"]


@pytest.fixture(scope="module")
def G():
    import gsdd_amd
    assert torch.cuda.is_available()
    gsdd_amd.lib()
    return gsdd_amd


def _span(rng, n):
    """a random interval [a, a + l) inside [0, n)"""
    l = int(rng.integers(1, n + 1))
    return int(rng.integers(0, n - l + 1)), l


def _rect(kind, W, H, prev, rng):
    (x, w), (y, h) = _span(rng, W), _span(rng, H)
    if kind == "full":
        return 0, 0, W, H
    if kind == "one":
        return x, y, 1, 1
    if kind == "left":
        return 0, y, w, h
    if kind == "top":
        return x, 0, w, h
    if kind == "right":
        return W - w, y, w, h
    if kind == "bottom":
        return x, H - h, w, h
    px, py, pw, ph = prev
    if kind == "overlap":                                           # holds a pixel of the predecessor
        cx, cy = px + int(rng.integers(0, pw)), py + int(rng.integers(0, ph))
        x0, y0 = int(rng.integers(0, cx + 1)), int(rng.integers(0, cy + 1))
        return x0, y0, int(rng.integers(cx, W)) - x0 + 1, int(rng.integers(cy, H)) - y0 + 1
    for lo, hi, axis in ((0, px, 0), (px + pw, W, 0), (0, py, 1), (py + ph, H, 1)):      # disjoint: beside, above or below it
        if hi > lo:
            a, l = _span(rng, hi - lo)
            return (lo + a, y, l, h) if axis == 0 else (x, lo + a, w, l)
    return x, y, w, h                                               # (the predecessor covers the canvas: nothing is disjoint)


def scene(W, H, F, seed, disposals=None, transparency=True, kinds=None):
    """tables as gsdd_gif_decode writes them: three colour tables of 256, 16 and 2 entries (zeros behind a table's size; indices that
    lie behind it occur), rectangles of every kind in turn, random disposals, a transparent index on every other frame"""
    rng = np.random.default_rng(seed)
    sizes = [256, 16, 2]
    palettes = np.zeros((3, 256, 4), dtype=np.uint8)
    for p, n in enumerate(sizes):
        palettes[p, :n, :3] = rng.integers(1, 256, (n, 3))
    frames, rasters, off, prev = [], [], 0, None
    for f in range(F):
        kind = (kinds or KINDS)[f % len(kinds or KINDS)]
        x, y, w, h = _rect(kind, W, H, prev, rng) if f else (0, 0, W, H)
        row = f % 3
        idx = rng.integers(0, sizes[row], (h, w))
        idx[rng.random((h, w)) < 0.1] = 255 - f % 7                 # behind the 16- and the 2-entry table: (0, 0, 0)
        transparent = -1
        if transparency and f % 2:
            transparent = int(idx[0, 0])
            idx[rng.random((h, w)) < 0.3] = transparent
        disposal = int(rng.integers(0, 4)) if disposals is None else disposals[f]
        frames.append([x, y, w, h, off, row, transparent, disposal])
        rasters.append(idx.reshape(-1).astype(np.uint8))
        off += w * h
        prev = (x, y, w, h)
    return dict(W=W, H=H, frames=np.array(frames, dtype=np.int32), palettes=palettes, raster=np.concatenate(rasters))


def run(G, s, select, matte=(0, 0, 0)):
    dev = torch.device("cuda")
    out = G.ops.gif_compose(torch.from_numpy(s["raster"]).to(dev), torch.from_numpy(s["frames"]).to(dev),
                            torch.from_numpy(s["palettes"]).to(dev), s["W"], s["H"], select, matte)
    return out.cpu().numpy()


def want(s, select, matte=(0, 0, 0)):
    return ref.compose(s["raster"], s["frames"], s["palettes"], s["W"], s["H"], list(select), matte)


def test_launch_covers_several_workgroups():
    with open(os.path.join(REPO, "gif-synthesis-with-discrete-diffusion_amd", "csrc", "gif_read.hip")) as f:
        threads, pix = (int(v) for v in re.search(r"constexpr int GIFR_THREADS = (\d+), GIFR_PIX = (\d+);", f.read()).groups())
    W, H = CANVASES[-1]
    owners = (W * H + pix - 1) // pix                               # threads that own pixels
    assert (W * H) % pix != 0 and (W * H) % 2 == 1 and (owners + threads - 1) // threads >= 2
    assert (64 * 64) % pix == 0 and 5 * 3 > pix > 1 * 1


@pytest.mark.parametrize("F", [1, 2, 7, 40])
@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_compose_equals_restatement(G, canvas, F):
    s = scene(*canvas, F, seed=F + canvas[0])
    matte = (0, 0, 0) if F % 2 else (250, 3, 128)
    select = list(range(F))
    got, exp = run(G, s, select, matte), want(s, select, matte)
    assert got.shape == (F, canvas[1], canvas[0], 3) and got.dtype == np.uint8
    assert np.array_equal(got, exp)
    if F == 40 and canvas == CANVASES[-1]:                          # what the scene claims to hold
        fr = s["frames"]
        assert set(fr[:, 7].tolist()) == {0, 1, 2, 3} and (fr[:, 6] >= 0).any() and (fr[:, 6] < 0).any()
        assert (fr[:, 0] == 0).any() and (fr[:, 1] == 0).any() and (fr[:, 0] + fr[:, 2] == 97).any() and (fr[:, 1] + fr[:, 3] == 61).any()
        assert ((fr[:, 2] == 1) & (fr[:, 3] == 1)).any() and ((fr[:, 2] == 97) & (fr[:, 3] == 61)).sum() >= 5
        apart = lambda a, b: a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]
        assert all(not apart(fr[f], fr[f - 1]) for f in range(6, 40, 8)) and any(apart(fr[f], fr[f - 1]) for f in range(7, 40, 8))
        assert (s["raster"] > 16).any() and (exp == 0).all(axis=-1).any()


@pytest.mark.parametrize("transparency", [False, True], ids=["opaque", "transparent"])
@pytest.mark.parametrize("d1", range(4))
@pytest.mark.parametrize("d0", range(4))
def test_every_pair_of_disposals(G, d0, d1, transparency):
    """frames 0 and 1 carry the pair, frame 2 shows what frame 1's disposal left behind; partial rectangles that overlap"""
    s = scene(9, 7, 3, seed=4 * d0 + d1, disposals=[d0, d1, 0], transparency=transparency, kinds=["full", "overlap", "overlap"])
    s["frames"][0, :4] = (1, 1, 6, 5)                               # the first frame leaves a border of matte
    assert np.array_equal(run(G, s, [0, 1, 2], (9, 200, 77)), want(s, [0, 1, 2], (9, 200, 77)))


def _small(disposals, rects, transparent=None, seed=3):
    rng = np.random.default_rng(seed)
    palettes = np.zeros((1, 256, 4), dtype=np.uint8)
    palettes[0, :, :3] = rng.integers(1, 256, (256, 3))
    frames, rasters, off = [], [], 0
    for f, ((x, y, w, h), d) in enumerate(zip(rects, disposals)):
        t = -1 if transparent is None else transparent[f]
        idx = rng.integers(1, 256, w * h).astype(np.uint8)
        if t == "all":
            t, idx = 0, np.zeros(w * h, dtype=np.uint8)
        frames.append([x, y, w, h, off, 0, t, d])
        rasters.append(idx)
        off += w * h
    return dict(W=8, H=6, frames=np.array(frames, dtype=np.int32), palettes=palettes, raster=np.concatenate(rasters))


def test_disposal_3_on_frame_0_restores_the_matte(G):
    s = _small([3, 1], [(1, 1, 5, 4), (6, 0, 2, 2)])
    got = run(G, s, [0, 1], (10, 20, 30))
    assert np.array_equal(got, want(s, [0, 1], (10, 20, 30)))
    assert (got[1, 1:5, 1:6] == (10, 20, 30)).all() and (got[0, 1:5, 1:6] != (10, 20, 30)).any()


def test_three_disposal_3_frames_in_a_row(G):
    s = _small([1, 3, 3, 3, 1], [(0, 0, 8, 6), (1, 1, 4, 3), (2, 2, 5, 3), (0, 3, 8, 3), (7, 5, 1, 1)])
    got = run(G, s, range(5))
    assert np.array_equal(got, want(s, range(5)))
    assert np.array_equal(got[4, :5], got[0, :5])                   # all three are gone again


def test_disposal_2_then_a_fully_transparent_frame(G):
    s = _small([1, 2, 1], [(0, 0, 8, 6), (2, 1, 4, 3), (0, 0, 8, 6)], transparent=[-1, -1, "all"])
    got = run(G, s, range(3), (1, 2, 3))
    assert np.array_equal(got, want(s, range(3), (1, 2, 3)))
    assert (got[2, 1:4, 2:6] == (1, 2, 3)).all() and np.array_equal(got[2, 4:], got[0, 4:])


SELECTS = {"all": list(range(7)), "first": [0], "last": [6], "every_third": [0, 3, 6], "last_repeated": [4, 5, 6, 6, 6, 6],
           "repeats_inside": [0, 0, 2, 2, 2, 5]}


@pytest.mark.parametrize("name", sorted(SELECTS))
def test_select(G, name):
    s = scene(97, 61, 7, seed=21)
    got = run(G, s, SELECTS[name], (7, 7, 70))
    assert np.array_equal(got, want(s, SELECTS[name], (7, 7, 70)))
    assert np.array_equal(got, want(s, range(7), (7, 7, 70))[SELECTS[name]])


def test_bad_arguments(G):
    import ctypes as C
    L, dev = G.lib(), torch.device("cuda")
    s = scene(5, 3, 2, seed=1)
    raster, frames, palettes = (torch.from_numpy(s[k]).to(dev) for k in ("raster", "frames", "palettes"))
    out = torch.full((3, 3, 5, 3), 0x5A, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(select, F=2, W=5, H=3, T=None, matte=0, ptrs=None):
        host = np.asarray(select, dtype=np.int32)
        sel = torch.from_numpy(host).to(dev)
        a = dict(raster=p(raster), frames=p(frames), palettes=p(palettes), select=p(sel), host=C.c_void_p(host.ctypes.data), out=p(out))
        a.update(ptrs or {})
        return L.gsdd_gif_compose(a["raster"], a["frames"], a["palettes"], F, W, H, a["select"], a["host"], len(host) if T is None else T,
                                  matte, a["out"], st)

    assert call([0, 1, 1]) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want(s, [0, 1, 1]))
    out.fill_(0x5A)
    for select in ([1, 0], [0, 1, 0], [-1, 0], [0, 2], [2]):
        assert call(select) == E_ARG, select
    assert b"gsdd_gif_compose" in L.gsdd_last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(W=-5), dict(T=0), dict(T=-1), dict(F=0), dict(matte=-1),
               dict(matte=1 << 24)):
        assert call([0, 1], **kw) == E_ARG, kw
    for name in ("raster", "frames", "palettes", "select", "host", "out"):
        assert call([0, 1], ptrs={name: None}) == E_ARG, name
    torch.cuda.synchronize()
    assert (out == 0x5A).all()                                      # nothing was launched
    for bad in ([1, 0], [0, 2], []):
        with pytest.raises(G.GsddError):
            G.ops.gif_compose(raster, frames, palettes, 5, 3, bad)
    for kw in (dict(matte=(0, 0, 256)), dict(matte=(0, 0)), dict(out=torch.empty((2, 3, 5, 4), dtype=torch.uint8, device=dev))):
        with pytest.raises(G.GsddError):
            G.ops.gif_compose(raster, frames, palettes, 5, 3, [0, 1], **kw)
    with pytest.raises(G.GsddError):
        G.ops.gif_compose(raster.cpu(), frames.cpu(), palettes.cpu(), 5, 3, [0, 1])
    with pytest.raises(G.GsddError):
        G.gif.read_gif(ref.build_gif(2, 2, [dict(indices=[[0, 1], [1, 0]])], global_palette=np.eye(3)), "cuda", frames=[1])


# ---------------------------------------------------------------------------------------------- files, end to end
def test_round_trip_of_the_projects_own_files(G, tmp_path):
    rng = np.random.default_rng(2)
    levels = rng.integers(0, 256, (2, 3, 20, 24, 3)).astype(np.uint8)            # B, T, H, W, RGB
    norm = ((levels.astype(np.float32) + 0.5) / 255.0 - np.float32([0.485, 0.456, 0.406])) / np.float32([0.229, 0.224, 0.225])
    clips = torch.from_numpy(np.ascontiguousarray(norm.transpose(0, 4, 1, 2, 3))).cuda()
    for mode in ("clip", "frame"):
        paths = [str(tmp_path / mode / f"{b}.gif") for b in range(2)]
        indices, palette, _ = G.gif.write_gifs(clips, paths, fps=10, palette=mode)
        idx, pal = indices.cpu().numpy().astype(np.int64), palette.cpu().numpy()
        for b, path in enumerate(paths):
            video, delays, info = G.gif.read_gif(path, "cuda")
            exp = np.stack([pal[b * 3 + t if mode == "frame" else b][idx[b, t]] for t in range(3)])
            assert np.array_equal(video.cpu().numpy(), exp)
            assert delays == [10] * 3 and (info["width"], info["height"], info["frames"], info["loop"]) == (24, 20, 3, 0)


def _pil_frames(data):
    return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


def _agreeing_file(seed, transparency):
    """the class every compositing rule agrees on: the first frame covers the canvas (and has no transparent pixel), disposals 0 / 1"""
    rng = np.random.default_rng(seed)
    W, H = 23, 17
    pal = rng.integers(0, 256, (32, 3))
    frames = [dict(indices=rng.integers(0, 32, (H, W)), disposal=1, delay=3)]
    for f in range(1, 6):
        (x, w), (y, h) = _span(rng, W), _span(rng, H)
        fr = dict(indices=rng.integers(0, 32, (h, w)), x=x, y=y, disposal=int(f % 2), delay=f, interlace=bool(f == 3))
        if transparency and f != 2:
            fr["transparent"] = int(rng.integers(0, 32))
            fr["indices"][rng.random((h, w)) < 0.4] = fr["transparent"]
        if f == 4:
            fr["palette"] = rng.integers(0, 256, (32, 3))
        frames.append(fr)
    return ref.build_gif(W, H, frames, global_palette=pal, loop=0)


@pytest.mark.parametrize("transparency", [False, True], ids=["opaque", "transparent"])
def test_pil_agrees_on_builder_files(G, transparency):
    data = _agreeing_file(5 + transparency, transparency)
    video, delays, _ = G.gif.read_gif(data, "cuda")
    d = ref.decode(data)
    assert np.array_equal(video.cpu().numpy(), ref.compose(d["raster"], d["frames"], d["palettes"], 23, 17, range(6)))
    assert np.array_equal(video.cpu().numpy(), _pil_frames(data))
    assert delays == [3, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("seed", [1, 2])
def test_pil_agrees_on_pil_written_files(G, seed):
    import test_gif_read_host as host
    data, T = host._pil_file(seed)
    info = G.gif.probe_gif(data)
    d = ref.decode(data)
    assert info["frames"] == T and set(d["frames"][:, 7].tolist()) <= {0, 1} and tuple(d["frames"][0, :4]) == (0, 0, 40, 32)
    video, _, _ = G.gif.read_gif(data, "cuda")
    assert np.array_equal(video.cpu().numpy(), _pil_frames(data))
    assert np.array_equal(video.cpu().numpy(), np.stack([np.asarray(im.convert("RGB")) for im in host._pil_clip(seed)]))


def test_index_behind_the_table_reads_black(G):
    idx = np.array([[0, 3, 4, 255], [200, 1, 2, 17]])
    data = ref.build_gif(4, 2, [dict(indices=idx, min_code=8)], global_palette=[[9, 9, 9], [1, 2, 3], [4, 5, 6], [7, 8, 9]])
    video, _, _ = G.gif.read_gif(data, "cuda", matte=(50, 60, 70))
    assert video.cpu().numpy()[0].tolist() == [[[9, 9, 9], [7, 8, 9], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [1, 2, 3], [4, 5, 6], [0, 0, 0]]]


# ---------------------------------------------------------------------------------------------- the datamodule
def _folder(tmp_path):
    """test/walk/{a (9 frames), a2 (5 frames)}.gif on a 20 x 14 canvas, test/wave/b.gif: 3 frames on 11 x 17 -- shorter than a window"""
    files = {}
    for k, (cls, name, (W, H), F) in enumerate([("walk", "a", (20, 14), 9), ("walk", "a2", (20, 14), 5), ("wave", "b", (11, 17), 3)]):
        s = scene(W, H, F, seed=30 + k)
        frames = []
        for f, (x, y, w, h, off, row, transparent, disposal) in enumerate(s["frames"].tolist()):
            fr = dict(indices=s["raster"][off:off + w * h].reshape(h, w), x=x, y=y, disposal=disposal, delay=f,
                      palette=s["palettes"][row, :[256, 16, 2][row], :3], min_code=8)
            if transparent >= 0:
                fr["transparent"] = transparent
            frames.append(fr)
        path = tmp_path / "data" / "test" / cls / f"{name}.gif"
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(ref.build_gif(W, H, frames, loop=0))
        files[name] = (str(path), s)
    tsv = tmp_path / "captions.tsv"
    tsv.write_text("https://38.media.tumblr.com/a.gif\ta dog walks\t9\nb.gif\tsomebody waves\na2\ta cat walks \n")
    return str(tmp_path / "data"), str(tsv), files


def test_gif_folder_datamodule(G, tmp_path):
    from gsdd_amd.data import preprocess
    from src.datamodules.clip_folder_datamodule import ShardedLoader
    from src.datamodules.gif_folder_datamodule import GifFolderDataModule, window_frames
    folder, tsv, files = _folder(tmp_path)
    kw = dict(sequence_length=4, resolution=8, batch_size=2, frames_between_clips=3, device="cuda")
    windows = [("a", [0, 1, 2, 3], 4, "a dog walks", 0), ("a", [3, 4, 5, 6], 4, "a dog walks", 0), ("a2", [0, 1, 2, 3], 4, "a cat walks", 0),
               ("b", [0, 1, 2, 2], 3, "somebody waves", 1)]
    assert window_frames(9, 4, 1, 3, "pad_last") == [[0, 1, 2, 3], [3, 4, 5, 6]] and window_frames(3, 4, 1, 3, "skip") == []
    assert window_frames(9, 3, 4, 100, "skip") == [[0, 4, 8]] and window_frames(6, 3, 4, 100, "pad_last") == [[0, 4, 4]]

    def expected(name, select):
        s = files[name][1]
        frames = ref.compose(s["raster"], s["frames"], s["palettes"], s["W"], s["H"], select)
        return preprocess(torch.from_numpy(frames).cuda(), 8)

    dm = GifFolderDataModule(folder, captions=tsv, **kw)
    loader = dm.test_dataloader()
    assert isinstance(loader, ShardedLoader) and loader.gsdd_sharded
    batches = list(loader)
    assert len(batches) == 2
    for b, batch in enumerate(batches):
        assert set(batch) == {"video", "text", "length", "label", "frame", "orig_length"}
        assert batch["video"].shape == (2, 3, 4, 8, 8) and batch["video"].dtype == torch.float32 and batch["video"].is_cuda
        assert batch["frame"].shape == (2, 1000) and batch["length"] == [3, 3]
        for i, (name, select, real, text, label) in enumerate(windows[2 * b:2 * b + 2]):
            assert torch.equal(batch["video"][i], expected(name, select)), (name, select)
            assert batch["text"][i] == text and int(batch["label"][i]) == label and batch["orig_length"][i] == real

    # the two shards of a data-parallel pair see the single-process batches
    for rank in (0, 1):
        dm.set_shard(rank, 2)
        mine = list(dm.test_dataloader())
        assert len(mine) == 1 and torch.equal(mine[0]["video"], batches[rank]["video"]) and mine[0]["text"] == batches[rank]["text"]

    # short="skip" drops the short file; without captions the text is the directory's name
    skip = list(GifFolderDataModule(folder, short="skip", **kw).test_dataloader())
    assert [b["video"].shape[0] for b in skip] == [2, 1] and sum((b["text"] for b in skip), []) == ["walk"] * 3
    assert torch.equal(skip[1]["video"][0], batches[1]["video"][0])
    plain = list(GifFolderDataModule(folder, **kw).test_dataloader())
    assert sum((b["text"] for b in plain), []) == ["walk", "walk", "walk", "wave"] and plain[1]["label"].tolist() == [0, 1]

    # a file that does not decode is an error naming the path; so is a file without a sentence
    broken = os.path.join(folder, "test", "wave", "broken.gif")
    with open(files["b"][0], "rb") as f:
        data = f.read()
    with open(broken, "wb") as f:
        f.write(data[:len(data) // 2])
    with pytest.raises(RuntimeError, match="broken.gif"):
        list(GifFolderDataModule(folder, **kw).test_dataloader())
    with open(broken, "wb") as f:
        f.write(data)
    with pytest.raises(KeyError, match="broken"):
        list(GifFolderDataModule(folder, captions=tsv, **kw).test_dataloader())
