"""`datamodule=tgif` as users reach it, without a GPU: the README's command line composes (configs/train.yaml through hydra_lite, for
both model configs, which interpolate ${datamodule.*} keys) and `cfg.datamodule` instantiates; the caption key; the windows; and the
dataset's host side -- file list, probes, captions -- which is built once per split."""
import os
import subprocess

import numpy as np
import pytest

import gif_read_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gsdd_amd():
    import gsdd_amd
    if "GSDD_LIB_PATH" not in os.environ:                 # incremental: a no-op when the library is newer than its sources
        subprocess.check_call(["bash", os.path.join(REPO, "build.sh")], cwd=REPO, stdout=subprocess.DEVNULL)
    gsdd_amd.lib()
    return gsdd_amd


@pytest.mark.parametrize("model", ["discrete_diffusion", "videogpt_vq_vae"])
def test_readme_command_line_composes_and_instantiates(model, monkeypatch, tmp_path):
    import src  # noqa: F401
    from gsdd_amd.hydra_lite import compose, instantiate
    monkeypatch.setenv("PROJECT_ROOT", REPO)
    tsv = tmp_path / "tgif-v1.0.tsv"
    tsv.write_text("https://38.media.tumblr.com/abc.gif\ta man waves\n")
    cfg = compose(os.path.join(REPO, "configs"), "train.yaml",
                  [f"model={model}", "datamodule=tgif", f"datamodule.data_folder={tmp_path}", f"datamodule.captions={tsv}"])
    assert cfg.datamodule._target_ == "src.datamodules.gif_folder_datamodule.GifFolderDataModule"
    assert cfg.model.collate_fn == cfg.datamodule.collate_fn == "ucf101_collate"
    assert cfg.datamodule.sequence_length == 16 and cfg.datamodule.resolution == 128 and cfg.datamodule.short == "pad_last"
    dm = instantiate(cfg.datamodule)
    assert type(dm).__name__ == "GifFolderDataModule" and dm.sequence_length == 16 and dm.batch_size == cfg.batch_size
    assert dm.args["captions"] == str(tsv) and dm.args["frame_stride"] == 1 and dm.args["frames_between_clips"] == 100
    # without overrides: no captions file, the folder under paths.datasets
    plain = compose(os.path.join(REPO, "configs"), "train.yaml", [f"model={model}", "datamodule=tgif"])
    assert instantiate(plain.datamodule).args["captions"] is None and plain.datamodule.data_folder.endswith(os.path.join("data", "TGIF"))


def test_clip_key():
    from src.datamodules.gif_folder_datamodule import clip_key
    assert clip_key("https://38.media.tumblr.com/tumblr_abc123_250.gif\n") == "tumblr_abc123_250"
    assert clip_key("  tumblr_abc123_250.gif ") == clip_key("tumblr_abc123_250") == clip_key("/data/TGIF/train/x/tumblr_abc123_250.gif")
    assert clip_key("a.gif.v2.gif") == "a.gif.v2" and clip_key("gift") == "gift" and clip_key("dir.gif/name") == "name"


def test_windows():
    from src.datamodules.gif_folder_datamodule import window_frames
    assert window_frames(16, 16, 1, 100, "skip") == [list(range(16))] and window_frames(15, 16, 1, 100, "skip") == []
    assert window_frames(15, 16, 1, 100, "pad_last") == [list(range(15)) + [14]]
    assert window_frames(250, 16, 1, 100, "skip") == [list(range(s, s + 16)) for s in (0, 100, 200)]
    assert window_frames(9, 3, 4, 100, "skip") == [[0, 4, 8]] and window_frames(8, 3, 4, 100, "pad_last") == [[0, 4, 4]]
    assert window_frames(1, 4, 2, 1, "pad_last") == [[0, 0, 0, 0]]


def test_dataset_host_side_is_built_once_per_split(gsdd_amd, tmp_path, monkeypatch):
    from src.datamodules.gif_folder_datamodule import GifFolderDataModule
    rng = np.random.default_rng(0)
    for cls, name, F in (("walk", "a", 6), ("wave", "b", 2)):
        path = tmp_path / "train" / cls / f"{name}.gif"
        path.parent.mkdir(parents=True)
        path.write_bytes(ref.build_gif(5, 4, [dict(indices=rng.integers(0, 4, (4, 5)), delay=1) for _ in range(F)],
                                       global_palette=rng.integers(0, 256, (4, 3))))
    tsv = tmp_path / "c.tsv"
    tsv.write_text("http://x/a.gif\tone\nb\ttwo\n")
    probes = []
    real = gsdd_amd.gif.probe_gif
    monkeypatch.setattr(gsdd_amd.gif, "probe_gif", lambda p: probes.append(p) or real(p))
    dm = GifFolderDataModule(str(tmp_path), sequence_length=4, resolution=8, batch_size=2, frames_between_clips=2, captions=str(tsv))
    ds = dm.dataset("train")
    assert [(os.path.basename(f), frames, n) for f, frames, n in ds.clips] == \
        [("a.gif", [0, 1, 2, 3], 4), ("a.gif", [2, 3, 4, 5], 4), ("b.gif", [0, 1, 1, 1], 2)]
    assert ds.classes == ["walk", "wave"] and ds.captions == {"a": "one", "b": "two"} and len(probes) == 2
    assert dm.dataset("train") is ds and len(probes) == 2                 # a second epoch does not read the folder again
    (tmp_path / "train" / "wave" / "c.gif").write_bytes(b"GIF89a")
    with pytest.raises(KeyError, match="c.gif"):
        GifFolderDataModule(str(tmp_path), sequence_length=4, captions=str(tsv)).dataset("train")
    with pytest.raises(RuntimeError, match="c.gif"):
        GifFolderDataModule(str(tmp_path), sequence_length=4).dataset("train")
