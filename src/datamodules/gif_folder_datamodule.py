"""Folder-of-GIFs datamodule: a working counterpart of the reference's TGIF dataset (src/datamodules/datasets/tgif-dataset.py, which is
not imported there, needs gulpio2 / pycocotools / nltk and whose video transform returns None).  The files are read as they are: the
library's host code decodes the LZW streams, the device composites the frames and resizes them (gsdd_amd.gif.read_gif ->
gsdd_amd.data.preprocess); no PIL, no .npy step.

    <data_folder>/<split>/**/<name>.gif

* text: with `captions` -- a TSV of `<url or name>\\t<sentence>[\\t...]`, the TGIF release's layout -- the sentence whose key equals
  the file's name (clip_key below: the last path component without its ".gif" -- for TGIF's names the key the reference's
  get_uid_tgif forms, tgif-dataset.py:27-28); a file without a sentence is an error.  Without `captions` the parent directory's name, as in the clip-folder dataset.  label = the index
  of the parent directory among the sorted directory names, either way.
* clips: windows of `sequence_length` frames, `frame_stride` apart, a new window every `frames_between_clips` frames.  A file too
  short for one window gives one clip padded with its last sampled frame (the reference's rule, tgif-dataset.py:125-131) with
  short="pad_last", none with short="skip".  Frame counts come from probe_gif (the block structure only, nothing is decoded).
* batches: canvas sizes differ per file, so items are preprocessed one at a time and stacked.  The batch dict, the sharding (set_shard,
  set_epoch, whole rounds of full batches) and ShardedLoader are the clip-folder module's.  `orig_length` is the number of frames of
  the window that are not padding.  A split's dataset (the file list, the probes, the windows) is built once and kept: an epoch
  does not read the folder again.  Decoded clips are not kept."""
import glob
import os
import posixpath

import torch

from src.datamodules.clip_folder_datamodule import ClipFolderDataModule


def clip_key(url_or_path):
    """The key a clip goes by in the captions file and on disk: the last component of a URL or path, without a closing ".gif".  For
    TGIF's URLs and file names this is the key the reference's get_uid_tgif forms.  Kept from it: surrounding white space is
    dropped, only "/" separates components (callers pass paths with os.sep replaced).  Not kept: a ".gif" INSIDE the name stays
    ("a.gif.v2.gif" -> "a.gif.v2", where the reference deletes every occurrence); both sides of the lookup use this function, so
    such a file still finds its sentence."""
    name = posixpath.basename(url_or_path.strip())
    return name[:-4] if name.endswith(".gif") else name


def read_captions(path):
    """TSV of <url or name> TAB <sentence> [TAB ...] -> {clip_key: sentence}"""
    out = {}
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            cols = line.rstrip("\n").split("\t")
            if len(cols) < 2:
                raise ValueError(f"{path}:{n}: expected <url or name> TAB <sentence>")
            out[clip_key(cols[0])] = cols[1].strip()
    return out


def window_frames(n_frames, sequence_length, frame_stride, frames_between_clips, short):
    """the frame numbers of every window of a file of n_frames frames"""
    span = (sequence_length - 1) * frame_stride + 1
    if n_frames >= span:
        return [list(range(s, s + span, frame_stride)) for s in range(0, n_frames - span + 1, frames_between_clips)]
    if short == "skip":
        return []
    real = list(range(0, n_frames, frame_stride))
    return [real + [real[-1]] * (sequence_length - len(real))]


class GifFolderDataset:
    def __init__(self, data_folder, sequence_length, split="train", resolution=64, frame_stride=1, frames_between_clips=100,
                 short="pad_last", captions=None, device="cuda"):
        from gsdd_amd.gif import probe_gif
        if short not in ("pad_last", "skip"):
            raise ValueError(f'short is "pad_last" or "skip", got {short!r}')
        if sequence_length < 1 or frame_stride < 1 or frames_between_clips < 1:
            raise ValueError("sequence_length, frame_stride and frames_between_clips are at least 1")
        self.sequence_length, self.resolution, self.device = sequence_length, resolution, device
        files = sorted(glob.glob(os.path.join(data_folder, split, "**", "*.gif"), recursive=True))
        self.classes = sorted(set(self._parent(f) for f in files))
        self.class_to_label = {c: i for i, c in enumerate(self.classes)}
        self.captions = None if captions is None else read_captions(captions)
        self.clips = []                                   # (file, frame numbers, frames that are not padding)
        for f in files:
            if self.captions is not None and clip_key(f.replace(os.sep, "/")) not in self.captions:
                raise KeyError(f"{f}: no sentence for {clip_key(f.replace(os.sep, '/'))!r} in {captions}")
            n = self._named(f, probe_gif, f)["frames"]
            for frames in window_frames(n, sequence_length, frame_stride, frames_between_clips, short):
                self.clips.append((f, frames, len(set(frames))))

    @staticmethod
    def _parent(f):
        return os.path.basename(os.path.dirname(f))

    @staticmethod
    def _named(path, fn, *args, **kw):
        """a file that does not decode is an error naming the path"""
        try:
            return fn(*args, **kw)
        except Exception as e:
            raise RuntimeError(f"{path}: {e}") from e

    @property
    def n_classes(self):
        return len(self.classes)

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, idx):
        from gsdd_amd.gif import read_gif
        f, frames, real = self.clips[idx]
        video, _, _ = self._named(f, read_gif, f, self.device, frames=frames)
        name = self._parent(f)
        text = name if self.captions is None else self.captions[clip_key(f.replace(os.sep, "/"))]
        return dict(frames=video, label=self.class_to_label[name], text=text, orig_length=real)


class GifFolderDataModule(ClipFolderDataModule):
    def __init__(self, data_folder, sequence_length=16, resolution=128, batch_size=16, frame_stride=1, frames_between_clips=100,
                 short="pad_last", captions=None, device="cuda", shuffle_seed=0, **reference_keys):
        # (reference_keys: dataname, num_workers, collate_fn, ... of the reference's datamodule configs; nothing here reads them)
        super().__init__(data_folder, sequence_length=sequence_length, resolution=resolution, batch_size=batch_size, device=device,
                         shuffle_seed=shuffle_seed, frame_stride=frame_stride, frames_between_clips=frames_between_clips, short=short,
                         captions=captions)
        self._datasets = {}                               # split -> GifFolderDataset: the folder is probed once, not once per epoch

    def dataset(self, split):
        if split not in self._datasets:
            self._datasets[split] = GifFolderDataset(split=split, device=self.device, **self.args)
        return self._datasets[split]

    def _batches(self, split, shuffle):
        # a copy of ClipFolderDataModule._batches' loop over another dataset (no .to(device): read_gif's frames are on the device);
        # the sharding rule is stated there, and the two must stay alike
        from gsdd_amd.data import preprocess
        ds = self.dataset(split)
        order = list(range(len(ds)))
        if shuffle:
            order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(self.shuffle_seed + self.epoch)).tolist()
        rank, world = self.shard
        nbatch = (len(order) + self.batch_size - 1) // self.batch_size if world == 1 else len(order) // self.batch_size
        for b in range(rank, (nbatch // world) * world, world):                          # (whole rounds: ClipFolderDataModule._batches)
            i = b * self.batch_size
            items = [ds[j] for j in order[i:i + self.batch_size]]
            video = torch.stack([preprocess(it["frames"], self.resolution) for it in items])     # (B,3,T,R,R)
            yield {"video": video, "text": [it["text"] for it in items], "length": [video.shape[1]] * len(items),
                   "label": torch.tensor([it["label"] for it in items]), "frame": torch.zeros(len(items), 1000),
                   "orig_length": [it["orig_length"] for it in items]}
