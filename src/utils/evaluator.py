"""FVD (and, with a scorer, CLIPSIM) evaluator with the reference's interface (src/utils/evaluator.py:10-116): push_vals(batch,
batch_idx, outputs) -> evaluate_metrics(...) -> {'fvd': ...} -> reset().  The statistic is gsdd_amd.metrics.frechet_distance (pinned to values of the
reference's function, tests/golden/frechet.npz).  The feature extractor is the reference's Kinetics-400 I3D
(src/models/motionencoder/pytorch_i3d.py -> gsdd_amd/i3d.py: the same architecture and state_dict keys on the HIP conv path,
pinned to the reference module on seeded weights) fed with clips de-normalised, resized to 224 and scaled to [-1, 1]; its
pretrained weights cannot be obtained offline, so `checkpoint_paths` must point at a supplied state_dict (or `videoencoder` at
any other module mapping (B,3,T,H,W) clips to features).  Unlike the reference (which never leaves train mode here:
evaluator.py:14-29), the extractor runs in eval mode.

CLIPSIM (not in the reference; text-to-video work on MSR-VTT reports it next to FVD): with `clip_scorer` set, push_vals also scores the
sampled clips against `batch["text"]` -- the mean over frames of the cosine between the caption's CLIP text feature and each frame's
CLIP image feature (gsdd_amd.metrics.clip_similarity, unscaled) -- and evaluate_metrics returns {'fvd': ..., 'clipsim': ...}, the mean
over every sample pushed.  The image tower is gsdd_amd.vision.ClipVisionTower on the HIP kernels; its preprocessing is torch's bicubic
on the quantised frames, not the `clip` package's PIL resize.  Without a scorer nothing of this runs and the dict is {'fvd': ...}.

PSNR and SSIM (not in the reference; what reconstruction, prediction, interpolation and inpainting work reports per frame): with
`paired_metrics` on, push_vals also scores every frame of `outputs` against the same frame of `batch["video"]` on their uint8 levels
(gsdd_amd.metrics.paired_frame_metrics: one HIP kernel per push) and evaluate_metrics adds {'psnr': ..., 'ssim': ...}: the mean over
every sample pushed and over the frames `paired_from_frame` .. T - 1, so that the conditioning frames of a prediction run
(`sample_condition_frames=N paired_from_frame=N`) stay out of the scalar.  A frame identical to its target has a PSNR of inf, and so
has a mean that contains one.  frame_curves() gives the per-frame means over the samples, all T frames.  Off by default: nothing new
runs and the dict is what it was.

LPIPS (not in the reference; reported next to PSNR and SSIM): with `lpips_scorer` set -- a gsdd_amd.lpips.Lpips, e.g. from
`lpips_from_pretrained` -- push_vals also scores every frame of `outputs` against the same frame of `batch["video"]` (AlexNet or VGG-16
features and the learned distance heads on the HIP kernels; the weights are the user's to supply) and evaluate_metrics adds
{'lpips': ...}, the mean over every sample pushed and over the frames `paired_from_frame` .. T - 1; frame_curves() gains 'lpips'.  It
needs neither `paired_metrics` nor the other scorer.  Unscaled, >= 0, lower is closer.  Without a scorer nothing of this runs."""
import torch

from gsdd_amd.hydra_lite import instantiate
from gsdd_amd.metrics import clip_similarity, frechet_distance, paired_frame_metrics

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class MeanPoolEncoder(torch.nn.Module):
    """A weight-free stand-in feature extractor (NOT I3D: the numbers it yields are no FVD): per-channel means over a `grid`^3 partition
    of every clip, (B, 3, T, H, W) -> (B, 3 * grid^3).  Lets the evaluation plumbing (`model.do_evaluation=true`,
    `model.evaluator.videoencoder._target_=src.utils.evaluator.MeanPoolEncoder`) run where no I3D weights exist."""

    def __init__(self, grid=2, **kwargs):
        super().__init__()
        self.grid = grid
        self.register_buffer("_anchor", torch.zeros(1))

    def forward(self, clips):
        return torch.nn.functional.adaptive_avg_pool3d(clips.float(), self.grid).flatten(1)


class ClipSimScorer:
    """CLIPSIM of clips against their captions.  text_embedder: any callable mapping a list of B strings to (B, E) features (a
    `CLIPTextEmbedding(weights=<directory>)` is one); vision_tower: a gsdd_amd.vision.ClipVisionTower of the same CLIP model, on the
    device it is to run on.  __call__(texts, clips (B, 3, T, H, W), ImageNet-normalised as the decoder returns them) -> (B,) fp64 on
    the host."""

    def __init__(self, text_embedder, vision_tower):
        self.text_embedder, self.vision_tower = text_embedder, vision_tower

    @torch.no_grad()
    def __call__(self, texts, clips):
        text = self.text_embedder(list(texts))
        frames = self.vision_tower(clips)
        return clip_similarity(text.detach().cpu(), frames.detach().cpu())


def clip_scorer_from_pretrained(weights, device="cuda"):
    """A ClipSimScorer with both towers of one CLIP model, from a LOCAL directory in the Hugging Face layout (config.json,
    model.safetensors, vocab.json, merges.txt of e.g. `openai/clip-vit-base-patch32`).  Nothing is ever fetched: the directory must
    exist.  Usable as a `_target_` of configs/model/evaluator.yaml's `clip_scorer`."""
    import os
    from transformers import CLIPVisionModelWithProjection
    from gsdd_amd.vision import ClipVisionTower
    from src.models.text_models.clip_text_embedding import CLIPTextEmbedding
    if not os.path.isdir(weights):
        raise FileNotFoundError(f"clip_scorer_from_pretrained({weights!r}): not a directory; a local copy of the CLIP model is needed "
                                "-- nothing is downloaded")
    vm = CLIPVisionModelWithProjection.from_pretrained(weights, local_files_only=True).eval()
    vc = vm.config
    text = CLIPTextEmbedding(clip_dim=vc.projection_dim, weights=weights).to(device)
    tower = ClipVisionTower.from_hf_state_dict(vm.state_dict(), vc.num_attention_heads, eps=vc.layer_norm_eps,
                                               hidden_act=vc.hidden_act).to(device)
    return ClipSimScorer(text, tower)


def lpips_from_pretrained(weights, net="alex", device="cuda"):
    """A gsdd_amd.lpips.Lpips scorer from LOCAL weights: one file with a full `lpips.LPIPS(net=...)` state dict, or a directory with
    the lpips package's `<net>.pth` and torchvision's `alexnet.pth` / `vgg16.pth` (gsdd_amd.lpips.Lpips.from_pretrained).  Nothing is ever
    fetched.  Usable as a `_target_` of configs/model/evaluator.yaml's `lpips_scorer`."""
    from gsdd_amd.lpips import Lpips
    return Lpips.from_pretrained(weights, net).to(device)


class Evaluator:
    def __init__(self, device, videoencoder, checkpoint_paths=None, target_resolution=224, clip_scorer=None, paired_metrics=False,
                 paired_from_frame=0, lpips_scorer=None):
        self.device, self.target_resolution = device, target_resolution
        if not isinstance(paired_from_frame, int) or isinstance(paired_from_frame, bool) or paired_from_frame < 0:
            raise ValueError(f"Evaluator: paired_from_frame is a frame number >= 0, got {paired_from_frame!r}")
        self.paired_metrics, self.paired_from_frame = bool(paired_metrics), paired_from_frame
        if isinstance(clip_scorer, dict):
            clip_scorer = instantiate(clip_scorer, _recursive_=False)
        self.clip_scorer = clip_scorer
        if isinstance(lpips_scorer, dict):
            lpips_scorer = instantiate(lpips_scorer, _recursive_=False)
        self.lpips_scorer = lpips_scorer
        self.videoencoder = instantiate(videoencoder, _recursive_=False) if isinstance(videoencoder, dict) else videoencoder
        if checkpoint_paths and checkpoint_paths != "__None__":
            self.videoencoder.load_state_dict(torch.load(checkpoint_paths, map_location="cpu", weights_only=True))
        elif any(True for _ in self.videoencoder.parameters()):
            import warnings
            warnings.warn("Evaluator: no checkpoint for the video encoder (model.evaluator.checkpoint_paths / eval_ckpt): it runs on its "
                          "random initialisation, and the distance it yields is not an FVD", UserWarning)
        self.videoencoder.to(device).eval()
        self.reset()

    def reset(self):
        self.all_video_embeds_generated, self.all_video_embeds_gt = [], []
        self.all_clip_scores = []
        self.all_frame_psnr, self.all_frame_ssim = [], []
        self.all_frame_lpips = []

    def _prepare(self, clips):
        """evaluator.py:42-70: undo the ImageNet normalisation, quantise to uint8, preprocess at 224 (x2: [-1, 1]-ish range),
        repeat frames of 4- / 8-frame clips to 16."""
        from gsdd_amd.data import preprocess
        x = clips.detach().to(self.device).float().permute(0, 2, 3, 4, 1)                 # (B,T,H,W,3)
        x = x * torch.tensor(STD, device=x.device) + torch.tensor(MEAN, device=x.device)
        x = (x * 255).to(torch.uint8)                                                     # astype('uint8') truncation, as there
        out = torch.stack([preprocess(v.contiguous(), self.target_resolution) for v in x]) * 2
        if out.shape[2] in (4, 8):
            out = torch.repeat_interleave(out, 16 // out.shape[2], dim=2)
        return out

    @torch.no_grad()
    def push_vals(self, batch, batch_idx, outputs):
        self.all_video_embeds_generated.append(self.videoencoder(self._prepare(outputs)).float().cpu())
        self.all_video_embeds_gt.append(self.videoencoder(self._prepare(batch["video"])).float().cpu())
        if self.clip_scorer is not None:
            self.all_clip_scores.append(self.clip_scorer(batch["text"], outputs))
        if self.paired_metrics:
            got = paired_frame_metrics(self._levels_operand(outputs), self._levels_operand(batch["video"]))
            self.all_frame_psnr.append(got["psnr"])
            self.all_frame_ssim.append(got["ssim"])
        if self.lpips_scorer is not None:
            got = self.lpips_scorer(self._levels_operand(outputs), self._levels_operand(batch["video"]))
            self.all_frame_lpips.append(torch.as_tensor(got["lpips"]).to(torch.float64).cpu())

    def _levels_operand(self, clips):
        """clips as the kernel takes them: float32 (B, 3, T, H, W) (or uint8 frames as they are), contiguous, on the evaluator's device"""
        x = clips.detach().to(self.device)
        return (x if x.dtype == torch.uint8 else x.float()).contiguous()

    def _paired(self, *lists):
        out = tuple(torch.cat(v) for v in lists)                                                # (samples, T) fp64 on the host
        if self.paired_from_frame >= out[0].shape[1]:
            raise ValueError(f"Evaluator: paired_from_frame = {self.paired_from_frame} leaves none of the clips' {out[0].shape[1]} frames")
        return out

    def frame_curves(self):
        """{'psnr': (T,), 'ssim': (T,)} fp64 (with paired_metrics) and {'lpips': (T,)} (with an lpips_scorer): per frame number the mean
        over every sample pushed (all frames, whatever paired_from_frame says) -- the curve prediction papers plot.  A frame number at
        which any sample equals its target has a PSNR of inf."""
        if not self.paired_metrics and self.lpips_scorer is None:
            raise ValueError("Evaluator.frame_curves: the evaluator was built without paired_metrics and without an lpips_scorer")
        curves = {}
        if self.paired_metrics:
            psnr, ssim = self._paired(self.all_frame_psnr, self.all_frame_ssim)
            curves.update(psnr=psnr.mean(dim=0), ssim=ssim.mean(dim=0))
        if self.lpips_scorer is not None:
            curves["lpips"] = self._paired(self.all_frame_lpips)[0].mean(dim=0)
        return curves

    def evaluate_metrics(self, val_dataset=None, generator=None):
        gen = torch.cat(self.all_video_embeds_generated).flatten(1)
        gt = torch.cat(self.all_video_embeds_gt).flatten(1)
        metrics = {"fvd": float(frechet_distance(gen, gt))}
        if self.clip_scorer is not None:
            metrics["clipsim"] = float(torch.cat(self.all_clip_scores).mean())
        if self.paired_metrics:
            psnr, ssim = self._paired(self.all_frame_psnr, self.all_frame_ssim)
            metrics["psnr"] = float(psnr[:, self.paired_from_frame:].mean())
            metrics["ssim"] = float(ssim[:, self.paired_from_frame:].mean())
        if self.lpips_scorer is not None:
            metrics["lpips"] = float(self._paired(self.all_frame_lpips)[0][:, self.paired_from_frame:].mean())
        return metrics
