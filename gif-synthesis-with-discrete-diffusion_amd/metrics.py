"""Fréchet distance between two feature sets: the statistic behind the reference's FVD
(src/utils/evaluator.py:118-179, itself the TF-GAN formulation).  The I3D feature extractor the reference feeds it with needs
weights that cannot be obtained offline, so only the statistic is provided; it is evaluation glue (plain torch linear algebra on
whatever device the features live on), not part of the hot path."""
import torch


def clip_similarity(text_embeds, frame_embeds, eps=1e-12):
    """CLIPSIM per sample: text_embeds (B, E), frame_embeds (B, T, E) -> (B,) fp64, the mean over the T frames of the cosine similarity
    between the caption's CLIP text feature and the frame's CLIP image feature.  Computed in fp64 with torch, like frechet_distance.
    UNSCALED: a cosine in [-1, 1]; some papers print 100 x this number (and CLIP's own logits carry its learned temperature)."""
    t = torch.as_tensor(text_embeds).to(torch.float64)
    f = torch.as_tensor(frame_embeds).to(torch.float64).to(t.device)
    if t.dim() != 2 or f.dim() != 3 or f.shape[0] != t.shape[0] or f.shape[2] != t.shape[1]:
        raise ValueError(f"clip_similarity: text_embeds {tuple(t.shape)} / frame_embeds {tuple(f.shape)} are not (B, E) / (B, T, E)")
    t = t / t.norm(dim=-1, keepdim=True).clamp_min(eps)
    f = f / f.norm(dim=-1, keepdim=True).clamp_min(eps)
    return (f * t[:, None, :]).sum(dim=-1).mean(dim=1)


def _frame_psnr(sse, values):
    """sse (B, T, 3) int64 -> (B, T) fp64 on the host: 10 log10(255^2 values / sum_c sse), inf where the frame has no error"""
    from .gif import psnr_from_sse
    total = sse.sum(dim=-1).cpu()
    return torch.tensor([psnr_from_sse(v, values) for v in total.flatten().tolist()], dtype=torch.float64).view(total.shape)


def paired_frame_metrics(pred, target, lpips=None):
    """PSNR and SSIM of every frame of `pred` against the same frame of `target`, on their uint8 levels.  Either operand is float32
    (B, 3, T, H, W), ImageNet-normalised as the decoder returns it (levels by the evaluator's rule: (x std + mean) 255 in fp32,
    truncated, clamped, NaN -> 0), or uint8 (B, T, H, W, 3) as read_gif and palette[indices] give it; both on a ROCm device, H, W >= 11.
    -> {"psnr": (B, T) fp64 dB over the frame's three channels, inf for a frame equal to its target, "ssim": (B, T) fp64, the mean over
    the channels of the Gaussian-window SSIM (Wang et al. 2004: 11 x 11, sigma 1.5, valid windows, data range 255), "sse": (B, T, 3)
    int64}, all on the host.  The per-pixel work is one HIP kernel (ops.paired_metrics; the rule in full: include/gsdd.h), the rest is
    torch on (B, T, 3) numbers in fp64.  SSIM is UNSCALED, in [-1, 1].
    lpips: a gsdd_amd.lpips.Lpips scorer on the operands' device, or None.  With one the dict also holds "lpips": (B, T) fp64, the
    frame pairs' LPIPS (unscaled, >= 0, 0 for equal frames), and the frames must reach the net's smallest side (31 for alex, 16 for
    vgg); without one nothing of it runs and the dict is the three entries above."""
    from . import ops
    sse, ssim = ops.paired_metrics(pred, target, want_ssim=True)
    H, W = (pred.shape[3], pred.shape[4]) if pred.dtype == torch.float32 else (pred.shape[2], pred.shape[3])
    out = {"psnr": _frame_psnr(sse, 3 * H * W), "ssim": ssim.cpu().sum(dim=-1) / 3.0, "sse": sse.cpu()}
    if lpips is not None:
        out["lpips"] = lpips(pred, target)["lpips"]
    return out


def psnr(pred, target):
    """The PSNR of paired_frame_metrics alone, (B, T) fp64 on the host: no SSIM is formed, so any H, W >= 1 is taken."""
    from . import ops
    sse, _ = ops.paired_metrics(pred, target, want_ssim=False)
    H, W = (pred.shape[3], pred.shape[4]) if pred.dtype == torch.float32 else (pred.shape[2], pred.shape[3])
    return _frame_psnr(sse, 3 * H * W)


def _sym_sqrt(mat, eps=1e-10):
    """U diag(sqrt(s)) V^T with singular values below eps left as they are (evaluator.py:119-122)."""
    u, s, vh = torch.linalg.svd(mat)
    si = torch.where(s < eps, s, torch.sqrt(s))
    return (u * si) @ vh


def trace_sqrt_product(sigma, sigma_v):
    """tr(sqrt(sigma^(1/2) sigma_v sigma^(1/2))) (evaluator.py:125-128)."""
    root = _sym_sqrt(sigma)
    return torch.trace(_sym_sqrt(root @ (sigma_v @ root)))


def covariance(x):
    """Unbiased covariance of observations in rows (evaluator.py:131-163 with rowvar=False)."""
    xc = x - x.mean(dim=0, keepdim=True)
    return (xc.t() @ xc) / (x.shape[0] - 1)


def frechet_distance(x1, x2):
    """|m1 - m2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2)) over features flattened per sample (evaluator.py:166-179)."""
    x1 = torch.as_tensor(x1).flatten(start_dim=1)
    x2 = torch.as_tensor(x2).flatten(start_dim=1)
    m, m_w = x1.mean(dim=0), x2.mean(dim=0)
    sigma, sigma_w = covariance(x1), covariance(x2)
    trace = torch.trace(sigma + sigma_w) - 2.0 * trace_sqrt_product(sigma, sigma_w)
    return trace + torch.sum((m - m_w) ** 2)
