"""LPIPS v0.1 (Zhang et al. 2018) on the HIP path: the AlexNet and VGG-16 feature towers and the learned per-layer distance heads, per
frame pair of two clips.  The rule in full: include/gsdd.h.

  uint8 levels -> scaled stem operand        gsdd_lpips_stem_rows (csrc/lpips.hip), the 3 x 256 table of stem_table()
  convolution + bias + ReLU                  gsdd_gemm, an implicit GEMM over a tap table; the first one with kw merged into the
                                             contraction, as the I3D stem (i3d.py::_unit)
  max pool (floor mode, no padding)          gsdd_pool3d
  unit-normalise, squared difference,
  learned 1 x 1 weights, spatial sum         gsdd_lpips_layer_distance (csrc/lpips.hip)

Both nets are ONE layer table (NETS below, data) walked by one loop.  A score, not a loss: there are no gradients.  The published
AlexNet / VGG / `lin` weights cannot be obtained offline and are the user's to supply (loaders below); parity is pinned on seeded weights
against an fp64 restatement (tests/lpips_ref.py)."""
import os

import torch

from . import ops
from ._lib import GsddError
from .vqvae import conv_taps, pack_conv0_weight, pack_conv_weight

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def _conv(cin, cout, k, stride=1, pad=None, tap=False):
    return {"op": "conv", "cin": cin, "cout": cout, "k": k, "stride": stride, "pad": k // 2 if pad is None else pad, "tap": tap}


def _pool(k, stride):
    return {"op": "pool", "k": k, "stride": stride}


# torchvision's `features` without the ReLUs (one follows every convolution); tap: the ReLU output is one of the five compared layers
NETS = {
    "alex": {"backbone": "alexnet", "min_side": 31,
             "layers": (_conv(3, 64, 11, 4, 2, tap=True), _pool(3, 2), _conv(64, 192, 5, tap=True), _pool(3, 2),
                        _conv(192, 384, 3, tap=True), _conv(384, 256, 3, tap=True), _conv(256, 256, 3, tap=True))},
    "vgg": {"backbone": "vgg16", "min_side": 16,
            "layers": (_conv(3, 64, 3), _conv(64, 64, 3, tap=True), _pool(2, 2), _conv(64, 128, 3), _conv(128, 128, 3, tap=True), _pool(2, 2),
                       _conv(128, 256, 3), _conv(256, 256, 3), _conv(256, 256, 3, tap=True), _pool(2, 2),
                       _conv(256, 512, 3), _conv(512, 512, 3), _conv(512, 512, 3, tap=True), _pool(2, 2),
                       _conv(512, 512, 3), _conv(512, 512, 3), _conv(512, 512, 3, tap=True))},
}
N_TAPS = 5


def stem_table():
    """float32 (3, 256) on the host: table[c][level] = (level / 127.5 - 1 - SHIFT[c]) / SCALE[c], evaluated in fp64 and rounded once"""
    level = torch.arange(256, dtype=torch.float64)
    shift, scale = torch.tensor(SHIFT, dtype=torch.float64), torch.tensor(SCALE, dtype=torch.float64)
    return (((level / 127.5 - 1.0)[None, :] - shift[:, None]) / scale[:, None]).to(torch.float32)


def conv_keys(net):
    """[(torchvision `features` index, lpips slice number 1 .. 5)] of the net's convolutions in order.  In `features` a convolution is
    followed by its ReLU (two places) and a pool takes one; the lpips package cuts `features` behind every compared ReLU."""
    keys, index, slice_no = [], 0, 1
    for lay in _net(net)["layers"]:
        if lay["op"] == "pool":
            index += 1
            continue
        keys.append((index, slice_no))
        index += 2
        slice_no += 1 if lay["tap"] else 0
    return keys


def tap_channels(net):
    return tuple(lay["cout"] for lay in _net(net)["layers"] if lay["op"] == "conv" and lay["tap"])


def feature_sizes(net, H, W):
    """[(H, W) behind every table entry] for frames of H x W; raises below the net's smallest frame"""
    spec = _net(net)
    if min(H, W) < spec["min_side"]:
        raise GsddError(f"Lpips({net!r}): frames of {H} x {W} are below the net's smallest side, {spec['min_side']}")
    sizes = []
    for lay in spec["layers"]:
        pad = lay["pad"] if lay["op"] == "conv" else 0
        H, W = (H + 2 * pad - lay["k"]) // lay["stride"] + 1, (W + 2 * pad - lay["k"]) // lay["stride"] + 1
        sizes.append((H, W))
    return sizes


def _net(net):
    if net not in NETS:
        raise GsddError(f"Lpips: net {net!r} is not one of {sorted(NETS)}")
    return NETS[net]


def _take(sd, key):
    if key not in sd:
        raise GsddError(f"Lpips: the state dict has no {key!r}")
    return sd[key]


class Lpips:
    """Frozen fp32 weights of one LPIPS net and its forward pass on the HIP kernels.

    net: "alex" or "vgg"; convs: [(weight (Cout, Cin, k, k), bias (Cout,))] of the net's convolutions in order (5 for alex, 13 for vgg);
    lins: the five learned weight vectors, (C,) or (1, C, 1, 1) as the lpips package stores them, >= 0.  budget_bytes bounds the
    feature buffers: frames are processed in chunks whose two ping-pong buffers stay under it (VGG's relu1_2 at 128 x 128 is 4 MB a
    frame).  exact_f32: the towers' contractions on the exact-f32 MFMA instead of the bf16x3 split (None: GSDD_GEMM_F32 decides)."""

    def __init__(self, net, convs, lins, budget_bytes=256 << 20, exact_f32=None):
        spec = _net(net)
        self.net, self.budget_bytes, self.exact_f32 = net, int(budget_bytes), exact_f32
        table = [lay for lay in spec["layers"] if lay["op"] == "conv"]
        convs, lins = list(convs), list(lins)
        if len(convs) != len(table) or len(lins) != N_TAPS:
            raise GsddError(f"Lpips({net!r}): {len(table)} convolutions and {N_TAPS} lin layers are needed, got {len(convs)} and {len(lins)}")
        self.w, self.b = [], []
        for i, (lay, (w, b)) in enumerate(zip(table, convs)):
            want = (lay["cout"], lay["cin"], lay["k"], lay["k"])
            if tuple(w.shape) != want or tuple(b.shape) != want[:1]:
                raise GsddError(f"Lpips({net!r}): convolution {i} must be {want} with a bias {want[:1]}, got {tuple(w.shape)} and "
                                f"{tuple(b.shape)}")
            w5 = w.detach().to(torch.float32)[:, :, None]                                    # (Cout, Cin, 1, k, k): a 3-D kernel of depth 1
            self.w.append(pack_conv0_weight(w5) if i == 0 else pack_conv_weight(w5))
            self.b.append(b.detach().to(torch.float32).contiguous())
        self.lin = []
        for k, (c, v) in enumerate(zip(tap_channels(net), lins)):
            if v.numel() != c or tuple(v.shape) not in ((c,), (1, c, 1, 1)):
                raise GsddError(f"Lpips({net!r}): lin{k} must be ({c},) or (1, {c}, 1, 1), got {tuple(v.shape)}")
            self.lin.append(v.detach().to(torch.float32).reshape(c).contiguous())
        self.table = stem_table()
        self._taps, self._buffers = {}, []

    # ------------------------------------------------------------------ weight import
    @classmethod
    def from_lpips_state_dict(cls, sd, net=None, **kwargs):
        """sd: a full `lpips.LPIPS(net=...).state_dict()`:
            net.slice{s}.{i}.weight | .bias    the backbone's convolutions, s = 1 .. 5 the slice that ends at the s-th compared ReLU and
                                               i torchvision's `features` index: alex (s, i) = (1, 0) (2, 3) (3, 6) (4, 8) (5, 10);
                                               vgg (1, 0) (1, 2) (2, 5) (2, 7) (3, 10) (3, 12) (3, 14) (4, 17) (4, 19) (4, 21) (5, 24)
                                               (5, 26) (5, 28)
            lin{k}.model.1.weight              (1, C, 1, 1), k = 0 .. 4
        The duplicates `lins.{k}.model.1.weight` and the constants `scaling_layer.shift | scale` are ignored.  net: "alex" or "vgg";
        by default told from the keys (`net.slice5.28.weight` exists in vgg alone)."""
        if net is None:
            net = "vgg" if "net.slice5.28.weight" in sd else "alex"
        convs = [(_take(sd, f"net.slice{s}.{i}.weight"), _take(sd, f"net.slice{s}.{i}.bias")) for i, s in conv_keys(net)]
        return cls(net, convs, [_take(sd, f"lin{k}.model.1.weight") for k in range(N_TAPS)], **kwargs)

    @classmethod
    def from_state_dicts(cls, backbone_sd, lin_sd, net, **kwargs):
        """backbone_sd: a torchvision `alexnet` / `vgg16` state dict (`features.{i}.weight | .bias`, i as in from_lpips_state_dict; the
        classifier's keys are ignored); lin_sd: the lpips package's `weights/v0.1/<net>.pth` (`lin{k}.model.1.weight`, k = 0 .. 4)."""
        convs = [(_take(backbone_sd, f"features.{i}.weight"), _take(backbone_sd, f"features.{i}.bias")) for i, _ in conv_keys(net)]
        return cls(net, convs, [_take(lin_sd, f"lin{k}.model.1.weight") for k in range(N_TAPS)], **kwargs)

    @classmethod
    def from_pretrained(cls, path, net="alex", **kwargs):
        """path: one file holding a full lpips state dict (from_lpips_state_dict), or a directory holding `<net>.pth` (the lin layers) and
        `alexnet.pth` / `vgg16.pth` (the torchvision backbone).  Loaded with torch.load(weights_only=True); nothing is ever fetched."""
        spec = _net(net)

        def load(p):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"Lpips.from_pretrained: {p!r} does not exist; the weights must be supplied -- nothing is downloaded")
            return torch.load(p, map_location="cpu", weights_only=True)
        if os.path.isdir(path):
            return cls.from_state_dicts(load(os.path.join(path, spec["backbone"] + ".pth")), load(os.path.join(path, net + ".pth")), net,
                                        **kwargs)
        return cls.from_lpips_state_dict(load(path), net, **kwargs)

    # ------------------------------------------------------------------ placement
    def to(self, device):
        dev = torch.device(device)
        self.w, self.b, self.lin = [t.to(dev) for t in self.w], [t.to(dev) for t in self.b], [t.to(dev) for t in self.lin]
        self.table = self.table.to(dev)
        self._taps, self._buffers = {}, []
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    @property
    def device(self):
        return self.table.device

    # ------------------------------------------------------------------ forward
    def frame_floats(self, H, W):
        """the floats of the largest feature map (the stem operand included) of one frame of H x W"""
        spec = _net(self.net)
        sizes = feature_sizes(self.net, H, W)
        stem = 4 * H * (W + 2 * spec["layers"][0]["pad"])
        return max([stem] + [(lay["cout"] if lay["op"] == "conv" else c_in) * h * w
                             for lay, (h, w), c_in in zip(spec["layers"], sizes, self._channels_in())])

    def _channels_in(self):
        c, out = 3, []
        for lay in _net(self.net)["layers"]:
            out.append(c)
            c = lay["cout"] if lay["op"] == "conv" else c
        return out

    def chunk_frames(self, H, W):
        """frame pairs per chunk: two ping-pong buffers of 2 x chunk frames stay under budget_bytes (one pair at the least)"""
        return max(1, self.budget_bytes // (2 * 2 * 4 * self.frame_floats(H, W)))

    def _tap_table(self, lay, first):
        key = (lay["k"], lay["pad"], first)
        if key not in self._taps:
            k, p = lay["k"], lay["pad"]
            # first: kw lives in the contraction, the taps run over kh alone and the W axis is padded by p in front (offset p - p = 0)
            taps = [(0, a - p, 0) for a in range(k)] if first else conv_taps((1, k, k), (1, 1, 1), (0, p, p))
            self._taps[key] = ops.taps_tensor(taps, self.device)
        return self._taps[key]

    def _pingpong(self, floats):
        """two flat buffers of at least `floats` floats, kept between calls (every kernel writes all of the view it is given)"""
        if not self._buffers or self._buffers[0].numel() < floats:
            self._buffers = [torch.zeros((floats,), dtype=torch.float32, device=self.device) for _ in range(2)]
        return self._buffers

    def _chunk(self, pred, target, frame0, m, H, W, out):
        """frame pairs frame0 .. frame0 + m - 1 -> out[frame0 : frame0 + m] (their five layer distances)"""
        spec = _net(self.net)
        bufs = self._pingpong(2 * m * self.frame_floats(H, W))
        p = spec["layers"][0]["pad"]
        h = bufs[1][:2 * m * H * (W + 2 * p) * 4].view(2 * m, H, W + 2 * p, 4)
        ops.lpips_stem_rows(pred, self.table, p, frame0, m, out=h[:m])
        ops.lpips_stem_rows(target, self.table, p, frame0, m, out=h[m:])
        dims, C_, conv, tap = (2 * m, 1, H, W + 2 * p), 4, 0, 0
        for i, (lay, (Ho, Wo)) in enumerate(zip(spec["layers"], feature_sizes(self.net, H, W))):
            k, s = lay["k"], lay["stride"]
            Co = lay["cout"] if lay["op"] == "conv" else C_
            o = bufs[i % 2][:2 * m * Ho * Wo * Co].view(2 * m * Ho * Wo, Co)
            if lay["op"] == "pool":
                ops.pool3d(h, dims, C_, (1, k, k), (1, s, s), (0, 0, 0), (1, Ho, Wo), o, mode="max")
            else:
                first = conv == 0
                w = self.w[conv]
                ops.gemm(h, w, o, in_dims=dims, out_grid=(1, Ho, Wo), stride=(1, s, s), taps=self._tap_table(lay, first), ntaps=w.shape[0],
                         cin=w.shape[2], in_pitch=4 if first else None, epi_shift=self.b[conv], act=ops.ACT_RELU, cout=Co,
                         exact_f32=self.exact_f32)
                conv += 1
                if lay["tap"]:
                    out[frame0:frame0 + m, tap] = ops.lpips_layer_distance(o, self.lin[tap], m)
                    tap += 1
            h, dims, C_ = o, (2 * m, 1, Ho, Wo), Co

    @torch.no_grad()
    def forward(self, pred, target, chunk=None):
        """pred, target: clips in paired_frame_metrics' operand forms -- float32 (B, 3, T, H, W), ImageNet-normalised as the decoder
        returns it (its levels by the uint8 rule), or uint8 (B, T, H, W, 3) --, each in its own form, of the same B, T, H, W, on the
        scorer's device -> {"lpips": (B, T) fp64, "layers": (B, T, 5) fp64} on the host: per frame pair the five layer distances and
        their sum.  Unscaled, >= 0, exactly 0 for equal frames.  chunk: frame pairs per pass (by default what budget_bytes allows);
        the result does not depend on it."""
        if self.device.type != "cuda":
            raise GsddError("Lpips.forward needs the weights on a ROCm device (no CPU fallback): call .to(device) first")
        _, shape = ops._paired_operand("pred", pred)
        _, shape_t = ops._paired_operand("target", target)
        if shape != shape_t or pred.device != target.device or pred.device != self.device:
            raise GsddError(f"Lpips.forward: pred is (B, T, H, W) = {shape} on {pred.device}, target {shape_t} on {target.device}, the "
                            f"weights on {self.device}")
        B, T, H, W = shape
        if min(shape) < 1:
            raise GsddError(f"Lpips.forward: empty operands {shape}")
        feature_sizes(self.net, H, W)                                           # (raises below the net's smallest frame)
        n = B * T
        m = self.chunk_frames(H, W) if chunk is None else int(chunk)
        if m < 1:
            raise GsddError(f"Lpips.forward: chunk = {chunk!r} is not a number of frame pairs >= 1")
        layers = torch.zeros((n, N_TAPS), dtype=torch.float64, device=self.device)
        for frame0 in range(0, n, m):
            self._chunk(pred, target, frame0, min(m, n - frame0), H, W, layers)
        layers = layers.cpu().view(B, T, N_TAPS)
        return {"lpips": layers.sum(dim=-1), "layers": layers}

    __call__ = forward
