"""torch fp64 restatement of LPIPS v0.1 (gsdd_amd/lpips.py, csrc/lpips.hip; the rule: include/gsdd.h): the input table, the AlexNet
and VGG-16 towers through F.conv2d / F.max_pool2d, the unit-normalised, weighted, spatially averaged squared difference of the five
compared layers.  Plain module (not a conftest), on top of tests/paired_ref.py's operand forms and contents.  Next to the rule it holds
what the tests judge it and the kernels by: the same restatement in fp32 (whose own error against fp64 sets the GPU tolerance), an
independent im2col formulation, the rule with a fault switched in, seeded weights in the published state-dict layouts, and the case
list the host and GPU tests share.  The layer tables are written out here once more, not imported from the package."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import paired_ref

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

# (kind, ...): ("conv", cin, cout, k, stride, pad, compared) / ("pool", k, stride); a ReLU follows every convolution
ALEX = (("conv", 3, 64, 11, 4, 2, True), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2, True), ("pool", 3, 2),
        ("conv", 192, 384, 3, 1, 1, True), ("conv", 384, 256, 3, 1, 1, True), ("conv", 256, 256, 3, 1, 1, True))


def _vgg16():
    out, cin = [], 3
    for block, (width, convs) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
        if block:
            out.append(("pool", 2, 2))
        for i in range(convs):
            out.append(("conv", cin, width, 3, 1, 1, i == convs - 1))
            cin = width
    return tuple(out)


LAYERS = {"alex": ALEX, "vgg": _vgg16()}
FEATURE_INDEX = {"alex": (0, 3, 6, 8, 10), "vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)}       # torchvision's `features`
SLICE = {"alex": (1, 2, 3, 4, 5), "vgg": (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)}                         # the lpips package's slices
BACKBONE = {"alex": "alexnet", "vgg": "vgg16"}
MIN_SIDE = {"alex": 31, "vgg": 16}
TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}


def table():
    """the input rule as 3 x 256 numbers: (level / 127.5 - 1 - shift_c) / scale_c in fp64, rounded to fp32 once -> float32 (3, 256)"""
    level = np.arange(256, dtype=np.float64)
    rows = [(level / 127.5 - 1.0 - SHIFT[c]) / SCALE[c] for c in range(3)]
    return np.stack(rows).astype(np.float32)


# ----------------------------------------------------------------------------- seeded weights, in the published layouts
def seeded_weights(net, seed=0, dead_layer=None):
    """-> (convs [(weight (Cout, Cin, k, k), bias (Cout,))], lins [(1, C, 1, 1)]) float32 from a torch.Generator: He-scaled normal
    convolution weights, biases 0.1 N(0, 1), lin weights uniform in [0, 1).  dead_layer: that convolution's biases are -10, so that its
    ReLU outputs are all zero (every position of that layer is a dead one)."""
    g = torch.Generator().manual_seed(1000 * seed + len(net))
    convs = []
    for lay in LAYERS[net]:
        if lay[0] != "conv":
            continue
        _, cin, cout, k = lay[:4]
        w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = 0.1 * torch.randn((cout,), generator=g)
        if dead_layer is not None and len(convs) == dead_layer:
            b = torch.full((cout,), -10.0)
        convs.append((w, b))
    lins = [torch.rand((1, c, 1, 1), generator=g) for c in TAP_CHANNELS[net]]
    return convs, lins


def lpips_state_dict(net, convs, lins):
    """what `lpips.LPIPS(net=...).state_dict()` holds: the backbone under net.slice{s}.{i}, the lin layers twice (lin{k} and the
    ModuleList lins.{k}), the scaling layer's constants"""
    sd = {"scaling_layer.shift": torch.tensor(SHIFT)[None, :, None, None], "scaling_layer.scale": torch.tensor(SCALE)[None, :, None, None]}
    for (w, b), i, s in zip(convs, FEATURE_INDEX[net], SLICE[net]):
        sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"] = w, b
    for k, v in enumerate(lins):
        sd[f"lin{k}.model.1.weight"] = v
        sd[f"lins.{k}.model.1.weight"] = v
    return sd


def backbone_state_dict(net, convs):
    """a torchvision alexnet / vgg16 state dict: features.{i}.* and a classifier the loader has to ignore"""
    sd = {"classifier.6.weight": torch.zeros((10, 16)), "classifier.6.bias": torch.zeros((10,))}
    for (w, b), i in zip(convs, FEATURE_INDEX[net]):
        sd[f"features.{i}.weight"], sd[f"features.{i}.bias"] = w, b
    return sd


def lin_state_dict(lins):
    """the lpips package's weights/v0.1/<net>.pth"""
    return {f"lin{k}.model.1.weight": v for k, v in enumerate(lins)}


# ----------------------------------------------------------------------------- THE RULE
def stem(lv, dtype=torch.float64, scaling=True, bgr=False):
    """levels (B, T, H, W, 3) uint8 -> (B T, 3, H, W): the table's values (scaling=False, a FAULT: level / 127.5 - 1 alone)"""
    lv = torch.from_numpy(np.ascontiguousarray(paired_ref.levels(lv))).flatten(0, 1).long()
    if scaling:
        t = torch.from_numpy(table()).to(dtype)
        x = torch.stack([t[c][lv[..., c]] for c in range(3)], dim=1)
    else:
        x = (lv.to(dtype) / 127.5 - 1.0).permute(0, 3, 1, 2)
    return x.flip(1) if bgr else x


def taps(net, x, convs, level_pad=False, pre_relu=False, ceil_pools=False):
    """x (N, 3, H, W) -> the five compared feature maps, in x's dtype.  level_pad (a FAULT): the first convolution pads with the value
    level 0 maps to; pre_relu (a FAULT): the compared maps are taken in front of their ReLU; ceil_pools (a FAULT)."""
    out, conv = [], 0
    h = x
    for lay in LAYERS[net]:
        if lay[0] == "pool":
            h = F.max_pool2d(h, lay[1], lay[2], ceil_mode=ceil_pools)
            continue
        _, _, _, k, stride, pad, compared = lay
        w, b = (t.to(x.dtype) for t in convs[conv])
        if conv == 0 and level_pad:
            t0 = torch.from_numpy(table()).to(x.dtype)[:, 0]
            padded = t0[None, :, None, None].expand(h.shape[0], 3, h.shape[2] + 2 * pad, h.shape[3] + 2 * pad).clone()
            padded[:, :, pad:pad + h.shape[2], pad:pad + h.shape[3]] = h
            z = F.conv2d(padded, w, b, stride=stride)
        else:
            z = F.conv2d(h, w, b, stride=stride, padding=pad)
        h = F.relu(z)
        if compared:
            out.append(z if pre_relu else h)
        conv += 1
    return out


def layer_distance(a, b, w, eps=EPS, spatial_sum=False):
    """a, b (N, C, H, W), w (C,) or (1, C, 1, 1) -> (N,): mean over positions of sum_c w_c (a^_c - b^_c)^2, eps outside the root"""
    na = a / (torch.sqrt((a * a).sum(dim=1, keepdim=True)) + eps)
    nb = b / (torch.sqrt((b * b).sum(dim=1, keepdim=True)) + eps)
    d = ((na - nb) ** 2 * w.to(a.dtype).reshape(1, -1, 1, 1)).sum(dim=1)
    return d.sum(dim=(1, 2)) if spatial_sum else d.mean(dim=(1, 2))


def lpips(net, a, b, weights, dtype=torch.float64, fault=None):
    """two operands in either form -> (B, T, 5) in `dtype`: the five layer distances of every frame pair (LPIPS is their sum).
    fault: one of FAULTS, or None for the rule."""
    convs, lins = weights
    f = dict(FAULTS[fault]) if fault else {}
    shape = paired_ref.levels(a).shape[:2]
    skip = f.pop("skip_tap", None)
    eps = f.pop("eps", EPS)
    spatial_sum = f.pop("spatial_sum", False)
    stem_kw = {k: f.pop(k) for k in ("scaling", "bgr") if k in f}
    with torch.no_grad():
        fa, fb = taps(net, stem(a, dtype, **stem_kw), convs, **f), taps(net, stem(b, dtype, **stem_kw), convs, **f)
        d = [layer_distance(x, y, w, eps, spatial_sum) for x, y, w in zip(fa, fb, lins)]
    if skip is not None:
        d[skip] = torch.zeros_like(d[skip])
    return torch.stack(d, dim=-1).view(*shape, 5)


# the faults of the rule that the tolerance has to tell from the rule: keyword arguments consumed by lpips()
FAULTS = {
    "level_space_padding": dict(level_pad=True),
    "no_scaling_layer": dict(scaling=False),
    "spatial_sum": dict(spatial_sum=True),
    "skipped_tap": dict(skip_tap=2),
    "bgr_order": dict(bgr=True),
    "tap_before_relu": dict(pre_relu=True),
    "ceil_mode_pools": dict(ceil_pools=True),
    "no_eps": dict(eps=0.0),
}


# ----------------------------------------------------------------------------- an independent formulation
def _unfolded(h, k, stride, pad, fill=0.0):
    """(N, C, H, W) -> (N, C, k k, positions), Ho, Wo"""
    N, C, H, W = h.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if pad:
        h = F.pad(h, (pad, pad, pad, pad), value=fill)
    return F.unfold(h, k, stride=stride).view(N, C, k * k, Ho * Wo), Ho, Wo


def lpips_im2col(net, a, b, weights):
    """the rule once more in fp64 without conv2d, max_pool2d or the normalised vectors: convolutions as one matrix product over
    unfolded patches, pools as a maximum over unfolded windows, and the distance expanded,
    sum_c w_c (a^_c - b^_c)^2 = sum w a a / (|a| + eps)^2 + sum w b b / (|b| + eps)^2 - 2 sum w a b / ((|a| + eps)(|b| + eps))"""
    convs, lins = weights
    out = []
    with torch.no_grad():
        ha, hb = stem(a), stem(b)
        conv = 0
        for lay in LAYERS[net]:
            nxt = []
            for h in (ha, hb):
                if lay[0] == "pool":
                    cols, Ho, Wo = _unfolded(h, lay[1], lay[2], 0)
                    nxt.append(cols.max(dim=2).values.view(h.shape[0], h.shape[1], Ho, Wo))
                else:
                    _, cin, cout, k, stride, pad, _ = lay
                    w, bias = (t.double() for t in convs[conv])
                    cols, Ho, Wo = _unfolded(h, k, stride, pad)
                    z = torch.einsum("ok,nkp->nop", w.reshape(cout, cin * k * k), cols.reshape(h.shape[0], cin * k * k, Ho * Wo))
                    nxt.append(torch.clamp_min(z + bias[None, :, None], 0.0).view(h.shape[0], cout, Ho, Wo))
            ha, hb = nxt
            if lay[0] == "conv":
                if lay[6]:
                    w = lins[len(out)].double().reshape(1, -1, 1, 1)
                    ra, rb = torch.sqrt((ha * ha).sum(1)) + EPS, torch.sqrt((hb * hb).sum(1)) + EPS
                    d = (w * ha * ha).sum(1) / (ra * ra) + (w * hb * hb).sum(1) / (rb * rb) - 2.0 * (w * ha * hb).sum(1) / (ra * rb)
                    out.append(d.mean(dim=(1, 2)))
                conv += 1
    shape = paired_ref.levels(a).shape[:2]
    return torch.stack(out, dim=-1).view(*shape, 5)


# ----------------------------------------------------------------------------- the case list
KINDS = ("random", "noise10", "ramp", "flat250", "black_white")
SHAPES = {"alex": ((2, 2, 31, 31), (2, 2, 31, 45), (2, 2, 32, 32), (2, 2, 47, 35), (2, 2, 64, 64), (1, 1, 128, 128)),
          "vgg": ((1, 2, 16, 16), (1, 2, 17, 23), (1, 2, 32, 32), (1, 2, 64, 64))}
FORMS = (("float", "float"), ("float", "uint8"), ("uint8", "float"), ("uint8", "uint8"))


def cases(net):
    """-> [(name, a levels, b levels, (form of a, form of b))]: every frame size with every content; the forms the GPU test hands the
    operands over in rotate through the four pairings"""
    out = []
    for s in SHAPES[net]:
        for kind in KINDS:
            a, b = paired_ref.content(kind, s, seed=7)
            out.append((f"{kind}_{s[2]}x{s[3]}", a, b, FORMS[len(out) % 4]))
    return out


@functools.lru_cache(maxsize=None)
def yardstick(net):
    """-> (rho, {case: the rule's (B, T, 5) fp64}, {case: its rho}): rho = the worst over all cases and frames of
    |fp32 restatement - fp64| / sqrt(fp64) on the frame's LPIPS.  The distance is a sum of squared differences, so an absolute feature
    error e moves it by about 2 sqrt(d) e: the error of an fp32 evaluation scales with the ROOT of the value.  The GPU bound on a frame
    is 4 rho sqrt(want).  Evaluated once per process for the host and the GPU tests alike."""
    weights = seeded_weights(net)
    want, per_case = {}, {}
    for name, a, b, _ in cases(net):
        d64 = lpips(net, a, b, weights)
        d32 = lpips(net, a, b, weights, dtype=torch.float32)
        assert d64.dtype == torch.float64 and d32.dtype == torch.float32
        v = d64.sum(dim=-1)
        per_case[name] = float(((d32.double().sum(dim=-1) - v).abs() / v.sqrt()).max())
        want[name] = d64
    return max(per_case.values()), want, per_case
