"""Cases behind tests/test_daformer_head_cpu.py and tests/test_gpu_daformer_head.py, and the plain-torch restatement of the DAFormer
head (G5/model/networks/segformer_head.py:167-466) with its concatenations formed: Linear embeddings as 1x1 convs, F.interpolate to
the first stage's grid, torch.cat in in_index order, 1x1 branch and three depthwise-3x3 (groups = C) / 1x1 branches at dilations 6,
12, 18, each conv -> BatchNorm -> ReLU, torch.cat, 3x3 bottleneck -> BatchNorm -> ReLU, 1x1 conv_seg.  It runs in any dtype on any
device; tools/gen_golden.py::gen_daformer_head uses `state`, `inputs` and `stored` so that the capture of the reference class and the
tests read the same weights, inputs and sample positions (nothing of them is stored but checksums).

The capture pins the ConvModule / DepthwiseSeparableConvModule blocks to mmcv 1.x's documented behaviour, not its code (the generator's
stand-in): parity is unpinned for them.
"""
import zlib

import torch
import torch.nn.functional as F

E = 256                                  # the reference hard-codes embed_dim (:200)
DILATIONS = (1, 6, 12, 18)
IN_CHANNELS, CHANNELS, CLASSES, BATCH = [8, 16, 24, 32], 32, 19, 2
GRIDS = ((40, 28), (20, 14), (10, 7), (5, 4))          # taps of dilation 18 land inside 40 x 28; 5 x 4 -> 28 wide: ratio 7
GRIDS_EVAL = ((37, 29), (19, 15), (10, 8), (5, 4))
SEED = 2601

# (N, H, W, C, dilation, ld_in, ld_out, channel offset of the slice view); ld 0 = dense
DW_CASES = {
    "dense": (2, 23, 19, 36, 1, 0, 0, 0),
    "pitched": (1, 23, 19, 36, 6, 48, 44, 0),
    "wider_than_map": (2, 13, 11, 64, 12, 0, 0, 0),      # dilation > W; rows 0 and 12 are the one pair in range
    "centre_only": (1, 7, 5, 4, 18, 0, 0, 0),
    "chunk_tail": (1, 64, 64, 260, 6, 0, 0, 0),          # 260 = 8 chunks of 32 + 4
    "head_width": (2, 40, 28, 1024, 18, 1280, 1280, 256),
}


def _gen(name):
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return g


def half_grid(t):
    """Values on the float16 grid: exact in fp32 and float64 alike."""
    return t.half().float()


def shapes(in_channels=IN_CHANNELS, channels=CHANNELS, classes=CLASSES):
    """State-dict keys and shapes of the head, in the reference's order (mmcv's block names)."""
    out = {}

    def block(prefix, wshape):
        out[prefix + ".conv.weight"] = wshape
        c = wshape[0]
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{prefix}.bn.{k}"] = (c,)
        out[f"{prefix}.bn.num_batches_tracked"] = ()

    for i, c in enumerate(in_channels):
        out[f"embed_layers.{i}.proj.weight"] = (E, c)
        out[f"embed_layers.{i}.proj.bias"] = (E,)
    block("fuse_layer.aspp_modules.0", (channels, 4 * E, 1, 1))
    for k in (1, 2, 3):
        block(f"fuse_layer.aspp_modules.{k}.depthwise_conv", (4 * E, 1, 3, 3))
        block(f"fuse_layer.aspp_modules.{k}.pointwise_conv", (channels, 4 * E, 1, 1))
    block("fuse_layer.bottleneck", (channels, 4 * channels, 3, 3))
    out["conv_seg.weight"] = (classes, channels, 1, 1)
    out["conv_seg.bias"] = (classes,)
    return out


def state(in_channels=IN_CHANNELS, channels=CHANNELS, classes=CLASSES, seed=SEED):
    """Seeded state dict on the float16 grid: conv / Linear weights at 1.5 x the fan-in scale (ReLUs on both sides), non-trivial
    BatchNorm affine pairs and running statistics."""
    sd = {}
    for k, shp in shapes(in_channels, channels, classes).items():
        g = _gen(f"{seed}:{k}")
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var"):
            sd[k] = half_grid(1.0 + 0.5 * torch.rand(shp, generator=g))
        elif k.endswith("running_mean"):
            sd[k] = half_grid(0.2 * torch.randn(shp, generator=g))
        elif len(shp) in (2, 4):
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            sd[k] = half_grid(torch.randn(shp, generator=g) * (1.5 / fan_in ** 0.5))
        elif k.endswith("bn.weight"):
            sd[k] = half_grid(1.0 + 0.2 * torch.randn(shp, generator=g))
        else:
            sd[k] = half_grid(0.2 * torch.randn(shp, generator=g))
    return sd


def inputs(grids=GRIDS, n=BATCH, in_channels=IN_CHANNELS, seed=SEED, tag="train"):
    return [half_grid(torch.randn((n, c, h, w), generator=_gen(f"{seed}:{tag}:c{i + 1}"))) for i, (c, (h, w)) in enumerate(zip(in_channels, grids))]


def probe(shape, seed=SEED):
    return half_grid(torch.randn(shape, generator=_gen(f"{seed}:probe")))


def checksum(ts):
    """Order-sensitive float64 checksum of a list of tensors (the fixture keeps it for `state` and `inputs`)."""
    tot = 0.0
    for t in ts:
        v = t.detach().to(torch.float64).reshape(-1)
        tot += float((v * torch.cos(torch.arange(1, v.numel() + 1, dtype=torch.float64) * 0.37)).sum())
    return tot


# ------------------------------------------------------------------------------------------------------------- the restatement
def _bn(x, sd, prefix, training, relu, masks=None, pre=None):
    y = F.batch_norm(x, sd[prefix + ".running_mean"], sd[prefix + ".running_var"], sd[prefix + ".weight"], sd[prefix + ".bias"], training, 0.1,
                     1e-5)
    if pre is not None:
        pre[prefix] = y.detach().cpu()
    if relu and masks is not None:
        return y * masks[prefix].to(device=y.device, dtype=y.dtype)       # the ReLU with ANOTHER run's decisions (see `forward`)
    return F.relu(y) if relu else y


def raw_features(sd, feats):
    size = feats[0].shape[2:]
    outs = []
    for i, f in enumerate(feats):
        t = F.conv2d(f, sd[f"embed_layers.{i}.proj.weight"][:, :, None, None], sd[f"embed_layers.{i}.proj.bias"])
        if t.shape[2:] != size:
            t = F.interpolate(t, size=size, mode="bilinear", align_corners=False)
        outs.append(t)
    return torch.cat(outs, dim=1)


def forward(sd, feats, training, relu=True, masks=None, pre=None):
    """(logits, feat, feat_raw); the running statistics in `sd` are updated in place when training.
    `pre` (a dict): receives every BatchNorm's output in front of its ReLU, by the BatchNorm's state-dict prefix.
    `masks` (prefix -> bool tensor): every ReLU becomes a multiplication by that mask -- the function another run evaluated, where
    that run decided a pre-activation of rounding size the other way.  Such a site changes the forward by its own size (nothing)
    and the gradients in front of it by O(1e-2) of scale, so two correct fp32 runs can only be compared element by element with a
    reference that takes the same decisions; the caller checks that the masks are legitimate (`mask_disagreements`)."""
    raw = raw_features(sd, feats)
    c = raw.shape[1]
    p = "fuse_layer.aspp_modules."
    kw = dict(masks=masks, pre=pre)
    outs = [_bn(F.conv2d(raw, sd[p + "0.conv.weight"]), sd, p + "0.bn", training, relu, **kw)]
    for k, d in enumerate(DILATIONS[1:], start=1):
        t = _bn(F.conv2d(raw, sd[f"{p}{k}.depthwise_conv.conv.weight"], None, 1, d, d, c), sd, f"{p}{k}.depthwise_conv.bn", training, relu, **kw)
        outs.append(_bn(F.conv2d(t, sd[f"{p}{k}.pointwise_conv.conv.weight"]), sd, f"{p}{k}.pointwise_conv.bn", training, relu, **kw))
    feat = _bn(F.conv2d(torch.cat(outs, dim=1), sd["fuse_layer.bottleneck.conv.weight"], None, 1, 1), sd, "fuse_layer.bottleneck.bn", training,
               relu, **kw)
    return F.conv2d(feat, sd["conv_seg.weight"], sd["conv_seg.bias"]), feat, raw


def mask_disagreements(masks, pre64):
    """Per BatchNorm: (number of sites where `masks` differs from the float64 run's own ReLU decision, the largest |float64
    pre-activation| among them in units of that tensor's max |pre-activation|)."""
    out = {}
    for k, m in masks.items():
        p = pre64[k].double()
        diff = m.cpu() != (p > 0)
        out[k] = (int(diff.sum()), float(p[diff].abs().max() / p.abs().max()) if bool(diff.any()) else 0.0)
    return out


def composed_raw_features(self, inputs):
    """feat_raw the reference's way on the GPU: embed, F.interpolate, torch.cat."""
    from diga_amd.model.networks.segformer_head import _pointwise        # (the module's embedding: only the resize and the cat are torch's)
    size = inputs[0].shape[2:]
    outs = []
    for i in self.in_index:
        lin = self.embed_layers[str(i)].proj
        t = _pointwise(inputs[i], lin.weight, lin.bias)
        outs.append(t if t.shape[2:] == size else F.interpolate(t, size=size, mode="bilinear", align_corners=False))
    return torch.cat(outs, dim=1).contiguous(memory_format=torch.channels_last)


def is_param(k):
    return not k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def head_step(sd, feats, prb, feats_eval, dtype, device="cpu", masks=None, pre=None):
    """One train-mode step (loss = <logits, probe>) and one eval-mode forward of the restatement: every tensor of the capture, whole,
    by name.  `masks`, `pre`: see `forward` (the train-mode pass only)."""
    sd = {k: (v.clone() if k.endswith("num_batches_tracked") else v.to(dtype).clone()).to(device) for k, v in sd.items()}
    for k, v in sd.items():
        if is_param(k):
            v.requires_grad_()
    xs = [f.detach().to(dtype).to(device).clone().requires_grad_() for f in feats]          # (fresh leaves: the caller's tensors stay as they are)
    logits, feat, raw = forward(sd, xs, True, masks=masks, pre=pre)
    (logits * prb.to(dtype).to(device)).sum().backward()
    res = {"logits": logits, "feat": feat, "feat_raw": raw}
    for i, x in enumerate(xs):
        res[f"dc{i + 1}"] = x.grad
    for k, v in sd.items():
        if is_param(k):
            res["g_" + k.replace(".", "_")] = v.grad
        elif not k.endswith("num_batches_tracked"):
            res["b_" + k.replace(".", "_")] = v
    with torch.no_grad():
        res["logits_eval"] = forward(sd, [f.to(dtype).to(device) for f in feats_eval], False)[0]
    return {k: v.detach().double().cpu() for k, v in res.items()}


# ------------------------------------------------------------------------------------------------------------- what the fixture keeps
WHOLE = ("logits", "logits_eval", "dc1", "dc2", "dc3", "dc4")
SAMPLES = {"feat_raw": 2048, "feat": 2048}           # every other tensor: 256 positions (all of it when it is smaller)


def positions(name, numel, count):
    """`count` fixed positions of a tensor of `numel` elements: a multiplicative hash of 0 .. count-1 offset by the name's crc32 (pure
    integer arithmetic: the same on every box)."""
    if numel <= count:
        return torch.arange(numel, dtype=torch.int64)
    k = torch.arange(count, dtype=torch.int64)
    return (k * 2654435761 + (zlib.crc32(name.encode()) & 0x7FFFFFFF)) % numel


def stored(res):
    """The capture's view of a `head_step`-shaped dict of whole float64 tensors: logits, input gradients and the eval-mode logits whole;
    of every other tensor a fixed sample (`<name>_sample`) and its L2 norm (`<name>_norm`)."""
    out = {}
    for k, v in res.items():
        v = v.detach().double().cpu()
        if k in WHOLE:
            out[k] = v
        else:
            flat = v.reshape(-1)
            out[k + "_sample"] = flat[positions(k, flat.numel(), SAMPLES.get(k, 256))].clone()
            out[k + "_norm"] = flat.norm().reshape(())
    return out


# ------------------------------------------------------------------------------------------------------------- depthwise identities
def dw_operands(name):
    """(x, w, dy) of a DW_CASES row on the float16 grid (products of two are exact in fp32), NCHW."""
    n, h, w_, c, d, _, _, _ = DW_CASES[name]
    g = _gen("dw:" + name)
    return (half_grid(torch.randn((n, c, h, w_), generator=g)), half_grid(torch.randn((c, 1, 3, 3), generator=g)),
            half_grid(torch.randn((n, c, h, w_), generator=g)))


def dw_by_taps(x, w9, d, flip=False):
    """The entry point's definition, tap by tap: x [N,C,H,W], w9 [9][C] -> y; a tap outside the map contributes zero."""
    n, c, h, w_ = x.shape
    xp = F.pad(x, (d, d, d, d))
    y = torch.zeros_like(x)
    for t in range(9):
        r, s = divmod(t, 3)
        y = y + w9[8 - t if flip else t][None, :, None, None] * xp[:, :, r * d:r * d + h, s * d:s * d + w_]
    return y


def dw_wgrad_by_taps(dy, x, d):
    """dw9[t][c] = sum over the pixels of dy[p, c] * x[p + off_t, c]."""
    n, c, h, w_ = x.shape
    xp = F.pad(x, (d, d, d, d))
    return torch.stack([(dy * xp[:, :, (t // 3) * d:(t // 3) * d + h, (t % 3) * d:(t % 3) * d + w_]).sum(dim=(0, 2, 3)) for t in range(9)])


def tap_major(w):
    return w.reshape(w.shape[0], 9).t().contiguous()
