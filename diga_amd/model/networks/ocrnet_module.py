"""Object-contextual representations head on the HIP kernels -- host mirror of the semi-supervised tree's
semi-supervised_segmentation/model/networks/ocrnet_module.py:12-247 (`ORegionModule`, `PixelRegionRelationModule`, `OCRNet`).

Same constructor arguments (`config['OCRNET_MODEL']`: RAW_IN_CHANNELS, PIXEL_REP_CHANNELS, KEY_CHANNELS, NUM_CLASSES), same state-dict
keys (the `nn.Sequential` index names `pixel_representations.0.weight` ... `segmentation_classes.0.bias`, BatchNorm buffers included),
same result `(soft_obj_reg, seg_classes, augmented_feats)`.  The HRNet backbone in front of it is not part of this module: it takes the
backbone's feature map.

What runs where:
  * convolutions are DigaConv2d, BatchNorms DigaTrainableBatchNorm2d with the ReLU fused (the `nn.ReLU` members stay in the
    Sequentials for their index names and are skipped); the key and value stacks run on the [N, C, K, 1] region tensor;
  * the two attention-shaped operations are csrc/ocr.hip, exact fp32 whatever conv_math is:
      ocr_region_gather(x [N,P,C], s [N,P,K])          -> [N,K,C]   softmax over the pixels of every class map, then s^T x (:24-44)
      ocr_object_attention(q [N,P,D], key, val, scale) -> [N,P,Dv]  K-way softmax of scale q key^T per pixel, then attn val (:77-95, :231)
    Both are module-level callables looked up at call time (a test substitutes a torch composition for either).  They save what
    their backward kernels read and nothing else; under no_grad (the teacher's pass) nothing is saved and no [N,P,K] attention
    map is kept (FUSED_ATTENTION_NO_GRAD below: that pass takes the torch composition for the attention, the one form that measured
    faster than its kernel);
  * `torch.cat([ocr_rep, pixel_rep])` (:238) is not formed by a copy: the BatchNorms of `ocr_up` and `pixel_representations` write
    their results into the two channel halves of one NHWC buffer (as the ASPP head's GroupNorms do) and `augmented_rep` reads the
    buffer.  The pixel half is read in place by the region-gather kernel (a pitched operand); the query convolution takes a dense
    input outside the bf16x6 loader path and copies that half once.
"""
import os
import sys

import torch
import torch.nn as nn

_pkg = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.path.dirname(_pkg) not in sys.path:
    sys.path.append(os.path.dirname(_pkg))
from diga_amd import _lib  # noqa: E402
from diga_amd.model.conv import DigaConv2d  # noqa: E402
from diga_amd.model.norm import DigaTrainableBatchNorm2d, alias_slice, assemble, nhwc  # noqa: E402

K_MAX = 32           # csrc/ocr.hip: run-time class count 1 .. 32
# The one rule about which form runs (profiles/r23_ocr_head.txt, six maps of 128 x 256, alternated pairs): every fused form beat its torch
# composition in every pair -- region gather forward 0.25 vs 0.33 ms and forward + backward 0.55 vs 0.58 ms, object attention forward +
# backward 0.585 vs 0.647 ms -- EXCEPT the attention forward that keeps no map (0.196 vs 0.150 ms: the wave-per-pixel kernel is bound by
# its LDS reads and cross-lane sums, not by HBM).  So a pass that will not be differentiated takes the composition for the attention;
# True makes it take the kernel (attn = NULL) as well.
FUSED_ATTENTION_NO_GRAD = False


def _rows(t, quad):
    """([N, P, C] fp32 tensor the kernels can read, pitch in floats): `t` itself when its rows are a dense enumeration of rows of a
    wider matrix (unit channel stride; for the channel tensors, `quad`, pitch % 4 == 0 and a 16-byte aligned base), else a copy."""
    if t.dtype != torch.float32:
        t = t.float()
    n, p, c = t.shape
    if t.is_contiguous():
        return t, c
    ld = t.stride(1)
    ok = t.stride(2) == 1 and ld >= c and t.stride(0) == p * ld and (not quad or (ld % 4 == 0 and t.data_ptr() % 16 == 0))
    return (t, ld) if ok else (t.contiguous(), c)


def _workspace(n, p, k, c, device):
    nbytes = _lib.lib.diga_ocr_workspace_bytes(n, p, k, c)
    if nbytes == 0:
        raise ValueError(f"OCR kernels: unsupported shape N={n} P={p} K={k} (1 .. {K_MAX}) C={c} (multiple of 4, <= 1024)")
    return _lib.workspace(nbytes, device, "ocr")


class _RegionGatherFn(torch.autograd.Function):
    """region[n, k, :] = sum_p softmax_p(s[n, :, k])[p] x[n, p, :].  Saved: x, s (views, no copies), `stat` (the softmax statistics
    and what the fp32 rounding of the result dropped, [N, K, C + 2] floats) and the result."""

    @staticmethod
    def forward(ctx, x, s):
        _lib.require_gpu(x, s)
        xr, ld_x = _rows(x.detach(), True)
        sr, ld_s = _rows(s.detach(), False)
        n, p, c = xr.shape
        k = sr.shape[2]
        region = torch.empty((n, k, c), dtype=torch.float32, device=xr.device)
        stat = torch.empty(n * k * (c + 2), dtype=torch.float32, device=xr.device)      # low-order part of region, then (max, 1 / sum)
        ws = _workspace(n, p, k, c, xr.device)
        _lib.call("diga_ocr_region_fwd", _lib.ptr(xr), ld_x, _lib.ptr(sr), ld_s, _lib.ptr(region), _lib.ptr(stat), n, p, k, c,
                  _lib.ptr(ws), ws.numel(), _lib.stream())
        ctx.save_for_backward(xr, sr, stat, region)
        ctx.lds = (ld_x, ld_s)
        return region

    @staticmethod
    def backward(ctx, g):
        xr, sr, stat, region = ctx.saved_tensors
        ld_x, ld_s = ctx.lds
        n, p, c = xr.shape
        k = sr.shape[2]
        g = g.float().contiguous()
        dx = torch.empty((n, p, c), dtype=torch.float32, device=xr.device)
        ds = torch.empty((n, p, k), dtype=torch.float32, device=xr.device)
        _lib.call("diga_ocr_region_bwd", _lib.ptr(xr), ld_x, _lib.ptr(sr), ld_s, _lib.ptr(stat), _lib.ptr(region), _lib.ptr(g),
                  _lib.ptr(dx), c, _lib.ptr(ds), k, n, p, k, c, _lib.stream())
        return dx, ds


def _attend_forward(q, key, val, scale, keep_attn):
    qr, ld_q = _rows(q, True)
    key, val = key.float().contiguous(), val.float().contiguous()
    n, p, d = qr.shape
    k, dv = key.shape[1], val.shape[2]
    if key.shape != (n, k, d) or val.shape[:2] != (n, k):
        raise ValueError(f"ocr_object_attention: q {tuple(q.shape)}, key {tuple(key.shape)}, val {tuple(val.shape)} do not fit")
    out = torch.empty((n, p, dv), dtype=torch.float32, device=qr.device)
    attn = torch.empty((n, p, k), dtype=torch.float32, device=qr.device) if keep_attn else None
    _lib.call("diga_ocr_attend_fwd", _lib.ptr(qr), ld_q, _lib.ptr(key), _lib.ptr(val), _lib.ptr(out), dv, _lib.ptr(attn), n, p, k, d,
              dv, float(scale), _lib.stream())
    return qr, ld_q, key, val, out, attn


class _ObjectAttentionFn(torch.autograd.Function):
    """out = softmax_k(scale q key^T) val.  `keep_attn` (decided by ocr_object_attention: grad mode on and an input that requires
    grad) makes the kernel write the [N, P, K] map the backward reads; saved then: q (a view), key, val, attn."""

    @staticmethod
    def forward(ctx, q, key, val, scale, keep_attn):
        _lib.require_gpu(q, key, val)
        qr, ld_q, k_, v_, out, attn = _attend_forward(q.detach(), key.detach(), val.detach(), scale, keep_attn)
        if keep_attn:
            ctx.save_for_backward(qr, k_, v_, attn)
        ctx.ld_q, ctx.scale = ld_q, float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.saved_tensors:
            raise RuntimeError("ocr_object_attention: backward through a forward pass that kept no attention map")
        qr, key, val, attn = ctx.saved_tensors
        n, p, d = qr.shape
        k, dv = key.shape[1], val.shape[2]
        gr, ld_g = _rows(g, True)
        dq = torch.empty((n, p, d), dtype=torch.float32, device=qr.device)
        d_key, d_val = torch.empty_like(key), torch.empty_like(val)
        ws = _workspace(n, p, k, max(d, dv), qr.device)
        _lib.call("diga_ocr_attend_bwd", _lib.ptr(qr), ctx.ld_q, _lib.ptr(key), _lib.ptr(val), _lib.ptr(attn), _lib.ptr(gr), ld_g,
                  _lib.ptr(dq), d, _lib.ptr(d_key), _lib.ptr(d_val), n, p, k, d, dv, ctx.scale, _lib.ptr(ws), ws.numel(), _lib.stream())
        return dq, d_key, d_val, None, None


def ocr_region_gather(x, s):
    """x [N, P, C] pixel representations (rows may be a channel slice of a wider buffer), s [N, P, K] soft-region logits ->
    [N, K, C] object region representations."""
    return _RegionGatherFn.apply(x, s)


def ocr_object_attention(q, key, val, scale):
    """q [N, P, D], key [N, K, D], val [N, K, Dv] -> [N, P, Dv]."""
    keep = torch.is_grad_enabled() and (q.requires_grad or key.requires_grad or val.requires_grad)
    if not keep and not FUSED_ATTENTION_NO_GRAD:
        _lib.require_gpu(q, key, val)
        return torch.matmul(torch.softmax(scale * torch.matmul(q, key.transpose(1, 2)), dim=2), val)
    return _ObjectAttentionFn.apply(q, key, val, scale, keep)


def _run(seq, x):
    """An nn.Sequential of the reference's layout with every BatchNorm + ReLU pair as one kernel."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, DigaTrainableBatchNorm2d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = m(x, relu=relu)
            i += 2 if relu else 1
        else:
            x = m(x)
            i += 1
    return x


def _conv_bn_relu(cin, cout, kernel_size=1, padding=0, bias=False, inplace=False):
    return [DigaConv2d(cin, cout, kernel_size=kernel_size, stride=1, padding=padding, bias=bias), DigaTrainableBatchNorm2d(cout),
            nn.ReLU(inplace=inplace)]


class ORegionModule(nn.Module):
    """Object region representations (:12-44): pixel representations [N, C, H, W] weighted by the soft object regions [N, K, H, W]
    normalised over the pixels -> [N, C, K, 1]."""

    def __init__(self, num_classes=0):
        super().__init__()
        self.num_classe = num_classes          # (the reference's spelling)

    def forward(self, pixel_representations, soft_object_regions):
        n, k, h, w = soft_object_regions.shape
        c = pixel_representations.shape[1]
        x = pixel_representations.permute(0, 2, 3, 1).reshape(n, h * w, c)      # a view for an NHWC buffer or a channel slice of one
        s = nhwc(soft_object_regions).view(n, h * w, k)
        region = ocr_region_gather(x, s)
        return region.view(n, k, 1, c).permute(0, 3, 1, 2)


class PixelRegionRelationModule(nn.Module):
    """Pixel-region relation (:48-95): query stack on the pixel representations, key stack on the region tensor, softmax over the
    classes of key_channels^-0.5 q key^T."""

    def __init__(self, in_channels, key_channels, bn_type=None):
        super().__init__()
        self.in_channels, self.key_channels = in_channels, key_channels
        self.pixel_rep = self._apply_conv(in_channels, key_channels)
        self.obj_reg_rep = self._apply_conv(in_channels, key_channels)

    def _apply_conv(self, in_channels, out_channels):
        return nn.Sequential(*_conv_bn_relu(in_channels, out_channels), *_conv_bn_relu(out_channels, out_channels))

    def query_key(self, pixel_rep, object_reg_rep):
        """(q [N, P, D], key [N, K, D]): the operands of ocr_object_attention."""
        n, _, h, w = pixel_rep.shape
        d = self.key_channels
        q = nhwc(_run(self.pixel_rep, pixel_rep)).view(n, h * w, d)
        key = nhwc(_run(self.obj_reg_rep, object_reg_rep)).view(n, -1, d)
        return q, key

    def forward(self, pixel_rep, object_reg_rep):
        """The [N, P, K] relation itself, as the reference returns it.  OCRNet.forward does not come through here (it never forms the
        map under no_grad and differentiates the fused operation).  Differentiable like the reference's: when a gradient can reach
        it, it is the torch composition (the attention backward kernel has no gradient input for the map); otherwise the kernel
        writes it."""
        q, key = self.query_key(pixel_rep, object_reg_rep)
        scale = self.key_channels ** -.5
        if torch.is_grad_enabled() and (q.requires_grad or key.requires_grad):
            return torch.softmax(scale * torch.matmul(q, key.transpose(1, 2)), dim=2)
        return _attend_forward(q, key, key, scale, True)[5]           # (the kernel's `out` is not used: val = key)


class OCRNet(nn.Module):
    """OCR head (:103-247).  Input: the backbone's feature map [N, RAW_IN_CHANNELS, h, w]; output: the soft object regions (auxiliary
    logits), the pixel-wise segmentation logits, the augmented features."""

    def __init__(self, config, **kwargs):
        super().__init__()
        self.ocrnet_config = config['OCRNET_MODEL']
        self.in_channels = self.ocrnet_config['RAW_IN_CHANNELS']
        self.num_classes = self.ocrnet_config['NUM_CLASSES']
        self.pix_rep_channels = self.ocrnet_config['PIXEL_REP_CHANNELS']
        self.key_channels = self.ocrnet_config['KEY_CHANNELS']
        if not 1 <= self.num_classes <= K_MAX or self.pix_rep_channels % 4 or self.key_channels % 4:
            raise NotImplementedError(f"OCRNet: 1 .. {K_MAX} classes, channel counts that are multiples of 4")
        cin, c, dk, k = self.in_channels, self.pix_rep_channels, self.key_channels, self.num_classes
        self.pixel_representations = nn.Sequential(*_conv_bn_relu(cin, c, kernel_size=3, padding=1, bias=True, inplace=True))
        self.soft_object_regions = nn.Sequential(*_conv_bn_relu(cin, cin, bias=True, inplace=True),
                                                 DigaConv2d(cin, k, kernel_size=1, stride=1, padding=0, bias=True))
        self.obj_region_representations = ORegionModule(k)
        self.pixel_region_relations = PixelRegionRelationModule(c, dk)
        self.value = nn.Sequential(*_conv_bn_relu(c, dk))
        self.ocr_up = nn.Sequential(*_conv_bn_relu(dk, c))
        self.augmented_rep = nn.Sequential(*_conv_bn_relu(2 * c, c), nn.Dropout2d(0.05))
        self.segmentation_classes = nn.Sequential(DigaConv2d(c, k, kernel_size=1, stride=1, padding=0, bias=True))
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def forward(self, raw_backbone_feats):
        _lib.require_gpu(raw_backbone_feats)
        n, _, h, w = raw_backbone_feats.shape
        c, dk, k = self.pix_rep_channels, self.key_channels, self.num_classes
        soft_obj_reg = _run(self.soft_object_regions, raw_backbone_feats)
        # [ocr_rep | pixel_rep]: the concatenation's buffer, filled by the two BatchNorms
        cat = torch.empty((n, h, w, 2 * c), dtype=torch.float32, device=raw_backbone_feats.device)
        conv, bn = self.pixel_representations[0], self.pixel_representations[1]
        pixel_rep = bn(conv(raw_backbone_feats), relu=True, out=alias_slice(cat, c, 2 * c))
        obj_reg_rep = self.obj_region_representations(pixel_rep, soft_obj_reg)                  # [N, C, K, 1]
        q, key = self.pixel_region_relations.query_key(pixel_rep, obj_reg_rep)
        val = nhwc(_run(self.value, obj_reg_rep)).view(n, k, dk)
        ocr_rep = ocr_object_attention(q, key, val, dk ** -.5)                                  # [N, P, dk]
        ocr_rep = ocr_rep.view(n, h, w, dk).permute(0, 3, 1, 2)
        conv, bn = self.ocr_up[0], self.ocr_up[1]
        ocr_rep = bn(conv(ocr_rep), relu=True, out=alias_slice(cat, 0, c))
        augmented_feats = _run(self.augmented_rep, assemble(cat, c, [ocr_rep, pixel_rep]))
        seg_classes = self.segmentation_classes(augmented_feats)
        return soft_obj_reg, seg_classes, augmented_feats
