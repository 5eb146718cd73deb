"""DAFormer decode head on the HIP kernels -- host mirror of G5/model/networks/segformer_head.py:167-307 (`DAFormerHead`) with its
`ASPPWrapper` / `DepthwiseSeparableASPPModule` (:310-466).  The reference needs mmcv and wires the class into nothing (SURVEY
section 2.1); here `SegFormerStudent(head="daformer")` builds it (diga_amd/model/segformer.py).

Same constructor arguments plus `return_raw`, same state-dict keys with mmcv's block names (`embed_layers.{0..3}.proj.*`,
`fuse_layer.aspp_modules.0.{conv,bn}.*`, `fuse_layer.aspp_modules.{1,2,3}.{depthwise_conv,pointwise_conv}.{conv,bn}.*`,
`fuse_layer.bottleneck.{conv,bn}.*`, `conv_seg.*`), same result: per stage a Linear embedding to 256 channels, bilinear resize
(align_corners=False) to the first stage's grid, concatenation in `in_index` order [c1, c2, c3, c4] (NOT the SegFormer head's reversed
order), a separable ASPP (1x1 branch + three depthwise-3x3 / 1x1 branches at dilations 6, 12, 18, each conv -> BatchNorm -> ReLU), a 3x3
bottleneck conv -> BatchNorm -> ReLU, Dropout2d, the 1x1 `conv_seg`.

What runs where.  Unlike the SegFormer head's 1x1 fuse conv, an ASPP does not commute with the resize: the 1024-channel concatenation
is read by five convolutions and is formed -- without F.interpolate and torch.cat.  Each stage is embedded on its OWN grid (`_pointwise`,
as segformer_head's `MLP`) and diga_pyramid_resize_fwd writes the resized map straight into its channel slice of one NHWC buffer
`feat_raw`.  Stage 0 is the exception the issue's text did not want: its embedding is a dense tensor that the same kernel COPIES into
slice 0 (equal grids: a plain copy, one more read and write of a quarter of the buffer, forward and backward) -- the implicit-GEMM
autograd function has no pitched output, and that is not built here.  The depthwise convs are
diga_dwconv3x3_f32 (csrc/dwconv.hip; forward, backward-data = the same kernel on reversed taps, weight gradient with per-block
partials): exact fp32 under every conv_math, logged in conv.path_log as arithmetic "f32/dw".  The BatchNorms behind the four branches
write into the four slices of a second concat buffer (`out=`), gradients are routed by norm.assemble / alias_slice as in
`Classifier_Module2` and the OCR head.  Every other conv is a DigaConv2d under the arithmetic the process selected.

Not built (each raises NotImplementedError): align_corners=True, `pool=True`, a context layer, the `sep_conv` / `conv` /
`rawconv_and_aspp` embed types, norm layers other than BN / SyncBN with trainable affine, activations other than ReLU / none.  The
BatchNorm behind a depthwise conv runs its own statistics pass.
"""
import os
import sys

import torch
import torch.nn as nn

_pkg = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.path.dirname(_pkg) not in sys.path:
    sys.path.append(os.path.dirname(_pkg))
from diga_amd import _lib  # noqa: E402
from diga_amd.model import conv as _conv  # noqa: E402
from diga_amd.model.conv import INLINE_WGRAD, DigaConv2d, _Call, _Conv2dFn  # noqa: E402
from diga_amd.model.norm import DigaTrainableBatchNorm2d, alias_slice, as_rows, assemble, nhwc, rows_ld  # noqa: E402

BUILT = ("DAFormerHead builds: four stages (input_transform='multiple_select'), 'mlp' embeddings, the 'aspp' fusion with sep=True, "
         "pool=False and no context layer, BN / SyncBN with trainable affine, ReLU or no activation, align_corners=False")
# torch on channels-last tensors in place of a kernel that lost to it in every measured pair (profiles/r26_daformer.txt); none did
USE_TORCH_DEPTHWISE = False


# (This module imports nothing from segformer_head.py, which re-exports its classes: the two restate these few lines instead of
#  importing each other.)
def _pointwise(x, w2d, bias=None):
    """1x1 convolution of an NCHW-shaped tensor with a [Cout, Cin] matrix on the implicit-GEMM kernels (segformer_head._pointwise)."""
    return _Conv2dFn.apply(x, w2d[:, :, None, None], bias, _Call(uses=INLINE_WGRAD))


class MLP(nn.Module):
    """Linear Embedding (segformer_head.py:12-22); the head applies `proj` as a 1x1 conv on the stage's own NHWC map."""

    def __init__(self, input_dim=2048, embed_dim=768):
        super().__init__()
        self.proj = nn.Linear(input_dim, embed_dim)

    def forward(self, x):
        return _pointwise(x, self.proj.weight, self.proj.bias).flatten(2).transpose(1, 2)


def _tap_major(weight):
    """[C, 1, 3, 3] parameter -> the kernel's [9][C] image (made per call: 36 KB at the head's width)."""
    return weight.detach().float().reshape(weight.shape[0], 9).t().contiguous()


class _DepthwiseFn(torch.autograd.Function):
    """y = depthwise 3x3 conv of x (NCHW-shaped over NHWC memory, dense or a channel slice), stride 1, padding = dilation.  Saved: x
    (a view, no copy) and the weight.  Backward: diga_dwconv3x3_f32(flip=1) on dy, diga_dwconv3x3_f32_wgrad."""

    @staticmethod
    def forward(ctx, x, weight, dilation):
        _lib.require_gpu(x, weight)
        xn = x.detach().permute(0, 2, 3, 1)
        if xn.dtype != torch.float32:
            xn = xn.float()
        xn, ld_x = as_rows(xn)
        n, h, w, c = xn.shape
        if tuple(weight.shape) != (c, 1, 3, 3) or c % 4:
            raise ValueError(f"depthwise 3x3: weight {tuple(weight.shape)} for {c} channels (a multiple of 4)")
        y = torch.empty((n, h, w, c), dtype=torch.float32, device=xn.device)
        _lib.call("diga_dwconv3x3_f32", _lib.ptr(xn), ld_x, _lib.ptr(_tap_major(weight)), _lib.ptr(y), c, n, h, w, c, int(dilation), 0,
                  _lib.stream())
        _conv._log_path("fwd", "f32/dw")
        ctx.save_for_backward(xn, weight)
        ctx.geom = (ld_x, int(dilation))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        xn, weight = ctx.saved_tensors
        ld_x, d = ctx.geom
        n, h, w, c = xn.shape
        g = gy.permute(0, 2, 3, 1)
        if g.dtype != torch.float32:
            g = g.float()
        g, ld_g = as_rows(g)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dxn = torch.empty((n, h, w, c), dtype=torch.float32, device=xn.device)
            _lib.call("diga_dwconv3x3_f32", _lib.ptr(g), ld_g, _lib.ptr(_tap_major(weight)), _lib.ptr(dxn), c, n, h, w, c, d, 1, _lib.stream())
            _conv._log_path("dgrad", "f32/dw")
            dx = dxn.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            ws = _lib.workspace(_lib.lib.diga_dwconv3x3_wgrad_workspace_bytes(n, h, w, c), xn.device, "dwconv")
            dw9 = torch.empty((9, c), dtype=torch.float32, device=xn.device)
            _lib.call("diga_dwconv3x3_f32_wgrad", _lib.ptr(g), ld_g, _lib.ptr(xn), ld_x, _lib.ptr(dw9), _lib.ptr(ws), ws.numel(), n, h, w, c, d,
                      _lib.stream())
            _conv._log_path("wgrad", "f32/dw")
            dw = dw9.t().reshape(c, 1, 3, 3).contiguous()
        return dx, dw, None


def depthwise_conv3x3(x, weight, dilation):
    """x [N, C, H, W] (NHWC memory), weight [C, 1, 3, 3] -> [N, C, H, W]; stride 1, padding = dilation."""
    if USE_TORCH_DEPTHWISE:
        _lib.require_gpu(x, weight)
        return torch.nn.functional.conv2d(x, weight, None, 1, dilation, dilation, weight.shape[0])
    return _DepthwiseFn.apply(x, weight, dilation)


class _ResizeIntoFn(torch.autograd.Function):
    """`out` (a channel slice of the concat buffer, norm.alias_slice) = bilinear resize of `src` to out's grid; returns out as an
    NCHW-shaped tensor.  Backward: the exact adjoint on the pitched slice of the buffer's gradient."""

    @staticmethod
    def forward(ctx, src, out):
        _lib.require_gpu(src, out)
        s = nhwc(src.detach())
        n, h, w, c = s.shape
        ld = rows_ld(out)
        if ld is None or out.shape[0] != n or out.shape[3] != c or out.dtype != torch.float32:
            raise ValueError("resize into a slice: a channel slice of a contiguous NHWC fp32 buffer of the source's batch and channel count")
        _lib.call("diga_pyramid_resize_fwd", _lib.ptr(s), h, w, _lib.ptr(out), ld, out.shape[1], out.shape[2], n, c, _lib.stream())
        ctx.shape = (n, h, w, c)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.shape
        gn = g.permute(0, 2, 3, 1)
        if gn.dtype != torch.float32:
            gn = gn.float()
        gn, ld = as_rows(gn)
        ds = torch.empty((n, h, w, c), dtype=torch.float32, device=gn.device)
        _lib.call("diga_pyramid_resize_bwd", _lib.ptr(gn), ld, gn.shape[1], gn.shape[2], _lib.ptr(ds), h, w, n, c, _lib.stream())
        return ds.permute(0, 3, 1, 2), None


def _check_cfgs(norm_cfg, act_cfg):
    if norm_cfg is None or norm_cfg.get("type") not in ("BN", "SyncBN") or not norm_cfg.get("requires_grad", True):
        raise NotImplementedError(f"norm_cfg={norm_cfg!r}. {BUILT}")
    if act_cfg is not None and act_cfg.get("type") != "ReLU":
        raise NotImplementedError(f"act_cfg={act_cfg!r}. {BUILT}")


class _DepthwiseConv3x3(nn.Module):
    """The `conv` of a depthwise mmcv block: an nn.Conv2d(C, C, 3, padding=d, dilation=d, groups=C, bias=False)'s one parameter, in
    its shape [C, 1, 3, 3]."""

    def __init__(self, channels, dilation):
        super().__init__()
        self.in_channels = self.out_channels = self.groups = channels
        self.kernel_size, self.stride, self.padding, self.dilation = (3, 3), (1, 1), (dilation, dilation), (dilation, dilation)
        self.weight = nn.Parameter(torch.empty(channels, 1, 3, 3))
        self.bias = None

    def forward(self, x):
        return depthwise_conv3x3(x, self.weight, self.dilation[0])


class DAConvModule(nn.Module):
    """mmcv's ConvModule as the ASPP uses it: conv without bias (bias='auto' is off when a norm follows) -> BatchNorm2d with trainable
    affine -> ReLU or nothing; attributes `conv`, `bn`, `activate`.  kernel 1, kernel 3 (padding = dilation) or the depthwise 3x3
    (groups == in_channels == out_channels).  `segformer_head.ConvModule` is the 1x1 + ReLU special case and stays as it is."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, dilation=1, groups=1, norm_cfg=None, act_cfg=dict(type='ReLU')):
        super().__init__()
        _check_cfgs(norm_cfg, act_cfg)
        if groups == 1:
            self.conv = DigaConv2d(in_channels, out_channels, kernel_size, padding=padding, dilation=dilation, bias=False)
        elif groups == in_channels == out_channels and kernel_size == 3 and padding == dilation:
            self.conv = _DepthwiseConv3x3(in_channels, dilation)
        else:
            raise NotImplementedError("DAConvModule: groups=1, or the depthwise 3x3 with padding = dilation")
        self.bn = DigaTrainableBatchNorm2d(out_channels)
        self.relu = act_cfg is not None
        if self.relu:
            self.activate = nn.ReLU(inplace=True)
        self.init_weights()

    def init_weights(self):
        """As mmcv 1.x's ConvModule does in its constructor (see segformer_head.ConvModule.init_weights): kaiming NORMAL, mode fan_out,
        nonlinearity 'relu' whatever the activation (only LeakyReLU changes it); BatchNorm weight 1, bias 0."""
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.bn.weight, 1.0)
        nn.init.constant_(self.bn.bias, 0.0)

    def forward(self, x, out=None):
        return self.bn(self.conv(x), relu=self.relu, out=out)


class DepthwiseSeparableConvModule(nn.Module):
    """mmcv's block of the same name: `depthwise_conv` = ConvModule(in, in, 3, groups=in) then `pointwise_conv` = ConvModule(in, out, 1),
    both with the block's norm_cfg and act_cfg."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, dilation=1, norm_cfg=None, act_cfg=dict(type='ReLU')):
        super().__init__()
        self.depthwise_conv = DAConvModule(in_channels, in_channels, kernel_size, padding=padding, dilation=dilation, groups=in_channels,
                                           norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.pointwise_conv = DAConvModule(in_channels, out_channels, 1, norm_cfg=norm_cfg, act_cfg=act_cfg)

    def forward(self, x, out=None):
        return self.pointwise_conv(self.depthwise_conv(x), out=out)


class ASPPWrapper(nn.Module):
    """segformer_head.py:310-373 with sep=True, pool=False, no context layer: `aspp_modules` (a 1x1 block for dilation 1, a separable
    block per further dilation) and the 3x3 `bottleneck` on their concatenation."""

    def __init__(self, in_channels, channels, sep, dilations, pool, norm_cfg, act_cfg, align_corners, context_cfg=None):
        super().__init__()
        if not sep or pool or context_cfg is not None or align_corners:
            raise NotImplementedError(f"ASPPWrapper(sep={sep}, pool={pool}, context_cfg={context_cfg}, align_corners={align_corners}). {BUILT}")
        assert isinstance(dilations, (list, tuple))
        self.dilations, self.align_corners, self.channels = tuple(dilations), align_corners, channels
        self.image_pool = self.context_layer = None
        mods = []
        for d in self.dilations:
            if d == 1:
                mods.append(DAConvModule(in_channels, channels, 1, norm_cfg=norm_cfg, act_cfg=act_cfg))
            else:
                mods.append(DepthwiseSeparableConvModule(in_channels, channels, 3, padding=d, dilation=d, norm_cfg=norm_cfg, act_cfg=act_cfg))
        self.aspp_modules = nn.ModuleList(mods)
        self.bottleneck = DAConvModule(len(self.dilations) * channels, channels, 3, padding=1, norm_cfg=norm_cfg, act_cfg=act_cfg)

    def forward(self, x):
        n, _, h, w = x.shape
        ch = self.channels
        cat = torch.empty((n, h, w, len(self.dilations) * ch), dtype=torch.float32, device=x.device)
        outs = [m(x, out=alias_slice(cat, k * ch, (k + 1) * ch)) for k, m in enumerate(self.aspp_modules)]
        return self.bottleneck(assemble(cat, ch, outs))


class DAFormerHead(nn.Module):
    """DAFormer: Improving Network Architectures and Training Strategies for Domain-Adaptive Semantic Segmentation, the decode head
    (segformer_head.py:167-307)."""

    def __init__(self, in_channels=None, channels=None, feature_strides=None, num_classes=None, in_index=None, act_cfg=None,
                 dropout_ratio=None, conv_cfg=None, norm_cfg=None, input_transform='multiple_select', align_corners=False,
                 return_raw=False, decoder_params=None):
        super().__init__()
        assert len(feature_strides) == len(in_channels)
        assert min(feature_strides) == feature_strides[0]
        assert isinstance(in_channels, (list, tuple)) and isinstance(in_index, (list, tuple)) and len(in_channels) == len(in_index)
        if input_transform != 'multiple_select' or len(in_channels) != 4:
            raise NotImplementedError(f"input_transform={input_transform!r} on {len(in_channels)} inputs. {BUILT}")
        if align_corners:
            raise NotImplementedError(f"align_corners=True. {BUILT}")
        if conv_cfg is not None:
            raise NotImplementedError(f"conv_cfg={conv_cfg!r}. {BUILT}")
        _check_cfgs(norm_cfg, act_cfg)
        self.in_channels, self.in_index, self.input_transform = list(in_channels), list(in_index), input_transform
        self.channels, self.num_classes, self.dropout_ratio = channels, num_classes, dropout_ratio
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        self.align_corners, self.feature_strides = align_corners, feature_strides
        self.return_raw = bool(return_raw)
        # the reference hard-codes these (:189-201); `decoder_params` overrides are checked against what is built
        params = dict(embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None), embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                      fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False, act_cfg=act_cfg, norm_cfg=norm_cfg),
                      embed_dim=256, conv_kernel_size=1)
        params.update(decoder_params or {})
        for key in ("embed_cfg", "embed_neck_cfg"):
            if params[key].get("type") != "mlp":
                raise NotImplementedError(f"{key} type {params[key].get('type')!r}. {BUILT}")
        fusion = dict(params["fusion_cfg"])
        if fusion.pop("type", None) != "aspp":
            raise NotImplementedError(f"fusion_cfg type {params['fusion_cfg'].get('type')!r}. {BUILT}")
        if params["conv_kernel_size"] != 1 or not isinstance(params["embed_dim"], int) or params["embed_dim"] % 4:
            raise NotImplementedError(f"conv_kernel_size=1 and one embed_dim that is a multiple of 4. {BUILT}")
        self.embedding_dim = e = params["embed_dim"]
        fusion.setdefault("align_corners", align_corners)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio and dropout_ratio > 0 else None
        self.embed_layers = nn.ModuleDict({str(i): MLP(input_dim=c, embed_dim=e) for i, c in zip(self.in_index, self.in_channels)})
        self.fuse_layer = ASPPWrapper(in_channels=4 * e, channels=channels, **fusion)
        self.conv_seg = DigaConv2d(channels, num_classes, kernel_size=1)

    def init_weights(self):
        """Initialize weights of classification layer (:270-272, mmcv normal_init: weight N(0, 0.01), bias 0)."""
        nn.init.normal_(self.conv_seg.weight, mean=0, std=0.01)
        if self.conv_seg.bias is not None:
            nn.init.constant_(self.conv_seg.bias, 0)

    def cls_seg(self, feat):
        if self.dropout is not None:
            feat = self.dropout(feat)
        return self.conv_seg(feat)

    def raw_features(self, inputs):
        """`feat_raw` (:287-303): [N, 4E, H, W] as an NCHW view of the one NHWC buffer the embeddings are resized into."""
        x = inputs
        _lib.require_gpu(x[self.in_index[0]])
        n, _, hh, ww = x[self.in_index[0]].shape
        e = self.embedding_dim
        raw = torch.empty((n, hh, ww, 4 * e), dtype=torch.float32, device=x[self.in_index[0]].device)
        slices = []
        for k, i in enumerate(self.in_index):
            lin = self.embed_layers[str(i)].proj
            emb = _pointwise(x[i], lin.weight, lin.bias)          # on the stage's own grid
            slices.append(_ResizeIntoFn.apply(emb, alias_slice(raw, k * e, (k + 1) * e)))
        return assemble(raw, e, slices)

    def forward(self, inputs):
        feat_raw = self.raw_features(inputs)
        feat = self.fuse_layer(feat_raw)
        x = self.cls_seg(feat)
        return x, (feat_raw if self.return_raw else feat)

