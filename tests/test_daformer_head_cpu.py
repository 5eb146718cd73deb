"""DAFormer decode head (diga_amd/model/networks/daformer_head.py, csrc/dwconv.hip, the resize kernels of csrc/pyramid.hip), the part
that needs no device: the restatement the GPU tests lean on against the capture of the reference class, the depthwise identities in
float64, the five exports and their argument rules, the module's state dict and its refusals, the student's wiring."""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_entry_check_cases as cc
import daformer_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(autouse=True)
def _leave_the_global_generator_alone():
    """Module constructors and torch.manual_seed draw from / reset torch's global generator, which tests elsewhere initialise layers
    from: every test of this file hands its state back as it found it."""
    with torch.random.fork_rng(devices=[]):
        yield


EXPORTS = {"diga_dwconv3x3_f32": ("int", 12), "diga_dwconv3x3_wgrad_workspace_bytes": ("size_t", 4), "diga_dwconv3x3_f32_wgrad": ("int", 13),
           "diga_pyramid_resize_fwd": ("int", 10), "diga_pyramid_resize_bwd": ("int", 10)}


# ---- (i) the restatement against the capture
def test_fixture_inputs_are_the_helper_s(golden):
    """The fixture stores no weight and no input: `state` and `inputs` must give the tensors the capture ran on."""
    z = golden("daformer_head")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "daformer_head.npz")) < 1000000
    sd = dc.state()
    got = dc.checksum([v for k, v in sd.items() if not k.endswith("num_batches_tracked")])
    assert abs(got - float(z["state_sum"])) <= 1e-12 * abs(float(z["state_sum"]))
    feats, feats_eval = dc.inputs(), dc.inputs(dc.GRIDS_EVAL, n=1, tag="eval")
    prb = dc.probe((dc.BATCH, dc.CLASSES) + dc.GRIDS[0])
    got = dc.checksum(feats + feats_eval + [prb])
    assert abs(got - float(z["inputs_sum"])) <= 1e-12 * abs(float(z["inputs_sum"]))


def test_restatement_reproduces_the_capture_in_float64(golden):
    """Same operations in float64, the concatenations formed and the Linear embeddings as 1x1 convs: every stored quantity to a
    hundredth of the reference's own fp32 error (floor 1e-12 of scale)."""
    z = golden("daformer_head")
    feats, feats_eval = dc.inputs(), dc.inputs(dc.GRIDS_EVAL, n=1, tag="eval")
    prb = dc.probe((dc.BATCH, dc.CLASSES) + dc.GRIDS[0])
    got = dc.stored(dc.head_step(dc.state(), feats, prb, feats_eval, torch.float64))
    names = [k for k in z if not k.startswith(("scale_", "err32_")) and k not in ("keys", "shapes", "nbt", "state_sum", "inputs_sum")]
    assert sorted(names) == sorted(got) and len(names) == 110
    for k in names:
        want, scale, e32 = z.t(k), float(z["scale_" + k]), float(z["err32_" + k])
        assert want.dtype == torch.float64 and want.shape == got[k].shape and scale > 0 and e32 > 0, k
        err = float((got[k] - want).abs().max()) / scale
        assert err <= max(0.01 * e32, 1e-12), (k, err, e32)
    assert tuple(z["logits"].shape) == (2, 19, 40, 28) and tuple(z["logits_eval"].shape) == (1, 19, 37, 29)


# ---- (ii) the depthwise identities, float64
@pytest.mark.parametrize("name", [n for n in dc.DW_CASES if n != "head_width"] + ["head_width"])
def test_depthwise_definitions_equal_torch_in_float64(name):
    """The entry points' definitions (tap-major [9][C] weights; backward-data = the forward with reversed taps; the weight gradient's
    formula) against F.conv2d(groups=C), conv2d_input and conv2d_weight: 1e-12 of the tensor's scale."""
    n, h, w_, c, d = dc.DW_CASES[name][:5]
    x, w, dy = (t.double() for t in dc.dw_operands(name))
    w9 = dc.tap_major(w)
    for got, ref, what in (
            (dc.dw_by_taps(x, w9, d), F.conv2d(x, w, None, 1, d, d, c), "y"),
            (dc.dw_by_taps(dy, w9, d, flip=True), torch.nn.grad.conv2d_input(x.shape, w, dy, 1, d, d, c), "dx"),
            (dc.dw_wgrad_by_taps(dy, x, d), dc.tap_major(torch.nn.grad.conv2d_weight(x, w.shape, dy, 1, d, d, c)), "dw9")):
        assert got.shape == ref.shape, what
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= 1e-12 * scale, (name, what)
    if name == "centre_only":
        assert torch.equal(dc.dw_by_taps(x, w9, d), w9[4][None, :, None, None] * x)
    if name == "wider_than_map":        # no column tap is in range; of the row taps only 0 <-> 12
        ref = F.conv2d(x, w, None, 1, d, d, c)
        assert torch.equal(ref[:, :, 1:12], (w9[4][None, :, None, None] * x)[:, :, 1:12])
        assert float((ref[:, :, 0] - (w9[4][None, :, None] * x[:, :, 0] + w9[7][None, :, None] * x[:, :, 12])).abs().max()) <= 1e-14 * 10


# ---- (iii) the exports and their rules
def test_exports_are_declared_bound_and_outside_the_recorded_families():
    from diga_amd import _lib
    with open(os.path.join(ROOT, "include", "diga_hip.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    for name, (res, nargs) in EXPORTS.items():
        assert f"{res} {name}(" in header, name
        assert name in doc, f"{name} is not named in INTEGRATION.md"
        r, args = _lib.SIGNATURES[name]
        assert r is (_lib.INT if res == "int" else _lib.SZ) and len(args) == nargs, name
        assert hasattr(_lib.lib, name)
        assert not cc.in_scope(name, res == "int"), name
    assert len(_lib.PROF_TAGS) == 23


# (fake, 16-byte aligned addresses: every call below is rejected before anything could use them)
DW = dict(order=["x", "x_ld", "w9", "y", "y_ld", "N", "H", "W", "C", "d", "flip", "stream"], name="diga_dwconv3x3_f32", who="dwconv3x3: ",
          valid=dict(x=0x100000, x_ld=64, w9=0x800000, y=0x200000, y_ld=64, N=2, H=9, W=7, C=64, d=6, flip=0, stream=0))
WG = dict(order=["dy", "dy_ld", "x", "x_ld", "dw9", "ws", "ws_bytes", "N", "H", "W", "C", "d", "stream"], name="diga_dwconv3x3_f32_wgrad",
          who="dwconv3x3_wgrad: ",
          valid=dict(dy=0x100000, dy_ld=64, x=0x200000, x_ld=64, dw9=0x800000, ws=0x900000, ws_bytes=2 * 3 * 9 * 64 * 4, N=2, H=9, W=7, C=64, d=6,
                     stream=0))
RF = dict(order=["src", "h", "w", "dst", "dst_ld", "H", "W", "N", "C", "stream"], name="diga_pyramid_resize_fwd", who="pyramid_resize_fwd: ",
          valid=dict(src=0x100000, h=5, w=4, dst=0x200000, dst_ld=64, H=10, W=8, N=2, C=16, stream=0))
RB = dict(order=["dout", "dout_ld", "H", "W", "ds", "h", "w", "N", "C", "stream"], name="diga_pyramid_resize_bwd", who="pyramid_resize_bwd: ",
          valid=dict(dout=0x100000, dout_ld=64, H=10, W=8, ds=0x200000, h=5, w=4, N=2, C=16, stream=0))
REJECTED = [
    (DW, "null_x", dict(x=0), "null pointer"),
    (DW, "null_w9", dict(w9=0), "null pointer"),
    (DW, "null_y", dict(y=0), "null pointer"),
    (DW, "align_x", dict(x=0x100004), "16-byte aligned"),
    (DW, "align_w9", dict(w9=0x800008), "16-byte aligned"),
    (DW, "align_y", dict(y=0x20000c), "16-byte aligned"),
    (DW, "c_mod4", dict(C=62), "C=62 must be a multiple of 4"),
    (DW, "x_ld_small", dict(x_ld=60), "bad x_ld"),
    (DW, "x_ld_mod4", dict(x_ld=66), "bad x_ld"),
    (DW, "y_ld_small", dict(y_ld=60), "bad y_ld"),
    (DW, "y_ld_mod4", dict(y_ld=66), "bad y_ld"),
    (DW, "x_ld_2p30", dict(x_ld=1 << 30), "bad x_ld"),
    (DW, "y_ld_2p30", dict(y_ld=1 << 30), "bad y_ld"),
    (DW, "operand_2p49", dict(N=1 << 20, H=1 << 9, W=1 << 20), "beyond 2^44 elements"),
    (DW, "dilation_zero", dict(d=0), "dilation=0 must be >= 1"),
    (DW, "dilation_negative", dict(d=-6), "dilation=-6 must be >= 1"),
    (DW, "flip_two", dict(flip=2), "flip is 0 or 1"),
    (DW, "negative_n", dict(N=-1), "bad shape"),
    (DW, "h_zero", dict(H=0), "bad shape"),
    (DW, "w_2p30", dict(W=1 << 30), "bad shape"),
    (DW, "alias_same", dict(y=0x100000), "must not alias"),
    (DW, "alias_overlap", dict(y=0x100000 + 64 * 4 * 10), "must not alias"),
    (DW, "alias_columns_overlap", dict(x_ld=128, y_ld=128, C=64, y=0x100000 + 32 * 4), "must not alias"),
    (DW, "alias_other_pitch", dict(x_ld=128, y_ld=192, C=64, y=0x100000 + 64 * 4), "must not alias"),
    (WG, "null_dy", dict(dy=0), "null pointer"),
    (WG, "null_x", dict(x=0), "null pointer"),
    (WG, "null_dw9", dict(dw9=0), "null pointer"),
    (WG, "null_ws", dict(ws=0), "null pointer"),
    (WG, "align_dy", dict(dy=0x100004), "16-byte aligned"),
    (WG, "align_x", dict(x=0x200008), "16-byte aligned"),
    (WG, "align_dw9", dict(dw9=0x80000c), "16-byte aligned"),
    (WG, "align_ws", dict(ws=0x900004), "16-byte aligned"),
    (WG, "c_mod4", dict(C=62), "C=62 must be a multiple of 4"),
    (WG, "dy_ld_small", dict(dy_ld=60), "bad dy_ld"),
    (WG, "dy_ld_mod4", dict(dy_ld=66), "bad dy_ld"),
    (WG, "x_ld_small", dict(x_ld=60), "bad x_ld"),
    (WG, "x_ld_mod4", dict(x_ld=66), "bad x_ld"),
    (WG, "dy_ld_2p30", dict(dy_ld=1 << 30), "bad dy_ld"),
    (WG, "x_ld_2p30", dict(x_ld=1 << 30), "bad x_ld"),
    (WG, "dilation_zero", dict(d=0), "dilation=0 must be >= 1"),
    (WG, "n_zero", dict(N=0), "bad shape"),
    (WG, "workspace_short", dict(ws_bytes=2 * 3 * 9 * 64 * 4 - 1), "workspace of 13823 bytes, 13824 needed"),
    (RF, "null_src", dict(src=0), "bad argument"),
    (RF, "c_mod4", dict(C=18), "bad argument"),
    (RF, "align_dst", dict(dst=0x200004), "16-byte aligned"),
    (RF, "dst_ld_small", dict(dst_ld=12), "bad dst_ld"),
    (RF, "dst_ld_mod4", dict(dst_ld=66), "bad dst_ld"),
    (RF, "downsample_h", dict(h=11), "upsampling only"),
    (RF, "downsample_w", dict(w=9), "upsampling only"),
    (RB, "null_ds", dict(ds=0), "bad argument"),
    (RB, "align_dout", dict(dout=0x100008), "16-byte aligned"),
    (RB, "dout_ld_small", dict(dout_ld=12), "bad dout_ld"),
    (RB, "dout_ld_mod4", dict(dout_ld=66), "bad dout_ld"),
    (RB, "downsample_h", dict(h=11), "the adjoint of an upsampling only"),
    (RB, "downsample_w", dict(w=9), "the adjoint of an upsampling only"),
]

needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="host checks only: run where no device is visible")


def _call(_lib, entry, **over):
    vals = dict(entry["valid"], **over)
    rc = getattr(_lib.lib, entry["name"])(*[vals[k] for k in entry["order"]])
    return rc, _lib.last_error()


@needs_no_device
@pytest.mark.parametrize("case", REJECTED, ids=[c[0]["name"][5:] + "-" + c[1] for c in REJECTED])
def test_rule_rejects_with_its_message(case):
    from diga_amd import _lib
    entry, _, over, message = case
    rc, said = _call(_lib, entry, **over)
    assert rc == EINVAL and said.startswith(entry["who"]) and message in said, (rc, said)


@needs_no_device
def test_disjoint_column_windows_of_one_matrix_do_not_alias_and_an_empty_batch_is_ok():
    """N == 0 passes every rule and returns before the launch (no device is visible here: a launch would report an error); with
    x = buf[.., 0:64] and y = buf[.., 64:128] of one 128-wide matrix the byte ranges interleave but no element is shared."""
    from diga_amd import _lib
    assert _call(_lib, DW, N=0)[0] == 0
    assert _call(_lib, DW, N=0, x_ld=128, y_ld=128, y=0x100000 + 64 * 4)[0] == 0


def test_workspace_query():
    from diga_amd import _lib
    q = _lib.lib.diga_dwconv3x3_wgrad_workspace_bytes
    assert q(2, 9, 7, 64) == 2 * 3 * 9 * 64 * 4 and q(16, 192, 192, 1024) == 16 * 48 * 9 * 1024 * 4
    assert q(0, 9, 7, 64) == 0 and q(2, 9, 7, 62) == 0 and q(2, 0, 7, 64) == 0


# ---- (iv) the module
def _head(**over):
    from diga_amd.model.networks.segformer_head import DAFormerHead        # (the reference's import path)
    kw = dict(in_channels=dc.IN_CHANNELS, channels=dc.CHANNELS, feature_strides=[4, 8, 16, 32], num_classes=dc.CLASSES, in_index=[0, 1, 2, 3],
              act_cfg=dict(type="ReLU"), dropout_ratio=0, norm_cfg=dict(type="BN", requires_grad=True), align_corners=False)
    kw.update(over)
    return DAFormerHead(**kw)


def test_state_dict_keys_and_shapes_are_the_fixture_s(golden):
    z = golden("daformer_head")
    head = _head()
    sd = head.state_dict()
    assert list(sd.keys()) == z["keys"].tolist() == list(dc.shapes())
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == z["shapes"].tolist()
    head.load_state_dict(dc.state())
    assert head.dropout is None and _head(dropout_ratio=0.1).dropout.p == 0.1
    assert not hasattr(_head(act_cfg=None).fuse_layer.bottleneck, "activate") and _head(norm_cfg=dict(type="SyncBN", requires_grad=True))
    from diga_amd.model.networks import daformer_head as dh
    from diga_amd.model.networks import segformer_head as sh
    assert sh.DAFormerHead is dh.DAFormerHead and sh.ASPPWrapper is dh.ASPPWrapper
    with pytest.raises(NotImplementedError):          # the SegFormer head's block is not widened
        sh.ConvModule(8, 8, 3, norm_cfg=dict(type="BN"))


def test_init_weights_follow_the_reference():
    torch.manual_seed(0)
    head = _head()
    head.init_weights()
    with torch.no_grad():
        assert float(head.conv_seg.bias.abs().max()) == 0 and 0.005 < float(head.conv_seg.weight.std()) < 0.02
        dw = head.fuse_layer.aspp_modules[1].depthwise_conv
        assert tuple(dw.conv.weight.shape) == (1024, 1, 3, 3)
        assert abs(float(dw.conv.weight.std()) - (2.0 / (1024 * 9)) ** 0.5) < 0.1 * (2.0 / (1024 * 9)) ** 0.5       # kaiming normal, fan_out
        assert float((dw.bn.weight - 1).abs().max()) == 0 and float(dw.bn.bias.abs().max()) == 0


UNSUPPORTED = {
    "align_corners": dict(align_corners=True),
    "pool": dict(decoder_params=dict(fusion_cfg=dict(type="aspp", sep=True, dilations=(1, 6, 12, 18), pool=True, act_cfg=None,
                                                     norm_cfg=dict(type="BN", requires_grad=True)))),
    "context_layer": dict(decoder_params=dict(fusion_cfg=dict(type="aspp", sep=True, dilations=(1, 6, 12, 18), pool=False, act_cfg=None,
                                                              norm_cfg=dict(type="BN", requires_grad=True),
                                                              context_cfg=dict(type="mlp")))),
    "dense_aspp": dict(decoder_params=dict(fusion_cfg=dict(type="aspp", sep=False, dilations=(1, 6, 12, 18), pool=False, act_cfg=None,
                                                           norm_cfg=dict(type="BN", requires_grad=True)))),
    "embed_sep_conv": dict(decoder_params=dict(embed_cfg=dict(type="sep_conv", kernel_size=3))),
    "embed_conv": dict(decoder_params=dict(embed_neck_cfg=dict(type="conv", kernel_size=3))),
    "fusion_conv": dict(decoder_params=dict(fusion_cfg=dict(type="conv", kernel_size=1))),
    "fusion_rawconv_and_aspp": dict(decoder_params=dict(fusion_cfg=dict(type="rawconv_and_aspp", kernel_size=1))),
    "group_norm": dict(norm_cfg=dict(type="GN", num_groups=32)),
    "no_norm": dict(norm_cfg=None),
    "frozen_affine": dict(norm_cfg=dict(type="BN", requires_grad=False)),
    "gelu": dict(act_cfg=dict(type="GELU")),
    "resize_concat": dict(input_transform="resize_concat"),
    "conv_cfg": dict(conv_cfg=dict(type="Conv2dAdaptivePadding")),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_unsupported_configuration_raises_naming_what_is_built(name):
    with pytest.raises(NotImplementedError, match="DAFormerHead builds"):
        _head(**UNSUPPORTED[name])


# ---- (v) the wiring
def test_student_constructs_with_the_daformer_head():
    """(mit_b1: the smallest backbone the attention kernel is built for -- mit_b0 has head_dim 32 and raises in MixTransfomer.py.)"""
    from diga_amd.model.networks.daformer_head import DAFormerHead
    from diga_amd.model.segformer import SegFormerStudent
    m = SegFormerStudent("mit_b1", head="daformer")
    assert isinstance(m.final, DAFormerHead) and m.head_kind == "daformer"
    assert m.final.in_channels == list(m.backbone.embed_dims) and m.final.channels == 256 and m.final.dropout.p == pytest.approx(0.1)
    assert m.final.return_raw is False and tuple(m.final.conv_seg.weight.shape) == (19, 256, 1, 1)
    m.set_head_dropout(0.0)
    assert m.final.dropout.p == 0.0
    groups = m.optim_parameters(1e-3)
    assert {id(p) for p in groups[1]["params"]} == {id(p) for p in m.final.parameters()} and groups[1]["lr"] == pytest.approx(1e-2)
    assert SegFormerStudent("mit_b1").head_kind == "segformer"
    with pytest.raises(ValueError):
        SegFormerStudent("mit_b1", head="uperhead")
