"""The downsample BatchNorm of a bottleneck folded into the junction relu(bn3(conv3) + skip) (config.fold_downsample_bn, default on): the
junction kernel applies the downsample BatchNorm's two coefficients to the raw downsample output on load instead of reading a tensor
that BatchNorm's own apply pass wrote.  Against the two-pass form (fold off: the kernels of before) everything the block produces is
equal bit for bit -- output, input gradient, every weight gradient, the running statistics of both BatchNorms -- under autograd and
under torch.no_grad() (the teacher's path).  Row counts (578, 289 x 2) are no multiples of 64."""
import pytest
import torch

from diga_amd import config
from oracle import detweights, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _keep_global_rng_state():
    """Layer constructors draw their initial weights from torch's global generators; hand them back as found."""
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _make_block(pfx, inplanes, planes, stride):
    from diga_amd.model import seg_model_noaux as sm
    from diga_amd.model.conv import DigaConv2d
    down = torch.nn.Sequential(DigaConv2d(inplanes, planes * 4, 1, stride=stride, bias=False), sm._frozen_bn(planes * 4))
    blk = sm.Bottleneck(inplanes, planes, stride, dilation=1, downsample=down)
    kinds = {"weight": "bn_w", "bias": "bn_b", "running_mean": "bn_rm", "running_var": "bn_rv"}
    own = blk.state_dict()
    for k, v in own.items():
        if k.endswith("num_batches_tracked"):
            continue
        kind = "conv" if v.dim() == 4 else kinds[k.rsplit(".", 1)[1]]
        own[k] = detweights.fill(f"{pfx}.{k}", tuple(v.shape), kind)
    blk.load_state_dict(own)
    return blk.to(DEV).train()


def _run(pfx, inplanes, planes, stride, x, probe, fold, grad):
    """One forward (+ backward) of a freshly built block; returns its tensors and the library calls it made."""
    from diga_amd import _lib
    blk = _make_block(pfx, inplanes, planes, stride)
    calls, real = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        with config.override(fold_downsample_bn=fold):
            if grad:
                xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
                y = blk(xd)
                (y * probe.to(DEV)).sum().backward()
            else:
                xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
                with torch.no_grad():
                    y = blk(xd)
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    out = {"y": y.detach().clone()}
    if grad:
        out["dx"] = xd.grad.clone()
        out.update({"d " + n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None})
    for bn in ("bn3", "downsample.1"):
        mod = blk.get_submodule(bn)
        out[bn + ".running_mean"], out[bn + ".running_var"] = mod.running_mean.clone(), mod.running_var.clone()
        out[bn + ".num_batches_tracked"] = mod.num_batches_tracked.clone()
    return out, calls


# name, N, H, W, inplanes, planes, stride
CASES = [("stride1_17", 2, 17, 17, 64, 64, 1), ("stride2_33", 2, 33, 33, 64, 64, 2)]


@pytest.mark.parametrize("grad", [True, False], ids=["autograd", "no_grad"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fold_equals_two_pass_form_bit_for_bit(case, grad):
    name, n, h, w, inplanes, planes, stride = case
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert (n * ho * wo) % 64 != 0
    g = synth.gen(4100 + h + stride)
    x = torch.randn((n, inplanes, h, w), generator=g).relu_() + 0.1 * torch.randn((n, inplanes, h, w), generator=g)
    probe = torch.randn((n, planes * 4, ho, wo), generator=g)
    two_pass, calls_off = _run("fold." + name, inplanes, planes, stride, x, probe, False, grad)
    folded, calls_on = _run("fold." + name, inplanes, planes, stride, x, probe, True, grad)
    assert "diga_bn_fwd_partials_resab" in calls_on and "diga_bn_fwd_partials_resab" not in calls_off, (calls_on, calls_off)
    assert set(folded) == set(two_pass)
    if grad:
        assert {"dx", "d conv1.weight", "d conv2.weight", "d conv3.weight", "d downsample.0.weight"} <= set(folded)
    for k in two_pass:
        assert torch.equal(folded[k], two_pass[k]), (name, k)
    # (the statistics moved: a block that left them at their initial values would pass the comparison above)
    fresh = detweights.fill(f"fold.{name}.downsample.1.running_mean", (planes * 4,), "bn_rm").to(DEV)
    assert not torch.equal(folded["downsample.1.running_mean"], fresh)
