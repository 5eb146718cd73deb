"""CPU-side checks of the bf16x6 arithmetic (conv_math = 2): configuration surface, C ABI surface, and a pure-torch restatement of
the three-plane split and the six-product sum (tools/bf16x6_emulation.py) that pins the arithmetic independently of the kernels."""
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ["diga_make_triplet", "diga_split_bf16x6_image_bytes", "diga_split_bf16x6_image", "diga_conv2d_nhwc_bf16x6",
                    "diga_conv2d_nhwc_bf16x6_epi", "diga_conv2d_wgrad_bf16x6_workspace_bytes", "diga_conv2d_wgrad_bf16x6"]


@pytest.fixture(autouse=True)
def _leave_global_rng_untouched():
    """The emulation seeds torch's global generator.  Tests that run later in the same process draw
    from it, so every test of this file hands the generators back in the state it found them."""
    cpu, gpu = torch.get_rng_state(), (torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def _emulation():
    spec = importlib.util.spec_from_file_location("bf16x6_emulation", os.path.join(ROOT, "tools", "bf16x6_emulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_config_accepts_bf16x6(monkeypatch):
    from diga_amd import _lib, config
    cfg = config.StepConfig().replace(conv_math=2)
    assert cfg.conv_math == 2
    with pytest.raises(ValueError):
        config.StepConfig().replace(conv_math=3)
    assert config.StepConfig().conv_math == 0                     # the default stays exact fp32
    monkeypatch.setenv("DIGA_CONV_MATH", "bf16x6")
    assert config.StepConfig.from_env().conv_math == 2
    monkeypatch.setenv("DIGA_CONV_MATH", "2")
    assert config.StepConfig.from_env().conv_math == 2
    monkeypatch.setenv("DIGA_CONV_MATH", "bf16x3")
    assert config.StepConfig.from_env().conv_math == 1
    monkeypatch.delenv("DIGA_CONV_MATH")
    assert config.StepConfig.from_env().conv_math == 0
    assert _lib.CONV_MATH_BF16X6 == 2
    before = _lib.get_conv_math()
    with config.override(conv_math=0):
        _lib.set_conv_math("bf16x6")
        assert _lib.get_conv_math() == 2
        _lib.set_conv_math(2)
        assert _lib.get_conv_math() == 2
        _lib.set_conv_math("f32")
        assert _lib.get_conv_math() == 0
        with pytest.raises(ValueError):
            _lib.set_conv_math(3)
        with pytest.raises(ValueError):
            _lib.set_conv_math(2, exact=True)
    assert _lib.get_conv_math() == before


def test_layer_math_sends_only_pointwise_layers_to_bf16x6():
    from diga_amd import config
    from diga_amd.model import conv as dc
    with config.override(conv_math=2):
        assert dc._layer_math(1, 1, 64) == 2
        assert dc._layer_math(1, 1, 2048) == 2
        assert dc._layer_math(3, 3, 256) == 0                     # multi-tap: exact fp32 (Winograd / direct)
        assert dc._layer_math(1, 1, 160, False) == 0              # the stem's im2col GEMM, folded options
    with config.override(conv_math=0):
        assert dc._layer_math(1, 1, 64) == 0
    with config.override(conv_math=1):
        assert dc._layer_math(1, 1, 64) == 1 and dc._layer_math(3, 3, 64) == 1
    assert dc.path_log is None


def test_entry_points_are_declared_and_bound():
    from diga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    assert re.search(r"#define\s+DIGA_CONV_MATH_BF16X6\s+2\b", hdr)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/diga_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert len(_lib.PROF_TAGS) == 23


def test_three_plane_split_is_exact_and_six_products_beat_the_fp32_chain():
    """The definition of the arithmetic, restated in torch (tools/bf16x6_emulation.py):
      * a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1) sum to a EXACTLY for normal fp32 values of magnitude 2^-100 .. 2^100,
        for +-0 and for values whose lowest mantissa bits are set (3 x 8 significand bits cover fp32's 24);
      * the six-product sum with the kernels' accumulation order (five corrections chained from zero per 32-deep K-step, one add
        into the running sum) is closer to float64 than the per-k fp32 chain at K = 64, 256, 1024, 2048.
    Documented, not asserted: a non-finite input keeps its inf / nan in plane 0 and turns the low planes (a - a0 = inf - inf) into nan,
    so the product is nan where fp32 might give inf; inputs below 2^-110 in magnitude push the low planes out of bf16's normal range
    (they lose bits or flush to zero) and the planes then no longer sum to the input -- an absolute error below 2^-133."""
    em = _emulation()
    g = torch.Generator().manual_seed(5)
    mant = 1.0 + torch.rand(200000, generator=g)
    expo = torch.randint(-100, 101, (200000,), generator=g).float()
    sign = torch.where(torch.rand(200000, generator=g) < 0.5, -1.0, 1.0)
    x = sign * mant * torch.exp2(expo)
    low = (torch.randint(0, 1 << 22, (4096,), generator=g, dtype=torch.int32) * 2 + 1) | 0x3F800000      # 1.xxx with the last bit set
    allbits = torch.tensor([0x3FFFFFFF, 0x3F800001, 0x3F7FFFFF, 0x00FFFFFF | (30 << 23)], dtype=torch.int32)
    x = torch.cat([x, low.view(torch.float32), allbits.view(torch.float32), torch.tensor([0.0, -0.0])])
    a0, a1, a2, res = em.split3(x)
    assert res == 0.0
    assert torch.equal(a0.double() + a1.double() + a2.double(), x.double())
    for p in (a0, a1, a2):
        assert torch.equal(em.bf(p), p)                           # every plane is a bf16 value
    for K in (64, 256, 1024, 2048):
        a, b = em.operands(512, K, 256, 0)
        ref = a.double() @ b.double()
        sc = float(ref.abs().max())
        e6 = float((em.product_fold(a, b).double() - ref).abs().max()) / sc
        e32 = float((em.product_chain(a, b).double() - ref).abs().max()) / sc
        print(f"K={K}: bf16x6 {e6:.2e}, fp32 per-k chain {e32:.2e} of scale")
        assert e6 < e32, (K, e6, e32)
