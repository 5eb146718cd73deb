"""OCR head, the part that needs no GPU: the module's state-dict layout, the float64 restatement (tests/ocr_cases.py) against the
capture of the reference class (tests/golden/ocr_head.npz, tools/gen_golden.py::gen_ocr_head), the C ABI of csrc/ocr.hip (declared,
bound, exported, documented) and its argument checks, all of which precede any device call."""
import os
import re

import numpy as np
import pytest
import torch

import ocr_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["diga_ocr_workspace_bytes", "diga_ocr_region_fwd", "diga_ocr_region_bwd", "diga_ocr_attend_fwd", "diga_ocr_attend_bwd"]


def test_state_dict_keys_are_the_reference_layout(golden):
    from diga_amd.model.networks.ocrnet_module import OCRNet
    z = golden("ocr_head")
    keys = [str(k) for k in z["keys"]]
    head = OCRNet(oc.SMALL_CFG)
    assert list(head.state_dict().keys()) == keys
    sd = oc.fixture_state(z)
    assert list(sd) == keys and list(oc.random_state(oc.SMALL_CFG, 0)) == keys
    head.load_state_dict(sd)                                   # shapes too
    for k, v in head.state_dict().items():
        assert torch.equal(v.float(), sd[k].float()), k
    # the BatchNorm pair of a fresh head is (1, 0), as the reference's init_weights leaves it
    fresh = OCRNet(oc.REAL_CFG)
    assert float(fresh.augmented_rep[1].weight.detach().min()) == 1.0 and float(fresh.augmented_rep[1].bias.detach().abs().max()) == 0.0
    assert fresh.augmented_rep[3].p == 0.05 and tuple(fresh.pixel_representations[0].weight.shape) == (512, 720, 3, 3)


def test_restatement_reproduces_the_capture_in_float64(golden):
    z = golden("ocr_head")
    sd = oc.fixture_state(z)
    x, x_eval = z.t("x").float(), z.t("x_eval").float()
    probes = [z.t("probe_soft").float(), z.t("probe_seg").float()]
    got = oc.head_step(sd, x, probes, 32, torch.float64)
    # the eval pass of the capture runs on the statistics the train pass left behind
    sd_after = dict(sd)
    for k in sd:
        if k.endswith(("running_mean", "running_var")):
            sd_after[k] = got["b_" + k.replace(".", "_")]
    got.update(oc.head_eval(sd_after, x_eval, 32, torch.float64))
    names = [k for k in z if k.startswith(("g_", "b_")) or k in ("soft", "seg", "aug", "dx", "soft_eval", "seg_eval", "aug_eval")]
    assert len(names) == 58 and set(names) <= set(got)
    for k in names:
        want = z.t(k)
        assert want.dtype == torch.float64 and got[k].shape == want.shape, k
        err = float((got[k] - want).abs().max()) / float(z["scale_" + k])
        assert err <= 1e-12, f"{k}: {err:.3e} of scale"


def test_fixture_yardsticks_are_fp32_sized(golden):
    """err32_* is the reference class in fp32 on the CPU against itself in float64: a few fp32 ulps to 1e-5 of scale everywhere."""
    z = golden("ocr_head")
    errs = {k: float(z[k]) for k in z if k.startswith("err32_")}
    assert len(errs) == 58 and int(z["nbt"]) == 4
    assert all(1e-9 < e < 2e-5 for e in errs.values()), errs


def test_exports_are_declared_bound_exported_and_documented():
    from diga_amd import _lib
    header = open(os.path.join(ROOT, "include", "diga_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"\b(diga_ocr_[a-z0-9_]+)\s*\(", header))
    assert declared == set(EXPORTS)
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert name in doc, f"{name} is not named in INTEGRATION.md"
    assert len(_lib.PROF_TAGS) == 23                           # no profiling tag was added


def test_workspace_bytes_is_monotone(golden):
    from diga_amd import _lib
    ws = _lib.lib.diga_ocr_workspace_bytes
    prev = 0
    for n in (1, 2, 3, 6, 64):
        cur = ws(n, 32768, 19, 512)
        assert cur > prev
        prev = cur
    prev = 0
    for p in (1, 2, 255, 256, 257, 5003, 32768, 131072, 1 << 22):
        cur = ws(6, p, 19, 512)
        assert cur > prev, p
        prev = cur
    assert ws(6, 32768, 19, 512) >= 8 * (6 * 128 * 19 * (512 + 2))          # the float64 partials and their (max, sum) pairs at least
    assert ws(6, 32768, 22, 512) > ws(6, 32768, 19, 512) and ws(6, 32768, 19, 512) > ws(6, 32768, 19, 256)
    for bad in ((0, 10, 19, 64), (1, 0, 19, 64), (1, 10, 0, 64), (1, 10, 33, 64), (1, 10, 19, 6), (1, 10, 19, 0), (1, 10, 19, 2048)):
        assert ws(*bad) == 0, bad


# ---- argument checks.  Pointers are made-up addresses: every case must be refused before anything is dereferenced or launched.
A16, A4 = 0x10000, 0x10004              # a 16-byte aligned address, and one aligned to 4 bytes only


def _region_fwd(**kw):
    a = dict(x=A16, ld_x=64, s=A4, ld_s=19, region=A16, stat=A16, N=2, P=143, K=19, C=64, ws=A16, ws_bytes=1 << 30)
    a.update(kw)
    return ("diga_ocr_region_fwd", [a["x"], a["ld_x"], a["s"], a["ld_s"], a["region"], a["stat"], a["N"], a["P"], a["K"], a["C"], a["ws"],
                                    a["ws_bytes"], None])


def _region_bwd(**kw):
    a = dict(x=A16, ld_x=64, s=A4, ld_s=19, stat=A16, region=A16, d_region=A16, dx=A16, ld_dx=64, ds=A4, ld_ds=19, N=2, P=143, K=19, C=64)
    a.update(kw)
    return ("diga_ocr_region_bwd", [a["x"], a["ld_x"], a["s"], a["ld_s"], a["stat"], a["region"], a["d_region"], a["dx"], a["ld_dx"], a["ds"],
                                    a["ld_ds"], a["N"], a["P"], a["K"], a["C"], None])


def _attend_fwd(**kw):
    a = dict(q=A16, ld_q=32, key=A16, val=A16, out=A16, ld_out=32, attn=A4, N=2, P=143, K=19, D=32, Dv=32)
    a.update(kw)
    return ("diga_ocr_attend_fwd", [a["q"], a["ld_q"], a["key"], a["val"], a["out"], a["ld_out"], a["attn"], a["N"], a["P"], a["K"], a["D"],
                                    a["Dv"], 0.25, None])


def _attend_bwd(**kw):
    a = dict(q=A16, ld_q=32, key=A16, val=A16, attn=A4, d_out=A16, ld_do=32, dq=A16, ld_dq=32, d_key=A16, d_val=A16, N=2, P=143, K=19, D=32,
             Dv=32, ws=A16, ws_bytes=1 << 30)
    a.update(kw)
    return ("diga_ocr_attend_bwd", [a["q"], a["ld_q"], a["key"], a["val"], a["attn"], a["d_out"], a["ld_do"], a["dq"], a["ld_dq"], a["d_key"],
                                    a["d_val"], a["N"], a["P"], a["K"], a["D"], a["Dv"], 0.25, a["ws"], a["ws_bytes"], None])


EINVAL_CASES = [
    # null pointers
    (_region_fwd(x=None), "null pointer"), (_region_fwd(stat=None), "null pointer"), (_region_fwd(ws=None), "null pointer"),
    (_region_bwd(d_region=None), "null pointer"), (_region_bwd(ds=None), "null pointer"),
    (_attend_fwd(val=None), "null pointer"), (_attend_fwd(out=None), "null pointer"),
    (_attend_bwd(attn=None), "null pointer"), (_attend_bwd(d_key=None), "null pointer"), (_attend_bwd(ws=None), "null pointer"),
    # misaligned pointers: 16 bytes on the channel tensors, 4 on the K-wide ones
    (_region_fwd(x=A4), "misaligned pointer"), (_region_fwd(s=A4 + 2), "misaligned pointer"), (_region_fwd(ws=A4), "misaligned pointer"),
    (_region_bwd(dx=A4), "misaligned pointer"), (_region_bwd(stat=A4), "misaligned pointer"), (_region_fwd(stat=A4), "misaligned pointer"),
    (_attend_fwd(key=A4), "misaligned pointer"), (_attend_fwd(attn=A4 + 2), "misaligned pointer"),
    (_attend_bwd(d_out=A4), "misaligned pointer"), (_attend_bwd(d_val=A4), "misaligned pointer"),
    # pitches smaller than the row (or, on a channel tensor, not a multiple of 4)
    (_region_fwd(ld_x=60), "pitch ld_x = 60 smaller than the row of 64"), (_region_fwd(ld_s=18), "pitch ld_s = 18 smaller than the row of 19"),
    (_region_fwd(ld_x=66), "pitch ld_x = 66 is not a multiple of 4"),
    (_region_bwd(ld_dx=32), "pitch ld_dx = 32 smaller than the row of 64"), (_region_bwd(ld_ds=16), "pitch ld_ds = 16 smaller than the row of 19"),
    (_attend_fwd(ld_q=28), "pitch ld_q = 28 smaller than the row of 32"), (_attend_fwd(ld_out=0), "pitch ld_out = 0 smaller than the row of 32"),
    (_attend_bwd(ld_do=31), "pitch ld_do = 31 smaller than the row of 32"), (_attend_bwd(ld_dq=8), "pitch ld_dq = 8 smaller than the row of 32"),
    # K outside 1 .. 32
    (_region_fwd(K=0, ld_s=19), "K = 0 outside 1 .. 32"), (_region_fwd(K=33, ld_s=40), "K = 33 outside 1 .. 32"),
    (_region_bwd(K=33, ld_s=40, ld_ds=40), "K = 33 outside 1 .. 32"), (_attend_fwd(K=0), "K = 0 outside 1 .. 32"),
    (_attend_fwd(K=40), "K = 40 outside 1 .. 32"), (_attend_bwd(K=-1), "K = -1 outside 1 .. 32"),
    # channel counts
    (_region_fwd(C=62), "channel count C = 62 is not a positive multiple of 4"), (_region_bwd(C=0), "channel count C = 0 is not a positive multiple of 4"),
    (_attend_fwd(D=30), "channel count D = 30 is not a positive multiple of 4"), (_attend_fwd(Dv=18), "channel count Dv = 18 is not a positive multiple of 4"),
    (_attend_bwd(Dv=30), "channel count Dv = 30 is not a positive multiple of 4"),
    (_region_fwd(C=2048, ld_x=2048), "channel count C = 2048 above 1024"),
    (_attend_fwd(K=32, D=1024, Dv=1024, ld_q=1024, ld_out=1024), "do not fit the 160 KB of LDS"),
    # batch and pixel counts
    (_region_fwd(N=0), "bad shape N = 0"), (_attend_fwd(P=0), "bad shape N = 2 (1 .. 65535), P = 0"), (_region_bwd(N=65536), "bad shape N = 65536"),
    # a workspace that is too small
    (_region_fwd(ws_bytes=1024), "workspace too small"), (_region_fwd(ws_bytes=0), "workspace too small"),
    (_attend_bwd(ws_bytes=4 * 2 * 143 * 19), "workspace too small"),
]


@pytest.mark.parametrize("idx", range(len(EINVAL_CASES)))
def test_entry_points_refuse_bad_arguments_before_any_device_call(idx):
    from diga_amd import _lib
    (name, args), message = EINVAL_CASES[idx]
    rc = getattr(_lib.lib, name)(*args)
    assert rc == -1, f"{name}{args}: code {rc}"                 # DIGA_EINVAL
    assert message in _lib.last_error(), (_lib.last_error(), message)
    with pytest.raises(RuntimeError, match=name):
        _lib.call(name, *args)


def test_workspace_bound_is_exactly_the_query():
    """One byte less than diga_ocr_workspace_bytes is refused (the accepted size is not probed here: it would launch)."""
    from diga_amd import _lib
    need = _lib.lib.diga_ocr_workspace_bytes(2, 143, 19, 64)
    name, args = _region_fwd(ws_bytes=need - 1)
    assert getattr(_lib.lib, name)(*args) == -1 and f"{need - 1} < {need} bytes" in _lib.last_error()
    need = _lib.lib.diga_ocr_workspace_bytes(2, 143, 19, 40)
    name, args = _attend_bwd(Dv=40, ld_do=40, ws_bytes=need - 1)
    assert getattr(_lib.lib, name)(*args) == -1 and f"{need - 1} < {need} bytes" in _lib.last_error()


def test_module_refuses_cpu_tensors_and_unsupported_configs():
    from diga_amd.model.networks import ocrnet_module as om
    with pytest.raises(RuntimeError, match="GPU only"):
        om.ocr_region_gather(torch.zeros(1, 4, 8), torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        om.ocr_object_attention(torch.zeros(1, 4, 8), torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), 1.0)
    with pytest.raises(NotImplementedError):
        om.OCRNet({"OCRNET_MODEL": {"RAW_IN_CHANNELS": 48, "PIXEL_REP_CHANNELS": 64, "KEY_CHANNELS": 32, "NUM_CLASSES": 40}})
    assert np.isclose(om.OCRNet(oc.SMALL_CFG).key_channels ** -.5, 32 ** -.5)
