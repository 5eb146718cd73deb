"""The bits of the exact-fp32 LDS-DMA kernels (csrc/conv.hip: gemm_f32_persistent_kernel, conv_fwd_dma_kernel, conv_wgrad_dma_kernel)
against a recording: for each case of tests/f32_gemm_bits_cases.py the SHA-256 of every buffer the call writes (outputs, statistics
records, partial sums of the backward-data epilogue, dw, and the workspaces with the Winograd-domain products and the split-K slabs)
equals the one in tests/golden/f32_gemm_bits.json, which was recorded on an MI355X from the library of the commit the fixture names.
The other tests of these kernels compare two launches of the same library with each other (persistent walk against per-tile launch) or
hold them to float64 at a tolerance; this one holds any change of how the work is laid over the blocks and the waves of a block -- the
loader role on fewer waves, half tiles in the persistent kernel's last round (both built against this file and measured, DESIGN
section 10) -- to the bits of the kernels as recorded."""
import pytest

import f32_gemm_bits_cases as fc

CASES = fc.cases()


@pytest.fixture(scope="module")
def recorded():
    return fc.load_fixture()


def test_fixture_holds_exactly_the_cases_and_they_reach_every_path(recorded):
    """(device-free)"""
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) and recorded["recorded_from"] and set(recorded["sha256"]) == set(ids)
    reached = [fc.kernel(c) for c in CASES]
    pers = [p for k, p in reached if k == "gemm_f32_persistent_kernel"]
    # all eight instantiations; each on a full and on a ragged M whose last round could be one of half tiles
    insts = {(s, b, i) for s in (False, True) for b in (False, True) for i in (0, 1, 2) if not (s and i)}
    assert len(insts) == 8
    for ragged in (False, True):
        assert {p["inst"] for p in pers if p["split"] and p["ragged"] == ragged} == insts
    # rest <= G / 2, rest > G / 2 and rest == 0; one, two and three K-steps per tile; ragged with and without a short last round
    assert {(p["split"], p["ragged"]) for p in pers} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {p["rest"] for p in pers} == {4, 133, 0} and {p["ksteps"] for p in pers} == {1, 2, 3}
    assert any(p.get("batched") for p in pers)
    fwd = [p for k, p in reached if k == "conv_fwd_dma_kernel"]
    assert {p["epi"] for p in fwd} == {False, True} and all(p["tiles"] < 512 <= p["tiles"] + 4 and p["ragged"] for p in fwd)
    wg = [p for k, p in reached if k == "conv_wgrad_dma_kernel"]
    assert {p["batched"] for p in wg} == {False, True}
    assert any(p["splits"] > 1 and p["ragged"] for p in wg) and any(p["splits"] == 1 and p["ragged"] for p in wg)
    assert len(pers) + len(fwd) + len(wg) == len(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_recording(case, recorded):
    import torch
    got = fc.run(case)
    want = recorded["sha256"][case[0]]
    assert set(got) == set(want)
    for name, t in got.items():
        if name in ("out", "dw"):
            assert not torch.isnan(t).any(), f"{case[0]}: {name}: elements left unwritten"
        assert fc.sha256(t) == want[name], f"{case[0]}: {name} differs from the bits recorded from {recorded['recorded_from']}"
