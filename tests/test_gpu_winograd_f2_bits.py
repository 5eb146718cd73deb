"""The bits of the Winograd passes at tile = 2 (csrc/winograd.hip) against a recording: for each case of tests/wino_f2_bits_cases.py the
SHA-256 of every buffer the call writes (out, the kept input transform, the epilogue's records, dw, and the workspace region by region:
tile table, U, V, M, Z, dU, the split-K slab) equals the one in tests/golden/wino_f2_bits.json, which was recorded on an MI355X from the
library of the commit the fixture names -- the last one in which F(2x2,3x3) had six hand-written kernels of its own beside the
winoM_* tile templates.  The other Winograd tests hold tile 2 to float64 and to the plain call at a tolerance or with the same source on
both sides; this one holds the M = 2 instantiations of the templates to the bits of the kernels they replaced (the input transform is
still the hand-written kernel: its template form gave the same bits and measured 1-3 % slower)."""
import pytest

import wino_f2_bits_cases as wc

CASES = wc.cases()


@pytest.fixture(scope="module")
def recorded():
    return wc.load_fixture()


def test_fixture_holds_exactly_the_cases_and_they_reach_every_kernel(recorded):
    """(device-free)"""
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) and recorded["recorded_from"] and set(recorded["sha256"]) == set(ids)
    # the host's selection rule over the cases: in the recorded revision the six hand-written kernels, now the four M = 2 instantiations
    # of the transforms, the input transform that stayed hand-written, and the 16 operand combinations of the epilogue transform on 4
    # tile lanes
    was = set().union(*(wc.kernels_f2(c) for c in CASES))
    assert was == wc.F2_KERNELS and len(was) == 6, was ^ wc.F2_KERNELS
    reached = set().union(*(wc.kernels(c) for c in CASES))
    assert reached == wc.ALL_KERNELS, reached ^ wc.ALL_KERNELS
    assert len(wc.ALL_KERNELS) == 5 + 16


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_recording(case, recorded):
    import torch
    got = wc.run(case)
    want = recorded["sha256"][case[0]]
    assert set(got) == set(want)
    for name, t in got.items():
        if name == "out":
            assert not torch.isnan(t).any(), f"{case[0]}: output elements left unwritten"
        assert wc.sha256(t) == want[name], f"{case[0]}: {name} differs from the bits recorded from {recorded['recorded_from']}"
