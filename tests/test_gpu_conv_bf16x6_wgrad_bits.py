"""The dw bits of every instantiation of conv_wgrad_x6_kernel (csrc/conv_bf16x6.h) against a recording: for each case of
tests/x6_wgrad_bits_cases.py the SHA-256 of the dw bytes equals the one in tests/golden/x6_wgrad_bits.json, which was recorded on an
MI355X from the library of the commit the fixture names -- the last one with a separate narrow-tile kernel.  The comparisons of
test_gpu_conv_bf16x6_wgrad_tiles.py (narrow tile against wide tile, every tile against float64) have the same source on both sides;
this one does not."""
import pytest

import x6_wgrad_bits_cases as bc
from test_bf16x6_wgrad_tiles_cpu import tile_rule, wide_splits

CASES = bc.cases()


@pytest.fixture(scope="module")
def recorded():
    return bc.load_fixture()


def test_fixture_holds_exactly_the_cases(recorded):
    """(needs no device)"""
    assert recorded["recorded_from"] and set(recorded["sha256"]) == {cid for cid, _ in CASES}
    # every instantiation is reached: the four narrow tiles and the wide one through the tiled entry point, the wide loader form, the
    # pass form and the batched form
    tiles = {tile_rule(c[5], c[2]) for c, _ in bc.tile_cases()}
    assert tiles == {(64, 64), (64, 128), (128, 128), (256, 64), (256, 128)}
    assert all(tile_rule(c[5], c[2]) == (256, 128) for c in bc.WIDE_CASES)
    for rows, batches, cout, cin, ranges in bc.BATCHED:
        assert wide_splits(rows, cout, cin, batches)[0] == ranges, (rows, batches, cout, cin)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,run", CASES, ids=[cid for cid, _ in CASES])
def test_dw_bits_equal_the_recording(cid, run, recorded):
    import torch
    dw = run()
    assert not torch.isnan(dw).any(), f"{cid}: dw elements left unwritten"
    assert bc.sha256(dw) == recorded["sha256"][cid], f"{cid}: dw differs from the bits recorded from {recorded['recorded_from']}"
