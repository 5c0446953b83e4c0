"""sum_text on a text of more than 2^32 bytes: periodic_text's dense log100 block * K + tail, about
4.07 GiB assembled on the device - the same K and lead as tests/test_gpu_text_past_4gib.py.  The LDS
front is 64-bit, so this text runs as every other does; what it shows is a sum and a count that no
32-bit counter holds, and chunk numbers and offsets above 2^32.

The dense log100 block is full of ONE head, which holds no digit: the oracle finds 49 million items
there and 8 numeric ones, all in the tail - the path that looks at every piece and counts none, and
a sum row of 2,856.  A sum row above 2^32 cannot come from that text, so the dense num3 block
(periodic_text's "extract" case) runs beside it: 667 million items, every one numeric, sums of
10^12 and 10^14.

The expectation is linear in the number of blocks: every block ends in the delimiter, so count and
sum for K blocks are the oracle's answer for 2 blocks plus (K - 2) times (the answer for 3 minus the
answer for 2), and min and max are those of 3 blocks.  test_the_extrapolation_rule (no GPU) proves
that against the oracle run directly over 5 blocks.  Needs 16 GiB of free device memory."""
import numpy as np
import pytest

import one_amd
from one_amd import _lib

import periodic_text as PT
import test_gpu_sum_text as ST

B32 = 1 << 32
K = -(-(B32 + (64 << 20)) // PT.N)
NEED = 16 << 30
KIND = "dense"
N_BINS = {"log100": 101, "num3": 4}
M64 = 2 ** 64


def _layout(name):
    lay0 = PT.layout(KIND, name)
    spans = PT.block_spans(name, lay0.block)
    return lay0.with_lead(PT.lead_for(lay0, B32, spans))


def _extrapolate(name, lay, k, last):
    """(n_lines, n_items, n_numeric, stats) for lead + block * k + tail from the oracle's answers
    for 2 and 3 blocks, in Python integers"""
    two = ST._expect(name, lay.text(2), N_BINS[name], last)
    three = ST._expect(name, lay.text(3), N_BINS[name], last)
    scal = tuple(a + (k - 2) * (b - a) for a, b in zip(two[:3], three[:3]))
    rows = [[(int(a) + (k - 2) * (int(b) - int(a))) % M64 for a, b in zip(two[3][r], three[3][r])]
            for r in (0, 1)]
    stats = np.array(rows + [three[3][2].tolist(), three[3][3].tolist()], dtype=np.uint64)
    return scal + (stats,)


@pytest.mark.parametrize("name", ["log100", "num3"])
def test_the_extrapolation_rule(name):
    lay = _layout(name)
    for last in (False, True):
        direct = ST._expect(name, lay.text(5), N_BINS[name], last)
        got = _extrapolate(name, lay, 5, last)
        assert got[:3] == direct[:3] and direct[1] > 1000
        assert np.array_equal(got[3], direct[3])
        if name == "num3":
            assert direct[2] == direct[1] and (direct[3][0] > 0).sum() >= 2
        else:
            assert direct[2] == 8       # the tail's: the block's head has no digit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["log100", "num3"])
def test_sum_text_past_4gib(name):
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("a text past 4 GiB needs 16 GiB of free device memory; %d MiB are free" % (free >> 20))
    lay = _layout(name)
    assert K * lay.P > B32 + (1 << 26)
    exe = one_amd.Executable(ST.CT._blob(name))
    dev = lay.device_text(K)
    assert dev.numel() == lay.length(K) > B32 + (1 << 26)
    try:
        for which, last in (("first", False), ("last", True)):
            want = _extrapolate(name, lay, K, last)
            assert want[1] > 10 ** 6
            if name == "num3":
                assert int(want[3][1].max()) > B32 and int(want[3][0].max()) > 10 ** 8
            got = one_amd.sum_text(exe, dev, N_BINS[name], which=which)
            assert one_amd.last_kernel() == "k_sum_text"
            torch.cuda.synchronize()
            assert tuple(int(x.item()) for x in got[:3]) == want[:3], which
            assert np.array_equal(ST._host_stats(got[3]), want[3]), which
            # accumulate: a second call into the same table doubles count and sum, and leaves min
            # and max
            again = one_amd.sum_text(exe, dev, N_BINS[name], which=which, into=got[3])
            torch.cuda.synchronize()
            out = ST._host_stats(again[3])
            assert np.array_equal(out[:2], want[3][:2] * np.uint64(2)), which
            assert np.array_equal(out[2:], want[3][2:]), which
    finally:
        del dev
        _lib.lib().redgpu_thread_release()
        torch.cuda.empty_cache()
