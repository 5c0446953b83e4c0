"""range_text on a text of more than 2^32 bytes: periodic_text's standard log100 block * K + tail,
about 4.07 GiB assembled on the device - the same K as tests/test_gpu_text_past_4gib.py.  What it
shows is the machine's state carried over 260,000 chunks, and line numbers, range numbers' records
and offsets above 2^32.

The toggle form over the result of the block's one head.  The block is arranged to END OUTSIDE a
range: where its events are odd in number one more event line is appended, so every copy of the
block begins outside, as the first does.  The expectation is then linear in the number of blocks:
the counts for K blocks are the oracle's answer for 2 blocks plus (K - 2) times (the answer for 3
minus the answer for 2); the records of the last block and the tail are those of the 3-block text,
K - 3 blocks further on; the output is the block's output K times and the tail's.
test_the_extrapolation_rule (no GPU) proves all three against the rule run directly over 5 blocks.

One more run has a single open line in the lead and no close anywhere: one range, the whole text
behind it inside by carry alone.  Needs 16 GiB of free device memory."""
import numpy as np
import pytest

import one_amd
from one_amd import _lib
from one_amd import workloads as W

import periodic_text as PT
import range_rule as R
import test_gpu_collect_text as CT

B32 = 1 << 32
K = -(-(B32 + (64 << 20)) // PT.N)
NEED = 16 << 30
NAME = "log100"
SETTING = dict(emit_open=True, emit_close=False)

_made = {}


def _result(head):
    v, _ = R.values_of(NAME, b"zz " + head + b"qq\n")
    assert len(v) == 1 and v[0] >= 1
    return int(v[0])


def _layout():
    """the standard block, its events made even in number, and the DFA's tail; the result that
    toggles"""
    if "lay" not in _made:
        lay0 = PT.layout("standard", NAME)
        v, _ = R.values_of(NAME, lay0.block)
        r = _result(W.log100_heads()[7])
        assert (v == r).sum() > 100
        block = lay0.block
        if (v == r).sum() % 2:
            block += b"one more: " + W.log100_heads()[7] + b"\n"
        tv, _ = R.values_of(NAME, lay0.tail)
        assert not (tv == r).any()          # the tail's lines are outside
        _made["lay"] = (PT.Layout(block, lay0.tail), r)
    return _made["lay"]


def _extrapolate(lay, r, k):
    """(n_lines, n_ranges, n_emitted, out_len), the last block's and the tail's records, and the
    output's period and rest, for block * k + tail"""
    two = R.expect(NAME, lay.text(2), r, None, **SETTING)
    three = R.expect(NAME, lay.text(3), r, None, **SETTING)
    counts = tuple(a + (k - 2) * (b - a) for a, b in zip(
        (two.n_lines, two.n_ranges, two.n_emitted, len(two.out)),
        (three.n_lines, three.n_ranges, three.n_emitted, len(three.out))))
    last = three.first_line >= np.uint64(2 * lay.L)
    moves = (lay.L, lay.L, lay.P, lay.P)
    records = tuple(col[last].astype(np.int64) + (k - 3) * m for col, m in zip(three.records, moves))
    period = len(three.out) - len(two.out)
    return counts, records, three.out[:period], three.out[3 * period:]


def test_the_extrapolation_rule():
    lay, r = _layout()
    one = R.expect(NAME, lay.block, r, None, **SETTING)
    assert one.kind[-1] != R.OPEN and one.kind[-1] != R.BODY        # the block ends outside
    direct = R.expect(NAME, lay.text(5), r, None, **SETTING)
    counts, records, period, rest = _extrapolate(lay, r, 5)
    assert counts == (direct.n_lines, direct.n_ranges, direct.n_emitted, len(direct.out))
    assert direct.n_ranges > 400 and period == one.out
    assert direct.out == period * 5 + rest
    for got, want in zip(records, direct.records):
        assert len(got) > 50 and np.array_equal(got, want[-len(got):].astype(np.int64))


@pytest.mark.gpu
def test_range_text_past_4gib():
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("a text past 4 GiB needs 16 GiB of free device memory; %d MiB are free" % (free >> 20))
    lay, r = _layout()
    assert K * lay.P > B32 + (1 << 26)
    exe = one_amd.Executable(CT._blob(NAME))
    dev = lay.device_text(K)
    assert dev.numel() == lay.length(K) > B32 + (1 << 26)
    try:
        counts, records, period, rest = _extrapolate(lay, r, K)
        assert counts[1] > 10 ** 6 and counts[3] == len(period) * K + len(rest)
        got = one_amd.range_text(exe, dev, r, None, out_cap=counts[3] + 16, rec_cap=counts[1] + 2,
                                 **SETTING)
        assert one_amd.last_kernel() == "k_range_text"
        torch.cuda.synchronize()
        assert tuple(int(t.item()) for t in got[:4]) == counts
        # the last block's and the tail's records: offsets above 2^32, and line numbers as they are
        # (4 GiB of such lines are fewer than 2^32 lines)
        n = len(records[0])
        for rec, want in zip(got[5:], records):
            assert rec[counts[1] - n:counts[1]].cpu().numpy().tolist() == want.tolist()
        assert int(records[3][-1]) > B32 and int(records[2][0]) > B32
        assert int(records[0][0]) > (K - 2) * lay.L
        # the output: the block's, K times, and the tail's
        m = len(period)
        want = torch.from_numpy(np.frombuffer(period, dtype=np.uint8).copy()).cuda()
        assert bool((got[4][:m * K].view(K, m) == want).all())
        assert got[4][m * K:counts[3]].cpu().numpy().tobytes() == rest
        del got, want
        torch.cuda.empty_cache()
        # a single open line in front, no close anywhere: the other two results never toggle it
        heads = W.log100_heads()
        o, c = _result(heads[11]), _result(heads[42])
        assert len({o, c, r}) == 3
        first = b"x " + heads[11] + b"y\n"
        dev = torch.cat([torch.from_numpy(np.frombuffer(first, dtype=np.uint8).copy()).cuda(), dev])
        lines = 1 + lay.n_lines(K)
        end = len(first) + PT.lines_end(lay, K)
        got = one_amd.range_text(exe, dev, o, c, out_cap=dev.numel(), rec_cap=2)
        torch.cuda.synchronize()
        assert [int(t.item()) for t in got[:4]] == [lines, 1, lines, end]
        assert end > B32                      # (fewer than 2^32 lines: out_len is what passes it)
        assert [int(t[0].item()) for t in got[5:]] == [0, lines - 1, 0, end]
        assert torch.equal(got[4][:end], dev[:end])
    finally:
        del dev
        _lib.lib().redgpu_thread_release()
        torch.cuda.empty_cache()
