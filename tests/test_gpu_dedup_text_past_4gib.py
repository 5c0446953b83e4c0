"""dedup_text on a text of more than 2^32 bytes: periodic_text's standard log100 block * K + tail,
about 4.07 GiB assembled on the device - the same K as tests/test_gpu_text_past_4gib.py - under
MATCH (the key is a line's first piece).  What it shows is the walk without the LDS front, KEYED
and MARK bits, `first` offsets, the mark's scan and the run copy at offsets above 2^32.

Every copy of the block holds the same keys, so the expectation comes from ONE block + tail: a
string's earliest occurrence is where it is there (in the first block, or - for a string the block
lacks - in the tail, K - 1 blocks further on), and its count is K times its count in the block
plus its count in the tail.  With the defaults the output is therefore the output of 1 block +
tail, byte for byte, while n_lines and n_keyed grow linearly in K; a count window selects the
strings by those totals.  test_the_extrapolation_rule (no GPU) proves this against dedup_rule run
directly over 3 blocks + tail.

Two more runs take min_count = K * c + t and that value + 1 for the block's most frequent string
(c times in the block, t in the tail): exactly on its count it alone is emitted, one above nothing
is.  Needs 16 GiB of free device memory."""
import numpy as np
import pytest

import one_amd
from one_amd import _lib

import dedup_rule as DR
import periodic_text as PT
import test_gpu_collect_text as CT
import test_gpu_dedup_text as DD

B32 = 1 << 32
K = -(-(B32 + (64 << 20)) // PT.N)
NEED = 16 << 30
NAME = "log100"
MAX = DR.MAX
SENT = 0x55


def _layout():
    return PT.layout("standard", NAME)


def _extrapolate(lay, k, lo=1, hi=MAX):
    """((n_lines, n_keyed, n_distinct, n_dropped, n_emitted), the output, the emitted lines of
    block + tail, the strings' (first line, count in the block, count in the tail)) for
    block * k + tail under MATCH, from block + tail alone"""
    t = DD._t(NAME, lay.text(1))
    assert t.n_lines == lay.L + lay.tail_lines
    seen = {}
    for i, key in enumerate(DR.keys(t, "match", 1)):
        if key is not None:
            row = seen.setdefault(key[1], [i, 0, 0])
            row[1 if i < lay.L else 2] += 1
    emitted = [i for i, cb, ct in seen.values() if lo <= k * cb + ct <= hi]
    assert emitted == sorted(emitted)
    keyed = sum(k * cb + ct for _, cb, ct in seen.values())
    counts = (lay.n_lines(k), keyed, len(seen), 0, len(emitted))
    return counts, t.join(emitted), emitted, seen


def _hot(seen):
    """the block's most frequent string: (its count in the block, its count in the tail)"""
    _, cb, ct = max(seen.values(), key=lambda row: row[1])
    return cb, ct


def test_the_extrapolation_rule():
    lay = _layout()
    direct = DD._t(NAME, lay.text(3))
    counts, out, emitted, seen = _extrapolate(lay, 3)
    assert DR.dedup(direct, "match", 1) == counts + (out,)
    # ... which is the output of 1 block + tail, while n_lines and n_keyed are linear in the blocks
    one = DR.dedup(DD._t(NAME, lay.text(1)), "match", 1)
    assert one[2:] == counts[2:] + (out,)
    two = _extrapolate(lay, 2)[0]
    assert counts[0] - two[0] == two[0] - one[0] == lay.L
    assert counts[1] - two[1] == two[1] - one[1] > 100
    # a string the block lacks is emitted from the tail
    assert any(i >= lay.L for i in emitted) and any(i < lay.L for i in emitted)
    assert all(cb == 0 for i, cb, ct in seen.values() if i >= lay.L)
    # a window exactly on and one above the hot string's count, and one that takes the rest
    cb, ct = _hot(seen)
    assert cb > 100
    for lo, hi in ((3 * cb + ct, MAX), (3 * cb + ct + 1, MAX), (1, 3 * cb + ct - 1), (2, 3 * cb)):
        counts, out, emitted, _ = _extrapolate(lay, 3, lo, hi)
        assert DR.dedup(direct, "match", 1, min_count=lo, max_count=hi) == counts + (out,), (lo, hi)
    assert len(_extrapolate(lay, 3, 3 * cb + ct)[2]) == 1
    assert len(_extrapolate(lay, 3, 3 * cb + ct + 1)[2]) == 0


def _run(exe, dev, want, **kw):
    """the device form into a sentinel-filled buffer against (counts, output)"""
    import torch
    counts, out = want
    buf = torch.full((len(out) + 16,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.dedup_text(exe, dev, what="match", max_distinct=4096, out=buf, out_cap=len(out),
                             **kw)
    assert one_amd.last_kernel() == "k_dedup_text"
    torch.cuda.synchronize()
    assert tuple(int(t.item()) for t in got[:6]) == counts + (len(out),), kw
    back = buf.cpu().numpy().tobytes()
    assert back[:len(out)] == out and back[len(out):] == bytes([SENT]) * 16, kw


@pytest.mark.gpu
def test_dedup_text_past_4gib():
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("a text past 4 GiB needs 16 GiB of free device memory; %d MiB are free" % (free >> 20))
    lay = _layout()
    assert K * lay.P > B32 + (1 << 26)
    counts, out, emitted, seen = _extrapolate(lay, K)
    one = DR.dedup(DD._t(NAME, lay.text(1)), "match", 1)
    # the output of 1 block + tail; n_lines and n_keyed linear in K
    assert out == one[5] and counts[2:] == one[2:5]
    assert counts[0] == lay.L * K + lay.tail_lines and counts[1] > 10 ** 6
    # a key that occurs only in the tail: its line, and so its `first`, lies above 2^32
    t = DD._t(NAME, lay.text(1))
    tail_lines = [i for i in emitted if i >= lay.L]
    assert tail_lines and int(t.offs[tail_lines[0]]) + (K - 1) * lay.P > B32
    exe = one_amd.Executable(CT._blob(NAME))
    dev = lay.device_text(K)
    assert dev.numel() == lay.length(K) > B32 + (1 << 26)
    try:
        _run(exe, dev, (counts, out))
        cb, ct = _hot(seen)
        for lo in (K * cb + ct, K * cb + ct + 1):
            c, o, e, _ = _extrapolate(lay, K, lo)
            assert len(e) == (1 if lo == K * cb + ct else 0)
            _run(exe, dev, (c, o), min_count=lo)
        # every later duplicate: all but the first lines, most of them above 2^32 (sizes only)
        got = one_amd.dedup_text(exe, dev, what="match", max_distinct=4096, invert=True, out_cap=0)
        torch.cuda.synchronize()
        assert int(got[4].item()) == counts[1] - counts[2]
    finally:
        del dev
        _lib.lib().redgpu_thread_release()
        torch.cuda.empty_cache()
