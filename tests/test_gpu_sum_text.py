"""sum_text (redgpu_sum_text[_dev]): per result the count, sum, minimum and maximum of the decimal
numbers found in a raw text's matches.  Every output is exact against plain Python over what the
CPU oracle gives - the pieces of test_gpu_extract_text._oracle, the results of
test_gpu_collect_text._want, `re` for the digits, Python integers for the reduction - never against
the code under test: the value rule with the 64-bit wrap, the first against the last run, every cut
of n_bins and max_per_line, every table placement, slots on both sides of the LDS boundary, the
chunk-border shapes, a hot slot, a text of more chunks than the grid has waves, accumulate with a
carry, a wrap and a merge, optional outputs, the identity with tally_text on the GPU, concurrent
streams and threads, and the C++ mirror."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import one_amd
from oracle import reda_writer
from one_amd import _lib
from golden_util import load_dfa

import test_gpu_collect_text as CT
import test_gpu_extract_text as XT
import test_gpu_grep_text as GT

pytestmark = pytest.mark.gpu

CHUNK = CT.CHUNK
N = CT.N
ALL = 1 << 62
SENT = 0x5555555555555555
FIRST, LAST = 0, 1
WHICH = {FIRST: "first", LAST: "last"}
M64 = 2 ** 64
KERNEL = "k_sum_text"
_u8 = CT._u8


# the expectation -------------------------------------------------------------------------------

def _number(piece, last):
    """the piece's number, or None: its first / last maximal run of digits as a decimal, when there
    is one and it is below 2^64"""
    runs = re.findall(rb"[0-9]+", piece)
    if not runs:
        return None
    v = int(runs[-1 if last else 0])
    return v if v < M64 else None


def _items(name, text, delim=0x0A, m=ALL):
    """(n_lines, [(result, piece)]) in text order: extract_text's pieces under max_per_line = m,
    each with the result of collect_text's record for it"""
    x = XT._oracle(name, text, delim)
    w = CT._want(name, text, delim)
    first = np.concatenate([[0], np.cumsum(w.counts)]).astype(np.int64)
    out = []
    for k, got in enumerate(x.per_line):
        assert len(got) == w.counts[k], (name, k)
        res = w.result[first[k]:first[k + 1]]
        out += [(int(r), p) for r, p in zip(res[:m], got[:m])]
    return x.n_lines, out


def _reduce(items, n_bins, last):
    """stats[4, n_bins + 1] as uint64 from (result, piece) pairs, in Python integers"""
    slots = n_bins + 1
    cnt, tot, lo, hi = [0] * slots, [0] * slots, [M64 - 1] * slots, [0] * slots
    for r, piece in items:
        v = _number(piece, last)
        if v is None:
            continue
        s = r if 0 <= r < n_bins else n_bins
        cnt[s] += 1
        tot[s] = (tot[s] + v) % M64
        lo[s] = min(lo[s], v)
        hi[s] = max(hi[s], v)
    return np.array([cnt, tot, lo, hi], dtype=np.uint64)


def _merge(a, b):
    """what accumulate does: counts and sums added modulo 2^64, min of mins, max of maxes"""
    return np.stack([a[0] + b[0], a[1] + b[1], np.minimum(a[2], b[2]), np.maximum(a[3], b[3])])


def _empty(n_bins):
    return _reduce([], n_bins, False)


def _expect(name, text, n_bins, last, m=ALL, delim=0x0A):
    """(n_lines, n_items, n_numeric, stats)"""
    n_lines, items = _items(name, text, delim, m)
    stats = _reduce(items, n_bins, last)
    return n_lines, len(items), int(stats[0].sum()), stats


def _dev_text(text, shift=0):
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + len(text)]
    if len(text):
        dev.copy_(torch.from_numpy(_u8(text).copy()))
    return dev


def _host_stats(t):
    return t.cpu().numpy().view(np.uint64)


def _check(exe, name, text, n_bins, which, m=ALL, delim=b"\n", forms=("host", "dev"), where=None):
    """both forms of the verb against the expectation; returns it"""
    import torch
    want = _expect(name, text, n_bins, which == LAST, m, delim[0])
    kw = dict(which=WHICH[which], max_per_line=m, delim=delim)
    where = (where, name, n_bins, which, m)
    if "host" in forms:
        got = one_amd.sum_text(exe, text, n_bins, **kw)
        assert one_amd.last_kernel() == KERNEL
        assert got[:3] == want[:3], where + (got[:3], want[:3])
        assert got[3].dtype == np.uint64 and got[3].shape == (4, n_bins + 1)
        assert np.array_equal(got[3], want[3]), where
    if "dev" in forms:
        got = one_amd.sum_text(exe, _dev_text(text, 1), n_bins, **kw)
        assert one_amd.last_kernel() == KERNEL
        torch.cuda.synchronize()
        assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int64 for x in got)
        assert all(x.shape == (1,) for x in got[:3]) and got[3].shape == (4, n_bins + 1)
        assert tuple(x.item() for x in got[:3]) == want[:3], where
        assert np.array_equal(_host_stats(got[3]), want[3]), where
    return want


# 1 ---------------------------------------------------------------------------------------------
def test_sum_text_value_rule_and_wrap():
    """num3: 2^63 twice wraps the sum to 0 and beyond; 2^64 - 1 fits, 2^64 and 30 nines do not"""
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    rows = [b"x %d y" % 2 ** 63, b"%d" % 2 ** 63, b"q %d" % (2 ** 64 - 1), b"%d z" % 2 ** 64,
            b"0" * 26 + b"42", b"9" * 30, b"7a", b"no digit here"]
    text = b"\n".join(rows) + b"\n"
    n_bins = exe.info["max_result"] + 1
    n_lines, items = _items(name, text)
    assert n_lines == 8 and [p for _, p in items] == [
        b"%d" % 2 ** 63, b"%d" % 2 ** 63, b"%d" % (2 ** 64 - 1), b"%d" % 2 ** 64, b"0" * 26 + b"42",
        b"9" * 30, b"7a"]
    assert [r for r, _ in items] == [1, 1, 1, 1, 1, 1, 2]
    by_hand = _empty(n_bins)
    by_hand[:, 1] = [4, (2 ** 63 + 2 ** 63 + 2 ** 64 - 1 + 42) % M64, 42, 2 ** 64 - 1]
    by_hand[:, 2] = [1, 7, 7, 7]
    assert int(by_hand[1, 1]) == 41
    for which in (FIRST, LAST):
        want = _check(exe, name, text, n_bins, which)
        assert np.array_equal(want[3], by_hand)
        assert want[1] - want[2] == 2 and want[1] == 7


# 2 ---------------------------------------------------------------------------------------------
def _two_runs_dfa():
    """[a-d][0-9]+(x[0-9]+)? - the letter picks the result (1..4).  States: error, initial, and per
    letter: behind the letter, digits (accepting), behind the x, digits (accepting)"""
    equiv = np.full(256, 6, dtype=np.uint8)
    for k, ch in enumerate(b"abcd"):
        equiv[ch] = k
    equiv[0x30:0x3A] = 4
    equiv[ord("x")] = 5
    trans = np.zeros((18, 7), dtype=np.int64)
    results = [0] * 18
    for k in range(4):
        b = 2 + 4 * k
        trans[1][k] = b
        trans[b][4] = b + 1
        trans[b + 1][4] = b + 1
        trans[b + 1][5] = b + 2
        trans[b + 2][4] = b + 3
        trans[b + 3][4] = b + 3
        results[b + 1] = results[b + 3] = k + 1
    return reda_writer.write_reda(trans, results, equiv=equiv)


TWO = "sum_two_runs"


def _two_runs_text(seed=7):
    """CT._delims' lines over dots, a piece planted every 14 bytes: a letter, 1-4 digits and, in
    every second piece, an x and 1-4 digits more"""
    key = ("sum two runs", seed)
    if key not in CT._texts:
        rng = np.random.default_rng(seed)
        a = np.full(N, 0x2E, dtype=np.uint8)
        ends = CT._delims(N, seed)
        begin = 0
        for e in ends:
            for at in range(begin + 1, e - 11, 14):
                p = bytes([b"abcd"[rng.integers(0, 4)]]) + b"%d" % rng.integers(0, 10 ** int(rng.integers(1, 5)))
                if rng.integers(0, 2):
                    p += b"x%d" % rng.integers(0, 10 ** int(rng.integers(1, 5)))
                a[at:at + len(p)] = _u8(p)
            begin = e + 1
        a[ends] = 0x0A
        CT._texts[key] = bytes(a)
    return CT._texts[key]


def _two_runs_exe():
    if TWO not in CT._blobs:
        CT._blobs[TWO] = _two_runs_dfa()
    return one_amd.Executable(CT._blobs[TWO])


def test_sum_text_first_against_last():
    exe = _two_runs_exe()
    assert exe.info["max_result"] == 4
    text = _two_runs_text()
    _, items = _items(TWO, text)
    runs = np.array([len(re.findall(rb"[0-9]+", p)) for _, p in items])
    per = np.bincount([r for r, _ in items], minlength=5)
    assert (runs == 2).sum() >= 200 and (runs == 1).sum() >= 200 and set(runs) == {1, 2}
    assert per[0] == 0 and (per[1:] >= 100).all(), per
    a = _check(exe, TWO, text, 5, FIRST)
    b = _check(exe, TWO, text, 5, LAST)
    assert np.array_equal(a[3][0], b[3][0]) and a[2] == a[1] == len(items)
    assert (a[3][1, 1:5] != b[3][1, 1:5]).all()


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [TWO, "num3"])
def test_sum_text_every_cut(name):
    """n_bins cuts the slots - the last one merges what is cut; max_per_line cuts the items"""
    import torch
    if name == TWO:
        exe, text = _two_runs_exe(), _two_runs_text()
    else:
        exe, text = one_amd.Executable(load_dfa(name)), CT._dense(CT.PIECES[name]())
    top = exe.info["max_result"] + 1
    for which in (FIRST, LAST):
        full = None
        for n_bins in (top, 2, 1, 0):
            want = _check(exe, name, text, n_bins, which)[3]
            if full is None:
                full = want
                assert (full[0, 1:top] > 0).sum() >= 2 and full[0, top] == 0
            assert np.array_equal(want[:, :n_bins], full[:, :n_bins])
            cut = full[:, n_bins:]
            assert want[:, n_bins].tolist() == [int(cut[0].sum()), sum(int(v) for v in cut[1]) % M64,
                                                int(cut[2].min()), int(cut[3].max())]
        got = one_amd.sum_text(exe, text, which=WHICH[which])
        assert got[3].shape == (4, top + 1) and np.array_equal(got[3], full)
    seen = []
    for m in (ALL, 2, 1, 0):
        want = _check(exe, name, text, top, LAST, m=m)
        n_lines, items = _items(name, text, m=m)
        assert want[1] == len(items)
        n_matches = one_amd.extract_text(exe, _dev_text(text), max_per_line=m, out_cap=0)[1].item()
        assert n_matches == want[1], (m, n_matches, want[1])
        seen.append(want[1])
        if m == 0:
            assert want[1:3] == (0, 0) and np.array_equal(want[3], _empty(top))
    assert seen[0] > seen[1] > seen[2] > seen[3] == 0, seen
    torch.cuda.synchronize()


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", GT._PLACEMENT_ROWS)
def test_sum_text_under_placement(dfa, opts, info):
    from test_gpu_long_placements import FACTS
    blob = CT._blob(dfa)
    facts = one_amd.Executable(blob, device="none").info
    for k, v in FACTS.get(dfa, {}).items():
        assert facts[k] == v, (dfa, k, facts[k], v)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    text = GT._placement_text(dfa)
    assert len(text) == N and text[-1] != 0x0A
    n_bins = got_info["max_result"] + 1
    for which in (FIRST, LAST):
        want = _check(exe, dfa, text, n_bins, which, where=opts)
        if dfa in ("aab", "leaky"):
            # no digit anywhere: every item is looked at and none is counted
            assert want[2] == 0 and want[1] >= 2000 and np.array_equal(want[3], _empty(n_bins))
        else:
            assert want[2] >= 150, (dfa, want[1:3])
        # ... and cut in the middle of the results
        _check(exe, dfa, text, max(1, n_bins // 2), which, forms=("dev",), where=opts)


# 5 ---------------------------------------------------------------------------------------------
def _letter_digits(results):
    """one letter of abcd, then [0-9]+: error, initial, and per letter the state behind it and the
    accepting state of the digits"""
    equiv = np.full(256, 5, dtype=np.uint8)
    for k, ch in enumerate(b"abcd"):
        equiv[ch] = k
    equiv[0x30:0x3A] = 4
    trans = np.zeros((10, 6), dtype=np.int64)
    res = [0] * 10
    for k in range(4):
        trans[1][k] = 2 + 2 * k
        trans[2 + 2 * k][4] = 3 + 2 * k
        trans[3 + 2 * k][4] = 3 + 2 * k
        res[3 + 2 * k] = results[k]
    return reda_writer.write_reda(trans, res, equiv=equiv)


def _letter_digits_text(seed=5):
    a = _u8(b"abcd0123456789.")[np.random.default_rng(seed).integers(0, 15, N)].copy()
    a[CT._delims(N, seed)] = 0x0A
    return bytes(a)


def test_sum_text_lds_boundary():
    """results on both sides of redgpu_sum_lds_bins: LDS slots, global slots, and the "everything
    else" slot on either side"""
    lib = _lib.lib()
    probe = one_amd.Executable(_letter_digits((1, 2, 3, 4)), device="none")
    L = lib.redgpu_sum_lds_bins(probe._h)
    assert 8 <= L <= 512 and L % 4 == 0
    results = (L - 1, L, L + 1, 70000)
    name = "sum_letter_digits_%d" % L
    CT._blobs[name] = _letter_digits(results)
    exe = one_amd.Executable(CT._blobs[name])
    assert lib.redgpu_sum_lds_bins(exe._h) == L and exe.info["max_result"] == 70000
    text = _letter_digits_text()
    _, items = _items(name, text)
    # (among 11,000 random runs of digits a few are 2^64 and more: they are in no slot)
    per = np.bincount([r for r, p in items if _number(p, False) is not None], minlength=70001)
    assert all(per[r] > 1000 for r in results) and 0 <= len(items) - int(per.sum()) < 20
    for n_bins in (L - 1, L, L + 1, L + 2, 70001):
        want = _check(exe, name, text, n_bins, FIRST)
        assert int(want[3][0, n_bins]) == sum(int(per[r]) for r in results if r >= n_bins)
    _check(exe, name, text, L, LAST)


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CT._shapes()))
def test_sum_text_shapes(shape):
    text = CT._shapes()[shape]
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    n_bins = exe.info["max_result"] + 1
    for which in (FIRST, LAST):
        want = _check(exe, name, text, n_bins, which, where=shape)
        if shape in ("no delimiter", "empty", "one byte, no delimiter"):
            assert want[:3] == (0, 0, 0) and np.array_equal(want[3], _empty(n_bins))
        elif shape == "a match in the tail":
            short = _expect(name, CT.SHORT, n_bins, which == LAST)
            assert want[2] == 3 * short[2] > 0      # the tail's number is in no line
            assert np.array_equal(want[3][0], 3 * short[3][0])
        elif shape.startswith("a num3 match ends"):
            at = int(shape.rsplit(" ", 1)[1])
            assert (CT._want(name, text).end == at).sum() == 1


# 7 ---------------------------------------------------------------------------------------------
def test_sum_text_hot_slot_and_rounds():
    """one chunk and five rounds with uneven counts; every line the same slot; 22 items a line"""
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    n_bins = exe.info["max_result"] + 1
    text = b"".join(b"%d " % (1000 + i) * (i % 10) + b"\n" for i in range(300))
    assert len(text) < CHUNK
    want = _check(exe, name, text, n_bins, FIRST)
    assert want[2] == sum(i % 10 for i in range(300)) == int(want[3][0, 1])
    assert int(want[3][1, 1]) == sum((1000 + i) * (i % 10) for i in range(300))
    # every line has one number, all of one result: ONE slot takes every item of every round
    text = b"".join(b"x" * (i % 90) + b" %d\n" % (7 * i + 1) for i in range(1200))
    assert len(text) > 3 * CHUNK
    for n_bins2 in (2, 1, 0):
        want = _check(exe, name, text, n_bins2, LAST)
        assert int(want[3][0].max()) == 1200 == want[2]
        assert (int(want[3][2].min()), int(want[3][3].max())) == (1, 7 * 1199 + 1)
    line = b"123 4567 89012 " * 7 + b"345\n"
    text = line * (N // len(line)) + b"12 tail"
    for which in (FIRST, LAST):
        want = _check(exe, name, text, n_bins, which)
        assert want[2] == 22 * (N // len(line)) == int(want[3][0, 1])
        assert want[3][:, 1].tolist()[2:] == [123, 89012]


# 8 ---------------------------------------------------------------------------------------------
def test_sum_text_above_the_grid():
    """160 MiB = 10,240 chunks against at most CUs x 2 workgroups: every wave takes further chunks,
    a workgroup's LDS front lives across all of them and is flushed once.  Everything stays on the
    device: a 1 MiB block that ends in a delimiter, tiled."""
    import torch
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 16
    block = CT._dense(b"12345a", seed=3, n=block_len, end_in_delim=True)
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    n_bins = exe.info["max_result"] + 1
    for which in (FIRST, LAST):
        n_lines, n_items, n_numeric, st = _expect(name, block, n_bins, which == LAST)
        assert n_numeric > 10000
        got = one_amd.sum_text(exe, dev, n_bins, which=WHICH[which])
        assert one_amd.last_kernel() == KERNEL
        assert tuple(x.item() for x in got[:3]) == (n_lines * tiles, n_items * tiles, n_numeric * tiles)
        out = _host_stats(got[3])
        assert np.array_equal(out[0], st[0] * np.uint64(tiles))
        assert np.array_equal(out[1], st[1] * np.uint64(tiles))       # (modulo 2^64 on both sides)
        assert np.array_equal(out[2:], st[2:])


# 9 ---------------------------------------------------------------------------------------------
def _raw(exe, form, which, data, n_bins, accumulate, stats, *, keep=(True, True, True), m=ALL,
         delim=0x0A, at=0):
    """redgpu_sum_text / _dev through ctypes: stats is a flat numpy uint64 array (host) or a flat
    int64 CUDA tensor (dev), the words from `at` on are the call's; returns the three scalars"""
    import torch
    lib = _lib.lib()
    if form == "host":
        sc = [C.c_uint64(SENT) for _ in range(3)]
        rc = lib.redgpu_sum_text(exe._h, which, data, len(data), delim, m, n_bins, accumulate,
                                 *[C.byref(s) if k else None for s, k in zip(sc, keep)],
                                 stats.ctypes.data + 8 * at)
        assert rc == 0, lib.redgpu_last_error()
        return tuple(s.value for s in sc)
    cnt = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    rc = lib.redgpu_sum_text_dev(exe._h, which, data.data_ptr() if data.numel() else None,
                                 data.numel(), delim, m, n_bins, accumulate,
                                 *[cnt.data_ptr() + 8 * i if k else None for i, k in enumerate(keep)],
                                 stats.data_ptr() + 8 * at, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return tuple(cnt.tolist())


@pytest.mark.parametrize("form,shift", [("host", 0), ("dev", 0), ("dev", 1), ("dev", 7), ("dev", 15)])
def test_sum_text_accumulate(form, shift):
    """two texts into one table: merged under accumulate (a count that carries past 2^32, a sum that
    wraps, a prefilled min that survives, a prefilled max that is replaced), overwritten without;
    the words around the call's 4 x (n_bins + 1) stay as they were"""
    import torch
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    # (numbers well above 17 in both slots, so that a prefilled min can survive)
    texts = [b"".join(b"w %d q %da\n" % (1000 + i + 7 * k, 5000 + 3 * i + k) for i in range(6000))
             for k in (0, 1)]
    assert all(len(t) > 4 * CHUNK for t in texts)
    n_bins, at = 3, 5
    slots = n_bins + 1
    room = at + 4 * slots + 7
    for which in (FIRST, LAST):
        wants = [_expect(name, t, n_bins, which == LAST) for t in texts]
        assert wants[0][2] > 500 and not np.array_equal(wants[0][3], wants[1][3])
        assert 17 < int(wants[0][3][2, 2]) and int(wants[0][3][3, 2]) < 2 ** 40
        assert wants[0][3][0, 1:3].tolist() == [6000, 6000]
        table = _empty(n_bins)
        table[:, 2] = [2 ** 32 - 1, M64 - 5, 17, 1]     # slot 2: carry, wrap, min stays, max goes
        table[:, 1] = [1, 10, 2 ** 63, 2 ** 63]         # slot 1: min goes, max stays
        start = np.full(room, SENT, dtype=np.uint64)
        start[at:at + 4 * slots] = table.reshape(-1)
        data = [t if form == "host" else _dev_text(t, shift) for t in texts]
        stats = start.copy() if form == "host" else torch.from_numpy(start.view(np.int64).copy()).cuda()
        host = lambda: stats if form == "host" else _host_stats(stats)  # noqa: E731
        expect = start.copy()
        for k in (0, 1):
            got = _raw(exe, form, which, data[k], n_bins, 1, stats, at=at)
            assert got == wants[k][:3], (which, k)
            table = _merge(table, wants[k][3])
            expect[at:at + 4 * slots] = table.reshape(-1)
            assert np.array_equal(host(), expect), (which, k)
        assert int(table[0, 2]) > 2 ** 32 and int(table[1, 2]) < 2 ** 40
        assert int(table[2, 2]) == 17 and int(table[3, 2]) > 1
        assert int(table[2, 1]) < 2 ** 63 and int(table[3, 1]) == 2 ** 63
        # accumulate = 0 overwrites all 4 x (n_bins + 1) words and nothing else
        assert _raw(exe, form, which, data[1], n_bins, 0, stats, at=at) == wants[1][:3]
        expect[at:at + 4 * slots] = wants[1][3].reshape(-1)
        assert np.array_equal(host(), expect) and (expect[:at] == SENT).all()
        assert (expect[at + 4 * slots:] == SENT).all()
    # the verb's into=
    into = None
    for t, d in zip(texts, data):
        into = one_amd.sum_text(exe, t if form == "host" else d, n_bins, which="last", into=into)[3]
    got = into if form == "host" else _host_stats(into)
    assert np.array_equal(got, _merge(wants[0][3], wants[1][3]))


# 10 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_sum_text_optional_outputs_null(form, delim):
    import torch
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]()).replace(b"\n", delim)
    n_bins = 2
    data = text if form == "host" else _dev_text(text)
    want = _expect(name, text, n_bins, False, delim=delim[0])
    assert want[0] >= 648 and want[2] > 100
    for keep in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        stats = np.full(4 * (n_bins + 1), SENT, dtype=np.uint64)
        if form == "dev":
            stats = torch.from_numpy(stats.view(np.int64).copy()).cuda()
        got = _raw(exe, form, FIRST, data, n_bins, 0, stats, keep=keep, delim=delim[0])
        assert got == tuple(w if k else SENT for w, k in zip(want[:3], keep)), keep
        out = stats if form == "host" else _host_stats(stats)
        assert np.array_equal(out.reshape(4, n_bins + 1), want[3]), keep
    # ... and with '\n' the same text has no line at all
    assert one_amd.sum_text(exe, text, n_bins)[:3] == (0, 0, 0)


def test_sum_text_empty_and_lineless_on_the_device():
    """the _dev form writes the zero counts and empties the slots on the stream - or leaves them
    alone under accumulate"""
    import torch
    exe = one_amd.Executable(load_dfa("num3"))
    for text in (b"", b"123, and no line end"):
        dev = torch.from_numpy(_u8(text).copy()).cuda()
        for which in (FIRST, LAST):
            stats = torch.full((10,), 77, dtype=torch.int64, device="cuda")
            assert _raw(exe, "dev", which, dev, 1, 1, stats, at=1) == (0, 0, 0)
            assert stats.tolist() == [77] * 10
            assert _raw(exe, "dev", which, dev, 1, 0, stats, at=1) == (0, 0, 0)
            assert stats.tolist() == [77, 0, 0, 0, 0, -1, -1, 0, 0, 77]
            assert one_amd.last_kernel() == KERNEL
    host = one_amd.sum_text(exe, b"", 1)
    assert host[:3] == (0, 0, 0) and np.array_equal(host[3], _empty(1))


# 11 --------------------------------------------------------------------------------------------
def test_sum_text_identities_on_the_gpu():
    """where every piece is numeric the count row is tally_text's histogram of the matches"""
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    n_bins = exe.info["max_result"] + 1
    tally = one_amd.tally_text(exe, text, n_bins)
    for which in ("first", "last"):
        got = one_amd.sum_text(exe, text, n_bins, which=which)
        assert got[:2] == tally[:2] and got[2] == got[1] > 500
        assert np.array_equal(got[3][0], tally[2])


# 12 --------------------------------------------------------------------------------------------
def test_sum_text_two_streams_and_threads():
    import torch
    names = ("num3", TWO)
    exes = [one_amd.Executable(load_dfa("num3")), _two_runs_exe()]
    texts = [CT._dense(CT.PIECES["num3"](), seed=2), _two_runs_text()]
    n_bins = [e.info["max_result"] + 1 for e in exes]
    wants = [_expect(n, t, nb, True) for n, t, nb in zip(names, texts, n_bins)]
    assert wants[0][:3] != wants[1][:3]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def same(got, want):
        assert tuple(int(x) for x in got[:3]) == want[:3]
        g = _host_stats(got[3]) if isinstance(got[3], torch.Tensor) else got[3]
        assert np.array_equal(g, want[3])
        return g.tobytes()

    outs = []
    for st, exe, d, nb in zip(streams, exes, devs, n_bins):
        with torch.cuda.stream(st):
            outs.append(one_amd.sum_text(exe, d, nb, which="last"))
    torch.cuda.synchronize()
    firsts = [same(got, w) for got, w in zip(outs, wants)]
    errors = []

    def work(exe, t, d, st, nb, w, first):
        # each thread on its own stream, with stats of its own: the device form, the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.sum_text(exe, d, nb, which="last")
                    st.synchronize()
                assert same(got, w) == first            # bit-identical from run to run
                assert same(one_amd.sum_text(exe, t, nb, which="last"), w) == first
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    args = list(zip(exes, texts, devs, streams, n_bins, wants, firsts))
    more = [torch.cuda.Stream() for _ in args]
    args += [a[:3] + (s,) + a[4:] for a, s in zip(args, more)]
    th = [threading.Thread(target=work, args=a) for a in args]
    assert len(th) == 4
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# 13 --------------------------------------------------------------------------------------------
def test_sum_text_cpp_mirror(tmp_path):
    """redgpu::sumText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "sum_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "sum_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    exe = _two_runs_exe()
    del exe
    text = _two_runs_text()
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = tmp_path / "two_runs.reda"
    dfa.write_bytes(CT._blobs[TWO])
    for n_bins in (5, 2):
        out = subprocess.run([prog, str(dfa), str(path), str(n_bins)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = {r.split()[0]: [int(v) for v in r.split()[1:]] for r in out.stdout.split("\n") if r}
        for block, last, m in (("first", False, ALL), ("last", True, ALL), ("one", False, 1),
                               ("default", False, ALL)):
            want = _expect(TWO, text, n_bins, last, m)
            assert rows[block + "_scalars"] == list(want[:3]), block
            for k, key in enumerate(("count", "sum", "min", "max")):
                assert rows[block + "_" + key] == [int(v) for v in want[3][k]], (block, key)
        assert rows["first_sum"] != rows["last_sum"] and rows["one_scalars"][1] < rows["first_scalars"][1]
