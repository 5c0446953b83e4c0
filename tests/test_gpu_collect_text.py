"""collect_text (redgpu_collect_text[_dev]): grep -o - every match of every line of a raw text, as
compact records in text order.  All seven outputs are exact against sampleLines' loop
(oracle.split_lines_loop) plus the CPU oracle's collect per line (and the reference's, when it is
built): the nine DFAs over a dense text, every table placement, the chunk-border shapes, rounds of
64 lines with uneven counts, truncation at every kind of cap, optional outputs, the device form at
odd pointer offsets, the composed route on the GPU, other delimiters, a text of more chunks than
the grid has waves, concurrent streams and threads, and the C++ mirror."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from one_amd import workloads as W
from golden_util import load_dfa

import test_gpu_grep_text as GT
import test_gpu_list_verbs as LV
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

CHUNK = 16384
N = 4 * CHUNK + 5
SENT = 0x55
PIECES = dict(GT.PIECES)
PIECES.update({"num3": lambda: b"12345a", "set5": lambda: b"?"})
OPEN = ["err", "aab", "ale", "log100", "num3", "set5"]   # several matches in a line
CLOSED = ["dotstar_err", "newyork", "uri"]               # suffix-closed: one match per hit line
NINE = OPEN + CLOSED
DTYPES = (np.uint64, np.uint64, np.int32, np.uint64, np.uint64)
NAMES = ("line", "begin", "result", "start", "end")

_blobs = {}
_oracles = {}
_texts = {}
_wants = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _blob(name):
    if name not in _blobs:
        _blobs[name] = LV.DFAS[name]() if name in LV.DFAS else load_dfa(name)
    return _blobs[name]


def _delims(n, seed):
    """the delimiter positions of test_gpu_grep_text._standard: gaps of 1-199 bytes"""
    rng = np.random.default_rng(seed)
    ends, pos = [], -1
    while True:
        pos += int(rng.integers(1, 200))
        if pos >= n:
            return ends
        ends.append(pos)


def _planted_lines(ends, n):
    """(begin, end) of the lines _standard plants: every line that crosses an odd multiple of
    16384 and every third other line, never a line that crosses an even multiple"""
    begin, other = 0, 0
    for e in ends:
        crossed = [m for m in range(CHUNK, n, CHUNK) if begin < m <= e]
        if crossed:
            plant = any((m // CHUNK) % 2 == 1 for m in crossed)
        else:
            plant = other % 3 == 0
            other += 1
        if plant:
            yield begin, e
        begin = e + 1


def _dense(piece: bytes, seed=1, n=N, end_in_delim=False):
    """_standard's text with its planted lines FULL of the piece: repeated from begin + 1 on,
    every len(piece) + 7 bytes, while it fits in front of the delimiter"""
    key = ("dense", piece, seed, n, end_in_delim)
    if key not in _texts:
        a = W.alphabet_bytes(n, seed).copy()
        a[a == 0x0A] = 0x20
        ends = _delims(n, seed)
        if end_in_delim and ends[-1] != n - 1:
            ends.append(n - 1)
        a[ends] = 0x0A
        p = _u8(piece)
        for begin, e in _planted_lines(ends, n):
            if e - begin >= len(p):
                for at in range(begin + 1, e - len(p) + 1, len(p) + 7):
                    a[at:at + len(p)] = p
        _texts[key] = bytes(a)
    return _texts[key]


def _random_text(kind, seed=1, n=N):
    """_standard's delimiters over random bytes (the random DFAs) or a / b / . (leaky)"""
    key = ("random", kind, seed, n)
    if key not in _texts:
        if kind == "leaky":
            a = _u8(b"ab.")[np.random.default_rng(seed + 1).integers(0, 3, n)].copy()
        else:
            a = W.random_bytes(n, seed).copy()
            a[a == 0x0A] = 0x20
        a[_delims(n, seed)] = 0x0A
        _texts[key] = bytes(a)
    return _texts[key]


class _Want:
    """the oracle's answer for (DFA, text, delimiter): the seven outputs and the per-line counts"""

    def __init__(self, name, text, delim):
        if name not in _oracles:
            _oracles[name] = O.CpuOracle(_blob(name))
        cpu = _oracles[name]
        lines = O.split_lines_loop(text, delim)
        self.n_lines = len(lines)
        # collect on every line alone: the lines back to back WITHOUT their delimiters, as a batch
        arr = _u8(b"".join(lines) + b"\0")
        bare = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
        self.begins = np.cumsum([0] + [len(x) + 1 for x in lines]).astype(np.uint64)[:len(lines)]
        cap = 64
        counts, r, s, e = cpu.collect_batch(arr, cap, offsets=bare)
        if len(lines) and int(counts.max()) >= cap:
            cap = int(counts.max()) + 1
            counts, r, s, e = cpu.collect_batch(arr, cap, offsets=bare)
        assert not len(lines) or cap > int(counts.max())
        self.counts = counts.astype(np.int64)
        keep = np.arange(cap)[None, :] < self.counts[:, None] if len(lines) else np.zeros((0, cap), bool)
        which = np.nonzero(keep)[0]                         # row-major: line order, then match order
        self.line = which.astype(np.uint64)
        self.begin = self.begins[which] if len(which) else np.zeros(0, np.uint64)
        self.result = r[keep]
        # (collect_batch's positions are relative to the line: shift them by the line's begin)
        self.start = s[keep] + self.begin
        self.end = e[keep] + self.begin
        self.n = len(self.line)
        # ... which is what the one-text call gives, and the reference too
        for k in range(0, len(lines), 97):
            recs, cnt = cpu.collect(lines[k], cap)
            assert cnt == self.counts[k]
            b = int(self.begins[k])
            mine = np.flatnonzero(self.line == k)
            assert [(int(self.result[j]), int(self.start[j]) - b, int(self.end[j]) - b)
                    for j in mine] == recs
        if O.have_ref():
            for k in range(0, len(lines), 5):
                recs, cnt = O.ref_collect(_blob(name), lines[k], cap)
                b = int(self.begins[k])
                mine = np.flatnonzero(self.line == k)
                assert cnt == self.counts[k] and recs[:cnt] == [
                    (int(self.result[j]), int(self.start[j]) - b, int(self.end[j]) - b) for j in mine]

    def arrays(self):
        return (self.line, self.begin, self.result, self.start, self.end)

    def crossing_both_sides(self, text_len):
        """lines that cross a multiple of 16384 with matches on both sides of it: one that begins
        in front of the border (it may reach across), one that begins at or behind it"""
        k = 0
        for m in range(CHUNK, text_len, CHUNK):
            left = set(self.line[self.start < m].tolist())
            right = set(self.line[self.start >= m].tolist())
            k += len(left & right)
        return k


def _want(name, text, delim=0x0A):
    key = (name, text, delim)
    if key not in _wants:
        _wants[key] = _Want(name, text, delim)
    return _wants[key]


def _same(got, want, upto=None, where=None):
    assert int(got[0]) == want.n_lines and int(got[1]) == want.n, (where, got[:2], want.n_lines, want.n)
    k = want.n if upto is None else min(upto, want.n)
    for g, w, what in zip(got[2:], want.arrays(), NAMES):
        g = np.asarray(g)
        assert len(g) == k, (where, what, len(g), k)
        assert np.array_equal(g.astype(w.dtype), w[:k]), (where, what)


def _guard(name, want, text):
    c = want.counts
    if name in OPEN:
        assert (c >= 2).sum() >= 150 and (c >= 5).sum() >= 70, (name, (c >= 2).sum(), (c >= 5).sum())
        assert want.crossing_both_sides(len(text)) >= 1, name
    else:
        assert (c >= 1).sum() >= 100 and (c >= 2).sum() == 0, (name, (c >= 1).sum())


# what the issue's table says of the dense text (matches, lines with >= 2, with >= 5, the largest
# count of a line, crossing lines with matches on both sides of the border)
TABLE = {
    "err": (1865, 197, 159, 17, 2), "aab": (2257, 202, 170, 20, 2), "ale": (2055, 200, 167, 18, 2),
    "log100": (741, 165, 77, 7, 1), "num3": (10014, 608, 542, 38, 3),
    "set5": (10759, 604, 554, 42, 3), "dotstar_err": (210, 0, 0, 1, 0),
    "newyork": (209, 0, 0, 1, 0), "uri": (163, 0, 0, 1, 0),
}


@pytest.mark.parametrize("name", NINE)
def test_collect_text_matrix_vs_oracle(name):
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    want = _want(name, text)
    _guard(name, want, text)
    c = want.counts
    assert want.n_lines == 648
    assert (want.n, int((c >= 2).sum()), int((c >= 5).sum()), int(c.max()),
            want.crossing_both_sides(len(text))) == TABLE[name]
    got = one_amd.collect_text(exe, text)
    assert one_amd.last_kernel() == "k_collect_text"
    _same(got, want, where=name)
    # the counts alone, and without the positions
    got = one_amd.collect_text(exe, text, cap=0)
    assert got[:2] == (want.n_lines, want.n) and all(len(x) == 0 for x in got[2:])
    got = one_amd.collect_text(exe, text, want_positions=False)
    assert got[5] is None and got[6] is None
    for g, w in zip(got[2:5], want.arrays()[:3]):
        assert np.array_equal(g, w)


_MORE_ROWS = [pytest.param(*p.values[:3], id=p.id) for p in LV.TABLE
              if p.values[0] in ("syn256", "rnd72", "leaky") and not p.values[1]]


@pytest.mark.parametrize("dfa,opts,info", LP.ROWS + _MORE_ROWS)
def test_collect_text_under_placement(dfa, opts, info):
    blob = _blob(dfa)
    facts = one_amd.Executable(blob, device="none").info
    for k, v in LP.FACTS.get(dfa, {}).items():
        assert facts[k] == v, (dfa, k, facts[k], v)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    if dfa in LP.PIECES:
        text = _dense(LP.PIECES[dfa][0])
    else:
        text = _random_text("leaky" if dfa == "leaky" else "random")
    want = _want(dfa, text)
    # not vacuous: hit lines in every chunk, and lines without a match among them (the hit bitmap
    # is not the delimiter bitmap)
    assert want.n >= 50 and (want.counts == 0).sum() >= 5, (dfa, want.n)
    hit_begins = want.begins[want.counts > 0]
    assert len(set((hit_begins // CHUNK).tolist())) >= 4, dfa
    got = one_amd.collect_text(exe, text)
    assert one_amd.last_kernel() == "k_collect_text"
    _same(got, want, where=(dfa, opts))
    _same(one_amd.collect_text(exe, text, cap=want.n // 2), want, upto=want.n // 2, where=(dfa, opts))


UNIT = b"b 123 aab 4567\n"        # 15 bytes: two matches of num3, one of aab
SHORT = b"an aab 123 here\nnothing\n\n12345a aab\nno\n"


def _body(n, end_match):
    """n bytes of UNIT lines and a last line WITHOUT its delimiter - z's, ending in "123" or "aab"
    under end_match"""
    units, rem = divmod(n, len(UNIT))
    if rem < 4:
        units, rem = units - 1, rem + len(UNIT)
    tail = b"z" * (rem - 3) + end_match if end_match else b"z" * rem
    out = UNIT * units + tail
    assert len(out) == n
    return out


def _shapes():
    out = {}
    for at in (CHUNK - 1, CHUNK, CHUNK + 1):
        # (the line behind a delimiter at 16383 begins exactly at 16384)
        out["delimiter at %d" % at] = _body(at, None) + b"\n" + UNIT * 3
        out["a num3 match ends in front of a delimiter at %d" % at] = _body(at, b"123") + b"\n" + UNIT * 3
        out["an aab match ends in front of a delimiter at %d" % at] = _body(at, b"aab") + b"\n" + UNIT * 3
    out["300 empty lines across a border"] = (_body(CHUNK - 150, None) + b"\n" * 300
                                              + b"aab 123 aab\n" + UNIT)
    out["a chunk of delimiters alone"] = (_body(CHUNK - 1, b"123") + b"\n" + b"\n" * CHUNK
                                          + b"x aab 123 4567\n" + UNIT * 2)
    out["one 40 KiB line"] = SHORT + b"123 aab " * 5120 + b"\n" + SHORT
    out["a match in the tail"] = SHORT * 3 + b"an aab and 123 in the tail"
    out["no delimiter"] = b"aab 123 without a line end"
    out["empty"] = b""
    out["one byte, a delimiter"] = b"\n"
    out["one byte, no delimiter"] = b"a"
    assert out["delimiter at 16383"][CHUNK - 1] == 0x0A and out["delimiter at 16384"][CHUNK] == 0x0A
    assert out["a chunk of delimiters alone"][CHUNK:2 * CHUNK] == b"\n" * CHUNK
    assert out["300 empty lines across a border"][CHUNK - 150:CHUNK + 150] == b"\n" * 300
    assert len(SHORT) + 40960 > 2 * CHUNK + len(SHORT)
    return out


@pytest.mark.parametrize("shape", list(_shapes()))
def test_collect_text_shapes(shape):
    text = _shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        want = _want(name, text)
        if shape in ("no delimiter", "empty", "one byte, no delimiter"):
            assert (want.n_lines, want.n) == (0, 0)
        elif shape == "one byte, a delimiter":
            assert (want.n_lines, want.n) == (1, 0)
        elif shape == "a match in the tail":
            assert want.n == 3 * _want(name, SHORT).n > 0     # the tail's matches are in no line
        elif shape == "one 40 KiB line":
            # thousands of records in ONE line, in each of its three chunks
            big = want.counts.max()
            assert big >= 5120 and want.crossing_both_sides(len(text)) == 2, (name, big)
        else:
            assert want.n > 1000, (shape, name, want.n)
        if shape.startswith("a %s match ends" % name):
            at = int(shape.rsplit(" ", 1)[1])
            assert (want.end == at).sum() == 1, (shape, name)
        got = one_amd.collect_text(exe, text)
        assert one_amd.last_kernel() == "k_collect_text"
        _same(got, want, where=(shape, name))
        _same(one_amd.collect_text(exe, text, cap=0), want, upto=0, where=(shape, name))


def test_collect_text_rounds_with_uneven_counts():
    """one chunk, 300 lines (five rounds of 64), line i with i % 10 matches: the prefix inside a
    round and the carry between rounds differ from lane to lane"""
    text = b"".join(b"aab " * (i % 10) + b"\n" for i in range(300))
    assert len(text) < CHUNK and max(len(x) for x in text.split(b"\n")) <= 40
    exe = one_amd.Executable(load_dfa("aab"))
    want = _want("aab", text)
    assert want.counts.tolist() == [i % 10 for i in range(300)]
    _same(one_amd.collect_text(exe, text), want)
    for cap in (1, 44, 45, 46, 290, 1000, want.n - 1):
        _same(one_amd.collect_text(exe, text, cap=cap), want, upto=cap, where=cap)


def _raw_host(exe, text, cap, room, keep=range(5), n_lines=True, delim=0x0A):
    """redgpu_collect_text through ctypes: sentinel-filled arrays of `room` entries"""
    lib = _lib.lib()
    arrs = [np.full(room, SENT, dtype=dt) if k in keep else None for k, dt in enumerate(DTYPES)]
    nm, nl = C.c_uint64(SENT), C.c_uint64(SENT)
    rc = lib.redgpu_collect_text(exe._h, text, len(text), delim, cap, C.byref(nl) if n_lines else None,
                                 C.byref(nm), *[a.ctypes.data if a is not None else None for a in arrs])
    assert rc == 0, lib.redgpu_last_error()
    return nl.value, nm.value, arrs


def _raw_dev(exe, dev, cap, room, delim=0x0A):
    """redgpu_collect_text_dev: sentinel-filled tensors of `room` entries, everything on the device"""
    import torch
    lib = _lib.lib()
    outs = [torch.full((room,), SENT, dtype=torch.int32 if dt is np.int32 else torch.int64,
                       device="cuda") for dt in DTYPES]
    cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rc = lib.redgpu_collect_text_dev(exe._h, dev.data_ptr() if dev.numel() else None, dev.numel(),
                                     delim, cap, cnt.data_ptr(), cnt.data_ptr() + 8,
                                     *[o.data_ptr() for o in outs],
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return cnt.tolist(), [o.cpu().numpy() for o in outs]


def _prefix_and_sentinels(arrs, want, cap, where):
    k = min(want.n, cap)
    for a, w, what in zip(arrs, want.arrays(), NAMES):
        assert np.array_equal(a[:k], w[:k].astype(a.dtype)), (where, what)
        assert (a[k:] == SENT).all(), (where, what)


def test_collect_text_truncation():
    import torch
    name = "num3"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    want = _want(name, text)
    n = want.n
    cum = np.concatenate([[0], np.cumsum(want.counts)])      # records in front of line k
    inside_line = int(cum[np.flatnonzero(want.counts >= 3)[5]]) + 1
    hit = np.flatnonzero(want.counts > 0)
    inside_round = int(cum[hit[100]])                        # the 37th hit line of the second round
    finish = want.begins + np.array([len(x) for x in O.split_lines_loop(text)], dtype=np.uint64)
    chunk1 = int(want.counts[finish < CHUNK].sum())          # matchBases of chunk 1
    assert 0 < chunk1 < n and 64 < (finish[hit] < CHUNK).sum() and hit[100] < (finish < CHUNK).sum()
    caps = [0, 1, n - 1, n, n + 1, inside_line, inside_round, chunk1 - 1, chunk1, chunk1 + 1]
    assert len(set(caps)) == len(caps)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    for cap in caps:
        nl, nm, arrs = _raw_host(exe, text, cap, n + 8)
        assert (nl, nm) == (want.n_lines, n), cap
        _prefix_and_sentinels(arrs, want, cap, ("host", cap))
        cnt, outs = _raw_dev(exe, dev, cap, n + 8)
        assert cnt == [want.n_lines, n], cap
        _prefix_and_sentinels(outs, want, cap, ("dev", cap))
        _same(one_amd.collect_text(exe, text, cap=cap), want, upto=cap, where=cap)


def test_collect_text_some_arrays_null():
    """each of the five arrays, and n_lines, may be NULL on its own"""
    name = "aab"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    want = _want(name, text)
    for keep in ([0], [1], [2], [3], [4], [1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4],
                 [0, 1, 2, 3], [0, 2], []):
        for n_lines in (True, False):
            nl, nm, arrs = _raw_host(exe, text, want.n, want.n, keep=keep, n_lines=n_lines)
            assert nm == want.n and nl == (want.n_lines if n_lines else SENT)
            for k in keep:
                assert np.array_equal(arrs[k], want.arrays()[k].astype(DTYPES[k])), (keep, k)


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("name", ["num3", "log100"])
def test_collect_text_device_form(name, shift):
    """everything device-resident, the text at any offset from a 16-byte boundary"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    want = _want(name, text)
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(_u8(text).copy()))
    assert dev.data_ptr() % 16 == shift
    for cap in (want.n + 8, want.n // 3):
        cnt, outs = _raw_dev(exe, dev, cap, want.n + 8)
        assert one_amd.last_kernel() == "k_collect_text"
        assert cnt == [want.n_lines, want.n]
        _prefix_and_sentinels(outs, want, cap, (name, shift, cap))
    # the verb: the counts come back as tensors
    out = one_amd.collect_text(exe, dev, cap=want.n)
    torch.cuda.synchronize()
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in out)
    assert out[0].shape == (1,) and out[1].shape == (1,) and out[0].dtype == torch.int64
    _same((out[0].item(), out[1].item()) + tuple(x.cpu().numpy() for x in out[2:]), want)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_text(exe, dev)                      # the device form needs its cap


def test_collect_text_empty_and_lineless_on_the_device():
    """the _dev form writes both zero counts on the stream"""
    import torch
    exe = one_amd.Executable(load_dfa("aab"))
    for text in (b"", b"aab, and no line end"):
        dev = torch.from_numpy(_u8(text).copy()).cuda()
        cnt, outs = _raw_dev(exe, dev, 4, 4)
        assert cnt == [0, 0] and all((o == SENT).all() for o in outs)


@pytest.mark.parametrize("name", ["num3", "log100"])
def test_collect_text_equals_the_composed_route(name):
    """split_lines + collect_batch(cap = 64, stride = 1), compacted in numpy - on the GPU"""
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    offs, n_lines = one_amd.split_lines(exe, text)
    counts, r, s, e = one_amd.collect_batch(exe, text, 64, offsets=offs, stride=1)
    assert int(counts.max()) < 64 and int(counts.sum()) > 500
    keep = np.arange(64)[None, :] < counts.astype(np.int64)[:, None]
    which = np.nonzero(keep)[0]
    begin = offs[:-1][which]
    got = one_amd.collect_text(exe, text)
    assert got[:2] == (n_lines, int(counts.sum()))
    for g, w in zip(got[2:], (which.astype(np.uint64), begin, r[keep], s[keep] + begin, e[keep] + begin)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("delim", [b"\x00", b";"])
def test_collect_text_other_delimiter(delim):
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]()).replace(b"\n", delim)
    want = _want(name, text, delim[0])
    assert want.n_lines >= 648 and want.n > 1000 and (want.counts >= 2).sum() >= 150
    _same(one_amd.collect_text(exe, text, delim=delim), want)
    # ... and with '\n' the same text has no line at all
    assert one_amd.collect_text(exe, text)[:2] == (0, 0)


def test_collect_text_above_the_grid():
    """160 MiB = 10,240 chunks.  k_ct_count runs at most CUs x 2 workgroups of 16 waves (err's table
    is 20 KB: two workgroups per CU) - 8,192 waves on 256 CUs - and k_ct_write CUs x 2 of 8 waves:
    every wave of both passes takes a second chunk.  Everything stays on the device: a 1 MiB block
    that ends in a delimiter, tiled; the expected records are the block's, tiled."""
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 16
    block = _dense(PIECES[name](), seed=3, n=block_len, end_in_delim=True)
    assert block[-1] == 0x0A
    want = _want(name, block)
    assert want.n > 10000 and (want.counts >= 2).sum() > 1000
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    total = want.n * tiles
    out = one_amd.collect_text(exe, dev, cap=total)
    assert one_amd.last_kernel() == "k_collect_text"
    t = torch.arange(tiles, dtype=torch.int64, device="cuda").repeat_interleave(want.n)
    shift = (0, 1, None, 1, 1)
    assert out[0].item() == want.n_lines * tiles and out[1].item() == total
    for g, w, sh, what in zip(out[2:], want.arrays(), shift, NAMES):
        exp = torch.from_numpy(np.tile(w.astype(np.int32 if sh is None else np.int64), tiles)).cuda()
        if what == "line":
            exp += t * want.n_lines
        elif sh:
            exp += t * block_len
        assert torch.equal(g, exp), what


def test_collect_text_two_streams_and_threads():
    import torch
    names = ("num3", "err")
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [_dense(PIECES[n](), seed=2 + k) for k, n in enumerate(names)]
    wants = [_want(n, t) for n, t in zip(names, texts)]
    assert wants[0].n != wants[1].n
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def host(got):
        k = int(got[1].item())
        return (int(got[0].item()), k) + tuple(x[:k].cpu().numpy() for x in got[2:])

    outs = []
    for st, exe, d, w in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.collect_text(exe, d, cap=w.n + 3))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        _same(host(got), w)
    errors = []

    def work(exe, t, d, st, w):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.collect_text(exe, d, cap=w.n + 3)
                    st.synchronize()
                _same(host(got), w)
                _same(one_amd.collect_text(exe, t), w)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_collect_text_cpp_mirror(tmp_path):
    """redgpu::collectText / collectTextCount (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "collect_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "collect_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "num3"
    text = _dense(PIECES[name]())
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    want = _want(name, text)
    # (the mirror's first room is len / 64 + 16 = 1040 records: this text needs the retry)
    assert want.n > len(text) // 64 + 16
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    for cap in (1 << 62, 7):
        out = subprocess.run([prog, dfa, str(path), str(cap)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.split("\n")
        k = min(cap, want.n)
        assert rows[0] == "count %d %d" % (want.n, want.n_lines) and rows[1] == "matches %d" % k, rows[:2]
        got = np.array([[int(v) for v in r.split()] for r in rows[2:2 + k]], dtype=np.int64).reshape(k, 5)
        for j, w in enumerate(want.arrays()):
            assert np.array_equal(got[:, j], w[:k].astype(np.int64)), j
        assert rows[2 + k] == "default %d" % want.n
