"""route_text (redgpu_route_text[_dev]): every line of a raw text routed to the bucket of the
result search<style,doLeader> reports for it, the text put back together bucket by bucket.  The
bytes, bin_lines, bin_offsets, out_len, n_routed and n_lines are exact against sampleLines' loop
(oracle.split_lines_loop) plus the CPU oracle's search per line (test_gpu_grep_text._want; the
reference's too when it is built) and a few lines of numpy - the bucket per line, a stable argsort,
the join: all of log100's classes under every cut of n_bins, the chunk-border shapes, every style,
leader setting and table placement, truncation at every kind of out_cap with a sentinel behind it,
the device form at odd pointer offsets, identities with tally_text and filter_text on the GPU, a
text of more chunks than the grid has waves, concurrent streams and threads, optional outputs, and
the C++ mirror."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
from one_amd import _lib
from one_amd import workloads as W
from golden_util import load_dfa

import test_gpu_grep_text as G

pytestmark = pytest.mark.gpu

CHUNK = 16384
SENT = 0x55
SENT64 = 0x5555555555555555

_expects = {}
_texts = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _values(name, text, style=1, lead=1, delim=0x0A):
    """search<style,lead>(line).result_ per line, 0 where it does not match - from the oracle"""
    w = G._want(name, text, style, lead, False, delim)
    v = np.zeros(w[0], dtype=np.int64)
    v[w[2].astype(np.int64)] = w[5]
    return v


class _Expect:
    """the rule of include/redgpu.h on the oracle's per-line search: the bucket per line, a stable
    argsort, the join"""

    def __init__(self, name, text, n_bins, drop, style, lead, delim):
        v = _values(name, text, style, lead, delim)
        offs = G._lines_of(text, delim).astype(np.int64)
        self.values, self.offs, self.n_bins = v, offs, n_bins
        self.n_lines = len(v)
        # (uint32_t)r < n_bins: a negative result would land in "everything else"
        self.bucket = np.where((v >= 0) & (v < n_bins), v, n_bins)
        keep = v != 0 if drop else np.ones(len(v), dtype=bool)
        self.keep = keep
        order = np.argsort(self.bucket, kind="stable")
        self.order = order[keep[order]]
        lens = np.diff(offs)
        self.bin_lines = np.bincount(self.bucket, minlength=n_bins + 1).astype(np.uint64)
        sizes = np.zeros(n_bins + 1, dtype=np.int64)
        np.add.at(sizes, self.bucket[keep], lens[keep])
        self.bin_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.out = b"".join(text[offs[i]:offs[i + 1]] for i in self.order)
        self.n_routed = int(keep.sum())
        assert len(self.out) == int(self.bin_offsets[-1])

    def section(self, b):
        return self.out[int(self.bin_offsets[b]):int(self.bin_offsets[b + 1])]


def _expect(name, text, n_bins, drop=False, style=1, lead=1, delim=0x0A):
    key = (name, text, n_bins, bool(drop), style, lead, delim)
    if key not in _expects:
        _expects[key] = _Expect(name, text, n_bins, bool(drop), style, lead, delim)
    return _expects[key]


def _dev_text(text, shift=0):
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    if len(text):
        dev.copy_(torch.from_numpy(_u8(text).copy()))
    return dev


def _same(exe, text, x, drop, style=1, lead=1, delim=b"\n", forms=("host", "dev"), where=None,
          n_bins="given"):
    """both forms of the verb against the expectation"""
    import torch
    kw = dict(drop_unmatched=drop, delim=delim)
    nb = x.n_bins if n_bins == "given" else n_bins
    if "host" in forms:
        got = one_amd.route_text(exe, text, nb, style, bool(lead), **kw)
        assert one_amd.last_kernel() == "k_route_text"
        assert got[:2] == (x.n_lines, x.n_routed), (where, got[:2], x.n_lines, x.n_routed)
        assert got[2].dtype == np.uint64 and np.array_equal(got[2], x.bin_lines), (where, got[2])
        assert got[3].dtype == np.uint64 and np.array_equal(got[3], x.bin_offsets), (where, got[3])
        assert len(got[4]) == len(x.out), (where, len(got[4]), len(x.out))
        assert got[4] == x.out, where
    if "dev" in forms:
        got = one_amd.route_text(exe, _dev_text(text, 1), nb, style, bool(lead),
                                 out_cap=len(x.out) + 3, **kw)
        assert one_amd.last_kernel() == "k_route_text"
        torch.cuda.synchronize()
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
        assert all(t.dtype == torch.int64 for t in got[:5])
        assert got[0].shape == got[1].shape == got[4].shape == (1,)
        assert (got[0].item(), got[1].item(), got[4].item()) == (x.n_lines, x.n_routed, len(x.out)), where
        assert np.array_equal(got[2].cpu().numpy().astype(np.uint64), x.bin_lines), where
        assert np.array_equal(got[3].cpu().numpy().astype(np.uint64), x.bin_offsets), where
        assert got[5][:len(x.out)].cpu().numpy().tobytes() == x.out, where


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filler", [0, 200])
def test_route_text_all_signatures(filler):
    """every one of log100's 100 results and lines that do not match, under every cut of n_bins"""
    heads = W.log100_heads()
    rows = []
    for i in range(300):
        rows.append(b"z" * filler + b"zz " + heads[(37 * i) % 100] + b"qq\n")
        if i % 4 == 1:
            rows.append(b"y" * (filler // 2) + b"nothing to see %d\n" % i)
    text = b"".join(rows) + b"a tail " + heads[3]
    assert (len(text) > 4 * CHUNK) == bool(filler)
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    assert exe.info["max_result"] == 100
    v = _values(name, text)
    assert len(v) == 375 and np.bincount(v, minlength=101).tolist() == [75] + [3] * 100
    # consecutive lines differ in value: every run of the write pass is one line
    assert (np.diff(v) != 0).all()
    for n_bins in (101, 100, 51, 7, 1, 0):
        for drop in (False, True):
            x = _expect(name, text, n_bins, drop)
            assert int(x.bin_lines.sum()) == 375 and x.n_routed == (300 if drop else 375)
            assert int(x.bin_lines[n_bins]) == (375 if n_bins == 0 else 3 * (101 - n_bins))
            _same(exe, text, x, drop, where=(filler, n_bins, drop))
    # n_bins=None: min(max_result + 1, 255)
    got = one_amd.route_text(exe, text)
    x = _expect(name, text, 101)
    assert len(got[2]) == 102 and len(got[3]) == 103 and got[4] == x.out


# 2 ---------------------------------------------------------------------------------------------
# which head the lines that cross no chunk border hold (None: no piece, the line does not match)
PLANT = [0, None, None, 1, None, 2, 2, None, 3, 0, None, None, 1, 1, 1, None, 2, None, 3, 3, 0,
         None, 1, None]
CROSS = {1: 4, 2: 9, 3: None, 4: 4}     # ... and the line across the border k * 16384
RARE = 50                               # in a few lines of chunk 0 and of chunk 3 alone


def _border_text(seed=1, n=4 * CHUNK + 5):
    """test_gpu_filter_text._text's text - alphabet bytes, delimiters at pseudo-random gaps of 1-199
    bytes, a line that ends at n - 2 - with log100 pieces of different signatures planted by
    PLANT / CROSS / RARE, and no delimiter from 16384 + 3000 to 2 * 16384 + 3500: a line longer than
    a chunk, across the border 2 * 16384"""
    key = ("border", seed, n)
    if key in _texts:
        return _texts[key]
    heads = W.log100_heads()
    a = W.alphabet_bytes(n, seed).copy()
    a[a == 0x0A] = 0x20
    rng = np.random.default_rng(seed)
    ends, pos = [], -1
    while True:
        pos += int(rng.integers(1, 200))
        if pos >= n - 2:
            break
        if not CHUNK + 3000 <= pos < 2 * CHUNK + 3500:
            ends.append(pos)
    ends.append(n - 2)
    a[ends] = 0x0A
    begin, other, rare = 0, 0, {0: 0, 3: 0}
    for e in ends:
        crossed = [m for m in range(CHUNK, n, CHUNK) if begin < m <= e]
        if crossed:
            head = CROSS[crossed[0] // CHUNK]
        elif e // CHUNK in rare and rare[e // CHUNK] < 3 and e - begin >= 60 and other % 5 == 2:
            head = RARE
            rare[e // CHUNK] += 1
            other += 1
        else:
            head = PLANT[other % len(PLANT)]
            other += 1
        if head is not None and e - begin >= len(heads[head]):
            p = _u8(heads[head])
            at = begin + (e - begin - len(p)) // 2
            a[at:at + len(p)] = p
        begin = e + 1
    _texts[key] = bytes(a)
    return _texts[key]


def _border_guards(x, text):
    """on the oracle's side, before any GPU call: the case cannot pass vacuously"""
    n = len(text)
    owner = (x.offs[1:] - 1) // CHUNK          # the chunk a line ENDS in
    full = [b for b in range(x.n_bins + 1) if x.bin_lines[b] >= 20]
    assert len(full) >= 4, x.bin_lines
    crossing = [i for i in range(x.n_lines)
                if any(x.offs[i] < m <= x.offs[i + 1] - 1 for m in range(CHUNK, n, CHUNK))]
    assert len(set(x.bucket[crossing].tolist())) >= 2, x.bucket[crossing]
    apart = [b for b in range(x.n_bins + 1)
             if set(owner[x.bucket == b].tolist()) == {0, 3}]
    assert apart, "no bucket with lines in chunk 0 and chunk 3 alone"
    assert any(len(set(x.bucket[owner == c].tolist())) >= 4 for c in range(4))
    assert np.diff(x.offs).max() > CHUNK


def test_route_text_chunk_borders():
    name = "log100"
    text = _border_text()
    assert len(text) == 4 * CHUNK + 5 and text[-1] != 0x0A
    cases = []
    for n_bins in (101, 7, 3):
        for drop in (False, True):
            x = _expect(name, text, n_bins, drop)
            if n_bins == 101:
                _border_guards(x, text)
            cases.append((drop, x))
    assert len(set(int(b) for b in cases[0][1].bucket)) >= 7
    exe = one_amd.Executable(load_dfa(name))
    for drop, x in cases:
        _same(exe, text, x, drop, where=("borders", x.n_bins, drop))


def test_route_text_chunk_of_delimiters():
    """a chunk whose every byte is a delimiter: 16,384 empty lines, all of bucket 0"""
    name = "log100"
    heads = W.log100_heads()
    front = b"".join(b"line %d " % k + heads[k % 5] + b"\n" for k in range(400))
    front = front[:front.rindex(b"\n", 0, CHUNK - 40) + 1]
    front += b"x" * (CHUNK - len(front) - 1) + b"\n"
    text = front + b"\n" * CHUNK + b"behind " + heads[2] + b"\n" + heads[4] + b"\nand a tail"
    assert len(front) == CHUNK and set(text[CHUNK:2 * CHUNK]) == {0x0A}
    exe = one_amd.Executable(load_dfa(name))
    for n_bins in (6, 0):
        for drop in (False, True):
            x = _expect(name, text, n_bins, drop)
            assert x.bin_lines[0] >= CHUNK and x.n_routed == (x.n_lines if not drop
                                                              else x.n_lines - int((x.values == 0).sum()))
            _same(exe, text, x, drop, where=("delimiters", n_bins, drop))


def _raw_host(exe, text, n_bins, out_cap, room, drop=0, style=1, have=(True, True, True), out=True):
    """redgpu_route_text through ctypes: sentinel-filled outputs; have = n_lines, n_routed,
    bin_lines.  Returns (n_lines, n_routed, out_len), bin_lines, bin_offsets, the buffer."""
    lib = _lib.lib()
    buf = np.full(room, SENT, dtype=np.uint8)
    c = [C.c_uint64(SENT64) for _ in range(3)]
    lines = np.full(n_bins + 2, SENT64, dtype=np.uint64)
    offs = np.full(n_bins + 3, SENT64, dtype=np.uint64)
    rc = lib.redgpu_route_text(exe._h, style, 1, drop, text, len(text), 0x0A, n_bins,
                               C.byref(c[0]) if have[0] else None,
                               C.byref(c[1]) if have[1] else None,
                               lines.ctypes.data if have[2] else None, offs.ctypes.data,
                               C.byref(c[2]), buf.ctypes.data if out else None, out_cap)
    assert rc == 0, lib.redgpu_last_error()
    return [v.value for v in c], lines, offs, buf


def _raw_dev(exe, dev, n_bins, out_cap, room, drop=0, style=1, out_shift=0, have=(True, True, True)):
    """redgpu_route_text_dev: sentinel-filled tensors, `room` bytes of the output from out_shift on
    handed over; everything on the device.  Returns as _raw_host, the WHOLE output tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    cnt = torch.full((3 + n_bins + 2 + n_bins + 3,), SENT64, dtype=torch.int64, device="cuda")
    at = lambda k: cnt.data_ptr() + 8 * k   # noqa: E731
    rc = lib.redgpu_route_text_dev(exe._h, style, 1, drop,
                                   dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A,
                                   n_bins, at(0) if have[0] else None, at(1) if have[1] else None,
                                   at(3) if have[2] else None, at(3 + n_bins + 2), at(2),
                                   buf.data_ptr() + out_shift, out_cap,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    host = cnt.cpu().numpy().astype(np.uint64)
    return (host[:3].tolist(), host[3:3 + n_bins + 2], host[3 + n_bins + 2:], buf.cpu().numpy())


def _counts_same(got, x, where, have=(True, True, True)):
    c, lines, offs = got[:3]
    want = [x.n_lines if have[0] else SENT64, x.n_routed if have[1] else SENT64, len(x.out)]
    assert c == want, (where, c, want)
    if have[2]:
        assert np.array_equal(lines[:-1], x.bin_lines), where
    else:
        assert (lines[:-1] == SENT64).all(), where
    assert np.array_equal(offs[:-1], x.bin_offsets), where
    assert lines[-1] == SENT64 and offs[-1] == SENT64, where   # nothing behind the arrays


def _prefix_and_sentinels(buf, want, out_cap, where, shift=0):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


def test_route_text_empty_and_lineless():
    exe = one_amd.Executable(load_dfa("log100"))
    piece = W.log100_heads()[7]
    for text in (b"", piece + b" and no line end", (piece + b" ") * 3000):
        dev = _dev_text(text)
        for n_bins in (0, 3):
            for drop in (0, 1):
                got = one_amd.route_text(exe, text, n_bins, drop_unmatched=bool(drop))
                assert got[:2] == (0, 0) and got[4] == b""
                assert not got[2].any() and not got[3].any()
                assert len(got[2]) == n_bins + 1 and len(got[3]) == n_bins + 2
                for raw in (_raw_host(exe, text, n_bins, 64, 64, drop),
                            _raw_dev(exe, dev, n_bins, 64, 64, drop)):
                    assert raw[0] == [0, 0, 0]
                    assert not raw[1][:-1].any() and not raw[2][:-1].any()
                    assert raw[1][-1] == SENT64 and raw[2][-1] == SENT64
                    assert (raw[3] == SENT).all()


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", G._PLACEMENT_ROWS)
def test_route_text_under_placement(dfa, opts, info):
    """only the class pass depends on the table's placement: every style, both leader settings"""
    text = G._placement_text(dfa)
    n_bins = min(one_amd.Executable(G._blob(dfa), device="none").info["max_result"] + 1, 255)
    cases = []
    for style in G.STYLES:
        for lead in (0, 1):
            if style in (1, 4):
                G._placement_guard(dfa, text, style, lead)
            drop = (style + lead) % 2 == 1
            cases.append((style, lead, drop, _expect(dfa, text, n_bins, drop, style, lead)))
    exe = one_amd.Executable(G._blob(dfa), **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    for style, lead, drop, x in cases:
        _same(exe, text, x, drop, style, lead, forms=("host",) if style in (2, 3, 5) else ("host", "dev"),
              where=(dfa, opts, style, lead, drop), n_bins=None)


@pytest.mark.parametrize("name", G.SEVEN)
def test_route_text_seven_dfas(name):
    """the golden DFAs over test_gpu_grep_text's standard text, every style and leader setting"""
    text = G._standard(G.PIECES[name]())
    exe = one_amd.Executable(load_dfa(name))
    n_bins = exe.info["max_result"] + 1
    for style in G.STYLES:
        for lead in (0, 1):
            if style != 5:
                G._guard(name, text, style, lead)
            drop = (style + lead) % 2 == 0
            x = _expect(name, text, n_bins, drop, style, lead)
            _same(exe, text, x, drop, style, lead, forms=("host",), where=(name, style, lead))


@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_route_text_other_delimiter(delim):
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text().replace(b"\n", delim)
    for drop in (False, True):
        x = _expect(name, text, 101, drop, delim=delim[0])
        assert x.n_lines >= 400 and 100 <= x.n_routed <= x.n_lines
        _same(exe, text, x, drop, delim=delim, where=(delim, drop))
    # ... and with '\n' the same text has no line at all
    got = one_amd.route_text(exe, text, 101)
    assert got[:2] == (0, 0) and got[4] == b"" and not got[3].any()


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [0, 1])
def test_route_text_truncation(drop):
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    n_bins = 7
    x = _expect(name, text, n_bins, bool(drop))
    n = len(x.out)
    # a boundary between two sections that both have bytes, and the middle of a line of the second
    b = next(k for k in range(1, n_bins + 1)
             if x.bin_offsets[k - 1] < x.bin_offsets[k] < x.bin_offsets[k + 1])
    edge = int(x.bin_offsets[b])
    assert x.out[edge - 1] == 0x0A
    inside = edge + 2
    while x.out[inside] == 0x0A or x.out[inside - 1] == 0x0A:
        inside += 1
    caps = [0, 1, 15, 16, 17, inside, edge - 1, edge, edge + 1, n - 1, n, n + 7]
    assert len(set(caps)) == len(caps) and max(caps[:-1]) <= n
    devs = [_dev_text(text, shift) for shift in (0, 1, 7)]
    for k, cap in enumerate(caps):
        got = _raw_host(exe, text, n_bins, cap, n + 64, drop)
        _counts_same(got, x, ("host", drop, cap))
        _prefix_and_sentinels(got[3], x.out, cap, ("host", drop, cap))
        # the device form: the text and - independently - the output off a 16-byte boundary
        shift = (0, 1, 7)[k % 3]
        got = _raw_dev(exe, devs[k % 3], n_bins, cap, n + 64, drop, out_shift=(0, 15, 9, 3)[k % 4])
        _counts_same(got, x, ("dev", drop, cap, shift))
        _prefix_and_sentinels(got[3], x.out, cap, ("dev", drop, cap, shift), shift=(0, 15, 9, 3)[k % 4])


def test_route_text_some_outputs_null():
    """n_lines, n_routed and bin_lines may be NULL each on its own, and out"""
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    x = _expect(name, text, 5, True)
    n = len(x.out)
    dev = _dev_text(text)
    for nl in (True, False):
        for nr in (True, False):
            for bl in (True, False):
                have = (nl, nr, bl)
                for out in (True, False):
                    got = _raw_host(exe, text, 5, n, n, 1, have=have, out=out)
                    _counts_same(got, x, ("host", have, out), have)
                    assert got[3].tobytes() == (x.out if out else bytes([SENT]) * n)
                got = _raw_dev(exe, dev, 5, n, n, 1, have=have)
                _counts_same(got, x, ("dev", have), have)
                _prefix_and_sentinels(got[3], x.out, n, have)


def test_route_text_device_verb():
    """the wrapper's device form: out=, out_cap=, the sizes only, and what it refuses"""
    import torch
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    x = _expect(name, text, 101)
    dev = _dev_text(text, 7)
    mine = torch.full((len(x.out) + 5,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.route_text(exe, dev, 101, out=mine)
    assert got[5] is mine and got[4].item() == len(x.out)
    assert mine.cpu().numpy().tobytes() == x.out + bytes([SENT]) * 5
    got = one_amd.route_text(exe, dev, 101, out_cap=0)                     # the sizes only
    assert (got[0].item(), got[1].item(), got[4].item()) == (x.n_lines, x.n_routed, len(x.out))
    assert np.array_equal(got[3].cpu().numpy().astype(np.uint64), x.bin_offsets)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, dev, 101)                                  # needs out or out_cap
    with pytest.raises(one_amd.RedExceptLimit):
        one_amd.route_text(exe, dev, 256, out_cap=0)


# 5 ---------------------------------------------------------------------------------------------
def test_route_text_identities():
    """beside the oracle: bin_lines are tally_text's LINES bins; with one bin the two sections are
    filter_text's two inverts; a section fed back lands entirely in its own bucket"""
    import torch
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    dev = _dev_text(text)
    for n_bins in (101, 7, 0):
        got = one_amd.route_text(exe, dev, n_bins, out_cap=0)
        tally = one_amd.tally_text(exe, dev, n_bins, matches=False)
        torch.cuda.synchronize()
        assert torch.equal(got[2], tally[2]) and got[0].item() == tally[0].item()
    got = one_amd.route_text(exe, dev, 1, out_cap=len(text))
    no = one_amd.filter_text(exe, dev, 1, True, invert=True, out_cap=len(text))
    yes = one_amd.filter_text(exe, dev, 1, True, out_cap=len(text))
    torch.cuda.synchronize()
    o = got[3].tolist()
    assert o[0] == 0 and o[1] == no[3].item() and o[2] - o[1] == yes[3].item() and o[2] == got[4].item()
    assert o[1] > 1000 and o[2] - o[1] > 1000
    assert torch.equal(got[5][:o[1]], no[4][:o[1]])
    assert torch.equal(got[5][o[1]:o[2]], yes[4][:o[2] - o[1]])
    # every section of the full routing is a raw text of its own bucket alone
    got = one_amd.route_text(exe, dev, 101, out_cap=len(text))
    torch.cuda.synchronize()
    o, lines = got[3].tolist(), got[2].tolist()
    fed = 0
    for b in range(102):
        if o[b + 1] == o[b]:
            assert lines[b] == 0
            continue
        back = one_amd.route_text(exe, got[5][o[b]:o[b + 1]], 101, out_cap=len(text))
        torch.cuda.synchronize()
        want = [0] * 102
        want[b] = lines[b]
        assert back[2].tolist() == want and back[4].item() == o[b + 1] - o[b]
        assert torch.equal(back[5][:o[b + 1] - o[b]], got[5][o[b]:o[b + 1]])
        fed += 1
    assert fed >= 7


# 6 ---------------------------------------------------------------------------------------------
def test_route_text_above_the_grid():
    """160 MiB = 10,240 chunks: more than the waves any pass has (k_ro_class CUs x 2 workgroups of
    16 waves, the other k_ro_* passes CUs x 8 of 4), so every wave takes a second chunk.  Everything
    stays on the device: a 1 MiB block that ends in a delimiter, tiled; section b of the expected
    output is the block's section b, tiled."""
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 8 * 4
    head = b"not this one\nnor this\n"
    body = G._standard(b"error", seed=5, n=block_len - 4096)
    block = head + body[:body.rindex(b"\n") + 1] + b"nor that\n"
    block = block + b" " * (block_len - len(block) - 1) + b"\n"
    x = _expect(name, block, 1, False, 4, 1)
    assert len(block) == block_len and x.bin_lines[1] > 1000 and x.bin_lines[0] > 1000
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    n = len(x.out) * tiles
    got = one_amd.route_text(exe, dev, 1, 4, True, out_cap=n + 16)
    assert one_amd.last_kernel() == "k_route_text"
    torch.cuda.synchronize()
    assert (got[0].item(), got[1].item(), got[4].item()) == (x.n_lines * tiles, x.n_routed * tiles, n)
    assert got[2].tolist() == [int(v) * tiles for v in x.bin_lines]
    assert got[3].tolist() == [int(v) * tiles for v in x.bin_offsets]
    exp = torch.cat([torch.from_numpy(_u8(x.section(b)).copy()).cuda().repeat(tiles)
                     for b in range(2)])
    assert torch.equal(got[5][:n], exp)


def test_route_text_two_streams_and_threads():
    import torch
    name = "log100"
    exes = [one_amd.Executable(load_dfa(name)) for _ in range(2)]
    texts = [_border_text(seed=2 + k) for k in range(2)]
    bins = [101, 6]
    wants = [_expect(name, t, nb, k == 1) for k, (t, nb) in enumerate(zip(texts, bins))]
    assert len(wants[0].out) != len(wants[1].out)
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def same(got, x):
        n = int(got[4].item())
        assert (got[0].item(), got[1].item(), n) == (x.n_lines, x.n_routed, len(x.out))
        assert np.array_equal(got[2].cpu().numpy().astype(np.uint64), x.bin_lines)
        assert np.array_equal(got[3].cpu().numpy().astype(np.uint64), x.bin_offsets)
        assert got[5][:n].cpu().numpy().tobytes() == x.out

    outs = []
    for k, (st, exe, d, x) in enumerate(zip(streams, exes, devs, wants)):
        with torch.cuda.stream(st):
            outs.append(one_amd.route_text(exe, d, bins[k], drop_unmatched=k == 1,
                                           out_cap=len(x.out) + 3))
    torch.cuda.synchronize()
    for got, x in zip(outs, wants):
        same(got, x)
    errors = []

    def work(k, exe, t, d, st, x):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.route_text(exe, d, bins[k], drop_unmatched=k == 1,
                                             out_cap=len(x.out) + 3)
                    st.synchronize()
                same(got, x)
                host = one_amd.route_text(exe, t, bins[k], drop_unmatched=k == 1)
                assert host[:2] == (x.n_lines, x.n_routed) and host[4] == x.out
                assert np.array_equal(host[3], x.bin_offsets)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(k,) + a)
          for k, a in enumerate(zip(exes, texts, devs, streams, wants))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# 7 ---------------------------------------------------------------------------------------------
def test_route_text_cpp_mirror(tmp_path):
    """redgpu::routeText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "route_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "route_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "log100"
    text = _border_text()
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), "12", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    every = _expect(name, text, 12, False)
    matched = _expect(name, text, 12, True)
    row = lambda what, v: what + "".join(" %d" % int(k) for k in v)   # noqa: E731
    assert run.stdout.split("\n")[:6] == [
        "all 0 %d" % every.n_routed, row("lines", every.bin_lines), row("offsets", every.bin_offsets),
        "matched %d %d" % (matched.n_lines, matched.n_routed), row("lines", matched.bin_lines),
        row("offsets", matched.bin_offsets)]
    assert matched.n_routed < every.n_routed == every.n_lines
    assert open(prefix + ".all", "rb").read() == every.out
    assert open(prefix + ".matched", "rb").read() == matched.out
