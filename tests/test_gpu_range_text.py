"""range_text (redgpu_range_text[_dev]): sed's /open/,/close/ line ranges of a raw text.  The bytes,
the four counts and the records are exact against tests/range_rule.py - the rule of include/redgpu.h
as a dozen lines of Python over the CPU oracle's search per line (test_gpu_grep_text._want; the
reference's too when it is built): a border text with ranges across the 16 KiB chunk borders under
every emit_open x emit_close x invert setting and every kind of max_ranges, the toggle form over the
golden DFAs under every style and leader setting, every table placement, the shapes at the
machinery's edges, the records at every kind of rec_cap, truncation at every kind of out_cap with a
sentinel behind it, the device form at odd pointer offsets, identities with filter_text on the GPU,
other delimiters, a text of more chunks than the grid has waves, concurrent streams and threads,
and the C++ mirror."""
import collections
import ctypes as C
import itertools
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
from one_amd import _lib
from one_amd import workloads as W
from golden_util import load_dfa

import range_rule as R
import test_gpu_filter_text as FT
import test_gpu_grep_text as G

pytestmark = pytest.mark.gpu

CHUNK = 16384
SENT = 0x55
SENT64 = 0x5555555555555555
ALL = R.UNBOUNDED
SETTINGS = list(itertools.product((True, False), (True, False), (False, True)))  # open, close, invert

_texts = {}
_results = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _head_result(k):
    """the result search reports for a line that holds log100's head k - from the oracle"""
    if k not in _results:
        v, _ = R.values_of("log100", b"zz " + W.log100_heads()[k] + b"qq\n")
        assert len(v) == 1 and v[0] >= 1
        _results[k] = int(v[0])
    return _results[k]


OPEN_HEAD, CLOSE_HEAD, NOISE = 11, 42, (5, 77)
# what the lines that cross no chunk border hold, outside the long range: O an open head, C a
# close head, x and y the two noise heads, . nothing - closes outside any range, opens inside one,
# noise inside and outside, ranges of one line (OC) and of many
PLANT = "C.OxC.C.OO.yC..O.CxOC.y.OxOC.C"
INSIDE = "O.x.y.O."   # ... and inside the long range: no close


def _dev_text(text, shift=0):
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    if len(text):
        dev.copy_(torch.from_numpy(_u8(text).copy()))
    return dev


def _border_text(seed=1, n=4 * CHUNK + 5):
    """test_gpu_route_text._border_text's text - alphabet bytes, delimiters at pseudo-random gaps of
    1-199 bytes, a line that ends at n - 2, no delimiter from 16384 + 3000 to 2 * 16384 + 3500 (a
    line longer than a chunk) - with log100 heads planted: a close as the very first line, PLANT's
    pattern up to 1,500 bytes in front of the first border, there an open, INSIDE's pattern (no
    close) up to 800 bytes behind the third border, there the close - one range from chunk 0 to
    chunk 3, the long line inside it - PLANT again, and an open as the very last line"""
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
        if pos >= n - 2 - 70:
            break
        if pos >= 70 and not CHUNK + 3000 <= pos < 2 * CHUNK + 3500:
            ends.append(pos)
    ends.append(n - 2)
    a[ends] = 0x0A
    which = {"O": OPEN_HEAD, "C": CLOSE_HEAD, "x": NOISE[0], "y": NOISE[1], ".": None}
    lo, hi = CHUNK - 1500, 3 * CHUNK + 800
    begin, other, state = 0, 0, "front"
    for k, e in enumerate(ends):
        fits = e - begin >= 60
        if k == 0:
            head = CLOSE_HEAD
        elif k == len(ends) - 1:
            head = OPEN_HEAD
        elif state == "front" and begin >= lo and fits:
            head, state = OPEN_HEAD, "long"
        elif state == "long" and begin >= hi and fits:
            head, state = CLOSE_HEAD, "back"
        else:
            pattern = INSIDE if state == "long" else PLANT
            head = which[pattern[other % len(pattern)]]
            other += 1
        if head is not None and fits:
            p = _u8(heads[head])
            at = begin + (e - begin - len(p)) // 2
            a[at:at + len(p)] = p
        begin = e + 1
    _texts[key] = bytes(a)
    return _texts[key]


def _border_results():
    return _head_result(OPEN_HEAD), _head_result(CLOSE_HEAD)


def _check(got, x, rec_cap, where, dev=False):
    """a call's answer against the expectation: the counts, the bytes, the records"""
    k = min(x.n_ranges, rec_cap)
    if dev:
        import torch
        torch.cuda.synchronize()
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got), where
        assert all(t.dtype == torch.int64 for t in got[:4] + got[5:]), where
        counts = tuple(int(t.item()) for t in got[:4])
        assert counts == (x.n_lines, x.n_ranges, x.n_emitted, len(x.out)), (where, counts)
        assert got[4][:len(x.out)].cpu().numpy().tobytes() == x.out, where
        rec = [t[:k].cpu().numpy().astype(np.uint64) for t in got[5:]]
        assert all(t.numel() == rec_cap for t in got[5:]), where
    else:
        assert got[:3] == (x.n_lines, x.n_ranges, x.n_emitted), (where, got[:3], x.n_ranges)
        assert len(got[3]) == len(x.out), (where, len(got[3]), len(x.out))
        assert got[3] == x.out, where
        rec = list(got[4:])
        assert all(r.dtype == np.uint64 and len(r) == k for r in rec), where
    for r, w, what in zip(rec, x.records, ("first_line", "last_line", "begin", "end")):
        assert np.array_equal(r, w[:k]), (where, what, r[:8], w[:8])


def _same(exe, text, x, o, c, emit_open=True, emit_close=True, invert=False, max_ranges=ALL,
          style=1, lead=1, delim=b"\n", forms=("host", "dev"), where=None):
    kw = dict(emit_open=emit_open, emit_close=emit_close, invert=invert, max_ranges=max_ranges,
              delim=delim)
    rec_cap = x.n_ranges + 2
    if "host" in forms:
        got = one_amd.range_text(exe, text, o, c, style, bool(lead), rec_cap=rec_cap, **kw)
        assert one_amd.last_kernel() == "k_range_text"
        _check(got, x, rec_cap, ("host", where))
    if "dev" in forms:
        got = one_amd.range_text(exe, _dev_text(text, 1), o, c, style, bool(lead), rec_cap=rec_cap,
                                 out_cap=len(x.out) + 3, **kw)
        assert one_amd.last_kernel() == "k_range_text"
        _check(got, x, rec_cap, ("dev", where), dev=True)


def _owner(x):
    """the chunk every line ENDS in"""
    return (x.offs[1:] - 1) // CHUNK


def _spans(x):
    """the ranges whose first and last byte lie in different chunks"""
    return [r for r in range(x.n_ranges) if int(x.begin[r]) // CHUNK != (int(x.end[r]) - 1) // CHUNK]


# 1 ---------------------------------------------------------------------------------------------
def _border_cuts(x):
    """max_ranges values: 0, 1, one that cuts inside a chunk, one that cuts at a chunk border (the
    first range left out is the first that begins in its chunk), unbounded"""
    owner = _owner(x)
    start_chunk = owner[x.first_line.astype(np.int64)]
    at_border = int((start_chunk < 3).sum())
    assert 3 < at_border < x.n_ranges - 3 and (start_chunk == 3).sum() >= 4
    assert start_chunk[2] == start_chunk[3] == 0
    return [0, 1, 3, at_border, at_border + 2, ALL]


def _border_guards(text, o, c):
    """on the oracle's side, before any GPU call: the case cannot pass vacuously"""
    n = len(text)
    x = R.expect("log100", text, o, c)
    owner = _owner(x)
    kind = np.array(x.kind)
    assert x.n_ranges >= 20, x.n_ranges
    assert len(_spans(x)) >= 2
    # the range from chunk 0 to chunk 3, the line longer than a chunk inside it
    long_ = [r for r in range(x.n_ranges)
             if int(x.begin[r]) < CHUNK and int(x.end[r]) > 3 * CHUNK]
    assert len(long_) == 1
    big = int(np.argmax(np.diff(x.offs)))
    assert np.diff(x.offs).max() > CHUNK and x.range_of[big] == long_[0] and kind[big] == R.BODY
    v = x.values
    assert ((v == o) & (kind == R.BODY)).sum() >= 3          # opens inside a range
    assert ((v == c) & (kind == R.OUTSIDE)).sum() >= 3       # closes outside any
    noise = np.isin(v, [_head_result(k) for k in NOISE])
    assert len(set(v[noise].tolist())) == 2
    assert (noise & (kind == R.BODY)).sum() >= 3 and (noise & (kind == R.OUTSIDE)).sum() >= 3
    assert v[0] == c and kind[0] == R.OUTSIDE                # a close as the very first line
    assert v[-1] == o and kind[-1] == R.OPEN                 # an open as the very last line
    assert text[-1] != 0x0A and x.offs[-1] == n - 1
    # an emitted and a non-emitted line on each side of every border.  The long range covers chunks
    # 1 and 2 whole, so there the two kinds come from two of the settings that are run: all ranges,
    # and max_ranges below the long range's number
    cuts = _border_cuts(x)
    assert any(k <= long_[0] for k in cuts[1:])
    few = R.expect("log100", text, o, c, max_ranges=1)
    for ch in range(4):
        here = owner == ch
        assert (x.emit[here]).any() and (~x.emit[here] | ~few.emit[here]).any(), ch
    for ch in (0, 3):
        assert (x.emit[owner == ch]).any() and (~x.emit[owner == ch]).any()
    return x


def test_range_text_chunk_borders():
    name = "log100"
    text = _border_text()
    assert len(text) == 4 * CHUNK + 5
    o, c = _border_results()
    assert o != c and not {o, c} & {_head_result(k) for k in NOISE}
    base = _border_guards(text, o, c)
    cases = []
    for eo, ec, inv in SETTINGS:
        cases.append(((eo, ec, inv, ALL), R.expect(name, text, o, c, eo, ec, inv)))
    for k, mx in enumerate(_border_cuts(base)):
        eo, ec, inv = SETTINGS[k % len(SETTINGS)]
        for inv in (False, True):
            cases.append(((eo, ec, inv, mx), R.expect(name, text, o, c, eo, ec, inv, mx)))
    assert len({x.out for _, x in cases}) >= 12
    exe = one_amd.Executable(load_dfa(name))
    for (eo, ec, inv, mx), x in cases:
        _same(exe, text, x, o, c, eo, ec, inv, mx, where=("borders", eo, ec, inv, mx))


# 2 ---------------------------------------------------------------------------------------------
def _toggle_case(name, style, lead):
    """filter_text's text, cut behind a line so that the events are odd in number, and the result
    that toggles - the oracle's most frequent one"""
    text = FT._text(name, style)
    v, offs = R.values_of(name, text, style, lead)
    r = collections.Counter(v[v > 0].tolist()).most_common(1)[0][0]
    events = np.flatnonzero(v == r)
    if len(events) % 2 == 0:
        text = text[:int(offs[events[-1]])]
        v, offs = R.values_of(name, text, style, lead)
        events = np.flatnonzero(v == r)
    assert len(events) % 2 == 1
    return text, int(r)


@pytest.mark.parametrize("name", G.SEVEN)
def test_range_text_toggle_form(name):
    cases = []
    for style in G.STYLES:
        for lead in (0, 1):
            text, r = _toggle_case(name, style, lead)
            eo, ec, inv = SETTINGS[(style + lead) % len(SETTINGS)]
            x = R.expect(name, text, r, None, eo, ec, inv, style=style, lead=lead)
            assert x.n_ranges >= 50, (name, style, lead, x.n_ranges)
            assert x.kind[int(x.last_line[-1])] != R.CLOSE      # the last range is unclosed
            assert int(x.last_line[-1]) == x.n_lines - 1
            assert len(_spans(x)) >= 1
            cases.append((style, lead, text, r, (eo, ec, inv), x))
    exe = one_amd.Executable(load_dfa(name))
    for style, lead, text, r, (eo, ec, inv), x in cases:
        _same(exe, text, x, r, None, eo, ec, inv, style=style, lead=lead,
              forms=("host", "dev") if style == 1 else ("host",), where=(name, style, lead))
        if style == 4 and lead:
            _same(exe, text, x, r, r, eo, ec, inv, style=style, lead=lead, forms=("host",),
                  where=(name, "close given"))


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", G._PLACEMENT_ROWS)
def test_range_text_under_placement(dfa, opts, info):
    """only the class pass depends on the table's placement: one setting, both inverts; the two
    most frequent results open and close (the toggle form where the DFA has one)"""
    text = G._placement_text(dfa)
    G._placement_guard(dfa, text, 1, 1)
    v, _ = R.values_of(dfa, text)
    top = [r for r, _ in collections.Counter(v[v > 0].tolist()).most_common(2)]
    o, c = top[0], top[-1]
    cases = [(inv, R.expect(dfa, text, o, c, True, False, inv)) for inv in (False, True)]
    assert cases[0][1].n_ranges >= 10
    exe = one_amd.Executable(G._blob(dfa), **opts)
    got_info = exe.info
    for k, want in info.items():
        assert got_info[k] == want, (dfa, opts, k, got_info[k], want)
    for inv, x in cases:
        _same(exe, text, x, o, c, True, False, inv, where=(dfa, opts, inv))


# 4 ---------------------------------------------------------------------------------------------
LONG = b"q" * (4 * CHUNK)   # with the bytes in front of it: three whole chunks without a delimiter


def _shapes():
    """shape -> (DFA, text, open head or None = the one result, close head, [settings], what the
    oracle must say); a setting is (emit_open, emit_close, max_ranges)"""
    heads = W.log100_heads()
    op, cl = b"x " + heads[OPEN_HEAD] + b"y\n", b"x " + heads[CLOSE_HEAD] + b"y\n"
    filler = b"".join(b"line %d of the filler\n" % k for k in range(1900))
    assert len(filler) > 40960
    every = [(True, True, ALL)]
    ones = b"1\n" * (3 * 8192)
    return {
        "one line that opens": ("log100", op, OPEN_HEAD, CLOSE_HEAD, every,
                                lambda x: (x.n_lines, x.n_ranges, x.n_emitted) == (1, 1, 1)),
        "nothing opens": ("log100", filler, OPEN_HEAD, CLOSE_HEAD, every,
                          lambda x: (x.n_lines, x.n_ranges, x.n_emitted) == (1900, 0, 0)),
        "only closes": ("log100", (cl + b"no\n") * 300 + filler, OPEN_HEAD, CLOSE_HEAD, every,
                        lambda x: x.n_ranges == 0 and (x.values > 0).sum() == 300),
        "an open that is never closed, 40 KiB before the end": (
            "log100", b"a\n" + op + filler + b"and a tail", OPEN_HEAD, CLOSE_HEAD,
            every + [(False, True, ALL)],
            lambda x: x.n_ranges == 1 and x.last_line[0] == x.n_lines - 1 == 1901 and
            x.n_emitted >= 1900 and int(x.end[0]) - int(x.begin[0]) > 40960),
        # 8,192 lines in every chunk, every one an event: ranges of two lines, 4,096 starts in a
        # chunk, and with the close lines left out 4,096 runs of one line - 64 rounds of 64 runs
        "one-byte lines, every line an event": (
            "num3", ones, None, None, every + [(True, False, ALL), (False, True, 5000)],
            lambda x: x.n_lines == 3 * 8192 and x.n_ranges in (3 * 4096, 5000) and
            (x.first_line[:4].tolist(), x.last_line[:4].tolist()) == ([0, 2, 4, 6], [1, 3, 5, 7])),
        "an open, three whole chunks without a delimiter, a close": (
            "log100", b"a\n" + op + LONG + b"\n" + cl + b"b\n", OPEN_HEAD, CLOSE_HEAD,
            every + [(False, False, ALL)],
            lambda x: x.n_ranges == 1 and x.kind == [R.OUTSIDE, R.OPEN, R.BODY, R.CLOSE, R.OUTSIDE]),
        "a tail that would open": (
            "log100", b"no\n" + cl + b"no\nx " + heads[OPEN_HEAD] + b"y and no end", OPEN_HEAD,
            CLOSE_HEAD, every, lambda x: (x.n_lines, x.n_ranges) == (3, 0)),
        "max_ranges lands on a range that is left open": (
            "log100", op + b"in\n" + cl + b"out\n" + op + filler, OPEN_HEAD, CLOSE_HEAD,
            [(True, True, 2), (True, True, 1), (False, False, 2), (True, True, 3)],
            lambda x: x.n_ranges in (1, 2) and
            (x.n_ranges == 1 or x.last_line[1] == x.n_lines - 1 == 1904)),
    }


@pytest.mark.parametrize("shape", list(_shapes()))
def test_range_text_shapes(shape):
    name, text, oh, ch, settings, check = _shapes()[shape]
    if oh is None:
        v, _ = R.values_of(name, text)
        assert (v == v[0]).all() and v[0] >= 1        # every line is an event
        o = c = int(v[0])
    else:
        o, c = _head_result(oh), _head_result(ch)
    cases = []
    for eo, ec, mx in settings:
        x = R.expect(name, text, o, c, eo, ec, False, mx)
        assert check(x), (shape, eo, ec, mx, x.n_lines, x.n_ranges, x.n_emitted)
        cases.append((eo, ec, False, mx, x))
        cases.append((eo, ec, True, mx, R.expect(name, text, o, c, eo, ec, True, mx)))
    if "three whole chunks" in shape:
        offs = cases[0][4].offs
        big = int(np.argmax(np.diff(offs)))
        first = (offs[big] + CHUNK - 1) // CHUNK
        assert (offs[big + 1] - 1) // CHUNK - first >= 3      # whole chunks without a delimiter
    exe = one_amd.Executable(load_dfa(name))
    for eo, ec, inv, mx, x in cases:
        _same(exe, text, x, o, c, eo, ec, inv, mx, where=(shape, eo, ec, inv, mx))


# 5, 6 ------------------------------------------------------------------------------------------
def _raw_host(exe, text, o, c, out_cap, room, rec_cap=0, rec_room=0, flags=(1, 1, 0), mx=ALL,
              have=(True, True, True), recs=(True,) * 4, out=True):
    """redgpu_range_text through ctypes: sentinel-filled outputs; have = n_lines, n_ranges,
    n_emitted.  Returns the four counts, the four record arrays (rec_room entries), the buffer."""
    lib = _lib.lib()
    buf = np.full(room, SENT, dtype=np.uint8)
    cnt = [C.c_uint64(SENT64) for _ in range(4)]
    rec = np.full((4, max(rec_room, 1)), SENT64, dtype=np.uint64)
    rc = lib.redgpu_range_text(
        exe._h, 1, 1, o, c, *flags, mx, text, len(text), 0x0A,
        *[C.byref(cnt[k]) if have[k] else None for k in range(3)], C.byref(cnt[3]),
        buf.ctypes.data if out else None, out_cap, rec_cap,
        *[rec[k].ctypes.data if recs[k] else None for k in range(4)])
    assert rc == 0, lib.redgpu_last_error()
    return [v.value for v in cnt], rec, buf


def _raw_dev(exe, dev, o, c, out_cap, room, rec_cap=0, rec_room=0, flags=(1, 1, 0), mx=ALL,
             have=(True, True, True), recs=(True,) * 4, out_shift=0):
    """redgpu_range_text_dev: sentinel-filled tensors, `room` bytes of the output from out_shift on
    handed over; everything on the device.  Returns as _raw_host, the WHOLE output tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    cnt = torch.full((4,), SENT64, dtype=torch.int64, device="cuda")
    rec = torch.full((4, max(rec_room, 1)), SENT64, dtype=torch.int64, device="cuda")
    rc = lib.redgpu_range_text_dev(
        exe._h, 1, 1, o, c, *flags, mx, dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A,
        *[cnt.data_ptr() + 8 * k if have[k] else None for k in range(3)], cnt.data_ptr() + 24,
        buf.data_ptr() + out_shift, out_cap, rec_cap,
        *[rec[k].data_ptr() if recs[k] else None for k in range(4)],
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return (cnt.cpu().numpy().astype(np.uint64).tolist(), rec.cpu().numpy().astype(np.uint64),
            buf.cpu().numpy())


def _counts_same(got, x, where, have=(True, True, True)):
    want = [v if h else SENT64 for v, h in zip((x.n_lines, x.n_ranges, x.n_emitted), have)]
    assert got[0] == want + [len(x.out)], (where, got[0], want)


def _records_same(rec, x, rec_cap, where, recs=(True,) * 4):
    k = min(x.n_ranges, rec_cap)
    for row, w, have in zip(rec, x.records, recs):
        if have:
            assert np.array_equal(row[:k], w[:k]), where
            assert (row[k:] == SENT64).all(), where      # nothing at or behind min(n_ranges, rec_cap)
        else:
            assert (row == SENT64).all(), where


def _prefix_and_sentinels(buf, want, out_cap, where, shift=0):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


def test_range_text_records():
    import torch
    name = "log100"
    text = _border_text()
    o, c = _border_results()
    dev = _dev_text(text)
    exe = one_amd.Executable(load_dfa(name))
    for mx in (ALL, 7):
        # (the records do not depend on the flags)
        x = R.expect(name, text, o, c, False, True, True, mx)
        n = x.n_ranges
        assert n >= 7 and x.kind[int(x.last_line[-1])] == (R.OPEN if mx == ALL else R.CLOSE)
        room = n + 8
        for rec_cap in (0, 1, n - 1, n, n + 5):
            got = _raw_host(exe, text, o, c, 0, 8, rec_cap, room, (0, 1, 1), mx)
            _counts_same(got, x, ("host", mx, rec_cap))
            _records_same(got[1], x, rec_cap, ("host", mx, rec_cap))
            got = _raw_dev(exe, dev, o, c, 0, 8, rec_cap, room, (0, 1, 1), mx)
            _counts_same(got, x, ("dev", mx, rec_cap))
            _records_same(got[1], x, rec_cap, ("dev", mx, rec_cap))
            assert (got[2] == SENT).all()
        for missing in range(4):
            recs = tuple(k != missing for k in range(4))
            got = _raw_host(exe, text, o, c, 0, 8, n, room, mx=mx, recs=recs)
            _records_same(got[1], x, n, ("host", mx, recs), recs)
            got = _raw_dev(exe, dev, o, c, 0, 8, n, room, mx=mx, recs=recs)
            _records_same(got[1], x, n, ("dev", mx, recs), recs)
    # data[begin[r]:end[r]] fed back: exactly one range, of all its lines
    x = R.expect(name, text, o, c)
    got = one_amd.range_text(exe, dev, o, c, out_cap=0, rec_cap=x.n_ranges)
    torch.cuda.synchronize()
    begin, end = got[7].tolist(), got[8].tolist()
    for r in range(x.n_ranges):
        part = dev[begin[r]:end[r]]
        back = one_amd.range_text(exe, part, o, c, out_cap=part.numel(), rec_cap=2)
        torch.cuda.synchronize()
        lines = int(x.last_line[r] - x.first_line[r]) + 1
        assert [int(t.item()) for t in back[:4]] == [lines, 1, lines, part.numel()], r
        assert torch.equal(back[4], part)
        assert [int(t[0].item()) for t in back[5:]] == [0, lines - 1, 0, part.numel()], r


@pytest.mark.parametrize("toggle", [False, True])
def test_range_text_truncation(toggle):
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    o, c = _border_results()
    if toggle:
        c = o
    x = R.expect(name, text, o, c, True, False)
    n = len(x.out)
    # the end of a run of emitted lines (the line behind it is not emitted), and the middle of a line
    lines = np.flatnonzero(x.emit)
    gap = int(np.flatnonzero(np.diff(lines) > 1)[3])
    edge = int(np.diff(x.offs)[lines[:gap + 1]].sum())
    assert x.out[edge - 1] == 0x0A and 100 < edge < n - 100
    inside = edge + 2
    while x.out[inside] == 0x0A or x.out[inside - 1] == 0x0A:
        inside += 1
    caps = [0, 1, 15, 16, 17, inside, edge - 1, edge, edge + 1, n - 1, n, n + 7]
    assert len(set(caps)) == len(caps) and max(caps[:-1]) <= n
    shifts = (0, 1, 7, 15)
    devs = [_dev_text(text, shift) for shift in shifts]
    for k, cap in enumerate(caps):
        got = _raw_host(exe, text, o, c, cap, n + 64, flags=(1, 0, 0))
        _counts_same(got, x, ("host", cap))
        _prefix_and_sentinels(got[2], x.out, cap, ("host", cap))
        # the device form: the text and - independently - the output off a 16-byte boundary
        out_shift = (0, 15, 7, 1, 15)[k % 5]
        got = _raw_dev(exe, devs[k % 4], o, c, cap, n + 64, flags=(1, 0, 0), out_shift=out_shift)
        _counts_same(got, x, ("dev", cap, shifts[k % 4]))
        _prefix_and_sentinels(got[2], x.out, cap, ("dev", cap, shifts[k % 4]), shift=out_shift)


def test_range_text_some_outputs_null():
    """n_lines, n_ranges and n_emitted may be NULL each on its own, and out"""
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    o, c = _border_results()
    x = R.expect(name, text, o, c)
    n = len(x.out)
    dev = _dev_text(text)
    for have in itertools.product((True, False), repeat=3):
        for out in (True, False):
            got = _raw_host(exe, text, o, c, n, n, have=have, out=out)
            _counts_same(got, x, ("host", have, out), have)
            assert got[2].tobytes() == (x.out if out else bytes([SENT]) * n)
        got = _raw_dev(exe, dev, o, c, n, n, have=have)
        _counts_same(got, x, ("dev", have), have)
        _prefix_and_sentinels(got[2], x.out, n, have)


def test_range_text_device_verb():
    """the wrapper's device form: out=, out_cap=, the sizes only, and what it refuses"""
    import torch
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    o, c = _border_results()
    x = R.expect(name, text, o, c)
    dev = _dev_text(text, 7)
    mine = torch.full((len(x.out) + 5,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.range_text(exe, dev, o, c, out=mine)
    assert got[4] is mine and got[3].item() == len(x.out) and got[5].numel() == 0
    assert mine.cpu().numpy().tobytes() == x.out + bytes([SENT]) * 5
    got = one_amd.range_text(exe, dev, o, c, out_cap=0)                    # the sizes only
    assert [t.item() for t in got[:4]] == [x.n_lines, x.n_ranges, x.n_emitted, len(x.out)]
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, dev, o, c)                                 # needs out or out_cap
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, dev, 0, out_cap=0)


# 7 ---------------------------------------------------------------------------------------------
def test_range_text_identities():
    """beside the oracle: with both flags the plain and the inverted output split the lines between
    them; filter_text with the same DFA selects the open lines among others; where open and close
    lines are adjacent everywhere, the ranges without their close lines are filter_text's output"""
    import torch
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text()
    o, c = _border_results()
    dev = _dev_text(text)
    for close in (c, o):
        plain = one_amd.range_text(exe, dev, o, close, out_cap=0)
        other = one_amd.range_text(exe, dev, o, close, invert=True, out_cap=0)
        sel = one_amd.filter_text(exe, dev, 1, True, out_cap=0)
        torch.cuda.synchronize()
        assert plain[3].item() + other[3].item() == text.rindex(b"\n") + 1
        assert plain[2].item() + other[2].item() == plain[0].item() == sel[0].item()
        assert sel[1].item() >= plain[1].item() >= 20
    # err has one result: in the toggle form every range here is two adjacent "error" lines, and
    # with the close lines left out the first of each pair alone
    pairs = b"".join(b"%d error a\n%d error b\nplain %d\n" % (k, k, k) for k in range(3000))
    assert len(pairs) > 4 * CHUNK
    err = one_amd.Executable(load_dfa("err"))
    dpairs = _dev_text(pairs)
    got = one_amd.range_text(err, dpairs, 1, emit_close=False, out_cap=len(pairs))
    inv = one_amd.range_text(err, dpairs, 1, emit_close=False, invert=True, out_cap=len(pairs))
    torch.cuda.synchronize()
    want = b"".join(b"%d error a\n" % k for k in range(3000))
    assert [t.item() for t in got[:4]] == [9000, 3000, 3000, len(want)]
    assert got[4][:len(want)].cpu().numpy().tobytes() == want
    assert inv[2].item() == 6000 and inv[3].item() == len(pairs) - len(want)
    # open lines every other line, nothing else matches
    heads = W.log100_heads()
    two = b"".join(b"x " + heads[OPEN_HEAD] + b"%d\n" % k + b"nothing %d\n" % k for k in range(900))
    dtwo = _dev_text(two)
    exe2 = one_amd.Executable(load_dfa(name))
    a = one_amd.range_text(exe2, dtwo, o, out_cap=len(two), emit_close=False)
    b = one_amd.filter_text(exe2, dtwo, 1, True, out_cap=len(two))
    torch.cuda.synchronize()
    # (toggle form: open lines alternate as open and close, so half of them are emitted)
    assert a[1].item() == 450 and b[1].item() == 900
    # ... and with a close result no line has, every open line begins nothing new: one range
    one = one_amd.range_text(exe2, dtwo, o, c, out_cap=len(two))
    torch.cuda.synchronize()
    assert [t.item() for t in one[:4]] == [1800, 1, 1800, len(two)]
    # single-line ranges: an open line, a close line, in turn; without the close lines the output
    # is filter_text's selection of the open lines' text alone
    adj = b"".join(b"x " + heads[OPEN_HEAD] + b"%d\n" % k + b"x " + heads[CLOSE_HEAD] + b"%d\n" % k
                   for k in range(1200))
    opens = b"".join(b"x " + heads[OPEN_HEAD] + b"%d\n" % k for k in range(1200))
    assert len(adj) > 4 * CHUNK
    dadj = _dev_text(adj)
    got = one_amd.range_text(exe2, dadj, o, c, emit_close=False, out_cap=len(adj))
    sel = one_amd.filter_text(exe2, _dev_text(opens), 1, True, out_cap=len(opens))
    torch.cuda.synchronize()
    assert [t.item() for t in got[:4]] == [2400, 1200, 1200, len(opens)]
    assert sel[3].item() == len(opens)
    assert torch.equal(got[4][:len(opens)], sel[4][:len(opens)])


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_range_text_other_delimiter(delim):
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _border_text().replace(b"\n", delim)
    o, c = _border_results()
    for eo, ec, inv in SETTINGS[1::3]:
        x = R.expect(name, text, o, c, eo, ec, inv, delim=delim[0])
        assert x.n_lines >= 400 and x.n_ranges >= 20
        _same(exe, text, x, o, c, eo, ec, inv, delim=delim, where=(delim, eo, ec, inv))
    # ... and with '\n' the same text has no line at all
    got = one_amd.range_text(exe, text, o, c, rec_cap=4)
    assert got[:4] == (0, 0, 0, b"") and all(len(r) == 0 for r in got[4:])


def test_range_text_empty_and_lineless():
    exe = one_amd.Executable(load_dfa("log100"))
    o, c = _border_results()
    piece = b"x " + W.log100_heads()[OPEN_HEAD]
    for text in (b"", piece + b" and no line end", (piece + b" ") * 3000):
        dev = _dev_text(text)
        for close in (c, o):
            for flags in ((1, 1, 0), (1, 1, 1)):
                got = one_amd.range_text(exe, text, o, close, invert=bool(flags[2]), rec_cap=3)
                assert got[:4] == (0, 0, 0, b"") and all(len(r) == 0 for r in got[4:])
                for raw in (_raw_host(exe, text, o, close, 64, 64, 3, 3, flags),
                            _raw_dev(exe, dev, o, close, 64, 64, 3, 3, flags)):
                    assert raw[0] == [0, 0, 0, 0]
                    assert (raw[1] == SENT64).all() and (raw[2] == SENT).all()


# 9 ---------------------------------------------------------------------------------------------
def test_range_text_above_the_grid():
    """160 MiB = 10,240 chunks: more than the waves any pass has (k_rg_class CUs x 2 workgroups of
    16 waves, the other k_rg_* passes CUs x 8 of 4), so every wave takes a second chunk, and the
    single-workgroup scans run ten tiles.  Everything stays on the device: a 1 MiB block that ends
    in a delimiter and OUTSIDE a range, tiled - the answer is the block's, tiled.  Then a text
    whose only event is an open in its first line: every chunk is inside by carry alone."""
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 8 * 4
    body = G._standard(b"error", seed=5, n=block_len - 4096)
    block = b"not this one\n" + body[:body.rindex(b"\n") + 1] + b"nor that\n"
    v, offs = R.values_of(name, block, 4, 1)
    if (v == 1).sum() % 2:                      # an even number of events: the block ends outside
        block += b"one more error\n"
    block = block + b" " * (block_len - len(block) - 1) + b"\n"
    x = R.expect(name, block, 1, None, True, False, style=4)
    assert len(block) == block_len and x.n_ranges > 1000 and x.kind[-1] == R.OUTSIDE
    assert x.n_emitted < x.n_lines - 100
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    n = len(x.out) * tiles
    got = one_amd.range_text(exe, dev, 1, None, 4, True, emit_close=False, out_cap=n + 16,
                             rec_cap=x.n_ranges * tiles)
    assert one_amd.last_kernel() == "k_range_text"
    torch.cuda.synchronize()
    assert [t.item() for t in got[:4]] == [x.n_lines * tiles, x.n_ranges * tiles,
                                          x.n_emitted * tiles, n]
    exp = torch.from_numpy(_u8(x.out).copy()).cuda().repeat(tiles)
    assert torch.equal(got[4][:n], exp)
    del exp
    for rec, per, step in zip(got[5:], x.records, (x.n_lines, x.n_lines, block_len, block_len)):
        want = (torch.from_numpy(per.astype(np.int64)).cuda().repeat(tiles) +
                torch.arange(tiles, device="cuda").repeat_interleave(x.n_ranges) * step)
        assert torch.equal(rec, want)
    # one open in the first line and nothing else
    quiet = (b"an error opens\n" + b"nothing to see here, move along\n" * 40000)[:block_len - 1] + b"\n"
    rest = (b"nothing to see here, move along\n" * 40000)[:block_len - 1] + b"\n"
    dev = torch.cat([torch.from_numpy(_u8(quiet).copy()).cuda(),
                     torch.from_numpy(_u8(rest).copy()).cuda().repeat(tiles - 1)])
    lines = quiet.count(b"\n") + rest.count(b"\n") * (tiles - 1)
    got = one_amd.range_text(exe, dev, 1, None, 4, True, out_cap=dev.numel(), rec_cap=2)
    torch.cuda.synchronize()
    assert [t.item() for t in got[:4]] == [lines, 1, lines, dev.numel()]
    assert torch.equal(got[4], dev)
    assert [t[0].item() for t in got[5:]] == [0, lines - 1, 0, dev.numel()]
    got = one_amd.range_text(exe, dev, 1, None, 4, True, invert=True, out_cap=64)
    torch.cuda.synchronize()
    assert [t.item() for t in got[:4]] == [lines, 1, 0, 0]


# 10 --------------------------------------------------------------------------------------------
def test_range_text_two_streams_and_threads():
    import torch
    name = "log100"
    o, c = _border_results()
    exes = [one_amd.Executable(load_dfa(name)) for _ in range(2)]
    texts = [_border_text(seed=2 + k) for k in range(2)]
    kws = [dict(emit_open=False), dict(invert=True, max_ranges=9)]
    closes = [c, o]
    wants = [R.expect(name, t, o, cl, **kw) for t, cl, kw in zip(texts, closes, kws)]
    assert len(wants[0].out) != len(wants[1].out) and min(w.n_ranges for w in wants) >= 9
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    outs = []
    for k, (st, exe, d, x) in enumerate(zip(streams, exes, devs, wants)):
        with torch.cuda.stream(st):
            outs.append(one_amd.range_text(exe, d, o, closes[k], out_cap=len(x.out) + 3,
                                           rec_cap=x.n_ranges + 2, **kws[k]))
    torch.cuda.synchronize()
    for got, x in zip(outs, wants):
        _check(got, x, x.n_ranges + 2, "two streams", dev=True)
    errors = []

    def work(k, exe, t, d, st, x):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.range_text(exe, d, o, closes[k], out_cap=len(x.out) + 3,
                                             rec_cap=x.n_ranges + 2, **kws[k])
                    st.synchronize()
                _check(got, x, x.n_ranges + 2, ("thread", k), dev=True)
                host = one_amd.range_text(exe, t, o, closes[k], rec_cap=x.n_ranges + 2, **kws[k])
                _check(host, x, x.n_ranges + 2, ("thread", k, "host"))
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(k,) + a)
          for k, a in enumerate(zip(exes, texts, devs, streams, wants))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# 11 --------------------------------------------------------------------------------------------
def test_range_text_cpp_mirror(tmp_path):
    """redgpu::rangeText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "range_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "range_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "log100"
    text = _border_text()
    o, c = _border_results()
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), str(o), str(c), prefix], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    show = R.expect(name, text, o, c)
    drop = R.expect(name, text, o, c, invert=True)
    body = R.expect(name, text, o, c, False, False, False, 3)
    want = ["print %d %d" % (show.n_ranges, show.n_emitted)]
    want += ["range %d %d %d %d" % tuple(int(col[r]) for col in show.records)
             for r in range(show.n_ranges)]
    want += ["delete %d %d" % (drop.n_ranges, drop.n_emitted),
             "body %d %d" % (body.n_ranges, body.n_emitted)]
    assert run.stdout.split("\n")[:len(want)] == want
    assert body.n_ranges == 3 and 0 < body.n_emitted < show.n_emitted
    assert open(prefix + ".print", "rb").read() == show.out
    assert open(prefix + ".delete", "rb").read() == drop.out
    assert open(prefix + ".body", "rb").read() == body.out
