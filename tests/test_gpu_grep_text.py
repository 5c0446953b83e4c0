"""grep_text (redgpu_grep_text[_dev]): the lines of a raw text that search<style,doLeader> selects,
as compact records in text order - all eight outputs exact against sampleLines' loop
(oracle.split_lines_loop) plus the CPU oracle's search per line (and the reference when present),
for every style, leader setting, invert, table placement, the chunk-border shapes, truncation,
limits, the device form at odd pointer offsets, concurrent streams and threads, and the C++
mirror.  test_grep_text_under_placement runs every (kind, verb) instantiation of k_gp_select and
k_gp_write: the rows of test_gpu_long_placements (kinds 2 to 7) and three of test_gpu_list_verbs."""
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

import test_gpu_list_verbs as LV
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

CHUNK = 16384
STYLES = [1, 2, 3, 4, 5]
PIECES = {
    "err": lambda: b"error", "dotstar_err": lambda: b"error", "newyork": lambda: b"New York",
    "uri": lambda: W.URI_PLANT.rstrip(), "log100": lambda: W.log100_heads()[7],
    "aab": lambda: b"aab", "ale": lambda: b"alee",
}
SEVEN = list(PIECES)

_oracles = {}
_texts = {}
_wants = {}


def _blob(name):
    """the DFA of a placement row from the row's factory (test_gpu_collect_text keeps the one copy;
    it imports this module, so it is imported here on first use), a golden DFA otherwise"""
    import test_gpu_collect_text as CT
    return CT._blob(name)


def _orc(name):
    if name not in _oracles:
        blob = _blob(name)
        _oracles[name] = (O.CpuOracle(blob), O.Reference(blob) if O.have_ref() else None)
    return _oracles[name]


def _lines_of(text, delim=0x0A):
    """offsets[] of sampleLines' lines (line k = [offs[k], offs[k + 1] - 1)), from its own loop"""
    lines = O.split_lines_loop(text, delim)
    return np.cumsum([0] + [len(x) + 1 for x in lines]).astype(np.uint64)


def _standard(piece: bytes, seed=1, n=4 * CHUNK + 5, end_in_delim=False):
    """Four split chunks and a tail of alphabet text, delimiters at pseudo-random gaps of 1-199
    bytes; the piece in every line that crosses an odd multiple of 16384 and in every third other
    line - but never in a line that crosses an even multiple.  end_in_delim: the last byte is a
    delimiter too, so the text is whole lines."""
    key = (piece, seed, n, end_in_delim)
    if key in _texts:
        return _texts[key]
    a = W.alphabet_bytes(n, seed).copy()
    a[a == 0x0A] = 0x20
    rng = np.random.default_rng(seed)
    ends, pos = [], -1
    while True:
        pos += int(rng.integers(1, 200))
        if pos >= n:
            break
        a[pos] = 0x0A
        ends.append(pos)
    if end_in_delim and ends[-1] != n - 1:
        a[n - 1] = 0x0A
        ends.append(n - 1)
    begin, other = 0, 0
    p = np.frombuffer(piece, dtype=np.uint8)
    for e in ends:
        crossed = [m for m in range(CHUNK, n, CHUNK) if begin < m <= e]
        if crossed:
            plant = any((m // CHUNK) % 2 == 1 for m in crossed)
        else:
            plant = other % 3 == 0
            other += 1
        if plant and e - begin >= len(p):
            at = begin + (e - begin - len(p)) // 2
            a[at:at + len(p)] = p
        begin = e + 1
    _texts[key] = bytes(a)
    return _texts[key]


def _want(name, text, style, lead, invert=False, delim=0x0A, max_count=1 << 62):
    """(n_lines, n_selected, line, begin, finish, result, start, end) from the oracle"""
    key = (name, text, style, lead, delim)
    if key not in _wants:
        cpu, ref = _orc(name)
        offs = _lines_of(text, delim)
        # search on every line alone: the lines back to back WITHOUT their delimiters, as a batch
        lines = O.split_lines_loop(text, delim)
        arr = np.frombuffer(b"".join(lines) + b"\0", dtype=np.uint8)
        bare = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
        r, s, e = cpu.batch("search", style, lead, arr, offsets=bare)
        for k in range(0, len(lines), 97):  # ... which is what the one-text call gives
            assert cpu.search(lines[k], style, bool(lead)) == (r[k], s[k], e[k])
        if ref is not None:
            rr, rs, re_ = ref.batch("search", style, lead, arr, offsets=bare)
            assert np.array_equal(r, rr) and np.array_equal(s, rs) and np.array_equal(e, re_)
        _wants[key] = (offs, r, s, e)
    offs, r, s, e = _wants[key]
    sel = np.flatnonzero((r > 0) != bool(invert))
    total = min(len(sel), max_count)
    sel = sel[:total]
    if invert:  # an unselected line's Outcome is (0, 0, 0) already
        assert not r[sel].any() and not s[sel].any() and not e[sel].any()
    return (len(offs) - 1, total, sel.astype(np.uint64), offs[sel], offs[sel + 1] - np.uint64(1),
            r[sel], s[sel], e[sel])


def _same(got, want, upto=None, where=None):
    assert int(got[0]) == want[0] and int(got[1]) == want[1], (where, got[:2], want[:2])
    k = want[1] if upto is None else min(upto, want[1])
    for g, w, what in zip(got[2:], want[2:], ("line", "begin", "finish", "result", "start", "end")):
        g = np.asarray(g)
        assert len(g) == k, (where, what, len(g), k)
        assert np.array_equal(g.astype(w.dtype), w[:k]), (where, what)


def _crossing(want_sel, text):
    """how many of the lines in `want_sel` (begin, finish arrays) cross a multiple of 16384"""
    b, f = want_sel
    return int(sum(any(int(x) < m <= int(y) for m in range(CHUNK, len(text), CHUNK))
                   for x, y in zip(b, f)))


def _guard(name, text, style, lead):
    """the standard text cannot pass vacuously: enough lines on both sides, on the borders too"""
    yes = _want(name, text, style, lead, False)
    no = _want(name, text, style, lead, True)
    assert yes[1] >= 100 and no[1] >= 100, (name, style, lead, yes[1], no[1])
    assert _crossing(yes[3:5], text) >= 2 and _crossing(no[3:5], text) >= 1, (name, style, lead)


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", SEVEN)
def test_grep_text_matrix_vs_oracle(name, style):
    exe = one_amd.Executable(load_dfa(name))
    text = _standard(PIECES[name]())
    for lead in (0, 1):
        if style != 5:
            _guard(name, text, style, lead)
        for invert in (False, True):
            want = _want(name, text, style, lead, invert)
            got = one_amd.grep_text(exe, text, style, bool(lead), invert=invert)
            assert one_amd.last_kernel() == "k_grep_text"
            _same(got, want, where=(name, style, lead, invert))


def _dev_call(exe, dev_text, style, lead, invert, cap, **kw):
    import torch
    out = one_amd.grep_text(exe, dev_text, style, bool(lead), invert=invert, cap=cap, **kw)
    torch.cuda.synchronize()
    k = min(int(out[1].item()), cap)
    return (int(out[0].item()), int(out[1].item())) + tuple(
        x[:k].cpu().numpy() if x is not None else None for x in out[2:])


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("name", ["log100", "aab"])
def test_grep_text_device_form(name, shift):
    """everything device-resident, the text at any offset from a 16-byte boundary"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = _standard(PIECES[name]())
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))
    assert dev.data_ptr() % 16 == shift
    for style in (STYLES if shift == 0 else (1, 4)):
        for lead in (0, 1):
            for invert in (False, True):
                want = _want(name, text, style, lead, invert)
                got = _dev_call(exe, dev, style, lead, invert, cap=want[0])
                assert one_amd.last_kernel() == "k_grep_text"
                _same(got, want, where=(name, shift, style, lead, invert))


@pytest.mark.parametrize("flags", [{}, {"force_generic": True}, {"force_global": True},
                                   {"force_hot": True}])
@pytest.mark.parametrize("name", ["uri", "syn256"])
def test_grep_text_every_table_placement(name, flags):
    exe = one_amd.Executable(load_dfa(name), **flags)
    text = _standard(PIECES["uri"]())
    for style in (1, 4):
        for lead in (0, 1):
            yes = _want(name, text, style, lead, False)
            no = _want(name, text, style, lead, True)
            if name == "syn256":  # selects nearly every line: invert is the "few selected" case
                assert yes[1] > 10 * max(no[1], 1) and no[1] < yes[0] // 8, (yes[1], no[1])
            for invert, want in ((False, yes), (True, no)):
                got = one_amd.grep_text(exe, text, style, bool(lead), invert=invert)
                assert one_amd.last_kernel() == "k_grep_text"
                _same(got, want, where=(name, flags, style, lead, invert))


def _mixed_text(kind="random", seed=1, n=4 * CHUNK + 5):
    """Random bytes (the random DFAs, syn256) or a / b / . (leaky) under _standard's delimiters,
    then a delimiter at every fourth byte of every third line of 12 bytes and more - short lines
    that mostly stay unselected, where the 1-199 byte lines are nearly all selected - and a 2-byte
    line across every even multiple of 16384."""
    import test_gpu_collect_text as CT
    key = ("mixed", kind, seed, n)
    if key not in _texts:
        if kind == "leaky":
            a = np.frombuffer(b"ab.", dtype=np.uint8)[
                np.random.default_rng(seed + 1).integers(0, 3, n)].copy()
        else:
            a = W.random_bytes(n, seed).copy()
            a[a == 0x0A] = 0x20
        ends = CT._delims(n, 1)
        a[ends] = 0x0A
        begin = 0
        for k, end in enumerate(ends):
            if k % 3 == 0 and end - begin >= 12:
                a[begin + 3:end:4] = 0x0A
            begin = end + 1
        for m in range(2 * CHUNK, n, 2 * CHUNK):
            a[m - 2] = a[m + 1] = 0x0A
        _texts[key] = bytes(a)
    return _texts[key]


def _placement_text(dfa):
    """what a placement row runs over: the regex DFAs' dense text, the mixed text otherwise"""
    import test_gpu_collect_text as CT
    if dfa in LP.PIECES:
        return CT._dense(LP.PIECES[dfa][0])
    return _mixed_text("leaky" if dfa == "leaky" else "random")


def _chunks_of(begins):
    return set((begins // np.uint64(CHUNK)).tolist())


def _placement_guard(dfa, text, style, lead):
    """on the oracle's output alone: both sides of the selection are large, begin in every one of
    the four chunks and have lines across a chunk border - k_gp_select's carried line and k_gp_write's
    record slots are exercised whichever way invert points"""
    yes = _want(dfa, text, style, lead, False)
    no = _want(dfa, text, style, lead, True)
    where = (dfa, style, lead)
    assert yes[1] >= 150 and no[1] >= 20, where + (yes[1], no[1])
    assert _chunks_of(yes[3]) >= {0, 1, 2, 3} and _chunks_of(no[3]) >= {0, 1, 2, 3}, where
    assert _crossing(yes[3:5], text) >= 2, where
    if dfa != "num3":       # (no line of num3's dense text that crosses a border stays unselected)
        assert _crossing(no[3:5], text) >= 1, where
    if dfa not in LP.PIECES and dfa != "leaky":
        assert len(set(yes[5].tolist())) >= 2, where + (set(yes[5].tolist()),)


_PLACEMENT_ROWS = LP.ROWS + [pytest.param(*p.values[:3], id=p.id) for p in LV.TABLE
                             if p.values[0] in ("syn256", "rnd72", "leaky") and not p.values[1]]


@pytest.mark.parametrize("dfa,opts,info", _PLACEMENT_ROWS)
def test_grep_text_under_placement(dfa, opts, info):
    """every table kind under both verbs of launchGrepText (search; match for a suffix-closed DFA
    without a leader), hot tables with 0 to 254 hot rows, a leader with the table in L2, a DFA
    without a pure dead state, u32 states with results in global memory"""
    import torch
    blob = _blob(dfa)
    facts = one_amd.Executable(blob, device="none").info
    for k, v in LP.FACTS.get(dfa, {}).items():
        assert facts[k] == v, (dfa, k, facts[k], v)
    text = _placement_text(dfa)
    assert len(text) == 4 * CHUNK + 5 and text[-1] != 0x0A
    for style in (1, 2, 3, 4):
        for lead in (0, 1):
            _placement_guard(dfa, text, style, lead)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    for style in STYLES:
        for lead in (0, 1):
            for invert in (False, True):
                want = _want(dfa, text, style, lead, invert)
                got = one_amd.grep_text(exe, text, style, bool(lead), invert=invert)
                assert one_amd.last_kernel() == "k_grep_text"
                _same(got, want, where=(dfa, opts, style, lead, invert))
    # truncation, grep -m and the select pass alone; the device form one byte off a 16-byte boundary
    style, lead = 4, 1
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + len(text)]
    dev.copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))
    assert dev.data_ptr() % 16 == 1
    for invert in (False, True):
        where = (dfa, opts, style, lead, invert)
        want = _want(dfa, text, style, lead, invert)
        cap = want[1] // 2
        _same(one_amd.grep_text(exe, text, style, bool(lead), invert=invert, cap=cap), want,
              upto=cap, where=where + ("cap",))
        _same(one_amd.grep_text(exe, text, style, bool(lead), invert=invert, max_count=7),
              _want(dfa, text, style, lead, invert, max_count=7), where=where + ("max_count",))
        got = one_amd.grep_text(exe, text, style, bool(lead), invert=invert, want_outcome=False)
        assert got[:2] == want[:2] and got[5] is None and got[6] is None and got[7] is None, where
        for g, w in zip(got[2:5], want[2:5]):
            assert np.array_equal(g, w), where + ("no outcome",)
        _same(_dev_call(exe, dev, style, lead, invert, cap=want[0]), want, where=where + ("dev",))
        assert one_amd.last_kernel() == "k_grep_text"


@pytest.mark.parametrize("name", ["set5", "newyork"])
def test_grep_text_results_other_than_one(name):
    exe = one_amd.Executable(load_dfa(name))
    if name == "newyork":
        text = _standard(b"New York")
        # "New" and "York" alone report other results than "New York"
        a = np.frombuffer(text, dtype=np.uint8).copy()
        offs = [int(o) for o in _lines_of(text)]
        for k in range(1, len(offs) - 1, 5):
            if offs[k + 1] - offs[k] > 8 and not any(
                    offs[k] < m <= offs[k + 1] for m in range(CHUNK, len(text), CHUNK)):
                a[offs[k]:offs[k] + 4] = np.frombuffer(b"New " if k % 2 else b"York", dtype=np.uint8)
        text = bytes(a)
    else:
        text = _standard(b"012345")
    for style in STYLES:
        for lead in (0, 1):
            want = _want(name, text, style, lead)
            if style in (1, 4):
                assert len(set(want[5].tolist())) >= 2, (name, style, lead, set(want[5].tolist()))
            _same(one_amd.grep_text(exe, text, style, bool(lead)), want, where=(name, style, lead))


def _shapes():
    piece = b"error"
    short = b"an error here\nnothing\n\nerror\nno\n"
    out = {
        "empty": b"",
        "no delimiter": b"an error without a line end",
        "only delimiters": b"\n" * (2 * CHUNK + 3),
        "delimiter at a chunk's last byte": (b"x" * 40 + b"\n") * 399 + b"y error " + b"z" * 16
                                            + b"\n" + short,
        "delimiter at a chunk's first byte": (b"x" * 40 + b"\n") * 399 + b"y error " + b"z" * 17
                                             + b"\n" + short,
        "one 40,000-byte line": short + b"q" * 33000 + piece + b"r" * (40000 - 33005) + b"\n" + short,
        "tail without a delimiter": short * 3 + b"an error in the tail",
    }
    assert (len(out["delimiter at a chunk's last byte"]) - len(short)) == CHUNK
    assert out["delimiter at a chunk's last byte"][CHUNK - 1] == 0x0A
    assert out["delimiter at a chunk's first byte"][CHUNK] == 0x0A
    big = out["one 40,000-byte line"]
    assert len(short) + 33000 > 2 * CHUNK and big.count(b"\n") == 11
    return out


@pytest.mark.parametrize("shape", list(_shapes()))
def test_grep_text_shapes(shape):
    text = _shapes()[shape]
    for name in ("err", "dotstar_err"):
        exe = one_amd.Executable(load_dfa(name))
        for style in (1, 4, 5):
            for lead in (0, 1):
                for invert in (False, True):
                    want = _want(name, text, style, lead, invert)
                    got = one_amd.grep_text(exe, text, style, bool(lead), invert=invert)
                    _same(got, want, where=(shape, name, style, lead, invert))
    n_lines = _want("err", text, 1, 1)[0]
    assert n_lines == {"empty": 0, "no delimiter": 0, "only delimiters": 2 * CHUNK + 3}.get(
        shape, n_lines)
    if shape == "tail without a delimiter":
        assert _want("err", text, 1, 1)[1] == 6  # the tail's "error" is in no line


def test_grep_text_empty_and_lineless_on_the_device():
    """the _dev form writes both zero counts on the stream"""
    import torch
    exe = one_amd.Executable(load_dfa("err"))
    for text in (b"", b"error, and no line end"):
        dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        for invert in (False, True):
            got = _dev_call(exe, dev, 1, 1, invert, cap=4)
            assert got[:2] == (0, 0)


def test_grep_text_other_delimiter():
    exe = one_amd.Executable(load_dfa("err"))
    text = _standard(b"error").replace(b"\n", b"\x00")
    for invert in (False, True):
        want = _want("err", text, 1, 1, invert, delim=0)
        assert want[0] > 600 and want[1] >= 100
        _same(one_amd.grep_text(exe, text, 1, True, invert=invert, delim=b"\x00"), want)
        # ... and with '\n' the same text has no line at all
        assert one_amd.grep_text(exe, text, 1, True, invert=invert)[:2] == (0, 0)


def test_grep_text_truncation_and_limits():
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    text = _standard(PIECES[name]())
    for invert in (False, True):
        full = _want(name, text, 4, 1, invert)
        count = full[1]
        assert count >= 100
        # cap below the count: the first cap records, the full count
        for cap in (1, 63, 64, 65, count - 1):
            _same(one_amd.grep_text(exe, text, 4, True, invert=invert, cap=cap), full, upto=cap,
                  where=("cap", cap, invert))
        # cap = 0 and no arrays: the count alone
        got = one_amd.grep_text(exe, text, 4, True, invert=invert, cap=0)
        assert got[:2] == (full[0], count) and all(len(x) == 0 for x in got[2:])
        # max_count
        for mx in (0, 1, 5, count + 3):
            want = _want(name, text, 4, 1, invert, max_count=mx)
            assert want[1] == min(mx, count)
            _same(one_amd.grep_text(exe, text, 4, True, invert=invert, max_count=mx), want,
                  where=("max", mx, invert))
            _same(one_amd.grep_text(exe, text, 4, True, invert=invert, max_count=mx, cap=3), want,
                  upto=3, where=("max and cap", mx, invert))
        # without the Outcome
        got = one_amd.grep_text(exe, text, 4, True, invert=invert, want_outcome=False)
        assert got[5] is None and got[6] is None and got[7] is None
        for g, w in zip(got[2:5], full[2:5]):
            assert np.array_equal(g, w)


def test_grep_text_some_arrays_null():
    """every array pointer, and n_lines, may be NULL on its own"""
    name = "aab"
    lib = _lib.lib()
    exe = one_amd.Executable(load_dfa(name))
    text = _standard(PIECES[name]())
    want = _want(name, text, 4, 0)
    cap = want[1]
    dtypes = [np.uint64, np.uint64, np.uint64, np.int32, np.uint64, np.uint64]
    for keep in ([0], [1], [2], [3], [4], [5], [0, 3], [1, 2, 5], [3, 4, 5], []):
        arrs = [np.full(cap, 0x55, dtype=dt) if k in keep else None for k, dt in enumerate(dtypes)]
        ns, nl = C.c_uint64(0), C.c_uint64(0)
        for n_lines in (C.byref(nl), None):
            rc = lib.redgpu_grep_text(exe._h, 4, 0, 0, text, len(text), 0x0A, 1 << 62, cap, n_lines,
                                      C.byref(ns), *[a.ctypes.data if a is not None else None
                                                     for a in arrs])
            assert rc == 0, lib.redgpu_last_error()
            assert ns.value == want[1]
            for k in keep:
                assert np.array_equal(arrs[k], want[2 + k].astype(dtypes[k])), (keep, k)
        assert nl.value == want[0]


@pytest.mark.parametrize("invert", [0, 1])
def test_grep_text_device_cap_below_count_leaves_the_rest_untouched(invert):
    """_dev with cap below the count: the first cap records, the full count, and nothing written
    from min(n_selected, cap) on - also when max_count is what ends the records"""
    import torch
    name = "log100"
    lib = _lib.lib()
    exe = one_amd.Executable(load_dfa(name))
    text = _standard(PIECES[name]())
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    full = _want(name, text, 4, 1, bool(invert))
    room = full[1] + 8
    for cap, mx in ((1, 1 << 62), (64, 1 << 62), (full[1] - 1, 1 << 62), (room, 5), (70, 66)):
        want = _want(name, text, 4, 1, bool(invert), max_count=mx)
        outs = [torch.full((room,), 0x55, dtype=torch.int32 if k == 3 else torch.int64,
                           device="cuda") for k in range(6)]
        cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        rc = lib.redgpu_grep_text_dev(exe._h, 4, 1, invert, dev.data_ptr(), dev.numel(), 0x0A, mx,
                                      cap, cnt.data_ptr(), cnt.data_ptr() + 8,
                                      *[o.data_ptr() for o in outs],
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.redgpu_last_error()
        torch.cuda.synchronize()
        assert cnt.tolist() == [want[0], want[1]], (cap, mx)
        k = min(want[1], cap)
        for o, w in zip(outs, want[2:]):
            o = o.cpu().numpy()
            assert np.array_equal(o[:k], w[:k].astype(o.dtype)), (cap, mx)
            assert (o[k:] == 0x55).all(), (cap, mx)


def test_grep_text_two_streams_and_threads():
    import torch
    names = ("log100", "err")
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [_standard(PIECES[n](), seed=2 + k) for k, n in enumerate(names)]
    wants = [_want(n, t, 4, 1) for n, t in zip(names, texts)]
    assert wants[0][1] != wants[1][1] or not np.array_equal(wants[0][2], wants[1][2])
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, exe, d, w in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.grep_text(exe, d, 4, True, cap=w[0]))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        k = int(got[1].item())
        _same((int(got[0].item()), k) + tuple(x[:k].cpu().numpy() for x in got[2:]), w)
    errors = []

    def work(exe, t, d, st, w):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.grep_text(exe, d, 4, True, cap=w[0])
                    st.synchronize()
                k = int(got[1].item())
                _same((int(got[0].item()), k) + tuple(x[:k].cpu().numpy() for x in got[2:]), w)
                _same(one_amd.grep_text(exe, t, 4, True), w)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_grep_text_cpp_mirror(tmp_path):
    """redgpu::grepText / grepCount (include/redgpu.hpp) compiled with g++, against the oracle"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "grep_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "grep_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "log100"
    text = b"ab\n" * 2000 + _standard(PIECES[name]())
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    # (the mirror's first room is len / 128 + 16 = 574 records: the inverted run needs the retry)
    for style, lead, invert, mx in ((4, 1, 0, 1 << 62), (1, 0, 1, 1 << 62), (4, 1, 0, 7)):
        want = _want(name, text, style, lead, bool(invert), max_count=mx)
        out = subprocess.run([prog, dfa, str(path), str(style), str(lead), str(invert), str(mx)],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.split("\n")
        assert rows[0] == "count %d" % want[1] and rows[1] == "hits %d" % want[1], rows[:2]
        got = np.array([[int(v) for v in r.split()] for r in rows[2:2 + want[1]]],
                       dtype=np.int64).reshape(want[1], 6)
        for k in range(6):
            assert np.array_equal(got[:, k], want[2 + k].astype(np.int64)), k
        dflt = _want(name, text, 1, 1)
        assert rows[2 + want[1]] == "default %d %d" % (dflt[1], dflt[1])
    assert _want(name, text, 1, 0, True)[1] > len(text) // 128 + 16
