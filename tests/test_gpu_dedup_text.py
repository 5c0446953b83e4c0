"""dedup_text (redgpu_dedup_text[_dev]): awk '!seen[$k]++' of a raw text - the lines chosen by the
content of their keys, put together as a text.  Every count and byte is exact against
tests/dedup_rule.py over the CPU oracle (text_rules.Text: the lines, search per line, collect's
pieces): the four modes x count windows x invert x keep_unkeyed on five DFAs, a hand-built text of
edge traps whose facts are asserted before the GPU is asked, the shapes, a hot key, a text of more
chunks than the grid has waves, tables exactly full and overflowing, a key of 2^24 bytes, truncation
with sentinels and NULL counters, every table placement, the device form at odd pointer offsets,
other delimiters, determinism, streams and threads, the composition with fields_text, the C++
mirror and a smoke run of scripts/fuzz_gpu.py's keys mode."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from golden_util import load_dfa

import dedup_rule as DR
import text_rules as TR
import test_gpu_collect_text as CT
import test_gpu_list_verbs as LV
import test_gpu_long_placements as LP
import test_gpu_uniq_text as UQ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
SENT = 0x55
SENT64 = 0x5555555555555555
MAX = DR.MAX
KERNEL = "k_dedup_text"
WINDOWS = [(1, MAX), (1, 1), (2, MAX), (3, 2)]
FUZZ_CASES, FUZZ_SEED = "32", "11"       # (test_dedup_rule.py holds the dry run of these to floors)
SEP = b"error"                           # the separator the err DFA finds

_cache = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _t(name, text, delim=0x0A):
    key = (name, text, delim)
    if key not in _cache:
        _cache[key] = TR.Text(O.CpuOracle(CT._blob(name)), text, delim)
    return _cache[key]


def _kw(what="whole", key_index=1, style=1, lead=1, window=(1, MAX), invert=False, keep=False):
    """(dedup_rule's arguments, dedup_text's)"""
    rule = dict(what=what, key_index=key_index, style=style, lead=lead, min_count=window[0],
                max_count=window[1], invert=invert, keep_unkeyed=keep)
    verb = dict(what=what, key_index=key_index, style=style, do_leader=bool(lead),
                min_count=window[0], max_count=window[1], invert=invert, keep_unkeyed=keep)
    return rule, verb


def _dev_call(exe, text, shift=1, room=None, **verb):
    """the device form into a sentinel-filled buffer: (the six counts, the buffer's bytes)"""
    import torch
    dev = UQ._dev_text(text, shift)
    buf = torch.full(((len(text) if room is None else room) + 16,), SENT, dtype=torch.uint8,
                     device="cuda")
    got = one_amd.dedup_text(exe, dev, out=buf, out_cap=len(buf) - 16, **verb)
    assert one_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    assert all(t.is_cuda and t.dtype == torch.int64 and t.shape == (1,) for t in got[:6])
    return tuple(int(t.item()) for t in got[:6]), buf.cpu().numpy().tobytes()


def _same(exe, name, text, delim=b"\n", forms=("host", "dev"), where=None, max_distinct=4096,
          **k):
    """both forms against the rule; returns the rule's tuple"""
    rule, verb = _kw(**k)
    want = DR.dedup(_t(name, text, delim[0]), **rule)
    verb.update(delim=delim, max_distinct=max_distinct)
    if "host" in forms:
        got = one_amd.dedup_text(exe, text, **verb)
        assert one_amd.last_kernel() == KERNEL
        assert got[:5] == want[:5], (where, k, got[:5], want[:5])
        assert got[5] == want[5], (where, k, len(got[5]), len(want[5]))
    if "dev" in forms:
        counts, back = _dev_call(exe, text, **verb)
        assert counts == want[:5] + (len(want[5]),), (where, k, counts, want[:5])
        n = len(want[5])
        assert back[:n] == want[5] and back[n:] == bytes([SENT]) * (len(back) - n), (where, k)
    return want


# 1 the matrix -------------------------------------------------------------------------------------
def _matrix_text(name):
    """about three chunks: a dense text of a chunk and a half, and its first 60 % again - lines
    that occur twice, lines that occur once, and a tail that repeats the first line"""
    half = CT._dense(CT.PIECES[name](), n=CHUNK + CHUNK // 2 + 3, end_in_delim=True)
    cut = half.rindex(b"\n", 0, len(half) * 6 // 10) + 1
    return half + half[:cut] + half[:half.index(b"\n")]


@pytest.mark.parametrize("name", ["log100", "num3", "uri", "aab", "err"])
def test_dedup_text_matrix_vs_oracle(name):
    text = _matrix_text(name)
    assert 2 * CHUNK < len(text) < 3 * CHUNK and not text.endswith(b"\n")
    t = _t(name, text)
    most = max(len(p) for p in t.pieces())
    assert most >= 1
    # the oracle's side first: every mode has keyed lines, strings that repeat and strings that do
    # not; one key index above what any line has leaves every line unkeyed
    for what, ks in (("whole", [1]), ("lines", [1]), ("match", [1, 2, most + 1]),
                     ("field", [1, 2, most + 2])):
        for k in ks:
            n_keyed, n_distinct, _ = DR.emitted(DR.keys(t, what, k))
            if k > 2:
                assert n_keyed == 0
            elif k == 1:
                assert 0 < n_distinct < n_keyed, (what, n_keyed, n_distinct)
    exe = one_amd.Executable(load_dfa(name))
    outs = set()
    for what, ks in (("whole", [1]), ("lines", [1]), ("match", [1, 2, most + 1]),
                     ("field", [1, 2, most + 2])):
        for k, window, invert, keep in itertools.product(ks, WINDOWS, (False, True), (False, True)):
            want = _same(exe, name, text, where=name, what=what, key_index=k,
                         window=window, invert=invert, keep=keep)
            outs.add(want[5])
    assert len(outs) >= 12, len(outs)
    # under LINES another style and no leader
    _same(exe, name, text, what="lines", style=4, lead=0, window=(2, MAX), keep=True)


# 2 edge traps -------------------------------------------------------------------------------------
def _filler(i, size):
    """a line of `size` bytes with its delimiter, its first field a key of its own"""
    head = b"f%05d" % i + SEP
    assert size > len(head)
    return head + b"." * (size - len(head) - 1) + b"\n"


def _trap_text():
    """four chunks and a tail, built by hand for the err DFA as the separator: (text, marks), marks
    naming the offsets the facts below are asserted at"""
    out, marks, n = bytearray(), {}, [0]

    def fill(upto):
        """filler lines of 60 to 89 bytes, and a last one that ends the text at exactly `upto`"""
        assert upto - len(out) > 200
        while len(out) < upto:
            room = upto - len(out)
            out.extend(_filler(n[0], room if room <= 200 else 60 + n[0] % 30))
            n[0] += 1
        assert len(out) == upto

    def put(name, line):
        marks[name] = len(out)
        out.extend(line + b"\n")

    put("ends_first", b"onlyends" + SEP + b"first chunk")
    put("long", b"longkey" + SEP + b"L" * 40000)                 # three chunks in one line
    put("round_a", b"dupA" + SEP + b"1")
    put("round_b", b"dupA" + SEP + b"2")
    for k, key in enumerate((b"pre", b"pref", b"prefi", b"prefix", b"prefiy", b"prefix")):
        put("prefix%d" % k, key + SEP + b"p")
    put("empty_end_a", b"abc" + SEP)                             # field 2: empty, ON the delimiter
    put("empty_mid", b"abd" + SEP + SEP + b"tail")               # field 2: empty, in the line
    put("empty_first", SEP + b"behind an empty first field")
    put("empty_line_a", b"")
    put("once", b"uniq1" + SEP + b"x")
    fill(3 * CHUNK - 40)
    put("border", b"dupA" + SEP + b"z" * (40 - 4 - len(SEP)))    # its delimiter: byte 3 * CHUNK
    fill(3 * CHUNK + 1024 + 31)
    put("bit31", b"w" + SEP + b"31")                             # begins on bit 31 of a word
    fill(3 * CHUNK + 2048 + 255)
    put("bit255", b"l" + SEP + b"255")                           # begins on a lane's last bit
    put("empty_end_b", b"xyz" + SEP)
    put("empty_line_b", b"")
    put("long_again", b"longkey" + SEP + b"short this time")
    fill(4 * CHUNK - 100)
    put("ends_last", b"onlyends" + SEP + b"last chunk")
    marks["tail"] = len(out)
    out.extend(b"uniq1" + SEP + b"in the tail, no delimiter")
    return bytes(out), marks


def _line_of(t, at):
    i = int(np.searchsorted(t.offs, at, side="right")) - 1
    assert int(t.offs[i]) == at, at
    return i


def _trap_facts():
    """the trap text, each fact asserted on the oracle's side: no GPU is asked"""
    text, m = _trap_text()
    assert 4 * CHUNK - 100 < len(text) < 4 * CHUNK + 100
    t = _t("err", text)
    at = {k: _line_of(t, v) for k, v in m.items() if k != "tail"}
    k1, k2 = DR.keys(t, "field", 1), DR.keys(t, "field", 2)
    fin = lambda name: int(t.offs[at[name] + 1]) - 1            # noqa: E731  the line's delimiter
    # equal keys in the first and in the last chunk only
    a, b = at["ends_first"], at["ends_last"]
    assert k1[a] == (0, b"onlyends") and k1[b][1] == b"onlyends" and k1[b][0] > 3 * CHUNK
    assert [k[1] for k in k1].count(b"onlyends") == 2
    # two equal keys in one round of 64 lines, in one lane's 256 bits
    a, b = at["round_a"], at["round_b"]
    assert b == a + 1 and k1[a][1] == k1[b][1] == b"dupA" and fin("round_a") >> 8 == fin("round_b") >> 8
    # a key whose line's delimiter is the first byte of the next chunk
    assert fin("border") == 3 * CHUNK and k1[at["border"]] == (3 * CHUNK - 40, b"dupA")
    # a key that starts on bit 31 of a word / on a lane's last bit, its delimiter in the next
    assert k1[at["bit31"]][0] % 32 == 31 and fin("bit31") >> 5 == (k1[at["bit31"]][0] >> 5) + 1
    assert k1[at["bit255"]][0] % 256 == 255 and fin("bit255") >> 8 == (k1[at["bit255"]][0] >> 8) + 1
    # a 40 KiB line over three chunks, keyed at its first field, which comes again later
    assert fin("long") - m["long"] > 2 * CHUNK and fin("long") // CHUNK == m["long"] // CHUNK + 2
    assert k1[at["long"]][1] == k1[at["long_again"]][1] == b"longkey"
    # an empty field as key at the line's very end: the key sits on the delimiter's bit
    assert k2[at["empty_end_a"]] == (fin("empty_end_a"), b"")
    assert k2[at["empty_end_b"]] == (fin("empty_end_b"), b"") and k2[at["empty_mid"]][1] == b""
    assert k2[at["empty_mid"]][0] < fin("empty_mid") - 4
    # an empty first field; an empty line: field 1 of it is the empty key too
    assert k1[at["empty_first"]] == (m["empty_first"], b"")
    assert k1[at["empty_line_a"]] == (m["empty_line_a"], b"") and k2[at["empty_line_a"]] is None
    # proper prefixes of each other, and keys equal but for the last byte
    assert [k1[at["prefix%d" % k]][1] for k in range(6)] == [b"pre", b"pref", b"prefi", b"prefix",
                                                           b"prefiy", b"prefix"]
    # the tail repeats a key that occurs once: it is no line, and the count stays 1
    assert text[m["tail"]:].startswith(b"uniq1" + SEP) and b"\n" not in text[m["tail"]:]
    assert [k[1] for k in k1].count(b"uniq1") == 1
    once = DR.dedup(t, "field", 1, min_count=1, max_count=1)
    assert t.line_bytes(at["once"]) in once[5] and t.line_bytes(at["round_a"]) not in once[5]
    whole = DR.keys(t, "whole")
    assert whole[at["empty_line_a"]][1] == whole[at["empty_line_b"]][1] == b""
    return text


def test_dedup_text_edge_traps():
    text = _trap_facts()
    exe = one_amd.Executable(load_dfa("err"))
    for what, k in (("field", 1), ("field", 2), ("match", 1), ("whole", 1), ("lines", 1)):
        for window, invert, keep in itertools.product(WINDOWS[:3], (False, True), (False, True)):
            _same(exe, "err", text, where="traps", what=what, key_index=k, window=window,
                  invert=invert, keep=keep)


def test_dedup_text_empty_lines():
    """An empty line is keyed by the empty string under WHOLE.  Under LINES it would be, were it
    selected: search over an empty line reports no match for any DFA the oracle knows
    (test_dedup_rule.py: test_no_dfa_selects_an_empty_line fails as soon as one does), so there it
    is unkeyed - the rule, asserted first, says which."""
    name = "aab"
    text = b"\naab\n\naab\ncd\n\n" * 1400 + b"zz aab\n\n"
    t = _t(name, text)
    empties = [i for i, line in enumerate(t.lines) if not line]
    sel = set(TR.selected(t).tolist())
    assert len(empties) > 4000 and not set(empties) & sel and len(sel) > 2000 and len(text) > CHUNK
    assert [k is None for k in DR.keys(t, "lines")].count(True) == t.n_lines - len(sel)
    assert DR.dedup(t, "whole")[1:5] == (t.n_lines, 4, 0, 4)
    exe = one_amd.Executable(load_dfa(name))
    for what in ("lines", "whole"):
        for window, invert, keep in itertools.product(WINDOWS[:3], (False, True), (False, True)):
            _same(exe, name, text, what=what, window=window, invert=invert, keep=keep)


# 3 the shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CT._shapes()))
def test_dedup_text_shapes(shape):
    text = CT._shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        for what, k in (("whole", 1), ("lines", 1), ("match", 1), ("match", 2), ("field", 2)):
            for invert, keep in ((False, False), (True, True)):
                want = _same(exe, name, text, where=(shape, name), what=what, key_index=k,
                             invert=invert, keep=keep)
                if shape in ("no delimiter", "empty", "one byte, no delimiter"):
                    assert want == (0, 0, 0, 0, 0, b"")
    if shape == "one byte, a delimiter":
        assert DR.dedup(_t("aab", text)) == (1, 1, 1, 0, 1, b"\n")
    if shape == "a chunk of delimiters alone":          # the empty lines: ONE distinct empty key
        per = DR.keys(_t("aab", text), "whole")
        assert [k[1] for k in per].count(b"") == CHUNK


# 4 a hot key --------------------------------------------------------------------------------------
def test_dedup_text_hot_key():
    text = CT.UNIT * 6000          # 90,000 bytes, 5.5 chunks, every line the same
    exe = one_amd.Executable(load_dfa("num3"))
    for what, k in (("whole", 1), ("lines", 1), ("match", 1), ("match", 2), ("field", 1),
                    ("field", 3)):
        want = _same(exe, "num3", text, what=what, key_index=k)
        assert want[:5] == (6000, 6000, 1, 0, 1) and want[5] == CT.UNIT
        want = _same(exe, "num3", text, what=what, key_index=k, invert=True)
        assert want[4] == 5999 and want[5] == text[len(CT.UNIT):]
        assert _same(exe, "num3", text, what=what, key_index=k, window=(6001, MAX))[4] == 0
        assert _same(exe, "num3", text, what=what, key_index=k, window=(6000, 6000))[4] == 1


def test_dedup_text_above_the_grid():
    """test_uniq_text_above_the_grid's 160 MiB: a 64 KiB block that ends in a delimiter, tiled on the
    device.  Every string's first occurrence lies in the first block and its count is the block's
    times the tiles: the defaults emit what the single block emits, and a min_count of tiles * c
    selects what min_count = c selects in the block - exactly on and one above a block's count."""
    import torch
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 4 * CHUNK, 2560
    assert tiles * 4 > props.multi_processor_count * 8 * 4
    body = CT._dense(b"12345a")
    block = body[:body.rindex(b"\n", 0, block_len - 64) + 1]
    block = block + b" " * (block_len - len(block) - 1) + b"\n"
    assert len(block) == block_len
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    t = _t("num3", block)
    exe = one_amd.Executable(load_dfa("num3"))
    for what in ("match", "whole"):
        per = DR.keys(t, what)
        strings = [k[1] for k in per if k is not None]
        c = sorted(strings.count(s) for s in set(strings))[len(set(strings)) // 2]
        assert len(set(strings)) > 20
        runs = [((1, MAX), (1, MAX)), ((tiles * c, MAX), (c, MAX)), ((tiles * c + 1, MAX), (c + 1, MAX)),
                ((1, tiles * c), (1, c))]
        for window, in_block in runs:
            want = DR.dedup(t, what, min_count=in_block[0], max_count=in_block[1])
            buf = torch.full((len(want[5]) + 16,), SENT, dtype=torch.uint8, device="cuda")
            got = one_amd.dedup_text(exe, dev, what=what, min_count=window[0], max_count=window[1],
                                     max_distinct=4096, out=buf, out_cap=len(want[5]))
            assert one_amd.last_kernel() == KERNEL
            torch.cuda.synchronize()
            assert [x.item() for x in got[:6]] == [want[0] * tiles, want[1] * tiles, want[2], 0,
                                                   want[4], len(want[5])], (what, window)
            back = buf.cpu().numpy().tobytes()
            assert back[:len(want[5])] == want[5] and back[len(want[5]):] == bytes([SENT]) * 16
        assert len(DR.dedup(t, what, min_count=c)[5]) > len(DR.dedup(t, what, min_count=c + 1)[5])


# 5 many keys, small tables ------------------------------------------------------------------------
@pytest.mark.parametrize("distinct,max_distinct", [(60, 32), (64, 32), (128, 32), (60, 64),
                                                   (64, 64), (128, 64), (200, 64)])
@pytest.mark.parametrize("what", ["match", "whole"])
def test_dedup_text_small_tables(distinct, max_distinct, what):
    slots = 2 * max_distinct
    text = UQ._keys_text(distinct)
    t = _t("num3", text)
    per = DR.keys(t, what)
    exact = DR.dedup(t, what)
    assert exact[1:5] == (3 * distinct, distinct, 0, distinct)
    exe = one_amd.Executable(load_dfa("num3"))
    if distinct <= slots:        # a table exactly full still drops nothing
        for invert in (False, True):
            _same(exe, "num3", text, max_distinct=max_distinct, what=what, invert=invert)
        return
    # overflow: which strings have a record depends on scheduling, what a mark says does not
    exact_lines = exact[5].split(b"\n")[:-1]
    verb = dict(what=what, max_distinct=max_distinct)
    host = one_amd.dedup_text(exe, text, **verb)
    counts, back = _dev_call(exe, text, **verb)
    for n_lines, n_keyed, n_distinct, n_dropped, n_emitted, out in (
            host, counts[:5] + (back[:counts[5]],)):
        assert (n_lines, n_keyed) == exact[:2]
        assert n_dropped > 0 and n_distinct == slots
        lines = out.split(b"\n")[:-1]
        assert len(lines) == n_emitted == len(set(lines)) and out.endswith(b"\n")
        # every emitted line is one the exact output holds, in its order; its key is in no
        # earlier line: the first line of its string
        it = iter(exact_lines)
        assert all(any(line == x for x in it) for line in lines)
        missing = len(exact_lines) - len(lines)
        assert n_emitted + missing == exact[4] and missing > 0
        firsts = {}
        for i, k in enumerate(per):
            firsts.setdefault(k[1], t.lines[i])
        assert set(lines) <= set(firsts.values())
    assert counts[5] == len(back[:counts[5]]) and back[counts[5]:] == bytes([SENT]) * (len(back) - counts[5])
    assert len(host[5]) == sum(len(x) + 1 for x in host[5].split(b"\n")[:-1])


# 6 a key of 2^24 bytes ----------------------------------------------------------------------------
@pytest.mark.parametrize("size,kept", [((1 << 24), 0), ((1 << 24) - 1, 1)])
def test_dedup_text_overlong_key(size, kept):
    long_line = b"error" + b"x" * (size - 5)
    short = b"a short error line"
    text = short + b"\n" + long_line + b"\n" + short + b"\nnothing\n"
    exe = one_amd.Executable(load_dfa("err"))
    got = one_amd.dedup_text(exe, text, max_distinct=32)
    assert one_amd.last_kernel() == KERNEL
    # a dropped line is keyed and not marked
    assert got[:5] == (4, 4, 2 + kept, 1 - kept, 2 + kept)
    assert got[5] == short + b"\n" + (long_line + b"\n" if kept else b"") + b"nothing\n"
    inv = one_amd.dedup_text(exe, text, max_distinct=32, invert=True)
    assert inv[:5] == (4, 4, 2 + kept, 1 - kept, 2 - kept)
    assert inv[5] == (b"" if kept else long_line + b"\n") + short + b"\n"
    # LINES: the selected lines alone are keyed
    got = one_amd.dedup_text(exe, text, what="lines", max_distinct=32, keep_unkeyed=True)
    assert got[:5] == (4, 3, 1 + kept, 1 - kept, 2 + kept)


# 7 truncation, NULL outputs -----------------------------------------------------------------------
def _raw(exe, text, dev, out_cap, counts=(1,) * 6, out=True, what=0, invert=0):
    """the C-ABI itself, sentinels in every output: ([six counters], the output buffer's bytes)"""
    import torch
    lib = _lib.lib()
    room = len(text) + 16
    args = [what, 1, 1, 1, 1, MAX, invert, 0]
    if dev is None:
        cnt = (C.c_uint64 * 6)(*([SENT64] * 6))
        buf = (C.c_uint8 * room)(*([SENT] * room))
        a = _u8(text)
        rc = lib.redgpu_dedup_text(
            exe._h, *args, a.ctypes.data if len(text) else None, len(text), 0x0A, 64,
            *[C.addressof(cnt) + 8 * i if h else None for i, h in enumerate(counts)],
            C.addressof(buf) if out else None, out_cap)
        assert rc == 0, lib.redgpu_last_error()
        return list(cnt), bytes(buf)
    cnt = torch.full((6,), SENT64, dtype=torch.int64, device="cuda")
    buf = torch.full((room,), SENT, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    rc = lib.redgpu_dedup_text_dev(
        exe._h, *args, dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A, 64,
        *[cnt.data_ptr() + 8 * i if h else None for i, h in enumerate(counts)],
        buf.data_ptr() if out else None, out_cap, st.cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    st.synchronize()
    return cnt.cpu().numpy().astype(np.uint64).tolist(), buf.cpu().numpy().tobytes()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_dedup_text_truncation_and_null_outputs(form):
    text = UQ._keys_text(20, rounds=2) + b"12 12 12\n" + b"a tail"
    t = _t("num3", text)
    want = DR.dedup(t, "whole")
    out = want[5]
    assert want[1:5] == (41, 21, 0, 21) and len(out) > 2000
    exe = one_amd.Executable(load_dfa("num3"))
    dev = UQ._dev_text(text, 7) if form == "dev" else None
    counts = list(want[:5]) + [len(out)]
    mid = len(t.lines[0]) + 1 + len(t.lines[1]) // 2      # in the middle of the second line
    for cap in (0, 1, mid, len(out) - 1, len(out), len(out) + 5):
        cnt, back = _raw(exe, text, dev, cap)
        assert cnt == counts, (cap, cnt)
        k = min(cap, len(out))
        assert back[:k] == out[:k] and back[k:] == bytes([SENT]) * (len(back) - k), cap
    for skip in range(6):
        have = [i != skip for i in range(6)]
        if skip == 5:
            continue        # (out_len is required: test_dedup_text_api.py)
        cnt, back = _raw(exe, text, dev, len(out), counts=have)
        assert cnt == [w if h else SENT64 for w, h in zip(counts, have)]
        assert back[:len(out)] == out
    cnt, back = _raw(exe, text, dev, len(out), counts=(0, 0, 0, 0, 0, 1))
    assert cnt == [SENT64] * 5 + [len(out)] and back[:len(out)] == out
    cnt, back = _raw(exe, text, dev, len(out), out=False)
    assert cnt == counts and back == bytes([SENT]) * len(back)
    # an empty text, one without a delimiter: all counts 0, nothing written
    for empty in (b"", b"123 and no line end"):
        d = UQ._dev_text(empty, 1) if form == "dev" else None
        cnt, back = _raw(exe, empty, d, 16)
        assert cnt == [0] * 6 and back == bytes([SENT]) * len(back)


# 8 every table placement --------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", UQ._ROWS)
def test_dedup_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    if dfa in LP.PIECES:
        half = CT._dense(LP.PIECES[dfa][0], n=CHUNK + 700, end_in_delim=True)
    else:
        half = CT._random_text("leaky" if dfa == "leaky" else "random", n=CHUNK + 700)
        half = half[:half.rindex(b"\n") + 1]
    text = half + half[:half.rindex(b"\n", 0, len(half) // 2) + 1]
    keyed = 0
    for what, k, style, lead in (("lines", 1, 1, 1), ("lines", 1, 4, 0), ("match", 1, 1, 1),
                                 ("match", 2, 1, 1), ("field", 1, 1, 1), ("field", 2, 1, 1)):
        for window, invert in (((1, MAX), False), ((2, MAX), True)):
            want = _same(exe, dfa, text, forms=("host",) if invert else ("host", "dev"),
                         where=(dfa, opts), what=what, key_index=k, style=style, lead=lead,
                         window=window, invert=invert, keep=invert)
            keyed += want[1]
    assert keyed > 100, (dfa, keyed)


# 9 the device form --------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_dedup_text_device_pointer_offsets(shift):
    import torch
    text = _matrix_text("num3")
    exe = one_amd.Executable(load_dfa("num3"))
    st = torch.cuda.Stream()
    for what in DR.WHATS:
        want = DR.dedup(_t("num3", text), what, invert=True)
        dev = UQ._dev_text(text, shift)
        assert dev.data_ptr() % 16 == shift
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = one_amd.dedup_text(exe, dev, what=what, invert=True, max_distinct=4096,
                                     out_cap=len(want[5]) + shift)
        st.synchronize()
        assert tuple(x.item() for x in got[:6]) == want[:5] + (len(want[5]),), (shift, what)
        assert got[6][:len(want[5])].cpu().numpy().tobytes() == want[5]


# 10 other delimiters ------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_dedup_text_other_delimiter(delim):
    text = _matrix_text("num3").replace(delim, b",").replace(b"\n", delim)
    assert b"\n" not in text and text.count(delim) > 300
    exe = one_amd.Executable(load_dfa("num3"))
    for what in DR.WHATS:
        want = _same(exe, "num3", text, delim=delim, what=what, window=(2, MAX), keep=True)
        assert want[4] > 0
    assert one_amd.dedup_text(exe, text)[:5] == (0, 0, 0, 0, 0)


# 11 determinism, streams and threads --------------------------------------------------------------
def test_dedup_text_bit_identical_runs():
    text = _matrix_text("num3")
    exe = one_amd.Executable(load_dfa("num3"))
    for what in DR.WHATS:
        runs = [_dev_call(exe, text, 0, what=what, invert=True, max_distinct=2048)
                for _ in range(3)]
        assert runs[0] == runs[1] == runs[2] and runs[0][0][3] == 0
        assert one_amd.dedup_text(exe, text, what=what) == one_amd.dedup_text(exe, text, what=what)


def test_dedup_text_two_streams_and_threads():
    import torch
    names = ["num3", "aab"]
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [_matrix_text(n) for n in names]
    wants = [DR.dedup(_t(n, x), "match", keep_unkeyed=True) for n, x in zip(names, texts)]
    assert wants[0][5] != wants[1][5]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(x).copy()).cuda() for x in texts]
    torch.cuda.synchronize()
    verb = dict(what="match", keep_unkeyed=True, max_distinct=4096)

    def check(got, w):
        assert tuple(x.item() for x in got[:6]) == w[:5] + (len(w[5]),)
        assert got[6][:len(w[5])].cpu().numpy().tobytes() == w[5]

    outs = []
    for st, exe, d, w in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.dedup_text(exe, d, out_cap=len(w[5]), **verb))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        check(got, w)
    errors = []

    def work(exe, x, d, st, w):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.dedup_text(exe, d, out_cap=len(w[5]), **verb)
                    st.synchronize()
                check(got, w)
                assert one_amd.dedup_text(exe, x, **verb) == w
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


# 12 composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["num3", "err"])
def test_dedup_text_composes_with_fields_text(name):
    text = _matrix_text(name)
    exe = one_amd.Executable(load_dfa(name))
    for k in (1, 2):
        # field k of the lines that have one (k = 2: the lines with a separator), then whole lines
        cut = one_amd.fields_text(exe, text, str(k), only_delimited=k > 1)
        whole = one_amd.dedup_text(exe, cut[3])
        field = one_amd.dedup_text(exe, text, what="field", key_index=k)
        assert whole[4] == field[4] > 1 and whole[2] == field[2] and whole[1] == field[1]
    m = one_amd.dedup_text(exe, text, what="match")
    u = one_amd.uniq_text(exe, text, max_per_line=1)
    assert (m[1], m[2]) == (u[1], len(u[3]))
    # dedup_text | tally_text: the output is a raw text
    assert one_amd.tally_text(exe, m[5], matches=False)[0] == m[4]


# 13 the C++ mirror --------------------------------------------------------------------------------
def test_dedup_text_cpp_mirror(tmp_path):
    """redgpu::dedupText (include/redgpu.hpp) compiled with g++"""
    prog = str(tmp_path / "dedup_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "dedup_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(ROOT, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "one_amd")], check=True)
    name, text = "num3", _matrix_text("num3")
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(ROOT, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), "2", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    t = _t(name, text)
    wants = [("whole", DR.dedup(t)),
             ("lines", DR.dedup(t, "lines", min_count=1, max_count=1, keep_unkeyed=True)),
             ("match", DR.dedup(t, "match", 2)),
             ("field", DR.dedup(t, "field", 2, invert=True))]
    assert run.stdout.split("\n")[:-1] == [
        "%s %d %d %d %d %d %d" % ((what,) + w[:5] + (len(w[5]),)) for what, w in wants]
    for what, w in wants:
        with open(prefix + "." + what, "rb") as f:
            assert f.read() == w[5], what


# 14 the fuzz --------------------------------------------------------------------------------------
def test_dedup_text_fuzz_smoke():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), FUZZ_CASES,
                          FUZZ_SEED, "keys"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "fuzz ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert KERNEL in out.stdout
