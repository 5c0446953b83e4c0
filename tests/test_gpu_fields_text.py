"""fields_text (redgpu_fields_text[_dev]): awk -F's columns of a raw text - of every line the
selected fields that exist, joined by sep, then the delimiter.  The four counts and every output
byte are exact against sampleLines' loop (oracle.split_lines_loop) and the CPU oracle's replace per
line: replace<styLast,false>(line, MARK, S) split at MARK - a byte no text here holds - IS the
field list; selection and joining are plain Python.  The reference's replace checks every fifth
line when it is built.  Three crafted separator DFAs ([ \\t]+, a comma, a comma and blanks) and four
of the fixtures; the matrix of selections x max_fields x only_delimited, the field index at bit 63,
the early exit, the line shapes, chunk and round borders, the wave hand-off in every position of a
line, sep of every length, other delimiters, truncation at every kind of out_cap with sentinels on
both sides, the device form at odd pointer offsets, streams and threads, every table placement,
fields -> uniq on the device, and the C++ mirror."""
import collections
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from one_amd import workloads as W
from one_amd.matcher import fields_mask
from golden_util import literal_dfa
from oracle.reda_writer import write_reda

import test_gpu_collect_text as CT
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

CHUNK = 16384
SENT = 0x55
MARK = b"\x01"
KERNEL = "k_fields_text"
UNBOUNDED = 1 << 62


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _classes(groups):
    equiv = np.zeros(256, dtype=np.uint8)
    for k, chars in enumerate(groups, 1):
        for ch in chars:
            equiv[ch] = k
    return equiv


def _ws_dfa():
    """[ \\t]+ : 0 = error, 1 = initial, 2 = accepting and looping on blanks"""
    trans = np.zeros((3, 2), dtype=np.int64)
    trans[1, 1] = trans[2, 1] = 2
    return write_reda(trans, [0, 0, 1], equiv=_classes([b" \t"]), initial=1)


def _comma_blanks_dfa():
    """, * : 0 = error, 1 = initial, 2 = accepting behind the comma and looping on blanks"""
    trans = np.zeros((3, 3), dtype=np.int64)
    trans[1, 1] = 2
    trans[2, 2] = 2
    return write_reda(trans, [0, 0, 1], equiv=_classes([b",", b" "]), initial=1)


CRAFTED = {"ws": _ws_dfa, "comma": lambda: literal_dfa(b","), "comma_blanks": _comma_blanks_dfa}
PLANTS = {"ws": [b" ", b"\t", b"  ", b" \t ", b"      "], "comma": [b",", b",", b",,", b","],
          "comma_blanks": [b",", b", ", b",   ", b",,", b", , "]}
FIXTURES = ["num3", "set5", "log100", "uri"]
SEVEN = list(CRAFTED) + FIXTURES
SELECTIONS = ["1", "2", "1,3", "2-", "1-", "63,64-"]

_blobs, _texts, _fields = {}, {}, {}


def _blob(name):
    if name not in _blobs:
        _blobs[name] = CRAFTED[name]() if name in CRAFTED else CT._blob(name)
    return _blobs[name]


def _planted(name, seed=1, n=CT.N, end_in_delim=False, every=11):
    """the alphabet (no blank, comma or line end in it) under test_gpu_grep_text's delimiters, with
    the DFA's separators planted every 1..2 * every bytes: leading, trailing and adjacent ones
    happen, as do lines without any and empty lines"""
    key = (name, seed, n, end_in_delim, every)
    if key not in _texts:
        a = W.alphabet_bytes(n, seed).copy()
        for ch in b" \t,\n":
            a[a == ch] = 0x78
        rng = np.random.default_rng(seed + 7)
        plants = PLANTS[name]
        at = int(rng.integers(0, 2 * every))
        while at < n - 8:
            p = _u8(plants[int(rng.integers(0, len(plants)))])
            a[at:at + len(p)] = p
            at += len(p) + int(rng.integers(0, 2 * every))
        ends = CT._delims(n, seed)
        if end_in_delim and ends[-1] != n - 1:
            ends.append(n - 1)
        a[ends] = 0x0A
        _texts[key] = bytes(a)
    return _texts[key]


def _dense(name, **kw):
    """one dense text per DFA, without MARK"""
    if name in CRAFTED:
        return _planted(name, **kw)
    return CT._dense(CT.PIECES[name](), **kw)


class _Fields:
    """the oracle's answer for (DFA, text, delimiter): every line's field list, per S"""

    def __init__(self, name, text, delim):
        assert MARK not in text and delim != MARK[0]
        self.cpu = O.CpuOracle(_blob(name))
        self.ref = O.Reference(_blob(name)) if O.have_ref() else None
        self.lines = O.split_lines_loop(text, delim)
        self.n_lines = len(self.lines)
        self.delim = bytes([delim])
        self._per = {}

    def per_line(self, max_fields=0):
        most = max_fields - 1 if max_fields else UNBOUNDED
        if most not in self._per:
            per = []
            for k, line in enumerate(self.lines):
                cnt, rest = self.cpu.replace(line, MARK, "last", False, most)
                got = rest.split(MARK)
                assert len(got) == cnt + 1 and cnt <= most
                if self.ref is not None and k % 5 == 0:
                    assert self.ref.replace(line, MARK, "last", False, most) == (cnt, rest), k
                per.append(got)
            self._per[most] = per
        return self._per[most]

    def out(self, fields, max_fields=0, only=False, sep=b" "):
        """(n_lines, n_emitted, n_fields, the output): selection and joining in plain Python"""
        mask = fields_mask(fields)
        emitted, written, rows = 0, 0, []
        for got in self.per_line(max_fields):
            if only and len(got) == 1:
                continue
            keep = [f for j, f in enumerate(got, 1) if (mask >> (min(j, 64) - 1)) & 1]
            emitted += 1
            written += len(keep)
            rows.append(sep.join(keep) + self.delim)
        return self.n_lines, emitted, written, b"".join(rows)


def _oracle(name, text, delim=0x0A):
    key = (name, text, delim)
    if key not in _fields:
        _fields[key] = _Fields(name, text, delim)
    return _fields[key]


def _same(exe, text, x, fields, max_fields=0, only=False, sep=b" ", delim=b"\n", where=None):
    want = x.out(fields, max_fields, only, sep)
    got = one_amd.fields_text(exe, text, fields, sep=sep, max_fields=max_fields,
                              only_delimited=only, delim=delim)
    assert one_amd.last_kernel() == KERNEL
    assert got[:3] == want[:3], (where, got[:3], want[:3])
    assert len(got[3]) == len(want[3]), (where, len(got[3]), len(want[3]))
    assert got[3] == want[3], where
    return got


def test_fields_text_issue_table_on_the_oracle():
    """the field lists the issue states, on the CPU oracle's side"""
    for line, name, most, want in [
            (b"  a b ", "ws", UNBOUNDED, [b"", b"a", b"b", b""]),
            (b"a,b,,c,", "comma", 1, [b"a", b"b,,c,"]),
            (b"", "ws", UNBOUNDED, [b""]), (b"", "comma", 0, [b""]), (b"", "num3", 3, [b""]),
            (b" ", "ws", UNBOUNDED, [b"", b""]),
            (b"x12y3456z", "num3", UNBOUNDED, [b"x", b"y", b"z"])]:
        cpu = O.CpuOracle(_blob(name))
        assert cpu.replace(line, MARK, "last", False, most)[1].split(MARK) == want, (line, name)


@pytest.mark.parametrize("name", SEVEN)
def test_fields_text_matrix_vs_oracle(name):
    exe = one_amd.Executable(_blob(name))
    text = _dense(name, end_in_delim=True)
    assert text[-1] == 0x0A
    x = _oracle(name, text)
    counts = [len(got) for got in x.per_line()]
    # not vacuous: lines without a separator, lines of many fields, empty fields
    # (uri is suffix-closed: a line has one separator at the most)
    many = 2 if name == "uri" else 4
    assert x.n_lines >= 600 and min(counts) == 1 and sum(c >= many for c in counts) >= 100, name
    assert sum(f == b"" for got in x.per_line() for f in got) >= (20 if name in CRAFTED else 1)
    if name == "uri":
        assert sum(len(l) - sum(map(len, got)) >= 64 for l, got in zip(x.lines, x.per_line())) > 50
    for fields in SELECTIONS:
        for max_fields in (0, 1, 2, 3):
            for only in (False, True):
                got = _same(exe, text, x, fields, max_fields, only, where=(name, fields, max_fields, only))
                if not only:
                    assert got[1] == x.n_lines
                if only and max_fields == 1:
                    assert got[1:] == (0, 0, b"")          # no line has a counted separator
    # identities beside the oracle: every field joined by sep is sed s/separator/sep/g ...
    for sep in (b" ", b"<->"):
        mine = one_amd.fields_text(exe, text, "1-", sep=sep)
        sed = one_amd.replace_text(exe, text, sep, one_amd.styLast, False)
        assert mine[3] == sed[2] and mine[0] == sed[0]
        assert mine[2] == sed[1] + x.n_lines
    # ... and one field a line is the text itself
    assert one_amd.fields_text(exe, text + b"a tail", "1", max_fields=1)[3] == text


FIELD_COUNTS = (62, 63, 64, 65, 130)


def test_fields_text_field_index_edges():
    """lines of 62 .. 130 fields: bit 62 is field 63 alone, bit 63 is field 64 and every later one"""
    name = "comma"
    exe = one_amd.Executable(_blob(name))
    text = b"".join(b",".join(b"f%d" % j for j in range(1, k + 1)) + b"\n" for k in FIELD_COUNTS) * 3
    x = _oracle(name, text)
    assert [len(g) for g in x.per_line()[:5]] == list(FIELD_COUNTS)
    for fields in ("63", "64-", "63,64-", "1,64-", "62"):
        for max_fields in (0, 63, 64, 65):
            got = _same(exe, text, x, fields, max_fields, sep=b"|", where=(fields, max_fields))
            if fields == "64-" and max_fields == 0:
                assert got[2] == 3 * (1 + 2 + 67)
                assert got[3].startswith(b"\n\nf64\nf64|f65\nf64|f65|f66|")
            if fields == "63" and max_fields == 63:
                assert got[3].startswith(b"\nf63\nf63,f64\nf63,f64,f65\n")


def test_fields_text_early_exit():
    """the chain is left behind the highest selected field: what follows holds separators (and
    fields) that are never looked at; counts and bytes say the same as the oracle, which walks
    every line to its end.  Under max_fields = 2 the last field is the REST of the line although
    the highest selected field is not below max_fields."""
    for name in ("comma", "ws", "num3"):
        exe = one_amd.Executable(_blob(name))
        text = _dense(name)
        x = _oracle(name, text)
        assert sum(len(g) >= 5 for g in x.per_line()) >= 100
        for fields in ("1", "1,2", "2", "3"):
            for max_fields in (0, 2):
                for only in (False, True):
                    got = _same(exe, text, x, fields, max_fields, only, where=(name, fields, max_fields))
                    assert got[2] <= len(fields.split(",")) * got[1]
    # spelled out on one line
    exe = one_amd.Executable(_blob("comma"))
    assert one_amd.fields_text(exe, b"a,b,c,d\n", "1,2", max_fields=2) == (1, 1, 2, b"a b,c,d\n")
    assert one_amd.fields_text(exe, b"a,b,c,d\n", "2", max_fields=2) == (1, 1, 1, b"b,c,d\n")
    assert one_amd.fields_text(exe, b"a,b,c,d\n", "1,2") == (1, 1, 2, b"a b\n")
    assert one_amd.fields_text(exe, b"a,b,c,d\n", "3", max_fields=2) == (1, 1, 0, b"\n")


SHAPES = {
    "empty lines": b"\n\n\na,b\n\n",
    "lines that are one separator": b",\n,\nx\n,\n",
    "separator first or last": b",a\na,\n,a,\n,\na\n",
    "two separators adjacent": b"a,,b\n,,\n,,c\nd,,\n",
    "no delimiter": b"a,b,c and no line end",
    "empty": b"",
    "a tail behind the last delimiter": b"a,b\nc,d\ne,f and a tail",
    "one byte, a delimiter": b"\n",
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fields_text_line_shapes(shape):
    text = SHAPES[shape]
    for name in ("comma", "comma_blanks"):
        exe = one_amd.Executable(_blob(name))
        x = _oracle(name, text)
        for fields in ("1", "2", "1,3", "2-", "1-"):
            for max_fields in (0, 2):
                for only in (False, True):
                    got = _same(exe, text, x, fields, max_fields, only, sep=b"+",
                                where=(shape, name, fields, max_fields, only))
                    if shape in ("no delimiter", "empty"):
                        assert got == (0, 0, 0, b"")
    exe = one_amd.Executable(_blob("comma"))
    if shape == "empty lines":
        assert one_amd.fields_text(exe, text, "1") == (5, 5, 5, b"\n\n\na\n\n")
        assert one_amd.fields_text(exe, text, "2") == (5, 5, 1, b"\n\n\nb\n\n")
        assert one_amd.fields_text(exe, text, "1", only_delimited=True) == (5, 1, 1, b"a\n")
    if shape == "two separators adjacent":
        assert one_amd.fields_text(exe, text, "1-", sep=b"+")[3] == b"a++b\n++\n++c\nd++\n"
    if shape == "a tail behind the last delimiter":
        assert one_amd.fields_text(exe, text, "2") == (2, 2, 2, b"b\nd\n")


@pytest.mark.parametrize("name", ["comma_blanks", "ws"])
def test_fields_text_lines_across_a_chunk_border(name):
    """a line of three fields and two separators of several bytes laid over byte 16384 at every
    offset of its 15 bytes (the delimiter included), short lines around it"""
    exe = one_amd.Executable(_blob(name))
    line = b"abc,  de, fgh\n" if name == "comma_blanks" else b"abc \t de  fgh\n"
    for shift in range(len(line) + 1):
        front = CHUNK - len(line) + shift
        body = (b"q,r s\n" * (front // 6 + 1))[-front:]
        text = body[:-1] + b"\n" + line + b"t,u v,w x\n" * 3
        assert text[front:front + len(line)] == line
        x = _oracle(name, text)
        for fields in ("1-", "2", "1,3"):
            _same(exe, text, x, fields, sep=b"--", where=(name, shift, fields))
        _same(exe, text, x, "2-", only=True, where=(name, shift))


@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_fields_text_rounds_of_64_lines(k):
    """the second chunk holds exactly k line ends: one round, one full round, a round and a line,
    two rounds and a line - the carry from round to round, and lanes without a line"""
    name = "comma"
    exe = one_amd.Executable(_blob(name))
    chunk0 = b"ab,cd,e\n" * (CHUNK // 8)
    rows = b"".join(b"%03d,y,%s\n" % (i, b"z" * (i % 3)) for i in range(k))
    rows = b"".join(r.ljust(7, b",")[:7] + b"\n" for r in rows.split(b"\n")[:-1])
    assert len(rows) == 8 * k
    over = b"w,v," * ((CHUNK - len(rows)) // 4 + 2) + b"\n"      # ends in the third chunk
    text = chunk0 + rows + over + b"a,b\n" * 5
    a = _u8(text)
    assert int((a[CHUNK:2 * CHUNK] == 0x0A).sum()) == k and len(chunk0) == CHUNK
    x = _oracle(name, text)
    for fields in ("1", "2,3", "1-"):
        for only in (False, True):
            _same(exe, text, x, fields, only=only, where=(k, fields, only))


def test_fields_text_above_the_grid():
    """160 MiB = 10,240 chunks, more than either pass has waves (at most CUs x 2 workgroups of 12
    and of 8): every wave takes a second chunk.  Everything stays on the device: a 1 MiB block
    that ends in a delimiter, tiled; the expected output is the block's, tiled."""
    import torch
    name = "comma_blanks"
    exe = one_amd.Executable(_blob(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 12
    block = _planted(name, seed=3, n=block_len, end_in_delim=True)
    x = _oracle(name, block)
    want = x.out("1,3", sep=b"\t")
    assert want[1] > 10000
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    got = one_amd.fields_text(exe, dev, "1,3", sep=b"\t", out_cap=len(want[3]) * tiles + 16)
    assert one_amd.last_kernel() == KERNEL
    assert [v.item() for v in got[:4]] == [v * tiles for v in want[:3]] + [len(want[3]) * tiles]
    exp = torch.from_numpy(_u8(want[3]).copy()).cuda().repeat(tiles)
    assert torch.equal(got[4][:len(want[3]) * tiles], exp)


HAND_SIZES = (63, 64, 65, 4097)


def test_fields_text_wave_hand_off():
    """fields of 63 (the window), 64, 65 and 4,097 bytes (the whole wave) in first, middle and LAST
    position of a line - the last is handed over from behind the chain - each beside lines of
    short fields in the neighbouring lanes"""
    for name, comma in (("comma", b","), ("comma_blanks", b",  ")):
        exe = one_amd.Executable(_blob(name))
        rows = []
        for size in HAND_SIZES:
            for pos in range(3):
                f = [b"s", b"tt", b"uuu"]
                f[pos] = bytes([0x41 + pos]) * size
                rows += [b"a,b,c", comma.join(f), b"d,e"]
        rows.append(b"L" * 200)                                        # one field, long, no separator
        text = b"\n".join(rows) + b"\n"
        x = _oracle(name, text)
        assert sorted({len(f) for g in x.per_line() for f in g if len(f) > 3}) == [63, 64, 65, 200, 4097]
        for fields in ("1-", "1", "2", "3", "1,3", "2-"):
            for max_fields in (0, 2):
                _same(exe, text, x, fields, max_fields, sep=b"; ", where=(name, fields, max_fields))
        _same(exe, text, x, "1-", only=True, sep=b"", where=name)


@pytest.mark.parametrize("sep", [b"", b"\t", b"<=>", b"12345678", b"\n", b"a\nb"])
def test_fields_text_sep(sep):
    """0, 1, 3 and 8 bytes; a sep that holds the delimiter byte is written as it is"""
    name = "ws"
    exe = one_amd.Executable(_blob(name))
    text = _dense(name)
    x = _oracle(name, text)
    for fields in ("1-", "1,3"):
        got = _same(exe, text, x, fields, sep=sep, where=(sep, fields))
        # a sep between every two fields written of a line, and nowhere else
        assert len(got[3]) == len(_same(exe, text, x, fields, sep=b"")[3]) + len(sep) * sum(
            max(0, len([f for j, f in enumerate(g, 1) if fields == "1-" or j in (1, 3)]) - 1)
            for g in x.per_line())
    if sep == b"\n":
        got = one_amd.fields_text(exe, text, "1-", sep=sep)
        assert got[3].count(b"\n") > got[1]
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, text, "1", sep=b"123456789")


@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_fields_text_other_delimiter(delim):
    name = "comma"
    exe = one_amd.Executable(_blob(name))
    text = _dense(name).replace(b"\n", delim)
    x = _oracle(name, text, delim[0])
    assert x.n_lines >= 600
    got = _same(exe, text, x, "2,3", delim=delim)
    assert b"\n" not in got[3] and got[3].count(delim) == got[1]
    _same(exe, text, x, "1-", only=True, delim=delim)
    # ... and with '\n' the same text has no line at all
    assert one_amd.fields_text(exe, text, "1") == (0, 0, 0, b"")


def _raw_host(exe, text, fields, sep, out_cap, room, have=(True, True, True), out=True, front=16):
    """redgpu_fields_text through ctypes: `room` bytes in the middle of a sentinel-filled buffer"""
    lib = _lib.lib()
    buf = np.full(front + room + 32, SENT, dtype=np.uint8)
    c = [C.c_uint64(SENT) for _ in range(4)]
    ptr = [C.byref(c[k]) if k == 3 or have[k] else None for k in range(4)]
    rc = lib.redgpu_fields_text(exe._h, text, len(text), 0x0A, fields_mask(fields), 0, 0,
                                int.from_bytes(sep, "little"), len(sep), *ptr,
                                buf.ctypes.data + front if out else None, out_cap)
    assert rc == 0, lib.redgpu_last_error()
    return [v.value for v in c], buf


def _raw_dev(exe, dev, fields, sep, out_cap, room, out_shift=16, have=(True, True, True),
             max_fields=0, only=0):
    """redgpu_fields_text_dev: a sentinel-filled tensor, `room` bytes of it from out_shift on
    handed over; everything on the device.  Returns the counts and the WHOLE tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((out_shift + room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    cnt = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    ptr = [cnt.data_ptr() + 8 * k if k == 3 or have[k] else None for k in range(4)]
    rc = lib.redgpu_fields_text_dev(exe._h, dev.data_ptr() if dev.numel() else None, dev.numel(),
                                    0x0A, fields_mask(fields), max_fields, only,
                                    int.from_bytes(sep, "little"), len(sep), *ptr,
                                    buf.data_ptr() + out_shift, out_cap,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return cnt.tolist(), buf.cpu().numpy()


def _prefix_and_sentinels(buf, want, out_cap, where, shift=16):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


@pytest.mark.parametrize("name", ["comma", "uri"])
def test_fields_text_truncation(name):
    """out is the middle of a larger buffer: exactly the first min(out_len, out_cap) bytes are
    written - the cut inside a field, inside sep, on the delimiter, at a 16-byte block edge, inside
    a field the wave copies (uri's lines have fields of hundreds of bytes)"""
    import torch
    exe = one_amd.Executable(_blob(name))
    text = _dense(name)
    x = _oracle(name, text)
    sep = b"\x02\x03\x04"
    assert not set(sep) & set(text)
    want = x.out("1-", sep=sep)
    out, n = want[3], len(want[3])
    counts = list(want[:3]) + [n]
    in_sep = out.index(sep, n // 2)
    on_delim = out.index(b"\n", n // 2)
    in_field = n // 3 + re.search(rb"[^\x02-\x04\n]{3}", out[n // 3:]).start() + 1
    caps = [0, 1, in_field, in_sep, in_sep + 1, in_sep + 2, in_sep + 3, on_delim, on_delim + 1,
            15, 16, 17, 4095, 4096, 4097, n - 1, n, n + 1]
    if name == "uri":
        big = re.search(rb"[^\x02-\x04\n]{100}", out[n // 2:]).start() + n // 2
        caps += [big + 1, big + 50, big + 99]
    assert max(caps) == n + 1
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    for cap in caps:
        got, buf = _raw_host(exe, text, "1-", sep, cap, n + 7)
        assert got == counts, (cap, got)
        _prefix_and_sentinels(buf, out, cap, ("host", cap))
        got, buf = _raw_dev(exe, dev, "1-", sep, cap, n + 7)
        assert got == counts, (cap, got)
        _prefix_and_sentinels(buf, out, cap, ("dev", cap))
    # out == NULL and out_cap == 0: the sizes only; the three other counts NULL each on its own
    got, buf = _raw_host(exe, text, "1-", sep, n, n, out=False)
    assert got == counts and (buf == SENT).all()
    for k in range(4):
        have = tuple(j != k for j in range(3))
        seen = [v if j == 3 or have[j] else SENT for j, v in enumerate(counts)]
        got, buf = _raw_host(exe, text, "1-", sep, n, n, have=have)
        assert got == seen, (have, got)
        _prefix_and_sentinels(buf, out, n, have)
        got, buf = _raw_dev(exe, dev, "1-", sep, n, n, have=have)
        assert got == seen, (have, got)
        _prefix_and_sentinels(buf, out, n, have)


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
def test_fields_text_device_form_at_odd_offsets(shift):
    """everything device-resident: the text at any offset from a 16-byte boundary, and -
    independently - the output (the window's blocks are those of the real address)"""
    import torch
    name = "uri" if shift % 4 == 3 else "comma_blanks"
    exe = one_amd.Executable(_blob(name))
    text = _dense(name)
    x = _oracle(name, text)
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(_u8(text).copy()))
    aligned = dev.clone()
    assert dev.data_ptr() % 16 == shift and aligned.data_ptr() % 16 == 0
    for fields, max_fields, only in (("1-", 0, 0), ("1,3", 3, 1)):
        want = x.out(fields, max_fields, bool(only), b", ")
        out, n = want[3], len(want[3])
        counts = list(want[:3]) + [n]
        for cap in (n, n // 3):
            got, res = _raw_dev(exe, dev, fields, b", ", cap, n, max_fields=max_fields, only=only)
            assert one_amd.last_kernel() == KERNEL
            assert got == counts
            _prefix_and_sentinels(res, out, cap, (name, "text", shift, fields, cap))
            got, res = _raw_dev(exe, aligned, fields, b", ", cap, n, out_shift=16 + shift,
                                max_fields=max_fields, only=only)
            assert got == counts
            _prefix_and_sentinels(res, out, cap, (name, "out", shift, fields, cap), shift=16 + shift)


def test_fields_text_device_form_counts_and_streams():
    """the counts come back as tensors; asynchronous on a stream that is not the default one"""
    import torch
    name = "ws"
    exe = one_amd.Executable(_blob(name))
    text = _dense(name)
    x = _oracle(name, text)
    want = x.out("2,4-", sep=b":")
    out = want[3]
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = one_amd.fields_text(exe, dev, "2,4-", sep=b":", out_cap=len(out) + 3)
        sizes = one_amd.fields_text(exe, dev, [2, 5], sep=b":", out_cap=0)
        mine = torch.full((len(out) + 5,), SENT, dtype=torch.uint8, device="cuda")
        into = one_amd.fields_text(exe, dev, "2,4-", sep=b":", out=mine)
    st.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got)
    assert all(v.shape == (1,) and v.dtype == torch.int64 for v in got[:4])
    assert [v.item() for v in got[:4]] == list(want[:3]) + [len(out)]
    assert got[4][:len(out)].cpu().numpy().tobytes() == out
    w25 = x.out([2, 5], sep=b":")
    assert [v.item() for v in sizes[:4]] == list(w25[:3]) + [len(w25[3])] and sizes[4].numel() == 0
    assert into[4] is mine and into[3].item() == len(out)
    assert mine.cpu().numpy().tobytes() == out + bytes([SENT]) * 5
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, dev, "1")                                # needs out or out_cap
    # an empty text and one without a line: the four zero counts on the stream, nothing else
    for t in (b"", b"a b and no line end"):
        d = torch.from_numpy(_u8(t).copy()).cuda()
        cnt, buf = _raw_dev(exe, d, "1", b" ", 8, 8)
        assert cnt == [0, 0, 0, 0] and (buf == SENT).all()


def test_fields_text_two_streams_and_threads():
    import torch
    names = ("ws", "uri")
    exes = [one_amd.Executable(_blob(n)) for n in names]
    texts = [_dense(n, seed=2 + k) for k, n in enumerate(names)]
    wants = [_oracle(n, t).out("1,3-", sep=b"/") for n, t in zip(names, texts)]
    assert len(wants[0][3]) != len(wants[1][3])
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def check(got, w):
        assert [v.item() for v in got[:4]] == list(w[:3]) + [len(w[3])]
        assert got[4][:len(w[3])].cpu().numpy().tobytes() == w[3]

    first = []
    for st, exe, d, w in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            first.append(one_amd.fields_text(exe, d, "1,3-", sep=b"/", out_cap=len(w[3]) + 3))
    torch.cuda.synchronize()
    for got, w in zip(first, wants):
        check(got, w)
    errors = []

    def work(exe, t, d, st, w):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.fields_text(exe, d, "1,3-", sep=b"/", out_cap=len(w[3]) + 3)
                    st.synchronize()
                    check(got, w)
                assert one_amd.fields_text(exe, t, "1,3-", sep=b"/") == w
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("dfa,opts,info", LP.ROWS)
def test_fields_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
    _blobs.setdefault(dfa, blob)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    if dfa in LP.PIECES:
        text = CT._dense(LP.PIECES[dfa][0])
    else:
        text = CT._random_text("leaky" if dfa == "leaky" else "random").replace(MARK, b"\x02")
    x = _oracle(dfa, text)
    counts = [len(g) for g in x.per_line()]
    assert sum(c >= 2 for c in counts) >= 50 and min(counts) == 1, (dfa, max(counts))
    _same(exe, text, x, "1,3", where=(dfa, opts))
    _same(exe, text, x, "2-", max_fields=3, only=True, sep=b"", where=(dfa, opts, "only"))


def test_fields_text_into_uniq_text():
    """cut -d, -f2 | sort | uniq -c without leaving the device: the second column's output is a raw
    text, uniq_text counts its lines by their bytes"""
    import torch
    rng = np.random.default_rng(5)
    rows = [b"id%d,k%d,%s" % (i, int(rng.integers(0, 37)), b"x" * int(rng.integers(0, 9)))
            for i in range(3000)]
    rows[10::50] = [b"no second field"] * len(rows[10::50])
    text = b"\n".join(rows) + b"\n"
    exe = one_amd.Executable(_blob("comma"))
    key = one_amd.Executable(literal_dfa(b"k"))
    x = _oracle("comma", text)
    want = collections.Counter(g[1] for g in x.per_line() if len(g) > 1)
    assert len(want) == 37 and sum(want.values()) == 3000 - 60
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    col = one_amd.fields_text(exe, dev, "2", out_cap=len(text))
    out_len = int(col[3].item())
    column = col[4][:out_len]
    got = one_amd.uniq_text(key, column, matches=False, max_distinct=64)
    torch.cuda.synchronize()
    n_distinct = int(got[3].item())
    assert int(got[0].item()) == 3000 and int(got[1].item()) == 3000 - 60 and int(got[2].item()) == 0
    data = column.cpu().numpy().tobytes()
    first, length, count = (v[:n_distinct].cpu().tolist() for v in got[4:7])
    assert {data[f:f + l]: c for f, l, c in zip(first, length, count)} == dict(want)


def test_fields_text_cpp_mirror(tmp_path):
    """redgpu::fieldsText (include/redgpu.hpp) compiled with g++, run with a blob and a text"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "fields_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "fields_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "num3"
    text = _dense(name)[:20000]
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    x = _oracle(name, text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), "%x" % fields_mask("1,3-"), "3", prefix],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = run.stdout.split("\n")
    for row, tag, want in zip(rows, ("all", "some"), (x.out("1,3-", sep=b", "),
                                                     x.out("1,3-", 3, True, b""))):
        assert row == "%s %d %d %d" % (tag, want[1], want[2], want[0]), rows[:2]
        with open(prefix + "." + tag, "rb") as f:
            assert f.read() == want[3], tag
