"""extract_text (redgpu_extract_text[_dev]): grep -o's output as a text - every match of every line
of a raw text as bytes, each followed by the delimiter, in text order.  The three counts and every
output byte are exact against sampleLines' loop (oracle.split_lines_loop), the CPU oracle's collect
per line for where a piece ENDS (test_gpu_collect_text._want) and the oracle's own replace for how
LONG it is - L(m) = len(replace<styLast,false>(line, "", m)), piece m has L(m - 1) - L(m) bytes -
with the reference's replace on a sample of lines when it is built: the nine DFAs over a dense text
(the issue's table asserted on the oracle's side first), max_per_line, every table placement, the
chunk-border shapes, rounds of 64 lines with uneven counts, truncation at every kind of out_cap with
sentinels on both sides, the device form at odd pointer offsets of the text and of the output,
identities with collect_text and replace_text on the GPU, other delimiters, a text of more chunks
than the grid has waves, concurrent streams and threads, and the C++ mirror."""
import ctypes as C
import os
import subprocess
import threading
import zlib

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from golden_util import load_dfa

import test_gpu_collect_text as CT
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

CHUNK = 16384
SENT = 0x55
ALL = 1 << 62
KERNEL = "k_extract_text"

_pieces = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _lacking(text, delim):
    """a byte the text does not hold (and that is not the delimiter), or None"""
    seen = np.bincount(_u8(text), minlength=256) if len(text) else np.zeros(256, dtype=np.int64)
    for b in range(1, 256):
        if not seen[b] and b != delim:
            return bytes([b])
    return None


def _by_lengths(rep, line, ends):
    """the pieces of one line from the lengths of replace(line, "", m): needs no marker byte"""
    out, before = [], len(line)
    for m, e in enumerate(ends, 1):
        k, rest = rep.replace(line, b"", "last", False, m)
        assert k == m, (k, m)
        size = before - len(rest)
        assert 0 < size <= e, (size, e)
        out.append(line[e - size:e])
        before = len(rest)
    return out


def _by_marker(rep, line, ends, mark):
    """the pieces of one line from ONE replace with a byte the line lacks: what stands between the
    marks is what no piece covers, so piece j begins behind gap j, which begins at e_(j-1)"""
    k, rest = rep.replace(line, mark, "last", False)
    gaps = rest.split(mark)
    assert k == len(ends) and len(gaps) == k + 1, (k, len(ends), len(gaps))
    out, at = [], 0
    for gap, e in zip(gaps, ends):
        a = at + len(gap)
        assert line[at:a] == gap and a < e, (at, a, e)
        out.append(line[a:e])
        at = e
    assert line[at:] == gaps[-1]
    return out


class _Pieces:
    """the oracle's answer for (DFA, text, delimiter): the pieces of every line, in order"""

    def __init__(self, name, text, delim, marker):
        self.want = w = CT._want(name, text, delim)
        cpu = CT._oracles[name]
        lines = O.split_lines_loop(text, delim)
        self.n_lines = w.n_lines
        self.delim = bytes([delim])
        mark = _lacking(text, delim) if marker else None
        self.marked = mark is not None
        ends = (w.end - w.begin).astype(np.int64)
        starts = (w.start - w.begin).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(w.counts)]).astype(np.int64)
        ref = O.Reference(CT._blob(name)) if O.have_ref() else None
        self.per_line = [[] for _ in lines]
        self.loose = 0                     # pieces that begin in front of the record's start
        hit = np.flatnonzero(w.counts > 0)
        for n, k in enumerate(hit):
            e = [int(v) for v in ends[first[k]:first[k + 1]]]
            line = lines[k]
            if len(e) <= 64 or mark is None:
                got = _by_lengths(cpu, line, e)
                if mark is not None:
                    assert got == _by_marker(cpu, line, e, mark), (name, k)
            else:
                # thousands of pieces in one line: the marker's answer, the lengths' at both ends
                got = _by_marker(cpu, line, e, mark)
                assert _by_lengths(cpu, line, e[:3]) == got[:3], (name, k)
                total, rest = cpu.replace(line, b"", "last", False)
                assert total == len(e) and len(line) - len(rest) == sum(len(p) for p in got)
            if ref is not None and n % 5 == 0:
                if len(e) <= 64:
                    assert _by_lengths(ref, line, e) == got, (name, k)
                elif mark is not None:
                    assert _by_marker(ref, line, e, mark) == got, (name, k)
            for p, en, st in zip(got, e, starts[first[k]:first[k + 1]]):
                assert p and self.delim not in p and en - len(p) <= st, (name, k)
                self.loose += en - len(p) != st
            self.per_line[k] = got

    def out(self, m=ALL):
        """(n_matches, the output) under max_per_line = m"""
        kept = [p for got in self.per_line for p in got[:m]]
        return len(kept), b"".join(p + self.delim for p in kept)

    def all(self):
        return [p for got in self.per_line for p in got]


def _oracle(name, text, delim=0x0A, marker=True):
    key = (name, text, delim, marker)
    if key not in _pieces:
        _pieces[key] = _Pieces(name, text, delim, marker)
    return _pieces[key]


def _same(exe, text, x, m=ALL, delim=b"\n", where=None):
    n, out = x.out(m)
    got = one_amd.extract_text(exe, text, max_per_line=m, delim=delim)
    assert one_amd.last_kernel() == KERNEL
    assert got[:2] == (x.n_lines, n), (where, got[:2], x.n_lines, n)
    assert len(got[2]) == len(out), (where, len(got[2]), len(out))
    assert got[2] == out, where
    return got


# the issue's table of the dense text: pieces, out_len, crc32(out), the shortest and the longest
# piece, pieces of >= 16 and of >= 64 bytes, pieces that begin in front of collect's start
TABLE = {
    "err": (1865, 11190, 0xec18365a, 5, 5, 0, 0, 0),
    "aab": (2257, 9028, 0x0fe5cf70, 3, 3, 0, 0, 0),
    "ale": (2055, 10358, 0xe3a90277, 3, 6, 0, 0, 0),
    "log100": (741, 15561, 0xd0405b22, 20, 20, 741, 0, 0),
    "num3": (10014, 31194, 0x7e95cff2, 1, 10, 0, 0, 0),
    "set5": (10759, 22803, 0xa6deac0a, 1, 7, 0, 0, 0),
    "dotstar_err": (210, 21330, 0x1ceaa1fc, 6, 198, 197, 152, 210),
    "newyork": (209, 21065, 0x71198279, 9, 189, 192, 148, 209),
    "uri": (163, 18024, 0x6078c41a, 51, 189, 163, 116, 161),
}


@pytest.mark.parametrize("name", CT.NINE)
def test_extract_text_matrix_vs_oracle(name):
    import torch
    text = CT._dense(CT.PIECES[name]())
    x = _oracle(name, text)
    # the oracle's side of the table, before any GPU call; both ways to the pieces were taken
    assert x.marked and x.n_lines == 648
    n, out = x.out()
    sizes = [len(p) for p in x.all()]
    assert (n, len(out), zlib.crc32(out), min(sizes), max(sizes), sum(s >= 16 for s in sizes),
            sum(s >= 64 for s in sizes), x.loose) == TABLE[name]
    assert n == x.want.n and len(out) == sum(sizes) + n
    exe = one_amd.Executable(load_dfa(name))
    _same(exe, text, x, where=name)
    # collect_text on the GPU: as many lines as records, every piece ends where its record does
    rec = one_amd.collect_text(exe, text)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    got = one_amd.extract_text(exe, dev, out_cap=len(out) + 3)
    torch.cuda.synchronize()
    assert [v.item() for v in got[:3]] == [x.n_lines, n, len(out)]
    mine = got[3][:len(out)].cpu().numpy().tobytes()
    assert mine == out
    offs, n_out = one_amd.split_lines(exe, mine)
    assert n_out == n == rec[1]
    parts = mine.split(b"\n")[:-1]
    assert all(text[int(e) - len(p):int(e)] == p for p, e in zip(parts, rec[6]))
    if name in CT.OPEN:
        assert mine == b"".join(text[int(s):int(e)] + b"\n" for s, e in zip(rec[5], rec[6]))
    else:
        assert mine != b"".join(text[int(s):int(e)] + b"\n" for s, e in zip(rec[5], rec[6]))


@pytest.mark.parametrize("name", ["num3", "aab", "dotstar_err"])
def test_extract_text_max_per_line(name):
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    x = _oracle(name, text)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    seen = set()
    for m in (0, 1, 2, 5, ALL):
        n, out = x.out(m)
        seen.add(n)
        got = _same(exe, text, x, m=m, where=(name, m))
        if m == 0:
            assert got == (x.n_lines, 0, b"")
        if m == 1:
            assert n == int((x.want.counts > 0).sum())
        sizes = one_amd.extract_text(exe, dev, max_per_line=m, out_cap=0)     # the counts alone
        torch.cuda.synchronize()
        assert [v.item() for v in sizes[:3]] == [x.n_lines, n, len(out)], (name, m)
        assert sizes[3].numel() == 0
    assert len(seen) == (5 if name in CT.OPEN else 2), (name, seen)


@pytest.mark.parametrize("dfa,opts,info", LP.ROWS + CT._MORE_ROWS)
def test_extract_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
    facts = one_amd.Executable(blob, device="none").info
    for k, v in LP.FACTS.get(dfa, {}).items():
        assert facts[k] == v, (dfa, k, facts[k], v)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    if dfa in LP.PIECES:
        text = CT._dense(LP.PIECES[dfa][0])
    else:
        text = CT._random_text("leaky" if dfa == "leaky" else "random")
    x = _oracle(dfa, text, marker=False)       # the lengths alone: random bytes leave no marker
    want = x.want
    # not vacuous: hit lines in every chunk, and lines without a match among them (the hit bitmap
    # is not the delimiter bitmap)
    assert want.n >= 50 and (want.counts == 0).sum() >= 5, (dfa, want.n)
    hit_begins = want.begins[want.counts > 0]
    assert len(set((hit_begins // CHUNK).tolist())) >= 4, dfa
    _same(exe, text, x, where=(dfa, opts))
    _same(exe, text, x, m=1, where=(dfa, opts, 1))


UNEVEN = b"".join(b"aab " * (i % 10) + b"\n" for i in range(300))


@pytest.mark.parametrize("shape", list(CT._shapes()) + ["uneven rounds"])
def test_extract_text_shapes(shape):
    """test_gpu_collect_text's shapes, and its uneven rounds: one chunk, 300 lines (five rounds of
    64), line i with i % 10 matches - the prefix inside a round and the carry between rounds
    differ from lane to lane"""
    text = UNEVEN if shape == "uneven rounds" else CT._shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        x = _oracle(name, text)
        n, out = x.out()
        if shape in ("no delimiter", "empty", "one byte, no delimiter"):
            assert (x.n_lines, n, out) == (0, 0, b"")
        elif shape == "one byte, a delimiter":
            assert (x.n_lines, n, out) == (1, 0, b"")
        elif shape == "a match in the tail":
            assert n == 3 * _oracle(name, CT.SHORT).out()[0] > 0  # the tail's matches are in no line
        elif shape == "one 40 KiB line":
            assert max(len(p) for p in x.per_line) >= 5120, name
        elif shape == "uneven rounds":
            assert len(text) < CHUNK
            if name == "aab":
                assert [len(p) for p in x.per_line] == [i % 10 for i in range(300)]
        else:
            assert n > 1000, (shape, name, n)
        _same(exe, text, x, where=(shape, name))
        _same(exe, text, x, m=2, where=(shape, name, 2))


def _raw_host(exe, text, out_cap, room, m=ALL, nl=True, nm=True, out=True, front=16):
    """redgpu_extract_text through ctypes: `room` bytes in the middle of a sentinel-filled buffer"""
    lib = _lib.lib()
    buf = np.full(front + room + 32, SENT, dtype=np.uint8)
    c = [C.c_uint64(SENT) for _ in range(3)]
    rc = lib.redgpu_extract_text(exe._h, text, len(text), 0x0A, m, C.byref(c[0]) if nl else None,
                                 C.byref(c[1]) if nm else None, C.byref(c[2]),
                                 buf.ctypes.data + front if out else None, out_cap)
    assert rc == 0, lib.redgpu_last_error()
    return [x.value for x in c], buf


def _raw_dev(exe, dev, out_cap, room, m=ALL, out_shift=16, have=(True, True)):
    """redgpu_extract_text_dev: a sentinel-filled tensor, `room` bytes of it from out_shift on
    handed over; everything on the device.  Returns the counts and the WHOLE tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((out_shift + room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    cnt = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    ptr = [cnt.data_ptr() + 8 * k if k == 2 or have[k] else None for k in range(3)]
    rc = lib.redgpu_extract_text_dev(exe._h, dev.data_ptr() if dev.numel() else None, dev.numel(),
                                     0x0A, m, *ptr, buf.data_ptr() + out_shift, out_cap,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return cnt.tolist(), buf.cpu().numpy()


def _prefix_and_sentinels(buf, want, out_cap, where, shift=16):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


@pytest.mark.parametrize("name", ["num3", "dotstar_err"])
def test_extract_text_truncation(name):
    """out is the middle of a larger buffer: exactly the first min(out_len, out_cap) bytes are
    written, the cut inside a lane's window (num3) or inside a piece the wave copies (dotstar_err)"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    x = _oracle(name, text)
    n_pieces, out = x.out()
    n = len(out)
    # a piece of a later chunk - of 64 bytes or more where there are such - and where it stands
    parts = x.all()
    at = np.concatenate([[0], np.cumsum([len(p) + 1 for p in parts])])
    later = int(np.searchsorted(x.want.begin, 2 * CHUNK))
    big = [j for j in range(later, len(parts)) if len(parts[j]) >= (64 if name == "dotstar_err" else 5)]
    j = big[0]
    first, size = int(at[j]), len(parts[j])
    assert out[first:first + size] == parts[j] and out[first + size] == 0x0A and first > 4096
    caps = [1, first, first + 1, first + size // 2, first + size - 1, first + size, first + size + 1,
            15, 16, 17, 4095, 4096, 4097, n - 1, n, n + 7]
    assert len(set(caps)) == len(caps) and max(caps[:-1]) <= n
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    counts = [x.n_lines, n_pieces, n]
    for cap in caps:
        got, buf = _raw_host(exe, text, cap, n + 7)
        assert got == counts, (cap, got)
        _prefix_and_sentinels(buf, out, cap, ("host", cap))
        got, buf = _raw_dev(exe, dev, cap, n + 7)
        assert got == counts, (cap, got)
        _prefix_and_sentinels(buf, out, cap, ("dev", cap))
    # out == NULL and out_cap == 0: the sizes only; n_lines and n_matches NULL each on its own
    got, buf = _raw_host(exe, text, n, n, out=False)
    assert got == counts and (buf == SENT).all()
    got, buf = _raw_host(exe, text, 0, n)
    assert got == counts and (buf == SENT).all()
    for nl in (True, False):
        for nm in (True, False):
            want = [v if on else SENT for v, on in zip(counts, (nl, nm, True))]
            got, buf = _raw_host(exe, text, n, n, nl=nl, nm=nm)
            assert got == want, (nl, nm, got)
            _prefix_and_sentinels(buf, out, n, (nl, nm))
            got, buf = _raw_dev(exe, dev, n, n, have=(nl, nm))
            assert got == want, (nl, nm, got)
            _prefix_and_sentinels(buf, out, n, (nl, nm))


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("name", ["num3", "uri"])
def test_extract_text_device_form(name, shift):
    """everything device-resident: the text at any offset from a 16-byte boundary, and -
    independently - the output (the window's blocks are those of the real address)"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    x = _oracle(name, text)
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(_u8(text).copy()))
    aligned = dev.clone()
    assert dev.data_ptr() % 16 == shift and aligned.data_ptr() % 16 == 0
    for m in (ALL, 2):
        n_pieces, out = x.out(m)
        n = len(out)
        counts = [x.n_lines, n_pieces, n]
        for cap in (n, n // 3):
            got, res = _raw_dev(exe, dev, cap, n, m=m)
            assert one_amd.last_kernel() == KERNEL
            assert got == counts
            _prefix_and_sentinels(res, out, cap, (name, "text", shift, m, cap))
            got, res = _raw_dev(exe, aligned, cap, n, m=m, out_shift=16 + shift)
            assert got == counts
            _prefix_and_sentinels(res, out, cap, (name, "out", shift, m, cap), shift=16 + shift)
    # the verb: the counts come back as tensors
    n_pieces, out = x.out()
    got = one_amd.extract_text(exe, dev, out_cap=len(out) + 3)
    torch.cuda.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got)
    assert all(v.shape == (1,) and v.dtype == torch.int64 for v in got[:3])
    assert [v.item() for v in got[:3]] == [x.n_lines, n_pieces, len(out)]
    assert got[3][:len(out)].cpu().numpy().tobytes() == out
    mine = torch.full((len(out) + 5,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.extract_text(exe, dev, out=mine)
    assert got[3] is mine and got[2].item() == len(out)
    assert mine.cpu().numpy().tobytes() == out + bytes([SENT]) * 5
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.extract_text(exe, dev)                                     # needs out or out_cap


def test_extract_text_empty_and_lineless_on_the_device():
    """the _dev form writes the three zero counts on the stream, and nothing else"""
    import torch
    exe = one_amd.Executable(load_dfa("aab"))
    for text in (b"", b"aab, and no line end"):
        dev = torch.from_numpy(_u8(text).copy()).cuda()
        got, buf = _raw_dev(exe, dev, 8, 8)
        assert got == [0, 0, 0] and (buf == SENT).all()
        assert one_amd.extract_text(exe, text) == (0, 0, b"")


@pytest.mark.parametrize("name", ["aab", "num3", "uri"])
def test_extract_text_identities(name):
    """beside the oracle, on the GPU: what replace_text removes is what extract_text emits; the
    output of an open DFA, fed back on the device, comes back unchanged - each piece is one whole
    match of its own line"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    lined = text[:text.rindex(b"\n") + 1]
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    got = one_amd.extract_text(exe, dev, out_cap=len(text))
    torch.cuda.synchronize()
    n_lines, n, out_len = (v.item() for v in got[:3])
    assert n > 100 and out_len <= len(text)
    rest = one_amd.replace_text(exe, lined, b"", one_amd.styLast, False)
    assert rest[0] == n_lines and rest[1] == n
    assert len(rest[2]) + out_len - n == len(lined)
    if name in CT.OPEN:
        mine = got[3][:out_len]
        back = one_amd.extract_text(exe, mine, out_cap=out_len + 1)
        torch.cuda.synchronize()
        assert [v.item() for v in back[:3]] == [n, n, out_len]
        assert torch.equal(back[3][:out_len], mine)


@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_extract_text_other_delimiter(delim):
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]()).replace(b"\n", delim)
    x = _oracle(name, text, delim[0])
    n, out = x.out()
    assert x.n_lines >= 648 and n > 1000 and out.count(delim) == n and b"\n" not in out
    _same(exe, text, x, delim=delim)
    # ... and with '\n' the same text has no line at all
    assert one_amd.extract_text(exe, text) == (0, 0, b"")


def test_extract_text_above_the_grid():
    """160 MiB = 10,240 chunks.  k_xt_size runs at most CUs x 2 workgroups of 16 waves (err's table
    is 20 KB: two workgroups per CU) - 8,192 waves on 256 CUs - and k_xt_write CUs x 2 of 8 waves:
    every wave of both passes takes a second chunk.  Everything stays on the device: a 1 MiB block
    that ends in a delimiter, tiled; the expected output is the block's, tiled."""
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 16
    block = CT._dense(CT.PIECES[name](), seed=3, n=block_len, end_in_delim=True)
    assert block[-1] == 0x0A
    x = _oracle(name, block)
    n, out = x.out()
    assert n > 10000 and (x.want.counts >= 2).sum() > 1000
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    got = one_amd.extract_text(exe, dev, out_cap=len(out) * tiles + 16)
    assert one_amd.last_kernel() == KERNEL
    assert [v.item() for v in got[:3]] == [x.n_lines * tiles, n * tiles, len(out) * tiles]
    exp = torch.from_numpy(_u8(out).copy()).cuda().repeat(tiles)
    assert torch.equal(got[3][:len(out) * tiles], exp)


def test_extract_text_two_streams_and_threads():
    import torch
    names = ("num3", "uri")
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [CT._dense(CT.PIECES[n](), seed=2 + k) for k, n in enumerate(names)]
    wants = [_oracle(n, t) for n, t in zip(names, texts)]
    outs = [w.out() for w in wants]
    assert len(outs[0][1]) != len(outs[1][1])
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def check(got, w, o):
        assert [v.item() for v in got[:3]] == [w.n_lines, o[0], len(o[1])]
        assert got[3][:len(o[1])].cpu().numpy().tobytes() == o[1]

    first = []
    for st, exe, d, o in zip(streams, exes, devs, outs):
        with torch.cuda.stream(st):
            first.append(one_amd.extract_text(exe, d, out_cap=len(o[1]) + 3))
    torch.cuda.synchronize()
    for got, w, o in zip(first, wants, outs):
        check(got, w, o)
    errors = []

    def work(exe, t, d, st, w, o):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.extract_text(exe, d, out_cap=len(o[1]) + 3)
                    st.synchronize()
                    check(got, w, o)
                assert one_amd.extract_text(exe, t) == (w.n_lines, o[0], o[1])
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants, outs)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_extract_text_cpp_mirror(tmp_path):
    """redgpu::extractText (include/redgpu.hpp) compiled with g++, run with a blob and a text"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "extract_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "extract_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "num3"
    text = CT._dense(CT.PIECES[name]())
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    x = _oracle(name, text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), "2", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = run.stdout.split("\n")
    for row, tag, m in zip(rows, ("all", "some"), (ALL, 2)):
        n, out = x.out(m)
        assert row == "%s %d %d" % (tag, n, x.n_lines), rows[:2]
        with open(prefix + "." + tag, "rb") as f:
            assert f.read() == out, tag
