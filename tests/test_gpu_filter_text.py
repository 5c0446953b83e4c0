"""filter_text (redgpu_filter_text[_dev]): grep's output - the lines of a raw text that
search<style,doLeader> selects, the first max_count of them, with `before` lines in front of and
`after` lines behind each, as a text.  The four counts and the bytes are exact against sampleLines'
loop (oracle.split_lines_loop) plus the CPU oracle's search per line (test_gpu_grep_text._want; the
reference's too when it is built) and a dozen lines of numpy for the context rule: the seven DFAs
under every style, leader setting, invert and four contexts, every table placement, the shapes
(context across delimiter-less chunks, 2,731 runs in a chunk, contexts larger than the text),
truncation at every kind of out_cap with a sentinel behind it, optional outputs, the device form at
odd pointer offsets of the text and of the output, identities with grep_text on the GPU, a text of
more chunks than the grid has waves, concurrent streams and threads, and the C++ mirror."""
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
ALL = 1 << 62
CONTEXTS = [(0, 0), (2, 0), (0, 3), (1, 1)]
# which of the lines that cross no chunk border hold the piece: runs of five planted and of six
# bare lines (a gap between runs of emitted lines needs before + after + 1 lines in a row that are
# not selected - under invert: that are), lone ones, and pairs two and three apart (their contexts
# overlap)
PLANT = "PNNPNNPPPPPNNNNNNPNPNNPN"

_texts = {}
_expects = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _text(name, style, seed=1, n=4 * CHUNK + 5):
    """test_gpu_grep_text._standard's text - alphabet bytes, delimiters at pseudo-random gaps of
    1-199 bytes, the piece in the lines across an odd multiple of 16384 and never in those across an
    even one - with three changes: the other lines are planted by PLANT, a line ends at n - 2 (so
    that one crosses 4 * 16384: two planted and two bare lines on the borders), and under styFull
    the piece (without log100's trailing blank) stands at the END of its line, where
    search<styFull> accepts it."""
    piece = G.PIECES[name]()
    full = style == 5
    if full:
        piece = piece.rstrip()
    key = (piece, full, seed, n)
    if key in _texts:
        return _texts[key]
    a = W.alphabet_bytes(n, seed).copy()
    a[a == 0x0A] = 0x20
    rng = np.random.default_rng(seed)
    ends, pos = [], -1
    while True:
        pos += int(rng.integers(1, 200))
        if pos >= n - 2:
            break
        ends.append(pos)
    ends.append(n - 2)
    a[ends] = 0x0A
    begin, other = 0, 0
    p = _u8(piece)
    for e in ends:
        crossed = [m for m in range(CHUNK, n, CHUNK) if begin < m <= e]
        if crossed:
            plant = any((m // CHUNK) % 2 == 1 for m in crossed)
        else:
            plant = PLANT[other % len(PLANT)] == "P"
            other += 1
        if plant and e - begin >= len(p):
            at = e - len(p) if full else begin + (e - begin - len(p)) // 2
            a[at:at + len(p)] = p
        begin = e + 1
    _texts[key] = bytes(a)
    return _texts[key]


class _Expect:
    """the rule of include/redgpu.h on the oracle's per-line search: the first max_count selected
    line numbers, [j - before, j + after] clipped and marked, the marked lines' bytes joined"""

    def __init__(self, name, text, style, lead, invert, before, after, max_count, delim):
        w = G._want(name, text, style, lead, invert, delim, max_count)
        self.n_lines, self.n_selected = w[0], w[1]
        self.sel = [int(j) for j in w[2]]
        self.offs = [int(o) for o in G._lines_of(text, delim)]
        self.before, self.after = before, after
        emit = np.zeros(self.n_lines, dtype=bool)
        for j in self.sel:
            emit[max(0, j - before):min(self.n_lines - 1, j + after) + 1] = True
        self.emit = emit
        self.lines = np.flatnonzero(emit)
        self.n_emitted = len(self.lines)
        self.out = b"".join(text[self.offs[i]:self.offs[i + 1]] for i in self.lines)
        self.counts = [self.n_lines, self.n_selected, self.n_emitted, len(self.out)]


def _expect(name, text, style=4, lead=1, invert=False, before=0, after=0, max_count=ALL,
            delim=0x0A):
    key = (name, text, style, lead, bool(invert), before, after, max_count, delim)
    if key not in _expects:
        _expects[key] = _Expect(name, text, style, lead, invert, before, after, max_count, delim)
    return _expects[key]


def _crosses(x, begin, finish, n):
    return any(begin < m <= finish for m in range(CHUNK, n, CHUNK))


def _guards(x, text, where):
    """on the oracle's side, before any GPU call: the case cannot pass vacuously"""
    n = len(text)
    assert x.n_selected >= 100 and x.n_lines - x.n_selected >= 100, where + (x.n_selected,)
    crossing = [i for i in x.lines if _crosses(x, x.offs[i], x.offs[i + 1] - 1, n)]
    assert len(crossing) >= 2, where + (crossing,)
    # a context [j - before, j + after] that begins in one chunk and ends in a later one
    spans = [j for j in x.sel
             if x.offs[max(0, j - x.before)] // CHUNK <
             (x.offs[min(x.n_lines - 1, j + x.after) + 1] - 1) // CHUNK]
    assert spans, where
    if x.before or x.after:  # (the contexts of two lines overlap only when they have a width)
        assert any(a + x.after >= b - x.before for a, b in zip(x.sel, x.sel[1:])), where
    assert (np.diff(x.lines) > 1).any(), where


def _same(exe, text, x, style=4, lead=1, invert=False, delim=b"\n", max_count=ALL, where=None):
    got = one_amd.filter_text(exe, text, style, bool(lead), invert=invert, before=x.before,
                              after=x.after, max_count=max_count, delim=delim)
    assert one_amd.last_kernel() == "k_filter_text"
    assert list(got[:3]) == x.counts[:3], (where, got[:3], x.counts)
    assert len(got[3]) == len(x.out), (where, len(got[3]), len(x.out))
    assert got[3] == x.out, where


@pytest.mark.parametrize("style", G.STYLES)
@pytest.mark.parametrize("name", G.SEVEN)
def test_filter_text_matrix_vs_oracle(name, style):
    text = _text(name, style)
    assert len(text) == 4 * CHUNK + 5
    cases = []
    for lead in (0, 1):
        for invert in (False, True):
            for before, after in CONTEXTS:
                x = _expect(name, text, style, lead, invert, before, after)
                _guards(x, text, (name, style, lead, invert, before, after))
                cases.append((lead, invert, x))
    exe = one_amd.Executable(load_dfa(name))
    for lead, invert, x in cases:
        _same(exe, text, x, style, lead, invert, where=(name, style, lead, invert, x.before, x.after))


@pytest.mark.parametrize("dfa,opts,info", G._PLACEMENT_ROWS)
def test_filter_text_under_placement(dfa, opts, info):
    """only the select pass depends on the table's placement: one context, both inverts"""
    text = G._placement_text(dfa)
    cases = []
    for style in (1, 4):
        for lead in (0, 1):
            G._placement_guard(dfa, text, style, lead)
            for invert in (False, True):
                cases.append((style, lead, invert, _expect(dfa, text, style, lead, invert, 1, 1)))
    exe = one_amd.Executable(G._blob(dfa), **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    for style, lead, invert, x in cases:
        _same(exe, text, x, style, lead, invert, where=(dfa, opts, style, lead, invert))


LONG = b"q" * (4 * CHUNK)   # with the bytes in front of it: three whole chunks without a delimiter


def _shapes():
    """shape -> (DFA, text, [(before, after, max_count)], what the oracle must say)"""
    filler = b"".join(b"line %d of the filler\n" % k for k in range(1900))
    assert len(filler) > 40960
    return {
        "one line": ("err", b"an error here\n", [(0, 0, ALL), (5, 5, ALL)],
                     lambda x: x.counts == [1, 1, 1, 14]),
        "selected first line, before = 5": ("err", b"error\n" + b"x\n" * 20, [(5, 0, ALL), (5, 1, ALL)],
                                            lambda x: x.sel == [0] and x.n_emitted == 1 + x.after),
        "selected last line, after = 5": ("err", b"x\n" * 20 + b"error\n", [(0, 5, ALL), (1, 5, ALL)],
                                          lambda x: x.sel == [20] and x.n_emitted == 1 + x.before),
        "a tail that would match": ("err", b"no\nerror\nno\nan error in the tail", [(0, 0, ALL), (1, 1, ALL)],
                                    lambda x: x.sel == [1] and b"tail" not in x.out),
        # 8,192 lines in every chunk, every third selected: 2,731 runs in a chunk, 128 rounds of 64
        "one-byte lines, every third selected": (
            "num3", (b"1\na\nb\n" * (CHUNK + 100))[:3 * CHUNK + 7] + b"\n",
            [(0, 0, ALL), (1, 0, ALL), (0, 1, ALL), (1, 1, ALL), (0, 0, 5000)],
            lambda x: x.n_lines > 3 * 8192 and abs(3 * x.n_selected - x.n_lines) < 3
            or x.n_selected == 5000),
        "a line of three whole chunks between selected lines": (
            "err", b"a\nerror\n" + LONG + b"\nerror\nb\n", [(1, 1, ALL), (0, 0, ALL)],
            lambda x: x.sel == [1, 3] and (x.n_emitted == 5) == (x.before == 1)),
        "context behind a line of three whole chunks": (
            "err", b"a\nb\nerror\n" + LONG + b"\nc\nd\ne\n", [(0, 2, ALL), (1, 1, ALL), (0, 3, ALL)],
            lambda x: x.sel == [2] and x.emit[3] and x.emit[4] == (x.after >= 2)),
        "context in front of a line of three whole chunks": (
            "err", b"a\nb\nc\n" + LONG + b"\nd\nerror\ne\n", [(2, 0, ALL), (3, 0, ALL), (4, 1, ALL)],
            lambda x: x.sel == [5] and x.emit[3] and x.emit[2] == (x.before >= 3)),
        "two selected lines 40 KiB apart, a context of a million": (
            "err", b"error\n" + filler + b"error\nmore\nlines\nand a tail", [(10 ** 6, 10 ** 6, ALL)],
            lambda x: x.n_selected == 2 and x.n_emitted == x.n_lines and x.out.endswith(b"lines\n")),
        "before = after = 2^64 - 1": (
            "err", b"x\n" * 9000 + b"error\n" + filler + b"tail", [(2 ** 64 - 1, 2 ** 64 - 1, ALL),
                                                                 (2 ** 64 - 1, 0, ALL), (0, 2 ** 64 - 1, 1)],
            lambda x: x.n_selected == 1 and x.n_emitted in (x.n_lines, 9001, 1901)),
        "max_count with matching lines in the trailing context": (
            "err", b"x\nerror 1\nerror 2\ny\nerror 3\nerror 4\nerror 5\nz\nz\nz\nerror 6\n",
            [(0, 2, 0), (0, 2, 1), (0, 2, 3), (1, 2, 3)],
            lambda x: x.n_selected == len(x.sel) and
            x.n_emitted == {0: 0, 1: 3, 3: 6 + x.before}[len(x.sel)]),
        "nothing selected": ("err", b"nothing\nto\nsee\n" * 3000, [(0, 0, ALL), (3, 3, ALL)],
                             lambda x: x.counts == [9000, 0, 0, 0]),
    }


@pytest.mark.parametrize("shape", list(_shapes()))
def test_filter_text_shapes(shape):
    name, text, settings, check = _shapes()[shape]
    cases = []
    for before, after, mx in settings:
        x = _expect(name, text, 4, 1, False, before, after, mx)
        assert check(x), (shape, before, after, mx, x.counts, x.sel[:8])
        cases.append((False, mx, x))
        cases.append((True, mx, _expect(name, text, 4, 1, True, before, after, mx)))
    if "three whole chunks" in shape:
        offs = cases[0][2].offs
        big = int(np.argmax(np.diff(offs)))
        first = (offs[big] + CHUNK - 1) // CHUNK
        assert (offs[big + 1] - 1) // CHUNK - first >= 3      # whole chunks without a delimiter
    exe = one_amd.Executable(load_dfa(name))
    for invert, mx, x in cases:
        _same(exe, text, x, invert=invert, max_count=mx, where=(shape, invert, x.before, x.after, mx))


def test_filter_text_empty_and_lineless():
    import torch
    exe = one_amd.Executable(load_dfa("err"))
    for text in (b"", b"error, and no line end", b"error " * 9000):
        for invert in (False, True):
            assert one_amd.filter_text(exe, text, invert=invert, before=2, after=2) == (0, 0, 0, b"")
            dev = torch.from_numpy(_u8(text).copy()).cuda()
            got, buf = _raw_dev(exe, dev, 64, 64, invert=int(invert), before=2, after=2)
            assert got == [0, 0, 0, 0] and (buf == SENT).all()


@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_filter_text_other_delimiter(delim):
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = _text(name, 4).replace(b"\n", delim)
    for invert in (False, True):
        x = _expect(name, text, 4, 1, invert, 1, 2, delim=delim[0])
        assert x.n_lines >= 600 and x.n_selected >= 100 and 0 < x.n_emitted < x.n_lines
        _same(exe, text, x, invert=invert, delim=delim, where=(delim, invert))
    # ... and with '\n' the same text has no line at all
    assert one_amd.filter_text(exe, text) == (0, 0, 0, b"")


def _raw_host(exe, text, out_cap, room, style=4, invert=0, before=0, after=0, mx=ALL, nl=True,
              ns=True, ne=True, out=True):
    """redgpu_filter_text through ctypes: a sentinel-filled buffer of `room` bytes"""
    lib = _lib.lib()
    buf = np.full(room, SENT, dtype=np.uint8)
    c = [C.c_uint64(SENT) for _ in range(4)]
    rc = lib.redgpu_filter_text(exe._h, style, 1, invert, before, after, mx, text, len(text), 0x0A,
                                C.byref(c[0]) if nl else None, C.byref(c[1]) if ns else None,
                                C.byref(c[2]) if ne else None, C.byref(c[3]),
                                buf.ctypes.data if out else None, out_cap)
    assert rc == 0, lib.redgpu_last_error()
    return [x.value for x in c], buf


def _raw_dev(exe, dev, out_cap, room, style=4, invert=0, before=0, after=0, mx=ALL, out_shift=0,
             have=(True, True, True)):
    """redgpu_filter_text_dev: a sentinel-filled tensor, `room` bytes of it from out_shift on handed
    over; everything on the device.  Returns the counts and the WHOLE tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    cnt = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    ptr = [cnt.data_ptr() + 8 * k if k == 3 or have[k] else None for k in range(4)]
    rc = lib.redgpu_filter_text_dev(exe._h, style, 1, invert, before, after, mx,
                                    dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A,
                                    *ptr, buf.data_ptr() + out_shift, out_cap,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return cnt.tolist(), buf.cpu().numpy()


def _prefix_and_sentinels(buf, want, out_cap, where, shift=0):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


def test_filter_text_truncation():
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = _text(name, 4)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    for before, after in ((0, 0), (1, 1)):
        x = _expect(name, text, 4, 1, False, before, after)
        n = len(x.out)
        # the first byte behind the first run, and the middle of a line of a later chunk
        gap = int(np.flatnonzero(np.diff(x.lines) > 1)[0])
        run_end = sum(x.offs[i + 1] - x.offs[i] for i in x.lines[:gap + 1])
        assert x.out[run_end - 1] == 0x0A
        k = int(np.flatnonzero(np.array(x.offs)[x.lines] > 2 * CHUNK)[0])
        while x.offs[x.lines[k] + 1] - x.offs[x.lines[k]] < 4:
            k += 1
        inside = sum(x.offs[i + 1] - x.offs[i] for i in x.lines[:k]) + 2
        assert x.out[inside] != 0x0A and x.out[inside - 1] != 0x0A
        caps = [0, 1, 15, 16, 17, n - 1, n, n + 7, run_end - 1, run_end, run_end + 1, inside]
        assert len(set(caps)) == len(caps)
        for cap in caps:
            got, buf = _raw_host(exe, text, cap, n + 64, before=before, after=after)
            assert got == x.counts, (before, cap, got)
            _prefix_and_sentinels(buf, x.out, cap, ("host", before, cap))
            got, buf = _raw_dev(exe, dev, cap, n + 64, before=before, after=after)
            assert got == x.counts, (before, cap, got)
            _prefix_and_sentinels(buf, x.out, cap, ("dev", before, cap))


def test_filter_text_some_outputs_null():
    """n_lines, n_selected and n_emitted may be NULL each on its own, and out"""
    import torch
    name = "aab"
    exe = one_amd.Executable(load_dfa(name))
    text = _text(name, 4)
    x = _expect(name, text, 4, 1, False, 1, 1)
    n = len(x.out)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    for nl in (True, False):
        for ns in (True, False):
            for ne in (True, False):
                want = [v if on else SENT for v, on in zip(x.counts, (nl, ns, ne, True))]
                for out in (True, False):
                    got, buf = _raw_host(exe, text, n, n, before=1, after=1, nl=nl, ns=ns, ne=ne,
                                         out=out)
                    assert got == want, (nl, ns, ne, out, got)
                    assert buf.tobytes() == (x.out if out else bytes([SENT]) * n)
                got, buf = _raw_dev(exe, dev, n, n, before=1, after=1, have=(nl, ns, ne))
                assert got == want, (nl, ns, ne, got)
                _prefix_and_sentinels(buf, x.out, n, (nl, ns, ne))


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("name", ["log100", "aab"])
def test_filter_text_device_form(name, shift):
    """everything device-resident: the text at any offset from a 16-byte boundary, and -
    independently - the output"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = _text(name, 4)
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(_u8(text).copy()))
    aligned = dev.clone()
    assert dev.data_ptr() % 16 == shift and aligned.data_ptr() % 16 == 0
    for invert in (0, 1):
        for before, after in ((0, 0), (1, 1)):
            x = _expect(name, text, 4, 1, bool(invert), before, after)
            n = len(x.out)
            for cap in (n, n // 3):
                kw = dict(invert=invert, before=before, after=after)
                got, out = _raw_dev(exe, dev, cap, n, **kw)
                assert one_amd.last_kernel() == "k_filter_text"
                assert got == x.counts
                _prefix_and_sentinels(out, x.out, cap, (name, "text", shift, invert, before, cap))
                got, out = _raw_dev(exe, aligned, cap, n, out_shift=shift, **kw)
                assert got == x.counts
                _prefix_and_sentinels(out, x.out, cap, (name, "out", shift, invert, before, cap),
                                      shift=shift)
    # the verb: the counts come back as tensors
    x = _expect(name, text, 4, 1, False, 2, 0)
    got = one_amd.filter_text(exe, dev, 4, True, before=2, out_cap=len(x.out) + 3)
    torch.cuda.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got)
    assert all(v.shape == (1,) and v.dtype == torch.int64 for v in got[:4])
    assert [v.item() for v in got[:4]] == x.counts
    assert got[4][:len(x.out)].cpu().numpy().tobytes() == x.out
    mine = torch.full((len(x.out) + 5,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.filter_text(exe, dev, 4, True, before=2, out=mine)
    assert got[4] is mine and got[3].item() == len(x.out)
    assert mine.cpu().numpy().tobytes() == x.out + bytes([SENT]) * 5
    got = one_amd.filter_text(exe, dev, 4, True, before=2, out_cap=0)      # the sizes only
    assert [v.item() for v in got[:4]] == x.counts
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.filter_text(exe, dev, 4, True)                             # needs out or out_cap


@pytest.mark.parametrize("name", ["uri", "aab"])
def test_filter_text_identities(name):
    """beside the oracle: grep_text's records spell the (0, 0) output; the two inverts share the
    lines out between them; the (0, 0) output, fed back on the device, is selected line by line"""
    import torch
    exe = one_amd.Executable(load_dfa(name))
    text = _text(name, 4)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    lens = []
    for invert in (False, True):
        x = _expect(name, text, 4, 1, invert)
        rec = one_amd.grep_text(exe, text, 4, True, invert=invert)
        joined = b"".join(text[int(b):int(f) + 1] for b, f in zip(rec[3], rec[4]))
        got = one_amd.filter_text(exe, dev, 4, True, invert=invert, out_cap=len(text))
        n = int(got[3].item())
        assert got[4][:n].cpu().numpy().tobytes() == joined == x.out
        lens.append(n)
        # (the unselected lines fed back under invert are selected under invert again)
        back = one_amd.grep_text(exe, got[4][:n], 4, True, invert=invert, cap=0)
        torch.cuda.synchronize()
        assert back[0].item() == back[1].item() == got[2].item() == x.n_emitted
    assert sum(lens) == text.rindex(b"\n") + 1


def test_filter_text_above_the_grid():
    """160 MiB = 10,240 chunks: more than the waves any pass has (k_gp_select CUs x 2 workgroups of
    16 waves, the k_ft_* passes CUs x 8 of 4), so every wave takes a second chunk.  Everything stays
    on the device: a 1 MiB block that ends in a delimiter, tiled; its first and its last line are
    neither selected nor in a context, so no context reaches into another tile and the expected
    output is the block's, tiled."""
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
    x = _expect(name, block, 4, 1, False, 1, 1)
    assert len(block) == block_len and x.n_selected > 1000 and x.n_emitted < x.n_lines - 100
    assert not x.emit[0] and not x.emit[-1] and 0 not in x.sel and x.n_lines - 1 not in x.sel
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    n = len(x.out) * tiles
    got = one_amd.filter_text(exe, dev, 4, True, before=1, after=1, out_cap=n + 16)
    assert one_amd.last_kernel() == "k_filter_text"
    assert [v.item() for v in got[:4]] == [v * tiles for v in x.counts]
    exp = torch.from_numpy(_u8(x.out).copy()).cuda().repeat(tiles)
    assert torch.equal(got[4][:n], exp)


def test_filter_text_two_streams_and_threads():
    import torch
    names = ("uri", "err")
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [_text(n, 4, seed=2 + k) for k, n in enumerate(names)]
    wants = [_expect(n, t, 4, 1, False, 1, 2) for n, t in zip(names, texts)]
    assert len(wants[0].out) != len(wants[1].out)
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def same(got, x):
        n = int(got[3].item())
        assert [int(v.item()) for v in got[:4]] == x.counts
        assert got[4][:n].cpu().numpy().tobytes() == x.out

    outs = []
    for st, exe, d, x in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.filter_text(exe, d, 4, True, before=1, after=2,
                                            out_cap=len(x.out) + 3))
    torch.cuda.synchronize()
    for got, x in zip(outs, wants):
        same(got, x)
    errors = []

    def work(exe, t, d, st, x):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.filter_text(exe, d, 4, True, before=1, after=2,
                                              out_cap=len(x.out) + 3)
                    st.synchronize()
                same(got, x)
                assert one_amd.filter_text(exe, t, 4, True, before=1, after=2) == (
                    x.n_lines, x.n_selected, x.n_emitted, x.out)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_filter_text_cpp_mirror(tmp_path):
    """redgpu::filterText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "filter_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "filter_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "err"
    text = _text(name, 4)
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), "2", "1", "7", prefix], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    plain = _expect(name, text, 4, 1, False)
    ctx = _expect(name, text, 4, 1, False, 2, 1)
    inv = _expect(name, text, 4, 1, True, 2, 1, 7)
    assert run.stdout.split("\n")[:3] == ["plain %d %d" % (plain.n_selected, plain.n_emitted),
                                          "context %d %d" % (ctx.n_selected, ctx.n_emitted),
                                          "inverted %d %d" % (inv.n_selected, inv.n_emitted)]
    assert inv.n_selected == 7 and plain.n_emitted < ctx.n_emitted
    assert open(prefix + ".plain", "rb").read() == plain.out
    assert open(prefix + ".context", "rb").read() == ctx.out
    assert open(prefix + ".inverted", "rb").read() == inv.out
