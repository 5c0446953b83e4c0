"""replace_text (redgpu_replace_text[_dev]): sed - every line of a raw text rewritten by
replace<style,doLeader> and the text put back together.  The three counts and the bytes are exact
against sampleLines' loop (oracle.split_lines_loop) plus the CPU oracle's replace per line (and the
reference's, when it is built): the nine DFAs over a dense text under every style, leader setting,
max and replacement length, every table placement, the chunk-border shapes, rounds of 64 lines with
uneven counts, truncation at every kind of out_cap with a sentinel behind it, optional outputs, the
device form at odd pointer offsets of the text and of the output, the composed route on the GPU,
the known answers, other delimiters, a text of more chunks than the grid has waves, concurrent
streams and threads, and the C++ mirror."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from golden_util import GOLD, load_dfa, unb64

import test_gpu_collect_text as CT
import test_gpu_list_verbs as LV
import test_gpu_long_placements as LP
from test_gpu_collect_text import PIECES, _dense, _random_text, _shapes, _u8

pytestmark = pytest.mark.gpu

CHUNK = 16384
SENT = 0x55
ALL = 1 << 62
STYLES = [one_amd.styInstant, one_amd.styFirst, one_amd.styTangent, one_amd.styLast, one_amd.styFull]
REPLS = (b"", b"x", b"<#>", b"0123456789abcdefghijABCDEFGHIJ0123456789")
NINE = CT.NINE

_cpus = {}
_refs = {}
_wants = {}


def _cpu(name):
    if name not in _cpus:
        _cpus[name] = O.CpuOracle(CT._blob(name))
    return _cpus[name]


class _Want:
    """the oracle's answer for (DFA, text, repl, style, leader, max, delimiter): per line the count
    and the rewritten bytes, and from them both outputs"""

    def __init__(self, name, text, repl, style, lead, mx, delim):
        cpu = _cpu(name)
        self.lines = O.split_lines_loop(text, delim)
        self.n_lines = len(self.lines)
        res = [cpu.replace(x, repl, style, lead, mx) for x in self.lines]
        self.counts = np.array([r[0] for r in res], dtype=np.int64)
        self.new = [r[1] for r in res]
        self.n_replaced = int(self.counts.sum())
        used = sum(len(x) + 1 for x in self.lines)
        self.tail = text[used:]
        d = bytes([delim])
        self.out = {0: b"".join(x + d for x in self.new) + self.tail,
                    1: b"".join(x + d for x, c in zip(self.new, self.counts) if c)}
        self.changed = int((self.counts > 0).sum())
        if O.have_ref():
            if name not in _refs:
                _refs[name] = O.Reference(CT._blob(name))
            for k in range(0, self.n_lines, 5):
                assert _refs[name].replace(self.lines[k], repl, style, lead, mx) == res[k], (name, k)

    def finish(self):
        """the offsets of the lines' delimiters"""
        return np.cumsum([len(x) + 1 for x in self.lines]).astype(np.int64) - 1

    def out_base(self, chunk, only_changed=0):
        """output bytes of the lines that end below chunk * 16384"""
        below = self.finish() < chunk * CHUNK
        sizes = np.array([len(x) + 1 for x in self.new], dtype=np.int64)
        if only_changed:
            sizes = sizes * (self.counts > 0)
        return int(sizes[below].sum())


def _want(name, text, repl=b"<#>", style=one_amd.styLast, lead=1, mx=ALL, delim=0x0A):
    key = (name, text, repl, int(style), int(lead), mx, delim)
    if key not in _wants:
        _wants[key] = _Want(name, text, repl, style, lead, mx, delim)
    return _wants[key]


def _same(exe, text, want, repl, style=one_amd.styLast, lead=1, mx=ALL, delim=b"\n", where=None):
    for oc in (0, 1):
        got = one_amd.replace_text(exe, text, repl, style, bool(lead), mx, only_changed=bool(oc),
                                   delim=delim)
        assert one_amd.last_kernel() == "k_replace_text"
        assert got[:2] == (want.n_lines, want.n_replaced), (where, oc, got[:2])
        assert len(got[2]) == len(want.out[oc]), (where, oc, len(got[2]), len(want.out[oc]))
        assert got[2] == want.out[oc], (where, oc)


# (replacements, changed lines of 648, out_len) for repl = b"<#>", do_leader = 1:
# styLast max = all, styLast max = 1, styInstant max = all
TABLE = {
    "err": ((1865, 210, 61811), (210, 210, 65121), (1865, 210, 61811)),
    "dotstar_err": ((210, 210, 45051), (210, 210, 45051), (1865, 210, 50016)),
    "newyork": ((209, 209, 45312), (209, 209, 45312), (2948, 209, 53529)),
    "uri": ((163, 163, 48169), (163, 163, 48169), (314, 163, 55268)),
    "log100": ((741, 193, 52944), (193, 193, 62260), (741, 193, 52944)),
    "aab": ((2257, 214, 65541), (214, 214, 65541), (2257, 214, 65541)),
    "ale": ((2055, 214, 63403), (214, 214, 65315), (2055, 214, 65541)),
    "num3": ((10014, 625, 74403), (625, 625, 65615), (19217, 625, 103975)),
    "set5": ((10759, 621, 85774), (621, 621, 66730), (12044, 621, 89629)),
}


@pytest.mark.parametrize("name", NINE)
def test_replace_text_dense_text_is_what_the_table_says(name):
    text = _dense(PIECES[name]())
    assert len(text) == 4 * CHUNK + 5
    for (style, mx), row in zip(((one_amd.styLast, ALL), (one_amd.styLast, 1), (one_amd.styInstant, ALL)),
                                TABLE[name]):
        w = _want(name, text, b"<#>", style, 1, mx)
        assert w.n_lines == 648 and len(w.tail) == 13
        assert (w.n_replaced, w.changed, len(w.out[0])) == row, (name, style, mx)
        # every chunk holds both changed and unchanged lines
        ch = w.finish() // CHUNK
        for k in range(4):
            here = w.counts[ch == k]
            assert (here > 0).any() and (here == 0).any(), (name, k)


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", NINE)
def test_replace_text_matrix_vs_oracle(name, style):
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    for lead in (0, 1):
        for mx in (0, 1, 2, ALL):
            for repl in REPLS:
                w = _want(name, text, repl, style, lead, mx)
                if mx == 0:
                    assert w.n_replaced == 0 and w.out[0] == text and w.out[1] == b""
                _same(exe, text, w, repl, style, lead, mx, where=(name, style, lead, mx, repl))
                del _wants[(name, text, repl, int(style), lead, mx, 0x0A)]


_MORE_ROWS = [pytest.param(*p.values[:3], id=p.id) for p in LV.TABLE
              if p.values[0] in ("syn256", "rnd72", "leaky") and not p.values[1]]


@pytest.mark.parametrize("dfa,opts,info", LP.ROWS + _MORE_ROWS)
def test_replace_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
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
    for style in (one_amd.styLast, one_amd.styInstant):
        for mx in (1, ALL):
            w = _want(dfa, text, b"<#>", style, 1, mx)
            # not vacuous: changed lines in every chunk, and unchanged lines among them
            assert w.changed >= 50 and w.n_lines - w.changed >= 5, (dfa, w.changed)
            assert len(set((w.finish()[w.counts > 0] // CHUNK).tolist())) >= 4, dfa
            _same(exe, text, w, b"<#>", style, 1, mx, where=(dfa, opts, style, mx))


def _more_shapes():
    out = dict(_shapes())
    short = CT.SHORT
    out["a 40 KiB line without a match between hit lines"] = short + b"no match, " * 4096 + b"\n" + short
    out["every line changes"] = CT.UNIT * 2500
    out["no line changes"] = b"nothing to see in this line\n" * 2500 + b"nor here"
    return out


@pytest.mark.parametrize("shape", list(_more_shapes()))
def test_replace_text_shapes(shape):
    text = _more_shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        for repl in (b"<#>", b"", b"0123456789"):
            w = _want(name, text, repl)
            if shape in ("no delimiter", "empty", "one byte, no delimiter"):
                assert (w.n_lines, w.n_replaced) == (0, 0) and w.out[0] == text and w.out[1] == b""
            elif shape == "one byte, a delimiter":
                assert (w.n_lines, w.n_replaced, w.out[0], w.out[1]) == (1, 0, b"\n", b"")
            elif shape == "a match in the tail":
                assert w.out[0].endswith(b"an aab and 123 in the tail") and w.n_replaced > 0
            elif shape == "one 40 KiB line":
                assert w.counts.max() >= 5120
            elif shape == "a 40 KiB line without a match between hit lines":
                big = int(np.argmax([len(x) for x in w.lines]))
                assert len(w.lines[big]) == 40960 and w.counts[big] == 0
                assert w.counts[big - 1] > 0 or w.counts[big - 2] > 0
                assert w.counts[big + 1] > 0
            elif shape == "every line changes":
                assert w.changed == w.n_lines == 2500
            elif shape == "no line changes":
                assert w.changed == 0 and w.out[0] == text and w.out[1] == b""
            else:
                assert w.n_replaced > 1000, (shape, name)
            _same(exe, text, w, repl, where=(shape, name, repl))


def test_replace_text_rounds_with_uneven_counts():
    """one chunk, 300 lines (five rounds of 64), line i with i % 10 matches: the prefixes inside a
    round and the carry between rounds differ from lane to lane"""
    text = b"".join(b"aab " * (i % 10) + b"\n" for i in range(300))
    assert len(text) < CHUNK
    exe = one_amd.Executable(load_dfa("aab"))
    for repl in (b"", b"seven77"):
        w = _want("aab", text, repl)
        assert w.counts.tolist() == [i % 10 for i in range(300)]
        _same(exe, text, w, repl, where=repl)
        w = _want("aab", text, repl, mx=3)
        assert w.counts.tolist() == [min(i % 10, 3) for i in range(300)]
        _same(exe, text, w, repl, mx=3, where=(repl, 3))


def _raw_host(exe, text, repl, out_cap, room, oc=0, style=4, mx=ALL, nl=True, nr=True, out=True):
    """redgpu_replace_text through ctypes: a sentinel-filled buffer of `room` bytes"""
    lib = _lib.lib()
    buf = np.full(room, SENT, dtype=np.uint8)
    c = [C.c_uint64(SENT) for _ in range(3)]
    rc = lib.redgpu_replace_text(exe._h, style, 1, oc, text, len(text), 0x0A, repl, len(repl), mx,
                                 C.byref(c[0]) if nl else None, C.byref(c[1]) if nr else None,
                                 C.byref(c[2]), buf.ctypes.data if out else None, out_cap)
    assert rc == 0, lib.redgpu_last_error()
    return [x.value for x in c], buf


def _raw_dev(exe, dev, repl, out_cap, room, oc=0, style=4, mx=ALL, out_shift=0):
    """redgpu_replace_text_dev: a sentinel-filled tensor, `room` bytes of it from out_shift on handed
    over; everything on the device.  Returns the counts and the WHOLE tensor."""
    import torch
    lib = _lib.lib()
    buf = torch.full((room + 32,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    drepl = torch.from_numpy(_u8(repl).copy()).cuda()
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    rc = lib.redgpu_replace_text_dev(exe._h, style, 1, oc, dev.data_ptr() if dev.numel() else None,
                                     dev.numel(), 0x0A, drepl.data_ptr() if len(repl) else None,
                                     len(repl), mx, cnt.data_ptr(), cnt.data_ptr() + 8,
                                     cnt.data_ptr() + 16, buf.data_ptr() + out_shift, out_cap,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return cnt.tolist(), buf.cpu().numpy()


def _prefix_and_sentinels(buf, want, out_cap, where, shift=0):
    k = min(len(want), out_cap)
    assert (buf[:shift] == SENT).all(), where
    assert buf[shift:shift + k].tobytes() == want[:k], where
    assert (buf[shift + k:] == SENT).all(), where


def test_replace_text_truncation():
    import torch
    name, repl = "num3", b"<#>"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    w = _want(name, text, repl)
    dev = torch.from_numpy(_u8(text).copy()).cuda()
    for oc in (0, 1):
        want = w.out[oc]
        n = len(want)
        base1 = w.out_base(1, oc)
        assert 0 < base1 < n and want[base1 - 1] == 0x0A
        in_repl = want.index(repl) + 1                     # behind the '<' of the first replacement
        counts = [w.n_lines, w.n_replaced, n]
        caps = [0, 1, 15, 16, 17, n - 1, n, n + 1, in_repl, base1 - 1, base1, base1 + 1]
        if not oc:
            # inside an unchanged stretch: the middle of a line without a replacement
            long = np.array([len(x) for x in w.new]) >= 8
            k = int(np.flatnonzero((w.counts == 0) & long)[3])
            at = sum(len(x) + 1 for x in w.new[:k]) + len(w.new[k]) // 2
            assert len(w.new[k]) >= 2 and want[at:at + 1] != b"\n"
            caps.append(at)
        assert want[in_repl - 1:in_repl + 2] == b"<#>" and len(set(caps)) == len(caps)
        for cap in caps:
            got, buf = _raw_host(exe, text, repl, cap, n + 64, oc)
            assert got == counts, (oc, cap, got)
            _prefix_and_sentinels(buf, want, cap, ("host", oc, cap))
            got, buf = _raw_dev(exe, dev, repl, cap, n + 64, oc)
            assert got == counts, (oc, cap, got)
            _prefix_and_sentinels(buf, want, cap, ("dev", oc, cap))


def test_replace_text_some_outputs_null():
    """n_lines and n_replaced may be NULL each on its own, and out"""
    name, repl = "aab", b"0123456789"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    w = _want(name, text, repl)
    n = len(w.out[0])
    for nl in (True, False):
        for nr in (True, False):
            for out in (True, False):
                got, buf = _raw_host(exe, text, repl, n, n, nl=nl, nr=nr, out=out)
                assert got == [w.n_lines if nl else SENT, w.n_replaced if nr else SENT, n]
                assert buf.tobytes() == (w.out[0] if out else bytes([SENT]) * n)


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("name", ["num3", "log100"])
def test_replace_text_device_form(name, shift):
    """everything device-resident: the text at any offset from a 16-byte boundary, and -
    independently - the output"""
    import torch
    repl = b"<#>"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    w = _want(name, text, repl)
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    dev.copy_(torch.from_numpy(_u8(text).copy()))
    aligned = dev.clone()
    assert dev.data_ptr() % 16 == shift and aligned.data_ptr() % 16 == 0
    for oc in (0, 1):
        n = len(w.out[oc])
        for cap in (n, n // 3):
            got, out = _raw_dev(exe, dev, repl, cap, n, oc)
            assert one_amd.last_kernel() == "k_replace_text"
            assert got == [w.n_lines, w.n_replaced, n]
            _prefix_and_sentinels(out, w.out[oc], cap, (name, "text", shift, oc, cap))
            got, out = _raw_dev(exe, aligned, repl, cap, n, oc, out_shift=shift)
            assert got == [w.n_lines, w.n_replaced, n]
            _prefix_and_sentinels(out, w.out[oc], cap, (name, "out", shift, oc, cap), shift=shift)
    # the verb: the counts come back as tensors
    got = one_amd.replace_text(exe, dev, repl, out_cap=len(w.out[0]) + 3)
    torch.cuda.synchronize()
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    assert all(x.shape == (1,) and x.dtype == torch.int64 for x in got[:3])
    assert [x.item() for x in got[:3]] == [w.n_lines, w.n_replaced, len(w.out[0])]
    assert got[3][:len(w.out[0])].cpu().numpy().tobytes() == w.out[0]
    mine = torch.full((len(w.out[1]) + 5,), SENT, dtype=torch.uint8, device="cuda")
    got = one_amd.replace_text(exe, dev, torch.from_numpy(_u8(repl).copy()).cuda(), only_changed=True,
                               out=mine)
    assert got[3] is mine and got[2].item() == len(w.out[1])
    assert mine.cpu().numpy().tobytes() == w.out[1] + bytes([SENT]) * 5
    got = one_amd.replace_text(exe, dev, repl, out_cap=0)               # the sizes only
    assert [x.item() for x in got[:3]] == [w.n_lines, w.n_replaced, len(w.out[0])]
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_text(exe, dev, repl)                            # needs out or out_cap


def test_replace_text_empty_and_lineless_on_the_device():
    """the _dev form writes the counts on the stream, and copies a text without a line"""
    import torch
    exe = one_amd.Executable(load_dfa("aab"))
    for text in (b"", b"aab, and no line end", b"aab " * 9000):
        dev = torch.from_numpy(_u8(text).copy()).cuda()
        got, out = _raw_dev(exe, dev, b"<#>", len(text) + 8, len(text) + 8)
        assert got == [0, 0, len(text)]
        _prefix_and_sentinels(out, text, len(text) + 8, text[:8])
        got, out = _raw_dev(exe, dev, b"<#>", len(text) + 8, len(text) + 8, oc=1)
        assert got == [0, 0, 0] and (out == SENT).all()
        got, out = _raw_dev(exe, dev, b"<#>", len(text) // 2, len(text) + 8, out_shift=3)
        assert got == [0, 0, len(text)]
        _prefix_and_sentinels(out, text, len(text) // 2, text[:8], shift=3)


@pytest.mark.parametrize("name", ["num3", "log100"])
def test_replace_text_equals_the_composed_route(name):
    """split_lines + replace_batch(stride = 1), the delimiters put back in numpy - on the GPU"""
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]())
    repl = b"<#>"
    offs, n_lines = one_amd.split_lines(exe, text)
    for style, mx in ((one_amd.styLast, ALL), (one_amd.styInstant, 1)):
        counts, ooff, out = one_amd.replace_batch(exe, text, repl, style, True, mx, offsets=offs,
                                                  stride=1)
        assert int(counts.sum()) > 150
        parts = [out[int(ooff[i]):int(ooff[i + 1])].tobytes() + b"\n" for i in range(n_lines)]
        tail = text[int(offs[-1]):]
        got = one_amd.replace_text(exe, text, repl, style, True, mx)
        assert got == (n_lines, int(counts.sum()), b"".join(parts) + tail)
        got = one_amd.replace_text(exe, text, repl, style, True, mx, only_changed=True)
        assert got == (n_lines, int(counts.sum()), b"".join(p for p, c in zip(parts, counts) if c))


def test_replace_text_kat():
    """the known answers of tests/golden/replace_kat.json: the texts of every entry with the same
    DFA, style, max (and replacement) joined by a delimiter byte that occurs in none of them"""
    groups = {}
    for k in json.load(open(os.path.join(GOLD, "replace_kat.json"))):
        groups.setdefault((k["reda"], k["style"], k["max"], k["repl"]), []).append(k)
    ran = 0
    for (reda, style, mx, repl), ks in groups.items():
        texts = [k["text"].encode() for k in ks]
        used = set(b"".join(texts))
        free = [d for d in (0x0A, 0x00, 0x3B, 0x7C, 0x01) if d not in used]
        if not free:
            continue
        d = bytes([free[0]])
        # (max_count is per line, as the known answers are)
        exe = one_amd.Executable(unb64(reda))
        text = b"".join(t + d for t in texts)
        want = b"".join(k["expect"].encode() + d for k in ks)
        got = one_amd.replace_text(exe, text + b"tail", repl.encode(), O.STYLES[style], True, mx, delim=d)
        assert got == (len(ks), sum(k["count"] for k in ks), want + b"tail"), (style, mx, repl)
        ran += len(ks)
    assert ran >= 30


@pytest.mark.parametrize("delim", [b"\x00", b";"])
def test_replace_text_other_delimiter(delim):
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = _dense(PIECES[name]()).replace(b"\n", delim)
    w = _want(name, text, b"<#>", delim=delim[0])
    assert w.n_lines >= 648 and w.n_replaced > 1000
    _same(exe, text, w, b"<#>", delim=delim)
    # ... and with '\n' the same text has no line at all: it is its own tail
    assert one_amd.replace_text(exe, text, b"<#>") == (0, 0, text)
    assert one_amd.replace_text(exe, text, b"<#>", only_changed=True) == (0, 0, b"")


def test_replace_text_above_the_grid():
    """160 MiB = 10,240 chunks: more than the waves either pass has (k_rt_count CUs x 2 workgroups
    of 16 waves, k_rt_write CUs x 2 of 8), so every wave takes a second chunk.  Everything stays on
    the device: a 1 MiB block that ends in a delimiter, tiled; the expected output is the block's,
    tiled."""
    import torch
    name, repl = "err", b"<#>"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 16
    block = _dense(PIECES[name](), seed=3, n=block_len, end_in_delim=True)
    assert block[-1] == 0x0A
    w = _want(name, block, repl)
    assert w.n_replaced > 10000 and w.tail == b"" and len(w.out[0]) != block_len
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    for oc in (0, 1):
        n = len(w.out[oc]) * tiles
        got = one_amd.replace_text(exe, dev, repl, only_changed=bool(oc), out_cap=n + 16)
        assert one_amd.last_kernel() == "k_replace_text"
        assert [x.item() for x in got[:3]] == [w.n_lines * tiles, w.n_replaced * tiles, n]
        exp = torch.from_numpy(_u8(w.out[oc]).copy()).cuda().repeat(tiles)
        assert torch.equal(got[3][:n], exp), oc
        del got, exp


def test_replace_text_two_streams_and_threads():
    import torch
    names = ("num3", "err")
    repl = b"<#>"
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [_dense(PIECES[n](), seed=2 + k) for k, n in enumerate(names)]
    wants = [_want(n, t, repl) for n, t in zip(names, texts)]
    assert len(wants[0].out[0]) != len(wants[1].out[0])
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def same(got, w):
        n = int(got[2].item())
        assert (int(got[0].item()), int(got[1].item()), n) == (w.n_lines, w.n_replaced, len(w.out[0]))
        assert got[3][:n].cpu().numpy().tobytes() == w.out[0]

    outs = []
    for st, exe, d, w in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.replace_text(exe, d, repl, out_cap=len(w.out[0]) + 3))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        same(got, w)
    errors = []

    def work(exe, t, d, st, w):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.replace_text(exe, d, repl, out_cap=len(w.out[0]) + 3)
                    st.synchronize()
                same(got, w)
                assert one_amd.replace_text(exe, t, repl) == (w.n_lines, w.n_replaced, w.out[0])
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_replace_text_cpp_mirror(tmp_path):
    """redgpu::replaceText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "replace_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "replace_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name, repl = "num3", b"<#>"
    text = _dense(PIECES[name]())
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    prefix = str(tmp_path / "out")
    run = subprocess.run([prog, dfa, str(path), repl.decode(), "2", prefix], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    two, every = _want(name, text, repl, mx=2), _want(name, text, repl)
    assert two.n_replaced != every.n_replaced
    assert run.stdout.split("\n")[:3] == ["all %d" % two.n_replaced, "changed %d" % two.n_replaced,
                                          "default %d" % every.n_replaced]
    assert open(prefix + ".all", "rb").read() == two.out[0]
    assert open(prefix + ".changed", "rb").read() == two.out[1]
    assert open(prefix + ".default", "rb").read() == every.out[0]
