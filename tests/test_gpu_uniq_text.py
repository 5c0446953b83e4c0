"""uniq_text (redgpu_uniq_text[_dev]): a raw text's distinct matches (or selected lines) counted by
their BYTES, one record per distinct string in the order of first appearance.  Every array and
counter is exact against a dict built from the oracle alone: the pieces and where they end from
test_gpu_extract_text._oracle / test_gpu_collect_text._want, the selected lines from the oracle's
search per line (test_gpu_grep_text._want), fed in text order into bytes -> (first offset, count).
The nine DFAs in both modes, the traps for the compare (prefixes, a last byte, chunks, a border),
a hot key and a text of more chunks than the grid has waves, tables exactly full and overflowing,
an item of 2^24 bytes, truncation with sentinels and NULL outputs, every table placement (one of
which leaves the LDS front no room), the device form at odd pointer offsets, determinism, streams
and threads, identities with extract_text / tally_text / grep_text on the GPU, other delimiters,
and the C++ mirror."""
import collections
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from golden_util import load_dfa

import test_gpu_collect_text as CT
import test_gpu_extract_text as XT
import test_gpu_grep_text as G
import test_gpu_list_verbs as LV
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

CHUNK = 16384
N = 4 * CHUNK + 5
SENT64 = 0x5555555555555555
ALL = 1 << 62
KERNEL = "k_uniq_text"
INSTANT, LAST = int(one_amd.styInstant), int(one_amd.styLast)

_expects = {}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


class _Expect:
    """items (offset, bytes) in text order -> the records: bytes -> (first, length, count), the
    dict's insertion order being the order of first appearance"""

    def __init__(self, items, n_lines, text):
        table = {}
        last = -1
        for at, s in items:
            assert at >= last, (at, last)
            assert text[at:at + len(s)] == s
            last = at
            if s in table:
                table[s][1] += 1
            else:
                table[s] = [at, 1]
        self.table = {s: (v[0], len(s), v[1]) for s, v in table.items()}
        rows = list(self.table.values())
        self.first = np.array([r[0] for r in rows], dtype=np.uint64)
        self.length = np.array([r[1] for r in rows], dtype=np.uint64)
        self.count = np.array([r[2] for r in rows], dtype=np.uint64)
        assert (np.diff(self.first.astype(np.int64)) > 0).all()
        self.n_lines, self.n_items, self.n = n_lines, len(items), len(rows)
        assert int(self.count.sum()) == self.n_items

    def arrays(self):
        return self.first, self.length, self.count


def _match_items(name, text, delim=0x0A, m=ALL):
    """extract_text's pieces under max_per_line = m, each with the offset it begins at"""
    x = XT._oracle(name, text, delim)
    w = x.want
    items, j = [], 0
    for got in x.per_line:
        for i, p in enumerate(got):
            if i < m:
                items.append((int(w.end[j]) - len(p), p))
            j += 1
    assert j == w.n
    return items, x.n_lines


def _line_items(name, text, style, lead, delim=0x0A):
    """the lines search<style,lead> selects, without their delimiters"""
    w = G._want(name, text, style, lead, False, delim)
    return [(int(b), text[int(b):int(f)]) for b, f in zip(w[3], w[4])], w[0]


def _expect(name, text, matches=True, style=INSTANT, lead=1, delim=0x0A, m=ALL):
    key = (name, text, matches, style, lead, delim, m) if not matches else (name, text, True, delim, m)
    if key not in _expects:
        items, n_lines = (_match_items(name, text, delim, m) if matches
                          else _line_items(name, text, style, lead, delim))
        _expects[key] = _Expect(items, n_lines, text)
    return _expects[key]


def _dev_text(text, shift=0):
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = buf[shift:shift + len(text)]
    if len(text):
        dev.copy_(torch.from_numpy(_u8(text).copy()))
    return dev


def _host_same(got, x, where=None, upto=None):
    k = x.n if upto is None else min(upto, x.n)
    assert got[:3] == (x.n_lines, x.n_items, 0), (where, got[:3], x.n_lines, x.n_items)
    for g, w, what in zip(got[3:], x.arrays(), ("first", "length", "count")):
        assert g.dtype == np.uint64 and len(g) == k, (where, what, len(g), k)
        assert np.array_equal(g, w[:k]), (where, what)


def _dev_same(got, x, where=None, upto=None):
    import torch
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 for t in got)
    assert all(t.shape == (1,) for t in got[:4])
    k = x.n if upto is None else min(upto, x.n)
    assert [t.item() for t in got[:4]] == [x.n_lines, x.n_items, 0, x.n], (where, got[:4])
    for g, w, what in zip(got[4:], x.arrays(), ("first", "length", "count")):
        assert np.array_equal(g[:k].cpu().numpy().astype(np.uint64), w[:k]), (where, what)


def _same(exe, text, x, matches=True, style=INSTANT, lead=1, delim=b"\n", m=ALL,
          forms=("host", "dev"), where=None, max_distinct=4096):
    import torch
    kw = dict(matches=matches, style=style, do_leader=bool(lead), delim=delim, max_per_line=m,
              max_distinct=max(max_distinct, x.n))
    if "host" in forms:
        got = one_amd.uniq_text(exe, text, **kw)
        assert one_amd.last_kernel() == KERNEL
        _host_same(got, x, where)
    if "dev" in forms:
        got = one_amd.uniq_text(exe, _dev_text(text, 1), cap=x.n + 3, **kw)
        assert one_amd.last_kernel() == KERNEL
        torch.cuda.synchronize()
        _dev_same(got, x, where)


# 1 the nine DFAs, both modes ----------------------------------------------------------------------
@pytest.mark.parametrize("name", CT.NINE)
def test_uniq_text_matrix_vs_oracle(name):
    text = CT._dense(CT.PIECES[name]())
    x = _expect(name, text)
    # the oracle's side first: extract_text's table of this text, and strings that repeat
    assert (x.n_items, x.n_lines) == (XT.TABLE[name][0], 648)
    if name in ("err", "aab", "log100"):
        assert x.n == 1 and int(x.count[0]) == x.n_items > 500       # ONE hot string
    elif name in ("num3", "set5", "ale"):
        assert 2 <= x.n < x.n_items // 2 and int(x.count.max()) > 100
    else:
        assert x.n > 100                        # a piece per hit line, from the line's begin
    exe = one_amd.Executable(load_dfa(name))
    _same(exe, text, x, where=name)
    for style, lead in ((INSTANT, 1), (LAST, 0)):
        y = _expect(name, text, False, style, lead)
        assert y.n_items >= 100 and y.n_lines == 648 and y.n >= 100, (name, y.n_items, y.n)
        _same(exe, text, y, False, style, lead, where=(name, style, lead))


# 2 traps for the compare --------------------------------------------------------------------------
POOL = [b"a 12 b", b"a 123 b", b"a 1234 b", b"a 1235 b", b"a 123a b", b"12", b"1234 1235 123 12",
        b"no digit here", b""]


def _trap_text():
    rng = np.random.default_rng(3)
    out = bytearray(b"first 777001 here\n")
    border = 1
    while len(out) < 4 * CHUNK - 300:
        room = border * CHUNK - len(out)
        if border <= 3 and room < 200:
            if border == 1:      # a piece ends on the border, its delimiter behind it
                out += b"z" * (room - 4) + b"1234\n"
            elif border == 2:    # a piece across the border
                out += b"z" * (room - 2) + b"1235 more\n"
            else:                # a piece ends on the border and the line goes on
                out += b"z" * (room - 3) + b"123 12 more\n"
            border += 1
            continue
        out += POOL[int(rng.integers(len(POOL)))] + b"\n"
    out += b"last 777001 and 777001 and 888002\n"
    out += b"the tail holds 999999 and no line end "
    out += b"t" * (N - len(out))
    return bytes(out)


def test_uniq_text_compare_traps():
    text = _trap_text()
    assert len(text) == N
    x = _expect("num3", text)
    t = x.table
    # a proper prefix of another piece (12 < 123 < 1234, 123a), pieces equal but for the last byte
    for s in (b"12", b"123", b"1234", b"1235", b"123a"):
        assert t[s][2] > 500, (s, t[s])
    assert b"999999" not in t and t[b"888002"][2] == 1
    # the same bytes in the first chunk and in the last one alone
    assert t[b"777001"] == (6, 6, 3) and text.count(b"777001") == 3
    assert text.index(b"777001", 7) > 3 * CHUNK
    # pieces that end on a border (delimiter behind / the line goes on) and one across it
    assert text[CHUNK - 4:CHUNK + 1] == b"1234\n" and text[2 * CHUNK - 2:2 * CHUNK + 2] == b"1235"
    assert text[3 * CHUNK - 3:3 * CHUNK + 1] == b"123 "
    assert x.n == 7
    exe = one_amd.Executable(load_dfa("num3"))
    _same(exe, text, x, where="traps")
    # whole lines as keys: equal lines in different chunks, the empty line among them
    y = _expect("num3", text, False)
    assert y.table[b"12"][2] > 50 and y.table[b"a 123 b"][2] > 50 and b"" not in y.table
    _same(exe, text, y, False, where="trap lines")


@pytest.mark.parametrize("shape", list(CT._shapes()))
def test_uniq_text_shapes(shape):
    text = CT._shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        x = _expect(name, text)
        if shape in ("no delimiter", "empty", "one byte, no delimiter", "one byte, a delimiter"):
            assert (x.n_items, x.n) == (0, 0)
        else:
            assert x.n_items >= 4 and 1 <= x.n <= 4, (shape, name, x.n_items, x.n)
        _same(exe, text, x, where=(shape, name))
        _same(exe, text, _expect(name, text, False), False, where=(shape, name, "lines"))


# 3 a hot key --------------------------------------------------------------------------------------
def test_uniq_text_hot_key():
    text = CT.UNIT * 6000          # 90,000 bytes, 5.5 chunks, every line the same
    for name, n in (("num3", 2), ("aab", 1)):
        x = _expect(name, text)
        assert x.n == n and int(x.count.min()) == 6000
        exe = one_amd.Executable(load_dfa(name))
        _same(exe, text, x, where=name)
        y = _expect(name, text, False)
        assert y.n == 1 and int(y.count[0]) == 6000 and int(y.length[0]) == len(CT.UNIT) - 1
        _same(exe, text, y, False, where=(name, "lines"))


def test_uniq_text_above_the_grid():
    """160 MiB = 10,240 chunks: more than the waves the walk has (CUs x 2 workgroups of 16 waves)
    and than the table-less passes have (CUs x 8 of 4), so every wave takes a second chunk and a
    workgroup's front is flushed with large counts.  Everything stays on the device: a 64 KiB
    block that ends in a delimiter, tiled; every string's count is the block's, times the tiles."""
    import torch
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 4 * CHUNK, 2560
    assert tiles * 4 > props.multi_processor_count * 8 * 4
    body = CT._dense(b"12345a")
    block = body[:body.rindex(b"\n", 0, block_len - 64) + 1]
    block = block + b" " * (block_len - len(block) - 1) + b"\n"
    assert len(block) == block_len
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    for name, matches in (("num3", True), ("err", True), ("num3", False)):
        if name == "err":
            body = CT._dense(b"error")
            blk = body[:body.rindex(b"\n", 0, block_len - 64) + 1]
            blk = blk + b" " * (block_len - len(blk) - 1) + b"\n"
            d = torch.from_numpy(_u8(blk).copy()).cuda().repeat(tiles)
        else:
            blk, d = block, dev
        x = _expect(name, blk, matches)
        assert x.n_items > 500 and (x.n == 1 if name == "err" else x.n > 50)
        exe = one_amd.Executable(load_dfa(name))
        got = one_amd.uniq_text(exe, d, matches=matches, max_distinct=4096, cap=x.n + 2)
        assert one_amd.last_kernel() == KERNEL
        torch.cuda.synchronize()
        assert [t.item() for t in got[:4]] == [x.n_lines * tiles, x.n_items * tiles, 0, x.n]
        assert np.array_equal(got[4][:x.n].cpu().numpy().astype(np.uint64), x.first)
        assert np.array_equal(got[5][:x.n].cpu().numpy().astype(np.uint64), x.length)
        assert np.array_equal(got[6][:x.n].cpu().numpy().astype(np.uint64), x.count * np.uint64(tiles))


# 4 many keys, small tables ------------------------------------------------------------------------
def _keys_text(distinct, rounds=3):
    """every line carries a number of its own; the whole set `rounds` times, three chunks and more"""
    lines = [b"k %06d %s\n" % (100000 + 7 * i, b"z" * (90 + i % 50)) for i in range(distinct)]
    return b"".join(lines) * rounds


@pytest.mark.parametrize("distinct,max_distinct", [(60, 32), (64, 32), (128, 32), (60, 64),
                                                   (64, 64), (128, 64), (200, 64)])
@pytest.mark.parametrize("matches", [True, False])
def test_uniq_text_small_tables(distinct, max_distinct, matches):
    import torch
    slots = 2 * max_distinct
    text = _keys_text(distinct)
    assert (len(text) > 2 * CHUNK) == (distinct >= 128) and len(text) > CHUNK // 2
    x = _expect("num3", text, matches)
    assert (x.n, x.n_items) == (distinct, 3 * distinct) and (x.count == 3).all()
    exe = one_amd.Executable(load_dfa("num3"))
    kw = dict(matches=matches, max_distinct=max_distinct)
    host = one_amd.uniq_text(exe, text, **kw)
    dev = one_amd.uniq_text(exe, _dev_text(text), cap=slots, **kw)
    torch.cuda.synchronize()
    if distinct <= slots:        # a table exactly full still drops nothing
        _host_same(host, x, (distinct, slots))
        assert [t.item() for t in dev[:4]] == [x.n_lines, x.n_items, 0, x.n]
        for g, w in zip(dev[4:], x.arrays()):
            assert np.array_equal(g[:x.n].cpu().numpy().astype(np.uint64), w)
        return
    # overflow: which strings have a record depends on scheduling, what a record says does not
    for n_lines, n_items, n_dropped, first, length, count in (
            host, (dev[0].item(), dev[1].item(), dev[2].item()) +
            tuple(t[:min(dev[3].item(), slots)].cpu().numpy().astype(np.uint64) for t in dev[4:])):
        assert (n_lines, n_items) == (x.n_lines, x.n_items)
        assert len(first) == len(length) == len(count) == slots       # n_distinct == table_slots
        assert int(count.sum()) + n_dropped == n_items and n_dropped > 0
        assert (np.diff(first.astype(np.int64)) > 0).all()
        for f, ln, c in zip(first.tolist(), length.tolist(), count.tolist()):
            assert x.table[text[f:f + ln]] == (f, ln, c)
    assert dev[3].item() == slots


# 5 an item of 2^24 bytes --------------------------------------------------------------------------
@pytest.mark.parametrize("size,records", [((1 << 24), 1), ((1 << 24) - 1, 2)])
def test_uniq_text_overlong_line(size, records):
    long_line = b"error" + b"x" * (size - 5)
    short = b"a short error line"
    text = short + b"\n" + long_line + b"\n" + short + b"\nnothing\n"
    cpu = O.CpuOracle(load_dfa("err"))
    assert len(long_line) == size and cpu.search(long_line, INSTANT, True)[0] > 0
    assert cpu.search(short, INSTANT, True)[0] > 0 and cpu.search(b"nothing", INSTANT, True)[0] == 0
    exe = one_amd.Executable(load_dfa("err"))
    got = one_amd.uniq_text(exe, text, matches=False, style=INSTANT, max_distinct=32)
    assert one_amd.last_kernel() == KERNEL
    assert got[:3] == (4, 3, 2 - records)
    want = [(0, len(short), 2), (len(short) + 1, size, 1)][:records]
    assert [tuple(int(v) for v in r) for r in zip(*got[3:])] == want


# 6 truncation, NULL outputs -----------------------------------------------------------------------
ROOM = 40


def _raw(exe, text, dev, matches, slots, cap, counts=(1, 1, 1, 1), arrays=(1, 1, 1)):
    """the C-ABI itself, sentinels in every output: ([four counters], [three arrays of ROOM])"""
    import torch
    lib = _lib.lib()
    what = 1 if matches else 0
    if dev is None:
        cnt = (C.c_uint64 * 4)(*([SENT64] * 4))
        arr = [(C.c_uint64 * ROOM)(*([SENT64] * ROOM)) for _ in range(3)]
        a = _u8(text)
        rc = lib.redgpu_uniq_text(
            exe._h, what, INSTANT, 1, a.ctypes.data if len(text) else None, len(text), 0x0A, ALL,
            slots, cap, *[C.addressof(cnt) + 8 * i if h else None for i, h in enumerate(counts)],
            *[C.addressof(v) if h else None for v, h in zip(arr, arrays)])
        assert rc == 0, lib.redgpu_last_error()
        return list(cnt), [np.array(v, dtype=np.uint64) for v in arr]
    cnt = torch.full((4,), SENT64, dtype=torch.int64, device="cuda")
    arr = torch.full((3, ROOM), SENT64, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    rc = lib.redgpu_uniq_text_dev(
        exe._h, what, INSTANT, 1, dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A, ALL,
        slots, cap, *[cnt.data_ptr() + 8 * i if h else None for i, h in enumerate(counts)],
        *[arr[i].data_ptr() if h else None for i, h in enumerate(arrays)], st.cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    st.synchronize()
    return cnt.cpu().numpy().astype(np.uint64).tolist(), list(arr.cpu().numpy().astype(np.uint64))


@pytest.mark.parametrize("form", ["host", "dev"])
def test_uniq_text_truncation_and_null_outputs(form):
    text = _keys_text(20) + b"12 12 12\n"
    x = _expect("num3", text)
    assert x.n == 21 < ROOM
    exe = one_amd.Executable(load_dfa("num3"))
    dev = _dev_text(text, 7) if form == "dev" else None
    want_counts = [x.n_lines, x.n_items, x.n, 0]
    for cap in (0, 1, x.n - 1, x.n, x.n + 5, ROOM, ALL):
        if cap > ROOM and form == "dev":
            continue        # (the device form is given the room it may use)
        cnt, arr = _raw(exe, text, dev, True, 64, cap)
        assert cnt == want_counts, (cap, cnt)
        k = min(cap, x.n)
        for g, w in zip(arr, x.arrays()):
            assert np.array_equal(g[:k], w[:k]) and (g[k:] == SENT64).all(), cap
    for skip in range(3):
        have = [i != skip for i in range(3)]
        cnt, arr = _raw(exe, text, dev, True, 64, ROOM, arrays=have)
        assert cnt == want_counts
        for i, (g, w) in enumerate(zip(arr, x.arrays())):
            if have[i]:
                assert np.array_equal(g[:x.n], w) and (g[x.n:] == SENT64).all()
            else:
                assert (g == SENT64).all()
    for skip in range(4):
        have = [i != skip for i in range(4)]
        cnt, arr = _raw(exe, text, dev, True, 64, ROOM, counts=have)
        assert cnt == [w if h else SENT64 for w, h in zip(want_counts, have)]
        assert np.array_equal(arr[2][:x.n], x.count)
    cnt, arr = _raw(exe, text, dev, True, 64, ROOM, counts=(0,) * 4, arrays=(0,) * 3)
    assert cnt == [SENT64] * 4 and all((g == SENT64).all() for g in arr)


# 7 every table placement --------------------------------------------------------------------------
CT._blobs.setdefault("rnd318", LV.random_dfa(318, 256, 4, dead_frac=0.05, accept_frac=0.1))
# rnd318 in LDS: 162,816 bytes of table leave 496 bytes of the workgroup's share - no front
_ROWS = LP.ROWS + CT._MORE_ROWS + [
    pytest.param("rnd318", dict(lds_table_max=200000), dict(table_kind=2, table_bytes=162816),
                 id="rnd318-lds_table_max=200000-kind2")]
_fronts = set()


@pytest.mark.parametrize("dfa,opts,info", _ROWS)
def test_uniq_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    front = _lib.lib().redgpu_uniq_lds_slots(exe._h)
    assert front in (0, 64, 128, 256, 512, 1024)
    assert (front == 0) == (dfa == "rnd318"), (dfa, front)
    if dfa in LP.PIECES:
        text = CT._dense(LP.PIECES[dfa][0])
    else:
        text = CT._random_text("leaky" if dfa == "leaky" else "random")
    x = _expect(dfa, text)
    assert x.n_items >= 50 and x.n >= 1, (dfa, x.n_items, x.n)
    _same(exe, text, x, where=(dfa, opts))
    # the selected lines: over test_gpu_grep_text's text of the row
    text = G._placement_text(dfa)
    for style, lead in ((INSTANT, 1), (LAST, 0)):
        y = _expect(dfa, text, False, style, lead)
        assert y.n_items >= 20, (dfa, style, lead, y.n_items)
        _same(exe, text, y, False, style, lead, forms=("host",), where=(dfa, opts, style, lead))


# 8 the device form --------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_uniq_text_device_pointer_offsets(shift):
    import torch
    text = CT._dense(b"12345a", seed=2)
    exe = one_amd.Executable(load_dfa("num3"))
    st = torch.cuda.Stream()
    for matches in (True, False):
        x = _expect("num3", text, matches)
        dev = _dev_text(text, shift)
        assert dev.data_ptr() % 16 == shift
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = one_amd.uniq_text(exe, dev, matches=matches, max_distinct=4096, cap=x.n)
        st.synchronize()
        _dev_same(got, x, (shift, matches))


def test_uniq_text_empty_and_lineless():
    exe = one_amd.Executable(load_dfa("num3"))
    for text in (b"", b"123 and no line end", b"123 " * 9000):
        for matches in (True, False):
            got = one_amd.uniq_text(exe, text, matches=matches)
            assert got[:3] == (0, 0, 0) and all(len(g) == 0 for g in got[3:])
            for dev in (None, _dev_text(text, 1)):
                cnt, arr = _raw(exe, text, dev, matches, 64, ROOM)
                assert cnt == [0, 0, 0, 0] and all((g == SENT64).all() for g in arr)


# 9 determinism, streams and threads ---------------------------------------------------------------
def test_uniq_text_bit_identical_runs():
    import torch
    text = CT._dense(b"12345a", seed=3)
    exe = one_amd.Executable(load_dfa("num3"))
    dev = _dev_text(text)
    runs = []
    for _ in range(2):
        got = one_amd.uniq_text(exe, dev, max_distinct=2048, cap=2048)
        torch.cuda.synchronize()
        assert got[2].item() == 0
        n = got[3].item()
        runs.append([t.cpu().numpy().copy() for t in got[:4]] + [t[:n].cpu().numpy().copy() for t in got[4:]])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert [a.tobytes() for a in one_amd.uniq_text(exe, text)[3:]] == \
        [a.tobytes() for a in one_amd.uniq_text(exe, text)[3:]]


def test_uniq_text_two_streams_and_threads():
    import torch
    names = ["num3", "aab"]
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [CT._dense(b"12345a", seed=4), CT._dense(b"aab", seed=5)]
    wants = [_expect(n, t) for n, t in zip(names, texts)]
    assert wants[0].n != wants[1].n
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, exe, d, x in zip(streams, exes, devs, wants):
        with torch.cuda.stream(st):
            outs.append(one_amd.uniq_text(exe, d, max_distinct=4096, cap=x.n + 1))
    torch.cuda.synchronize()
    for got, x in zip(outs, wants):
        _dev_same(got, x)
    errors = []

    def work(exe, t, d, st, x):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.uniq_text(exe, d, max_distinct=4096, cap=x.n + 1)
                    st.synchronize()
                _dev_same(got, x)
                _host_same(one_amd.uniq_text(exe, t, max_distinct=4096), x)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# 10 identities on the GPU -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["num3", "uri", "ale"])
def test_uniq_text_identities(name):
    text = CT._dense(CT.PIECES[name]())
    exe = one_amd.Executable(load_dfa(name))
    for m in (ALL, 1, 3):
        got = one_amd.uniq_text(exe, text, max_per_line=m)
        out = one_amd.extract_text(exe, text, max_per_line=m)
        pieces = out[2].split(b"\n")[:-1]
        assert got[1] == out[1] == len(pieces) and got[2] == 0
        counter = collections.Counter(pieces)
        mine = {text[int(f):int(f + ln)]: int(c) for f, ln, c in zip(*got[3:])}
        assert mine == dict(counter) and len(mine) == len(got[3])
        # ... in the order of first appearance
        seen = list(dict.fromkeys(pieces))
        assert [text[int(f):int(f + ln)] for f, ln in zip(got[3], got[4])] == seen
    assert one_amd.uniq_text(exe, text)[1] == one_amd.tally_text(exe, text)[1]
    for style in (INSTANT, LAST):
        lines = one_amd.uniq_text(exe, text, matches=False, style=style)
        assert lines[1] == one_amd.grep_text(exe, text, style)[1] > 0
        assert lines[1] == one_amd.tally_text(exe, text, matches=False, style=style)[1]


# 11 other delimiters ------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_uniq_text_other_delimiter(delim):
    text = CT._dense(b"12345a").replace(delim, b",").replace(b"\n", delim)
    assert text.count(delim) == 648 and b"\n" not in text
    exe = one_amd.Executable(load_dfa("num3"))
    for matches in (True, False):
        x = _expect("num3", text, matches, delim=delim[0])
        assert x.n_lines == 648 and x.n_items > 300
        _same(exe, text, x, matches, delim=delim, where=(delim, matches))
    assert one_amd.uniq_text(exe, text)[:2] == (0, 0)


# 12 the C++ mirror --------------------------------------------------------------------------------
def test_uniq_text_cpp_mirror(tmp_path):
    """redgpu::uniqText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "uniq_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "uniq_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "num3"
    text = CT._dense(b"12345a")
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    run = subprocess.run([prog, dfa, str(path), "4096"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    want = []
    for what, x in (("matches", _expect(name, text)), ("lines", _expect(name, text, False))):
        want.append("%s %d %d 0 %d" % (what, x.n_lines, x.n_items, x.n))
        want += ["%d %d %d" % r for r in zip(x.first.tolist(), x.length.tolist(), x.count.tolist())]
    assert run.stdout.split("\n")[:-1] == want
