"""group_text (redgpu_group_text[_dev]): awk '{ n[$k]++; s[$k] += $v }' of a raw text - one record
per distinct key string with the count, sum, minimum and maximum of its lines' numbers.  Every
scalar and every record is exact against tests/group_rule.py over the CPU oracle (text_rules.Text:
the lines and collect's pieces): both modes x six (key, value) index pairs x both `which` on five
DFAs, hand-built number and key traps whose facts are asserted before the GPU is asked, the shapes,
a hot key with and without the on-chip front, sums that wrap, a text of more chunks than the grid
has waves, tables exactly full and overflowing, a key of 2^24 bytes, cap and NULL outputs with
sentinels, every table placement, the device form at odd pointer offsets, other delimiters,
determinism, streams and threads, the C++ mirror and a smoke run of scripts/fuzz_gpu.py's groups
mode."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import threading

import numpy as np
import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

import group_rule as GR
import test_gpu_collect_text as CT
import test_gpu_dedup_text as DD
import test_gpu_long_placements as LP
import test_gpu_uniq_text as UQ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
SENT64 = 0x5555555555555555
M64 = 1 << 64
KERNEL = "k_group_text"
SEP = DD.SEP                             # the separator the err DFA finds
FUZZ_CASES, FUZZ_SEED = "24", "13"
_t = DD._t


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _check(got, want, where):
    """a host-form tuple against the rule's"""
    assert got[:4] == want[:4], (where, got[:4], want[:4])
    for g, w, what in zip(got[4:], want[4:], ("first", "length", "count", "stats")):
        assert g.dtype == np.uint64 and g.shape == w.shape, (where, what, g.shape, w.shape)
        assert np.array_equal(g, w), (where, what)


def _flat(got):
    """a tuple of scalars and arrays as something == compares bit for bit"""
    return [x if isinstance(x, int) else x.tobytes() for x in got]


def _dev_tuple(got, n=None):
    """the device form's nine tensors as the host form's tuple, and n_distinct"""
    import torch
    torch.cuda.synchronize()
    assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int64 for x in got)
    assert all(x.shape == (1,) for x in got[:5])
    nd = int(got[4].item())
    n = min(nd, got[5].numel()) if n is None else n
    arrays = [x[..., :n].cpu().numpy().view(np.uint64).copy() for x in got[5:]]
    return tuple(int(x.item()) for x in got[:4]) + tuple(arrays), nd


def _same(exe, name, text, what="field", k=1, v=2, which="first", delim=b"\n",
          forms=("host", "dev"), where=None, max_distinct=4096, shift=1):
    """both forms against the rule; returns the rule's tuple"""
    want = GR.group(_t(name, text, delim[0]), what, k, v, which)
    verb = dict(what=what, key_index=k, value_index=v, which=which, delim=delim,
                max_distinct=max_distinct)
    where = (where, what, k, v, which)
    if "host" in forms:
        got = one_amd.group_text(exe, text, **verb)
        assert one_amd.last_kernel() == KERNEL
        _check(got, want, where)
    if "dev" in forms:
        got = one_amd.group_text(exe, UQ._dev_text(text, shift), cap=len(want[4]) + 3, **verb)
        assert one_amd.last_kernel() == KERNEL
        got, nd = _dev_tuple(got)
        assert nd == len(want[4]), (where, nd)
        _check(got, want, where)
    return want


def _record(want, text, key):
    """the rule's record of one key string: (count, [numeric, sum, min, max])"""
    for j, (at, n) in enumerate(zip(want[4].tolist(), want[5].tolist())):
        if text[at:at + n] == key:
            return int(want[6][j]), [int(x) for x in want[7][:, j]]
    raise KeyError(key)


# 1 the matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["num3", "err", "aab", "log100", "uri"])
def test_group_text_matrix_vs_oracle(name):
    # (test_group_rule.py holds these texts to floors on the oracle's side)
    text = DD._matrix_text(name)
    assert 2 * CHUNK < len(text) < 3 * CHUNK and not text.endswith(b"\n")
    t = _t(name, text)
    most = max(len(p) for p in t.pieces())
    exe = one_amd.Executable(load_dfa(name))
    seen = set()
    for what in GR.WHATS:
        for k, v in ((1, 2), (2, 1), (1, 1), (1, 0), (2, most + 1), (most + 2, 1)):
            for which in ("first", "last"):
                want = _same(exe, name, text, what, k, v, which, where=name)
                seen.add((want[1], want[2], len(want[4])))
                if k > 2:
                    assert want[1:4] == (0, 0, 0) and len(want[4]) == 0
    assert len(seen) >= 5, seen


# 2 number traps -----------------------------------------------------------------------------------
def _number_lines():
    """(key, value item) pairs for FIELD with the err DFA as the separator"""
    return [(b"max", b"18446744073709551615"), (b"over", b"18446744073709551616"),
            (b"over", b"4"), (b"zeros", b"0" * 25 + b"7"), (b"oct", b"007"), (b"oct", b"x010y"),
            (b"none", b"no digit here"), (b"none", b""), (b"cross", b"abcdefghijklmn1234567xyz"),
            (b"cross", b"abcdefghijklmnop" + b"9" * 3), (b"tail", b"abc123"),
            (b"tail", b"0123456789abcdef" * 2 + b"77"), (b"pi", b"3.14"), (b"pi", b"2.71"),
            (b"two", b"12 apples and 30 pears"), (b"two", b"5"), (b"max", b"1")]


def test_group_text_number_traps_field():
    r = 100                                                   # every line that often
    lines = [k + SEP + v + b"\n" for k, v in _number_lines()]
    lines += [b"bare\n", b"bare\n", b"max" + SEP + b"2" + SEP + b"9999\n"]   # keyed, no value item
    text = b"".join(lines) * r + b"max" + SEP + b"99 in the tail"
    assert 2 * CHUNK < len(text) < 4 * CHUNK
    t = _t("err", text)
    first, last = GR.group(t, "field", 1, 2, "first"), GR.group(t, "field", 1, 2, "last")
    big = M64 - 1
    # the facts, on the rule's side: 2^64 - 1 is a number and 2^64 is none; leading zeros count
    # against nothing; an item without a digit, an empty item and a missing item are not numeric
    assert _record(first, text, b"max") == (3 * r, [3 * r, (r * (big + 1 + 2)) % M64, 1, big])
    assert _record(first, text, b"over") == (2 * r, [r, 4 * r, 4, 4])
    assert _record(first, text, b"zeros") == (r, [r, 7 * r, 7, 7])
    assert _record(first, text, b"oct") == (2 * r, [2 * r, r * 17, 7, 10])
    assert _record(first, text, b"none") == (2 * r, [0, 0, big, 0])
    assert _record(first, text, b"bare") == (2 * r, [0, 0, big, 0])
    # a run across byte 16 of its item, one that begins there, one that ends on the item's last byte
    assert _record(first, text, b"cross") == (2 * r, [2 * r, r * (1234567 + 999), 999, 1234567])
    assert _record(first, text, b"tail") == (2 * r, [2 * r, r * (123 + 123456789), 123, 123456789])
    assert _record(last, text, b"tail") == (2 * r, [2 * r, r * (123 + 77), 77, 123])
    assert _record(first, text, b"pi") == (2 * r, [2 * r, r * 5, 2, 3])
    assert _record(last, text, b"pi") == (2 * r, [2 * r, r * (14 + 71), 14, 71])
    assert _record(first, text, b"two")[1][1:] == [r * 17, 5, 12]
    assert _record(last, text, b"two")[1][1:] == [r * 35, 5, 30]
    exe = one_amd.Executable(load_dfa("err"))
    for which in ("first", "last"):
        for k, v in ((1, 2), (2, 1), (1, 3), (2, 2), (1, 1)):
            _same(exe, "err", text, "field", k, v, which, where="numbers")


def test_group_text_number_traps_match():
    # num3's pieces are the numbers: key piece 1, value piece 2; a digit right behind the value
    # piece ("123a4": the piece ends with the a) is not seen
    lines = [b"7 123a4\n", b"7 18446744073709551615\n", b"8 18446744073709551616\n", b"8 x\n",
             b"9 " + b"0" * 25 + b"7\n", b"9 007\n", b"7 55\n", b"10\n", b"no number\n"]
    text = b"".join(lines) * 300 + b"7 1"
    t = _t("num3", text)
    want = GR.group(t, "match", 1, 2)
    assert [p[3] - p[2] for p in t.pieces()[0]] == [1, 4, 1]       # "7", "123a", "4"
    assert _record(want, text, b"7") == (900, [900, (300 * (123 + M64 - 1 + 55)) % M64, 55, M64 - 1])
    assert _record(want, text, b"8") == (600, [0, 0, M64 - 1, 0])
    assert _record(want, text, b"9") == (600, [600, 300 * 14, 7, 7])
    assert _record(want, text, b"10") == (300, [0, 0, M64 - 1, 0])
    assert want[:4] == (2700, 2400, 1500, 0)
    exe = one_amd.Executable(load_dfa("num3"))
    for which in ("first", "last"):
        for k, v in ((1, 2), (2, 1), (1, 3), (3, 1), (2, 2)):
            _same(exe, "num3", text, "match", k, v, which, where="numbers")
    # aab's pieces hold no digit: the digits right in front of and behind the value piece are not
    # seen, so no line is numeric
    text = (b"aab 5aab6\n" + b"1aab2 aab\n" + b"aab\n") * 1200 + b"aab 7"
    want = GR.group(_t("aab", text), "match", 1, 2)
    assert want[:4] == (3600, 3600, 0, 0) and len(want[4]) == 1
    exe = one_amd.Executable(load_dfa("aab"))
    for k, v in ((1, 2), (2, 1), (1, 1)):
        _same(exe, "aab", text, "match", k, v, where="adjacent digits")


# 3 key traps --------------------------------------------------------------------------------------
def _placed_text():
    """three chunks and a tail for the err DFA as the separator: empty keys, a key that is the
    line's last field, a key that ends on a chunk's last byte and one that begins on a chunk's first:
    (text, where the one begins, where the other)"""
    out, n = bytearray(), [0]

    def fill(upto):
        assert upto - len(out) > 200
        while len(out) < upto:
            room = upto - len(out)
            out.extend(DD._filler(n[0], room if room <= 200 else 60 + n[0] % 30))
            n[0] += 1
        assert len(out) == upto

    lines = [SEP + b"11", SEP + b"31", b"5" + SEP, b"8" + SEP, b"100" + SEP + b"lastkey",
             b"250" + SEP + b"lastkey", b"", b"lastkey" + SEP + b"3", b"edge" + SEP + b"1"]
    out.extend(b"\n".join(lines) + b"\n")
    fill(CHUNK - 4)
    ends_at = len(out)
    out.extend(b"edge" + SEP + b"41\n")                      # "edge" = bytes [CHUNK - 4, CHUNK)
    fill(2 * CHUNK)
    begins_at = len(out)
    out.extend(b"edge" + SEP + b"500\n")                     # begins on byte 2 * CHUNK
    fill(3 * CHUNK - 30)
    out.extend(b"7" + SEP + b"edge\n" + b"edge" + SEP + b"in the tail 9")
    return bytes(out), ends_at, begins_at


def test_group_text_key_traps():
    text, ends_at, begins_at = _placed_text()
    assert ends_at + 4 == CHUNK and begins_at == 2 * CHUNK and text[begins_at - 1] == 0x0A
    t = _t("err", text)
    f12, f21 = GR.group(t, "field", 1, 2), GR.group(t, "field", 2, 1)
    big = M64 - 1
    # an empty key at the line's begin (two lines and the empty line: field 1 of it is empty too,
    # and it has no field 2) and at its end, where it sits on the delimiter
    assert _record(f12, text, b"") == (3, [2, 42, 11, 31])
    assert _record(f21, text, b"") == (2, [2, 13, 5, 8])
    # the key is the line's last field, its end the line's end; the key behind the value
    assert _record(f21, text, b"lastkey") == (2, [2, 350, 100, 250])
    assert _record(f12, text, b"lastkey") == (1, [1, 3, 3, 3])
    # "edge": four lines in three chunks, one key ends a chunk and one begins a chunk; the tail's is
    # no line
    assert _record(f12, text, b"edge") == (3, [3, 542, 1, 500])
    assert _record(f21, text, b"edge") == (1, [1, 7, 7, 7])
    assert _record(f12, text, b"5") == (1, [0, 0, big, 0])       # its value item is empty
    exe = one_amd.Executable(load_dfa("err"))
    for which in ("first", "last"):
        for k, v in ((1, 2), (2, 1), (1, 1), (2, 2), (3, 1), (1, 0)):
            _same(exe, "err", text, "field", k, v, which, where="keys")
        for k, v in ((1, 1), (1, 2)):
            _same(exe, "err", text, "match", k, v, which, where="keys")


@pytest.mark.parametrize("shape", list(CT._shapes()))
def test_group_text_shapes(shape):
    text = CT._shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        for what, k, v in (("match", 1, 2), ("match", 2, 1), ("field", 1, 2), ("field", 2, 3),
                           ("field", 3, 1)):
            want = _same(exe, name, text, what, k, v, "last", where=(shape, name))
            if shape in ("no delimiter", "empty", "one byte, no delimiter"):
                assert want[:4] == (0, 0, 0, 0) and len(want[4]) == 0


# 4 a hot key, sums that wrap ----------------------------------------------------------------------
def _hot_text():
    return b"".join(b"hot" + SEP + b"%d\n" % i for i in range(6000))


def test_group_text_hot_key_with_and_without_the_front(tmp_path):
    text = _hot_text()
    assert len(text) > 4 * CHUNK
    want = GR.group(_t("err", text), "field", 1, 2)
    assert want[:4] == (6000, 6000, 6000, 0)
    assert _record(want, text, b"hot") == (6000, [6000, 17997000, 0, 5999]) and len(want[4]) == 1
    exe = one_amd.Executable(load_dfa("err"))
    assert _lib.lib().redgpu_group_lds_slots(exe._h) >= 64
    _same(exe, "err", text, "field", 1, 2)
    mine = _flat(one_amd.group_text(exe, text))
    # the same in a process of its own under REDGPU_UNIQ_PLAIN=1, both forms: bit for bit what the
    # front gave
    out = str(tmp_path / "plain.pickle")
    script = ("import os, pickle, sys, one_amd\n"
              "import test_gpu_group_text as G\n"
              "assert os.environ['REDGPU_UNIQ_PLAIN'] == '1'\n"
              "exe = one_amd.Executable(G.load_dfa('err'))\n"
              "host = one_amd.group_text(exe, G._hot_text())\n"
              "dev, nd = G._dev_tuple(one_amd.group_text(exe, G.UQ._dev_text(G._hot_text(), 1), cap=4))\n"
              "assert one_amd.last_kernel() == G.KERNEL and nd == 1\n"
              "pickle.dump([G._flat(host), G._flat(dev)], open(sys.argv[1], 'wb'))\n")
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                           [p for p in [os.environ.get("PYTHONPATH")] if p])
    run = subprocess.run([sys.executable, "-c", script, out], capture_output=True, text=True,
                         cwd=ROOT, env=dict(os.environ, REDGPU_UNIQ_PLAIN="1", PYTHONPATH=path))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    with open(out, "rb") as f:
        host, dev = pickle.load(f)
    assert host == mine and dev == mine


def test_group_text_sum_wraps():
    text = (b"w" + SEP + b"18446744073709551615\n") * 5 + b"w" + SEP + b"1"
    exe = one_amd.Executable(load_dfa("err"))
    want = _same(exe, "err", text, "field", 1, 2)
    assert _record(want, text, b"w") == (5, [5, M64 - 5, M64 - 1, M64 - 1])


def test_group_text_above_the_grid():
    """test_uniq_text_above_the_grid's 160 MiB: a 64 KiB block that ends in a delimiter, tiled on the
    device.  Every record's first lies in block 0; count and the COUNT and SUM rows are the block's
    times the tiles, modulo 2^64; min and max are the block's."""
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
    for k, v in ((1, 2), (2, 1)):
        want = GR.group(t, "match", k, v)
        n = len(want[4])
        assert n > 20 and want[2] > 100
        got, nd = _dev_tuple(one_amd.group_text(exe, dev, what="match", key_index=k, value_index=v,
                                                max_distinct=4096, cap=n + 2))
        assert one_amd.last_kernel() == KERNEL
        assert nd == n and got[:4] == (want[0] * tiles, want[1] * tiles, want[2] * tiles, 0)
        assert np.array_equal(got[4], want[4]) and int(got[4].max()) < block_len
        assert np.array_equal(got[5], want[5])
        assert np.array_equal(got[6], want[6] * np.uint64(tiles))
        assert np.array_equal(got[7][0], want[7][0] * np.uint64(tiles))
        assert np.array_equal(got[7][1], want[7][1] * np.uint64(tiles))     # (modulo 2^64)
        assert np.array_equal(got[7][2:], want[7][2:])


# 5 many keys, small tables ------------------------------------------------------------------------
def _field_keys_text(distinct, rounds=3):
    """UQ._keys_text for the err DFA as the separator: field 1 a key of the line's own, field 2 its
    number"""
    lines = [b"k%06d" % (100000 + 7 * i) + SEP + b"%d %s\n" % (i, b"z" * (90 + i % 50))
             for i in range(distinct)]
    return b"".join(lines) * rounds


@pytest.mark.parametrize("distinct,max_distinct", [(60, 32), (64, 32), (128, 32), (60, 64),
                                                   (64, 64), (128, 64), (200, 64)])
@pytest.mark.parametrize("what", ["match", "field"])
def test_group_text_small_tables(distinct, max_distinct, what):
    slots = 2 * max_distinct
    name, text, k, v = (("num3", UQ._keys_text(distinct), 1, 1) if what == "match"
                        else ("err", _field_keys_text(distinct), 1, 2))
    t = _t(name, text)
    exact = GR.group(t, what, k, v)
    assert exact[:4] == (3 * distinct, 3 * distinct, 3 * distinct, 0) and len(exact[4]) == distinct
    recs = GR.records(t, what, k, v)
    exe = one_amd.Executable(load_dfa(name))
    # the rule alone says which cases overflow: more strings than slots
    if distinct <= slots:        # a table exactly full still drops nothing
        _same(exe, name, text, what, k, v, max_distinct=max_distinct)
        return
    verb = dict(what=what, key_index=k, value_index=v, max_distinct=max_distinct)
    host = one_amd.group_text(exe, text, **verb)
    dev, nd = _dev_tuple(one_amd.group_text(exe, UQ._dev_text(text), cap=slots, **verb))
    assert nd == slots
    for n_lines, n_keyed, n_numeric, n_dropped, first, length, count, stats in (host, dev):
        # what overflow leaves defined
        assert (n_lines, n_keyed) == exact[:2] and len(first) == slots and n_dropped > 0
        assert int(count.sum()) + n_dropped == n_keyed
        assert int(stats[0].sum()) == n_numeric
        assert np.all(np.diff(first.astype(np.int64)) > 0)
        # every record written is the rule's record of its string, in all seven values
        for j in range(slots):
            key = text[int(first[j]):int(first[j]) + int(length[j])]
            assert [int(first[j]), int(length[j]), int(count[j])] + [int(x) for x in stats[:, j]] \
                == recs[key], (j, key)


# 6 a key of 2^24 bytes ----------------------------------------------------------------------------
@pytest.mark.parametrize("size,kept", [((1 << 24), 0), ((1 << 24) - 1, 1)])
def test_group_text_overlong_key(size, kept):
    text = (b"short" + SEP + b"4\n" + b"x" * size + SEP + b"70\n" + b"short" + SEP + b"6\n")
    exe = one_amd.Executable(load_dfa("err"))
    got = one_amd.group_text(exe, text, max_distinct=32)
    assert one_amd.last_kernel() == KERNEL
    # a dropped line is keyed, and neither its count nor its number enters a record
    assert got[:4] == (3, 3, 2 + kept, 1 - kept)
    want_first = [0] + ([len(b"short") + len(SEP) + 2] if kept else [])
    assert got[4].tolist() == want_first and got[5].tolist() == [5] + ([size] if kept else [])
    assert got[6].tolist() == [2] + ([1] if kept else [])
    assert got[7].tolist() == [[2] + [1] * kept, [10] + [70] * kept, [4] + [70] * kept,
                               [6] + [70] * kept]


# 7 cap and NULL outputs ---------------------------------------------------------------------------
def _raw(exe, text, dev, cap, scalars=(1,) * 5, arrays=(1,) * 4, room=None):
    """the C-ABI itself, sentinels in every output: ([five scalars], first, length, count, stats of
    four rows of `room` cells - the row stride is cap)"""
    import torch
    lib = _lib.lib()
    room = max(cap, 1) + 4 if room is None else room
    args = [1, 1, 2, 0]                 # FIELD, key 1, value 2, FIRST
    if dev is None:
        cnt = (C.c_uint64 * 5)(*([SENT64] * 5))
        bufs = [(C.c_uint64 * n)(*([SENT64] * n)) for n in (room, room, room, 4 * room)]
        a = _u8(text)
        rc = lib.redgpu_group_text(
            exe._h, *args, a.ctypes.data if len(text) else None, len(text), 0x0A, 64, cap,
            *[C.addressof(cnt) + 8 * i if h else None for i, h in enumerate(scalars)],
            *[C.addressof(b) if h else None for b, h in zip(bufs, arrays)])
        assert rc == 0, lib.redgpu_last_error()
        return list(cnt), [np.array(b, dtype=np.uint64) for b in bufs]
    cnt = torch.full((5,), SENT64, dtype=torch.int64, device="cuda")
    bufs = [torch.full((n,), SENT64, dtype=torch.int64, device="cuda")
            for n in (room, room, room, 4 * room)]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    rc = lib.redgpu_group_text_dev(
        exe._h, *args, dev.data_ptr() if dev.numel() else None, dev.numel(), 0x0A, 64, cap,
        *[cnt.data_ptr() + 8 * i if h else None for i, h in enumerate(scalars)],
        *[b.data_ptr() if h else None for b, h in zip(bufs, arrays)], st.cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    st.synchronize()
    return (cnt.cpu().numpy().view(np.uint64).tolist(),
            [b.cpu().numpy().view(np.uint64) for b in bufs])


@pytest.mark.parametrize("form", ["host", "dev"])
def test_group_text_cap_and_null_outputs(form):
    text = _field_keys_text(20, rounds=2) + b"k100000" + SEP + b"1000\n" + b"a tail"
    t = _t("err", text)
    want = GR.group(t, "field", 1, 2)
    n = len(want[4])
    assert want[:4] == (41, 41, 41, 0) and n == 20
    exe = one_amd.Executable(load_dfa("err"))
    dev = UQ._dev_text(text, 7) if form == "dev" else None
    scalars = [want[0], want[1], want[2], n, 0]

    def held(bufs, cap, have=(1,) * 4):
        """exactly min(n, cap) records, and sentinels behind them in every array and every row"""
        k = min(n, cap)
        for b, w, h in zip(bufs[:3], want[4:7], have[:3]):
            assert np.array_equal(b[:k], w[:k]) if h else np.all(b == SENT64)
            assert np.all(b[k:] == SENT64)
        rows = bufs[3]
        if not have[3] or cap == 0:
            assert np.all(rows == SENT64)
            return
        for r in range(4):
            assert np.array_equal(rows[r * cap:r * cap + k], want[7][r, :k]), (cap, r)
            assert np.all(rows[r * cap + k:(r + 1) * cap] == SENT64), (cap, r)
        assert np.all(rows[4 * cap:] == SENT64)

    for cap in (0, 1, n - 1, n, n + 5):
        cnt, bufs = _raw(exe, text, dev, cap)
        assert cnt == scalars, (cap, cnt)
        held(bufs, cap)
    for skip in range(5):
        have = [i != skip for i in range(5)]
        cnt, bufs = _raw(exe, text, dev, n, scalars=have)
        assert cnt == [w if h else SENT64 for w, h in zip(scalars, have)]
        held(bufs, n)
    cnt, bufs = _raw(exe, text, dev, n, scalars=(0,) * 5)
    assert cnt == [SENT64] * 5
    held(bufs, n)
    for skip in range(4):
        have = [i != skip for i in range(4)]
        cnt, bufs = _raw(exe, text, dev, n - 3, arrays=have)
        assert cnt == scalars
        held(bufs, n - 3, have)
    cnt, bufs = _raw(exe, text, dev, n, arrays=(0,) * 4)
    assert cnt == scalars and all(np.all(b == SENT64) for b in bufs)
    # an empty text, one without a delimiter: all scalars 0, nothing written
    for empty in (b"", b"k" + SEP + b"123 and no line end"):
        d = UQ._dev_text(empty, 1) if form == "dev" else None
        cnt, bufs = _raw(exe, empty, d, 4)
        assert cnt == [0] * 5 and all(np.all(b == SENT64) for b in bufs)


# 8 every table placement --------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", UQ._ROWS)
def test_group_text_under_placement(dfa, opts, info):
    blob = CT._blob(dfa)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for key, val in info.items():
        assert got_info[key] == val, (dfa, opts, key, got_info[key], val)
    front = _lib.lib().redgpu_group_lds_slots(exe._h)
    assert front in (0, 64, 128, 256) and front <= _lib.lib().redgpu_uniq_lds_slots(exe._h)
    if dfa in LP.PIECES:
        half = CT._dense(LP.PIECES[dfa][0], n=CHUNK + 700, end_in_delim=True)
    else:
        half = CT._random_text("leaky" if dfa == "leaky" else "random", n=CHUNK + 700)
        half = half[:half.rindex(b"\n") + 1]
    text = half + half[:half.rindex(b"\n", 0, len(half) // 2) + 1]
    keyed = 0
    for what in GR.WHATS:
        for k, v, which in ((1, 2, "first"), (2, 1, "last"), (1, 1, "last")):
            want = _same(exe, dfa, text, what, k, v, which, where=(dfa, opts),
                         forms=("host", "dev") if k == 1 else ("host",))
            keyed += want[1]
    assert keyed > 100, (dfa, keyed)


# 9 the device form --------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_group_text_device_pointer_offsets(shift):
    import torch
    text = DD._matrix_text("num3")
    exe = one_amd.Executable(load_dfa("num3"))
    st = torch.cuda.Stream()
    for what, k, v in (("match", 1, 2), ("match", 2, 1), ("field", 2, 1)):
        want = GR.group(_t("num3", text), what, k, v, "last")
        dev = UQ._dev_text(text, shift)
        assert dev.data_ptr() % 16 == shift
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = one_amd.group_text(exe, dev, what=what, key_index=k, value_index=v, which="last",
                                     max_distinct=4096, cap=len(want[4]))
        st.synchronize()
        got, nd = _dev_tuple(got)
        assert nd == len(want[4])
        _check(got, want, (shift, what, k, v))


# 10 other delimiters ------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
def test_group_text_other_delimiter(delim):
    text = DD._matrix_text("num3").replace(delim, b",").replace(b"\n", delim)
    assert b"\n" not in text and text.count(delim) > 300
    exe = one_amd.Executable(load_dfa("num3"))
    for what, k, v in (("match", 1, 2), ("field", 2, 1)):
        want = _same(exe, "num3", text, what, k, v, delim=delim)
        assert want[1] > 0
    assert one_amd.group_text(exe, text)[:4] == (0, 0, 0, 0)


# 11 determinism, streams and threads --------------------------------------------------------------
def test_group_text_bit_identical_runs():
    text = DD._matrix_text("num3")
    exe = one_amd.Executable(load_dfa("num3"))
    for what, k, v in (("match", 1, 2), ("field", 2, 1)):
        verb = dict(what=what, key_index=k, value_index=v, max_distinct=2048)
        runs = [_dev_tuple(one_amd.group_text(exe, UQ._dev_text(text), cap=600, **verb))
                for _ in range(2)]
        assert _flat(runs[0][0]) == _flat(runs[1][0]) and runs[0][1] == runs[1][1]
        assert runs[0][0][3] == 0
        assert _flat(one_amd.group_text(exe, text, **verb)) == _flat(one_amd.group_text(exe, text, **verb))


def test_group_text_two_streams_and_threads():
    import torch
    names = ["num3", "err"]
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [DD._matrix_text(n) for n in names]
    verbs = [dict(what="match", key_index=1, value_index=2), dict(what="field", key_index=1,
                                                                   value_index=1)]
    wants = [GR.group(_t(n, x), v["what"], v["key_index"], v["value_index"])
             for n, x, v in zip(names, texts, verbs)]
    assert _flat(wants[0]) != _flat(wants[1])
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(x).copy()).cuda() for x in texts]
    torch.cuda.synchronize()
    outs = []
    for st, exe, d, w, v in zip(streams, exes, devs, wants, verbs):
        with torch.cuda.stream(st):
            outs.append(one_amd.group_text(exe, d, max_distinct=4096, cap=len(w[4]), **v))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        _check(_dev_tuple(got)[0], w, "two streams")
    errors = []

    def work(exe, x, d, st, w, v):
        # each thread on its own stream: the device form, and the host form beside it
        try:
            for _ in range(2):
                with torch.cuda.stream(st):
                    got = one_amd.group_text(exe, d, max_distinct=4096, cap=len(w[4]), **v)
                    st.synchronize()
                _check(tuple(int(t.item()) for t in got[:4]) +
                       tuple(t.cpu().numpy().view(np.uint64) for t in got[5:]), w, "thread")
                _check(one_amd.group_text(exe, x, max_distinct=4096, **v), w, "thread, host")
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a)
          for a in list(zip(exes, texts, devs, streams, wants, verbs)) * 2]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


# 12 the C++ mirror --------------------------------------------------------------------------------
def test_group_text_cpp_mirror(tmp_path):
    """redgpu::groupText (include/redgpu.hpp) compiled with g++"""
    prog = str(tmp_path / "group_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "group_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(ROOT, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "one_amd")], check=True)
    name, text = "num3", DD._matrix_text("num3")
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(ROOT, "tests", "golden", "dfas", name + ".reda")
    run = subprocess.run([prog, dfa, str(path), "2", "1"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    t = _t(name, text)
    lines = []
    for what, which in (("match", "first"), ("field", "last")):
        w = GR.group(t, what, 2, 1, which)
        lines.append("%s %d %d %d %d %d" % (what, w[0], w[1], w[2], len(w[4]), w[3]))
        for j in range(len(w[4])):
            lines.append(" ".join(str(int(x)) for x in
                                  [w[4][j], w[5][j], w[6][j]] + w[7][:, j].tolist()))
    assert len(lines) > 100 and run.stdout.split("\n")[:-1] == lines


# 13 the fuzz --------------------------------------------------------------------------------------
def test_group_text_fuzz_smoke():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), FUZZ_CASES,
                          FUZZ_SEED, "groups"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "fuzz ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert KERNEL in out.stdout
