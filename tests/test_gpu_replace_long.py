"""replace_long (redgpu_replace_long[_dev]): replaceCore over ONE long text, chunk-parallel,
bit-exact against the CPU oracle (and the reference when present) - count and bytes - for every
style, leader setting, max count, replacement length and chunk size; the routes, matches that
span many chunks, match-dense text, chains that never resynchronise, truncation, the device form,
concurrent streams and threads."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from one_amd import workloads as W
from oracle.reda_writer import random_dfa, write_reda
from golden_util import GOLD, literal_dfa, load_dfa, scan_round_text, unb64

pytestmark = pytest.mark.gpu

DEAD = ["num3", "set5", "log100", "aab", "ale", "num3defg"]   # DFAs with a pure dead state
DENSE = ["newyork", "uri", "syn256"]                          # ... and without one
STYLES = [1, 2, 3, 4, 5]
ALL = 1 << 62
CLOSED = {"newyork": b"New York", "uri": b"http://www.example.com/index.html"}

_cache = {}


def _expect(blob, text, repl, style, lead, mx, key=None):
    """(count, bytes) of the CPU oracle, checked against the reference when it is built; cached
    under `key` (a DFA/text name) so a chunk-size sweep computes it once."""
    k = (key, style, lead, repl, mx) if key is not None else None
    if k is not None and k in _cache:
        return _cache[k]
    want = O.CpuOracle(blob).replace(text, repl, style, bool(lead), mx)
    if O.have_ref():
        assert O.Reference(blob).replace(text, repl, style, bool(lead), mx) == want
    if k is not None:
        _cache[k] = want
    return want


def _check(exe, blob, text, chunk, repl=b"<#>", style=4, lead=1, mx=ALL, key=None, dev=False):
    arg = text
    if dev:
        import torch
        arg = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    cnt, got = one_amd.replace_long(exe, arg, repl, style, bool(lead), mx, chunk_bytes=chunk)
    if dev:
        got = got.cpu().numpy().tobytes()
    want = _expect(blob, text, repl, style, lead, mx, key)
    assert cnt == want[0], (cnt, want[0])
    assert got == want[1]
    return cnt


def _planted(blob, n, chunk, seed, alphabet=True, name=None, every=None):
    """n bytes of text with the matched substrings of a sample planted across chunk borders
    (every `every` bytes when given); DFAs without a pure dead state get their own match, and
    the text ends in one."""
    gen = W.alphabet_bytes if alphabet else W.random_bytes
    a = gen(n, seed).copy()
    if name in CLOSED:
        pieces = [CLOSED[name]]
    else:
        sample = bytes(gen(1 << 14, seed + 1))
        recs, _ = O.CpuOracle(blob).collect(sample, 64)
        pieces = [sample[s:e] for _, s, e in recs if 0 < e - s <= 64]
    if pieces and n:
        for k, b in enumerate(range(every or chunk, n, every or chunk)):
            p = pieces[k % len(pieces)]
            at = b - len(p) // 2 - (k % 3)
            if at >= 0 and at + len(p) <= n:
                a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
        if (name in DENSE or every) and n >= len(pieces[0]):
            a[n - len(pieces[0]):] = np.frombuffer(pieces[0], dtype=np.uint8)
    return bytes(a)


def test_replace_kat_through_replace_long():
    for k in json.load(open(os.path.join(GOLD, "replace_kat.json"))):
        exe = one_amd.Executable(unb64(k["reda"]))
        sty = O.STYLES[k["style"]]
        for chunk in (0, 16, 64, 1024):
            got = one_amd.replace_long(exe, k["text"].encode(), k["repl"].encode(), sty, True,
                                       k["max"], chunk_bytes=chunk)
            assert got == (k["count"], k["expect"].encode()), (k, chunk)
            for c in (1, 2, 3):
                got = one_amd.replace_long(exe, k["text"].encode(), k["repl"].encode(), sty, True,
                                           k["max"], chunk_bytes=c)
                assert got == (k["count"], k["expect"].encode()), (k, c)


@pytest.mark.parametrize("chunk", [16, 64, 1024, 0])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", DEAD)
def test_replace_long_matrix_vs_oracle(name, style, lead, chunk):
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    c = chunk or 256
    for n in (0, 1, c - 1, c, c + 1, 5 * c + 3):
        text = _planted(blob, n, c, 11 + n, name=name)
        _check(exe, blob, text, chunk, style=style, lead=lead, key=(name, "len", c, n))
    n = 5 * c + 3
    text = _planted(blob, n, c, 11 + n, name=name)
    for repl in (b"", b"x", b"<#>", b"0123456789" * 4):
        for mx in (0, 1, 7, ALL):
            _check(exe, blob, text, chunk, repl, style, lead, mx, key=(name, "len", c, n))
    for alphabet in (True, False):
        # (the 3 MiB texts are planted at the automatic chunk size and at 1024: every forced
        # chunk size divides one of them, and their expected outputs are shared)
        text = _planted(blob, 3 << 20, 256 if c <= 256 else 1024, 5, alphabet, name)
        key = (name, "3M", min(max(c, 256), 1024), alphabet)
        _check(exe, blob, text, chunk, style=style, lead=lead, key=key)
        _check(exe, blob, text, chunk, b"", style, lead, key=key)
        _check(exe, blob, text, chunk, b"<#>", style, lead, 7, key=key)


@pytest.mark.parametrize("chunk", [16, 1024, 0])
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", DENSE)
def test_replace_long_dense_dfas(name, style, chunk):
    """No pure dead state: texts of at most 16 KiB, or a match planted every 256 bytes and at the
    end (every failing attempt then dies within a gap), 1 MiB at most - the CPU side stays cheap.
    syn256 under styFull matches only at the end of the text, so every attempt walks to it: 2 KiB
    there (quadratic on the device's one lane as on the CPU, at a global-table load per byte)."""
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    slow = name == "syn256" and style == 5
    for lead in (0, 1):
        for n in (0, 1, 255, 2048) if slow else (0, 1, 255, 4099, 16384):
            text = _planted(blob, n, 256, 3 + n, name=name)
            for repl, mx in ((b"<#>", ALL), (b"", ALL), (b"0123456789" * 4, 7)):
                _check(exe, blob, text, chunk, repl, style, lead, mx, key=(name, "s", n))
    if slow:
        return
    n = 1 << 20 if name != "syn256" else 1 << 18
    text = _planted(blob, n, 256, 17, name=name, every=256)
    for lead in (0, 1):
        _check(exe, blob, text, chunk, style=style, lead=lead, key=(name, "planted"))


@pytest.mark.parametrize("name", DEAD + DENSE)
@pytest.mark.parametrize("style", STYLES)
def test_replace_long_routes(name, style):
    """Automatic chunking, 1 MiB (256 KiB for syn256): chunks for every DFA with a pure dead state
    under every style, and for those without one under the styles whose attempts stop at their
    first accept (Instant) or first non-accept behind one (First, Tangent); one chunk - the chain
    in order on one lane - for those without one under Last and Full, and for short texts."""
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    dense = exe.info["n_pure_dead"] == 0
    assert dense == (name in DENSE)
    if name == "syn256" and style == 5:
        # (every attempt walks to the end of the text: 2 KiB, the short-text route only)
        _check(exe, blob, _planted(blob, 2048, 256, 3, name=name), 0, style=style)
        assert one_amd.last_kernel() == "k_replace_long<one>"
        return
    else:
        text = _planted(blob, (1 << 18) if name == "syn256" else (1 << 20), 256, 3, name=name,
                        every=256 if dense else None)
    _check(exe, blob, text, 0, style=style, key=(name, "route"))
    want = "k_replace_long<one>" if dense and style in (4, 5) else "k_replace_long"
    assert one_amd.last_kernel() == want, one_amd.last_kernel()
    _check(exe, blob, text[:16383], 0, style=style)
    assert one_amd.last_kernel() == "k_replace_long<one>"
    _check(exe, blob, text[:16383], 4096, style=style)
    assert one_amd.last_kernel() == "k_replace_long"


def _span_dfa():
    # "x", any number of "y", "z": 0 = error, 1 = initial, 2 = inside, 3 = accept (then error)
    trans = np.array([[0, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 3], [0, 0, 0, 0]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("x")], equiv[ord("y")], equiv[ord("z")] = 1, 2, 3
    return write_reda(trans, np.array([0, 0, 0, 1]), equiv=equiv, initial=1)


def test_replace_long_match_spanning_many_chunks():
    blob = _span_dfa()
    exe = one_amd.Executable(blob)
    long = b"x" + b"y" * 3000 + b"z"
    text = b"ab" * 333 + long + b"c" * 777 + b"xz" + long + b"d" * 5000 + b"xyyz" + b"e" * 99
    for chunk in (16, 64, 1024, 4096):
        for style in STYLES:
            for repl in (b"", b"R", b"<#>" * 20):
                for mx in (1, 2, ALL):
                    cnt = _check(exe, blob, text, chunk, repl, style, 1, mx, key="span")
                    assert cnt == (0 if style == 5 else min(mx, 4))
        assert one_amd.last_kernel() == "k_replace_long"
    # an attempt that never ends: x and a run of y to the end of the text
    _check(exe, blob, b"q" * 100 + b"x" + b"y" * 100000, 16)
    _check(exe, blob, b"q" * 100 + b"x" + b"y" * 100000 + b"z", 16)


def test_replace_long_dense_matches_and_the_tail_behind_max_count():
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    text = bytes(W.alphabet_bytes(4 << 20, 31))
    full = _check(exe, blob, text, 0, key="dense4M")
    assert one_amd.last_kernel() == "k_replace_long"
    assert full > (4 << 20) // 64          # match-dense: millions of short gaps at 64 MiB
    for mx in (1, 2, 1000):                # nearly all of the text is "tail"
        assert _check(exe, blob, text, 0, mx=mx, key="dense4M") == mx
    _check(exe, blob, text, 0, b"", key="dense4M")
    _check(exe, blob, text, 0, b"0123456789" * 4, key="dense4M", dev=True)
    _check(exe, blob, text, 64, mx=1, key="dense4M")


def _aa_dfa():
    # 0 = error (pure dead end), 1 = initial, 2 = "a", 3 = "aa" (accepts, every byte -> error)
    trans = np.array([[0, 0], [0, 2], [0, 3], [0, 0]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("a")] = 1
    return write_reda(trans, np.array([0, 0, 0, 1]), equiv=equiv, initial=1)


def test_replace_long_chains_that_never_meet():
    """'aa' over a run of a behind one b: the true chain takes odd positions, every warm-up guess
    even ones; the rounds run out and the serial finish walks the rest, exactly."""
    blob = _aa_dfa()
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] >= 1
    text = b"b" + b"a" * ((1 << 20) - 1)
    for chunk in (16, 64):
        for repl in (b"X", b"12345"):
            assert _check(exe, blob, text, chunk, repl, key="aa") == ((1 << 20) - 1) // 2
            assert one_amd.last_kernel() == "k_replace_long"
    _check(exe, blob, b"a" * (1 << 20), 16, b"X")


def test_replace_long_truncation():
    import torch
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    text = _planted(blob, 1 << 20, 64, 9)
    lib = _lib.lib()
    for repl in (b"<#>", b"", b"0123456789" * 4):
        for chunk in (0, 64):
            k, want = _expect(blob, text, repl, 4, 1, ALL, key="trunc")
            assert k > 10
            dtext = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
            for cap in (0, 1, len(want) - 1, len(want)):
                # device form: the guard bytes sit right behind out_cap
                buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                cnt, got, out_len = one_amd.replace_long(exe, dtext, repl, chunk_bytes=chunk,
                                                         out=buf[:cap])
                assert (cnt, out_len) == (k, len(want))
                host = buf.cpu().numpy().tobytes()
                assert host[:cap] == want[:cap]
                assert host[cap:] == b"\xa5" * 64
                # host form
                hbuf = np.full(cap + 64, 0xA5, dtype=np.uint8)
                c, ol = C.c_uint64(0), C.c_uint64(0)
                assert lib.redgpu_replace_long(exe._h, 4, 1, text, len(text), chunk, repl,
                                               len(repl), ALL, C.byref(c), C.byref(ol),
                                               hbuf.ctypes.data, cap) == 0
                assert (c.value, ol.value) == (k, len(want))
                assert hbuf[:cap].tobytes() == want[:cap]
                assert hbuf[cap:].tobytes() == b"\xa5" * 64
            # sizes only
            c, ol = C.c_uint64(0), C.c_uint64(0)
            assert lib.redgpu_replace_long(exe._h, 4, 1, text, len(text), chunk, repl, len(repl),
                                           ALL, C.byref(c), C.byref(ol), None, 0) == 0
            assert (c.value, ol.value) == (k, len(want))


def test_replace_long_unaligned_device_buffers():
    import torch
    blob = load_dfa("set5")
    exe = one_amd.Executable(blob)
    text = _planted(blob, (1 << 18) + 5, 256, 13)
    k, want = _expect(blob, text, b"<#>", 4, 1, ALL)
    for shift_in in (0, 1, 7):
        for shift_out in (0, 3, 15):
            src = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
            src[shift_in:shift_in + len(text)] = torch.from_numpy(
                np.frombuffer(text, dtype=np.uint8).copy()).cuda()
            buf = torch.full((len(want) + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            cnt, got, out_len = one_amd.replace_long(
                exe, src[shift_in:shift_in + len(text)], b"<#>",
                out=buf[shift_out:shift_out + len(want)])
            host = buf.cpu().numpy().tobytes()
            assert (cnt, out_len) == (k, len(want))
            assert host[shift_out:shift_out + len(want)] == want
            assert host[:shift_out] == b"\xa5" * shift_out
            assert host[shift_out + len(want):] == b"\xa5" * (32 - shift_out)


def test_replace_long_device_form_20_mib():
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    n = 20 << 20
    text = _planted(blob, n, 256, 7)
    cnt = _check(exe, blob, text, 0, dev=True)
    assert one_amd.last_kernel() == "k_replace_long"
    assert (n + 255) // 256 > 65536 and cnt > 0


def test_replace_long_second_round_of_block_totals():
    """1,049,602 chunks of 16 bytes are 1,026 blocks of 1024: the scans of the block totals carry
    their sums and the covered-up-to max into a second round, and records lie behind it.  The
    golden newyork DFA is suffix-closed without a pure dead end: under styLast its replace of this
    text is ONE record, and under the styles that stop early every attempt outruns the chunks'
    budget, so one lane walks the text (23 s on an MI355X) - the chunked route gets "New York" as
    an anchored literal: a record per plant."""
    text, chunk, border = scan_round_text()
    assert _expect(load_dfa("newyork"), text, b"<#>", 4, 1, ALL, key="scan_round_golden")[0] == 1
    blob = literal_dfa(b"New York")
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] >= 1
    count, want = _expect(blob, text, b"<#>", 4, 1, ALL, key="scan_round")
    assert count == len(text) // 4096 and len(want) == len(text) - 5 * count
    # replacement k stands 5 k bytes in front of where record k began
    at, starts = want.find(b"<#>"), []
    while at >= 0:
        starts.append(at + 5 * len(starts))
        at = want.find(b"<#>", at + 3)
    assert len(starts) == count and all(text[s:s + 8] == b"New York" for s in starts)
    assert sum(1 for s in starts if s < border) >= 4000
    assert sum(1 for s in starts if s >= border) >= 4
    assert _check(exe, blob, text, chunk, key="scan_round", dev=True) == count
    assert one_amd.last_kernel() == "k_replace_long"


def test_replace_long_two_streams_and_threads():
    import torch
    blob = load_dfa("set5")
    exe = one_amd.Executable(blob)
    texts = [_planted(blob, 2 << 20, 64, s) for s in (21, 22)]
    want = [_expect(blob, t, b"<#>", 4, 1, ALL) for t in texts]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, d in zip(streams, devs):
        with torch.cuda.stream(st):
            outs.append(one_amd.replace_long(exe, d, b"<#>", chunk_bytes=64))
    torch.cuda.synchronize()
    for (cnt, got), w in zip(outs, want):
        assert (cnt, got.cpu().numpy().tobytes()) == w
    errors = []

    def work(t, w):
        try:
            for _ in range(3):
                assert one_amd.replace_long(exe, t, b"<#>", chunk_bytes=128) == w
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(t, w)) for t, w in zip(texts, want)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("dead", [0.0, 0.05])
@pytest.mark.parametrize("chunk", [16, 64, 0])
def test_replace_long_random_dfas(dead, chunk):
    blob = random_dfa(40, 256, 17, dead_frac=dead, accept_frac=0.1)
    exe = one_amd.Executable(blob)
    for n in (1000, 1 << 18):
        text = bytes(W.random_bytes(n, n))
        for style in STYLES:
            if dead == 0.0 and style == 5 and n > 2048:
                # no pure dead state and styFull: every attempt walks to the end of the text, the
                # CPU checker is quadratic (190 s for 2^18 bytes) and so is the device's one lane
                # (80 s for 16 KiB) - 2 KiB, as for syn256
                text = text[:2048]
            for lead in (0, 1):
                _check(exe, blob, text, chunk, style=style, lead=lead,
                       key=("rnd", dead, len(text)))
