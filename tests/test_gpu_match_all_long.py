"""match_all_long (redgpu_match_all_long[_dev]): matchAll over ONE long text, chunk-parallel,
bit-exact against the CPU oracle (and, with do_leader, the reference when it is built) - count,
results, starts, ends - across chunk borders, forced and automatic chunk sizes, runs and starts
that span many chunks, DFAs whose entry guesses never converge (the serial finish), every table
placement, truncation at cap, the one-lane routes and concurrent streams.

What keeps the file from passing vacuously is asserted on the ORACLE's output when a text is
built, and on one_amd.last_kernel() after every call."""
import json
import os
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import workloads as W
from oracle.reda_writer import random_dfa, write_reda
from golden_util import GOLD, load_dfa, scan_round_text, unb64

pytestmark = pytest.mark.gpu

N = 65536 + 5            # 4097 chunks of 16, 66 of 1000, 257 of the automatic 256
MIN_AUTO = 16384         # below it the automatic size stays on one lane
FILL = 0x01              # a byte no regex DFA here starts with
PIECES = {
    "uri": W.URI_PLANT.rstrip(),
    "uri_user": W.URI_USER_PLANT.rstrip(),
    "uri_v6": W.URI_V6_PLANT.rstrip(),
    "newyork": b"New York",
}


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _dev(text):
    import torch
    return torch.from_numpy(_u8(text).copy()).cuda()


def _planted(n, piece):
    """n fill bytes with `piece` centred on every multiple of 1000 and of 768, jittered"""
    a = np.full(n, FILL, dtype=np.uint8)
    borders = sorted(set(range(1000, n, 1000)) | set(range(768, n, 768)))
    for k, b in enumerate(borders):
        at = b - len(piece) // 2 - k % 3
        if at >= 0 and at + len(piece) <= n:
            a[at:at + len(piece)] = _u8(piece)
    return bytes(a)


class _Dfa:
    """a blob with its checkers; expectations are computed once per (text, leader)"""

    def __init__(self, blob):
        self.blob = blob
        self.cpu = O.CpuOracle(blob)
        self.ref = O.Reference(blob) if O.have_ref() else None
        self.memo = {}

    def expect(self, text, lead):
        key = (text, bool(lead))
        if key not in self.memo:
            recs, k = self.cpu.match_all(text, bool(lead), 4096)
            if k > len(recs):
                recs, k = self.cpu.match_all(text, bool(lead), k)
            assert len(recs) == k
            if self.ref is not None and lead:
                ref, rk = self.ref.match_all(text, max(k, 1))
                assert rk == k and ref[:k] == recs
            self.memo[key] = recs
        return self.memo[key]

    def expect_cap(self, text, lead, cap):
        """the checkers' own truncation: record cap - 1 carries its final end"""
        recs, k = self.cpu.match_all(text, bool(lead), max(cap, 1))
        assert k == len(self.expect(text, lead))
        return recs[:cap]


_dfas = {}


def _dfa(name, make=None):
    if name not in _dfas:
        _dfas[name] = _Dfa(make() if make else load_dfa(name))
    return _dfas[name]


def _route(n, chunk):
    return "k_matchall" if n == 0 or (not chunk and n < MIN_AUTO) else "k_match_all_long"


def _check(exe, d, text, chunk, lead, *, cap=None, dev=False, route=None):
    cnt, r, s, e = one_amd.match_all_long(exe, _dev(text) if dev else text, cap, bool(lead),
                                          chunk_bytes=chunk)
    kernel = one_amd.last_kernel()
    if dev:
        r, s, e = r.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()
    recs = d.expect(text, lead)
    what = (len(text), chunk, lead, cap, dev, kernel)
    assert cnt == len(recs), what + (cnt, len(recs))
    got = list(zip(r.tolist(), s.tolist(), e.tolist()))
    assert got == (recs if cap is None else d.expect_cap(text, lead, cap)), what
    assert kernel == (route or _route(len(text), chunk)), what
    return cnt


def _border_records(recs, c):
    return sum(1 for _, s, e in recs if s // c != (e - 1) // c)


# ---- 1. the golden known answers through the long path ------------------------------------------
def test_match_all_kat_through_match_all_long():
    for k in json.load(open(os.path.join(GOLD, "matchall_kat.json"))):
        blob, text = unb64(k["reda"]), unb64(k["text"])
        exe = one_amd.Executable(blob)
        want = [tuple(x) for x in k["expect"]]
        assert one_amd.match_all(exe, text) == want, k["src"]
        for chunk in (0, 1, 3, 16):
            cnt, r, s, e = one_amd.match_all_long(exe, text, chunk_bytes=chunk)
            assert one_amd.last_kernel() == _route(len(text), chunk)
            assert list(zip(r.tolist(), s.tolist(), e.tolist())) == want and cnt == len(want), \
                (k["src"], chunk)


# ---- 2. lengths around the chunk size, planted texts ---------------------------------------------
@pytest.mark.parametrize("chunk", [16, 64, 1000, 0])
@pytest.mark.parametrize("name", ["uri", "uri_user", "uri_v6", "newyork", "syn256"])
def test_match_all_long_lengths_vs_oracle(name, chunk):
    d = _dfa(name)
    exe = one_amd.Executable(d.blob)
    c = chunk or 256

    def text(n):
        return bytes(W.random_bytes(n, 7)) if name == "syn256" else _planted(n, PIECES[name])

    full = text(N)
    for lead in (False, True):
        recs = d.expect(full, lead)
        if name == "syn256":
            assert len(recs) >= 5000, len(recs)
        else:
            assert len(recs) >= 250, (name, lead, len(recs))
            assert _border_records(recs, c) >= 60, (name, lead, c, _border_records(recs, c))
    for n in (0, 1, c - 1, c, c + 1, 5 * c + 3, N):
        t = full if n == N else text(n)
        for lead in (False, True):
            for dev in (False, True):
                _check(exe, d, t, chunk, lead, dev=dev)
    assert _route(N, chunk) == "k_match_all_long"


# ---- 3. runs and starts that span many chunks: a word set ----------------------------------------
WORDS = [b"ab", b"abc", b"b", b"cab", b"hhhh", b"a"]


def _wordset_dfa():
    """Aho-Corasick as a dense DFA over the classes of abcdefgh + other; state 0 = error, 1 = the
    root; word k has result k + 1, inherited along failure links"""
    goto, out = [{}], [0]
    for r, w in enumerate(WORDS, 1):
        s = 0
        for ch in w:
            ch -= ord("a")
            if ch not in goto[s]:
                goto[s][ch] = len(goto)
                goto.append({})
                out.append(0)
            s = goto[s][ch]
        out[s] = r
    n = len(goto)
    delta = np.zeros((n, 9), dtype=np.int64)     # class 8 (other) -> the root
    fail = [0] * n
    queue = []
    for ch in range(8):
        t = goto[0].get(ch, 0)
        delta[0, ch] = t
        if t:
            queue.append(t)
    while queue:
        s = queue.pop(0)
        if not out[s]:
            out[s] = out[fail[s]]
        for ch in range(8):
            t = goto[s].get(ch)
            if t is None:
                delta[s, ch] = delta[fail[s], ch]
            else:
                fail[t] = delta[fail[s], ch]
                delta[s, ch] = t
                queue.append(t)
    trans = np.zeros((n + 1, 9), dtype=np.int64)
    trans[1:] = delta + 1
    equiv = np.full(256, 8, dtype=np.uint8)
    equiv[ord("a"):ord("a") + 8] = np.arange(8, dtype=np.uint8)
    return write_reda(trans, np.array([0] + out), equiv=equiv, initial=1)


def _wordset_texts():
    return (b"h" * 5000 + b"abcab" + b"a" * 3000,
            bytes((W.random_bytes(1 << 14, 3) % 8 + ord("a")).astype(np.uint8)))


@pytest.mark.parametrize("chunk", [1, 7, 16, 64, 4096])
def test_match_all_long_word_set(chunk):
    d = _dfa("wordset", _wordset_dfa)
    exe = one_amd.Executable(d.blob)
    runs, rnd = _wordset_texts()
    recs = d.expect(runs, True)
    assert len(recs) == 7 and max(e - s for _, s, e in recs) >= 2000, recs
    assert recs[0] == (5, 0, 5000) and recs[-1][2] == len(runs)
    assert len(d.expect(rnd, True)) >= 3000
    for t in (runs, rnd):
        for lead in (False, True):
            _check(exe, d, t, chunk, lead)
        _check(exe, d, t, chunk, True, dev=True)


# ---- 4. random DFAs (the serial finish at chunk 16) and placements --------------------------------
_ND = dict(dead_frac=0.0, accept_frac=0.1)
HOT40 = dict(force_hot=True, lds_table_max=40 * 256)
RANDOM = {
    "rnd270nd": lambda: random_dfa(270, 256, 4, **_ND),
    "rnd270half": lambda: random_dfa(270, 256, 4, dead_frac=0.0, accept_frac=0.5, max_result=2),
    "rnd1500nd": lambda: random_dfa(1500, 40, 91, **_ND),
    "rnd80knd": lambda: random_dfa(80000, 4, 5, **_ND),
    "log100": lambda: load_dfa("log100"),
}


def _row(dfa, opts, kind):
    tag = "+".join("%s=%s" % (k, v) if v is not True else k for k, v in opts.items()) or "default"
    return pytest.param(dfa, opts, kind, id="%s-%s-kind%d" % (dfa, tag, kind))


ROWS = [
    _row("rnd270nd", {}, 2),
    _row("rnd270nd", dict(force_global=True), 4),
    _row("rnd270nd", HOT40, 6),
    _row("rnd270half", {}, 2),
    _row("rnd1500nd", {}, 3),
    _row("rnd80knd", {}, 5),
    _row("log100", {}, 7),
    _row("log100", dict(force_global=True), 4),
]


@pytest.mark.parametrize("dfa,opts,kind", ROWS)
def test_match_all_long_under_placement(dfa, opts, kind):
    d = _dfa(dfa, RANDOM[dfa])
    exe = one_amd.Executable(d.blob, **opts)
    assert exe.info["table_kind"] == kind, (dfa, opts, exe.info["table_kind"])
    text = bytes(W.random_bytes(N, 7))
    if dfa != "log100":
        assert exe.info["n_pure_dead"] == 0
        for lead in (False, True):
            assert len(d.expect(text, lead)) >= 1000, (dfa, lead)
    for chunk in (16, 1000, 0):
        for lead in (False, True):
            _check(exe, d, text, chunk, lead)
    _check(exe, d, text, 16, True, dev=True)


# ---- 5. walks that die, and the leader -----------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 0])
def test_match_all_long_dead_walks_and_leader(chunk):
    d = _dfa("rnd270dead", lambda: random_dfa(270, 256, 4, dead_frac=0.05, accept_frac=0.1))
    exe = one_amd.Executable(d.blob)
    assert exe.info["n_pure_dead"] >= 1
    text = bytes(W.random_bytes(N, 7))
    for lead in (False, True):
        _check(exe, d, text, chunk, lead)

    d = _dfa("log100")
    exe = one_amd.Executable(d.blob)
    text = W.log100_heads()[0].rstrip() + b"\x01" * 5000
    assert d.expect(text, True) == [(1, 0, 22), (1, 0, 29)]
    for lead in (False, True):
        _check(exe, d, text, chunk, lead)

    d = _dfa("num3")
    exe = one_amd.Executable(d.blob)
    assert exe.info["leader_len"] == 1
    hit, miss = b"1234567 " + b"\x01" * 70000, b"x1234567 " + b"\x01" * 70000
    assert d.expect(hit, True) == [(1, 0, 7)] and d.expect(miss, True) == []
    for t in (hit, miss):
        for lead in (False, True):
            _check(exe, d, t, chunk, lead)
            _check(exe, d, t, chunk, lead, dev=True)


# ---- 6. routes -----------------------------------------------------------------------------------
def _leaky_dead_end_dfa():
    """0 = error, 1 = initial, 2 = flagged a dead end although 'a' leads out of it, 3 = accepts:
    the walk stops at state 2 (Matcher.h:755-756), which a chunked walk would not see"""
    #                  other a  b
    trans = np.array([[0, 0, 0], [1, 3, 2], [2, 3, 2], [1, 3, 2]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("a")], equiv[ord("b")] = 1, 2
    return write_reda(trans, np.array([0, 0, 0, 1]), equiv=equiv, initial=1,
                      dead_end=np.array([True, False, True, False]))


def test_match_all_long_routes():
    d = _dfa("uri")
    exe = one_amd.Executable(d.blob)
    full = _planted(N, PIECES["uri"])
    for n, chunk, route in ((1000, 0, "k_matchall"), (0, 0, "k_matchall"), (0, 16, "k_matchall"),
                            (N, 0, "k_match_all_long"), (1000, 16, "k_match_all_long"),
                            (1000, 1000, "k_match_all_long"), (N, 1 << 20, "k_match_all_long")):
        _check(exe, d, full[:n], chunk, True, route=route)
    # a flagged dead end with a way out: one lane, whatever the chunk size
    d = _dfa("leaky", _leaky_dead_end_dfa)
    exe = one_amd.Executable(d.blob)
    assert exe.info["n_pure_dead"] >= 1
    text = b"aab" + b"a" * 20000 + b"xaab"
    assert d.expect(text, True) == [(1, 0, 2)]      # nothing behind the b is seen
    for chunk in (0, 16, 1000):
        for lead in (False, True):
            _check(exe, d, text, chunk, lead, route="k_matchall")
    _check(exe, d, text, 16, True, dev=True, route="k_matchall")


# ---- 7. cap ---------------------------------------------------------------------------------------
def test_match_all_long_cap():
    d = _dfa("uri")
    exe = one_amd.Executable(d.blob)
    text = _planted(N, PIECES["uri"])
    count = len(d.expect(text, True))
    assert count > 11
    for chunk in (16, 0):
        for cap in (0, 1, 10, count - 1, count):
            for dev in (False, True):
                assert _check(exe, d, text, chunk, True, cap=cap, dev=dev) == count
    # record cap - 1 gets its final end although its run crosses hundreds of chunk borders
    d = _dfa("wordset", _wordset_dfa)
    exe = one_amd.Executable(d.blob)
    runs, rnd = _wordset_texts()
    assert d.expect_cap(runs, True, 1) == [(5, 0, 5000)]
    assert d.expect_cap(runs, True, 7)[6][2] == len(runs)
    for cap in (0, 1, 2, 6, 7, 8):
        _check(exe, d, runs, 7, True, cap=cap)
    count = len(d.expect(rnd, True))
    for cap in (1, 100, count - 1, count):
        _check(exe, d, rnd, 7, True, cap=cap)
        _check(exe, d, rnd, 7, True, cap=cap, dev=True)


# ---- 8. many chunks at the automatic size ---------------------------------------------------------
def test_match_all_long_many_chunks_automatic():
    """20 MiB on the automatic route: 256-byte chunks on 256 CUs, i.e. more than 64 Ki chunks."""
    d = _dfa("uri")
    exe = one_amd.Executable(d.blob)
    n = 20 << 20
    text = _planted(n, PIECES["uri"])
    cnt = _check(exe, d, text, 0, True, dev=True)
    assert one_amd.last_kernel() == "k_match_all_long"
    assert (n + 255) // 256 > 65536 and cnt > 100000


# ---- 9. two streams, two host threads -------------------------------------------------------------
def test_match_all_long_two_streams_and_threads():
    import torch
    d = _dfa("uri")
    exe = one_amd.Executable(d.blob)
    texts = [bytes([FILL]) * k + _planted(2 << 20, PIECES["uri"]) for k in (0, 77)]
    want = [d.expect(t, True) for t in texts]
    assert all(len(w) > 1000 for w in want) and want[0] != want[1]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [_dev(t) for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, t in zip(streams, devs):
        with torch.cuda.stream(st):
            outs.append(one_amd.match_all_long(exe, t, chunk_bytes=64))
    torch.cuda.synchronize()
    for (cnt, r, s, e), recs in zip(outs, want):
        assert cnt == len(recs)
        assert list(zip(r.cpu().tolist(), s.cpu().tolist(), e.cpu().tolist())) == recs
    errors = []

    def work(t, recs):
        try:
            for _ in range(3):
                cnt, r, s, e = one_amd.match_all_long(exe, t, chunk_bytes=64)
                assert cnt == len(recs)
                assert list(zip(r.tolist(), s.tolist(), e.tolist())) == recs
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(t, w)) for t, w in zip(texts, want)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ---- 10. rounds or serial lane: how a call resolved its chunks -------------------------------------
def _resolved(exe, text, chunk):
    """redgpu_diag_match_all_long_dev after one device call: (rewalked per round, first chunk
    still open or None, chunks the serial lane walked, chunks)"""
    import torch
    from one_amd import _lib
    d = _dev(text)
    one_amd.match_all_long(exe, d, 0, True, chunk_bytes=chunk)
    assert one_amd.last_kernel() == "k_match_all_long"
    stats = torch.zeros(8, dtype=torch.int32, device=d.device)
    rc = _lib.lib().redgpu_diag_match_all_long_dev(exe._h, stats.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().redgpu_last_error()
    s = stats.cpu().tolist()
    assert s[5] == 1
    return s[0:4], None if s[4] == s[7] else s[4], s[6], s[7]


def test_match_all_long_rounds_or_serial_lane():
    # num3 behind its only match: the text is fill bytes, over which the walk from the initial
    # state - the 64 warm-up bytes of every guess - and the true walk both sit in a dead end, and
    # the DFA has one pure dead end only, so every guessed entry is the true one: nothing is
    # walked again, in the rounds or on the serial lane
    d = _dfa("num3")
    exe = one_amd.Executable(d.blob)
    assert exe.info["n_pure_dead"] == 1
    text = b"1234567 " + bytes([FILL]) * 70000
    for walk in (text[:192], text[192:256]):
        st = np.full(1, O.STATE_INITIAL, dtype=np.uint32)
        d.cpu.advance_batch(_u8(walk), st, offsets=[0, len(walk)])
        nxt = np.full(256, st[0], dtype=np.uint32)
        res = d.cpu.advance_batch(np.arange(256, dtype=np.uint8), nxt, stride=1, n=256)
        assert (nxt == st[0]).all() and (res == 0).all()
    for chunk in (0, 16):
        chunks = (len(text) + (chunk or 256) - 1) // (chunk or 256)
        assert _resolved(exe, text, chunk) == ([0, 0, 0, 0], None, 0, chunks)
    # the serial lane has work exactly when the rounds left a chunk open
    d = _dfa("uri")
    exe = one_amd.Executable(d.blob)
    rounds, first, serial, chunks = _resolved(exe, _planted(N, PIECES["uri"]), 0)
    assert chunks == 257 and (serial > 0) == (first is not None), (rounds, first, serial)
    # a random dense DFA of 270 states forgets its entry slowly: two walks over the same bytes
    # merge with a chance of about 1/270 per byte, so after the 64 warm-up bytes about 4 in 5
    # guesses are wrong, every round adds one 16-byte chunk to what an entry was derived from, and
    # after four rounds (128 bytes) about 3 in 5 chunks are still left to the serial lane (a CPU
    # model of the same steps: 3204, 3026, 2856, 2674 queued, first open chunk 13, 2510 on the
    # serial lane).  Asserted with room: half the chunks per round, a quarter on the serial lane.
    d = _dfa("rnd270nd", RANDOM["rnd270nd"])
    exe = one_amd.Executable(d.blob)
    rounds, first, serial, chunks = _resolved(exe, bytes(W.random_bytes(N, 7)), 16)
    assert chunks == 4097 and all(q >= 2048 for q in rounds), rounds
    assert first is not None and serial >= 1024, (first, serial)
    # the one-lane route leaves nothing to ask about
    import torch
    from one_amd import _lib
    one_amd.match_all_long(exe, _dev(b"abc"), 0, True)
    assert one_amd.last_kernel() == "k_matchall"
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert _lib.lib().redgpu_diag_match_all_long_dev(
        exe._h, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == _lib.EAPI


# ---- 11. more than 1024 * 1024 chunks: the block totals' second round of 1024 --------------------
def test_match_all_long_second_round_of_block_totals():
    """1,049,602 chunks of 16 bytes are 1,026 blocks of 1024: the scan of the block totals carries
    its sum and its max into a second round, and records open behind it."""
    text, chunk, border = scan_round_text()
    d = _dfa("newyork")
    exe = one_amd.Executable(d.blob)
    recs = d.expect(text, True)
    assert sum(1 for _, s, _ in recs if s < border) >= 4000
    assert sum(1 for _, s, _ in recs if s >= border) >= 4
    assert _check(exe, d, text, chunk, True, dev=True, route="k_match_all_long") == len(recs)
