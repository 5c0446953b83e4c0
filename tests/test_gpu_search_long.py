"""search_long (redgpu_search_long[_dev]): searchCore over ONE long text, chunk-parallel, the
Outcome bit-exact against the CPU oracle (and the reference when present) for every style, leader
setting and chunk size: texts without a match, a match at each place a chunk layout can put it,
the lowest start winning over matches that finish first, attempts that never die (the bounded
walk and the serial finish), DFAs without a pure dead state, the routes, random DFAs, the device
form, concurrent streams and threads."""
import ctypes as C
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from one_amd import workloads as W
from oracle.reda_writer import random_dfa, write_reda
from golden_util import kat_items, load_dfa, unb64

pytestmark = pytest.mark.gpu

DEAD = ["num3", "set5", "log100", "aab", "ale", "num3defg"]   # DFAs with a pure dead state
DENSE = ["newyork", "uri", "syn256"]                          # ... and without one
STYLES = [1, 2, 3, 4, 5]
CLOSED = {"newyork": b"New York", "uri": b"http://www.example.com/index.html"}
FILL = 0x01                                                   # a byte no DFA here starts with
KNOWN = {"aab": [b"aab"], "ale": [b"aleee", b"alex", b"aleeex"], "num3": [b"123", b"4567"],
         "num3defg": [b"123", b"45d", b"6789defg"]}

_cache = {}
_oracles = {}
_pieces_of = {}
_blank_of = {}


def _expect(tag, blob, text, style, lead):
    """(result, start, end) of the CPU oracle, checked against the reference when it is built;
    cached per DFA tag and text, so a chunk-size sweep computes it once."""
    k = (tag, text, style, lead)
    if k not in _cache:
        if tag not in _oracles:
            _oracles[tag] = (O.CpuOracle(blob), O.Reference(blob) if O.have_ref() else None)
        cpu, ref = _oracles[tag]
        want = tuple(int(v) for v in cpu.search(text, style, bool(lead)))
        if ref is not None:
            assert tuple(int(v) for v in ref.search(text, style, bool(lead))) == want
        _cache[k] = want
    return _cache[k]


def _check(exe, tag, blob, text, chunk, style=4, lead=1):
    got = one_amd.search_long(exe, text, style, bool(lead), chunk_bytes=chunk)
    want = _expect(tag, blob, text, style, lead)
    assert got == want, (tag, len(text), chunk, style, lead, got, want)
    return got


def _pieces(name, blob):
    """matched substrings of at most 64 bytes: what a text is planted with"""
    if name not in _pieces_of:
        if name in CLOSED:
            p = [CLOSED[name]]
        elif name == "log100":
            p = [h.rstrip() for h in W.log100_heads()[:7]]
        else:
            sample = bytes(W.alphabet_bytes(1 << 14, 12))
            cpu = O.CpuOracle(blob)
            recs, _ = cpu.collect(sample, 64)
            p = KNOWN.get(name, []) + [sample[s:e] for _, s, e in recs if 0 < e - s <= 64]
            assert all(cpu.search(k, 4, False)[0] > 0 for k in KNOWN.get(name, [])), name
        assert p, name
        _pieces_of[name] = p
    return _pieces_of[name]


def _blank(name, blob, n, seed):
    """n alphabet bytes with every match overwritten: no attempt of any style, with or without
    the leader, ever reaches an accepting state (styInstant without the leader finds nothing)."""
    if (name, n) not in _blank_of:
        a = W.alphabet_bytes(n, seed).copy()
        cpu = O.CpuOracle(blob)
        while True:
            r, s, e = cpu.search(bytes(a), 1, False)
            if r == 0:
                break
            a[min(s, e - 1):e] = FILL
        _blank_of[(name, n)] = a
    return _blank_of[(name, n)]


def _placed(name, blob, n, c, seed):
    """the texts of one shape: no match at all, and the only planted match at position 0,
    straddling a chunk border, wholly in the last chunk, ending at the last byte"""
    base = _blank(name, blob, n, seed)
    out = [bytes(base)]
    pieces = _pieces(name, blob)
    last = ((n - 1) // c) * c if n else 0
    for k, at_of in enumerate((lambda L: 0, lambda L: c * max(1, (n - 1) // c // 2) - L // 2,
                               lambda L: last, lambda L: n - L)):
        p = pieces[k % len(pieces)]
        at = at_of(len(p))
        if at < 0 or at + len(p) > n:
            continue
        a = base.copy()
        a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
        out.append(bytes(a))
    return out


def _planted(blob, n, chunk, seed, alphabet=True, name=None, every=None):
    """n bytes of text with matched substrings planted across chunk borders (every `every` bytes
    when given); DFAs without a pure dead state get their own match, and the text ends in one."""
    gen = W.alphabet_bytes if alphabet else W.random_bytes
    a = gen(n, seed).copy()
    pieces = _pieces(name, blob)
    if n:
        for k, b in enumerate(range(every or chunk, n, every or chunk)):
            p = pieces[k % len(pieces)]
            at = b - len(p) // 2 - (k % 3)
            if at >= 0 and at + len(p) <= n:
                a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
        if (name in DENSE or every) and n >= len(pieces[0]):
            a[n - len(pieces[0]):] = np.frombuffer(pieces[0], dtype=np.uint8)
    return bytes(a)


def test_search_kat_through_search_long():
    n = 0
    for name, fmt, blob, calls in kat_items():
        exe = one_amd.Executable(blob)
        tag = ("kat", name, fmt)
        for text in sorted({unb64(c["text"]) for c in calls}):
            for style in STYLES:
                for chunk in (0, 1, 2, 3, 16, 64):
                    _check(exe, tag, blob, text, chunk, style, 1)
                    n += 1
    assert n > 400


@pytest.mark.parametrize("chunk", [16, 64, 1024, 0])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", DEAD)
def test_search_long_matrix_vs_oracle(name, style, lead, chunk):
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    c = chunk or 256
    found = 0
    for n in (0, 1, c - 1, c, c + 1, 5 * c + 3):
        texts = _placed(name, blob, n, c, 11 + n)
        assert _expect(name, blob, texts[0], 1, 0)[0] == 0      # the generator's own promise
        assert _check(exe, name, blob, texts[0], chunk, style, lead) == (0, 0, 0)
        for text in texts[1:]:
            found += _check(exe, name, blob, text, chunk, style, lead)[0] > 0
    if style != 5:
        assert found > 0            # (styFull needs the match to end the text)


def test_search_long_lowest_start_wins_a_match_in_every_chunk():
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    n = 1 << 20
    for chunk in (16, 1024):
        a = np.full(n, FILL, dtype=np.uint8)
        pieces = [p for p in _pieces("num3", blob) if len(p) <= 12]
        for k, b in enumerate(range(chunk, n, chunk)):
            p = pieces[k % len(pieces)]
            at = b - len(p) // 2
            a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
        text = bytes(a)
        for style in STYLES:
            got = _check(exe, "num3", blob, text, chunk, style, 1)
            assert one_amd.last_kernel() == "k_search_long"
            if style != 5:
                assert got[0] > 0 and got[2] <= 2 * chunk, got   # the first chunk's


def _span_dfa():
    # "x", any number of "y", "z": 0 = error, 1 = initial, 2 = inside, 3 = accept (then error)
    trans = np.array([[0, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 3], [0, 0, 0, 0]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("x")], equiv[ord("y")], equiv[ord("z")] = 1, 2, 3
    return write_reda(trans, np.array([0, 0, 0, 1]), equiv=equiv, initial=1)


def test_search_long_long_match_that_starts_first_wins():
    blob = _span_dfa()
    exe = one_amd.Executable(blob)
    text = b"q" * 100 + b"x" + b"y" * 3000 + b"z" + b"xz" * 2000
    for chunk in (16, 64):
        for style in STYLES:
            for lead in (0, 1):
                got = _check(exe, "span", blob, text, chunk, style, lead)
                assert one_amd.last_kernel() == "k_search_long"
                if style != 5:
                    assert got == (1, 100, 3102), got


def test_search_long_attempts_that_never_die():
    """x and a run of y to the end of the text: the chunk that owns x runs out of its budget,
    the serial finish walks the attempt to its end - a match with the trailing z, none without."""
    blob = _span_dfa()
    exe = one_amd.Executable(blob)
    for tail in (b"", b"z"):
        text = b"q" * 100 + b"x" + b"y" * 100000 + tail
        for style in STYLES:
            got = _check(exe, "span", blob, text, 16, style, 1)
            assert got == ((1, 100, len(text)) if tail else (0, 0, 0)), got
    assert one_amd.last_kernel() == "k_search_long"


@pytest.mark.parametrize("chunk", [16, 1024, 0])
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("name", DENSE)
def test_search_long_dense_dfas(name, style, chunk):
    """No pure dead state: texts of at most 16 KiB, or a match planted every 256 bytes and at the
    end, 1 MiB at most; syn256 under styFull matches only at the end of the text, so every attempt
    walks to it: 2 KiB there (quadratic on the device's one lane as on the CPU)."""
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    slow = name == "syn256" and style == 5
    for lead in (0, 1):
        for n in (0, 1, 255, 2048) if slow else (0, 1, 255, 4099, 16384):
            _check(exe, name, blob, _planted(blob, n, 256, 3 + n, name=name), chunk, style, lead)
    if slow:
        return
    n = 1 << 20 if name != "syn256" else 1 << 18
    text = _planted(blob, n, 256, 17, name=name, every=256)
    for lead in (0, 1):
        _check(exe, name, blob, text, chunk, style, lead)


def test_search_long_routes():
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    text = _planted(blob, 1 << 16, 256, 3, name="num3")
    _check(exe, "num3", blob, text, 0)
    assert one_amd.last_kernel() == "k_search_long"
    _check(exe, "num3", blob, text[:16383], 0)
    assert one_amd.last_kernel() == "k_search_long<one>"
    _check(exe, "num3", blob, text[:16383], 4096)
    assert one_amd.last_kernel() == "k_search_long"
    _check(exe, "num3", blob, b"", 0)
    assert one_amd.last_kernel() == "k_search_long<one>"
    blob = load_dfa("newyork")
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] == 0
    text = _planted(blob, 1 << 16, 256, 3, name="newyork", every=256)
    for lead in (0, 1):
        _check(exe, "newyork", blob, text, 0, 4, lead)
        assert one_amd.last_kernel() == "k_search_long<one>"
    # without a pure dead state the styles that stop behind an accept still take chunks, unless
    # the DFA is suffix-closed and searched without a leader: that search is one anchored walk
    _check(exe, "newyork", blob, text, 0, 1, 0)
    assert exe.info["suffix_closed"] and one_amd.last_kernel() == "k_search_long<one>"
    blob = load_dfa("syn256")
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] == 0 and not exe.info["suffix_closed"]
    text = _planted(blob, 1 << 16, 256, 3, name="syn256", every=256)
    for style, want in ((1, "k_search_long"), (2, "k_search_long"), (3, "k_search_long"),
                        (4, "k_search_long<one>")):
        _check(exe, "syn256", blob, text, 0, style, 1)
        assert one_amd.last_kernel() == want, (style, one_amd.last_kernel())


@pytest.mark.parametrize("dead", [0.3, 0.0])
@pytest.mark.parametrize("chunk", [16, 0])
def test_search_long_random_dfas(dead, chunk):
    blob = random_dfa(40, 256, 17, dead_frac=dead, accept_frac=0.1)
    exe = one_amd.Executable(blob)
    assert (exe.info["n_pure_dead"] > 0) == (dead > 0)
    tag = ("rnd", dead)
    for n in (1000, 1 << 16) if dead else (1000, 1 << 12):
        text = bytes(W.random_bytes(n, n))
        for style in STYLES:
            for lead in (0, 1):
                _check(exe, tag, blob, text, chunk, style, lead)


def _late_match_text(n, at):
    """log100 finds nothing in alphabet text: the only match is the one planted at `at`"""
    a = W.alphabet_bytes(n, 5).copy()
    p = _pieces("log100", load_dfa("log100"))[0]
    a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return bytes(a)


def test_search_long_device_form_8_mib():
    import torch
    blob = load_dfa("log100")
    exe = one_amd.Executable(blob)
    n = 8 << 20
    text = _late_match_text(n, (7 << 20) + 12345)
    host = _check(exe, "log100", blob, text, 0)
    assert one_amd.last_kernel() == "k_search_long"
    assert host[0] > 0 and host[1] == (7 << 20) + 12345
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for chunk in (0, 4096):
        got = one_amd.search_long(exe, dev, chunk_bytes=chunk)
        assert all(g.is_cuda and g.numel() == 1 for g in got)
        assert tuple(int(g.item()) for g in got) == host
    # no match at all: every chunk walked, 0 / 0 / 0
    none = torch.from_numpy(W.alphabet_bytes(n, 5).copy()).cuda()
    assert tuple(int(g.item()) for g in one_amd.search_long(exe, none)) == (0, 0, 0)


def test_search_long_unaligned_device_pointers_and_null_positions():
    import torch
    blob = load_dfa("set5")
    exe = one_amd.Executable(blob)
    lib = _lib.lib()
    n = (1 << 18) + 5
    base = np.full(n, FILL, dtype=np.uint8)
    p = _pieces("set5", blob)[0]
    base[n - 1000:n - 1000 + len(p)] = np.frombuffer(p, dtype=np.uint8)
    text = bytes(base)
    want = _expect("set5", blob, text, 4, 1)
    assert want[0] > 0
    stream = torch.cuda.current_stream().cuda_stream
    for shift in (0, 1, 7):
        src = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        src[shift:shift + n] = torch.from_numpy(base).cuda()
        got = one_amd.search_long(exe, src[shift:shift + n])
        assert tuple(int(g.item()) for g in got) == want
        # result only: start and end NULL
        res = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        assert lib.redgpu_search_long_dev(exe._h, 4, 1, src.data_ptr() + shift, n, 0,
                                          res.data_ptr() + 4, None, None, stream) == 0
        assert res.tolist() == [-7, want[0], -7]
    r = C.c_int32(-7)
    assert lib.redgpu_search_long(exe._h, 4, 1, text, n, 64, C.byref(r), None, None) == 0
    assert r.value == want[0]


def test_search_long_two_streams_and_threads():
    import torch
    blob = load_dfa("log100")
    exe = one_amd.Executable(blob)
    texts = [_late_match_text(2 << 20, at) for at in ((1 << 20) + 77, (2 << 20) - 4000)]
    want = [_expect("log100", blob, t, 4, 1) for t in texts]
    assert all(w[0] > 0 for w in want) and want[0] != want[1]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, d in zip(streams, devs):
        with torch.cuda.stream(st):
            outs.append(one_amd.search_long(exe, d, chunk_bytes=64))
    torch.cuda.synchronize()
    for got, w in zip(outs, want):
        assert tuple(int(g.item()) for g in got) == w
    errors = []

    def work(t, w):
        try:
            for _ in range(3):
                assert one_amd.search_long(exe, t, chunk_bytes=128) == w
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(t, w)) for t, w in zip(texts, want)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_search_long_leader_in_front_of_an_accepting_initial_state():
    """searchCore starts from the initial state's result (Matcher.h:571) and keeps it when no
    position passes the leader test: result > 0 with start = end = 0.  One attempt that runs, even
    a failing one, clears it.  "ab" with an initial state that accepts, leader "a"."""
    trans = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 3], [0, 0, 0]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("a")], equiv[ord("b")] = 1, 2
    blob = write_reda(trans, np.array([0, 2, 0, 1]), equiv=equiv, initial=1, leader=bytes([1]),
                      leader_next=2)
    exe = one_amd.Executable(blob)
    assert exe.info["leader_len"] == 1
    for n in (40, 1 << 15):
        none = b"q" * n
        ran = b"q" * (n - 9) + b"a" + b"q" * 8            # the test passes once, the attempt fails
        hit = b"q" * (n // 2) + b"aq" + b"q" * 7 + b"ab" + b"q" * 5
        for chunk in (16, 64, 0):
            for style in STYLES:
                assert _check(exe, "initacc", blob, none, chunk, style, 1) == (2, 0, 0)
                assert _check(exe, "initacc", blob, none, chunk, style, 0) == (0, 0, 0)
                assert _check(exe, "initacc", blob, ran, chunk, style, 1) == (0, 0, 0)
                for lead in (0, 1):
                    _check(exe, "initacc", blob, hit, chunk, style, lead)
            if n > 16384 or chunk:
                assert one_amd.last_kernel() == "k_search_long"
