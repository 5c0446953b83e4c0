"""collect_long (redgpu_collect_long[_dev]): Red::collect over ONE long text, chunk-parallel,
bit-exact against the CPU oracle (and the reference when present) - count, results, starts, ends
- across chunk borders, forced and automatic chunk sizes, the one-lane and suffix-closed routes,
chains that never resynchronise, truncation and concurrent streams."""
import json
import os
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import workloads as W
from oracle.reda_writer import random_dfa, write_reda
from golden_util import GOLD, literal_dfa, load_dfa, scan_round_text, unb64

pytestmark = pytest.mark.gpu

DFAS = ["newyork", "set5", "num3", "log100", "uri", "aab", "ale", "syn256"]


def _expect(blob, text):
    cpu = O.CpuOracle(blob)
    recs, k = cpu.collect(text, 4096)
    if k > len(recs):
        recs, k = cpu.collect(text, k)
    if O.have_ref():
        ref, rk = O.ref_collect(blob, text, max(k, 1))
        assert rk == k and ref[:k] == recs[:k]
    return recs, k


def _check(exe, blob, text, chunk, *, dev=False):
    import torch
    arg = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda() if dev else text
    cnt, r, s, e = one_amd.collect_long(exe, arg, chunk_bytes=chunk)
    if dev:
        r, s, e = r.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()
    recs, k = _expect(blob, text)
    assert cnt == k, (cnt, k)
    got = list(zip(r.tolist(), s.tolist(), e.tolist()))
    assert got == recs
    return cnt


# Suffix-closed DFAs without a pure dead state (newyork, uri): every attempt runs to the end of
# the text, and the CPU checkers' collect - like the reference's - walks every position behind
# the last match to the end: quadratic.  Their texts end in a match, so that tail is empty.
CLOSED = {"newyork": b"New York", "uri": b"http://www.example.com/index.html"}


def _planted(blob, n, chunk, seed, alphabet=True, name=None):
    """n bytes of text with the matched substrings of a sample planted across chunk borders."""
    gen = W.alphabet_bytes if alphabet else W.random_bytes
    a = gen(n, seed).copy()
    if name in CLOSED:
        pieces = [CLOSED[name]]
    else:
        sample = bytes(gen(1 << 14, seed + 1))
        recs, _ = O.CpuOracle(blob).collect(sample, 64)
        pieces = [sample[s:e] for _, s, e in recs if 0 < e - s <= 64]
    if name in CLOSED and n >= len(pieces[0]):
        a[n - len(pieces[0]):] = np.frombuffer(pieces[0], dtype=np.uint8)
    if pieces and n:
        for k, b in enumerate(range(chunk, n, chunk)):
            p = pieces[k % len(pieces)]
            at = b - len(p) // 2 - (k % 3)
            if at >= 0 and at + len(p) <= n:
                a[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return bytes(a)


def test_collect_kat_through_collect_long():
    kat = json.load(open(os.path.join(GOLD, "collect_kat.json")))
    blob, text = unb64(kat["reda"]), unb64(kat["text"])
    exe = one_amd.Executable(blob)
    want = [tuple(x) for x in kat["expect"]]
    for chunk in (0, 16, 64, 1024):
        cnt, r, s, e = one_amd.collect_long(exe, text, chunk_bytes=chunk)
        assert list(zip(r.tolist(), s.tolist(), e.tolist())) == want and cnt == len(want)
        assert list(zip(r.tolist(), s.tolist(), e.tolist())) == one_amd.collect(exe, text)
    assert one_amd.collect_long(exe, b"new york", chunk_bytes=4)[0] == 1


@pytest.mark.parametrize("name", DFAS)
@pytest.mark.parametrize("chunk", [16, 64, 1024, 0])
def test_collect_long_lengths_vs_oracle(name, chunk):
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    c = chunk or 256
    for n in (0, 1, c - 1, c, c + 1, 5 * c + 3):
        _check(exe, blob, _planted(blob, n, c, 11 + n, name=name), chunk)
    for alphabet in (True, False):
        _check(exe, blob, _planted(blob, 3 << 20, c, 5, alphabet, name), chunk)


@pytest.mark.parametrize("name", DFAS)
def test_collect_long_routes(name):
    blob = load_dfa(name)
    exe = one_amd.Executable(blob)
    info = exe.info
    text = _planted(blob, 1 << 20, 256, 3, name=name)
    _check(exe, blob, text, 0)
    k = one_amd.last_kernel()
    if info["n_pure_dead"] == 0 and not info["suffix_closed"]:
        assert k == "k_collect", k          # dense (SYN-256): the one-lane route
    elif info["n_pure_dead"] == 0:
        assert k == "k_collect_long<closed>", k
    else:
        assert k == "k_collect_long", k


@pytest.mark.parametrize("dead", [0.0, 0.05])
@pytest.mark.parametrize("chunk", [16, 64, 0])
def test_collect_long_random_dfas(dead, chunk):
    blob = random_dfa(40, 256, 17, dead_frac=dead, accept_frac=0.1)
    exe = one_amd.Executable(blob)
    for n in (1000, 1 << 18):
        _check(exe, blob, bytes(W.random_bytes(n, n)), chunk)


def test_collect_long_many_chunks_automatic():
    """20 MiB on the automatic route: 256-byte chunks on 256 CUs, i.e. more than 64 Ki chunks."""
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    n = 20 << 20
    text = _planted(blob, n, 256, 7)
    cnt = _check(exe, blob, text, 0, dev=True)
    assert one_amd.last_kernel() == "k_collect_long"
    assert (n + 255) // 256 > 65536 and cnt > 0


def _aa_dfa():
    # 0 = error (pure dead end), 1 = initial, 2 = "a", 3 = "aa" (accepts, every byte -> error)
    trans = np.array([[0, 0], [0, 2], [0, 3], [0, 0]])
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[ord("a")] = 1
    return write_reda(trans, np.array([0, 0, 0, 1]), equiv=equiv, initial=1)


def test_collect_long_chains_that_never_meet():
    """'aa' over a run of a behind one b: the true chain takes odd positions, every warm-up guess
    even ones, and a re-walk fixes one chunk per round - the rounds run out and the serial finish
    walks the rest, exactly."""
    blob = _aa_dfa()
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] >= 1
    text = b"b" + b"a" * ((1 << 20) - 1)
    for chunk in (16, 64):
        assert _check(exe, blob, text, chunk) == ((1 << 20) - 1) // 2
        assert one_amd.last_kernel() == "k_collect_long"
    _check(exe, blob, b"a" * (1 << 20), 16)


def test_collect_long_second_round_of_block_totals():
    """1,049,602 chunks of 16 bytes are 1,026 blocks of 1024: the scan of the block totals carries
    its sum into a second round, and records lie behind it.  The golden newyork DFA is suffix-closed
    without a pure dead end - its collect of this text is ONE record, on the route
    k_collect_long<closed>, whatever the chunk size - so the chunked route gets "New York" as an
    anchored literal: a record per plant."""
    text, chunk, border = scan_round_text()
    blob = load_dfa("newyork")
    assert _expect(blob, text)[1] == 1
    blob = literal_dfa(b"New York")
    exe = one_amd.Executable(blob)
    assert exe.info["n_pure_dead"] >= 1
    recs, k = _expect(blob, text)
    assert k == len(recs) == len(text) // 4096
    assert all(text[s:e] == b"New York" and r == 1 for r, s, e in recs)
    assert sum(1 for _, s, _ in recs if s < border) >= 4000
    assert sum(1 for _, s, _ in recs if s >= border) >= 4
    assert _check(exe, blob, text, chunk, dev=True) == k
    assert one_amd.last_kernel() == "k_collect_long"


def test_collect_long_cap_smaller_than_count():
    blob = load_dfa("num3")
    exe = one_amd.Executable(blob)
    text = _planted(blob, 1 << 20, 64, 9)
    recs, k = _expect(blob, text)
    assert k > 10
    for cap in (0, 1, 10):
        cnt, r, s, e = one_amd.collect_long(exe, text, cap, chunk_bytes=64)
        assert cnt == k and len(r) == cap
        assert list(zip(r.tolist(), s.tolist(), e.tolist())) == recs[:cap]


def test_collect_long_two_streams_and_threads():
    import torch
    blob = load_dfa("set5")
    exe = one_amd.Executable(blob)
    texts = [_planted(blob, 2 << 20, 64, s) for s in (21, 22)]
    want = [_expect(blob, t) for t in texts]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    torch.cuda.synchronize()
    outs = []
    for st, d in zip(streams, devs):
        with torch.cuda.stream(st):
            outs.append(one_amd.collect_long(exe, d, chunk_bytes=64))
    torch.cuda.synchronize()
    for (cnt, r, s, e), (recs, k) in zip(outs, want):
        assert cnt == k
        assert list(zip(r.cpu().tolist(), s.cpu().tolist(), e.cpu().tolist())) == recs
    errors = []

    def work(t, w):
        try:
            for _ in range(3):
                cnt, r, s, e = one_amd.collect_long(exe, t, chunk_bytes=128)
                assert cnt == w[1]
                assert list(zip(r.tolist(), s.tolist(), e.tolist())) == w[0]
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(t, w)) for t, w in zip(texts, want)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
