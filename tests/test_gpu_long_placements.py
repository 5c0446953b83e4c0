"""collect_long, replace_long and search_long under EVERY table placement (Tab<KIND> 2 to 7; the
other long-text files only ever build kind 1, and kind 7 for log100): one table of (DFA,
Executable options, expected info), each row bit-exact against the CPU oracle (and the reference
when it is built) for every style, leader setting and the chunk sizes 16, 1000 and automatic, on
texts of 64 KiB + 5 bytes - 4097 chunks of 16: more than one 1024-thread block, more than 64
tickets of 64 chunks, an unaligned tail.  Per DFA: a text with matches across chunk borders, one
without any match, one whose first match lies beyond three quarters of it, and 1000 bytes for the
one-lane routes and the batch kernels behind them.  The kind-5 row (more than 65,536 states) also
runs the batch verbs.

What keeps the file from passing vacuously is asserted on the ORACLE's output when a DFA's texts
are built (_Case), and on one_amd.last_kernel() after every call (the _route_* functions restate
launchCollectLong / launchReplaceLong / launchSearchLong).

DFAs without a pure dead state: an attempt that has not matched never ends before the end of the
text, so the CPU checkers - and the device's one lane - are quadratic under styLast and styFull
and on text without a match: those cases run on 2 KiB + 5 bytes.  For the same reason such a DFA
cannot give 50 collect records or two styLast replacements (one styLast attempt reaches the last
accept of the text): the oracle must report at least one there, and at least 50 / more than one
everywhere else.  A random DFA without a pure dead state has no text whose first match STARTS
late either (the attempt at 0 walks until it accepts): its late text is the one whose first match
ENDS beyond three quarters.

max_count 0 is replaceCore's `max` = 0: nothing is replaced (the text comes back as it went in).
It runs, next to a small max_count and no limit; "more than once" is asked of the unlimited run."""
import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import workloads as W
from oracle.reda_writer import random_dfa
from golden_util import load_dfa

pytestmark = pytest.mark.gpu

N = 65536 + 5            # 4097 chunks of 16, 66 of 1000, 257 of the automatic 256
SMALL = 2048 + 5         # the quadratic cases of the DFAs without a pure dead state
SHORT = 1000             # below the automatic route's 16 KiB: one lane
MIN_AUTO = 16384
CHUNKS = (16, 1000, 0)
STYLES = (1, 2, 3, 4, 5)
LEADS = (0, 1)
ALL = 1 << 62
FILL = 0x01              # a byte no regex DFA here starts with
LONG = b"<" + b"0123456789" * 7 + b">"      # 72 bytes: longer than every planted match

_RND = dict(dead_frac=0.05, accept_frac=0.1)
DFAS = {
    "log100": lambda: load_dfa("log100"),
    "uri_user": lambda: load_dfa("uri_user"),
    "uri_v6": lambda: load_dfa("uri_v6"),
    "uri": lambda: load_dfa("uri"),
    "num3": lambda: load_dfa("num3"),
    "aab": lambda: load_dfa("aab"),
    "rnd270": lambda: random_dfa(270, 256, 4, **_RND),
    "rnd270nd": lambda: random_dfa(270, 256, 4, dead_frac=0.0, accept_frac=0.1),
    "rnd1500": lambda: random_dfa(1500, 40, 91, **_RND),
    "rnd80k": lambda: random_dfa(80000, 4, 5, **_RND),
}
# what a regex DFA's texts are planted with (the random DFAs match random bytes often enough)
PIECES = {
    "log100": [h.rstrip() for h in W.log100_heads()[:7]],
    "uri_user": [W.URI_USER_PLANT.rstrip()],
    "uri_v6": [W.URI_V6_PLANT.rstrip()],
    "uri": [W.URI_PLANT.rstrip()],
    "num3": [b"123", b"4567"],
    "aab": [b"aab"],
}
# facts about the DFAs the table below relies on (redgpu_info of a host-only handle)
FACTS = {
    "log100": dict(states_used=3150, n_pure_dead=1),
    "uri_user": dict(states_used=342, n_pure_dead=0, suffix_closed=1),
    "uri_v6": dict(states_used=3253),
    "uri": dict(states_used=212),
    "num3": dict(leader_len=1),
    "aab": dict(leader_len=3),
    "rnd270": dict(n_pure_dead=1, suffix_closed=0),
    "rnd270nd": dict(n_pure_dead=0, suffix_closed=0),
    "rnd1500": dict(n_pure_dead=1),
    "rnd80k": dict(states_used=78032, n_pure_dead=1),
}


def _row(dfa, opts=None, **info):
    opts = opts or {}
    tag = "+".join("%s=%s" % (k, v) if v is not True else k for k, v in opts.items()) or "default"
    return pytest.param(dfa, opts, info, id="%s-%s-kind%d" % (dfa, tag, info["table_kind"]))


HOT40 = dict(force_hot=True, lds_table_max=40 * 256)
ROWS = [
    _row("log100", table_kind=7),
    _row("log100", dict(force_hot=True), table_kind=6, n_hot=254),
    _row("log100", dict(lds_table_max=16 * 256), table_kind=6, n_hot=16),   # signatures walk cold rows
    _row("log100", dict(force_global=True), table_kind=4),
    _row("uri_user", table_kind=3),
    _row("uri_user", dict(force_hot=True), table_kind=6),
    _row("uri_user", dict(force_global=True), table_kind=4),
    _row("uri_v6", table_kind=6),
    _row("uri_v6", dict(force_global=True), table_kind=4),
    _row("uri", dict(lds_table_max=16 * 256), table_kind=6, n_hot=0),       # an all-255 hot table
    _row("num3", dict(force_global=True), table_kind=4),                    # leader: eq in LDS,
    _row("aab", dict(force_global=True), table_kind=4),                     # the table in L2
    _row("rnd270", table_kind=2),                                           # 137 KB: a block per CU
    _row("rnd270", HOT40, table_kind=6, n_hot=40),
    _row("rnd270", dict(force_global=True), table_kind=4),
    _row("rnd270nd", table_kind=2),
    _row("rnd1500", table_kind=3),                                          # 120 KB class table
    _row("rnd1500", HOT40, table_kind=6),
    _row("rnd80k", table_kind=5, n_hot=0),                                  # results in global memory
]


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _plant(a, pieces, every, end_in_piece):
    """pieces over the multiples of `every` (each straddles a border of 16 as well)"""
    n = len(a)
    for k, b in enumerate(range(every, n, every)):
        p = pieces[k % len(pieces)]
        at = b - len(p) // 2 - (k % 3)
        if at >= 0 and at + len(p) <= n:
            a[at:at + len(p)] = _u8(p)
    if end_in_piece:
        a[n - len(pieces[0]):] = _u8(pieces[0])
    return a


class _Case:
    """One DFA: its checkers, its texts and the expected output of every call, computed once and
    shared by the DFA's placements."""

    def __init__(self, name):
        self.name = name
        self.blob = DFAS[name]()
        self.cpu = O.CpuOracle(self.blob)
        self.ref = O.Reference(self.blob) if O.have_ref() else None
        i = one_amd.Executable(self.blob, device="none").info
        for k, v in FACTS[name].items():
            assert i[k] == v, (name, k, i[k], v)
        self.npd, self.closed, self.leader_len = i["n_pure_dead"], i["suffix_closed"], i["leader_len"]
        self.dense = self.npd == 0
        self.memo = {}
        self.texts = {}
        if name in PIECES:
            self._regex_texts(PIECES[name])
        else:
            self._random_texts()
        self.texts["short"] = self.texts["hits_s" if self.dense else "hits"][:SHORT]
        self._not_vacuous()

    # ---- texts -----------------------------------------------------------------------------
    def _blank(self, n, seed):
        """n alphabet bytes with every match overwritten: styInstant without the leader finds
        nothing, so no attempt of any style, with or without the leader, accepts anywhere"""
        a = W.alphabet_bytes(n, seed).copy()
        base = 0
        while True:
            r, s, e = self.cpu.search(bytes(a[base:]), 1, False)
            if r == 0:
                break
            a[base + min(s, e - 1):base + e] = FILL
            base += min(s, e - 1)
        return a

    def _regex_texts(self, pieces):
        for p in pieces:
            assert self.cpu.search(p, 4, False)[0] > 0, (self.name, p)
        small_n = SMALL if self.dense else N
        self.texts["hits"] = bytes(_plant(W.alphabet_bytes(N, 12).copy(), pieces, 1000, self.dense))
        if self.dense:
            self.texts["hits_s"] = bytes(_plant(W.alphabet_bytes(SMALL, 13).copy(), pieces, 250, True))
        none = self._blank(small_n, 14)
        self.texts["none"] = bytes(none)
        at = small_n * 3 // 4 + small_n // 100
        none[at:at + len(pieces[0])] = _u8(pieces[0])
        self.texts["late"] = bytes(none)

    def _dies(self, walk):
        """the anchored walk over `walk` ends in a dead end: every byte leads back to the state it
        is in, with result 0"""
        st = np.full(1, O.STATE_INITIAL, dtype=np.uint32)
        self.cpu.advance_batch(_u8(walk), st, offsets=[0, len(walk)])
        nxt = np.full(256, st[0], dtype=np.uint32)
        res = self.cpu.advance_batch(np.arange(256, dtype=np.uint8), nxt, stride=1, n=256)
        return bool((nxt == st[0]).all() and (res == 0).all())

    def _random_texts(self):
        small_n = SMALL if self.dense else N
        hits = W.random_bytes(N, 15)
        self.texts["hits"] = bytes(hits)
        if self.dense:
            self.texts["hits_s"] = bytes(W.random_bytes(SMALL, 16))
        cut = small_n * 3 // 4 + small_n // 100
        cands = [bytes([b]) for b in range(256)] + [bytes([a, b]) for a in range(16) for b in range(16)]
        # (few classes: longer patterns over the first four bytes, which are four classes)
        cands += [bytes(int(d) for d in np.base_repr(v, 4).zfill(k)) for k in (3, 4) for v in range(4 ** k)]
        for pat in cands:
            # a filler the oracle confirms match-free (600 bytes first: cheap where it is not) ...
            probe = (pat * 600)[:600]
            if self.cpu.search(probe, 1, False)[0] or self.cpu.collect(probe, 1)[1]:
                continue
            # ... and, with a pure dead state, one whose walk DIES: an attempt that circles in the
            # filler alive walks on into whatever follows (and makes every checker quadratic)
            if not self.dense and not all(self._dies(probe[k:]) for k in range(len(pat))):
                continue
            none = (pat * small_n)[:small_n]
            if self.cpu.search(none, 1, False)[0] or self.cpu.collect(none, 1)[1]:
                continue
            # ... and behind which the first match lies in the last quarter
            late = none[:cut] + bytes(hits[cut:small_n])
            r, s, e = self.cpu.search(late, 1, False)
            if r > 0 and (e if self.dense else s) > small_n * 3 // 4:
                self.texts["none"], self.texts["late"] = none, late
                return
        raise AssertionError("no match-free filler for " + self.name)

    def texts_for(self, style):
        if self.dense and style in (4, 5):
            return ("hits_s", "none", "late")
        return ("hits", "none", "late")

    def collect_texts(self):
        # (collect is styLast without the leader; a suffix-closed DFA's chain is ONE attempt)
        if self.dense and not self.closed:
            return ("hits_s", "none", "late")
        return ("hits", "none", "late")

    # ---- expectations ------------------------------------------------------------------------
    def search(self, key, style, lead):
        k = ("search", key, style, lead)
        if k not in self.memo:
            t = self.texts[key]
            want = tuple(int(v) for v in self.cpu.search(t, style, bool(lead)))
            if self.ref is not None:
                assert tuple(int(v) for v in self.ref.search(t, style, bool(lead))) == want
            self.memo[k] = want
        return self.memo[k]

    def replace(self, key, repl, style, lead, mx):
        k = ("replace", key, repl, style, lead, mx)
        if k not in self.memo:
            t = self.texts[key]
            want = self.cpu.replace(t, repl, style, bool(lead), mx)
            if self.ref is not None:
                assert self.ref.replace(t, repl, style, bool(lead), mx) == want
            self.memo[k] = want
        return self.memo[k]

    def collect(self, key):
        k = ("collect", key)
        if k not in self.memo:
            t = self.texts[key]
            recs, cnt = self.cpu.collect(t, 4096)
            if cnt > len(recs):
                recs, cnt = self.cpu.collect(t, cnt)
            if self.ref is not None:
                ref, rk = O.ref_collect(self.blob, t, max(cnt, 1))
                assert rk == cnt and ref[:cnt] == recs[:cnt]
            self.memo[k] = (recs, cnt)
        return self.memo[k]

    def short_repl(self):
        """a replacement shorter than a typical (median) match of the hits text (without a pure dead
        state collect reports ONE span: the planted pieces then, or nothing for a random DFA)"""
        if self.dense:
            return b"#" if self.name in PIECES and 1 < len(PIECES[self.name][0]) < len(LONG) else b""
        recs, _ = self.collect(self.collect_texts()[0])
        med = sorted(e - s for _, s, e in recs)[len(recs) // 2]
        assert 1 <= med < len(LONG)
        return b"#" if med > 1 else b""

    def _not_vacuous(self):
        n_hits = len(self.texts["hits"])
        assert n_hits == N and len(self.texts["none"]) == len(self.texts["late"])
        recs, cnt = self.collect(self.collect_texts()[0])
        assert cnt >= (1 if self.dense else 50), (self.name, cnt)
        assert self.collect("none") == ([], 0)
        n_late = len(self.texts["late"])
        r, s, e = self.search("late", 1, 0)
        assert r > 0 and (e if self.dense and not self.closed else s) > n_late * 3 // 4
        for style in STYLES:
            for lead in LEADS:
                assert self.search("none", style, lead) == (0, 0, 0)
                assert self.replace("none", LONG, style, lead, ALL) == (0, self.texts["none"])
                if style == 5:
                    continue
                key = self.texts_for(style)[0]
                assert self.search(key, style, lead)[0] > 0, (self.name, style, lead)
                cnt = self.replace(key, LONG, style, lead, ALL)[0]
                assert cnt > (0 if self.dense and style == 4 else 1), (self.name, style, lead, cnt)


_cases = {}
_exes = {}


def _case(name):
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


def _exe(dfa, opts, info):
    """the row's Executable; its placement is asserted, so a change of placement policy cannot
    turn this file into a repeat of another kind"""
    key = (dfa, tuple(sorted(opts.items())))
    if key not in _exes:
        _exes.clear()                       # (one row's image at a time)
        _exes[key] = one_amd.Executable(_case(dfa).blob, **opts)
    exe = _exes[key]
    got = exe.info
    assert got["table_kind"] == info["table_kind"], (dfa, opts, got["table_kind"])
    for k, v in info.items():
        assert got[k] == v, (dfa, opts, k, got[k], v)
    return exe


# ---- the routes (kernels.hip: launchCollectLong, launchReplaceLong, launchSearchLong) ---------
def _early(case, style):
    return case.npd > 0 or style in (1, 2, 3)


def _route_collect(case, n, chunk, cap):
    closed = case.dense and case.closed and cap > 0
    if n == 0 or (not chunk and n < MIN_AUTO) or (case.dense and not closed):
        return "k_collect"
    return "k_collect_long<closed>" if closed else "k_collect_long"


def _route_replace(case, n, chunk, style):
    c = chunk or (n if n < MIN_AUTO or not _early(case, style) else 256)
    return "k_replace_long<one>" if c >= n else "k_replace_long"


def _route_search(case, n, chunk, style, lead):
    lead = lead and case.leader_len > 0
    if n == 0 or (not chunk and (n < MIN_AUTO or not _early(case, style) or (case.closed and not lead))):
        return "k_search_long<one>"
    return "k_search_long"


def _dev(text):
    import torch
    return torch.from_numpy(_u8(text).copy()).cuda()


def _collect(exe, case, key, chunk, cap=None, dev=False):
    text = case.texts[key]
    recs, k = case.collect(key)
    cnt, r, s, e = one_amd.collect_long(exe, _dev(text) if dev else text, cap, chunk_bytes=chunk)
    kernel = one_amd.last_kernel()
    if dev:
        r, s, e = r.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()
    what = (case.name, key, chunk, cap, dev, kernel)
    assert cnt == k, what + (cnt, k)
    assert list(zip(r.tolist(), s.tolist(), e.tolist())) == (recs if cap is None else recs[:cap]), what
    assert kernel == _route_collect(case, len(text), chunk, max(k, 4096) if cap is None else cap), what


def _replace(exe, case, key, chunk, repl, style, lead, mx, dev=False):
    text = case.texts[key]
    want = case.replace(key, repl, style, lead, mx)
    cnt, got = one_amd.replace_long(exe, _dev(text) if dev else text, repl, style, bool(lead), mx,
                                    chunk_bytes=chunk)
    kernel = one_amd.last_kernel()
    if dev:
        got = got.cpu().numpy().tobytes()
    what = (case.name, key, chunk, len(repl), style, lead, mx, dev, kernel)
    assert cnt == want[0], what + (cnt, want[0])
    assert got == want[1], what
    assert kernel == _route_replace(case, len(text), chunk, style), what


def _search(exe, case, key, chunk, style, lead, dev=False):
    text = case.texts[key]
    want = case.search(key, style, lead)
    got = one_amd.search_long(exe, _dev(text) if dev else text, style, bool(lead), chunk_bytes=chunk)
    kernel = one_amd.last_kernel()
    if dev:
        got = tuple(int(g.item()) for g in got)
    what = (case.name, key, chunk, style, lead, dev, kernel)
    assert got == want, what + (got, want)
    assert kernel == _route_search(case, len(text), chunk, style, lead), what


# ---- the tests: one per table row and verb --------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", ROWS)
def test_collect_long_under_placement(dfa, opts, info):
    case = _case(dfa)
    exe = _exe(dfa, opts, info)
    keys = case.collect_texts()
    for key in keys:
        for chunk in CHUNKS:
            _collect(exe, case, key, chunk)
    k = case.collect(keys[0])[1]
    for chunk in CHUNKS:
        _collect(exe, case, keys[0], chunk, cap=k // 2)      # cap below the count
    _collect(exe, case, keys[0], 16, dev=True)
    if not case.dense:
        # every pure-dead DFA took the chunked chain at each forced size and at the automatic one
        assert _route_collect(case, N, 16, 1) == _route_collect(case, N, 0, 1) == "k_collect_long"


@pytest.mark.parametrize("dfa,opts,info", ROWS)
def test_replace_long_under_placement(dfa, opts, info):
    case = _case(dfa)
    exe = _exe(dfa, opts, info)
    short = case.short_repl()
    for style in STYLES:
        keys = case.texts_for(style)
        for lead in LEADS:
            for chunk in CHUNKS:
                for repl, mx in ((LONG, ALL), (short, ALL), (LONG, 3), (short, 0)):
                    _replace(exe, case, keys[0], chunk, repl, style, lead, mx)
                for key in keys[1:]:
                    _replace(exe, case, key, chunk, LONG, style, lead, ALL)
    _replace(exe, case, case.texts_for(4)[0], 16, LONG, 4, 1, ALL, dev=True)
    for style in STYLES if not case.dense else (1, 2, 3):
        assert _route_replace(case, N, 16, style) == _route_replace(case, N, 0, style) == "k_replace_long"


@pytest.mark.parametrize("dfa,opts,info", ROWS)
def test_search_long_under_placement(dfa, opts, info):
    case = _case(dfa)
    exe = _exe(dfa, opts, info)
    for style in STYLES:
        for lead in LEADS:
            for key in case.texts_for(style):
                for chunk in CHUNKS:
                    _search(exe, case, key, chunk, style, lead)
    _search(exe, case, case.texts_for(4)[0], 16, 4, 1, dev=True)
    for style in STYLES if not case.dense else (1, 2, 3):
        assert _route_search(case, N, 16, style, 1) == "k_search_long"
        if not case.closed or case.leader_len:
            assert _route_search(case, N, 0, style, 1) == "k_search_long"


@pytest.mark.parametrize("dfa,opts,info", ROWS)
def test_one_lane_routes_under_placement(dfa, opts, info):
    """1000 bytes at the automatic chunk size: one lane - k_collect, the chain on one chunk, the
    batch search kernel - under the row's placement"""
    case = _case(dfa)
    exe = _exe(dfa, opts, info)
    short = case.short_repl()
    _collect(exe, case, "short", 0)
    assert one_amd.last_kernel() == "k_collect"
    for style in STYLES:
        for lead in LEADS:
            _search(exe, case, "short", 0, style, lead)
            assert one_amd.last_kernel() == "k_search_long<one>"
            for repl, mx in ((LONG, ALL), (short, 2)):
                _replace(exe, case, "short", 0, repl, style, lead, mx)
                assert one_amd.last_kernel() == "k_replace_long<one>"


def test_batch_verbs_with_u32_states():
    """REDGPU_TAB_GLOBAL_U32: every batch verb over 3,000 ragged lines of 0 to 120 bytes.  Every
    accepting device state is numbered above 65,535, so each record, and each token advance_batch
    hands back and takes again, carries a state id that does not fit 16 bits."""
    dfa, opts, info = [p.values for p in ROWS if p.values[0] == "rnd80k"][0]
    case = _case(dfa)
    exe = _exe(dfa, opts, info)
    got_info = exe.info
    assert got_info["table_kind"] == 5 and got_info["first_accept"] > 65535
    data, offs = W.ragged_lines(3000, 0, 120, 77, alphabet=False)
    cpu = case.cpu
    n = len(offs) - 1
    matched = 0
    for style in (4, 5):
        for lead in LEADS:
            for verb, fn in (("match", one_amd.match_batch), ("search", one_amd.search_batch)):
                got = fn(exe, data, style, bool(lead), offsets=offs)
                exp = cpu.batch(verb, style, lead, data, offsets=offs, threads=4)
                assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (verb, style, lead)
                matched += int((exp[0] > 0).sum())
            for verb, fn in (("check", one_amd.check_batch), ("scan", one_amd.scan_batch)):
                got = fn(exe, data, style, bool(lead), offsets=offs)
                exp = cpu.batch(verb, style, lead, data, offsets=offs, threads=4)[0]
                assert np.array_equal(got, exp), (verb, style, lead)
                matched += int((exp > 0).sum())
            counts, ooff, out = one_amd.replace_batch(exe, data, b"<#>", style, bool(lead), 3,
                                                      offsets=offs)
            for i in range(0, n, 7):
                k, o = cpu.replace(data[int(offs[i]):int(offs[i + 1])].tobytes(), b"<#>", style,
                                   bool(lead), 3)
                assert k == int(counts[i]) and o == out[int(ooff[i]):int(ooff[i + 1])].tobytes(), i
    assert matched > 1000
    cap = 4
    for lead in LEADS:
        got = one_amd.match_all_batch(exe, data, cap, bool(lead), offsets=offs)
        exp = cpu.match_all_batch(data, cap, do_leader=bool(lead), offsets=offs)
        m = np.arange(cap)[None, :] < np.minimum(exp[0], cap).astype(np.int64)[:, None]
        assert np.array_equal(got[0], exp[0]) and exp[0].sum() > 100
        assert all(np.array_equal(g[m], e[m]) for g, e in zip(got[1:], exp[1:]))
    got = one_amd.collect_batch(exe, data, cap, offsets=offs)
    exp = cpu.collect_batch(data, cap, offsets=offs)
    m = np.arange(cap)[None, :] < np.minimum(exp[0], cap).astype(np.int64)[:, None]
    assert np.array_equal(got[0], exp[0]) and exp[0].sum() > 100
    assert all(np.array_equal(g[m], e[m]) for g, e in zip(got[1:], exp[1:]))
    # advance: every line in two halves, the second from the token the first left behind
    mid = (offs[:-1] + offs[1:]) // np.uint64(2)
    halves = np.empty(2 * n + 1, dtype=np.uint64)
    halves[0::2] = offs
    halves[1::2] = mid
    st = np.full(n, one_amd.STATE_INITIAL, dtype=np.uint32)
    ost = np.full(n, O.STATE_INITIAL, dtype=np.uint32)
    alive = 0
    for half in (0, 1):
        lens = (halves[half + 1::2] - halves[half:-1:2]).astype(np.int64)
        part = np.zeros(n + 1, dtype=np.uint64)
        part[1:] = np.cumsum(lens)
        buf = np.concatenate([data[int(a):int(b)] for a, b in
                              zip(halves[half:-1:2], halves[half + 1::2])] + [np.zeros(0, np.uint8)])
        got = one_amd.advance_batch(exe, buf, st, offsets=part)
        exp = cpu.advance_batch(buf, ost, offsets=part)
        assert np.array_equal(got, exp), half
        if half == 0:
            alive = int(((st > 65535) & (st != one_amd.STATE_INITIAL)).sum())
    assert alive > 20             # tokens above 65,535 went out and came back
    whole = one_amd.advance_batch(exe, data, np.full(n, one_amd.STATE_INITIAL, dtype=np.uint32),
                                  offsets=offs)
    assert np.array_equal(whole, got)
