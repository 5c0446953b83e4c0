"""The per-line record-list verbs - collect_batch, match_all_batch, replace_batch, advance_batch -
and the kernels behind them (k_collect, k_matchall, k_matchall_blocks, k_replace with its scan,
k_advance): bit-exact against the CPU oracle (and, for matchAll with the leader and for replace, a
sample of lines against the reference when it is built) under every table placement, at the block
borders of the block-wise matchAll kernel, at the end of caller-owned device buffers, above the
grid-stride and scan thresholds, with a truncated replace output, and from several streams and
threads.  Slots at or past min(count, cap) are unspecified and masked out.

What keeps a case from passing vacuously is asserted on the ORACLE's output when the inputs are
built, before any GPU call, and on one_amd.last_kernel() after the matchAll calls.

launchMatchAllK's rule (launchers.h), which the expected kernel names below are worked out from:
    tab  = 512 + up16(table_bytes) + up16(4 * states)        (table + staged results)
    the block form needs an LDS kind (1, 2, 3, 7), absorbing pure dead ends, no force_generic,
        and tab + 512 * 64 + 256 <= 163,840
    resident(T) = min(163,840 // (tab + 64 * T + 256), 2048 // T)  workgroups of T threads per CU
    T = 1024 when resident(1024) * 1024 >= resident(512) * 512, else 512
    W = 1 up to 256 states, else 2
Kind 2 (a fused u16 table, chosen only above 256 states) never qualifies: 257 states are
131,584 + 1,040 + 512 = 133,136 bytes, and 133,136 + 33,024 = 166,160 > 163,840."""
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import _lib
from one_amd import workloads as W
from oracle.reda_writer import random_dfa, write_reda
from golden_util import load_dfa
import test_gpu_long_placements as LP
from test_gpu_match_all_long import WORDS, _leaky_dead_end_dfa, _wordset_dfa

pytestmark = pytest.mark.gpu

NL = 2500                 # lines per batch: more than two 1024-thread workgroups, a ragged third
STRIDES = (33, 64, 96, 200)
MA_CAPS = (0, 1, 2, 5)    # and one at the batch's largest count
ALL = 1 << 62
SENT = 0x55               # what outputs are pre-filled with


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _t(a):
    """a host array as a device tensor (uint64 offsets as int64)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def _h(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return off


def _same_lists(got, exp, cap, what, want_start=True, want_end=True):
    """counts in full, the records below min(count, cap)"""
    gc = np.asarray(got[0]).astype(np.uint64)
    assert np.array_equal(gc, exp[0]), what + ("counts", np.flatnonzero(gc != exp[0])[:5].tolist())
    if cap == 0:
        return
    n = len(exp[0])
    m = np.arange(cap)[None, :] < np.minimum(exp[0], cap).astype(np.int64)[:, None]
    wanted = (True, want_start, want_end)
    for k, name in enumerate(("result", "start", "end")):
        g = got[1 + k]
        if not wanted[k]:
            assert g is None, what + (name,)
            continue
        g = np.asarray(g).reshape(n, cap)
        e = exp[1 + k]
        bad = m & (g.astype(e.dtype) != e)
        assert not bad.any(), what + (name, np.argwhere(bad)[:3].tolist(),
                                      g[bad][:3].tolist(), e[bad][:3].tolist())


# =================================================================================================
# 1. the placement table
# =================================================================================================
DFAS = dict(LP.DFAS)
DFAS.update({
    "syn256": lambda: load_dfa("syn256"),
    "rnd72": lambda: random_dfa(72, 256, 4, dead_frac=0.05, accept_frac=0.1),
    "leaky": _leaky_dead_end_dfa,   # a pure dead end with a way out: the walk's stop is observable
})
# heads that give num3 its second matchAll record, beside LP.PIECES' (which give one each),
# and a URI of uri_v6 that fits a 33-byte line
MORE_PIECES = {"num3": [b"12345a", b"987x"], "uri_v6": [b"ftp://a.io/x"]}
# matchAll records a line of these anchored DFAs can have at most: their walk dies behind the match
# (aab: "aab" and nothing else; num3: digits, then digits and a letter; log100: a signature, then its
# " code=N" tail).  Every other DFA here must give 200 lines with two records and 50 with three.
MAX_RECORDS = {"aab": 1, "num3": 2, "log100": 2}

PLAIN = "k_matchall"
BLOCKS = "k_matchall_blocks<%d,%d>"
# The block rows.  tab, resident(1024) and resident(512) by the rule in the module docstring, from
# the table_bytes and states_used asserted with the row:
#   log100   kind 7: tab = 512 + 36,304 + 12,608 = 49,424; 163,840 // 115,216 = 1 -> 1024 lanes;
#                    163,840 // 82,448 = 1 -> 512 lanes: 1024 threads; 3,150 states: W = 2
#   uri_user kind 3: tab = 512 + 17,104 + 1,376 = 18,992; 163,840 // 84,784 = 1 -> 1024 lanes;
#                    min(163,840 // 52,016, 4) = 3 -> 1536 lanes: 512 threads; 342 states: W = 2
#   rnd1500  kind 3: tab = 512 + 120,000 + 6,000 = 126,512; 163,840 // 192,304 = 0;
#                    163,840 // 159,536 = 1 -> 512 lanes: 512 threads; 1,500 states: W = 2
#   uri      kind 1: tab = 512 + 54,272 + 848 = 55,632; 163,840 // 121,424 = 1 -> 1024 lanes;
#                    163,840 // 88,656 = 1 -> 512 lanes: 1024 threads; 212 states: W = 1
#   syn256   kind 1: tab = 512 + 65,536 + 1,024 = 67,072; 163,840 // 132,864 = 1 -> 1024 lanes;
#                    163,840 // 100,096 = 1 -> 512 lanes: 1024 threads; 256 states: W = 1
#   rnd72    kind 1: tab = 512 + 18,432 + 288 = 19,232; 163,840 // 85,024 = 1 -> 1024 lanes;
#                    min(163,840 // 52,256, 4) = 3 -> 1536 lanes: 512 threads; 72 states: W = 1
# The plain rows: kinds 4, 5 and 6 keep their table outside LDS; kind 2 never fits (docstring:
# rnd270 is 512 + 138,240 + 1,088 + 33,024 = 172,864); force_generic; leaky's dead end is not absorbing.
_BLOCK_ROWS = {
    "log100-default-kind7": (BLOCKS % (1024, 2), dict(table_bytes=36292, states_used=3150)),
    "uri_user-default-kind3": (BLOCKS % (512, 2), dict(table_bytes=17100, states_used=342)),
    "rnd1500-default-kind3": (BLOCKS % (512, 2), dict(table_bytes=120000, states_used=1500)),
}


def _table():
    rows = []
    for p in LP.ROWS:
        dfa, opts, info = p.values
        kernel, facts = _BLOCK_ROWS.get(p.id, (PLAIN, {}))
        assert kernel != PLAIN or info["table_kind"] in (2, 4, 5, 6), p.id
        rows.append(pytest.param(dfa, opts, dict(info, **facts), kernel, id=p.id))
    for dfa, opts, info, kernel in (
            ("uri", {}, dict(table_kind=1, table_bytes=54272, states_used=212), BLOCKS % (1024, 1)),
            ("syn256", {}, dict(table_kind=1, table_bytes=65536, states_used=256), BLOCKS % (1024, 1)),
            ("rnd72", {}, dict(table_kind=1, table_bytes=18432, states_used=72, n_pure_dead=1),
             BLOCKS % (512, 1)),
            ("uri", dict(force_generic=True), dict(table_kind=1), PLAIN),
            ("leaky", {}, dict(table_kind=1, n_pure_dead=1), PLAIN)):
        rows.append(pytest.param(dfa, opts, info, kernel,
                                 id="%s-%s-kind%d" % (dfa, "+".join(opts) or "default", info["table_kind"])))
    return rows


TABLE = _table()


def test_table_covers_every_route():
    """the names the table asserts: the four block instantiations, and the per-byte kernel under
    kinds 2, 4, 5 and 6, under force_generic and for the dead end with a way out"""
    names = {p.values[3] for p in TABLE}
    assert names == {PLAIN} | {BLOCKS % (t, w) for t in (1024, 512) for w in (1, 2)}
    plain = [p.values for p in TABLE if p.values[3] == PLAIN]
    assert {v[2]["table_kind"] for v in plain} >= {2, 4, 5, 6}
    assert any(v[1].get("force_generic") for v in plain) and any(v[0] == "leaky" for v in plain)
    for kind in (1, 2, 3, 4, 5, 6, 7):      # collect, replace and advance: every kind, 2,500 lines
        assert any(p.values[2]["table_kind"] == kind for p in TABLE), kind


def _fill(name, lens, seed):
    """the lines' bytes: planted alphabet text for the regex DFAs (most lines START with a piece -
    matchAll is one anchored walk - and go on piece after piece), a / b / other for leaky, random
    bytes for the random DFAs"""
    rng = np.random.default_rng(seed + 1)
    off = _offsets(lens)
    total = int(off[-1])
    if name == "leaky":
        return _u8(b"ab.")[rng.integers(0, 3, total)].copy(), off
    if name not in LP.PIECES:
        return W.random_bytes(total, seed), off
    data = W.alphabet_bytes(total, seed).copy()
    pieces = [_u8(p) for p in LP.PIECES[name] + MORE_PIECES.get(name, [])]
    for i, n in enumerate(lens):
        if i % 8 == 7:
            continue
        at = 0 if i % 3 else int(rng.integers(0, 9))
        k, o = i, int(off[i])
        while at < n:
            p = pieces[k % len(pieces)]
            k += 1
            m = min(len(p), n - at)
            data[o + at:o + at + m] = p[:m]
            at += len(p) + int(rng.integers(0, 3))
    return data, off


class _Batch:
    def __init__(self, key, data, off=None, stride=0):
        self.key, self.data, self.off, self.stride = key, data, off, stride
        self.n = len(off) - 1 if off is not None else len(data) // stride
        self.kw = dict(offsets=off) if off is not None else dict(stride=stride, n=self.n)
        self._dev = None

    def line(self, i):
        if self.off is not None:
            return self.data[int(self.off[i]):int(self.off[i + 1])].tobytes()
        return self.data[i * self.stride:(i + 1) * self.stride].tobytes()

    def dev(self):
        if self._dev is None:
            self._dev = (_t(self.data), dict(offsets=_t(self.off)) if self.off is not None
                         else dict(stride=self.stride, n=self.n))
        return self._dev


class _Data:
    """One DFA: its checkers, its batches and the oracle's answers, computed once and shared by the
    DFA's placements."""

    def __init__(self, name, index):
        self.name = name
        self.blob = DFAS[name]()
        self.cpu = O.CpuOracle(self.blob)
        self.ref = O.Reference(self.blob) if O.have_ref() else None
        i = one_amd.Executable(self.blob, device="none").info
        self.dense = i["n_pure_dead"] == 0
        rng = np.random.default_rng(index)
        lens = np.concatenate([np.arange(131), rng.integers(0, 301, NL - 131 - 3),
                               rng.integers(1000, 3001, 3)]).astype(np.int64)
        rng.shuffle(lens)
        assert len(lens) == NL and set(range(131)) <= set(lens.tolist()) and (lens >= 1000).sum() == 3
        self.ragged = _Batch("ragged", *_fill(name, lens, 7))
        # without a pure dead state the oracle and the lane are quadratic under collect and
        # styLast / styFull replace (test_gpu_long_placements): the lines of at most 300 bytes
        self.short = _Batch("short", *_fill(name, lens[lens <= 300], 7)) if self.dense else self.ragged
        self.fixed = {s: _Batch("fixed%d" % s, _fill(name, np.full(NL, s), 11 + s)[0], stride=s)
                      for s in STRIDES}
        self.stride = STRIDES[index % len(STRIDES)]      # the stride of the other three verbs
        self.memo = {}
        self._guards()

    def match_all(self, b, lead, cap):
        k = ("ma", b.key, lead, cap)
        if k not in self.memo:
            self.memo[k] = self.cpu.match_all_batch(b.data, cap, do_leader=bool(lead), **b.kw)
            if self.ref is not None and lead and cap >= max(1, int(self.memo[k][0].max())):
                for i in range(0, b.n, 97):
                    recs, cnt = self.ref.match_all(b.line(i), cap)
                    c, r, s, e = (a[i] for a in self.memo[k])
                    assert cnt == c and recs == list(zip(r.tolist(), s.tolist(), e.tolist()))[:len(recs)], \
                        (self.name, b.key, cap, i)
        return self.memo[k]

    def big_cap(self, b):
        return max(6, max(int(self.match_all(b, lead, 1)[0].max()) for lead in (0, 1)))

    def collect(self, b, cap):
        k = ("co", b.key, cap)
        if k not in self.memo:
            self.memo[k] = self.cpu.collect_batch(b.data, cap, **b.kw)
        return self.memo[k]

    def replace(self, b, repl, style, lead, mx):
        """(counts, out_offsets, out) as the verb returns them, from the oracle line by line"""
        k = ("re", b.key, repl, style, lead, mx)
        if k not in self.memo:
            outs = [self.cpu.replace(b.line(i), repl, style, bool(lead), mx) for i in range(b.n)]
            if self.ref is not None:
                for i in range(0, b.n, 97):
                    assert self.ref.replace(b.line(i), repl, style, bool(lead), mx) == outs[i], \
                        (self.name, b.key, repl, style, lead, mx, i)
            self.memo[k] = (np.array([c for c, _ in outs], dtype=np.uint64),
                            _offsets([len(o) for _, o in outs]), _u8(b"".join(o for _, o in outs)))
        return self.memo[k]

    def _guards(self):
        most = MAX_RECORDS.get(self.name, 3)
        for b in [self.ragged] + list(self.fixed.values()):
            for lead in (0, 1):
                c = self.match_all(b, lead, 1)[0]
                what = (self.name, b.key, lead, int((c >= 1).sum()), int((c >= 2).sum()), int((c > 2).sum()))
                assert (c >= 1).sum() >= 200, what
                if b.stride == 33:       # (too short for a third record of the URI DFAs)
                    continue
                assert (c >= min(most, 2)).sum() >= 200, what
                if most >= 3:
                    assert (c > 2).sum() >= 50, what
                else:
                    assert c.max() == most, what
            if b.stride in (0, self.stride):
                bb = self.short if b is self.ragged else b
                cc = self.collect(bb, 1)[0]
                assert (cc >= 1).sum() >= 200, (self.name, bb.key, int((cc >= 1).sum()))


_datas = {}
_exes = {}


def _data(name):
    if name not in _datas:
        _datas[name] = _Data(name, sorted(DFAS).index(name))
    return _datas[name]


def _exe(dfa, opts, info):
    """the row's Executable, built once and shared by the row's tests; its placement and the facts
    the expected kernel name was worked out from are asserted"""
    key = (dfa, tuple(sorted(opts.items())))
    if key not in _exes:
        _exes.clear()                       # (one row's image at a time)
        _exes[key] = one_amd.Executable(_data(dfa).blob, **opts)
    exe = _exes[key]
    got = exe.info
    for k, v in info.items():
        assert got[k] == v, (dfa, opts, k, got[k], v)
    return exe


@pytest.mark.parametrize("dfa,opts,info,kernel", TABLE)
def test_match_all_batch_under_placement(dfa, opts, info, kernel):
    d = _data(dfa)
    exe = _exe(dfa, opts, info)
    for b in [d.ragged] + list(d.fixed.values()):
        ddata, dkw = b.dev()
        for lead in (0, 1):
            for cap in MA_CAPS + (d.big_cap(b),):
                exp = d.match_all(b, lead, cap)
                what = (dfa, b.key, lead, cap)
                got = one_amd.match_all_batch(exe, b.data, cap, bool(lead), **b.kw)
                assert one_amd.last_kernel() == kernel, what + (one_amd.last_kernel(),)
                _same_lists(got, exp, cap, what + ("host",))
                got = one_amd.match_all_batch(exe, ddata, cap, bool(lead), **dkw)
                assert one_amd.last_kernel() == kernel, what + (one_amd.last_kernel(),)
                _same_lists([_h(g) for g in got], exp, cap, what + ("device",))


@pytest.mark.parametrize("dfa,opts,info,kernel", TABLE)
def test_collect_batch_under_placement(dfa, opts, info, kernel):
    d = _data(dfa)
    exe = _exe(dfa, opts, info)
    for b in (d.short, d.fixed[d.stride]):
        ddata, dkw = b.dev()
        big = max(4, int(d.collect(b, 1)[0].max()))
        for cap in (1, 3, big):
            exp = d.collect(b, cap)
            got = one_amd.collect_batch(exe, b.data, cap, **b.kw)
            assert one_amd.last_kernel() == "k_collect"
            _same_lists(got, exp, cap, (dfa, b.key, cap, "host"))
            got = one_amd.collect_batch(exe, ddata, cap, **dkw)
            _same_lists([_h(g) for g in got], exp, cap, (dfa, b.key, cap, "device"))


# every style and leader setting with the 7-byte replacement and no limit, and beside it one of
# the other (max_count, replacement) pairs each, so that all of {0, 1, no limit} x {empty, 1 byte,
# 7 bytes} run under every table kind
REPLS = (b"", b"#", b"<seven>")
_OTHER = [(mx, r) for mx in (0, 1, ALL) for r in REPLS if (mx, r) != (ALL, REPLS[2])]


def _replace_cases():
    k = 0
    for style in (1, 2, 3, 4, 5):
        for lead in (0, 1):
            yield style, lead, ALL, REPLS[2]
            yield (style, lead) + _OTHER[k % len(_OTHER)]
            k += 1


@pytest.mark.parametrize("dfa,opts,info,kernel", TABLE)
def test_replace_batch_under_placement(dfa, opts, info, kernel):
    import torch
    d = _data(dfa)
    exe = _exe(dfa, opts, info)
    assert {(mx, r) for _, _, mx, r in _replace_cases()} == {(mx, r) for mx in (0, 1, ALL) for r in REPLS}
    fixed = d.fixed[d.stride]
    ddata, dkw = fixed.dev()
    replaced = 0
    for style, lead, mx, repl in _replace_cases():
        b = d.short if style in (4, 5) else d.ragged
        exp = d.replace(b, repl, style, lead, mx)
        replaced += int(exp[0].sum())
        got = one_amd.replace_batch(exe, b.data, repl, style, bool(lead), mx, **b.kw)
        assert one_amd.last_kernel() == "k_replace"
        what = (dfa, b.key, style, lead, mx, repl)
        for g, e, name in zip(got, exp, ("counts", "out_offsets", "out")):
            assert np.array_equal(g, e), what + (name,)
        # the device form: sizes first, then into a tensor of exactly that size
        exp = d.replace(fixed, repl, style, lead, mx)
        cnt, ooff, none = one_amd.replace_batch(exe, ddata, repl, style, bool(lead), mx, **dkw)
        assert none is None and np.array_equal(_h(ooff, np.uint64), exp[1]), what
        out = torch.full((len(exp[2]) + 16,), SENT, dtype=torch.uint8, device="cuda")
        cnt, ooff, out = one_amd.replace_batch(exe, ddata, repl, style, bool(lead), mx,
                                               out=out, out_cap=len(exp[2]), **dkw)
        assert np.array_equal(_h(cnt, np.uint64), exp[0]), what
        assert np.array_equal(_h(ooff, np.uint64), exp[1]), what
        assert np.array_equal(_h(out)[:len(exp[2])], exp[2]) and (_h(out)[len(exp[2]):] == SENT).all(), what
    assert replaced >= 200, (dfa, replaced)


def _cut_batches(b, seed):
    """every line in three chunks, cut as test_stateful_matcher_on_gpu cuts them: chunk k of all
    lines packed back to back, with its offsets"""
    lens = (b.off[1:] - b.off[:-1]).astype(np.int64) if b.off is not None else np.full(b.n, b.stride)
    base = b.off[:-1].astype(np.int64) if b.off is not None else np.arange(b.n) * b.stride
    rng = np.random.default_rng(seed)
    c1 = (rng.random(b.n) * (lens + 1)).astype(np.int64)            # 0..len
    c2 = c1 + (rng.random(b.n) * (lens - c1 + 1)).astype(np.int64)  # c1..len
    cuts = [np.zeros_like(lens), c1, c2, lens]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        clen = hi - lo
        coff = _offsets(clen)
        idx = np.repeat(base + lo - coff[:-1].astype(np.int64), clen) + np.arange(int(coff[-1]))
        yield b.data[idx], coff


@pytest.mark.parametrize("dfa,opts,info,kernel", TABLE)
def test_advance_batch_under_placement(dfa, opts, info, kernel):
    import torch
    d = _data(dfa)
    exe = _exe(dfa, opts, info)
    for b, dev in ((d.ragged, False), (d.fixed[d.stride], True)):
        state = np.full(b.n, one_amd.STATE_INITIAL, dtype=np.uint32)
        dstate = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
        ostate = np.full(b.n, O.STATE_INITIAL, dtype=np.uint32)
        accepted = 0
        for k, (chunk, coff) in enumerate(_cut_batches(b, 3)):
            exp = d.cpu.advance_batch(chunk, ostate, offsets=coff)
            if dev:
                if len(chunk) == 0:
                    chunk = np.zeros(1, dtype=np.uint8)      # (a device pointer even for no bytes)
                got = _h(one_amd.advance_batch(exe, _t(chunk), dstate, offsets=_t(coff)))
            else:
                got = one_amd.advance_batch(exe, chunk, state, offsets=coff)
            assert np.array_equal(got, exp), (dfa, b.key, k, np.flatnonzero(got != exp)[:5].tolist())
            accepted += int((exp > 0).sum())
        # the three chunks end where one chunk over the whole line ends
        whole = one_amd.advance_batch(exe, b.data, np.full(b.n, one_amd.STATE_INITIAL, dtype=np.uint32),
                                      **b.kw)
        assert np.array_equal(whole, exp), (dfa, b.key)
        assert accepted >= 20, (dfa, b.key, accepted)     # (results, not only zeros, were compared)


# =================================================================================================
# 2. block borders of k_matchall_blocks, constructed
# =================================================================================================
def _ac_dfa(words):
    """_wordset_dfa's construction for any (word over a..h, result) list: Aho-Corasick as a dense
    DFA over the classes of abcdefgh + other; state 0 = error, 1 = the root; results inherited
    along failure links"""
    goto, out = [{}], [0]
    for w, r in words:
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


_WORDSET = [(w, k + 1) for k, w in enumerate(WORDS)]
# 300 words of result 0 over d, e, f, g - letters no word of WORDS has: more than 256 reachable
# states, the same results everywhere (a filler is never a suffix of what WORDS' words end in)
_FILLERS = [(bytes(b"defg"[(k >> (2 * j)) & 3] for j in range(5)), 0) for k in range(300)]

# The two DFAs, and the kernel launchMatchAllK's rule gives each (module docstring):
#   wordset1: 12 states, kind 1, 3,072 bytes: tab = 512 + 3,072 + 48 = 3,632;
#             min(163,840 // 69,424, 2) = 2 -> 2048 lanes; min(163,840 // 36,656, 4) = 4 -> 2048
#             lanes: 1024 threads (>=), W = 1
#   wordset2: 652 states, kind 3, 9 classes, 11,736 bytes: tab = 512 + 11,744 + 2,608 = 14,864;
#             min(163,840 // 80,656, 2) = 2 -> 2048 lanes; min(163,840 // 47,888, 4) = 3 -> 1536
#             lanes: 1024 threads, W = 2
_WS = {
    1: ("wordset1", lambda: _ac_dfa(_WORDSET), BLOCKS % (1024, 1),
        dict(table_kind=1, states_used=12, table_bytes=3072)),
    2: ("wordset2", lambda: _ac_dfa(_WORDSET + _FILLERS), BLOCKS % (1024, 2),
        dict(table_kind=3, states_used=652, table_bytes=11736)),
}
_ws_cache = {}


def _ws(w):
    """(blob, oracle, Executable) of the word-set DFA whose walk stages w bytes per state"""
    if w not in _ws_cache:
        name, make, kernel, info = _WS[w]
        blob = make()
        if w == 1:
            assert blob == _wordset_dfa()
        exe = one_amd.Executable(blob)
        got = exe.info
        for k, v in info.items():
            assert got[k] == v, (name, k, got[k], v)
        assert (got["states_used"] > 256) == (w == 2)
        _ws_cache[w] = (blob, O.CpuOracle(blob), exe, kernel)
    return _ws_cache[w]


def _straddles(P):
    """a record crosses position P as a border of every block size P is a multiple of"""
    def check(recs):
        return all(any(s // B != (e - 1) // B and s < P < e for _, s, e in recs)
                   for B in (32, 64) if P % B == 0)
    return check


def _border_lines(P):
    """(tag, line, guard on the oracle's records) for every border case at position P.  '.' (class
    other) leads back to the root, the initial state, from everywhere."""
    dot = b"."
    out = []
    for o in (-1, 0, 1):
        q = P + o
        # a run of one result that begins before the border and ends behind it
        out.append(("across%+d" % o, dot * (q - 8) + b"h" * 14 + dot * 2,
                    lambda r, q=q: (5, q - 8, q + 6) in r and _straddles(P)(r)))
        # a run whose last position is q - 1 (o = 0: the last position of a block)
        out.append(("ends%+d" % o, dot * (q - 4) + b"bbbb" + dot * 2, lambda r, q=q: r == [(3, q - 4, q)]))
        # a run whose first position is q (o = 0: the first position of a block)
        out.append(("begins%+d" % o, dot * q + b"bbb" + dot, lambda r, q=q: r == [(3, q, q + 3)]))
        # two results adjacent across the border: ...ab | c...
        out.append(("adjacent%+d" % o, dot * (q - 2) + b"abc" + dot,
                    lambda r, q=q, o=o: r == [(6, q - 2, q - 1), (1, q - 2, q), (2, q - 2, q + 1)] and
                    (o != 0 or _straddles(P)(r))))
        # the walk leaves the initial state at q - 1 and accepts at q (matchStart is carried), or
        # three positions on
        out.append(("carried%+d" % o, dot * (q - 1) + b"ca" + dot,
                    lambda r, q=q, o=o: r == [(6, q - 1, q + 1)] and (o != 0 or _straddles(P)(r))))
        out.append(("carried_h%+d" % o, dot * (q - 1) + b"hhhhh" + dot,
                    lambda r, q=q, o=o: r == [(5, q - 1, q + 4)] and (o != 0 or _straddles(P)(r))))
    # record j (cap - 1 for cap = j + 1) opens before the border, its run ends two blocks of 64 on ...
    for j in (0, 1, 2):
        head = b"b." * j + dot * (P - 6 - 2 * j)            # j one-byte records, then to P - 6
        long_end = P + 128 + 10                             # the run's end, mid-block
        run = b"h" * (long_end - (P - 6))
        first = [(3, 2 * k, 2 * k + 1) for k in range(j)] + [(5, P - 6, long_end)]
        # ... and the line ends; or record j + 1 opens right behind it, or after a gap
        out.append(("late_end_j%d" % j, head + run + dot * 3,
                    lambda r, f=first: r == f and _straddles(P)(r) and _straddles(P + 64)(r)))
        out.append(("late_next_j%d" % j, head + run + b"ab" + dot,
                    lambda r, f=first, e=long_end: r == f + [(6, P - 6, e + 1), (1, P - 6, e + 2)]))
        out.append(("late_gap_j%d" % j, head + run + dot * 2 + b"b" + dot,
                    lambda r, f=first, e=long_end: r == f + [(3, e + 2, e + 3)]))
        # ... or the run ends on the last position of a block and record j + 1 opens in the next
        # block (its end comes from the carried curEnd, not from this block's mask)
        run2 = b"h" * (P + 128 - (P - 6))
        out.append(("late_border_j%d" % j, head + run2 + dot * 3 + b"b" + dot,
                    lambda r, f=first: r == f[:-1] + [(5, P - 6, P + 128), (3, P + 131, P + 132)]))
    return out


def _ma_dev(exe, ddata, doff, cap, ws, we, lead=True):
    got = one_amd.match_all_batch(exe, ddata, cap, lead, offsets=doff, want_start=ws, want_end=we)
    return [None if g is None else _h(g) for g in got]


@pytest.mark.parametrize("P", [32, 64, 128])
@pytest.mark.parametrize("w", [1, 2])
def test_match_all_block_borders(w, P):
    blob, cpu, exe, kernel = _ws(w)
    # the batch the line is embedded in: 1,500 runs of h of 40 to 139 bytes, the line at lane 700
    hl = 40 + (np.arange(1500) * 37) % 100
    for tag, line, guard in _border_lines(P):
        recs, cnt = cpu.match_all(line, True, 64)
        assert cnt == len(recs) and guard(recs), (w, P, tag, recs)
        big = max(cnt, 4)
        lens = hl.copy()
        lens[700] = len(line)
        off = _offsets(lens)
        data = np.full(int(off[-1]), ord("h"), dtype=np.uint8)
        data[int(off[700]):int(off[701])] = _u8(line)
        batches = ((_u8(line).copy(), _offsets([len(line)])), (data, off))
        for bdata, boff in batches:
            ddata, doff = _t(bdata), _t(boff)
            for cap in (0, 1, 2, 3, big):
                exp = cpu.match_all_batch(bdata, cap, do_leader=True, offsets=boff)
                assert exp[0][0 if len(boff) == 2 else 700] == cnt
                for ws, we in ((True, True), (True, False), (False, True), (False, False)):
                    got = _ma_dev(exe, ddata, doff, cap, ws, we)
                    assert one_amd.last_kernel() == kernel, (tag, one_amd.last_kernel())
                    _same_lists(got, exp, cap, (w, P, tag, len(boff) - 1, cap, ws, we), ws, we)


# =================================================================================================
# 3. the end of the caller's buffer (device form)
# =================================================================================================
def _sentinel(n_bytes, dtype):
    import torch
    return torch.full((n_bytes,), SENT, dtype=torch.uint8, device="cuda").view(dtype)


def _untouched(t):
    import torch
    return bool((t.contiguous().view(torch.uint8) == SENT).all().item())


def _ma_into(exe, ddata, doff, stride, n, cap, ws, we):
    """match_all_batch into sentinel-filled tensors with room for three more lines -> host
    (counts, result, start, end) of the n lines; the slack, and the arrays not passed, must come
    back untouched"""
    import torch
    extra = 3
    counts = _sentinel((n + extra) * 8, torch.int64)
    res = _sentinel((n + extra) * cap * 4, torch.int32)
    st = _sentinel((n + extra) * cap * 8, torch.int64)
    en = _sentinel((n + extra) * cap * 8, torch.int64)
    one_amd.match_all_batch(exe, ddata, cap, True, offsets=doff, stride=stride,
                            out=(counts, res, st if ws else None, en if we else None))
    assert _untouched(counts[n:]) and _untouched(res[n * cap:])
    assert _untouched(st[n * cap:] if ws else st) and _untouched(en[n * cap:] if we else en)
    return (_h(counts[:n]), _h(res[:n * cap]), _h(st[:n * cap]) if ws else None,
            _h(en[:n * cap]) if we else None)


@pytest.mark.parametrize("which", ["syn256", "wordset2"])
def test_match_all_at_the_end_of_the_buffer(which):
    import torch
    if which == "syn256":
        blob = load_dfa("syn256")
        exe, cpu, kernel = one_amd.Executable(blob), O.CpuOracle(blob), BLOCKS % (1024, 1)
        pool = W.random_bytes(71 * 64 + 200, 31)
    else:
        blob, cpu, exe, kernel = _ws(2)
        pool = (_u8(b"abcdefgh.")[W.random_bytes(71 * 64 + 200, 32) % 9]).copy()
    body = [pool[64 * k:64 * k + 64].tobytes() for k in range(70)]
    caps = (2, 96)                                      # 96: above any count of an 80-byte line
    for L in range(81):
        last = pool[70 * 64 + 37:70 * 64 + 37 + L].tobytes()
        # a byte that changes the last line's records when the walk goes on into it
        own = cpu.match_all(last, True, 128)
        hostile = next((v for v in range(256) if cpu.match_all(last + bytes([v]) * 16, True, 128) != own), None)
        assert hostile is not None, (which, L)
        lines = body + [last]
        middle = body[:35] + [last] + body[35:]
        n = len(lines)
        data, off = _u8(b"".join(lines)), _offsets([len(x) for x in lines])
        exp = {cap: cpu.match_all_batch(data, cap, do_leader=True, offsets=off) for cap in caps}
        assert int(exp[96][0].max()) <= 96 and int(exp[96][0].sum()) >= 70
        what = (which, L)
        # the tensor ends with the last line's last byte
        exact = _t(data)
        assert exact.numel() == 70 * 64 + L
        doff = _t(off)
        for cap in caps:
            for ws, we in ((True, True), (False, False), (True, False), (False, True)):
                got = _ma_into(exe, exact, doff, 0, n, cap, ws, we)
                assert one_amd.last_kernel() == kernel
                _same_lists(got, exp[cap], cap, what + ("exact", cap, ws, we), ws, we)
        # the same bytes as a view at an odd offset of a tensor full of the hostile byte
        for shift in (1, 7, 15):
            big = torch.full((shift + len(data) + 64,), hostile, dtype=torch.uint8, device="cuda")
            big[shift:shift + len(data)] = exact
            for cap in caps:
                got = _ma_into(exe, big[shift:shift + len(data)], doff, 0, n, cap, True, True)
                _same_lists(got, exp[cap], cap, what + ("view", shift, cap))
        at_end = got                                    # (cap 96, the view at 15)
        # the same L bytes as a middle line: the same records
        mdata, moff = _u8(b"".join(middle)), _offsets([len(x) for x in middle])
        mexp = cpu.match_all_batch(mdata, 96, do_leader=True, offsets=moff)
        mgot = _ma_into(exe, _t(mdata), _t(moff), 0, n, 96, True, True)
        _same_lists(mgot, mexp, 96, what + ("middle",))
        k = int(exp[96][0][70])
        assert k == int(mgot[0][35])
        for a, b2 in zip(at_end[1:], mgot[1:]):
            assert np.array_equal(a.reshape(n, 96)[70, :k], b2.reshape(n, 96)[35, :k]), what
        # trimmed ragged lines: every line with the hostile byte as its delimiter, stride = 1
        tdata = _u8(b"".join(x + bytes([hostile]) for x in lines))
        toff = _offsets([len(x) + 1 for x in lines])
        for cap in caps:
            got = _ma_into(exe, _t(tdata), _t(toff), 1, n, cap, True, True)
            _same_lists(got, exp[cap], cap, what + ("trimmed", cap))


# =================================================================================================
# 4. many lines: the grid-stride loops, and the scan's second level
# =================================================================================================
def test_list_verbs_above_the_grid():
    """more lines than the grid has lanes, so every lane's `line += step` loop runs a second time.
    SYN-256 (kind 1, 256 states, tab = 67,072 by the docstring's rule):
      match_all_batch -> k_matchall_blocks<1024,1>: resident(1024) = 1 workgroup of 1024 per CU;
      collect_batch   -> k_collect, 1024 threads: 512 + 65,536 + 1,024 = 67,072 <= 80 KiB of LDS,
                         so launchCollectK's perCu is 2."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blob = load_dfa("syn256")
    exe, cpu = one_amd.Executable(blob), O.CpuOracle(blob)
    assert exe.info["table_kind"] == 1 and exe.info["states_used"] == 256
    L, cap = 16, 3
    for verb, per_cu in (("match_all", 1), ("collect", 2)):
        grid = cus * per_cu * 1024
        n = grid + 1500
        data = W.random_bytes(n * L, 41 + per_cu)
        ddata = _t(data)
        if verb == "match_all":
            exp = cpu.match_all_batch(data, cap, do_leader=True, stride=L, n=n)
            got = one_amd.match_all_batch(exe, ddata, cap, True, stride=L, n=n)
            assert one_amd.last_kernel() == BLOCKS % (1024, 1)
        else:
            exp = cpu.collect_batch(data, cap, stride=L, n=n)
            got = one_amd.collect_batch(exe, ddata, cap, stride=L, n=n)
            assert one_amd.last_kernel() == "k_collect"
        # lines of the second trip have records, some of them more than cap
        assert (exp[0][grid:] >= 1).sum() >= 500 and (exp[0][grid:] > cap).sum() >= 1, verb
        _same_lists([_h(g) for g in got], exp, cap, (verb, n))


def test_replace_batch_above_a_million_lines():
    """1,048,576 + 1,500 lines: k_scan_tops sums two partials per thread (per = 2), and k_replace's
    grid-stride loop runs many times.  The lines are drawn from 64 distinct ones, which the oracle
    rewrites; counts, out_offsets and the output are assembled from those."""
    import torch
    blob = load_dfa("num3")
    exe, cpu = one_amd.Executable(blob), O.CpuOracle(blob)
    n, L, repl = 1048576 + 1500, 8, b"#"
    rng = np.random.default_rng(5)
    pool = np.unique(_u8(b"0123456789ab .")[rng.integers(0, 14, (400, L))], axis=0)[:64]
    assert pool.shape == (64, L)
    outs = [cpu.replace(p.tobytes(), repl, 4, True) for p in pool]
    pc = np.array([c for c, _ in outs], dtype=np.uint64)
    plen = np.array([len(o) for _, o in outs], dtype=np.int64)
    assert (pc >= 1).sum() >= 32 and len(set(plen.tolist())) >= 4      # offsets that are no multiples of L
    pbytes, poff = _u8(b"".join(o for _, o in outs)), _offsets(plen).astype(np.int64)
    idx = rng.integers(0, 64, n)
    counts, lens = pc[idx], plen[idx]
    ooff = _offsets(lens)
    total = int(ooff[-1])
    src = np.repeat(poff[idx] - ooff[:-1].astype(np.int64), lens) + np.arange(total)
    want = pbytes[src]
    ddata = _t(pool[idx].reshape(-1))
    out = torch.full((total + 64,), SENT, dtype=torch.uint8, device="cuda")
    gc, go, out = one_amd.replace_batch(exe, ddata, repl, 4, True, stride=L, n=n, out=out, out_cap=total)
    assert one_amd.last_kernel() == "k_replace"
    assert np.array_equal(_h(gc, np.uint64), counts)
    assert np.array_equal(_h(go, np.uint64), ooff)
    got = _h(out)
    assert np.array_equal(got[:total], want) and (got[total:] == SENT).all()


# =================================================================================================
# 5. replace_batch: an output that does not fit
# =================================================================================================
def _replace_host_raw(exe, b, repl, style, lead, mx, out, out_cap):
    """redgpu_replace_batch as it stands (one_amd.replace_batch calls it again with the full size)"""
    counts = np.full(b.n, 0x5555555555555555, dtype=np.uint64)
    ooff = np.full(b.n + 1, 0x5555555555555555, dtype=np.uint64)
    r = _u8(repl)
    rc = _lib.lib().redgpu_replace_batch(
        exe._h, style, lead, b.data.ctypes.data, b.off.ctypes.data, 0, b.n,
        r.ctypes.data if r.size else None, r.size, mx, counts.ctypes.data, ooff.ctypes.data,
        out.ctypes.data if out is not None else None, out_cap)
    assert rc == 0, _lib.lib().redgpu_last_error()
    return counts, ooff


def test_replace_batch_output_truncated():
    """every line that fits entirely below out_cap is written, nothing else is touched, and counts
    and out_offsets are complete whatever out_cap is - host and device form"""
    import torch
    d = _data("num3")
    exe = one_amd.Executable(d.blob)
    lens = (np.arange(300) * 7) % 90
    b = _Batch("trunc", *_fill("num3", lens, 23))
    repl, style, lead = b"<seven>", 4, 1
    counts, ooff, want = d.replace(b, repl, style, lead, ALL)
    total = int(ooff[-1])
    k = 150
    assert counts.sum() >= 300 and 0 < ooff[k - 1] < ooff[k] < ooff[k + 1] < total
    ddata, doff = _t(b.data), _t(b.off)
    for out_cap in (0, 1, int(ooff[k]), int(ooff[k]) - 1, total):
        fit = int(ooff[np.searchsorted(ooff, out_cap, side="right") - 1])  # the last fitting line's end
        assert fit == {0: 0, 1: 0, int(ooff[k]): int(ooff[k]), int(ooff[k]) - 1: int(ooff[k - 1]),
                       total: total}[out_cap]
        # host form
        out = np.full(total + 32, SENT, dtype=np.uint8)
        gc, go = _replace_host_raw(exe, b, repl, style, lead, ALL, out, out_cap)
        assert np.array_equal(gc, counts) and np.array_equal(go, ooff), out_cap
        assert np.array_equal(out[:fit], want[:fit]) and (out[fit:] == SENT).all(), out_cap
        # device form
        dout = torch.full((total + 32,), SENT, dtype=torch.uint8, device="cuda")
        gc, go, _ = one_amd.replace_batch(exe, ddata, repl, style, bool(lead), offsets=doff,
                                          out=dout, out_cap=out_cap)
        assert np.array_equal(_h(gc, np.uint64), counts) and np.array_equal(_h(go, np.uint64), ooff)
        got = _h(dout)
        assert np.array_equal(got[:fit], want[:fit]) and (got[fit:] == SENT).all(), out_cap
    # sizes only
    gc, go = _replace_host_raw(exe, b, repl, style, lead, ALL, None, 0)
    assert np.array_equal(gc, counts) and np.array_equal(go, ooff)
    gc, go, none = one_amd.replace_batch(exe, ddata, repl, style, bool(lead), offsets=doff)
    assert none is None and np.array_equal(_h(gc, np.uint64), counts) and np.array_equal(_h(go, np.uint64), ooff)


# =================================================================================================
# 6. two streams, four threads, one handle
# =================================================================================================
def test_list_verbs_two_streams_and_threads():
    import torch
    d = _data("rnd72")
    exe = one_amd.Executable(d.blob)
    b = d.ragged
    ddata, dkw = b.dev()
    cap, repl = 3, b"<#>"
    rexp = d.replace(b, repl, 2, 1, ALL)
    total = len(rexp[2])

    def run():
        ma = one_amd.match_all_batch(exe, ddata, cap, True, **dkw)
        co = one_amd.collect_batch(exe, ddata, cap, **dkw)
        out = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
        re = one_amd.replace_batch(exe, ddata, repl, 2, True, out=out, **dkw)
        return ma, co, re

    def check(ma, co, re, what):
        _same_lists([_h(g) for g in ma], d.match_all(b, 1, cap), cap, what + ("match_all",))
        _same_lists([_h(g) for g in co], d.collect(b, cap), cap, what + ("collect",))
        for g, e in zip(re, rexp):
            assert np.array_equal(_h(g).view(e.dtype), e), what + ("replace",)

    single = run()
    torch.cuda.synchronize()
    check(*single, ("single",))
    streams = [torch.cuda.Stream() for _ in range(2)]
    errors = []

    def work(k):
        try:
            st = streams[k % 2]
            for rep in range(3):
                with torch.cuda.stream(st):
                    got = run()
                    st.synchronize()
                check(*got, ("thread", k, rep))
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
