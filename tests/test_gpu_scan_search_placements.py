"""scan_batch and search_batch - k_scan_marked and k_generic's scan and search instantiations, both
behind launchGeneric - at every start filter and table placement: one table of (DFA, Executable
options, expected info, expected kernel per leader setting), every row bit-exact against the CPU
oracle (and every 97th line against the reference when it is built) for every style, leader
setting, on a ragged batch and a fixed stride, from host and device buffers, on the default route
and under force_generic.  one_amd.last_kernel() is asserted after every GPU call.

The route, restated here from the oracle and redgpu_info alone (launchers.h: scanMarkable,
launchGeneric):
    start bytes, without the leader = the byte values that leave the initial state for a state
        that is not a dead end with result 0; with the leader (do_leader and leader_len > 0) =
        the byte values of the leader's first class
    markable = 1 <= number of start bytes <= 64     (1..4: a packed list; 5..64: the flag table)
    tab      = up16(table_bytes) for the LDS kinds 1, 2, 3, 7; 65,536 for kind 6; 0 for kinds 4, 5
    staged   = states <= 4,096 and tab + 4 * states <= 146 KiB        (results ride behind the table)
    markLds  = 512 + tab + (up16(4 * states) if staged) + 8,192 (bitmap) + 256 * (6 * 4 + 8)
               (candidate list and seven per-line arrays) + 32 + 256 (flag table)
    k_scan_marked runs iff the verb is scan or search, the DFA is markable, force_generic is not
        set and markLds <= 158 KiB = 161,792; everything else is k_generic
A kind-2 table fits up to 280 states (512 + 143,360 + 1,120 + 16,672 = 161,664); the 285-state row
is 512 + 145,920 + 1,152 + 16,672 = 164,256 and must report k_generic.
A suffix-closed DFA without the leader never gets here as scan or search (normalizeVerbStyle turns
them into check and match): for those rows the table names the family launchRaggedFamily gives
them, as test_gpu_match_text_placements does, and _as_check_or_match restates the rest.

What keeps a case from passing vacuously is asserted on the ORACLE's output when the inputs are
built (_Data._guards), before any GPU call.

DFAs without a pure dead state: an attempt that has not matched never ends before the end of the
line, so the oracle's (and the lane's) scan is quadratic in the line length: those keep to the
lines of at most 300 bytes, as in test_gpu_list_verbs."""
import numpy as np
import pytest

import one_amd
import oracle as O
from one_amd import workloads as W
from oracle.reda_writer import write_reda
import test_gpu_long_placements as LP

pytestmark = pytest.mark.gpu

NL = 2500
STRIDES = (33, 64, 96, 200)
STYLES = (1, 2, 3, 4, 5)
LEADS = (0, 1)
SENT = 0x55
MARKED, GENERIC = "k_scan_marked", "k_generic"
MARK_LDS_MAX = 158 * 1024
THREADS = 8


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _up16(x):
    return (x + 15) & ~15


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return off


def _t(a):
    """a host array as a device tensor (uint64 offsets as int64)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


# =================================================================================================
# 1. the route, restated
# =================================================================================================
def _start_bytes(blob, cpu, lead):
    """the set scanMarkable counts, from the oracle (without the leader) or the blob's equivalence
    map and leader (with it; reda_writer's layout: leader length at 14, map at 32, leader at 288)"""
    if lead and blob[14]:
        equiv = np.frombuffer(blob, dtype=np.uint8, count=256, offset=32)
        return set(np.flatnonzero(equiv == blob[288]).tolist())
    every = np.arange(256, dtype=np.uint8)
    st = np.full(256, O.STATE_INITIAL, dtype=np.uint32)
    res = cpu.advance_batch(every, st, stride=1, n=256)
    dead = {}
    for tok in np.unique(st).tolist():
        nxt = np.full(256, tok, dtype=np.uint32)
        r2 = cpu.advance_batch(every, nxt, stride=1, n=256)
        # a dead end with result 0: every byte leads back to the state, with result 0
        dead[tok] = bool((nxt == tok).all() and (r2 == 0).all())
    return {b for b in range(256) if res[b] != 0 or not dead[int(st[b])]}


def _mark_lds(info):
    kind, n = info["table_kind"], info["states_used"]
    tab = _up16(info["table_bytes"]) if kind in (1, 2, 3, 7) else 65536 if kind == 6 else 0
    staged = n <= 4096 and tab + 4 * n <= 146 * 1024
    return 512 + tab + (_up16(4 * n) if staged else 0) + 8192 + 256 * (6 * 4 + 8) + 32 + 256


def _route(blob, cpu, info, opts, lead):
    """(kernel, reason) of scan_batch / search_batch; (None, "other_verb") where they run as check
    and match"""
    lead = bool(lead and info["leader_len"])
    if info["suffix_closed"] and not lead:
        return None, "other_verb"
    if opts.get("force_generic"):
        return GENERIC, "force_generic"
    if not 1 <= len(_start_bytes(blob, cpu, lead)) <= 64:
        return GENERIC, "unmarkable"
    if _mark_lds(info) > MARK_LDS_MAX:
        return GENERIC, "lds"
    return MARKED, "marked"


# =================================================================================================
# 2. crafted start-filter DFAs
# =================================================================================================
def _equiv(n_cls, sizes):
    """byte -> class: class c of `sizes` gets exactly sizes[c] byte values ('A' onwards), the other
    byte values go round the other classes"""
    eq = np.zeros(256, dtype=np.uint8)
    nxt, taken = 0x41, set()
    for c, k in sizes.items():
        for _ in range(k):
            eq[nxt] = c
            taken.add(nxt)
            nxt += 1
    others = [c for c in range(n_cls) if c not in sizes]
    for i, b in enumerate(b for b in range(256) if b not in taken):
        eq[b] = others[i % len(others)]
    return eq


class _Crafted:
    """random_dfa's recipe (state 0 = error, 1 = initial) with dead_frac 0.25, so attempts die within
    a few bytes, and then:
      the initial state's row: dead except for the classes of `start`;
      without a leader: they lead to the heads, states 2 and 3, which accept (results 1 and 2)
        when accept_first, else have result 0 and, with `second`, a row that is dead except for
        the classes of `second`;
      with a leader (class space): the prefix states 1, 2, .. form its forced chain - dead except
        for the leader's class - and leader_next is the first ordinary state;
      class n_cls - 1 chains the ordinary states, so all n_states are reachable."""

    def __init__(self, n_states, n_cls, seed, start=(), *, sizes=None, accept_first=False,
                 second=None, leader=(), init_result=0):
        rng = np.random.default_rng(seed)
        trans = rng.integers(1, n_states, size=(n_states, n_cls), dtype=np.int64)
        trans[rng.random((n_states, n_cls)) < 0.25] = 0
        results = np.where(rng.random(n_states) < 0.15, rng.integers(1, 6, size=n_states), 0)
        trans[0, :] = 0
        results[0] = 0
        results[1] = init_result
        self.equiv = np.arange(256, dtype=np.uint8) if n_cls == 256 else _equiv(n_cls, sizes)
        chain = n_cls - 1
        if leader:
            assert not start
            start = (leader[0],)
            for i, c in enumerate(leader):
                trans[1 + i, :] = 0
                trans[1 + i, c] = 2 + i
                if i:
                    results[1 + i] = 0
            free = 1 + len(leader)
            results[free] = 0
        else:
            trans[1, :] = 0
            for i, c in enumerate(start):
                trans[1, c] = 2 + i % 2
            free = 4
            for h in (2, 3):
                results[h] = h - 1 if accept_first else 0
                if second is not None:
                    trans[h, :] = 0
                    trans[h, list(second)] = free + np.arange(len(second)) + (h - 2)
                else:
                    trans[h, chain] = free
        trans[np.arange(free, n_states - 1), chain] = np.arange(free + 1, n_states)
        self.trans, self.results, self.leader, self.free = trans, results, tuple(leader), free
        self.n_cls = n_cls
        self.blob = write_reda(trans, results, equiv=self.equiv, initial=1, leader=bytes(leader),
                               leader_next=free if leader else None)

    # ---- what the tables say, for the facts a row claims -------------------------------------
    def alive(self, s):
        return bool(self.results[s] != 0 or (self.trans[s] != s).any())

    def facts(self):
        """(start bytes, first step accepts, second-byte set) without the leader, and the byte
        sets of the leader's first and second class"""
        t1 = self.trans[1, self.equiv]
        starts = [b for b in range(256) if self.alive(int(t1[b]))]
        firsts = sorted({int(t) for t in self.trans[1] if self.alive(int(t))})
        accepts = any(self.results[f] > 0 for f in firsts)
        second = [b for b in range(256)
                  if any(self.alive(int(self.trans[f, self.equiv[b]])) for f in firsts)]
        lead1 = np.flatnonzero(self.equiv == self.leader[0]).tolist() if self.leader else []
        lead2 = np.flatnonzero(self.equiv == self.leader[1]).tolist() if len(self.leader) > 1 else []
        return dict(n1=len(starts), first_accepts=accepts, n2=len(second), lead1=len(lead1),
                    lead2=len(lead2), starts=starts)

    # ---- plants ------------------------------------------------------------------------------
    def byte_of(self, cls, rng):
        v = np.flatnonzero(self.equiv == cls)
        return int(v[rng.integers(0, v.size)])

    def walk(self, rng, accepts=1):
        """bytes along live transitions from the initial state up to the accepts-th accepting
        state whose result differs from the one before; None when the walk got stuck"""
        st, out, seen, prev = 1, bytearray(), 0, 0
        for _ in range(24):
            live = np.flatnonzero(self.trans[st])
            if live.size == 0:
                return None
            c = int(live[rng.integers(0, live.size)])
            out.append(self.byte_of(c, rng))
            st = int(self.trans[st, c])
            r = int(self.results[st])
            if r > 0 and r != prev:
                seen, prev = seen + 1, r
                if seen == accepts:
                    return bytes(out)
        return None

    def pieces(self, seed):
        rng = np.random.default_rng(seed)
        whole = [w for w in (self.walk(rng, 1) for _ in range(60)) if w][:6]
        twice = [w for w in (self.walk(rng, 2) for _ in range(200)) if w][:4]
        assert len(whole) == 6 and len(twice) >= 2
        out = whole + twice + whole[:3]
        out += [w[:1] for w in whole[:2]] + [w[:2] for w in whole[:2]]     # start byte; + follower
        k = len(self.leader)
        if k:
            lead = whole[0][:k]                      # (every walk begins with the forced leader)
            out += [lead, lead[:k - 1] + b"\x00"]    # the whole leader; cut one byte short
            out += [lead + w for w in whole[:3]]     # the attempt behind a consumed leader
            for j in range(1, k):
                out += [lead[:j] + w for w in whole[:3]]   # a leader cut short runs into a whole one
        return out


# name -> (constructor arguments, facts the row is in the table for)
_A = [ord("a") + k for k in range(26)]
_SIXTY4 = list(range(0x30, 0x30 + 64))
_SIXTY5 = list(range(0x30, 0x30 + 65))
_LD = 64                                             # classes of the leader DFAs
CRAFTED = {
    # packed list of 1, 2, 3, 4 start bytes; the second filter with 1, 4, 5 (disabled) and many
    "s1": (dict(n_states=200, n_cls=256, seed=11, start=_A[:1], second=[ord("x")]),
           dict(n1=1, n2=1, first_accepts=False)),
    "s2": (dict(n_states=200, n_cls=256, seed=12, start=_A[:2], second=[ord("w") + k for k in range(4)]),
           dict(n1=2, n2=4, first_accepts=False)),
    "s3": (dict(n_states=200, n_cls=256, seed=13, start=_A[:3], second=[ord("v") + k for k in range(5)]),
           dict(n1=3, n2=5, first_accepts=False)),
    "s4": (dict(n_states=256, n_cls=256, seed=14, start=_A[:4]), dict(n1=4, first_accepts=False)),
    # the flag table: 5 and 64 start bytes, its follower rule with 1 and 5 second bytes
    "s5": (dict(n_states=200, n_cls=256, seed=15, start=_A[:5], second=[ord("x")]),
           dict(n1=5, n2=1, first_accepts=False)),
    "s64": (dict(n_states=200, n_cls=256, seed=16, start=_SIXTY4, second=[ord("v") + k for k in range(5)]),
            dict(n1=64, n2=5, first_accepts=False)),
    "s65": (dict(n_states=200, n_cls=256, seed=17, start=_SIXTY5, second=[ord("v") + k for k in range(5)]),
            dict(n1=65, n2=5, first_accepts=False)),
    # a first step that accepts: no follower filter (list and table)
    "acc3": (dict(n_states=200, n_cls=256, seed=18, start=_A[:3], accept_first=True),
             dict(n1=3, first_accepts=True)),
    "acc5": (dict(n_states=200, n_cls=256, seed=19, start=_A[:5], accept_first=True),
             dict(n1=5, first_accepts=True)),
    # an accepting initial state, without and with a leader
    "init2": (dict(n_states=200, n_cls=256, seed=20, start=_A[:2], second=[ord("w") + k for k in range(4)],
                   init_result=3), dict(n1=2, n2=4, first_accepts=False)),
    "initld": (dict(n_states=200, n_cls=_LD, seed=21, sizes={5: 4}, leader=(5,), init_result=3),
               dict(lead1=4, n1=4)),
    # leaders of 1, 2 and 3 classes; a first class of 1, 4, 5, 64 bytes; the second class the same
    # as the first (aab's shape) or another one
    "ld1": (dict(n_states=200, n_cls=_LD, seed=22, sizes={5: 1}, leader=(5,)), dict(lead1=1, n1=1)),
    "ld2": (dict(n_states=200, n_cls=_LD, seed=23, sizes={5: 4, 6: 3}, leader=(5, 6)),
            dict(lead1=4, lead2=3, n1=4, n2=3)),
    "ld2t": (dict(n_states=200, n_cls=_LD, seed=24, sizes={5: 5, 6: 2}, leader=(5, 6)),
             dict(lead1=5, lead2=2, n1=5, n2=2)),
    "ld3": (dict(n_states=200, n_cls=_LD, seed=25, sizes={5: 64, 6: 1, 7: 2}, leader=(5, 6, 7)),
            dict(lead1=64, lead2=1, n1=64, n2=1)),
    "ld3same": (dict(n_states=200, n_cls=_LD, seed=26, sizes={5: 4, 7: 2}, leader=(5, 5, 7)),
                dict(lead1=4, lead2=4, n1=4, n2=4)),
    "ld3samet": (dict(n_states=200, n_cls=_LD, seed=27, sizes={5: 5, 7: 2}, leader=(5, 5, 7)),
                 dict(lead1=5, lead2=5, n1=5, n2=5)),
    # the placements
    "k2": (dict(n_states=270, n_cls=256, seed=28, start=_A[:3], second=[ord("w") + k for k in range(4)]),
           dict(n1=3, n2=4)),
    "k2big": (dict(n_states=285, n_cls=256, seed=29, start=_A[:3], second=[ord("w") + k for k in range(4)]),
              dict(n1=3, n2=4)),
    "k3": (dict(n_states=1500, n_cls=40, seed=30, sizes={5: 6, 6: 2}, leader=(5, 6)),
           dict(lead1=6, lead2=2, n1=6, n2=2)),
    "k5": (dict(n_states=80000, n_cls=4, seed=31, sizes={3: 3}, start=[3]), dict(n1=3)),
}
# regex DFAs: plants beside LP.PIECES'.  aab's leader is a, a, b: "aaab" is the line scan with the
# leader misses (the attempt at 0 consumes the second a) and search finds.
MORE_PIECES = {"aab": [b"aaab", b"aaaab", b"aa"], "num3": [b"12345a", b"987x", b"12"],
               "log100": [b"ERROR [net", b"EERROR [net] abc failed"]}

# ---- the guards' weaker bounds (section "What keeps a case from passing vacuously") ------------
# guard -> {DFA: (bound, reason)}; every other DFA meets the bound in the second column of _BOUNDS
_BOUNDS = dict(match=1 << 30, first_last=20, scan_search=20)
WEAKER = {
    # lines that must match under scan (the bound is a tenth of the lines otherwise)
    "match": {
        # aab's leader is the whole pattern: scan with the leader starts an attempt BEHIND it, in
        # the accepting post-leader state, and the next byte ends it with result 0 - only a line
        # that ends in aab matches
        "aab+lead": (50, "scan with the leader matches only where aab ends the line"),
    },
    "first_last": {
        **{n: (0, "one result value") for n in ("uri", "uri_user", "uri_v6", "aab")},
        # 100 results, anchored: a line's first and last accepting state belong to ONE signature
        "log100": (0, "an attempt accepts for one signature only"),
    },
    "scan_search": {},
}


def _bound(guard, name):
    return WEAKER[guard].get(name, (_BOUNDS[guard], ""))[0]


DFAS = dict(LP.DFAS)
_crafted = {}


def _crafted_dfa(name):
    if name not in _crafted:
        args, facts = CRAFTED[name]
        c = _Crafted(**args)
        got = c.facts()
        for k, v in facts.items():
            assert got[k] == v, (name, k, got[k], v)
        _crafted[name] = c
    return _crafted[name]


for _n in CRAFTED:
    DFAS[_n] = (lambda n: lambda: _crafted_dfa(n).blob)(_n)


# =================================================================================================
# 3. batches and expectations
# =================================================================================================
class _Batch:
    def __init__(self, key, data, off=None, stride=0):
        self.key, self.data, self.off, self.stride = key, data, off, stride
        self.n = len(off) - 1 if off is not None else len(data) // stride
        self.kw = dict(offsets=off) if off is not None else dict(stride=stride, n=self.n)
        self.lens = ((off[1:] - off[:-1]).astype(np.int64) if off is not None
                     else np.full(self.n, stride, dtype=np.int64))
        self._dev = None

    def dev(self):
        if self._dev is None:
            self._dev = (_t(self.data if len(self.data) else np.zeros(1, np.uint8)),
                         dict(offsets=_t(self.off)) if self.off is not None
                         else dict(stride=self.stride, n=self.n))
        return self._dev

    def sample(self, every=97):
        """every 97th line as a batch of its own, and the lines' numbers"""
        idx = np.arange(0, self.n, every)
        base = self.off[:-1].astype(np.int64) if self.off is not None else np.arange(self.n) * self.stride
        lens = self.lens[idx]
        off = _offsets(lens)
        src = np.repeat(base[idx] - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))
        return idx, self.data[src] if len(src) else np.zeros(0, np.uint8), off


def _quiet_pattern(cpu):
    """a short pattern whose repetition holds no match of any attempt (styInstant without the
    leader finds nothing)"""
    cands = [b" ", b".", b"\x00"] + [bytes([b]) for b in range(256)]
    cands += [bytes([a, b]) for a in range(16) for b in range(16)]
    cands += [bytes(int(d) for d in np.base_repr(v, 4).zfill(k)) for k in (3, 4) for v in range(4 ** k)]
    for pat in cands:
        probe = (pat * 3100)[:3100]
        if cpu.search(probe[:300], 1, False)[0] == 0 and cpu.search(probe, 1, False)[0] == 0:
            return pat
    raise AssertionError("no quiet filler")


class _Data:
    """One DFA: its checker, its batches and the oracle's answers, computed once and shared by the
    DFA's placements."""

    def __init__(self, name, index):
        self.name = name
        self.blob = DFAS[name]()
        self.cpu = O.CpuOracle(self.blob)
        self.ref = O.Reference(self.blob) if O.have_ref() else None
        self.info = one_amd.Executable(self.blob, device="none").info
        self.dense = self.info["n_pure_dead"] == 0
        self.quiet = _u8(_quiet_pattern(self.cpu))
        self.pieces = self._pieces()
        rng = np.random.default_rng(index)
        lens = np.concatenate([np.arange(131), rng.integers(0, 301, NL - 131),
                               rng.integers(1000, 3001, 3)]).astype(np.int64)
        rng.shuffle(lens)
        assert (lens <= 300).sum() == NL and set(range(131)) <= set(lens.tolist()) and (lens >= 1000).sum() == 3
        if self.dense:
            lens = lens[lens <= 300]
        self.ragged = _Batch("ragged", *self.fill(lens, 7))
        # the first stride, from the DFA's turn on, that holds its longest piece; a suffix-closed DFA
        # (scan and search run as check and match) takes none of whole 64-byte blocks, which would
        # bring in the streaming family's routes (test_gpu_multibatch, test_gpu_stream_resident)
        self.stride = [s for s in STRIDES[index % 4:] + STRIDES
                       if s >= max(len(p) for p in self.pieces) + 8 and
                       not (self.info["suffix_closed"] and s % 64 == 0)][0]
        self.fixed = _Batch("fixed%d" % self.stride, self.fill(np.full(NL, self.stride), 11)[0],
                            stride=self.stride)
        self.memo = {}
        self.results = set()
        self._guards()

    def _pieces(self):
        if self.name in CRAFTED:
            return [_u8(p) for p in _crafted_dfa(self.name).pieces(5)]
        if self.name in LP.PIECES:
            return [_u8(p) for p in LP.PIECES[self.name] + MORE_PIECES.get(self.name, [])]
        # a random DFA: matches cut out of random bytes
        out = []
        for k in range(400):
            w = W.random_bytes(24, 1000 + k).tobytes()
            r, s, e = self.cpu.search(w, 4, False)
            if r > 0:
                out.append(_u8(w[s:e]))
            if len(out) == 8:
                return out
        raise AssertionError("no pieces for " + self.name)

    def noise(self, n, seed):
        if self.name in LP.PIECES:
            return W.alphabet_bytes(max(n, 1), seed)[:n].copy()
        return W.random_bytes(max(n, 1), seed)[:n].copy()

    def fill(self, lens, seed):
        """Even lines carry a plant, odd ones none; the filler is quiet (no match of any attempt) or
        noise (alphabet text for the regex DFAs, random bytes for the others).  Plant k is piece
        k mod P at place (k div P) mod 4 - the line's first byte, its last, the buffer positions
        congruent to 15 and to 0 mod 16 (the marking sweep's 16-byte pieces) - in a quiet line when
        (k div 4P) is even; odd lines are quiet when i mod 4 is 1."""
        off = _offsets(lens)
        total = int(off[-1])
        data = self.noise(total, seed)
        rep = np.tile(self.quiet, total // len(self.quiet) + 1)
        P = len(self.pieces)
        k = 0
        for i, n in enumerate(lens):
            n, o = int(n), int(off[i])
            if i % 2:
                if i % 4 == 1:
                    data[o:o + n] = rep[:n]
                continue
            p, where, quiet = self.pieces[k % P], (k // P) % 4, (k // (4 * P)) % 2 == 0
            k += 1
            if quiet:
                data[o:o + n] = rep[:n]
            if len(p) > n:
                continue
            at = (0, n - len(p), (15 - o) % 16, (16 - o) % 16 + 16)[where]
            if at + len(p) > n:
                at = n - len(p)
            data[o + at:o + at + len(p)] = p
        return data, off

    def exp(self, b, verb, style, lead):
        k = (b.key, verb, style, lead)
        if k not in self.memo:
            got = self.cpu.batch(verb, style, lead, b.data, threads=THREADS, **b.kw)
            if self.ref is not None:
                idx, sdata, soff = b.sample()
                rr = self.ref.batch(verb, style, lead, sdata, offsets=soff)
                for g, r in zip(got, rr):
                    assert np.array_equal(g[idx], r), (self.name, b.key, verb, style, lead)
            self.memo[k] = got
        return self.memo[k]

    def _guards(self):
        for b in (self.ragged, self.fixed):
            for lead in LEADS:
                what = (self.name, b.key, lead)
                low = min(_bound("match", self.name + "+lead" if lead else self.name), b.n // 10)
                starts = ends = False
                for style in (1, 4):
                    r = self.exp(b, "scan", style, lead)[0]
                    assert (r > 0).sum() >= low and (r == 0).sum() >= b.n // 10, \
                        what + ("scan", style, int((r > 0).sum()), int((r == 0).sum()))
                    r, s, e = self.exp(b, "search", style, lead)
                    assert (r > 0).sum() >= b.n // 10 and (r == 0).sum() >= b.n // 10, \
                        what + ("search", style, int((r > 0).sum()), int((r == 0).sum()))
                    starts = starts or bool(((r > 0) & (s == 0)).any())
                    ends = ends or bool(((r > 0) & (e == b.lens.astype(np.uint64))).any())
                    self.results |= set(r.tolist())
                assert starts and ends, what + ("a match at a line's first / last byte", starts, ends)
                differ = int((self.exp(b, "scan", 2, lead)[0] != self.exp(b, "scan", 4, lead)[0]).sum())
                assert differ >= _bound("first_last", self.name), what + ("first/last", differ)
                if lead and self.info["leader_len"]:
                    differ = max(int((self.exp(b, "scan", style, 1)[0] !=
                                      self.exp(b, "search", style, 1)[0]).sum()) for style in STYLES)
                    assert differ >= _bound("scan_search", self.name), what + ("scan/search", differ)
        if _bound("first_last", self.name):
            assert len(self.results - {0}) > 1, self.name
        init = self.cpu.scan(b"", 4, False)
        if init > 0:
            # an accepting initial state: empty lines, lines without a start byte (both keep the
            # initial state's result) and lines where an attempt runs and fails (result 0)
            for b in (self.ragged, self.fixed):
                for lead in LEADS:
                    is_start = np.isin(b.data, list(_start_bytes(self.blob, self.cpu, lead)))
                    upto = np.concatenate([[0], np.cumsum(is_start)])
                    bounds = b.off.astype(np.int64) if b.off is not None else np.arange(b.n + 1) * b.stride
                    has = (upto[bounds[1:]] - upto[bounds[:-1]]) > 0
                    what = (self.name, b.key, lead)
                    lead = bool(lead and self.info["leader_len"])
                    for verb in ("scan", "search"):
                        r = self.exp(b, verb, 4, lead)[0]
                        empty, none = b.lens == 0, (b.lens > 0) & ~has
                        assert (r[empty] == init).all() and (r[none] == (init if lead else 0)).all(), what
                        assert empty.sum() >= (1 if b.off is not None else 0) and none.sum() >= 20, what
                        assert (has & (r == 0)).sum() >= 20, what + (verb, "no failed attempt")
                        if lead:
                            # ... and, with the leader, lines with a start byte that no attempt got past
                            assert (has & (r == init)).sum() >= 20, what + (verb, "leader never passed")


_datas = {}
_exes = {}


def _data(name):
    if name not in _datas:
        _datas[name] = _Data(name, sorted(DFAS).index(name))
    return _datas[name]


def _exe(dfa, opts, info=None):
    """the row's Executable; its placement and the facts the expected kernel name was worked out
    from are asserted"""
    key = (dfa, tuple(sorted(opts.items())))
    if key not in _exes:
        if len(_exes) > 3:
            _exes.clear()
        _exes[key] = one_amd.Executable(_data(dfa).blob, **opts)
    exe = _exes[key]
    got = exe.info
    for k, v in (info or {}).items():
        assert got[k] == v, (dfa, opts, k, got[k], v)
    return exe


def _h(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


AS = "check/match:"       # a table entry AS + family: scan runs as check, search as match


def _as_check_or_match(entry, d, b, verb, style, positions):
    """The kernel of a suffix-closed DFA without a leader (normalizeVerbStyle, then launchBatch):
    scan is check - under styLast when the style exits early and the DFA has one result and does
    not die early -, search is match.  These batches have fewer than 4,096 lines (no k_early, no
    k_style_blocks), no kind-1 table (no k_fixed) and no stride of whole 64-byte blocks (no
    k_stream), so only launchRaggedFamily is left before k_generic: ragged lines under styLast /
    styFull over the streaming class table ("cls") or the hot rows ("hot") - the rows
    test_gpu_match_text_placements.KERNELS names so."""
    family = entry[len(AS):]
    assert b.n < 4096 and (b.off is not None or b.stride % 64)
    if verb == "scan":
        positions = False
        if style in (1, 2, 3) and len(d.results - {0}) == 1 and not d.info["early_death"]:
            style = 4
    if not family or b.off is None or style not in (4, 5):
        return GENERIC
    mode = {(4, True): "last,start,end", (4, False): "last,end", (5, True): "full,start",
            (5, False): "full"}[style, positions]
    return "k_ragged<%s,%s>" % (mode, family)


def _named(kernel, what, got=None):
    got = one_amd.last_kernel() if got is None else got
    assert got == kernel, what + (got, kernel)


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("result", "start", "end")):
        if g is None:
            continue
        g = np.asarray(g)
        bad = np.flatnonzero(g.astype(e.dtype) != e)
        assert bad.size == 0 and len(g) == len(e), \
            what + (name, bad[:5].tolist(), g[bad[:5]].tolist(), e[bad[:5]].tolist())


def _scan(exe, d, b, style, lead, kernel, dev=False):
    exp = d.exp(b, "scan", style, lead)
    what = (d.name, b.key, "scan", style, lead, dev)
    if dev:
        ddata, dkw = b.dev()
        got = _h(one_amd.scan_batch(exe, ddata, style, bool(lead), **dkw))
    else:
        got = one_amd.scan_batch(exe, b.data, style, bool(lead), **b.kw)
    kernel_ran = one_amd.last_kernel()
    _same((got,), exp, what)             # (results first: a wrong name then shows beside right ones)
    if kernel.startswith(AS):
        kernel = _as_check_or_match(kernel, d, b, "scan", style, False)
    _named(kernel, what, kernel_ran)


def _search(exe, d, b, style, lead, kernel, dev=False, want_start=True):
    exp = d.exp(b, "search", style, lead)
    what = (d.name, b.key, "search", style, lead, dev, want_start)
    if dev:
        ddata, dkw = b.dev()
        got = one_amd.search_batch(exe, ddata, style, bool(lead), want_start=want_start, **dkw)
        got = [None if g is None else _h(g) for g in got]
    else:
        got = one_amd.search_batch(exe, b.data, style, bool(lead), want_start=want_start, **b.kw)
    kernel_ran = one_amd.last_kernel()
    assert (got[1] is None) == (not want_start), what
    _same(got, exp, what)
    if kernel.startswith(AS):
        kernel = _as_check_or_match(kernel, d, b, "search", style, want_start)
    _named(kernel, what, kernel_ran)


# =================================================================================================
# the table
# =================================================================================================
def _row(dfa, opts, info, free, lead, why):
    """free / lead: the kernel without and with the leader; why: the reasons, in that order"""
    tag = "+".join("%s=%s" % (k, v) if v is not True else k for k, v in opts.items()) or "default"
    return pytest.param(dfa, opts, info, (free, lead), why,
                        id="%s-%s-kind%d" % (dfa, tag, info["table_kind"]))


M, G = MARKED, GENERIC
_MM = (M, M, ("marked", "marked"))
_GG = (G, G, ("unmarkable", "unmarkable"))
_OW = ("other_verb", "other_verb")
# LP.ROWS' DFAs, by the restated rule (none of the markable ones comes near the LDS bound):
#   log100: E, W, I, D, F start a signature - 5 start bytes, the flag table; no leader
#   num3: the ten digits, with the leader and without; aab: "a"
#   uri_user, uri_v6, uri: loose starts - suffix-closed, no leader: check and match
#     (_as_check_or_match; the family by row, below)
#   rnd270, rnd270nd, rnd1500, rnd80k: 246, 256, 238, 256 start bytes
_LP_ROUTES = {"log100": _MM, "num3": _MM, "aab": _MM, "rnd270": _GG, "rnd270nd": _GG,
              "rnd1500": _GG, "rnd80k": _GG}
# launchRaggedFamily's table for the suffix-closed rows: uri_user's streaming class table (25 classes
# x 342 states), the 254 hot rows of uri_user under force_hot and of uri_v6; none under
# force_global (kind 4) and for uri with lds_table_max = 4096 (no hot row)
_AS_ROWS = {"uri_user-default-kind3": "cls", "uri_user-force_hot-kind6": "hot",
            "uri_user-force_global-kind4": "", "uri_v6-default-kind6": "hot",
            "uri_v6-force_global-kind4": "", "uri-lds_table_max=4096-kind6": ""}
HOT10 = dict(force_hot=True, lds_table_max=10240)


def _table():
    rows = []
    for p in LP.ROWS:
        dfa, opts, info = p.values
        if p.id in _AS_ROWS:
            rows.append(_row(dfa, opts, info, AS + _AS_ROWS[p.id], AS + _AS_ROWS[p.id], _OW))
        else:
            rows.append(_row(dfa, opts, info, *_LP_ROUTES[dfa]))
    k1 = dict(table_kind=1)
    for name in CRAFTED:
        if name in ("k2", "k2big", "k3", "k5", "s65"):
            continue
        rows.append(_row(name, {}, k1, *_MM))
    rows += [
        _row("s65", {}, k1, *_GG),
        _row("s2", dict(force_generic=True), k1, G, G, ("force_generic", "force_generic")),
        _row("ld3", dict(force_generic=True), k1, G, G, ("force_generic", "force_generic")),
        _row("s2", dict(force_global=True), dict(table_kind=4), *_MM),
        _row("ld2t", dict(force_global=True), dict(table_kind=4), *_MM),
        # 512 + 138,240 + 1,088 + 16,672 = 156,512 <= 161,792
        _row("k2", {}, dict(table_kind=2, states_used=270, table_bytes=138240), *_MM),
        _row("k2", HOT10, dict(table_kind=6, states_used=270, n_hot=40), *_MM),
        # 512 + 145,920 + 1,152 + 16,672 = 164,256 > 161,792; k_generic: 512 + 147,072 = 147,584
        _row("k2big", {}, dict(table_kind=2, states_used=285, table_bytes=145920), G, G, ("lds", "lds")),
        # 512 + 120,000 + 6,000 + 16,672 = 143,184
        _row("k3", {}, dict(table_kind=3, states_used=1500, table_bytes=120000), *_MM),
        _row("k3", HOT10, dict(table_kind=6, states_used=1500), *_MM),
        _row("k5", {}, dict(table_kind=5, states_used=80000), *_MM),
    ]
    return rows


TABLE = _table()


def test_table_covers_every_route():
    """k_scan_marked rows at every table kind; k_generic rows for each reason: not markable,
    force_generic, the marks not fitting LDS; the flag table and the list, with and without a
    leader; and the crafted facts the rows are there for"""
    marked = [p.values for p in TABLE if MARKED in p.values[3]]
    assert {v[2]["table_kind"] for v in marked} == {1, 2, 3, 4, 5, 6, 7}
    reasons = {w for p in TABLE for k, w in zip(p.values[3], p.values[4]) if k == GENERIC}
    assert reasons == {"unmarkable", "force_generic", "lds"}
    for p in TABLE:
        for k, w in zip(p.values[3], p.values[4]):
            assert (k == MARKED) == (w == "marked") and k.startswith(AS) == (w == "other_verb"), p.id
    facts = {n: _crafted_dfa(n).facts() for n in CRAFTED}
    assert {f["n1"] for f in facts.values()} >= {1, 2, 3, 4, 5, 64, 65}
    assert {f["lead1"] for f in facts.values()} >= {1, 4, 5, 64}
    assert {len(_crafted_dfa(n).leader) for n in CRAFTED} >= {0, 1, 2, 3}
    free = [f for n, f in facts.items() if not _crafted_dfa(n).leader]
    assert any(f["first_accepts"] for f in free)
    assert {f["n2"] for f in free if not f["first_accepts"]} >= {1, 4, 5}
    for n in ("init2", "initld"):
        assert _crafted_dfa(n).results[1] > 0


@pytest.mark.parametrize("dfa,opts,info,kernels,why", TABLE)
def test_scan_and_search_under_placement(dfa, opts, info, kernels, why):
    d = _data(dfa)
    exe = _exe(dfa, opts, info)
    gen = exe if opts.get("force_generic") else _exe(dfa, dict(opts, force_generic=True), info)
    for lead in LEADS:
        kernel, reason = _route(d.blob, d.cpu, exe.info, opts, lead)
        assert reason == why[lead], (dfa, lead, reason)
        assert kernels[lead].startswith(AS) if kernel is None else kernel == kernels[lead], (dfa, lead)
    forced = [GENERIC for k in kernels]           # (every family declines under force_generic)
    for b in (d.ragged, d.fixed):
        for style in STYLES:
            for lead in LEADS:
                for e, names in ((exe, kernels), (gen, forced)):
                    _scan(e, d, b, style, lead, names[lead])
                    _search(e, d, b, style, lead, names[lead])
                    _search(e, d, b, style, lead, names[lead], want_start=False)


# =================================================================================================
# 4. the kernel's forms, each reached by construction
# =================================================================================================
def _forms_dfa():
    """acc3: a first step that accepts - no follower filter, so a group's candidate count is the
    number of start bytes inside its lines"""
    d = _data("acc3")
    c = _crafted_dfa("acc3")
    f = c.facts()
    assert f["first_accepts"] and f["n1"] == 3
    return d, _exe("acc3", {}, dict(table_kind=1)), _u8(bytes(f["starts"]))


def _run_all(exe, d, b, kernel, styles=STYLES, leads=LEADS, dev=False):
    for style in styles:
        for lead in leads:
            _scan(exe, d, b, style, lead, kernel, dev=dev)
            _search(exe, d, b, style, lead, kernel, dev=dev)


def _placed(d, starts, lens, count, seed, one_line=None):
    """lines of quiet filler (no start byte) with exactly `count` start bytes, at distinct random
    positions (all inside line `one_line` when given)"""
    off = _offsets(lens)
    total = int(off[-1])
    data = np.tile(d.quiet, total // len(d.quiet) + 1)[:total].copy()
    assert not np.isin(data, starts).any()
    rng = np.random.default_rng(seed)
    lo, hi = (0, total) if one_line is None else (int(off[one_line]), int(off[one_line + 1]))
    at = lo + rng.choice(hi - lo, size=count, replace=False)
    data[at] = starts[rng.integers(0, len(starts), count)]
    assert int(np.isin(data, starts).sum()) == count
    return data, off


@pytest.mark.parametrize("form,count", [("spread", 0), ("spread", 1), ("spread", 255), ("spread", 256),
                                        ("spread_one_line", 256), ("own", 257), ("own_one_line", 257),
                                        ("own_all", None)])
def test_visiting_forms(form, count):
    """One call of at most 256 lines spanning at most 65,536 bytes is one workgroup (mb = ceil(n /
    256) = 1) with one group.  `if (total <= uint32_t(kThreads))` (k_scan_marked.h) decides: up to
    256 candidates are spread one per thread - also when all 256 sit in one line -, 257 and more are
    visited by their own lines' lanes."""
    d, exe, starts = _forms_dfa()
    lens = 20 + (np.arange(200) * 7) % 41
    lens[::17] = 0
    if form == "own_all":
        off = _offsets(lens)
        data = starts[np.random.default_rng(3).integers(0, 3, int(off[-1]))].copy()
        count = int(off[-1])
    else:
        one = int(np.argmax(lens >= 60)) if form.endswith("one_line") else None
        if one is not None:
            lens[one] = 300
        data, off = _placed(d, starts, lens, count, 5, one)
    assert len(lens) <= 256 and int(off[-1]) <= 65536 - 16
    assert int(np.isin(data, starts).sum()) == count and (count <= 256) == form.startswith("spread")
    b = _Batch("%s%d" % (form, count), data, off)
    r = d.exp(b, "scan", 1, 0)[0]
    assert int((r > 0).sum()) == len({int(k) for k in np.searchsorted(off, np.flatnonzero(np.isin(data, starts)),
                                                                   side="right")})
    _run_all(exe, d, b, MARKED)
    _run_all(exe, d, b, MARKED, styles=(1, 4), dev=True)


@pytest.mark.parametrize("dfa", ["s2", "ld2", "init2"])
def test_start_byte_on_the_last_byte_of_the_sweep(dfa):
    """The packed list's follower filter is switched off for the last 16-byte piece of a group's
    sweep (`if (k + 1 >= pieces) f.n2 = 0`), whose last byte has no follower in hand.  A line's last
    position walks the same with or without a mark - one step that cannot accept, or a leader cut
    short - so only agreement with the oracle can be asked for: groups that end on a 16-byte border
    with a start byte, behind first bytes that may and may not follow one."""
    d = _data(dfa)
    exe = _exe(dfa, {}, dict(table_kind=1))
    start = min(_start_bytes(d.blob, d.cpu, 0) & _start_bytes(d.blob, d.cpu, 1))
    for first in (int(d.pieces[0][1]), int(d.quiet[0]), start):
        for n_lines in (1, 7):
            data = np.tile(d.quiet, 16 * n_lines)[:16 * n_lines].copy()
            data[15::16] = start
            data[-16] = first
            b = _Batch("last%d_%d" % (first, n_lines), data, stride=16)
            _run_all(exe, d, b, MARKED)
            _run_all(exe, d, b, MARKED, styles=(1, 4), dev=True)


HALVING = {
    # 76,800 bytes: 128 lines are 38,400
    "once": [300] * 256,
    # 256,000 -> 128,000 -> 64,000
    "twice": [1000] * 256,
    # the first 128 lines fit; then 128 -> 64; then 64 -> 32 -> 16: the long line ends a group of 16
    # lines (15 * 200 + 60,000 = 63,000 bytes): with neighbours this short it cannot stand alone
    "long_last": [200] * 255 + [60000],
    # 6,000 + 60,000 > 65,536 on either side: halved down to the long line alone, which the bitmap
    # still covers
    "long_alone": [100] * 100 + [6000, 60000, 6000] + [100] * 100,
}


@pytest.mark.parametrize("which", sorted(HALVING))
@pytest.mark.parametrize("dfa", ["s2", "ld2t"])
def test_batch_halving(dfa, which):
    d = _data(dfa)
    exe = _exe(dfa, {}, dict(table_kind=1))
    lens = np.array(HALVING[which])
    assert len(lens) <= 256 and lens.sum() > 65536 and lens.max() < 65536 - 16
    b = _Batch(which, *d.fill(lens, 21))
    for lead in LEADS:
        r = d.exp(b, "search", 4, lead)[0]
        assert 10 <= (r > 0).sum() <= b.n - 10, (dfa, which, lead)
    _run_all(exe, d, b, MARKED)


def _planted_line(d, n, seed):
    """a line of n bytes with a match at its first bytes and one ending on its last byte"""
    line = d.fill(np.array([n]), seed)[0]
    p = d.pieces[0]
    r, s, e = d.cpu.search(p.tobytes(), 4, False)
    assert r > 0 and (s, e) == (0, len(p))
    line[:len(p)] = p
    line[n - len(p):] = p
    return line


@pytest.mark.parametrize("n", [65535, 65536, 65537])
@pytest.mark.parametrize("dfa", ["s2", "ld2t"])
def test_the_64_kib_edge(dfa, n):
    """One line as a device tensor whose first byte sits at 0, 1 and 15 mod 16.  tooLong is
    (address mod 16) + n > 65,536: false for (65,535; 0), (65,535; 1) and (65,536; 0) - the bitmap
    covers the line - and true for the other six, which one lane walks the old way."""
    import torch
    d = _data(dfa)
    exe = _exe(dfa, {}, dict(table_kind=1))
    line = _planted_line(d, n, n)
    b = _Batch("edge%d" % n, line, _offsets([n]))
    for lead in LEADS:
        r, s, e = d.exp(b, "search", 1, lead)
        assert r[0] > 0 and s[0] == 0
        r, s, e = d.exp(b, "search", 4, lead)
        assert r[0] > 0
    too_long = []
    doff = _t(b.off)
    for k in (0, 1, 15):
        buf = torch.full((k + n + 64,), int(d.pieces[0][0]), dtype=torch.uint8, device="cuda")
        buf[k:k + n] = torch.from_numpy(line)
        view = buf[k:k + n]
        assert view.data_ptr() % 16 == k
        too_long.append(k + n > 65536)
        for style in STYLES:
            for lead in LEADS:
                what = (dfa, n, k, style, lead)
                got = _h(one_amd.scan_batch(exe, view, style, bool(lead), offsets=doff))
                _named(MARKED, what)
                _same((got,), d.exp(b, "scan", style, lead), what)
                got = one_amd.search_batch(exe, view, style, bool(lead), offsets=doff)
                _named(MARKED, what)
                _same([_h(g) for g in got], d.exp(b, "search", style, lead), what)
    assert too_long == {65535: [False, False, True], 65536: [False, True, True], 65537: [True] * 3}[n]
    # the tail of a line whose match ends on its last byte, searched from a late start
    tail = _Batch("edge_tail%d" % n, line, np.array([0, n - 40, n], dtype=np.uint64))
    _run_all(exe, d, tail, MARKED, styles=(1, 4), dev=True)


@pytest.mark.parametrize("dfa", ["s2", "ld2t"])
def test_a_line_beyond_the_bitmap_among_short_ones(dfa):
    d = _data(dfa)
    exe = _exe(dfa, {}, dict(table_kind=1))
    lens = np.array([5] * 100 + [70000] + [0] * 50 + [17] * 100)
    data, off = d.fill(lens, 31)
    data[int(off[100]):int(off[101])] = _planted_line(d, 70000, 32)
    b = _Batch("beyond", data, off)
    assert d.exp(b, "search", 4, 0)[0][100] > 0
    _run_all(exe, d, b, MARKED)


@pytest.mark.parametrize("stride,n", [(1, 600), (5, 600), (15, 600), (16, 600), (17, 600), (255, 256),
                                      (256, 256), (257, 256), (255, 768), (256, 768), (257, 768),
                                      (255, 600), (257, 600), (70000, 3)])
def test_fixed_strides(stride, n):
    """A workgroup's share is lines n * blockIdx / gridDim onwards, with gridDim = ceil(n / 256): 256
    lines (one workgroup) and 768 (three) give every workgroup a group of 256 lines, 600 lines
    give 200 each.  A group of 256 lines starts on a 16-byte border of the staged buffer, so it
    spans 256 * stride bytes: 65,280 at 255 (fits), 65,536 at 256 (fills the bitmap exactly, not
    halved: the test is `>`), 65,792 at 257 (overflows it by 256: halved to 128 lines).  70,000:
    every line is beyond the bitmap."""
    per_group = min(256, n // -(-n // 256))
    if n in (256, 768):
        assert per_group == 256 and n % 256 == 0
        assert (256 * stride > 65536) == (stride == 257) and (256 * stride == 65536) == (stride == 256)
    elif stride < 1000:
        assert per_group * stride <= 65536
    for dfa in ("s2", "ld2t"):
        d = _data(dfa)
        exe = _exe(dfa, {}, dict(table_kind=1))
        b = _Batch("stride%d_%d" % (stride, n), d.fill(np.full(n, stride), 40 + stride)[0], stride=stride)
        r = d.exp(b, "search", 4, 1)[0]
        assert (r > 0).any() or stride < 5, (dfa, stride)
        if n in (256, 768):
            # matches on both sides of the halving point, line 128 of each group
            g = r.reshape(-1, 256)
            assert ((g[:, :128] > 0).sum(axis=1) >= 5).all() and ((g[:, 128:] > 0).sum(axis=1) >= 5).all()
        _run_all(exe, d, b, MARKED, styles=(1, 2, 4) if stride > 1000 else STYLES)


@pytest.mark.parametrize("n", [2501, 600000])
def test_above_the_grid(n):
    """600,000 lines: more than 256 x 8 x CUs for any CU count of this part, so a workgroup walks
    several groups whose first line is no multiple of 256; 2,501 lines: ten workgroups of 250 or
    251 lines.  scan with the leader, search without."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == 2501 or n > 256 * 8 * cus
    d = _data("ld2t")
    exe = _exe("ld2t", {}, dict(table_kind=1))
    rng = np.random.default_rng(n)
    lens = rng.integers(4, 13, n)
    # the lines, drawn from 4,096 distinct ones
    pool = _Batch("pool", *d.fill(np.full(4096, 12), 51), )
    pick = rng.integers(0, 4096, n)
    off = _offsets(lens)
    src = np.repeat(pick * 12 - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]))
    b = _Batch("grid%d" % n, pool.data[src], off)
    ddata, dkw = b.dev()
    exp = d.cpu.batch("scan", 4, 1, b.data, offsets=off, threads=THREADS)[0]
    assert n // 50 <= (exp > 0).sum() <= n - n // 50
    got = _h(one_amd.scan_batch(exe, ddata, 4, True, **dkw))
    _named(MARKED, ("scan", n))
    _same((got,), (exp,), ("scan", n))
    exp = d.cpu.batch("search", 1, 0, b.data, offsets=off, threads=THREADS)
    assert n // 50 <= (exp[0] > 0).sum() <= n - n // 50
    got = [_h(g) for g in one_amd.search_batch(exe, ddata, 1, False, **dkw)]
    _named(MARKED, ("search", n))
    _same(got, exp, ("search", n))


# =================================================================================================
# 5. device-resident calls: misaligned input, caller-owned outputs, a second stream
# =================================================================================================
def _sentinel(n, dtype):
    import torch
    return torch.full((n * dtype.itemsize,), SENT, dtype=torch.uint8, device="cuda").view(dtype)


def _untouched(t):
    import torch
    return bool((t.contiguous().view(torch.uint8) == SENT).all().item())


@pytest.mark.parametrize("dfa,opts,kind", [("s2", {}, 1), ("ld2t", {}, 1), ("ld3", {}, 1), ("init2", {}, 1),
                                           ("aab", dict(force_global=True), 4), ("k2big", {}, 2)])
def test_device_resident_calls(dfa, opts, kind):
    """the text as a slice at 0, 1 and 15 mod 16 of a tensor with 64 guard bytes of a start byte on
    either side (memory the sweep may read, bytes that must never show in a result); the outputs
    as slices of sentinel-filled tensors; one setting on a second stream"""
    import torch
    d = _data(dfa)
    exe = _exe(dfa, opts, dict(table_kind=kind))
    kernel = _route(d.blob, d.cpu, exe.info, opts, 0)[0]
    assert kernel == _route(d.blob, d.cpu, exe.info, opts, 1)[0] == (GENERIC if dfa == "k2big" else MARKED)
    guard = min(_start_bytes(d.blob, d.cpu, 0) & _start_bytes(d.blob, d.cpu, 1))
    side = torch.cuda.Stream()
    pad = 24
    for b in (d.ragged, d.fixed):
        n, size = b.n, len(b.data)
        kw = dict(offsets=_t(b.off)) if b.off is not None else dict(stride=b.stride, n=n)
        for k in (0, 1, 15):
            buf = torch.full((64 + 16 + size + 64,), guard, dtype=torch.uint8, device="cuda")
            lo = 64 + k
            buf[lo:lo + size] = torch.from_numpy(b.data)
            view = buf[lo:lo + size]
            assert view.data_ptr() % 16 == k
            for style in (STYLES if k == 15 else (1, 4)):
                for lead in LEADS:
                    what = (dfa, b.key, k, style, lead)
                    second = k == 1 and style == 4
                    with torch.cuda.stream(side if second else torch.cuda.current_stream()):
                        if second:
                            side.wait_stream(torch.cuda.default_stream())
                        res = _sentinel(n + 2 * pad, torch.int32)
                        one_amd.scan_batch(exe, view, style, bool(lead), out=res[pad:pad + n], **kw)
                        _named(kernel, what)
                        sres = _sentinel(n + 2 * pad, torch.int32)
                        st = _sentinel(n + 2 * pad, torch.int64)
                        en = _sentinel(n + 2 * pad, torch.int64)
                        one_amd.search_batch(exe, view, style, bool(lead),
                                             out=(sres[pad:pad + n], st[pad:pad + n], en[pad:pad + n]), **kw)
                        _named(kernel, what)
                        if second:
                            side.synchronize()
                    for t in (res, sres, st, en):
                        assert _untouched(t[:pad]) and _untouched(t[pad + n:]), what
                    _same((_h(res[pad:pad + n]),), d.exp(b, "scan", style, lead), what + ("scan",))
                    _same([_h(t[pad:pad + n]) for t in (sres, st, en)], d.exp(b, "search", style, lead),
                          what + ("search",))
            torch.cuda.synchronize()
