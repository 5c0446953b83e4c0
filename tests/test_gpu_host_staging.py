"""The layer in front of the kernels: the host-buffer forms' staging (HostCall in redgpu.cpp,
HostStage::move in host_stage.cpp), on every route - caller-pinned memory (route 0), the thread's
pinned arena (route 1), whole pages registered for the call with the partial end pages through the
arena (route 2) - at the 8 MiB call threshold, the 16 MiB transfer threshold, page offsets 0, 1 and
4095, behind one another on one thread, and under redgpu_dfa_tune.  The arithmetic itself is held
against a brute-force rule on the CPU (tests/test_host_stage_plan.py); here the routes are COUNTED
(redgpu_host_route_counts) and the answers compared with the oracle.

Conventions of every test:
  * expectations come from the oracle: CpuOracle.batch for the batch verbs, periodic_text's expansion
    of the oracle's answer for the text verbs (tests/test_periodic_expectation.py proves it);
  * where the test places the caller's buffers (tests a, b, c, e, f, g) they are views into ONE
    page-aligned backing array, back to back, so neighbours share pages; 64 fence bytes stand in
    front of and behind every one and are checked after the call, and outputs are pre-filled with a
    pattern that must survive behind the promised prefix;
  * around every call the route counts' delta is taken: "handed over pageable" never moves, and
    redgpu_host_pins_held() is 0 after every call.

The transfers of each form, counted in redgpu.cpp (the small ones that end in the library's own
stack variables or vectors are pageable memory too and take the arena):
  match_batch (fixed stride, one chunk)  data up; result, start, end down                      = 4
              (+ 1 with offsets; per chunk the four again when the batch is cut)
  replace_text   data, repl up; the three sizes down; out down                                  = 4
  collect_text   data up; the two counts down; line, begin, result, start, end down            = 7
  tally_text (accumulate)  data up; the two counts down; the bins down (into a vector)         = 3
  dfa_tune       data up (the histogram comes back inside the _dev form, not through the stage) = 1
  advance_batch  data, state up; state back into the same buffer, result down                  = 4

Which test reaches which of the 26 host forms that stage through HostCall, on which route (0 caller-
pinned, 1 arena, 2 registered; the forms' few-byte counts and sizes take route 1 in every call):
  match_batch                 0: caller_pinned_memory (chunked, one chunk, mixed); 1: small_calls,
                              call_threshold[below], transfer_threshold, size_ladder; 2: call_threshold[at],
                              transfer_threshold[outputs-above], size_ladder, tune (the calls behind it)
  replace_text, collect_text, 1: small_calls, call_threshold[below] (replace_text: size_ladder too);
  tally_text                  2: call_threshold[at], text_verbs_on_the_registered_route
  grep_text, filter_text, extract_text, fields_text, route_text, uniq_text, range_text, sum_text,
  match_text, split_lines, collect_long, match_all_long, replace_long, search_long
                              2: text_verbs_on_the_registered_route (their outputs are the Python
                              form's own arrays; 1 is what every older test of theirs takes)
  check_batch, scan_batch, search_batch, collect_batch, match_all_batch, replace_batch
                              2: batch_verbs_on_the_registered_route
  advance_batch               2: a_buffer_that_goes_up_and_comes_back
  dfa_tune                    2: tune_with_a_large_sample_leaves_nothing_behind
Route 0 is reached through match_batch alone (runHost passes `direct`); no test hands pinned memory
to another form, or memory that is pinned only in part.
"""
import numpy as np
import pytest

import one_amd
from one_amd import _lib
from one_amd import workloads as W
import oracle as O
from golden_util import load_dfa

import periodic_text as PT

pytestmark = pytest.mark.gpu

PAGE, GUARD = 4096, 64
FILL, FENCE = 0xA5, 0x5C
MIB = 1 << 20
DIRECT_FROM, BOUNCE_MAX, MIN_PAGES = 8 * MIB, 16 * MIB, 16    # one_amd/csrc/host_stage_plan.h
FORMS = ["match_batch", "replace_text", "collect_text", "tally_text"]
REPLACE = ("replace", "dense", "err", b"<error!>", PT.ALL, 0)
COLLECT = ("collect", "dense", "log100")
TALLY = ("tally", "dense", "log100", 101, True)

_exes, _cpus = {}, {}


def _blob(name):
    import test_gpu_fields_text as FL
    return FL._blob(name) if name in ("err", "log100", "num3", "uri", "newyork", "ws", "comma") \
        else load_dfa(name)


def _exe(name):
    if name not in _exes:
        _exes[name] = one_amd.Executable(_blob(name))
    return _exes[name]


def _cpu(name):
    if name not in _cpus:
        _cpus[name] = O.CpuOracle(_blob(name))
    return _cpus[name]


class Arena:
    """caller buffers carved back to back out of one page-aligned backing array"""

    def __init__(self, nbytes, backing=None):
        room = nbytes + 2 * PAGE
        self.raw = np.empty(room, dtype=np.uint8) if backing is None else backing
        assert self.raw.dtype == np.uint8 and self.raw.nbytes >= room
        skip = -self.raw.ctypes.data % PAGE
        self.mem = self.raw[skip:skip + (self.raw.nbytes - skip) // PAGE * PAGE]
        assert self.mem.ctypes.data % PAGE == 0 and self.mem.nbytes % PAGE == 0
        self.at, self.fences = 0, []

    def carve(self, count, dtype, page_off=None, fill=False):
        """count entries of dtype: at byte page_off of a page, else 8-byte aligned behind the last"""
        size = int(count) * np.dtype(dtype).itemsize
        lo = self.at + GUARD
        lo += (page_off - lo) % PAGE if page_off is not None else -lo % 8
        hi = lo + size
        assert hi + GUARD <= self.mem.nbytes, "arena too small"
        self.mem[lo - GUARD:lo] = FENCE
        self.mem[hi:hi + GUARD] = FENCE
        self.fences.append((lo, hi))
        self.at = hi + GUARD
        view = self.mem[lo:hi]
        if fill:
            view[:] = FILL
        return view.view(dtype)

    def check(self):
        for lo, hi in self.fences:
            assert (self.mem[lo - GUARD:lo] == FENCE).all(), ("bytes in front of a buffer written", lo)
            assert (self.mem[hi:hi + GUARD] == FENCE).all(), ("bytes behind a buffer written", hi)


def _untouched(view, frm):
    """the pattern survives from entry `frm` on"""
    return bool((view[frm:].view(np.uint8) == FILL).all())


class Routes:
    """the route counts' delta of the calls inside; nothing pageable, nothing held afterwards"""

    def __enter__(self):
        self.before = one_amd.host_route_counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            after = one_amd.host_route_counts()
            self.delta = tuple(a - b for a, b in zip(after, self.before))
            assert self.delta[3] == 0, ("handed over pageable", self.delta)
            assert one_amd.host_pins_held() == 0
        return False


def _route(buf, nbytes, input_bytes):
    """the route of one transfer of PAGEABLE memory (buf None: the library's own few bytes)"""
    if input_bytes < DIRECT_FROM and nbytes <= BOUNCE_MAX:
        return 1
    if buf is None:
        return 1
    a = buf.ctypes.data
    whole = (a + nbytes) // PAGE - -(-a // PAGE)
    return 2 if whole >= MIN_PAGES else 1


def _delta(transfers, input_bytes):
    d = [0, 0, 0, 0]
    for buf, nbytes in transfers:
        if nbytes:
            d[_route(buf, nbytes, input_bytes)] += 1
    return tuple(d)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


# the four forms with placed buffers: each returns (delta, transfers, input bytes) -----------------

def _match_batch(name, arena, src, stride, n, offsets=None, page_off=None, outs=None, keep=None,
                 style=4, lead=0):
    """redgpu_match_batch over src (fixed stride, or offsets - a view into the arena when given as
    keep=(data, offsets) from an earlier call) against CpuOracle.batch"""
    outs = outs or arena
    if keep is None:
        data = arena.carve(src.size, np.uint8, page_off)
        data[:] = src
        offs = None
        if offsets is not None:
            offs = arena.carve(len(offsets), np.uint64)
            offs[:] = offsets
    else:
        data, offs = keep
    res = outs.carve(n + 8, np.int32, fill=True)
    st = outs.carve(n + 8, np.uint64, fill=True)
    en = outs.carve(n + 8, np.uint64, fill=True)
    with Routes() as r:
        rc = _lib.lib().redgpu_match_batch(_exe(name)._h, style, lead, _ptr(data), _ptr(offs),
                                           stride, n, _ptr(res), _ptr(st), _ptr(en))
    assert rc == _lib.OK, _lib.lib().redgpu_last_error()
    if offs is not None:
        want = _cpu(name).batch("match", style, lead, data, offsets=offs.copy(), threads=8)
    else:
        want = _cpu(name).batch("match", style, lead, data, stride=stride, n=n, threads=8)
    for got, exp, key in zip((res, st, en), want, ("result", "start", "end")):
        assert np.array_equal(got[:n], exp), (key, n, stride)
        assert _untouched(got, n), (key, "written behind n")
    arena.check()
    outs.check()
    moved = [(offs, (n + 1) * 8)] if offs is not None else []
    total = int(offs[n]) if offs is not None else stride * n
    first = int(offs[0]) if offs is not None else 0
    moved += [(data[first:], total - first), (res, n * 4), (st, n * 8), (en, n * 8)]
    return r.delta, moved, total, (data, offs)


def _lead_to(lay0, target):
    """(K, lead): lead + block * K + tail has exactly `target` bytes; the lead is lines of '~'"""
    K = (target - len(lay0.tail)) // lay0.P
    assert K >= 3, "too short for the periodic expansion"
    d = target - K * lay0.P - len(lay0.tail)
    lead = b""
    while len(lead) < d:
        n = min(64, d - len(lead))
        lead += b"~" * (n - 1) + b"\n"
    return K, lead


def _text_and_answer(case, target):
    """a text of exactly `target` bytes and the oracle's answer for it"""
    lay0 = PT.layout(case[1], case[2])
    if target >= 3 * lay0.P + len(lay0.tail):
        K, lead = _lead_to(lay0, target)
        text = lay0.with_lead(lead).text(K)
        x = PT.expected(case, K, lead)
    else:       # a short text: whole lines of the block and an unterminated rest, the oracle directly
        cut = lay0.block.rfind(b"\n", 0, max(1, target - 8)) + 1
        text = lay0.block[:cut] + (b"left over " * (target // 10 + 1))[:target - cut]
        x = PT.whole(PT.answer(case, text))
    assert len(text) == target, (len(text), target)
    return text, x


def _place_text(arena, text, page_off):
    data = arena.carve(len(text), np.uint8, page_off)
    data[:] = np.frombuffer(text, dtype=np.uint8)
    return data


def _replace_text(arena, target, page_off=None):
    _, _, name, repl, mx, oc = REPLACE
    text, x = _text_and_answer(REPLACE, target)
    want = x.streams["out"].numpy().tobytes()
    data = _place_text(arena, text, page_off)
    rp = arena.carve(len(repl), np.uint8)
    rp[:] = np.frombuffer(repl, dtype=np.uint8)
    nums = arena.carve(3, np.uint64, fill=True)
    cap = len(want) + 40
    out = arena.carve(cap, np.uint8, fill=True)
    with Routes() as r:
        rc = _lib.lib().redgpu_replace_text(
            _exe(name)._h, PT.LAST, 1, oc, _ptr(data), len(text), PT.DELIM, _ptr(rp), len(repl), mx,
            nums.ctypes.data, nums.ctypes.data + 8, nums.ctypes.data + 16, _ptr(out), cap)
    assert rc == _lib.OK, _lib.lib().redgpu_last_error()
    assert nums.tolist() == [x.counts["n_lines"], x.counts["n_replaced"], len(want)], target
    assert out[:len(want)].tobytes() == want, target
    assert _untouched(out, len(want))
    arena.check()
    return r.delta, [(data, len(text)), (rp, len(repl)), (None, 24), (out, len(want))], len(text)


def _collect_text(arena, target, page_off=None):
    name = COLLECT[2]
    text, x = _text_and_answer(COLLECT, target)
    total = x.counts["n_rows"]
    cap = total + 8
    data = _place_text(arena, text, page_off)
    nums = arena.carve(2, np.uint64, fill=True)
    cols = {k: arena.carve(cap, np.int32 if k == "result" else np.uint64, fill=True)
            for k in ("line", "begin", "result", "start", "end")}
    with Routes() as r:
        rc = _lib.lib().redgpu_collect_text(
            _exe(name)._h, _ptr(data), len(text), PT.DELIM, cap, nums.ctypes.data,
            nums.ctypes.data + 8, *(_ptr(cols[k]) for k in ("line", "begin", "result", "start", "end")))
    assert rc == _lib.OK, _lib.lib().redgpu_last_error()
    assert nums.tolist() == [x.counts["n_lines"], total] and total > 100, target
    for k, got in cols.items():
        assert np.array_equal(got[:total].astype(np.int64), x.rows[k].numpy().astype(np.int64)), (k, target)
        assert _untouched(got, total), (k, "written behind the records")
    arena.check()
    moved = [(data, len(text)), (None, 16)] + [(got, total * got.itemsize) for got in cols.values()]
    return r.delta, moved, len(text)


def _tally_text(arena, target, page_off=None):
    _, _, name, n_bins, matches = TALLY
    text, x = _text_and_answer(TALLY, target)
    data = _place_text(arena, text, page_off)
    nums = arena.carve(2, np.uint64, fill=True)
    bins = arena.carve(n_bins + 1, np.uint64)
    base = np.arange(n_bins + 1, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    bins[:] = base
    with Routes() as r:
        rc = _lib.lib().redgpu_tally_text(
            _exe(name)._h, one_amd.matcher.TALLY_MATCHES, PT.INSTANT, 1, _ptr(data), len(text),
            PT.DELIM, n_bins, 1, nums.ctypes.data, nums.ctypes.data + 8, _ptr(bins))
    assert rc == _lib.OK, _lib.lib().redgpu_last_error()
    assert nums.tolist() == [x.counts["n_lines"], x.counts["n_items"]], target
    assert (bins.astype(np.int64) - base.astype(np.int64)).tolist() == x.counts["bins"].tolist(), target
    assert int(x.counts["bins"].sum()) > 100
    arena.check()
    return r.delta, [(data, len(text)), (None, 16), (None, (n_bins + 1) * 8)], len(text)


def _fixed(target, stride=None):
    """(stride, n, bytes) of a fixed-stride syn256 batch of exactly `target` bytes"""
    stride = stride or next(s for s in (64, 47, 10, 1) if target % s == 0)
    n = target // stride
    return stride, n, W.fixed_lines(n, stride, 77 + n % 13, alphabet=False)


def _run(form, arena, target, page_off=None, stride=None):
    if form == "match_batch":
        stride, n, src = _fixed(target, stride)
        return _match_batch("syn256", arena, src, stride, n, page_off=page_off)[:3]
    return {"replace_text": _replace_text, "collect_text": _collect_text,
            "tally_text": _tally_text}[form](arena, target, page_off)


# how many transfers each form makes, by route: a small call, and a call of 8 MiB or more whose
# record columns, text output and per-line outputs all own 16 whole pages (the module's docstring
# names the transfers)
SMALL = {"match_batch": (0, 4, 0, 0), "replace_text": (0, 4, 0, 0), "collect_text": (0, 7, 0, 0),
         "tally_text": (0, 3, 0, 0)}
LARGE = {"match_batch": (0, 0, 4, 0), "replace_text": (0, 2, 2, 0), "collect_text": (0, 1, 6, 0),
         "tally_text": (0, 2, 1, 0)}


# a. small calls: the arena alone -----------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_small_calls_go_through_the_arena(form):
    arena = Arena(8 * MIB)
    delta, moved, total = _run(form, arena, 300 * 1024 + (0 if form == "match_batch" else 7), page_off=1)
    assert delta == SMALL[form] == _delta(moved, total), (delta, moved)


# b. the 8 MiB call threshold, at page offsets 0, 1 and 4095 ---------------------------------------------

@pytest.mark.parametrize("page_off", [0, 1, 4095])
@pytest.mark.parametrize("size", [DIRECT_FROM - 1, DIRECT_FROM], ids=["below", "at"])
@pytest.mark.parametrize("form", FORMS)
def test_the_call_threshold(form, size, page_off):
    """below: everything through the arena.  At the threshold: the data and every output that owns
    16 whole pages are registered for the call - result, start and end (the record columns; the
    output text) sit back to back and share pages - and the counts and sizes take the arena"""
    arena = Arena(48 * MIB)
    delta, moved, total = _run(form, arena, size, page_off)
    assert total == size
    want = SMALL[form] if size < DIRECT_FROM else LARGE[form]
    assert delta == want == _delta(moved, total), (delta, want, [(n) for _, n in moved])


# c. the 16 MiB transfer threshold inside a small call ----------------------------------------------------

@pytest.mark.parametrize("n,want", [(2_200_000, (0, 2, 2, 0)), (2_000_000, (0, 4, 0, 0))],
                         ids=["outputs-above", "outputs-below"])
def test_the_transfer_threshold_in_a_small_call(n, want):
    """stride 3: 6.6 MiB of input is a small call, but start and end are 8 bytes a line - 17.6 MiB
    each, above kBounceMax, so they are registered; with 2.0 M lines they are 15.3 MiB and go
    through the arena in 4 MiB pieces (an arena that fills mid-call and starts over)"""
    src = (W.random_bytes(3 * n, 5) % 2 + 97).astype(np.uint8)      # "a" / "b": an eighth is "aab"
    arena = Arena(3 * n + 20 * n + 4 * MIB)
    delta, moved, total, _ = _match_batch("aab", arena, src, 3, n, page_off=1)
    assert total < DIRECT_FROM and (n * 8 > BOUNCE_MAX) == (want[2] > 0)
    assert delta == want == _delta(moved, total), delta


# d. every remaining host form once on the registered route ---------------------------------------------

K8 = -(-(DIRECT_FROM + 1) // PT.N)       # block * K8 is just over 8 MiB


def _host_text(arena, text):
    """the text at page offset 1 of the arena"""
    return _place_text(arena, text, 1)


def _periodic(case):
    lay = PT.layout(case[1], case[2])
    assert lay.length(K8) > DIRECT_FROM
    return lay.text(K8), PT.expected(case, K8)


def _d_grep(arena):
    case = ("grep", "standard", "log100", PT.LAST, 1, False)
    text, x = _periodic(case)
    total = x.counts["n_rows"]
    got = one_amd.grep_text(_exe("log100"), _host_text(arena, text), PT.LAST, True, cap=total + 8)
    assert got[:2] == (x.counts["n_lines"], total) and total > 1000
    for g, key in zip(got[2:], ("line", "begin", "finish", "result", "start", "end")):
        assert np.array_equal(g.astype(np.int64), x.rows[key].numpy().astype(np.int64)), key


def _d_collect(arena):
    text, x = _periodic(COLLECT)
    total = x.counts["n_rows"]
    got = one_amd.collect_text(_exe("log100"), _host_text(arena, text), cap=total + 8)
    assert got[:2] == (x.counts["n_lines"], total) and total > 1000
    for g, key in zip(got[2:], ("line", "begin", "result", "start", "end")):
        assert np.array_equal(g.astype(np.int64), x.rows[key].numpy().astype(np.int64)), key


def _d_tally(arena):
    text, x = _periodic(TALLY)
    got = one_amd.tally_text(_exe("log100"), _host_text(arena, text), 101, matches=True)
    assert got[:2] == (x.counts["n_lines"], x.counts["n_items"])
    assert got[2].astype(np.int64).tolist() == x.counts["bins"].tolist()


def _d_replace(arena):
    text, x = _periodic(REPLACE)
    got = one_amd.replace_text(_exe("err"), _host_text(arena, text), REPLACE[3], PT.LAST, True, PT.ALL)
    assert got[:2] == (x.counts["n_lines"], x.counts["n_replaced"]) and got[1] > 1000
    assert got[2] == x.streams["out"].numpy().tobytes()


def _d_filter(arena):
    case = ("filter", "standard", "log100", False, 2, 2)
    text, x = _periodic(case)
    got = one_amd.filter_text(_exe("log100"), _host_text(arena, text), PT.INSTANT, True, before=2,
                              after=2)
    assert got[:3] == tuple(x.counts[k] for k in ("n_lines", "n_selected", "n_emitted"))
    assert got[3] == x.streams["out"].numpy().tobytes() and got[1] > 1000


def _d_extract(arena):
    case = ("extract", "standard", "log100", PT.ALL)
    text, x = _periodic(case)
    got = one_amd.extract_text(_exe("log100"), _host_text(arena, text))
    assert got[:2] == (x.counts["n_lines"], x.counts["n_matches"]) and got[1] > 1000
    assert got[2] == x.streams["out"].numpy().tobytes()


def _d_fields(arena):
    case = ("fields", "planted", "comma", "2-", False, b" | ")
    text, x = _periodic(case)
    got = one_amd.fields_text(_exe("comma"), _host_text(arena, text), "2-", sep=b" | ")
    assert got[:3] == tuple(x.counts[k] for k in ("n_lines", "n_emitted", "n_fields"))
    assert got[3] == x.streams["out"].numpy().tobytes() and got[2] > 1000


def _d_route(arena):
    case = ("route", "standard", "log100", 101, False)
    text, x = _periodic(case)
    offsets = PT.route_offsets(x, 101)
    got = one_amd.route_text(_exe("log100"), _host_text(arena, text), 101, PT.INSTANT, True)
    assert got[:2] == (x.counts["n_lines"], x.counts["n_routed"])
    assert got[2].astype(np.int64).tolist() == x.counts["bin_lines"].tolist()
    assert got[3].astype(np.int64).tolist() == offsets.tolist()
    want = b"".join(x.streams[b].numpy().tobytes() for b in range(102))
    assert got[4] == want and len(want) > DIRECT_FROM // 2


def _d_uniq(arena):
    kind, name, matches, m = PT.UNIQ_CASES[0]
    lay = PT.layout(kind, name)
    items, _ = PT.uniq_items(name, lay.short(), matches, m=m)
    n_items, first, length, count = PT.uniq_expand(items, lay, K8)
    got = one_amd.uniq_text(_exe(name), _host_text(arena, lay.text(K8)), matches=True,
                            max_distinct=1 << 16)
    assert got[:3] == (lay.n_lines(K8), n_items, 0) and len(first) > 100
    for g, w, key in zip(got[3:], (first, length, count), ("first", "length", "count")):
        assert g.astype(np.int64).tolist() == w.tolist(), key


def _d_range(arena):
    """the oracle's rule run directly over the whole text (tests/range_rule.py)"""
    import range_rule as R
    import test_gpu_range_text_past_4gib as RP
    lay, r = RP._layout()
    text = lay.text(K8)
    assert len(text) > DIRECT_FROM
    x = R.expect(RP.NAME, text, r, None, **RP.SETTING)
    got = one_amd.range_text(_exe("log100"), _host_text(arena, text), r, None, rec_cap=x.n_ranges + 2,
                             **RP.SETTING)
    assert got[:3] == (x.n_lines, x.n_ranges, x.n_emitted) and x.n_ranges > 1000
    assert got[3] == x.out
    for g, w, key in zip(got[4:], x.records, ("first_line", "last_line", "begin", "end")):
        assert np.array_equal(g.astype(np.int64), np.asarray(w).astype(np.int64)), key


def _d_sum(arena):
    """linear in the blocks (tests/test_gpu_sum_text_past_4gib.py proves the rule on the CPU)"""
    import test_gpu_sum_text_past_4gib as SP
    lay = PT.layout("dense", "num3")
    assert lay.length(K8) > DIRECT_FROM
    data = _host_text(arena, lay.text(K8))
    for which, last in (("first", False), ("last", True)):
        want = SP._extrapolate("num3", lay, K8, last)
        got = one_amd.sum_text(_exe("num3"), data, SP.N_BINS["num3"], which=which)
        assert got[:3] == tuple(int(v) for v in want[:3]) and got[2] > 1000, which
        assert np.array_equal(got[3], want[3]), which


def _d_match_text(arena):
    case = ("match", "standard", "uri", PT.LAST, 0)
    text, x = _periodic(case)
    n = x.counts["n_lines"]
    lay = PT.layout(case[1], case[2])
    offs, cnt, res, st, en = one_amd.match_text(_exe("uri"), _host_text(arena, text), PT.LAST, False,
                                                cap=n + 3)
    assert cnt == n and len(offs) == n + 1 and int(offs[n]) == PT.lines_end(lay, K8)
    assert np.array_equal(offs[:n].astype(np.int64), x.rows["offsets"].numpy().astype(np.int64))
    for g, key in ((res, "result"), (st, "start"), (en, "end")):
        assert np.array_equal(g.astype(np.int64), x.rows[key].numpy().astype(np.int64)), key
    assert int((res > 0).sum()) > 1000


def _d_split_lines(arena):
    case = ("lines", "standard", "log100")
    text, x = _periodic(case)
    n = x.counts["n_lines"]
    offs, cnt = one_amd.split_lines(_exe("log100"), _host_text(arena, text), cap=n)
    assert cnt == n and int(offs[n]) == PT.lines_end(PT.layout("standard", "log100"), K8)
    assert np.array_equal(offs[:n].astype(np.int64), x.rows["offsets"].numpy().astype(np.int64))


def _same_records(got, recs):
    total = recs.counts["n_rows"]
    assert got[0] == total and total > 1000
    for g, key in zip(got[1:], ("result", "start", "end")):
        assert np.array_equal(g.astype(np.int64), recs.rows[key].numpy().astype(np.int64)), key


def _d_collect_long(arena):
    name = PT.LONG_NAME
    lay = PT.layout("standard", name)
    recs = PT.expand(PT.collect_long_answer(name, lay.short()), lay, K8)
    got = one_amd.collect_long(_exe(name), _host_text(arena, lay.text(K8)),
                               cap=recs.counts["n_rows"] + 8)
    _same_records(got, recs)


def _d_match_all_long(arena):
    lay = PT.Layout(PT.newyork_block() + b"\n", PT.NEWYORK_TAIL)
    recs = PT.expand(PT.match_all_long_answer("newyork", lay.short(), 1), lay, K8)
    assert lay.length(K8) > DIRECT_FROM
    got = one_amd.match_all_long(_exe("newyork"), _host_text(arena, lay.text(K8)),
                                 recs.counts["n_rows"] + 8, True)
    _same_records(got, recs)


def _d_replace_long(arena):
    name = PT.LONG_NAME
    lay = PT.layout("standard", name)
    repl, mx = PT.LONG_REPLS[1]
    ans = PT.replace_long_answer(name, lay.short(), repl, mx, lay.byte_cuts())
    out = PT.expand(ans, lay, K8).streams["out"].numpy().tobytes()
    got = one_amd.replace_long(_exe(name), _host_text(arena, lay.text(K8)), repl, PT.LAST, True, mx)
    assert got[0] == PT.replaced_count(ans, K8) > 1000
    assert got[1] == out and len(out) > lay.length(K8)


def _d_search_long(arena):
    name = PT.SEARCH_NAME
    text = PT.blank_block(name) * K8 + PT.SEARCH_TAIL
    filler = len(text) - len(PT.SEARCH_TAIL)
    assert filler > DIRECT_FROM
    data = _host_text(arena, text)
    for style, lead in PT.SEARCH_SETTINGS:
        alone = [int(v) for v in _cpu(name).search(PT.SEARCH_TAIL, style, bool(lead))]
        want = (alone[0], alone[1] + filler, alone[2] + filler)
        assert want[0] > 0
        assert one_amd.search_long(_exe(name), data, style, bool(lead)) == want, (style, lead)


_D = {"grep_text": _d_grep, "collect_text": _d_collect, "tally_text": _d_tally,
      "replace_text": _d_replace, "filter_text": _d_filter, "extract_text": _d_extract,
      "fields_text": _d_fields, "route_text": _d_route, "uniq_text": _d_uniq,
      "range_text": _d_range, "sum_text": _d_sum, "match_text": _d_match_text,
      "split_lines": _d_split_lines, "collect_long": _d_collect_long,
      "match_all_long": _d_match_all_long, "replace_long": _d_replace_long,
      "search_long": _d_search_long}


@pytest.mark.parametrize("verb", sorted(_D))
def test_text_verbs_on_the_registered_route(verb):
    """a text just over 8 MiB at page offset 1 through the Python form of every raw-text and
    long-text verb (its outputs are the wrapper's own numpy arrays): the text is registered, nothing
    goes pageable, and every output equals the oracle's"""
    arena = Arena(12 * MIB)
    with Routes() as r:
        _D[verb](arena)
    arena.check()
    assert r.delta[0] == 0 and r.delta[2] >= 1, r.delta


def _batch_forms(arena, name, src, stride, n):
    """check / scan / search / collect / match_all / replace over one placed fixed-stride batch"""
    exe, cpu = _exe(name), _cpu(name)
    data = arena.carve(src.size, np.uint8, 1)
    data[:] = src
    for verb, fn, style in (("check", one_amd.check_batch, 5), ("scan", one_amd.scan_batch, 4)):
        assert np.array_equal(fn(exe, data, style, 0, stride=stride, n=n),
                              cpu.batch(verb, style, 0, data, stride=stride, n=n, threads=8)[0]), verb
    got = one_amd.search_batch(exe, data, 4, 0, stride=stride, n=n)
    for g, e in zip(got, cpu.batch("search", 4, 0, data, stride=stride, n=n, threads=8)):
        assert np.array_equal(g, e), "search"
    counts, res, st, en = one_amd.collect_batch(exe, data, 4, stride=stride, n=n)
    wc, wr, ws, we = cpu.collect_batch(data, 4, stride=stride, n=n)
    kept = np.arange(4)[None, :] < np.minimum(wc, 4)[:, None]
    assert np.array_equal(counts, wc) and int(wc.sum()) > 100
    for g, e in ((res, wr), (st, ws), (en, we)):
        assert np.array_equal(np.asarray(g)[kept], e[kept]), "collect_batch"
    # match_all_batch (collect_batch's staging, its own kernel) and replace_batch, line by line
    lines = [data[i * stride:(i + 1) * stride].tobytes() for i in range(n)]
    counts, res, st, en = one_amd.match_all_batch(exe, data, 4, True, stride=stride, n=n)
    found = 0
    for i, line in enumerate(lines):
        recs, cnt = cpu.match_all(line, True, 4)
        assert int(counts[i]) == cnt, ("match_all_batch", i)
        assert [(int(res[i, j]), int(st[i, j]), int(en[i, j])) for j in range(len(recs))] == recs, i
        found += cnt
    assert found > 1000
    counts, offs, out = one_amd.replace_batch(exe, data, b"<u>", 4, True, stride=stride, n=n)
    assert int(offs[n]) == len(out) and int(counts.sum()) > 1000
    for i in range(0, n, 4):
        k, new = cpu.replace(lines[i], b"<u>", 4, True)
        assert int(counts[i]) == k and out[int(offs[i]):int(offs[i + 1])].tobytes() == new, i


def test_batch_verbs_on_the_registered_route():
    """the other batch verbs' host forms over 8 MiB and a little at page offset 1"""
    n, stride = 32768 + 40, 256
    src = W.fixed_lines(n, stride, 33, alphabet=True, plant=W.URI_PLANT, plant_every=2, plant_at=40)
    arena = Arena(12 * MIB)
    with Routes() as r:
        _batch_forms(arena, "uri", src, stride, n)
    arena.check()
    assert r.delta[0] == 0 and r.delta[2] >= 5, r.delta


def test_a_buffer_that_goes_up_and_comes_back():
    """advance_batch uploads the states and downloads them into the same buffer: in a call of 8 MiB
    or more its pages are registered ONCE (data, state, state back, result: four transfers, all
    registered), released once, and the call behind it starts with no error left over (registered
    twice, the second release failed and the next call's launch check reported it)"""
    n, stride = 131_072 + 40, 64
    src = W.fixed_lines(n, stride, 34, alphabet=False)
    arena = Arena(12 * MIB)
    data = arena.carve(src.size, np.uint8, 1)
    data[:] = src
    state = arena.carve(n, np.uint32)
    state[:] = one_amd.STATE_INITIAL
    with Routes() as r:
        res = one_amd.advance_batch(_exe("syn256"), data, state, stride=stride, n=n)
    want_state = np.full(n, O.STATE_INITIAL, dtype=np.uint32)
    want = _cpu("syn256").advance_batch(data, want_state, stride=stride, n=n)
    assert np.array_equal(res, want) and int((res > 0).sum()) > 10_000
    arena.check()
    assert r.delta == (0, 0, 4, 0), r.delta
    delta, _, _, _ = _match_batch("syn256", Arena(2 * MIB), src[:1024 * stride], stride, 1024, page_off=1)
    assert delta == (0, 4, 0, 0), delta


# e. caller-pinned memory -----------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["host_register", "torch_pin_memory"])
def test_caller_pinned_memory(how):
    """pinned buffers are copied as they are (route 0) and a batch above 16 MiB with 4,096 lines or
    more is cut into chunks of 8 MiB that alternate between the thread's two streams"""
    size = 100 * MIB
    if how == "host_register":
        holder = None
        arena = Arena(size)
        assert one_amd.host_register(arena.mem) == _lib.OK
    else:
        import torch
        holder = torch.empty(size + 2 * PAGE, dtype=torch.uint8).pin_memory()
        arena = Arena(size, holder.numpy())
    try:
        # fixed stride, 20.1 MiB: chunks of 131,072 lines - three of them, four transfers each
        n, stride = 330_000, 64
        src = W.fixed_lines(n, stride, 91, alphabet=False)
        delta, _, total, _ = _match_batch("syn256", arena, src, stride, n, page_off=1)
        assert total > 2 * DIRECT_FROM and 2 * 131072 < n <= 3 * 131072
        assert delta == (12, 0, 0, 0), delta
        # ragged, 22.9 MiB: every chunk but the last holds 8 MiB of line starts and less than a
        # line more - three chunks; the offsets go up once
        src, offs = W.ragged_lines(160_000, 1, 300, 92, alphabet=False)
        assert 2 * DIRECT_FROM + 400 * 300 < int(offs[-1]) < 3 * DIRECT_FROM - 600
        delta, _, _, keep = _match_batch("syn256", arena, src, 0, len(offs) - 1, offsets=offs,
                                         page_off=4095)
        assert delta == (13, 0, 0, 0), delta
        # a sub-batch whose offsets[0] != 0 (still above 16 MiB): the device rebase on both streams
        sub = keep[1][400:]
        assert int(sub[0]) > 0 and int(sub[-1]) - int(sub[0]) > 2 * DIRECT_FROM
        delta, _, _, _ = _match_batch("syn256", arena, None, 0, len(sub) - 1, keep=(keep[0], sub))
        assert delta == (13, 0, 0, 0), delta
        # 10 MiB and a little, pinned: one chunk
        n, stride = 163_840 + 8, 64
        src = W.fixed_lines(n, stride, 93, alphabet=False)
        delta, _, _, keep = _match_batch("syn256", arena, src, stride, n, page_off=0)
        assert delta == (4, 0, 0, 0), delta
        # pinned data, pageable outputs: not a pinned call, so one chunk; the data as it is, the
        # outputs registered for the call
        outs = Arena(8 * MIB)
        delta, moved, total, _ = _match_batch("syn256", arena, None, stride, n, keep=keep, outs=outs)
        assert delta == (1, 0, 3, 0), delta
        assert _delta(moved[1:], total) == (0, 0, 3, 0)
    finally:
        if how == "host_register":
            assert one_amd.host_unregister(arena.mem) == _lib.OK
    del holder


def test_register_refuses_null_and_empty():
    buf = np.zeros(PAGE, dtype=np.uint8)
    assert one_amd.host_register(None, PAGE) == _lib.EAPI
    assert one_amd.host_register(buf, 0) == _lib.EAPI
    assert one_amd.host_unregister(None) == _lib.EAPI


# f. the size ladder on one thread ------------------------------------------------------------------------

LADDER = [12 * MIB, 100, DIRECT_FROM - 100 * 1024, 1024, 900 * 1024, 1100 * 1024, 600 * 1024,
          DIRECT_FROM, 64 * 1024]


def test_the_size_ladder_on_one_thread():
    """large and small calls behind one another: a short text in a device buffer that a 12 MiB text
    grew (what lies behind `len` there is the earlier text, not zeros), an arena that fills
    mid-call and waits (the 600 KiB step: stride 4, so result, start and end are 600 KiB, 1.2 MiB
    and 1.2 MiB behind 600 KiB of data in an arena of about 1.7 MiB), an arena replaced by a larger
    one (1.1 MiB behind 900 KiB), and the same small call again after redgpu_thread_release()"""
    one_amd.thread_release()
    for size in LADDER:
        arena = Arena(6 * size + 4 * MIB)
        # (the 600 KiB step with stride 4: three outputs of 600 KiB and more in one call)
        delta, moved, total = _run("match_batch", arena, size, page_off=1,
                                   stride=4 if size == 600 * 1024 else None)
        assert total == size and delta == _delta(moved, total), (size, delta)
    for size in LADDER:
        arena = Arena(4 * size + 4 * MIB)
        delta, moved, total = _run("replace_text", arena, size, page_off=1)
        assert delta == _delta(moved, total), (size, delta)
    one_amd.thread_release()
    assert one_amd.host_pins_held() == 0
    for form in ("match_batch", "replace_text"):
        delta, moved, total = _run(form, Arena(MIB), 64 * 1024, page_off=1)
        assert delta == SMALL[form], (form, delta)


# g. dfa_tune with a sample of 8 MiB or more ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["syn256", "uri_v6"])
def test_tune_with_a_large_sample_leaves_nothing_behind(name):
    """redgpu_dfa_tune ends like every other host form: the stream drained and the sample's
    registration released when it returns - for a table fused in LDS (syn256: the _dev form returns
    before any synchronisation) as for hot rows (uri_v6)"""
    if name == "syn256":
        n, stride = 131_072 + 28, 64
        sample = W.fixed_lines(n, stride, 51, alphabet=False)
        held = W.fixed_lines(n, stride, 52, alphabet=False)
    else:
        n, stride = 32_768 + 32, 256
        sample = W.fixed_lines(n, stride, 31, alphabet=True, plant=W.URI_PLANT, plant_every=2, plant_at=40)
        held = W.fixed_lines(n, stride, 32, alphabet=True, plant=W.URI_PLANT, plant_every=2, plant_at=17)
    assert sample.nbytes >= DIRECT_FROM
    exe = one_amd.Executable(load_dfa(name))
    _exes[("tuned", name)], _cpus[("tuned", name)] = exe, O.CpuOracle(load_dfa(name))
    try:
        assert exe.info["table_kind"] == (1 if name == "syn256" else 6)
        before = one_amd.host_route_counts()
        exe.tune(sample, stride=stride, n=n)
        held_now = one_amd.host_pins_held()
        after = one_amd.host_route_counts()
        assert held_now == 0, "redgpu_dfa_tune returned with %d registrations / downloads held" % held_now
        assert tuple(a - b for a, b in zip(after, before)) == (0, 0, 1, 0)
        # a small call on a fresh buffer, then the tuned handle on 8 MiB of held-out lines
        delta, _, _, _ = _match_batch(("tuned", name), Arena(2 * MIB), held[:4096 * stride], stride,
                                      4096, page_off=1)
        assert delta == (0, 4, 0, 0), delta
        delta, _, _, _ = _match_batch(("tuned", name), Arena(16 * MIB), held, stride, n, page_off=4095)
        assert delta == (0, 0, 4, 0), delta
    finally:
        # the sample outlives whatever the call left registered
        one_amd.thread_release()
        del _exes[("tuned", name)], _cpus[("tuned", name)]
    del sample
