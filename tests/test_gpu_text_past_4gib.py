"""Every raw-text verb on a text of more than 2^32 bytes: block * K + tail of about 4.07 GiB,
assembled on the device, every output bit-exact against periodic_text's expansion of the oracle's
answer for block * 3 + tail (tests/test_periodic_expectation.py proves the expansion), compared on
the device in slices.  K = ceil((2^32 + 64 MiB) / P) with P = 65,541, so several 16 MiB scan tiles
lie above the boundary, chunk borders and 16-byte store blocks meet every phase of the block, and a
few whole lines in front of block 0 put one match of the block across byte 2^32 itself.  What each
case asserts depends on positions, line indices or scanned sums above 2^32: the records' begin /
start / end, the lines' offsets, out_len and the bytes behind 2^32 of the outputs, route_text's
bin_offsets, uniq_text's first.  Then a text of 2^32 + 2^20 + 3 one-byte lines in front of a block
(line indices above 2^32), and the four long-text verbs over ONE text of that length each.

Device forms and the default table placement only.  Needs 16 GiB of free device memory.

Wall time per test on an MI355X, the module run alone (44 tests, 15.7 s in all; each text of 4.07 GiB
is assembled in 1.4 s the first time, in milliseconds from then on):
  lines / match_text / match_batch / search_batch / collect_batch: log100 1.31 s, uri 0.08 s
  grep_text 0.13-0.18 s a case; filter_text 0.15-0.25 s; extract_text 0.25-0.43 s
  route_text 0.10-0.22 s; uniq_text 0.05 s (lines), 0.12 s (max_per_line 1), 2.26 s (675 million
  items of 490 strings without the LDS front - the one case that shows what 4 GiB cost there)
  collect_text 0.11-0.41 s; tally_text 0.04-0.22 s; replace_text 0.06-0.29 s
  fields_text 0.05-0.35 s (the last case with uniq_text over its 4.5 GiB output)
  line indices above 2^32: 0.18 s; collect_long and replace_long 3.0 s (four rewrites of the text)
  search_long 0.57 s (twelve walks); match_all_long 0.02 s a leader setting
Peak device memory, all of it (texts, outputs, scratch, slices): 11.0 GiB."""
import numpy as np
import pytest

import one_amd
from one_amd import _lib

import periodic_text as PT

pytestmark = pytest.mark.gpu

B32 = 1 << 32
K = -(-(B32 + (64 << 20)) // PT.N)
SENT = 0x55
NEED = 16 << 30

# the route each batch over the lines takes: the ragged kernels (uri: no leader), the leader's
# early-death walk and the marked scan (log100)
KERNELS = {
    ("match", "standard", "uri", PT.LAST, 0): "k_ragged<last,start,end>",
    ("match", "standard", "uri", PT.FULL, 0): "k_ragged<full,start>",
    ("match", "standard", "log100", PT.LAST, 1): "k_early<match>",
    ("search_lines", "standard", "uri", PT.INSTANT, 0): "k_style_blocks<match>",
    ("search_lines", "standard", "log100", PT.INSTANT, 1): "k_scan_marked",
}

_exes = {}


def _exe(name):
    import test_gpu_fields_text as FL
    if name not in _exes:
        _exes[name] = one_amd.Executable(FL._blob(name))
    return _exes[name]


@pytest.fixture(scope="module")
def texts():
    """get(kind, name) -> (layout, device text): one long text alive at a time, built when the
    block changes, freed with the calling thread's scratch at the module's end"""
    import torch
    torch.cuda.empty_cache()        # (what earlier modules left in torch's cache counts as free)
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("a text past 4 GiB needs 16 GiB of free device memory; %d MiB are free" % (free >> 20))
    held = {}

    def get(kind, name):
        if held.get("key") != (kind, name):
            held.clear()
            torch.cuda.empty_cache()
            lay0 = PT.layout(kind, name)
            spans = PT.block_spans(name, lay0.block)
            lay = lay0.with_lead(PT.lead_for(lay0, B32, spans))
            assert K * lay.P > B32 + (1 << 26) and lay.P % 16
            assert PT.straddles(lay, B32, spans), (kind, name)
            dev = lay.device_text(K)
            assert dev.numel() == lay.length(K) > B32 + (1 << 26)
            held.update(key=(kind, name), lay=lay, dev=dev)
        return held["lay"], held["dev"]

    def drop():
        held.clear()
        torch.cuda.empty_cache()

    get.drop = drop
    yield get
    held.clear()
    _lib.lib().redgpu_thread_release()
    torch.cuda.empty_cache()


def _ints(*tensors):
    import torch
    torch.cuda.synchronize()
    return [int(t.item()) for t in tensors]


def _both_sides(exp, where):
    """an ascending column of offsets has at least 1,000 entries on each side of 2^32"""
    at = PT.first_at_least(exp, B32)
    assert at >= 1000 and len(exp) - at >= 1000, (where, at, len(exp))
    return at


def _room(exp_len, out_cap):
    """an output buffer of out_cap bytes with 64 sentinel bytes behind min(out_len, out_cap)"""
    import torch
    buf = torch.empty(out_cap + 64, dtype=torch.uint8, device="cuda")
    w = min(exp_len, out_cap)
    buf[w:w + 64] = SENT
    return buf, w


def _out_same(buf, w, stream, where):
    stream.same_dev(buf, upto=w, where=where)
    assert bool((buf[w:w + 64] == SENT).all()), (where, "bytes behind the output were written")


# split_lines, match_text and the ragged batches over the same offsets -----------------------------

@pytest.mark.parametrize("name", ["log100", "uri"])
def test_lines_match_text_and_ragged_batches(texts, name):
    import torch
    lay, dev = texts("standard", name)
    exe = _exe(name)
    n = lay.n_lines(K)
    first = True
    for case in PT.cases_of("match") + PT.cases_of("search_lines"):
        if case[2] != name:
            continue
        verb, _, _, style, lead = case
        x = PT.expected(case, K, lay.lead)
        assert x.counts["n_lines"] == n
        if verb == "match":
            at = _both_sides(x.rows["offsets"], case)
            offs, cnt, res, st, en = one_amd.match_text(exe, dev, style, bool(lead), cap=n + 3)
            kernel = one_amd.last_kernel()
            assert kernel == KERNELS[case], (case, kernel)
            assert _ints(cnt) == [n]
            x.rows["offsets"].same_dev(offs, upto=n, where=(case, "offsets"))
            assert _ints(offs[n], offs[at]) == [PT.lines_end(lay, K), x.rows["offsets"].at(at)]
            assert PT.lines_end(lay, K) > B32 + (1 << 26)
            for got, key in ((res, "result"), (st, "start"), (en, "end")):
                x.rows[key].same_dev(got, upto=n, where=(case, key, kernel))
            if first:
                # split_lines alone, and its count without room for a line
                first = False
                o2, c2 = one_amd.split_lines(exe, dev, cap=n)
                assert one_amd.last_kernel() == "k_split_scatter"
                assert _ints(c2) == [n] and torch.equal(o2, offs[:n + 1])
                assert _ints(one_amd.split_lines(exe, dev, cap=0)[1]) == [n]
                del o2
            # the ragged kernels with offsets[] above 2^32
            r, s, e = one_amd.match_batch(exe, dev, style, bool(lead), offsets=offs[:n + 1], stride=1)
            kernel = one_amd.last_kernel()
            assert kernel == KERNELS[case], (case, kernel)
            for got, key in ((r, "result"), (s, "start"), (e, "end")):
                x.rows[key].same_dev(got, where=(case, "match_batch", key, kernel))
            del r, s, e, res, st, en
            held_offs = offs[:n + 1]
        else:
            r, s, e = one_amd.search_batch(exe, dev, style, bool(lead), offsets=held_offs, stride=1)
            kernel = one_amd.last_kernel()
            assert kernel == KERNELS[case], (case, kernel)
            for got, key in ((r, "result"), (s, "start"), (e, "end")):
                x.rows[key].same_dev(got, where=(case, "search_batch", key, kernel))
            assert _ints((r > 0).sum())[0] > 2000
            del r, s, e
    if name == "log100":
        # collect_batch(cap=4) over the same offsets: no line of this block has more records
        recs = PT.expected(("collect", "standard", name), K, lay.lead)
        per = PT.expected(("collect_counts", "standard", name), K, lay.lead).rows["counts"]
        assert max(int(p.max()) for p in per.parts) <= 4 and recs.counts["n_rows"] > n // 4
        counts, r, s, e = one_amd.collect_batch(exe, dev, 4, offsets=held_offs, stride=1)
        kernel = one_amd.last_kernel()
        assert kernel == "k_collect", kernel
        per.same_dev(counts, where=("collect_batch", "counts", kernel))
        kept = torch.arange(4, device="cuda")[None, :] < counts[:, None]
        for got, key in ((r, "result"), (s, "start_in_line"), (e, "end_in_line")):
            recs.rows[key].same_dev(got[kept], where=("collect_batch", key, kernel))


# grep_text ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("grep"), ids=PT.case_id)
def test_grep_text(texts, case):
    _, kind, name, style, lead, invert = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    n, total = x.counts["n_lines"], x.counts["n_rows"]
    at = _both_sides(x.rows["finish"], case)
    if not invert:
        # the record of the line that holds byte 2^32: its match lies across the boundary
        begin = x.rows["begin"].at(at)
        assert begin < B32 <= x.rows["finish"].at(at)
        if style == PT.LAST:
            assert begin + x.rows["start"].at(at) < B32 < begin + x.rows["end"].at(at)
    got = one_amd.grep_text(exe, dev, style, bool(lead), invert=invert, cap=total + 8)
    assert one_amd.last_kernel() == "k_grep_text"
    assert _ints(got[0], got[1]) == [n, total], case
    for g, key in zip(got[2:], ("line", "begin", "finish", "result", "start", "end")):
        x.rows[key].same_dev(g, where=(case, key))
    assert _ints(got[3][total - 1])[0] > B32 + (1 << 26)
    del got
    # grep -m: the last kept record lies above 2^32
    mx = at + 1500
    got = one_amd.grep_text(exe, dev, style, bool(lead), invert=invert, cap=mx + 8, max_count=mx)
    assert _ints(got[0], got[1]) == [n, mx], case
    for g, key in zip(got[2:], ("line", "begin", "finish", "result", "start", "end")):
        x.rows[key].same_dev(g, upto=mx, where=(case, "max_count", key))
    assert _ints(got[3][mx - 1])[0] > B32
    del got
    # grep -c
    got = one_amd.grep_text(exe, dev, style, bool(lead), invert=invert, cap=0)
    assert _ints(got[0], got[1]) == [n, total], case


# filter_text ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("filter"), ids=PT.case_id)
def test_filter_text(texts, case):
    _, kind, name, invert, before, after = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    out = x.streams["out"]
    kw = dict(invert=invert, before=before, after=after)
    counts = [x.counts[k] for k in ("n_lines", "n_selected", "n_emitted")] + [len(out)]
    if (before, after) == (9, 9):
        # wider than a block's longest gap between selected lines: every line is emitted
        assert counts[2] == counts[0] and len(out) == PT.lines_end(lay, K)
    caps = [len(out) + 1000]
    if (before, after) == (2, 2):
        caps += [len(out), B32 + 5]
    for cap in caps:
        if len(out) <= B32 + 5 and cap == B32 + 5:
            continue
        buf, w = _room(len(out), cap)
        got = one_amd.filter_text(exe, dev, PT.INSTANT, True, out=buf, out_cap=cap, **kw)
        assert one_amd.last_kernel() == "k_filter_text"
        assert _ints(*got[:4]) == counts, (case, cap)
        _out_same(buf, w, out, (case, cap))
        del buf, got
    # grep -m: the mx-th selected line lies above 2^32
    at = PT.first_at_least(x.rows["sel"], lay.line_at(K, B32)[0])
    mx = at + 1500
    assert at >= 1000 and mx + 1000 < counts[1], (case, at, counts)
    emitted, out_len = PT.filter_first(x, mx)
    buf, w = _room(out_len, out_len + 1000)
    got = one_amd.filter_text(exe, dev, PT.INSTANT, True, out=buf, max_count=mx, **kw)
    assert _ints(*got[:4]) == [counts[0], mx, emitted, out_len], (case, "max_count")
    _out_same(buf, w, out, (case, "max_count"))
    # the sizes alone
    got = one_amd.filter_text(exe, dev, PT.INSTANT, True, out_cap=0, **kw)
    assert _ints(*got[:4]) == counts, (case, "sizes")


# extract_text --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("extract"), ids=PT.case_id)
def test_extract_text(texts, case):
    _, kind, name, m = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    out = x.streams["out"]
    counts = [x.counts["n_lines"], x.counts["n_matches"], len(out)]
    got = one_amd.extract_text(exe, dev, max_per_line=m, out_cap=0)
    assert one_amd.last_kernel() == "k_extract_text"
    assert _ints(*got[:3]) == counts, (case, "sizes")
    if kind == "dense":
        return              # (the dense block: the sizes only - 600 million pieces)
    for cap in (len(out) + 1000, len(out), len(out) // 2 + 5):
        buf, w = _room(len(out), cap)
        got = one_amd.extract_text(exe, dev, max_per_line=m, out=buf, out_cap=cap)
        assert _ints(*got[:3]) == counts, (case, cap)
        _out_same(buf, w, out, (case, cap))
        del buf, got


# route_text ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("route"), ids=PT.case_id)
def test_route_text(texts, case):
    import torch
    _, kind, name, n_bins, drop = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    offsets = PT.route_offsets(x, n_bins)
    out_len = int(offsets[-1])
    if not drop:
        assert out_len == PT.lines_end(lay, K), case
        assert int((offsets > B32).sum()) >= (90 if n_bins == 101 else 1), offsets
    buf, w = _room(out_len, out_len + 1000)
    got = one_amd.route_text(exe, dev, n_bins, PT.INSTANT, True, drop_unmatched=drop, out=buf)
    assert one_amd.last_kernel() == "k_route_text"
    assert _ints(got[0], got[1], got[4]) == [x.counts["n_lines"], x.counts["n_routed"], out_len], case
    assert got[2].cpu().tolist() == x.counts["bin_lines"].tolist(), case
    assert got[3].cpu().tolist() == offsets.tolist(), case
    for b in range(n_bins + 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        x.streams[b].same_dev(buf[lo:hi], where=(case, "section", b))
    assert bool((buf[w:w + 64] == SENT).all()), case
    # bin_lines is tally_text's histogram of the lines, bit for bit
    tally = one_amd.tally_text(exe, dev, n_bins, matches=False, style=PT.INSTANT, do_leader=True)
    torch.cuda.synchronize()
    assert torch.equal(tally[2], got[2]) and _ints(tally[0])[0] == x.counts["n_lines"]
    del buf, got
    # truncated above the boundary, inside a line
    if not drop:
        buf, w = _room(out_len, B32 + 5)
        got = one_amd.route_text(exe, dev, n_bins, PT.INSTANT, True, out=buf, out_cap=B32 + 5)
        assert _ints(got[4]) == [out_len] and got[3].cpu().tolist() == offsets.tolist()
        for b in range(n_bins + 1):
            lo, hi = min(int(offsets[b]), w), min(int(offsets[b + 1]), w)
            x.streams[b].same_dev(buf[lo:hi], upto=hi - lo, where=(case, "cut section", b))
        assert bool((buf[w:w + 64] == SENT).all()), case


# uniq_text: lines ----------------------------------------------------------------------------------

def _uniq_same(got, n_lines, want, where):
    n_items, first, length, count = want
    assert _ints(*got[:4]) == [n_lines, n_items, 0, len(first)], where
    for g, w, key in zip(got[4:], (first, length, count), ("first", "length", "count")):
        assert g[:len(w)].cpu().tolist() == w.tolist(), (where, key)


@pytest.mark.parametrize("case", PT.UNIQ_CASES, ids=PT.case_id)
def test_uniq_text(texts, case):
    kind, name, matches, m = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    items, n_lines = PT.uniq_items(name, lay.short(), matches, m=m)
    want = PT.uniq_expand(items, lay, K)
    # the tail's strings are first seen above 2^32; the block's are counted once per block
    own = want[1] > B32
    assert own.sum() >= 3 and (want[3][~own] >= K).all() and (~own).sum() >= 10, case
    got = one_amd.uniq_text(exe, dev, matches=matches, style=PT.INSTANT, do_leader=True,
                            max_per_line=m, max_distinct=1 << 20, cap=len(want[1]) + 3)
    assert one_amd.last_kernel() == "k_uniq_text"
    _uniq_same(got, lay.n_lines(K), want, case)


# collect_text, tally_text --------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("collect"), ids=PT.case_id)
def test_collect_text(texts, case):
    _, kind, name = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    n, total = x.counts["n_lines"], x.counts["n_rows"]
    at = _both_sides(x.rows["end"], case)
    assert x.rows["start"].at(at) < B32 < x.rows["end"].at(at) or name == "uri"
    got = one_amd.collect_text(exe, dev, cap=total + 8)
    assert one_amd.last_kernel() == "k_collect_text"
    assert _ints(got[0], got[1]) == [n, total], case
    for g, key in zip(got[2:], ("line", "begin", "result", "start", "end")):
        x.rows[key].same_dev(g, where=(case, key))
    assert _ints(got[6][total - 1])[0] > B32 + (1 << 26)
    del got
    # a cap that cuts the list between two records of one line, above 2^32
    cap = at + 1000
    if kind == "dense" and name != "uri":      # (the others: one record per line)
        while x.rows["line"].at(cap - 1) != x.rows["line"].at(cap):
            cap += 1
    got = one_amd.collect_text(exe, dev, cap=cap)
    assert _ints(got[0], got[1]) == [n, total], (case, cap)
    for g, key in zip(got[2:], ("line", "begin", "result", "start", "end")):
        x.rows[key].same_dev(g, upto=cap, where=(case, "cap", key))
    del got
    got = one_amd.collect_text(exe, dev, cap=0)
    assert _ints(got[0], got[1]) == [n, total], (case, "counts")


@pytest.mark.parametrize("case", PT.cases_of("tally"), ids=PT.case_id)
def test_tally_text(texts, case):
    """4 GiB and more are counted in global memory alone (no LDS bins)"""
    import torch
    _, kind, name, n_bins, matches = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    bins = x.counts["bins"]
    assert int(bins.sum()) == (x.counts["n_items"] if matches else x.counts["n_lines"])
    assert int(bins.max()) > 1000000 and (bins > 0).sum() >= (1 if n_bins == 8 else 4), bins
    got = one_amd.tally_text(exe, dev, n_bins, matches=matches, style=PT.INSTANT, do_leader=True)
    assert one_amd.last_kernel() == "k_tally_text"
    assert _ints(got[0], got[1]) == [x.counts["n_lines"], x.counts["n_items"]], case
    assert got[2].cpu().tolist() == bins.tolist(), case
    # accumulate: a second call into the same bins doubles them
    again = one_amd.tally_text(exe, dev, n_bins, matches=matches, style=PT.INSTANT, do_leader=True,
                               into=got[2])
    torch.cuda.synchronize()
    assert again[2].cpu().tolist() == (2 * bins).tolist(), case


# replace_text --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("replace"), ids=PT.case_id)
def test_replace_text(texts, case):
    _, kind, name, repl, mx, oc = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    out = x.streams["out"]
    counts = [x.counts["n_lines"], x.counts["n_replaced"], len(out)]
    length = lay.length(K)
    if not oc:
        # out_len below, at and above the text's length
        side = (len(repl) > 5) - (len(repl) < 5)
        assert (len(out) > length) - (len(out) < length) == side, (case, len(out), length)
        assert out.parts[3].tobytes().endswith(lay.tail[-10:])      # the tail is copied
    caps = [len(out) + 1000]
    if len(repl) == 8 and not oc:
        caps += [len(out), B32 + 5]
    for cap in caps:
        buf, w = _room(len(out), cap)
        got = one_amd.replace_text(exe, dev, repl, PT.LAST, True, mx, only_changed=bool(oc),
                                   out=buf, out_cap=cap)
        assert one_amd.last_kernel() == "k_replace_text"
        assert _ints(*got[:3]) == counts, (case, cap)
        _out_same(buf, w, out, (case, cap))
        del buf, got


# fields_text, and its output into uniq_text ----------------------------------------------------------

@pytest.mark.parametrize("case", PT.cases_of("fields"), ids=PT.case_id)
def test_fields_text(texts, case):
    _, kind, name, fields, only, sep = case
    lay, dev = texts(kind, name)
    exe = _exe(name)
    x = PT.expected(case, K, lay.lead)
    out = x.streams["out"]
    counts = [x.counts[k] for k in ("n_lines", "n_emitted", "n_fields")] + [len(out)]
    buf, w = _room(len(out), len(out) + 1000)
    got = one_amd.fields_text(exe, dev, fields, sep=sep, only_delimited=only, out=buf)
    assert one_amd.last_kernel() == "k_fields_text"
    assert _ints(*got[:4]) == counts, case
    _out_same(buf, w, out, case)
    if sep != b" | ":
        return
    # awk -F, '{ $1 = ""; print }' | sort | uniq -c on the device: the output is a text of more than
    # 2^32 bytes, its lines keyed by their bytes, the tail's first seen above 2^32
    assert len(out) > B32 + (1 << 24)
    olay, oK = PT.stream_layout(out)
    items, _ = PT.uniq_items("num3", olay.short(), False)
    want = PT.uniq_expand(items, olay, oK)
    assert (want[1] > B32).sum() >= 3 and len(want[1]) > 100
    column = buf[:len(out)]
    got = one_amd.uniq_text(_exe("num3"), column, matches=False, style=PT.INSTANT, do_leader=True,
                            max_distinct=1 << 20, cap=len(want[1]) + 3)
    assert one_amd.last_kernel() == "k_uniq_text"
    _uniq_same(got, counts[1], want, (case, "uniq"))


# line indices above 2^32 ---------------------------------------------------------------------------

def test_line_indices_past_4gi_lines(texts):
    """2^32 + 2^20 + 3 one-byte lines in front of a block and its tail: every chunk of 16,384 lines
    is textLines' 256-round extreme, and the block's records carry line indices above 2^32"""
    import torch
    texts.drop()
    D = B32 + (1 << 20) + 3
    name = "log100"
    lay = PT.layout("standard", name)
    short = lay.block + lay.tail
    exe = _exe(name)
    dev = torch.cat([torch.full((D,), PT.DELIM, dtype=torch.uint8, device="cuda"),
                     torch.from_numpy(PT._u8(short).copy()).cuda()])
    n = D + lay.L + lay.tail_lines

    def same(got, ans, names, total):
        for t, key in zip(got, names):
            arr, kind = ans.rows[key]
            want = arr.astype(np.int64) + (D if kind else 0)
            assert t[:total].cpu().tolist() == want.tolist(), key
            if kind:
                assert int(want.min()) > B32

    assert _ints(one_amd.split_lines(exe, dev, cap=0)[1]) == [n]
    # tally_text by lines: the empty lines are 2^32 and more items of value 0
    t = PT.tally_answer(name, short, 101, False)
    bins = t.sums["bins"][2](t.sums["bins"][0])
    bins[0] += D
    got = one_amd.tally_text(exe, dev, 101, matches=False, style=PT.INSTANT, do_leader=True)
    assert one_amd.last_kernel() == "k_tally_text"
    assert _ints(got[0], got[1]) == [n, int(t.sums["n_items"][2](t.sums["n_items"][0]))]
    assert got[2].cpu().tolist() == bins.tolist() and int(bins[0]) > B32
    # grep_text and collect_text: the block's records, moved
    g = PT.grep_answer(name, short, PT.INSTANT, 1)
    total = len(g.row_line)
    got = one_amd.grep_text(exe, dev, PT.INSTANT, True, cap=total + 8)
    assert _ints(got[0], got[1]) == [n, total] and total > 150
    same(got[2:], g, ("line", "begin", "finish", "result", "start", "end"), total)
    c = PT.collect_answer(name, short)
    total = len(c.row_line)
    got = one_amd.collect_text(exe, dev, cap=total + 8)
    assert _ints(got[0], got[1]) == [n, total] and total > 150
    same(got[2:], c, ("line", "begin", "result", "start", "end"), total)
    # filter_text: grep -A 2 (no context in front: the first selected line follows the empty ones)
    f = PT.filter_answer(name, short, PT.INSTANT, 1, False, 0, 2)
    out = f.streams["out"][0]
    buf, w = _room(len(out), len(out) + 1000)
    got = one_amd.filter_text(exe, dev, PT.INSTANT, True, after=2, out=buf)
    assert _ints(*got[:4]) == [n, len(f.row_line), int(f.emit.sum()), len(out)]
    assert buf[:w].cpu().numpy().tobytes() == out and bool((buf[w:w + 64] == SENT).all())


# the long-text verbs: ONE text of more than 2^32 bytes -------------------------------------------------

def _same_slices(a, b, where):
    import torch
    assert a.numel() == b.numel(), where
    for lo in range(0, a.numel(), PT.SLICE):
        assert torch.equal(a[lo:lo + PT.SLICE], b[lo:lo + PT.SLICE]), (where, lo)


def test_collect_long_and_replace_long(texts):
    """an anchored DFA with a pure dead state and no line end in its language: every attempt is
    dead at a block's begin (test_periodic_expectation proves it), so the long text's records and
    rewritten bytes are the block's, repeated"""
    name = PT.LONG_NAME
    lay, dev = texts("standard", name)
    exe = _exe(name)
    short = lay.short()
    recs = PT.expand(PT.collect_long_answer(name, short), lay, K)
    total = recs.counts["n_rows"]
    at = _both_sides(recs.rows["end"], "collect_long")
    assert recs.rows["start"].at(at) < B32 < recs.rows["end"].at(at)
    cnt, r, s, e = one_amd.collect_long(exe, dev, cap=total + 8)
    assert one_amd.last_kernel() == "k_collect_long"
    assert cnt == total
    for got, key in ((r, "result"), (s, "start"), (e, "end")):
        recs.rows[key].same_dev(got, where=("collect_long", key))
    assert _ints(s[total - 1])[0] > B32 + (1 << 26)
    del r, s, e
    for repl, mx in PT.LONG_REPLS:
        ans = PT.replace_long_answer(name, short, repl, mx, lay.byte_cuts())
        out = PT.expand(ans, lay, K).streams["out"]
        assert (len(out) > lay.length(K)) == (len(repl) > 20) and PT.replaced_count(ans, K) == total
        buf, w = _room(len(out), max(len(out), lay.length(K)) + 1000)
        got = one_amd.replace_long(exe, dev, repl, PT.LAST, True, mx, out=buf[:len(out) + 1000])
        assert one_amd.last_kernel() == "k_replace_long"
        assert (got[0], got[2]) == (total, len(out)), (repl, got[0], got[2])
        _out_same(buf, w, out, ("replace_long", repl))
        # max_count: the last replacement lies above 2^32, the text behind it is copied
        m = at + 1500
        out_len, cut, rest = PT.replace_long_first(recs, repl, m, lay.length(K))
        assert rest > B32 and cut + 64 < len(out) and out_len + 1064 <= buf.numel()
        buf[out_len:out_len + 64] = SENT
        got = one_amd.replace_long(exe, dev, repl, PT.LAST, True, m, out=buf[:out_len + 1000])
        assert (got[0], got[2]) == (m, out_len), (repl, m, got[0], got[2])
        out.same_dev(buf, upto=cut, where=("replace_long", repl, "max_count"))
        _same_slices(buf[cut:out_len], dev[rest:], ("replace_long", repl, "the rest"))
        assert bool((buf[out_len:out_len + 64] == SENT).all())
        del buf, got


def test_search_long(texts):
    """a filler without a match, the first match in the tail: its start is above 2^32"""
    import torch
    texts.drop()
    name = PT.SEARCH_NAME
    exe = _exe(name)
    cpu = PT._long_cpu(name)
    block, tail = PT.blank_block(name), PT.SEARCH_TAIL
    body = torch.from_numpy(PT._u8(block).copy()).cuda().repeat(K)
    dev = torch.cat([body, torch.from_numpy(PT._u8(tail).copy()).cuda()])
    del body
    filler = dev[:K * len(block)]
    assert filler.numel() > B32 + (1 << 26) and filler.is_contiguous()
    for style, lead in PT.SEARCH_SETTINGS:
        alone = [int(v) for v in cpu.search(tail, style, bool(lead))]
        want = [alone[0], alone[1] + filler.numel(), alone[2] + filler.numel()]
        assert want[0] > 0 and want[1] > B32
        got = one_amd.search_long(exe, dev, style, bool(lead))
        assert one_amd.last_kernel() == "k_search_long"
        assert _ints(*got) == want, (style, lead)
        # the whole text walked with nobody lowering `best`
        got = one_amd.search_long(exe, filler, style, bool(lead))
        assert one_amd.last_kernel() == "k_search_long"
        assert _ints(*got) == [0, 0, 0], (style, lead)
    del dev, filler


@pytest.mark.parametrize("lead", [0, 1])
def test_match_all_long(texts, lead):
    """a DFA that never dies: ONE walk over the whole text, in the same state at every block's
    begin (test_periodic_expectation proves it)"""
    import torch
    texts.drop()
    name = "newyork"
    exe = _exe(name)
    lay = PT.Layout(PT.newyork_block() + b"\n", PT.NEWYORK_TAIL)
    assert lay.P % 16 and lay.length(K) > B32 + (1 << 26)
    dev = lay.device_text(K)
    recs = PT.expand(PT.match_all_long_answer(name, lay.short(), lead), lay, K)
    total = recs.counts["n_rows"]
    _both_sides(recs.rows["end"], "match_all_long")
    cnt, r, s, e = one_amd.match_all_long(exe, dev, total + 8, bool(lead))
    assert one_amd.last_kernel() == "k_match_all_long"
    assert cnt == total
    for got, key in ((r, "result"), (s, "start"), (e, "end")):
        recs.rows[key].same_dev(got, where=("match_all_long", lead, key))
    assert _ints(s[total - 1])[0] > B32 + (1 << 26)
