"""The rules of the eight newer raw-text verbs (include/redgpu.h) in plain Python and numpy, over
ANY oracle - a CpuOracle, or anything with its batch, collect, collect_batch and replace - and not
over a golden DFA's name: what scripts/fuzz_gpu.py's `lines` and `pieces` modes check the GPU
against, and what test_text_rules.py proves equal to the per-verb expectations of the
tests/test_gpu_<verb>.py modules.  Two primitives, each computed once per Text: the LINES
(sampleLines' loop, and per (style, leader) search's result on every line alone) and the PIECES (per
line collect's records and the span [a, e) extract_text emits for each, from one replace with a
marker byte the line lacks).  On top of them one pure function per verb, which returns exactly what
the verb's host form returns.  A helper, not a test."""
import re

import numpy as np

import oracle as O
import range_rule

ALL = 1 << 62
M64 = 1 << 64
CHUNK = 16384


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def by_lengths(cpu, line, ends):
    """[a_j] of one line from the lengths of replace(line, "", m): needs no marker byte"""
    out, before = [], len(line)
    for m, e in enumerate(ends, 1):
        k, rest = cpu.replace(line, b"", "last", False, m)
        assert k == m, (k, m)
        size = before - len(rest)
        assert 0 < size <= e, (size, e)
        out.append(e - size)
        before = len(rest)
    return out


def by_marker(cpu, line, ends, mark):
    """[a_j] of one line from ONE replace with a byte the line lacks: what stands between the marks
    is what no piece covers, so piece j begins behind gap j, which begins at e_(j-1)"""
    k, rest = cpu.replace(line, mark, "last", False)
    gaps = rest.split(mark)
    assert k == len(ends) and len(gaps) == k + 1, (k, len(ends), len(gaps))
    out, at = [], 0
    for gap, e in zip(gaps, ends):
        a = at + len(gap)
        assert line[at:a] == gap and a < e, (at, a, e)
        out.append(a)
        at = e
    assert line[at:] == gaps[-1]
    return out


class Text:
    """one text under one delimiter: its lines, and what the oracle says of every line alone"""

    def __init__(self, cpu, text, delim=0x0A):
        self.cpu, self.text, self.delim = cpu, bytes(text), int(delim)
        self.lines = O.split_lines_loop(self.text, self.delim)
        self.n_lines = n = len(self.lines)
        lens = np.array([len(x) for x in self.lines], dtype=np.int64)
        # line k = text[offs[k] : offs[k + 1] - 1], its delimiter behind it; the tail is no line
        self.offs = np.concatenate([[0], np.cumsum(lens + 1)]).astype(np.int64)
        self.tail = self.text[int(self.offs[-1]):]
        # ... and the lines back to back without their delimiters: the oracle's verb on each alone
        self.bare = _u8(b"".join(self.lines) + b"\0")
        self.boffs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self._values, self._pieces, self._memo = {}, None, {}

    def line_bytes(self, i):
        """line i with its delimiter"""
        return self.text[int(self.offs[i]):int(self.offs[i + 1])]

    def join(self, which):
        return b"".join(self.line_bytes(i) for i in which)

    def values(self, style=1, lead=1):
        """search<style,lead>(line).result_ per line, 0 where it does not match"""
        key = (int(style), int(bool(lead)))
        if key not in self._values:
            r = self.cpu.batch("search", key[0], key[1], self.bare, offsets=self.boffs)[0]
            self._values[key] = np.where(r > 0, r, 0).astype(np.int64)
        return self._values[key]

    def _line_pieces(self, line, recs):
        ends = [e for _, _, e in recs]
        absent = np.flatnonzero(np.bincount(_u8(line), minlength=256) == 0)
        absent = absent[absent != self.delim]
        if len(absent):
            begins = by_marker(self.cpu, line, ends, bytes([int(absent[0])]))
        else:                   # the line holds all 255 candidates
            begins = by_lengths(self.cpu, line, ends)
        for a, (_, s, e) in zip(begins, recs):
            assert a <= s and a < e, (a, s, e)
        return tuple((r, s, a, e) for a, (r, s, e) in zip(begins, recs))

    def pieces(self):
        """per line the tuple of (result, start, a, e): collect's records and where the attempt that
        found each began, all relative to the line; memoised by the line's bytes"""
        if self._pieces is None:
            cap = 8
            counts, r, s, e = self.cpu.collect_batch(self.bare, cap, offsets=self.boffs)
            per = [()] * self.n_lines
            for k in np.flatnonzero(counts).tolist():
                line = self.lines[k]
                if line not in self._memo:
                    c = int(counts[k])
                    if c <= cap:
                        recs = list(zip(r[k, :c].tolist(), s[k, :c].tolist(), e[k, :c].tolist()))
                    else:
                        recs, again = self.cpu.collect(line, c)
                        assert again == c
                    self._memo[line] = self._line_pieces(line, recs)
                per[k] = self._memo[line]
            self._pieces = per
        return self._pieces

    def items(self, max_per_line=ALL):
        """(line, result, start, a, e) of every piece extract_text emits under max_per_line"""
        return [(k,) + p for k, got in enumerate(self.pieces()) for p in got[:max_per_line]]

    def piece_bytes(self, item):
        k, _, _, a, e = item
        return self.lines[k][a:e]


def slots(values, n_bins):
    """slot r for (uint32_t)r < n_bins, everything else in slot n_bins"""
    v = np.asarray(values, dtype=np.int64)
    return np.where((v >= 0) & (v < n_bins), v, n_bins)


def tally(t, n_bins, matches=True, style=1, lead=1, into=None):
    """(n_lines, n_items, bins)"""
    v = (np.array([it[1] for it in t.items()], dtype=np.int64) if matches
         else t.values(style, lead))
    bins = np.bincount(slots(v, n_bins), minlength=n_bins + 1).astype(np.uint64)
    return t.n_lines, int((v > 0).sum()), bins if into is None else into + bins


def selected(t, style=1, lead=1, invert=False, max_count=ALL):
    """the line numbers grep_text selects"""
    return np.flatnonzero((t.values(style, lead) > 0) != bool(invert))[:max_count]


def filter(t, style=1, lead=1, invert=False, before=0, after=0, max_count=ALL):
    """(n_lines, n_selected, n_emitted, bytes)"""
    sel = selected(t, style, lead, invert, max_count)
    n = t.n_lines
    edge = np.zeros(n + 1, dtype=np.int64)          # +1 where a context begins, -1 behind its end
    np.add.at(edge, np.maximum(sel - before, 0), 1)
    np.add.at(edge, np.minimum(sel + after, n - 1) + 1, -1)
    emit = np.flatnonzero(np.cumsum(edge[:n]) > 0)
    return n, len(sel), len(emit), t.join(emit)


def extract(t, max_per_line=ALL):
    """(n_lines, n_matches, bytes)"""
    d = bytes([t.delim])
    got = t.items(max_per_line)
    return t.n_lines, len(got), b"".join(t.piece_bytes(it) + d for it in got)


def route(t, n_bins, style=1, lead=1, drop_unmatched=False):
    """(n_lines, n_routed, bin_lines, bin_offsets, bytes)"""
    v = t.values(style, lead)
    bucket = slots(v, n_bins)
    keep = v != 0 if drop_unmatched else np.ones(len(v), dtype=bool)
    order = np.argsort(bucket, kind="stable")
    order = order[keep[order]]
    sizes = np.zeros(n_bins + 1, dtype=np.int64)
    np.add.at(sizes, bucket[keep], np.diff(t.offs)[keep])
    return (t.n_lines, int(keep.sum()), np.bincount(bucket, minlength=n_bins + 1).astype(np.uint64),
            np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), t.join(order))


def uniq(t, matches=True, style=1, lead=1, max_per_line=ALL):
    """(n_lines, n_items, n_dropped, first, length, count): no item is dropped"""
    if matches:
        found = [(int(t.offs[it[0]]) + it[3], t.piece_bytes(it)) for it in t.items(max_per_line)]
    else:
        found = [(int(t.offs[k]), t.lines[k]) for k in selected(t, style, lead)]
    table = {}
    for at, s in found:
        if s in table:
            table[s][2] += 1
        else:
            table[s] = [at, len(s), 1]
    rows = np.array(list(table.values()), dtype=np.uint64).reshape(-1, 3)
    return t.n_lines, len(found), 0, rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()


def fields_of(t, max_fields=0):
    """every line's field list: cut at the first max_fields - 1 separators (all under 0)"""
    most = max_fields - 1 if max_fields else ALL
    per = []
    for line, got in zip(t.lines, t.pieces()):
        out, at = [], 0
        for _, _, a, e in got[:most]:
            out.append(line[at:a])
            at = e
        out.append(line[at:])
        per.append(out)
    return per


def fields(t, select, sep=b" ", max_fields=0, only_delimited=False):
    """(n_lines, n_emitted, n_fields, bytes); select is the 64-bit mask"""
    d = bytes([t.delim])
    emitted, written, rows = 0, 0, []
    for got in fields_of(t, max_fields):
        if only_delimited and len(got) == 1:
            continue
        keep = [f for j, f in enumerate(got, 1) if (select >> (min(j, 64) - 1)) & 1]
        emitted += 1
        written += len(keep)
        rows.append(sep.join(keep) + d)
    return t.n_lines, emitted, written, b"".join(rows)


def number(piece, last):
    """the piece's first / last maximal run of digits as a decimal, None without one or from 2^64"""
    runs = re.findall(rb"[0-9]+", piece)
    v = int(runs[-1 if last else 0]) if runs else M64
    return v if v < M64 else None


def empty_stats(n_bins):
    return np.array([[0] * (n_bins + 1), [0] * (n_bins + 1), [M64 - 1] * (n_bins + 1),
                     [0] * (n_bins + 1)], dtype=np.uint64)


def merge_stats(a, b):
    """accumulate: counts and sums added modulo 2^64, min of mins, max of maxes"""
    return np.stack([a[0] + b[0], a[1] + b[1], np.minimum(a[2], b[2]), np.maximum(a[3], b[3])])


def sum(t, n_bins, which="first", max_per_line=ALL, into=None):
    """(n_lines, n_items, n_numeric, stats)"""
    got = t.items(max_per_line)
    cnt, tot, lo, hi = ([0] * (n_bins + 1), [0] * (n_bins + 1), [M64 - 1] * (n_bins + 1),
                        [0] * (n_bins + 1))
    numeric = 0
    for it in got:
        v = number(t.piece_bytes(it), which == "last")
        if v is None:
            continue
        s = it[1] if 0 <= it[1] < n_bins else n_bins
        numeric += 1
        cnt[s] += 1
        tot[s] = (tot[s] + v) % M64
        lo[s] = min(lo[s], v)
        hi[s] = max(hi[s], v)
    stats = np.array([cnt, tot, lo, hi], dtype=np.uint64)
    return t.n_lines, len(got), numeric, stats if into is None else merge_stats(into, stats)


def range_expect(t, open_result, close_result=None, style=1, lead=1, emit_open=True,
                 emit_close=True, invert=False, max_ranges=ALL):
    """range_rule's state machine on this text's values: its Expect"""
    close_result = open_result if close_result is None else close_result
    return range_rule.Expect(t.values(style, lead), t.offs, t.text, open_result, close_result,
                             emit_open, emit_close, invert, max_ranges)


def range(t, open_result, close_result=None, style=1, lead=1, emit_open=True, emit_close=True,
          invert=False, max_ranges=ALL, rec_cap=0):
    """(n_lines, n_ranges, n_emitted, bytes, first_line, last_line, begin, end)"""
    x = range_expect(t, open_result, close_result, style, lead, emit_open, emit_close, invert,
                     max_ranges)
    return (x.n_lines, x.n_ranges, x.n_emitted, x.out) + tuple(r[:rec_cap] for r in x.records)
