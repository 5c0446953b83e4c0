"""The expected answer of a text too long for the oracle: block * K + tail.

The block is one of the ~64 KiB texts the per-verb GPU modules build, ENDING in the delimiter, so
every copy of it starts a line and no line reaches from one copy into the next.  The oracle classes
of those modules (imported, not copied) run on the SHORT text lead + block * 3 + tail; what they
give is brought into a per-line form (Answer) and cut at the block ends into HEAD (the lead and
block 0), MIDDLE (block 1), LAST (block 2) and TAIL.  The long text's answer is then

    HEAD  ||  MIDDLE, K - 2 times  ||  LAST  ||  TAIL

where every absolute offset of MIDDLE copy k is k * P bytes, every line index k * L lines larger
than in the short text (P = len(block), L = the block's lines), and LAST and TAIL are moved by
K - 3 copies.  Block 1 has a block in front of it and one behind it, as every block of the long
text but the first and the last has: that is what makes filter_text's context across a block border
come out right.  tests/test_periodic_expectation.py proves each expansion against the oracle run
directly over block * K + tail at K = 5 and K = 6.

Three expansions, each as numpy on the host (Expansion.numpy) and as torch on the device in slices
(Expansion.same_dev): records, output bytes, and counts (sums over lines or records).  No device
comparison allocates more than a few slices of SLICE bytes."""
import copy

import numpy as np

SLICE = 128 << 20          # bytes of expected data produced and compared at a time on the device
DELIM = 0x0A
ALL = 1 << 62


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


class Layout:
    """lead + block * K + tail: the lead (whole lines, may be empty) only moves the block's phase
    against the 2^32 boundary and belongs to HEAD"""

    def __init__(self, block, tail, lead=b""):
        assert block and block[-1] == DELIM, "the block must end in the delimiter"
        assert not lead or lead[-1] == DELIM, "the lead must be whole lines"
        self.block, self.tail, self.lead = bytes(block), bytes(tail), bytes(lead)
        self.P = len(block)
        self.L = block.count(bytes([DELIM]))
        self.lead_lines = lead.count(bytes([DELIM]))
        self.tail_lines = tail.count(bytes([DELIM]))

    def with_lead(self, lead):
        return Layout(self.block, self.tail, lead)

    def text(self, K):
        """on the host - for the short texts only"""
        return self.lead + self.block * K + self.tail

    def short(self):
        return self.text(3)

    def length(self, K):
        return len(self.lead) + self.P * K + len(self.tail)

    def n_lines(self, K):
        return self.lead_lines + self.L * K + self.tail_lines

    def line_cuts(self):
        return [self.lead_lines + self.L * k for k in (1, 2, 3)]

    def byte_cuts(self):
        return [len(self.lead) + self.P * k for k in (1, 2, 3)]

    def line_at(self, K, pos):
        """(line index, begin, finish) of the long text's line that holds byte `pos` of a block"""
        k, rel = divmod(pos - len(self.lead), self.P)
        assert 0 <= k < K
        ends = np.flatnonzero(_u8(self.block) == DELIM)
        j = int(np.searchsorted(ends, rel, "left"))
        begin = int(ends[j - 1]) + 1 if j else 0
        base = len(self.lead) + k * self.P
        return self.lead_lines + k * self.L + j, base + begin, base + int(ends[j])

    def device_text(self, K, device="cuda"):
        """the long text, assembled on the device"""
        import torch
        body = torch.from_numpy(_u8(self.block).copy()).to(device).repeat(K)
        ends = [torch.from_numpy(_u8(x).copy()).to(device) for x in (self.lead, self.tail)]
        if not self.lead and not self.tail:
            return body
        out = torch.cat([ends[0], body, ends[1]])
        del body
        return out


class Expansion:
    """HEAD || MIDDLE^(K-2) || LAST || TAIL of one array; `shift` is added k times to MIDDLE copy k
    and K - 3 times to LAST and TAIL"""

    def __init__(self, parts, K, shift=0):
        assert len(parts) == 4 and K >= 2
        self.parts = [np.ascontiguousarray(p) for p in parts]
        self.K, self.shift = K, int(shift)
        self.dtype = self.parts[0].dtype
        h, m, l, t = (len(p) for p in self.parts)
        if K == 2:
            assert m == 0
        self.edges = [0, h, h + (K - 2) * m, h + (K - 2) * m + l, h + (K - 2) * m + l + t]
        self.n = self.edges[-1]
        self._dev = {}

    def __len__(self):
        return self.n

    def _moved(self, part, times):
        if not self.shift or not len(part):
            return part
        return (part.astype(np.int64) + times * self.shift).astype(self.dtype)

    def numpy(self):
        h, m, l, t = self.parts
        mid = np.tile(m, self.K - 2)
        if self.shift and len(m):
            mid = (mid.astype(np.int64) +
                   np.repeat(np.arange(self.K - 2, dtype=np.int64), len(m)) * self.shift).astype(self.dtype)
        return np.concatenate([h, mid, self._moved(l, self.K - 3), self._moved(t, self.K - 3)])

    def at(self, i):
        """element i, by arithmetic"""
        i = int(i)
        assert 0 <= i < self.n
        e = self.edges
        if i < e[1]:
            return int(self.parts[0][i])
        if i < e[2]:
            k, j = divmod(i - e[1], len(self.parts[1]))
            return int(self.parts[1][j]) + k * self.shift
        part = self.parts[2] if i < e[3] else self.parts[3]
        return int(part[i - (e[2] if i < e[3] else e[3])]) + (self.K - 3) * self.shift

    def tail_index(self):
        """the index of the TAIL's first element"""
        return self.edges[3]

    def _part_dev(self, k, device):
        import torch
        key = (k, str(device))
        if key not in self._dev:
            p = self.parts[k]
            if p.dtype == np.uint64:
                p = p.astype(np.int64)
            self._dev[key] = torch.from_numpy(p.copy()).to(device)
        return self._dev[key]

    def slice_dev(self, a, b, device="cuda"):
        """elements [a, b) as a tensor on the device (uint64 arrays as int64)"""
        import torch
        assert 0 <= a <= b <= self.n
        e, got = self.edges, []
        for k in range(4):
            lo, hi = max(a, e[k]), min(b, e[k + 1])
            if lo >= hi:
                continue
            part = self._part_dev(k, device)
            if k == 1:
                m = len(self.parts[1])
                x0, cnt = lo - e[1], hi - lo
                phase = x0 % m
                x = part.repeat((phase + cnt + m - 1) // m)[phase:phase + cnt]
                if self.shift:
                    x = x + torch.div(torch.arange(x0, x0 + cnt, device=device), m,
                                      rounding_mode="floor") * self.shift
            else:
                x = part[lo - e[k]:hi - e[k]]
                if self.shift and k >= 2:
                    x = x + (self.K - 3) * self.shift
            got.append(x)
        if not got:
            return self._part_dev(0, device)[:0]
        return got[0] if len(got) == 1 else torch.cat(got)

    def same_dev(self, got, upto=None, where=None):
        """got[:min(upto, n)] equals the expansion, compared on the device slice by slice"""
        import torch
        n = self.n if upto is None else min(int(upto), self.n)
        assert got.numel() >= n, (where, got.numel(), n)
        step = max(1, SLICE // max(1, got.element_size()))
        for a in range(0, n, step):
            b = min(n, a + step)
            want = self.slice_dev(a, b, got.device)
            assert want.dtype == got.dtype, (where, want.dtype, got.dtype)
            if not torch.equal(got[a:b], want):
                bad = int((got[a:b] != want).nonzero()[0]) + a
                raise AssertionError((where, "element", bad, "is", int(got[bad]), "expected",
                                      self.at(bad), "of", n))
            del want


class Answer:
    """what an oracle class gave for ONE text, in the form that can be cut at block ends.
    rows:    name -> (array with one entry per record, kind); kind "byte" = an absolute offset,
             "line" = a line index, None = neither (a result, a position inside the line)
    row_line: the line of every record, ascending
    streams: name -> (bytes, per-line sizes): the output bytes and how many of them each line
             contributed, in line order; bytes behind the lines' share belong to the TAIL
    sums:    name -> (array, "line" | "row", fn): a count that is fn(entries of a part), summed
             over the parts; fn returns an int or an int array"""

    def __init__(self, n_lines):
        self.n_lines = int(n_lines)
        self.rows, self.row_line, self.row_pos = {}, np.zeros(0, dtype=np.int64), None
        self.streams, self.sums = {}, {}
        self.sums["n_lines"] = (np.ones(self.n_lines, dtype=np.int64), "line", np.sum)


class Expected:
    """counts: name -> int or int array; rows / streams: name -> Expansion"""

    def __init__(self):
        self.counts, self.rows, self.streams = {}, {}, {}

    def host(self):
        """everything as plain numpy / ints / bytes, for == against another Expected.host()"""
        out = {}
        for k, v in self.counts.items():
            out[("count", k)] = np.asarray(v).astype(np.int64).tolist()
        for k, v in self.rows.items():
            out[("rows", k)] = v.numpy().astype(np.int64).tolist()
        for k, v in self.streams.items():
            out[("stream", k)] = v.numpy().tobytes()
        return out


def _build(ans, line_cuts, K, P, L, byte_cuts=None):
    x = Expected()
    cuts = [min(c, ans.n_lines) for c in line_cuts]
    if ans.row_pos is None:
        rl = np.asarray(ans.row_line, dtype=np.int64)
        rcuts = [int(v) for v in np.searchsorted(rl, cuts, "left")]
    else:       # a long-text verb's records: cut where they begin, not by their line
        rl = np.asarray(ans.row_pos, dtype=np.int64)
        rcuts = [int(v) for v in np.searchsorted(rl, byte_cuts, "left")]
    assert not len(rl) or (np.diff(rl) >= 0).all()

    def four(arr, c):
        return [arr[:c[0]], arr[c[0]:c[1]], arr[c[1]:c[2]], arr[c[2]:]]

    for name, (arr, kind) in ans.rows.items():
        assert len(arr) == len(rl), name
        x.rows[name] = Expansion(four(np.asarray(arr), rcuts), K, {"byte": P, "line": L, None: 0}[kind])
    x.counts["n_rows"] = len(rl[:rcuts[0]]) + (K - 2) * (rcuts[1] - rcuts[0]) + len(rl) - rcuts[1]
    for name, (data, sizes) in ans.streams.items():
        if ans.row_pos is not None:     # a long-text verb's output: `sizes` are the three cuts
            assert list(sizes) == sorted(sizes) and sizes[2] <= len(data)
            x.streams[name] = Expansion(four(_u8(data), [int(c) for c in sizes]), K)
            continue
        assert len(sizes) == ans.n_lines, name
        cs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
        assert cs[-1] <= len(data), name
        x.streams[name] = Expansion(four(_u8(data), [int(cs[c]) for c in cuts]), K)
    for name, (arr, axis, fn) in ans.sums.items():
        parts = four(np.asarray(arr), cuts if axis == "line" else rcuts)
        vals = [np.asarray(fn(p)).astype(np.int64) for p in parts]
        x.counts[name] = vals[0] + (K - 2) * vals[1] + vals[2] + vals[3]
    return x


def expand(ans, lay, K):
    """the answer for lay's short text, expanded to lead + block * K + tail"""
    assert K >= 3
    if ans.row_pos is None:
        assert ans.n_lines == lay.n_lines(3), (ans.n_lines, lay.n_lines(3))
    x = _build(ans, lay.line_cuts(), K, lay.P, lay.L, lay.byte_cuts())
    assert ans.row_pos is not None or x.counts["n_lines"] == lay.n_lines(K)
    x.answer, x.lay, x.K = ans, lay, K
    return x


def whole(ans):
    """the answer of a text as it is: all of it HEAD, nothing repeated"""
    big = ans.n_lines + 1
    return _build(ans, [big, big, big], 2, 0, 0, [ALL, ALL, ALL])


# the oracle classes of the per-verb modules, brought into the per-line form ---------------------

def lines_answer(text):
    """split_lines: offsets[k] = where line k begins; the closing offset is lines_end()"""
    import test_gpu_grep_text as GT
    offs = GT._lines_of(text)
    a = Answer(len(offs) - 1)
    a.row_line = np.arange(a.n_lines, dtype=np.int64)
    a.rows["offsets"] = (offs[:-1], "byte")
    return a


def lines_end(lay, K):
    """offsets[n_lines]: one past the last delimiter"""
    last = lay.tail.rfind(bytes([DELIM]))
    return len(lay.lead) + lay.P * K + last + 1


def search_lines_answer(name, text, style, lead):
    """search<style,lead> on every line alone (what match_batch / search_batch over
    (offsets, stride=1) and grep_text's records are made of): result, start, end per line"""
    import test_gpu_grep_text as GT
    GT._want(name, text, style, lead, False)
    offs, r, s, e = GT._wants[(name, text, style, lead, DELIM)]
    a = Answer(len(offs) - 1)
    a.row_line = np.arange(a.n_lines, dtype=np.int64)
    a.rows.update(result=(r, None), start=(s, None), end=(e, None))
    return a


def match_lines_answer(name, text, style, lead):
    """match_text: match<style,lead> on every line alone, and check's result"""
    import test_gpu_match_text_placements as MT
    offs, n, (r, s, e), c = MT._expect(name, ("periodic", text), text, style, lead)
    a = Answer(n)
    a.row_line = np.arange(n, dtype=np.int64)
    a.rows.update(offsets=(offs[:-1], "byte"), result=(r, None), start=(s, None), end=(e, None),
                  check=(c, None))
    return a


def grep_answer(name, text, style, lead, invert=False):
    import test_gpu_grep_text as GT
    w = GT._want(name, text, style, lead, invert)
    a = Answer(w[0])
    a.row_line = w[2].astype(np.int64)
    for key, arr, kind in zip(("line", "begin", "finish", "result", "start", "end"), w[2:],
                              ("line", "byte", "byte", None, None, None)):
        a.rows[key] = (arr, kind)
    return a


def collect_answer(name, text):
    import test_gpu_collect_text as CT
    w = CT._want(name, text)
    a = Answer(w.n_lines)
    a.row_line = w.line.astype(np.int64)
    for key, arr, kind in zip(CT.NAMES, w.arrays(), ("line", "byte", None, "byte", "byte")):
        a.rows[key] = (arr, kind)
    # (collect_batch's positions are relative to the line)
    a.rows["start_in_line"] = (w.start - w.begin, None)
    a.rows["end_in_line"] = (w.end - w.begin, None)
    return a


def collect_counts_answer(name, text):
    """collect_batch over (offsets, stride=1): how many records every line has"""
    import test_gpu_collect_text as CT
    w = CT._want(name, text)
    a = Answer(w.n_lines)
    a.row_line = np.arange(w.n_lines, dtype=np.int64)
    a.rows["counts"] = (w.counts.astype(np.uint64), None)
    return a


def tally_answer(name, text, n_bins, matches, style=1, lead=1):
    import test_gpu_tally_text as TT
    n_lines, n_items, values = TT._items(name, text, matches, style, lead)
    a = Answer(n_lines)
    if matches:
        import test_gpu_collect_text as CT
        a.row_line = CT._want(name, text).line.astype(np.int64)
        axis = "row"
    else:
        axis = "line"
    a.sums["bins"] = (values, axis, lambda v: TT._bins(v, n_bins))
    a.sums["n_items"] = (values, axis, lambda v: int((np.asarray(v) > 0).sum()))
    return a


def replace_answer(name, text, repl, style, lead, mx, only_changed):
    import test_gpu_replace_text as RT
    w = RT._want(name, text, repl, style, lead, mx)
    a = Answer(w.n_lines)
    sizes = np.array([len(x) + 1 for x in w.new], dtype=np.int64)
    if only_changed:
        sizes = sizes * (w.counts > 0)
    a.streams["out"] = (w.out[1 if only_changed else 0], sizes)
    a.sums["n_replaced"] = (w.counts, "line", np.sum)
    return a


def filter_answer(name, text, style, lead, invert, before, after):
    import test_gpu_filter_text as FT
    x = FT._expect(name, text, style, lead, invert, before, after)
    a = Answer(x.n_lines)
    sel = np.zeros(x.n_lines, dtype=np.int64)
    sel[x.sel] = 1
    a.streams["out"] = (x.out, np.diff(np.asarray(x.offs, dtype=np.int64)) * x.emit)
    a.row_line = np.asarray(x.sel, dtype=np.int64)
    a.rows["sel"] = (a.row_line.astype(np.uint64), "line")
    a.emit, a.after = x.emit.astype(np.int64), after
    a.sums["n_selected"] = (sel, "line", np.sum)
    a.sums["n_emitted"] = (x.emit.astype(np.int64), "line", np.sum)
    return a


def extract_answer(name, text, m=ALL):
    import test_gpu_extract_text as XT
    x = XT._oracle(name, text)
    n, out = x.out(m)
    a = Answer(x.n_lines)
    a.streams["out"] = (out, np.array([sum(len(p) + 1 for p in got[:m]) for got in x.per_line],
                                      dtype=np.int64))
    a.sums["n_matches"] = (np.array([len(got[:m]) for got in x.per_line], dtype=np.int64), "line",
                           np.sum)
    assert int(a.sums["n_matches"][0].sum()) == n
    return a


def fields_answer(name, text, fields, only, sep, max_fields=0):
    """test_gpu_fields_text._Fields.out gives the whole text's output: the share of every line is
    what the same method gives for a copy of the object that holds that line alone"""
    import test_gpu_fields_text as FL
    x = FL._oracle(name, text)
    n_lines, emitted, written, out = x.out(fields, max_fields, only, sep)
    per = x.per_line(max_fields)
    most = max_fields - 1 if max_fields else FL.UNBOUNDED
    sizes, emit, wrote = (np.zeros(n_lines, dtype=np.int64) for _ in range(3))
    for k in range(n_lines):
        one = copy.copy(x)
        one._per = {most: per[k:k + 1]}
        _, emit[k], wrote[k], piece = one.out(fields, max_fields, only, sep)
        sizes[k] = len(piece)
    assert (int(emit.sum()), int(wrote.sum()), int(sizes.sum())) == (emitted, written, len(out))
    a = Answer(n_lines)
    a.streams["out"] = (out, sizes)
    a.sums["n_emitted"] = (emit, "line", np.sum)
    a.sums["n_fields"] = (wrote, "line", np.sum)
    return a


def route_answer(name, text, n_bins, drop, style=1, lead=1):
    """one stream per bucket: the bucket's section of the output"""
    import test_gpu_route_text as RO
    x = RO._expect(name, text, n_bins, drop, style, lead)
    a = Answer(x.n_lines)
    lens = np.diff(x.offs)
    for b in range(n_bins + 1):
        a.streams[b] = (x.section(b), lens * (x.keep & (x.bucket == b)))
    a.sums["bin_lines"] = (x.bucket, "line", lambda v: np.bincount(v, minlength=n_bins + 1))
    a.sums["n_routed"] = (x.keep.astype(np.int64), "line", np.sum)
    return a


def route_offsets(x, n_bins):
    """bin_offsets[n_bins + 2] of an expanded route_answer: the sections' lengths, summed"""
    return np.concatenate([[0], np.cumsum([len(x.streams[b]) for b in range(n_bins + 1)])]).astype(
        np.int64)


def uniq_items(name, text, matches, style=1, lead=1, m=ALL):
    """(items, n_lines): uniq_text's items (offset, bytes) in text order"""
    import test_gpu_uniq_text as UT
    return UT._match_items(name, text, m=m) if matches else UT._line_items(name, text, style, lead)


def uniq_expand(items, lay, K):
    """(n_items, first, length, count) of the long text from the short text's items: a string's
    count is summed over the copies, its first occurrence is in block 0 (every string of a later
    block stands there too) or in the tail, K - 3 blocks further on than in the short text"""
    cuts = lay.byte_cuts()
    table = {}
    for at, s in items:
        part = int(np.searchsorted(cuts, at, "right"))
        if s not in table:
            assert part in (0, 3), (at, s)
            table[s] = [at + (K - 3) * lay.P if part == 3 else at, len(s), [0, 0, 0, 0]]
        table[s][2][part] += 1
    rows = sorted((f, n, c[0] + (K - 2) * c[1] + c[2] + c[3]) for f, n, c in table.values())
    arr = np.array(rows, dtype=np.int64).reshape(len(rows), 3)
    return int(arr[:, 2].sum()), arr[:, 0], arr[:, 1], arr[:, 2]


def prefix_through(sizes, lay, K, line):
    """sum of a per-line quantity of the SHORT text over the long text's lines 0..line"""
    c = [0] + lay.line_cuts()
    sizes = np.asarray(sizes, dtype=np.int64)
    head, mid, last = (int(sizes[c[k]:c[k + 1]].sum()) for k in range(3))
    if line < c[1]:
        return int(sizes[:line + 1].sum())
    k, j = divmod(line - c[1], lay.L)          # k whole blocks behind block 0, j into the next
    if k < K - 2:
        return head + k * mid + int(sizes[c[1]:c[1] + j + 1].sum())
    if k == K - 2:
        return head + (K - 2) * mid + int(sizes[c[2]:c[2] + j + 1].sum())
    return head + (K - 2) * mid + last + int(sizes[c[3]:c[3] + (line - c[1] - (K - 1) * lay.L) + 1].sum())


# the blocks, the tails and the cases shared by the CPU proof and the GPU module ------------------

N = 4 * 16384 + 5


def standard_block(name):
    """test_gpu_grep_text._standard: the piece in about a third of the lines (sparse records)"""
    import test_gpu_collect_text as CT      # (its PIECES has every DFA's piece)
    import test_gpu_grep_text as GT
    return GT._standard(CT.PIECES[name](), n=N, end_in_delim=True)


def dense_block(name):
    """test_gpu_collect_text._dense: the planted lines full of the piece"""
    import test_gpu_collect_text as CT
    return CT._dense(CT.PIECES[name](), n=N, end_in_delim=True)


def planted_block(name):
    """test_gpu_fields_text._planted: separators every few bytes"""
    import test_gpu_fields_text as FL
    return FL._planted(name, n=N, end_in_delim=True)


def _tail_of(pieces, last):
    """17 lines, the k-th with k bytes in front of its piece - so whatever the tail's own phase,
    one of them straddles a 16-byte boundary - then a fragment without a delimiter"""
    rows = [b"z" * k + b" " + pieces[k % len(pieces)] + b" t" + bytes([0x61 + k]) for k in range(17)]
    return b"\n".join(rows) + b"\n" + b"left over " + last


def tail_for(name):
    """a short text of its own for every DFA: matches that stand nowhere in the block (where the
    DFA's language has more than one word), lines that stand nowhere in it, no delimiter at the end"""
    from one_amd import workloads as W
    heads = W.log100_heads()
    return {
        "err": _tail_of([b"error", b"errors error"], b"error"),
        "log100": _tail_of([heads[50], heads[51] + heads[52]], heads[53]),
        "uri": _tail_of([b"http://tail.example.org/p%d" % k for k in range(5)], b"http://x.io/y"),
        "num3": _tail_of([b"31415", b"27182 9999a", b"1618"], b"4242"),
        "ws": _tail_of([b"T1 \t T2", b"T3  T4\tT5 T6"], b"T7 T8"),
        "comma": _tail_of([b"T1,T2", b"T3,,T4,T5,T6"], b"T7,T8"),
    }[name]


BLOCKS = {"standard": standard_block, "dense": dense_block, "planted": planted_block}
_layouts = {}


def layout(kind, name):
    if (kind, name) not in _layouts:
        tail = tail_for(name)
        assert tail[-1] != DELIM, "the tail must not end in the delimiter"
        _layouts[(kind, name)] = Layout(BLOCKS[kind](name), tail)
    return _layouts[(kind, name)]


LAST, FULL, INSTANT = 4, 5, 1
ANSWERS = {
    "lines": lambda text, name: lines_answer(text),
    "match": lambda text, name, style, lead: match_lines_answer(name, text, style, lead),
    "search_lines": lambda text, name, style, lead: search_lines_answer(name, text, style, lead),
    "grep": lambda text, name, style, lead, invert: grep_answer(name, text, style, lead, invert),
    "collect": lambda text, name: collect_answer(name, text),
    "collect_counts": lambda text, name: collect_counts_answer(name, text),
    "tally": lambda text, name, n_bins, matches: tally_answer(name, text, n_bins, matches),
    "replace": lambda text, name, repl, mx, oc: replace_answer(name, text, repl, LAST, 1, mx, oc),
    "filter": lambda text, name, invert, before, after: filter_answer(name, text, INSTANT, 1, invert,
                                                                      before, after),
    "extract": lambda text, name, m: extract_answer(name, text, m),
    "fields": lambda text, name, fields, only, sep: fields_answer(name, text, fields, only, sep),
    "route": lambda text, name, n_bins, drop: route_answer(name, text, n_bins, drop),
}
# (verb, block kind, DFA, the verb's parameters): what tests/test_gpu_text_past_4gib.py runs, and
# what tests/test_periodic_expectation.py therefore proves
CASES = [
    ("lines", "standard", "log100"),
    ("match", "standard", "uri", LAST, 0), ("match", "standard", "uri", FULL, 0),
    ("match", "standard", "log100", LAST, 1),
    ("search_lines", "standard", "uri", INSTANT, 0), ("search_lines", "standard", "log100", INSTANT, 1),
    ("grep", "standard", "log100", INSTANT, 1, False), ("grep", "standard", "log100", LAST, 1, False),
    ("grep", "standard", "log100", INSTANT, 1, True), ("grep", "standard", "log100", LAST, 0, True),
    ("collect", "dense", "log100"), ("collect", "dense", "uri"),
    ("collect", "standard", "log100"), ("collect_counts", "standard", "log100"),
    ("tally", "dense", "log100", 8, True), ("tally", "dense", "log100", 101, True),
    ("tally", "dense", "log100", 8, False), ("tally", "dense", "log100", 101, False),
    ("replace", "dense", "err", b"x", ALL, 0), ("replace", "dense", "err", b"ERROR", 1, 0),
    ("replace", "dense", "err", b"<error!>", ALL, 0), ("replace", "dense", "err", b"<error!>", 1, 1),
    ("filter", "standard", "log100", False, 0, 0), ("filter", "standard", "log100", False, 2, 0),
    ("filter", "standard", "log100", True, 0, 2), ("filter", "standard", "log100", False, 2, 2),
    ("filter", "standard", "log100", False, 9, 9),
    ("extract", "standard", "log100", ALL), ("extract", "standard", "log100", 1),
    ("extract", "dense", "num3", ALL),
    ("fields", "planted", "ws", "1", False, b" "), ("fields", "planted", "ws", "1,3", True, b""),
    ("fields", "planted", "ws", "2-", False, b"12345678"),
    ("fields", "planted", "comma", "2-", True, b";"), ("fields", "planted", "comma", "1,3", False, b""),
    ("fields", "planted", "comma", "2", True, b" "), ("fields", "planted", "comma", "2-", False, b" | "),
    ("route", "standard", "log100", 101, False), ("route", "standard", "log100", 101, True),
    ("route", "standard", "log100", 2, False), ("route", "standard", "log100", 2, True),
]
# uniq_text: (block kind, DFA, matches, max_per_line)
UNIQ_CASES = [("standard", "num3", True, ALL), ("standard", "num3", True, 1),
              ("standard", "log100", False, ALL)]


def case_id(case):
    return "-".join(x.decode() if isinstance(x, bytes) else str(x) for x in case)


def cases_of(verb):
    return [c for c in CASES if c[0] == verb]


def answer(case, text):
    return ANSWERS[case[0]](text, *case[2:])


_expanded = {}


def expected(case, K, lead=b""):
    """the case's expansion to K blocks (behind `lead`), computed once"""
    key = (case, K, lead)
    if key not in _expanded:
        lay = layout(case[1], case[2]).with_lead(lead)
        _expanded[key] = expand(answer(case, lay.short()), lay, K)
    return _expanded[key]


def block_spans(name, block):
    """[start, end) of every match of the DFA in the block's lines, block-relative"""
    import test_gpu_fields_text as FL
    if name not in FL.CRAFTED:
        a = collect_answer(name, block)
        return list(zip(a.rows["start"][0].astype(np.int64).tolist(),
                        a.rows["end"][0].astype(np.int64).tolist()))
    import oracle as O
    cpu, spans, begin = O.CpuOracle(FL._blob(name)), [], 0
    for line in O.split_lines_loop(block, DELIM):
        recs, cnt = cpu.collect(line, 4096)
        assert cnt == len(recs)
        spans += [(begin + s, begin + e) for _, s, e in recs]
        begin += len(line) + 1
    return spans


def lead_for(lay, boundary, spans):
    """whole lines to put in front of block 0 so that byte `boundary` - 1 and byte `boundary` of
    the long text both lie in one match of a block: the fewest bytes that do it, in lines of at
    most 64 bytes that hold nothing but '~'"""
    assert not lay.lead
    rel = boundary % lay.P
    if any(e - s >= 2 for s, e in spans):
        d = min((rel - (s + 1)) % lay.P for s, e in spans if e - s >= 2)
    else:                       # one-byte matches: byte `boundary` is one
        d = min((rel - s) % lay.P for s, e in spans)
    lead = b""
    while len(lead) < d:
        n = min(64, d - len(lead))
        lead += b"~" * (n - 1) + b"\n"
    return lead


def straddles(lay, boundary, spans):
    """does a match of some block hold both byte boundary - 1 and byte boundary?  (Where every
    match is one byte: is byte boundary one?)"""
    rel = (boundary - len(lay.lead)) % lay.P
    if any(e - s >= 2 for s, e in spans):
        return any(s < rel < e for s, e in spans)
    return any(s == rel for s, e in spans)


def first_at_least(exp, value):
    """the index of the first element of an ascending Expansion that is >= value (len if none)"""
    lo, hi = 0, len(exp)
    while lo < hi:
        mid = (lo + hi) // 2
        if exp.at(mid) >= value:
            hi = mid
        else:
            lo = mid + 1
    return lo


def filter_first(x, mx):
    """(n_emitted, out_len) of an expanded filter_answer under max_count = mx <= n_selected: the
    output is the unbounded one's up to the line `after` behind the mx-th selected line (a line in
    front of that one which a later selected line's `before` reaches is in the mx-th's own)"""
    ans, lay, K = x.answer, x.lay, x.K
    last = min(x.rows["sel"].at(mx - 1) + ans.after, lay.n_lines(K) - 1)
    return (prefix_through(ans.emit, lay, K, last),
            prefix_through(ans.streams["out"][1], lay, K, last))


def stream_layout(exp):
    """an expanded output as a text of its own: lead = HEAD, block = MIDDLE, tail = LAST + TAIL,
    with K - 2 blocks"""
    h, m, l, t = (p.tobytes() for p in exp.parts)
    return Layout(m, l + t, h), exp.K - 2


# the long-text verbs: ONE text, no lines --------------------------------------------------------------

def _long_cpu(name):
    import oracle as O
    import test_gpu_collect_text as CT
    if name not in CT._oracles:
        CT._oracles[name] = O.CpuOracle(CT._blob(name))
    return CT._oracles[name]


def _records_answer(recs, count):
    assert count == len(recs)
    a = Answer(0)
    arr = np.array(recs, dtype=np.int64).reshape(len(recs), 3)
    a.row_pos = arr[:, 1]
    a.rows.update(result=(arr[:, 0].astype(np.int32), None), start=(arr[:, 1].astype(np.uint64), "byte"),
                  end=(arr[:, 2].astype(np.uint64), "byte"))
    return a


def collect_long_answer(name, text):
    """Red::collect over the whole text (test_gpu_collect_long._expect)"""
    import test_gpu_collect_long as CL
    import test_gpu_collect_text as CT
    return _records_answer(*CL._expect(CT._blob(name), text))


def match_all_long_answer(name, text, lead):
    cpu = _long_cpu(name)
    recs, count = cpu.match_all(text, bool(lead), 4096)
    if count > len(recs):
        recs, count = cpu.match_all(text, bool(lead), count)
    return _records_answer(recs, count)


def replace_long_answer(name, text, repl, mx, byte_cuts):
    """replace<styLast,true> over the whole text; the output is cut where the rewritten prefixes
    text[:cut] end - no match reaches across a block end (dies_at_line_ends)"""
    import test_gpu_collect_text as CT
    import test_gpu_replace_long as RL
    count, out = RL._expect(CT._blob(name), text, repl, LAST, 1, mx)
    a = Answer(0)
    a.row_pos = np.zeros(0, dtype=np.int64)
    cuts, done = [], []
    for c in byte_cuts:
        if c >= len(text):
            cuts.append(len(out))
            continue
        k, pre = RL._expect(CT._blob(name), text[:c], repl, LAST, 1, mx)
        assert out.startswith(pre)
        cuts.append(len(pre))
        done.append(k)
    a.streams["out"] = (out, cuts)
    # the count, cut the same way: per "line" one entry would do; here the four parts directly
    parts = np.diff([0] + done + [count]) if len(done) == 3 else np.array([count, 0, 0, 0])
    a.part_counts = parts
    return a


def replaced_count(ans, K):
    h, m, l, t = (int(v) for v in ans.part_counts)
    return h + (K - 2) * m + l + t


def dies_at_line_ends(name, block):
    """the state argument for collect_long / replace_long: whichever byte of the block an attempt
    begins at, it is in the pure dead state behind its line's delimiter - so at every block start
    (the block ends in a delimiter) the chain of searches is where it is at the text's begin"""
    import oracle as O
    cpu = _long_cpu(name)
    data = _u8(block)
    ends = np.flatnonzero(data == DELIM)
    begin, pieces = 0, []
    for e in ends:
        pieces += [data[p:e + 1] for p in range(begin, e + 1)]
        begin = int(e) + 1
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
    st = np.full(len(pieces), O.STATE_INITIAL, dtype=np.uint32)
    cpu.advance_batch(np.concatenate(pieces), st, offsets=offsets)
    dead = np.unique(st)
    if len(dead) != 1:
        return False
    nxt = np.full(256, dead[0], dtype=np.uint32)
    res = cpu.advance_batch(np.arange(256, dtype=np.uint8), nxt, stride=1, n=256)
    return bool((nxt == dead[0]).all() and (res == 0).all())


def state_after(name, text):
    """the state of ONE walk over the text from the initial state (match_all_long's walk)"""
    import oracle as O
    st = np.full(1, O.STATE_INITIAL, dtype=np.uint32)
    _long_cpu(name).advance_batch(_u8(text), st, offsets=[0, len(text)])
    return int(st[0])


def blank_block(name, n=N):
    """test_gpu_search_long._blank: alphabet bytes with every match overwritten"""
    import test_gpu_collect_text as CT
    import test_gpu_search_long as SL
    return bytes(SL._blank(name, CT._blob(name), n, 21))


def newyork_block(n=N):
    """test_gpu_match_all_long._planted: fill bytes with "New York" every few hundred bytes"""
    import test_gpu_match_all_long as MA
    return MA._planted(n, b"New York")


LONG_NAME = "log100"                    # collect_long / replace_long: the standard block and tail
LONG_REPLS = [(b"x", ALL), (b"<a longer replacement>", ALL)]
SEARCH_NAME, SEARCH_TAIL = "num3", b"qq zz ww 31415 yy"
SEARCH_SETTINGS = [(style, lead) for style in (INSTANT, 2, LAST) for lead in (0, 1)]
NEWYORK_TAIL = b"\x01\x01 New York \x01 New \x01\x01 York New York"


def span_sum(start, end, count):
    """the sum of end - start over the first `count` records of two Expansions cut alike"""
    lens = [e.astype(np.int64) - s.astype(np.int64) for s, e in zip(start.parts, end.parts)]
    total, left = 0, int(count)
    for k, part in enumerate(lens):
        if k == 1 and len(part):
            whole_copies = min(left // len(part), start.K - 2)
            total += whole_copies * int(part.sum())
            left -= whole_copies * len(part)
            if whole_copies < start.K - 2:
                return total + int(part[:left].sum())
            continue
        take = min(left, len(part))
        total += int(part[:take].sum())
        left -= take
    assert left == 0
    return total


def replace_long_first(records, repl, mx, length):
    """replace_long under max_count = mx <= the records: (out_len, cut, rest) - the output is the
    unbounded one's first `cut` bytes, then the text from byte `rest` on"""
    rest = records.rows["end"].at(mx - 1)
    cut = rest - span_sum(records.rows["start"], records.rows["end"], mx) + mx * len(repl)
    return cut + length - rest, cut, rest
