"""range_text's rule (include/redgpu.h) in plain Python, for the tests: rule() over a list of
per-line values, and expect(), which feeds it the CPU oracle's search per line and cuts the text.
A helper, not a test."""
import numpy as np

OUTSIDE, OPEN, BODY, CLOSE = range(4)
UNBOUNDED = 1 << 62


def kinds(values, open_result, close_result=None):
    """what every line is, and the number of the range it belongs to (-1 outside): the two-state
    machine, read in text order"""
    close_result = open_result if close_result is None else close_result
    kind, rng, inside, begun = [], [], False, 0
    for v in values:
        if not inside:
            inside = v == open_result
            begun += inside
            kind.append(OPEN if inside else OUTSIDE)
        else:
            inside = v != close_result
            kind.append(BODY if inside else CLOSE)
        rng.append(begun - 1 if kind[-1] != OUTSIDE else -1)
    return kind, rng


def rule(values, open_result, close_result=None, emit_open=True, emit_close=True, invert=False,
         max_ranges=UNBOUNDED):
    """(emit mask, records [(first_line, last_line)], n_ranges) of the rule over per-line values"""
    kind, rng = kinds(values, open_result, close_result)
    shown = {OUTSIDE: False, OPEN: bool(emit_open), BODY: True, CLOSE: bool(emit_close)}
    emit, records = [], []
    for i, (k, r) in enumerate(zip(kind, rng)):
        counted = k != OUTSIDE and r < max_ranges
        if counted and k == OPEN:
            records.append([i, i])
        elif counted:
            records[-1][1] = i          # a range still open at the last line ends there
        emit.append((counted and shown[k]) != bool(invert))
    return emit, [tuple(r) for r in records], len(records)


class Expect:
    """the rule on the oracle's per-line search of a text: the counts, the output, the records"""

    def __init__(self, values, offs, text, open_result, close_result, emit_open, emit_close, invert,
                 max_ranges):
        self.values, self.offs = values, offs
        self.kind, self.range_of = kinds(values.tolist(), open_result, close_result)
        emit, rec, self.n_ranges = rule(values.tolist(), open_result, close_result, emit_open,
                                        emit_close, invert, max_ranges)
        self.emit = np.array(emit, dtype=bool)
        self.n_lines, self.n_emitted = len(values), int(self.emit.sum())
        self.out = b"".join(text[offs[i]:offs[i + 1]] for i in np.flatnonzero(self.emit))
        self.first_line = np.array([r[0] for r in rec], dtype=np.uint64)
        self.last_line = np.array([r[1] for r in rec], dtype=np.uint64)
        self.begin = np.array([offs[r[0]] for r in rec], dtype=np.uint64)
        self.end = np.array([offs[r[1] + 1] for r in rec], dtype=np.uint64)
        self.records = (self.first_line, self.last_line, self.begin, self.end)


_expects = {}


def values_of(name, text, style=1, lead=1, delim=0x0A):
    """search<style,lead>(line).result_ per line, 0 where it does not match - from the oracle - and
    the lines' offsets"""
    import test_gpu_grep_text as G
    w = G._want(name, text, style, lead, False, delim)
    v = np.zeros(w[0], dtype=np.int64)
    v[w[2].astype(np.int64)] = w[5]
    return v, G._lines_of(text, delim).astype(np.int64)


def expect(name, text, open_result, close_result=None, emit_open=True, emit_close=True,
           invert=False, max_ranges=UNBOUNDED, style=1, lead=1, delim=0x0A):
    close_result = open_result if close_result is None else close_result
    key = (name, text, open_result, close_result, bool(emit_open), bool(emit_close), bool(invert),
           max_ranges, style, lead, delim)
    if key not in _expects:
        v, offs = values_of(name, text, style, lead, delim)
        _expects[key] = Expect(v, offs, text, open_result, close_result, emit_open, emit_close,
                               invert, max_ranges)
    return _expects[key]
