"""dedup_text's rule (include/redgpu.h) in plain Python over a text_rules.Text: every line's key
from the Text's two primitives - the LINES (selected()) and the PIECES (pieces(), fields_of()) -
then the marks from one dict, then the emitted lines.  dedup() returns exactly what the verb's host
form returns while nothing is dropped; what scripts/fuzz_gpu.py's `keys` mode and
tests/test_gpu_dedup_text.py check the GPU against.  A helper, not a test."""
import text_rules as R

MAX = (1 << 64) - 1
WHATS = ("whole", "lines", "match", "field")


def keys(t, what="whole", key_index=1, style=1, lead=1):
    """per line its key's (absolute offset, bytes), None for an unkeyed line"""
    per = [None] * t.n_lines
    if what == "whole":
        for i, line in enumerate(t.lines):
            per[i] = (int(t.offs[i]), line)
    elif what == "lines":
        for i in R.selected(t, style, lead).tolist():
            per[i] = (int(t.offs[i]), t.lines[i])
    elif what == "match":
        for i, got in enumerate(t.pieces()):
            if len(got) >= key_index:
                _, _, a, e = got[key_index - 1]
                per[i] = (int(t.offs[i]) + a, t.lines[i][a:e])
    elif what == "field":
        for i, (got, cut) in enumerate(zip(t.pieces(), R.fields_of(t))):
            if len(cut) >= key_index:
                at = got[key_index - 2][3] if key_index > 1 else 0
                per[i] = (int(t.offs[i]) + at, cut[key_index - 1])
    else:
        raise ValueError(what)
    return per


def emitted(per, min_count=1, max_count=MAX, invert=False, keep_unkeyed=False):
    """(n_keyed, n_distinct, the emitted line numbers) from keys()' list"""
    count, first = {}, {}
    for i, k in enumerate(per):
        if k is not None:
            count[k[1]] = count.get(k[1], 0) + 1
            first.setdefault(k[1], i)
    out = []
    for i, k in enumerate(per):
        if k is None:
            if keep_unkeyed:
                out.append(i)
        else:
            marked = first[k[1]] == i and min_count <= count[k[1]] <= max_count
            if marked != bool(invert):
                out.append(i)
    return len(per) - per.count(None), len(count), out


def dedup(t, what="whole", key_index=1, style=1, lead=1, min_count=1, max_count=MAX, invert=False,
          keep_unkeyed=False):
    """(n_lines, n_keyed, n_distinct, n_dropped, n_emitted, bytes): no key is dropped"""
    n_keyed, n_distinct, out = emitted(keys(t, what, key_index, style, lead), min_count, max_count,
                                       invert, keep_unkeyed)
    return t.n_lines, n_keyed, n_distinct, 0, len(out), t.join(out)
