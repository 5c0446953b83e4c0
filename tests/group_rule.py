"""group_text's rule (include/redgpu.h) in plain Python over a text_rules.Text: every line's key by
dedup_rule.keys, its value item from the same two primitives (pieces(), fields_of()), the value's
number by text_rules.number, then one dict in the order of first appearance.  group() returns
exactly what the verb's host form returns while nothing is dropped; records() the same per key
string, for the cases in which the table overflows.  What scripts/fuzz_gpu.py's `groups` mode and
tests/test_gpu_group_text.py check the GPU against.  A helper, not a test."""
import numpy as np

import dedup_rule as D
import text_rules as R

M64 = R.M64
WHATS = ("match", "field")


def values(t, what="field", value_index=2):
    """per line its value item's bytes, None where the line has no such item"""
    per = [None] * t.n_lines
    if value_index == 0:
        return per
    if what == "match":
        for i, got in enumerate(t.pieces()):
            if len(got) >= value_index:
                _, _, a, e = got[value_index - 1]
                per[i] = t.lines[i][a:e]
    elif what == "field":
        for i, cut in enumerate(R.fields_of(t)):
            if len(cut) >= value_index:
                per[i] = cut[value_index - 1]
    else:
        raise ValueError(what)
    return per


def numbers(t, what="field", key_index=1, value_index=2, which="first"):
    """per line (key offset, key bytes, the value's number or None), None for an unkeyed line"""
    out = []
    for k, v in zip(D.keys(t, what, key_index), values(t, what, value_index)):
        if k is None:
            out.append(None)
        else:
            out.append((k[0], k[1], None if v is None else R.number(v, which == "last")))
    return out


def records(t, what="field", key_index=1, value_index=2, which="first"):
    """{key bytes: [first, length, count, numeric, sum, min, max]} in the order of first appearance"""
    table = {}
    for it in numbers(t, what, key_index, value_index, which):
        if it is None:
            continue
        at, key, v = it
        rec = table.setdefault(key, [at, len(key), 0, 0, 0, M64 - 1, 0])
        rec[2] += 1
        if v is not None:
            rec[3] += 1
            rec[4] = (rec[4] + v) % M64
            rec[5] = min(rec[5], v)
            rec[6] = max(rec[6], v)
    return table


def group(t, what="field", key_index=1, value_index=2, which="first"):
    """(n_lines, n_keyed, n_numeric, n_dropped, first, length, count, stats): no key is dropped"""
    table = records(t, what, key_index, value_index, which)
    rows = np.array(list(table.values()), dtype=np.uint64).reshape(-1, 7)
    return (t.n_lines, int(rows[:, 2].sum()), int(rows[:, 3].sum()), 0, rows[:, 0].copy(),
            rows[:, 1].copy(), rows[:, 2].copy(), rows[:, 3:7].T.copy())
