"""tests/group_rule.py (group_text's rule over a text_rules.Text) needs no GPU to be held to account:
it equals a brute force written from the header's words alone - plain loops over bytes and a dict,
no `re`, over items that come from the per-verb oracles of the extract_text and fields_text modules
and not from text_rules - on the five DFAs of test_gpu_group_text's matrix; the header's identities
hold (the counts are dedup_text's, the records without a value uniq_text's, the statistics merged
over all keys sum_text's); and the matrix cannot pass vacuously: every matrix text meets floors on
what the oracle's side holds, and scripts/fuzz_gpu.py's `groups` mode, run dry at the case count
and seed of test_gpu_group_text's smoke test, meets floors of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_rule as DR
import group_rule as GR
import text_rules as TR

import test_gpu_dedup_text as DD
import test_gpu_extract_text as XT
import test_gpu_fields_text as FD
import test_gpu_group_text as GG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DFAS = ["num3", "err", "aab", "log100", "uri"]
M64 = 1 << 64


def _pairs(t):
    """test_gpu_group_text's (key_index, value_index) pairs"""
    most = max(len(p) for p in t.pieces())
    return [(1, 2), (2, 1), (1, 1), (1, 0), (2, most + 1), (most + 2, 1)]


def _brute_number(item, last):
    """the first / last maximal run of bytes '0'..'9' as a decimal, digit by digit: None without a
    run or from 2^64 on"""
    runs, run = [], None
    for byte in item:
        if 0x30 <= byte <= 0x39:
            run = (0 if run is None else run) * 10 + (byte - 0x30)
        elif run is not None:
            runs.append(run)
            run = None
    if run is not None:
        runs.append(run)
    if not runs:
        return None
    v = runs[-1] if last else runs[0]
    return v if v < M64 else None


def _brute(name, text, what, k, v, which):
    """(n_lines, n_keyed, n_numeric, [key bytes, count, numeric, sum, min, max] in the order of first
    appearance): the items from the per-verb oracles, a loop and a dict"""
    per = XT._oracle(name, text).per_line if what == "match" else FD._oracle(name, text).per_line()
    order, table = [], {}
    keyed = numeric = 0
    for items in per:
        if len(items) < k:
            continue                                  # unkeyed: the value is not looked at
        key = bytes(items[k - 1])
        keyed += 1
        if key not in table:
            table[key] = [key, 0, 0, 0, M64 - 1, 0]
            order.append(key)
        rec = table[key]
        rec[1] += 1
        if v == 0 or len(items) < v:
            continue
        x = _brute_number(bytes(items[v - 1]), which == "last")
        if x is None:
            continue
        numeric += 1
        rec[2] += 1
        rec[3] = (rec[3] + x) % M64
        rec[4] = min(rec[4], x)
        rec[5] = max(rec[5], x)
    return len(per), keyed, numeric, [table[key] for key in order]


def test_brute_number_is_text_rules_number():
    for item in (b"", b"abc", b"7", b"007", b"a12b345", b"3.14", b"18446744073709551615",
                 b"18446744073709551616", b"x18446744073709551616y5", b"0" * 25 + b"7", b"9 " * 4,
                 b"12 99999999999999999999999"):
        for last in (False, True):
            assert _brute_number(item, last) == TR.number(item, last), (item, last)


@pytest.mark.parametrize("name", DFAS)
def test_rule_equals_the_brute_force(name):
    text = DD._matrix_text(name)
    t = DD._t(name, text)
    seen = set()
    for what in GR.WHATS:
        for k, v in _pairs(t):
            for which in ("first", "last"):
                n_lines, keyed, numeric, rows = _brute(name, text, what, k, v, which)
                got = GR.group(t, what, k, v, which)
                assert got[:4] == (n_lines, keyed, numeric, 0), (what, k, v, which, got[:4])
                first, length, count, stats = got[4:]
                assert len(first) == len(rows) and stats.shape == (4, len(rows))
                assert np.all(np.diff(first.astype(np.int64)) > 0)
                for j, (key, c, n, s, lo, hi) in enumerate(rows):
                    at = int(first[j])
                    assert text[at:at + int(length[j])] == key and text.index(b"\n", at) >= at + len(key)
                    assert (int(count[j]), [int(x) for x in stats[:, j]]) == (c, [n, s, lo, hi]), \
                        (what, k, v, which, j)
                seen.add((keyed, numeric, len(rows)))
    assert len(seen) >= 5, seen


@pytest.mark.parametrize("name", DFAS)
def test_rule_identities(name):
    text = DD._matrix_text(name)
    t = DD._t(name, text)
    for what in GR.WHATS:
        for k, v in _pairs(t):
            got = GR.group(t, what, k, v)
            per = DR.keys(t, what, k)
            n_keyed, n_distinct, _ = DR.emitted(per)
            assert (got[1], len(got[4])) == (n_keyed, n_distinct)
            assert int(got[6].sum()) == got[1] and int(got[7][0].sum()) == got[2] <= got[1]
            # count is dedup_rule.emitted's per-string count: a record of count c begins in a line the
            # window (c, c) marks, and in none the window (c + 1, MAX) marks
            for c in sorted(set(got[6].tolist())):
                _, _, exact = DR.emitted(per, c, c)
                _, _, above = DR.emitted(per, c + 1)
                holds = np.searchsorted(t.offs, got[4][got[6] == c].astype(np.int64), side="right") - 1
                assert holds.tolist() == exact and not set(holds.tolist()) & set(above)
            # without a value the records are the same and no line is numeric
            bare = GR.group(t, what, k, 0)
            assert bare[2] == 0 and all(np.array_equal(a, b) for a, b in zip(bare[4:7], got[4:7]))
            assert np.array_equal(bare[7], np.repeat(TR.empty_stats(0), len(got[4]), axis=1))
    # ... and under MATCH at key 1 they are uniq_text's over the lines' first pieces
    uniq = TR.uniq(t, True, max_per_line=1)
    bare = GR.group(t, "match", 1, 0)
    assert (bare[0], bare[1]) == (uniq[0], uniq[1])
    assert all(np.array_equal(a, b) for a, b in zip(bare[4:7], uniq[3:6]))
    # key == value == piece 1: the groups' statistics merged are sum_text's single slot
    for which in ("first", "last"):
        got = GR.group(t, "match", 1, 1, which)
        want = TR.sum(t, 0, which, max_per_line=1)
        merged = TR.empty_stats(0)
        for j in range(len(got[4])):
            merged = TR.merge_stats(merged, got[7][:, j:j + 1])
        assert (got[0], got[1], got[2]) == want[:3] and np.array_equal(merged, want[3]), (name, which)


@pytest.mark.parametrize("name", DFAS)
def test_matrix_texts_meet_the_floors(name):
    """by the oracle: one configuration of the matrix on this text has at least 20 distinct keys, of
    which some occur once and some more than once, and lines that are numeric, keyed but not
    numeric, and unkeyed - all at once"""
    text = DD._matrix_text(name)
    t = DD._t(name, text)
    full = []
    for what in GR.WHATS:
        for k, v in _pairs(t):
            per = GR.numbers(t, what, k, v)
            recs = GR.records(t, what, k, v)
            once = sum(1 for r in recs.values() if r[2] == 1)
            keyed = sum(1 for p in per if p is not None)
            numeric = sum(1 for p in per if p is not None and p[2] is not None)
            if (len(recs) >= 20 and once > 0 and len(recs) - once > 0 and numeric > 0 and
                    keyed - numeric > 0 and t.n_lines - keyed > 0):
                full.append((what, k, v))
            if k > 2:
                assert keyed == 0, (what, k)        # an index above every line's items
    assert full, name


def test_fuzz_dry_run_meets_the_floors():
    cases, seed = GG.FUZZ_CASES, GG.FUZZ_SEED
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), cases, seed,
                          "groups", "dry"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "fuzz dry" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "kernels: {}" in out.stdout          # no GPU call was made
    row = None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[:3] == ["cover", "groups", "group_text"]:
            row = {k: int(v) for k, v in (kv.split("=") for kv in w[3:])}
    assert row, out.stdout[-1000:]
    n = row["cases"]
    assert n >= int(cases) * 0.9, row                # (a refused create skips a case)
    for key in ("match", "field", "first", "last"):
        assert 4 * row[key] >= n, (key, row)
    assert 4 * row["repeated"] >= n, row             # a key that occurs twice or more
    assert 4 * row["unkeyed"] >= n, row              # an unkeyed line
    assert 5 * row["numeric"] >= n, row              # a numeric line
    assert 5 * row["not_numeric"] >= n, row          # a keyed line that is not numeric
    assert 10 * row["empty_key"] >= n, row           # an empty key
    assert row["no_value"] >= 1 and row["value_first"] >= 2, row
    assert row["chunk"] >= 3 and row["capped"] >= 3 and row["dev"] >= 3, row
