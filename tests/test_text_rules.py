"""tests/text_rules.py (the eight newer raw-text verbs' rules over any oracle) needs no GPU to be
held to account.  The new rules are the old ones: for every verb, on the verb's own standard and
dense texts over log100, num3 and the loose-start uri, under parameter settings that change the
output, text_rules' answer equals the answer of the expectation in the verb's tests/test_gpu_<verb>.py
module, byte for byte and count for count.  And the fuzz that uses them cannot pass vacuously:
scripts/fuzz_gpu.py's `lines` and `pieces` modes, run dry at the case count and seed of
test_differential_fuzz_smoke, meet floors on what the oracle's side of their cases held."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import one_amd
import oracle as O
import range_rule
import text_rules as TR

import test_gpu_collect_text as CT
import test_gpu_extract_text as XT
import test_gpu_fields_text as FD
import test_gpu_filter_text as FL
import test_gpu_grep_text as GT
import test_gpu_range_text as RG
import test_gpu_route_text as RT
import test_gpu_sum_text as ST
import test_gpu_tally_text as TT
import test_gpu_uniq_text as UQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFAS = ["log100", "num3", "uri"]
ALL = TR.ALL

_cache = {}


def _texts(name):
    """the standard and the dense text every verb's module is run on"""
    piece = CT.PIECES[name]()
    return [GT._standard(piece), CT._dense(piece)]


def _t(name, text, delim=0x0A):
    key = (name, text, delim)
    if key not in _cache:
        _cache[key] = TR.Text(O.CpuOracle(CT._blob(name)), text, delim)
    return _cache[key]


def _most(name):
    return int(one_amd.Executable(CT._blob(name), device="none").info["max_result"])


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w), k
        else:
            assert not isinstance(g, np.ndarray) and g == w, \
                (k, g if not isinstance(g, bytes) else len(g))


@pytest.mark.parametrize("name", DFAS)
def test_tally_rule_is_the_modules(name):
    full = _most(name) + 1
    for text in _texts(name):
        t = _t(name, text)
        for matches, style, lead, n_bins in ((True, 1, 1, full), (True, 1, 1, 1), (False, 1, 1, full),
                                             (False, 4, 0, full // 2), (False, 5, 1, 0)):
            n_lines, n_items, values = TT._items(name, text, matches, style, lead)
            want = (n_lines, n_items, TT._bins(values, n_bins))
            assert int(want[2].sum()) == (n_items if matches else n_lines) > 0
            _same(TR.tally(t, n_bins, matches, style, lead), want)
            prev = np.arange(n_bins + 1, dtype=np.uint64) * np.uint64(1 << 40)
            _same(TR.tally(t, n_bins, matches, style, lead, into=prev), want[:2] + (prev + want[2],))


@pytest.mark.parametrize("name", DFAS)
def test_filter_rule_is_the_modules(name):
    texts = _texts(name) + ([FL._text(name, 4), FL._text(name, 5)] if name in GT.PIECES else [])
    emitted = set()
    for text in texts:
        t = _t(name, text)
        for style, lead, invert, before, after, mx in ((4, 1, False, 0, 0, ALL), (1, 0, True, 2, 1, ALL),
                                                      (5, 1, False, 1, 3, 7), (2, 1, True, 100000, 0, 1),
                                                      (3, 0, False, 0, 100000, 0)):
            x = FL._expect(name, text, style, lead, invert, before, after, mx)
            _same(TR.filter(t, style, lead, invert, before, after, mx),
                  (x.n_lines, x.n_selected, x.n_emitted, x.out))
            emitted.add(x.n_emitted)
    assert len(emitted) >= 5, emitted


@pytest.mark.parametrize("name", DFAS)
def test_extract_rule_is_the_modules(name):
    for text in _texts(name):
        x = XT._oracle(name, text)
        outs = set()
        for m in (ALL, 1, 2, 0):
            n, out = x.out(m)
            _same(TR.extract(_t(name, text), m), (x.n_lines, n, out))
            outs.add(out)
        assert len(outs) >= (4 if name in CT.OPEN and text is not _texts(name)[0] else 2)
    # the loose start: pieces that begin in front of collect's start, as the module counts them
    if name == "uri":
        loose = [it for it in _t(name, text).items() if it[3] < it[2]]
        assert len(loose) == x.loose > 100


@pytest.mark.parametrize("name", DFAS)
def test_route_rule_is_the_modules(name):
    full = min(_most(name) + 1, 255)
    for text in _texts(name):
        for n_bins, drop, style, lead in ((full, False, 1, 1), (full, True, 4, 0), (1, True, 1, 1),
                                          (0, False, 5, 1), (max(full // 2, 1), False, 2, 0)):
            x = RT._expect(name, text, n_bins, drop, style, lead)
            _same(TR.route(_t(name, text), n_bins, style, lead, drop),
                  (x.n_lines, x.n_routed, x.bin_lines, x.bin_offsets, x.out))
            assert 0 < x.n_routed and (x.n_routed < x.n_lines) == drop


@pytest.mark.parametrize("name", DFAS)
def test_uniq_rule_is_the_modules(name):
    for text in _texts(name):
        for matches, style, lead, m in ((True, 1, 1, ALL), (True, 1, 1, 1), (False, 1, 1, ALL),
                                        (False, 4, 0, ALL), (False, 5, 1, ALL)):
            x = UQ._expect(name, text, matches, style, lead, 0x0A, m)
            got = TR.uniq(_t(name, text), matches, style, lead, m)
            _same(got, (x.n_lines, x.n_items, 0) + x.arrays())
            assert x.n_items > 0 or style == 5


@pytest.mark.parametrize("name", DFAS)
def test_fields_rule_is_the_modules(name):
    written = set()
    for text in _texts(name):
        x = FD._oracle(name, text)
        for fields, max_fields, only, sep in (("1", 0, False, b" "), ("1,3", 0, True, b" "),
                                              ("2-", 2, False, b"<->"), ("64-", 0, False, b""),
                                              ("1,2,64-", 5, True, b"12345678"), ("1-", 1, True, b",")):
            want = x.out(fields, max_fields, only, sep)
            _same(TR.fields(_t(name, text), one_amd.matcher.fields_mask(fields), sep, max_fields, only),
                  want)
            written.add(want[1:3])
    assert len(written) >= 6, written


@pytest.mark.parametrize("name", DFAS)
def test_sum_rule_is_the_modules(name):
    full = _most(name) + 1
    numeric = 0
    for text in _texts(name):
        for n_bins, last, m in ((full, False, ALL), (full, True, ALL), (1, True, 1), (0, False, 2)):
            want = ST._expect(name, text, n_bins, last, m)
            which = "last" if last else "first"
            _same(TR.sum(_t(name, text), n_bins, which, m), want)
            prev = ST._reduce([(1, b"7"), (0, b"x18446744073709551615")], n_bins, False)
            _same(TR.sum(_t(name, text), n_bins, which, m, into=prev),
                  want[:3] + (ST._merge(prev, want[3]),))
            numeric += want[2]
    assert numeric > 1000 or name != "num3"     # (log100's planted head holds no digit)
    for piece in (b"", b"abc", b"12", b"a007b9", b"18446744073709551615", b"18446744073709551616x1",
                  b"1x" + b"9" * 30):
        for last in (False, True):
            assert TR.number(piece, last) == ST._number(piece, last), piece


@pytest.mark.parametrize("name", DFAS)
def test_range_rule_is_the_modules(name):
    texts = _texts(name) + ([RG._border_text()] if name == "log100" else [])
    ranges = 0
    for text in texts:
        t = _t(name, text)
        for style, lead in ((1, 1), (4, 0)):
            v = t.values(style, lead)
            seen = np.bincount(v[v > 0])
            top = [int(r) for r in np.argsort(-seen, kind="stable")[:2] if seen[r]]
            o, c = (RG._border_results() if text is texts[-1] and name == "log100" else
                    (top[0], top[-1]))
            for close, eo, ec, inv, mx, rec_cap in ((None, True, True, False, ALL, 1 << 20),
                                                    (c, False, True, True, 2, 1),
                                                    (c, True, False, False, ALL, 0),
                                                    (o + 1, False, False, True, 0, 5)):
                x = range_rule.expect(name, text, o, close, eo, ec, inv, mx, style, lead)
                got = TR.range(t, o, close, style, lead, eo, ec, inv, mx, rec_cap)
                k = min(x.n_ranges, rec_cap)
                _same(got, (x.n_lines, x.n_ranges, x.n_emitted, x.out) +
                      tuple(r[:k] for r in x.records))
                ranges += x.n_ranges
    assert ranges > 100


# the dry run ----------------------------------------------------------------------------------
WRITERS = {"filter_text", "route_text", "range_text", "extract_text", "fields_text"}
PIECE_VERBS = {"extract_text", "fields_text", "uniq_text", "sum_text"}
VERBS = {"lines": ["tally_text", "filter_text", "route_text", "range_text", "uniq_text"],
         "pieces": ["tally_text", "extract_text", "uniq_text", "sum_text", "fields_text"]}


def _owed(mode, verb):
    """which items of the issue's list belong to a verb of a mode"""
    owed = set()
    if verb in ("tally_text", "route_text", "sum_text"):
        owed.add("overflow")
    if verb in WRITERS:
        owed.add("truncated")
    if verb in ("extract_text", "fields_text"):
        owed.add("piece64")
    if mode == "pieces" and verb in PIECE_VERBS:
        owed.add("loose")
    if verb == "sum_text":
        owed |= {"over64bit", "numeric"}
    if verb == "range_text":
        owed.add("range_border")
    if verb == "filter_text":
        owed.add("merged_border")
    return owed


def _smoke_args():
    """the case count and the seed test_differential_fuzz_smoke hands the script"""
    with open(os.path.join(ROOT, "tests", "test_gpu_parity.py")) as f:
        m = re.search(r'"fuzz_gpu\.py"\), "(\d+)", "(\d+)"\]', f.read())
    return m.group(1), m.group(2)


@pytest.mark.parametrize("mode", ["lines", "pieces"])
def test_fuzz_dry_run_meets_the_floors(mode):
    cases, seed = _smoke_args()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), cases, seed,
                          mode, "dry"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "fuzz dry" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "kernels: {}" in out.stdout          # no GPU call was made
    rows = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[:2] == ["cover", mode]:
            rows[w[2]] = {k: int(v) for k, v in (kv.split("=") for kv in w[3:])}
        elif w[:2] == ["special", mode]:
            special = {k: int(v) for k, v in (kv.split("=") for kv in w[2:])}
    assert list(rows) == VERBS[mode], rows
    for verb, row in rows.items():
        assert row["cases"] >= int(cases) * 0.9, (verb, row)    # (a refused create skips a case)
        assert 2 * row["item"] >= row["cases"], (verb, row)
        assert 4 * row["chunk"] >= row["cases"], (verb, row)
        assert set(row) == {"cases", "item", "chunk"} | _owed(mode, verb), (verb, row)
        for k in _owed(mode, verb):
            assert row[k] >= 3, (verb, k, row)
    assert set(special) == {"empty", "all_delims", "delim0", "no_dead", "acc09"}
    assert all(v >= 2 for v in special.values()), special
