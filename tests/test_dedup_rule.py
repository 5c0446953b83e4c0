"""tests/dedup_rule.py (dedup_text's rule over a text_rules.Text) needs no GPU to be held to account:
it equals a brute force written from the header's words alone - a loop and a dict over keys that
come from the per-verb oracles of the extract_text, fields_text and grep_text modules, not from
text_rules - on log100, num3 and uri in all four modes; the header's identities hold; and the fuzz
that uses it cannot pass vacuously: scripts/fuzz_gpu.py's `keys` mode, run dry at the case count
and seed of test_gpu_dedup_text's smoke test, meets floors on what the oracle's side held."""
import os
import subprocess
import sys

import numpy as np
import pytest

import one_amd
import oracle as O
import dedup_rule as DR
import text_rules as TR

import test_gpu_collect_text as CT
import test_gpu_dedup_text as DD
import test_gpu_extract_text as XT
import test_gpu_fields_text as FD
import test_gpu_grep_text as GT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFAS = ["log100", "num3", "uri"]
MAX = DR.MAX
SETTINGS = [(1, MAX, False, False), (1, 1, False, True), (2, MAX, True, False), (3, 2, False, True),
            (2, 3, True, True), (1, MAX, True, True)]


def _texts(name):
    """test_gpu_dedup_text's matrix text (lines that repeat) and the module's standard text"""
    return [DD._matrix_text(name), GT._standard(CT.PIECES[name](), n=2 * DR.R.CHUNK + 5)]


def _brute_keys(name, text, what, k, style=1, lead=1):
    """per line the key's bytes or None, from the header's words: the line; the line if search
    selects it; the k-th piece extract_text emits; the k-th of the fields fields_text cuts"""
    lines = O.split_lines_loop(text, 0x0A)
    if what == "whole":
        return list(lines)
    if what == "lines":
        cpu = O.CpuOracle(CT._blob(name))
        return [line if cpu.search(line, style, bool(lead))[0] > 0 else None for line in lines]
    if what == "match":
        per = XT._oracle(name, text).per_line
        return [p[k - 1] if len(p) >= k else None for p in per]
    per = FD._oracle(name, text).per_line()
    return [f[k - 1] if len(f) >= k else None for f in per]


def _brute(text, keys, lo, hi, invert, keep):
    """(n_lines, n_keyed, n_distinct, 0, n_emitted, bytes): a loop with a dict"""
    seen = {}
    for i, key in enumerate(keys):
        if key is not None:
            seen.setdefault(key, [i, 0])[1] += 1
    out, at = [], 0
    for i, key in enumerate(keys):
        end = text.index(b"\n", at) + 1
        if key is None:
            emit = keep
        else:
            first, count = seen[key]
            emit = (first == i and lo <= count <= hi) != invert
        if emit:
            out.append(text[at:end])
        at = end
    keyed = sum(k is not None for k in keys)
    return len(keys), keyed, len(seen), 0, len(out), b"".join(out)


@pytest.mark.parametrize("name", DFAS)
def test_rule_equals_the_brute_force(name):
    outs = set()
    for text in _texts(name):
        t = DD._t(name, text)
        for what, k, style, lead in (("whole", 1, 1, 1), ("lines", 1, 1, 1), ("lines", 1, 4, 0),
                                     ("match", 1, 1, 1), ("match", 2, 1, 1), ("field", 1, 1, 1),
                                     ("field", 2, 1, 1), ("field", 3, 1, 1), ("match", 99, 1, 1)):
            keys = _brute_keys(name, text, what, k, style, lead)
            assert len(keys) == t.n_lines
            # dedup_rule's keys: the same bytes, at an offset inside the line or on its delimiter
            for i, (mine, theirs) in enumerate(zip(DR.keys(t, what, k, style, lead), keys)):
                assert (mine is None) == (theirs is None), (what, k, i)
                if mine is not None:
                    assert mine[1] == theirs and text[mine[0]:mine[0] + len(theirs)] == theirs
                    assert t.offs[i] <= mine[0] and mine[0] + len(theirs) <= t.offs[i + 1] - 1
            for lo, hi, invert, keep in SETTINGS:
                want = _brute(text, keys, lo, hi, invert, keep)
                got = DR.dedup(t, what, k, style, lead, lo, hi, invert, keep)
                assert got == want, (name, what, k, lo, hi, invert, keep, got[:5], want[:5])
                outs.add(got[5])
    assert len(outs) > 30, len(outs)       # (2 texts x 9 keys x 6 settings: many coincide)


@pytest.mark.parametrize("name", DFAS)
def test_rule_identities(name):
    text = DD._matrix_text(name)
    t = DD._t(name, text)
    for what, k in (("whole", 1), ("lines", 1), ("match", 1), ("match", 2), ("field", 1),
                    ("field", 2)):
        plain = DR.dedup(t, what, k)
        later = DR.dedup(t, what, k, invert=True)
        assert plain[4] == plain[2] and later[4] == plain[1] - plain[2]
        # the marked and the later duplicates are all the keyed lines; with the unkeyed, all lines
        both = DR.dedup(t, what, k, keep_unkeyed=True)[4] + later[4]
        assert both == t.n_lines
        assert DR.dedup(t, what, k, min_count=2, max_count=1)[4] == 0
        once, more = DR.dedup(t, what, k, max_count=1), DR.dedup(t, what, k, min_count=2)
        assert once[4] + more[4] == plain[4] and (once[4] > 0 or more[4] > 0 or plain[1] == 0)
    # n_distinct is uniq_text's on the same items, whose first[] fall inside exactly the lines the
    # default setting emits
    for what, uniq in (("match", TR.uniq(t, True, max_per_line=1)), ("lines", TR.uniq(t, False))):
        plain = DR.dedup(t, what)
        assert (plain[1], plain[2]) == (uniq[1], len(uniq[3]))
        _, _, emitted = DR.emitted(DR.keys(t, what))
        holds = (np.searchsorted(t.offs, uniq[3].astype(np.int64), side="right") - 1).tolist()
        assert holds == emitted and len(emitted) > 0


def test_whole_is_lines_under_a_dfa_that_selects_every_line():
    # num3 over a text whose every line holds a number: search selects them all
    text = b"".join(b"%d line %d\n" % (i % 7, i % 3) for i in range(500)) + b"9 tail"
    t = DD._t("num3", text)
    assert len(TR.selected(t)) == t.n_lines == 500
    for lo, hi, invert, keep in SETTINGS:
        assert DR.dedup(t, "whole", 1, 1, 1, lo, hi, invert, keep) == \
            DR.dedup(t, "lines", 1, 1, 1, lo, hi, invert, keep)
    assert DR.dedup(t, "whole")[1:5] == (500, 21, 0, 21)


@pytest.mark.parametrize("name", DFAS)
def test_field_is_whole_over_the_cut_column(name):
    """FIELD at key_index emits, line for line, what WHOLE emits over fields(select = that field) of
    the lines that have the field: all of them for field 1, the delimited ones for field 2"""
    text = DD._matrix_text(name)
    t = DD._t(name, text)
    cpu = O.CpuOracle(CT._blob(name))
    for k in (1, 2):
        rows = TR.fields(t, 1 << (k - 1), only_delimited=k > 1)
        have = [i for i, f in enumerate(TR.fields_of(t)) if len(f) >= k]
        assert rows[1] == len(have) > 0
        column = TR.Text(cpu, rows[3])
        assert column.n_lines == len(have)
        for lo, hi, invert, _ in SETTINGS:
            _, _, mine = DR.emitted(DR.keys(t, "field", k), lo, hi, invert)
            _, _, theirs = DR.emitted(DR.keys(column, "whole"), lo, hi, invert)
            assert mine == [have[j] for j in theirs], (name, k, lo, hi, invert)


def test_no_dfa_selects_an_empty_line():
    """The issue's trap "an empty selected line under LINES" needs a DFA whose search selects the
    empty line.  None does: over every golden DFA and over random ones whose states nearly all
    accept, under every style and leader setting, search over no bytes reports no match - so
    test_gpu_dedup_text.py runs the empty lines as unkeyed under LINES.  If this ever fails, such
    a DFA exists and that trap has to be built with it."""
    import glob
    from golden_util import load_dfa
    from oracle.reda_writer import random_dfa
    blobs = {os.path.basename(p)[:-5]: load_dfa(os.path.basename(p)[:-5])
             for p in glob.glob(os.path.join(ROOT, "tests", "golden", "dfas", "*.reda"))}
    assert len(blobs) >= 9
    for seed in range(1, 41):
        blobs["rnd%d" % seed] = random_dfa(17, 7, seed, dead_frac=0.05, accept_frac=0.9)
    selecting = []
    for name, blob in blobs.items():
        cpu = O.CpuOracle(blob)
        for style in range(1, 6):
            for lead in (False, True):
                if cpu.search(b"", style, lead)[0] > 0:
                    selecting.append((name, style, lead))
    assert not selecting, selecting


def test_fuzz_dry_run_meets_the_floors():
    cases, seed = DD.FUZZ_CASES, DD.FUZZ_SEED
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), cases, seed,
                          "keys", "dry"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "fuzz dry" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "kernels: {}" in out.stdout          # no GPU call was made
    row = None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[:3] == ["cover", "keys", "dedup_text"]:
            row = {k: int(v) for k, v in (kv.split("=") for kv in w[3:])}
    assert row, out.stdout[-1000:]
    n = row["cases"]
    assert n >= int(cases) * 0.9, row                # (a refused create skips a case)
    for what in DR.WHATS:
        assert 10 * row[what] >= n, (what, row)
    assert 2 * row["repeated"] >= n, row             # a string that occurs twice or more
    assert 4 * row["unkeyed"] >= n, row              # an unkeyed line
    assert 4 * row["window"] >= n, row               # a count window that changes the output
    assert 10 * row["empty_key"] >= n, row           # an empty key
    assert row["chunk"] >= 3 and row["truncated"] >= 3, row
