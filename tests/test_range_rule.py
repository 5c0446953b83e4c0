"""range_text's rule as tests/range_rule.py states it, without a GPU: against the local sed's
/A/,/B/ address ranges on a few hundred random small texts, and the rule's own properties on the
same texts."""
import random
import shutil
import subprocess

import pytest

import range_rule as R

A, B = 1, 2


def _texts(n=300, seed=7):
    """lists of lines marked A, B or neither (the marks are the only capitals), as values and as a
    text that ends in a delimiter"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        count = rng.randrange(0, 40)
        density = rng.choice([0.1, 0.3, 0.6, 1.0])
        values, lines = [], []
        for i in range(count):
            v = rng.choice([A, B]) if rng.random() < density else 0
            values.append(v)
            lines.append("line %d %s x" % (i, {0: "-", A: "A", B: "B"}[v]))
        out.append((values, "".join(x + "\n" for x in lines)))
    return out


TEXTS = _texts()


def _cut(text, emit):
    lines = text.split("\n")[:-1]
    assert len(lines) == len(emit)
    return "".join(x + "\n" for x, e in zip(lines, emit) if e)


def _sed(args, text):
    return subprocess.run(["sed"] + args, input=text.encode(), capture_output=True,
                          check=True).stdout.decode()


@pytest.mark.skipif(shutil.which("sed") is None, reason="no sed on this machine")
def test_the_rule_is_seds():
    ranges = toggles = 0
    for values, text in TEXTS:
        emit, rec, n = R.rule(values, A, B)
        assert _sed(["-n", "/A/,/B/p"], text) == _cut(text, emit)
        assert _sed(["/A/,/B/d"], text) == _cut(text, R.rule(values, A, B, invert=True)[0])
        ranges += n
        # one pattern that toggles: every marked line is an event
        both = [1 if v else 0 for v in values]
        emit, rec, n = R.rule(both, 1)
        assert _sed(["-n", "/[AB]/,/[AB]/p"], text) == _cut(text, emit)
        toggles += n
    assert ranges > 300 and toggles > 300


def test_the_rule_on_a_text_by_hand():
    #         0  1  2  3  4  5  6  7  8  9
    values = [B, A, 0, A, B, B, A, B, 0, A]
    emit, rec, n = R.rule(values, A, B)
    assert rec == [(1, 4), (6, 7), (9, 9)] and n == 3
    assert emit == [False, True, True, True, True, False, True, True, False, True]
    assert R.kinds(values, A, B)[0] == [R.OUTSIDE, R.OPEN, R.BODY, R.BODY, R.CLOSE, R.OUTSIDE,
                                        R.OPEN, R.CLOSE, R.OUTSIDE, R.OPEN]
    # the toggle form: an open line is never also the close line
    emit, rec, n = R.rule([1, 1, 0, 1, 0, 1, 1], 1)
    assert rec == [(0, 1), (3, 5), (6, 6)]
    assert R.rule([], A, B) == ([], [], 0)


def test_the_rules_own_properties():
    cut = 0
    for values, text in TEXTS:
        for o, c in ((A, B), (A, A)):
            emit, rec, n = R.rule(values, o, c)
            # invert is the exact complement, whatever the flags
            for eo in (False, True):
                for ec in (False, True):
                    plain = R.rule(values, o, c, eo, ec)[0]
                    other = R.rule(values, o, c, eo, ec, invert=True)[0]
                    assert [not e for e in plain] == other
            # records are disjoint and ascending, and they cover the emitted lines exactly
            assert all(f <= l for f, l in rec)
            assert all(rec[k][1] < rec[k + 1][0] for k in range(len(rec) - 1))
            covered = [any(f <= i <= l for f, l in rec) for i in range(len(values))]
            assert covered == emit
            # without the two flags: exactly the lines strictly inside the records - but the last
            # line of a range nothing closes is a body line
            bare = R.rule(values, o, c, False, False)[0]
            kind = R.kinds(values, o, c)[0]
            inside = [any(f < i < l or (f < i == l and kind[i] == R.BODY) for f, l in rec)
                      for i in range(len(values))]
            assert bare == inside
            assert R.rule(values, o, c, False, False)[1] == rec
            # max_ranges = k keeps the first k records, and their lines alone
            for k in (0, 1, 2, n, n + 3):
                e2, rec2, n2 = R.rule(values, o, c, max_ranges=k)
                assert rec2 == rec[:k] and n2 == min(n, k)
                assert e2 == [any(f <= i <= l for f, l in rec[:k]) for i in range(len(values))]
                cut += k < n
    assert cut > 300
