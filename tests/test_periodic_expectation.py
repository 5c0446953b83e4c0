"""periodic_text's expansions, proven against the plain oracle - without a GPU.

For every verb and parameter set that tests/test_gpu_text_past_4gib.py runs (periodic_text.CASES and
UNIQ_CASES) the answer of lead + block * 3 + tail, expanded to K blocks, equals what the SAME
oracle class gives when it runs directly over block * K + tail: every count, every record, every
output byte - at K = 5 and at K = 6, which together show that MIDDLE does not depend on K.  Then the
tails' own promises (strings that the block does not hold, no delimiter at the end), the device
slicing of Expansion run against its numpy form through a stand-in for torch-on-the-device (the
CPU), and the arithmetic helpers."""
import numpy as np
import pytest

import periodic_text as PT

KS = (5, 6)


@pytest.mark.parametrize("case", PT.CASES, ids=PT.case_id)
def test_expansion_equals_the_direct_oracle(case):
    lay = PT.layout(case[1], case[2])
    assert lay.P == PT.N and lay.P % 16 and lay.L > 300 and lay.tail_lines == 17
    short = PT.answer(case, lay.short())
    for K in KS:
        want = PT.whole(PT.answer(case, lay.text(K))).host()
        got = PT.expand(short, lay, K).host()
        assert got.keys() == want.keys()
        for key in want:
            assert got[key] == want[key], (case, K, key)
    # not vacuous: the block's share repeats, and the tail adds something of its own
    x = PT.expand(short, lay, 5)
    for e in list(x.rows.values()) + [s for k, s in x.streams.items() if k == "out"]:
        assert all(len(p) > 0 for p in e.parts[:3]), (case, [len(p) for p in e.parts])
    assert x.counts["n_lines"] == lay.n_lines(5)


def test_expansion_with_a_lead_in_front():
    """whole lines in front of block 0 belong to HEAD: the same proof with a lead"""
    lead = b"one line\n\nand a third\n"
    for case in (PT.cases_of("grep")[1], PT.cases_of("filter")[3], PT.cases_of("replace")[0],
                 PT.cases_of("route")[1]):
        lay = PT.layout(case[1], case[2]).with_lead(lead)
        short = PT.answer(case, lay.short())
        for K in KS:
            assert PT.expand(short, lay, K).host() == PT.whole(PT.answer(case, lay.text(K))).host(), (
                case, K)


@pytest.mark.parametrize("case", PT.UNIQ_CASES, ids=PT.case_id)
def test_uniq_expansion_equals_the_direct_oracle(case):
    import test_gpu_uniq_text as UT
    kind, name, matches, m = case
    lay = PT.layout(kind, name)
    items, n_lines = PT.uniq_items(name, lay.short(), matches, m=m)
    assert n_lines == lay.n_lines(3)
    for K in KS:
        text = lay.text(K)
        direct = UT._Expect(*PT.uniq_items(name, text, matches, m=m), text)
        n_items, first, length, count = PT.uniq_expand(items, lay, K)
        assert n_items == direct.n_items
        for g, w in zip((first, length, count), direct.arrays()):
            assert np.array_equal(g.astype(np.uint64), w), (case, K)
        # the tail's strings are records of their own, behind every block
        own = first >= lay.length(K) - len(lay.tail)
        assert own.sum() >= 3 and (count[~own] >= K).all(), (case, K, int(own.sum()))


@pytest.mark.parametrize("name", ["err", "log100", "uri", "num3", "ws", "comma"])
def test_tails(name):
    kind = "planted" if name in ("ws", "comma") else "standard"
    lay = PT.layout(kind, name)
    tail = lay.tail
    assert tail[-1] != PT.DELIM and lay.tail_lines == 17
    lines = tail.split(b"\n")
    for row in lines[:-1]:
        assert row + b"\n" not in lay.block          # no line of the tail is a line of the block
    if name in ("log100", "uri", "num3"):
        # what the DFA matches in the tail stands nowhere in the block
        x = PT.expand(PT.collect_answer(name, lay.short()), lay, 3)
        at = x.rows["start"].tail_index()
        # (uri is suffix-closed: its piece is what extract_text emits, from the line's begin on)
        s = x.rows["begin" if name == "uri" else "start"].numpy()[at:]
        e = x.rows["end"].numpy()[at:]
        assert len(s) >= 17
        short = lay.short()
        for a, b in zip(s, e):
            assert short[int(a):int(b)] not in lay.block, short[int(a):int(b)]
        # whatever the tail's phase: a match of one of its lines straddles a 16-byte boundary
        for phase in range(16):
            assert any((int(a) + phase) // 16 != (int(b) - 1 + phase) // 16 for a, b in zip(s, e))


def test_expansion_slices_equal_its_numpy_form(monkeypatch):
    """slice_dev / same_dev on the CPU device, with slices far smaller than the arrays"""
    import torch
    monkeypatch.setattr(PT, "SLICE", 4096)
    rng = np.random.default_rng(3)
    for shift, dtype in ((0, np.uint8), (65541, np.uint64), (648, np.uint64), (0, np.int32)):
        parts = [rng.integers(0, 200, n).astype(dtype) for n in (700, 333, 333, 41)]
        x = PT.Expansion(parts, 9, shift)
        want = x.numpy()
        assert len(want) == len(x) == 700 + 7 * 333 + 333 + 41
        full = torch.from_numpy(want.astype(np.int64) if dtype == np.uint64 else want.copy())
        x.same_dev(full)
        x.same_dev(full, upto=1500)
        for a, b in ((0, 0), (0, len(x)), (650, 1100), (1033, 1034), (2900, len(x))):
            assert np.array_equal(x.slice_dev(a, b, "cpu").numpy(), full.numpy()[a:b])
        for i in (0, 699, 700, 1032, 1033, 3030, 3031, 3363, 3364, len(x) - 1):
            assert x.at(i) == int(want[i])
            bad = full.clone()
            bad[i] += 1
            with pytest.raises(AssertionError):
                x.same_dev(bad)
        x.same_dev(bad, upto=len(x) - 1)


def test_prefix_through_and_line_at():
    lay = PT.layout("standard", "log100").with_lead(b"a\nbb\n")
    K = 6
    text = lay.text(K)
    rng = np.random.default_rng(4)
    sizes3 = rng.integers(0, 9, lay.n_lines(3))
    # a per-line quantity that is periodic: the short text's, expanded
    c = lay.line_cuts()
    long_sizes = np.concatenate([sizes3[:c[0]]] + [sizes3[c[0]:c[1]]] * (K - 2) + [sizes3[c[1]:]])
    assert len(long_sizes) == lay.n_lines(K)
    for line in (0, 1, 2, c[0] - 1, c[0], c[0] + 5, c[0] + 4 * lay.L - 1, c[0] + 4 * lay.L,
                 c[0] + 5 * lay.L - 1, c[0] + 5 * lay.L, lay.n_lines(K) - 1):
        assert PT.prefix_through(sizes3, lay, K, line) == int(long_sizes[:line + 1].sum()), line
    for pos in (5, 6, len(lay.lead) + lay.P - 1, len(lay.lead) + lay.P, len(lay.lead) + 3 * lay.P + 777):
        line, begin, finish = lay.line_at(K, pos)
        assert begin <= pos <= finish and text[finish] == PT.DELIM
        assert (begin == 0 or text[begin - 1] == PT.DELIM) and PT.DELIM not in text[begin:finish]
        assert text[:begin].count(b"\n") == line


@pytest.mark.parametrize("kind,name", [("standard", "log100"), ("dense", "err"), ("planted", "ws"),
                                       ("standard", "num3")])
def test_lead_puts_a_match_across_the_boundary(kind, name):
    lay0 = PT.layout(kind, name)
    spans = PT.block_spans(name, lay0.block)
    assert len(spans) >= 100
    for boundary in (1 << 32, 3 * lay0.P + 1, 2 * lay0.P + 40000):
        lay = lay0.with_lead(PT.lead_for(lay0, boundary, spans))
        assert len(lay.lead) < 2048 and PT.straddles(lay, boundary, spans)
        if boundary < (1 << 32):        # ... and in the text itself
            text = lay.text(5)
            x = PT.whole(PT.collect_answer(name, text)) if name != "ws" else None
            if x is not None:
                s, e = x.rows["start"].numpy(), x.rows["end"].numpy()
                assert ((s < boundary) & (e > boundary)).sum() == 1
    x = PT.expected(PT.cases_of("grep")[0], 7)
    begin = x.rows["begin"]
    want = begin.numpy()
    for v in (0, 1, int(want[5]), int(want[5]) + 1, 3 * lay0.P, int(want[-1]), int(want[-1]) + 1):
        assert PT.first_at_least(begin, v) == int(np.searchsorted(want, v, "left"))


def test_filter_max_count_is_a_prefix_of_the_unbounded_output():
    import test_gpu_filter_text as FT
    for case in PT.cases_of("filter"):
        _, kind, name, invert, before, after = case
        lay = PT.layout(kind, name)
        for K in KS:
            x = PT.expand(PT.answer(case, lay.short()), lay, K)
            text = lay.text(K)
            n = int(x.counts["n_selected"])
            for mx in (1, 2, n // 3, n // 2 + 1, n - 1, n):
                d = FT._expect(name, text, PT.INSTANT, 1, invert, before, after, max_count=mx)
                assert d.n_selected == mx
                emitted, out_len = PT.filter_first(x, mx)
                assert (emitted, out_len) == (d.n_emitted, len(d.out)), (case, K, mx)
                assert x.streams["out"].numpy()[:out_len].tobytes() == d.out, (case, K, mx)


def test_fields_into_uniq_expansion():
    """fields_text's expanded output is a periodic text of its own: uniq_text over it"""
    import test_gpu_fields_text as FL
    import test_gpu_uniq_text as UT
    case = PT.cases_of("fields")[-1]
    assert case[3:] == ("2-", False, b" | ")
    lay = PT.layout(case[1], case[2])
    short = PT.answer(case, lay.short())
    for K in KS:
        out = PT.expand(short, lay, K).streams["out"]
        olay, oK = PT.stream_layout(out)
        assert oK == K - 2 and olay.text(oK) == out.numpy().tobytes()
        direct_out = FL._oracle(case[2], lay.text(K)).out(*case[3:4], 0, case[4], case[5])[3]
        assert direct_out == olay.text(oK) and len(direct_out) > lay.length(K)
        items, _ = PT.uniq_items("num3", olay.short(), False)
        direct = UT._Expect(*PT.uniq_items("num3", direct_out, False), direct_out)
        n_items, first, length, count = PT.uniq_expand(items, olay, oK)
        assert n_items == direct.n_items and direct.n > 100
        for g, w in zip((first, length, count), direct.arrays()):
            assert np.array_equal(g.astype(np.uint64), w), K


# the long-text verbs ---------------------------------------------------------------------------------

def test_collect_long_and_replace_long_expansions():
    name = PT.LONG_NAME
    lay = PT.layout("standard", name).with_lead(b"~~~\n~\n")
    # the state argument: every attempt is dead behind its line's delimiter, '\n' is in no match
    assert PT.dies_at_line_ends(name, lay.block)
    assert PT.dies_at_line_ends(name, lay.lead) and PT.dies_at_line_ends(name, lay.tail + b"\n")
    short = PT.collect_long_answer(name, lay.short())
    assert len(short.row_pos) > 3 * 150
    shorts = {(r, mx): PT.replace_long_answer(name, lay.short(), r, mx, lay.byte_cuts())
              for r, mx in PT.LONG_REPLS}
    for K in KS:
        text = lay.text(K)
        assert PT.expand(short, lay, K).host() == PT.whole(PT.collect_long_answer(name, text)).host()
        # ... which are collect_text's per-line ones, and the match in the tail's last piece, that
        # is no line
        per_line = PT.whole(PT.collect_answer(name, text)).rows["end"].numpy().tolist()
        ends = PT.expand(short, lay, K).rows["end"].numpy().tolist()
        assert ends[:-1] == per_line and ends[-1] > lay.length(K) - 30
        for (r, mx), ans in shorts.items():
            direct = PT.replace_long_answer(name, text, r, mx, [PT.ALL] * 3)
            x = PT.expand(ans, lay, K)
            assert x.streams["out"].numpy().tobytes() == direct.streams["out"][0], (r, K)
            assert PT.replaced_count(ans, K) == int(direct.part_counts[0]) > 150 * K
            # max_count: the unbounded output up to the mx-th replacement, then the text
            recs = PT.expand(short, lay, K)
            for m in (1, 200, 450, recs.counts["n_rows"] - 3, recs.counts["n_rows"]):
                want = PT.replace_long_answer(name, text, r, m, [PT.ALL] * 3)
                assert int(want.part_counts[0]) == m
                out_len, cut, rest = PT.replace_long_first(recs, r, m, len(text))
                assert x.streams["out"].numpy()[:cut].tobytes() + text[rest:] == want.streams["out"][0]
                assert out_len == len(want.streams["out"][0])


def test_search_long_expansion():
    name = PT.SEARCH_NAME
    cpu = PT._long_cpu(name)
    block = PT.blank_block(name)
    assert len(block) == PT.N
    tail = PT.SEARCH_TAIL
    for style, lead in PT.SEARCH_SETTINGS:
        assert tuple(cpu.search(block * 2, style, bool(lead))) == (0, 0, 0)
        alone = tuple(int(v) for v in cpu.search(tail, style, bool(lead)))
        assert alone[0] > 0 and alone[2] > alone[1] > 0, (style, lead, alone)
        for K in (1, 3, 5):
            got = tuple(int(v) for v in cpu.search(block * K + tail, style, bool(lead)))
            assert got == (alone[0], alone[1] + K * PT.N, alone[2] + K * PT.N), (style, lead, K)


def test_match_all_long_expansion():
    name = "newyork"
    block, tail = PT.newyork_block(), PT.NEWYORK_TAIL
    lay = PT.Layout(block + b"\n", tail)
    # the state argument: the walk never dies, and it enters every block in the same state
    s0 = PT.state_after(name, b"")
    s = [PT.state_after(name, lay.block * k) for k in (1, 2, 3)]
    assert s[0] == s[1] == s[2] and not PT.dies_at_line_ends(name, b"New\n")
    for lead in (0, 1):
        short = PT.match_all_long_answer(name, lay.short(), lead)
        assert len(short.row_pos) > 3 * 100
        for K in KS:
            direct = PT.whole(PT.match_all_long_answer(name, lay.text(K), lead))
            assert PT.expand(short, lay, K).host() == direct.host(), (lead, K)
    assert s0 is not None
