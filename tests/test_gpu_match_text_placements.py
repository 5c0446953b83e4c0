"""match_text and its check form (redgpu_match_text[_dev], redgpu_check_text_dev) under EVERY table
placement: the rows of test_grep_text_under_placement over the same texts (four split chunks and
an unaligned tail), against oracle.split_lines plus the CPU oracle's match / check on the lines
with their delimiters removed - the host form, the device form with room for more and for fewer
lines than the text has, and want_start = want_end = False.  match is anchored, and the dense text
plants its pieces one byte into their lines: log100, num3 and aab (not suffix-closed) also run over
a copy of it with every line-leading piece moved to the line's first byte.

The split leaves the line count on the device (Batch::nDev).  launchBatch hands such a batch to
launchRaggedFamily alone, and redgpu.cpp's textDev reads the count on the host and calls runDev
when that family declines: KERNELS restates, row by row, which of the two happens."""
import numpy as np
import pytest

import one_amd
import oracle as O

import test_gpu_grep_text as GT

pytestmark = pytest.mark.gpu

STYLES = ((1, 0), (4, 0), (4, 1), (5, 0))

# The kernel behind the device form under styLast / styFull without a leader ("*" = the walk's
# mode: last,start,end / last,end / full,start / full), from launchRaggedFamily's three tests, the
# row's asserted info and dfa_image.cpp.  Every test there wants the DFA not to die early
# (early_death = 0) and its pure dead ends to be absorbing, and then
#   k_ragged<*>      table kind 1 of at most 64 KiB and 256 states:
#                      syn256 (65,536 bytes, 256 states, fast_path = 1)
#   k_ragged<*,hot>  table kind 6 with at least one hot row:
#                      uri_user under force_hot and uri_v6 (254 hot rows each)
#   k_ragged<*,cls>  the streaming class table, built for kinds 2 and 3 with at most 127 classes,
#                    of at most 65 KiB: uri_user (25 classes x 342 states x 2 + 256 = 17,356 bytes)
# Every other row takes the host-count fallback, and there launchBatch ends in k_generic: with
# offsets the fixed-stride family declines, k_early wants 16,384 lines (the texts have 648 or
# 5,771), k_style_blocks takes the early-exit styles only, and the ragged family declines again:
#   early_death = 1    log100, num3, aab, rnd270, rnd1500, rnd80k, rnd72 - whatever the placement
#   kind 4             uri_user and uri_v6 under force_global: no class or hot table is built
#   kind 6, n_hot = 0  uri with lds_table_max = 4096: no hot row to stream over
#   kind 2             rnd270nd has 256 classes: no streaming class table
#   kind 1             leaky: its pure dead end has a way out (fast_path = 0)
# styInstant never reaches k_ragged as match (check may: normalizeVerbStyle turns it into styLast
# for a DFA with one result), and a leader the DFA has (num3, aab) keeps styLast away from it too.
KERNELS = {
    "log100-default-kind7": "k_generic",
    "log100-force_hot-kind6": "k_generic",
    "log100-lds_table_max=4096-kind6": "k_generic",
    "log100-force_global-kind4": "k_generic",
    "uri_user-default-kind3": "k_ragged<*,cls>",
    "uri_user-force_hot-kind6": "k_ragged<*,hot>",
    "uri_user-force_global-kind4": "k_generic",
    "uri_v6-default-kind6": "k_ragged<*,hot>",
    "uri_v6-force_global-kind4": "k_generic",
    "uri-lds_table_max=4096-kind6": "k_generic",
    "num3-force_global-kind4": "k_generic",
    "aab-force_global-kind4": "k_generic",
    "rnd270-default-kind2": "k_generic",
    "rnd270-force_hot+lds_table_max=10240-kind6": "k_generic",
    "rnd270-force_global-kind4": "k_generic",
    "rnd270nd-default-kind2": "k_generic",
    "rnd1500-default-kind3": "k_generic",
    "rnd1500-force_hot+lds_table_max=10240-kind6": "k_generic",
    "rnd80k-default-kind5": "k_generic",
    "syn256-default-kind1": "k_ragged<*>",
    "rnd72-default-kind1": "k_generic",
    "leaky-default-kind1": "k_generic",
}
# what KERNELS relies on beside the row's own info
EARLY_DEATH = {"log100": 1, "uri_user": 0, "uri_v6": 0, "uri": 0, "num3": 1, "aab": 1, "rnd270": 1,
               "rnd270nd": 0, "rnd1500": 1, "rnd80k": 1, "syn256": 0, "rnd72": 1, "leaky": 0}
FAST_PATH = {"syn256": 1, "rnd72": 0, "leaky": 0}

_expected = {}


def test_kernel_table_names_every_row():
    assert set(KERNELS) == {p.id for p in GT._PLACEMENT_ROWS}
    assert {k.split("<")[0] for k in KERNELS.values()} == {"k_ragged", "k_generic"}
    assert {k for k in KERNELS.values() if "*" in k} == {"k_ragged<*>", "k_ragged<*,hot>",
                                                        "k_ragged<*,cls>"}


def _kernel(row, style, positions):
    mode = {(4, True): "last,start,end", (4, False): "last,end", (5, True): "full,start",
            (5, False): "full"}[style, positions]
    return KERNELS[row].replace("*", mode)


def _texts_of(dfa):
    """the row's text of test_grep_text_under_placement; for a regex DFA that is not suffix-closed
    also that text with the piece behind a line's first byte moved onto it: lines match starts in"""
    text = GT._placement_text(dfa)
    if dfa not in ("log100", "num3", "aab"):     # (the three uri DFAs are suffix-closed)
        return {"text": text}
    key = ("anchored", dfa)
    if key not in _expected:
        a = np.frombuffer(text, dtype=np.uint8).copy()
        p = np.frombuffer(GT.LP.PIECES[dfa][0], dtype=np.uint8)
        for begin in GT._lines_of(text)[:-1].tolist():
            if bytes(a[begin + 1:begin + 1 + len(p)]) == bytes(p):
                a[begin:begin + len(p)] = p
        assert (a == 0x0A).sum() == text.count(b"\n")
        _expected[key] = bytes(a)
    return {"text": text, "anchored": _expected[key]}


def _expect(dfa, which, text, style, lead):
    """(offsets, n, match's Outcomes, check's results): oracle.split_lines and the oracle on the
    lines with their delimiters removed; the reference too when it is built"""
    key = (dfa, which, style, lead)
    if key not in _expected:
        cpu, ref = GT._orc(dfa)
        a = np.frombuffer(text, dtype=np.uint8)
        offs = O.split_lines(a)
        n = len(offs) - 1
        assert [len(x) for x in O.split_lines_loop(text)] == (np.diff(offs.astype(np.int64)) - 1).tolist()
        keep = a[:int(offs[-1])]
        compact = np.ascontiguousarray(keep[keep != 0x0A])
        coffs = offs - np.arange(n + 1, dtype=np.uint64)
        m = cpu.batch("match", style, lead, compact, offsets=coffs, threads=4)
        c = cpu.batch("check", style, lead, compact, offsets=coffs, threads=4)[0]
        if ref is not None:
            rm = ref.batch("match", style, lead, compact, offsets=coffs, threads=4)
            assert all(np.array_equal(x, y) for x, y in zip(m, rm))
            assert np.array_equal(c, ref.batch("check", style, lead, compact, offsets=coffs, threads=4)[0])
        _expected[key] = (offs, n, m, c)
    return _expected[key]


@pytest.mark.parametrize("dfa,opts,info", GT._PLACEMENT_ROWS)
def test_match_text_under_placement(dfa, opts, info, request):
    import torch
    row = request.node.callspec.id
    blob = GT._blob(dfa)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    assert got_info["early_death"] == EARLY_DEATH[dfa], dfa
    if dfa in FAST_PATH:
        assert got_info["fast_path"] == FAST_PATH[dfa], dfa
    hits = misses = moved = 0
    for which, text in _texts_of(dfa).items():
        dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        for style, lead in STYLES:
            where = (dfa, opts, which, style, lead)
            offs, n, (er, es, ee), ec = _expect(dfa, which, text, style, lead)
            assert n >= 648
            if (style, lead) == (4, 0):
                hits += int((er > 0).sum())
                misses += int((er == 0).sum())
                moved += int((es != 0).sum())
            # the host form, match and check
            goffs, found, r, s, e = one_amd.match_text(exe, text, style, lead)
            assert found == n and np.array_equal(goffs, offs), where
            assert np.array_equal(r, er) and np.array_equal(s, es) and np.array_equal(e, ee), where
            _, found, r, s, e = one_amd.match_text(exe, text, style, lead, want_start=False,
                                                   want_end=False)
            assert found == n and s is None and e is None and np.array_equal(r, ec), where
            # the device form: room for more lines than there are, and for a third of them
            ragged = style != 1 and not (lead and got_info["leader_len"])
            for cap in (n + 7, max(1, n // 3)):
                k = min(n, cap)
                doffs, dcnt, dr, ds, de = one_amd.match_text(exe, dev, style, lead, cap=cap)
                kernel = one_amd.last_kernel()
                torch.cuda.synchronize()
                where = (dfa, opts, which, style, lead, cap, kernel)
                assert int(dcnt.item()) == n, where
                assert np.array_equal(doffs[:k + 1].cpu().numpy().astype(np.uint64), offs[:k + 1]), where
                assert np.array_equal(dr[:k].cpu().numpy(), er[:k]), where
                assert np.array_equal(ds[:k].cpu().numpy().astype(np.uint64), es[:k]), where
                assert np.array_equal(de[:k].cpu().numpy().astype(np.uint64), ee[:k]), where
                if ragged:
                    assert kernel == _kernel(row, style, True), where
                else:
                    assert not kernel.startswith("k_ragged"), where
                doffs, dcnt, cr, cs, ce = one_amd.match_text(exe, dev, style, lead, cap=cap,
                                                             want_start=False, want_end=False)
                kernel = one_amd.last_kernel()
                torch.cuda.synchronize()
                where = (dfa, opts, which, style, lead, cap, kernel, "check")
                assert cs is None and ce is None and int(dcnt.item()) == n, where
                assert np.array_equal(doffs[:k + 1].cpu().numpy().astype(np.uint64), offs[:k + 1]), where
                assert np.array_equal(cr[:k].cpu().numpy(), ec[:k]), where
                if ragged:
                    assert kernel == _kernel(row, style, False), where
    # not vacuous under styLast: lines that match and lines that do not; a start that is not the
    # line's first byte wherever the DFA can give one (a loose start, or an accepting initial state)
    assert hits >= 100 and misses >= 100, (dfa, hits, misses)
    if dfa not in ("log100", "num3", "aab", "rnd80k"):
        assert moved >= 1, (dfa, moved)
