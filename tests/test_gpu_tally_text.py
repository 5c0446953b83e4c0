"""tally_text (redgpu_tally_text[_dev]): how many lines (search<style,doLeader> per line), or how
many matches (Red::collect per line), of a raw text report each result.  The bins are exact
against np.bincount over what the CPU oracle (and the reference, when it is built) gives for
sampleLines' lines - never against the code under test: all of log100's signatures, the nine DFAs,
every table placement, results on both sides of the LDS boundary, the chunk-border shapes, a hot
bin, a text of more chunks than the grid has waves, accumulate with a 64-bit carry, optional
outputs, the identities with collect_text and grep_text on the GPU, concurrent streams and threads,
and the C++ mirror."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import one_amd
import oracle as O
from oracle import reda_writer
from one_amd import _lib
from one_amd import workloads as W
from golden_util import load_dfa

import test_gpu_collect_text as CT
import test_gpu_grep_text as GT
import test_gpu_list_verbs as LV  # noqa: F401  (the placement rows' DFA factories, through CT._blob)

pytestmark = pytest.mark.gpu

CHUNK = CT.CHUNK
N = CT.N
SENT = 0x5555555555555555
LINES, MATCHES = 0, 1
_u8 = CT._u8


def _items(name, text, matches, style=1, lead=1, delim=0x0A):
    """(n_lines, n_items, the value of every item) from the oracle: the records' results of
    test_gpu_collect_text._Want, or search's result on every line of test_gpu_grep_text._want"""
    if matches:
        w = CT._want(name, text, delim)
        return w.n_lines, w.n, w.result.astype(np.int64)
    GT._want(name, text, style, lead, False, delim)
    offs, r, _, _ = GT._wants[(name, text, style, lead, delim)]
    return len(offs) - 1, int((r > 0).sum()), r.astype(np.int64)


def _bins(values, n_bins):
    """bins[r] for (uint32_t)r < n_bins, everything else in bins[n_bins]"""
    v = np.asarray(values, dtype=np.int64)
    slot = np.where((v >= 0) & (v < n_bins), v, n_bins)
    return np.bincount(slot, minlength=n_bins + 1).astype(np.uint64)


def _dev_text(text, shift=0):
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + len(text)]
    if len(text):
        dev.copy_(torch.from_numpy(_u8(text).copy()))
    return dev


def _check(exe, name, text, n_bins, matches, style=1, lead=1, delim=b"\n", forms=("host", "dev"),
           where=None):
    """both forms of the verb against the oracle's bincount; returns the expected bins"""
    import torch
    n_lines, n_items, values = _items(name, text, matches, style, lead, delim[0])
    want = _bins(values, n_bins)
    assert int(want.sum()) == (n_items if matches else n_lines)
    kw = dict(matches=matches, style=style, do_leader=bool(lead), delim=delim)
    where = (where, name, n_bins, matches, style, lead)
    if "host" in forms:
        got = one_amd.tally_text(exe, text, n_bins, **kw)
        assert one_amd.last_kernel() == "k_tally_text"
        assert got[:2] == (n_lines, n_items), where + (got[:2], n_lines, n_items)
        assert got[2].dtype == np.uint64 and np.array_equal(got[2], want), where
    if "dev" in forms:
        got = one_amd.tally_text(exe, _dev_text(text, 1), n_bins, **kw)
        assert one_amd.last_kernel() == "k_tally_text"
        torch.cuda.synchronize()
        assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int64 for x in got)
        assert got[0].shape == (1,) and got[1].shape == (1,) and got[2].shape == (n_bins + 1,)
        assert (got[0].item(), got[1].item()) == (n_lines, n_items), where
        assert np.array_equal(got[2].cpu().numpy().astype(np.uint64), want), where
    return want


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filler", [0, 200])
def test_tally_text_all_signatures(filler):
    """every one of log100's 100 results, in both modes, under every cut of n_bins"""
    heads = W.log100_heads()
    text = b"".join(b"z" * filler + b"zz " + heads[i % 100] + b"qq " + heads[(7 * i + 3) % 100] * (i % 3)
                    + b"\n" for i in range(300))
    assert (len(text) > 4 * CHUNK) == bool(filler)
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    assert exe.info["max_result"] == 100
    n_lines, n_matches, values = _items(name, text, True)
    assert (n_lines, n_matches) == (300, 600)
    assert np.bincount(values, minlength=101).tolist() == [0] + [6] * 100
    _, n_sel, per_line = _items(name, text, False, 1, 1)
    assert n_sel == 300 and per_line.tolist() == [i % 100 + 1 for i in range(300)]
    for matches in (True, False):
        total = 600 if matches else 300
        full = None
        for n_bins in (101, 100, 51, 1, 0):
            want = _check(exe, name, text, n_bins, matches)
            if full is None:
                full = want
                assert want[101] == 0 and want[0] == 0 and (want[1:101] == total // 100).all()
            # the "everything else" slot takes what is cut, the slots sum to the total
            assert np.array_equal(want[:n_bins], full[:n_bins])
            assert int(want[n_bins]) == int(full[n_bins:].sum()) and int(want.sum()) == total
        # n_bins=None: max_result + 1
        got = one_amd.tally_text(exe, text, matches=matches)
        assert len(got[2]) == 102 and np.array_equal(got[2], full)


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CT.NINE)
def test_tally_text_nine_dfas(name):
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    n_bins = exe.info["max_result"] + 1
    want = _check(exe, name, text, n_bins, True)
    assert int(want.sum()) == CT.TABLE[name][0]
    seen = {}
    for style in (1, 4):
        for lead in (0, 1):
            seen[style, lead] = _check(exe, name, text, n_bins, False, style, lead)
            assert int(seen[style, lead].sum()) == 648 and seen[style, lead][0] > 20
    if name == "newyork":
        # "New York" under instant stops at "New" (1), under last it goes on to the longer pattern (2)
        a, b = seen[1, 1], seen[4, 1]
        assert not np.array_equal(a, b), (a, b)
        assert a[1:].max() > 100 and b[1:].max() > 100 and a[1:].argmax() != b[1:].argmax(), (a, b)


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dfa,opts,info", GT._PLACEMENT_ROWS)
def test_tally_text_under_placement(dfa, opts, info):
    from test_gpu_long_placements import FACTS
    blob = CT._blob(dfa)
    facts = one_amd.Executable(blob, device="none").info
    for k, v in FACTS.get(dfa, {}).items():
        assert facts[k] == v, (dfa, k, facts[k], v)
    exe = one_amd.Executable(blob, **opts)
    got_info = exe.info
    for k, v in info.items():
        assert got_info[k] == v, (dfa, opts, k, got_info[k], v)
    text = GT._placement_text(dfa)
    assert len(text) == N and text[-1] != 0x0A
    n_bins = got_info["max_result"] + 1
    want = _check(exe, dfa, text, n_bins, True, where=opts)
    assert int(want.sum()) >= 50 and want[n_bins] == 0
    for style in (1, 4):
        for lead in (0, 1):
            want = _check(exe, dfa, text, n_bins, False, style, lead, where=opts)
            # not vacuous: lines on both sides
            assert want[0] >= 20 and int(want[1:].sum()) >= 150, (dfa, style, lead, want[0])
    # ... and cut in the middle of the results
    _check(exe, dfa, text, max(1, n_bins // 2), True, forms=("dev",), where=opts)
    _check(exe, dfa, text, 1, False, 4, 1, forms=("dev",), where=opts)


# 4 ---------------------------------------------------------------------------------------------
def _four_letters(results):
    """error, initial, and one accepting state per letter a / b / c / d: every letter is a match of
    its own"""
    equiv = np.full(256, 4, dtype=np.uint8)
    for k, ch in enumerate(b"abcd"):
        equiv[ch] = k
    trans = np.zeros((6, 5), dtype=np.int64)
    trans[1] = [2, 3, 4, 5, 0]
    return reda_writer.write_reda(trans, [0, 0] + list(results), equiv=equiv)


def _letters_text(seed=5):
    a = _u8(b"abcd.")[np.random.default_rng(seed).integers(0, 5, N)].copy()
    a[CT._delims(N, seed)] = 0x0A
    return bytes(a)


def test_tally_text_lds_boundary():
    """results on both sides of redgpu_tally_lds_bins: LDS counters, global counters, and the
    "everything else" slot on either side"""
    lib = _lib.lib()
    probe = one_amd.Executable(_four_letters((1, 2, 3, 4)), device="none")
    L = lib.redgpu_tally_lds_bins(probe._h)
    assert 8 <= L <= 4096
    results = (L - 1, L, L + 1, 70000)
    name = "four_letters_%d" % L
    CT._blobs[name] = _four_letters(results)
    exe = one_amd.Executable(CT._blobs[name])
    assert lib.redgpu_tally_lds_bins(exe._h) == L and exe.info["max_result"] == 70000
    text = _letters_text()
    n_lines, n_matches, values = _items(name, text, True)
    per = np.bincount(values, minlength=70001)
    assert n_lines > 600 and all(per[r] > 10000 for r in results) and int(per.sum()) == n_matches
    for n_bins in (L - 1, L, L + 1, L + 2, 70001):
        for matches in (True, False):
            want = _check(exe, name, text, n_bins, matches)
            if matches:
                assert int(want[n_bins]) == sum(int(per[r]) for r in results if r >= n_bins)


def test_tally_text_sparse_results_up_to_100000():
    name = "rnd300_100000"
    CT._blobs[name] = reda_writer.random_dfa(300, 256, 11, accept_frac=0.2, max_result=100000,
                                             dead_frac=0.05)
    exe = one_amd.Executable(CT._blobs[name])
    text = CT._random_text("random")
    _, n_matches, values = _items(name, text, True)
    distinct = set(values.tolist())
    assert len(distinct) >= 40 and max(distinct) > 90000 and n_matches > 1000, (len(distinct), n_matches)
    for matches in (True, False):
        want = _check(exe, name, text, 100001, matches)
        assert want[100001] == 0


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CT._shapes()))
def test_tally_text_shapes(shape):
    text = CT._shapes()[shape]
    for name in ("aab", "num3"):
        exe = one_amd.Executable(load_dfa(name))
        n_bins = exe.info["max_result"] + 1
        for matches in (True, False):
            want = _check(exe, name, text, n_bins, matches, where=shape)
            if shape in ("no delimiter", "empty", "one byte, no delimiter"):
                assert not want.any()
            elif shape == "a match in the tail":
                short = _items(name, CT.SHORT, matches)
                assert int(want[1:].sum()) == 3 * short[1] > 0   # the tail's are in no line


# 6 ---------------------------------------------------------------------------------------------
def test_tally_text_hot_bin_and_rounds():
    """one chunk and five rounds with uneven counts; every line the same result; 22 matches a line"""
    exe = one_amd.Executable(load_dfa("aab"))
    text = b"".join(b"aab " * (i % 10) + b"\n" for i in range(300))
    assert len(text) < CHUNK
    n_bins = exe.info["max_result"] + 1
    want = _check(exe, "aab", text, n_bins, True)
    assert want[0] == 0 and int(want.sum()) == sum(i % 10 for i in range(300))
    want = _check(exe, "aab", text, n_bins, False)
    assert want[0] == 30 and int(want.sum()) == 300
    # every line matches, all the same result: ONE bin takes every item of every round
    text = b"".join(b"x" * (i % 90) + b" aab\n" for i in range(1200))
    assert len(text) > 3 * CHUNK
    for matches in (True, False):
        for n_bins in (2, 1, 0):
            want = _check(exe, "aab", text, n_bins, matches)
            assert int(want.max()) == 1200 == int(want.sum())
    exe = one_amd.Executable(load_dfa("num3"))
    line = b"123 4567 89012 " * 7 + b"345\n"
    text = line * (N // len(line)) + b"12 tail"
    n_bins = exe.info["max_result"] + 1
    want = _check(exe, "num3", text, n_bins, True)
    assert int(want.sum()) >= 20 * (N // len(line))
    _check(exe, "num3", text, n_bins, False, 4, 0)


# 7 ---------------------------------------------------------------------------------------------
def test_tally_text_above_the_grid():
    """160 MiB = 10,240 chunks against at most CUs x 2 workgroups of 16 waves: every wave takes
    further chunks, a workgroup's LDS counters live across all of them and are flushed once.
    Everything stays on the device: a 1 MiB block that ends in a delimiter, tiled."""
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    props = torch.cuda.get_device_properties(0)
    block_len, tiles = 1 << 20, 160
    assert tiles * (block_len // CHUNK) > props.multi_processor_count * 2 * 16
    block = CT._dense(CT.PIECES[name](), seed=3, n=block_len, end_in_delim=True)
    dev = torch.from_numpy(_u8(block).copy()).cuda().repeat(tiles)
    n_bins = exe.info["max_result"] + 1
    for matches in (True, False):
        n_lines, n_items, values = _items(name, block, matches)
        assert n_items > 1000
        got = one_amd.tally_text(exe, dev, n_bins, matches=matches)
        assert one_amd.last_kernel() == "k_tally_text"
        assert (got[0].item(), got[1].item()) == (n_lines * tiles, n_items * tiles)
        assert np.array_equal(got[2].cpu().numpy().astype(np.uint64),
                              _bins(values, n_bins) * np.uint64(tiles))


# 8 ---------------------------------------------------------------------------------------------
def _raw(exe, form, what, data, n_bins, accumulate, bins, *, n_lines=True, n_items=True,
         style=1, lead=1, delim=0x0A, at=0):
    """redgpu_tally_text / _dev through ctypes: bins is a numpy uint64 array (host) or an int64
    CUDA tensor (dev), the slots from `at` on are the call's; returns (n_lines, n_items)"""
    import torch
    lib = _lib.lib()
    if form == "host":
        nl, ni = C.c_uint64(SENT), C.c_uint64(SENT)
        rc = lib.redgpu_tally_text(exe._h, what, style, lead, data, len(data), delim, n_bins,
                                   accumulate, C.byref(nl) if n_lines else None,
                                   C.byref(ni) if n_items else None, bins.ctypes.data + 8 * at)
        assert rc == 0, lib.redgpu_last_error()
        return nl.value, ni.value
    cnt = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    rc = lib.redgpu_tally_text_dev(exe._h, what, style, lead,
                                   data.data_ptr() if data.numel() else None, data.numel(), delim,
                                   n_bins, accumulate, cnt.data_ptr() if n_lines else None,
                                   cnt.data_ptr() + 8 if n_items else None,
                                   bins.data_ptr() + 8 * at,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.redgpu_last_error()
    torch.cuda.synchronize()
    return tuple(cnt.tolist())


@pytest.mark.parametrize("form,shift", [("host", 0), ("dev", 0), ("dev", 1), ("dev", 7), ("dev", 15)])
def test_tally_text_accumulate(form, shift):
    """two texts into one array: added under accumulate (with a 64-bit carry), overwritten
    without; the slots around the call's n_bins + 1 stay as they were"""
    import torch
    name = "log100"
    exe = one_amd.Executable(load_dfa(name))
    texts = [CT._dense(CT.PIECES[name](), seed=s) for s in (1, 2)]
    n_bins, at, room = 101, 3, 120
    for what in (MATCHES, LINES):
        items = [_items(name, t, what == MATCHES) for t in texts]
        wants = [_bins(v, n_bins) for _, _, v in items]
        assert wants[0][8] > 50 and not np.array_equal(wants[0], wants[1])
        start = np.full(room, SENT, dtype=np.uint64)
        start[at + 8] = 2 ** 32 - 1          # the carry out of the low word must show
        start[at + 5] = 0
        data = [t if form == "host" else _dev_text(t, shift) for t in texts]
        bins = start.copy() if form == "host" else torch.from_numpy(start.view(np.int64).copy()).cuda()
        host = lambda: bins if form == "host" else bins.cpu().numpy().view(np.uint64)  # noqa: E731
        expect = start.copy()
        for k in (0, 1):
            got = _raw(exe, form, what, data[k], n_bins, 1, bins, at=at)
            assert got == items[k][:2], (what, k)
            expect[at:at + n_bins + 1] += wants[k]
            assert np.array_equal(host(), expect), (what, k)
        assert int(expect[at + 8]) == 2 ** 32 - 1 + int(wants[0][8]) + int(wants[1][8]) > 2 ** 32
        # accumulate = 0 overwrites all n_bins + 1 slots, sentinels included, and nothing else
        assert _raw(exe, form, what, data[1], n_bins, 0, bins, at=at) == items[1][:2]
        expect[at:at + n_bins + 1] = wants[1]
        assert np.array_equal(host(), expect) and (expect[:at] == SENT).all()
        assert (expect[at + n_bins + 1:] == SENT).all()
    # the verb's into=
    into = None
    for t, d in zip(texts, data):
        if form == "host":
            into = one_amd.tally_text(exe, t, n_bins, into=into)[2]
        else:
            into = one_amd.tally_text(exe, d, n_bins, into=into)[2]
    got = into if form == "host" else into.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, sum(_bins(_items(name, t, True)[2], n_bins) for t in texts))


# 9 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [b";", b"\x00"])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_tally_text_optional_outputs_null(form, delim):
    import torch
    name = "err"
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]()).replace(b"\n", delim)
    n_bins = 2
    data = text if form == "host" else _dev_text(text)
    for what in (MATCHES, LINES):
        n_lines, n_items, values = _items(name, text, what == MATCHES, delim=delim[0])
        assert n_lines >= 648 and n_items > 100
        for keep_lines, keep_items in ((True, False), (False, True), (False, False)):
            bins = np.full(n_bins + 1, SENT, dtype=np.uint64)
            if form == "dev":
                bins = torch.from_numpy(bins.view(np.int64).copy()).cuda()
            got = _raw(exe, form, what, data, n_bins, 0, bins, n_lines=keep_lines,
                       n_items=keep_items, delim=delim[0])
            assert got == (n_lines if keep_lines else SENT, n_items if keep_items else SENT)
            out = bins if form == "host" else bins.cpu().numpy().view(np.uint64)
            assert np.array_equal(out, _bins(values, n_bins)), (what, keep_lines, keep_items)
    # ... and with '\n' the same text has no line at all
    assert one_amd.tally_text(exe, text, n_bins)[:2] == (0, 0)


def test_tally_text_empty_and_lineless_on_the_device():
    """the _dev form writes the zero counts and zeroes the bins on the stream - or leaves them
    alone under accumulate"""
    import torch
    exe = one_amd.Executable(load_dfa("aab"))
    for text in (b"", b"aab, and no line end"):
        dev = torch.from_numpy(_u8(text).copy()).cuda()
        for what in (MATCHES, LINES):
            bins = torch.full((6,), 77, dtype=torch.int64, device="cuda")
            assert _raw(exe, "dev", what, dev, 3, 1, bins, at=1) == (0, 0)
            assert bins.tolist() == [77] * 6
            assert _raw(exe, "dev", what, dev, 3, 0, bins, at=1) == (0, 0)
            assert bins.tolist() == [77, 0, 0, 0, 0, 77]
            assert one_amd.last_kernel() == "k_tally_text"


# 10 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["num3", "log100", "set5"])
def test_tally_text_identities_on_the_gpu(name):
    exe = one_amd.Executable(load_dfa(name))
    text = CT._dense(CT.PIECES[name]())
    n_bins = exe.info["max_result"] + 1
    rec = one_amd.collect_text(exe, text)
    got = one_amd.tally_text(exe, text, n_bins)
    assert got[:2] == rec[:2] and rec[1] > 500
    assert np.array_equal(got[2], np.bincount(rec[4], minlength=n_bins + 1).astype(np.uint64))
    for style in (1, 4):
        for lead in (False, True):
            sel = one_amd.grep_text(exe, text, style, lead, cap=0)
            got = one_amd.tally_text(exe, text, n_bins, matches=False, style=style, do_leader=lead)
            assert got[:2] == sel[:2] and int(got[2][1:].sum()) == sel[1] > 100
            assert int(got[2].sum()) == sel[0]


# 11 --------------------------------------------------------------------------------------------
def test_tally_text_two_streams_and_threads():
    import torch
    names = ("num3", "err")
    exes = [one_amd.Executable(load_dfa(n)) for n in names]
    texts = [CT._dense(CT.PIECES[n](), seed=2 + k) for k, n in enumerate(names)]
    n_bins = [e.info["max_result"] + 1 for e in exes]
    wants = [(_items(n, t, True)[:2], _bins(_items(n, t, True)[2], nb))
             for n, t, nb in zip(names, texts, n_bins)]
    assert wants[0][0] != wants[1][0]
    streams = [torch.cuda.Stream() for _ in texts]
    devs = [torch.from_numpy(_u8(t).copy()).cuda() for t in texts]
    torch.cuda.synchronize()

    def same(got, want):
        assert (int(got[0]), int(got[1])) == want[0]
        g = got[2].cpu().numpy() if isinstance(got[2], torch.Tensor) else got[2]
        assert np.array_equal(g.astype(np.uint64), want[1])

    outs = []
    for st, exe, d, nb in zip(streams, exes, devs, n_bins):
        with torch.cuda.stream(st):
            outs.append(one_amd.tally_text(exe, d, nb))
    torch.cuda.synchronize()
    for got, w in zip(outs, wants):
        same(got, w)
    errors = []

    def work(exe, t, d, st, nb, w):
        # each thread on its own stream, with bins of its own: the device form, the host form beside it
        try:
            for _ in range(3):
                with torch.cuda.stream(st):
                    got = one_amd.tally_text(exe, d, nb)
                    st.synchronize()
                same(got, w)
                same(one_amd.tally_text(exe, t, nb), w)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    th = [threading.Thread(target=work, args=a) for a in zip(exes, texts, devs, streams, n_bins, wants)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# 12 --------------------------------------------------------------------------------------------
def test_tally_text_cpp_mirror(tmp_path):
    """redgpu::tallyText (include/redgpu.hpp) compiled with g++"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "tally_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "tally_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    name = "newyork"
    text = CT._dense(CT.PIECES[name]())
    path = tmp_path / "text.bin"
    path.write_bytes(text)
    dfa = os.path.join(root, "tests", "golden", "dfas", name + ".reda")
    for n_bins in (3, 1):
        out = subprocess.run([prog, dfa, str(path), str(n_bins)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = {r.split()[0]: [int(v) for v in r.split()[1:]] for r in out.stdout.split("\n") if r}
        m = _bins(_items(name, text, True)[2], n_bins).tolist()
        assert rows["matches"] == m and rows["default"] == m and sum(m) > 100
        assert rows["instant"] == _bins(_items(name, text, False, 1, 1)[2], n_bins).tolist()
        assert rows["last"] == _bins(_items(name, text, False, 4, 0)[2], n_bins).tolist()
        if n_bins == 3:
            assert rows["instant"] != rows["last"]
