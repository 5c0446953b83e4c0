"""The dispatch, cell by cell: which kernel launchBatch / launchBatches / launchAdvance name for
check_batch, match_batch and match_batch(want_start=False) under styles Last and Full, on every
family of the whole-line walks (k_stream over the fused table, the hot rows and both class-table
forms, k_stream4, k_stream<advance...>, k_fixed, the speculative chunks, k_ragged, k_stream_multi
plain and lean).  one_amd.last_kernel() is compared as an EXACT string - the other GPU tests pin
these names by prefix or suffix at most - and every cell's results against the same call on an
Executable(force_generic=True), the one-line-per-lane kernels.  The DFAs and the forcing options
are those of test_gpu_parity.py's hot-row, class-table, chains and chunking tests.

Wall time on an MI355X, the module run alone: 24 cases in 12.4 s, of which 11.3 s are the process's
first import and use of torch (it lands in test_stream_multi_names, the first case with a device
tensor); every other case takes 0.01 - 0.3 s."""
import numpy as np
import pytest

import one_amd
from golden_util import load_dfa
from oracle.reda_writer import random_dfa
from one_amd import workloads as W

pytestmark = pytest.mark.gpu

LAST, FULL = 4, 5
# (verb, want_start)
CALLS = [("check", False), ("match", True), ("match", False)]
CELLS = [(verb, ws, sty) for verb, ws in CALLS for sty in (LAST, FULL)]

# the name's table-form suffix; "cls_big": a class table above 64 KB, the index form
FORMS = {"fused": "", "hot": ",hot", "cls": ",cls", "cls_big": ",cls"}


def _mode(verb, want_start, style):
    """the StreamMode part of a name: check stores no positions, styFull's end is the line's"""
    start = verb == "match" and want_start
    if style == LAST:
        return "last,start,end" if start else "last,end"
    return "full,start" if start else "full"


_blobs = {}


def _blob(form):
    if form not in _blobs:
        _blobs[form] = (random_dfa(1500, 40, 91, dead_frac=0.0, accept_frac=0.15)
                        if form == "cls_big" else
                        load_dfa({"fused": "syn256", "hot": "uri_v6", "cls": "uri_user"}[form]))
    return _blobs[form]


def _pair(form, **kw):
    """the Executable under test and the per-lane one; the table kind is what the form says"""
    exe = one_amd.Executable(_blob(form), **kw)
    kind = exe.info["table_kind"]
    assert {"fused": kind == 1, "hot": kind == 6, "cls": kind in (2, 3),
            "cls_big": kind == 3 and exe.info["table_bytes"] > 65536}[form], exe.info
    return exe, one_amd.Executable(_blob(form), force_generic=True)


def _fixed(form, n, stride, seed):
    if form in ("fused", "cls_big"):
        return W.fixed_lines(n, stride, seed, alphabet=False)
    plant = W.URI_V6_PLANT if form == "hot" else W.URI_USER_PLANT
    return W.fixed_lines(n, stride, seed, alphabet=True, plant=plant, plant_every=3,
                         plant_at=max(0, stride // 2 - 20))


def _call(exe, verb, want_start, style, data, **where):
    if verb == "check":
        return [one_amd.check_batch(exe, data, style, False, **where)]
    return [x for x in one_amd.match_batch(exe, data, style, False, want_start=want_start, **where)
            if x is not None]


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for a, b in zip(got, exp):
        if hasattr(a, "cpu"):
            a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b), what


def _cells(exe, gen, name_of, data, **where):
    for verb, ws, sty in CELLS:
        got = _call(exe, verb, ws, sty, data, **where)
        k = one_amd.last_kernel()
        assert k == name_of(verb, ws, sty), (verb, ws, sty, k)
        exp = _call(gen, verb, ws, sty, data, **where)
        assert one_amd.last_kernel() == "k_generic"
        _same(got, exp, (verb, ws, sty, k))


@pytest.mark.parametrize("stride,n", [(64, 333), (128, 300)])
@pytest.mark.parametrize("form", list(FORMS))
def test_stream_names(form, stride, n):
    exe, gen = _pair(form)
    _cells(exe, gen, lambda v, ws, s: "k_stream<%s%s>" % (_mode(v, ws, s), FORMS[form]),
           _fixed(form, n, stride, 11 + stride), stride=stride, n=n)


@pytest.mark.parametrize("stride,n", [(64, 333), (128, 300)])
def test_stream4_names(stride, n):
    exe, gen = _pair("fused", force_stream=True, stream_chains=4, no_chunking=True)
    _cells(exe, gen, lambda v, ws, s: "k_stream4<%s>" % _mode(v, ws, s),
           _fixed("fused", n, stride, 12 + stride), stride=stride, n=n)


@pytest.mark.parametrize("form", list(FORMS))
def test_advance_names(form):
    exe, gen = _pair(form)
    n, stride = 333, 64
    data = _fixed(form, n, stride, 13)
    state = np.full(n, one_amd.STATE_INITIAL, dtype=np.uint32)
    gstate = state.copy()
    res = one_amd.advance_batch(exe, data, state, stride=stride, n=n)
    assert one_amd.last_kernel() == "k_stream<advance%s>" % FORMS[form]
    gres = one_amd.advance_batch(gen, data, gstate, stride=stride, n=n)
    assert one_amd.last_kernel() == "k_advance"
    assert np.array_equal(res, gres) and np.array_equal(state, gstate)


def test_fixed_names():
    exe, gen = _pair("fused")
    names = {("check", False): "k_fixed<check>", ("match", True): "k_fixed<match,start>",
             ("match", False): "k_fixed<match>"}
    _cells(exe, gen, lambda v, ws, s: names[v, ws], _fixed("fused", 333, 48, 14), stride=48, n=333)


@pytest.mark.parametrize("form", ["fused", "hot", "cls"])
def test_chunk_names(form):
    exe, gen = _pair(form, force_chunking=True)
    _cells(exe, gen, lambda v, ws, s: "k_stream<chunk%s>+k_chunk" % FORMS[form],
           _fixed(form, 5, 4096, 15), stride=4096, n=5)


@pytest.mark.parametrize("form", list(FORMS))
def test_ragged_names(form):
    exe, gen = _pair(form)
    data, offsets = W.ragged_lines(300, 1, 200, 16, alphabet=form in ("hot", "cls"))
    data = data.copy()
    if form in ("hot", "cls"):
        plant = np.frombuffer(W.URI_V6_PLANT if form == "hot" else W.URI_USER_PLANT, dtype=np.uint8)
        for k in range(0, data.size - 100, 600):
            data[k:k + len(plant)] = plant
    _cells(exe, gen, lambda v, ws, s: "k_ragged<%s%s>" % (_mode(v, ws, s), FORMS[form]),
           data, offsets=offsets)


def _batches_cells(exe, gen, name_of, host, stride, n):
    """two equal batches through the batches entry points, against the per-lane kernels"""
    import torch
    dev = torch.from_numpy(host).cuda()
    for verb, ws, sty in CELLS:
        if verb == "check":
            outs = [[r] for r in one_amd.check_batches(exe, [dev, dev], sty, False, stride=stride)]
        else:
            outs = [[x for x in o if x is not None] for o in
                    one_amd.match_batches(exe, [dev, dev], sty, False, stride=stride,
                                          want_start=ws)]
        k = one_amd.last_kernel()
        assert k == name_of(verb, ws, sty), (verb, ws, sty, k)
        exp = _call(gen, verb, ws, sty, dev, stride=stride, n=n)
        torch.cuda.synchronize()
        for got in outs:
            _same(got, exp, (verb, ws, sty, k))


def test_stream_multi_names():
    # 2 x 137 tiles of 1,024 lines: no fewer than the card has CUs, so the run is ONE launch
    n, stride = 140000, 64
    exe, gen = _pair("fused")
    _batches_cells(exe, gen, lambda v, ws, s: "k_stream_multi<%s>" % _mode(v, ws, s),
                   _fixed("fused", n, stride, 17), stride, n)


def test_stream_multi_lean_names():
    # the lean step is for lines of 512 bytes and more; styFull without start has none, and two
    # batches of so few tiles then run one by one on k_stream
    n, stride = 3000, 512
    exe, gen = _pair("fused", no_chunking=True, force_lean=True)

    def name_of(v, ws, s):
        mode = _mode(v, ws, s)
        return "k_stream<full>" if mode == "full" else "k_stream_multi<%s,lean>" % mode
    _batches_cells(exe, gen, name_of, _fixed("fused", n, stride, 18), stride, n)
