"""redgpu_tally_text[_dev] / redgpu_tally_lds_bins (how many lines, or matches, of a raw text
report each result): the C-ABI face that needs no GPU - the symbols, refused arguments with the
caller's memory untouched, refused device-less handles, the LDS rule as a host function."""
import ctypes as C

import numpy as np
import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"
SENT = 0x5555555555555555
K_TALLY_LDS_BINS = 4096          # k_tally_text.h: kTallyLdsBins


def _args(what=1, style=1, data=TEXT, n_bins=3, accumulate=0, n_lines=None, n_items=None, bins=None):
    """(what, style, do_leader, data, len, delim, n_bins, accumulate, n_lines, n_items, bins)"""
    return [what, style, 1, data, len(TEXT), 0x0A, n_bins, accumulate, n_lines, n_items, bins]


def _outs():
    return C.c_uint64(7), C.c_uint64(7), (C.c_uint64 * 6)(*([SENT] * 6))


def _untouched(nl, ni, bins):
    assert nl.value == 7 and ni.value == 7 and list(bins) == [SENT] * 6


def test_tally_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_tally_text", "redgpu_tally_text_dev", "redgpu_tally_lds_bins"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "tally_text" in one_amd.__all__
    assert callable(one_amd.tally_text)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_tally_text_null_handle_refused(form):
    lib = _lib.lib()
    f = lib.redgpu_tally_text if form == "host" else lib.redgpu_tally_text_dev
    extra = [] if form == "host" else [None]
    nl, ni, bins = _outs()
    for acc in (0, 1):
        rc = f(None, *_args(accumulate=acc, n_lines=C.byref(nl), n_items=C.byref(ni), bins=bins),
               *extra)
        assert rc == _lib.EAPI
        assert "handle" in lib.redgpu_last_error().decode()
    _untouched(nl, ni, bins)
    assert lib.redgpu_tally_lds_bins(None) == 0


@pytest.mark.parametrize("form", ["host", "dev"])
def test_tally_text_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_tally_text if form == "host" else lib.redgpu_tally_text_dev
    extra = [] if form == "host" else [None]
    nl, ni, bins = _outs()
    out = dict(n_lines=C.byref(nl), n_items=C.byref(ni))
    err = lambda: lib.redgpu_last_error().decode()  # noqa: E731
    # each refused for its own reason: the argument checks run before the handle's device is
    # looked at
    assert f(exe._h, *_args(bins=None, **out), *extra) == _lib.EAPI
    assert "bins" in err(), err()
    assert f(exe._h, *_args(data=None, bins=bins, **out), *extra) == _lib.EAPI
    assert "null data" in err(), err()
    for what in (2, -1, 7):
        assert f(exe._h, *_args(what=what, bins=bins, **out), *extra) == _lib.EAPI
        assert "what" in err(), err()
    # a style that does not exist: LINES mode alone looks at it
    for style in (0, 6):
        assert f(exe._h, *_args(what=0, style=style, bins=bins, **out), *extra) == _lib.EEXEC
        assert "style" in err(), err()
        assert f(exe._h, *_args(what=1, style=style, bins=bins, **out), *extra) == _lib.EAPI
        assert "device" in err(), err()
    assert f(exe._h, *_args(n_bins=(1 << 31) + 1, bins=bins, **out), *extra) == _lib.ELIMIT
    assert "n_bins" in err(), err()
    # ... and with nothing wrong, for the missing device; the optional outputs NULL is no fault
    for what in (0, 1):
        for acc in (0, 1):
            assert f(exe._h, *_args(what=what, accumulate=acc, bins=bins, **out), *extra) == _lib.EAPI
            assert "device" in err(), err()
            assert f(exe._h, *_args(what=what, accumulate=acc, bins=bins), *extra) == _lib.EAPI
            assert "device" in err(), err()
    assert f(exe._h, *_args(n_bins=0, bins=bins, **out), *extra) == _lib.EAPI
    assert "device" in err(), err()
    _untouched(nl, ni, bins)


def test_tally_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    into = np.full(exe.info["max_result"] + 2, 9, dtype=np.uint64)
    for kw in ({}, {"matches": False}, {"n_bins": 0}, {"delim": b";"}, {"into": into}):
        with pytest.raises(one_amd.RedExceptApi):
            one_amd.tally_text(exe, TEXT, **kw)
        with pytest.raises(one_amd.RedExceptApi):
            one_amd.tally_text(exe, b"", **kw)
    assert (into == 9).all()
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.tally_text(exe, TEXT, into=np.zeros(3, dtype=np.int64))      # not uint64
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.tally_text(exe, TEXT, 5, into=np.zeros(5, dtype=np.uint64))  # not n_bins + 1
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.tally_text(exe, TEXT, -1)


@pytest.mark.parametrize("name", ["num3", "log100", "uri", "syn256"])
def test_tally_lds_bins_is_a_host_function(name):
    """valid without a device; at most kTallyLdsBins, a multiple of 4, the same from call to call;
    a small table leaves room for all of them"""
    lib = _lib.lib()
    exe = one_amd.Executable(load_dfa(name), device="none")
    got = lib.redgpu_tally_lds_bins(exe._h)
    assert 0 <= got <= K_TALLY_LDS_BINS and got % 4 == 0
    assert lib.redgpu_tally_lds_bins(exe._h) == got
    if name == "num3":      # (a table of a few hundred bytes)
        assert exe.info["table_bytes"] <= 4096 and got == K_TALLY_LDS_BINS, (name, got)
