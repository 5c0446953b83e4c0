"""redgpu_sum_text[_dev] / redgpu_sum_lds_bins (per result the count, sum, min and max of the numbers
in a raw text's matches): the C-ABI face that needs no GPU - the symbols, refused arguments with the
caller's memory untouched, refused device-less handles, the LDS rule as a host function - and the
number rule of the GPU module's expectation helper on hand-written pieces: the yardstick itself."""
import ctypes as C

import numpy as np
import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

import test_gpu_sum_text as ST

TEXT = b"123 45\nabc\n45\n"
SENT = 0x5555555555555555
K_SUM_LDS_BINS = 512             # k_sum_text.h: kSumLdsBins
WORDS = 4 * 4 + 4                # stats of n_bins = 3, and four words behind them


def _args(which=0, data=TEXT, per=1 << 62, n_bins=3, accumulate=0, n_lines=None, n_items=None,
          n_numeric=None, stats=None):
    """(which, data, len, delim, max_per_line, n_bins, accumulate, n_lines, n_items, n_numeric, stats)"""
    return [which, data, len(TEXT), 0x0A, per, n_bins, accumulate, n_lines, n_items, n_numeric, stats]


def _outs():
    return (C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), (C.c_uint64 * WORDS)(*([SENT] * WORDS)))


def _untouched(nl, ni, nn, stats):
    assert nl.value == 7 and ni.value == 7 and nn.value == 7 and list(stats) == [SENT] * WORDS


def test_sum_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_sum_text", "redgpu_sum_text_dev", "redgpu_sum_lds_bins"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "sum_text" in one_amd.__all__
    assert callable(one_amd.sum_text)
    assert (one_amd.SUM_FIRST, one_amd.SUM_LAST) == (0, 1)
    assert (one_amd.SUM_COUNT, one_amd.SUM_SUM, one_amd.SUM_MIN, one_amd.SUM_MAX) == (0, 1, 2, 3)
    for name in ("SUM_FIRST", "SUM_LAST", "SUM_COUNT", "SUM_SUM", "SUM_MIN", "SUM_MAX"):
        assert name in one_amd.__all__, name


@pytest.mark.parametrize("form", ["host", "dev"])
def test_sum_text_null_handle_refused(form):
    lib = _lib.lib()
    f = lib.redgpu_sum_text if form == "host" else lib.redgpu_sum_text_dev
    extra = [] if form == "host" else [None]
    nl, ni, nn, stats = _outs()
    for acc in (0, 1):
        rc = f(None, *_args(accumulate=acc, n_lines=C.byref(nl), n_items=C.byref(ni),
                            n_numeric=C.byref(nn), stats=stats), *extra)
        assert rc == _lib.EAPI
        assert "handle" in lib.redgpu_last_error().decode()
    _untouched(nl, ni, nn, stats)
    assert lib.redgpu_sum_lds_bins(None) == 0


@pytest.mark.parametrize("form", ["host", "dev"])
def test_sum_text_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_sum_text if form == "host" else lib.redgpu_sum_text_dev
    extra = [] if form == "host" else [None]
    nl, ni, nn, stats = _outs()
    out = dict(n_lines=C.byref(nl), n_items=C.byref(ni), n_numeric=C.byref(nn))
    err = lambda: lib.redgpu_last_error().decode()  # noqa: E731
    # each refused for its own reason: the argument checks run before the handle's device is
    # looked at
    assert f(exe._h, *_args(stats=None, **out), *extra) == _lib.EAPI
    assert "stats" in err(), err()
    assert f(exe._h, *_args(data=None, stats=stats, **out), *extra) == _lib.EAPI
    assert "null data" in err(), err()
    for which in (2, -1):
        assert f(exe._h, *_args(which=which, stats=stats, **out), *extra) == _lib.EAPI
        assert "which" in err(), err()
    assert f(exe._h, *_args(n_bins=(1 << 31) + 1, stats=stats, **out), *extra) == _lib.ELIMIT
    assert "n_bins" in err(), err()
    # ... and with nothing wrong, for the missing device; the optional outputs NULL is no fault
    for which in (0, 1):
        for acc in (0, 1):
            for per in (1 << 62, 1, 0):
                a = dict(which=which, accumulate=acc, per=per, stats=stats)
                assert f(exe._h, *_args(**a, **out), *extra) == _lib.EAPI
                assert "device" in err(), err()
                assert f(exe._h, *_args(**a), *extra) == _lib.EAPI
                assert "device" in err(), err()
    assert f(exe._h, *_args(n_bins=0, stats=stats, **out), *extra) == _lib.EAPI
    assert "device" in err(), err()
    _untouched(nl, ni, nn, stats)


def test_sum_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    into = np.full((4, exe.info["max_result"] + 2), 9, dtype=np.uint64)
    for kw in ({}, {"which": "last"}, {"n_bins": 0}, {"delim": b";"}, {"max_per_line": 1},
               {"into": into}):
        with pytest.raises(one_amd.RedExceptApi):
            one_amd.sum_text(exe, TEXT, **kw)
        with pytest.raises(one_amd.RedExceptApi):
            one_amd.sum_text(exe, b"", **kw)
    assert (into == 9).all()
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, 2, into=np.zeros((4, 3), dtype=np.int64))     # not uint64
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, 5, into=np.zeros((4, 5), dtype=np.uint64))    # not n_bins + 1
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, 2, into=np.zeros(12, dtype=np.uint64))        # not (4, .)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, -1)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, max_per_line=-1)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.sum_text(exe, TEXT, which="middle")


@pytest.mark.parametrize("name", ["num3", "log100", "uri", "syn256", "err", "aab"])
def test_sum_lds_bins_is_a_host_function(name):
    """valid without a device; between 8 and kSumLdsBins for the fixture DFAs, a multiple of 4, the
    same from call to call; a small table leaves room for all of them"""
    lib = _lib.lib()
    exe = one_amd.Executable(load_dfa(name), device="none")
    got = lib.redgpu_sum_lds_bins(exe._h)
    assert 8 <= got <= K_SUM_LDS_BINS and got % 4 == 0, (name, got)
    assert lib.redgpu_sum_lds_bins(exe._h) == got
    # the same 16 KiB at most that tally_text's counters take: 32 bytes a slot against 4
    assert got == min(K_SUM_LDS_BINS, (lib.redgpu_tally_lds_bins(exe._h) // 8) & ~3) or \
        lib.redgpu_tally_lds_bins(exe._h) == 4096
    if name == "num3":      # (a table of a few hundred bytes)
        assert exe.info["table_bytes"] <= 4096 and got == K_SUM_LDS_BINS, (name, got)


# the number rule, on the helper alone -------------------------------------------------------------

RULE = [
    (b"t12x345", 12, 345),
    (b"abc", None, None),
    (b"18446744073709551615", 2 ** 64 - 1, 2 ** 64 - 1),
    (b"18446744073709551616", None, None),
    (b"0" * 26 + b"42", 42, 42),
    (b"9" * 30, None, None),
    (b"-5", 5, 5),
    (b"3.14", 3, 14),
    (b"7a", 7, 7),
    (b"", None, None),
    (b"x 18446744073709551616 7", None, 7),
    (b"1,000", 1, 0),
]


@pytest.mark.parametrize("piece,first,last", RULE)
def test_number_rule_of_the_expectation(piece, first, last):
    assert ST._number(piece, False) == first
    assert ST._number(piece, True) == last


def test_reduction_of_the_expectation():
    """count, sum modulo 2^64, min, max per slot; the cut slots merge into the last; items without
    a number are in no statistic"""
    items = [(1, b"a9"), (1, b"18446744073709551615"), (2, b"x"), (3, b"5 6"), (1, b"2"),
             (5, b"18446744073709551616"), (7, b"4")]
    st = ST._reduce(items, 4, False)
    assert st.dtype == np.uint64 and st.shape == (4, 5)
    assert st[:, 1].tolist() == [3, (9 + 2 ** 64 - 1 + 2) % 2 ** 64, 2, 2 ** 64 - 1]
    assert st[:, 2].tolist() == [0, 0, 2 ** 64 - 1, 0] == st[:, 0].tolist()
    assert st[:, 3].tolist() == [1, 5, 5, 5] and st[:, 4].tolist() == [1, 4, 4, 4]
    assert ST._reduce(items, 4, True)[:, 3].tolist() == [1, 6, 6, 6]
    one = ST._reduce(items, 0, False)
    assert one.shape == (4, 1) and one[:, 0].tolist() == [5, (9 + 2 ** 64 - 1 + 2 + 5 + 4) % 2 ** 64,
                                                          2, 2 ** 64 - 1]
    # the merge accumulate performs
    both = ST._merge(st, st)
    assert both[:, 1].tolist() == [6, (2 * (9 + 2 ** 64 - 1 + 2)) % 2 ** 64, 2, 2 ** 64 - 1]
    assert both[:, 2].tolist() == [0, 0, 2 ** 64 - 1, 0]
