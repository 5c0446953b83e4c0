"""redgpu_collect_text[_dev] (every match of every line of a raw text, as compact records): the
C-ABI face that needs no GPU - the symbols, refused NULL arguments, refused device-less handles."""
import ctypes as C

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"


def _args(data=TEXT, n_matches=None, arrays=None, cap=4):
    """(data, len, delim, cap, n_lines, n_matches, five arrays)"""
    a = arrays or [None] * 5
    return [data, len(TEXT), 0x0A, cap, None, n_matches, *a]


def test_collect_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_collect_text", "redgpu_collect_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "collect_text" in one_amd.__all__
    assert callable(one_amd.collect_text)


def test_collect_text_null_handle_refused():
    lib = _lib.lib()
    cnt = C.c_uint64(7)
    assert lib.redgpu_collect_text(None, *_args(n_matches=C.byref(cnt))) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_collect_text_dev(None, *_args(n_matches=C.byref(cnt)), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert cnt.value == 7


@pytest.mark.parametrize("form", ["host", "dev"])
def test_collect_text_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_collect_text if form == "host" else lib.redgpu_collect_text_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(7)
    line = (C.c_uint64 * 4)()
    arrays = [line, None, None, None, None]
    # NULL n_matches, NULL data with len > 0: each refused for its own reason (the argument
    # checks run before the handle's device is looked at)
    assert f(exe._h, *_args(n_matches=None, arrays=arrays), *extra) == _lib.EAPI
    assert "n_matches" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, n_matches=C.byref(cnt), arrays=arrays), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; every array NULL is no fault
    assert f(exe._h, *_args(n_matches=C.byref(cnt), arrays=arrays), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(n_matches=C.byref(cnt), cap=0), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert cnt.value == 7
    assert list(line) == [0, 0, 0, 0]


def test_collect_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_text(exe, TEXT, cap=0)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_text(exe, b"", cap=0)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_text(exe, b"", delim=b";", want_positions=False)
