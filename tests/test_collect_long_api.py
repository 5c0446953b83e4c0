"""redgpu_collect_long[_dev] (Red::collect over one long text, chunk-parallel): the C-ABI face
that needs no GPU - the symbols, refused NULL arguments, refused device-less handles.  The
arguments are checked before the handle's device image is looked at, as for the other long-text
verbs (test_match_all_long_api.py)."""
import ctypes as C

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa


def test_collect_long_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_collect_long", "redgpu_collect_long_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "collect_long" in one_amd.__all__
    assert callable(one_amd.collect_long)


def test_collect_long_null_handle_refused():
    lib = _lib.lib()
    cnt = C.c_uint64(7)
    text = b"new york"
    assert lib.redgpu_collect_long(None, text, len(text), 0, 0, C.byref(cnt), None, None,
                                   None) == _lib.EAPI
    assert "null dfa handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_collect_long_dev(None, text, len(text), 0, 0, C.byref(cnt), None, None, None,
                                       None) == _lib.EAPI
    assert "null dfa handle" in lib.redgpu_last_error().decode()
    assert cnt.value == 7


@pytest.mark.parametrize("form", ["host", "dev"])
def test_collect_long_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_collect_long if form == "host" else lib.redgpu_collect_long_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(7)
    res = (C.c_int32 * 4)()
    # NULL count, NULL result with cap > 0, NULL data with len > 0: each refused for its own
    # reason although the handle has no device (the argument checks run first)
    for args, why in (([b"123", 3, 0, 4, None, res, None, None], "null count buffer"),
                      ([b"123", 3, 0, 4, C.byref(cnt), None, None, None], "null result buffer"),
                      ([None, 3, 0, 4, C.byref(cnt), res, None, None], "null data buffer")):
        for chunk in (0, 16):
            args[2] = chunk
            assert f(exe._h, *args, *extra) == _lib.EAPI
            assert why in lib.redgpu_last_error().decode(), (why, lib.redgpu_last_error())
    # several NULL at once are refused as well
    for args in ([b"123", 3, 0, 4, None, None, None, None],
                 [b"123", 3, 0, 4, C.byref(cnt), None, None, None],
                 [None, 3, 0, 4, C.byref(cnt), None, None, None]):
        assert f(exe._h, *args, *extra) == _lib.EAPI
    # ... and with nothing NULL, for the missing device
    assert f(exe._h, b"123", 3, 0, 4, C.byref(cnt), res, None, None, *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # NULL result is fine when cap == 0, NULL data when len == 0: the refusal is then the device's
    assert f(exe._h, b"123", 3, 0, 0, C.byref(cnt), None, None, None, *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, None, 0, 0, 0, C.byref(cnt), None, None, None, *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert cnt.value == 7


@pytest.mark.parametrize("form", ["host", "dev"])
def test_collect_long_limits_refused_before_the_device(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_collect_long if form == "host" else lib.redgpu_collect_long_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(0)
    # (nothing is read: the refusals come from the lengths alone)
    assert f(exe._h, b"123", 1 << 40, 0, 0, C.byref(cnt), None, None, None, *extra) == _lib.ELIMIT
    assert "text too large" in lib.redgpu_last_error().decode()
    assert f(exe._h, b"123", 1 << 31, 1, 0, C.byref(cnt), None, None, None, *extra) == _lib.ELIMIT
    assert "too many chunks" in lib.redgpu_last_error().decode()


def test_collect_long_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_long(exe, b"abc 123 def", cap=4)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_long(exe, b"", cap=0, chunk_bytes=16)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_long(exe, b"123", cap=-1)
    lib = _lib.lib()
    cnt = C.c_uint64(0)
    res = (C.c_int32 * 4)()
    assert lib.redgpu_collect_long(exe._h, b"123", 3, 16, 4, C.byref(cnt), res, None,
                                   None) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
