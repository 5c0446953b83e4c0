"""redgpu_match_all_long[_dev] (matchAll over one long text, chunk-parallel): the C-ABI face
that needs no GPU - the symbols, refused NULL arguments, refused device-less handles."""
import ctypes as C

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa


def test_match_all_long_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_match_all_long", "redgpu_match_all_long_dev",
                 "redgpu_diag_match_all_long_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "match_all_long" in one_amd.__all__
    assert callable(one_amd.match_all_long)


def test_match_all_long_null_handle_refused():
    lib = _lib.lib()
    cnt = C.c_uint64(7)
    text = b"new york"
    assert lib.redgpu_match_all_long(None, 1, text, len(text), 0, 0, C.byref(cnt), None, None,
                                     None) == _lib.EAPI
    assert lib.redgpu_match_all_long_dev(None, 1, text, len(text), 0, 0, C.byref(cnt), None, None,
                                         None, None) == _lib.EAPI
    assert cnt.value == 7


@pytest.mark.parametrize("form", ["host", "dev"])
def test_match_all_long_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_match_all_long if form == "host" else lib.redgpu_match_all_long_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(0)
    res = (C.c_int32 * 4)()
    # NULL count, NULL result with cap > 0, NULL data with len > 0: each refused for its own
    # reason (the argument checks run before the handle's device is looked at)
    for args, why in (([b"123", 3, 0, 4, None, res, None, None], "null count"),
                      ([b"123", 3, 0, 4, C.byref(cnt), None, None, None], "null result"),
                      ([None, 3, 0, 4, C.byref(cnt), res, None, None], "null data")):
        for lead in (0, 1):
            assert f(exe._h, lead, *args, *extra) == _lib.EAPI
            assert why in lib.redgpu_last_error().decode(), (why, lib.redgpu_last_error())
    # ... and with nothing NULL, for the missing device
    assert f(exe._h, 1, b"123", 3, 0, 4, C.byref(cnt), res, None, None, *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # NULL result is fine when cap == 0: the refusal is then the device's
    assert f(exe._h, 1, b"123", 3, 0, 0, C.byref(cnt), None, None, None, *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()


def test_match_all_long_diag_refused_without_a_call():
    lib = _lib.lib()
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    out = (C.c_uint32 * 8)()
    assert lib.redgpu_diag_match_all_long_dev(None, out, None) == _lib.EAPI
    assert lib.redgpu_diag_match_all_long_dev(exe._h, out, None) == _lib.EAPI


def test_match_all_long_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.match_all_long(exe, b"1234567 abc", cap=4)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.match_all_long(exe, b"", cap=0, do_leader=False, chunk_bytes=16)
    lib = _lib.lib()
    cnt = C.c_uint64(0)
    res = (C.c_int32 * 4)()
    assert lib.redgpu_match_all_long(exe._h, 1, b"123", 3, 16, 4, C.byref(cnt), res, None,
                                     None) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_match_all_long_limits_refused_before_the_device(form):
    """as for the other long-text verbs: a text too large or cut into too many chunks is refused
    as such in both forms, before the handle's device image is looked at"""
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_match_all_long if form == "host" else lib.redgpu_match_all_long_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(0)
    # (nothing is read: the refusals come from the lengths alone)
    assert f(exe._h, 1, b"123", 1 << 40, 0, 0, C.byref(cnt), None, None, None,
             *extra) == _lib.ELIMIT
    assert "text too large" in lib.redgpu_last_error().decode()
    assert f(exe._h, 1, b"123", 1 << 31, 1, 0, C.byref(cnt), None, None, None,
             *extra) == _lib.ELIMIT
    assert "too many chunks" in lib.redgpu_last_error().decode()
