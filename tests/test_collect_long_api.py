"""redgpu_collect_long[_dev] (Red::collect over one long text, chunk-parallel): the C-ABI face
that needs no GPU - the symbols, refused NULL arguments, refused device-less handles."""
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


def test_collect_long_null_handle_refused():
    lib = _lib.lib()
    cnt = C.c_uint64(7)
    text = b"new york"
    assert lib.redgpu_collect_long(None, text, len(text), 0, 0, C.byref(cnt), None, None,
                                   None) == _lib.EAPI
    assert lib.redgpu_collect_long_dev(None, text, len(text), 0, 0, C.byref(cnt), None, None,
                                       None, None) == _lib.EAPI
    assert cnt.value == 7


@pytest.mark.parametrize("form", ["host", "dev"])
def test_collect_long_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_collect_long if form == "host" else lib.redgpu_collect_long_dev
    extra = [] if form == "host" else [None]
    cnt = C.c_uint64(0)
    # NULL count, NULL result with cap > 0, NULL data with len > 0
    for args in ([b"123", 3, 0, 4, None, None, None, None],
                 [b"123", 3, 0, 4, C.byref(cnt), None, None, None],
                 [None, 3, 0, 4, C.byref(cnt), None, None, None]):
        assert f(exe._h, *args, *extra) == _lib.EAPI


def test_collect_long_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_long(exe, b"abc 123 def", cap=4)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.collect_long(exe, b"", cap=0, chunk_bytes=16)
    lib = _lib.lib()
    cnt = C.c_uint64(0)
    res = (C.c_int32 * 4)()
    assert lib.redgpu_collect_long(exe._h, b"123", 3, 16, 4, C.byref(cnt), res, None,
                                   None) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
