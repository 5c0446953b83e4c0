"""redgpu_replace_text[_dev] (every line of a raw text rewritten, the text put back together): the
C-ABI face that needs no GPU - the symbols, refused NULL arguments, refused device-less handles."""
import ctypes as C

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"
REPL = b"<#>"
SENT = 7


def _args(data=TEXT, repl=REPL, counts=(None, None, None), out=None, out_cap=0, style=4):
    """(style, do_leader, only_changed, data, len, delim, repl, repl_len, max_count, n_lines,
    n_replaced, out_len, out, out_cap)"""
    return [style, 1, 0, data, len(TEXT), 0x0A, repl, len(REPL), 1 << 62, *counts, out, out_cap]


def _counts():
    c = [C.c_uint64(SENT) for _ in range(3)]
    return c, tuple(C.byref(x) for x in c)


def test_replace_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_replace_text", "redgpu_replace_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "replace_text" in one_amd.__all__
    assert callable(one_amd.replace_text)


def test_replace_text_null_handle_refused():
    lib = _lib.lib()
    c, refs = _counts()
    assert lib.redgpu_replace_text(None, *_args(counts=refs)) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_replace_text_dev(None, *_args(counts=refs), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert [x.value for x in c] == [SENT] * 3


@pytest.mark.parametrize("form", ["host", "dev"])
def test_replace_text_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_replace_text if form == "host" else lib.redgpu_replace_text_dev
    extra = [] if form == "host" else [None]
    c, refs = _counts()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    # NULL out_len, NULL data with len > 0, NULL repl with repl_len > 0: each refused for its own
    # reason (the argument checks run before the handle's device is looked at)
    assert f(exe._h, *_args(counts=(refs[0], refs[1], None), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "out_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(repl=None, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "null replacement" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; n_lines / n_replaced / out NULL is no fault
    assert f(exe._h, *_args(counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(counts=(None, None, refs[2])), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # a style that does not exist is no API fault
    assert f(exe._h, *_args(counts=refs, style=9), *extra) == _lib.EEXEC
    assert [x.value for x in c] == [SENT] * 3
    assert list(out) == [SENT] * 32


def test_replace_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_text(exe, TEXT, REPL)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_text(exe, TEXT, b"", max_count=1, only_changed=True)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_text(exe, b"", REPL, delim=b";")
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_text(exe, TEXT, REPL, out_cap=0)
