"""redgpu_search_long[_dev] (searchCore over one long text, chunk-parallel): the C-ABI face that
needs no GPU - the symbols, refused NULL arguments and styles, refused device-less handles, the
C++ mirror."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _forms():
    lib = _lib.lib()
    return (("host", lib.redgpu_search_long, []), ("dev", lib.redgpu_search_long_dev, [None]))


def _outs():
    return C.c_int32(7), C.c_uint64(8), C.c_uint64(9)


def _untouched(res, st, en):
    return (res.value, st.value, en.value) == (7, 8, 9)


def test_search_long_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_search_long", "redgpu_search_long_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "search_long" in one_amd.__all__
    assert callable(one_amd.search_long)


def test_search_long_null_handle_refused():
    res, st, en = _outs()
    text = b"new york"
    for _, f, extra in _forms():
        assert f(None, one_amd.styLast, 1, text, len(text), 0, C.byref(res), C.byref(st),
                 C.byref(en), *extra) == _lib.EAPI
        assert "handle" in _lib.lib().redgpu_last_error().decode()
    assert _untouched(res, st, en)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_search_long_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    res, st, en = _outs()
    sty = one_amd.styLast
    # NULL result, NULL data with len > 0
    for args, what in (([b"123", 3, 0, None, C.byref(st), C.byref(en)], "result"),
                       ([None, 3, 0, C.byref(res), C.byref(st), C.byref(en)], "data")):
        assert f(exe._h, sty, 1, *args, *extra) == _lib.EAPI, what
        assert what in lib.redgpu_last_error().decode(), what
    assert _untouched(res, st, en)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("style", [0, 6, -1, 99])
def test_search_long_bad_style_refused(form, style):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    res, st, en = _outs()
    assert f(exe._h, style, 1, b"123", 3, 0, C.byref(res), C.byref(st), C.byref(en),
             *extra) == _lib.EEXEC
    assert _untouched(res, st, en)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_search_long_limits(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    res, st, en = _outs()
    # (nothing is read before the limits are checked)
    assert f(exe._h, one_amd.styLast, 1, b"123", 1 << 40, 0, C.byref(res), C.byref(st),
             C.byref(en), *extra) == _lib.ELIMIT
    assert f(exe._h, one_amd.styLast, 1, b"123", 1 << 39, 16, C.byref(res), C.byref(st),
             C.byref(en), *extra) == _lib.ELIMIT
    assert _untouched(res, st, en)


def test_search_long_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.search_long(exe, b"abc 123 def")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.search_long(exe, b"", one_amd.styFirst, False, chunk_bytes=16)
    lib = _lib.lib()
    res, st, en = _outs()
    for _, f, extra in _forms():
        assert f(exe._h, one_amd.styLast, 1, b"123", 3, 16, C.byref(res), C.byref(st),
                 C.byref(en), *extra) == _lib.EAPI
        assert "device" in lib.redgpu_last_error().decode()
        # start and end are optional: still the handle that is refused
        assert f(exe._h, one_amd.styLast, 1, b"123", 3, 16, C.byref(res), None, None,
                 *extra) == _lib.EAPI
        assert "device" in lib.redgpu_last_error().decode()
    assert _untouched(res, st, en)


def test_search_long_hpp_mirror_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "redgpu.hpp"\n'
                  "redgpu::Outcome f(const redgpu::Executable &e) {\n"
                  '  redgpu::Outcome a = redgpu::searchLong(e, "a 123 b", redgpu::styLast);\n'
                  '  redgpu::Outcome b = redgpu::searchLong<redgpu::styFirst, false>(e, "a 123 b");\n'
                  "  return a == b ? a : b; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
