"""redgpu_replace_long[_dev] (replaceCore over one long text, chunk-parallel): the C-ABI face
that needs no GPU - the symbols, refused NULL arguments and styles, refused device-less handles,
the C++ mirror."""
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
    return (("host", lib.redgpu_replace_long, []), ("dev", lib.redgpu_replace_long_dev, [None]))


def test_replace_long_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_replace_long", "redgpu_replace_long_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "replace_long" in one_amd.__all__
    assert callable(one_amd.replace_long)


def test_replace_long_null_handle_refused():
    cnt, olen = C.c_uint64(7), C.c_uint64(9)
    text = b"new york"
    for _, f, extra in _forms():
        assert f(None, one_amd.styLast, 1, text, len(text), 0, b"x", 1, 1, C.byref(cnt),
                 C.byref(olen), None, 0, *extra) == _lib.EAPI
    assert (cnt.value, olen.value) == (7, 9)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_replace_long_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    cnt, olen = C.c_uint64(0), C.c_uint64(0)
    sty = one_amd.styLast
    # NULL count, NULL out_len, NULL data with len > 0, NULL repl with repl_len > 0
    for args, what in (([b"123", 3, 0, b"x", 1, 1, None, C.byref(olen), None, 0], "count"),
                       ([b"123", 3, 0, b"x", 1, 1, C.byref(cnt), None, None, 0], "out_len"),
                       ([None, 3, 0, b"x", 1, 1, C.byref(cnt), C.byref(olen), None, 0], "data"),
                       ([b"123", 3, 0, None, 1, 1, C.byref(cnt), C.byref(olen), None, 0],
                        "replacement")):
        assert f(exe._h, sty, 1, *args, *extra) == _lib.EAPI, what
        assert what in lib.redgpu_last_error().decode(), what


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("style", [0, 6, -1, 99])
def test_replace_long_bad_style_refused(form, style):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    cnt, olen = C.c_uint64(0), C.c_uint64(0)
    assert f(exe._h, style, 1, b"123", 3, 0, b"x", 1, 1, C.byref(cnt), C.byref(olen), None, 0,
             *extra) == _lib.EEXEC


@pytest.mark.parametrize("form", ["host", "dev"])
def test_replace_long_limits(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    f, extra = {k: (fn, ex) for k, fn, ex in _forms()}[form]
    cnt, olen = C.c_uint64(0), C.c_uint64(0)
    # (nothing is read before the limits are checked)
    assert f(exe._h, one_amd.styLast, 1, b"123", 1 << 40, 0, b"x", 1, 1, C.byref(cnt),
             C.byref(olen), None, 0, *extra) == _lib.ELIMIT
    assert f(exe._h, one_amd.styLast, 1, b"123", 1 << 39, 16, b"x", 1, 1, C.byref(cnt),
             C.byref(olen), None, 0, *extra) == _lib.ELIMIT


def test_replace_long_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_long(exe, b"abc 123 def", b"#")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.replace_long(exe, b"", b"", one_amd.styFirst, False, 0, chunk_bytes=16)
    lib = _lib.lib()
    cnt, olen = C.c_uint64(0), C.c_uint64(0)
    out = (C.c_uint8 * 8)()
    for _, f, extra in _forms():
        assert f(exe._h, one_amd.styLast, 1, b"123", 3, 16, b"x", 1, 1, C.byref(cnt),
                 C.byref(olen), out, 8, *extra) == _lib.EAPI
        assert "device" in lib.redgpu_last_error().decode()


def test_replace_long_hpp_mirror_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "redgpu.hpp"\n'
                  "size_t f(const redgpu::Executable &e, std::string &o) {\n"
                  '  return redgpu::replaceLong(e, "a 123 b", "#", o, 1, redgpu::styLast); }\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
