"""redgpu_extract_text[_dev] (every match of every line of a raw text, as a text): the C-ABI face
that needs no GPU - the symbols, refused NULL arguments, refused device-less handles, and the C++
mirror compiled against include/redgpu.hpp."""
import ctypes as C
import os
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"
SENT = 7


def _args(data=TEXT, length=len(TEXT), counts=(None, None, None), out=None, out_cap=0):
    """(data, len, delim, max_per_line, n_lines, n_matches, out_len, out, out_cap)"""
    return [data, length, 0x0A, 1 << 62, *counts, out, out_cap]


def _counts():
    c = [C.c_uint64(SENT) for _ in range(3)]
    return c, tuple(C.byref(x) for x in c)


def test_extract_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_extract_text", "redgpu_extract_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "extract_text" in one_amd.__all__
    assert callable(one_amd.extract_text)


def test_extract_text_null_handle_refused():
    lib = _lib.lib()
    c, refs = _counts()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    assert lib.redgpu_extract_text(None, *_args(counts=refs, out=out, out_cap=32)) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_extract_text_dev(None, *_args(counts=refs, out=out, out_cap=32), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert [x.value for x in c] == [SENT] * 3
    assert list(out) == [SENT] * 32


@pytest.mark.parametrize("form", ["host", "dev"])
def test_extract_text_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_extract_text if form == "host" else lib.redgpu_extract_text_dev
    extra = [] if form == "host" else [None]
    c, refs = _counts()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    # NULL out_len, NULL data with len > 0: each refused for its own reason (the argument checks run
    # before the handle's device is looked at)
    assert f(exe._h, *_args(counts=refs[:2] + (None,), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "out_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; n_lines / n_matches / out NULL is no
    # fault, nor is a NULL data with len == 0
    assert f(exe._h, *_args(counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(counts=(None, None, refs[2])), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(data=None, length=0, counts=refs), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # a text split refuses is a limit
    assert f(exe._h, *_args(length=1 << 45, counts=refs, out=out, out_cap=32), *extra) == _lib.ELIMIT
    assert [x.value for x in c] == [SENT] * 3
    assert list(out) == [SENT] * 32


def test_extract_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.extract_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.extract_text(exe, TEXT, max_per_line=1)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.extract_text(exe, b"", delim=b";")
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.extract_text(exe, TEXT, out_cap=0)


def test_extract_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/extract_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "extract_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "extract_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
