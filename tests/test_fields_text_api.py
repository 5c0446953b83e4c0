"""redgpu_fields_text[_dev] (awk -F's columns of a raw text, as a text): the C-ABI face that needs
no GPU - the symbols, refused arguments, refused device-less handles, the Python mirror's field
list parser, and the C++ mirror compiled against include/redgpu.hpp."""
import ctypes as C
import os
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"
SENT = 7


def _args(data=TEXT, length=len(TEXT), select=1, sep_len=1, counts=(None, None, None, None),
          out=None, out_cap=0):
    """(data, len, delim, select, max_fields, only_delimited, sep, sep_len, n_lines, n_emitted,
    n_fields, out_len, out, out_cap)"""
    return [data, length, 0x0A, select, 0, 0, 0x20, sep_len, *counts, out, out_cap]


def _counts():
    c = [C.c_uint64(SENT) for _ in range(4)]
    return c, tuple(C.byref(x) for x in c)


def test_fields_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_fields_text", "redgpu_fields_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "fields_text" in one_amd.__all__
    assert callable(one_amd.fields_text)


def test_fields_text_null_handle_refused():
    lib = _lib.lib()
    c, refs = _counts()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    assert lib.redgpu_fields_text(None, *_args(counts=refs, out=out, out_cap=32)) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_fields_text_dev(None, *_args(counts=refs, out=out, out_cap=32), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert [x.value for x in c] == [SENT] * 4
    assert list(out) == [SENT] * 32


@pytest.mark.parametrize("form", ["host", "dev"])
def test_fields_text_bad_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_fields_text if form == "host" else lib.redgpu_fields_text_dev
    extra = [] if form == "host" else [None]
    c, refs = _counts()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    # NULL out_len, NULL data with len > 0, no field selected, a sep of nine bytes: each refused for
    # its own reason (the argument checks run before the handle's device is looked at)
    assert f(exe._h, *_args(counts=refs[:3] + (None,), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "out_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(select=0, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "select" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(sep_len=9, counts=refs, out=out, out_cap=32), *extra) == _lib.EAPI
    assert "sep_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; the three other counts / out NULL is no
    # fault, nor is a NULL data with len == 0, a sep of 0 or 8 bytes, or bit 63 of select
    for ok in (_args(counts=refs, out=out, out_cap=32), _args(counts=(None, None, None, refs[3])),
               _args(data=None, length=0, counts=refs), _args(sep_len=0, counts=refs),
               _args(sep_len=8, counts=refs), _args(select=1 << 63, counts=refs)):
        assert f(exe._h, *ok, *extra) == _lib.EAPI
        assert "device" in lib.redgpu_last_error().decode()
    # a text split refuses is a limit
    assert f(exe._h, *_args(length=1 << 45, counts=refs, out=out, out_cap=32), *extra) == _lib.ELIMIT
    assert [x.value for x in c] == [SENT] * 4
    assert list(out) == [SENT] * 32


def test_fields_text_device_none_handle_refused():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, TEXT, "1")
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, TEXT, [1, 3], sep=b"", max_fields=2, only_delimited=True)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, b"", "2-", delim=b";")
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.fields_text(exe, TEXT, "1", out_cap=0)


def test_fields_text_field_list_parser():
    from one_amd.matcher import fields_mask
    assert fields_mask("1,3,5-") == 0xFFFFFFFFFFFFFFF5
    assert fields_mask("1") == 1 and fields_mask("63") == 1 << 62
    assert fields_mask("64-") == 1 << 63 and fields_mask("63,64-") == 3 << 62
    assert fields_mask("1-") == (1 << 64) - 1
    assert fields_mask([1, 3]) == 5 and fields_mask((63,)) == 1 << 62
    assert fields_mask(" 2 , 4- ") == fields_mask("2,4-")
    for bad in ("64", "2-70", "0", "", "1,,2", "-3", "a", "65-", "1-2", [0], [64], [], [1.5]):
        with pytest.raises(one_amd.RedExceptApi):
            fields_mask(bad)
    # the verb parses before it looks at the handle or the text; a sep of nine bytes is refused
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    for bad in ("64", "2-70", "0", ""):
        with pytest.raises(one_amd.RedExceptApi, match="fields"):
            one_amd.fields_text(exe, TEXT, bad)
    with pytest.raises(one_amd.RedExceptApi, match="sep"):
        one_amd.fields_text(exe, TEXT, "1", sep=b"123456789")


def test_fields_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/fields_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "fields_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "fields_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
