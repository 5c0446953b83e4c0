"""redgpu_range_text[_dev] (sed's /open/,/close/ line ranges of a raw text): the C-ABI face that needs
no GPU - the symbols and their prototypes, refused NULL arguments and results below 1, refused
device-less handles, the wrapper's own argument errors, and the C++ mirror compiled against
include/redgpu.hpp."""
import ctypes as C
import os
import re
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n"
SENT = 7
REC = 8


def _args(data=TEXT, length=len(TEXT), open_result=1, close_result=2, counts=(None,) * 4, out=None,
          out_cap=0, rec_cap=0, recs=(None,) * 4, style=4):
    """(style, do_leader, open_result, close_result, emit_open, emit_close, invert, max_ranges,
    data, len, delim, n_lines, n_ranges, n_emitted, out_len, out, out_cap, rec_cap, first_line,
    last_line, begin, end)"""
    return [style, 1, open_result, close_result, 1, 1, 0, 1 << 62, data, length, 0x0A, *counts, out,
            out_cap, rec_cap, *recs]


class _Outs:
    """sentinel-filled n_lines, n_ranges, n_emitted, out_len and the four record arrays"""

    def __init__(self):
        self.counts = [C.c_uint64(SENT) for _ in range(4)]
        self.recs = [(C.c_uint64 * REC)(*([SENT] * REC)) for _ in range(4)]

    def refs(self, out_len=True, others=True):
        return tuple(C.byref(c) if have else None
                     for c, have in zip(self.counts, (others, others, others, out_len)))

    def untouched(self):
        return ([c.value for c in self.counts] == [SENT] * 4 and
                all(list(r) == [SENT] * REC for r in self.recs))


def test_range_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_range_text", "redgpu_range_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "range_text" in one_amd.__all__
    assert callable(one_amd.range_text)


def test_range_text_prototypes_match_the_header():
    """the header declares both forms with the documented argument lists, and the ctypes
    prototypes have as many arguments of the same widths"""
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = ("const redgpu_dfa *dfa, int style, int do_leader, int32_t open_result, "
            "int32_t close_result, int emit_open, int emit_close, int invert, uint64_t max_ranges, "
            "const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *n_lines, "
            "uint64_t *n_ranges, uint64_t *n_emitted, uint64_t *out_len, uint8_t *out, "
            "uint64_t out_cap, uint64_t rec_cap, uint64_t *first_line, uint64_t *last_line, "
            "uint64_t *begin, uint64_t *end")
    lib = _lib.lib()
    for name, tail in (("redgpu_range_text", ""), ("redgpu_range_text_dev", ", void *stream")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == want + tail, name
        kinds = []
        for arg in (want + tail).split(", "):
            kinds.append(C.c_void_p if "*" in arg else
                         {"int": C.c_int, "int32_t": C.c_int32, "uint64_t": C.c_uint64,
                          "uint8_t": C.c_uint8}[arg.split()[0]])
        f = getattr(lib, name)
        assert f.restype is C.c_int
        assert list(f.argtypes) == kinds, name


def test_range_text_null_handle_refused():
    lib = _lib.lib()
    o = _Outs()
    assert lib.redgpu_range_text(None, *_args(counts=o.refs(), rec_cap=REC, recs=o.recs)) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_range_text_dev(None, *_args(counts=o.refs(), rec_cap=REC, recs=o.recs),
                                     None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert o.untouched()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_range_text_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_range_text if form == "host" else lib.redgpu_range_text_dev
    extra = [] if form == "host" else [None]
    o = _Outs()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    full = dict(out=out, out_cap=32, rec_cap=REC, recs=o.recs)
    # NULL out_len, NULL data with len > 0, a result below 1: each refused for its own reason (the
    # argument checks run before the handle's device is looked at)
    assert f(exe._h, *_args(counts=o.refs(out_len=False), **full), *extra) == _lib.EAPI
    assert "out_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, counts=o.refs(), **full), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(open_result=0, counts=o.refs(), **full), *extra) == _lib.EAPI
    assert "open_result" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(close_result=-1, counts=o.refs(), **full), *extra) == _lib.EAPI
    assert "close_result" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(open_result=-5, close_result=-5, counts=o.refs(), **full),
             *extra) == _lib.EAPI
    assert "open_result" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; n_lines / n_ranges / n_emitted / out / the
    # records NULL is no fault, nor is a NULL data with len == 0, nor the toggle form
    assert f(exe._h, *_args(counts=o.refs(), **full), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(counts=o.refs(others=False)), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(counts=o.refs(), rec_cap=REC), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(data=None, length=0, counts=o.refs()), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(open_result=3, close_result=3, counts=o.refs()), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # a style that does not exist is no API fault; a text split refuses is a limit
    assert f(exe._h, *_args(counts=o.refs(), style=9, **full), *extra) == _lib.EEXEC
    assert f(exe._h, *_args(length=1 << 45, counts=o.refs(), **full), *extra) == _lib.ELIMIT
    assert o.untouched()
    assert list(out) == [SENT] * 32


def test_range_text_wrapper_argument_errors():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    # a device-less handle, whatever else is asked
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, TEXT, 1)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, TEXT, 1, 2, one_amd.styLast, False, emit_open=False, invert=True,
                           max_ranges=3, rec_cap=4)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, b"", 2, delim=b";")
    # the two results
    for bad in ((0, None), (-1, 1), (1, 0), (1, -7), (1 << 31, 1)):
        with pytest.raises(one_amd.RedExceptApi, match="result"):
            one_amd.range_text(exe, TEXT, *bad)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, TEXT, 1, max_ranges=-1)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, TEXT, 1, rec_cap=-1)
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.range_text(exe, TEXT, 1, out_cap=0)


def test_range_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/range_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "range_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "range_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
