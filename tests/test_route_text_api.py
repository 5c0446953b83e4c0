"""redgpu_route_text[_dev] (a raw text's lines grouped by result, as a text): the C-ABI face that
needs no GPU - the symbols and their prototypes, refused NULL arguments, the bin limit, refused
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
N_BINS = 3


def _args(data=TEXT, length=len(TEXT), n_bins=N_BINS, outs=(None,) * 5, out=None, out_cap=0,
          style=4):
    """(style, do_leader, drop_unmatched, data, len, delim, n_bins, n_lines, n_routed, bin_lines,
    bin_offsets, out_len, out, out_cap)"""
    return [style, 1, 0, data, length, 0x0A, n_bins, *outs, out, out_cap]


class _Outs:
    """sentinel-filled n_lines, n_routed, bin_lines[260], bin_offsets[260], out_len"""

    def __init__(self):
        self.n_lines, self.n_routed, self.out_len = (C.c_uint64(SENT) for _ in range(3))
        self.bin_lines = (C.c_uint64 * 260)(*([SENT] * 260))
        self.bin_offsets = (C.c_uint64 * 260)(*([SENT] * 260))

    def refs(self, bin_lines=True, bin_offsets=True, out_len=True, counts=True):
        return (C.byref(self.n_lines) if counts else None,
                C.byref(self.n_routed) if counts else None,
                self.bin_lines if bin_lines else None,
                self.bin_offsets if bin_offsets else None,
                C.byref(self.out_len) if out_len else None)

    def untouched(self):
        return ([self.n_lines.value, self.n_routed.value, self.out_len.value] == [SENT] * 3 and
                list(self.bin_lines) == [SENT] * 260 and list(self.bin_offsets) == [SENT] * 260)


def test_route_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_route_text", "redgpu_route_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "route_text" in one_amd.__all__
    assert callable(one_amd.route_text)


def test_route_text_prototypes_match_the_header():
    """the header declares both forms with the documented argument lists, and the ctypes
    prototypes have as many arguments of the same widths"""
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = ("const redgpu_dfa *dfa, int style, int do_leader, int drop_unmatched, "
            "const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins, "
            "uint64_t *n_lines, uint64_t *n_routed, uint64_t *bin_lines, uint64_t *bin_offsets, "
            "uint64_t *out_len, uint8_t *out, uint64_t out_cap")
    lib = _lib.lib()
    for name, tail in (("redgpu_route_text", ""), ("redgpu_route_text_dev", ", void *stream")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == want + tail, name
        kinds = []
        for arg in (want + tail).split(", "):
            kinds.append(C.c_void_p if "*" in arg else
                         {"int": C.c_int, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8}[arg.split()[0]])
        f = getattr(lib, name)
        assert f.restype is C.c_int
        assert list(f.argtypes) == kinds, name


def test_route_text_null_handle_refused():
    lib = _lib.lib()
    o = _Outs()
    assert lib.redgpu_route_text(None, *_args(outs=o.refs())) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_route_text_dev(None, *_args(outs=o.refs()), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert o.untouched()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_route_text_null_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_route_text if form == "host" else lib.redgpu_route_text_dev
    extra = [] if form == "host" else [None]
    o = _Outs()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    # NULL bin_offsets, NULL out_len, NULL data with len > 0: each refused for its own reason (the
    # argument checks run before the handle's device is looked at)
    assert f(exe._h, *_args(outs=o.refs(bin_offsets=False), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "bin_offsets" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(outs=o.refs(out_len=False), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "out_len" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(data=None, outs=o.refs(), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "null data" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    # ... and with nothing wrong, for the missing device; n_lines / n_routed / bin_lines / out NULL
    # is no fault, nor is a NULL data with len == 0, nor n_bins == 0 or 255
    assert f(exe._h, *_args(outs=o.refs(), out=out, out_cap=32), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(outs=o.refs(bin_lines=False, counts=False)), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    assert f(exe._h, *_args(data=None, length=0, outs=o.refs()), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    for n_bins in (0, 255):
        assert f(exe._h, *_args(n_bins=n_bins, outs=o.refs()), *extra) == _lib.EAPI
        assert "device" in lib.redgpu_last_error().decode()
    # a style that does not exist is no API fault; a text split refuses is a limit, and so are
    # more bins than 8 bit-planes hold
    assert f(exe._h, *_args(outs=o.refs(), style=9), *extra) == _lib.EEXEC
    assert f(exe._h, *_args(length=1 << 45, outs=o.refs(), out=out, out_cap=32), *extra) == _lib.ELIMIT
    assert f(exe._h, *_args(n_bins=256, outs=o.refs(), out=out, out_cap=32), *extra) == _lib.ELIMIT
    assert "n_bins" in lib.redgpu_last_error().decode(), lib.redgpu_last_error()
    assert f(exe._h, *_args(n_bins=1 << 40, outs=o.refs()), *extra) == _lib.ELIMIT
    assert o.untouched()
    assert list(out) == [SENT] * 32


def test_route_text_wrapper_argument_errors():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    # a device-less handle, whatever else is asked
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, TEXT, 1, one_amd.styLast, False, drop_unmatched=True)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, b"", 0, delim=b";")
    # the bin count
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, TEXT, -1)
    with pytest.raises(one_amd.RedExceptLimit):
        one_amd.route_text(exe, TEXT, 256)
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.route_text(exe, TEXT, out_cap=0)


def test_route_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/route_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "route_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "route_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
