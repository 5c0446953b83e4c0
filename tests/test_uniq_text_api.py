"""redgpu_uniq_text[_dev] (a raw text's distinct matches, or selected lines, counted by their
bytes): the C-ABI face that needs no GPU - the symbols and their prototypes, refused NULL
arguments, a bad `what`, a bad table size, the text limit, refused device-less handles, the
wrapper's own argument errors, and the C++ mirror compiled against include/redgpu.hpp."""
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
ROWS = 8


def _args(what=1, data=TEXT, length=len(TEXT), slots=64, cap=ROWS, outs=(None,) * 7, style=4,
          per=1 << 62):
    """(what, style, do_leader, data, len, delim, max_per_line, table_slots, cap, n_lines, n_items,
    n_distinct, n_dropped, first, length, count)"""
    return [what, style, 1, data, length, 0x0A, per, slots, cap, *outs]


class _Outs:
    """sentinel-filled counters and first / length / count of ROWS each"""

    def __init__(self):
        self.counts = [C.c_uint64(SENT) for _ in range(4)]
        self.arrays = [(C.c_uint64 * ROWS)(*([SENT] * ROWS)) for _ in range(3)]

    def refs(self, counts=True, arrays=True):
        return tuple(C.byref(c) if counts else None for c in self.counts) + \
            tuple(a if arrays else None for a in self.arrays)

    def untouched(self):
        return (all(c.value == SENT for c in self.counts) and
                all(list(a) == [SENT] * ROWS for a in self.arrays))


def test_uniq_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_uniq_text", "redgpu_uniq_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "uniq_text" in one_amd.__all__
    assert callable(one_amd.uniq_text)


def test_uniq_text_prototypes_match_the_header():
    """the header declares both forms with the documented argument lists, and the ctypes
    prototypes have as many arguments of the same widths"""
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+REDGPU_UNIQ_LINES\s+0\b", text)
    assert re.search(r"#define\s+REDGPU_UNIQ_MATCHES\s+1\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = ("const redgpu_dfa *dfa, int what, int style, int do_leader, const uint8_t *data, "
            "uint64_t len, uint8_t delim, uint64_t max_per_line, uint64_t table_slots, "
            "uint64_t cap, uint64_t *n_lines, uint64_t *n_items, uint64_t *n_distinct, "
            "uint64_t *n_dropped, uint64_t *first, uint64_t *length, uint64_t *count")
    lib = _lib.lib()
    for name, tail in (("redgpu_uniq_text", ""), ("redgpu_uniq_text_dev", ", void *stream")):
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


def test_uniq_text_null_handle_refused():
    lib = _lib.lib()
    o = _Outs()
    assert lib.redgpu_uniq_text(None, *_args(outs=o.refs())) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_uniq_text_dev(None, *_args(outs=o.refs()), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert o.untouched()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_uniq_text_bad_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_uniq_text if form == "host" else lib.redgpu_uniq_text_dev
    extra = [] if form == "host" else [None]
    o = _Outs()
    err = lambda: lib.redgpu_last_error().decode()   # noqa: E731
    # NULL data with len > 0, a bad what, a bad table size: each refused for its own reason (the
    # argument checks run before the handle's device is looked at), in tally_text's order
    assert f(exe._h, *_args(data=None, what=5, slots=3, outs=o.refs()), *extra) == _lib.EAPI
    assert "null data" in err(), err()
    for what in (-1, 2, 5):
        assert f(exe._h, *_args(what=what, slots=3, style=9, outs=o.refs()), *extra) == _lib.EAPI
        assert "what" in err(), err()
    for slots in (0, 1, 32, 63, 65, 96, 127, (1 << 32) + 1, 1 << 33, (1 << 64) - 1):
        for what in (0, 1):
            assert f(exe._h, *_args(what=what, slots=slots, style=9, outs=o.refs()), *extra) == _lib.EAPI
            assert "table_slots" in err(), (slots, err())
    # ... and with nothing wrong, for the missing device: every output NULL is no fault, nor is a
    # NULL data with len == 0, nor the smallest and the largest table, nor cap == 0
    for kw in (dict(), dict(outs=(None,) * 7), dict(data=None, length=0), dict(slots=1 << 32),
               dict(what=0), dict(cap=0), dict(per=0)):
        kw.setdefault("outs", o.refs())
        assert f(exe._h, *_args(**kw), *extra) == _lib.EAPI, kw
        assert "device" in err(), (kw, err())
    # a style that does not exist is no API fault and is looked at under LINES alone; a text
    # split refuses is a limit, and so is one of 2^40 - 1 bytes
    assert f(exe._h, *_args(what=0, style=9, outs=o.refs()), *extra) == _lib.EEXEC
    assert f(exe._h, *_args(what=1, style=9, outs=o.refs()), *extra) == _lib.EAPI
    assert "device" in err(), err()
    assert f(exe._h, *_args(length=1 << 45, outs=o.refs()), *extra) == _lib.ELIMIT
    assert f(exe._h, *_args(length=(1 << 40) - 1, outs=o.refs()), *extra) == _lib.ELIMIT
    assert f(exe._h, *_args(length=(1 << 40) - 2, outs=o.refs()), *extra) == _lib.EAPI
    assert "device" in err(), err()
    assert o.untouched()


def test_uniq_text_wrapper_argument_errors():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    # a device-less handle, whatever else is asked
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.uniq_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.uniq_text(exe, TEXT, matches=False, style=one_amd.styLast, do_leader=False)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.uniq_text(exe, b"", delim=b";", max_distinct=1, cap=0)
    # the table's size, the cap, the per-line limit
    for kw in (dict(max_distinct=0), dict(max_distinct=-3), dict(max_distinct=(1 << 31) + 1),
               dict(cap=-1), dict(max_per_line=-1)):
        with pytest.raises(one_amd.RedExceptApi):
            one_amd.uniq_text(exe, TEXT, **kw)
    # positional options are not taken
    with pytest.raises(TypeError):
        one_amd.uniq_text(exe, TEXT, True)


def test_uniq_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/uniq_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "uniq_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "uniq_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
