"""redgpu_dedup_text[_dev] (awk '!seen[$k]++' of a raw text): the C-ABI face that needs no GPU - the
symbols and their prototypes, every refusal with its own message and the caller's memory untouched,
refused device-less handles, the wrapper's own argument errors, and the C++ mirror compiled against
include/redgpu.hpp."""
import ctypes as C
import os
import re
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

TEXT = b"123 45\nabc\n45\n123 45\n"
SENT = 7
WHOLE, LINES, MATCH, FIELD = 0, 1, 2, 3


def _args(what=WHOLE, style=4, key_index=1, data=TEXT, length=len(TEXT), slots=64,
          counts=(None,) * 6, out=None, out_cap=0):
    """(what, style, do_leader, key_index, min_count, max_count, invert, keep_unkeyed, data, len,
    delim, table_slots, n_lines, n_keyed, n_distinct, n_dropped, n_emitted, out_len, out, out_cap)"""
    return [what, style, 1, key_index, 1, (1 << 64) - 1, 0, 0, data, length, 0x0A, slots, *counts,
            out, out_cap]


class _Outs:
    """sentinel-filled n_lines, n_keyed, n_distinct, n_dropped, n_emitted, out_len"""

    def __init__(self):
        self.counts = [C.c_uint64(SENT) for _ in range(6)]

    def refs(self, out_len=True, others=True):
        return tuple(C.byref(c) if have else None
                     for c, have in zip(self.counts, (others,) * 5 + (out_len,)))

    def untouched(self):
        return [c.value for c in self.counts] == [SENT] * 6


def test_dedup_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_dedup_text", "redgpu_dedup_text_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "dedup_text" in one_amd.__all__
    assert callable(one_amd.dedup_text)
    text = open(_lib.HEADER).read()
    for k, name in enumerate(("WHOLE", "LINES", "MATCH", "FIELD")):
        assert re.search(r"#define REDGPU_DEDUP_%s\s+%d\b" % (name, k), text), name


def test_dedup_text_prototypes_match_the_header():
    """the header declares both forms with the documented argument lists, and the ctypes
    prototypes have as many arguments of the same widths"""
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = ("const redgpu_dfa *dfa, int what, int style, int do_leader, uint64_t key_index, "
            "uint64_t min_count, uint64_t max_count, int invert, int keep_unkeyed, "
            "const uint8_t *data, uint64_t len, uint8_t delim, uint64_t table_slots, "
            "uint64_t *n_lines, uint64_t *n_keyed, uint64_t *n_distinct, uint64_t *n_dropped, "
            "uint64_t *n_emitted, uint64_t *out_len, uint8_t *out, uint64_t out_cap")
    lib = _lib.lib()
    for name, tail in (("redgpu_dedup_text", ""), ("redgpu_dedup_text_dev", ", void *stream")):
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


def test_dedup_text_null_handle_refused():
    lib = _lib.lib()
    o = _Outs()
    assert lib.redgpu_dedup_text(None, *_args(counts=o.refs())) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_dedup_text_dev(None, *_args(counts=o.refs()), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert o.untouched()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_dedup_text_bad_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_dedup_text if form == "host" else lib.redgpu_dedup_text_dev
    extra = [] if form == "host" else [None]
    o = _Outs()
    out = (C.c_uint8 * 32)(*([SENT] * 32))
    full = dict(out=out, out_cap=32)

    def refused(word, code=_lib.EAPI, **kw):
        counts = kw.pop("counts", o.refs())
        assert f(exe._h, *_args(counts=counts, **full, **kw), *extra) == code, (word, kw)
        assert word in lib.redgpu_last_error().decode(), (word, lib.redgpu_last_error())

    # each refused for its own reason (the argument checks run before the handle's device is
    # looked at)
    refused("out_len", counts=o.refs(out_len=False))
    refused("null data", data=None)
    for what in (-1, 4, 99):
        refused("what", what=what)
    for what in (MATCH, FIELD):
        refused("key_index", what=what, key_index=0)
    for slots in (0, 32, 63, 65, 96, (1 << 32) + 1, 1 << 33):
        refused("table_slots", slots=slots)
    # ... in the header's order: a bad `what` in front of a bad table
    refused("what", what=7, slots=3)
    # with nothing wrong, for the missing device: the five other counters and out NULL are no fault,
    # nor is a NULL data with len == 0, key_index 0 where it is not looked at, the largest table
    for kw in (dict(), dict(counts=o.refs(others=False)), dict(data=None, length=0),
               dict(what=WHOLE, key_index=0), dict(what=LINES, key_index=0), dict(slots=1 << 32),
               dict(what=MATCH, key_index=(1 << 64) - 1), dict(what=FIELD, key_index=3)):
        refused("device", **kw)
    assert f(exe._h, *_args(counts=o.refs(), what=FIELD), *extra) == _lib.EAPI
    assert "device" in lib.redgpu_last_error().decode()
    # a style that does not exist is no API fault, and is looked at under LINES alone; a text split
    # refuses is a limit, as is one of 2^40 - 1 bytes
    refused("", code=_lib.EEXEC, what=LINES, style=9)
    for what in (WHOLE, MATCH, FIELD):
        refused("device", what=what, style=9)
    refused("", code=_lib.ELIMIT, length=1 << 45)
    refused("", code=_lib.ELIMIT, length=(1 << 40) - 1)
    refused("device", length=(1 << 40) - 2)
    assert o.untouched()
    assert list(out) == [SENT] * 32


def test_dedup_text_wrapper_argument_errors():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    # a device-less handle, whatever else is asked
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.dedup_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.dedup_text(exe, TEXT, what="field", key_index=2, min_count=2, max_count=5,
                           invert=True, keep_unkeyed=True, max_distinct=7)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.dedup_text(exe, b"", what="lines", style=one_amd.styLast, delim=b";")
    with pytest.raises(one_amd.RedExceptApi, match="what"):
        one_amd.dedup_text(exe, TEXT, what="words")
    with pytest.raises(one_amd.RedExceptApi, match="what"):
        one_amd.dedup_text(exe, TEXT, what=2)
    for what in ("match", "field"):
        for bad in (0, -1):
            with pytest.raises(one_amd.RedExceptApi, match="key_index"):
                one_amd.dedup_text(exe, TEXT, what=what, key_index=bad)
    with pytest.raises(one_amd.RedExceptApi, match="key_index"):
        one_amd.dedup_text(exe, TEXT, what="match", key_index=1 << 64)
    for kw in (dict(min_count=-1), dict(max_count=-1), dict(min_count=1 << 64),
               dict(max_count=1 << 64)):
        with pytest.raises(one_amd.RedExceptApi, match="count"):
            one_amd.dedup_text(exe, TEXT, **kw)
    for bad in (0, -3, (1 << 31) + 1):
        with pytest.raises(one_amd.RedExceptApi, match="max_distinct"):
            one_amd.dedup_text(exe, TEXT, max_distinct=bad)
    # out= / out_cap= go with a device text
    with pytest.raises(one_amd.RedExceptApi, match="out"):
        one_amd.dedup_text(exe, TEXT, out_cap=0)


def test_dedup_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/dedup_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = str(tmp_path / "dedup_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "dedup_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(root, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(root, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
