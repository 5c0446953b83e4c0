"""redgpu_group_text[_dev] and redgpu_group_lds_slots (awk '{ s[$k] += $v }' of a raw text): the C-ABI
face that needs no GPU - the symbols and their prototypes, every refusal with its own message and
the caller's memory untouched, refused device-less handles, the front's size as a pure host
function, the wrapper's own argument errors, and the C++ mirror compiled against
include/redgpu.hpp."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

import one_amd
from one_amd import _lib
from golden_util import load_dfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = b"a 1\nb 22\na 3\nc\n"
SENT = 7
MATCH, FIELD = 0, 1
WANT = ("const redgpu_dfa *dfa, int what, uint64_t key_index, uint64_t value_index, int which, "
        "const uint8_t *data, uint64_t len, uint8_t delim, uint64_t table_slots, uint64_t cap, "
        "uint64_t *n_lines, uint64_t *n_keyed, uint64_t *n_numeric, uint64_t *n_distinct, "
        "uint64_t *n_dropped, uint64_t *first, uint64_t *length, uint64_t *count, uint64_t *stats")


class _Outs:
    """sentinel-filled scalars (five) and arrays (first, length, count of 4 cells, stats of 16)"""

    def __init__(self):
        self.scalars = [C.c_uint64(SENT) for _ in range(5)]
        self.arrays = [(C.c_uint64 * n)(*([SENT] * n)) for n in (4, 4, 4, 16)]

    def refs(self, scalars=True, arrays=True):
        return ([C.byref(c) if scalars else None for c in self.scalars] +
                [C.addressof(a) if arrays else None for a in self.arrays])

    def untouched(self):
        return ([c.value for c in self.scalars] == [SENT] * 5 and
                all(list(a) == [SENT] * len(a) for a in self.arrays))


def _args(outs, what=FIELD, key_index=1, value_index=2, which=0, data=TEXT, length=len(TEXT),
          slots=64, cap=4):
    return [what, key_index, value_index, which, data, length, 0x0A, slots, cap, *outs]


def test_group_text_symbols_exported():
    lib = _lib.lib()
    for name in ("redgpu_group_text", "redgpu_group_text_dev", "redgpu_group_lds_slots"):
        assert hasattr(lib, name), name
        assert name in _lib.declared_symbols(), name
    assert "group_text" in one_amd.__all__
    assert callable(one_amd.group_text)
    text = open(_lib.HEADER).read()
    for k, name in enumerate(("MATCH", "FIELD")):
        assert re.search(r"#define REDGPU_GROUP_%s\s+%d\b" % (name, k), text), name


def test_group_text_prototypes_match_the_header():
    """the header declares the three functions with the documented argument lists, and the ctypes
    prototypes have as many arguments of the same widths"""
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.lib()
    for name, tail in (("redgpu_group_text", ""), ("redgpu_group_text_dev", ", void *stream")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == WANT + tail, name
        kinds = []
        for arg in (WANT + tail).split(", "):
            kinds.append(C.c_void_p if "*" in arg else
                         {"int": C.c_int, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8}[arg.split()[0]])
        f = getattr(lib, name)
        assert f.restype is C.c_int
        assert list(f.argtypes) == kinds, name
    m = re.search(r"\buint32_t\s+redgpu_group_lds_slots\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()) == "const redgpu_dfa *dfa"
    assert lib.redgpu_group_lds_slots.restype is C.c_uint32
    assert list(lib.redgpu_group_lds_slots.argtypes) == [C.c_void_p]


def test_group_text_null_handle_refused():
    lib = _lib.lib()
    o = _Outs()
    assert lib.redgpu_group_text(None, *_args(o.refs())) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert lib.redgpu_group_text_dev(None, *_args(o.refs()), None) == _lib.EAPI
    assert "handle" in lib.redgpu_last_error().decode()
    assert o.untouched()


@pytest.mark.parametrize("form", ["host", "dev"])
def test_group_text_bad_arguments_refused(form):
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    lib = _lib.lib()
    f = lib.redgpu_group_text if form == "host" else lib.redgpu_group_text_dev
    extra = [] if form == "host" else [None]
    o = _Outs()

    def refused(word, code=_lib.EAPI, outs=None, **kw):
        assert f(exe._h, *_args(o.refs() if outs is None else outs, **kw), *extra) == code, (word, kw)
        assert word in lib.redgpu_last_error().decode(), (word, lib.redgpu_last_error())

    # each refused for its own reason (the argument checks run before the handle's device is
    # looked at)
    refused("null data", data=None)
    for what in (-1, 2, 3, 99):
        refused("what", what=what)
    for which in (-1, 2, 7):
        refused("which", which=which)
    for what in (MATCH, FIELD):
        refused("key_index", what=what, key_index=0)
    for slots in (0, 32, 63, 65, 96, (1 << 32) + 1, 1 << 33):
        refused("table_slots", slots=slots)
    # ... in the header's order: a bad `what` in front of a bad `which`, that in front of a bad
    # key_index, that in front of a bad table
    refused("what", what=7, which=5, key_index=0, slots=3)
    refused("which", which=5, key_index=0, slots=3)
    refused("key_index", key_index=0, slots=3)
    # with nothing wrong, for the missing device: every output NULL is no fault, nor is a NULL data
    # with len == 0, a value_index of 0, below or far above the key's, the largest table, cap 0
    for kw in (dict(), dict(outs=o.refs(scalars=False)), dict(outs=o.refs(arrays=False)),
               dict(outs=o.refs(False, False)), dict(data=None, length=0), dict(value_index=0),
               dict(key_index=2, value_index=1), dict(key_index=3, value_index=3),
               dict(what=MATCH, key_index=(1 << 64) - 1, value_index=(1 << 64) - 1),
               dict(slots=1 << 32), dict(cap=0), dict(which=1)):
        refused("device", **kw)
    # a text split refuses is a limit, as is one of 2^40 - 1 bytes
    refused("", code=_lib.ELIMIT, length=1 << 45)
    refused("", code=_lib.ELIMIT, length=(1 << 40) - 1)
    refused("device", length=(1 << 40) - 2)
    assert o.untouched()


def test_group_lds_slots_is_a_pure_host_function():
    lib = _lib.lib()
    assert lib.redgpu_group_lds_slots(None) == 0
    seen = set()
    names = sorted(os.path.basename(p)[:-5]
                   for p in glob.glob(os.path.join(ROOT, "tests", "golden", "dfas", "*.reda")))
    assert len(names) >= 9
    for name in names:
        exe = one_amd.Executable(load_dfa(name), device="none")
        n = lib.redgpu_group_lds_slots(exe._h)
        assert n == lib.redgpu_group_lds_slots(exe._h)
        # a power of two that 16 KiB hold at 48 bytes a slot, no front below 64 slots - and never
        # more slots than uniq_text's front of 16-byte slots has
        assert n == 0 or (64 <= n <= 16384 // 48 and n & (n - 1) == 0), (name, n)
        assert n <= lib.redgpu_uniq_lds_slots(exe._h), name
        seen.add(n)
    assert 256 in seen, seen                # a small table leaves room for the whole front


def test_group_text_wrapper_argument_errors():
    exe = one_amd.Executable(load_dfa("num3"), device="none")
    # a device-less handle, whatever else is asked
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.group_text(exe, TEXT)
    with pytest.raises(one_amd.RedExceptApi):
        one_amd.group_text(exe, TEXT, what="match", key_index=2, value_index=0, which="last",
                           delim=b";", max_distinct=7, cap=3)
    for bad in ("words", "whole", 1):
        with pytest.raises(one_amd.RedExceptApi, match="what"):
            one_amd.group_text(exe, TEXT, what=bad)
    for bad in ("middle", 0):
        with pytest.raises(one_amd.RedExceptApi, match="which"):
            one_amd.group_text(exe, TEXT, which=bad)
    for bad in (0, -1, 1 << 64):
        with pytest.raises(one_amd.RedExceptApi, match="key_index"):
            one_amd.group_text(exe, TEXT, key_index=bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(one_amd.RedExceptApi, match="value_index"):
            one_amd.group_text(exe, TEXT, value_index=bad)
    for bad in (0, -3, (1 << 31) + 1):
        with pytest.raises(one_amd.RedExceptApi, match="max_distinct"):
            one_amd.group_text(exe, TEXT, max_distinct=bad)
    with pytest.raises(one_amd.RedExceptApi, match="cap"):
        one_amd.group_text(exe, TEXT, cap=-1)


def test_group_text_cpp_mirror_compiles(tmp_path):
    """tests/cpp/group_text_test.cpp against include/redgpu.hpp and the library; without its
    arguments the program says so and touches no device"""
    prog = str(tmp_path / "group_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "group_text_test.cpp"), "-o", prog,
                    "-L", os.path.join(ROOT, "one_amd"), "-lredgpu", "-lpthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "one_amd")], check=True)
    assert subprocess.run([prog]).returncode == 2
