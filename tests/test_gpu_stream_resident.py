"""GPU parity of the 64-byte multi-batch walk (k_stream_multi.h, the form for 64-byte lines: one
register block per line, reloaded in place for the workgroup's next tile, a workgroup of more
than 512 threads) at the line counts that surround every workgroup size the form can take -
512, 640, 768 or 1024 threads, tiles of 1024, 1280, 1536 or 2048 lines - so the file does not
depend on which of them is in the library.  Everything goes through redgpu_match_batches_dev with
raw device pointers, stride 64, match<styLast, false>.  Every batch of every call: against the CPU
oracle line for line (result, start, end), against the single-batch entry point, and every output
plane's guard elements - 16 in front of element 0 and 16 from element n on - untouched.

A call of fewer than 256 tiles of 1024 lines runs as single launches (launchStreamBatches), so each
list of line counts is run twice: as it stands, and with one aligned batch of 256 such tiles behind
it, which makes the call ONE launch of k_stream_multi with the list's tiles at its front;
last_kernel() is asserted there.  A launch takes 32 batches at the most: the list of 32 batches gets
the filler behind its first 31 and, in a second call, behind its last 31.

The text DFAs' lines: every third line carries a match that ends on the line's LAST byte (the last
reload and the last store of a line carry information), every seventh is blank and matches
nothing; the fixtures assert both on the oracle's answers."""
import numpy as np
import pytest

import one_amd
import oracle as O
from golden_util import load_dfa
from one_amd import _lib
from one_amd import workloads as W

pytestmark = pytest.mark.gpu

STRIDE = 64
STYLE = 4          # styLast
GUARD = 16
FILLER = 256 * 1024
MAX_BATCHES = 32   # kMultiMax
RES_SENTINEL = -0x5A5A5A5B
POS_SENTINEL = 0x7A7A7A7A7A7A7A7A

SHARES = (512, 640, 768, 1024)      # a chain's share of a tile = the workgroup's threads
TILES = tuple(2 * t for t in SHARES)


def _around(n):
    return [n - 1, n, n + 1]


COUNTS = (
    [[1]] +
    # a chain's share, a tile and two tiles of each geometry, each at n - 1, n and n + 1
    [_around(t) + _around(2 * t) + _around(4 * t) for t in SHARES] +
    # 32 batches, 1 line and one tile + 1 lines alternating (the tiles of every geometry in turn),
    # each batch with its own input buffer: a reload across a batch border that uses the wrong
    # batch's pointer shows in the results
    [[1 if k % 2 == 0 else TILES[(k // 2) % 4] + 1 for k in range(MAX_BATCHES)]] +
    # more tiles than three times the grid (2 x 256 workgroups) of the largest tile: a workgroup
    # reloads across several tiles and a border
    [[3 * 512 * 2048 + 2049, 2049]]
)

# per plane: elements by which the view is moved off its alignment (result, start, end);
# start None = start = NULL
VARIANTS = {
    "aligned": lambda k: (0, 0, 0),
    "start_null": lambda k: (0, None, 0),
    "result_offset": lambda k: (1, 0, 0),         # result 4-byte aligned only
    "start_end_offset": lambda k: (0, 1, 1),      # start and end 8-byte aligned only
}

_URI_HEAD, _URI_TAIL = b"https://ab-c.example.com:8080/p/", b".y?q=1&r=%20#frag"
# (match is anchored: the URI fills its line; "an error" closes a line of anything)
PLANTS = {"uri": _URI_HEAD + b"x" * (STRIDE - len(_URI_HEAD) - len(_URI_TAIL)) + _URI_TAIL,
          "dotstar_err": b"an error"}


def _lines(name, n, seed):
    if name == "syn256":
        return W.fixed_lines(n, STRIDE, seed, alphabet=False)
    plant = PLANTS[name]
    buf = W.fixed_lines(n, STRIDE, seed, plant=plant, plant_every=3, plant_at=STRIDE - len(plant))
    buf.reshape(n, STRIDE)[5::7, :] = 0     # blank lines
    return buf


_cache = {}


def _batch(name, n, seed):
    """(host lines, device lines, oracle Outcomes, single-batch Outcomes), made once per batch."""
    import torch
    key = (name, n, seed)
    if key not in _cache:
        blob = load_dfa(name)
        exe = one_amd.Executable(blob)
        h = _lines(name, n, seed)
        d = torch.from_numpy(h).cuda()
        exp = O.CpuOracle(blob).batch("match", STYLE, 0, h, stride=STRIDE, n=n, threads=4)
        if name != "syn256" and n >= 64:
            planted, blank = np.arange(n) % 3 == 0, np.arange(n) % 7 == 5
            assert (exp[2][planted & ~blank] == STRIDE).all(), "a planted match ends on the last byte"
            assert (exp[0][blank] == 0).all(), "a blank line matches nothing"
        one = one_amd.match_batch(exe, d, STYLE, 0, stride=STRIDE, n=n)
        torch.cuda.synchronize()
        one = tuple(x.cpu().numpy() for x in one)
        assert np.array_equal(one[0], exp[0]) and np.array_equal(one[1].astype(np.uint64), exp[1])
        assert np.array_equal(one[2].astype(np.uint64), exp[2])
        _cache[key] = (h, d, exp, one)
    return _cache[key]


class _Plane:
    """n elements with GUARD sentinels on each side, the view moved `off` elements further."""

    def __init__(self, n, dtype, sentinel, off):
        import torch
        self.n, self.lo, self.sentinel = n, GUARD + off, sentinel
        self.t = torch.full((n + 2 * GUARD + 1,), sentinel, dtype=dtype, device="cuda")
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()

    def check(self, what):
        a = self.t.cpu().numpy()
        assert (a[:self.lo] == self.sentinel).all(), ("written in front of element 0", what)
        assert (a[self.lo + self.n:] == self.sentinel).all(), ("written at or past element n", what)
        return a[self.lo:self.lo + self.n]


def _run_call(name, exe, batches, variant, filler):
    """One call of redgpu_match_batches_dev over `batches` (+ the filler batch), all checks."""
    import torch
    batches = list(batches) + ([_batch(name, FILLER, 5)] if filler else [])
    ns = [len(b[2][0]) for b in batches]
    assert len(ns) <= MAX_BATCHES or not filler
    descs = (_lib.BatchDesc * len(ns))()
    planes = []
    for k, n in enumerate(ns):
        ro, so, eo = VARIANTS[variant](k)
        if filler and k == len(ns) - 1 and variant != "start_null":
            ro, so, eo = 0, 0, 0      # (start is NULL for every batch of a call or for none)
        r = _Plane(n, torch.int32, RES_SENTINEL, ro)
        s = _Plane(n, torch.int64, POS_SENTINEL, so) if so is not None else None
        e = _Plane(n, torch.int64, POS_SENTINEL, eo)
        assert r.ptr % 8 == (4 if ro else 0) and e.ptr % 16 == (8 if eo else 0)
        planes.append((r, s, e))
        descs[k] = _lib.BatchDesc(batches[k][1].data_ptr(), None, STRIDE, n, r.ptr,
                                  s.ptr if s is not None else None, e.ptr)
    rc = _lib.lib().redgpu_match_batches_dev(exe._h, STYLE, 0, descs, len(ns),
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().redgpu_last_error()
    kernel = one_amd.last_kernel()
    torch.cuda.synchronize()
    if filler:
        assert kernel == ("k_stream_multi<last,end>" if variant == "start_null"
                          else "k_stream_multi<last,start,end>"), kernel
    for k, n in enumerate(ns):
        what = (name, ns[:4], len(ns), variant, filler, k, n, kernel)
        _, _, exp, one = batches[k]
        r, s, e = planes[k]
        gr = r.check(what)
        assert np.array_equal(gr, exp[0]), ("result", what)
        assert np.array_equal(gr, one[0]), ("result, single batch", what)
        ge = e.check(what)
        assert np.array_equal(ge.astype(np.uint64), exp[2]), ("end", what)
        assert np.array_equal(ge, one[2]), ("end, single batch", what)
        if s is not None:
            gs = s.check(what)
            assert np.array_equal(gs.astype(np.uint64), exp[1]), ("start", what)
            assert np.array_equal(gs, one[1]), ("start, single batch", what)


def _id(counts):
    if len(counts) > 9:
        return "%dx(1,tile+1)" % len(counts)
    return "+".join(map(str, counts))


@pytest.mark.parametrize("counts", COUNTS, ids=_id)
@pytest.mark.parametrize("name", ["syn256", "uri", "dotstar_err"])
def test_resident_walk_vs_oracle(name, counts):
    exe = one_amd.Executable(load_dfa(name))
    batches = [_batch(name, n, 11 * k + n % 997) for k, n in enumerate(counts)]
    room = MAX_BATCHES - 1
    windows = [batches] if len(batches) <= room else [batches[:room], batches[-room:]]
    try:
        for variant in VARIANTS:
            _run_call(name, exe, batches, variant, False)
            for w in windows:
                _run_call(name, exe, w, variant, True)
    finally:
        for key in [k for k in _cache if k[1] > FILLER]:   # the 200 MB batch: not kept
            del _cache[key]
