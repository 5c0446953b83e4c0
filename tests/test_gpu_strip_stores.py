"""GPU parity of the 64-byte walk's Outcome stores (k_stream_multi.h, the form for 64-byte lines:
non-temporal stores of an int32 and two uint64 per line) at the line counts and plane alignments
where a store wider than its element, or a line-to-lane mapping other than c * 512 + tid, would go
wrong - the forms measured and dropped in profiles/outcome_store_ab.txt, and whatever replaces
these stores next.  Everything goes through redgpu_match_batches_dev with raw device pointers,
stride 64, match<styLast, false>.  Every batch of every call: against the CPU oracle line for line
(result, start, end), against the single-batch entry point, and every output plane's guard
elements - 16 in front of element 0 and 16 from element n on - untouched.

A call of fewer than 256 tiles runs as single launches (launchStreamBatches), so each list of line
counts is run twice: as it stands, and with one aligned batch of 256 full tiles behind it, which
makes the call ONE launch of k_stream_multi with the list's tiles at its front."""
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
RES_SENTINEL = -0x5A5A5A5B
POS_SENTINEL = 0x7A7A7A7A7A7A7A7A

# the smallest counts at which a mapping or a pairing of lines can go wrong: one line; around a
# wave (64), two waves (128), a tile (1024), two tiles; batch borders on full tiles, on a one-line
# tile, full and ragged tiles alternating within one launch; more tiles than the grid, so that a
# workgroup walks several tiles and crosses a batch border
COUNTS = [
    [1],
    [63, 64, 65],
    [127, 128, 129],
    [1023, 1024, 1025],
    [2047, 2049],
    [1024, 1, 3072, 1025],
    [524288 + 1025, 2048],
]

# per plane: elements by which the view is moved off its alignment (result, start, end);
# start None = start = NULL
VARIANTS = {
    "aligned": lambda k: (0, 0, 0),
    "start_null": lambda k: (0, None, 0),
    "result_offset": lambda k: (1, 0, 0),         # result 4-byte aligned only
    "start_end_offset": lambda k: (0, 1, 1),      # start and end 8-byte aligned only
    "mixed": lambda k: (0, 0, 0) if k % 2 else (1, 1, 1),
}


def _lines(name, n, seed):
    if name == "syn256":
        return W.fixed_lines(n, STRIDE, seed, alphabet=False)
    plant = {"uri": W.URI_PLANT, "dotstar_err": b"an error"}[name]
    buf = W.fixed_lines(n, STRIDE, seed, plant=plant, plant_every=3, plant_at=7)
    v = buf.reshape(n, STRIDE)
    v[1::5, :len(plant[:STRIDE])] = np.frombuffer(plant[:STRIDE], dtype=np.uint8)
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


def _run_call(name, exe, counts, variant, filler):
    import torch
    ns = list(counts) + ([FILLER] if filler else [])
    batches = [_batch(name, n, 11 * k + n % 997) for k, n in enumerate(counts)]
    if filler:
        batches.append(_batch(name, FILLER, 5))
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
        what = (name, counts, variant, filler, k, n, kernel)
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


@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("name", ["syn256", "uri", "dotstar_err"])
def test_outcome_stores_vs_oracle(name, counts):
    exe = one_amd.Executable(load_dfa(name))
    for variant in VARIANTS:
        for filler in (False, True):
            _run_call(name, exe, counts, variant, filler)


def test_calibration_kernel_runs():
    """redgpu_diag_lines_dev (bench.py's memory roof of this shape) requests and stores as the walk
    does and has no answers to check: the call returns 0 and the stream drains, at fewer tiles
    than the grid and at more."""
    import torch
    exe = one_amd.Executable(load_dfa("syn256"))
    l = _lib.lib()
    sink = torch.zeros(1, dtype=torch.int32, device="cuda")
    for n in (2048, 1024 * 513):
        data = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
        r = torch.empty(n, dtype=torch.int32, device="cuda")
        s = torch.empty(n, dtype=torch.int64, device="cuda")
        e = torch.empty(n, dtype=torch.int64, device="cuda")
        rc = l.redgpu_diag_lines_dev(exe._h, data.data_ptr(), n, STRIDE, r.data_ptr(), s.data_ptr(),
                                     e.data_ptr(), sink.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, l.redgpu_last_error()
        torch.cuda.synchronize()
