"""GB/s of text per call of sum_text (per result the count, sum, min and max of the numbers in the
matches) over a raw text of delimiter-terminated lines, alternated in one process:
  (a) redgpu_sum_text_dev, FIRST and LAST, n_bins = max_result + 1;
  (b) the walk alone: redgpu_extract_text_dev, sizes only (out_cap = 0) - the same lines, the same
      chain, the pieces sized and not read again: the yardstick;
  (c) the route a caller had before: extract_text_dev's output and collect_text_dev's result column
      (the caps taken from counts the caller is GIVEN here - a caller who has to find them pays (b)
      on top), both downloaded, the first run of digits of every piece parsed and reduced on the host
      with numpy (runs located with vector operations, no Python loop over the pieces).  Wall clock,
      the median of 3: the host side takes seconds where the others take milliseconds;
  (d) (a) with REDGPU_SUM_PLAIN=1: four atomics per item, no carried run, no peel.
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_tally_text.py's), the DFA's piece at
the start of every 100th line (about 1 %), or of every line for num3.  letters4 is the statistics in
GLOBAL memory under load: the same line ends over random bytes of "abcd0123456789.", a DFA
(oracle.reda_writer) for one letter and [0-9]+ with the results L - 1, L, L + 1 and 70000
(L = redgpu_sum_lds_bins), so three items in four are 64-bit global atomics on three slots.
Device events around each call of (a), (b) and (d), the median of 10 after a warm-up call of each
route.  Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/sum_text_<MiB>mib.jsonl.
usage: bench_sum_text.py [MiB] [input ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import time
import numpy as np
import torch, one_amd
from one_amd import _lib
from one_amd import workloads as W
from oracle import reda_writer

args = sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["log100", "uri", "err", "num3", "letters4"]
PIECES = {"err": b"error", "log100": W.log100_heads()[7], "uri": W.URI_PLANT.rstrip(),
          "num3": b"12345a"}
EVERY = {"num3": 1}
REPS, HOST_REPS = 10, 3
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "sum_text_%dmib.jsonl" % mib)
rows = []


def make_text(piece, n, every):
    """lines of 32..256 bytes (delimiter included), the piece at the start of every `every`-th"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    n_lines = int(np.searchsorted(ends, n, side="right"))
    ends = ends[:n_lines]
    a = W.alphabet_bytes(n, 1).copy()
    a[a == 0x0A] = 0x20
    a[ends - 1] = 0x0A
    begins = np.concatenate([[0], ends[:-1]])[::every]
    p = np.frombuffer(piece, dtype=np.uint8)
    begins = begins[begins + len(p) < n]  # (a piece longer than its line runs into the next one)
    a[begins[:, None] + np.arange(len(p))[None, :]] = p[None, :]
    return a


def letter_digits(results):
    """one letter of abcd, then [0-9]+: error, initial, and per letter the state behind it and the
    accepting state of the digits"""
    equiv = np.full(256, 5, dtype=np.uint8)
    for k, ch in enumerate(b"abcd"):
        equiv[ch] = k
    equiv[0x30:0x3A] = 4
    trans = np.zeros((10, 6), dtype=np.int64)
    res = [0] * 10
    for k in range(4):
        trans[1][k] = 2 + 2 * k
        trans[2 + 2 * k][4] = 3 + 2 * k
        trans[3 + 2 * k][4] = 3 + 2 * k
        res[3 + 2 * k] = results[k]
    return reda_writer.write_reda(trans, res, equiv=equiv)


def timed(fn):
    """milliseconds between two device events around fn(), and what it returned"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def walled(fn):
    """milliseconds of wall clock around fn() (it ends on the host), and what it returned"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms, n):
    g = sorted(n / (m * 1e6) for m in ms)
    return {"median_GBps": g[len(g) // 2], "min_GBps": g[0], "max_GBps": g[-1]}


def plainly(fn):
    def run():
        os.environ["REDGPU_SUM_PLAIN"] = "1"
        try:
            return fn()
        finally:
            os.environ["REDGPU_SUM_PLAIN"] = "0"
    return run


def host_reduce(out, result, n_bins):
    """stats[4, n_bins + 1] from extract_text's output (pieces, each followed by '\\n') and the
    pieces' results: the FIRST run of digits of every piece, in numpy"""
    st = np.zeros((4, n_bins + 1), dtype=np.uint64)
    st[2] = np.uint64(2 ** 64 - 1)
    if not out.size:
        return st
    digit = (out >= 0x30) & (out <= 0x39)
    prev = np.concatenate([[False], digit[:-1]])
    nxt = np.concatenate([digit[1:], [False]])
    begins = np.flatnonzero(digit & ~prev)
    lasts = np.flatnonzero(digit & ~nxt)            # (a delimiter ends every piece, so every run too)
    ends = np.flatnonzero(out == 0x0A)
    piece = np.searchsorted(ends, begins)           # the piece every run is in
    first = np.concatenate([[True], piece[1:] != piece[:-1]]) if piece.size else np.zeros(0, bool)
    b, e, piece = begins[first], lasts[first] + 1, piece[first]
    length = e - b
    # (a run of 20 digits and more may be 2^64 and more: parsed one by one, there are few)
    long_ = np.flatnonzero(length > 19)
    longs = [(int(piece[k]), int(out[b[k]:e[k]].tobytes())) for k in long_]
    keep = length <= 19
    b, e, piece, length = b[keep], e[keep], piece[keep], length[keep]
    # digit i of a run weighs 10^(e - 1 - i)
    idx = np.repeat(b, length) + (np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length))
    weight = np.uint64(10) ** (np.repeat(e, length) - 1 - idx).astype(np.uint64)
    value = np.add.reduceat((out[idx] - 0x30).astype(np.uint64) * weight, np.cumsum(length) - length) \
        if length.size else np.zeros(0, np.uint64)
    fits = [(k, v) for k, v in longs if v < 2 ** 64]
    piece = np.concatenate([piece, np.array([k for k, _ in fits], dtype=piece.dtype)])
    value = np.concatenate([value, np.array([v for _, v in fits], dtype=np.uint64)])
    slot = result[piece].astype(np.int64)
    slot = np.where((slot >= 0) & (slot < n_bins), slot, n_bins)
    if not slot.size:
        return st
    order = np.argsort(slot, kind="stable")
    slot, value = slot[order], value[order]
    at = np.flatnonzero(np.concatenate([[True], slot[1:] != slot[:-1]]))
    st[0][slot[at]] = np.diff(np.concatenate([at, [slot.size]])).astype(np.uint64)
    st[1][slot[at]] = np.add.reduceat(value, at)
    st[2][slot[at]] = np.minimum.reduceat(value, at)
    st[3][slot[at]] = np.maximum.reduceat(value, at)
    return st


for name in names:
    every = EVERY.get(name, 100)
    if name == "letters4":
        probe = one_amd.Executable(letter_digits((1, 2, 3, 4)), device="none")
        L = int(_lib.lib().redgpu_sum_lds_bins(probe._h))
        exe = one_amd.Executable(letter_digits((L - 1, L, L + 1, 70000)))
        host = make_text(b"", mib << 20, 1)
        ends = host == 0x0A
        host = np.frombuffer(b"abcd0123456789.", dtype=np.uint8)[
            np.random.default_rng(7).integers(0, 15, host.size)].copy()
        host[ends] = 0x0A
    else:
        blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
        exe = one_amd.Executable(blob)
        host = make_text(PIECES[name], mib << 20, every)
    lds_bins = int(_lib.lib().redgpu_sum_lds_bins(exe._h))
    n = host.size
    dev = torch.from_numpy(host).cuda()
    n_bins = exe.info["max_result"] + 1
    sizes = one_amd.extract_text(exe, dev, out_cap=0)
    total, out_len = int(sizes[1].item()), int(sizes[2].item())
    out_buf = torch.empty(out_len + 16, dtype=torch.uint8, device="cuda")

    def sum_first():
        return one_amd.sum_text(exe, dev, n_bins, which="first")

    def sum_last():
        return one_amd.sum_text(exe, dev, n_bins, which="last")

    def walk_alone():
        return one_amd.extract_text(exe, dev, out_cap=0)

    def composed():
        one_amd.extract_text(exe, dev, out=out_buf, out_cap=out_len)
        rec = one_amd.collect_text(exe, dev, cap=total + 16, want_positions=False)
        out = out_buf[:out_len].cpu().numpy()
        result = rec[4][:total].cpu().numpy()
        return host_reduce(out, result, n_bins)

    routes = {"sum_first": sum_first, "sum_last": sum_last, "extract_text_sizes_only": walk_alone,
              "sum_first_plain": plainly(sum_first), "sum_last_plain": plainly(sum_last)}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    outs["composed_extract_collect_host"] = composed()  # warm-up
    ms["composed_extract_collect_host"] = []
    for _ in range(HOST_REPS):
        t, outs["composed_extract_collect_host"] = walled(composed)
        ms["composed_extract_collect_host"].append(t)
    # every route computes the same things
    a, z = outs["sum_first"], outs["sum_last"]
    assert int(a[1].item()) == total == int(outs["extract_text_sizes_only"][1].item()) == int(z[1].item())
    assert torch.equal(a[3], outs["sum_first_plain"][3]) and torch.equal(z[3], outs["sum_last_plain"][3])
    first = a[3].cpu().numpy().view(np.uint64)
    assert np.array_equal(first, outs["composed_extract_collect_host"])
    n_numeric = int(a[2].item())
    assert n_numeric == int(first[0].sum())
    row = {"input": name, "mib": mib, "lines": int(a[0].item()), "items": total, "n_numeric": n_numeric,
           "n_numeric_last": int(z[2].item()), "every": every, "n_bins": n_bins, "lds_bins": lds_bins,
           "stats_bytes": 32 * (n_bins + 1), "composed_bytes_downloaded": out_len + 4 * total,
           "items_in_lds_slots_share": float(first[0][:lds_bins].sum()) / max(1, n_numeric)}
    for k in ms:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    row["ratio_sum_first_to_walk"] = med("sum_first") / med("extract_text_sizes_only")
    row["ratio_sum_last_to_walk"] = med("sum_last") / med("extract_text_sizes_only")
    row["ratio_plain_first_to_walk"] = med("sum_first_plain") / med("extract_text_sizes_only")
    row["ratio_sum_first_to_composed"] = med("sum_first") / med("composed_extract_collect_host")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, out_buf
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
