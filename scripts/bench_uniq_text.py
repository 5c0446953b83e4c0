"""GB/s of text per call of uniq_text (grep -o | sort | uniq -c keyed by the matched bytes) over a
raw text of delimiter-terminated lines, all device-resident and alternated in one process:
  (a) redgpu_uniq_text_dev, MATCHES, max_distinct = 2^20 (a table of 2^21 slots, 32 MiB);
  (b) the same with REDGPU_UNIQ_PLAIN=1: no LDS front, every item to the global table;
  (c) the walk alone: redgpu_extract_text_dev sizes only (the same chain, a hit bitmap, two sums
      and a scan) and redgpu_tally_text_dev (the same chain, a histogram by result);
  (d) the composed route a caller had before: extract_text_dev with its output (the room taken
      from a count the caller is GIVEN here), the download, and collections.Counter over the
      pieces on the host - timed with a host clock around the whole, the others with device events.
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_tally_text.py's), the DFA's piece at
the start of every 100th line (about 1 %), or of every line for num3 and err_dense.  aab_hot is
one hot piece in every line; distinct1m is num3 over digit-free lines that each begin with one of
2^20 seven-digit numbers (about 0.86 M distinct pieces, the table 41 % full).
The median of 10 after a warm-up call of each route ((d): of 3).
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/uniq_text_<MiB>mib.jsonl.
usage: bench_uniq_text.py [MiB] [--profile] [input ...]   (--profile: two calls of (a) per input
and nothing else - for a kernel trace)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import collections
import json
import time
import numpy as np
import torch, one_amd
from one_amd import _lib
from one_amd import workloads as W

args = [a for a in sys.argv[1:] if a != "--profile"]
profile = "--profile" in sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["log100", "err", "uri", "num3", "err_dense", "aab_hot", "distinct1m"]
PIECES = {"err": b"error", "log100": W.log100_heads()[7], "uri": W.URI_PLANT.rstrip(),
          "num3": b"12345a", "aab": b"aab"}
EVERY = {"num3": 1, "err_dense": 1, "aab_hot": 1}
REPS, HOST_REPS = 10, 3
MAX_DISTINCT = 1 << 20
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "uniq_text_%dmib.jsonl" % mib)
rows = []


def make_text(piece, n, every, numbers=False):
    """lines of 32..256 bytes (delimiter included), the piece at the start of every `every`-th;
    numbers: no digit but a seven-digit number of its own at the start of every line"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    n_lines = int(np.searchsorted(ends, n, side="right"))
    ends = ends[:n_lines]
    a = W.alphabet_bytes(n, 1).copy()
    a[a == 0x0A] = 0x20
    begins = np.concatenate([[0], ends[:-1]])
    if numbers:
        a[(a >= 0x30) & (a <= 0x39)] = 0x78
        value = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0xD151) % np.uint64(MAX_DISTINCT)
                 ).astype(np.int64) + 1000000
        for k in range(7):
            a[begins + k] = 0x30 + (value // 10 ** (6 - k)) % 10
        a[begins + 7] = 0x20
    a[ends - 1] = 0x0A
    begins = begins[::every]
    p = np.frombuffer(piece, dtype=np.uint8)
    begins = begins[begins + len(p) < n]  # (a piece longer than its line runs into the next one)
    a[begins[:, None] + np.arange(len(p))[None, :]] = p[None, :]
    return a


def timed(fn):
    """milliseconds between two device events around fn(), and what it returned"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms, n):
    g = sorted(n / (m * 1e6) for m in ms)
    return {"median_GBps": g[len(g) // 2], "min_GBps": g[0], "max_GBps": g[-1]}


def plainly(fn):
    def run():
        os.environ["REDGPU_UNIQ_PLAIN"] = "1"
        try:
            return fn()
        finally:
            os.environ["REDGPU_UNIQ_PLAIN"] = "0"
    return run


for name in names:
    dfa = "num3" if name == "distinct1m" else name.split("_")[0]
    every = EVERY.get(name, 100)
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", dfa + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    if name == "distinct1m":
        host = make_text(b"", mib << 20, 1, numbers=True)
    else:
        host = make_text(PIECES[dfa], mib << 20, every)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    n_bins = exe.info["max_result"] + 1

    def uniq():
        return one_amd.uniq_text(exe, dev, max_distinct=MAX_DISTINCT)

    if profile:
        uniq()
        uniq()
        torch.cuda.synchronize()
        continue
    sized = one_amd.extract_text(exe, dev, out_cap=0)
    total, out_len = int(sized[1].item()), int(sized[2].item())

    def extract_sizes():
        return one_amd.extract_text(exe, dev, out_cap=0)

    def tally():
        return one_amd.tally_text(exe, dev, n_bins)

    def composed():
        got = one_amd.extract_text(exe, dev, out_cap=out_len)
        pieces = got[3][:out_len].cpu().numpy().tobytes().split(b"\n")
        pieces.pop()
        return collections.Counter(pieces)

    routes = {"uniq_text": uniq, "uniq_text_plain": plainly(uniq),
              "extract_text_sizes_only": extract_sizes, "tally_text": tally}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    ms["composed_extract_download_counter"] = []
    for _ in range(HOST_REPS):
        t, counter = host_timed(composed)
        ms["composed_extract_download_counter"].append(t)
    # every route counts the same things
    u, p = outs["uniq_text"], outs["uniq_text_plain"]
    n_lines, n_items, n_dropped, n_distinct = (int(t.item()) for t in u[:4])
    assert n_items == total == int(outs["tally_text"][1].item()) and n_dropped == 0
    assert all(torch.equal(a[:n_distinct] if a.numel() > 1 else a, b[:n_distinct] if b.numel() > 1 else b)
               for a, b in zip(u, p))
    assert n_distinct == len(counter) and int(u[6][:n_distinct].sum().item()) == total
    first, length, count = (t[:n_distinct].cpu().numpy() for t in u[4:])
    assert (np.diff(first) > 0).all()
    for j in list(range(min(n_distinct, 50))) + list(range(max(0, n_distinct - 50), n_distinct)):
        assert counter[host[first[j]:first[j] + length[j]].tobytes()] == count[j]
    row = {"input": name, "dfa": dfa, "mib": mib, "lines": n_lines, "items": n_items,
           "distinct": n_distinct, "every": every, "table_slots": 2 * MAX_DISTINCT,
           "load_factor": n_distinct / (2.0 * MAX_DISTINCT), "top_count": int(count.max()) if n_distinct else 0,
           "lds_slots": int(_lib.lib().redgpu_uniq_lds_slots(exe._h)),
           "pieces_bytes": out_len, "record_bytes": 24 * n_distinct}
    for k in ms:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    row["spread_uniq_text"] = (row["uniq_text"]["max_GBps"] - row["uniq_text"]["min_GBps"]) / med("uniq_text")
    row["ratio_uniq_to_extract_sizes"] = med("uniq_text") / med("extract_text_sizes_only")
    row["ratio_uniq_to_tally"] = med("uniq_text") / med("tally_text")
    row["ratio_uniq_to_plain"] = med("uniq_text") / med("uniq_text_plain")
    row["ratio_uniq_to_composed"] = med("uniq_text") / med("composed_extract_download_counter")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev
if not profile:
    with open(OUT, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in rows)
