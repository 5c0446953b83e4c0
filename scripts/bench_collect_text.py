"""GB/s of text per call of grep -o over a raw text of delimiter-terminated lines, all
device-resident and alternated in one process:
  (a) redgpu_collect_text_dev, the counts only;
  (b) redgpu_collect_text_dev with all records;
  (c) redgpu_grep_text_dev(styLast, no leader), the count only - the yardstick for the walk: both
      verbs drive the same lines, grep stops at a line's first match, collect goes on through it;
  (d) the composed route a caller had before: split_lines on the device, the line count read back,
      collect_batch on the device with cap = 8 records per line, a torch compaction.
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_grep_text.py's), the DFA's piece at
the start of every 100th line (about 1 %), or of every line for num3 ("dense").  Device events
around each call, the median of 10 after a warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/collect_text_<MiB>mib.jsonl.
usage: bench_collect_text.py [MiB] [--profile] [dfa ...]   (--profile: two calls of (b) on the
first DFA, nothing else - for a kernel trace)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import workloads as W

args = [a for a in sys.argv[1:] if a != "--profile"]
profile = "--profile" in sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["log100", "err", "uri", "num3"]
PIECES = {"err": b"error", "log100": W.log100_heads()[7], "uri": W.URI_PLANT.rstrip(),
          "num3": b"12345a"}
EVERY = {"num3": 1}
REPS = 10
LINE_CAP = 8
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "collect_text_%dmib.jsonl" % mib)
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


def timed(fn):
    """milliseconds between two device events around fn(), and what it returned"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def stats(ms, n):
    g = sorted(n / (m * 1e6) for m in ms)
    return {"median_GBps": g[len(g) // 2], "min_GBps": g[0], "max_GBps": g[-1]}


for name in names:
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    every = EVERY.get(name, 100)
    host = make_text(PIECES[name], mib << 20, every)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    room_lines = n // 32 + 1  # what a caller who does not know the line count makes room for
    total = int(one_amd.collect_text(exe, dev, cap=0)[1].item())
    room = total + 16

    def count_only():
        return one_amd.collect_text(exe, dev, cap=0)

    def all_records():
        return one_amd.collect_text(exe, dev, cap=room)

    def grep_count():
        return one_amd.grep_text(exe, dev, one_amd.styLast, False, cap=0)

    def composed():
        offs, cnt = one_amd.split_lines(exe, dev, cap=room_lines)
        k = int(cnt.item())  # the host waits for the split
        counts, r, s, e = one_amd.collect_batch(exe, dev, LINE_CAP, offsets=offs[:k + 1], stride=1)
        kept = counts.clamp(max=LINE_CAP)
        keep = torch.arange(LINE_CAP, device=dev.device)[None, :] < kept[:, None]
        line = torch.nonzero(keep)[:, 0]
        begin = offs[line]
        return k, counts, line, begin, r[keep], s[keep] + begin, e[keep] + begin

    if profile:
        all_records(); all_records()
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"count_only": count_only, "all_records": all_records, "grep_count": grep_count,
              "composed": composed}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    b, d = outs["all_records"], outs["composed"]
    n_lines = int(b[0].item())
    assert n_lines == d[0] and int(b[1].item()) == total == int(outs["count_only"][1].item())
    cut = int((d[1] > LINE_CAP).sum().item())  # lines the composed route cut at its per-line cap
    if cut == 0:
        for x, y in zip(b[2:], d[2:]):
            assert torch.equal(x[:total], y.to(x.dtype)), name
    row = {"dfa": name, "mib": mib, "lines": n_lines, "matches": total, "every": every,
           "lines_cut_by_composed_cap": cut,
           "collect_text_count_only": stats(ms["count_only"], n),
           "collect_text_all_records": stats(ms["all_records"], n),
           "grep_text_count_only_last_nolead": stats(ms["grep_count"], n),
           "composed_dev_cap8": stats(ms["composed"], n)}
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
