"""GB/s of text per call of sed over a raw text of delimiter-terminated lines, all device-resident
and alternated in one process:
  (a) redgpu_replace_text_dev, the sizes only;
  (b) redgpu_replace_text_dev with the output;
  (c) (b) under only_changed;
  (d) the composed route a caller had before: split_lines on the device, the line count read back,
      replace_batch on the device, sizes plus bytes (its output has no delimiters and no tail; that
      is noted, not corrected for);
  (e) redgpu_collect_text_dev, the counts only - the yardstick for the walk;
  (f) out.copy_(text) - the roof of the assembly.
styLast, repl = b"<#>", every match.  Lines of 32..256 bytes of alphabet text joined by '\\n'
(bench_collect_text.py's), the DFA's piece at the start of every 100th line (about 1 %), or of
every line for num3 ("dense").  Device events around each call, the median of 10 after a warm-up
call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/replace_text_<MiB>mib.jsonl.
usage: bench_replace_text.py [MiB] [--profile] [dfa ...]   (--profile: two calls of (b) on the
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
REPL = b"<#>"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "replace_text_%dmib.jsonl" % mib)
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
    drepl = torch.from_numpy(np.frombuffer(REPL, dtype=np.uint8).copy()).cuda()
    room_lines = n // 32 + 1  # what a caller who does not know the line count makes room for
    sizes = one_amd.replace_text(exe, dev, drepl, out_cap=0)
    n_lines, n_replaced, out_len = (int(x.item()) for x in sizes[:3])
    changed_len = int(one_amd.replace_text(exe, dev, drepl, only_changed=True, out_cap=0)[2].item())
    out = torch.empty(out_len + 64, dtype=torch.uint8, device="cuda")
    out_changed = torch.empty(changed_len + 64, dtype=torch.uint8, device="cuda")
    out_batch = torch.empty(out_len + 64, dtype=torch.uint8, device="cuda")
    roof = torch.empty_like(dev)

    def sizes_only():
        return one_amd.replace_text(exe, dev, drepl, out_cap=0)

    def with_output():
        return one_amd.replace_text(exe, dev, drepl, out=out)

    def only_changed():
        return one_amd.replace_text(exe, dev, drepl, only_changed=True, out=out_changed)

    def composed():
        offs, cnt = one_amd.split_lines(exe, dev, cap=room_lines)
        k = int(cnt.item())  # the host waits for the split
        counts, ooff, o = one_amd.replace_batch(exe, dev, REPL, one_amd.styLast, True, offsets=offs[:k + 1],
                                                stride=1, out=out_batch)
        return k, counts, ooff, o

    def collect_count():
        return one_amd.collect_text(exe, dev, cap=0)

    def copy():
        return roof.copy_(dev)

    if profile:
        with_output(); with_output()
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"sizes_only": sizes_only, "with_output": with_output, "only_changed": only_changed,
              "composed": composed, "collect_count": collect_count, "copy": copy}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    b, d = outs["with_output"], outs["composed"]
    assert [int(x.item()) for x in b[:3]] == [n_lines, n_replaced, out_len] and d[0] == n_lines
    assert int(d[1].sum().item()) == n_replaced
    # the composed route's bytes are the verb's without the delimiters (and without the tail)
    mine = b[3][:out_len]
    tail = n - int(torch.nonzero(dev == 0x0A)[-1].item()) - 1
    keep = torch.ones(out_len, dtype=torch.bool, device="cuda")
    keep[(d[2][1:n_lines + 1] + torch.arange(n_lines, device="cuda")).long()] = False
    if tail:
        keep[out_len - tail:] = False
    assert torch.equal(mine[keep], d[3][:int(d[2][n_lines].item())]), name
    del keep, mine
    row = {"dfa": name, "mib": mib, "lines": n_lines, "replacements": n_replaced, "every": every,
           "out_len": out_len, "out_len_only_changed": changed_len,
           "replace_text_sizes_only": stats(ms["sizes_only"], n),
           "replace_text_with_output": stats(ms["with_output"], n),
           "replace_text_only_changed": stats(ms["only_changed"], n),
           "composed_dev_no_delimiters": stats(ms["composed"], n),
           "collect_text_count_only": stats(ms["collect_count"], n),
           "copy_text": stats(ms["copy"], n)}
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, out, out_changed, out_batch, roof
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
