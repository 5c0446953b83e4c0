"""GB/s of text per call of grep over a raw text of delimiter-terminated lines: redgpu_grep_text_dev
(a) against the composed device route a caller had before it (b: split_lines on the device, the
line count read back, search_batch on the device, torch.nonzero and gathers), alternated in one
process; and both host forms (c: redgpu_grep_text against split_lines + search_batch + a numpy
filter).  Lines of 32..256 bytes of alphabet text joined by '\\n', the DFA's piece at the start of
every 100th (about 1 %) or every 2nd (about 50 %) line; styInstant with the leader.  Wall-clock
per call behind a device synchronisation (route b waits on the host by construction).
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/grep_text_<MiB>mib.jsonl.
usage: bench_grep_text.py [MiB] [--profile] [dfa ...]   (--profile: two calls of (a) and of
(b) on the first DFA at 1 %, nothing else - for a kernel trace)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import workloads as W

args = [a for a in sys.argv[1:] if a != "--profile"]
profile = "--profile" in sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["err", "log100", "uri"]
PIECES = {"err": b"error", "log100": W.log100_heads()[7], "uri": W.URI_PLANT.rstrip()}
STYLE, LEAD = one_amd.styInstant, True
REPS = 5
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "grep_text_%dmib.jsonl" % mib)
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


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def stats(ms, n):
    g = sorted(n / (m * 1e6) for m in ms)
    return {"median_GBps": g[len(g) // 2], "min_GBps": g[0], "max_GBps": g[-1]}


for name in names:
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    for every in (100, 2):
        host = make_text(PIECES[name], mib << 20, every)
        n = host.size
        dev = torch.from_numpy(host).cuda()
        room = n // 32 + 1  # what a caller who does not know the line count makes room for

        def grep_dev():
            return one_amd.grep_text(exe, dev, STYLE, LEAD, cap=room)

        def composed_dev():
            offs, cnt = one_amd.split_lines(exe, dev, cap=room)
            k = int(cnt.item())  # the host waits for the split
            r, s, e = one_amd.search_batch(exe, dev, STYLE, LEAD, offsets=offs[:k + 1], stride=1)
            idx = torch.nonzero(r > 0).squeeze(1)
            return k, idx, offs[idx], offs[idx + 1] - 1, r[idx], s[idx], e[idx]

        if profile:
            grep_dev(); grep_dev(); composed_dev(); composed_dev()
            torch.cuda.synchronize()
            sys.exit(0)
        grep_dev(); composed_dev()
        a_ms, b_ms = [], []
        for _ in range(REPS):
            ms, ga = wall(grep_dev)
            a_ms.append(ms)
            ms, gb = wall(composed_dev)
            b_ms.append(ms)
        route_b = one_amd.last_kernel()
        k = int(ga[1].item())
        n_lines = int(ga[0].item())
        assert n_lines == gb[0] and k == gb[1].numel()
        for x, y in zip(ga[2:], gb[1:]):
            assert torch.equal(x[:k], y.to(x.dtype)), name
        # the count alone (grep -c)
        c_ms = [wall(lambda: one_amd.grep_text(exe, dev, STYLE, LEAD, cap=0))[0] for _ in range(REPS)]

        def grep_host():
            return one_amd.grep_text(exe, host, STYLE, LEAD, cap=room)

        def composed_host():
            offs, _ = one_amd.split_lines(exe, host)
            r, s, e = one_amd.search_batch(exe, host, STYLE, LEAD, offsets=offs, stride=1)
            idx = np.flatnonzero(r > 0)
            return idx, offs[idx], offs[idx + 1] - 1, r[idx], s[idx], e[idx]

        grep_host(); composed_host()
        ha_ms, hb_ms = [], []
        for _ in range(3):
            ms, ha = wall(grep_host)
            ha_ms.append(ms)
            ms, hb = wall(composed_host)
            hb_ms.append(ms)
        assert ha[1] == k and all(np.array_equal(x, y.astype(x.dtype)) for x, y in zip(ha[2:], hb))
        row = {"dfa": name, "mib": mib, "lines": n_lines, "selected": k, "every": every,
               "grep_dev": stats(a_ms, n), "composed_dev": stats(b_ms, n), "composed_route": route_b,
               "grep_dev_count_only": stats(c_ms, n), "grep_host": stats(ha_ms, n),
               "composed_host": stats(hb_ms, n)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del dev
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
