"""GB/s of text per call of extract_text (grep -o's output as a text) over a raw text of
delimiter-terminated lines, all device-resident and alternated in one process:
  (a) redgpu_extract_text_dev, the sizes only (out_cap = 0);
  (b) redgpu_extract_text_dev with the output;
  (c) redgpu_collect_text_dev, the counts only - the yardstick for (a): the same walk;
  (d) the composed route a caller had before: redgpu_collect_text_dev with its records (room for
      exactly the matches: the route is GIVEN the count), then a torch gather of
      [end - piece length, end) and the delimiters.  For the open DFAs that is [start, end); for uri,
      whose pieces begin in front of the record's start, the route is also GIVEN the piece lengths
      (taken from (b)'s output outside the timing) - it has no way to them of its own;
  (e) (b) with the hand-off to the wave off (REDGPU_XT_HAND = 1 << 30): every piece through its
      lane's window.
bench_collect_text.py's texts: lines of 32..256 bytes of alphabet text joined by '\\n', the DFA's
piece at the start of every 100th line (about 1 %), or of every line for num3 ("dense": ~22 matches
in a line).  Device events around each call, the median of 10 after a warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/extract_text_<MiB>mib.jsonl.
usage: bench_extract_text.py [MiB] [--profile] [dfa ...]   (--profile: two calls of (a) and two of
(b) on the first DFA, nothing else - for a kernel trace)"""
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
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "extract_text_%dmib.jsonl" % mib)
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
    sizes = one_amd.extract_text(exe, dev, out_cap=0)
    total, out_len = int(sizes[1].item()), int(sizes[2].item())
    room = torch.empty(out_len + 16, dtype=torch.uint8, device=dev.device)

    def sizes_only():
        return one_amd.extract_text(exe, dev, out_cap=0)

    def with_output():
        return one_amd.extract_text(exe, dev, out=room)

    def without_hand_off():
        os.environ["REDGPU_XT_HAND"] = str(1 << 30)
        try:
            return one_amd.extract_text(exe, dev, out=room)
        finally:
            del os.environ["REDGPU_XT_HAND"]

    def collect_count():
        return one_amd.collect_text(exe, dev, cap=0)

    # what the composed route is given: the count, the output's length, and the piece lengths where
    # the records do not hold them
    first = with_output()
    torch.cuda.synchronize()
    text_out = first[3][:out_len]
    seps = torch.nonzero(text_out == 0x0A)[:, 0]
    given = torch.diff(seps, prepend=seps.new_full((1,), -1)) - 1  # piece lengths
    assert given.numel() == total
    rec = one_amd.collect_text(exe, dev, cap=total)
    torch.cuda.synchronize()
    loose = int((rec[6][:total] - rec[5][:total] != given).sum().item())
    del rec

    def composed():
        r = one_amd.collect_text(exe, dev, cap=total)
        end = r[6][:total]
        size = given if loose else end - r[5][:total]
        size1 = size + 1
        at = torch.cumsum(size1, 0) - size1
        piece = torch.repeat_interleave(torch.arange(total, device=dev.device), size1,
                                        output_size=out_len)
        pos = torch.arange(out_len, device=dev.device) - at[piece]
        sep = pos == size[piece]
        out = dev[((end - size)[piece] + pos).clamp_(max=n - 1)]
        out[sep] = 0x0A
        return out

    if profile:
        sizes_only(); sizes_only(); with_output(); with_output()
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"sizes_only": sizes_only, "with_output": with_output, "collect_count": collect_count,
              "composed": composed, "without_hand_off": without_hand_off}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    b = outs["with_output"]
    assert [int(v.item()) for v in b[:3]] == [int(v.item()) for v in outs["sizes_only"][:3]]
    assert int(b[1].item()) == total == int(outs["collect_count"][1].item())
    want = outs["composed"]
    assert torch.equal(b[3][:out_len], want), name
    assert torch.equal(outs["without_hand_off"][3][:out_len], want), name
    big = int((given >= 64).sum().item())
    row = {"dfa": name, "mib": mib, "lines": int(b[0].item()), "matches": total, "every": every,
           "out_len": out_len, "pieces_of_64_bytes_or_more": big,
           "pieces_in_front_of_start": loose,
           "extract_text_sizes_only": stats(ms["sizes_only"], n),
           "extract_text_with_output": stats(ms["with_output"], n),
           "extract_text_without_hand_off": stats(ms["without_hand_off"], n),
           "collect_text_count_only": stats(ms["collect_count"], n),
           "composed_collect_text_gather": stats(ms["composed"], n)}
    row["sizes_only_over_collect_count"] = (row["extract_text_sizes_only"]["median_GBps"] /
                                            row["collect_text_count_only"]["median_GBps"])
    row["with_output_over_composed"] = (row["extract_text_with_output"]["median_GBps"] /
                                        row["composed_collect_text_gather"]["median_GBps"])
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
