"""GB/s of text per call of range_text (sed's /open/,/close/ line ranges of a raw text, as a text)
over a raw text of delimiter-terminated lines, all device-resident and alternated in one process,
with two of log100's results as open and close:
  (a) redgpu_range_text_dev, the sizes only (out_cap = 0);
  (b) redgpu_range_text_dev with the output: the whole ranges (both flags set), and the ranges
      without their close lines (emit_close = False);
  (c) redgpu_route_text_dev, the sizes only, with n_bins = 101: the line index and the same walk
      with plane stores - what this verb adds on top is the range bookkeeping;
  (d) the composed route a caller had before: grep_text_dev's line / begin / finish / result
      records (the cap, the output size and where the last line ends taken from counts the caller is
      GIVEN here - a caller who has to find them pays a walk and a read-back on top), a DOWNLOAD of
      the records, the two-state machine over the events in numpy on the host, an upload of the
      ranges' begins and lengths, then a ragged gather in torch (repeat_interleave, an index per
      output byte).  It produces the whole ranges, (b)'s first form.
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_route_text.py's), the open head and
the close head in turn at the start of every 100th line (sparse: 1 line in 100 an event, ranges of
about 100 lines) or of every line (dense: every line an event, ranges of two lines - without their
close lines every run of the write pass is ONE line, its weakest case).  Device events around each
call - the composed route's download and host work lie between them - the median of 10 after a
warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/range_text_<MiB>mib.jsonl.
usage: bench_range_text.py [MiB] [--profile] [every ...]   (--profile: two calls of (a) and two of
(b)'s first form at the first `every`, nothing else - for a kernel trace)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import workloads as W

args = [a for a in sys.argv[1:] if a != "--profile"]
profile = "--profile" in sys.argv[1:]
mib = int(args[0]) if args else 256
everies = [int(a) for a in args[1:]] or [100, 1]
name = "log100"
OPEN_HEAD, CLOSE_HEAD = 11, 42
REPS = 10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "range_text_%dmib.jsonl" % mib)
rows = []


def make_text(pieces, n, every):
    """lines of 32..256 bytes (delimiter included), pieces[k % len] at the start of the k-th of every
    `every`-th line"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    n_lines = int(np.searchsorted(ends, n, side="right"))
    ends = ends[:n_lines]
    a = W.alphabet_bytes(n, 1).copy()
    a[a == 0x0A] = 0x20
    a[ends - 1] = 0x0A
    begins = np.concatenate([[0], ends[:-1]])[::every]
    room = lens[:n_lines][::every] - 1  # the line without its delimiter
    for k, piece in enumerate(pieces):
        p = np.frombuffer(piece, dtype=np.uint8)
        at = begins[k::len(pieces)]
        at = at[room[k::len(pieces)] >= len(p)]  # (a line too short for its piece stays bare)
        a[at[:, None] + np.arange(len(p))[None, :]] = p[None, :]
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


blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
exe = one_amd.Executable(blob)
n_bins = exe.info["max_result"] + 1
style, lead = one_amd.styInstant, True
heads = W.log100_heads()
# the two results, from the verb itself: a line with the head alone is one range in toggle form
results = []
for h in (heads[OPEN_HEAD], heads[CLOSE_HEAD]):
    probe = torch.from_numpy(np.frombuffer(h + b"x\n", dtype=np.uint8).copy()).cuda()
    got = one_amd.route_text(exe, probe, n_bins, style, lead, out_cap=0)
    results.append(int(torch.nonzero(got[2])[0].item()))
o, c = results
assert o != c and o >= 1 and c >= 1
for every in everies:
    host = make_text([heads[OPEN_HEAD], heads[CLOSE_HEAD]], mib << 20, every)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    got = one_amd.range_text(exe, dev, o, c, style, lead, out_cap=0, rec_cap=1)
    n_lines, n_ranges, n_emitted, out_len = (int(got[k].item()) for k in range(4))
    got = one_amd.range_text(exe, dev, o, c, style, lead, invert=True, out_cap=0)
    text_end = out_len + int(got[3].item())       # the position behind the last delimiter
    matched = int(one_amd.grep_text(exe, dev, style, lead, cap=0)[1].item())
    room = torch.empty(out_len + 16, dtype=torch.uint8, device="cuda")

    def sizes_only():
        return one_amd.range_text(exe, dev, o, c, style, lead, out_cap=0)

    def with_output(emit_close=True):
        return one_amd.range_text(exe, dev, o, c, style, lead, emit_close=emit_close, out=room)

    def route_sizes():
        return one_amd.route_text(exe, dev, n_bins, style, lead, out_cap=0)

    def composed():
        got = one_amd.grep_text(exe, dev, style, lead, cap=matched)
        begin, fin, res = (got[k].cpu().numpy() for k in (3, 4, 5))      # the read-back
        ev = np.flatnonzero((res == o) | (res == c))
        is_open = res[ev] == o
        prev_open = np.concatenate([[False], is_open[:-1]])
        starts, ends = ev[is_open & ~prev_open], ev[~is_open & prev_open]
        first = begin[starts].astype(np.int64)
        last = fin[ends].astype(np.int64) + 1
        if len(last) < len(first):                                      # a range nothing closes
            last = np.concatenate([last, [text_end]])
        d_first = torch.from_numpy(first).cuda()
        lens = torch.from_numpy(last - first).cuda()
        at = torch.cumsum(lens, 0) - lens  # where each range goes
        src = torch.repeat_interleave(d_first - at, lens, output_size=out_len)
        return dev[src + torch.arange(out_len, device="cuda")]

    if profile:
        for f in (sizes_only, sizes_only, with_output, with_output):
            f()
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"route_text_sizes_only": route_sizes, "sizes_only": sizes_only,
              "with_output": with_output, "with_output_no_close": lambda: with_output(False),
              "composed": composed}
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    # every route sees the same lines, and the composed output is the same bytes
    counts = [n_lines, n_ranges, n_emitted, out_len]
    assert [int(outs["sizes_only"][k].item()) for k in range(4)] == counts, every
    assert int(outs["route_text_sizes_only"][0].item()) == n_lines
    no_close = [int(outs["with_output_no_close"][k].item()) for k in range(4)]
    with_output()
    assert torch.equal(room[:out_len], outs["composed"]), every
    row = {"dfa": name, "mib": mib, "open_result": o, "close_result": c, "every": every,
           "lines": n_lines, "matched": matched, "ranges": n_ranges, "emitted": n_emitted,
           "out_len": out_len, "emitted_no_close": no_close[2], "out_len_no_close": no_close[3]}
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    for k in ("sizes_only", "with_output", "with_output_no_close"):
        row["ratio_%s_to_route_text_sizes_only" % k] = med(k) / med("route_text_sizes_only")
        row["ratio_%s_to_composed" % k] = med(k) / med("composed")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room, outs
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
