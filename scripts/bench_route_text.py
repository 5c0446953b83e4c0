"""GB/s of text per call of route_text (a raw text's lines grouped by result, as a text) over a raw
text of delimiter-terminated lines, all device-resident and alternated in one process, with
n_bins = max_result + 1 (every result its own bucket):
  (a) redgpu_route_text_dev, the sizes only (out_cap = 0);
  (b) redgpu_route_text_dev with the output, all lines and under drop_unmatched;
  (c) redgpu_tally_text_dev LINES with the same n_bins: the line index and the walk alone - the
      floor this verb cannot beat, since its class pass is the same walk;
  (d) the composed route a caller had before: grep_text_dev's begin / finish / result records (the
      cap and the output size taken from counts the caller is GIVEN here - a caller who has to find
      them pays a walk and a read-back on top), a stable torch sort by bucket, then a ragged gather
      in torch (repeat_interleave over finish - begin + 1, an index per output byte).  Under
      drop_unmatched that is one grep_text call; with all lines it needs the lines that do not match
      as well, a second call under invert.
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_tally_text.py's), a piece at the
start of every 100th line (about 1 %) or of every line, the pieces going round the DFA's
signatures (log100: all 100), so that neighbouring planted lines never share a bucket - with every
line planted each run of the write pass is ONE line, its weakest case.  Device events around each
call, the median of 10 after a warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/route_text_<MiB>mib.jsonl.
usage: bench_route_text.py [MiB] [--profile] [every ...]   (--profile: two calls of
(a) and two of (b) at the first `every`, nothing else - for a kernel trace)"""
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
REPS = 10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "route_text_%dmib.jsonl" % mib)
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
for every in everies:
    host = make_text(W.log100_heads(), mib << 20, every)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    sizes = {}
    for drop in (False, True):
        got = one_amd.route_text(exe, dev, n_bins, style, lead, drop_unmatched=drop, out_cap=0)
        sizes[drop] = [int(got[k].item()) for k in (0, 1, 4)]
    n_lines, matched, all_len = sizes[False][0], sizes[True][1], sizes[False][2]
    room = torch.empty(all_len + 16, dtype=torch.uint8, device="cuda")

    def sizes_only(drop):
        return one_amd.route_text(exe, dev, n_bins, style, lead, drop_unmatched=drop, out_cap=0)

    def with_output(drop):
        return one_amd.route_text(exe, dev, n_bins, style, lead, drop_unmatched=drop, out=room)

    def tally():
        return one_amd.tally_text(exe, dev, n_bins, matches=False, style=style, do_leader=lead)

    def composed(drop):
        got = one_amd.grep_text(exe, dev, style, lead, cap=matched)
        begin, fin, res = got[3], got[4], got[5].to(torch.int64)
        if not drop:
            no = one_amd.grep_text(exe, dev, style, lead, invert=True, cap=n_lines - matched,
                                   want_outcome=False)
            begin, fin = torch.cat([no[3], begin]), torch.cat([no[4], fin])
            res = torch.cat([torch.zeros_like(no[3], dtype=torch.int64), res])
        bucket = torch.where(res < n_bins, res, torch.full_like(res, n_bins))
        order = torch.sort(bucket, stable=True)[1]
        begin, lens = begin[order], (fin - begin + 1)[order]
        total = sizes[drop][2]
        first = torch.cumsum(lens, 0) - lens  # where each line goes
        src = torch.repeat_interleave(begin - first, lens, output_size=total)
        return dev[src + torch.arange(total, device="cuda")]

    if profile:
        for f in (sizes_only, sizes_only, with_output, with_output):
            f(False)
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"tally_text_lines": tally}
    for drop in (False, True):
        tag = "drop" if drop else "all"
        routes["sizes_only_" + tag] = lambda drop=drop: sizes_only(drop)
        routes["with_output_" + tag] = lambda drop=drop: with_output(drop)
        routes["composed_" + tag] = lambda drop=drop: composed(drop)
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    # every route sees the same lines, and the composed outputs are the same bytes
    for drop in (False, True):
        tag = "drop" if drop else "all"
        for form in ("sizes_only_", "with_output_"):
            assert [int(outs[form + tag][k].item()) for k in (0, 1, 4)] == sizes[drop], (every, form, tag)
        assert torch.equal(outs["sizes_only_" + tag][2], outs["tally_text_lines"][2])
        with_output(drop)
        assert torch.equal(room[:sizes[drop][2]], outs["composed_" + tag]), (every, tag)
    row = {"dfa": name, "mib": mib, "n_bins": n_bins, "every": every, "lines": n_lines,
           "matched": matched, "out_len_all": all_len, "out_len_drop": sizes[True][2]}
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    for tag in ("all", "drop"):
        row["ratio_sizes_only_%s_to_tally" % tag] = med("sizes_only_" + tag) / med("tally_text_lines")
        row["ratio_with_output_%s_to_tally" % tag] = med("with_output_" + tag) / med("tally_text_lines")
        row["ratio_with_output_%s_to_composed" % tag] = med("with_output_" + tag) / med("composed_" + tag)
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room, outs
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
