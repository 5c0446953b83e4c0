"""GB/s of text per call of filter_text (grep's output with -A / -B context, as a text) over a raw
text of delimiter-terminated lines, all device-resident and alternated in one process, at the
contexts (before, after) = (0, 0) and (2, 2):
  (a) redgpu_filter_text_dev, the sizes only (out_cap = 0);
  (b) redgpu_filter_text_dev with the output;
  (c) redgpu_grep_text_dev with cap = 0: the line index and the select pass alone - the floor this
      verb cannot beat, since it runs the same kernels first;
  (d) the composed route a caller had before, at (0, 0) only (it has no context form):
      grep_text_dev's begin / finish records (the cap and the output size taken from counts the
      caller is GIVEN here - a caller who has to find them pays (c) and a read-back on top), then a
      ragged gather in torch (repeat_interleave over finish - begin + 1, an index per output byte).
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_tally_text.py's), the DFA's piece at
the start of every 100th line (about 1 %), or of every line for num3.  Device events around each
call, the median of 10 after a warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/filter_text_<MiB>mib.jsonl.
usage: bench_filter_text.py [MiB] [--profile] [dfa ...]   (--profile: two calls of (a) and two of
(b) at (2, 2) on the first DFA, nothing else - for a kernel trace)"""
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
CONTEXTS = ((0, 0), (2, 2))
REPS = 10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "filter_text_%dmib.jsonl" % mib)
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
    every = EVERY.get(name, 100)
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    host = make_text(PIECES[name], mib << 20, every)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    style, lead = one_amd.styInstant, True
    sizes = {}
    for ctx in CONTEXTS:
        got = one_amd.filter_text(exe, dev, style, lead, before=ctx[0], after=ctx[1], out_cap=0)
        sizes[ctx] = [int(x.item()) for x in got[:4]]
    n_lines, selected, _, plain_len = sizes[(0, 0)]
    room = torch.empty(max(s[3] for s in sizes.values()) + 16, dtype=torch.uint8, device="cuda")

    def sizes_only(ctx):
        return one_amd.filter_text(exe, dev, style, lead, before=ctx[0], after=ctx[1], out_cap=0)

    def with_output(ctx):
        return one_amd.filter_text(exe, dev, style, lead, before=ctx[0], after=ctx[1], out=room)

    def grep_count():
        return one_amd.grep_text(exe, dev, style, lead, cap=0)

    def composed():
        got = one_amd.grep_text(exe, dev, style, lead, cap=selected, want_outcome=False)
        begin, lens = got[3], got[4] - got[3] + 1
        first = torch.cumsum(lens, 0) - lens  # where each line goes
        src = torch.repeat_interleave(begin - first, lens, output_size=plain_len)
        return got[0], got[1], dev[src + torch.arange(plain_len, device="cuda")]

    if profile:
        for f in (sizes_only, sizes_only, with_output, with_output):
            f((2, 2))
        torch.cuda.synchronize()
        sys.exit(0)
    routes = {"grep_text_count_only": grep_count, "composed_grep_gather_0_0": composed}
    for ctx in CONTEXTS:
        routes["sizes_only_%d_%d" % ctx] = lambda ctx=ctx: sizes_only(ctx)
        routes["with_output_%d_%d" % ctx] = lambda ctx=ctx: with_output(ctx)
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    # every route selects the same lines, and the two (0, 0) outputs are the same bytes
    assert int(outs["grep_text_count_only"][1].item()) == selected
    for ctx in CONTEXTS:
        for form in ("sizes_only_%d_%d", "with_output_%d_%d"):
            assert [int(x.item()) for x in outs[form % ctx][:4]] == sizes[ctx], (name, ctx, form)
    with_output((0, 0))
    assert torch.equal(room[:plain_len], outs["composed_grep_gather_0_0"][2])
    row = {"dfa": name, "mib": mib, "lines": n_lines, "selected": selected, "every": every}
    for ctx in CONTEXTS:
        row["emitted_%d_%d" % ctx] = sizes[ctx][2]
        row["out_len_%d_%d" % ctx] = sizes[ctx][3]
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    for ctx in CONTEXTS:
        row["ratio_sizes_only_%d_%d_to_grep_count" % ctx] = med("sizes_only_%d_%d" % ctx) / med("grep_text_count_only")
        row["ratio_with_output_%d_%d_to_grep_count" % ctx] = med("with_output_%d_%d" % ctx) / med("grep_text_count_only")
    row["ratio_with_output_0_0_to_composed"] = med("with_output_0_0") / med("composed_grep_gather_0_0")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room, outs
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
