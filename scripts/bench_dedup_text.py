"""GB/s of text per call of dedup_text (awk '!seen[$k]++' of a raw text, as a text) over a raw text
of delimiter-terminated lines, all device-resident and alternated in one process, with num3's
numbers as the keys (MATCH, FIELD: as the separators) and letters-only lines around them:
  (a) the walk: redgpu_dedup_text_dev, the sizes only (out_cap = 0), per mode, beside
      redgpu_uniq_text_dev (cap = 0) on the same items - the walk this verb extends; what is new on
      top of it is the KEYED bit, the mark pass and the emit pass;
  (b) the output: redgpu_dedup_text_dev with the output, per mode, beside the composed route a
      caller had before: uniq_text_dev's records (given their number), a torch.searchsorted of
      first[] into the line ends, then a ragged gather of those lines in torch;
  (c) invert (every later duplicate) on its own: the composed route cannot produce it.
The regimes are uniq_text's: a key in 1 line of 100 (`sparse`), ONE hot key in every line (`hot`),
a key in every line drawn from about 65 K distinct numbers (`k65`) and from about 1 M (`m1`).
Lines of 32..256 bytes joined by '\\n' (bench_range_text.py's), the key " <number> " at the start of
every `every`-th line.  Device events around each call, the median of 10 after a warm-up call of
each route.  Pass / fail rests on exactness (tests/test_gpu_dedup_text.py), not on these rates.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/dedup_text_<MiB>mib.jsonl.
usage: bench_dedup_text.py [MiB] [regime ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import workloads as W

args = sys.argv[1:]
mib = int(args[0]) if args else 256
REGIMES = {"sparse": (100, 1 << 16), "hot": (1, 1), "k65": (1, 1 << 16), "m1": (1, 1 << 20)}
regimes = args[1:] or list(REGIMES)
name = "num3"
REPS = 10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "dedup_text_%dmib.jsonl" % mib)
rows = []


def make_text(n, every, distinct):
    """letters-only lines of 32..256 bytes (delimiter included); every `every`-th line begins with
    "<7 digits> ", the number one of `distinct`"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    n_lines = int(np.searchsorted(ends, n, side="right"))
    ends = ends[:n_lines]
    a = (W.splitmix64(np.arange(n, dtype=np.uint64), 0xA1FA) % np.uint64(26)).astype(np.uint8) + 97
    a[ends - 1] = 0x0A
    begins = np.concatenate([[0], ends[:-1]])[::every]
    which = (W.splitmix64(np.arange(len(begins), dtype=np.uint64), 0xD15C) % np.uint64(distinct)).astype(np.int64)
    digits = (1000000 + which)[:, None] // (10 ** np.arange(6, -1, -1))[None, :] % 10 + 0x30
    a[begins[:, None] + np.arange(7)[None, :]] = digits.astype(np.uint8)
    a[begins + 7] = 0x20
    return a, ends


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
for regime in regimes:
    every, distinct = REGIMES[regime]
    host, line_ends = make_text(mib << 20, every, distinct)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    d_ends = torch.from_numpy(line_ends).cuda()          # (given to the composed route)
    room = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    md = 1 << 22 if regime == "m1" else 1 << 18
    # (whole lines are all distinct, about 1.9 M of them, and num3 selects every keyed one)
    MODES = {"whole": dict(what="whole", max_distinct=1 << 22), "lines": dict(what="lines", max_distinct=1 << 22),
             "match": dict(what="match", max_distinct=md),
             # (field 1 of a line without a number is the whole line: as many strings as "whole")
             "field": dict(what="field", max_distinct=1 << 22)}
    got = one_amd.dedup_text(exe, dev, out_cap=0, **MODES["match"])
    n_lines, n_keyed, n_distinct, n_dropped, n_emitted, out_len = (int(got[k].item()) for k in range(6))
    assert n_dropped == 0 and n_emitted == n_distinct
    for mode, kw in MODES.items():      # no mode times an overflowing table
        sized = one_amd.dedup_text(exe, dev, out_cap=0, **kw)
        assert int(sized[3].item()) == 0, (regime, mode, int(sized[3].item()))
    sized = one_amd.uniq_text(exe, dev, matches=False, max_distinct=1 << 22, cap=0)
    assert int(sized[2].item()) == 0, regime

    def composed():
        got = one_amd.uniq_text(exe, dev, max_per_line=1, max_distinct=md, cap=n_distinct)
        first = got[4][:n_distinct]
        line = torch.searchsorted(d_ends, first, right=True)       # the line each first[] lies in
        last = d_ends[line]
        begin = torch.where(line > 0, d_ends[torch.clamp(line - 1, min=0)], torch.zeros_like(last))
        lens = last - begin
        at = torch.cumsum(lens, 0) - lens
        src = torch.repeat_interleave(begin - at, lens, output_size=out_len)
        return dev[src + torch.arange(out_len, device="cuda")]

    routes = {"uniq_text_matches_cap0": lambda: one_amd.uniq_text(exe, dev, max_per_line=1, max_distinct=md, cap=0),
              "uniq_text_lines_cap0": lambda: one_amd.uniq_text(exe, dev, matches=False, max_distinct=1 << 22, cap=0),
              "composed_match": composed}
    for mode, kw in MODES.items():
        routes["sizes_only_" + mode] = lambda kw=kw: one_amd.dedup_text(exe, dev, out_cap=0, **kw)
        routes["with_output_" + mode] = lambda kw=kw: one_amd.dedup_text(exe, dev, out=room, **kw)
    routes["with_output_match_invert"] = lambda: one_amd.dedup_text(exe, dev, out=room, invert=True,
                                                                    **MODES["match"])
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    # the composed output is the same bytes
    one_amd.dedup_text(exe, dev, out=room, **MODES["match"])
    torch.cuda.synchronize()
    assert torch.equal(room[:out_len], outs["composed_match"]), regime
    row = {"dfa": name, "mib": mib, "regime": regime, "lines": n_lines, "keyed": n_keyed,
           "distinct": n_distinct, "emitted": n_emitted, "out_len": out_len}
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    row["ratio_sizes_only_match_to_uniq_text"] = med("sizes_only_match") / med("uniq_text_matches_cap0")
    row["ratio_sizes_only_lines_to_uniq_text"] = med("sizes_only_lines") / med("uniq_text_lines_cap0")
    row["ratio_with_output_match_to_composed"] = med("with_output_match") / med("composed_match")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room, outs
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
