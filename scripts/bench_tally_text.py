"""GB/s of text per call of tally_text (grep -c per result / grep -o | sort | uniq -c) over a raw
text of delimiter-terminated lines, all device-resident and alternated in one process:
  (a) redgpu_tally_text_dev, MATCHES and LINES (styInstant, leader), n_bins = max_result + 1;
  (b) the same with REDGPU_TALLY_PLAIN=1: an atomic per item, no ballot, no peel, no run lengths;
  (c) the walk without the tally: redgpu_collect_text_dev with cap = 0 (MATCHES) and
      redgpu_grep_text_dev with cap = 0 (LINES) - the same lines, the same lane functions, plus a
      hit / selected bitmap and a count scan, minus the histogram;
  (d) the composed route a caller had before: collect_text_dev with every record (the cap taken
      from a count the caller is GIVEN here - a caller who has to find it pays (c) on top), then
      torch.bincount over result;
  (e) on log100, n_bins = 101 against n_bins = 100001, and the share of the items that are counted
      in LDS (the items whose slot is below redgpu_tally_lds_bins, from the bins themselves).
Lines of 32..256 bytes of alphabet text joined by '\\n' (bench_collect_text.py's), the DFA's piece at
the start of every 100th line (about 1 %), or of every line for num3 and err_dense.  letters4 is
the counters in GLOBAL memory under load: the same line ends over random letters of "abcd.", a DFA
(oracle.reda_writer) that reports every a / b / c / d as a match of its own with the results
L - 1, L, L + 1 and 70000 (L = redgpu_tally_lds_bins), so three items in four are 64-bit global
atomics on three addresses.  Device events
around each call, the median of 10 after a warm-up call of each route.
Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/tally_text_<MiB>mib.jsonl.
usage: bench_tally_text.py [MiB] [input ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import _lib
from one_amd import workloads as W
from oracle import reda_writer

args = sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["log100", "err", "uri", "num3", "err_dense", "letters4"]
PIECES = {"err": b"error", "log100": W.log100_heads()[7], "uri": W.URI_PLANT.rstrip(),
          "num3": b"12345a"}
EVERY = {"num3": 1, "err_dense": 1}
REPS = 10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                   "tally_text_%dmib.jsonl" % mib)
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


def four_letters(results):
    """error, initial, and one accepting state per letter a / b / c / d"""
    equiv = np.full(256, 4, dtype=np.uint8)
    for k, ch in enumerate(b"abcd"):
        equiv[ch] = k
    trans = np.zeros((6, 5), dtype=np.int64)
    trans[1] = [2, 3, 4, 5, 0]
    return reda_writer.write_reda(trans, [0, 0] + list(results), equiv=equiv)


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


def plainly(fn):
    def run():
        os.environ["REDGPU_TALLY_PLAIN"] = "1"
        try:
            return fn()
        finally:
            os.environ["REDGPU_TALLY_PLAIN"] = "0"
    return run


for name in names:
    dfa = name.split("_")[0]
    every = EVERY.get(name, 100)
    if name == "letters4":
        probe = one_amd.Executable(four_letters((1, 2, 3, 4)), device="none")
        L = int(_lib.lib().redgpu_tally_lds_bins(probe._h))
        exe = one_amd.Executable(four_letters((L - 1, L, L + 1, 70000)))
        host = make_text(b"", mib << 20, 1)
        ends = host == 0x0A
        host = np.frombuffer(b"abcd.", dtype=np.uint8)[
            np.random.default_rng(7).integers(0, 5, host.size)].copy()
        host[ends] = 0x0A
    else:
        blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", dfa + ".reda"), "rb").read()
        exe = one_amd.Executable(blob)
        host = make_text(PIECES[dfa], mib << 20, every)
    lds_bins = int(_lib.lib().redgpu_tally_lds_bins(exe._h))
    n = host.size
    dev = torch.from_numpy(host).cuda()
    n_bins = exe.info["max_result"] + 1
    total = int(one_amd.collect_text(exe, dev, cap=0)[1].item())
    room = total + 16
    style, lead = one_amd.styInstant, True

    def tally_matches(nb=n_bins):
        return one_amd.tally_text(exe, dev, nb)

    def tally_lines():
        return one_amd.tally_text(exe, dev, n_bins, matches=False, style=style, do_leader=lead)

    def collect_count():
        return one_amd.collect_text(exe, dev, cap=0)

    def grep_count():
        return one_amd.grep_text(exe, dev, style, lead, cap=0)

    def composed():
        got = one_amd.collect_text(exe, dev, cap=room, want_positions=False)
        return got[0], got[1], torch.bincount(got[4][:total], minlength=n_bins + 1)

    routes = {"tally_matches": tally_matches, "tally_lines": tally_lines,
              "tally_matches_plain": plainly(tally_matches), "tally_lines_plain": plainly(tally_lines),
              "collect_text_count_only": collect_count, "grep_text_count_only": grep_count,
              "composed_collect_bincount": composed}
    if name == "log100":
        routes["tally_matches_100001_bins"] = lambda: tally_matches(100001)
    outs = {k: f() for k, f in routes.items()}  # warm-up
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    # every route counts the same things
    m, l, c = outs["tally_matches"], outs["tally_lines"], outs["composed_collect_bincount"]
    n_lines = int(m[0].item())
    assert int(m[1].item()) == total == int(outs["collect_text_count_only"][1].item())
    assert torch.equal(m[2], c[2]) and int(m[2].sum().item()) == total
    assert torch.equal(m[2], outs["tally_matches_plain"][2]) and torch.equal(l[2], outs["tally_lines_plain"][2])
    selected = int(outs["grep_text_count_only"][1].item())
    assert int(l[1].item()) == selected == int(l[2][1:].sum().item()) and int(l[2].sum().item()) == n_lines
    row = {"input": name, "dfa": dfa, "mib": mib, "lines": n_lines, "matches": total,
           "lines_selected": selected, "every": every, "n_bins": n_bins, "lds_bins": lds_bins,
           "bins_bytes": 8 * (n_bins + 1), "composed_record_bytes": 36 * total,
           "items_counted_in_lds_share": {
               "matches": float(m[2][:lds_bins].sum().item()) / max(1, total),
               "lines": float(l[2][:lds_bins].sum().item()) / max(1, n_lines)}}
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]  # noqa: E731
    row["ratio_tally_matches_to_collect_count"] = med("tally_matches") / med("collect_text_count_only")
    row["ratio_tally_lines_to_grep_count"] = med("tally_lines") / med("grep_text_count_only")
    row["ratio_plain_matches_to_collect_count"] = med("tally_matches_plain") / med("collect_text_count_only")
    row["ratio_plain_lines_to_grep_count"] = med("tally_lines_plain") / med("grep_text_count_only")
    row["ratio_tally_matches_to_composed"] = med("tally_matches") / med("composed_collect_bincount")
    if name == "log100":
        w = outs["tally_matches_100001_bins"]
        assert torch.equal(w[2][:n_bins], m[2][:n_bins]) and int(w[2][n_bins:].sum().item()) == 0
        row["items_counted_in_lds_share"]["matches_100001_bins"] = \
            float(w[2][:lds_bins].sum().item()) / max(1, total)
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
