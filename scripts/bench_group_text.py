"""GB/s of text per call of group_text (awk '{ n[$k]++; s[$k] += $v }' of a raw text, one record per
key) over a raw text of delimiter-terminated lines, all device-resident and alternated in one
process.  Every line is "<key><sep><value><sep>letters": under `match` the DFA is num3, the key and
the value are the line's first two numbers (pieces 1 and 2) and <sep> is a blank; under `field` the
DFA is aab as the SEPARATOR and the key and the value are fields 1 and 2.  Beside
redgpu_group_text_dev (cap = the distinct keys: the records are written):
  (a) redgpu_dedup_text_dev in the same mode at the same key_index, the sizes only: the same chain
      up to the key and the same inserts, without the value, the number and the statistics - the
      floor;
  (b) redgpu_sum_text_dev over the same DFA: the chain over ALL pieces of a line with the number
      reader, its slots by result;
  (c) the composed route a caller had before: extract_text_dev (match, two pieces a line) or
      fields_text_dev (field, fields 1 and 2) of key and value, a download of that text, and a
      Python dict - wall clock, one run.
group_text_dev and (a) run with the on-chip front and, under REDGPU_UNIQ_PLAIN=1 (read per call),
without it.  The texts: about 1 M distinct keys (`m1`), about 65 K (`k65`), and ONE key in every
line (`hot`).  Lines of 32..256 bytes joined by '\\n' (bench_dedup_text.py's).  Device events around
each call, the median of 10 after a warm-up call of each route.  Pass / fail rests on exactness
(tests/test_gpu_group_text.py), not on these rates.  Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/group_text_<MiB>mib.jsonl.
usage: bench_group_text.py [MiB] [regime ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import time
import numpy as np
import torch, one_amd
from one_amd import _lib, workloads as W

args = sys.argv[1:]
mib = int(args[0]) if args else 256
REGIMES = {"m1": 1 << 20, "k65": 1 << 16, "hot": 1}
regimes = args[1:] or list(REGIMES)
MODES = {"match": ("num3", b" "), "field": ("aab", b"aab")}
REPS = 10
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "profiles", "group_text_%dmib.jsonl" % mib)
rows = []


def make_text(n, distinct, sep):
    """letters-only lines of 32..256 bytes (delimiter included), each beginning with "<7 digits>",
    the separator, "<5 digits>" and the separator: the key one of `distinct` numbers, the value any"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    n_lines = int(np.searchsorted(ends, n, side="right"))
    ends = ends[:n_lines]
    # (letters c..z: no line holds the separator "aab" by chance)
    a = (W.splitmix64(np.arange(n, dtype=np.uint64), 0xA1FA) % np.uint64(24)).astype(np.uint8) + 99
    a[ends - 1] = 0x0A
    begins = np.concatenate([[0], ends[:-1]])
    idx = np.arange(n_lines, dtype=np.uint64)
    key = (W.splitmix64(idx, 0xD15C) % np.uint64(distinct)).astype(np.int64) + 1000000
    val = (W.splitmix64(idx, 0x7A1E) % np.uint64(90000)).astype(np.int64) + 10000
    s = np.frombuffer(sep, dtype=np.uint8)
    at = begins.copy()
    for number, width in ((key, 7), (val, 5)):
        digits = number[:, None] // (10 ** np.arange(width - 1, -1, -1))[None, :] % 10 + 0x30
        a[at[:, None] + np.arange(width)[None, :]] = digits.astype(np.uint8)
        at += width
        a[at[:, None] + np.arange(len(s))[None, :]] = s[None, :]
        at += len(s)
    assert int((at - begins).max()) < 32
    return a, key, val


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


def plain(fn):
    """fn() without the on-chip front: the library reads the knob at every call"""
    def run():
        os.environ["REDGPU_UNIQ_PLAIN"] = "1"
        try:
            return fn()
        finally:
            del os.environ["REDGPU_UNIQ_PLAIN"]
    return run


os.environ.pop("REDGPU_UNIQ_PLAIN", None)
for regime in regimes:
    distinct = REGIMES[regime]
    md = 1 << 22 if regime == "m1" else 1 << 18
    for mode, (name, sep) in MODES.items():
        with open(os.path.join(HERE, "..", "tests", "golden", "dfas", name + ".reda"), "rb") as f:
            exe = one_amd.Executable(f.read())
        host, key, val = make_text(mib << 20, distinct, sep)
        n = host.size
        dev = torch.from_numpy(host).cuda()
        verb = dict(what=mode, key_index=1, value_index=2, max_distinct=md)
        got = one_amd.group_text(exe, dev, cap=0, **verb)
        n_lines, n_keyed, n_numeric, n_dropped, n_distinct = (int(got[k].item()) for k in range(5))
        # what the generator says: every line keyed and numeric, the sums its own
        assert (n_lines, n_keyed, n_numeric, n_dropped) == (len(key),) * 3 + (0,), (regime, mode)
        assert n_distinct == len(np.unique(key))
        cap = n_distinct
        room = torch.empty(n // 4, dtype=torch.uint8, device="cuda")

        def composed():
            if mode == "match":
                cut = one_amd.extract_text(exe, dev, max_per_line=2, out=room)
                text = room[:int(cut[2].item())].cpu().numpy().tobytes()
                toks = text.split(b"\n")[:-1]
                pairs = zip(toks[0::2], toks[1::2])
            else:
                cut = one_amd.fields_text(exe, dev, "1,2", sep=b" ", out=room)
                text = room[:int(cut[3].item())].cpu().numpy().tobytes()
                pairs = (line.split(b" ") for line in text.split(b"\n")[:-1])
            table = {}
            for k, v in pairs:
                x = int(v)
                r = table.get(k)
                if r is None:
                    table[k] = [1, x, x, x]
                else:
                    r[0] += 1
                    r[1] += x
                    if x < r[2]:
                        r[2] = x
                    if x > r[3]:
                        r[3] = x
            return table

        group = lambda: one_amd.group_text(exe, dev, cap=cap, **verb)            # noqa: E731
        floor = lambda: one_amd.dedup_text(exe, dev, what=mode, key_index=1,     # noqa: E731
                                           max_distinct=md, out_cap=0)
        routes = {"group_text_dev": group, "group_text_dev_plain": plain(group),
                  "dedup_text_sizes_only": floor, "dedup_text_sizes_only_plain": plain(floor),
                  "sum_text_dev": lambda: one_amd.sum_text(exe, dev)}
        outs = {k: f() for k, f in routes.items()}  # warm-up
        assert int(outs["dedup_text_sizes_only"][2].item()) == n_distinct
        ms = {k: [] for k in routes}
        for _ in range(REPS):
            for k, f in routes.items():
                t, outs[k] = timed(f)
                ms[k].append(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = composed()
        composed_ms = (time.perf_counter() - t0) * 1e3
        # the three answers are the same: with the front, without it, and the dict's
        a, b = outs["group_text_dev"], outs["group_text_dev_plain"]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (regime, mode)
        first, length, count = (a[k].cpu().numpy() for k in (5, 6, 7))
        st = a[8].cpu().numpy().view(np.uint64)
        assert len(table) == n_distinct
        for j in range(0, n_distinct, max(1, n_distinct // 1000)):
            k = host[first[j]:first[j] + length[j]].tobytes()
            assert [int(count[j])] + [int(x) for x in st[1:, j]] == table[k], (regime, mode, j)
        row = {"mode": mode, "dfa": name, "mib": mib, "regime": regime, "lines": n_lines,
               "distinct": n_distinct, "lds_slots": int(_lib.lib().redgpu_group_lds_slots(exe._h))}
        for k in routes:
            row[k] = stats(ms[k], n)
        row["composed"] = {"once_GBps": n / (composed_ms * 1e6), "ms": composed_ms}
        med = lambda k: row[k]["median_GBps"]  # noqa: E731
        row["ratio_to_floor"] = med("group_text_dev") / med("dedup_text_sizes_only")
        row["ratio_plain_to_floor_plain"] = med("group_text_dev_plain") / med("dedup_text_sizes_only_plain")
        row["ratio_to_sum_text"] = med("group_text_dev") / med("sum_text_dev")
        row["ratio_to_composed"] = med("group_text_dev") / row["composed"]["once_GBps"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del dev, room, outs, table
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
