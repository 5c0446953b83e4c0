"""GB/s of text per call of fields_text (awk -F's columns of a raw text) over a raw text of
delimiter-terminated lines, all device-resident and alternated in one process:
  (a) redgpu_fields_text_dev "1-", the sizes only (out_cap = 0);
  (b) redgpu_fields_text_dev "1-" with the output;
  (c) "1,3" with the output;
  (d) "1" with the output - the chain is left behind the first separator of every line;
  (e) redgpu_extract_text_dev, the sizes only, same DFA and text - the walk alone, existing code;
  (f) redgpu_replace_text_dev(sep, styLast, no leader) - the route equal to (b);
  (g) the composed route a caller had before, for "1,3": redgpu_split_lines_dev, then
      redgpu_collect_batch_dev(cap = 8), then a torch gather of the two fields, the joiner and
      the delimiters.  It is GIVEN the line count and the output's length.
bench_extract_text.py's lines: 32..256 bytes of alphabet text (blanks and commas taken out)
joined by '\\n'.  For the crafted DFAs [ \\t]+ and , a separator is planted every 8..28 bytes, about
8 fields a line; num3 (a fixture) runs over bench_extract_text.py's dense text, its piece at the
start of every line.  Device events around each call, the median of 10 after a warm-up call of
each route.  Developer tool (bench.py is the contract bench).
The rows are printed and written to profiles/fields_text_<MiB>mib.jsonl.
usage: bench_fields_text.py [MiB] [dfa ...]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import json
import numpy as np
import torch, one_amd
from one_amd import workloads as W

args = sys.argv[1:]
mib = int(args[0]) if args else 256
names = args[1:] or ["ws", "comma", "num3"]
REPS = 10
SEP = b" "
OUT = os.path.join(ROOT, "profiles", "fields_text_%dmib.jsonl" % mib)
rows = []


def crafted(name):
    """[ \\t]+ and , as serialized DFAs: 0 = error, 1 = initial, 2 = accepting"""
    import oracle
    if not os.path.exists(oracle.LIB_ORACLE):
        oracle.build(ref=False)
    from oracle.reda_writer import write_reda
    equiv = np.zeros(256, dtype=np.uint8)
    equiv[list(b" \t" if name == "ws" else b",")] = 1
    trans = np.zeros((3, 2), dtype=np.int64)
    trans[1, 1] = 2
    if name == "ws":
        trans[2, 1] = 2
    return write_reda(trans, [0, 0, 1], equiv=equiv, initial=1)


def make_text(name, n):
    """lines of 32..256 bytes (delimiter included); separators every 8..28 bytes (ws: a blank, a
    tab or two blanks; comma: a comma), or num3's piece at the start of every line"""
    n_lines = n // 144 + 1
    lens = (W.splitmix64(np.arange(n_lines, dtype=np.uint64), 0x5EED) % np.uint64(225)).astype(np.int64) + 32
    ends = np.cumsum(lens)
    ends = ends[:int(np.searchsorted(ends, n, side="right"))]
    a = W.alphabet_bytes(n, 1).copy()
    for ch in b" \t,\n":
        a[a == ch] = 0x78
    if name == "num3":
        begins = np.concatenate([[0], ends[:-1]])
        p = np.frombuffer(b"12345a", dtype=np.uint8)
        begins = begins[begins + len(p) < n]
        a[begins[:, None] + np.arange(len(p))[None, :]] = p[None, :]
    else:
        gaps = (W.splitmix64(np.arange(n // 8, dtype=np.uint64), 0xF1E1D) % np.uint64(21)).astype(np.int64) + 8
        at = np.cumsum(gaps)
        at = at[at < n - 2]
        if name == "ws":
            kind = at % 3
            a[at] = np.where(kind == 1, 0x09, 0x20)
            a[at[kind == 2] + 1] = 0x20
        else:
            a[at] = 0x2C
    a[ends - 1] = 0x0A
    return a[:ends[-1]].copy()  # (no tail: replace_text would copy it, fields_text leaves it out)


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
    if name in ("ws", "comma"):
        blob = crafted(name)
    else:
        blob = open(os.path.join(ROOT, "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    host = make_text(name, mib << 20)
    n = host.size
    dev = torch.from_numpy(host).cuda()
    sized = {f: [int(v.item()) for v in one_amd.fields_text(exe, dev, f, sep=SEP, out_cap=0)[:4]]
             for f in ("1-", "1,3", "1")}
    n_lines = sized["1-"][0]
    room = torch.empty(max(v[3] for v in sized.values()) + 16, dtype=torch.uint8, device=dev.device)
    other = torch.empty(sized["1-"][3] + 16, dtype=torch.uint8, device=dev.device)

    def sizes_only():
        return one_amd.fields_text(exe, dev, "1-", sep=SEP, out_cap=0)

    def all_fields():
        return one_amd.fields_text(exe, dev, "1-", sep=SEP, out=room)

    def one_and_three():
        return one_amd.fields_text(exe, dev, "1,3", sep=SEP, out=room)

    def first_field():
        return one_amd.fields_text(exe, dev, "1", sep=SEP, out=room)

    def extract_sizes():
        return one_amd.extract_text(exe, dev, out_cap=0)

    def replace_sep():
        return one_amd.replace_text(exe, dev, SEP, one_amd.styLast, False, out=other)

    out13 = sized["1,3"][3]

    def composed():
        offs, _ = one_amd.split_lines(exe, dev, cap=n_lines)
        cnt, _, st, en = one_amd.collect_batch(exe, dev, 8, offsets=offs, stride=1)
        cnt = cnt.to(torch.int64)
        begin = offs[:n_lines]
        length = offs[1:n_lines + 1] - begin - 1
        len1 = torch.where(cnt > 0, st[:, 0].to(torch.int64), length)
        has3 = cnt > 1
        from3 = en[:, 1].to(torch.int64)
        len3 = torch.where(has3, torch.where(cnt > 2, st[:, 2].to(torch.int64), length) - from3,
                           torch.zeros_like(length))
        joined = has3.to(torch.int64) * len(SEP)
        size = len1 + joined + len3 + 1
        at = torch.cumsum(size, 0) - size
        line = torch.repeat_interleave(torch.arange(n_lines, device=dev.device), size,
                                       output_size=out13)
        pos = torch.arange(out13, device=dev.device) - at[line]
        in1 = pos < len1[line]
        in3 = pos >= (len1 + joined)[line]
        src = begin[line] + torch.where(in1, pos, from3[line] + pos - (len1 + joined)[line])
        out = dev[src.clamp_(0, n - 1)]
        out[~in1 & ~in3] = SEP[0]
        out[pos == size[line] - 1] = 0x0A
        return out

    routes = {"sizes_only": sizes_only, "all_fields": all_fields, "fields_1_3": one_and_three,
              "field_1": first_field, "extract_text_sizes_only": extract_sizes,
              "replace_text_sep": replace_sep, "composed_split_collect_gather": composed}
    outs = {}
    for k, f in routes.items():  # warm-up, and the routes checked against each other
        outs[k] = f()
        torch.cuda.synchronize()
        if k == "all_fields":
            kept = outs[k][4][:sized["1-"][3]].clone()
        if k == "fields_1_3":
            kept13 = outs[k][4][:out13].clone()
    assert [int(v.item()) for v in outs["sizes_only"][:4]] == sized["1-"]
    rep = outs["replace_text_sep"]
    assert int(rep[2].item()) == sized["1-"][3] and torch.equal(rep[3][:sized["1-"][3]], kept), name
    assert torch.equal(outs["composed_split_collect_gather"], kept13), name
    ms = {k: [] for k in routes}
    for _ in range(REPS):
        for k, f in routes.items():
            t, outs[k] = timed(f)
            ms[k].append(t)
    row = {"dfa": name, "mib": mib, "lines": n_lines,
           "fields_per_line": sized["1-"][2] / max(n_lines, 1),
           "out_len": {f: v[3] for f, v in sized.items()},
           "fields_written": {f: v[2] for f, v in sized.items()}}
    for k in routes:
        row[k] = stats(ms[k], n)
    med = lambda k: row[k]["median_GBps"]
    row["sizes_only_over_extract_sizes_only"] = med("sizes_only") / med("extract_text_sizes_only")
    row["all_fields_over_replace_text"] = med("all_fields") / med("replace_text_sep")
    row["fields_1_3_over_composed"] = med("fields_1_3") / med("composed_split_collect_gather")
    row["field_1_over_all_fields"] = med("field_1") / med("all_fields")
    print(json.dumps(row), flush=True)
    rows.append(row)
    del dev, room, other, kept, kept13, outs
with open(OUT, "w") as f:
    f.writelines(json.dumps(r) + "\n" for r in rows)
