"""Differential fuzz on the GPU: random DFAs x random line shapes x every verb / style / leader x
random placement and kernel-selection flags, against the CPU oracle.  Not part of the pytest
suite (it is open-ended); a failure prints the case and exits non-zero.
usage: fuzz_gpu.py [cases] [seed] [hot | cls | lists | blocks | long | text | lines | pieces | keys | groups]
       [dry]
long: the DFAs and placement flags of the general mode, one buffer of 2 KiB to 128 KiB as ONE
text through collect_long, replace_long, search_long and match_all_long (random style, leader
setting, chunk size, cap / max count and replacement).  Without a pure dead state an attempt that
does not accept walks to the end of the text - quadratic on the CPU and on the device's one lane -
so those DFAs get the first KiB of the buffer, and so do DFAs whose pure dead state the text's
walks do not reach (walks_die); match_all_long is one anchored walk and always gets all of it.
text: the same DFAs and flags, one buffer of 0 to 96 KiB as a raw text through grep_text,
collect_text, replace_text and match_text, each against sampleLines' loop (oracle.split_lines_loop)
plus the oracle's verb on every line alone.  The delimiter is '\n', 0, ' ' or a byte of the data, put
at a random density over whatever the data holds of it; where walks do not die (as above) a
delimiter comes at least every 1024 bytes, since search over a line is quadratic there.
lines: text's DFAs (the random ones with max_result drawn from 1 to 5000 too, so that results above
route_text's 255 buckets and the LDS bins exist), flags, delimiters and densities - the draws
weighted so that most cases have an item: fewer golden DFAs, tiny and never-accepting ones, fewer
texts without a line or of empty lines only, something planted for a golden DFA to find - text's
buffer kinds and one of digit runs, 0 to 96 KiB (one case in twenty empty), through the verbs whose item
is a line's search result - tally_text(matches=False), filter_text, route_text, range_text and
uniq_text(matches=False) - each once with random parameters against tests/text_rules.py.  The verbs
that write a text run through their host form one time in three, else through the device form: the
text at a pointer offset of 0 to 15, the output a 0x55-filled buffer handed over at out_cap = exact,
0 or half the expected length - the counts, min(out_len, out_cap) bytes and the sentinels behind
them (range_text's records likewise, behind min(n_ranges, rec_cap)).  The others take the host form
or the device form at an odd offset.
pieces: the same, through the verbs whose items come from collect's chain -
tally_text(matches=True), extract_text, uniq_text(matches=True), sum_text and fields_text.
dry (a fifth argument, lines and pieces only): no device is touched - DFA facts come from a
device-less handle, the case generator and text_rules run, the GPU calls do not.  Both modes end
with one `cover` line per verb: in how many cases the oracle's side had an item at all (in front
of any cap: max_count, max_ranges, max_per_line, max_fields), a text
longer than one 16 KiB chunk, an item in the overflow slot, a truncated output, a piece of 64
bytes or more, a piece that begins in front of its record's start, a number from 2^64, a range or a
merged context across a chunk border; and one `special` line for the inputs nobody designs.
tests/test_text_rules.py holds the dry run of the smoke test's cases and seed to floors on these.
keys: dedup_text alone, with cases of its own (the draws of lines and pieces are not touched: their
dry runs print what they printed before) - a golden or a random DFA under random placement flags,
a text of 0 to 1,000 lines of which almost half come from a pool of at most 8 strings, whole or with
something behind them, so that keys repeat, now and then a tail that repeats the first line and
under `whole` a long line twice; a random mode, key index, style, leader setting, count window,
invert, keep_unkeyed and delimiter, through the host form one time in three, else the device form
at a pointer offset of 0 to 15 into a 0x55-filled buffer at out_cap = exact, 0 or half - against
tests/dedup_rule.py.  dry works as above and ends with one `cover keys dedup_text` line: how many
cases ran each mode, held a string that occurs twice or more, an unkeyed line, a count window that
changes the output, an empty key, more than one chunk, a truncated output;
tests/test_dedup_rule.py holds it to floors.
groups: group_text alone, likewise with cases of its own - a golden or a random DFA under random
placement flags, a text of 0 to 1,000 lines of one to four tokens each, the tokens from a pool of at
most 8 keys and one of at most 6 numbers (small ones, 2^64 - 1, 2^64, leading zeros, none), so that
keys repeat and carry numbers; a random mode, key index, value index (0, below, at and above the
key's), `which`, delimiter and cap, through the host form or the device form at an odd pointer
offset - against tests/group_rule.py.  dry works as above and ends with one `cover groups
group_text` line; tests/test_group_rule.py holds it to floors."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import one_amd
import oracle as O
from oracle.reda_writer import random_dfa
from golden_util import load_dfa, CONFIG_DFAS

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
HOT_BIAS = len(sys.argv) > 3 and sys.argv[3] in ("hot", "cls")  # big DFAs, block-multiple strides
CLS_BIAS = len(sys.argv) > 3 and sys.argv[3] == "cls"           # ... of the class-table size
LISTS = len(sys.argv) > 3 and sys.argv[3] == "lists"            # only the record-list verbs
BLOCKS = len(sys.argv) > 3 and sys.argv[3] == "blocks"          # >= 4096 lines, check / match /
                                                                # match_all: the block kernels
LONG = len(sys.argv) > 3 and sys.argv[3] == "long"              # one text, the *_long verbs
TEXT = len(sys.argv) > 3 and sys.argv[3] == "text"              # one raw text, the *_text verbs
LINES = len(sys.argv) > 3 and sys.argv[3] == "lines"            # ... the newer ones: a line's result
PIECES = len(sys.argv) > 3 and sys.argv[3] == "pieces"          # ... the newer ones: collect's chain
NEWER = LINES or PIECES
DRY = NEWER and len(sys.argv) > 4 and sys.argv[4] == "dry"      # the generator and the rules alone
rng = np.random.default_rng(seed)
ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 ./:-_=&?%@[]", dtype=np.uint8)


def make_dfa():
    if CLS_BIAS:
        n = int(rng.choice([257, 300, 700, 1300, 2000]))
        c = int(rng.choice([2, 7, 25, 40, 100, 127]))
        s = int(rng.integers(0, 1 << 30))
        dead = float(rng.choice([0.0, 0.002, 0.02]))
        return "rnd(%d,%d,%d,dead=%.3f)" % (n, c, s, dead), random_dfa(n, c, s, dead_frac=dead, accept_frac=0.2)
    if HOT_BIAS:
        k = int(rng.integers(0, 4))
        if k == 0:
            name = ["uri_v6", "uri_user", "log100"][int(rng.integers(0, 3))]
            return name, load_dfa(name)
        n = int(rng.choice([300, 800, 2500]))
        c = int(rng.choice([7, 30, 64]))
        s = int(rng.integers(0, 1 << 30))
        dead = float(rng.choice([0.0, 0.002, 0.02]))
        return "rnd(%d,%d,%d,dead=%.3f)" % (n, c, s, dead), random_dfa(n, c, s, dead_frac=dead, accept_frac=0.2)
    k = int(rng.integers(0, 10))
    if k < 4:
        name = CONFIG_DFAS[int(rng.integers(0, len(CONFIG_DFAS)))]
        return name, load_dfa(name)
    n = int(rng.choice([2, 5, 17, 100, 255, 256, 257, 300, 800, 2500]))
    c = int(rng.choice([1, 2, 7, 30, 64, 128, 256]))
    dead = float(rng.choice([0.0, 0.0, 0.01, 0.05, 0.3, 0.9]))  # 0.9: sparse rows (kind 7) when big
    acc = float(rng.choice([0.0, 0.05, 0.2, 0.9]))
    s = int(rng.integers(0, 1 << 30))
    return "rnd(%d,%d,%d,dead=%.2f,acc=%.2f)" % (n, c, s, dead, acc), \
        random_dfa(n, c, s, dead_frac=dead, accept_frac=acc)


def make_lines():
    total_cap = 600_000
    if BLOCKS:
        if rng.random() < 0.6:
            L = int(rng.choice([32, 33, 48, 63, 64, 65, 80, 100, 127, 129]))
            n = int(rng.integers(4096, 6000))
            return dict(stride=L, n=n), n * L
        n = int(rng.choice([4096, 5000, 9000]))
        lens = rng.integers(0, 140, n) if rng.random() < 0.7 else rng.geometric(1 / 30, n) - 1
        lens = np.minimum(lens, 300).astype(np.int64)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        return dict(offsets=off), int(off[-1])
    if rng.random() < 0.5:
        L = int(rng.choice([64, 128, 192, 256, 1024, 4096] if HOT_BIAS else
                           [0, 1, 15, 16, 17, 48, 63, 64, 65, 128, 192, 256, 1000, 4096]))
        n = int(rng.integers(1, max(2, min(40000, total_cap // max(L, 1)))))
        return dict(stride=L, n=n), n * L
    n = int(rng.choice([1, 2, 100, 3000, 20000]))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        lens = rng.integers(0, 200, n)
    elif kind == 1:
        lens = rng.geometric(1 / 40, n) - 1
    else:
        lens = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 70, n))
    if rng.random() < 0.2:
        lens[int(rng.integers(0, n))] = int(rng.integers(3000, 9000))
    lens = np.minimum(lens, max(1, total_cap // n)).astype(np.int64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return dict(offsets=off), int(off[-1])


def make_data(nbytes, blob_name):
    k = int(rng.integers(0, 4))
    if k == 0:
        d = rng.integers(0, 256, nbytes, dtype=np.uint8)
    elif k == 1:
        d = ALPHA[rng.integers(0, len(ALPHA), nbytes)]
    elif k == 2:
        d = rng.integers(0, 4, nbytes, dtype=np.uint8) + 97
    else:
        d = ALPHA[rng.integers(0, len(ALPHA), nbytes)].copy()
        plants = [b"error", b"https://ab-c.example.com:8080/p?q=1#f ", b"New York", b"123abcd", b"aab",
                  b"ERROR [net] conn failed code=7", b"ssh://u@h.example.org:22/x "]
        for _ in range(max(1, nbytes // 300)):
            p = np.frombuffer(plants[int(rng.integers(0, len(plants)))], dtype=np.uint8)
            if nbytes > len(p):
                at = int(rng.integers(0, nbytes - len(p)))
                d[at:at + len(p)] = p
    return np.ascontiguousarray(d)


def walks_die(cpu, data):
    """64 walks of 256 bytes from the initial state, spread over data: at most one in eight may
    still be alive (a state is a dead end when every byte leads back to it with result 0)"""
    k, L = 64, 256
    if len(data) < L:
        return False
    pos = np.linspace(0, len(data) - L, k).astype(np.int64)
    buf = np.concatenate([data[p:p + L] for p in pos])
    st = np.full(k, O.STATE_INITIAL, dtype=np.uint32)
    cpu.advance_batch(buf, st, stride=L, n=k)
    alive = 0
    for t in set(st.tolist()):
        nxt = np.full(256, t, dtype=np.uint32)
        res = cpu.advance_batch(np.arange(256, dtype=np.uint8), nxt, stride=1, n=256)
        if not ((nxt == t).all() and (res == 0).all()):
            alive += int((st == t).sum())
    return alive * 8 <= k


def long_case(desc, blob, exe, cpu, data):
    """collect_long, replace_long, search_long and match_all_long over data as one text; the
    failing call or None"""
    whole = data
    if exe.info["n_pure_dead"] == 0 or not walks_die(cpu, data):
        data = data[:1024]
    text = data.tobytes()
    for verb in ("collect_long", "replace_long", "search_long", "match_all_long"):
        sty = int(rng.integers(1, 6))
        lead = int(rng.integers(0, 2))
        chunk = int(rng.choice([0, 1, 3, 16, 64, 1000, 4096]))
        if verb == "collect_long":
            cap = [None, 0, 5, 4096][int(rng.integers(0, 4))]
            recs, k = cpu.collect(text, 4096)
            if k > len(recs):
                recs, k = cpu.collect(text, k)
            cnt, r, s, e = one_amd.collect_long(exe, data, cap, chunk_bytes=chunk)
            ok = cnt == k and list(zip(r.tolist(), s.tolist(), e.tolist())) == \
                (recs if cap is None else recs[:cap])
            what = (verb, chunk, cap)
        elif verb == "replace_long":
            repl = [b"", b"#", b"<<>>", b"0123456789" * 4][int(rng.integers(0, 4))]
            mx = int(rng.choice([0, 1, 3, 1 << 40]))
            ok = one_amd.replace_long(exe, data, repl, sty, bool(lead), mx, chunk_bytes=chunk) == \
                cpu.replace(text, repl, sty, bool(lead), mx)
            what = (verb, chunk, sty, lead, repl, mx)
        elif verb == "match_all_long":
            cap = [None, 0, 5, 4096][int(rng.integers(0, 4))]
            recs, k = cpu.match_all(whole.tobytes(), bool(lead), 4096 if cap is None else max(cap, 1))
            if cap is None and k > len(recs):
                recs, k = cpu.match_all(whole.tobytes(), bool(lead), k)
            cnt, r, s, e = one_amd.match_all_long(exe, whole, cap, bool(lead), chunk_bytes=chunk)
            ok = cnt == k and list(zip(r.tolist(), s.tolist(), e.tolist())) == \
                (recs if cap is None else recs[:cap])
            what = (verb, chunk, lead, cap, len(whole))
        else:
            ok = one_amd.search_long(exe, data, sty, bool(lead), chunk_bytes=chunk) == \
                tuple(int(v) for v in cpu.search(text, sty, bool(lead)))
            what = (verb, chunk, sty, lead)
        kern = one_amd.last_kernel()
        stats[kern] = stats.get(kern, 0) + 1
        if not ok:
            return what + (len(text), kern)
    return None


REPLS = [b"", b"#", b"<<>>", b"0123456789" * 4]
SENT = 0x55
UNLIMITED = 1 << 62


def text_case(desc, blob, exe, cpu, data):
    """grep_text, collect_text, replace_text and match_text over data as a raw text; the failing
    call or None"""
    import torch
    delim = [0x0A, 0x00, 0x20, int(data[int(rng.integers(0, len(data)))]) if len(data) else 0x0A][
        int(rng.integers(0, 4))]
    density = [0.0, 1 / 2000, 1 / 100, 1 / 8, 1.0][int(rng.integers(0, 5))]
    data = data.copy()
    data[rng.random(len(data)) < density] = delim
    if exe.info["n_pure_dead"] == 0 or not walks_die(cpu, data):
        data[1023::1024] = delim
    text = data.tobytes()
    # sampleLines' loop: line k = text[begins[k] : begins[k] + len(lines[k])], its delimiter behind it
    lines = O.split_lines_loop(text, delim)
    n = len(lines)
    lens = np.array([len(x) for x in lines], dtype=np.int64)
    begins = (np.cumsum(lens + 1) - (lens + 1)).astype(np.uint64)
    tail = text[int(lens.sum()) + n:]
    # ... and the lines back to back without their delimiters: the oracle's verb on each alone
    bare = np.frombuffer(b"".join(lines) + b"\0", dtype=np.uint8)
    boffs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    shape = (len(text), delim, density, n)

    def same(got, want):
        return len(got) == len(want) and all(
            (g is None and w is None) or (g is not None and w is not None and
                                          np.array_equal(np.asarray(g).astype(np.int64),
                                                         np.asarray(w).astype(np.int64)))
            for g, w in zip(got, want))

    for verb in ("grep_text", "collect_text", "replace_text", "match_text"):
        sty = int(rng.integers(1, 6))
        lead = int(rng.integers(0, 2))
        if verb == "grep_text":
            invert = bool(rng.integers(0, 2))
            mx = int(rng.choice([0, 1, 7, UNLIMITED]))
            cap = [None, 0, 3][int(rng.integers(0, 3))]
            r, s, e = cpu.batch("search", sty, lead, bare, offsets=boffs, threads=4)
            sel = np.flatnonzero((r > 0) != invert)
            total = min(len(sel), mx)
            sel = sel[:total if cap is None else min(total, cap)]
            want = (n, total, sel, begins[sel], begins[sel] + lens[sel].astype(np.uint64),
                    r[sel], s[sel], e[sel])
            got = one_amd.grep_text(exe, data, sty, bool(lead), invert=invert, delim=delim, cap=cap,
                                    max_count=mx)
            ok = got[:2] == want[:2] and same(got[2:], want[2:])
            what = (verb, sty, lead, invert, mx, cap)
        elif verb == "collect_text":
            cap = [None, 0, 5][int(rng.integers(0, 3))]
            pos = bool(rng.integers(0, 2))
            counts, r, s, e = cpu.collect_batch(bare, 8, offsets=boffs)
            recs = []           # (line, result, start, end), positions relative to the line
            for k in np.flatnonzero(counts).tolist():
                c = int(counts[k])
                if c <= 8:
                    mine = list(zip(r[k, :c].tolist(), s[k, :c].tolist(), e[k, :c].tolist()))
                else:
                    mine, again = cpu.collect(lines[k], c)
                    assert again == c
                recs += [(k,) + m for m in mine]
            total = len(recs)
            recs = np.array(recs[:total if cap is None else cap], dtype=np.int64).reshape(-1, 4)
            b = begins[recs[:, 0]].astype(np.int64)
            want = (n, total, recs[:, 0], b, recs[:, 1], recs[:, 2] + b if pos else None,
                    recs[:, 3] + b if pos else None)
            got = one_amd.collect_text(exe, data, delim=delim, cap=cap, want_positions=pos)
            ok = got[:2] == want[:2] and same(got[2:], want[2:])
            what = (verb, cap, pos)
        elif verb == "replace_text":
            repl = REPLS[int(rng.integers(0, len(REPLS)))]
            mx = int(rng.choice([0, 1, 3, UNLIMITED]))
            oc = bool(rng.integers(0, 2))
            out_cap = [None, 0, "half"][int(rng.integers(0, 3))]
            memo = {}
            for x in lines:
                if x not in memo:
                    memo[x] = cpu.replace(x, repl, sty, bool(lead), mx)
            d = bytes([delim])
            if oc:              # only the lines with a replacement, each with its delimiter; no tail
                out = b"".join(memo[x][1] + d for x in lines if memo[x][0] > 0)
            else:
                out = b"".join(memo[x][1] + d for x in lines) + tail
            n_repl = sum(memo[x][0] for x in lines)
            if out_cap is None:
                got = one_amd.replace_text(exe, data, repl, sty, bool(lead), mx, only_changed=oc,
                                           delim=delim)
                ok = got == (n, n_repl, out)
            else:
                # the device form into a sentinel-filled buffer: min(out_len, room) bytes written
                room = 0 if out_cap == 0 else len(out) // 2
                buf = torch.full((len(out) + 16,), SENT, dtype=torch.uint8, device="cuda")
                dev = torch.from_numpy(data).cuda()
                g = one_amd.replace_text(exe, dev, repl, sty, bool(lead), mx, only_changed=oc,
                                         delim=delim, out=buf, out_cap=room)
                torch.cuda.synchronize()
                back = buf.cpu().numpy().tobytes()
                ok = (int(g[0].item()), int(g[1].item()), int(g[2].item())) == (n, n_repl, len(out)) \
                    and back[:room] == out[:room] and back[room:] == bytes([SENT]) * (len(back) - room)
            what = (verb, sty, lead, repl, mx, oc, out_cap)
        else:
            check = bool(rng.integers(0, 2))
            r, s, e = cpu.batch("check" if check else "match", sty, lead, bare, offsets=boffs, threads=4)
            offs = np.concatenate([begins, [len(text) - len(tail)]]).astype(np.uint64)
            want = (offs, r, None if check else s, None if check else e)
            got = one_amd.match_text(exe, data, sty, bool(lead), delim=delim, want_start=not check,
                                     want_end=not check)
            ok = got[1] == n and same((got[0],) + got[2:], want)
            what = (verb, sty, lead, "check" if check else "match")
        kern = one_amd.last_kernel()
        stats[kern] = stats.get(kern, 0) + 1
        if not ok:
            return what + shape + (kern,)
    return None


# the newer raw-text verbs: modes lines and pieces -------------------------------------------------
if NEWER:
    import text_rules as TR
    from one_amd import workloads as W
    from one_amd.matcher import fields_mask
    PLANTS_WIDE = [b"error", b"an error: x", b"New York", b"123abcd ", b"aab", W.URI_PLANT,
                   W.URI_USER_PLANT, W.URI_V6_PLANT] + W.log100_heads()[::9]
CHUNK = 16384
SENT64 = 0x5555555555555555
SEPS = np.frombuffer(b" ,.:-x", dtype=np.uint8)
WRITERS = ("filter_text", "route_text", "range_text", "extract_text", "fields_text")
VERBS_OF = {"lines": ("tally_text", "filter_text", "route_text", "range_text", "uniq_text"),
            "pieces": ("tally_text", "extract_text", "uniq_text", "sum_text", "fields_text")}
# which of the dry run's items belong to which verb (item and chunk belong to all)
COVER_OF = {"overflow": ("tally_text", "route_text", "sum_text"), "truncated": WRITERS,
            "piece64": ("extract_text", "fields_text"),
            "loose": ("extract_text", "fields_text", "uniq_text", "sum_text"),
            "over64bit": ("sum_text",), "numeric": ("sum_text",), "range_border": ("range_text",),
            "merged_border": ("filter_text",)}
cover = {}
special = dict(empty=0, all_delims=0, delim0=0, no_dead=0, acc09=0)


def make_dfa_wide():
    """make_dfa's general draw - fewer golden DFAs, more accepting states, so that most cases have
    an item - the random DFAs with max_result drawn as well"""
    k = int(rng.integers(0, 10))
    if k < 3:
        name = CONFIG_DFAS[int(rng.integers(0, len(CONFIG_DFAS)))]
        return name, load_dfa(name)
    n = int(rng.choice([2, 5, 17, 17, 100, 100, 255, 256, 257, 300, 800, 2500]))
    c = int(rng.choice([1, 2, 7, 30, 64, 128, 256]))
    dead = float(rng.choice([0.0, 0.0, 0.01, 0.05, 0.3, 0.9]))
    acc = float(rng.choice([0.0, 0.05, 0.05, 0.2, 0.2, 0.2, 0.2, 0.9, 0.9, 0.9, 0.9, 0.9]))
    most = int(rng.choice([1, 5, 40, 300, 5000]))
    s = int(rng.integers(0, 1 << 30))
    special["acc09"] += acc == 0.9
    return "rnd(%d,%d,%d,dead=%.2f,acc=%.2f,max_result=%d)" % (n, c, s, dead, acc, most), \
        random_dfa(n, c, s, dead_frac=dead, accept_frac=acc, max_result=most)


def make_data_wide(nbytes, blob_name):
    """make_data's four kinds and a fifth: runs of 1 to 25 digits, a separator between two; under
    a golden DFA mostly with something planted that it matches, every 100 bytes or so"""
    if rng.random() >= 0.25:
        d = make_data(nbytes, blob_name)
    else:
        d = rng.integers(0x30, 0x3A, nbytes, dtype=np.uint8)
        ends = np.cumsum(rng.integers(1, 26, nbytes // 2 + 1) + 1) - 1
        ends = ends[ends < nbytes]
        d[ends] = SEPS[rng.integers(0, len(SEPS), len(ends))]
    if blob_name in CONFIG_DFAS and rng.random() < 0.8:
        d = d.copy()
        for _ in range(nbytes // 100):
            p = np.frombuffer(PLANTS_WIDE[int(rng.integers(0, len(PLANTS_WIDE)))], dtype=np.uint8)
            if nbytes > len(p):
                at = int(rng.integers(0, nbytes - len(p)))
                d[at:at + len(p)] = p
    return np.ascontiguousarray(d)


def raw_text(exe, cpu, data):
    """text_case's delimiters and densities over data, the two densities at which most texts have no
    item (no line at all, every line empty) drawn less often: (data, delim, density)"""
    delim = [0x0A, 0x00, 0x20, int(data[int(rng.integers(0, len(data)))]) if len(data) else 0x0A][
        int(rng.integers(0, 4))]
    density = float(rng.choice([0.0, 1 / 2000, 1 / 100, 1 / 8, 1.0], p=[0.1, 0.2, 0.3, 0.3, 0.1]))
    data = data.copy()
    data[rng.random(len(data)) < density] = delim
    if exe.info["n_pure_dead"] == 0 or not walks_die(cpu, data):
        data[1023::1024] = delim
    special["empty"] += len(data) == 0
    special["all_delims"] += len(data) > 0 and bool((data == delim).all())
    special["delim0"] += delim == 0
    special["no_dead"] += exe.info["n_pure_dead"] == 0
    return data, delim, density


def draw_bins(most, limit=None):
    """n_bins from {0, 1, a value below the DFA's largest result, max_result + 1, None}"""
    nb = [0, 1, int(rng.integers(1, max(2, most))), most + 1, None][int(rng.integers(0, 5))]
    return nb if nb is None or limit is None else min(nb, limit)


def draw_form(writer):
    """(device form?, the text's pointer offset, out_cap's kind): a writer's host form one time in
    three, else the device form at an offset of 0 to 15; the others' one time in two, else the
    device form at an odd offset"""
    if writer:
        return (int(rng.integers(0, 3)) > 0, int(rng.integers(0, 16)),
                ["exact", 0, "half"][int(rng.integers(0, 3))])
    return bool(rng.integers(0, 2)), 2 * int(rng.integers(0, 8)) + 1, None


def noted(verb, big, **flags):
    """count what this case had for the verb's row of the dry run's table"""
    row = cover.setdefault(verb, dict(cases=0, item=0, chunk=0))
    row["cases"] += 1
    row["chunk"] += big
    for k, v in flags.items():
        assert k == "item" or verb in COVER_OF[k], (verb, k)
        row[k] = row.get(k, 0) + bool(v)


def dev_text(data, shift):
    import torch
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + len(data)]
    if len(data):
        dev.copy_(torch.from_numpy(data))
    return dev


def room_of(kind, out):
    return len(out) if kind == "exact" else 0 if kind == 0 else len(out) // 2


def same_arrays(got, want):
    return len(got) == len(want) and all(
        np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64))
        for g, w in zip(got, want))


def wrote(call, data, shift, kind, want, at):
    """a writer's device form into a sentinel-filled buffer: want is the host form's tuple, its
    bytes at index `at`; the counts, min(out_len, room) bytes and every sentinel behind them"""
    import torch
    out = want[at]
    room = room_of(kind, out)
    buf = torch.full((len(out) + 16,), SENT, dtype=torch.uint8, device="cuda")
    got = call(dev_text(data, shift), out=buf, out_cap=room)
    torch.cuda.synchronize()
    back = buf.cpu().numpy().tobytes()
    rest = [g.cpu().numpy() for g in got[:at] + got[at + 2:]]
    return int(got[at].item()) == len(out) and back[:room] == out[:room] and \
        back[room:] == bytes([SENT]) * (len(back) - room) and \
        same_arrays(rest, [np.atleast_1d(w) for w in want[:at] + want[at + 1:]])


def range_dev(exe, data, shift, kind, want, rec_cap, sty, lead, o, c, eo, ec, inv, mx, delim):
    """range_text's device form through the C ABI, so that the records too lie in sentinel-filled
    memory: nothing is written at or behind min(n_ranges, rec_cap)"""
    import torch
    from one_amd import _lib
    out = want[3]
    room = room_of(kind, out)
    buf = torch.full((len(out) + 16,), SENT, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    rec = torch.full((4, rec_cap + 2), SENT64, dtype=torch.int64, device="cuda")
    dev = dev_text(data, shift)
    rc = _lib.lib().redgpu_range_text_dev(
        exe._h, sty, lead, o, c, int(eo), int(ec), int(inv), mx,
        dev.data_ptr() if len(data) else None, len(data), delim, cnt.data_ptr(), cnt.data_ptr() + 8,
        cnt.data_ptr() + 16, cnt.data_ptr() + 24, buf.data_ptr() if room else None, room, rec_cap,
        rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), rec[3].data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    if rc != _lib.OK:
        raise one_amd.RedExcept(_lib.lib().redgpu_last_error().decode())
    torch.cuda.synchronize()
    back = buf.cpu().numpy().tobytes()
    k = min(want[1], rec_cap)
    rows = rec.cpu().numpy().view(np.uint64)
    return cnt.tolist() == [want[0], want[1], want[2], len(out)] and back[:room] == out[:room] and \
        back[room:] == bytes([SENT]) * (len(back) - room) and \
        same_arrays(list(rows[:, :k]), want[4:]) and bool((rows[:, k:] == SENT64).all())


def counted(call, data, dev, shift, want):
    """a verb that returns counts and arrays, host form or device form at an odd offset, against
    that form's tuple `want`"""
    if not dev:
        got = call(data)
    else:
        import torch
        got = call(dev_text(data, shift))
        torch.cuda.synchronize()
        got = [g.cpu().numpy().view(np.uint64) for g in got]
    return same_arrays([np.atleast_1d(g) for g in got], [np.atleast_1d(w) for w in want])


def lines_case(desc, blob, exe, cpu, data):
    """the verbs whose item is a line's search result, each once; the failing call or None"""
    data, delim, density = raw_text(exe, cpu, data)
    t = TR.Text(cpu, data.tobytes(), delim)
    most, big = int(exe.info["max_result"]), len(data) > CHUNK
    shape = (len(data), delim, density, t.n_lines)
    for verb in VERBS_OF["lines"]:
        sty = int(rng.integers(1, 6))
        lead = int(rng.integers(0, 2))
        v = t.values(sty, lead)
        dev, shift, kind = draw_form(verb in WRITERS)
        if verb == "tally_text":
            nb = draw_bins(most)
            n_bins = most + 1 if nb is None else nb
            prev = rng.integers(0, 1000, n_bins + 1).astype(np.uint64) if rng.random() < 1 / 3 else None
            want = TR.tally(t, n_bins, False, sty, lead, into=prev)
            noted(verb, big, item=(v > 0).any(), overflow=(v >= max(n_bins, 1)).any())
            what = (verb, sty, lead, nb, prev is not None, dev, shift)
            if not DRY:
                def call(x):
                    import torch
                    into = None if prev is None else prev.copy() if not dev else \
                        torch.from_numpy(prev.astype(np.int64)).cuda()
                    return one_amd.tally_text(exe, x, nb, matches=False, style=sty,
                                              do_leader=bool(lead), delim=delim, into=into)
                ok = counted(call, data, dev, shift, want)
        elif verb == "filter_text":
            invert = bool(rng.integers(0, 2))
            before, after = (int(x) for x in rng.choice([0, 1, 2, 7, 100000], 2))
            mx = int(rng.choice([0, 1, 7, UNLIMITED]))
            want = TR.filter(t, sty, lead, invert, before, after, mx)
            sel = TR.selected(t, sty, lead, invert, mx)
            merged = [1 for a, b in zip(sel, sel[1:]) if b - a >= 2 and b - before <= a + after + 1
                      and (t.offs[a + 1] - 1) // CHUNK < t.offs[b] // CHUNK]
            noted(verb, big, item=((v > 0) != invert).any(), merged_border=merged,
                  truncated=dev and room_of(kind, want[3]) < len(want[3]))
            what = (verb, sty, lead, invert, before, after, mx, dev, shift, kind)
            if not DRY:
                kw = dict(invert=invert, before=before, after=after, max_count=mx, delim=delim)
                if dev:
                    ok = wrote(lambda x, **o: one_amd.filter_text(exe, x, sty, bool(lead), **kw, **o),
                               data, shift, kind, want, 3)
                else:
                    ok = one_amd.filter_text(exe, data, sty, bool(lead), **kw) == want
        elif verb == "route_text":
            nb = draw_bins(most, 255)
            n_bins = min(most + 1, 255) if nb is None else nb
            drop = bool(rng.integers(0, 2))
            want = TR.route(t, n_bins, sty, lead, drop)
            noted(verb, big, item=(v > 0).any(), overflow=(v >= max(n_bins, 1)).any(),
                  truncated=dev and room_of(kind, want[4]) < len(want[4]))
            what = (verb, sty, lead, nb, drop, dev, shift, kind)
            if not DRY:
                if dev:
                    ok = wrote(lambda x, **o: one_amd.route_text(exe, x, nb, sty, bool(lead),
                                                                 drop_unmatched=drop, delim=delim, **o),
                               data, shift, kind, want, 4)
                else:
                    got = one_amd.route_text(exe, data, nb, sty, bool(lead), drop_unmatched=drop,
                                             delim=delim)
                    ok = got[:2] == want[:2] and got[4] == want[4] and same_arrays(got[2:4], want[2:4])
        elif verb == "range_text":
            # the two most frequent positive results of this text (1 where there is none), both
            # ways round, the toggle form, or one that the text does not have
            seen = np.bincount(v[v > 0])
            top = [int(r) for r in np.argsort(-seen, kind="stable")[:2] if seen[r]] or [1]
            k = int(rng.integers(0, 4))
            o, c = top[0], top[-1]
            if k == 1:
                o, c = c, o
            elif k == 2:
                c = o
            elif k == 3:
                o, c = (most + 1, c) if rng.integers(0, 2) else (o, most + 1)
            eo, ec, inv = (bool(x) for x in rng.integers(0, 2, 3))
            mx = int(rng.choice([0, 1, 3, UNLIMITED]))
            x = TR.range_expect(t, o, c, sty, lead, eo, ec, inv, mx)
            rec_cap = [0, 2, x.n_ranges + 2][int(rng.integers(0, 3))]
            want = TR.range(t, o, c, sty, lead, eo, ec, inv, mx, rec_cap)
            noted(verb, big, item=(v == o).any(),
                  range_border=(x.begin // CHUNK < (x.end - 1) // CHUNK).any(),
                  truncated=dev and room_of(kind, want[3]) < len(want[3]))
            what = (verb, sty, lead, o, c, eo, ec, inv, mx, rec_cap, dev, shift, kind)
            if not DRY:
                if dev:
                    ok = range_dev(exe, data, shift, kind, want, rec_cap, sty, lead, o, c, eo, ec,
                                   inv, mx, delim)
                else:
                    got = one_amd.range_text(exe, data, o, c, sty, bool(lead), emit_open=eo,
                                             emit_close=ec, invert=inv, max_ranges=mx, delim=delim,
                                             rec_cap=rec_cap)
                    ok = got[:4] == want[:4] and same_arrays(got[4:], want[4:])
        else:
            want = TR.uniq(t, False, sty, lead)
            n = len(want[3])
            md = max(1, n) + [0, 1, 100][int(rng.integers(0, 3))]
            noted(verb, big, item=(v > 0).any())
            what = (verb, sty, lead, md, dev, shift)
            if not DRY:
                def call(x):
                    return one_amd.uniq_text(exe, x, matches=False, style=sty, do_leader=bool(lead),
                                             delim=delim, max_distinct=md,
                                             **(dict(cap=n) if dev else {}))
                # (the device form reports n_distinct too, and writes cap = n rows)
                ok = counted(call, data, dev, shift, want[:3] + (n,) + want[3:] if dev else want)
        if DRY:
            continue
        kern = one_amd.last_kernel()
        stats[kern] = stats.get(kern, 0) + 1
        if not ok:
            return what + shape + (kern,)
    return None


def pieces_case(desc, blob, exe, cpu, data):
    """the verbs whose items come from collect's chain, each once; the failing call or None"""
    data, delim, density = raw_text(exe, cpu, data)
    t = TR.Text(cpu, data.tobytes(), delim)
    most, big = int(exe.info["max_result"]), len(data) > CHUNK
    shape = (len(data), delim, density, t.n_lines)
    has = any(t.pieces())
    for verb in VERBS_OF["pieces"]:
        dev, shift, kind = draw_form(verb in WRITERS)
        per = int(rng.choice([0, 1, 3, UNLIMITED]))
        got = t.items(per)
        loose = any(it[3] < it[2] for it in got)
        if verb == "tally_text":
            nb = draw_bins(most)
            n_bins = most + 1 if nb is None else nb
            prev = rng.integers(0, 1000, n_bins + 1).astype(np.uint64) if rng.random() < 1 / 3 else None
            want = TR.tally(t, n_bins, True, into=prev)
            noted(verb, big, item=has, overflow=any(it[1] >= n_bins for it in t.items()))
            what = (verb, nb, prev is not None, dev, shift)
            if not DRY:
                def call(x):
                    import torch
                    into = None if prev is None else prev.copy() if not dev else \
                        torch.from_numpy(prev.astype(np.int64)).cuda()
                    return one_amd.tally_text(exe, x, nb, matches=True, delim=delim, into=into)
                ok = counted(call, data, dev, shift, want)
        elif verb == "extract_text":
            want = TR.extract(t, per)
            noted(verb, big, item=has, loose=loose,
                  piece64=any(it[4] - it[3] >= 64 for it in got),
                  truncated=dev and room_of(kind, want[2]) < len(want[2]))
            what = (verb, per, dev, shift, kind)
            if not DRY:
                if dev:
                    ok = wrote(lambda x, **o: one_amd.extract_text(exe, x, max_per_line=per,
                                                                   delim=delim, **o),
                               data, shift, kind, want, 2)
                else:
                    ok = one_amd.extract_text(exe, data, max_per_line=per, delim=delim) == want
        elif verb == "uniq_text":
            want = TR.uniq(t, True, max_per_line=per)
            n = len(want[3])
            md = max(1, n) + [0, 1, 100][int(rng.integers(0, 3))]
            noted(verb, big, item=has, loose=loose)
            what = (verb, per, md, dev, shift)
            if not DRY:
                def call(x):
                    return one_amd.uniq_text(exe, x, matches=True, max_per_line=per, delim=delim,
                                             max_distinct=md, **(dict(cap=n) if dev else {}))
                ok = counted(call, data, dev, shift, want[:3] + (n,) + want[3:] if dev else want)
        elif verb == "sum_text":
            which = ["first", "last"][int(rng.integers(0, 2))]
            nb = draw_bins(most)
            n_bins = most + 1 if nb is None else nb
            prev = None
            if rng.random() < 1 / 3:        # an earlier table: small counts, sums that wrap
                prev = np.stack([rng.integers(0, 1000, n_bins + 1).astype(np.uint64)] +
                                [rng.integers(0, 1 << 64, n_bins + 1, dtype=np.uint64)
                                 for _ in range(3)])
            want = TR.sum(t, n_bins, which, per, into=prev)
            parts = [t.piece_bytes(it) for it in got]
            noted(verb, big, item=has, loose=loose, numeric=want[2] > 0,
                  overflow=any(it[1] >= n_bins for it in got),
                  over64bit=any(TR.number(p, which == "last") is None and any(48 <= b <= 57 for b in p)
                                for p in parts))
            what = (verb, which, per, nb, prev is not None, dev, shift)
            if not DRY:
                def call(x):
                    import torch
                    into = None if prev is None else prev.copy() if not dev else \
                        torch.from_numpy(prev.view(np.int64).copy()).cuda()
                    return one_amd.sum_text(exe, x, nb, which=which, max_per_line=per, delim=delim,
                                            into=into)
                ok = counted(call, data, dev, shift, want)
        else:
            k = int(rng.integers(0, 5))
            fields = ["1", "1,3", "2-", "64-", None][k]
            if fields is None:              # a random 64-bit mask, as a cut-style list
                mask = int(rng.integers(1, 1 << 63)) | int(rng.integers(0, 2)) << 63
                fields = ",".join(["%d" % (b + 1) for b in range(63) if mask >> b & 1] +
                                  ["64-"] * (mask >> 63))
            sep = rng.integers(0, 256, int(rng.choice([0, 1, 3, 8])), dtype=np.uint8).tobytes()
            max_fields = int(rng.choice([0, 1, 2, 5]))
            only = bool(rng.integers(0, 2))
            want = TR.fields(t, fields_mask(fields), sep, max_fields, only)
            cut = t.items(max_fields - 1 if max_fields else UNLIMITED)
            noted(verb, big, item=has, loose=any(it[3] < it[2] for it in cut),
                  piece64=any(it[4] - it[3] >= 64 for it in cut),
                  truncated=dev and room_of(kind, want[3]) < len(want[3]))
            what = (verb, fields, sep, max_fields, only, dev, shift, kind)
            if not DRY:
                kw = dict(sep=sep, max_fields=max_fields, only_delimited=only, delim=delim)
                if dev:
                    ok = wrote(lambda x, **o: one_amd.fields_text(exe, x, fields, **kw, **o),
                               data, shift, kind, want, 3)
                else:
                    ok = one_amd.fields_text(exe, data, fields, **kw) == want
        if DRY:
            continue
        kern = one_amd.last_kernel()
        stats[kern] = stats.get(kern, 0) + 1
        if not ok:
            return what + shape + (kern,)
    return None


# dedup_text: mode keys ----------------------------------------------------------------------------
KEYS = len(sys.argv) > 3 and sys.argv[3] == "keys"
KEYS_DRY = KEYS and len(sys.argv) > 4 and sys.argv[4] == "dry"
WINDOWS = [(1, None), (1, 1), (2, None), (3, 2), (2, 2), (1, 3), (0, 1)]


def keys_text(name, what):
    """(lines, delim): 0 to 1,000 lines (one case in twenty none), almost half of them drawn from a pool
    of at most 8 strings - whole, or with something behind them - so that keys repeat; where the
    DFA is walked no line is longer than 230 bytes (a search that does not die is quadratic)"""
    delim = [0x0A, 0x00, 0x3B][int(rng.integers(0, 3))]
    n = 0 if rng.random() < 0.05 else int(rng.integers(1, 1001))
    src = make_data_wide(max(64 * 1024, 1), name)
    src = src[src != delim]
    pool = []
    for _ in range(int(rng.integers(1, 9))):
        k = int(rng.choice([0, 0, 1, 3, 8, 20, 70]))
        at = int(rng.integers(0, len(src) - k))
        pool.append(src[at:at + k].tobytes())
    if name == "num3" or rng.random() < 0.3:      # keys a number DFA finds, or cuts fields at
        pool[0] = [b"ab 12 cd 345 ", b"7 up 7", b"12ab", b"x1y22z333"][int(rng.integers(0, 4))]
    lines = []
    for _ in range(n):
        r = rng.random()
        if r < 0.35:
            lines.append(pool[int(rng.integers(0, len(pool)))])
        elif r < 0.45:
            k = int(rng.integers(1, 30))
            at = int(rng.integers(0, len(src) - k))
            lines.append(pool[int(rng.integers(0, len(pool)))] + src[at:at + k].tobytes())
        else:
            k = int(rng.choice([0, 1, 5, 30, 60, 120, 200]))
            at = int(rng.integers(0, len(src) - k))
            lines.append(src[at:at + k].tobytes())
    if n and what == "whole" and rng.random() < 0.3:     # one long line, twice
        k = int(rng.integers(3000, 40000))
        at = int(rng.integers(0, len(src) - k))
        for _ in range(2):
            lines.insert(int(rng.integers(0, len(lines) + 1)), src[at:at + k].tobytes())
    return lines, delim


def keys_main():
    import dedup_rule as DR
    import text_rules as TR
    global PLANTS_WIDE
    from one_amd import workloads as W
    PLANTS_WIDE = [b"error", b"an error: x", b"New York", b"123abcd ", b"aab", W.URI_PLANT,
                   W.URI_USER_PLANT, W.URI_V6_PLANT] + W.log100_heads()[::9]
    t0 = time.time()
    stats = {}
    row = dict(cases=0, whole=0, lines=0, match=0, field=0, repeated=0, unkeyed=0, window=0,
               empty_key=0, chunk=0, truncated=0)
    for case in range(cases):
        if rng.random() < 0.35:
            name = ["num3", "num3", "aab", "err"][int(rng.integers(0, 4))]
            blob = load_dfa(name)
        else:
            name, blob = make_dfa_wide()
        flags = {}
        for f, p in (("force_global", 0.15), ("force_hot", 0.2)):
            if rng.random() < p:
                flags[f] = True
        if rng.random() < 0.3:
            flags["lds_table_max"] = int(rng.choice([8 * 256, 40 * 256, 100 * 256, 20000, 70000]))
        try:
            exe = one_amd.Executable(blob, **(dict(device="none") if KEYS_DRY else {}), **flags)
        except one_amd.RedExcept as e:
            print("create refused:", name, flags, e)
            continue
        cpu = O.CpuOracle(blob)
        # (every second draw takes the modes in turn: none of them is rare under any seed)
        what = DR.WHATS[case % 4 if rng.random() < 0.5 else int(rng.integers(0, 4))]
        key_index = int(rng.choice([1, 1, 1, 2, 2, 3, 9]))
        sty, lead = int(rng.integers(1, 6)), int(rng.integers(0, 2))
        lo, hi = WINDOWS[int(rng.choice(len(WINDOWS), p=[0.25, 0.2, 0.2, 0.05, 0.1, 0.15, 0.05]))]
        invert, keep = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        lines, delim = keys_text(name, what)
        d = bytes([delim])
        tail = [b"", b"", lines[0] if lines else b"tail"][int(rng.integers(0, 3))]
        data = np.frombuffer(b"".join(x + d for x in lines) + tail, dtype=np.uint8).copy()
        desc = (case, name, flags, what, key_index, sty, lead, (lo, hi), invert, keep, delim,
                len(data))
        t = TR.Text(cpu, data.tobytes(), delim)
        per = DR.keys(t, what, key_index, sty, lead)
        kw = dict(min_count=lo, max_count=DR.MAX if hi is None else hi, invert=invert,
                  keep_unkeyed=keep)
        want = DR.dedup(t, what, key_index, sty, lead, **kw)
        strings = [k[1] for k in per if k is not None]
        plain = DR.dedup(t, what, key_index, sty, lead, invert=invert, keep_unkeyed=keep)
        dev, shift, kind = draw_form(True)
        row["cases"] += 1
        row[what] += 1
        row["repeated"] += len(set(strings)) < len(strings)
        row["unkeyed"] += None in per
        row["window"] += (lo, hi) != (1, None) and want != plain
        row["empty_key"] += b"" in strings
        row["chunk"] += len(data) > CHUNK
        row["truncated"] += dev and kind != "exact" and len(want[5]) > 1
        if not KEYS_DRY:
            call = lambda x, **more: one_amd.dedup_text(      # noqa: E731
                exe, x, what=what, key_index=key_index, style=sty, do_leader=bool(lead),
                min_count=lo, max_count=hi, invert=invert, keep_unkeyed=keep, delim=d,
                max_distinct=512, **more)
            try:
                ok = wrote(call, data, shift, kind, want, 5) if dev else call(data) == want
            except one_amd.RedExcept as e:
                print("ERROR", desc, e)
                sys.exit(1)
            kern = one_amd.last_kernel()
            stats[kern] = stats.get(kern, 0) + 1
            if not ok:
                print("MISMATCH", desc, "dedup_text", "dev" if dev else "host", shift, kind)
                sys.exit(1)
        if case % 25 == 0:
            print("case", case, "%.0fs" % (time.time() - t0), flush=True)
    print("cover keys dedup_text", " ".join("%s=%d" % kv for kv in row.items()))
    print("fuzz dry:" if KEYS_DRY else "fuzz ok:", cases, "cases; kernels:",
          dict(sorted(stats.items())))


if KEYS:
    keys_main()
    sys.exit(0)


# group_text: mode groups ---------------------------------------------------------------------------
GROUPS = len(sys.argv) > 3 and sys.argv[3] == "groups"
GROUPS_DRY = GROUPS and len(sys.argv) > 4 and sys.argv[4] == "dry"
NUMBERS = [b"0", b"7", b"007", b"12", b"345", b"99999", b"18446744073709551615",
           b"18446744073709551616", b"0" * 25 + b"7", b"3.14", b"x1y22z333", b"", b"none"]


def groups_text(name):
    """(lines, delim): 0 to 1,000 lines (one case in twenty none), each one to four tokens - a key
    from a pool of at most 8 strings, a number from a pool of at most 6, now and then other bytes -
    joined by one separator of the case's, so that keys repeat and carry numbers; no line is longer
    than 230 bytes (a search that does not die is quadratic)"""
    delim = [0x0A, 0x00, 0x3B][int(rng.integers(0, 3))]
    n = 0 if rng.random() < 0.05 else int(rng.integers(1, 1001))
    src = make_data_wide(64 * 1024, name)
    src = src[src != delim]
    keys = []
    for _ in range(int(rng.integers(1, 9))):
        k = int(rng.choice([0, 1, 3, 8, 20]))
        at = int(rng.integers(0, len(src) - k))
        keys.append(src[at:at + k].tobytes())
    nums = [NUMBERS[int(rng.integers(0, len(NUMBERS)))] for _ in range(int(rng.integers(1, 7)))]
    sep = [b" ", b"error", b" aab ", b",", b" 12 "][int(rng.integers(0, 5))]
    if name == "num3":
        keys = [b"k%c" % (0x61 + i) for i in range(len(keys))]    # (a number DFA cuts at digits)
    lines = []
    for _ in range(n):
        toks = []
        for _ in range(int(rng.integers(1, 5))):
            r = rng.random()
            if r < 0.45:
                toks.append(keys[int(rng.integers(0, len(keys)))])
            elif r < 0.85:
                toks.append(nums[int(rng.integers(0, len(nums)))])
            else:
                k = int(rng.choice([0, 1, 5, 30, 60]))
                at = int(rng.integers(0, len(src) - k))
                toks.append(src[at:at + k].tobytes())
        lines.append(sep.join(toks)[:230].replace(bytes([delim]), b"_"))
    return lines, delim


def groups_main():
    import group_rule as GR
    import text_rules as TR
    global PLANTS_WIDE
    from one_amd import workloads as W
    PLANTS_WIDE = [b"error", b"an error: x", b"New York", b"123abcd ", b"aab", W.URI_PLANT,
                   W.URI_USER_PLANT, W.URI_V6_PLANT] + W.log100_heads()[::9]
    t0 = time.time()
    stats = {}
    row = dict(cases=0, match=0, field=0, first=0, last=0, repeated=0, unkeyed=0, numeric=0,
               not_numeric=0, no_value=0, value_first=0, empty_key=0, chunk=0, capped=0, dev=0)
    for case in range(cases):
        if rng.random() < 0.5:
            name = ["num3", "aab", "err", "err"][int(rng.integers(0, 4))]
            blob = load_dfa(name)
        else:
            name, blob = make_dfa_wide()
        flags = {}
        for f, p in (("force_global", 0.15), ("force_hot", 0.2)):
            if rng.random() < p:
                flags[f] = True
        if rng.random() < 0.3:
            flags["lds_table_max"] = int(rng.choice([8 * 256, 40 * 256, 100 * 256, 20000, 70000]))
        try:
            exe = one_amd.Executable(blob, **(dict(device="none") if GROUPS_DRY else {}), **flags)
        except one_amd.RedExcept as e:
            print("create refused:", name, flags, e)
            continue
        cpu = O.CpuOracle(blob)
        # (every second draw takes the modes in turn: neither is rare under any seed)
        what = GR.WHATS[case % 2 if rng.random() < 0.5 else int(rng.integers(0, 2))]
        key_index = int(rng.choice([1, 1, 1, 2, 2, 3, 9]))
        value_index = int(rng.choice([0, 1, 1, 2, 2, 2, 3, 4, 9]))
        which = ["first", "last"][int(rng.integers(0, 2))]
        lines, delim = groups_text(name)
        d = bytes([delim])
        tail = [b"", b"", lines[0] if lines else b"tail"][int(rng.integers(0, 3))]
        data = np.frombuffer(b"".join(x + d for x in lines) + tail, dtype=np.uint8).copy()
        t = TR.Text(cpu, data.tobytes(), delim)
        per = GR.numbers(t, what, key_index, value_index, which)
        want = GR.group(t, what, key_index, value_index, which)
        n = len(want[4])
        dev, shift, _ = draw_form(False)
        cap = [None, n, n // 2, 0, n + 3][int(rng.integers(0, 5))]
        desc = (case, name, flags, what, key_index, value_index, which, delim, len(data), cap)
        strings = [p[1] for p in per if p is not None]
        row["cases"] += 1
        row[what] += 1
        row[which] += 1
        row["repeated"] += len(set(strings)) < len(strings)
        row["unkeyed"] += None in per
        row["numeric"] += want[2] > 0
        row["not_numeric"] += want[2] < want[1]
        row["no_value"] += value_index == 0
        row["value_first"] += 0 < value_index < key_index
        row["empty_key"] += b"" in strings
        row["chunk"] += len(data) > CHUNK
        row["capped"] += cap is not None and cap < n
        row["dev"] += dev
        if not GROUPS_DRY:
            verb = dict(what=what, key_index=key_index, value_index=value_index, which=which,
                        delim=d, max_distinct=1024, cap=cap)
            k = n if cap is None else min(n, cap)
            cut = want[:4] + tuple(a[..., :k] for a in want[4:])
            try:
                if dev:
                    import torch
                    got = one_amd.group_text(exe, dev_text(data, shift), **verb)
                    torch.cuda.synchronize()
                    ok = [int(x.item()) for x in got[:5]] == list(want[:4]) + [n] and \
                        same_arrays([x[..., :k].cpu().numpy().view(np.uint64) for x in got[5:]],
                                    cut[4:])
                else:
                    got = one_amd.group_text(exe, data, **verb)
                    ok = got[:4] == cut[:4] and same_arrays(got[4:], cut[4:]) and \
                        all(g.shape == w.shape for g, w in zip(got[4:], cut[4:]))
            except one_amd.RedExcept as e:
                print("ERROR", desc, e)
                sys.exit(1)
            kern = one_amd.last_kernel()
            stats[kern] = stats.get(kern, 0) + 1
            if not ok:
                print("MISMATCH", desc, "group_text", "dev" if dev else "host", shift)
                sys.exit(1)
        if case % 25 == 0:
            print("case", case, "%.0fs" % (time.time() - t0), flush=True)
    print("cover groups group_text", " ".join("%s=%d" % kv for kv in row.items()))
    print("fuzz dry:" if GROUPS_DRY else "fuzz ok:", cases, "cases; kernels:",
          dict(sorted(stats.items())))


if GROUPS:
    groups_main()
    sys.exit(0)

t0 = time.time()
stats = {}
for case in range(cases):
    name, blob = make_dfa_wide() if NEWER else make_dfa()
    if LONG:
        shape, nbytes = {}, int(rng.integers(2048, 128 * 1024 + 1))
    elif TEXT:
        shape, nbytes = {}, int(rng.integers(0, 96 * 1024 + 1))
    elif NEWER:                                # one case in twenty is the empty text
        shape, nbytes = {}, 0 if rng.random() < 0.05 else int(rng.integers(0, 96 * 1024 + 1))
    else:
        shape, nbytes = make_lines()
    data = make_data_wide(nbytes, name) if NEWER else make_data(nbytes, name)
    flags = {}
    for f, p in ((("force_generic", 0.05), ("no_bucketing", 0.3), ("force_stream", 0.5)) if CLS_BIAS else
                 (("force_generic", 0.05), ("force_global", 0.0), ("force_hot", 0.8),
                  ("no_bucketing", 0.3), ("force_stream", 0.7), ("force_chunking", 0.4)) if HOT_BIAS else
                 (("force_generic", 0.15), ("force_global", 0.15), ("force_hot", 0.25),
                  ("no_bucketing", 0.2), ("force_stream", 0.3), ("force_chunking", 0.3))):
        if rng.random() < p:
            flags[f] = True
    if rng.random() < 0.25:
        flags["force_early"] = True        # k_early for match over any LDS-resident table
    if rng.random() < 0.3:
        flags["stream_chains"] = int(rng.choice([2, 4]))  # k_stream / k_stream4 whatever the size
    if rng.random() < 0.3 and not CLS_BIAS:
        flags["lds_table_max"] = int(rng.choice([8 * 256, 40 * 256, 100 * 256, 20000, 70000]))
    try:
        exe = one_amd.Executable(blob, **(dict(device="none") if DRY else {}), **flags)
    except one_amd.RedExcept as e:
        print("create refused:", name, flags, e)
        continue
    cpu = O.CpuOracle(blob)
    desc = (case, name, {k: (v if not hasattr(v, "shape") else "offsets[%d]" % (len(v) - 1)) for k, v in shape.items()}, flags, exe.info["table_kind"])
    if LONG or TEXT or NEWER:
        try:
            bad = (long_case if LONG else text_case if TEXT else lines_case if LINES else
                   pieces_case)(desc, blob, exe, cpu, data)
        except one_amd.RedExcept as e:
            print("ERROR", desc, e)
            sys.exit(1)
        if bad:
            print("MISMATCH", desc, bad)       # (cases and seed reproduce it)
            sys.exit(1)
        if case % 25 == 0:
            print("case", case, "%.0fs" % (time.time() - t0), flush=True)
        continue
    verbs = (["match", "check", "advance", "match", "check"] if HOT_BIAS else
             ["match", "check", "scan", "search", "advance", "match_all", "collect", "replace"])
    if BLOCKS:
        verbs = ["match", "check", "match_all", "match", "check"]
    if LISTS:
        verbs = ["match_all", "collect", "match_all"]
    for verb in (rng.choice(verbs, 3) if HOT_BIAS or LISTS or BLOCKS else rng.choice(verbs, 3, replace=False)):
        sty = int(rng.choice([4, 5, 4, 5, 1, 2, 3])) if HOT_BIAS else int(rng.integers(1, 6))
        lead = int(rng.integers(0, 2))
        kw = dict(shape)
        try:
            if verb in ("match", "search"):
                fn = one_amd.match_batch if verb == "match" else one_amd.search_batch
                got = fn(exe, data, sty, lead, **kw)
                exp = cpu.batch(verb, sty, lead, data, threads=4, **kw)
                ok = all(np.array_equal(g, e) for g, e in zip(got, exp))
            elif verb in ("check", "scan"):
                if verb == "scan" and nbytes > 150_000:
                    continue  # O(n*m) on loose-start DFAs
                fn = one_amd.check_batch if verb == "check" else one_amd.scan_batch
                got = fn(exe, data, sty, lead, **kw)
                exp = cpu.batch(verb, sty, lead, data, threads=4, **kw)[0]
                ok = np.array_equal(got, exp)
            elif verb == "advance":
                n = kw["n"] if "n" in kw else len(kw["offsets"]) - 1
                st = np.full(n, one_amd.STATE_INITIAL, dtype=np.uint32)
                ost = np.full(n, O.STATE_INITIAL, dtype=np.uint32)
                got = one_amd.advance_batch(exe, data, st, **kw)
                exp = cpu.advance_batch(data, ost, **kw)
                ok = np.array_equal(got, exp)
            elif verb in ("match_all", "collect"):
                if nbytes > 150_000 and not (BLOCKS and verb == "match_all"):
                    continue  # (collect is quadratic without a pure dead state; matchAll is one walk)
                cap = 4
                if verb == "match_all":
                    got = one_amd.match_all_batch(exe, data, cap, bool(lead), **kw)
                    exp = cpu.match_all_batch(data, cap, do_leader=bool(lead), **kw)
                else:
                    got = one_amd.collect_batch(exe, data, cap, **kw)
                    exp = cpu.collect_batch(data, cap, **kw)
                ok = np.array_equal(got[0], exp[0])
                m = np.arange(cap)[None, :] < np.minimum(exp[0], cap).astype(np.int64)[:, None]
                ok = ok and all(np.array_equal(g[m], e[m]) for g, e in zip(got[1:], exp[1:]))
            else:
                if nbytes > 60_000:
                    continue
                repl = [b"", b"#", b"<<>>"][int(rng.integers(0, 3))]
                mx = int(rng.choice([0, 1, 3, 1 << 40]))
                counts, ooff, out = one_amd.replace_batch(exe, data, repl, sty, bool(lead), mx, **kw)
                n = len(counts)
                ok = True
                for i in rng.integers(0, n, min(n, 40)):
                    if "offsets" in kw:
                        t = data[int(kw["offsets"][i]):int(kw["offsets"][i + 1])].tobytes()
                    else:
                        t = data[i * kw["stride"]:(i + 1) * kw["stride"]].tobytes()
                    k, o = cpu.replace(t, repl, sty, bool(lead), mx)
                    if k != int(counts[i]) or o != out[int(ooff[i]):int(ooff[i + 1])].tobytes():
                        ok = False
            kern = one_amd.last_kernel()
            stats[kern] = stats.get(kern, 0) + 1
            if not ok:
                print("MISMATCH", desc, verb, sty, lead, kern)
                np.savez("gpurun_out/fuzz_fail.npz", blob=np.frombuffer(blob, dtype=np.uint8), data=data,
                         **{k: v for k, v in shape.items() if hasattr(v, "shape")})
                sys.exit(1)
        except one_amd.RedExcept as e:
            print("ERROR", desc, verb, sty, lead, e)
            sys.exit(1)
    if case % 25 == 0:
        print("case", case, "%.0fs" % (time.time() - t0), flush=True)
if NEWER:       # what the oracle's side of the cases held, per verb (see the docstring)
    for verb in VERBS_OF[sys.argv[3]]:
        print("cover", sys.argv[3], verb, " ".join("%s=%d" % kv for kv in cover.get(verb, {}).items()))
    print("special", sys.argv[3], " ".join("%s=%d" % kv for kv in special.items()))
print("fuzz dry:" if DRY else "fuzz ok:", cases, "cases; kernels:", dict(sorted(stats.items())))
