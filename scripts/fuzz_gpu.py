"""Differential fuzz on the GPU: random DFAs x random line shapes x every verb / style / leader x
random placement and kernel-selection flags, against the CPU oracle.  Not part of the pytest
suite (it is open-ended); a failure prints the case and exits non-zero.
usage: fuzz_gpu.py [cases] [seed] [hot | cls | lists | blocks | long | text]
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
delimiter comes at least every 1024 bytes, since search over a line is quadratic there."""
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


t0 = time.time()
stats = {}
for case in range(cases):
    name, blob = make_dfa()
    if LONG:
        shape, nbytes = {}, int(rng.integers(2048, 128 * 1024 + 1))
    elif TEXT:
        shape, nbytes = {}, int(rng.integers(0, 96 * 1024 + 1))
    else:
        shape, nbytes = make_lines()
    data = make_data(nbytes, name)
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
        exe = one_amd.Executable(blob, **flags)
    except one_amd.RedExcept as e:
        print("create refused:", name, flags, e)
        continue
    cpu = O.CpuOracle(blob)
    desc = (case, name, {k: (v if not hasattr(v, "shape") else "offsets[%d]" % (len(v) - 1)) for k, v in shape.items()}, flags, exe.info["table_kind"])
    if LONG or TEXT:
        try:
            bad = (long_case if LONG else text_case)(desc, blob, exe, cpu, data)
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
print("fuzz ok:", cases, "cases; kernels:", dict(sorted(stats.items())))
