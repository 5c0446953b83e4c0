"""ms per call of search over ONE long text: the chunk-parallel route (redgpu_search_long_dev,
styLast with the leader) from device events, 10 calls timed one by one.  Per DFA:
  plain     the alphabet text as it is (log100 finds nothing in it: every position is tried),
            beside redgpu_collect_long_dev on the same text;
  early     (DFAs that find nothing in the plain text) the only match planted at `early MiB` of
            the text and, separately, in a text of 4 x that size: the two should cost about the
            same, and far less than the text without a match; beside collect_long(cap = 1),
            which walks everything;
  one lane  redgpu_search_batch_dev with n = 1 on a prefix, one call, against the chunked route
            on the same prefix; both must give the same Outcome.
chunk= forces the chunk size of the search_long calls (0: automatic).  Developer tool (bench.py is
the contract bench).  usage: bench_search_long.py [MiB] [one-lane MiB] [early MiB] [chunk] [dfa ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import _lib, workloads as W

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
lane_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 8
early_mib = int(sys.argv[3]) if len(sys.argv) > 3 else 1
chunk = int(sys.argv[4]) if len(sys.argv) > 4 else 0
names = sys.argv[5:] or ["num3", "log100", "ale"]
l = _lib.lib()
PLANT = {"log100": W.log100_heads()[0].rstrip()}


def timed(fn, it=10):
    """ms of each of `it` calls behind one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(it):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    s = sorted(ms)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1]}


for name in names:
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    n = mib << 20
    host = W.alphabet_bytes(n, 1)
    data = torch.from_numpy(host).cuda()
    st = torch.cuda.current_stream().cuda_stream
    res = torch.zeros(1, dtype=torch.int32, device="cuda")
    pos = torch.zeros(2, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    cres = torch.zeros(16, dtype=torch.int32, device="cuda")
    cpos = torch.zeros(32, dtype=torch.int64, device="cuda")

    def search_call(d, c=chunk):
        rc = l.redgpu_search_long_dev(exe._h, 4, 1, d.data_ptr(), d.numel(), c, res.data_ptr(),
                                      pos.data_ptr(), pos.data_ptr() + 8, st)
        assert rc == 0, l.redgpu_last_error()

    def outcome():
        return [int(res.item())] + [int(v) for v in pos.tolist()]

    def collect_call(d, cap):
        rc = l.redgpu_collect_long_dev(exe._h, d.data_ptr(), d.numel(), 0, cap, cnt.data_ptr(),
                                       cres.data_ptr(), cpos.data_ptr(), cpos.data_ptr() + 128, st)
        assert rc == 0, l.redgpu_last_error()

    search_call(data)
    plain = outcome()
    route = one_amd.last_kernel()
    t_plain = timed(lambda: search_call(data))
    t_col = timed(lambda: collect_call(data, 16))
    row = {"dfa": name, "mib": mib, "chunk": chunk, "route": route, "outcome": plain,
           "search_ms": stats(t_plain), "search_GBps": n / stats(t_plain)["median"] / 1e6,
           "collect_long_ms": stats(t_col), "collect_long_matches": int(cnt.item()),
           "search_over_collect": stats(t_plain)["median"] / stats(t_col)["median"]}
    # the only match planted early: in the whole text and in a text of 4 x early MiB
    if plain[0] == 0 and name in PLANT and 4 * early_mib <= mib:
        at = early_mib << 20
        planted = host.copy()
        planted[at:at + len(PLANT[name])] = np.frombuffer(PLANT[name], dtype=np.uint8)
        big = torch.from_numpy(planted).cuda()
        small = big[: 4 * at].clone()
        search_call(big)
        o_big = outcome()
        search_call(small)
        assert outcome() == o_big and o_big[0] > 0 and o_big[1] == at, (name, o_big, outcome())
        t_big = timed(lambda: search_call(big))
        t_small = timed(lambda: search_call(small))
        t_cbig = timed(lambda: collect_call(big, 1))
        t_csmall = timed(lambda: collect_call(small, 1))
        row.update({"early_mib": early_mib, "early_outcome": o_big, "early_in_text_ms": stats(t_big),
                    "early_in_4x_ms": stats(t_small), "collect_cap1_text_ms": stats(t_cbig),
                    "collect_cap1_4x_ms": stats(t_csmall),
                    "early_over_no_match": stats(t_big)["median"] / stats(t_plain)["median"]})
    # the one-lane route on a prefix, one call; both routes must give the same Outcome
    lane = data[: lane_mib << 20]
    search_call(lane)
    o_long = outcome()
    t_long8 = timed(lambda: search_call(lane))
    r1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    p1 = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, lane.numel()], dtype=torch.int64, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = l.redgpu_search_batch_dev(exe._h, 4, 1, lane.data_ptr(), off.data_ptr(), 0, 1,
                                   r1.data_ptr(), p1.data_ptr(), p1.data_ptr() + 8, st)
    assert rc == 0, l.redgpu_last_error()
    b.record()
    torch.cuda.synchronize()
    lane_ms = a.elapsed_time(b)
    assert [int(r1.item())] + [int(v) for v in p1.tolist()] == o_long, (name, o_long)
    row.update({"lane_mib": lane_mib, "prefix_outcome": o_long, "long_on_prefix_ms": stats(t_long8),
                "lane_ms": lane_ms, "speedup_on_prefix": lane_ms / stats(t_long8)["median"]})
    print(json.dumps(row), flush=True)
