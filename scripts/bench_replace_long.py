"""GB/s of text per call of replace over ONE long text: the chunk-parallel route
(redgpu_replace_long_dev, styLast, every match, a 3-byte replacement) on an alphabet text, from
device events, 10 calls timed one by one; beside it redgpu_collect_long_dev on the same text (the
walk the two share), a plain device-to-device copy of the text (the floor of the assembly), and
the one-lane route (redgpu_replace_batch_dev, a batch of one line, one call) on a prefix, where
both routes must give the same count and the same bytes.  Developer tool (bench.py is the
contract bench).  usage: bench_replace_long.py [MiB] [one-lane MiB] [dfa ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import torch, one_amd
from one_amd import _lib, workloads as W

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
lane_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 8
names = sys.argv[3:] or ["num3", "set5", "log100", "ale"]
l = _lib.lib()
CAP = 1 << 20
ALL = 1 << 62
REPL = b"<#>"


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
    data = torch.from_numpy(W.alphabet_bytes(n, 1)).cuda()
    repl = torch.tensor(list(REPL), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def replace_call(d, o):
        rc = l.redgpu_replace_long_dev(exe._h, 4, 1, d.data_ptr(), d.numel(), 0, repl.data_ptr(),
                                       len(REPL), ALL, sizes.data_ptr(), sizes.data_ptr() + 8,
                                       o.data_ptr() if o is not None else None,
                                       o.numel() if o is not None else 0, st)
        assert rc == 0, l.redgpu_last_error()
    replace_call(data, None)
    count, out_len = sizes.tolist()
    route = one_amd.last_kernel()
    out = torch.empty(out_len, dtype=torch.uint8, device="cuda")
    t_rep = timed(lambda: replace_call(data, out))
    t_plan = timed(lambda: replace_call(data, None))
    # the shared walk: collect_long on the same text
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    r = torch.empty(CAP, dtype=torch.int32, device="cuda")
    s = torch.empty(CAP, dtype=torch.int64, device="cuda")
    e = torch.empty(CAP, dtype=torch.int64, device="cuda")

    def collect_call():
        rc = l.redgpu_collect_long_dev(exe._h, data.data_ptr(), n, 0, CAP, cnt.data_ptr(),
                                       r.data_ptr(), s.data_ptr(), e.data_ptr(), st)
        assert rc == 0, l.redgpu_last_error()
    t_col = timed(collect_call)
    # the floor of the assembly: a device-to-device copy of the text
    dst = torch.empty_like(data)
    t_cpy = timed(lambda: dst.copy_(data))
    # the one-lane route on a prefix, one call; counts and bytes of both routes must agree
    lane = data[: lane_mib << 20]
    off = torch.tensor([0, lane.numel()], dtype=torch.int64, device="cuda")
    cnt1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    ooff = torch.zeros(2, dtype=torch.int64, device="cuda")
    replace_call(lane, None)
    c2, len2 = sizes.tolist()
    out2 = torch.empty(len2, dtype=torch.uint8, device="cuda")
    t_long8 = timed(lambda: replace_call(lane, out2))
    out1 = torch.empty(len2 + 64, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = l.redgpu_replace_batch_dev(exe._h, 4, 1, lane.data_ptr(), off.data_ptr(), 0, 1,
                                    repl.data_ptr(), len(REPL), ALL, cnt1.data_ptr(),
                                    ooff.data_ptr(), out1.data_ptr(), out1.numel(), st)
    assert rc == 0, l.redgpu_last_error()
    b.record()
    torch.cuda.synchronize()
    lane_ms = a.elapsed_time(b)
    assert int(cnt1.item()) == c2 and int(ooff[1].item()) == len2, (name, c2, len2)
    assert torch.equal(out1[:len2], out2), name
    med = stats(t_rep)["median"]
    med8 = stats(t_long8)["median"]
    row = {"dfa": name, "mib": mib, "route": route, "count": count, "out_len": out_len,
           "replace_ms": stats(t_rep), "replace_GBps": n / med / 1e6,
           "sizes_only_ms": stats(t_plan), "collect_long_ms": stats(t_col),
           "copy_ms": stats(t_cpy), "extra_over_collect_ms": med - stats(t_col)["median"],
           "extra_over_collect_in_copies": (med - stats(t_col)["median"]) / stats(t_cpy)["median"],
           "lane_mib": lane_mib, "long_on_prefix_ms": stats(t_long8), "lane_ms": lane_ms,
           "lane_GBps": (lane_mib << 20) / lane_ms / 1e6, "speedup_on_prefix": lane_ms / med8}
    print(json.dumps(row), flush=True)
