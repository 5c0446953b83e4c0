"""GB/s of text per call of Red::collect over ONE long text: the chunk-parallel route
(redgpu_collect_long_dev) against the one-lane route (redgpu_collect_batch_dev, a batch of one
line) on the same alphabet text, from device events; the reference's single-threaded
Red::collect (oracle.ref_collect, when built) on the host for scale.  Developer tool (bench.py is
the contract bench).  usage: bench_collect_long.py [MiB] [one-lane MiB] [dfa ...]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import torch, one_amd
from one_amd import _lib, workloads as W

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
lane_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 8
names = sys.argv[3:] or ["newyork", "num3", "log100", "uri"]
l = _lib.lib()
CAP = 1 << 20


def timed(fn, it):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it


out = []
for name in names:
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    host = W.alphabet_bytes(mib << 20, 1)
    data = torch.from_numpy(host).cuda()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    r = torch.empty(CAP, dtype=torch.int32, device="cuda")
    s = torch.empty(CAP, dtype=torch.int64, device="cuda")
    e = torch.empty(CAP, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def long_call(d=data):
        rc = l.redgpu_collect_long_dev(exe._h, d.data_ptr(), d.numel(), 0, CAP, cnt.data_ptr(),
                                       r.data_ptr(), s.data_ptr(), e.data_ptr(), st)
        assert rc == 0, l.redgpu_last_error()
    ms = timed(long_call, 10)
    route = one_amd.last_kernel()
    found = int(cnt.item())
    # the one-lane route on a prefix of the same text (at 64 MiB it would take seconds)
    lane = data[: lane_mib << 20]
    off = torch.tensor([0, lane.numel()], dtype=torch.int64, device="cuda")
    cnt1 = torch.zeros(1, dtype=torch.int64, device="cuda")

    def lane_call():
        rc = l.redgpu_collect_batch_dev(exe._h, lane.data_ptr(), off.data_ptr(), 0, 1, CAP,
                                        cnt1.data_ptr(), r.data_ptr(), s.data_ptr(), e.data_ptr(), st)
        assert rc == 0, l.redgpu_last_error()
    ms1 = timed(lane_call, 2)
    # the same prefix through the new route, for the exact count check
    long_call(lane)
    torch.cuda.synchronize()
    assert int(cnt.item()) == int(cnt1.item()), (name, int(cnt.item()), int(cnt1.item()))
    row = {"dfa": name, "mib": mib, "route": route, "matches": found, "long_us": ms * 1e3,
           "long_GBps": (mib << 20) / ms / 1e6, "lane_mib": lane_mib, "lane_us": ms1 * 1e3,
           "lane_GBps": (lane_mib << 20) / ms1 / 1e6}
    row["speedup"] = row["long_GBps"] / row["lane_GBps"]
    try:
        import oracle
        info = exe.info
        if info["n_pure_dead"] == 0 and info["suffix_closed"]:
            # every attempt runs to the end of the text and the reference walks each position
            # behind the last match to the end: quadratic, not timed
            row["ref_s"] = None
        elif oracle.have_ref() and os.environ.get("NO_REF") is None:
            text = host.tobytes()
            t0 = time.perf_counter()
            _, k = oracle.ref_collect(blob, text, 1)
            row["ref_s"] = time.perf_counter() - t0
            row["ref_GBps"] = len(text) / row["ref_s"] / 1e9
            assert k == found, (k, found)
    except ImportError:
        pass
    out.append(row)
    print(json.dumps(row), flush=True)
