"""GB/s of text per call of matchAll over ONE long text: the chunk-parallel route
(redgpu_match_all_long_dev, with cap = the count and with cap = 0) against the one-lane route
(redgpu_match_all_batch_dev, a batch of one line) on a prefix of the same text, and
redgpu_collect_long_dev on the same text, from device events.  Alphabet text with a matching piece
planted around every multiple of 1000 and of 768 for the regex DFAs, random bytes for syn256.
Each row also says how the 64 MiB call resolved its chunks (redgpu_diag_match_all_long_dev: chunks
walked again per round, chunks left to the serial lane), and "floor_ok": the chunked route is at
least 100 x the one-lane route on the prefix (false = the call fell to the serial lane).
Developer tool (bench.py is the contract bench).
usage: bench_match_all_long.py [MiB] [one-lane MiB] [dfa ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import json
import numpy as np
import torch, one_amd
from one_amd import _lib, workloads as W

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 64
lane_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 8
names = sys.argv[3:] or ["newyork", "uri", "uri_v6", "syn256"]
l = _lib.lib()
PIECES = {"newyork": b"New York", "uri": W.URI_PLANT.rstrip(), "uri_v6": W.URI_V6_PLANT.rstrip()}


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


def make_text(name, n):
    if name not in PIECES:
        return W.random_bytes(n, 7).copy()
    a = W.alphabet_bytes(n, 1).copy()
    piece = np.frombuffer(PIECES[name], dtype=np.uint8)
    for k, b in enumerate(sorted(set(range(1000, n, 1000)) | set(range(768, n, 768)))):
        at = b - len(piece) // 2 - k % 3
        if at + len(piece) <= n:
            a[at:at + len(piece)] = piece
    return a


for name in names:
    blob = open(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "dfas", name + ".reda"), "rb").read()
    exe = one_amd.Executable(blob)
    info = exe.info
    data = torch.from_numpy(make_text(name, mib << 20)).cuda()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def long_call(d, cap, r=None, s=None, e=None):
        rc = l.redgpu_match_all_long_dev(exe._h, 1, d.data_ptr(), d.numel(), 0, cap, cnt.data_ptr(),
                                         r.data_ptr() if cap else None, s.data_ptr() if cap else None,
                                         e.data_ptr() if cap else None, st)
        assert rc == 0, l.redgpu_last_error()

    ms0 = timed(lambda: long_call(data, 0), 10)
    route = one_amd.last_kernel()
    found = int(cnt.item())
    cap = max(found, 1)
    r = torch.empty(cap, dtype=torch.int32, device="cuda")
    s = torch.empty(cap, dtype=torch.int64, device="cuda")
    e = torch.empty(cap, dtype=torch.int64, device="cuda")
    ms = timed(lambda: long_call(data, cap, r, s, e), 10)
    assert int(cnt.item()) == found
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = l.redgpu_diag_match_all_long_dev(exe._h, stats.data_ptr(), st)
    assert rc == 0, l.redgpu_last_error()
    stats = stats.cpu().tolist()
    # the one-lane route, and the chunked one, on a prefix of the same text
    lane = data[: lane_mib << 20]
    off = torch.tensor([0, lane.numel()], dtype=torch.int64, device="cuda")
    cnt1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    r1, s1, e1 = torch.empty_like(r), torch.empty_like(s), torch.empty_like(e)

    def lane_call():
        rc = l.redgpu_match_all_batch_dev(exe._h, 1, lane.data_ptr(), off.data_ptr(), 0, 1, cap,
                                          cnt1.data_ptr(), r1.data_ptr(), s1.data_ptr(),
                                          e1.data_ptr(), st)
        assert rc == 0, l.redgpu_last_error()
    ms_lane = timed(lane_call, 1)
    ms_pre = timed(lambda: long_call(lane, cap, r, s, e), 10)
    k = int(cnt.item())
    assert k == int(cnt1.item()), (name, k, int(cnt1.item()))
    assert torch.equal(r[:k], r1[:k]) and torch.equal(s[:k], s1[:k]) and torch.equal(e[:k], e1[:k]), name
    row = {"dfa": name, "mib": mib, "route": route, "records": found,
           "long_us": ms * 1e3, "long_GBps": (mib << 20) / ms / 1e6,
           "count_only_us": ms0 * 1e3, "count_only_GBps": (mib << 20) / ms0 / 1e6,
           "lane_mib": lane_mib, "lane_records": k, "lane_us": ms_lane * 1e3,
           "lane_GBps": (lane_mib << 20) / ms_lane / 1e6, "long_on_lane_text_us": ms_pre * 1e3,
           "speedup_on_lane_text": ms_lane / ms_pre, "floor_ok": ms_lane / ms_pre >= 100.0,
           "chunks": stats[7], "rewalked_per_round": stats[0:4],
           "rounds_used": sum(1 for q in stats[0:4] if q),
           "first_open_chunk": None if stats[4] == stats[7] else stats[4],
           "serial_rewalked": stats[6]}
    # collect_long on the same text (dense DFAs that are not suffix-closed take its one-lane
    # route, seconds per call at this size: not timed)
    if info["n_pure_dead"] == 0 and not info["suffix_closed"]:
        row["collect_long_us"] = None
    else:
        ccap = 1 << 20
        cr = torch.empty(ccap, dtype=torch.int32, device="cuda")
        cs = torch.empty(ccap, dtype=torch.int64, device="cuda")
        ce = torch.empty(ccap, dtype=torch.int64, device="cuda")

        def collect_call():
            rc = l.redgpu_collect_long_dev(exe._h, data.data_ptr(), data.numel(), 0, ccap,
                                           cnt.data_ptr(), cr.data_ptr(), cs.data_ptr(),
                                           ce.data_ptr(), st)
            assert rc == 0, l.redgpu_last_error()
        msc = timed(collect_call, 3)
        row["collect_long_route"] = one_amd.last_kernel()
        row["collect_long_records"] = int(cnt.item())
        row["collect_long_us"] = msc * 1e3
        row["collect_long_GBps"] = (mib << 20) / msc / 1e6
    print(json.dumps(row), flush=True)
