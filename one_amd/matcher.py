"""Host-side mirror of the reference's matcher interface for the batch path.

Names follow /root/reference/quol/red: `Executable` (include/Executable.h:28-76), `Style`
(include/Matcher.h:67-74), `Outcome` fields result/start/end (include/Outcome.h:32-35), verbs
`check` / `match` / `scan` (include/Matcher.h:79-92,133-169) and the exception classes of
include/Except.h.  Everything here is plumbing over the C-ABI (include/redgpu.h): inputs may be
host arrays (numpy / bytes -> the library stages them) or torch tensors resident on the GPU
(-> the *_dev entry points, asynchronous on torch's current stream).
"""
from __future__ import annotations

import ctypes as C
import os
import enum

import numpy as np

from . import _lib


class Style(enum.IntEnum):  # include/Matcher.h:67-74
    styInvalid = 0
    styInstant = 1
    styFirst = 2
    styTangent = 3
    styLast = 4
    styFull = 5


styInstant, styFirst, styTangent, styLast, styFull = (Style.styInstant, Style.styFirst,
                                                      Style.styTangent, Style.styLast,
                                                      Style.styFull)


# include/Except.h:9-19
class RedExcept(RuntimeError):
    pass


class RedExceptApi(RedExcept):
    pass


class RedExceptExec(RedExcept):
    pass


class RedExceptLimit(RedExcept):
    pass


class RedExceptHip(RedExceptExec):
    """HIP runtime / device failure (no reference analogue)."""


_EXC = {_lib.EAPI: RedExceptApi, _lib.EEXEC: RedExceptExec, _lib.ELIMIT: RedExceptLimit,
        _lib.EHIP: RedExceptHip}


def _check(rc: int) -> None:
    if rc != _lib.OK:
        msg = _lib.lib().redgpu_last_error().decode()
        raise _EXC.get(rc, RedExcept)(msg)


def check_header(blob: bytes):
    """checkHeader (lib/Serializer.cpp:270-298): None when good, else the message."""
    msg = C.c_char_p()
    rc = _lib.lib().redgpu_reda_check(blob, len(blob), C.byref(msg))
    return None if rc == _lib.OK else msg.value.decode()


class Executable:
    """A validated serialized DFA uploaded to one GPU (mirrors zezax::red::Executable).

    device: HIP ordinal, None = current device, "none" = host-only handle (validate + repack,
    no HIP call; batch verbs on it raise RedExceptApi)."""

    def __init__(self, serialized: bytes, device=None, *, force_generic=False,
                 force_global=False, force_hot=False, no_bucketing=False,
                 force_stream=False, no_chunking=False, force_chunking=False,
                 lds_table_max=0, stream_chains=0, force_early=False, force_lean=False,
                 lean_chains=2, force_pieces=False):
        if serialized is None or len(serialized) == 0:
            raise RedExceptApi("serialized dfa string_view is empty")  # Executable.cpp:66
        o = _lib.Opts()
        o.device = (_lib.DEVICE_NONE if device == "none" else
                    _lib.DEVICE_CURRENT if device is None else int(device))
        o.lds_table_max = lds_table_max
        o.flags = Executable._flags_of(force_generic=force_generic, force_global=force_global,
                                       force_hot=force_hot, no_bucketing=no_bucketing,
                                       force_stream=force_stream, no_chunking=no_chunking,
                                       force_chunking=force_chunking, stream_chains=stream_chains,
                                       force_early=force_early, force_lean=force_lean,
                                       lean_chains=lean_chains, force_pieces=force_pieces)
        self._h = C.c_void_p()
        blob = bytes(serialized)
        _check(_lib.lib().redgpu_dfa_create(blob, len(blob), C.byref(o), C.byref(self._h)))

    @staticmethod
    def _flags_of(force_generic=False, force_global=False, force_hot=False, no_bucketing=False,
                  force_stream=False, no_chunking=False, force_chunking=False, stream_chains=0,
                  force_early=False, force_lean=False, lean_chains=2, force_pieces=False,
                  **_ignored) -> int:
        return ((_lib.F_FORCE_GENERIC if force_generic else 0) |
                (_lib.F_FORCE_GLOBAL if force_global else 0) |
                (_lib.F_FORCE_HOT if force_hot else 0) |
                (_lib.F_NO_BUCKETING if no_bucketing else 0) |
                (_lib.F_FORCE_STREAM if force_stream else 0) |
                (_lib.F_NO_CHUNKING if no_chunking else 0) |
                (_lib.F_FORCE_CHUNKING if force_chunking else 0) |
                (_lib.F_FORCE_EARLY if force_early else 0) |
                (_lib.F_FORCE_LEAN if force_lean else 0) |
                (_lib.F_LEAN_CHAINS_4 if lean_chains == 4 else 0) |
                (_lib.F_FORCE_PIECES if force_pieces else 0) |
                (_lib.F_STREAM_CHAINS_2 if stream_chains == 2 else 0) |
                (_lib.F_STREAM_CHAINS_4 if stream_chains == 4 else 0))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.redgpu_dfa_destroy(h)  # (at interpreter exit the module may be gone)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self) -> dict:
        i = _lib.Info()
        _check(_lib.lib().redgpu_dfa_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in _lib.Info._fields_}

    def tune(self, data, *, offsets=None, stride=0, n=None) -> dict:
        """redgpu_dfa_tune: re-rank the LDS-resident hot rows by the visits a sample of real
        input makes (host bytes / numpy, or a CUDA uint8 tensor).  Returns the new info."""
        l = _lib.lib()
        if _is_torch(data):
            import torch
            if offsets is not None:
                n = offsets.numel() - 1
            elif n is None:
                n = data.numel() // stride if stride else 0
            _check(l.redgpu_dfa_tune_dev(self._h, data.data_ptr(),
                                         offsets.data_ptr() if offsets is not None else None,
                                         stride, n,
                                         torch.cuda.current_stream(data.device).cuda_stream))
            return self.info
        a = _host_u8(data)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = len(offsets) - 1
        elif n is None:
            n = a.size // stride if stride else 0
        _check(l.redgpu_dfa_tune(self._h, a.ctypes.data if a.size else None,
                                 offsets.ctypes.data if offsets is not None else None, stride, n))
        return self.info

    def serialized(self) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        _check(_lib.lib().redgpu_dfa_serialized(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value)


def last_kernel() -> str:
    return _lib.lib().redgpu_last_kernel().decode()


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _host_u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    a = np.ascontiguousarray(data)
    if a.dtype != np.uint8:
        raise RedExceptApi("input bytes must be uint8")
    return a


_TRACE = bool(os.environ.get("REDGPU_PY_TRACE"))  # debugging aid: host buffer addresses per call


def _run(verb: str, exe: Executable, style, do_leader, data, offsets, stride, n, want_start,
         want_end, out=None):
    """Returns (result, start, end); start/end are None when not requested / not a match verb."""
    l = _lib.lib()
    style = int(style)
    lead = 1 if do_leader else 0
    if _is_torch(data):
        import torch
        if not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
            raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
        dev = data.device
        if offsets is not None:
            if (not _is_torch(offsets) or offsets.dtype not in (torch.int64, torch.uint64)
                    or not offsets.is_cuda or not offsets.is_contiguous()):
                raise RedExceptApi("device offsets must be a contiguous int64 CUDA tensor")
            n = offsets.numel() - 1
            stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
        elif n is None:
            n = data.numel() // stride if stride else 0
        if out is None:
            res = torch.empty(n, dtype=torch.int32, device=dev)
            st = torch.empty(n, dtype=torch.int64, device=dev) if want_start else None
            en = torch.empty(n, dtype=torch.int64, device=dev) if want_end else None
        else:
            res, st, en = out
        stream = torch.cuda.current_stream(dev).cuda_stream
        op = offsets.data_ptr() if offsets is not None else None
        if verb in ("match", "search"):
            fdev = l.redgpu_match_batch_dev if verb == "match" else l.redgpu_search_batch_dev
            rc = fdev(exe._h, style, lead, data.data_ptr(), op, stride, n,
                      res.data_ptr(), st.data_ptr() if st is not None else None,
                      en.data_ptr() if en is not None else None, stream)
        else:
            f = l.redgpu_check_batch_dev if verb == "check" else l.redgpu_scan_batch_dev
            rc = f(exe._h, style, lead, data.data_ptr(), op, stride, n, res.data_ptr(), stream)
        _check(rc)
        return res, st, en

    a = _host_u8(data)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
        if len(offsets) and int(offsets[-1]) > a.size:
            raise RedExceptApi("offsets run past the data buffer")
    else:
        if n is None:
            n = a.size // stride if stride else 0
        if stride * n > a.size:
            raise RedExceptApi("stride * n runs past the data buffer")
    res = np.zeros(n, dtype=np.int32)
    st = np.zeros(n, dtype=np.uint64) if want_start else None
    en = np.zeros(n, dtype=np.uint64) if want_end else None
    op = offsets.ctypes.data if offsets is not None else None
    dp = a.ctypes.data if a.size else None
    if _TRACE:
        print("redgpu host call %s n=%d data=%#x+%d offsets=%s res=%#x start=%s end=%s" % (
            verb, n, dp or 0, a.size, "%#x" % op if op else None, res.ctypes.data,
            "%#x" % st.ctypes.data if st is not None else None,
            "%#x" % en.ctypes.data if en is not None else None), flush=True)
    if verb in ("match", "search"):
        fhost = l.redgpu_match_batch if verb == "match" else l.redgpu_search_batch
        rc = fhost(exe._h, style, lead, dp, op, stride, n, res.ctypes.data,
                   st.ctypes.data if st is not None else None,
                   en.ctypes.data if en is not None else None)
    else:
        f = l.redgpu_check_batch if verb == "check" else l.redgpu_scan_batch
        rc = f(exe._h, style, lead, dp, op, stride, n, res.ctypes.data)
    _check(rc)
    return res, st, en


_VERBS = {"check": _lib.VERB_CHECK, "match": _lib.VERB_MATCH, "scan": _lib.VERB_SCAN,
          "search": _lib.VERB_SEARCH}


class Group:
    """One image of the same serialized DFA on each of several GPUs of a node (the device form
    of tools/thr_red.cpp:84-91: N workers over one shared Red).  devices may repeat a device."""

    def __init__(self, serialized: bytes, devices, **flags):
        o = _lib.Opts()
        o.flags = Executable._flags_of(**flags)
        o.lds_table_max = flags.get("lds_table_max", 0)
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        blob = bytes(serialized)
        _check(_lib.lib().redgpu_group_create(blob, len(blob), C.byref(o), devs, len(devices),
                                              C.byref(self._h)))
        self.devices = [int(d) for d in devices]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.redgpu_group_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self, n, *, offsets=None, stride=0):
        """cuts[0..G]: shard g = lines [cuts[g], cuts[g+1]) - equal lines, or equal bytes when
        (host) offsets are given."""
        cuts = np.zeros(len(self.devices) + 1, dtype=np.uint64)
        op = None
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            op = offsets.ctypes.data
        _check(_lib.lib().redgpu_group_plan(self._h, op, stride, n, cuts.ctypes.data))
        return cuts

    def batch(self, verb, data, style, do_leader=True, *, offsets=None, stride=0, n=None):
        """Host buffers: (result, start, end) over all shards, one host thread per device."""
        a = _host_u8(data)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = len(offsets) - 1
        elif n is None:
            n = a.size // stride if stride else 0
        pos = verb in ("match", "search")
        res = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.uint64) if pos else None
        en = np.zeros(n, dtype=np.uint64) if pos else None
        _check(_lib.lib().redgpu_group_batch(
            self._h, _VERBS[verb], int(style), 1 if do_leader else 0,
            a.ctypes.data if a.size else None,
            offsets.ctypes.data if offsets is not None else None, int(stride or 0), n,
            res.ctypes.data, st.ctypes.data if pos else None, en.ctypes.data if pos else None))
        return res, st, en

    def batch_dev(self, verb, shards, style, do_leader=True, *, stride=0, gather="peer"):
        """Device-resident shards: shards[g] = CUDA uint8 tensor on device g, or (data, offsets)
        for ragged lines.  Returns (result, start, end) CUDA tensors on devices[0], complete on
        torch's current stream of that device."""
        import torch
        G = len(self.devices)
        assert len(shards) == G
        datas, offs, ns = [], [], []
        for sh in shards:
            d, o = sh if isinstance(sh, tuple) else (sh, None)
            datas.append(d)
            offs.append(o)
            ns.append((o.numel() - 1) if o is not None else (d.numel() // stride if stride else 0))
        ragged = offs[0] is not None
        total = sum(ns)
        root = torch.device("cuda", self.devices[0])
        pos = verb in ("match", "search")
        res = torch.empty(total, dtype=torch.int32, device=root)
        st = torch.empty(total, dtype=torch.int64, device=root) if pos else None
        en = torch.empty(total, dtype=torch.int64, device=root) if pos else None
        dp = (C.c_void_p * G)(*[d.data_ptr() for d in datas])
        op = (C.c_void_p * G)(*[o.data_ptr() for o in offs]) if ragged else None
        na = (C.c_uint64 * G)(*ns)
        # every shard is ordered against torch's current stream of ITS device: the scan waits for
        # what that stream has queued (the op that produced the shard) and the stream waits for the
        # scan before it may reuse the shard's memory (torch's caching allocator is stream-ordered)
        ss = (C.c_void_p * G)(*[torch.cuda.current_stream(d.device).cuda_stream for d in datas])
        _check(_lib.lib().redgpu_group_batch_dev(
            self._h, _VERBS[verb], int(style), 1 if do_leader else 0, dp, op, int(stride or 0), na,
            res.data_ptr(), st.data_ptr() if pos else None, en.data_ptr() if pos else None,
            _lib.GATHER_RCCL if gather == "rccl" else _lib.GATHER_PEER, ss,
            torch.cuda.current_stream(root).cuda_stream))
        return res, st, en


def check_batch(exe, data, style, do_leader=True, *, offsets=None, stride=0, n=None, out=None):
    """check<style,doLeader> over every line (include/Matcher.h:363-410) -> result int32[n]."""
    return _run("check", exe, style, do_leader, data, offsets, stride, n, False, False,
                None if out is None else (out, None, None))[0]


def scan_batch(exe, data, style, do_leader=True, *, offsets=None, stride=0, n=None, out=None):
    """scan<style,doLeader> over every line (include/Matcher.h:498-554) -> result int32[n]."""
    return _run("scan", exe, style, do_leader, data, offsets, stride, n, False, False,
                None if out is None else (out, None, None))[0]


def match_batch(exe, data, style, do_leader=True, *, offsets=None, stride=0, n=None,
                want_start=True, want_end=True, out=None):
    """match<style,doLeader> over every line (include/Matcher.h:413-495) ->
    (result int32[n], start uint64[n] | None, end uint64[n] | None), the Outcome fields."""
    return _run("match", exe, style, do_leader, data, offsets, stride, n, want_start, want_end,
                out)


def batch_descs(batches, *, stride=0, want_start=True, want_end=True, outs=None, verb="match"):
    """The redgpu_batch array of a *_batches_dev call over CUDA tensors.  batches[k] = data, or
    (data, offsets) for ragged lines; outs[k] = (result, start, end) tensors (allocated when None).
    Returns (descriptor array, outs) - keep both alive until the stream has passed the call."""
    import torch
    pos = verb == "match"
    descs = (_lib.BatchDesc * len(batches))()
    made = []
    for k, sh in enumerate(batches):
        d, o = sh if isinstance(sh, tuple) else (sh, None)
        if not _is_torch(d) or not d.is_cuda or d.dtype != torch.uint8 or not d.is_contiguous():
            raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
        n = (o.numel() - 1) if o is not None else (d.numel() // stride if stride else 0)
        if outs is None or outs[k] is None:
            res = torch.empty(n, dtype=torch.int32, device=d.device)
            st = torch.empty(n, dtype=torch.int64, device=d.device) if pos and want_start else None
            en = torch.empty(n, dtype=torch.int64, device=d.device) if pos and want_end else None
        else:
            res, st, en = outs[k]
        made.append((res, st, en))
        descs[k] = _lib.BatchDesc(d.data_ptr(), o.data_ptr() if o is not None else None,
                                  int(stride or 0), n, res.data_ptr(),
                                  st.data_ptr() if st is not None else None,
                                  en.data_ptr() if en is not None else None)
    return descs, made


def match_batches(exe, batches, style, do_leader=True, *, stride=0, want_start=True,
                  want_end=True, outs=None):
    """match<style,doLeader> over every line of SEVERAL device-resident batches in one call
    (redgpu_match_batches_dev: the caller's loop over its inputs, tools/bench.cpp:60-71) ->
    [(result, start, end)] per batch, complete on torch's current stream."""
    import torch
    descs, made = batch_descs(batches, stride=stride, want_start=want_start, want_end=want_end,
                              outs=outs)
    dev = (batches[0][0] if isinstance(batches[0], tuple) else batches[0]).device
    _check(_lib.lib().redgpu_match_batches_dev(exe._h, int(style), 1 if do_leader else 0, descs,
                                               len(batches),
                                               torch.cuda.current_stream(dev).cuda_stream))
    return made


def check_batches(exe, batches, style, do_leader=True, *, stride=0, outs=None):
    """check<style,doLeader> over several device-resident batches in one call -> [result]."""
    import torch
    descs, made = batch_descs(batches, stride=stride, outs=None if outs is None else
                              [(o, None, None) for o in outs], verb="check")
    dev = (batches[0][0] if isinstance(batches[0], tuple) else batches[0]).device
    _check(_lib.lib().redgpu_check_batches_dev(exe._h, int(style), 1 if do_leader else 0, descs,
                                               len(batches),
                                               torch.cuda.current_stream(dev).cuda_stream))
    return [m[0] for m in made]


def search_batch(exe, data, style, do_leader=True, *, offsets=None, stride=0, n=None,
                 want_start=True, want_end=True, out=None):
    """search<style,doLeader> over every line (include/Matcher.h:557-640): the first match found
    sliding over the line -> (result, start, end) like match_batch."""
    return _run("search", exe, style, do_leader, data, offsets, stride, n, want_start, want_end,
                out)


def _list_dev(entry, head, data, cap, offsets, stride, n, want_start, want_end, out):
    """The device form of the record-list verbs (redgpu_collect_batch_dev,
    redgpu_match_all_batch_dev) over torch CUDA tensors, asynchronous on the current stream ->
    (counts int64[n], result int32[n,cap], start int64[n,cap] | None, end int64[n,cap] | None).
    out = (counts, result, start, end): the caller's tensors instead of fresh ones (contiguous, on
    the data's device, n / n * cap elements; result may be None when cap = 0, start / end None
    for "not wanted"); they are returned as given."""
    import torch
    if not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
        raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
    cap = int(cap)
    if cap < 0:
        raise RedExceptApi("cap must be >= 0")
    dev = data.device
    if offsets is not None:
        if (not _is_torch(offsets) or offsets.dtype not in (torch.int64, torch.uint64)
                or not offsets.is_cuda or not offsets.is_contiguous()):
            raise RedExceptApi("device offsets must be a contiguous int64 CUDA tensor")
        n = offsets.numel() - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
    elif n is None:
        n = data.numel() // stride if stride else 0
    if out is None:
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        res = torch.empty((n, cap), dtype=torch.int32, device=dev)
        st = torch.empty((n, cap), dtype=torch.int64, device=dev) if want_start else None
        en = torch.empty((n, cap), dtype=torch.int64, device=dev) if want_end else None
    else:
        counts, res, st, en = out
        need = [(counts, 8, n)] + ([(res, 4, n * cap)] if cap or res is not None else [])
        need += [(t, 8, n * cap) for t in (st, en) if t is not None]
        for t, size, room in need:
            if (not _is_torch(t) or t.device != dev or not t.is_contiguous() or
                    t.element_size() != size or t.numel() < room):
                raise RedExceptApi("out tensors must be contiguous, on the data's device and hold "
                                   "n counts / n * cap records")

    def ptr(t):
        return t.data_ptr() if t is not None and t.numel() else None

    _check(entry(*head, ptr(data), offsets.data_ptr() if offsets is not None else None, stride, n,
                 cap, ptr(counts), ptr(res), ptr(st), ptr(en),
                 torch.cuda.current_stream(dev).cuda_stream))
    return counts, res, st, en


def collect_batch(exe, data, cap, *, offsets=None, stride=0, n=None, want_start=True,
                  want_end=True, out=None):
    """Red::collect (lib/Red.cpp:103-116) over every line: all non-overlapping matches in order.
    Host arrays in, host arrays out: (counts uint64[n], result int32[n,cap], start uint64[n,cap],
    end uint64[n,cap]); counts[i] may exceed cap (only the first cap records are kept).
    torch CUDA tensors in (data uint8, offsets int64): redgpu_collect_batch_dev, asynchronous on
    the current stream, CUDA tensors out (_list_dev: want_start / want_end = False pass that
    array as NULL and return None for it; out = the caller's output tensors)."""
    if _is_torch(data):
        return _list_dev(_lib.lib().redgpu_collect_batch_dev, (exe._h,), data, cap, offsets, stride,
                         n, want_start, want_end, out)
    if out is not None or not (want_start and want_end):
        raise RedExceptApi("out=, want_start= and want_end= go with CUDA tensor input")
    a = _host_u8(data)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
    elif n is None:
        n = a.size // stride if stride else 0
    counts = np.zeros(n, dtype=np.uint64)
    res = np.zeros((n, cap), dtype=np.int32)
    st = np.zeros((n, cap), dtype=np.uint64)
    en = np.zeros((n, cap), dtype=np.uint64)
    _check(_lib.lib().redgpu_collect_batch(
        exe._h, a.ctypes.data if a.size else None,
        offsets.ctypes.data if offsets is not None else None, stride, n, cap, counts.ctypes.data,
        res.ctypes.data, st.ctypes.data, en.ctypes.data))
    return counts, res, st, en


def collect(exe, text: bytes, cap: int = 64):
    """Red::collect on one text -> list of (result, start, end)."""
    counts, res, st, en = collect_batch(exe, text, cap, offsets=[0, len(text)])
    k = int(min(counts[0], cap))
    return [(int(res[0, i]), int(st[0, i]), int(en[0, i])) for i in range(k)]


def _device_text(text):
    """a long-text verb's device input, checked -> (device, torch's current stream on it)"""
    import torch
    if not text.is_cuda or text.dtype != torch.uint8 or not text.is_contiguous():
        raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
    return text.device, torch.cuda.current_stream(text.device)


def _delim_byte(delim) -> int:
    """a raw-text verb's delim - bytes (the first one counts) or an int - as the C calls' byte"""
    return delim[0] if isinstance(delim, (bytes, bytearray)) else int(delim)


def _device_raw_text(data):
    """a raw-text verb's device input, checked -> (device, its pointer or None when empty, its
    length, the handle of torch's current stream on the device)"""
    dev, stream = _device_text(data)
    return dev, data.data_ptr() if data.numel() else None, data.numel(), stream.cuda_stream


def _device_out_room(verb, data, out, out_cap):
    """the output of a text-output verb's device form -> (out, room): out= is checked, out_cap
    alone makes a tensor of that size; the room is out's size, or out_cap where that is smaller"""
    import torch
    if out is None and out_cap is None:
        raise RedExceptApi("device %s needs out or out_cap (room for the output)" % verb)
    if out is None:
        out = torch.empty(int(out_cap), dtype=torch.uint8, device=data.device)
    elif (not _is_torch(out) or not out.is_cuda or out.dtype != torch.uint8 or
          not out.is_contiguous() or out.device != data.device):
        raise RedExceptApi("out must be a contiguous uint8 CUDA tensor on the text's device")
    return out, out.numel() if out_cap is None else min(int(out_cap), out.numel())


def _host_text_only(out, out_cap):
    """a text-output verb with a host text takes neither out= nor out_cap="""
    if out is not None or out_cap is not None:
        raise RedExceptApi("out= and out_cap= go with a CUDA tensor text")


def _host_text_out(cap, call):
    """the output of a text-output verb's host form: call(buffer pointer, cap) -> out_len with a
    buffer of cap bytes, once more with the exact size when that was too small (never, where cap
    is the text's length and the output no longer than the text) -> the output's bytes"""
    cap = int(cap)
    for _ in range(2):
        buf = np.zeros(max(cap, 1), dtype=np.uint8)
        out_len = int(call(buf.ctypes.data, cap))
        if out_len <= cap:
            break
        cap = out_len
    return buf[:out_len].tobytes()


def _long_records(entry, head, text, cap, chunk_bytes):
    """collect_long / match_all_long: redgpu_<entry>[_dev](*head, data, len, chunk_bytes, room,
    count, result, start, end[, stream]) over a host or a device text; with cap=None once more
    with room for every record when the first 4096 slots were not enough"""
    if cap is not None and cap < 0:
        raise RedExceptApi("cap must be >= 0")
    room = 4096 if cap is None else cap
    if _is_torch(text):
        import torch
        dev, stream = _device_text(text)
        for _ in range(2):
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            res = torch.empty(max(room, 1), dtype=torch.int32, device=dev)
            st = torch.empty(max(room, 1), dtype=torch.int64, device=dev)
            en = torch.empty(max(room, 1), dtype=torch.int64, device=dev)
            _check(getattr(_lib.lib(), "redgpu_%s_dev" % entry)(
                *head, text.data_ptr() if text.numel() else None, text.numel(), int(chunk_bytes),
                room, cnt.data_ptr(), res.data_ptr(), st.data_ptr(), en.data_ptr(),
                stream.cuda_stream))
            count = int(cnt.item())
            if cap is not None or count <= room:
                break
            room = count
    else:
        a = _host_u8(text)
        for _ in range(2):
            cnt = C.c_uint64(0)
            res = np.zeros(max(room, 1), dtype=np.int32)
            st = np.zeros(max(room, 1), dtype=np.uint64)
            en = np.zeros(max(room, 1), dtype=np.uint64)
            _check(getattr(_lib.lib(), "redgpu_" + entry)(
                *head, a.ctypes.data if a.size else None, a.size, int(chunk_bytes), room,
                C.byref(cnt), res.ctypes.data, st.ctypes.data, en.ctypes.data))
            count = int(cnt.value)
            if cap is not None or count <= room:
                break
            room = count
    k = min(count, room)
    return count, res[:k], st[:k], en[:k]


def collect_long(exe, text, cap=None, *, chunk_bytes=0):
    """Red::collect (lib/Red.cpp:103-116) over ONE long text, chunk-parallel on the GPU
    (redgpu_collect_long[_dev]) -> (count, result int32[k], start uint64[k], end uint64[k]) with
    k = min(count, cap).  text: bytes / numpy uint8 (staged by the library) or a contiguous uint8
    CUDA tensor (the _dev form on torch's current stream; the arrays come back as CUDA tensors and
    count as an int after a synchronisation of that stream).  cap=None: room for every match (a
    second call when the first 4096 slots were not enough).  chunk_bytes=0: automatic."""
    return _long_records("collect_long", (exe._h,), text, cap, chunk_bytes)


def match_all_long(exe, text, cap=None, do_leader=True, *, chunk_bytes=0):
    """matchAll (include/Matcher.h:711-766; lib/Matcher.cpp:97-102 runs it with doLeader = true)
    over ONE long text, chunk-parallel on the GPU (redgpu_match_all_long[_dev]) -> (count, result
    int32[k], start uint64[k], end uint64[k]) with k = min(count, cap).  text, cap and chunk_bytes
    as in collect_long: bytes / numpy uint8, or a contiguous uint8 CUDA tensor on torch's current
    stream (the arrays then come back as CUDA tensors)."""
    return _long_records("match_all_long", (exe._h, 1 if do_leader else 0), text, cap, chunk_bytes)


def match_all_batch(exe, data, cap, do_leader=True, *, offsets=None, stride=0, n=None,
                    want_start=True, want_end=True, out=None):
    """matchAll (include/Matcher.h:711-766; the reference's public entry, lib/Matcher.cpp:97-102,
    runs with doLeader = true) over every line: one anchored walk reporting each maximal run of
    one accepted result.  Same return shape as collect_batch, and the same device form for torch
    CUDA tensors (redgpu_match_all_batch_dev)."""
    if _is_torch(data):
        return _list_dev(_lib.lib().redgpu_match_all_batch_dev, (exe._h, int(bool(do_leader))),
                         data, cap, offsets, stride, n, want_start, want_end, out)
    if out is not None or not (want_start and want_end):
        raise RedExceptApi("out=, want_start= and want_end= go with CUDA tensor input")
    a = _host_u8(data)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
    elif n is None:
        n = a.size // stride if stride else 0
    counts = np.zeros(n, dtype=np.uint64)
    res = np.zeros((n, cap), dtype=np.int32)
    st = np.zeros((n, cap), dtype=np.uint64)
    en = np.zeros((n, cap), dtype=np.uint64)
    _check(_lib.lib().redgpu_match_all_batch(
        exe._h, int(bool(do_leader)), a.ctypes.data if a.size else None,
        offsets.ctypes.data if offsets is not None else None, stride, n, cap, counts.ctypes.data,
        res.ctypes.data, st.ctypes.data, en.ctypes.data))
    return counts, res, st, en


def match_all(exe, text: bytes, cap: int = 64):
    """matchAll(exec, text, out) on one text -> list of (result, start, end)."""
    counts, res, st, en = match_all_batch(exe, text, cap, True, offsets=[0, len(text)])
    k = int(min(counts[0], cap))
    return [(int(res[0, i]), int(st[0, i]), int(en[0, i])) for i in range(k)]


STATE_INITIAL = 0xFFFFFFFF


def advance_batch(exe, data, state, *, offsets=None, stride=0, n=None, out=None):
    """n StatefulMatchers (include/Matcher.h:770-792) advanced by one chunk each.
    `state` (uint32[n], in/out, updated in place) holds each matcher's state token -
    STATE_INITIAL for a fresh matcher; returns result int32[n] = result() after the chunk.
    numpy arrays run through the host entry point, torch CUDA tensors (data uint8, state int32
    viewed as u32) asynchronously on the current stream."""
    l = _lib.lib()
    if _is_torch(data):
        import torch
        if not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
            raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
        dev = data.device
        if offsets is not None:
            if (not _is_torch(offsets) or offsets.dtype not in (torch.int64, torch.uint64)
                    or not offsets.is_cuda or not offsets.is_contiguous()):
                raise RedExceptApi("device offsets must be a contiguous int64 CUDA tensor")
            n = offsets.numel() - 1
            stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
        elif n is None:
            n = data.numel() // stride if stride else 0
        if (not _is_torch(state) or state.numel() != n or state.element_size() != 4 or
                state.device != dev or not state.is_contiguous()):
            raise RedExceptApi("state must be a 4-byte tensor of n elements on the data's device")
        res = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
        _check(l.redgpu_advance_batch_dev(
            exe._h, data.data_ptr(), offsets.data_ptr() if offsets is not None else None, stride,
            n, state.data_ptr(), res.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return res
    a = _host_u8(data)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
    elif n is None:
        n = a.size // stride if stride else 0
    if not (isinstance(state, np.ndarray) and state.dtype == np.uint32 and state.size == n and
            state.flags.c_contiguous):
        raise RedExceptApi("state must be a contiguous uint32 array of n elements")
    res = np.zeros(n, dtype=np.int32)
    _check(l.redgpu_advance_batch(exe._h, a.ctypes.data if a.size else None,
                                  offsets.ctypes.data if offsets is not None else None, stride,
                                  n, state.ctypes.data, res.ctypes.data))
    return res


def replace_batch(exe, data, repl: bytes, style, do_leader=True, max_count=(1 << 62), *,
                  offsets=None, stride=0, n=None, out=None, out_cap=None, sizes=None):
    """replace<style,doLeader> (include/Matcher.h:643-706) over every line: each match replaced
    by `repl`, at most max_count per line.  Host arrays in and out:
    (counts uint64[n], out_offsets uint64[n+1], out uint8[out_offsets[n]]).
    torch CUDA tensors in (data uint8, offsets int64): redgpu_replace_batch_dev in ONE call,
    asynchronous on the current stream -> (counts int64[n], out_offsets int64[n+1], out).  out =
    a contiguous uint8 CUDA tensor to write into and out_cap its capacity (default: its size):
    every line that fits entirely below out_cap is written, nothing is retried; out = None gives
    the sizes only.  sizes = (counts, out_offsets): the caller's tensors instead of fresh ones."""
    if _is_torch(data):
        import torch
        if not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
            raise RedExceptApi("device input must be a contiguous uint8 CUDA tensor")
        dev = data.device
        if offsets is not None:
            if (not _is_torch(offsets) or offsets.dtype not in (torch.int64, torch.uint64)
                    or not offsets.is_cuda or not offsets.is_contiguous()):
                raise RedExceptApi("device offsets must be a contiguous int64 CUDA tensor")
            n = offsets.numel() - 1
            stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
        elif n is None:
            n = data.numel() // stride if stride else 0
        if out is not None:
            if (not _is_torch(out) or not out.is_cuda or out.dtype != torch.uint8 or
                    not out.is_contiguous() or out.device != dev):
                raise RedExceptApi("out must be a contiguous uint8 CUDA tensor on the data's device")
            out_cap = out.numel() if out_cap is None else int(out_cap)
            if not 0 <= out_cap <= out.numel():
                raise RedExceptApi("out_cap runs past the out tensor")
        elif out_cap:
            raise RedExceptApi("out_cap goes with out=")
        if sizes is None:
            counts = torch.empty(n, dtype=torch.int64, device=dev)
            ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        else:
            counts, ooff = sizes
            for t, room in ((counts, n), (ooff, n + 1)):
                if (not _is_torch(t) or t.device != dev or not t.is_contiguous() or
                        t.element_size() != 8 or t.numel() < room):
                    raise RedExceptApi("sizes tensors must be contiguous, on the data's device and "
                                       "hold n counts / n + 1 offsets")
        r = np.frombuffer(bytes(repl), dtype=np.uint8)
        drepl = torch.from_numpy(r.copy()).to(dev) if r.size else None
        _check(_lib.lib().redgpu_replace_batch_dev(
            exe._h, int(style), 1 if do_leader else 0, data.data_ptr() if data.numel() else None,
            offsets.data_ptr() if offsets is not None else None, stride, n,
            drepl.data_ptr() if drepl is not None else None, r.size, int(max_count),
            counts.data_ptr(), ooff.data_ptr(), out.data_ptr() if out is not None else None,
            out_cap if out is not None else 0, torch.cuda.current_stream(dev).cuda_stream))
        return counts, ooff, out
    if out is not None or out_cap is not None or sizes is not None:
        raise RedExceptApi("out=, out_cap= and sizes= go with CUDA tensor input")
    a = _host_u8(data)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = int(stride or 0)  # with offsets: trailing bytes to drop per line
    elif n is None:
        n = a.size // stride if stride else 0
    counts = np.zeros(n, dtype=np.uint64)
    ooff = np.zeros(n + 1, dtype=np.uint64)
    r = np.frombuffer(bytes(repl), dtype=np.uint8)
    f = _lib.lib().redgpu_replace_batch
    args = (exe._h, int(style), 1 if do_leader else 0, a.ctypes.data if a.size else None,
            offsets.ctypes.data if offsets is not None else None, stride, n,
            r.ctypes.data if r.size else None, r.size, int(max_count), counts.ctypes.data,
            ooff.ctypes.data)
    # first guess: output about as long as the input; retry once with the exact size
    cap = int(a.size + 64)
    out = np.zeros(cap, dtype=np.uint8)
    _check(f(*args, out.ctypes.data, cap))
    total = int(ooff[n]) if n else 0
    if total > cap:
        out = np.zeros(total, dtype=np.uint8)
        _check(f(*args, out.ctypes.data, total))
    return counts, ooff, out[:total]


def replace(exe, text: bytes, repl: bytes, max_count, style, do_leader=True):
    """replace(exec, text, repl, out, max, style) on one text -> (count, rewritten bytes)."""
    counts, ooff, out = replace_batch(exe, text, repl, style, do_leader, max_count,
                                      offsets=[0, len(text)])
    return int(counts[0]), out.tobytes()


def replace_long(exe, text, repl: bytes, style=styLast, do_leader=True, max_count=(1 << 62), *,
                 chunk_bytes=0, out=None):
    """replace<style,doLeader> (include/Matcher.h:643-706; what Red's replaceOne* / replaceAll*,
    include/Red.h:139-238, end in) over ONE long text, chunk-parallel on the GPU
    (redgpu_replace_long[_dev]) -> (count, rewritten).  text: bytes / numpy uint8 (staged by the
    library; rewritten comes back as bytes) or a contiguous uint8 CUDA tensor (the _dev form on
    torch's current stream: a sizes-only call, then an output tensor of exactly out_len bytes;
    rewritten is a CUDA uint8 tensor and count an int after a synchronisation of that stream).
    out=: a contiguous uint8 CUDA tensor to write into, in ONE call - rewritten is then
    out[:min(out_len, out.numel())] and the third value returned is out_len.  max_count=1 is
    replaceOne*.  chunk_bytes=0: automatic."""
    r = np.frombuffer(bytes(repl), dtype=np.uint8)
    l = _lib.lib()
    if _is_torch(text):
        import torch
        dev, stream = _device_text(text)
        drepl = torch.from_numpy(r.copy()).to(dev) if r.size else None
        sizes = torch.zeros(2, dtype=torch.int64, device=dev)

        def call(o):
            _check(l.redgpu_replace_long_dev(
                exe._h, int(style), 1 if do_leader else 0,
                text.data_ptr() if text.numel() else None, text.numel(), int(chunk_bytes),
                drepl.data_ptr() if drepl is not None else None, r.size, int(max_count),
                sizes.data_ptr(), sizes.data_ptr() + 8, o.data_ptr() if o is not None and o.numel() else None,
                o.numel() if o is not None else 0, stream.cuda_stream))
            return [int(v) for v in sizes.tolist()]

        if out is not None:
            _device_out_room("replace_long", text, out, None)
            count, out_len = call(out)
            return count, out[:min(out_len, out.numel())], out_len
        count, out_len = call(None)
        res = torch.empty(out_len, dtype=torch.uint8, device=dev)
        if out_len:
            call(res)
        return count, res
    if out is not None:
        raise RedExceptApi("out= goes with a CUDA tensor text")
    a = _host_u8(text)
    cnt = C.c_uint64(0)
    olen = C.c_uint64(0)

    def host_call(buf, cap):
        _check(l.redgpu_replace_long(
            exe._h, int(style), 1 if do_leader else 0, a.ctypes.data if a.size else None, a.size,
            int(chunk_bytes), r.ctypes.data if r.size else None, r.size, int(max_count),
            C.byref(cnt), C.byref(olen), buf, cap))
        return olen.value

    # first guess: output about as long as the input
    rewritten = _host_text_out(a.size + 64, host_call)
    return int(cnt.value), rewritten


def search_long(exe, text, style=styLast, do_leader=True, *, chunk_bytes=0):
    """search<style,doLeader> (include/Matcher.h:172-173, core :557-640; what Red's search* and
    partialMatch end in) over ONE long text, chunk-parallel on the GPU (redgpu_search_long[_dev])
    -> (result, start, end): the match of the lowest start position, (0, 0, 0) without one.
    text: bytes / numpy uint8 (staged by the library; three ints come back) or a contiguous uint8
    CUDA tensor (the _dev form on torch's current stream: three one-element CUDA tensors - int32,
    int64, int64 - and no synchronisation).  A match near the front ends the call early.
    chunk_bytes=0: automatic."""
    l = _lib.lib()
    if _is_torch(text):
        import torch
        dev, stream = _device_text(text)
        res = torch.empty(1, dtype=torch.int32, device=dev)
        pos = torch.empty(2, dtype=torch.int64, device=dev)
        _check(l.redgpu_search_long_dev(
            exe._h, int(style), 1 if do_leader else 0, text.data_ptr() if text.numel() else None,
            text.numel(), int(chunk_bytes), res.data_ptr(), pos.data_ptr(), pos.data_ptr() + 8,
            stream.cuda_stream))
        return res, pos[0:1], pos[1:2]
    a = _host_u8(text)
    res, st, en = C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
    _check(l.redgpu_search_long(exe._h, int(style), 1 if do_leader else 0,
                                a.ctypes.data if a.size else None, a.size, int(chunk_bytes),
                                C.byref(res), C.byref(st), C.byref(en)))
    return int(res.value), int(st.value), int(en.value)


def split_lines(exe, data, delim=b"\n", cap=None):
    """redgpu_split_lines: offsets of the delimiter-terminated lines of a raw text buffer, found
    on the device (the rule of lib/Util.cpp:109-130: bytes after the last delimiter are not a
    line).  Line k = data[offsets[k] : offsets[k+1]] INCLUDING its delimiter - pass the offsets
    to the *_batch verbs with stride=1.  Returns (offsets, n_found): numpy uint64[min(n, cap)+1]
    for host input; for a CUDA uint8 tensor, an int64 tensor of cap+1 entries and a 1-element
    int64 tensor, both on the device, asynchronously on the current stream."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if _is_torch(data):
        import torch
        dev, _, _, stream = _device_raw_text(data)
        if cap is None:
            raise RedExceptApi("device split_lines needs cap (room in the offsets tensor)")
        offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        _check(l.redgpu_split_lines_dev(exe._h, data.data_ptr(), data.numel(), d, offs.data_ptr(),
                                        cap, cnt.data_ptr(), stream))
        return offs, cnt
    a = _host_u8(data)
    cnt = C.c_uint64(0)
    dp = a.ctypes.data if a.size else None
    if cap is None:
        # size the result exactly: a first call that keeps no line only counts
        one = np.zeros(1, dtype=np.uint64)
        _check(l.redgpu_split_lines(exe._h, dp, a.size, d, one.ctypes.data, 0, C.byref(cnt)))
        cap = int(cnt.value)
    offs = np.zeros(cap + 1, dtype=np.uint64)
    _check(l.redgpu_split_lines(exe._h, dp, a.size, d, offs.ctypes.data, cap, C.byref(cnt)))
    return offs[: min(cnt.value, cap) + 1], int(cnt.value)


def match_text(exe, data, style, do_leader=True, *, delim=b"\n", cap=None, want_start=True,
               want_end=True):
    """redgpu_match_text[_dev]: the delimiter-terminated lines of a raw text buffer, each
    matched (tools/skim_red.cpp:36-46 over lib/Util.cpp:109-130's lines), in one call.
    Host input -> (offsets uint64[k+1], n_found, result int32[k], start | None, end | None) with
    k = min(n_found, cap); cap=None sizes the arrays with a counting call first.
    A CUDA uint8 tensor -> (offsets int64[cap+1], count int64[1], result int32[cap], start, end)
    tensors, asynchronously on the current stream; entries from min(count, cap) on are untouched.
    want_start = want_end = False is check<style,doLeader>."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if _is_torch(data):
        import torch
        dev, _, _, stream = _device_raw_text(data)
        if cap is None:
            raise RedExceptApi("device match_text needs cap (room in the output tensors)")
        offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        res = torch.empty(cap, dtype=torch.int32, device=dev)
        st = torch.empty(cap, dtype=torch.int64, device=dev) if want_start else None
        en = torch.empty(cap, dtype=torch.int64, device=dev) if want_end else None
        if st is None and en is None:
            _check(l.redgpu_check_text_dev(exe._h, int(style), 1 if do_leader else 0,
                                           data.data_ptr(), data.numel(), d, offs.data_ptr(), cap,
                                           cnt.data_ptr(), res.data_ptr(), stream))
        else:
            _check(l.redgpu_match_text_dev(exe._h, int(style), 1 if do_leader else 0,
                                           data.data_ptr(), data.numel(), d, offs.data_ptr(), cap,
                                           cnt.data_ptr(), res.data_ptr(),
                                           st.data_ptr() if st is not None else None,
                                           en.data_ptr() if en is not None else None, stream))
        return offs, cnt, res, st, en
    a = _host_u8(data)
    dp = a.ctypes.data if a.size else None
    cnt = C.c_uint64(0)
    if cap is None:
        one = np.zeros(1, dtype=np.uint64)
        _check(l.redgpu_split_lines(exe._h, dp, a.size, d, one.ctypes.data, 0, C.byref(cnt)))
        cap = int(cnt.value)
    offs = np.zeros(cap + 1, dtype=np.uint64)
    res = np.zeros(cap, dtype=np.int32)
    st = np.zeros(cap, dtype=np.uint64) if want_start else None
    en = np.zeros(cap, dtype=np.uint64) if want_end else None
    _check(l.redgpu_match_text(exe._h, int(style), 1 if do_leader else 0, dp, a.size, d,
                               offs.ctypes.data, cap, C.byref(cnt), res.ctypes.data,
                               st.ctypes.data if st is not None else None,
                               en.ctypes.data if en is not None else None))
    k = min(int(cnt.value), cap)
    return (offs[:k + 1], int(cnt.value), res[:k], st[:k] if st is not None else None,
            en[:k] if en is not None else None)


def grep_text(exe, data, style=styInstant, do_leader=True, *, invert=False, delim=b"\n", cap=None,
              max_count=1 << 62, want_outcome=True):
    """redgpu_grep_text[_dev]: the delimiter-terminated lines of a raw text buffer that
    search<style,doLeader> selects (result > 0; invert=True: the others, grep -v), as compact
    records in text order - include/Red.h:65's "appropriate for grep", tools/skim_red.cpp:36-46's
    loop.  Record j: line[j] = the line's 0-based index, begin[j] / finish[j] = the offsets of its
    first byte and of its delimiter, result / start / end[j] = the Outcome of search on that line
    alone (positions relative to begin[j]; (0, 0, 0) under invert).  n_selected = min(selected
    lines, max_count) (grep -m) and may exceed cap.
    Host input -> (n_lines, n_selected, line, begin, finish, result, start, end): numpy arrays
    trimmed to min(n_selected, cap); cap=None sizes them with a counting call first (the text is
    then uploaded twice - pass a cap to avoid that - unless nothing is selected); cap=0 only
    counts (grep -c).  want_outcome=False leaves result / start / end None (no line is walked a
    second time).
    A CUDA uint8 tensor needs cap -> the same tuple as device tensors, n_lines and n_selected as
    1-element int64 tensors, asynchronously on the current stream and without any read-back;
    entries from min(n_selected, cap) on are untouched."""
    l = _lib.lib()
    d = _delim_byte(delim)
    style, lead, inv = int(style), 1 if do_leader else 0, 1 if invert else 0
    max_count = int(max_count)
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        if cap is None:
            raise RedExceptApi("device grep_text needs cap (room in the output tensors)")
        cnt = torch.empty(2, dtype=torch.int64, device=dev)
        ln, bg, fn = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(3))
        res = torch.empty(cap, dtype=torch.int32, device=dev) if want_outcome else None
        st = torch.empty(cap, dtype=torch.int64, device=dev) if want_outcome else None
        en = torch.empty(cap, dtype=torch.int64, device=dev) if want_outcome else None
        _check(l.redgpu_grep_text_dev(
            exe._h, style, lead, inv, ptr, size, d, max_count, cap, cnt.data_ptr(),
            cnt.data_ptr() + 8, ln.data_ptr(), bg.data_ptr(), fn.data_ptr(),
            res.data_ptr() if want_outcome else None, st.data_ptr() if want_outcome else None,
            en.data_ptr() if want_outcome else None, stream))
        return cnt[0:1], cnt[1:2], ln, bg, fn, res, st, en
    a = _host_u8(data)
    dp = a.ctypes.data if a.size else None
    nl, ns = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        _check(l.redgpu_grep_text(exe._h, style, lead, inv, dp, a.size, d, max_count, 0,
                                  C.byref(nl), C.byref(ns), None, None, None, None, None, None))
        cap = int(ns.value)
        if cap == 0:  # nothing selected: the counting call said it all
            none = lambda dt: np.zeros(0, dtype=dt) if want_outcome else None  # noqa: E731
            u = np.zeros(0, dtype=np.uint64)
            return (int(nl.value), 0, u, u.copy(), u.copy(), none(np.int32), none(np.uint64),
                    none(np.uint64))
    cap = int(cap)
    ln, bg, fn = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    res = np.zeros(cap, dtype=np.int32) if want_outcome else None
    st = np.zeros(cap, dtype=np.uint64) if want_outcome else None
    en = np.zeros(cap, dtype=np.uint64) if want_outcome else None
    _check(l.redgpu_grep_text(
        exe._h, style, lead, inv, dp, a.size, d, max_count, cap, C.byref(nl), C.byref(ns),
        ln.ctypes.data, bg.ctypes.data, fn.ctypes.data,
        res.ctypes.data if want_outcome else None, st.ctypes.data if want_outcome else None,
        en.ctypes.data if want_outcome else None))
    k = min(int(ns.value), cap)
    cut = lambda x: x[:k] if x is not None else None  # noqa: E731
    return (int(nl.value), int(ns.value), ln[:k], bg[:k], fn[:k], cut(res), cut(st), cut(en))


def collect_text(exe, data, *, delim=b"\n", cap=None, want_positions=True):
    """redgpu_collect_text[_dev]: grep -o - every match of every delimiter-terminated line of a raw
    text buffer, as compact records in text order: Red::collect (lib/Red.cpp:103-116) inside
    tools/skim_red.cpp:36-46's line loop.  Record j: line[j] = the line's 0-based index, begin[j] =
    the offset of its first byte, result[j], and start[j] / end[j] as ABSOLUTE offsets in the text
    (collect_long's convention; start[j] - begin[j] is the position in the line).  n_matches is the
    number of records found and may exceed cap: the cap cuts the whole list, never a line's.
    Host input -> (n_lines, n_matches, line, begin, result, start, end): numpy arrays trimmed to
    min(n_matches, cap); cap=None sizes them with a counting call first (the text is then uploaded
    twice - pass a cap to avoid that - unless nothing matches); cap=0 only counts.
    want_positions=False leaves start / end None.
    A CUDA uint8 tensor needs cap -> the same tuple as device tensors, n_lines and n_matches as
    1-element int64 tensors, asynchronously on the current stream and without any read-back;
    entries from min(n_matches, cap) on are untouched."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        if cap is None:
            raise RedExceptApi("device collect_text needs cap (room in the output tensors)")
        cnt = torch.empty(2, dtype=torch.int64, device=dev)
        ln, bg = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2))
        res = torch.empty(cap, dtype=torch.int32, device=dev)
        st = torch.empty(cap, dtype=torch.int64, device=dev) if want_positions else None
        en = torch.empty(cap, dtype=torch.int64, device=dev) if want_positions else None
        _check(l.redgpu_collect_text_dev(
            exe._h, ptr, size, d, cap, cnt.data_ptr(), cnt.data_ptr() + 8, ln.data_ptr(),
            bg.data_ptr(), res.data_ptr(), st.data_ptr() if want_positions else None,
            en.data_ptr() if want_positions else None, stream))
        return cnt[0:1], cnt[1:2], ln, bg, res, st, en
    a = _host_u8(data)
    dp = a.ctypes.data if a.size else None
    nl, nm = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        _check(l.redgpu_collect_text(exe._h, dp, a.size, d, 0, C.byref(nl), C.byref(nm), None, None,
                                     None, None, None))
        cap = int(nm.value)
        if cap == 0:  # nothing matches: the counting call said it all
            pos = lambda: np.zeros(0, dtype=np.uint64) if want_positions else None  # noqa: E731
            u = np.zeros(0, dtype=np.uint64)
            return int(nl.value), 0, u, u.copy(), np.zeros(0, dtype=np.int32), pos(), pos()
    cap = int(cap)
    ln, bg = (np.zeros(cap, dtype=np.uint64) for _ in range(2))
    res = np.zeros(cap, dtype=np.int32)
    st = np.zeros(cap, dtype=np.uint64) if want_positions else None
    en = np.zeros(cap, dtype=np.uint64) if want_positions else None
    _check(l.redgpu_collect_text(
        exe._h, dp, a.size, d, cap, C.byref(nl), C.byref(nm), ln.ctypes.data, bg.ctypes.data,
        res.ctypes.data, st.ctypes.data if want_positions else None,
        en.ctypes.data if want_positions else None))
    k = min(int(nm.value), cap)
    cut = lambda x: x[:k] if x is not None else None  # noqa: E731
    return int(nl.value), int(nm.value), ln[:k], bg[:k], res[:k], cut(st), cut(en)


TALLY_LINES, TALLY_MATCHES = 0, 1
UNIQ_LINES, UNIQ_MATCHES = 0, 1
SUM_FIRST, SUM_LAST = 0, 1
SUM_COUNT, SUM_SUM, SUM_MIN, SUM_MAX = 0, 1, 2, 3  # the rows of sum_text's stats
_SUM_WHICH = {"first": SUM_FIRST, "last": SUM_LAST}


def tally_text(exe, data, n_bins=None, *, matches=True, style=styInstant, do_leader=True,
               delim=b"\n", into=None):
    """redgpu_tally_text[_dev]: grep -c per result (matches=False: one item per delimiter-terminated
    line, its value the result of search<style,doLeader> on the line, 0 when it does not match) or
    grep -o | sort | uniq -c (matches=True: one item per record collect_text would report, its
    value the record's result) - only the histogram leaves the device.  bins has n_bins + 1 slots:
    bins[r] counts the items of value r < n_bins, bins[n_bins] everything else; n_bins=None means
    exe.info["max_result"] + 1, so that every result has a slot of its own.  n_items = the items of
    value > 0 (the selected lines / the matches).  Counts are exact 64-bit integer sums.
    Host input -> (n_lines, n_items, bins): bins a uint64 array of n_bins + 1; into= takes such an
    array and ADDS to it (a stream of buffers tallied into one histogram) and returns it.
    A CUDA uint8 tensor -> the same tuple as device tensors, n_lines and n_items as 1-element int64
    tensors and bins as int64 (into= an int64 CUDA tensor of n_bins + 1), asynchronously on the
    current stream and without any read-back."""
    l = _lib.lib()
    d = _delim_byte(delim)
    what = TALLY_MATCHES if matches else TALLY_LINES
    style, lead = int(style), 1 if do_leader else 0
    n_bins = int(exe.info["max_result"]) + 1 if n_bins is None else int(n_bins)
    if n_bins < 0:
        raise RedExceptApi("n_bins must not be negative")
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        if into is None:
            bins = torch.empty(n_bins + 1, dtype=torch.int64, device=dev)
        else:
            if (not _is_torch(into) or not into.is_cuda or into.device != dev or
                    into.dtype != torch.int64 or not into.is_contiguous() or
                    into.numel() != n_bins + 1):
                raise RedExceptApi("into must be a contiguous int64 CUDA tensor of n_bins + 1 on "
                                   "the input's device")
            bins = into
        cnt = torch.empty(2, dtype=torch.int64, device=dev)
        _check(l.redgpu_tally_text_dev(
            exe._h, what, style, lead, ptr, size, d, n_bins, 0 if into is None else 1,
            cnt.data_ptr(), cnt.data_ptr() + 8, bins.data_ptr(), stream))
        return cnt[0:1], cnt[1:2], bins
    a = _host_u8(data)
    dp = a.ctypes.data if a.size else None
    if into is None:
        bins = np.zeros(n_bins + 1, dtype=np.uint64)
    else:
        if (not isinstance(into, np.ndarray) or into.dtype != np.uint64 or into.ndim != 1 or
                into.size != n_bins + 1 or not into.flags.c_contiguous):
            raise RedExceptApi("into must be a contiguous uint64 array of n_bins + 1")
        bins = into
    nl, ni = C.c_uint64(0), C.c_uint64(0)
    _check(l.redgpu_tally_text(exe._h, what, style, lead, dp, a.size, d, n_bins,
                               0 if into is None else 1, C.byref(nl), C.byref(ni),
                               bins.ctypes.data))
    return int(nl.value), int(ni.value), bins


def sum_text(exe, data, n_bins=None, *, which="first", max_per_line=1 << 62, delim=b"\n",
             into=None):
    """redgpu_sum_text[_dev]: per result the count, sum, minimum and maximum of the decimal numbers
    found in a raw text's matches - awk '{ n[c]++; s[c] += $x; if ($x > m[c]) m[c] = $x }'.  The
    items are extract_text's pieces (at most max_per_line of a line), an item's slot is
    collect_text's result for it (slot r for r < n_bins, else slot n_bins; n_bins=None means
    exe.info["max_result"] + 1), its number the first (which="first") or last (which="last") run
    of digits 0-9 inside the piece, read as an unsigned decimal.  An item without a digit, or
    whose run is 2^64 or more, is counted in n_items and in no statistic; signs, fractions, hex and
    thousands separators are not interpreted.  stats has shape (4, n_bins + 1), the rows SUM_COUNT,
    SUM_SUM (modulo 2^64), SUM_MIN, SUM_MAX; a slot without numeric items reads 0, 0, 2^64 - 1, 0.
    Everything is exact and bit-identical from run to run.
    Host input -> (n_lines, n_items, n_numeric, stats): stats a uint64 array; into= takes such an
    array, MERGES into it (counts and sums added, min and max merged: a stream of buffers reduced
    into one table) and returns it.
    A CUDA uint8 tensor -> the same tuple as device tensors, the three counts as 1-element int64
    tensors and stats as int64 of shape (4, n_bins + 1) (into= such a CUDA tensor), asynchronously
    on the current stream and without any read-back.  The words are unsigned: an empty slot's min
    reads -1 there, and stats.cpu().numpy().view(numpy.uint64) gives the values as they are."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if which not in _SUM_WHICH:
        raise RedExceptApi('which must be "first" or "last"')
    w, per = _SUM_WHICH[which], int(max_per_line)
    n_bins = int(exe.info["max_result"]) + 1 if n_bins is None else int(n_bins)
    if n_bins < 0 or per < 0:
        raise RedExceptApi("n_bins and max_per_line must not be negative")
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        if into is None:
            stats = torch.empty((4, n_bins + 1), dtype=torch.int64, device=dev)
        else:
            if (not _is_torch(into) or not into.is_cuda or into.device != dev or
                    into.dtype != torch.int64 or not into.is_contiguous() or
                    tuple(into.shape) != (4, n_bins + 1)):
                raise RedExceptApi("into must be a contiguous int64 CUDA tensor of shape "
                                   "(4, n_bins + 1) on the input's device")
            stats = into
        cnt = torch.empty(3, dtype=torch.int64, device=dev)
        _check(l.redgpu_sum_text_dev(
            exe._h, w, ptr, size, d, per, n_bins, 0 if into is None else 1, cnt.data_ptr(),
            cnt.data_ptr() + 8, cnt.data_ptr() + 16, stats.data_ptr(), stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], stats
    a = _host_u8(data)
    dp = a.ctypes.data if a.size else None
    if into is None:
        stats = np.zeros((4, n_bins + 1), dtype=np.uint64)
    else:
        if (not isinstance(into, np.ndarray) or into.dtype != np.uint64 or
                into.shape != (4, n_bins + 1) or not into.flags.c_contiguous):
            raise RedExceptApi("into must be a contiguous uint64 array of shape (4, n_bins + 1)")
        stats = into
    nl, ni, nn = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(l.redgpu_sum_text(exe._h, w, dp, a.size, d, per, n_bins, 0 if into is None else 1,
                             C.byref(nl), C.byref(ni), C.byref(nn), stats.ctypes.data))
    return int(nl.value), int(ni.value), int(nn.value), stats


def uniq_text(exe, data, *, matches=True, style=styInstant, do_leader=True, max_per_line=1 << 62,
              delim=b"\n", max_distinct=1 << 20, cap=None):
    """redgpu_uniq_text[_dev]: grep -o | sort | uniq -c keyed by the matched BYTES - the distinct
    byte strings among a raw text's items and how often each occurs, in the order of first
    appearance.  matches=True: the items are extract_text's pieces (at most max_per_line of a
    line); matches=False: the lines grep_text selects with search<style,doLeader>, without their
    delimiters.  Record j is (first[j], length[j], count[j]): the string is
    data[first[j] : first[j] + length[j]], first[j] its earliest occurrence (strictly ascending),
    count[j] all its occurrences, exact.  The hash table has table_slots = the power of two at or
    above 2 * max_distinct (at least 64) slots of 16 bytes; n_dropped counts the items in no
    record - those of 2^24 bytes or more, and those that found the table full (then call again
    with a larger max_distinct).  While n_dropped is 0 every output is bit-identical from run to
    run.
    Host input -> (n_lines, n_items, n_dropped, first, length, count): uint64 arrays of
    min(n_distinct, cap) rows, cap=None meaning all of them.
    A CUDA uint8 tensor -> (n_lines, n_items, n_dropped, n_distinct, first, length, count): the
    counts as 1-element int64 tensors, the arrays int64 of cap rows (cap=None: max_distinct) of
    which the first min(n_distinct, cap) are written, asynchronously on the current stream and
    without any read-back."""
    l = _lib.lib()
    d = _delim_byte(delim)
    what = UNIQ_MATCHES if matches else UNIQ_LINES
    style, lead, per = int(style), 1 if do_leader else 0, int(max_per_line)
    max_distinct = int(max_distinct)
    if max_distinct < 1 or max_distinct > 1 << 31:
        raise RedExceptApi("max_distinct must be in [1, 2^31]")
    if per < 0 or (cap is not None and int(cap) < 0):
        raise RedExceptApi("max_per_line and cap must not be negative")
    slots = 64
    while slots < 2 * max_distinct:
        slots *= 2
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        rows = max_distinct if cap is None else int(cap)
        cnt = torch.empty(4, dtype=torch.int64, device=dev)
        rec = torch.empty((3, rows), dtype=torch.int64, device=dev)
        _check(l.redgpu_uniq_text_dev(
            exe._h, what, style, lead, ptr, size, d, per, slots, rows, cnt.data_ptr(),
            cnt.data_ptr() + 8, cnt.data_ptr() + 16, cnt.data_ptr() + 24,
            rec[0].data_ptr() if rows else None, rec[1].data_ptr() if rows else None,
            rec[2].data_ptr() if rows else None, stream))
        return cnt[0:1], cnt[1:2], cnt[3:4], cnt[2:3], rec[0], rec[1], rec[2]
    a = _host_u8(data)
    # no more records than slots, nor than bytes
    rows = min(slots, int(a.size)) if cap is None else min(int(cap), slots, int(a.size))
    rec = np.zeros((3, max(rows, 1)), dtype=np.uint64)
    nl, ni, nd, nx = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(l.redgpu_uniq_text(
        exe._h, what, style, lead, a.ctypes.data if a.size else None, a.size, d, per, slots, rows,
        C.byref(nl), C.byref(ni), C.byref(nd), C.byref(nx), rec[0].ctypes.data, rec[1].ctypes.data,
        rec[2].ctypes.data))
    n = min(int(nd.value), rows)
    return (int(nl.value), int(ni.value), int(nx.value), rec[0, :n].copy(), rec[1, :n].copy(),
            rec[2, :n].copy())


def replace_text(exe, data, repl, style=styLast, do_leader=True, max_count=1 << 62, *,
                 only_changed=False, delim=b"\n", out=None, out_cap=None):
    """redgpu_replace_text[_dev]: sed - every delimiter-terminated line of a raw text buffer
    rewritten by replace<style,doLeader>(line, repl, max_count) (include/Matcher.h:186-191, core
    :643-706, inside tools/skim_red.cpp:36-46's line loop) and the lines put back together as a
    text: each rewritten line, its delimiter, and behind the last line the tail, unchanged.
    max_count is per line: 1 is sed s/x/y/, the default s/x/y/g, 0 copies the text.
    only_changed=True is sed -n 's/x/y/p': only the lines with a replacement, no tail.
    Host input -> (n_lines, n_replaced, bytes).
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_replaced, out_len, out): the
    counts as 1-element int64 tensors, asynchronously on the current stream and without any
    read-back; out_len may exceed the room, bytes of out from min(out_len, room) on are untouched.
    repl is bytes or, for the device form, a uint8 CUDA tensor too."""
    l = _lib.lib()
    d = _delim_byte(delim)
    style, lead, oc = int(style), 1 if do_leader else 0, 1 if only_changed else 0
    max_count = int(max_count)
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("replace_text", data, out, out_cap)
        if _is_torch(repl):
            if (not repl.is_cuda or repl.dtype != torch.uint8 or not repl.is_contiguous() or
                    repl.device != dev):
                raise RedExceptApi("repl must be bytes or a contiguous uint8 CUDA tensor")
            drepl = repl
        else:
            r = np.frombuffer(bytes(repl), dtype=np.uint8)
            drepl = torch.from_numpy(r.copy()).to(dev)
        cnt = torch.empty(3, dtype=torch.int64, device=dev)
        _check(l.redgpu_replace_text_dev(
            exe._h, style, lead, oc, ptr, size, d, drepl.data_ptr() if drepl.numel() else None,
            drepl.numel(), max_count, cnt.data_ptr(), cnt.data_ptr() + 8, cnt.data_ptr() + 16,
            out.data_ptr() if room else None, room, stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    r = np.frombuffer(bytes(repl), dtype=np.uint8)
    nl, nr, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(buf, cap):
        _check(l.redgpu_replace_text(
            exe._h, style, lead, oc, a.ctypes.data if a.size else None, a.size, d,
            r.ctypes.data if r.size else None, r.size, max_count, C.byref(nl), C.byref(nr),
            C.byref(olen), buf, cap))
        return olen.value

    # first guess: output about as long as the input
    text = _host_text_out(a.size + 64, call)
    return int(nl.value), int(nr.value), text


def filter_text(exe, data, style=styInstant, do_leader=True, *, invert=False, before=0, after=0,
                max_count=1 << 62, delim=b"\n", out=None, out_cap=None):
    """redgpu_filter_text[_dev]: grep - the delimiter-terminated lines of a raw text buffer that
    search<style,doLeader> selects (grep_text's rule; invert=True is grep -v), the first max_count
    of them (grep -m), with `before` lines in front of and `after` lines behind each (grep -B /
    -A), put together as a text: every emitted line once, in text order, with its delimiter, no
    group separator.  The tail behind the last delimiter is not a line and is never emitted.
    Host input -> (n_lines, n_selected, n_emitted, bytes).
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_selected, n_emitted, out_len,
    out): the counts as 1-element int64 tensors, asynchronously on the current stream and without
    any read-back; out_len may exceed the room, bytes of out from min(out_len, room) on are
    untouched.  The output is a raw text that every text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    style, lead, inv = int(style), 1 if do_leader else 0, 1 if invert else 0
    before, after, max_count = int(before), int(after), int(max_count)
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("filter_text", data, out, out_cap)
        cnt = torch.empty(4, dtype=torch.int64, device=dev)
        _check(l.redgpu_filter_text_dev(
            exe._h, style, lead, inv, before, after, max_count, ptr, size, d, cnt.data_ptr(),
            cnt.data_ptr() + 8, cnt.data_ptr() + 16, cnt.data_ptr() + 24,
            out.data_ptr() if room else None, room, stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], cnt[3:4], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    nl, ns, ne, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(buf, cap):
        _check(l.redgpu_filter_text(
            exe._h, style, lead, inv, before, after, max_count, a.ctypes.data if a.size else None,
            a.size, d, C.byref(nl), C.byref(ns), C.byref(ne), C.byref(olen), buf, cap))
        return olen.value

    # the output is no longer than the text
    text = _host_text_out(a.size, call)
    return int(nl.value), int(ns.value), int(ne.value), text


def route_text(exe, data, n_bins=None, style=styInstant, do_leader=True, *, drop_unmatched=False,
               delim=b"\n", out=None, out_cap=None):
    """redgpu_route_text[_dev]: awk '{ print > file[class] }' - every delimiter-terminated line of
    a raw text buffer routed to the bucket of the result search<style,doLeader> reports for it
    (tally_text's matches=False value and slot rule: bucket r for a result r < n_bins, bucket
    n_bins for everything else), and the text put back together bucket by bucket: bucket 0's
    lines, then bucket 1's, ..., inside a bucket in text order, each with its delimiter - a stable
    partition.  n_bins=None means min(exe.info["max_result"] + 1, 255); more than 255 is refused.
    drop_unmatched=True leaves the lines that do not match out of the output (they are still
    counted in bin_lines[0]).  bin_lines has n_bins + 1 entries (tally_text's bins), bin_offsets
    n_bins + 2: where each bucket's section begins in the output, and its length.  The tail
    behind the last delimiter is not a line and is never emitted.
    Host input -> (n_lines, n_routed, bin_lines, bin_offsets, bytes): the two as uint64 arrays.
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_routed, bin_lines, bin_offsets,
    out_len, out): the counts as int64 tensors, asynchronously on the current stream and without
    any read-back; out_len may exceed the room, bytes of out from min(out_len, room) on are
    untouched.  Every section of the output is a raw text that every text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    style, lead, drop = int(style), 1 if do_leader else 0, 1 if drop_unmatched else 0
    n_bins = min(int(exe.info["max_result"]) + 1, 255) if n_bins is None else int(n_bins)
    if n_bins < 0:
        raise RedExceptApi("n_bins must not be negative")
    if n_bins > 255:
        raise RedExceptLimit("n_bins must not exceed 255")
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("route_text", data, out, out_cap)
        # n_lines, n_routed, out_len, bin_lines[n_bins + 1], bin_offsets[n_bins + 2]
        cnt = torch.empty(3 + 2 * n_bins + 3, dtype=torch.int64, device=dev)
        lines_at, offs_at = 3, 3 + n_bins + 1
        _check(l.redgpu_route_text_dev(
            exe._h, style, lead, drop, ptr, size, d, n_bins, cnt.data_ptr(), cnt.data_ptr() + 8,
            cnt.data_ptr() + 8 * lines_at, cnt.data_ptr() + 8 * offs_at, cnt.data_ptr() + 16,
            out.data_ptr() if room else None, room, stream))
        return cnt[0:1], cnt[1:2], cnt[lines_at:offs_at], cnt[offs_at:], cnt[2:3], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    nl, nr, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    bin_lines = np.zeros(n_bins + 1, dtype=np.uint64)
    bin_offsets = np.zeros(n_bins + 2, dtype=np.uint64)

    def call(buf, cap):
        _check(l.redgpu_route_text(
            exe._h, style, lead, drop, a.ctypes.data if a.size else None, a.size, d, n_bins,
            C.byref(nl), C.byref(nr), bin_lines.ctypes.data, bin_offsets.ctypes.data,
            C.byref(olen), buf, cap))
        return olen.value

    # the output is no longer than the text
    text = _host_text_out(a.size, call)
    return int(nl.value), int(nr.value), bin_lines, bin_offsets, text


def range_text(exe, data, open_result, close_result=None, style=styInstant, do_leader=True, *,
               emit_open=True, emit_close=True, invert=False, max_ranges=1 << 62, delim=b"\n",
               out=None, out_cap=None, rec_cap=0):
    """redgpu_range_text[_dev]: sed -n '/open/,/close/p' - the delimiter-terminated lines of a raw
    text buffer read in text order with a state that is outside or inside: outside, a line whose
    search<style,doLeader> result is open_result begins a range (its open line); inside, the next
    line whose result is close_result ends it (its close line), every other line is a body line; a
    range still open at the last line ends there.  close_result=None means open_result: the
    toggle form, sed -n '/```/,/```/p'.  Only ranges numbered below max_ranges count.  Emitted are
    a counted range's body lines, its open line under emit_open and its close line under
    emit_close - under invert=True exactly the other lines (sed '/A/,/B/d') - in text order, each
    with its delimiter.  The records do not depend on emit_open, emit_close or invert: for every
    counted range r < rec_cap its first and last line numbers and data[begin[r]:end[r]], its bytes.
    The tail behind the last delimiter is not a line and is never emitted.
    Host input -> (n_lines, n_ranges, n_emitted, bytes, first_line, last_line, begin, end): the
    records as uint64 arrays of min(n_ranges, rec_cap) entries.
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_ranges, n_emitted, out_len, out,
    first_line, last_line, begin, end): the counts as 1-element int64 tensors, the records as
    int64 tensors of rec_cap entries of which the first min(n_ranges, rec_cap) are written,
    asynchronously on the current stream and without any read-back; out_len may exceed the room,
    bytes of out from min(out_len, room) on are untouched.  The output is a raw text that every
    text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    style, lead, inv = int(style), 1 if do_leader else 0, 1 if invert else 0
    eo, ec = 1 if emit_open else 0, 1 if emit_close else 0
    open_result = int(open_result)
    close_result = open_result if close_result is None else int(close_result)
    max_ranges, rec_cap = int(max_ranges), int(rec_cap)
    if open_result < 1 or close_result < 1:
        raise RedExceptApi("open_result and close_result must be at least 1")
    if open_result >= 1 << 31 or close_result >= 1 << 31:
        raise RedExceptApi("open_result and close_result must fit 31 bits")
    if max_ranges < 0 or rec_cap < 0:
        raise RedExceptApi("max_ranges and rec_cap must not be negative")
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("range_text", data, out, out_cap)
        cnt = torch.empty(4, dtype=torch.int64, device=dev)
        rec = torch.empty((4, rec_cap), dtype=torch.int64, device=dev)
        at = [rec[k].data_ptr() if rec_cap else None for k in range(4)]
        _check(l.redgpu_range_text_dev(
            exe._h, style, lead, open_result, close_result, eo, ec, inv, max_ranges, ptr, size, d,
            cnt.data_ptr(), cnt.data_ptr() + 8, cnt.data_ptr() + 16, cnt.data_ptr() + 24,
            out.data_ptr() if room else None, room, rec_cap, at[0], at[1], at[2], at[3], stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], cnt[3:4], out, rec[0], rec[1], rec[2], rec[3]
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    nl, nr, ne, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    # there are no more ranges than bytes
    rec_cap = min(rec_cap, int(a.size))
    rec = np.zeros((4, max(rec_cap, 1)), dtype=np.uint64)

    def call(buf, cap):
        _check(l.redgpu_range_text(
            exe._h, style, lead, open_result, close_result, eo, ec, inv, max_ranges,
            a.ctypes.data if a.size else None, a.size, d, C.byref(nl), C.byref(nr), C.byref(ne),
            C.byref(olen), buf, cap, rec_cap, rec[0].ctypes.data, rec[1].ctypes.data,
            rec[2].ctypes.data, rec[3].ctypes.data))
        return olen.value

    # the output is no longer than the text
    text = _host_text_out(a.size, call)
    got = min(int(nr.value), rec_cap)
    return (int(nl.value), int(nr.value), int(ne.value), text,
            rec[0, :got].copy(), rec[1, :got].copy(), rec[2, :got].copy(), rec[3, :got].copy())


DEDUP_WHOLE, DEDUP_LINES, DEDUP_MATCH, DEDUP_FIELD = 0, 1, 2, 3
_DEDUP_WHAT = {"whole": DEDUP_WHOLE, "lines": DEDUP_LINES, "match": DEDUP_MATCH,
               "field": DEDUP_FIELD}


def dedup_text(exe, data, *, what="whole", key_index=1, style=styInstant, do_leader=True,
               min_count=1, max_count=None, invert=False, keep_unkeyed=False, delim=b"\n",
               max_distinct=1 << 20, out=None, out_cap=None):
    """redgpu_dedup_text[_dev]: awk '!seen[$k]++' - the delimiter-terminated lines of a raw text
    buffer chosen by the CONTENT of their keys.  Every line has at most one key: the line itself
    (what="whole", the DFA is not walked), the line if search<style,doLeader> selects it ("lines",
    uniq_text's matches=False item), the key_index-th piece extract_text emits for it ("match"),
    or its key_index-th field with the DFA as the separator ("field", fields_text's rule; a field
    may be empty); a line without one is unkeyed.  A keyed line is marked iff it holds the earliest
    occurrence of its key's string and min_count <= count <= max_count (None: no upper bound),
    count being all the string's occurrences.  Emitted are the keyed lines with marked != invert
    and, under keep_unkeyed, the unkeyed ones, in text order, each with its delimiter: the defaults
    are awk '!seen[k]++', (1, 1) is uniq -u and (2, None) uniq -d in text order, invert=True is
    awk 'seen[k]++'.  The hash table has the power of two at or above 2 * max_distinct (at least
    64) slots of 16 bytes; n_dropped counts the keyed lines whose key got no record - keys of 2^24
    bytes or more, and those that found the table full (then call again with a larger
    max_distinct); they are not marked.  While n_dropped is 0 the output is bit-identical from run
    to run.  The tail behind the last delimiter is not a line: never emitted, and no key.
    Host input -> (n_lines, n_keyed, n_distinct, n_dropped, n_emitted, bytes).
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_keyed, n_distinct, n_dropped,
    n_emitted, out_len, out): the counts as 1-element int64 tensors, asynchronously on the current
    stream and without any read-back; out_len may exceed the room, bytes of out from
    min(out_len, room) on are untouched.  The output is a raw text that every text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if what not in _DEDUP_WHAT:
        raise RedExceptApi('what must be "whole", "lines", "match" or "field"')
    w = _DEDUP_WHAT[what]
    style, lead = int(style), 1 if do_leader else 0
    inv, keep = 1 if invert else 0, 1 if keep_unkeyed else 0
    key_index, min_count = int(key_index), int(min_count)
    max_count = (1 << 64) - 1 if max_count is None else int(max_count)
    max_distinct = int(max_distinct)
    if w in (DEDUP_MATCH, DEDUP_FIELD) and key_index < 1:
        raise RedExceptApi("key_index must be at least 1")
    if key_index < 0 or key_index >= 1 << 64:
        raise RedExceptApi("key_index must fit 64 bits")
    if not (0 <= min_count < 1 << 64 and 0 <= max_count < 1 << 64):
        raise RedExceptApi("min_count and max_count must be in [0, 2^64)")
    if max_distinct < 1 or max_distinct > 1 << 31:
        raise RedExceptApi("max_distinct must be in [1, 2^31]")
    slots = 64
    while slots < 2 * max_distinct:
        slots *= 2
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("dedup_text", data, out, out_cap)
        cnt = torch.empty(6, dtype=torch.int64, device=dev)
        at = [cnt.data_ptr() + 8 * k for k in range(6)]
        _check(l.redgpu_dedup_text_dev(
            exe._h, w, style, lead, key_index, min_count, max_count, inv, keep, ptr, size, d, slots,
            at[0], at[1], at[2], at[3], at[4], at[5], out.data_ptr() if room else None, room,
            stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], cnt[3:4], cnt[4:5], cnt[5:6], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    n = [C.c_uint64(0) for _ in range(6)]

    def call(buf, cap):
        _check(l.redgpu_dedup_text(
            exe._h, w, style, lead, key_index, min_count, max_count, inv, keep,
            a.ctypes.data if a.size else None, a.size, d, slots, C.byref(n[0]), C.byref(n[1]),
            C.byref(n[2]), C.byref(n[3]), C.byref(n[4]), C.byref(n[5]), buf, cap))
        return n[5].value

    # the output is no longer than the text
    text = _host_text_out(a.size, call)
    return tuple(int(x.value) for x in n[:5]) + (text,)


GROUP_MATCH, GROUP_FIELD = 0, 1
_GROUP_WHAT = {"match": GROUP_MATCH, "field": GROUP_FIELD}


def group_text(exe, data, *, what="field", key_index=1, value_index=2, which="first",
               delim=b"\n", max_distinct=1 << 20, cap=None):
    """redgpu_group_text[_dev]: awk '{ n[$k]++; s[$k] += $v; if ($v > m[$k]) m[$k] = $v }' - one
    record per distinct KEY string of a raw text's delimiter-terminated lines, with the statistics
    of the lines' numbers.  The items of a line are the pieces extract_text emits for it
    (what="match") or its fields with the DFA as the separator ("field", fields_text's rule; a
    field may be empty), numbered from 1: item key_index is the key - a line with fewer items is
    unkeyed and contributes nothing - and item value_index (0: none; below, at or above key_index)
    the value, whose number is sum_text's: the first (which="first") or last ("last") run of digits
    0-9 inside the item, read as an unsigned decimal.  A keyed line is numeric iff its value item
    exists, has a run, and the run is below 2^64.  Record j, in the order of first appearance, is
    (first[j], length[j], count[j], stats[:, j]): the key is data[first[j] : first[j] + length[j]]
    (first strictly ascending), count[j] its keyed lines, stats' rows SUM_COUNT (its numeric lines),
    SUM_SUM (modulo 2^64), SUM_MIN, SUM_MAX; a key without numeric lines reads 0, 0, 2^64 - 1, 0.
    The hash table has the power of two at or above 2 * max_distinct (at least 64) slots of 48
    bytes; n_dropped counts the keyed lines in no record - keys of 2^24 bytes or more, and those
    that found the table full (then call again with a larger max_distinct) - which enter no record
    with either their count or their number; n_numeric counts the numeric lines in the records.
    While n_dropped is 0 every output is bit-identical from run to run.
    Host input -> (n_lines, n_keyed, n_numeric, n_dropped, first, length, count, stats): uint64
    arrays of min(n_distinct, cap) records (stats of shape (4, that)), cap=None meaning all.
    A CUDA uint8 tensor -> (n_lines, n_keyed, n_numeric, n_dropped, n_distinct, first, length,
    count, stats): the counts as 1-element int64 tensors, the arrays int64 of cap records (cap=None:
    max_distinct; stats of shape (4, cap)) of which the first min(n_distinct, cap) are written,
    asynchronously on the current stream and without any read-back.  The words are unsigned:
    stats.cpu().numpy().view(numpy.uint64) gives the values as they are."""
    l = _lib.lib()
    d = _delim_byte(delim)
    if what not in _GROUP_WHAT:
        raise RedExceptApi('what must be "match" or "field"')
    if which not in _SUM_WHICH:
        raise RedExceptApi('which must be "first" or "last"')
    w, wh = _GROUP_WHAT[what], _SUM_WHICH[which]
    key_index, value_index, max_distinct = int(key_index), int(value_index), int(max_distinct)
    if key_index < 1 or key_index >= 1 << 64:
        raise RedExceptApi("key_index must be in [1, 2^64)")
    if value_index < 0 or value_index >= 1 << 64:
        raise RedExceptApi("value_index must be in [0, 2^64)")
    if max_distinct < 1 or max_distinct > 1 << 31:
        raise RedExceptApi("max_distinct must be in [1, 2^31]")
    if cap is not None and int(cap) < 0:
        raise RedExceptApi("cap must not be negative")
    slots = 64
    while slots < 2 * max_distinct:
        slots *= 2
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        rows = max_distinct if cap is None else int(cap)
        cnt = torch.empty(5, dtype=torch.int64, device=dev)
        rec = torch.empty((3, rows), dtype=torch.int64, device=dev)
        stats = torch.empty((4, rows), dtype=torch.int64, device=dev)
        at = [cnt.data_ptr() + 8 * k for k in range(5)]
        _check(l.redgpu_group_text_dev(
            exe._h, w, key_index, value_index, wh, ptr, size, d, slots, rows, at[0], at[1], at[2],
            at[3], at[4], rec[0].data_ptr() if rows else None, rec[1].data_ptr() if rows else None,
            rec[2].data_ptr() if rows else None, stats.data_ptr() if rows else None, stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], cnt[4:5], cnt[3:4], rec[0], rec[1], rec[2], stats
    a = _host_u8(data)
    # no more records than slots, nor than bytes
    rows = min(slots, int(a.size)) if cap is None else min(int(cap), slots, int(a.size))
    wide = max(rows, 1)
    rec = np.zeros((3, wide), dtype=np.uint64)
    stats = np.zeros((4, wide), dtype=np.uint64)
    n = [C.c_uint64(0) for _ in range(5)]
    _check(l.redgpu_group_text(
        exe._h, w, key_index, value_index, wh, a.ctypes.data if a.size else None, a.size, d, slots,
        wide if rows else 0, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), C.byref(n[3]),
        C.byref(n[4]), rec[0].ctypes.data, rec[1].ctypes.data, rec[2].ctypes.data,
        stats.ctypes.data))
    got = min(int(n[3].value), rows)
    return (int(n[0].value), int(n[1].value), int(n[2].value), int(n[4].value),
            rec[0, :got].copy(), rec[1, :got].copy(), rec[2, :got].copy(), stats[:, :got].copy())


def extract_text(exe, data, *, max_per_line=1 << 62, delim=b"\n", out=None, out_cap=None):
    """redgpu_extract_text[_dev]: grep -o as a text - every match of every delimiter-terminated
    line of a raw text buffer (Red::collect's chain, collect_text's records), as bytes: the span
    replace<styLast,false> would substitute, from where the matching attempt began (at or before
    the record's start) to the record's end, each followed by the delimiter, in text order.  Only
    the first max_per_line matches of a line are emitted (1 = the first of every line, 0 = none).
    Host input -> (n_lines, n_matches, bytes).
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_matches, out_len, out): the
    counts as 1-element int64 tensors, asynchronously on the current stream and without any
    read-back; out_len may exceed the room, bytes of out from min(out_len, room) on are
    untouched.  The output is a raw text that every text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    max_per_line = int(max_per_line)
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("extract_text", data, out, out_cap)
        cnt = torch.empty(3, dtype=torch.int64, device=dev)
        _check(l.redgpu_extract_text_dev(
            exe._h, ptr, size, d, max_per_line, cnt.data_ptr(), cnt.data_ptr() + 8,
            cnt.data_ptr() + 16, out.data_ptr() if room else None, room, stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    nl, nm, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(buf, cap):
        _check(l.redgpu_extract_text(
            exe._h, a.ctypes.data if a.size else None, a.size, d, max_per_line, C.byref(nl),
            C.byref(nm), C.byref(olen), buf, cap))
        return olen.value

    # first guess: output about as long as the input (it can reach twice that: one-byte pieces
    # and their delimiters)
    text = _host_text_out(a.size + 64, call)
    return int(nl.value), int(nm.value), text


def fields_mask(fields) -> int:
    """The 64-bit select mask of redgpu_fields_text: bit k - 1 stands for field k (1..63), bit 63
    for field 64 and every later one.  fields is a cut-style list - "1,3,5-": single 1-based
    indices and open ranges "k-", comma-separated - or an iterable of 1-based ints.  A closed range
    ("2-7") or an index above 63 is refused: bit 63 cannot stand for field 64 alone."""
    if isinstance(fields, (bytes, bytearray)):
        fields = bytes(fields).decode("ascii", "replace")
    mask = 0
    if isinstance(fields, str):
        for part in fields.split(","):
            part = part.strip()
            open_range = part.endswith("-")
            digits = part[:-1] if open_range else part
            if not digits.isdigit() or not digits.isascii():
                raise RedExceptApi("fields: %r is neither an index k nor an open range k-" % part)
            k = int(digits)
            if k < 1 or (k > 64 if open_range else k > 63):
                raise RedExceptApi("fields: %r is outside 1..63 (open ranges: 1..64)" % part)
            mask |= ((1 << 64) - 1) & ~((1 << (k - 1)) - 1) if open_range else 1 << (k - 1)
    else:
        for k in fields:
            if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 63:
                raise RedExceptApi("fields: %r is no index in 1..63" % (k,))
            mask |= 1 << (int(k) - 1)
    if mask == 0:
        raise RedExceptApi("fields selects nothing")
    return mask


def fields_text(exe, data, fields, *, sep=b" ", max_fields=0, only_delimited=False, delim=b"\n",
                out=None, out_cap=None):
    """redgpu_fields_text[_dev]: awk -F / cut - exe's DFA describes the SEPARATOR; of every
    delimiter-terminated line of a raw text buffer the selected fields that exist, in ascending
    order, joined by sep (0..8 bytes), then the delimiter.  The separators of a line are the pieces
    extract_text emits for it, only the first max_fields - 1 of them when max_fields > 0 (the last
    field is then the rest of the line); fields may be empty (re.split's, not awk's whitespace
    mode).  fields: fields_mask's argument.  only_delimited (cut -s): lines without a separator
    are not emitted; otherwise output line k corresponds to input line k.
    Host input -> (n_lines, n_emitted, n_fields, bytes).
    A CUDA uint8 tensor needs out (a contiguous uint8 CUDA tensor to write into) or out_cap (one
    of that size is made; 0 gives the sizes only) -> (n_lines, n_emitted, n_fields, out_len, out):
    the counts as 1-element int64 tensors, asynchronously on the current stream and without any
    read-back; out_len may exceed the room, bytes of out from min(out_len, room) on are
    untouched.  The output is a raw text that every text verb accepts."""
    l = _lib.lib()
    d = _delim_byte(delim)
    select = fields_mask(fields)
    sep = bytes(sep)
    if len(sep) > 8:
        raise RedExceptApi("sep is longer than 8 bytes")
    sep_word = int.from_bytes(sep, "little")
    max_fields = int(max_fields)
    only = 1 if only_delimited else 0
    if _is_torch(data):
        import torch
        dev, ptr, size, stream = _device_raw_text(data)
        out, room = _device_out_room("fields_text", data, out, out_cap)
        cnt = torch.empty(4, dtype=torch.int64, device=dev)
        _check(l.redgpu_fields_text_dev(
            exe._h, ptr, size, d, select, max_fields, only, sep_word, len(sep), cnt.data_ptr(),
            cnt.data_ptr() + 8, cnt.data_ptr() + 16, cnt.data_ptr() + 24,
            out.data_ptr() if room else None, room, stream))
        return cnt[0:1], cnt[1:2], cnt[2:3], cnt[3:4], out
    _host_text_only(out, out_cap)
    a = _host_u8(data)
    nl, ne, nf, olen = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(buf, cap):
        _check(l.redgpu_fields_text(
            exe._h, a.ctypes.data if a.size else None, a.size, d, select, max_fields, only,
            sep_word, len(sep), C.byref(nl), C.byref(ne), C.byref(nf), C.byref(olen), buf, cap))
        return olen.value

    # first guess: output about as long as the input (a long sep between short fields makes it
    # longer)
    text = _host_text_out(a.size + 64, call)
    return int(nl.value), int(ne.value), int(nf.value), text


class StatefulMatcher:
    """Mirror of zezax::red::StatefulMatcher (include/Matcher.h:770-792): `advance(byte)` and
    `result()`; `advance_bytes` feeds a whole chunk in one kernel launch.  The executable must
    outlive the matcher, as in the reference."""

    def __init__(self, exe):
        self._exe = exe
        self._state = np.full(1, STATE_INITIAL, dtype=np.uint32)
        self._result = int(advance_batch(exe, b"", self._state, offsets=[0, 0])[0])

    def advance(self, byte) -> int:
        b = bytes([byte]) if isinstance(byte, int) else bytes(byte[:1])
        return self.advance_bytes(b)

    def advance_bytes(self, chunk: bytes) -> int:
        self._result = int(advance_batch(self._exe, chunk, self._state,
                                         offsets=[0, len(chunk)])[0])
        return self._result

    def result(self) -> int:
        return self._result


# single-input forms keep the reference's signatures; they are batches of one ON THE GPU
def check(exe, text: bytes, style, do_leader=True) -> int:
    return int(check_batch(exe, text, style, do_leader, offsets=[0, len(text)])[0])


def scan(exe, text: bytes, style, do_leader=True) -> int:
    return int(scan_batch(exe, text, style, do_leader, offsets=[0, len(text)])[0])


def match(exe, text: bytes, style, do_leader=True):
    r, s, e = match_batch(exe, text, style, do_leader, offsets=[0, len(text)])
    return int(r[0]), int(s[0]), int(e[0])


def search(exe, text: bytes, style, do_leader=True):
    r, s, e = search_batch(exe, text, style, do_leader, offsets=[0, len(text)])
    return int(r[0]), int(s[0]), int(e[0])


# the host-buffer staging: caller-pinned memory and the diagnostics of include/redgpu.h ----------

def _span(buf, nbytes):
    """(address, bytes) of a numpy array, or of a plain address with nbytes"""
    if isinstance(buf, np.ndarray):
        if not buf.flags.c_contiguous:
            raise RedExceptApi("a buffer to pin must be contiguous")
        return buf.ctypes.data, buf.nbytes if nbytes is None else int(nbytes)
    return buf, 0 if nbytes is None else int(nbytes)


def host_register(buf, nbytes=None) -> int:
    """redgpu_host_register: pin caller memory (a contiguous numpy array, or an address with
    nbytes) so that the host-buffer forms copy it as it is.  Returns the C-ABI's code, REDGPU_OK
    or an error (nothing is raised: the refusals are part of the interface)."""
    p, n = _span(buf, nbytes)
    return int(_lib.lib().redgpu_host_register(p, n))


def host_unregister(buf) -> int:
    """redgpu_host_unregister of what host_register pinned; returns the C-ABI's code."""
    p, _ = _span(buf, None)
    return int(_lib.lib().redgpu_host_unregister(p))


class pinned_host:
    """with pinned_host(array): the array's bytes are registered inside the block"""

    def __init__(self, buf):
        self.buf = buf

    def __enter__(self):
        _check(host_register(self.buf))
        return self.buf

    def __exit__(self, *exc):
        _check(host_unregister(self.buf))
        return False


def host_route_counts():
    """redgpu_host_route_counts: transfers of caller memory so far, process-wide, by route -
    (caller-pinned, through a pinned arena, registered for the call, handed over pageable)"""
    c = (C.c_uint64 * 4)()
    _lib.lib().redgpu_host_route_counts(c)
    return tuple(int(v) for v in c)


def host_pins_held() -> int:
    """redgpu_host_pins_held: the calling thread's registrations not yet released plus its
    downloads not yet flushed - 0 whenever a host-buffer form has returned"""
    return int(_lib.lib().redgpu_host_pins_held())


def thread_release() -> None:
    """redgpu_thread_release: free the calling thread's staging (streams, buffers, arena)"""
    _lib.lib().redgpu_thread_release()
