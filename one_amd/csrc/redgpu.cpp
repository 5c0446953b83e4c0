// redgpu.cpp - the C-ABI of include/redgpu.h over the gfx950 kernels.  Host C++ (built with
// hipcc for the HIP runtime API).  There is no CPU compute path in this file or behind it:
// every batch entry point either launches a kernel or fails.
#include "../../include/redgpu.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include "dfa_image.h"
#include "host_stage.h"
#include "kernels.h"
#include "redgpu_internal.h"

using namespace redgpu;

namespace {

// a handle that can compute: refused before any HIP call when it has no device image
int checkHandle(const redgpu_dfa *dfa) {
  if (!dfa) return fail(REDGPU_EAPI, "null dfa handle");
  if (dfa->im->device < 0) return fail(REDGPU_EAPI, "dfa handle has no device image");
  return REDGPU_OK;
}

int checkStyle(int style) {
  if (style < REDGPU_STY_INSTANT || style > REDGPU_STY_FULL)
    return fail(REDGPU_EEXEC, "unsupported style");  // lib/Matcher.cpp:45
  return REDGPU_OK;
}

LaunchCfg cfgOfFlags(const redgpu_dfa *dfa, uint32_t extraFlags) {
  return LaunchCfg{dfa->numCUs, ((dfa->flags | extraFlags) & REDGPU_F_FORCE_GENERIC) ? 1 : 0,
                   (dfa->flags & REDGPU_F_NO_BUCKETING) ? 1 : 0,
                   (dfa->flags & REDGPU_F_FORCE_STREAM) ? 1 : 0,
                   (dfa->flags & REDGPU_F_NO_CHUNKING) ? 1 : 0,
                   (dfa->flags & REDGPU_F_FORCE_CHUNKING) ? 1 : 0,
                   (dfa->flags & REDGPU_F_FORCE_EARLY) ? 1 : 0,
                   (dfa->flags & REDGPU_F_FORCE_LEAN) ? 1 : 0,
                   (dfa->flags & REDGPU_F_LEAN_CHAINS_4) ? 1 : 0,
                   (dfa->flags & REDGPU_F_STREAM_CHAINS_2) ? 2
                   : (dfa->flags & REDGPU_F_STREAM_CHAINS_4) ? 4 : 0};
}

LaunchCfg cfgOf(const redgpu_dfa *dfa, uint32_t extraFlags = 0) {
  LaunchCfg cfg = cfgOfFlags(dfa, extraFlags);
  cfg.forcePieces = (dfa->flags & REDGPU_F_FORCE_PIECES) ? 1 : 0;
  return cfg;
}

// the rules checkBatch applies where the entry point asks for them
enum BatchRule : unsigned {
  kStrideLimit = 1,    // without offsets, lines of 2^40 bytes and more are refused
  kTrailingLimit = 2,  // with offsets, at most 16 trailing bytes are dropped per line
};

// What a batch (data, offsets, stride, n > 0) must be; with offsets, stride is the number of
// trailing bytes to drop per line.  The offsets of a device batch (total == nullptr) cannot be
// read, so it has bytes when it has offsets or a stride.  A host batch reports *total, its
// bytes, and *maxLen, its longest line; its offsets must be monotone (a decreasing pair would
// underflow a line length on the device and send the walk far outside the buffer), and with
// `cap` records per line (the list verbs) n * cap must stay countable.  A host form leaves the
// trailing-bytes limit to the _dev form it stages into.  The checks fire in the order written.
int checkBatch(const uint8_t *data, const uint64_t *offsets, uint64_t stride, uint64_t n,
               unsigned rules, uint64_t *total = nullptr, uint64_t *maxLen = nullptr,
               uint64_t cap = 0) {
  if (!total && !data && (offsets || stride)) return fail(REDGPU_EAPI, "null data buffer");
  if ((rules & kStrideLimit) && !offsets && stride >= (1ull << 40))
    return fail(REDGPU_ELIMIT, "stride too large");
  if (total) {
    uint64_t m = 0;
    for (uint64_t i = 0; offsets && i < n; ++i) {
      if (offsets[i] > offsets[i + 1]) return fail(REDGPU_EAPI, "offsets not monotonic");
      const uint64_t l = offsets[i + 1] - offsets[i];
      m = l > m ? l : m;
    }
    if (maxLen) *maxLen = m;
    if (cap && n > (~0ull / 16) / cap) return fail(REDGPU_ELIMIT, "n * cap too large");
    *total = offsets ? offsets[n] : stride * n;
    if (*total && !data) return fail(REDGPU_EAPI, "null data buffer");
  }
  if ((rules & kTrailingLimit) && offsets && stride > 16)
    return fail(REDGPU_EAPI, "with offsets, stride is the number of trailing bytes to drop per "
                             "line (0..16)");
  return REDGPU_OK;
}

int runDev(const redgpu_dfa *dfa, int verb, int style, int doLeader, const uint8_t *data,
           const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
           uint64_t *start, uint64_t *end, hipStream_t stream, uint32_t extraFlags = 0) {
  if (int rc = checkHandle(dfa)) return rc;
  if (int rc = checkStyle(style)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!result) return fail(REDGPU_EAPI, "null result buffer");
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit | kTrailingLimit)) return rc;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  Batch b{data, offsets, stride, n, result, start, end};
  const LaunchCfg cfg = cfgOf(dfa, extraFlags);
  const char *name = "";
  hipError_t e = launchBatch(dfa->im->dev, b, verb, style, doLeader ? 1 : 0, cfg, stream, &name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// K batches, in order, on one stream (redgpu_*_batches_dev): each validated as runDev validates
// its one batch, then handed to launchBatches, which folds runs of streaming-kernel batches
// into single launches.
int runDevMany(const redgpu_dfa *dfa, int verb, int style, int doLeader, const redgpu_batch *bs,
               uint32_t nb, hipStream_t stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (int rc = checkStyle(style)) return rc;
  if (nb == 0) return REDGPU_OK;
  if (!bs) return fail(REDGPU_EAPI, "null batch descriptors");
  std::vector<Batch> v;
  v.reserve(nb);
  for (uint32_t k = 0; k < nb; ++k) {
    const redgpu_batch &b = bs[k];
    if (b.n == 0) continue;
    if (!b.result) return fail(REDGPU_EAPI, "null result buffer");
    if (int rc = checkBatch(b.data, b.offsets, b.stride, b.n, kStrideLimit | kTrailingLimit))
      return rc;
    const bool pos = verb == kMatch || verb == kSearch;
    v.push_back(Batch{b.data, b.offsets, b.stride, b.n, b.result, pos ? b.start : nullptr,
                      pos ? b.end : nullptr});
  }
  if (v.empty()) return REDGPU_OK;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  const LaunchCfg cfg = cfgOf(dfa);
  const char *name = "";
  hipError_t e = launchBatches(dfa->im->dev, v.data(), uint32_t(v.size()), verb, style,
                               doLeader ? 1 : 0, cfg, stream, &name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// device buffer slots of a HostStage
enum StageSlot : int {
  kSlData = 0,   // +parity
  kSlRes = 2,    // +parity
  kSlStart = 4,  // +parity
  kSlEnd = 6,    // +parity
  kSlOff = 8,
  kSlAux0 = 9,   // counts / state / replacement ...
  kSlAux1 = 10,
  kSlAux2 = 11,
  kSlAux3 = 12,
};

// One call of a host-buffer form: the device scope, the calling thread's HostStage and its
// beginCall(inputBytes), device buffers from the stage's slots, and the copies between them and
// the caller's memory.  The first step that fails drains both streams - no download may land in
// caller memory after the call has returned - and sets rc(); every later step does nothing.
// Every buffer of a call is taken before its first copy: growing a slot waits for the streams.
class HostCall {
 public:
  HostCall(const redgpu_dfa *dfa, uint64_t inputBytes) : scope_(dfa->im->device) {
    if (scope_.err != hipSuccess) {
      rc_ = failHip(scope_.err, "hipSetDevice");
      return;
    }
    const hipError_t e = hostStage(dfa->im->device, &st_);
    if (e != hipSuccess) {
      rc_ = failHip(e, "host staging (streams)");
      return;
    }
    st_->beginCall(inputBytes);
  }
  bool ok() const { return rc_ == REDGPU_OK; }
  int rc() const { return rc_; }
  HostStage &stage() const { return *st_; }
  hipStream_t stream() const { return st_->streams[0]; }

  template <class T> T *buf(int slot, uint64_t count, const char *what) {
    void *p = nullptr;
    if (ok()) check(st_->get(slot, count * sizeof(T), &p), "hipMalloc ", what);
    return static_cast<T *>(p);
  }
  // caller memory to and from the device on streams[idx]; `direct`: the caller pinned it
  template <class T>
  void upload(T *dev, const T *host, uint64_t count, const char *what, int idx = 0,
              bool direct = false) {
    if (ok()) check(st_->copyIn(dev, host, count * sizeof(T), idx, direct), "copy ", what);
  }
  template <class T>
  void download(T *host, const T *dev, uint64_t count, const char *what, int idx = 0,
                bool direct = false) {
    if (ok()) check(st_->copyOut(host, dev, count * sizeof(T), idx, direct), "copy ", what);
  }
  // the form's _dev call, which returns an error code of its own
  template <class F> void run(F &&devCall) {
    if (ok() && (rc_ = devCall()) != REDGPU_OK) (void)st_->sync();
  }
  // streams[idx] (-1: both) drained, the downloads behind it in the caller's memory; rc()
  int wait(int idx = 0) {
    if (ok()) check(idx < 0 ? st_->sync() : st_->syncStream(idx), "hipStreamSynchronize");
    return rc_;
  }
  // (only while ok())
  void check(hipError_t e, const char *what, const char *noun = "") {
    if (e == hipSuccess) return;
    (void)st_->sync();
    rc_ = failHip(e, (std::string(what) + noun).c_str());
  }

 private:
  DeviceScope scope_;
  HostStage *st_ = nullptr;
  int rc_ = REDGPU_OK;
};

// The _dev form of a raw-text verb behind its argument check: the device, ONE allocation of
// scratchBytes for the call - carved up by the verb's launcher, which launch(scratch, cfg, &name)
// calls - everything on `s`, nothing read back
template <class F>
int rawTextDev(const redgpu_dfa *dfa, hipStream_t s, uint64_t scratchBytes, F &&launch) {
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  void *scratch = nullptr;
  HIP_TRY(scratchFor(s, size_t(scratchBytes), &scratch), "hipMalloc scratch");
  const LaunchCfg cfg = cfgOf(dfa);
  const char *name = "";
  const hipError_t e = launch(scratch, cfg, &name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// The arguments of both forms of a long-text verb (collect_long, match_all_long, replace_long,
// search_long): what can be refused without a device first, in this order - no handle, a bad style
// (style null: the verb takes none), the verb's own refusals as listed, a text too large or cut
// into too many chunks, and last whether the handle has a device image (so a device-less handle
// still names a bad argument).
struct Refusal {
  bool bad;
  const char *why;
};

static int checkLongText(const redgpu_dfa *dfa, const int *style,
                         std::initializer_list<Refusal> refusals, uint64_t len,
                         uint32_t chunkBytes) {
  if (!dfa) return fail(REDGPU_EAPI, "null dfa handle");
  if (style)
    if (int rc = checkStyle(*style)) return rc;
  for (const Refusal &r : refusals)
    if (r.bad) return fail(REDGPU_EAPI, r.why);
  if (len >= (1ull << 40)) return fail(REDGPU_ELIMIT, "text too large");
  if (chunkBytes && (len + chunkBytes - 1) / chunkBytes >= (1ull << 31))
    return fail(REDGPU_ELIMIT, "too many chunks");
  return checkHandle(dfa);
}

// The _dev form of a long-text verb behind its argument check: the device, the verb's launcher -
// which launch(&name) calls, and which takes its scratch from the stream's - nothing read back
template <class F>
static int longTextDev(const redgpu_dfa *dfa, F &&launch) {
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  const char *name = "";
  const hipError_t e = launch(&name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// The host form of the two verbs that return (count, result, start, end) up to cap: the whole
// text goes up once, dev(data, count, result, start, end, stream) is the verb's _dev form over the
// staged buffers, the count and the records that were kept come back
template <class F>
static int longRecordsHost(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint64_t cap,
                           uint64_t *count, int32_t *result, uint64_t *start, uint64_t *end,
                           F &&dev) {
  if (cap > (~0ull / 16)) return fail(REDGPU_ELIMIT, "cap too large");
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dCnt = call.buf<uint64_t>(kSlAux0, 1, "count");
  int32_t *dRes = call.buf<int32_t>(kSlRes, cap + 1, "result");
  uint64_t *dStart = start ? call.buf<uint64_t>(kSlStart, cap + 1, "start") : nullptr;
  uint64_t *dEnd = end ? call.buf<uint64_t>(kSlEnd, cap + 1, "end") : nullptr;
  call.upload(dData, data, len, "data");
  call.run([&] { return dev(dData, dCnt, cap ? dRes : nullptr, dStart, dEnd, call.stream()); });
  uint64_t found = 0;
  call.download(&found, dCnt, 1, "count");
  if (int rc = call.wait()) return rc;
  *count = found;
  const uint64_t got = found < cap ? found : cap;
  if (got) {
    call.download(result, dRes, got, "result");
    if (start) call.download(start, dStart, got, "start");
    if (end) call.download(end, dEnd, got, "end");
  }
  return call.wait();
}

// The optional record columns of the grep_text / collect_text host forms: device buffers of cap
// records for the columns the caller asked for, and the filled prefixes back
struct RecordCols {
  uint64_t *line, *begin, *finish;
  int32_t *result;
  uint64_t *start, *end;

  RecordCols onDevice(HostCall &call, uint64_t cap) const {
    RecordCols d{};
    if (line && cap) d.line = call.buf<uint64_t>(kSlOff, cap, "line");
    if (begin && cap) d.begin = call.buf<uint64_t>(kSlAux1, cap, "begin");
    if (finish && cap) d.finish = call.buf<uint64_t>(kSlAux2, cap, "finish");
    if (result && cap) d.result = call.buf<int32_t>(kSlRes, cap, "result");
    if (start && cap) d.start = call.buf<uint64_t>(kSlStart, cap, "start");
    if (end && cap) d.end = call.buf<uint64_t>(kSlEnd, cap, "end");
    return d;
  }
  // (this = the caller's columns, d = onDevice's)
  void download(HostCall &call, const RecordCols &d, uint64_t got) const {
    if (!got) return;
    if (d.line) call.download(line, d.line, got, "line");
    if (d.begin) call.download(begin, d.begin, got, "begin");
    if (d.finish) call.download(finish, d.finish, got, "finish");
    if (d.result) call.download(result, d.result, got, "result");
    if (d.start) call.download(start, d.start, got, "start");
    if (d.end) call.download(end, d.end, got, "end");
  }
};

// The two phases of the host forms that assemble a text on the device (replace_long, replace_text,
// filter_text, route_text, range_text, extract_text, fields_text), behind their uploads: phase 1
// (sizes only), the nSizes size words into `sizes`, and - when out is given and put =
// min(sizes[outLenAt], outCap) is not 0 - a device output of put bytes, phase 2, and the bytes on
// their way to `out`.  dev(dOut, room, phases) is the verb's ...Dev call over the staged buffers.
// The caller adds its own downloads, waits, and only then writes the caller's counts from `sizes`,
// so a call that fails has changed none of them.
template <class F>
static void textOutHost(HostCall &call, const uint64_t *dSizes, uint64_t *sizes, uint64_t nSizes,
                        uint64_t outLenAt, uint8_t *out, uint64_t outCap, F &&dev) {
  call.run([&] { return dev(nullptr, 0, 1); });
  call.download(sizes, dSizes, nSizes, "sizes");
  if (call.wait()) return;
  const uint64_t put = sizes[outLenAt] < outCap ? sizes[outLenAt] : outCap;
  if (!out || !put) return;
  // (the streams are drained: growing the slot waits for nothing)
  uint8_t *dOut = call.buf<uint8_t>(kSlAux3, put, "out");
  call.run([&] { return dev(dOut, put, 2); });
  call.download(out, dOut, put, "out");
}

// offsets of a chunk that does not start at byte 0, rebased to the chunk's own buffer: the
// kernels may read data[0, offsets[n]) anywhere (lanes without a line re-read block 0), so a
// chunk is always presented as a batch of its own
__global__ void __launch_bounds__(256)
k_rebase(const uint64_t *in, uint64_t n1, uint64_t base, uint64_t *out) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n1; i += step)
    out[i] = in[i] - base;
}

// (the chunk plan of a host-buffer batch, chunkCuts: host_stage_plan.h)

// host-buffer form: the batch is cut into chunks of ~32 MiB of input that alternate between the
// thread's two private streams - copy in, kernel, copy out per chunk - so that with pinned
// caller memory (registered for the duration of the call when the batch has several chunks)
// the upload of one chunk runs beside the download of the previous one.  No allocation, no
// stream creation and no device-wide synchronisation per call (host_stage.h).
int runHost(const redgpu_dfa *dfa, int verb, int style, int doLeader, const uint8_t *data,
            const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
            uint64_t *start, uint64_t *end) {
  if (int rc = checkHandle(dfa)) return rc;
  if (int rc = checkStyle(style)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!result) return fail(REDGPU_EAPI, "null result buffer");
  uint64_t total = 0, maxLen = 0;
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit, &total, &maxLen)) return rc;
  // the block-wise ragged kernels keep line positions in 32 bits: a line of 4 GiB or more takes
  // the general kernel (64-bit positions) - here, where the offsets can be read
  const uint32_t extra = maxLen >= (1ull << 32) - 256 ? REDGPU_F_FORCE_GENERIC : 0u;
  HostCall call(dfa, total);
  if (!call.ok()) return call.rc();
  HostStage &st = call.stage();

  // Caller memory that is already pinned (redgpu_host_register, hipHostMalloc, torch's
  // pin_memory) is copied as it is: its copies are asynchronous as they stand, so even a batch
  // of a few MiB is worth cutting - chunks of 8 MiB alternate between the two streams and the
  // upload of one runs beside the walk and the download of the one before.  Pageable memory
  // keeps the 32 MiB chunks and is only cut above 64 MiB: below that the pinning costs more
  // than the overlap returns.  Its transfers go the way HostStage::copyIn / copyOut choose (a
  // small call's through the thread's pinned arena, a large one's whole pages registered for
  // the call - per chunk when there are several).
  const bool callerPinned = isPinnedHost(data) && isPinnedHost(result) &&
                            (!start || isPinnedHost(start)) && (!end || isPinnedHost(end));
  const std::vector<uint64_t> cuts =
      chunkCuts(offsets, stride, n, total, callerPinned ? (8ull << 20) : (32ull << 20));
  const size_t nChunks = cuts.size() - 1;
  const bool multi = nChunks > 1;
  uint64_t maxBytes = 0, maxLines = 0;
  for (size_t c = 0; c < nChunks; ++c) {
    const uint64_t lo = cuts[c], hi = cuts[c + 1];
    const uint64_t bytes = offsets ? offsets[hi] - offsets[lo] : (hi - lo) * stride;
    if (bytes > maxBytes) maxBytes = bytes;
    if (hi - lo > maxLines) maxLines = hi - lo;
  }
  uint8_t *dData[2] = {};
  int32_t *dRes[2] = {};
  uint64_t *dStart[2] = {}, *dEnd[2] = {}, *dReb[2] = {}, *dOff = nullptr;
  for (int k = 0; k < (multi ? 2 : 1); ++k) {
    dData[k] = call.buf<uint8_t>(kSlData + k, maxBytes, "data");
    dRes[k] = call.buf<int32_t>(kSlRes + k, maxLines, "result");
    if (start) dStart[k] = call.buf<uint64_t>(kSlStart + k, maxLines, "start");
    if (end) dEnd[k] = call.buf<uint64_t>(kSlEnd + k, maxLines, "end");
  }
  if (offsets) {
    dOff = call.buf<uint64_t>(kSlOff, n + 1, "offsets");
    if (multi || offsets[0])
      for (int k = 0; k < (multi ? 2 : 1); ++k)
        dReb[k] = call.buf<uint64_t>(kSlAux0 + k, maxLines + 1, "chunk offsets");
    call.upload(dOff, offsets, n + 1, "offsets", 0, callerPinned);
    if (multi && call.ok()) {  // stream 1's chunks read the offsets uploaded on stream 0
      call.check(hipEventRecord(st.ready, st.streams[0]), "hipEventRecord");
      if (call.ok())
        call.check(hipStreamWaitEvent(st.streams[1], st.ready, 0), "hipStreamWaitEvent");
    }
  }
  for (size_t c = 0; c < nChunks && call.ok(); ++c) {
    const int k = int(c & 1);
    hipStream_t s = st.streams[k];
    const uint64_t lo = cuts[c], hi = cuts[c + 1], nl = hi - lo;
    const uint64_t byteLo = offsets ? offsets[lo] : lo * stride;
    const uint64_t bytes = offsets ? offsets[hi] - byteLo : nl * stride;
    call.upload(dData[k], data + byteLo, bytes, "data", k, callerPinned);
    const uint64_t *chunkOff = offsets ? dOff + lo : nullptr;
    if (offsets && byteLo && call.ok()) {
      const uint32_t blocks = uint32_t((nl + 256) / 256 < 1024 ? (nl + 256) / 256 : 1024);
      hipLaunchKernelGGL(k_rebase, dim3(blocks), dim3(256), 0, s, dOff + lo, nl + 1, byteLo,
                         dReb[k]);
      chunkOff = dReb[k];
    }
    call.run([&] {
      return runDev(dfa, verb, style, doLeader, dData[k], chunkOff, stride, nl, dRes[k],
                    dStart[k], dEnd[k], s, extra);
    });
    call.download(result + lo, dRes[k], nl, "result", k, callerPinned);
    if (start) call.download(start + lo, dStart[k], nl, "start", k, callerPinned);
    if (end) call.download(end + lo, dEnd[k], nl, "end", k, callerPinned);
  }
  return call.wait(-1);
}

// the two verbs that emit a variable-length record list per line
enum ListVerb : int { kListCollect = 0, kListMatchAll = 1, kListMatchAllLeader = 2 };

int collectDev(const redgpu_dfa *dfa, int listVerb, const uint8_t *data, const uint64_t *offsets,
               uint64_t stride, uint64_t n, uint64_t cap, uint64_t *counts, int32_t *result,
               uint64_t *start, uint64_t *end, hipStream_t stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!counts) return fail(REDGPU_EAPI, "null counts buffer");
  if (cap && !result) return fail(REDGPU_EAPI, "null result buffer");
  if (int rc = checkBatch(data, offsets, stride, n, 0)) return rc;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  Batch b{data, offsets, stride, n, result, start, end};
  LaunchCfg cfg{dfa->numCUs, (dfa->flags & REDGPU_F_FORCE_GENERIC) ? 1 : 0};
  const char *name = "k_collect";
  hipError_t e = listVerb == kListCollect
                     ? launchCollect(dfa->im->dev, b, cap, counts, cfg, stream)
                     : launchMatchAll(dfa->im->dev, b, cap, counts, listVerb == kListMatchAllLeader,
                                      cfg, stream, &name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// Uploads im->img to im->device.  Caller holds the device scope.
int uploadImage(SharedImage *im) {
  const DfaImage &img = im->img;
  uint8_t eqLead[1024];
  std::memcpy(eqLead, img.equiv, 256);
  std::memcpy(eqLead + 256, img.leader, 256);
  std::memcpy(eqLead + 512, img.startFlags[0], 256);
  std::memcpy(eqLead + 768, img.startFlags[1], 256);
  const size_t tabBytes = (img.table.size() + 15) & ~size_t(15);
  hipError_t e;
  if ((e = hipMalloc(&im->dTable, tabBytes + 16)) != hipSuccess) return failHip(e, "hipMalloc table");
  if ((e = hipMalloc(&im->dResult, img.nStates * sizeof(int32_t) + 16)) != hipSuccess)
    return failHip(e, "hipMalloc result");
  if ((e = hipMalloc(&im->dEquivLeader, 1024 + 64)) != hipSuccess) return failHip(e, "hipMalloc equiv");
  if ((e = hipMemset(im->dTable, 0, tabBytes + 16)) != hipSuccess) return failHip(e, "hipMemset");
  // The table and the result array are heap memory of this process (std::vector): uploaded
  // THROUGH A PINNED BUFFER of the library's own, never as they are - above ~1 MiB the runtime
  // would pin the vector's pages on the fly, by address, and a GPU fault at a heap address was
  // seen three times exactly here, under the 2 MiB table of SYN-4K, when the heap around it
  // had just been registered and released for a host-buffer call.
  auto upload = [](void *dst, const void *src, size_t bytes) -> hipError_t {
    if (bytes == 0) return hipSuccess;
    void *pin = nullptr;
    hipError_t e2 = hipHostMalloc(&pin, bytes, hipHostMallocDefault);
    if (e2 != hipSuccess) return e2;
    std::memcpy(pin, src, bytes);
    e2 = hipMemcpy(dst, pin, bytes, hipMemcpyHostToDevice);
    (void)hipHostFree(pin);
    return e2;
  };
  if ((e = upload(im->dTable, img.table.data(), img.table.size())) != hipSuccess)
    return failHip(e, "upload table");
  if ((e = upload(im->dResult, img.result.data(), img.nStates * sizeof(int32_t))) != hipSuccess)
    return failHip(e, "upload result");
  if ((e = hipMemcpy(im->dEquivLeader, eqLead, 1024, hipMemcpyHostToDevice)) != hipSuccess)
    return failHip(e, "upload equiv");

  DevDfa &d = im->dev;
  d.table = static_cast<const uint8_t *>(im->dTable);
  d.result = static_cast<const int32_t *>(im->dResult);
  d.equivLeader = static_cast<const uint8_t *>(im->dEquivLeader);
  d.sink = static_cast<uint8_t *>(im->dEquivLeader) + 512;
  d.tableKind = img.tableKind;
  d.tableBytes = (img.primaryBytes + 15u) & ~15u;  // the tableKind table only (LDS staging size)
  d.nStates = img.nStates;
  d.nClasses = img.nClasses;
  d.init = img.init;
  d.leaderNext = img.leaderNext;
  d.nPureDead = img.nPureDead;
  d.firstAccept = img.firstAccept;
  d.leaderLen = img.leaderLen;
  d.deadAbsorbing = img.deadAbsorbing ? 1 : 0;
  d.hotLo = img.hotLo;
  d.nHot = img.nHot;
  d.hot8Off = img.hot8Off;
  d.hotShift = img.hotShift;
  d.earlyDeath = img.earlyDeath ? 1 : 0;
  d.clsOff = img.clsOff;
  d.clsRowBytes = img.clsRowBytes;
  d.clsBytes = img.clsBytes;
  d.clsIndexForm = img.clsIndexForm ? 1 : 0;
  d.sparseCombOff = img.sparseCombOff;
  d.sparseDefault = img.sparseDefault;
  d.tuned = img.tuned ? 1 : 0;
  d.forgetful = img.forgetful ? 1 : 0;
  d.suffixClosed = img.suffixClosed ? 1 : 0;
  d.uniformResult = img.uniformResult ? 1 : 0;
  d.leaderForced = img.leaderForced ? 1 : 0;
  {
    const char *e = getenv("REDGPU_GATHER_NT");
    d.gatherNt = e && e[0] == '1';
  }
  d.startLeadWord = img.startLeadWord;
  d.startLeadCount = img.startLeadCount;
  d.startFreeWord = img.startFreeWord;
  d.startFreeCount = img.startFreeCount;
  d.start2LeadWord = img.start2LeadWord;
  d.start2LeadCount = img.start2LeadCount;
  d.start2FreeWord = img.start2FreeWord;
  d.start2FreeCount = img.start2FreeCount;
  for (int k = 0; k < 2; ++k) {
    d.startTotal[k] = img.startTotal[k];
    d.startFollow[k] = img.startFollow[k] ? 1u : 0u;
  }
  return REDGPU_OK;
}

// Loader cache (the reference's load path, lib/Serializer.cpp:257-267, hands
// every caller its own Executable): a service that creates many handles from the same blob pays
// for validation, repack and upload once per (blob, device, build options).  Entries are weak:
// the image goes away with its last handle.
struct CacheKey {
  uint32_t checksum;
  size_t len;
  int device;
  uint32_t buildFlags, ldsTableMax;
  bool operator==(const CacheKey &o) const {
    return checksum == o.checksum && len == o.len && device == o.device &&
           buildFlags == o.buildFlags && ldsTableMax == o.ldsTableMax;
  }
};
struct CacheKeyHash {
  size_t operator()(const CacheKey &k) const {
    uint64_t h = k.checksum;
    h = h * 1099511628211ull ^ k.len;
    h = h * 1099511628211ull ^ uint64_t(uint32_t(k.device));
    h = h * 1099511628211ull ^ k.buildFlags;
    h = h * 1099511628211ull ^ k.ldsTableMax;
    return size_t(h);
  }
};
std::mutex gCacheMutex;
std::unordered_map<CacheKey, std::weak_ptr<SharedImage>, CacheKeyHash> gCache;
constexpr uint32_t kBuildFlagMask = REDGPU_F_FORCE_GLOBAL | REDGPU_F_FORCE_HOT;

} // namespace

extern "C" {

int redgpu_version(void) { return 100; }

const char *redgpu_last_error(void) { return tlsError.c_str(); }

const char *redgpu_last_kernel(void) { return tlsKernel; }

int redgpu_reda_check(const void *reda, size_t len, const char **msg) {
  const char *m = (reda && len) ? checkHeader(reda, len) : "serialized dfa is empty";
  if (msg) *msg = m;
  if (m) return fail(REDGPU_EAPI, m);
  return REDGPU_OK;
}

int redgpu_dfa_create(const void *reda, size_t len, const redgpu_opts *opts, redgpu_dfa **out) {
  if (!out) return fail(REDGPU_EAPI, "null output handle");
  *out = nullptr;
  redgpu_opts o{};
  o.device = REDGPU_DEVICE_CURRENT;
  if (opts) o = *opts;
  if (!reda || len == 0) return fail(REDGPU_EAPI, "serialized dfa is empty");
  if (const char *m = checkHeader(reda, len)) return fail(REDGPU_EAPI, m);

  int dev = o.device;
  int numCUs = 0;
  if (dev != REDGPU_DEVICE_NONE) {
    if (dev == REDGPU_DEVICE_CURRENT) {
      hipError_t e = hipGetDevice(&dev);
      if (e != hipSuccess) return failHip(e, "hipGetDevice");
    }
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return failHip(e, "hipGetDeviceProperties");
    numCUs = prop.multiProcessorCount;
  }

  redgpu_dfa *h = new (std::nothrow) redgpu_dfa();
  if (!h) return fail(REDGPU_ELIMIT, "out of host memory");
  h->flags = o.flags;
  h->ldsTableMax = o.lds_table_max;
  h->numCUs = numCUs;

  // the header is valid, so the checksum is the FNV-1a-32 of the payload: the cache key
  const CacheKey key{calcChecksum(reda, len), len, dev, o.flags & kBuildFlagMask, o.lds_table_max};
  {
    std::lock_guard<std::mutex> lock(gCacheMutex);
    auto it = gCache.find(key);
    if (it != gCache.end()) {
      if (std::shared_ptr<SharedImage> hit = it->second.lock()) {
        if (hit->blob.size() == len && std::memcmp(hit->blob.data(), reda, len) == 0) {
          h->im = std::move(hit);
          *out = h;
          return REDGPU_OK;
        }
      } else {
        gCache.erase(it);
      }
    }
  }

  auto im = std::make_shared<SharedImage>();
  int code = REDGPU_OK;
  std::string err = buildImage(reda, len, o.lds_table_max, (o.flags & REDGPU_F_FORCE_GLOBAL) != 0,
                               im->img, code, (o.flags & REDGPU_F_FORCE_HOT) != 0);
  if (!err.empty()) {
    delete h;
    return fail(code, err);
  }
  im->blob.assign(static_cast<const uint8_t *>(reda), static_cast<const uint8_t *>(reda) + len);
  im->buildFlags = key.buildFlags;
  im->ldsTableMax = o.lds_table_max;
  im->device = dev;
  if (dev != REDGPU_DEVICE_NONE) {
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) { delete h; return failHip(scope.err, "hipSetDevice"); }
    if (int rc = uploadImage(im.get())) { delete h; return rc; }
  }
  h->im = im;
  {
    std::lock_guard<std::mutex> lock(gCacheMutex);
    gCache[key] = im;
  }
  *out = h;
  return REDGPU_OK;
}

void redgpu_dfa_destroy(redgpu_dfa *h) {
  delete h;  // the shared image goes with its last handle (~SharedImage frees the device side)
}

int redgpu_dfa_info(const redgpu_dfa *h, redgpu_info *out) {
  if (!h || !out) return fail(REDGPU_EAPI, "null argument");
  const DfaImage &img = h->im->img;
  out->format = img.format;
  out->n_classes = img.nClasses;
  out->leader_len = img.leaderLen;
  out->states_total = img.statesTotal;
  out->states_used = img.nStates;
  out->n_pure_dead = img.nPureDead;
  out->first_accept = img.firstAccept;
  out->table_kind = img.tableKind;
  out->table_bytes = img.primaryBytes;
  out->max_result = img.maxResult;
  out->device = h->im->device;
  out->checksum = img.checksum;
  out->fast_path = (img.tableKind == REDGPU_TAB_LDS_FUSED_U8 && img.deadAbsorbing &&
                    !(h->flags & REDGPU_F_FORCE_GENERIC) &&
                    (!img.earlyDeath || (h->flags & REDGPU_F_FORCE_STREAM))) ? 1 : 0;
  out->n_hot = img.nHot;
  out->hot_lo = img.hotLo;
  out->hot_coverage_ppm = img.hotCoveragePpm;
  out->early_death = img.earlyDeath ? 1 : 0;
  out->forgetful = img.forgetful ? 1 : 0;
  out->suffix_closed = img.suffixClosed ? 1 : 0;
  out->image_refs = uint32_t(h->im.use_count());
  return REDGPU_OK;
}

int redgpu_dfa_serialized(const redgpu_dfa *h, const void **reda, size_t *len) {
  if (!h || !reda || !len) return fail(REDGPU_EAPI, "null argument");
  *reda = h->im->blob.data();
  *len = h->im->blob.size();
  return REDGPU_OK;
}

int redgpu_check_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result) {
  return runHost(dfa, kCheck, style, do_leader, data, offsets, stride, n, result, nullptr,
                 nullptr);
}

int redgpu_match_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                       uint64_t *start, uint64_t *end) {
  return runHost(dfa, kMatch, style, do_leader, data, offsets, stride, n, result, start, end);
}

int redgpu_scan_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                      const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result) {
  return runHost(dfa, kScan, style, do_leader, data, offsets, stride, n, result, nullptr,
                 nullptr);
}

int redgpu_search_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                        const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                        uint64_t *start, uint64_t *end) {
  return runHost(dfa, kSearch, style, do_leader, data, offsets, stride, n, result, start, end);
}

int redgpu_search_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                            const uint64_t *offsets, uint64_t stride, uint64_t n,
                            int32_t *result, uint64_t *start, uint64_t *end, void *stream) {
  return runDev(dfa, kSearch, style, do_leader, data, offsets, stride, n, result, start, end,
                static_cast<hipStream_t>(stream));
}

int redgpu_collect_batch_dev(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                             uint64_t stride, uint64_t n, uint64_t cap, uint64_t *counts,
                             int32_t *result, uint64_t *start, uint64_t *end, void *stream) {
  return collectDev(dfa, kListCollect, data, offsets, stride, n, cap, counts, result, start, end,
                    static_cast<hipStream_t>(stream));
}

int redgpu_match_all_batch_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                               const uint64_t *offsets, uint64_t stride, uint64_t n,
                               uint64_t cap, uint64_t *counts, int32_t *result, uint64_t *start,
                               uint64_t *end, void *stream) {
  return collectDev(dfa, do_leader ? kListMatchAllLeader : kListMatchAll, data, offsets, stride, n,
                    cap, counts, result, start, end, static_cast<hipStream_t>(stream));
}

static int listHost(const redgpu_dfa *dfa, int listVerb, const uint8_t *data,
                    const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t cap,
                    uint64_t *counts, int32_t *result, uint64_t *start, uint64_t *end);

int redgpu_collect_batch(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                         uint64_t stride, uint64_t n, uint64_t cap, uint64_t *counts,
                         int32_t *result, uint64_t *start, uint64_t *end) {
  return listHost(dfa, kListCollect, data, offsets, stride, n, cap, counts, result, start, end);
}

int redgpu_match_all_batch(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t cap,
                           uint64_t *counts, int32_t *result, uint64_t *start, uint64_t *end) {
  return listHost(dfa, do_leader ? kListMatchAllLeader : kListMatchAll, data, offsets, stride, n,
                  cap, counts, result, start, end);
}

static int listHost(const redgpu_dfa *dfa, int listVerb, const uint8_t *data,
                    const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t cap,
                    uint64_t *counts, int32_t *result, uint64_t *start, uint64_t *end) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!counts) return fail(REDGPU_EAPI, "null counts buffer");
  if (cap && !result) return fail(REDGPU_EAPI, "null result buffer");
  uint64_t total = 0;
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit, &total, nullptr, cap)) return rc;
  HostCall call(dfa, total);
  const uint64_t slots = n * cap;
  uint8_t *dData = call.buf<uint8_t>(kSlData, total, "data");
  uint64_t *dCnt = call.buf<uint64_t>(kSlAux0, n, "counts");
  int32_t *dRes = call.buf<int32_t>(kSlRes, slots + 1, "result");
  uint64_t *dStart = start ? call.buf<uint64_t>(kSlStart, slots + 1, "start") : nullptr;
  uint64_t *dEnd = end ? call.buf<uint64_t>(kSlEnd, slots + 1, "end") : nullptr;
  uint64_t *dOff = offsets ? call.buf<uint64_t>(kSlOff, n + 1, "offsets") : nullptr;
  if (offsets) call.upload(dOff, offsets, n + 1, "offsets");
  call.upload(dData, data, total, "data");
  call.run([&] {
    return collectDev(dfa, listVerb, dData, dOff, stride, n, cap, dCnt, dRes, dStart, dEnd,
                      call.stream());
  });
  call.download(counts, dCnt, n, "counts");
  if (slots) {
    call.download(result, dRes, slots, "result");
    if (start) call.download(start, dStart, slots, "start");
    if (end) call.download(end, dEnd, slots, "end");
  }
  return call.wait();
}

static int checkRecordsLong(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                            uint32_t chunkBytes, uint64_t cap, const uint64_t *count,
                            const int32_t *result) {
  return checkLongText(dfa, nullptr,
                       {{!count, "null count buffer"},
                        {cap && !result, "null result buffer"},
                        {len && !data, "null data buffer"}},
                       len, chunkBytes);
}

// Red::collect over one text, chunk-parallel (k_collect_long.h)
int redgpu_collect_long_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                            uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                            uint64_t *start, uint64_t *end, void *stream) {
  if (int rc = checkRecordsLong(dfa, data, len, chunk_bytes, cap, count, result)) return rc;
  return longTextDev(dfa, [&](const char **name) {
    const LaunchCfg cfg{dfa->numCUs, (dfa->flags & REDGPU_F_FORCE_GENERIC) ? 1 : 0};
    return launchCollectLong(dfa->im->dev, data, len, chunk_bytes, cap, count, result, start, end,
                             cfg, static_cast<hipStream_t>(stream), name);
  });
}

int redgpu_collect_long(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                        uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                        uint64_t *start, uint64_t *end) {
  if (int rc = checkRecordsLong(dfa, data, len, chunk_bytes, cap, count, result)) return rc;
  return longRecordsHost(dfa, data, len, cap, count, result, start, end,
                         [&](const uint8_t *d, uint64_t *c, int32_t *r, uint64_t *s, uint64_t *e,
                             hipStream_t st) {
                           return redgpu_collect_long_dev(dfa, d, len, chunk_bytes, cap, c, r, s, e, st);
                         });
}

// the control words of this thread's last chunked match_all_long call, and the stream it ran on
static thread_local const uint32_t *tlsMlCtl = nullptr;
static thread_local hipStream_t tlsMlStream = nullptr;

// matchAll over one text, chunk-parallel (k_match_all_long.h)
int redgpu_match_all_long_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                              uint64_t len, uint32_t chunk_bytes, uint64_t cap, uint64_t *count,
                              int32_t *result, uint64_t *start, uint64_t *end, void *stream) {
  if (int rc = checkRecordsLong(dfa, data, len, chunk_bytes, cap, count, result)) return rc;
  return longTextDev(dfa, [&](const char **name) {
    const LaunchCfg cfg{dfa->numCUs, (dfa->flags & REDGPU_F_FORCE_GENERIC) ? 1 : 0};
    tlsMlStream = static_cast<hipStream_t>(stream);
    return launchMatchAllLong(dfa->im->dev, do_leader ? 1 : 0, data, len, chunk_bytes, cap, count,
                              result, start, end, cfg, tlsMlStream, name, &tlsMlCtl);
  });
}

int redgpu_match_all_long(const redgpu_dfa *dfa, int do_leader, const uint8_t *data, uint64_t len,
                          uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                          uint64_t *start, uint64_t *end) {
  if (int rc = checkRecordsLong(dfa, data, len, chunk_bytes, cap, count, result)) return rc;
  return longRecordsHost(dfa, data, len, cap, count, result, start, end,
                         [&](const uint8_t *d, uint64_t *c, int32_t *r, uint64_t *s, uint64_t *e,
                             hipStream_t st) {
                           return redgpu_match_all_long_dev(dfa, do_leader, d, len, chunk_bytes, cap, c,
                                                            r, s, e, st);
                         });
}

// how the calling thread's last redgpu_match_all_long_dev call resolved its chunks
int redgpu_diag_match_all_long_dev(const redgpu_dfa *dfa, uint32_t *stats, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!stats) return fail(REDGPU_EAPI, "null stats buffer");
  if (!tlsMlCtl || tlsMlStream != static_cast<hipStream_t>(stream))
    return fail(REDGPU_EAPI, "no chunked match_all_long call of this thread on this stream");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  const hipError_t e = hipMemcpyAsync(stats, tlsMlCtl, 8 * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                      static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return failHip(e, "hipMemcpyAsync");
  return REDGPU_OK;
}

int redgpu_replace_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                             const uint64_t *offsets, uint64_t stride, uint64_t n,
                             const uint8_t *repl, uint64_t repl_len, uint64_t max_count,
                             uint64_t *counts, uint64_t *out_offsets, uint8_t *out,
                             uint64_t out_cap, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (int rc = checkStyle(style)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!counts || !out_offsets) return fail(REDGPU_EAPI, "null output buffer");
  if (int rc = checkBatch(data, offsets, stride, n, kTrailingLimit)) return rc;
  if (repl_len && !repl) return fail(REDGPU_EAPI, "null replacement");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  Batch b{data, offsets, stride, n, nullptr, nullptr, nullptr};
  LaunchCfg cfg{dfa->numCUs, 0};
  hipError_t e = launchReplace(dfa->im->dev, b, style, do_leader ? 1 : 0, repl, repl_len, max_count,
                               counts, out_offsets, out, out_cap, cfg,
                               static_cast<hipStream_t>(stream));
  tlsKernel = "k_replace";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_replace_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                         const uint64_t *offsets, uint64_t stride, uint64_t n, const uint8_t *repl,
                         uint64_t repl_len, uint64_t max_count, uint64_t *counts,
                         uint64_t *out_offsets, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkHandle(dfa)) return rc;
  if (int rc = checkStyle(style)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!counts || !out_offsets) return fail(REDGPU_EAPI, "null output buffer");
  uint64_t total = 0;
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit, &total)) return rc;
  if (repl_len && !repl) return fail(REDGPU_EAPI, "null replacement");
  HostCall call(dfa, total);
  uint8_t *dData = call.buf<uint8_t>(kSlData, total, "data");
  uint8_t *dRepl = call.buf<uint8_t>(kSlAux0, repl_len, "repl");
  uint64_t *dCnt = call.buf<uint64_t>(kSlAux1, n, "counts");
  uint64_t *dOutOff = call.buf<uint64_t>(kSlAux2, n + 1, "out offsets");
  uint8_t *dOut = out && out_cap ? call.buf<uint8_t>(kSlAux3, out_cap, "out") : nullptr;
  uint64_t *dOff = offsets ? call.buf<uint64_t>(kSlOff, n + 1, "offsets") : nullptr;
  if (offsets) call.upload(dOff, offsets, n + 1, "offsets");
  call.upload(dData, data, total, "data");
  call.upload(dRepl, repl, repl_len, "repl");
  call.run([&] {
    return redgpu_replace_batch_dev(dfa, style, do_leader, dData, dOff, stride, n, dRepl,
                                    repl_len, max_count, dCnt, dOutOff, dOut,
                                    dOut ? out_cap : 0, call.stream());
  });
  call.download(counts, dCnt, n, "counts");
  call.download(out_offsets, dOutOff, n + 1, "out offsets");
  if (int rc = call.wait()) return rc;
  if (!dOut) return REDGPU_OK;
  // the lines that fit are a prefix (offsets are monotone): copy up to the last one that does
  uint64_t lo = 0, hi = n;  // largest k with out_offsets[k] <= out_cap
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (out_offsets[mid] <= out_cap) lo = mid; else hi = mid - 1;
  }
  if (!out_offsets[lo]) return REDGPU_OK;
  call.download(out, dOut, out_offsets[lo], "out");
  return call.wait();
}

static int checkReplaceLong(const redgpu_dfa *dfa, int style, const uint8_t *data, uint64_t len,
                            uint32_t chunkBytes, const uint8_t *repl, uint64_t replLen,
                            const uint64_t *count, const uint64_t *outLen) {
  return checkLongText(dfa, &style,
                       {{!count, "null count buffer"},
                        {!outLen, "null out_len buffer"},
                        {len && !data, "null data buffer"},
                        {replLen && !repl, "null replacement"}},
                       len, chunkBytes);
}

// replaceCore over one text, chunk-parallel (k_replace_long.h); phases as launchReplaceLong's
static int replaceLongDev(const redgpu_dfa *dfa, int style, int doLeader, const uint8_t *data,
                          uint64_t len, uint32_t chunkBytes, const uint8_t *repl, uint64_t replLen,
                          uint64_t maxCount, uint64_t *count, uint64_t *outLen, uint8_t *out,
                          uint64_t outCap, int phases, hipStream_t stream) {
  if (int rc = checkReplaceLong(dfa, style, data, len, chunkBytes, repl, replLen, count, outLen))
    return rc;
  return longTextDev(dfa, [&](const char **name) {
    return launchReplaceLong(dfa->im->dev, style, doLeader ? 1 : 0, data, len, chunkBytes, repl,
                             replLen, maxCount, count, outLen, out, outCap, phases,
                             LaunchCfg{dfa->numCUs, 0}, stream, name);
  });
}

int redgpu_replace_long_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                            uint64_t len, uint32_t chunk_bytes, const uint8_t *repl,
                            uint64_t repl_len, uint64_t max_count, uint64_t *count,
                            uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream) {
  return replaceLongDev(dfa, style, do_leader, data, len, chunk_bytes, repl, repl_len, max_count,
                        count, out_len, out, out_cap, 3, static_cast<hipStream_t>(stream));
}

// the text and repl go up once, then textOutHost; phase 1 leaves the records in the stream's
// scratch, phase 2 assembles the output from them: the text is walked once
int redgpu_replace_long(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                        uint64_t len, uint32_t chunk_bytes, const uint8_t *repl, uint64_t repl_len,
                        uint64_t max_count, uint64_t *count, uint64_t *out_len, uint8_t *out,
                        uint64_t out_cap) {
  if (int rc = checkReplaceLong(dfa, style, data, len, chunk_bytes, repl, repl_len, count, out_len))
    return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint8_t *dRepl = call.buf<uint8_t>(kSlAux0, repl_len, "repl");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 2, "sizes");
  call.upload(dData, data, len, "data");
  call.upload(dRepl, repl, repl_len, "repl");
  uint64_t sizes[2] = {0, 0};
  textOutHost(call, dSizes, sizes, 2, 1, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return replaceLongDev(dfa, style, do_leader, dData, len, chunk_bytes, dRepl, repl_len,
                          max_count, dSizes, dSizes + 1, dOut, room, phases, call.stream());
  });
  if (int rc = call.wait()) return rc;
  *count = sizes[0];
  *out_len = sizes[1];
  return REDGPU_OK;
}

static int checkSearchLong(const redgpu_dfa *dfa, int style, const uint8_t *data, uint64_t len,
                           uint32_t chunkBytes, const int32_t *result) {
  return checkLongText(dfa, &style,
                       {{!result, "null result buffer"}, {len && !data, "null data buffer"}}, len,
                       chunkBytes);
}

// searchCore over one text, chunk-parallel (k_search_long.h)
int redgpu_search_long_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           uint64_t len, uint32_t chunk_bytes, int32_t *result, uint64_t *start,
                           uint64_t *end, void *stream) {
  if (int rc = checkSearchLong(dfa, style, data, len, chunk_bytes, result)) return rc;
  return longTextDev(dfa, [&](const char **name) {
    return launchSearchLong(dfa->im->dev, style, do_leader ? 1 : 0, data, len, chunk_bytes, result,
                            start, end, cfgOf(dfa), static_cast<hipStream_t>(stream), name);
  });
}

// the text goes up once, the three values of the Outcome come back
int redgpu_search_long(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       uint64_t len, uint32_t chunk_bytes, int32_t *result, uint64_t *start,
                       uint64_t *end) {
  if (int rc = checkSearchLong(dfa, style, data, len, chunk_bytes, result)) return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  int32_t *dRes = call.buf<int32_t>(kSlRes, 1, "result");
  uint64_t *dPos = call.buf<uint64_t>(kSlAux0, 2, "start and end");
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_search_long_dev(dfa, style, do_leader, dData, len, chunk_bytes, dRes, dPos,
                                  dPos + 1, call.stream());
  });
  int32_t res = 0;
  uint64_t pos[2] = {0, 0};
  call.download(&res, dRes, 1, "result");
  call.download(pos, dPos, 2, "start and end");
  if (int rc = call.wait()) return rc;
  *result = res;
  if (start) *start = pos[0];
  if (end) *end = pos[1];
  return REDGPU_OK;
}

int redgpu_split_lines_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t *offsets, uint64_t cap, uint64_t *n_lines, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!offsets || !n_lines) return fail(REDGPU_EAPI, "null output buffer");
  if (len && !data) return fail(REDGPU_EAPI, "null data buffer");
  if (splitChunks(len) >= (1ull << 31)) return fail(REDGPU_ELIMIT, "buffer too large");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t nChunks = splitChunks(len);
  void *scratch = nullptr;
  // counts u32[nChunks], bases u64[nChunks], then the delimiter masks (2 bytes per 16 of input):
  // the calling thread's scratch for this stream (kernels.h) - what the next launch on the
  // stream does with the same buffer comes behind these kernels
  const size_t countBytes = (size_t(nChunks) * 4 + 15) & ~size_t(15);
  const size_t headBytes = countBytes + size_t(nChunks) * 8 + 16;
  HIP_TRY(scratchFor(s, headBytes + splitMaskBytes(len) + 16, &scratch), "hipMalloc scratch");
  uint32_t *counts = static_cast<uint32_t *>(scratch);
  uint64_t *bases = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(scratch) + countBytes);
  uint16_t *masks = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(scratch) + headBytes);
  hipError_t e = launchSplitLines(data, len, delim, offsets, cap, n_lines, counts, bases, masks, s);
  tlsKernel = "k_split_scatter";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

// raw text -> lines -> check / match, one call, everything on `stream`
static int textDev(const redgpu_dfa *dfa, int verb, int style, int doLeader, const uint8_t *data,
                   uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap, uint64_t *n_lines,
                   int32_t *result, uint64_t *start, uint64_t *end, void *stream) {
  if (!dfa) return fail(REDGPU_EAPI, "null dfa handle");
  if (int rc = checkStyle(style)) return rc;
  if (cap && !result) return fail(REDGPU_EAPI, "null result buffer");
  if (int rc = redgpu_split_lines_dev(dfa, data, len, delim, offsets, cap, n_lines, stream)) return rc;
  if (cap > len) cap = len;  // a buffer holds no more lines than bytes
  if (cap == 0) return REDGPU_OK;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Batch b{data, offsets, 1, cap, result, start, end};
  b.nDev = n_lines;
  const LaunchCfg cfg = cfgOf(dfa);
  const char *name = "";
  hipError_t e = launchBatch(dfa->im->dev, b, verb, style, doLeader ? 1 : 0, cfg, s, &name);
  if (e == hipSuccess) {
    tlsKernel = name;
    return REDGPU_OK;
  }
  if (e != hipErrorNotSupported) return failHip(e, "kernel launch");
  (void)hipGetLastError();
  // a kernel family that takes its line count from the host: wait for the split
  uint64_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, n_lines, 8, hipMemcpyDeviceToHost, s), "copy line count");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return runDev(dfa, verb, style, doLeader, data, offsets, 1, n < cap ? n : cap, result, start,
                end, s);
}

int redgpu_check_text_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                          uint64_t *n_lines, int32_t *result, void *stream) {
  return textDev(dfa, kCheck, style, do_leader, data, len, delim, offsets, cap, n_lines, result,
                 nullptr, nullptr, stream);
}

int redgpu_match_text_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                          uint64_t *n_lines, int32_t *result, uint64_t *start, uint64_t *end,
                          void *stream) {
  return textDev(dfa, kMatch, style, do_leader, data, len, delim, offsets, cap, n_lines, result,
                 start, end, stream);
}

// host-buffer form: one upload, split + verb on the device, the filled prefixes back
int redgpu_match_text(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                      uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                      uint64_t *n_lines, int32_t *result, uint64_t *start, uint64_t *end) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!n_lines) return fail(REDGPU_EAPI, "null output buffer");
  if (cap && (!offsets || !result)) return fail(REDGPU_EAPI, "null output buffer");
  if (len && !data) return fail(REDGPU_EAPI, "null data buffer");
  HostCall call(dfa, len);
  if (cap > len) cap = len;
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 1, "count");
  uint64_t *dOff = call.buf<uint64_t>(kSlOff, cap + 1, "offsets");
  int32_t *dRes = call.buf<int32_t>(kSlRes, cap, "result");
  uint64_t *dStart = start ? call.buf<uint64_t>(kSlStart, cap, "start") : nullptr;
  uint64_t *dEnd = end ? call.buf<uint64_t>(kSlEnd, cap, "end") : nullptr;
  call.upload(dData, data, len, "data");
  call.run([&] {
    return textDev(dfa, start || end ? kMatch : kCheck, style, do_leader, dData, len, delim, dOff,
                   cap, dN, dRes, dStart, dEnd, call.stream());
  });
  call.download(n_lines, dN, 1, "count");
  if (int rc = call.wait()) return rc;
  const uint64_t got = *n_lines < cap ? *n_lines : cap;
  if (cap) call.download(offsets, dOff, got + 1, "offsets");
  if (got) {
    call.download(result, dRes, got, "result");
    if (start) call.download(start, dStart, got, "start");
    if (end) call.download(end, dEnd, got, "end");
  }
  return call.wait();
}

// The arguments of both forms of a raw-text verb (grep_text, collect_text, tally_text,
// replace_text): what can be refused without a device first, in this order - no handle, no `need`
// buffer (needError), no data, the verb's own refusal (ownError, null = none), a bad style (style
// null: the verb takes none), a text (uniq_text: of maxLen bytes or more) or (tally_text,
// route_text) a bin count too large, a handle that is not one.
static int checkRawText(const redgpu_dfa *dfa, const void *need, const char *needError,
                        const uint8_t *data, uint64_t len, const char *ownError, const int *style,
                        uint64_t nBins = 0, uint64_t maxBins = 1ull << 31,
                        uint64_t maxLen = ~0ull) {
  if (!dfa) return fail(REDGPU_EAPI, "null dfa handle");
  if (!need) return fail(REDGPU_EAPI, needError);
  if (len && !data) return fail(REDGPU_EAPI, "null data buffer");
  if (ownError) return fail(REDGPU_EAPI, ownError);
  if (style)
    if (int rc = checkStyle(*style)) return rc;
  if (splitChunks(len) >= (1ull << 31) || len >= maxLen)
    return fail(REDGPU_ELIMIT, "buffer too large");
  if (nBins > maxBins) return fail(REDGPU_ELIMIT, "n_bins too large");
  return checkHandle(dfa);
}

// raw text -> the lines search selects, as records in text order (k_grep.h): everything on
// `stream`, no count read back
int redgpu_grep_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                         const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_count,
                         uint64_t cap, uint64_t *n_lines, uint64_t *n_selected, uint64_t *line,
                         uint64_t *begin, uint64_t *finish, int32_t *result, uint64_t *start,
                         uint64_t *end, void *stream) {
  if (int rc = checkRawText(dfa, n_selected, "null n_selected buffer", data, len, nullptr, &style))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, grepScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchGrepText(dfa->im->dev, style, do_leader ? 1 : 0, invert ? 1 : 0, data, len, delim,
                          max_count, cap, n_lines, n_selected, line, begin, finish, result, start,
                          end, scratch, cfg, s, name);
  });
}

// host-buffer form: one upload of the text, then the two counts and the filled prefixes back
int redgpu_grep_text(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                     const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_count,
                     uint64_t cap, uint64_t *n_lines, uint64_t *n_selected, uint64_t *line,
                     uint64_t *begin, uint64_t *finish, int32_t *result, uint64_t *start,
                     uint64_t *end) {
  if (int rc = checkRawText(dfa, n_selected, "null n_selected buffer", data, len, nullptr, &style))
    return rc;
  if (cap > len) cap = len;  // a buffer holds no more lines than bytes
  if (cap > max_count) cap = max_count;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 2, "counts");
  const RecordCols host{line, begin, finish, result, start, end};
  const RecordCols d = host.onDevice(call, cap);
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_grep_text_dev(dfa, style, do_leader, invert, dData, len, delim, max_count, cap,
                                dN, dN + 1, d.line, d.begin, d.finish, d.result, d.start, d.end,
                                call.stream());
  });
  uint64_t counts[2] = {0, 0};
  call.download(counts, dN, 2, "counts");
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = counts[0];
  *n_selected = counts[1];
  host.download(call, d, counts[1] < cap ? counts[1] : cap);
  return call.wait();
}

// raw text -> every match of every line, as records in text order (k_collect_text.h): everything
// on `stream`, no count read back
int redgpu_collect_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t cap, uint64_t *n_lines, uint64_t *n_matches, uint64_t *line,
                            uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end,
                            void *stream) {
  if (int rc = checkRawText(dfa, n_matches, "null n_matches buffer", data, len, nullptr, nullptr))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, collectTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchCollectText(dfa->im->dev, data, len, delim, cap, n_lines, n_matches, line, begin,
                             result, start, end, scratch, cfg, s, name);
  });
}

// host-buffer form: one upload of the text, then the two counts and the filled prefixes back
int redgpu_collect_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t cap, uint64_t *n_lines, uint64_t *n_matches, uint64_t *line,
                        uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end) {
  if (int rc = checkRawText(dfa, n_matches, "null n_matches buffer", data, len, nullptr, nullptr))
    return rc;
  if (cap > len) cap = len;  // a match has a byte of its own: no more records than bytes
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 2, "counts");
  const RecordCols host{line, begin, nullptr, result, start, end};
  const RecordCols d = host.onDevice(call, cap);
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_collect_text_dev(dfa, dData, len, delim, cap, dN, dN + 1, d.line, d.begin,
                                   d.result, d.start, d.end, call.stream());
  });
  uint64_t counts[2] = {0, 0};
  call.download(counts, dN, 2, "counts");
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = counts[0];
  *n_matches = counts[1];
  host.download(call, d, counts[1] < cap ? counts[1] : cap);
  return call.wait();
}

// the arguments of both tally_text forms
static int checkTallyText(const redgpu_dfa *dfa, int what, int style, const uint8_t *data,
                          uint64_t len, uint64_t nBins, const uint64_t *bins) {
  const bool lines = what == REDGPU_TALLY_LINES;
  return checkRawText(dfa, bins, "null bins buffer", data, len,
                      lines || what == REDGPU_TALLY_MATCHES
                          ? nullptr
                          : "what is neither REDGPU_TALLY_LINES nor REDGPU_TALLY_MATCHES",
                      lines ? &style : nullptr, nBins);
}

// raw text -> how many lines / matches report each result (k_tally_text.h): everything on
// `stream`, nothing read back
int redgpu_tally_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                          const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                          int accumulate, uint64_t *n_lines, uint64_t *n_items, uint64_t *bins,
                          void *stream) {
  if (int rc = checkTallyText(dfa, what, style, data, len, n_bins, bins)) return rc;
  // REDGPU_TALLY_PLAIN=1: an atomic per item, no ballot and no peel (measurements)
  const char *env = getenv("REDGPU_TALLY_PLAIN");
  const int plain = env && env[0] == '1';
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, tallyTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchTallyText(dfa->im->dev, what, style, do_leader ? 1 : 0, data, len, delim, n_bins,
                           accumulate ? 1 : 0, plain, n_lines, n_items, bins, scratch, cfg, s, name);
  });
}

// host-buffer form: one upload of the text, device bins of the call's own, then the two counts
// and the n_bins + 1 slots back - added to the caller's on the host under accumulate
int redgpu_tally_text(const redgpu_dfa *dfa, int what, int style, int do_leader,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                      int accumulate, uint64_t *n_lines, uint64_t *n_items, uint64_t *bins) {
  if (int rc = checkTallyText(dfa, what, style, data, len, n_bins, bins)) return rc;
  std::vector<uint64_t> got;
  if (accumulate) {
    try {
      got.resize(size_t(n_bins + 1));
    } catch (const std::bad_alloc &) {
      return fail(REDGPU_ELIMIT, "out of host memory");
    }
  }
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 2, "counts");
  uint64_t *dBins = call.buf<uint64_t>(kSlAux1, n_bins + 1, "bins");
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_tally_text_dev(dfa, what, style, do_leader, dData, len, delim, n_bins, 0, dN,
                                 dN + 1, dBins, call.stream());
  });
  uint64_t counts[2] = {0, 0};
  call.download(counts, dN, 2, "counts");
  // (nothing of the caller's is written before the last copy has arrived)
  if (accumulate) call.download(got.data(), dBins, n_bins + 1, "bins");
  if (int rc = call.wait()) return rc;
  if (!accumulate) {
    call.download(bins, dBins, n_bins + 1, "bins");
    if (int rc = call.wait()) return rc;
  } else {
    for (uint64_t i = 0; i <= n_bins; ++i) bins[i] += got[size_t(i)];
  }
  if (n_lines) *n_lines = counts[0];
  if (n_items) *n_items = counts[1];
  return REDGPU_OK;
}

uint32_t redgpu_tally_lds_bins(const redgpu_dfa *dfa) {
  if (!dfa) return 0;
  const DfaImage &img = dfa->im->img;
  return tallyLdsBins(img.tableKind, (img.primaryBytes + 15u) & ~15u, img.nStates);
}

// the arguments of both sum_text forms
static int checkSumText(const redgpu_dfa *dfa, int which, const uint8_t *data, uint64_t len,
                        uint64_t nBins, const uint64_t *stats) {
  return checkRawText(dfa, stats, "null stats buffer", data, len,
                      which == REDGPU_SUM_FIRST || which == REDGPU_SUM_LAST
                          ? nullptr
                          : "which is neither REDGPU_SUM_FIRST nor REDGPU_SUM_LAST",
                      nullptr, nBins);
}

// raw text -> per result the count, sum, min and max of the numbers in the matches
// (k_sum_text.h): everything on `stream`, nothing read back
int redgpu_sum_text_dev(const redgpu_dfa *dfa, int which, const uint8_t *data, uint64_t len,
                        uint8_t delim, uint64_t max_per_line, uint64_t n_bins, int accumulate,
                        uint64_t *n_lines, uint64_t *n_items, uint64_t *n_numeric, uint64_t *stats,
                        void *stream) {
  if (int rc = checkSumText(dfa, which, data, len, n_bins, stats)) return rc;
  // REDGPU_SUM_PLAIN=1: four atomics per item, no carried run and no peel (measurements)
  const char *env = getenv("REDGPU_SUM_PLAIN");
  const int plain = env && env[0] == '1';
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, sumTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchSumText(dfa->im->dev, which, data, len, delim, max_per_line, n_bins,
                         accumulate ? 1 : 0, plain, n_lines, n_items, n_numeric, stats, scratch, cfg,
                         s, name);
  });
}

// host-buffer form: one upload of the text, device stats of the call's own, then the three
// scalars and the 4 x (n_bins + 1) words back - merged into the caller's on the host under
// accumulate
int redgpu_sum_text(const redgpu_dfa *dfa, int which, const uint8_t *data, uint64_t len,
                    uint8_t delim, uint64_t max_per_line, uint64_t n_bins, int accumulate,
                    uint64_t *n_lines, uint64_t *n_items, uint64_t *n_numeric, uint64_t *stats) {
  if (int rc = checkSumText(dfa, which, data, len, n_bins, stats)) return rc;
  const uint64_t slots = n_bins + 1, words = 4 * slots;
  std::vector<uint64_t> got;
  if (accumulate) {
    try {
      got.resize(size_t(words));
    } catch (const std::bad_alloc &) {
      return fail(REDGPU_ELIMIT, "out of host memory");
    }
  }
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 3, "counts");
  uint64_t *dStats = call.buf<uint64_t>(kSlAux1, words, "stats");
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_sum_text_dev(dfa, which, dData, len, delim, max_per_line, n_bins, 0, dN, dN + 1,
                               dN + 2, dStats, call.stream());
  });
  uint64_t counts[3] = {0, 0, 0};
  call.download(counts, dN, 3, "counts");
  // (nothing of the caller's is written before the last copy has arrived)
  if (accumulate) call.download(got.data(), dStats, words, "stats");
  if (int rc = call.wait()) return rc;
  if (!accumulate) {
    call.download(stats, dStats, words, "stats");
    if (int rc = call.wait()) return rc;
  } else {
    for (uint64_t i = 0; i < slots; ++i) {
      stats[i] += got[size_t(i)];
      stats[slots + i] += got[size_t(slots + i)];
      uint64_t &lo = stats[2 * slots + i], &hi = stats[3 * slots + i];
      if (got[size_t(2 * slots + i)] < lo) lo = got[size_t(2 * slots + i)];
      if (got[size_t(3 * slots + i)] > hi) hi = got[size_t(3 * slots + i)];
    }
  }
  if (n_lines) *n_lines = counts[0];
  if (n_items) *n_items = counts[1];
  if (n_numeric) *n_numeric = counts[2];
  return REDGPU_OK;
}

uint32_t redgpu_sum_lds_bins(const redgpu_dfa *dfa) {
  if (!dfa) return 0;
  const DfaImage &img = dfa->im->img;
  return sumLdsBins(img.tableKind, (img.primaryBytes + 15u) & ~15u, img.nStates);
}

// the arguments of both replace_text forms
static int checkReplaceText(const redgpu_dfa *dfa, int style, const uint8_t *data, uint64_t len,
                            const uint8_t *repl, uint64_t replLen, const uint64_t *outLen) {
  return checkRawText(dfa, outLen, "null out_len buffer", data, len,
                      replLen && !repl ? "null replacement" : nullptr, &style);
}

// raw text -> every line rewritten, the text put back together (k_replace_text.h): everything on
// `stream`, nothing read back; phases as launchReplaceText's
static int replaceTextDev(const redgpu_dfa *dfa, int style, int doLeader, int onlyChanged,
                          const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                          uint64_t replLen, uint64_t maxCount, uint64_t *nLines,
                          uint64_t *nReplaced, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                          int phases, hipStream_t s) {
  if (int rc = checkReplaceText(dfa, style, data, len, repl, replLen, outLen)) return rc;
  return rawTextDev(dfa, s, replaceTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchReplaceText(dfa->im->dev, style, doLeader ? 1 : 0, onlyChanged ? 1 : 0, data, len,
                             delim, repl, replLen, maxCount, nLines, nReplaced, outLen, out, outCap,
                             phases, scratch, cfg, s, name);
  });
}

int redgpu_replace_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int only_changed,
                            const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                            uint64_t repl_len, uint64_t max_count, uint64_t *n_lines,
                            uint64_t *n_replaced, uint64_t *out_len, uint8_t *out, uint64_t out_cap,
                            void *stream) {
  return replaceTextDev(dfa, style, do_leader, only_changed, data, len, delim, repl, repl_len,
                        max_count, n_lines, n_replaced, out_len, out, out_cap, 3,
                        static_cast<hipStream_t>(stream));
}

// host-buffer form: the text and repl go up once, then textOutHost; phase 1 leaves the sizes, the
// bitmaps and the chunks' output bases in the stream's scratch, phase 2 assembles the output
int redgpu_replace_text(const redgpu_dfa *dfa, int style, int do_leader, int only_changed,
                        const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                        uint64_t repl_len, uint64_t max_count, uint64_t *n_lines,
                        uint64_t *n_replaced, uint64_t *out_len, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkReplaceText(dfa, style, data, len, repl, repl_len, out_len)) return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint8_t *dRepl = call.buf<uint8_t>(kSlAux0, repl_len, "repl");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 3, "sizes");
  call.upload(dData, data, len, "data");
  call.upload(dRepl, repl, repl_len, "repl");
  uint64_t sizes[3] = {0, 0, 0};
  textOutHost(call, dSizes, sizes, 3, 2, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return replaceTextDev(dfa, style, do_leader, only_changed, dData, len, delim, dRepl, repl_len,
                          max_count, dSizes, dSizes + 1, dSizes + 2, dOut, room, phases,
                          call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_replaced) *n_replaced = sizes[1];
  *out_len = sizes[2];
  return REDGPU_OK;
}

// raw text -> the selected lines and their context, as a text (k_filter_text.h): everything on
// `stream`, nothing read back; phases as launchFilterText's
static int filterTextDev(const redgpu_dfa *dfa, int style, int doLeader, int invert,
                         uint64_t before, uint64_t after, uint64_t maxCount, const uint8_t *data,
                         uint64_t len, uint8_t delim, uint64_t *nLines, uint64_t *nSelected,
                         uint64_t *nEmitted, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                         int phases, hipStream_t s) {
  if (int rc = checkRawText(dfa, outLen, "null out_len buffer", data, len, nullptr, &style))
    return rc;
  return rawTextDev(dfa, s, filterTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchFilterText(dfa->im->dev, style, doLeader ? 1 : 0, invert ? 1 : 0, before, after,
                            maxCount, data, len, delim, nLines, nSelected, nEmitted, outLen, out,
                            outCap, phases, scratch, cfg, s, name);
  });
}

int redgpu_filter_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                           uint64_t before, uint64_t after, uint64_t max_count,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *n_lines,
                           uint64_t *n_selected, uint64_t *n_emitted, uint64_t *out_len,
                           uint8_t *out, uint64_t out_cap, void *stream) {
  return filterTextDev(dfa, style, do_leader, invert, before, after, max_count, data, len, delim,
                       n_lines, n_selected, n_emitted, out_len, out, out_cap, 3,
                       static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the bitmaps
// and the chunks' output bases in the stream's scratch, phase 2 copies the runs
int redgpu_filter_text(const redgpu_dfa *dfa, int style, int do_leader, int invert, uint64_t before,
                       uint64_t after, uint64_t max_count, const uint8_t *data, uint64_t len,
                       uint8_t delim, uint64_t *n_lines, uint64_t *n_selected, uint64_t *n_emitted,
                       uint64_t *out_len, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkRawText(dfa, out_len, "null out_len buffer", data, len, nullptr, &style))
    return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 4, "sizes");
  call.upload(dData, data, len, "data");
  uint64_t sizes[4] = {0, 0, 0, 0};
  textOutHost(call, dSizes, sizes, 4, 3, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return filterTextDev(dfa, style, do_leader, invert, before, after, max_count, dData, len, delim,
                         dSizes, dSizes + 1, dSizes + 2, dSizes + 3, dOut, room, phases,
                         call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_selected) *n_selected = sizes[1];
  if (n_emitted) *n_emitted = sizes[2];
  *out_len = sizes[3];
  return REDGPU_OK;
}

// the arguments of both route_text forms
static int checkRouteText(const redgpu_dfa *dfa, int style, const uint8_t *data, uint64_t len,
                          uint64_t nBins, const uint64_t *binOffsets, const uint64_t *outLen) {
  if (dfa && !binOffsets) return fail(REDGPU_EAPI, "null bin_offsets buffer");
  return checkRawText(dfa, outLen, "null out_len buffer", data, len, nullptr, &style, nBins, 255);
}

// raw text -> its lines grouped by result, as a text (k_route_text.h): everything on `stream`,
// nothing read back; phases as launchRouteText's
static int routeTextDev(const redgpu_dfa *dfa, int style, int doLeader, int dropUnmatched,
                        const uint8_t *data, uint64_t len, uint8_t delim, uint64_t nBins,
                        uint64_t *nLines, uint64_t *nRouted, uint64_t *binLines,
                        uint64_t *binOffsets, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                        int phases, hipStream_t s) {
  if (int rc = checkRouteText(dfa, style, data, len, nBins, binOffsets, outLen)) return rc;
  return rawTextDev(dfa, s, routeTextScratchBytes(len, nBins, dropUnmatched ? 1 : 0),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchRouteText(dfa->im->dev, style, doLeader ? 1 : 0, dropUnmatched ? 1 : 0, data, len,
                           delim, nBins, nLines, nRouted, binLines, binOffsets, outLen, out, outCap,
                           phases, scratch, cfg, s, name);
  });
}

int redgpu_route_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int drop_unmatched,
                          const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                          uint64_t *n_lines, uint64_t *n_routed, uint64_t *bin_lines,
                          uint64_t *bin_offsets, uint64_t *out_len, uint8_t *out, uint64_t out_cap,
                          void *stream) {
  return routeTextDev(dfa, style, do_leader, drop_unmatched, data, len, delim, n_bins, n_lines,
                      n_routed, bin_lines, bin_offsets, out_len, out, out_cap, 3,
                      static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the bitmaps
// and the (bucket, chunk) output bases in the stream's scratch, phase 2 copies the runs
int redgpu_route_text(const redgpu_dfa *dfa, int style, int do_leader, int drop_unmatched,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                      uint64_t *n_lines, uint64_t *n_routed, uint64_t *bin_lines,
                      uint64_t *bin_offsets, uint64_t *out_len, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkRouteText(dfa, style, data, len, n_bins, bin_offsets, out_len)) return rc;
  // the three counts, bin_lines[n_bins + 1], bin_offsets[n_bins + 2]
  const uint64_t nSizes = 3 + (n_bins + 1) + (n_bins + 2);
  uint64_t sizes[3 + 256 + 257] = {};
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, nSizes, "sizes");
  uint64_t *dLines = dSizes + 3, *dOffsets = dLines + n_bins + 1;
  call.upload(dData, data, len, "data");
  textOutHost(call, dSizes, sizes, nSizes, 2, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return routeTextDev(dfa, style, do_leader, drop_unmatched, dData, len, delim, n_bins, dSizes,
                        dSizes + 1, dLines, dOffsets, dSizes + 2, dOut, room, phases,
                        call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_routed) *n_routed = sizes[1];
  *out_len = sizes[2];
  for (uint64_t i = 0; i <= n_bins && bin_lines; ++i) bin_lines[i] = sizes[3 + i];
  for (uint64_t i = 0; i <= n_bins + 1; ++i) bin_offsets[i] = sizes[3 + n_bins + 1 + i];
  return REDGPU_OK;
}

// the arguments of both range_text forms
static int checkRangeText(const redgpu_dfa *dfa, int style, int32_t openResult,
                          int32_t closeResult, const uint8_t *data, uint64_t len,
                          const uint64_t *outLen) {
  const char *own = nullptr;
  if (openResult < 1) own = "open_result is less than 1";
  else if (closeResult < 1) own = "close_result is less than 1";
  return checkRawText(dfa, outLen, "null out_len buffer", data, len, own, &style);
}

// raw text -> the lines of its /open/,/close/ ranges, as a text, and a record per range
// (k_range_text.h): everything on `stream`, nothing read back; phases as launchRangeText's
static int rangeTextDev(const redgpu_dfa *dfa, int style, int doLeader, int32_t openResult,
                        int32_t closeResult, int emitOpen, int emitClose, int invert,
                        uint64_t maxRanges, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t *nLines, uint64_t *nRanges, uint64_t *nEmitted, uint64_t *outLen,
                        uint8_t *out, uint64_t outCap, uint64_t recCap, uint64_t *firstLine,
                        uint64_t *lastLine, uint64_t *begin, uint64_t *end, int phases,
                        hipStream_t s) {
  if (int rc = checkRangeText(dfa, style, openResult, closeResult, data, len, outLen)) return rc;
  return rawTextDev(dfa, s, rangeTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchRangeText(dfa->im->dev, style, doLeader ? 1 : 0, openResult, closeResult,
                           emitOpen ? 1 : 0, emitClose ? 1 : 0, invert ? 1 : 0, maxRanges, data, len,
                           delim, nLines, nRanges, nEmitted, outLen, out, outCap, recCap, firstLine,
                           lastLine, begin, end, phases, scratch, cfg, s, name);
  });
}

int redgpu_range_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int32_t open_result,
                          int32_t close_result, int emit_open, int emit_close, int invert,
                          uint64_t max_ranges, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t *n_lines, uint64_t *n_ranges, uint64_t *n_emitted,
                          uint64_t *out_len, uint8_t *out, uint64_t out_cap, uint64_t rec_cap,
                          uint64_t *first_line, uint64_t *last_line, uint64_t *begin,
                          uint64_t *end, void *stream) {
  return rangeTextDev(dfa, style, do_leader, open_result, close_result, emit_open, emit_close,
                      invert, max_ranges, data, len, delim, n_lines, n_ranges, n_emitted, out_len,
                      out, out_cap, rec_cap, first_line, last_line, begin, end, 3,
                      static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the bitmaps,
// the chunks' output bases and the records on the device, phase 2 copies the runs (and reads no
// record argument), and the records that exist come back behind the output
int redgpu_range_text(const redgpu_dfa *dfa, int style, int do_leader, int32_t open_result,
                      int32_t close_result, int emit_open, int emit_close, int invert,
                      uint64_t max_ranges, const uint8_t *data, uint64_t len, uint8_t delim,
                      uint64_t *n_lines, uint64_t *n_ranges, uint64_t *n_emitted, uint64_t *out_len,
                      uint8_t *out, uint64_t out_cap, uint64_t rec_cap, uint64_t *first_line,
                      uint64_t *last_line, uint64_t *begin, uint64_t *end) {
  if (int rc = checkRangeText(dfa, style, open_result, close_result, data, len, out_len)) return rc;
  // no more ranges than lines, nor lines than bytes
  if (rec_cap > len) rec_cap = len;
  if (rec_cap > max_ranges) rec_cap = max_ranges;
  uint64_t *host[4] = {first_line, last_line, begin, end};
  if (!first_line && !last_line && !begin && !end) rec_cap = 0;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 4, "sizes");
  uint64_t *dRec = rec_cap ? call.buf<uint64_t>(kSlAux0, 4 * rec_cap, "records") : nullptr;
  uint64_t *dev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4 && dRec; ++i)
    if (host[i]) dev[i] = dRec + uint64_t(i) * rec_cap;
  call.upload(dData, data, len, "data");
  uint64_t sizes[4] = {0, 0, 0, 0};
  textOutHost(call, dSizes, sizes, 4, 3, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return rangeTextDev(dfa, style, do_leader, open_result, close_result, emit_open, emit_close,
                        invert, max_ranges, dData, len, delim, dSizes, dSizes + 1, dSizes + 2,
                        dSizes + 3, dOut, room, rec_cap, dev[0], dev[1], dev[2], dev[3], phases,
                        call.stream());
  });
  const uint64_t got = sizes[1] < rec_cap ? sizes[1] : rec_cap;
  for (int i = 0; i < 4 && got; ++i)
    if (dev[i]) call.download(host[i], dev[i], got, "records");
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_ranges) *n_ranges = sizes[1];
  if (n_emitted) *n_emitted = sizes[2];
  *out_len = sizes[3];
  return REDGPU_OK;
}

// the arguments of both uniq_text forms (every output may be NULL: the handle stands in for the
// buffer checkRawText asks for)
static int checkUniqText(const redgpu_dfa *dfa, int what, int style, const uint8_t *data,
                         uint64_t len, uint64_t tableSlots) {
  const bool lines = what == REDGPU_UNIQ_LINES;
  const char *own = nullptr;
  if (!lines && what != REDGPU_UNIQ_MATCHES)
    own = "what is neither REDGPU_UNIQ_LINES nor REDGPU_UNIQ_MATCHES";
  else if (tableSlots < 64 || tableSlots > (1ull << 32) || (tableSlots & (tableSlots - 1)))
    own = "table_slots is no power of two in [64, 2^32]";
  // (a key packs offset + 1 above a 24-bit length: texts of 2^40 - 1 bytes and more are refused)
  return checkRawText(dfa, dfa, "", data, len, own, lines ? &style : nullptr, 0, 1ull << 31,
                      (1ull << 40) - 1);
}

// raw text -> its distinct matches (or selected lines) counted by their bytes (k_uniq_text.h):
// everything on `stream`, nothing read back
int redgpu_uniq_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                         const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_per_line,
                         uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_items,
                         uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *first,
                         uint64_t *length, uint64_t *count, void *stream) {
  if (int rc = checkUniqText(dfa, what, style, data, len, table_slots)) return rc;
  // REDGPU_UNIQ_PLAIN=1: no LDS front, every item goes to the global table (measurements, DESIGN
  // 4.3m)
  const char *env = getenv("REDGPU_UNIQ_PLAIN");
  const int plain = env && env[0] == '1';
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, uniqTextScratchBytes(len, table_slots),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchUniqText(dfa->im->dev, what, style, do_leader ? 1 : 0, data, len, delim,
                          max_per_line, table_slots, cap, plain, n_lines, n_items, n_distinct,
                          n_dropped, first, length, count, scratch, cfg, s, name);
  });
}

// host-buffer form: one upload of the text, the table in the stream's scratch, device records of
// the call's own, then the four counts and the records that exist back
int redgpu_uniq_text(const redgpu_dfa *dfa, int what, int style, int do_leader,
                     const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_per_line,
                     uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_items,
                     uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *first, uint64_t *length,
                     uint64_t *count) {
  if (int rc = checkUniqText(dfa, what, style, data, len, table_slots)) return rc;
  // no more records than slots, nor than bytes: an item has a byte of its own (a line its
  // delimiter, a match at least the byte it ends behind)
  if (cap > table_slots) cap = table_slots;
  if (cap > len) cap = len;
  if (!first && !length && !count) cap = 0;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 4, "counts");
  uint64_t *dFirst = first && cap ? call.buf<uint64_t>(kSlAux1, cap, "first") : nullptr;
  uint64_t *dLength = length && cap ? call.buf<uint64_t>(kSlAux2, cap, "length") : nullptr;
  uint64_t *dCount = count && cap ? call.buf<uint64_t>(kSlAux3, cap, "count") : nullptr;
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_uniq_text_dev(dfa, what, style, do_leader, dData, len, delim, max_per_line,
                                table_slots, cap, dN, dN + 1, dN + 2, dN + 3, dFirst, dLength,
                                dCount, call.stream());
  });
  uint64_t counts[4] = {0, 0, 0, 0};
  call.download(counts, dN, 4, "counts");
  if (int rc = call.wait()) return rc;
  const uint64_t put = counts[2] < cap ? counts[2] : cap;
  if (dFirst && put) call.download(first, dFirst, put, "first");
  if (dLength && put) call.download(length, dLength, put, "length");
  if (dCount && put) call.download(count, dCount, put, "count");
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = counts[0];
  if (n_items) *n_items = counts[1];
  if (n_distinct) *n_distinct = counts[2];
  if (n_dropped) *n_dropped = counts[3];
  return REDGPU_OK;
}

uint32_t redgpu_uniq_lds_slots(const redgpu_dfa *dfa) {
  if (!dfa) return 0;
  const DfaImage &img = dfa->im->img;
  return uniqLdsSlots(img.tableKind, (img.primaryBytes + 15u) & ~15u, img.nStates);
}

// the arguments of both dedup_text forms
static int checkDedupText(const redgpu_dfa *dfa, int what, int style, uint64_t keyIndex,
                          const uint8_t *data, uint64_t len, uint64_t tableSlots,
                          const uint64_t *outLen) {
  const bool indexed = what == REDGPU_DEDUP_MATCH || what == REDGPU_DEDUP_FIELD;
  const char *own = nullptr;
  if (what < REDGPU_DEDUP_WHOLE || what > REDGPU_DEDUP_FIELD)
    own = "what is none of REDGPU_DEDUP_WHOLE, _LINES, _MATCH, _FIELD";
  else if (indexed && keyIndex == 0)
    own = "key_index is 0";
  else if (tableSlots < 64 || tableSlots > (1ull << 32) || (tableSlots & (tableSlots - 1)))
    own = "table_slots is no power of two in [64, 2^32]";
  // (a key packs offset + 1 above a 24-bit length, as uniq_text's)
  return checkRawText(dfa, outLen, "null out_len buffer", data, len, own,
                      what == REDGPU_DEDUP_LINES ? &style : nullptr, 0, 1ull << 31,
                      (1ull << 40) - 1);
}

// raw text -> the lines chosen by their keys' strings, as a text (k_dedup_text.h): everything on
// `stream`, nothing read back; phases as launchDedupText's
static int dedupTextDev(const redgpu_dfa *dfa, int what, int style, int doLeader,
                        uint64_t keyIndex, uint64_t minCount, uint64_t maxCount, int invert,
                        int keepUnkeyed, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t tableSlots, uint64_t *nLines, uint64_t *nKeyed,
                        uint64_t *nDistinct, uint64_t *nDropped, uint64_t *nEmitted,
                        uint64_t *outLen, uint8_t *out, uint64_t outCap, int phases,
                        hipStream_t s) {
  if (int rc = checkDedupText(dfa, what, style, keyIndex, data, len, tableSlots, outLen)) return rc;
  // REDGPU_UNIQ_PLAIN=1: no LDS front, as uniq_text's (measurements)
  const char *env = getenv("REDGPU_UNIQ_PLAIN");
  const int plain = env && env[0] == '1';
  return rawTextDev(dfa, s, dedupTextScratchBytes(len, tableSlots),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchDedupText(dfa->im->dev, what, style, doLeader ? 1 : 0, keyIndex, minCount,
                           maxCount, invert ? 1 : 0, keepUnkeyed ? 1 : 0, data, len, delim,
                           tableSlots, plain, nLines, nKeyed, nDistinct, nDropped, nEmitted, outLen,
                           out, outCap, phases, scratch, cfg, s, name);
  });
}

int redgpu_dedup_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                          uint64_t key_index, uint64_t min_count, uint64_t max_count, int invert,
                          int keep_unkeyed, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t table_slots, uint64_t *n_lines, uint64_t *n_keyed,
                          uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *n_emitted,
                          uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream) {
  return dedupTextDev(dfa, what, style, do_leader, key_index, min_count, max_count, invert,
                      keep_unkeyed, data, len, delim, table_slots, n_lines, n_keyed, n_distinct,
                      n_dropped, n_emitted, out_len, out, out_cap, 3,
                      static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the table,
// the bitmaps and the chunks' output bases in the stream's scratch, phase 2 copies the runs
int redgpu_dedup_text(const redgpu_dfa *dfa, int what, int style, int do_leader, uint64_t key_index,
                      uint64_t min_count, uint64_t max_count, int invert, int keep_unkeyed,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t table_slots,
                      uint64_t *n_lines, uint64_t *n_keyed, uint64_t *n_distinct,
                      uint64_t *n_dropped, uint64_t *n_emitted, uint64_t *out_len, uint8_t *out,
                      uint64_t out_cap) {
  if (int rc = checkDedupText(dfa, what, style, key_index, data, len, table_slots, out_len))
    return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 6, "sizes");
  call.upload(dData, data, len, "data");
  uint64_t sizes[6] = {0, 0, 0, 0, 0, 0};
  textOutHost(call, dSizes, sizes, 6, 5, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return dedupTextDev(dfa, what, style, do_leader, key_index, min_count, max_count, invert,
                        keep_unkeyed, dData, len, delim, table_slots, dSizes, dSizes + 1,
                        dSizes + 2, dSizes + 3, dSizes + 4, dSizes + 5, dOut, room, phases,
                        call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_keyed) *n_keyed = sizes[1];
  if (n_distinct) *n_distinct = sizes[2];
  if (n_dropped) *n_dropped = sizes[3];
  if (n_emitted) *n_emitted = sizes[4];
  *out_len = sizes[5];
  return REDGPU_OK;
}

// the arguments of both group_text forms (every output may be NULL: the handle stands in for the
// buffer checkRawText asks for)
static int checkGroupText(const redgpu_dfa *dfa, int what, uint64_t keyIndex, int which,
                          const uint8_t *data, uint64_t len, uint64_t tableSlots) {
  const char *own = nullptr;
  if (what != REDGPU_GROUP_MATCH && what != REDGPU_GROUP_FIELD)
    own = "what is neither REDGPU_GROUP_MATCH nor REDGPU_GROUP_FIELD";
  else if (which != REDGPU_SUM_FIRST && which != REDGPU_SUM_LAST)
    own = "which is neither REDGPU_SUM_FIRST nor REDGPU_SUM_LAST";
  else if (keyIndex == 0)
    own = "key_index is 0";
  else if (tableSlots < 64 || tableSlots > (1ull << 32) || (tableSlots & (tableSlots - 1)))
    own = "table_slots is no power of two in [64, 2^32]";
  // (a key packs offset + 1 above a 24-bit length, as uniq_text's)
  return checkRawText(dfa, dfa, "", data, len, own, nullptr, 0, 1ull << 31, (1ull << 40) - 1);
}

// raw text -> one record per distinct key string with the statistics of its lines' numbers
// (k_group_text.h): everything on `stream`, nothing read back
int redgpu_group_text_dev(const redgpu_dfa *dfa, int what, uint64_t key_index, uint64_t value_index,
                          int which, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_keyed,
                          uint64_t *n_numeric, uint64_t *n_distinct, uint64_t *n_dropped,
                          uint64_t *first, uint64_t *length, uint64_t *count, uint64_t *stats,
                          void *stream) {
  if (int rc = checkGroupText(dfa, what, key_index, which, data, len, table_slots)) return rc;
  // REDGPU_UNIQ_PLAIN=1: no LDS front, as uniq_text's (measurements)
  const char *env = getenv("REDGPU_UNIQ_PLAIN");
  const int plain = env && env[0] == '1';
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rawTextDev(dfa, s, groupTextScratchBytes(len, table_slots),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchGroupText(dfa->im->dev, what, key_index, value_index, which, data, len, delim,
                           table_slots, cap, plain, n_lines, n_keyed, n_numeric, n_distinct,
                           n_dropped, first, length, count, stats, scratch, cfg, s, name);
  });
}

// host-buffer form: one upload of the text, the table in the stream's scratch, device records of
// the call's own (seven words a record, the four rows of stats at the device cap's stride), then
// the five scalars and the records that exist back - stats row by row, at the caller's stride
int redgpu_group_text(const redgpu_dfa *dfa, int what, uint64_t key_index, uint64_t value_index,
                      int which, const uint8_t *data, uint64_t len, uint8_t delim,
                      uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_keyed,
                      uint64_t *n_numeric, uint64_t *n_distinct, uint64_t *n_dropped,
                      uint64_t *first, uint64_t *length, uint64_t *count, uint64_t *stats) {
  if (int rc = checkGroupText(dfa, what, key_index, which, data, len, table_slots)) return rc;
  // no more records than slots, nor than lines, nor lines than bytes
  uint64_t devCap = cap;
  if (devCap > table_slots) devCap = table_slots;
  if (devCap > len) devCap = len;
  if (!first && !length && !count && !stats) devCap = 0;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 5, "counts");
  uint64_t *dFirst = first && devCap ? call.buf<uint64_t>(kSlAux1, devCap, "first") : nullptr;
  uint64_t *dLength = length && devCap ? call.buf<uint64_t>(kSlAux2, devCap, "length") : nullptr;
  uint64_t *dCount = count && devCap ? call.buf<uint64_t>(kSlAux3, devCap, "count") : nullptr;
  uint64_t *dStats = stats && devCap ? call.buf<uint64_t>(kSlOff, 4 * devCap, "stats") : nullptr;
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_group_text_dev(dfa, what, key_index, value_index, which, dData, len, delim,
                                 table_slots, devCap, dN, dN + 1, dN + 2, dN + 3, dN + 4, dFirst,
                                 dLength, dCount, dStats, call.stream());
  });
  uint64_t counts[5] = {0, 0, 0, 0, 0};
  call.download(counts, dN, 5, "counts");
  if (int rc = call.wait()) return rc;
  const uint64_t put = counts[3] < devCap ? counts[3] : devCap;
  if (dFirst && put) call.download(first, dFirst, put, "first");
  if (dLength && put) call.download(length, dLength, put, "length");
  if (dCount && put) call.download(count, dCount, put, "count");
  for (uint64_t row = 0; row < 4 && dStats && put; ++row)
    call.download(stats + row * cap, dStats + row * devCap, put, "stats");
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = counts[0];
  if (n_keyed) *n_keyed = counts[1];
  if (n_numeric) *n_numeric = counts[2];
  if (n_distinct) *n_distinct = counts[3];
  if (n_dropped) *n_dropped = counts[4];
  return REDGPU_OK;
}

uint32_t redgpu_group_lds_slots(const redgpu_dfa *dfa) {
  if (!dfa) return 0;
  const DfaImage &img = dfa->im->img;
  return groupLdsSlots(img.tableKind, (img.primaryBytes + 15u) & ~15u, img.nStates);
}

// raw text -> every match of every line as bytes, one per output line (k_extract_text.h):
// everything on `stream`, nothing read back; phases as launchExtractText's
static int extractTextDev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t maxPerLine, uint64_t *nLines, uint64_t *nMatches,
                          uint64_t *outLen, uint8_t *out, uint64_t outCap, int phases,
                          hipStream_t s) {
  if (int rc = checkRawText(dfa, outLen, "null out_len buffer", data, len, nullptr, nullptr))
    return rc;
  // REDGPU_XT_HAND=n: pieces of n bytes or more go to the whole wave (measurements, DESIGN 4.3k;
  // unset or 0 = the kernel's default)
  const char *env = getenv("REDGPU_XT_HAND");
  const uint32_t hand = env ? uint32_t(strtoul(env, nullptr, 10)) : 0u;
  return rawTextDev(dfa, s, extractTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchExtractText(dfa->im->dev, data, len, delim, maxPerLine, hand, nLines, nMatches,
                             outLen, out, outCap, phases, scratch, cfg, s, name);
  });
}

int redgpu_extract_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t max_per_line, uint64_t *n_lines, uint64_t *n_matches,
                            uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream) {
  return extractTextDev(dfa, data, len, delim, max_per_line, n_lines, n_matches, out_len, out,
                        out_cap, 3, static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the bitmaps
// and the chunks' output bases in the stream's scratch, phase 2 assembles the pieces
int redgpu_extract_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t max_per_line, uint64_t *n_lines, uint64_t *n_matches,
                        uint64_t *out_len, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkRawText(dfa, out_len, "null out_len buffer", data, len, nullptr, nullptr))
    return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 3, "sizes");
  call.upload(dData, data, len, "data");
  uint64_t sizes[3] = {0, 0, 0};
  textOutHost(call, dSizes, sizes, 3, 2, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return extractTextDev(dfa, dData, len, delim, max_per_line, dSizes, dSizes + 1, dSizes + 2,
                          dOut, room, phases, call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_matches) *n_matches = sizes[1];
  *out_len = sizes[2];
  return REDGPU_OK;
}

// the arguments of both fields_text forms
static int checkFieldsText(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                           uint64_t select, uint32_t sepLen, const uint64_t *outLen) {
  const char *own = nullptr;
  if (select == 0) own = "select is 0: no field is selected";
  else if (sepLen > 8) own = "sep_len is above 8";
  return checkRawText(dfa, outLen, "null out_len buffer", data, len, own, nullptr);
}

// raw text -> the selected fields of every line, joined by sep, one line per output line
// (k_fields_text.h): everything on `stream`, nothing read back; phases as launchFieldsText's
static int fieldsTextDev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                         uint64_t select, uint64_t maxFields, int onlyDelimited, uint64_t sep,
                         uint32_t sepLen, uint64_t *nLines, uint64_t *nEmitted, uint64_t *nFields,
                         uint64_t *outLen, uint8_t *out, uint64_t outCap, int phases,
                         hipStream_t s) {
  if (int rc = checkFieldsText(dfa, data, len, select, sepLen, outLen)) return rc;
  return rawTextDev(dfa, s, fieldsTextScratchBytes(len),
                    [&](void *scratch, const LaunchCfg &cfg, const char **name) {
    return launchFieldsText(dfa->im->dev, data, len, delim, select, maxFields, onlyDelimited, sep,
                            sepLen, nLines, nEmitted, nFields, outLen, out, outCap, phases,
                            scratch, cfg, s, name);
  });
}

int redgpu_fields_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t select, uint64_t max_fields, int only_delimited, uint64_t sep,
                           uint32_t sep_len, uint64_t *n_lines, uint64_t *n_emitted,
                           uint64_t *n_fields, uint64_t *out_len, uint8_t *out, uint64_t out_cap,
                           void *stream) {
  return fieldsTextDev(dfa, data, len, delim, select, max_fields, only_delimited, sep, sep_len,
                       n_lines, n_emitted, n_fields, out_len, out, out_cap, 3,
                       static_cast<hipStream_t>(stream));
}

// host-buffer form: the text goes up once, then textOutHost; phase 1 leaves the sizes, the bitmaps
// and the chunks' output bases in the stream's scratch, phase 2 assembles the lines
int redgpu_fields_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                       uint64_t select, uint64_t max_fields, int only_delimited, uint64_t sep,
                       uint32_t sep_len, uint64_t *n_lines, uint64_t *n_emitted,
                       uint64_t *n_fields, uint64_t *out_len, uint8_t *out, uint64_t out_cap) {
  if (int rc = checkFieldsText(dfa, data, len, select, sep_len, out_len)) return rc;
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dSizes = call.buf<uint64_t>(kSlAux1, 4, "sizes");
  call.upload(dData, data, len, "data");
  uint64_t sizes[4] = {0, 0, 0, 0};
  textOutHost(call, dSizes, sizes, 4, 3, out, out_cap,
              [&](uint8_t *dOut, uint64_t room, int phases) {
    return fieldsTextDev(dfa, dData, len, delim, select, max_fields, only_delimited, sep, sep_len,
                         dSizes, dSizes + 1, dSizes + 2, dSizes + 3, dOut, room, phases,
                         call.stream());
  });
  if (int rc = call.wait()) return rc;
  if (n_lines) *n_lines = sizes[0];
  if (n_emitted) *n_emitted = sizes[1];
  if (n_fields) *n_fields = sizes[2];
  *out_len = sizes[3];
  return REDGPU_OK;
}

int redgpu_split_lines(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                       uint64_t *offsets, uint64_t cap, uint64_t *n_lines) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!offsets || !n_lines) return fail(REDGPU_EAPI, "null output buffer");
  if (len && !data) return fail(REDGPU_EAPI, "null data buffer");
  HostCall call(dfa, len);
  uint8_t *dData = call.buf<uint8_t>(kSlData, len, "data");
  uint64_t *dN = call.buf<uint64_t>(kSlAux0, 1, "count");
  // count first (room for no line at all), then size the device offsets to what will be kept
  uint64_t *dOff = call.buf<uint64_t>(kSlOff, 1, "offsets");
  call.upload(dData, data, len, "data");
  call.run([&] {
    return redgpu_split_lines_dev(dfa, dData, len, delim, dOff, 0, dN, call.stream());
  });
  call.download(n_lines, dN, 1, "count");
  if (int rc = call.wait()) return rc;
  const uint64_t got = *n_lines < cap ? *n_lines : cap;
  if (got) {
    dOff = call.buf<uint64_t>(kSlOff, got + 1, "offsets");
    call.run([&] {
      return redgpu_split_lines_dev(dfa, dData, len, delim, dOff, got, dN, call.stream());
    });
  }
  call.download(offsets, dOff, got + 1, "offsets");
  return call.wait();
}

int redgpu_diag_read_dev(const redgpu_dfa *dfa, const void *data, uint64_t bytes, uint32_t *sink,
                         void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!data || !sink) return fail(REDGPU_EAPI, "null buffer");
  if (reinterpret_cast<uintptr_t>(data) % 16) return fail(REDGPU_EAPI, "buffer not 16-byte aligned");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipError_t e = launchDiagRead(data, bytes, sink, dfa->numCUs, static_cast<hipStream_t>(stream));
  tlsKernel = "k_diag_read";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_diag_lines_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t n_lines,
                          uint64_t line_bytes, int32_t *result, uint64_t *start, uint64_t *end,
                          uint32_t *sink, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (line_bytes != 64 && (line_bytes % 128 || line_bytes == 0 || line_bytes >= (1ull << 31)))
    return fail(REDGPU_EAPI, "line_bytes must be 64 or a multiple of 128");
  if (!data || !sink || (line_bytes == 64 && (!result || !start || !end)))
    return fail(REDGPU_EAPI, "null buffer");
  if (reinterpret_cast<uintptr_t>(data) % 16) return fail(REDGPU_EAPI, "buffer not 16-byte aligned");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipError_t e = launchDiagLines(data, n_lines, uint32_t(line_bytes), result, start, end, sink,
                                 dfa->numCUs, static_cast<hipStream_t>(stream));
  tlsKernel = "k_diag_lines";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_diag_lds_dev(const redgpu_dfa *dfa, uint32_t rounds, uint32_t *sink, uint64_t *lookups,
                        void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!sink) return fail(REDGPU_EAPI, "null buffer");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipError_t e = launchDiagLds(dfa->im->dev, rounds, sink, dfa->numCUs,
                               static_cast<hipStream_t>(stream), lookups);
  tlsKernel = "k_diag_lds";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_diag_l2_dev(const redgpu_dfa *dfa, const uint16_t *table, uint32_t rounds, uint32_t *sink,
                       uint64_t *lookups, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (!table || !sink) return fail(REDGPU_EAPI, "null buffer");
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  hipError_t e = launchDiagL2(table, rounds, sink, dfa->numCUs, static_cast<hipStream_t>(stream),
                              lookups);
  tlsKernel = "k_diag_l2";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_diag_walked_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t *walked,
                           void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!walked) return fail(REDGPU_EAPI, "null buffer");
  if (int rc = checkBatch(data, offsets, stride, n, kTrailingLimit)) return rc;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  Batch b{data, offsets, stride, n, nullptr, nullptr, nullptr};
  LaunchCfg cfg{dfa->numCUs, 0};
  hipError_t e = launchWalked(dfa->im->dev, b, do_leader ? 1 : 0,
                              reinterpret_cast<unsigned long long *>(walked), cfg,
                              static_cast<hipStream_t>(stream));
  tlsKernel = "k_walked";
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_host_register(void *ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(REDGPU_EAPI, "null buffer");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) return failHip(e, "hipHostRegister");
  return REDGPU_OK;
}

int redgpu_host_unregister(void *ptr) {
  if (!ptr) return fail(REDGPU_EAPI, "null buffer");
  hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) return failHip(e, "hipHostUnregister");
  return REDGPU_OK;
}

void redgpu_thread_release(void) { hostStageReleaseThread(); }

void redgpu_host_route_counts(uint64_t counts[4]) { if (counts) hostRouteCounts(counts); }

uint64_t redgpu_scratch_entries(void) { return scratchEntries(); }

uint64_t redgpu_host_pins_held(void) { return hostStageHeld(); }

int redgpu_dfa_tune_dev(redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                        uint64_t stride, uint64_t n, void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (int rc = checkBatch(data, offsets, stride, n, 0)) return rc;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  // a fused u8 table in LDS (<= 256 states) already takes the streaming kernels
  if (dfa->im->img.tableKind == REDGPU_TAB_LDS_FUSED_U8) return REDGPU_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t nStates = dfa->im->img.nStates;
  uint32_t *dHist = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dHist), size_t(nStates) * 4), "hipMalloc histogram");
  auto done = [&](int rc) { (void)hipFree(dHist); return rc; };
  hipError_t e = hipMemsetAsync(dHist, 0, size_t(nStates) * 4, s);
  if (e != hipSuccess) return done(failHip(e, "hipMemsetAsync"));
  Batch b{data, offsets, stride, n, nullptr, nullptr, nullptr};
  LaunchCfg cfg{dfa->numCUs, 0};
  e = launchVisits(dfa->im->dev, b, dHist, cfg, s);
  tlsKernel = "k_visits";
  if (e != hipSuccess) return done(failHip(e, "kernel launch"));
  std::vector<uint32_t> hist(nStates);
  e = hipMemcpyAsync(hist.data(), dHist, size_t(nStates) * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return done(failHip(e, "histogram copy"));
  (void)hipFree(dHist);
  dHist = nullptr;

  // device index -> blob state id, then the same builder with the observed visits
  std::vector<double> measured(dfa->im->img.statesTotal, 0.0);
  for (uint32_t i = 0; i < nStates; ++i) measured[dfa->im->img.rawOf[i]] = double(hist[i]);
  DfaImage img;
  int code = REDGPU_OK;
  std::string err = buildImage(dfa->im->blob.data(), dfa->im->blob.size(), dfa->ldsTableMax,
                               (dfa->flags & REDGPU_F_FORCE_GLOBAL) != 0, img, code,
                               (dfa->flags & REDGPU_F_FORCE_HOT) != 0, &measured);
  if (!err.empty()) return fail(code, err);
  // all work queued on the device so far may still read the old tables
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return failHip(e, "hipDeviceSynchronize");
  // copy on tune: other handles that share the image keep the one they were created with
  auto im = std::make_shared<SharedImage>();
  im->blob = dfa->im->blob;
  im->img = std::move(img);
  im->device = dfa->im->device;
  im->buildFlags = dfa->im->buildFlags;
  im->ldsTableMax = dfa->im->ldsTableMax;
  if (int rc = uploadImage(im.get())) return rc;
  dfa->im = std::move(im);
  return REDGPU_OK;
}

int redgpu_dfa_tune(redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets, uint64_t stride,
                    uint64_t n) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  uint64_t total = 0;
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit, &total)) return rc;
  HostCall call(dfa, total);
  uint8_t *dData = call.buf<uint8_t>(kSlData, total, "data");
  uint64_t *dOff = offsets ? call.buf<uint64_t>(kSlOff, n + 1, "offsets") : nullptr;
  if (offsets) call.upload(dOff, offsets, n + 1, "offsets");
  call.upload(dData, data, total, "data");
  // tune_dev returns early for a fused u8 table, with the uploads still in flight: like every
  // host form, drain the stream and release the call's registrations on every path
  call.run([&] { return redgpu_dfa_tune_dev(dfa, dData, dOff, stride, n, call.stream()); });
  return call.wait();
}

int redgpu_advance_batch_dev(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                             uint64_t stride, uint64_t n, uint32_t *state, int32_t *result,
                             void *stream) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!state) return fail(REDGPU_EAPI, "null state buffer");
  if (!result) return fail(REDGPU_EAPI, "null result buffer");
  if (int rc = checkBatch(data, offsets, stride, n, 0)) return rc;
  DeviceScope scope(dfa->im->device);
  if (scope.err != hipSuccess) return failHip(scope.err, "hipSetDevice");
  Batch b{data, offsets, stride, n, result, nullptr, nullptr};
  LaunchCfg cfg{dfa->numCUs, (dfa->flags & REDGPU_F_FORCE_GENERIC) ? 1 : 0};
  const char *name = "";
  hipError_t e = launchAdvance(dfa->im->dev, b, state, cfg, static_cast<hipStream_t>(stream), &name);
  tlsKernel = name;
  if (e != hipSuccess) return failHip(e, "kernel launch");
  return REDGPU_OK;
}

int redgpu_advance_batch(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                         uint64_t stride, uint64_t n, uint32_t *state, int32_t *result) {
  if (int rc = checkHandle(dfa)) return rc;
  if (n == 0) return REDGPU_OK;
  if (!state) return fail(REDGPU_EAPI, "null state buffer");
  if (!result) return fail(REDGPU_EAPI, "null result buffer");
  uint64_t total = 0;
  if (int rc = checkBatch(data, offsets, stride, n, kStrideLimit, &total)) return rc;
  HostCall call(dfa, total);
  uint8_t *dData = call.buf<uint8_t>(kSlData, total, "data");
  uint32_t *dState = call.buf<uint32_t>(kSlAux0, n, "state");
  int32_t *dRes = call.buf<int32_t>(kSlRes, n, "result");
  uint64_t *dOff = offsets ? call.buf<uint64_t>(kSlOff, n + 1, "offsets") : nullptr;
  if (offsets) call.upload(dOff, offsets, n + 1, "offsets");
  call.upload(dData, data, total, "data");
  call.upload(dState, state, n, "state");
  call.run([&] {
    return redgpu_advance_batch_dev(dfa, dData, dOff, stride, n, dState, dRes, call.stream());
  });
  call.download(state, dState, n, "state back");
  call.download(result, dRes, n, "result");
  return call.wait();
}

int redgpu_check_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n,
                           int32_t *result, void *stream) {
  return runDev(dfa, kCheck, style, do_leader, data, offsets, stride, n, result, nullptr,
                nullptr, static_cast<hipStream_t>(stream));
}

int redgpu_match_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n,
                           int32_t *result, uint64_t *start, uint64_t *end, void *stream) {
  return runDev(dfa, kMatch, style, do_leader, data, offsets, stride, n, result, start, end,
                static_cast<hipStream_t>(stream));
}

int redgpu_check_batches_dev(const redgpu_dfa *dfa, int style, int do_leader,
                             const redgpu_batch *batches, uint32_t n_batches, void *stream) {
  return runDevMany(dfa, kCheck, style, do_leader, batches, n_batches,
                    static_cast<hipStream_t>(stream));
}

int redgpu_match_batches_dev(const redgpu_dfa *dfa, int style, int do_leader,
                             const redgpu_batch *batches, uint32_t n_batches, void *stream) {
  return runDevMany(dfa, kMatch, style, do_leader, batches, n_batches,
                    static_cast<hipStream_t>(stream));
}

int redgpu_scan_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                          void *stream) {
  return runDev(dfa, kScan, style, do_leader, data, offsets, stride, n, result, nullptr,
                nullptr, static_cast<hipStream_t>(stream));
}

} // extern "C"
