// k_match_all_long.h - matchAllCore (include/Matcher.h:711-766; matchAll, lib/Matcher.cpp:97-102)
// over ONE long text, across the chip (included by kernels.hip inside its namespace, after
// k_collect_long.h).
//
// matchAll is one anchored walk s_i = next(s_{i-1}, T[i]) from the initial state, and all it
// reports is a function of that state sequence.  With r_i = result(s_i) (0 = not accepting):
//   a record OPENS at i when s_i accepts and r_i != r_{i-1} (r_{-1} = 0, :747-752, :757);
//   its result is r_i, its END the first j > i with r_j != r_i, or n (:747-748);
//   its START the last position <= i at which the walk left the initial state, or 0 (:726-731).
// (The stop at a pure dead end, :755-756, changes nothing when dead ends are absorbing - the only
// DFAs that come here.)  The text is cut into chunks [lo, hi) of C bytes, one per lane.  From its
// entry state q a chunk yields its exit state, the number of records it opens (its first position
// compares against result(q), chunk 0's against 0), 1 + the position of its last escape from the
// initial state (0 = none), and `head`, the number of leading positions whose result is
// result(q) - where the run that was open on entry ends.  The steps, all on the caller's stream:
//   k_ml_init    the leader test (one lookingAt, :333-345) and the control words;
//   k_ml_walk    every chunk at once from a GUESSED entry: the state after walking the kMlWarm
//                bytes in front of it from the initial state (chunk 0: the initial state, exact);
//   rounds       k_ml_resolve queues every chunk whose entry is not its predecessor's exit as it
//                stands, k_ml_rewalk walks those again; kMlRounds at most, each a no-op once one
//                queued nothing.  Exits are compared, so a re-walk that ends in the same exit
//                leaves its successor valid;
//   k_ml_check / k_ml_serial  the first chunk still inconsistent, and one lane that goes on from
//                it in text order, unbounded, skipping chunks whose entry already matches (the
//                DFAs whose guesses never converge);
//   fold         k_long.h's scan kernels: the exclusive sum of the counts (the total is the call's
//                count) and the exclusive prefix max of the escapes, over all chunks;
//   k_ml_emit    the chunks that open a record below `cap` walk once more from their resolved
//                entry and write their records in place; a record whose run goes on past its
//                chunk gets its end from the first later chunk the run does not fill (`head`), so
//                every end has exactly one writer however many chunks a run spans.
// A chunk walks exactly its own bytes, so there is no speculation budget, and nothing is kept per
// record or per text byte: 36 bytes of scratch per chunk.
#pragma once

constexpr int kMlRounds = 4;
constexpr uint32_t kMlWarm = 64;
constexpr int kMlOpen = kMlRounds;    // ctl: the first chunk still inconsistent
constexpr int kMlGo = kMlRounds + 1;  // ctl: 1 = the leader test passed (or there is none)
constexpr int kMlSerial = kMlRounds + 2;  // ctl: chunks the serial lane walked again
constexpr int kMlChunks = kMlRounds + 3;  // ctl: m (what redgpu_diag_match_all_long_dev hands out)
constexpr int kMlCtlWords = kMlRounds + 4;

struct MlBufs {
  uint32_t *ent, *exit;  // [m] entry state the values below were computed from / exit state
  uint32_t *cnt, *head;  // [m] records opened / leading positions with the entry's result
  uint32_t *work;        // [m] re-walk queue
  uint32_t *ctl;         // [kMlRounds] queued per round, [kMlOpen], [kMlGo], [kMlSerial], [kMlChunks]
  uint64_t *esc;         // [m] 1 + last escape position, 0 = none; after the scans: the
                         //     block-exclusive max of the chunks before
  uint64_t *off;         // [m] block-exclusive sum of cnt
  uint64_t *blockOff, *blockEsc;  // [nb] per 1024 chunks: totals, then their exclusive scans
  uint64_t m;
  uint32_t chunk;
};

struct MlChunk {
  uint32_t exit, cnt, head;
  uint64_t esc;
};

// the count-only pass of chunk [lo, hi) from entry state q (first = chunk 0: nothing before it)
template <class T>
__device__ __forceinline__ MlChunk mlCount(const T &tab, const LaneCtx &c, const uint8_t *p,
                                           uint64_t lo, uint64_t hi, uint32_t q, bool first) {
  const int32_t rq = first ? 0 : c.resultOf(q);
  uint32_t s = q, cnt = 0, head = 0;
  int32_t prev = rq;
  bool inHead = true;
  uint64_t esc = 0;
  walkBytes(p, lo, hi, [&](uint32_t byte, uint64_t i) -> bool {
    const uint32_t was = s;
    s = tab.next(s, byte);
    if (was == c.init && s != was) esc = i + 1;
    const bool acc = s >= c.firstAccept;
    const int32_t r = acc ? c.res[s] : 0;
    if (acc && r != prev) ++cnt;
    prev = r;
    if (inHead && r == rq) ++head;
    else inHead = false;
    return s >= c.nPureDead;  // absorbing: nothing opens, escapes or changes state past one
  });
  return MlChunk{s, cnt, head, esc};
}

template <class T>
__device__ __forceinline__ void mlStore(const T &tab, const LaneCtx &c, const uint8_t *p, uint64_t n,
                                        const MlBufs &b, uint64_t j, uint32_t q) {
  const LongSpan sp = longSpan(j, b.chunk, n);
  const MlChunk k = mlCount(tab, c, p, sp.lo, sp.hi, q, j == 0);
  b.exit[j] = k.exit;
  b.cnt[j] = k.cnt;
  b.head[j] = k.head;
  b.esc[j] = k.esc;
}

__global__ void __launch_bounds__(64)
k_ml_init(DevDfa d, const uint8_t *p, uint64_t n, MlBufs b, int lead) {
  if (threadIdx.x < uint32_t(kMlRounds)) b.ctl[threadIdx.x] = 0;
  if (threadIdx.x == uint32_t(kMlOpen)) b.ctl[kMlOpen] = uint32_t(b.m);
  if (threadIdx.x == uint32_t(kMlSerial)) b.ctl[kMlSerial] = 0;
  if (threadIdx.x == uint32_t(kMlChunks)) b.ctl[kMlChunks] = uint32_t(b.m);
  if (threadIdx.x == uint32_t(kMlGo)) {
    const LaneCtx c{d.equivLeader, d.equivLeader + 256, d.result, d.init, d.leaderNext, d.nPureDead,
                    d.firstAccept, d.leaderLen};
    b.ctl[kMlGo] = !lead || lookingAt(c, p, 0, n) ? 1u : 0u;
  }
}

// every chunk from its guessed entry (chunk 0 from the initial state, exactly)
template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_ml_walk(DevDfa d, const uint8_t *p, uint64_t n, MlBufs b) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (!b.ctl[kMlGo]) return;  // uniform: the leader test failed
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < b.m; j += step) {
    const uint64_t lo = j * b.chunk;
    uint32_t q = c.init;
    if (j)
      walkBytes(p, lo > kMlWarm ? lo - kMlWarm : 0, lo, [&](uint32_t byte, uint64_t) -> bool {
        q = tab.next(q, byte);
        return true;
      });
    b.ent[j] = q;
    mlStore(tab, c, p, n, b, j, q);
  }
}

// round r: queue every chunk whose entry is not its predecessor's exit
__global__ void __launch_bounds__(256) k_ml_resolve(MlBufs b, int round) {
  if (!b.ctl[kMlGo] || (round > 0 && b.ctl[round - 1] == 0)) return;
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x + 1; j < b.m; j += step) {
    const uint32_t want = b.exit[j - 1];
    if (b.ent[j] == want) continue;
    b.ent[j] = want;
    b.work[atomicAdd(&b.ctl[round], 1u)] = uint32_t(j);
  }
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_ml_rewalk(DevDfa d, const uint8_t *p, uint64_t n, MlBufs b, int round) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (!b.ctl[kMlGo] || b.ctl[round] == 0) return;  // uniform: nothing queued this round
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const uint32_t queued = b.ctl[round];
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < queued; i += step) {
    const uint32_t j = b.work[i];
    mlStore(tab, c, p, n, b, j, b.ent[j]);
  }
}

// the first chunk whose entry is not its predecessor's exit
__global__ void __launch_bounds__(256) k_ml_check(MlBufs b) {
  if (!b.ctl[kMlGo]) return;
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x + 1; j < b.m; j += step)
    if (b.ent[j] != b.exit[j - 1]) atomicMin(&b.ctl[kMlOpen], uint32_t(j));
}

// one lane, in text order, from the first inconsistent chunk: every exit it reads is final
template <int KIND>
__global__ void __launch_bounds__(64) k_ml_serial(DevDfa d, const uint8_t *p, uint64_t n, MlBufs b) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (!b.ctl[kMlGo] || b.ctl[kMlOpen] >= b.m) return;  // uniform: everything is final
  const Tab<KIND> tab = stageTab<KIND, 64>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  if (threadIdx.x) return;
  uint32_t walked = 0;
  for (uint64_t j = b.ctl[kMlOpen]; j < b.m; ++j) {
    const uint32_t want = b.exit[j - 1];  // (the first inconsistent chunk is never chunk 0)
    if (b.ent[j] == want) continue;
    b.ent[j] = want;
    mlStore(tab, c, p, n, b, j, want);
    ++walked;
  }
  b.ctl[kMlSerial] = walked;
}

// the records, in place.  Chunk j closes the run that was open on its entry (end[off - 1]) when
// the run ends inside it or it is the last chunk; then, when it opens records below cap, walks
// again: result and start where a record opens, its end where its run ends inside the chunk (n
// at the end of the last chunk).  The walk stops behind record cap - 1's end.
template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_ml_emit(DevDfa d, const uint8_t *p, uint64_t n, MlBufs b, uint64_t cap, int32_t *result,
          uint64_t *start, uint64_t *end) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (!b.ctl[kMlGo]) return;
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < b.m; j += step) {
    const uint64_t off = b.blockOff[j / 1024] + b.off[j];
    if (off > cap) continue;  // (record off - 1 is not kept either)
    const LongSpan sp = longSpan(j, b.chunk, n);
    const uint64_t lo = sp.lo, hi = sp.hi;
    const bool last = j + 1 == b.m;
    const uint32_t q = b.ent[j];
    const int32_t rq = j ? c.resultOf(q) : 0;
    if (rq > 0 && off > 0 && end) {
      const uint32_t head = b.head[j];
      if (head < hi - lo || last) end[off - 1] = lo + head;
    }
    if (b.cnt[j] == 0 || off >= cap) continue;
    const uint64_t before = b.blockEsc[j / 1024] > b.esc[j] ? b.blockEsc[j / 1024] : b.esc[j];
    uint32_t s = q;
    int32_t prev = rq;
    uint64_t k = off, esc = before;
    bool open = false;  // record k - 1 (< cap) was opened here and its run goes on
    walkBytes(p, lo, hi, [&](uint32_t byte, uint64_t i) -> bool {
      const uint32_t was = s;
      s = tab.next(s, byte);
      if (was == c.init && s != was) esc = i + 1;
      const bool acc = s >= c.firstAccept;
      const int32_t r = acc ? c.res[s] : 0;
      if (r != prev) {
        if (open) {
          if (end) end[k - 1] = i;
          open = false;
        }
        if (acc) {
          if (k < cap) {
            result[k] = r;
            if (start) start[k] = esc ? esc - 1 : 0;
            open = true;
          }
          ++k;
        }
        prev = r;
      }
      return open || (k < cap && s >= c.nPureDead);
    });
    if (open && last && end) end[k - 1] = n;
  }
}

template <int KIND>
hipError_t launchMatchAllLongK(const DevDfa &d, const uint8_t *p, uint64_t n, const MlBufs &b,
                               int lead, uint64_t cap, uint64_t *count, int32_t *result,
                               uint64_t *start, uint64_t *end, const LaunchCfg &cfg,
                               hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const LongPlan g = longPlan<KIND>(d, b.m, b.chunk, cfg);
  hipError_t e = setLds(k_ml_walk<KIND, kThreads>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_ml_rewalk<KIND, kThreads>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_ml_serial<KIND>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_ml_emit<KIND, kThreads>, g.ldsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ml_init, dim3(1), dim3(64), 0, stream, d, p, n, b, lead);
  hipLaunchKernelGGL((k_ml_walk<KIND, kThreads>), dim3(g.blocks), dim3(kThreads), g.ldsBytes, stream,
                     d, p, n, b);
  for (int round = 0; round < kMlRounds; ++round) {
    hipLaunchKernelGGL(k_ml_resolve, dim3(g.small), dim3(256), 0, stream, b, round);
    hipLaunchKernelGGL((k_ml_rewalk<KIND, kThreads>), dim3(g.blocks), dim3(kThreads), g.ldsBytes,
                       stream, d, p, n, b, round);
  }
  hipLaunchKernelGGL(k_ml_check, dim3(g.small), dim3(256), 0, stream, b);
  hipLaunchKernelGGL((k_ml_serial<KIND>), dim3(1), dim3(64), g.ldsBytes, stream, d, p, n, b);
  // fold: the exclusive sum of the counts and the exclusive max of the escapes, in place, shut
  // (*count = 0) when the leader test failed
  const uint64_t nb = (b.m + 1023) / 1024;
  const uint32_t *go = b.ctl + kMlGo;
  hipLaunchKernelGGL((k_long_scan1<true, uint32_t>), dim3(uint32_t(nb)), dim3(1024), 0, stream, b.m,
                     static_cast<const uint32_t *>(b.cnt), b.off, b.esc, b.blockOff, b.blockEsc, go);
  hipLaunchKernelGGL(k_long_scan2<true>, dim3(1), dim3(1024), 0, stream, b.blockOff, b.blockEsc, nb,
                     go, count);
  if (cap)
    hipLaunchKernelGGL((k_ml_emit<KIND, kThreads>), dim3(g.blocks), dim3(kThreads), g.ldsBytes,
                       stream, d, p, n, b, cap, result, start, end);
  return hipGetLastError();
}
