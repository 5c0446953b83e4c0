// k_search_long.h - searchCore (include/Matcher.h:557-640) over ONE long text, across the chip
// (included by kernels.hip inside its namespace, after k_replace_long.h).
//
// searchCore returns the Outcome of the LOWEST position whose anchored attempt succeeds - the
// attempt (k_long.h: longChain) being its inner loop under the call's style, with the leader test
// (lookingAt) in front when asked for.  An attempt's Outcome depends on its position alone, so
// there is nothing to guess and nothing to walk again (k_collect_long.h's entries and rounds):
// the text is cut into chunks of C bytes, chunk j owns the attempt positions [j * C, (j + 1) *
// C), tries them in increasing order and stops at its first success.  All queued on the caller's
// stream:
//   k_sl_init    best = stop = first open chunk = "none", every chunk "untouched";
//   k_sl_walk    persistent waves; wave w of W takes the tickets w, w + W, w + 2 W, ... - a ticket
//                is 64 consecutive chunks, a chunk per lane - so at any time the chip works on
//                one window of W * 64 * C bytes that moves up the text.  A success stores its
//                record (result, start, end) in the chunk's slot and lowers `best` (u64, atomic
//                min) to the attempt position.  Every lane reads `best` before its chunk, and
//                again before every run of kSlPoll attempt positions of a long one (the load is
//                issued in front of the run it follows, so nobody waits for it): a chunk is
//                dropped, and no further ticket taken, once `best` is below the position that
//                would be tried next.  A match at x therefore costs about x plus one window, not
//                the text.  `stop` is the same for suffix-closed DFAs without the leader: a
//                failed attempt that read to the end of the text alive ends every later position
//                (what k_collect_long.h's chain calls exit n).
//                Attempts are bounded: a chunk walks at most `budget` bytes past the first bytes
//                of its attempts (16 x C + 1 KiB, k_long.h's longPlan) - "x", then y without
//                end, on every lane at once would otherwise pin the chip - and a chunk that runs
//                out leaves the position it had reached;
//   k_sl_check / k_sl_serial   the first chunk with an undecided position below best and stop,
//                and ONE lane that finishes from it in order, unbounded: every chunk below it is
//                decided, a decided chunk with a match ends the search, so does a success of its
//                own (k_collect_long.h's check and serial finish, over k_long.h's longChain).
//                The bound costs time, never the Outcome;
//   k_sl_finish  result, start and end from best and the winner's slot, or 0 / 0 / 0.
// Per chunk: one state word (u32: 0 = untouched, else 1 + the first undecided position relative to
// the chunk, C = all decided; bit 31 = that position is a match) and one record slot (i32 + 2 x
// u64), written by a match only: 24 bytes of scratch per chunk.
// What stays on one lane (route "k_search_long<one>", the batch kernels over a batch of one):
// short texts; DFAs without a pure dead state under styLast / styFull, whose failing attempts
// cannot end early; and suffix-closed DFAs without the leader, whose search IS one anchored walk
// (normalizeVerbStyle).  Making ONE anchored walk parallel - a closed DFA, or a single match of
// many megabytes - is not done here.
#pragma once

constexpr uint32_t kSlPoll = 256;            // attempt positions between two looks at best / stop
constexpr uint32_t kSlHit = 0x80000000u;     // state word: the position is a match
constexpr uint64_t kSlNone = ~0ull;
constexpr uint64_t kSlMinChunk = 16;         // automatic chunking: one 16-byte load per lane
constexpr uint64_t kSlWindows = 16;          // ... and this many windows per text where it allows

// chunk bytes: forced, or small enough that the text is kSlWindows windows of every lane of the
// chip (2048 per CU), rounded up to 16 bytes (there is no warm-up in front of a chunk to pay for,
// as in k_collect_long.h, and a wave's 64 chunks are one contiguous read)
inline uint64_t searchLongChunk(uint64_t n, uint32_t chunkBytes, const LaunchCfg &cfg) {
  if (chunkBytes) return chunkBytes;
  const uint64_t lanes = uint64_t(cfg.numCUs > 0 ? cfg.numCUs : 1) * 2048 * kSlWindows;
  const uint64_t c = ((n + lanes - 1) / lanes + 15) & ~uint64_t(15);
  return c < kSlMinChunk ? kSlMinChunk : c;
}

struct SlBufs {
  uint64_t *ctl;     // [0] best, [1] stop, [2] first open chunk, [3] an attempt ran (mark)
  uint32_t *state;   // [m]
  int32_t *res;      // [m] the chunk's match: result,
  uint64_t *rst, *ren;  // start, end
  uint64_t m;
  uint32_t chunk;
};

__device__ __forceinline__ uint64_t slLoad(const uint64_t *w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// with mark every position that passes the leader test must be seen: no start filter
__device__ __forceinline__ StartFilter slFilter(const DevDfa &d, int mark) {
  return mark ? StartFilter{0, 0, 0, 0, false} : longFilter(d);
}

__global__ void __launch_bounds__(256) k_sl_init(SlBufs b) {
  const uint64_t at = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (at < 3) b.ctl[at] = kSlNone;
  if (at == 3) b.ctl[3] = 0;
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = at; j < b.m; j += step) b.state[j] = 0;
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_sl_walk(DevDfa d, const uint8_t *p, uint64_t n, SlBufs b, uint64_t budget, LongAttempt a,
          int mark) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const StartFilter flt = slFilter(d, mark);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  uint64_t best = slLoad(b.ctl), stop = slLoad(b.ctl + 1);
  for (uint64_t t = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); t * 64 < b.m;
       t += waves) {
    const uint64_t first = t * 64 * b.chunk;
    if (first > best || first >= stop) break;  // nothing from this ticket on can be the Outcome
    const uint64_t j = t * 64 + lane;
    if (j >= b.m) break;
    const LongSpan sp = longSpan(j, b.chunk, n);
    const uint64_t lo = sp.lo, hi = sp.hi;
    uint64_t reach = lo, left = budget;
    bool hit = false;
    while (reach < hi && reach <= best && reach < stop) {
      // (asked for here, looked at behind the run)
      const uint64_t nowBest = slLoad(b.ctl), nowStop = slLoad(b.ctl + 1);
      const uint64_t sub = hi - reach > kSlPoll ? reach + kSlPoll : hi;
      const LongHit h = longChain<false, true>(tab, c, flt, p, n, reach, sub, left, a, mark,
                                                 b.ctl + 3);
      best = nowBest;
      stop = nowStop;
      reach = h.at;
      if (h.how == 0) continue;
      if (h.how == 1) {
        b.res[j] = c.res[h.acc];
        b.rst[j] = h.ms;
        b.ren[j] = h.me;
        hit = true;
        atomicMin(reinterpret_cast<unsigned long long *>(b.ctl), static_cast<unsigned long long>(h.at));
        if (h.at < best) best = h.at;
      } else if (h.how == 2) {
        atomicMin(reinterpret_cast<unsigned long long *>(b.ctl + 1), static_cast<unsigned long long>(h.at));
        if (h.at < stop) stop = h.at;
        reach = hi;
      }
      break;
    }
    b.state[j] = uint32_t(reach - lo + 1) | (hit ? kSlHit : 0u);
  }
}

// position from which chunk j is undecided (its end: all of it is decided); *hit: it is a match
__device__ __forceinline__ uint64_t slReach(const SlBufs &b, uint64_t j, bool *hit) {
  const uint32_t s = b.state[j];
  *hit = (s & kSlHit) != 0;
  return j * b.chunk + (s ? (s & ~kSlHit) - 1 : 0u);
}

// the first chunk that still has an undecided position below best and stop
__global__ void __launch_bounds__(256) k_sl_check(SlBufs b, uint64_t n) {
  const uint64_t lim = b.ctl[0] < b.ctl[1] ? b.ctl[0] : b.ctl[1];
  uint64_t jEnd = b.m;
  if (lim != kSlNone && lim / b.chunk + 1 < jEnd) jEnd = lim / b.chunk + 1;
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < jEnd; j += step) {
    bool hit;
    const uint64_t reach = slReach(b, j, &hit);
    if (!hit && reach < longSpan(j, b.chunk, n).hi && reach < lim)
      atomicMin(reinterpret_cast<unsigned long long *>(b.ctl + 2), static_cast<unsigned long long>(j));
  }
}

// one lane, in order, from the first open chunk, unbounded: every chunk below the one in hand is
// decided and has no match (the lane's wave steps over the decided chunks, 64 at a look)
template <int KIND>
__global__ void __launch_bounds__(64)
k_sl_serial(DevDfa d, const uint8_t *p, uint64_t n, SlBufs b, LongAttempt a, int mark) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (b.ctl[2] >= b.m) return;  // uniform: everything below best and stop is decided
  const Tab<KIND> tab = stageTab<KIND, 64>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const StartFilter flt = slFilter(d, mark);
  const uint64_t lim = b.ctl[0] < b.ctl[1] ? b.ctl[0] : b.ctl[1];
  uint64_t j = b.ctl[2];
  while (j < b.m && j * b.chunk < lim) {
    // the next chunk that is not decided to its end without a match: the wave looks at 64
    const uint64_t mine = j + threadIdx.x;
    bool open = false;
    if (mine < b.m) {
      bool hit;
      const uint64_t reach = slReach(b, mine, &hit);
      open = hit || reach < longSpan(mine, b.chunk, n).hi;
    }
    const unsigned long long mask = __ballot(open);
    if (!mask) { j += 64; continue; }
    j += uint64_t(__ffsll(mask)) - 1;
    int done = 1;
    if (threadIdx.x == 0) {
      bool hit;
      const uint64_t reach = slReach(b, j, &hit);
      // (a match here is best itself: no chunk below has one)
      if (!hit && reach < lim) {
        const uint64_t hi = longSpan(j, b.chunk, n).hi;
        uint64_t left = kClOpen;
        const LongHit h = longChain<false, true>(tab, c, flt, p, n, reach, hi, left, a, mark,
                                                 b.ctl + 3);
        if (h.how == 1) {
          b.res[j] = c.res[h.acc];
          b.rst[j] = h.ms;
          b.ren[j] = h.me;
          b.ctl[0] = h.at;
        }
        done = h.how != 0;  // (2: nothing at or behind h.at matches)
      }
    }
    if (__shfl(done, 0)) break;
    ++j;
  }
}

// the Outcome: the slot of best's chunk, or no match - 0 / 0 / 0, the result being the initial
// state's when no attempt ran at all (mark)
__global__ void __launch_bounds__(64)
k_sl_finish(SlBufs b, const int32_t *resTab, uint32_t init, int mark, int32_t *result,
            uint64_t *start, uint64_t *end) {
  if (threadIdx.x) return;
  const uint64_t best = b.ctl[0];
  int32_t r = 0;
  uint64_t s = 0, e = 0;
  if (best != kSlNone) {
    const uint64_t j = best / b.chunk;
    r = b.res[j];
    s = b.rst[j];
    e = b.ren[j];
  } else if (mark && !b.ctl[3]) {
    r = resTab[init];
  }
  *result = r;
  if (start) *start = r ? s : 0;
  if (end) *end = r ? e : 0;
}

template <int KIND>
hipError_t launchSearchLongK(const DevDfa &d, const uint8_t *p, uint64_t n, const SlBufs &b,
                             const LongAttempt a, int mark, int32_t *result, uint64_t *start,
                             uint64_t *end, const LaunchCfg &cfg, hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const LongPlan g = longPlan<KIND>(d, b.m, b.chunk, cfg);
  hipError_t e = setLds(k_sl_walk<KIND, kThreads>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_sl_serial<KIND>, g.ldsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sl_init, dim3(g.small), dim3(256), 0, stream, b);
  hipLaunchKernelGGL((k_sl_walk<KIND, kThreads>), dim3(g.blocks), dim3(kThreads), g.ldsBytes, stream,
                     d, p, n, b, g.budget, a, mark);
  hipLaunchKernelGGL(k_sl_check, dim3(g.small), dim3(256), 0, stream, b, n);
  hipLaunchKernelGGL((k_sl_serial<KIND>), dim3(1), dim3(64), g.ldsBytes, stream, d, p, n, b, a,
                     mark);
  hipLaunchKernelGGL(k_sl_finish, dim3(1), dim3(64), 0, stream, b, d.result, d.init, mark,
                     result, start, end);
  return hipGetLastError();
}
