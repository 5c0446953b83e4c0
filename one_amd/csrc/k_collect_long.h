// k_collect_long.h - Red::collect (lib/Red.cpp:103-116) over ONE long text, across the chip
// (included by kernels.hip inside its namespace, after k_long.h).
//
// collect is a chain: p0 = 0, m_k = the first position >= p_k whose anchored attempt
// (searchCore's inner loop, include/Matcher.h:557-640, <styLast, false>) matches, p_{k+1} = the
// end of that match.  The text is cut into chunks [lo, hi) of C bytes; a chunk owns the attempts
// at the positions inside it.  From an entry q it runs the chain until the next attempt position
// reaches hi (exit hi), a match ends at e >= hi (exit e), or a suffix-closed attempt reaches the
// end of the text without a match (exit n: nothing later can match).  Its records and its exit
// are a function of q alone, so with q_0 = 0 and q_{j+1} = exit_j(q_j) the concatenated records
// are exactly Red::collect's.  The steps, all queued on the caller's stream:
//   k_cl_walk    every chunk at once from a GUESSED entry: the chain run over the kClWarm bytes
//                in front of the chunk (search chains resynchronise within a match or two);
//   rounds       k_cl_resolve queues every chunk whose entry is not its predecessor's exit (as
//                it stands), k_cl_rewalk walks them again from it and stops where the new chain
//                hits a record start of the old one - the old records from there on are kept;
//                kClRounds rounds at most, each a no-op once one queued nothing;
//   k_cl_check / k_cl_serial  the first chunk still open, and one lane that walks on from it
//                in order, unbounded (the chains that never resynchronise: "aa" on a run of a);
//   fold         k_long.h's scan kernels, an exclusive scan of the per-chunk counts (the total
//                is the call's count), and k_cl_scatter, a wave per chunk, up to `cap` records.
// Speculative walks are bounded: a chunk walks at most `budget` bytes of attempts past their
// first byte (an attempt that never dies would otherwise make every chunk walk to the end of
// the text); a chunk that runs out is left open (exit kClOpen) for the serial finish.
// Record slots: C per chunk (a chunk holds at most C attempts), result i32 + attempt position u32
// (chunk-relative) + start u64 + end u64 = 24 bytes per slot, so ~24 bytes of scratch per text
// byte.  (A record's start is the attempt's last "left the initial state", Matcher.h:582-587:
// two attempts can report the same one, so chains are compared by attempt position.)
// The same chain serves replaceCore over one text (k_replace_long.h): every kernel here takes a
// MODE - kClCollect is the above, kClReplace swaps the attempt for replaceCore's (LongAttempt: style
// and leader test) and keeps lean slots (attempt position + end, 12 bytes; res and rst unused).
#pragma once

constexpr int kClRounds = 4;
constexpr uint32_t kClWarm = 64;
constexpr uint64_t kClOpen = ~0ull;  // exit not known (the budget ran out)
constexpr uint64_t kClMinText = 16384;  // automatic chunking: shorter texts stay on one lane
constexpr uint64_t kClMinChunk = 256;   // ... and chunks of at least 4 x the warm-up

// chunk bytes: forced, or enough chunks for every lane of the chip (2048 per CU), rounded up to
// 64 bytes, at least kClMinChunk
inline uint64_t collectLongChunk(uint64_t n, uint32_t chunkBytes, const LaunchCfg &cfg) {
  if (chunkBytes) return chunkBytes;
  const uint64_t lanes = uint64_t(cfg.numCUs > 0 ? cfg.numCUs : 1) * 2048;
  const uint64_t c = ((n + lanes - 1) / lanes + 63) & ~uint64_t(63);
  return c < kClMinChunk ? kClMinChunk : c;
}

struct ClBufs {
  uint64_t *ent, *exit;  // [m] entry the records were computed from / exit
  uint32_t *cnt, *work;  // [m] records, re-walk queue
  uint32_t *ctl;         // [kClRounds] queued per round, [kClRounds] first open chunk
  uint64_t *off;         // [m] block-exclusive scan of cnt
  uint64_t *blockOff;    // [nb] block totals, then their exclusive scan
  int32_t *res;          // [m * slots]
  uint32_t *rat;         // [m * slots] attempt position - chunk begin
  uint64_t *rst, *ren;   // [m * slots] start, end
  uint64_t slots, m;
  uint32_t chunk;
};

// MODE of the chain kernels: whose attempt runs at a position, and what a record slot keeps
constexpr int kClCollect = 0;  // k_collect's attempt (searchCore <styLast, false>); result, at, start, end
constexpr int kClReplace = 1;  // replaceCore's (k_replace_long.h): LongAttempt's style and leader; at, end

// The chain over the attempt positions [q, hi) of p[0, n): k_long.h's longChain from where the
// match before ended.  emit(result, at, start, end) per match, false = stop here (the return value
// is then meaningless).  Returns the exit, or kClOpen when the attempts walked more than `budget`
// bytes past their first one.  The attempt is k_collect's, or (kClReplace) replaceCore's under
// a.style with the leader test; result and start are then 0 and the attempt position.
template <int MODE = kClCollect, class T, class E>
__device__ __forceinline__ uint64_t clChain(const T &tab, const LaneCtx &c, const StartFilter &flt,
                                            const uint8_t *p, uint64_t n, uint64_t q, uint64_t hi,
                                            uint64_t budget, E &&emit, const LongAttempt a = LongAttempt{}) {
  uint64_t pos = q;
  while (pos < hi) {
    const LongHit h = longChain<MODE == kClCollect, MODE == kClCollect>(tab, c, flt, p, n, pos, hi,
                                                                        budget, a);
    if (h.how == 0) return hi;
    if (h.how == 2) return n;
    if (h.how == 3) return kClOpen;
    if (!emit(MODE == kClReplace ? 0 : c.res[h.acc], h.at, h.ms, h.me)) return 0;
    pos = h.me;
  }
  return pos;
}

// chunk j walked again from entry q: phase 1 finds where the new chain meets a record start of
// the old one (only when the old walk finished: its exit is known), phase 2 moves the old tail
// behind the new head and writes the head.  Without a meeting point the new chain is the record.
template <int MODE = kClCollect, class T>
__device__ void clRewalk(const T &tab, const LaneCtx &c, const StartFilter &flt, const uint8_t *p,
                         uint64_t n, const ClBufs &b, uint64_t j, uint64_t q, uint64_t budget,
                         const LongAttempt a = LongAttempt{}) {
  const LongSpan sp = longSpan(j, b.chunk, n);
  const uint64_t lo = sp.lo, hi = sp.hi;
  const uint64_t base = j * b.slots;
  const uint32_t cnt0 = b.cnt[j];
  const uint64_t oldExit = b.exit[j];
  const bool conv = oldExit != kClOpen;
  uint32_t r = 0, k = 0;
  bool hit = false;
  const uint64_t ex = clChain<MODE>(tab, c, flt, p, n, q, hi, budget, [&](int32_t, uint64_t at, uint64_t, uint64_t) {
    if (conv) {
      const uint32_t rel = uint32_t(at - lo);
      while (k < cnt0 && b.rat[base + k] < rel) ++k;
      if (k < cnt0 && b.rat[base + k] == rel) { hit = true; return false; }
    }
    ++r;
    return true;
  }, a);
  if (!hit && ex == kClOpen) {
    b.exit[j] = kClOpen;
    b.cnt[j] = 0;
    return;
  }
  if (hit) {
    const uint32_t tail = cnt0 - k;
    if (r < k) {
      for (uint32_t t = 0; t < tail; ++t) {
        if constexpr (MODE == kClCollect) {
          b.res[base + r + t] = b.res[base + k + t];
          b.rst[base + r + t] = b.rst[base + k + t];
        }
        b.rat[base + r + t] = b.rat[base + k + t];
        b.ren[base + r + t] = b.ren[base + k + t];
      }
    } else if (r > k) {
      for (uint32_t t = tail; t-- > 0;) {
        if constexpr (MODE == kClCollect) {
          b.res[base + r + t] = b.res[base + k + t];
          b.rst[base + r + t] = b.rst[base + k + t];
        }
        b.rat[base + r + t] = b.rat[base + k + t];
        b.ren[base + r + t] = b.ren[base + k + t];
      }
    }
    b.cnt[j] = r + tail;
  } else {
    b.cnt[j] = r;
    b.exit[j] = ex;
  }
  if (r == 0) return;
  uint32_t w = 0;
  (void)clChain<MODE>(tab, c, flt, p, n, q, hi, budget, [&](int32_t rv, uint64_t at, uint64_t s, uint64_t e) {
    if constexpr (MODE == kClCollect) {
      b.res[base + w] = rv;
      b.rst[base + w] = s;
    }
    b.rat[base + w] = uint32_t(at - lo);
    b.ren[base + w] = e;
    return ++w < r;
  }, a);
}

__global__ void __launch_bounds__(64) k_cl_init(ClBufs b) {
  if (threadIdx.x < uint32_t(kClRounds)) b.ctl[threadIdx.x] = 0;
  if (threadIdx.x == uint32_t(kClRounds)) b.ctl[kClRounds] = uint32_t(b.m);
}

// every chunk from its guessed entry (chunk 0 from 0, exactly)
template <int KIND, int kThreads, int MODE = kClCollect>
__global__ void __launch_bounds__(kThreads)
k_cl_walk(DevDfa d, const uint8_t *p, uint64_t n, ClBufs b, uint64_t budget, LongAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const StartFilter flt = longFilter(d);
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < b.m; j += step) {
    const LongSpan sp = longSpan(j, b.chunk, n);
    const uint64_t lo = sp.lo, hi = sp.hi;
    uint64_t q = 0;
    if (j) {
      q = clChain<MODE>(tab, c, flt, p, n, lo > kClWarm ? lo - kClWarm : 0, lo, budget,
                        [](int32_t, uint64_t, uint64_t, uint64_t) { return true; }, a);
      if (q == kClOpen) q = lo;
    }
    const uint64_t base = j * b.slots;
    uint32_t k = 0;
    const uint64_t ex = clChain<MODE>(tab, c, flt, p, n, q, hi, budget, [&](int32_t rv, uint64_t at, uint64_t s, uint64_t e) {
      if constexpr (MODE == kClCollect) {
        b.res[base + k] = rv;
        b.rst[base + k] = s;
      }
      b.rat[base + k] = uint32_t(at - lo);
      b.ren[base + k] = e;
      ++k;
      return true;
    }, a);
    b.ent[j] = q;
    b.exit[j] = ex;
    b.cnt[j] = ex == kClOpen ? 0u : k;
  }
}

// round r: queue every chunk whose entry is not its predecessor's (known) exit
__global__ void __launch_bounds__(256) k_cl_resolve(ClBufs b, int round) {
  if (round > 0 && b.ctl[round - 1] == 0) return;
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < b.m; j += step) {
    const uint64_t want = j ? b.exit[j - 1] : 0;
    if (want == kClOpen || b.ent[j] == want) continue;
    b.ent[j] = want;
    b.work[atomicAdd(&b.ctl[round], 1u)] = uint32_t(j);
  }
}

template <int KIND, int kThreads, int MODE = kClCollect>
__global__ void __launch_bounds__(kThreads)
k_cl_rewalk(DevDfa d, const uint8_t *p, uint64_t n, ClBufs b, int round, uint64_t budget,
            LongAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (b.ctl[round] == 0) return;  // uniform: nothing queued this round
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const StartFilter flt = longFilter(d);
  const uint32_t cnt = b.ctl[round];
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < cnt; i += step) {
    const uint32_t j = b.work[i];
    clRewalk<MODE>(tab, c, flt, p, n, b, j, b.ent[j], budget, a);
  }
}

// the first chunk whose record is not final: its exit is open, or its entry is not its
// predecessor's exit
__global__ void __launch_bounds__(256) k_cl_check(ClBufs b) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < b.m; j += step) {
    const uint64_t want = j ? b.exit[j - 1] : 0;
    if (b.exit[j] == kClOpen || (want != kClOpen && b.ent[j] != want))
      atomicMin(&b.ctl[kClRounds], uint32_t(j));
  }
}

// one lane, in order, from the first open chunk: every exit it reads is final
template <int KIND, int MODE = kClCollect>
__global__ void __launch_bounds__(64)
k_cl_serial(DevDfa d, const uint8_t *p, uint64_t n, ClBufs b, LongAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (b.ctl[kClRounds] >= b.m) return;  // uniform: everything is final
  const Tab<KIND> tab = stageTab<KIND, 64>(d, lds);
  const LaneCtx c = longCtx<KIND>(d, lds);
  const StartFilter flt = longFilter(d);
  if (threadIdx.x) return;
  for (uint64_t j = b.ctl[kClRounds]; j < b.m; ++j) {
    const uint64_t want = j ? b.exit[j - 1] : 0;
    if (b.ent[j] == want && b.exit[j] != kClOpen) continue;
    b.ent[j] = want;
    clRewalk<MODE>(tab, c, flt, p, n, b, j, want, kClOpen, a);
  }
}

// fold 3: a wave per chunk copies its records to their place in the caller's arrays (< cap)
__global__ void __launch_bounds__(256)
k_cl_scatter(ClBufs b, uint64_t cap, int32_t *result, uint64_t *start, uint64_t *end) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < b.m; j += waves) {
    const uint64_t at = b.blockOff[j / 1024] + b.off[j];
    if (at >= cap) continue;
    const uint32_t cnt = b.cnt[j];
    const uint64_t base = j * b.slots;
    for (uint32_t i = lane; i < cnt && at + i < cap; i += 64) {
      result[at + i] = b.res[base + i];
      if (start) start[at + i] = b.rst[base + i];
      if (end) end[at + i] = b.ren[base + i];
    }
  }
}

// the suffix-closed route (no pure dead state: every attempt runs to the end of the text, so
// the chain is ONE attempt, the match<styLast,false> of the whole text): count from its result
__global__ void __launch_bounds__(64) k_cl_closed(const int32_t *result, uint64_t *count) {
  if (threadIdx.x == 0) *count = result[0] > 0 ? 1u : 0u;
}

// the chain of every chunk, final: walk, rounds, check + serial finish, and the scan of the counts
template <int KIND, int MODE>
hipError_t launchClChain(const DevDfa &d, const uint8_t *p, uint64_t n, const ClBufs &b,
                         const LongAttempt a, uint64_t *count, const LaunchCfg &cfg,
                         hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const LongPlan g = longPlan<KIND>(d, b.m, b.chunk, cfg);
  hipError_t e = setLds(k_cl_walk<KIND, kThreads, MODE>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_cl_rewalk<KIND, kThreads, MODE>, g.ldsBytes);
  if (e == hipSuccess) e = setLds(k_cl_serial<KIND, MODE>, g.ldsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cl_init, dim3(1), dim3(64), 0, stream, b);
  hipLaunchKernelGGL((k_cl_walk<KIND, kThreads, MODE>), dim3(g.blocks), dim3(kThreads), g.ldsBytes,
                     stream, d, p, n, b, g.budget, a);
  for (int round = 0; round < kClRounds; ++round) {
    hipLaunchKernelGGL(k_cl_resolve, dim3(g.small), dim3(256), 0, stream, b, round);
    hipLaunchKernelGGL((k_cl_rewalk<KIND, kThreads, MODE>), dim3(g.blocks), dim3(kThreads),
                       g.ldsBytes, stream, d, p, n, b, round, g.budget, a);
  }
  hipLaunchKernelGGL(k_cl_check, dim3(g.small), dim3(256), 0, stream, b);
  hipLaunchKernelGGL((k_cl_serial<KIND, MODE>), dim3(1), dim3(64), g.ldsBytes, stream, d, p, n, b, a);
  // fold: the exclusive scan of the per-chunk counts; the total is the call's count
  const uint64_t nb = (b.m + 1023) / 1024;
  uint64_t *const none = nullptr;
  hipLaunchKernelGGL((k_long_scan1<false, uint32_t>), dim3(uint32_t(nb)), dim3(1024), 0, stream, b.m,
                     static_cast<const uint32_t *>(b.cnt), b.off, none, b.blockOff, none,
                     static_cast<const uint32_t *>(nullptr));
  hipLaunchKernelGGL(k_long_scan2<false>, dim3(1), dim3(1024), 0, stream, b.blockOff, none, nb,
                     static_cast<const uint32_t *>(nullptr), count);
  return hipGetLastError();
}

template <int KIND>
hipError_t launchCollectLongK(const DevDfa &d, const uint8_t *p, uint64_t n, const ClBufs &b,
                              uint64_t cap, uint64_t *count, int32_t *result, uint64_t *start,
                              uint64_t *end, const LaunchCfg &cfg, hipStream_t stream) {
  const hipError_t e = launchClChain<KIND, kClCollect>(d, p, n, b, LongAttempt{}, count, cfg, stream);
  if (e != hipSuccess) return e;
  if (cap) {
    uint64_t sb = (b.m + 3) / 4;
    if (sb > uint64_t(cfg.numCUs) * 16) sb = uint64_t(cfg.numCUs) * 16;
    hipLaunchKernelGGL(k_cl_scatter, dim3(uint32_t(sb)), dim3(256), 0, stream, b, cap, result, start,
                       end);
  }
  return hipGetLastError();
}
