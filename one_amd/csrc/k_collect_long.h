// k_collect_long.h - Red::collect (lib/Red.cpp:103-116) over ONE long text, across the chip
// (included by kernels.hip inside its namespace, after k_lists.h).
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
//   fold         k_cl_scan1 / k_cl_scan2, an exclusive scan of the per-chunk counts (the total
//                is the call's count), and k_cl_scatter, a wave per chunk, up to `cap` records.
// Speculative walks are bounded: a chunk walks at most `budget` bytes of attempts past their
// first byte (an attempt that never dies would otherwise make every chunk walk to the end of
// the text); a chunk that runs out is left open (exit kClOpen) for the serial finish.
// Record slots: C per chunk (a chunk holds at most C attempts), result i32 + attempt position u32
// (chunk-relative) + start u64 + end u64 = 24 bytes per slot, so ~24 bytes of scratch per text
// byte.  (A record's start is the attempt's last "left the initial state", Matcher.h:582-587:
// two attempts can report the same one, so chains are compared by attempt position.)
// The same chain serves replaceCore over one text (k_replace_long.h): every kernel here takes a
// MODE - kClCollect is the above, kClReplace swaps the attempt for replaceCore's (ClAttempt: style
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
constexpr int kClReplace = 1;  // replaceCore's (k_replace_long.h): ClAttempt's style and leader; at, end

struct ClAttempt {
  int style = kStyLast;
  int lead = 0;
};

// The chain over the attempt positions [q, hi) of p[0, n).  emit(result, at, start, end) per match,
// false = stop here (the return value is then meaningless).  Returns the exit, or kClOpen when the
// attempts walked more than `budget` bytes past their first one.  The attempt is k_collect's, or
// (kClReplace) replaceCore's under a.style with the leader test: Instant stops at the first
// accept, First and Tangent at the first non-accept behind one (First also where the result
// changes), Full forgets its accept at every non-accept; result and start are then 0.
template <int MODE = kClCollect, class T, class E>
__device__ __forceinline__ uint64_t clChain(const T &tab, const LaneCtx &c, const StartFilter &flt,
                                            const uint8_t *p, uint64_t n, uint64_t q, uint64_t hi,
                                            uint64_t budget, E &&emit, const ClAttempt a = ClAttempt{}) {
  uint64_t pos = q;
  while (pos < hi) {
    int how = 0;  // 1 = a match, 2 = suffix-closed stop, 3 = out of budget
    uint32_t accS = 0;
    uint64_t mA = 0, mS = 0, mE = 0;
    walkBytesPeek(p, pos, hi, flt, [] {}, [&](uint32_t byte, uint64_t i, uint32_t nextByte) -> bool {
      uint32_t st = tab.next(c.init, byte);
      bool any = false;
      uint64_t ms = i, me = i;
      uint32_t aS = 0;
      if (st >= c.firstAccept) { aS = st; me = i + 1; any = true; }
      else if (st < c.nPureDead) return true;
      else if (nextByte != kNoPeek && tab.next(st, nextByte) < c.nPureDead) return true;
      int32_t prev = 0;  // (kClReplace, styFirst) the result of the accepts so far
      if constexpr (MODE == kClReplace) {
        if (a.lead && !lookingAt(c, p, i, n)) return true;
        if (any && a.style == kStyFirst) prev = c.res[st];
      }
      const uint64_t lim = n - i - 1 > budget ? i + 1 + budget : n;
      uint64_t at = i + 1;
      auto stepOne = [&](uint32_t b2, uint64_t q2) -> bool {
        const uint32_t was = st;
        st = tab.next(st, b2);
        at = q2 + 1;
        const bool acc = st >= c.firstAccept;
        if constexpr (MODE == kClReplace) {
          if (acc) {
            if (a.style == kStyFirst) {
              const int32_t r = c.res[st];
              if (prev && r != prev) return false;
              prev = r;
            }
            aS = st; me = q2 + 1; any = true;
            return a.style != kStyInstant;
          }
          if (a.style == kStyFull) any = false;
          else if (any && (a.style == kStyFirst || a.style == kStyTangent)) return false;
          return st >= c.nPureDead;
        } else {
          if (was == c.init && st != was) ms = q2;
          if (acc) { aS = st; me = q2 + 1; any = true; }
          return acc || st >= c.nPureDead;
        }
      };
      uint64_t q2 = i + 1;
      bool alive = !(MODE == kClReplace && any && a.style == kStyInstant);
      for (uint32_t k = 0; k < 6 && q2 < lim && alive; ++k, ++q2) alive = stepOne(uint32_t(p[q2]), q2);
      if (alive)
        walkBytes(p, q2, lim, [&](uint32_t b2, uint64_t q3) -> bool { return alive = stepOne(b2, q3); });
      budget -= at - i - 1;
      if (alive && lim < n) { how = 3; return false; }
      if (!any) {
        if (c.suffixClosed && alive && !(MODE == kClReplace && a.lead)) { how = 2; return false; }  // L = SIGMA* L
        return true;
      }
      how = 1; accS = aS; mA = i; mS = ms; mE = me;
      return false;
    });
    if (how == 0) return hi;
    if (how == 2) return n;
    if (how == 3) return kClOpen;
    if (!emit(MODE == kClReplace ? 0 : c.res[accS], mA, mS, mE)) return 0;
    pos = mE;
  }
  return pos;
}

// chunk j walked again from entry q: phase 1 finds where the new chain meets a record start of
// the old one (only when the old walk finished: its exit is known), phase 2 moves the old tail
// behind the new head and writes the head.  Without a meeting point the new chain is the record.
template <int MODE = kClCollect, class T>
__device__ void clRewalk(const T &tab, const LaneCtx &c, const StartFilter &flt, const uint8_t *p,
                         uint64_t n, const ClBufs &b, uint64_t j, uint64_t q, uint64_t budget,
                         const ClAttempt a = ClAttempt{}) {
  const uint64_t lo = j * b.chunk;
  const uint64_t hi = lo + b.chunk < n ? lo + b.chunk : n;
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

template <int KIND>
__device__ __forceinline__ LaneCtx clCtx(const DevDfa &d, uint8_t *lds) {
  LaneCtx c{lds, lds + 256, resOf<KIND>(d, lds), d.init, d.leaderNext, d.nPureDead, d.firstAccept,
            d.leaderLen};
  c.suffixClosed = d.suffixClosed;
  return c;
}

__device__ __forceinline__ StartFilter clFilter(const DevDfa &d) {
  return StartFilter{d.startFreeWord, d.startFreeCount <= 4 ? d.startFreeCount : 0u,
                     d.start2FreeWord, d.start2FreeCount <= 4 ? d.start2FreeCount : 0u, false};
}

__global__ void __launch_bounds__(64) k_cl_init(ClBufs b) {
  if (threadIdx.x < uint32_t(kClRounds)) b.ctl[threadIdx.x] = 0;
  if (threadIdx.x == uint32_t(kClRounds)) b.ctl[kClRounds] = uint32_t(b.m);
}

// every chunk from its guessed entry (chunk 0 from 0, exactly)
template <int KIND, int kThreads, int MODE = kClCollect>
__global__ void __launch_bounds__(kThreads)
k_cl_walk(DevDfa d, const uint8_t *p, uint64_t n, ClBufs b, uint64_t budget, ClAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = clCtx<KIND>(d, lds);
  const StartFilter flt = clFilter(d);
  const uint64_t step = uint64_t(gridDim.x) * kThreads;
  for (uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x; j < b.m; j += step) {
    const uint64_t lo = j * b.chunk;
    const uint64_t hi = lo + b.chunk < n ? lo + b.chunk : n;
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
            ClAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (b.ctl[round] == 0) return;  // uniform: nothing queued this round
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = clCtx<KIND>(d, lds);
  const StartFilter flt = clFilter(d);
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
k_cl_serial(DevDfa d, const uint8_t *p, uint64_t n, ClBufs b, ClAttempt a) {
  extern __shared__ __align__(16) uint8_t lds[];
  if (b.ctl[kClRounds] >= b.m) return;  // uniform: everything is final
  const Tab<KIND> tab = stageTab<KIND, 64>(d, lds);
  const LaneCtx c = clCtx<KIND>(d, lds);
  const StartFilter flt = clFilter(d);
  if (threadIdx.x) return;
  for (uint64_t j = b.ctl[kClRounds]; j < b.m; ++j) {
    const uint64_t want = j ? b.exit[j - 1] : 0;
    if (b.ent[j] == want && b.exit[j] != kClOpen) continue;
    b.ent[j] = want;
    clRewalk<MODE>(tab, c, flt, p, n, b, j, want, kClOpen, a);
  }
}

// fold 1: block-exclusive scan of the counts (1024 chunks per block), block totals behind
__global__ void __launch_bounds__(1024) k_cl_scan1(ClBufs b) {
  __shared__ uint64_t s[1024];
  const uint64_t j = uint64_t(blockIdx.x) * 1024 + threadIdx.x;
  const uint64_t v = j < b.m ? b.cnt[j] : 0;
  s[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const uint64_t add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  if (j < b.m) b.off[j] = s[threadIdx.x] - v;
  if (threadIdx.x == 1023) b.blockOff[blockIdx.x] = s[1023];
}

// fold 2: one workgroup, exclusive scan of the block totals in place; *count = the sum
__global__ void __launch_bounds__(1024) k_cl_scan2(ClBufs b, uint64_t nb, uint64_t *count) {
  __shared__ uint64_t s[1024];
  uint64_t carry = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += 1024) {
    const uint64_t i = t0 + threadIdx.x;
    const uint64_t v = i < nb ? b.blockOff[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
      const uint64_t add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nb) b.blockOff[i] = carry + s[threadIdx.x] - v;
    carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
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
                         const ClAttempt a, uint64_t *count, const LaunchCfg &cfg,
                         hipStream_t stream) {
  constexpr bool kLds = Tab<KIND>::kInLds || KIND == REDGPU_TAB_HOT_ROWS;
  constexpr int kThreads = kLds ? 1024 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_cl_walk<KIND, kThreads, MODE>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_cl_rewalk<KIND, kThreads, MODE>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_cl_serial<KIND, MODE>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint64_t perCu = kLds ? (ldsBytes <= 80 * 1024 ? 2 : 1) : 8;
  uint64_t blocks = (b.m + kThreads - 1) / kThreads;
  if (blocks > uint64_t(cfg.numCUs) * perCu) blocks = uint64_t(cfg.numCUs) * perCu;
  if (blocks == 0) blocks = 1;
  uint64_t small = (b.m + 255) / 256;
  if (small > uint64_t(cfg.numCUs) * 8) small = uint64_t(cfg.numCUs) * 8;
  // (speculative attempts: 16 bytes per chunk byte past their first, and 1 KiB)
  const uint64_t budget = uint64_t(b.chunk) * 16 + 1024;
  hipLaunchKernelGGL(k_cl_init, dim3(1), dim3(64), 0, stream, b);
  hipLaunchKernelGGL((k_cl_walk<KIND, kThreads, MODE>), dim3(uint32_t(blocks)), dim3(kThreads),
                     ldsBytes, stream, d, p, n, b, budget, a);
  for (int round = 0; round < kClRounds; ++round) {
    hipLaunchKernelGGL(k_cl_resolve, dim3(uint32_t(small)), dim3(256), 0, stream, b, round);
    hipLaunchKernelGGL((k_cl_rewalk<KIND, kThreads, MODE>), dim3(uint32_t(blocks)), dim3(kThreads),
                       ldsBytes, stream, d, p, n, b, round, budget, a);
  }
  hipLaunchKernelGGL(k_cl_check, dim3(uint32_t(small)), dim3(256), 0, stream, b);
  hipLaunchKernelGGL((k_cl_serial<KIND, MODE>), dim3(1), dim3(64), ldsBytes, stream, d, p, n, b, a);
  const uint64_t nb = (b.m + 1023) / 1024;
  hipLaunchKernelGGL(k_cl_scan1, dim3(uint32_t(nb)), dim3(1024), 0, stream, b);
  hipLaunchKernelGGL(k_cl_scan2, dim3(1), dim3(1024), 0, stream, b, nb, count);
  return hipGetLastError();
}

template <int KIND>
hipError_t launchCollectLongK(const DevDfa &d, const uint8_t *p, uint64_t n, const ClBufs &b,
                              uint64_t cap, uint64_t *count, int32_t *result, uint64_t *start,
                              uint64_t *end, const LaunchCfg &cfg, hipStream_t stream) {
  const hipError_t e = launchClChain<KIND, kClCollect>(d, p, n, b, ClAttempt{}, count, cfg, stream);
  if (e != hipSuccess) return e;
  if (cap) {
    uint64_t sb = (b.m + 3) / 4;
    if (sb > uint64_t(cfg.numCUs) * 16) sb = uint64_t(cfg.numCUs) * 16;
    hipLaunchKernelGGL(k_cl_scatter, dim3(uint32_t(sb)), dim3(256), 0, stream, b, cap, result, start,
                       end);
  }
  return hipGetLastError();
}
