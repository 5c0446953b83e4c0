// k_collect_text.h - grep -o over a raw text: every match of every line, as compact records in text
// order (Red::collect, lib/Red.cpp:103-116, inside the line loop of tools/skim_red.cpp:36-46 over
// the lines lib/Util.cpp:109-130 cuts)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_grep.h).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it - so nothing is proportional to the line
// count or to the record count, and nothing waits for either.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk], open[chunk], and the HIT bitmap (the selected bitmap's layout) zeroed;
//   k_ct_count      table staged once per workgroup, a wave per chunk, chunks grid-strided, rounds of
//                   64 lines (k_text.h: textLines).  A lane runs the collect chain (collectLane) over its
//                   line, counts its matches and sets the line's bit in the hit bitmap when it has
//                   one; matchCounts[chunk] = the wave's sum;
//   k_split_scan    again, over matchCounts: matchBases[chunk] = records in front of the chunk, and
//                   the total straight into *n_matches (its thread 0 stores it);
//   k_ct_write      (skipped when the call only counts) a wave per chunk over the HIT bitmap; chunks
//                   without a hit, or whose matchBases is at or past the cap, are skipped.  Per round
//                   of 64 hit lines a lane finds its line's begin / finish / index (k_text.h:
//                   TextHits), walks the line to count its matches, the wave takes an exclusive prefix of
//                   the counts (shuffles) plus the carry of the earlier rounds, and the lane walks
//                   its line again and stores record matchBases[chunk] + prefix + i while that is
//                   below the cap - the walk ends where the cap does.
// No per-line count is stored anywhere; no workgroup waits for another: the order of the records
// comes from the passes.
#pragma once

// Red::collect over p[0..n) (lib/Red.cpp:103-116): all non-overlapping matches in order, by
// repeated search<styLast,false> from the end of the previous match - k_lists.h:k_collect's loop
// body, with the record handed to f(accepting state, start, end) instead of stored; f returns
// whether the chain goes on.  Returns the matches found (those f saw).
// An f that takes a fourth argument is also handed where the attempt that matched BEGAN: [at, end)
// is the span replaceCore substitutes, and at <= start (a loose-start DFA leaves its initial state
// later).  For an f of three arguments nothing of this exists: the code is what it was.
template <class T, class F>
__device__ __forceinline__ uint64_t collectLane(const T &tab, const LaneCtx &c, const uint8_t *p,
                                                uint64_t n, F &&f) {
  constexpr bool kWantsAt = std::is_invocable_v<F &, uint32_t, uint64_t, uint64_t, uint64_t>;
  const StartFilter flt{c.startWord[0], c.startCount[0] <= 4 ? c.startCount[0] : 0u,
                        c.start2Word[0], c.start2Count[0] <= 4 ? c.start2Count[0] : 0u, false};
  uint64_t found = 0, pos = 0;
  while (pos < n) {
    // search<styLast,false> from pos (Matcher.h:557-640), lean: an attempt carries the state,
    // the last accepting state, its end and the last "left the initial state" position; the
    // result table is read once per match.  Attempts that outlive a few bytes go on in
    // 16-byte requests (a dense DFA's attempt runs to the end of the line).
    bool got = false;
    uint32_t accS = 0;
    uint64_t mS = 0, mE = 0;
    [[maybe_unused]] uint64_t mA = 0;
    walkBytesPeek(p, pos, n, flt, [] {}, [&](uint32_t byte, uint64_t i, uint32_t nextByte) -> bool {
      uint32_t st = tab.next(c.init, byte);
      bool any = false;
      uint64_t ms = i, me = i;
      uint32_t aS = 0;
      if (st >= c.firstAccept) { aS = st; me = i + 1; any = true; }
      else if (st < c.nPureDead) return true;
      else if (nextByte != kNoPeek && tab.next(st, nextByte) < c.nPureDead) return true;
      auto stepOne = [&](uint32_t b2, uint64_t q) -> bool {
        const uint32_t was = st;
        st = tab.next(st, b2);
        if (was == c.init && st != was) ms = q;
        const bool acc = st >= c.firstAccept;
        if (acc) { aS = st; me = q + 1; any = true; }
        return acc || st >= c.nPureDead;
      };
      uint64_t q = i + 1;
      bool alive = true;
      for (uint32_t k = 0; k < 6 && q < n && alive; ++k, ++q) alive = stepOne(uint32_t(p[q]), q);
      if (alive) {
        // (walkBytes stops when stepOne says so: alive = the walk reached the end of the line)
        walkBytes(p, q, n, [&](uint32_t b2, uint64_t q2) -> bool { return alive = stepOne(b2, q2); });
      }
      if (!any) return !(c.suffixClosed && alive);  // L = SIGMA* L: no later start can match either
      got = true; accS = aS; mS = ms; mE = me;
      if constexpr (kWantsAt) mA = i;
      return false;
    });
    if (!got) break;
    ++found;
    if constexpr (kWantsAt) {
      if (!f(accS, mS, mE, mA)) break;
    } else if (!f(accS, mS, mE)) break;
    pos = mE;
  }
  return found;
}

// b.selMasks = the hit bitmap, b.selCounts = matchCounts, b.selBases = matchBases
template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_ct_count(DevDfa d, const uint8_t *data, GpBufs b) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    uint64_t mine = 0;
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (have) {
        const uint64_t found = collectLane(tab, c, data + beg, fin - beg,
                                           [](uint32_t, uint64_t, uint64_t) { return true; });
        if (found) {
          atomicOr(reinterpret_cast<uint32_t *>(b.selMasks) + (fin >> 5), 1u << (fin & 31u));
          mine += found;
        }
      }
    });
    for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0) b.selCounts[ch] = uint32_t(mine);
  }
}

struct CtOut {
  uint64_t limit;  // records to place: the cap
  uint64_t *line, *begin;
  int32_t *result;
  uint64_t *start, *end;
};

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_ct_write(DevDfa d, const uint8_t *data, GpBufs b, CtOut out) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    const uint64_t first = b.selBases[ch];
    if (first >= out.limit || b.selCounts[ch] == 0) continue;  // (uniform)
    const TextHits h(b, ch, lane);
    uint64_t carry = first;  // index of the round's first record
    for (uint32_t k0 = 0; k0 < h.s.total && carry < out.limit; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool have = k < h.s.total;
      uint64_t beg, fin;
      uint32_t index;
      h.line(h.s.select(have ? k : h.s.total - 1), beg, fin, index);  // the hit line
      // the counting walk, then the lanes' exclusive prefix
      uint64_t cnt = 0;
      if (have)
        cnt = collectLane(tab, c, data + beg, fin - beg,
                          [](uint32_t, uint64_t, uint64_t) { return true; });
      uint64_t incl = cnt;
      for (int sh = 1; sh < 64; sh <<= 1) {
        const uint64_t v = __shfl_up(incl, sh);
        if (lane >= uint32_t(sh)) incl += v;
      }
      uint64_t rec = carry + (incl - cnt);
      carry += __shfl(incl, 63);
      if (cnt && rec < out.limit) {  // (every lane is back at the next round's shuffles)
        const uint64_t lineNo = b.bases[ch] + index;
        collectLane(tab, c, data + beg, fin - beg, [&](uint32_t accS, uint64_t mS, uint64_t mE) {
          if (out.line) out.line[rec] = lineNo;
          if (out.begin) out.begin[rec] = beg;
          if (out.result) out.result[rec] = c.res[accS];
          if (out.start) out.start[rec] = beg + mS;
          if (out.end) out.end[rec] = beg + mE;
          return ++rec < out.limit;
        });
      }
    }
  }
}

template <int KIND>
hipError_t launchCollectTextK(const DevDfa &d, const uint8_t *data, const GpBufs &b,
                              const CtOut &out, bool write, uint64_t *nMatches, uint64_t *matchBases,
                              uint64_t *dummy, const LaunchCfg &cfg, hipStream_t stream) {
  // threads and resident workgroups by k_text.h's rule (textBlocks), but for the write pass of the
  // LDS placements: it holds two chunk views and the prefix beside the chain, and at 1024 threads
  // (128 VGPRs) it spills 22-27 of them (92-112 bytes of private memory per lane), where k_ct_count
  // and k_gp_select spill none - so it runs 512 threads (158 VGPRs, no spill)
  constexpr int kThreads = kStagedThreads<KIND>;
  constexpr int kWriteThreads = kStagedLds<KIND> ? 512 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_ct_count<KIND, kThreads>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_ct_write<KIND, kWriteThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  if (b.nChunks) {
    hipLaunchKernelGGL((k_ct_count<KIND, kThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg)), dim3(kThreads),
                       ldsBytes, stream, d, data, b);
  }
  // (the scan's total is *n_matches; its offsets[0] store goes to a spare word)
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, b.selCounts, b.nChunks,
                     matchBases, nMatches, dummy, uint64_t(0));
  if (write && b.nChunks) {
    hipLaunchKernelGGL((k_ct_write<KIND, kWriteThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kWriteThreads, cfg)),
                       dim3(kWriteThreads), ldsBytes, stream, d, data, b, out);
  }
  return hipGetLastError();
}
