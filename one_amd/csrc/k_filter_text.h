// k_filter_text.h - grep over a raw text with its output as a text: the lines search<style,doLeader>
// selects (the first max_count of them), `before` lines in front of and `after` lines behind each
// (grep -B / -A), every emitted line once, in text order, with its delimiter
// (tools/skim_red.cpp:36-46's loop over the lines lib/Util.cpp:109-130 cuts, printing the line)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_replace_text.h;
// DESIGN 4.3j).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  Past the select pass no line is walked:
// the context is arithmetic on line NUMBERS, and a lane does it for the delimiters among its own 256
// bits of the chunk, in registers.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h), and the
//                   SELECTED bitmap zeroed;
//   k_gp_select / k_split_scan / k_gp_total   (k_grep.h, as they stand) the SELECTED bitmap,
//                   selCounts[chunk], selBases[chunk], *n_selected = min(selected, max_count);
//   k_ft_edges      a wave per chunk: the chunk's COUNTED selected lines are its first
//                   min(selCounts, max_count - selBases) selected ones (ftFirst); prevSel[chunk] = 1 +
//                   the line number (bases[chunk] + rank) of the last of them (0 = none),
//                   nextRev[nChunks - 1 - chunk] = ~ the line number of the first (0 = none);
//   k_gp_open       (k_text.h, as it stands) twice: its exclusive max-scan in place turns prevSel
//                   into "1 + the last counted selected line in front of the chunk" and nextRev -
//                   stored back to front and complemented, so that the same scan is an exclusive
//                   suffix min - into "~ the first counted selected line behind the chunk";
//   k_ft_mark       a wave per chunk.  A lane's carries: the nearest counted selected line in front
//                   of / behind its 256 bits (a max- / min-scan over the lanes, seeded with the
//                   chunk's two values).  It then steps through its own delimiters, downwards for
//                   `before` (skipped when 0) and upwards for `after`, with the nearest counted
//                   selected line at or behind / at or before the current one in a register: line i
//                   is emitted iff next - i <= before or i - prev <= after - differences of line
//                   numbers with prev <= i <= next, so no value of before / after overflows.  The
//                   lane's 256 EMIT bits are stored over its SELECTED bits (a chunk reads its own
//                   bits only, and they are in registers by then); emitBytes[chunk] = the emitted
//                   lines' bytes with their delimiters (u64: a line may begin many chunks back),
//                   emitLines[chunk] = their number;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_ft_totals     one workgroup: *n_emitted = the sum of emitLines, *out_len = the total;
//   k_ft_write      (skipped when the call only sizes) a wave per chunk; chunks without an emitted
//                   line or with outBases[chunk] >= out_cap are skipped.  A RUN is a maximal stretch
//                   of consecutive emitted lines of the chunk - contiguous in the source.  Each lane
//                   marks, among its own delimiters, those that begin a run (the delimiter below is
//                   not emitted, or is in front of the chunk) and those that end one; per round of 64
//                   runs lane j takes the j-th begin and the j-th end (GpChunk::select), the begin of
//                   the first line from TextHits::line (open[chunk] when the line began in an earlier
//                   chunk), a prefix over the lengths places the runs, and each is one rtCopyWave by
//                   the whole wave, cut at out_cap.  No table, no LDS.
// No per-line value is stored anywhere; no workgroup waits for another.  Nothing is read outside
// data[0, len) - a run is [a line's begin, a delimiter's position] - and nothing is written at or
// behind out_cap.
#pragma once

constexpr uint64_t kFtNone = ~0ull;

// position of the lowest set bit of m, which has one
__device__ __forceinline__ uint32_t ftLowest(const GpBits &m) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 3; k >= 0; --k)
    if (m.w[k]) r = uint32_t(64 * k + __ffsll(static_cast<long long>(m.w[k])) - 1);
  return r;
}

// the set bits of m below bit p (p < 256)
__device__ __forceinline__ uint32_t ftBelow(const GpBits &m, uint32_t p) {
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = uint32_t(64 * k);
    uint64_t x = m.w[k];
    if (p < lo + 64) x = p > lo ? x & ((1ull << (p - lo)) - 1) : 0;
    n += uint32_t(__popcll(x));
  }
  return n;
}

// this lane's part of the chunk's first n set bits (s scanned)
__device__ __forceinline__ GpBits ftFirst(const GpChunk &s, uint32_t n) {
  GpBits c = s.m;
  const uint32_t own = s.m.count();
  if (s.excl + own > n) {
    // the lane keeps its first n - excl bits: those below its bit of that rank (which it has)
    const uint32_t keep = n > s.excl ? n - s.excl : 0;
    const uint32_t cut = gpSelect256(s.m, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = uint32_t(64 * k);
      if (cut < lo + 64) c.w[k] = cut > lo ? c.w[k] & ((1ull << (cut - lo)) - 1) : 0;
    }
  }
  return c;
}

// the chunk's counted selected lines: the first min(selected, max_count - selBases) selected ones
__device__ __forceinline__ uint32_t ftCounted(uint32_t selected, uint64_t selBase,
                                              uint64_t maxCount) {
  if (selBase >= maxCount) return 0;
  return selected < maxCount - selBase ? selected : uint32_t(maxCount - selBase);
}

__device__ __forceinline__ void ftStoreBits(uint16_t *bitmap, uint64_t chunk, uint32_t lane,
                                            const GpBits &m) {
  uint4 *q = reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(bitmap) +
                                       chunk * (kSplitChunk / 8) + lane * 32u);
  q[0] = make_uint4(uint32_t(m.w[0]), uint32_t(m.w[0] >> 32), uint32_t(m.w[1]),
                    uint32_t(m.w[1] >> 32));
  q[1] = make_uint4(uint32_t(m.w[2]), uint32_t(m.w[2] >> 32), uint32_t(m.w[3]),
                    uint32_t(m.w[3] >> 32));
}

// a mark pass's tail (k_ft_mark, k_dedup_text.h: k_dd_emit): the lane's 256 EMIT bits stored, and
// the wave's sums of the lanes' emitted bytes and lines left as emitBytes[chunk], emitLines[chunk]
__device__ __forceinline__ void ftStoreEmit(uint16_t *bitmap, uint64_t chunk, uint32_t lane,
                                            const GpBits &e, uint64_t bytes, uint32_t lines,
                                            uint64_t *emitBytes, uint32_t *emitLines) {
  ftStoreBits(bitmap, chunk, lane, e);
  for (int o = 32; o; o >>= 1) {
    bytes += __shfl_xor(bytes, o);
    lines += __shfl_xor(lines, o);
  }
  if (lane == 0) {
    emitBytes[chunk] = bytes;
    emitLines[chunk] = lines;
  }
}

// f(k, bit) over the set bits of m, from the lowest / from the highest: k = the word, as a
// std::integral_constant (no register is indexed by a variable), bit = the bit's mask in it
template <int K, class F>
__device__ __forceinline__ void ftWordUp(uint64_t x, F &&f) {
  while (x) {
    const uint64_t bit = x & (0 - x);
    x ^= bit;
    f(std::integral_constant<int, K>(), bit);
  }
}
template <int K, class F>
__device__ __forceinline__ void ftWordDown(uint64_t x, F &&f) {
  while (x) {
    const uint64_t bit = 1ull << (63 - __clzll(static_cast<long long>(x)));
    x ^= bit;
    f(std::integral_constant<int, K>(), bit);
  }
}
template <class F>
__device__ __forceinline__ void ftEachUp(const GpBits &m, F &&f) {
  ftWordUp<0>(m.w[0], f);
  ftWordUp<1>(m.w[1], f);
  ftWordUp<2>(m.w[2], f);
  ftWordUp<3>(m.w[3], f);
}
template <class F>
__device__ __forceinline__ void ftEachDown(const GpBits &m, F &&f) {
  ftWordDown<3>(m.w[3], f);
  ftWordDown<2>(m.w[2], f);
  ftWordDown<1>(m.w[1], f);
  ftWordDown<0>(m.w[0], f);
}

// per chunk: prevSel[chunk] = 1 + the number of its last counted selected line (0 = none),
// nextRev[nChunks - 1 - chunk] = ~ the number of its first (0 = none)
__global__ void __launch_bounds__(256)
k_ft_edges(GpBufs b, uint64_t maxCount, uint64_t *prevSel, uint64_t *nextRev) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    uint64_t last1 = 0, first = kFtNone;
    const uint32_t n = ftCounted(b.selCounts[ch], b.selBases[ch], maxCount);
    if (n) {  // (uniform)
      GpChunk s, g;
      s.m = gpLoadBits(b.selMasks, ch, lane);
      s.scan(lane);
      g.m = gpLoadBits(b.masks, ch, lane);
      g.scan(lane);
      const GpBits c = ftFirst(s, n);
      if (c.count()) {
        const uint64_t lineBase = b.bases[ch] + g.excl;
        last1 = lineBase + ftBelow(g.m, c.last() - 1) + 1;
        first = lineBase + ftBelow(g.m, ftLowest(c));
      }
      for (int o = 32; o; o >>= 1) {
        const uint64_t v = __shfl_xor(last1, o), u = __shfl_xor(first, o);
        last1 = v > last1 ? v : last1;
        first = u < first ? u : first;
      }
    }
    if (lane == 0) {
      prevSel[ch] = last1;
      nextRev[b.nChunks - 1 - ch] = ~first;
    }
  }
}

// prevSel / nextRev as k_gp_open's scans leave them.  The chunk's EMIT bits over its SELECTED bits,
// emitBytes[chunk], emitLines[chunk].
__global__ void __launch_bounds__(256)
k_ft_mark(GpBufs b, uint64_t maxCount, uint64_t before, uint64_t after, const uint64_t *prevSel,
          const uint64_t *nextRev, uint64_t *emitBytes, uint32_t *emitLines) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    const TextHits h(b, ch, lane);  // (h.s: the SELECTED bits)
    const GpBits c = ftFirst(h.s, ftCounted(h.s.total, b.selBases[ch], maxCount));
    const uint64_t lineBase = b.bases[ch] + h.g.excl;  // the number of the lane's first line
    // 1 + the last counted selected line in front of the lane's bits (0 = none), the first one
    // behind them (kFtNone = none)
    const bool has = c.count() != 0;
    uint64_t prev1 = has ? lineBase + ftBelow(h.g.m, c.last() - 1) + 1 : 0;
    uint64_t next = has ? lineBase + ftBelow(h.g.m, ftLowest(c)) : kFtNone;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t v = __shfl_up(prev1, o), u = __shfl_down(next, o);
      if (lane >= uint32_t(o) && v > prev1) prev1 = v;
      if (lane + uint32_t(o) < 64 && u < next) next = u;
    }
    prev1 = __shfl_up(prev1, 1);
    next = __shfl_down(next, 1);
    if (lane == 0) prev1 = 0;
    if (lane == 63) next = kFtNone;
    const uint64_t prevChunk = prevSel[ch], nextChunk = ~nextRev[b.nChunks - 1 - ch];
    if (prevChunk > prev1) prev1 = prevChunk;
    if (nextChunk < next) next = nextChunk;

    GpBits e{{0, 0, 0, 0}};
    const uint32_t own = h.g.m.count();
    if (before) {  // (uniform) downwards: next = the nearest counted selected line at or behind
      uint32_t t = own;
      ftEachDown(h.g.m, [&](auto word, uint64_t bit) {
        constexpr int k = decltype(word)::value;
        const uint64_t i = lineBase + --t;
        if (c.w[k] & bit) next = i;
        if (next != kFtNone && next - i <= before) e.w[k] |= bit;
      });
    }
    // upwards: prev1 - 1 = the nearest counted selected line at or before; the emitted lines'
    // bytes, from behind the delimiter below (h.behind for the lane's first) to their own
    uint64_t bytes = 0, begin = h.behind;
    uint32_t t = 0, lines = 0;
    ftEachUp(h.g.m, [&](auto word, uint64_t bit) {
      constexpr int k = decltype(word)::value;
      const uint64_t i = lineBase + t++;
      if (c.w[k] & bit) prev1 = i + 1;
      if (prev1 && i - (prev1 - 1) <= after) e.w[k] |= bit;
      const uint64_t behind = h.base + lane * 256u + uint32_t(64 * k) +
                              uint32_t(__ffsll(static_cast<long long>(bit)));
      if (e.w[k] & bit) {
        bytes += behind - begin;
        ++lines;
      }
      begin = behind;
    });
    ftStoreEmit(b.selMasks, ch, lane, e, bytes, lines, emitBytes, emitLines);
  }
}

// one workgroup: *nEmitted = the sum of emitLines, *outLen = the scan's total (outTotal == nullptr:
// the text is empty)
__global__ void __launch_bounds__(1024)
k_ft_totals(const uint32_t *emitLines, uint64_t nChunks, const uint64_t *outTotal, uint64_t *outLen,
            uint64_t *nEmitted) {
  __shared__ uint64_t ws[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 1024) sum += emitLines[i];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) ws[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t all = 0;
    for (int w = 0; w < 16; ++w) all += ws[w];
    *nEmitted = all;
    *outLen = outTotal ? *outTotal : 0;
  }
}

// The runs of one chunk's emitted lines (e: this lane's EMIT bits, a subset of its delimiter bits)
// copied to out from dstAt on, cut at cap - k_ft_write's body, and k_route_text.h's once per
// bucket.  h: the chunk's views (h.s is not read).  Every lane calls; dstAt and cap are uniform.
__device__ __forceinline__ void ftWriteRuns(const uint8_t *data, const TextHits &h, const GpBits &e,
                                            uint64_t dstAt, uint8_t *out, uint64_t cap,
                                            uint32_t lane) {
  // is the delimiter below the lane's bits emitted (none: no), and the one above them
  const uint32_t own = h.g.m.count();
  uint32_t below = 0, above = 0xffffffffu;
  if (own) {
    uint32_t top = 0, bottom = 0;  // is the lane's highest / lowest delimiter emitted
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t x = h.g.m.w[k], y = h.g.m.w[3 - k];
      if (x) top = (e.w[k] >> (63 - __clzll(static_cast<long long>(x)))) & 1u;
      if (y) bottom = (e.w[3 - k] >> (__ffsll(static_cast<long long>(y)) - 1)) & 1u;
    }
    below = (lane << 1 | top) + 1;
    above = lane << 1 | bottom;
  }
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(below, o), u = __shfl_down(above, o);
    if (lane >= uint32_t(o) && v > below) below = v;
    if (lane + uint32_t(o) < 64 && u < above) above = u;
  }
  below = __shfl_up(below, 1);
  above = __shfl_down(above, 1);
  bool on = lane != 0 && below != 0 && ((below - 1) & 1u);
  bool onAbove = lane != 63 && above != 0xffffffffu && (above & 1u);
  // the delimiters that begin a run of emitted lines, and those that end one
  GpBits begins{{0, 0, 0, 0}}, ends{{0, 0, 0, 0}};
  ftEachUp(h.g.m, [&](auto word, uint64_t bit) {
    constexpr int k = decltype(word)::value;
    const bool is = (e.w[k] & bit) != 0;
    if (is && !on) begins.w[k] |= bit;
    on = is;
  });
  ftEachDown(h.g.m, [&](auto word, uint64_t bit) {
    constexpr int k = decltype(word)::value;
    const bool is = (e.w[k] & bit) != 0;
    if (is && !onAbove) ends.w[k] |= bit;
    onAbove = is;
  });
  GpChunk first, last;
  first.m = begins;
  last.m = ends;
  first.scan(lane);
  last.scan(lane);  // (last.total == first.total: the runs)
  for (uint32_t k0 = 0; k0 < first.total && dstAt < cap; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool have = k < first.total;
    const uint32_t pick = have ? k : first.total - 1;
    const uint32_t endPos = last.select(pick);
    uint64_t beg, fin;
    uint32_t index;  // (not needed here)
    h.line(first.select(pick), beg, fin, index);  // the run's first line
    const uint64_t mine = have ? h.base + endPos + 1 - beg : 0;
    uint64_t incl = mine;
    for (int sh = 1; sh < 64; sh <<= 1) {
      const uint64_t v = __shfl_up(incl, sh);
      if (lane >= uint32_t(sh)) incl += v;
    }
    const uint64_t dst = dstAt + (incl - mine);
    dstAt += __shfl(incl, 63);
    // the runs, one after the other, by the whole wave
    uint64_t todo = __ballot(have);
    while (todo) {
      const int j = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      rtCopyWave(out, __shfl(dst, j), data + __shfl(beg, j), __shfl(mine, j), cap, lane);
    }
  }
}

// b.selMasks = the EMIT bitmap
__global__ void __launch_bounds__(256)
k_ft_write(const uint8_t *data, GpBufs b, const uint64_t *emitBytes, const uint64_t *outBases,
           uint8_t *out, uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    const uint64_t dstAt = outBases[ch];
    if (dstAt >= cap || emitBytes[ch] == 0) continue;  // (uniform)
    const TextHits h(b, ch, lane);                     // (h.s: the EMIT bits)
    ftWriteRuns(data, h, h.s.m, dstAt, out, cap, lane);
  }
}
