// k_extract_text.h - grep -o over a raw text with its output as a text: every match of every line
// as bytes, each followed by the delimiter, in text order (Red::collect, lib/Red.cpp:103-116, inside
// the line loop of tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts; a piece is the
// span replace<styLast,false> substitutes, include/Matcher.h:643-706: from where the successful
// attempt BEGAN to the match's end)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_collect_text.h and
// k_replace_text.h, whose rtCopyWave it uses).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it - so nothing is proportional to the line
// count or to the match count, and nothing waits for either.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk], open[chunk], and the HIT bitmap (the selected bitmap's layout) zeroed;
//   k_xt_size       table staged once per workgroup, a wave per chunk, chunks grid-strided, rounds of
//                   64 lines (k_text.h: textLines).  A lane runs the collect chain (collectLane) over its
//                   line, up to max_per_line pieces; outBytes[chunk] = the sum of (piece length + 1),
//                   pieceCounts[chunk] = the pieces, both u64; a line with a piece sets its
//                   delimiter's bit in the hit bitmap;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_xt_totals     one workgroup: *n_matches = the sum of pieceCounts, *out_len = the total;
//   k_xt_write      (skipped when the call only sizes) a wave per chunk over the HIT bitmap; chunks
//                   without a hit or with outBases[chunk] >= out_cap are skipped.  Per round of 64 hit
//                   lines a lane finds its line's begin / finish (k_text.h: TextHits) and sizes it
//                   again; the wave's exclusive prefix plus the carry of the earlier rounds gives
//                   every lane ONE contiguous run of the output, p1 d p2 d ...  The lane walks its
//                   line once more and assembles the run in a 16-byte register window (XtWindow)
//                   laid over the 16-byte blocks of the real address out + offset: a block that
//                   lies wholly inside the run, cut at out_cap, is one 16-byte store; the run's two
//                   ragged ends go out as the widest aligned 8 / 4 / 2 / 1-byte stores that stay
//                   inside it.  The source is read 8 bytes at a time.  A piece of kXtHand bytes or
//                   more is not taken through the window: the lane closes its window in front of
//                   it, leaves the chain, and the WHOLE WAVE copies the pieces so handed over one
//                   after the other (rtCopyWave); the lane then goes on with the chain behind it.
// No per-line or per-match value is stored anywhere; no workgroup waits for another.  Nothing is
// read outside data[0, len) and nothing is written at or behind out_cap, or outside a lane's run.
#pragma once

// pieces from this length on are copied by the whole wave (DESIGN 4.3k has the measurement)
constexpr uint32_t kXtHand = 64;

// b.selMasks = the hit bitmap; b.selCounts / b.selBases are not used here
struct XtBufs {
  uint64_t *outBytes;        // [nChunks] output bytes of the chunk's lines
  uint64_t *pieceCounts;     // [nChunks] pieces of the chunk's lines
  const uint64_t *outBases;  // [nChunks + 1] exclusive scan of outBytes, the total behind it
};

// the first maxPer (> 0) pieces of p[0..n): their number, and the sum of (length + 1) added to bytes
template <class T>
__device__ __forceinline__ uint64_t xtSizeLane(const T &tab, const LaneCtx &c, const uint8_t *p,
                                               uint64_t n, uint64_t maxPer, uint64_t &bytes) {
  // (the chain's own count is not looked at: one counter less in registers)
  uint64_t left = maxPer;
  collectLane(tab, c, p, n, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
    bytes += mE - at + 1;
    return --left != 0;
  });
  return maxPer - left;
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_xt_size(DevDfa d, const uint8_t *data, GpBufs b, XtBufs x, uint64_t maxPer) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    uint64_t bytes = 0, pieces = 0;
    if (maxPer) {  // (uniform)
      textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
        if (have) {
          const uint64_t cnt = xtSizeLane(tab, c, data + beg, fin - beg, maxPer, bytes);
          if (cnt) {
            atomicOr(reinterpret_cast<uint32_t *>(b.selMasks) + (fin >> 5), 1u << (fin & 31u));
            pieces += cnt;
          }
        }
      });
    }
    for (int o = 32; o; o >>= 1) {
      bytes += __shfl_xor(bytes, o);
      pieces += __shfl_xor(pieces, o);
    }
    if (lane == 0) {
      x.outBytes[ch] = bytes;
      x.pieceCounts[ch] = pieces;
    }
  }
}

// one workgroup: *nMatches = the sum of pieceCounts, *outLen = the scan's total (outTotal ==
// nullptr: the text is empty)
__global__ void __launch_bounds__(1024)
k_xt_totals(const uint64_t *pieceCounts, uint64_t nChunks, const uint64_t *outTotal,
            uint64_t *outLen, uint64_t *nMatches) {
  __shared__ uint64_t ws[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 1024) sum += pieceCounts[i];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) ws[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t all = 0;
    for (int w = 0; w < 16; ++w) all += ws[w];
    *nMatches = all;
    *outLen = outTotal ? *outTotal : 0;
  }
}

// A lane's run of the output, assembled 16 bytes at a time.  Positions are counted from `base`,
// the 16-byte aligned address at or below out, so a block of the window IS an aligned 16 bytes of
// memory.  The window holds the bytes [from, at) of the block at rounds down to; `end` is where the
// lane stops (its run's end, cut at out_cap): put() drops what would lie at or behind it.
struct XtWindow {
  uint8_t *base;
  uint64_t at, from, end;
  uint64_t lo, hi;  // the block's bytes 0..7, 8..15

  __device__ __forceinline__ void open(uint64_t pos) {
    at = from = pos;
    lo = hi = 0;
  }
  __device__ __forceinline__ bool full() const { return at >= end; }

  // s bytes (1, 2, 4, 8) of the block from its byte x, which is a multiple of s
  __device__ __forceinline__ uint64_t part(uint32_t x) const {
    return (x & 8u ? hi : lo) >> (8u * (x & 7u));
  }

  // the block's bytes [a, b) to memory: all 16 in one store, else the widest aligned stores that
  // stay inside - upwards while the alignment grows, then downwards
  __device__ __forceinline__ void store(uint64_t block, uint32_t a, uint32_t b) const {
    uint8_t *q = base + block;
    if (a == 0 && b == 16) {
      *reinterpret_cast<uint4 *>(q) =
          make_uint4(uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32));
      return;
    }
    if ((a & 1u) && a + 1 <= b) { q[a] = uint8_t(part(a)); a += 1; }
    if ((a & 2u) && a + 2 <= b) { *reinterpret_cast<uint16_t *>(q + a) = uint16_t(part(a)); a += 2; }
    if ((a & 4u) && a + 4 <= b) { *reinterpret_cast<uint32_t *>(q + a) = uint32_t(part(a)); a += 4; }
    if ((a & 8u) && a + 8 <= b) { *reinterpret_cast<uint64_t *>(q + a) = hi; a += 8; }
    // (a is now a multiple of a power of two above b - a, or of 16)
    if (a + 8 <= b) { *reinterpret_cast<uint64_t *>(q + a) = part(a); a += 8; }
    if (a + 4 <= b) { *reinterpret_cast<uint32_t *>(q + a) = uint32_t(part(a)); a += 4; }
    if (a + 2 <= b) { *reinterpret_cast<uint16_t *>(q + a) = uint16_t(part(a)); a += 2; }
    if (a + 1 <= b) q[a] = uint8_t(part(a));
  }

  // what the window holds goes out; it is empty behind this (at a block's end or not)
  __device__ __forceinline__ void close() {
    if (at > from) {
      const uint64_t block = from & ~15ull;
      store(block, uint32_t(from - block), uint32_t(at - block));
    }
    from = at;
    lo = hi = 0;
  }

  // the low k bytes (1..8) of v behind what the window holds
  __device__ __forceinline__ void put(uint64_t v, uint32_t k) {
    if (at >= end) return;
    if (k > end - at) k = uint32_t(end - at);
    if (k < 8) v &= (1ull << (8u * k)) - 1;
    const uint32_t pos = uint32_t(at) & 15u;
    uint64_t over = 0;  // what belongs to the next block
    if (pos < 8) {
      lo |= v << (8u * pos);
      if (pos) hi |= v >> (64u - 8u * pos);
    } else {
      const uint32_t sh = 8u * (pos - 8u);
      hi |= v << sh;
      if (sh) over = v >> (64u - sh);
    }
    at += k;
    if (pos + k >= 16) {
      const uint64_t block = from & ~15ull;
      store(block, uint32_t(from - block), 16);
      from = block + 16;
      lo = over;
      hi = 0;
    }
  }
};

// 8 bytes of data from position s (only the first k count): one load where 8 bytes are there,
// byte loads at the text's very end
__device__ __forceinline__ uint64_t xtLoad8(const uint8_t *data, uint64_t len, uint64_t s,
                                            uint32_t k) {
  if (s + 8 <= len) return *reinterpret_cast<const uint64_t *>(data + s);
  uint64_t v = 0;
  for (uint32_t i = 0; i < k; ++i) v |= uint64_t(data[s + i]) << (8u * i);
  return v;
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_xt_write(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, XtBufs x, uint64_t maxPer,
           uint32_t delim, uint32_t hand, uint8_t *out, uint64_t cap) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  // the window counts from the aligned address at or below out
  const uint64_t mis = reinterpret_cast<uintptr_t>(out) & 15u;
  XtWindow w;
  w.base = out - mis;
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    const uint64_t first = x.outBases[ch];
    if (first >= cap || x.outBytes[ch] == 0) continue;  // (uniform)
    const TextHits h(b, ch, lane);
    uint64_t carry = first;  // where the round's first run goes
    for (uint32_t k0 = 0; k0 < h.s.total && carry < cap; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool have = k < h.s.total;
      uint64_t beg, fin;
      uint32_t index;  // (not needed here)
      h.line(h.s.select(have ? k : h.s.total - 1), beg, fin, index);  // the hit line
      // the sizing walk, then the lanes' exclusive prefix
      uint64_t mine = 0;
      if (have) xtSizeLane(tab, c, data + beg, fin - beg, maxPer, mine);
      uint64_t incl = mine;
      for (int sh = 1; sh < 64; sh <<= 1) {
        const uint64_t v = __shfl_up(incl, sh);
        if (lane >= uint32_t(sh)) incl += v;
      }
      const uint64_t dst = carry + (incl - mine);
      carry += __shfl(incl, 63);
      // the lane's run: out[dst, dst + mine), cut at cap
      const uint64_t stop = dst + mine < cap ? dst + mine : cap;
      w.end = mis + stop;
      w.open(mis + dst);
      uint64_t pos = 0;  // where in the line the chain goes on
      bool more = mine != 0 && dst < cap;
      while (__ballot(more)) {
        uint64_t bigSrc = 0, bigDst = 0, bigLen = 0;
        if (more) {
          more = false;
          const uint64_t lineAt = beg + pos;
          collectLane(tab, c, data + lineAt, fin - lineAt,
                      [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
            uint64_t s = lineAt + at, n = mE - at;
            if (n >= hand) {
              // to the wave: the window ends in front of the piece and begins again behind it
              w.close();
              bigSrc = s;
              bigDst = w.at - mis;
              bigLen = n;
              w.open(w.at + n);
              w.put(delim, 1);
              pos += mE;
              more = !w.full();
              return false;
            }
            for (; n; s += 8) {
              const uint32_t take = n < 8 ? uint32_t(n) : 8u;
              w.put(xtLoad8(data, len, s, take), take);
              n -= take;
            }
            w.put(delim, 1);
            return !w.full();
          });
        }
        // the pieces handed over, one after the other, by the whole wave
        uint64_t todo = __ballot(bigLen != 0);
        while (todo) {
          const int j = __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1;
          rtCopyWave(out, __shfl(bigDst, j), data + __shfl(bigSrc, j), __shfl(bigLen, j), cap, lane);
        }
      }
      w.close();
    }
  }
}

template <int KIND>
hipError_t launchExtractTextK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                              const XtBufs &x, uint64_t maxPer, uint8_t delim, uint32_t hand,
                              bool size, uint8_t *out, uint64_t cap, const LaunchCfg &cfg,
                              hipStream_t stream) {
  // threads and resident workgroups by k_text.h's rule (textBlocks): the sizing pass as k_ct_count,
  // the write pass - two chunk views, the prefix and the window beside the chain - at 512 threads
  // under the LDS placements so that it does not spill (profiles/extract_text_resources.md)
  constexpr int kThreads = kStagedThreads<KIND>;
  constexpr int kWriteThreads = kStagedLds<KIND> ? 512 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_xt_size<KIND, kThreads>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_xt_write<KIND, kWriteThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  if (size) {
    hipLaunchKernelGGL((k_xt_size<KIND, kThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg)), dim3(kThreads),
                       ldsBytes, stream, d, data, b, x, maxPer);
  } else {
    hipLaunchKernelGGL((k_xt_write<KIND, kWriteThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kWriteThreads, cfg)),
                       dim3(kWriteThreads), ldsBytes, stream, d, data, len, b, x, maxPer,
                       uint32_t(delim), hand, out, cap);
  }
  return hipGetLastError();
}
