// k_route_text.h - a raw text's lines routed to their class: the text stably partitioned by the
// result search<style,doLeader> reports per line (awk '{ print > file[class] }' over the line loop
// of tools/skim_red.cpp:36-46, the lines lib/Util.cpp:109-130 cuts) - bucket 0's lines, then bucket
// 1's, ..., each bucket's lines in text order with their delimiters, and where each bucket begins
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_filter_text.h;
// DESIGN 4.3l).
//
// A line's value r is k_tally_text.h's LINES item, its bucket tally_text's slot: r when
// (uint32_t)r < nBins, else nBins.  What is kept per line is its CODE, in P bit-planes laid out like
// the SELECTED bitmap (bit p of the code at the line's delimiter in plane p): the bucket, P = the
// bit width of nBins (0 .. 8) - a line of value 0 has code 0 and costs no store.  Under
// drop_unmatched with nBins == 0 the one bucket holds dropped and emitted lines alike, so the code
// is "the line matches" in one plane (zeroCode); in every other case code 0 IS value 0.
// The lines are driven as k_text.h drives them - a wave per 16 KiB chunk, a chunk owning the lines
// that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h); the planes
//                   zeroed (a memset on the stream);
//   k_ro_class      k_gp_select's walk: table staged once per workgroup, a wave per chunk, rounds
//                   of 64 lines; the lane's line gives its code, and per set bit of it an atomic or
//                   of the line's delimiter bit into that plane.  The only pass that walks bytes;
//   k_ro_size       no table.  A wave per chunk, a lane steps through the delimiters among its own
//                   256 bits: the code from the planes, the length from the delimiter below
//                   (h.behind for the lane's first).  A lane sums a stretch of equal codes in
//                   registers and adds it to the wave's own LDS rows of nCodes byte sums and line
//                   counts; these go to sizes[code * nChunks + chunk] and lines[...], code-major.
//                   Dropped lines (code 0 under drop_unmatched) count as lines and add 0 bytes;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) ONE exclusive scan over all nCodes *
//                   nChunks sizes: outBases[code * nChunks + chunk], the total behind them;
//   k_ro_finish     a workgroup per code: bin_lines[code] = the sum of its row of lines,
//                   bin_offsets[code] = its first outBases; workgroup 0 also *out_len, the last
//                   offset, *n_lines and *n_routed;
//   k_ro_write      (skipped when the call only sizes) a wave per chunk, and for every code with
//                   bytes in the chunk and a base below out_cap: EMIT = the delimiters whose
//                   planes spell the code, and k_filter_text.h's run copy (ftWriteRuns) to the
//                   code's base.  No table, no LDS, no line walked.
// No per-line value is stored anywhere but the planes; no workgroup waits for another.  Nothing is
// read outside data[0, len) and nothing is written at or behind out_cap.
#pragma once

constexpr int kRoMaxPlanes = 8;
constexpr uint32_t kRoMaxBins = 255;  // nBins + 1 buckets fit kRoMaxPlanes bits

struct RoBufs {
  uint16_t *planes;          // nPlanes bitmaps of the delimiter bitmap's layout, one after the other
  uint64_t planeU16;         // u16 per plane: nChunks * (kSplitChunk / 16)
  const uint32_t *counts;    // [nChunks] delimiters in the chunk (k_split_count)
  uint64_t *sizes;           // [nCodes * nChunks] output bytes of the code's lines in the chunk
  uint32_t *lines;           // [nCodes * nChunks] their number (dropped ones included)
  const uint64_t *outBases;  // [nCodes * nChunks + 1] exclusive scan of sizes, the total behind it
  uint32_t nBins, nCodes, nPlanes;
  int zeroCode, drop;
};

__device__ __forceinline__ uint32_t roCode(const RoBufs &r, int32_t v) {
  if (r.zeroCode) return v != 0;
  return uint32_t(v) < r.nBins ? uint32_t(v) : r.nBins;
}

// a lane's 256 bits of every plane of a chunk (planes that do not exist read as 0)
struct RoPlanes {
  GpBits p[kRoMaxPlanes];
  __device__ __forceinline__ RoPlanes(const RoBufs &r, uint64_t ch, uint32_t lane) {
#pragma unroll
    for (int i = 0; i < kRoMaxPlanes; ++i) {
      if (uint32_t(i) < r.nPlanes) p[i] = gpLoadBits(r.planes + uint64_t(i) * r.planeU16, ch, lane);
      else p[i] = GpBits{{0, 0, 0, 0}};
    }
  }
  // the code at `bit` of word K
  template <int K>
  __device__ __forceinline__ uint32_t code(uint64_t bit) const {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kRoMaxPlanes; ++i) c |= uint32_t((p[i].w[K] & bit) != 0) << i;
    return c;
  }
  // the bits of g whose code is c
  __device__ __forceinline__ GpBits equal(const GpBits &g, uint32_t c) const {
    GpBits e = g;
#pragma unroll
    for (int i = 0; i < kRoMaxPlanes; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) e.w[k] &= (c >> i) & 1u ? p[i].w[k] : ~p[i].w[k];
    }
    return e;
  }
};

template <int KIND, int kThreads, int VERB>
__global__ void __launch_bounds__(kThreads)
k_ro_class(DevDfa d, const uint8_t *data, GpBufs b, int style, int lead, RoBufs r) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  const uint64_t planeWords = r.planeU16 / 2;
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (have) {
        uint64_t st, en;
        const int32_t v = gpLine<VERB>(tab, c, data + beg, fin - beg, style, lead != 0, st, en);
        uint32_t *word = reinterpret_cast<uint32_t *>(r.planes) + (fin >> 5);  // the line's delimiter
        for (uint32_t code = roCode(r, v); code; code &= code - 1)
          atomicOr(word + uint64_t(__ffs(int(code)) - 1) * planeWords, 1u << (fin & 31u));
      }
    });
  }
}

// b.selMasks is not a verb's bitmap here (TextHits loads one: the launcher passes the delimiters')
__global__ void __launch_bounds__(256) k_ro_size(GpBufs b, RoBufs r) {
  __shared__ unsigned long long sumBytes[4][kRoMaxBins + 1];
  __shared__ uint32_t sumLines[4][kRoMaxBins + 1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long *wb = sumBytes[wave];
  uint32_t *wl = sumLines[wave];
  // (a row's slot c is zeroed, read and zeroed again by lane c % 64 alone; the other lanes only add
  // to it, in between - one wave, whose LDS operations are carried out in order)
  for (uint32_t c = lane; c < r.nCodes; c += 64) {
    wb[c] = 0;
    wl[c] = 0;
  }
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + wave; ch < b.nChunks; ch += waves) {
    if (r.counts[ch]) {  // (uniform)
      const TextHits h(b, ch, lane);
      const RoPlanes pl(r, ch, lane);
      __threadfence_block();
      uint32_t cur = 0, curLines = 0;
      uint64_t curBytes = 0, begin = h.behind;
      auto flush = [&] {
        if (curLines) {
          if (!(r.drop && cur == 0)) atomicAdd(wb + cur, static_cast<unsigned long long>(curBytes));
          atomicAdd(wl + cur, curLines);
        }
      };
      ftEachUp(h.g.m, [&](auto word, uint64_t bit) {
        constexpr int k = decltype(word)::value;
        const uint32_t code = pl.code<k>(bit);
        const uint64_t behind = h.base + lane * 256u + uint32_t(64 * k) +
                                uint32_t(__ffsll(static_cast<long long>(bit)));
        if (code != cur) {
          flush();
          cur = code;
          curLines = 0;
          curBytes = 0;
        }
        curBytes += behind - begin;
        ++curLines;
        begin = behind;
      });
      flush();
      __threadfence_block();
    }
    for (uint32_t c = lane; c < r.nCodes; c += 64) {
      const uint64_t at = uint64_t(c) * b.nChunks + ch;
      r.sizes[at] = wb[c];
      r.lines[at] = wl[c];
      wb[c] = 0;
      wl[c] = 0;
    }
  }
}

// a workgroup per code (nChunks == 0: every count and offset is 0)
__global__ void __launch_bounds__(256)
k_ro_finish(RoBufs r, uint64_t nChunks, const uint64_t *linesFound, uint64_t *nLines,
            uint64_t *nRouted, uint64_t *binLines, uint64_t *binOffsets, uint64_t *outLen) {
  __shared__ uint64_t ws[4];
  const uint32_t code = blockIdx.x;
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 256) sum += r.lines[uint64_t(code) * nChunks + i];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint64_t mine = ws[0] + ws[1] + ws[2] + ws[3];
  if (!r.zeroCode) {  // a code is a bucket
    if (binLines) binLines[code] = mine;
    binOffsets[code] = nChunks ? r.outBases[uint64_t(code) * nChunks] : 0;
  }
  if (code == 0) {
    const uint64_t found = *linesFound;
    const uint64_t total = nChunks ? r.outBases[uint64_t(r.nCodes) * nChunks] : 0;
    if (r.zeroCode) {  // one bucket: the lines that do not match (this row) and those that do
      if (binLines) binLines[0] = found;
      binOffsets[0] = 0;
    }
    binOffsets[r.nBins + 1] = total;
    *outLen = total;
    if (nLines) *nLines = found;
    if (nRouted) *nRouted = found - (r.drop ? mine : 0);
  }
}

__global__ void __launch_bounds__(256)
k_ro_write(const uint8_t *data, GpBufs b, RoBufs r, uint8_t *out, uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    if (r.counts[ch] == 0) continue;  // (uniform)
    const TextHits h(b, ch, lane);
    const RoPlanes pl(r, ch, lane);
    for (uint32_t c0 = 0; c0 < r.nCodes; c0 += 64) {
      const uint32_t c = c0 + lane;
      uint64_t size = 0, dst = 0;
      if (c < r.nCodes) {
        size = r.sizes[uint64_t(c) * b.nChunks + ch];
        dst = r.outBases[uint64_t(c) * b.nChunks + ch];
      }
      // the codes with bytes in this chunk, one after the other, by the whole wave
      uint64_t todo = __ballot(size != 0 && dst < cap);
      while (todo) {
        const int j = __ffsll(static_cast<long long>(todo)) - 1;
        todo &= todo - 1;
        ftWriteRuns(data, h, pl.equal(h.g.m, c0 + uint32_t(j)), __shfl(dst, j), out, cap, lane);
      }
    }
  }
}

template <int KIND, int VERB>
hipError_t launchRouteClassK(const DevDfa &d, const uint8_t *data, const GpBufs &b, int style,
                             int lead, const RoBufs &r, const LaunchCfg &cfg, hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  const hipError_t e = setLds(k_ro_class<KIND, kThreads, VERB>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks = textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg);
  hipLaunchKernelGGL((k_ro_class<KIND, kThreads, VERB>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, b, style, lead, r);
  return hipGetLastError();
}
