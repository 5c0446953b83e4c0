// k_replace_text.h - sed over a raw text: every line rewritten by replace<style,doLeader> and the
// lines put back together as a text (include/Matcher.h:186-191, core :643-706, inside the line
// loop of tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_grep.h).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it - so nothing is proportional to the line
// count, and nothing waits for it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk], open[chunk], and the HIT bitmap (the selected bitmap's layout) zeroed;
//   k_rt_count      table staged once per workgroup, a wave per chunk, chunks grid-strided, rounds of
//                   64 lines (k_text.h: textLines).  A lane runs replaceLane without an output over its
//                   line; outBytes[chunk] = the sum of (rewritten length + 1) over the chunk's lines
//                   (under only_changed: over its changed lines), replCounts[chunk] = the sum of the
//                   lines' replacement counts, both u64; a line with a replacement sets its
//                   delimiter's bit in the hit bitmap;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_rt_totals     one workgroup: *n_replaced = the sum of replCounts, where the tail begins (behind
//                   the text's last delimiter), *out_len = the total (+ the tail's length);
//   k_rt_write      (skipped when the call only sizes) a wave per chunk; chunks without a line or
//                   with outBases[chunk] >= out_cap are skipped.  The chunk's source is
//                   [open[chunk], behind its last delimiter).  Per round of 64 HIT lines a lane finds
//                   its line's begin / finish (k_text.h: TextHits) and sizes it again (replaceLane, no
//                   output); the wave's exclusive prefix over (unchanged bytes in front of the line +
//                   rewritten length + 1) plus the carry of the earlier rounds places the unchanged
//                   stretch in front of every hit line and the line itself.  The stretches - and
//                   the one behind the chunk's last hit line - are copied by the WHOLE WAVE
//                   (rtCopyWave: aligned 16-byte stores, loads at whatever the shift makes them, byte
//                   stores at the two ends); then every lane writes its rewritten line and the
//                   delimiter (replaceLaneT<true>: every store below out_cap).  Under only_changed
//                   there are no stretches;
//   k_rt_tail       (not under only_changed) a grid-strided copy of the tail to its place.
// No per-line value is stored anywhere; no workgroup waits for another.  Nothing is written at or
// behind out_cap.
#pragma once

// b.selMasks = the hit bitmap; b.selCounts / b.selBases are not used here
struct RtBufs {
  uint64_t *outBytes;        // [nChunks] output bytes of the chunk's lines
  uint64_t *replCounts;      // [nChunks] replacements in the chunk's lines
  const uint64_t *outBases;  // [nChunks + 1] exclusive scan of outBytes, the total behind it
};

struct RtArgs {
  int style, lead, onlyChanged;
  uint32_t delim;
  const uint8_t *repl;
  uint64_t replLen, max;
};

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_rt_count(DevDfa d, const uint8_t *data, GpBufs b, RtBufs r, RtArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    uint64_t bytes = 0, repls = 0;
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (have) {
        uint64_t len = 0;
        const uint64_t cnt = replaceLane(tab, c, data + beg, fin - beg, a.style, a.lead != 0,
                                         a.repl, a.replLen, a.max, nullptr, len);
        if (cnt) {
          atomicOr(reinterpret_cast<uint32_t *>(b.selMasks) + (fin >> 5), 1u << (fin & 31u));
          repls += cnt;
        }
        if (cnt || !a.onlyChanged) bytes += len + 1;
      }
    });
    for (int o = 32; o; o >>= 1) {
      bytes += __shfl_xor(bytes, o);
      repls += __shfl_xor(repls, o);
    }
    if (lane == 0) {
      r.outBytes[ch] = bytes;
      r.replCounts[ch] = repls;
    }
  }
}

// one workgroup: *nReplaced = the sum of replCounts; tailAt[0] = where the tail begins (behind the
// text's last delimiter; 0 when it has none), tailAt[1] = where it goes (the lines' total);
// *outLen = that total, plus the tail's length unless only_changed drops it.  outTotal == nullptr:
// the text is empty.
__global__ void __launch_bounds__(1024)
k_rt_totals(const uint64_t *replCounts, uint64_t nChunks, const uint64_t *outTotal,
            const uint16_t *masks, const uint64_t *open, uint64_t len, int onlyChanged,
            uint64_t *tailAt, uint64_t *outLen, uint64_t *nReplaced) {
  __shared__ uint64_t ws[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 1024) sum += replCounts[i];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) ws[wave] = sum;
  uint32_t last = 0;  // 1 + the last chunk's highest delimiter bit
  if (wave == 0 && nChunks) {
    const uint32_t mine = gpLoadBits(masks, nChunks - 1, lane).last();
    last = mine ? lane * 256u + mine : 0u;
    for (int o = 32; o; o >>= 1) {
      const uint32_t v = __shfl_xor(last, o);
      last = v > last ? v : last;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t all = 0;
    for (int w = 0; w < 16; ++w) all += ws[w];
    *nReplaced = all;
    const uint64_t total = outTotal ? *outTotal : 0;
    uint64_t tail = 0;
    if (nChunks) tail = last ? (nChunks - 1) * kSplitChunk + last : open[nChunks - 1];
    tailAt[0] = tail;
    tailAt[1] = total;
    *outLen = total + (onlyChanged ? 0 : len - tail);
  }
}

// the whole wave copies src[0..n) to out[dst..dst + n), cut at cap: byte stores up to the first
// 16-byte boundary of the destination, aligned 16-byte stores (the loads are at whatever the shift
// between the two makes them - the memory pipeline splits them), byte stores behind the last
// whole piece.  Nothing is read outside src[0..n) and nothing written at or behind out + cap.
// (wave-uniform arguments)
__device__ __forceinline__ void rtCopyWave(uint8_t *out, uint64_t dst, const uint8_t *src,
                                           uint64_t n, uint64_t cap, uint32_t lane) {
  if (dst >= cap) return;
  if (n > cap - dst) n = cap - dst;
  uint8_t *q = out + dst;
  uint64_t head = (16u - (reinterpret_cast<uintptr_t>(q) & 15u)) & 15u;
  if (head > n) head = n;
  if (lane < head) q[lane] = src[lane];
  const uint64_t pieces = (n - head) >> 4;
  const uint8_t *s16 = src + head;
  uint4 *q16 = reinterpret_cast<uint4 *>(q + head);
  uint64_t i = lane;
  for (; i + 192 < pieces; i += 256) {  // four requests in flight per lane
    const uint4 v0 = *reinterpret_cast<const uint4 *>(s16 + i * 16);
    const uint4 v1 = *reinterpret_cast<const uint4 *>(s16 + (i + 64) * 16);
    const uint4 v2 = *reinterpret_cast<const uint4 *>(s16 + (i + 128) * 16);
    const uint4 v3 = *reinterpret_cast<const uint4 *>(s16 + (i + 192) * 16);
    q16[i] = v0;
    q16[i + 64] = v1;
    q16[i + 128] = v2;
    q16[i + 192] = v3;
  }
  for (; i < pieces; i += 64) q16[i] = *reinterpret_cast<const uint4 *>(s16 + i * 16);
  const uint64_t done = head + pieces * 16;
  if (lane < n - done) q[done + lane] = src[done + lane];
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_rt_write(DevDfa d, const uint8_t *data, GpBufs b, RtBufs r, RtArgs a, uint8_t *out,
           uint64_t cap) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    const uint64_t first = r.outBases[ch];
    if (first >= cap || r.outBytes[ch] == 0) continue;  // (uniform; a line gives a byte at least)
    // (h.srcEnd, behind the chunk's last delimiter, is where its source ends)
    const TextHits h(b, ch, lane);
    uint64_t srcAt = b.open[ch];  // the source behind the lines placed so far ...
    uint64_t dstAt = first;       // ... and where it goes
    for (uint32_t k0 = 0; k0 < h.s.total && dstAt < cap; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool have = k < h.s.total;
      uint64_t beg, fin;
      uint32_t index;  // (not needed here)
      h.line(h.s.select(have ? k : h.s.total - 1), beg, fin, index);  // the hit line
      // the unchanged bytes between the hit line below and this one
      uint64_t gapSrc = __shfl_up(fin, 1) + 1;
      if (lane == 0) gapSrc = srcAt;
      const uint64_t gap = have && !a.onlyChanged ? beg - gapSrc : 0;
      // the sizing walk, then the lanes' exclusive prefix over stretch + line + delimiter
      uint64_t newLen = 0;
      if (have)
        replaceLane(tab, c, data + beg, fin - beg, a.style, a.lead != 0, a.repl, a.replLen, a.max,
                    nullptr, newLen);
      const uint64_t mine = have ? gap + newLen + 1 : 0;
      uint64_t incl = mine;
      for (int sh = 1; sh < 64; sh <<= 1) {
        const uint64_t v = __shfl_up(incl, sh);
        if (lane >= uint32_t(sh)) incl += v;
      }
      const uint64_t gapDst = dstAt + (incl - mine);
      const uint32_t lastLane = (h.s.total - k0 < 64 ? h.s.total - k0 : 64u) - 1;
      srcAt = __shfl(fin, int(lastLane)) + 1;
      dstAt += __shfl(incl, 63);
      // the stretches, one after the other, by the whole wave
      uint64_t todo = __ballot(gap != 0);
      while (todo) {
        const int j = __ffsll(static_cast<long long>(todo)) - 1;
        todo &= todo - 1;
        rtCopyWave(out, __shfl(gapDst, j), data + __shfl(gapSrc, j), __shfl(gap, j), cap, lane);
      }
      // the rewritten line and its delimiter, by its lane
      const uint64_t lineDst = gapDst + gap;
      if (have && lineDst < cap) {
        const uint64_t room = cap - lineDst;
        uint64_t len2 = 0;
        replaceLaneT<true>(tab, c, data + beg, fin - beg, a.style, a.lead != 0, a.repl, a.replLen,
                           a.max, out + lineDst, room, len2);
        if (newLen < room) out[lineDst + newLen] = uint8_t(a.delim);
      }
    }
    // the unchanged lines behind the chunk's last hit line
    if (!a.onlyChanged) rtCopyWave(out, dstAt, data + srcAt, h.srcEnd - srcAt, cap, lane);
  }
}

// the tail (data[tailAt[0]..len)) to out + tailAt[1], cut at cap: rtCopyWave's pieces, grid-strided
__global__ void __launch_bounds__(256)
k_rt_tail(const uint8_t *data, uint64_t len, const uint64_t *tailAt, uint8_t *out, uint64_t cap) {
  const uint64_t from = tailAt[0], dst = tailAt[1];
  if (dst >= cap || from >= len) return;
  uint64_t n = len - from;
  if (n > cap - dst) n = cap - dst;
  const uint8_t *src = data + from;
  uint8_t *q = out + dst;
  uint64_t head = (16u - (reinterpret_cast<uintptr_t>(q) & 15u)) & 15u;
  if (head > n) head = n;
  const uint64_t pieces = (n - head) >> 4;
  const uint64_t done = head + pieces * 16;
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) q[threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x < n - done) q[done + threadIdx.x] = src[done + threadIdx.x];
  }
  uint4 *q16 = reinterpret_cast<uint4 *>(q + head);
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < pieces; i += step)
    q16[i] = *reinterpret_cast<const uint4 *>(src + head + i * 16);
}

template <int KIND>
hipError_t launchReplaceTextK(const DevDfa &d, const uint8_t *data, const GpBufs &b,
                              const RtBufs &r, const RtArgs &a, bool count, uint8_t *out,
                              uint64_t cap, const LaunchCfg &cfg, hipStream_t stream) {
  // threads and resident workgroups by k_text.h's rule (textBlocks): the count pass as k_ct_count,
  // the write pass - two chunk views, the prefix and the stretch beside replaceCore - at 512
  // threads under the LDS placements so that it does not spill (DESIGN 4.3h has the report)
  constexpr int kThreads = kStagedThreads<KIND>;
  constexpr int kWriteThreads = kStagedLds<KIND> ? 512 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_rt_count<KIND, kThreads>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_rt_write<KIND, kWriteThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  if (count) {
    hipLaunchKernelGGL((k_rt_count<KIND, kThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg)), dim3(kThreads),
                       ldsBytes, stream, d, data, b, r, a);
  } else {
    hipLaunchKernelGGL((k_rt_write<KIND, kWriteThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kWriteThreads, cfg)),
                       dim3(kWriteThreads), ldsBytes, stream, d, data, b, r, a, out, cap);
  }
  return hipGetLastError();
}
