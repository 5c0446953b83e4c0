// k_dedup_text.h - awk '!seen[$k]++' over a raw text: every line has at most one KEY, a byte string
// inside it, and the lines chosen by their keys' strings - the first line of each string whose
// number of occurrences lies in [min_count, max_count], or under invert every other keyed line -
// are put together as a text (sort -u -k in text order, uniq -u, uniq -d; under invert
// awk 'seen[$k]++').  The key is the line (WHOLE), the line when search<style,doLeader> selects it
// (LINES: k_uniq_text.h's item), the key_index-th piece k_extract_text.h emits for the line (MATCH),
// or the key_index-th field k_fields_text.h cuts it into (FIELD)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_uniq_text.h, whose
// table it keeps, and k_filter_text.h, whose run copy writes the output).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h); the KEYED and
//                   the MARK bitmap (one bit per byte of the text, the delimiter bitmap's layout)
//                   zeroed (a memset on the stream);
//   k_uq_zero       (k_uniq_text.h, as it stands) the hash table and the counters zeroed;
//   k_dedup_text    the only pass that walks bytes: k_uniq_text's walk with ONE item per line.  Table
//                   staged once per workgroup (WHOLE stages none: no DFA is walked), a wave per
//                   chunk, chunks grid-strided, rounds of 64 lines.  A lane finds its line's key
//                   [a, e): LINES runs gpLine, MATCH counts collectLane's callbacks up to key_index
//                   and leaves the chain, FIELD keeps the end of the previous separator in a register
//                   and takes [e_(k-1), a_k) at the key_index-th separator - behind which the line is
//                   left - or [e_(k-1), line end) when the chain ends one separator short.  A keyed
//                   line ors its delimiter's bit into KEYED and inserts its key as k_uniq_text does
//                   (uqHash, uqFront, uqInsert; the front flushed by uqFlush);
//   k_dd_mark       no table of the DFA from here on.  A thread per slot: an occupied slot is counted
//                   (*n_distinct, one atomic per workgroup); one whose count lies in
//                   [min_count, max_count] finds the line of its `first` - the delimiter bitmap is
//                   scanned forward from bit `first`, the first word masked, then word by word, to
//                   the first set bit: the key lies in [line begin, delimiter], so that is the line's
//                   own delimiter (an empty key at the line's end sits ON it) - and ors that bit
//                   into MARK.  Lines never share a bit and a string has one `first`: one mark per
//                   string;
//   k_dd_emit       a wave per chunk, a lane's 256 bits of the three bitmaps in registers:
//                   EMIT = (invert ? KEYED & ~MARK : MARK) | (keep_unkeyed ? DELIM & ~KEYED : 0),
//                   stored over MARK; emitBytes[chunk], emitLines[chunk] as k_ft_mark leaves them
//                   (ftStoreEmit);
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_ft_totals     (k_filter_text.h, as it stands) *n_emitted, *out_len;
//   k_ft_write      (likewise; skipped when the call only sizes) the runs of emitted lines copied by
//                   ftWriteRuns, cut at out_cap.
// No per-line value is stored anywhere but the two bitmaps; no workgroup waits for another; every
// loop is bounded by the table's size, a key's or a line's length, a lane's 256 bits or the chunk
// count.  Nothing is read outside data[0, len) - a key is a range of its line - and nothing is
// written at or behind out_cap.  A dropped key (2^24 bytes or longer, or the table is full) leaves
// its line keyed and not marked; a mark comes from a record, whose count and first offset are exact
// whatever was dropped.
//
// scratch (kernels.hip: DedupScratch): 16 bytes per slot, three bitmaps of len / 8 bytes (rounded
// up to whole chunks), 40 bytes per chunk, 8 per 1,024 chunks and 72, rounded up to 16.
#pragma once

constexpr int kDdWhole = 0, kDdLines = 1, kDdLinesMatch = 2, kDdMatch = 3, kDdField = 4;  // MODE

// where the front begins: behind the DFA's table, or - WHOLE stages none - at the LDS's first byte
template <int KIND, int MODE>
__host__ __device__ inline size_t dedupLdsOff(const DevDfa &d) {
  return MODE == kDdWhole ? 0 : tallyLdsOff<KIND>(d);
}

// the key data[a, e) of the line data[beg, fin): false = the line is unkeyed
template <int MODE, class T>
__device__ __forceinline__ bool ddKey(const T &tab, const LaneCtx &c, const uint8_t *data,
                                      uint64_t beg, uint64_t fin, int style, int lead,
                                      uint64_t keyIndex, uint64_t &a, uint64_t &e) {
  bool keyed = false;
  if constexpr (MODE == kDdMatch) {
    uint64_t left = keyIndex;
    collectLane(tab, c, data + beg, fin - beg, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
      if (--left) return true;
      a = beg + at;
      e = beg + mE;
      keyed = true;
      return false;
    });
  } else if constexpr (MODE == kDdField) {
    // `seen` separators so far, the last of them ended at prev
    uint64_t seen = 0, prev = 0;
    collectLane(tab, c, data + beg, fin - beg, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
      if (++seen == keyIndex) {
        a = beg + prev;
        e = beg + at;
        keyed = true;
        return false;
      }
      prev = mE;
      return true;
    });
    if (!keyed && seen + 1 == keyIndex) {  // the line's last field
      a = beg + prev;
      e = fin;
      keyed = true;
    }
  } else {
    uint64_t st, en;
    const int32_t r = gpLine<MODE == kDdLines ? kSearch : kMatch>(tab, c, data + beg, fin - beg,
                                                                  style, lead != 0, st, en);
    a = beg;
    e = fin;
    keyed = r > 0;
  }
  return keyed;
}

// keyOf(beg, fin, a, e): the line's key.  o.nItems counts the keyed lines.
template <int kThreads, class K>
__device__ __forceinline__ void ddWalk(const uint8_t *data, uint64_t len, const GpBufs &b,
                                       const UqOut &o, uint32_t *keyedBits,
                                       unsigned long long *keys, uint32_t *counts, K &&keyOf) {
  const uint32_t L = o.ldsSlots;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  uint64_t items = 0, dropped = 0;  // this lane's
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (!have) return;
      uint64_t a = 0, e = 0;
      if (!keyOf(beg, fin, a, e)) return;
      atomicOr(keyedBits + (fin >> 5), 1u << (fin & 31u));
      ++items;
      const uint64_t n = e - a;
      if (n >= kUqMaxItem) {
        ++dropped;
        return;
      }
      const uint64_t h = uqHash(data, len, a, n);
      if (uqFront(keys, counts, L, data, len, a, n, h)) return;
      if (!uqInsert(o, data, len, a, n, h, 1ull)) ++dropped;
    });
  }
  for (int sh = 32; sh; sh >>= 1) items += __shfl_xor(items, sh);
  if (lane == 0 && items) atomicAdd(o.nItems, static_cast<unsigned long long>(items));
  dropped += uqFlush<kThreads>(o, data, len, keys, counts, L);
  for (int sh = 32; sh; sh >>= 1) dropped += __shfl_xor(dropped, sh);
  if (lane == 0 && dropped) atomicAdd(o.nDropped, static_cast<unsigned long long>(dropped));
}

template <int KIND, int kThreads, int MODE>
__global__ void __launch_bounds__(kThreads)
k_dedup_text(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, int style, int lead,
             uint64_t keyIndex, UqOut o, uint32_t *keyedBits) {
  extern __shared__ __align__(16) uint8_t lds[];
  unsigned long long *keys =
      reinterpret_cast<unsigned long long *>(lds + dedupLdsOff<KIND, MODE>(d));
  uint32_t *counts = reinterpret_cast<uint32_t *>(keys + o.ldsSlots);
  const uint32_t L = o.ldsSlots;
  // (zeroed in front of stageTab's barrier, or of WHOLE's own)
  for (uint32_t i = threadIdx.x; i < L; i += kThreads) {
    keys[i] = 0;
    counts[i] = 0;
    counts[L + i] = 0;  // (the tags)
  }
  if constexpr (MODE == kDdWhole) {
    __syncthreads();
    ddWalk<kThreads>(data, len, b, o, keyedBits, keys, counts,
                     [&](uint64_t beg, uint64_t fin, uint64_t &a, uint64_t &e) {
      a = beg;
      e = fin;
      return true;
    });
  } else {
    const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
    const LaneCtx c = gpCtx<KIND>(d, lds);
    ddWalk<kThreads>(data, len, b, o, keyedBits, keys, counts,
                     [&](uint64_t beg, uint64_t fin, uint64_t &a, uint64_t &e) {
      return ddKey<MODE>(tab, c, data, beg, fin, style, lead, keyIndex, a, e);
    });
  }
}

// per occupied slot: counted for *nDistinct; with its count in [minCount, maxCount] the bit of the
// delimiter at or behind `first` - its line's - set in the MARK bitmap.  nWords: the bitmaps' words
__global__ void __launch_bounds__(256)
k_dd_mark(const unsigned long long *table, uint64_t slots, uint64_t minCount, uint64_t maxCount,
          const uint32_t *delimBits, uint64_t nWords, uint32_t *markBits,
          unsigned long long *nDistinct) {
  __shared__ uint32_t waveOccupied[4];
  const uint64_t step = uint64_t(gridDim.x) * 256;
  uint32_t occupied = 0;  // (a thread sees fewer than 2^32 slots)
  for (uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x; s < slots; s += step) {
    const unsigned long long k = table[2 * s];
    if (!k) continue;
    ++occupied;
    const unsigned long long count = table[2 * s + 1];
    if (count < minCount || count > maxCount) continue;
    const uint64_t first = (k >> 24) - 1;
    uint64_t w = first >> 5;
    if (w >= nWords) continue;  // (no key begins behind the text)
    uint32_t x = delimBits[w] & (~0u << (first & 31u));
    while (!x && ++w < nWords) x = delimBits[w];
    if (x) atomicOr(markBits + w, x & (0u - x));  // (a key's line has its delimiter)
  }
  for (int o = 32; o; o >>= 1) occupied += __shfl_xor(occupied, o);
  if ((threadIdx.x & 63u) == 0) waveOccupied[threadIdx.x >> 6] = occupied;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long all = static_cast<unsigned long long>(waveOccupied[0]) +
                                   waveOccupied[1] + waveOccupied[2] + waveOccupied[3];
    if (all) atomicAdd(nDistinct, all);
  }
}

// b.selMasks = the MARK bitmap: its bits are read first, and the chunk's EMIT bits stored over them
__global__ void __launch_bounds__(256)
k_dd_emit(GpBufs b, const uint16_t *keyedBits, int invert, int keepUnkeyed, uint64_t *emitBytes,
          uint32_t *emitLines) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    const TextHits h(b, ch, lane);  // (h.s: the MARK bits)
    const GpBits keyed = gpLoadBits(keyedBits, ch, lane);
    GpBits e;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e.w[k] = invert ? keyed.w[k] & ~h.s.m.w[k] : h.s.m.w[k];
      if (keepUnkeyed) e.w[k] |= h.g.m.w[k] & ~keyed.w[k];
    }
    // the emitted lines' bytes, from behind the delimiter below (h.behind for the lane's first) to
    // their own
    uint64_t bytes = 0, begin = h.behind;
    uint32_t lines = 0;
    ftEachUp(h.g.m, [&](auto word, uint64_t bit) {
      constexpr int k = decltype(word)::value;
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

template <int KIND, int MODE>
hipError_t launchDedupK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                        int style, int lead, uint64_t keyIndex, const UqOut &o, uint32_t *keyedBits,
                        const LaunchCfg &cfg, hipStream_t stream) {
  // LINES: k_uniq_text's geometry (launchUniqK).  MATCH and FIELD carry the piece count and the
  // key's span beside collectLane's chain: under the LDS placements they run 768 threads, as
  // k_fd_size and k_sum_text do, and keep out of private memory (profiles/dedup_text_resources.md).
  // WHOLE has no table: 1,024 threads around the front alone, two workgroups a CU
  constexpr bool kChain = MODE == kDdMatch || MODE == kDdField;
  constexpr int kThreads = MODE == kDdWhole ? 1024
                           : kChain         ? (kStagedLds<KIND> ? 768 : 256)
                                            : kStagedThreads<KIND>;
  const size_t ldsBytes = dedupLdsOff<KIND, MODE>(d) + size_t(o.ldsSlots) * 16 + 16;
  const hipError_t e = setLds(k_dedup_text<KIND, kThreads, MODE>, ldsBytes);
  if (e != hipSuccess) return e;
  uint32_t blocks;
  if constexpr (MODE == kDdWhole) {
    const uint64_t want = (b.nChunks + kThreads / 64 - 1) / (kThreads / 64);
    const uint64_t most = uint64_t(cfg.numCUs) * 2;
    blocks = uint32_t(want > most ? most : want);
  } else {
    blocks = textBlocks<KIND>(b.nChunks, 512 + ldsTableBytes<KIND>(d), kThreads, cfg);
  }
  hipLaunchKernelGGL((k_dedup_text<KIND, kThreads, MODE>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, len, b, style, lead, keyIndex, o, keyedBits);
  return hipGetLastError();
}
