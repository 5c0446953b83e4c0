// k_group_text.h - awk '{ n[$k]++; s[$k] += $v; if ($v > m[$k]) m[$k] = $v }' over a raw text: every
// line has at most one KEY and at most one VALUE, two items of the same line, and per distinct key
// STRING one record leaves the chip - where it first appears, its length, how many lines carry it,
// and the count, sum, minimum and maximum of those lines' numbers.  An item is a piece
// k_extract_text.h emits for the line (MATCH) or a field k_fields_text.h cuts it into (FIELD)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_uniq_text.h, whose
// table, front and ordering pass it keeps, k_sum_text.h, whose number readers it uses, and
// k_dedup_text.h, whose walk it follows).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h), the FIRST
//                   bitmap zeroed;
//   k_uq_zero       (k_uniq_text.h, as it stands) the hash table and three counters zeroed;
//   k_gr_zero       the side array emptied (count 0, sum 0, min ~0, max 0) and *n_numeric zeroed;
//   k_group_text    the only pass that walks bytes: k_dedup_text's walk with TWO items per line.  ONE
//                   collectLane chain per line; the callback keeps the key's span and the value's
//                   span in registers as the chain passes them and leaves the chain behind the later
//                   of the two (FIELD: either may be the line's last field, which ends at the line's
//                   end).  A keyed line hashes its key (uqHash), reads its value's number (smFirst /
//                   smLast) and inserts: the count first, then - a numeric line - the four statistics
//                   beside the slot that holds the key;
//   k_uq_mark / k_uq_pop / k_scan_*   (as they stand) the records' order: first appearance;
//   k_gr_emit       per occupied slot its rank (uqRank) and, below the cap, the record's seven
//                   values; *n_distinct.
// The global table keeps k_uniq_text.h's two words per slot; the statistics live in a side array
// [4][slots] indexed by the slot uqInsertSlot returns - a slot's string never changes and a slot is
// never given up, so the slot an insert returns is the string's for good, and four native 64-bit
// atomics (add, add, umin, umax) on its cells are all a numeric line costs there.
// The LDS front: k_uniq_text.h's (key, 32-bit count, 32-bit tag) slots with four 64-bit statistics
// beside each, 48 bytes a slot, sized by the same share rule (groupLdsSlotsK).  A line whose key has
// a place there costs LDS atomics only.  The front is flushed once, at workgroup end: the count
// through uqInsertSlot, weighted, and then the statistics onto the slot it returned.  A slot whose
// flush finds the table full drops its whole count, and none of its numbers are counted numeric: an
// item is either wholly in its key's record or dropped.
// No lane waits for another; every loop is bounded by the table's size, an item's or a line's length,
// or the chunk count.  Nothing is read outside data[0, len) - both items are ranges of their line -
// and nothing is written at or behind cap.
//
// scratch (kernels.hip: GroupScratch): 16 + 32 bytes per slot, the two bitmaps (len / 4, rounded up
// to whole chunks), k_uniq_text.h's 164 bytes per chunk, 8 per 1,024 chunks and 72, rounded up to 16.
#pragma once

constexpr uint32_t kGrLdsSlots = 256;  // 48 bytes each: at most 16 KiB of front per workgroup
constexpr int kGrMatch = 0, kGrField = 1;  // MODE

struct GrOut {
  unsigned long long *table;  // [2 * slots]: key, count (k_uniq_text.h)
  unsigned long long *side;   // [4][slots]: numeric count, sum, min, max
  uint64_t slots;             // a power of two
  unsigned long long *nKeyed, *nDropped, *nNumeric;  // zeroed on the stream
  uint32_t ldsSlots;          // L: a power of two, or 0
};

// the slots the workgroup's share of the LDS has room for behind the table (uniqLdsSlotsK's rule):
// a power of two, 48 bytes each
template <int KIND>
__host__ inline uint32_t groupLdsSlotsK(const DevDfa &d) {
  const size_t share = size_t(160) * 1024 / tallyPerCu<KIND>(d);
  const size_t used = tallyLdsOff<KIND>(d) + 16;
  const size_t room = share > used ? (share - used) / 48 : 0;
  uint32_t l = kGrLdsSlots;
  while (l && l > room) l >>= 1;
  return l >= kUqLdsMin ? l : 0;
}

// empties the side array (n = 0: nothing of it) and zeroes the numeric counter
__global__ void __launch_bounds__(256)
k_gr_zero(unsigned long long *side, uint64_t n, unsigned long long *nNumeric) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += step) {
    side[i] = 0;
    side[n + i] = 0;
    side[2 * n + i] = ~0ull;
    side[3 * n + i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *nNumeric = 0;
}

// the key data[a, e) and the value data[va, ve) of the line data[beg, fin): false = the line is
// unkeyed; valued = the line has a valueIndex-th item.  last = max(keyIndex, valueIndex): the chain
// is left behind its last-th piece (MATCH) or separator (FIELD)
template <int MODE, class T>
__device__ __forceinline__ bool grItems(const T &tab, const LaneCtx &c, const uint8_t *data,
                                        uint64_t beg, uint64_t fin, uint64_t keyIndex,
                                        uint64_t valueIndex, uint64_t last, uint64_t &a,
                                        uint64_t &e, uint64_t &va, uint64_t &ve, bool &valued) {
  bool keyed = false;
  valued = false;
  uint64_t seen = 0;  // pieces (MATCH) or separators (FIELD) so far
  if constexpr (MODE == kGrMatch) {
    collectLane(tab, c, data + beg, fin - beg, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
      ++seen;
      if (seen == keyIndex) {
        a = beg + at;
        e = beg + mE;
        keyed = true;
      }
      if (seen == valueIndex) {
        va = beg + at;
        ve = beg + mE;
        valued = true;
      }
      return seen < last;
    });
  } else {
    uint64_t prev = 0;  // where the last separator ended
    collectLane(tab, c, data + beg, fin - beg, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
      ++seen;
      if (seen == keyIndex) {
        a = beg + prev;
        e = beg + at;
        keyed = true;
      }
      if (seen == valueIndex) {
        va = beg + prev;
        ve = beg + at;
        valued = true;
      }
      prev = mE;
      return seen < last;
    });
    if (seen < last) {  // the chain ended with the line: field seen + 1 is the line's last
      if (seen + 1 == keyIndex) {
        a = beg + prev;
        e = fin;
        keyed = true;
      }
      if (seen + 1 == valueIndex) {
        va = beg + prev;
        ve = fin;
        valued = true;
      }
    }
  }
  return keyed;
}

// `count` numeric lines of the string in global slot s: their sum, minimum and maximum
__device__ __forceinline__ void grStats(const GrOut &o, uint64_t s, unsigned long long count,
                                        unsigned long long sum, unsigned long long lo,
                                        unsigned long long hi) {
  unsigned long long *p = o.side + s;
  atomicAdd(p, count);
  atomicAdd(p + o.slots, sum);
  atomicMin(p + 2 * o.slots, lo);
  atomicMax(p + 3 * o.slots, hi);
}

template <int KIND, int kThreads, int MODE>
__global__ void __launch_bounds__(kThreads)
k_group_text(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, uint64_t keyIndex,
             uint64_t valueIndex, int which, GrOut o) {
  extern __shared__ __align__(16) uint8_t lds[];
  // the front: keys[L], stats[L][4], counts[L], tags[L]
  const uint32_t L = o.ldsSlots;
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds + tallyLdsOff<KIND>(d));
  unsigned long long *stats = keys + L;
  uint32_t *counts = reinterpret_cast<uint32_t *>(stats + 4u * size_t(L));
  // (emptied in front of stageTab's barrier)
  for (uint32_t i = threadIdx.x; i < L; i += kThreads) {
    keys[i] = 0;
    stats[4u * i] = 0;
    stats[4u * i + 1] = 0;
    stats[4u * i + 2] = ~0ull;
    stats[4u * i + 3] = 0;
    counts[i] = 0;
    counts[L + i] = 0;  // (the tags)
  }
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  const uint64_t last = keyIndex > valueIndex ? keyIndex : valueIndex;
  uint64_t keyedLines = 0, dropped = 0, numericLines = 0;  // this lane's
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (!have) return;
      uint64_t a = 0, e = 0, va = 0, ve = 0;
      bool valued;
      if (!grItems<MODE>(tab, c, data, beg, fin, keyIndex, valueIndex, last, a, e, va, ve, valued))
        return;
      ++keyedLines;
      const uint64_t n = e - a;
      if (n >= kUqMaxItem) {
        ++dropped;
        return;
      }
      const uint64_t h = uqHash(data, len, a, n);
      uint64_t v = 0;
      const bool numeric = valued && (which == kSumLast ? smLast(data, len, va, ve, v)
                                                        : smFirst(data, len, va, ve, v));
      const uint32_t fs = uqFrontSlot(keys, counts, L, data, len, a, n, h);
      if (fs != kUqNoFront) {
        if (numeric) {
          unsigned long long *p = stats + 4u * fs;
          atomicAdd(p, 1ull);
          atomicAdd(p + 1, static_cast<unsigned long long>(v));
          atomicMin(p + 2, static_cast<unsigned long long>(v));
          atomicMax(p + 3, static_cast<unsigned long long>(v));
        }
        return;
      }
      const uint64_t s = uqInsertSlot(o.table, o.slots, data, len, a, n, h, 1ull);
      if (s == kUqNoSlot) {
        ++dropped;
        return;
      }
      if (numeric) {
        grStats(o, s, 1ull, v, v, v);
        ++numericLines;
      }
    });
  }
  // the front through the global insert, weighted by its counts; the statistics follow the count
  if (L) {  // (uniform)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < L; i += kThreads) {
      const unsigned long long k = keys[i];
      if (!k) continue;
      const uint64_t a = (k >> 24) - 1, n = k & (kUqMaxItem - 1);
      const uint64_t s = uqInsertSlot(o.table, o.slots, data, len, a, n, counts[L + i], counts[i]);
      if (s == kUqNoSlot) {
        dropped += counts[i];
        continue;
      }
      const unsigned long long cnt = stats[4u * i];
      if (!cnt) continue;
      grStats(o, s, cnt, stats[4u * i + 1], stats[4u * i + 2], stats[4u * i + 3]);
      numericLines += cnt;
    }
  }
  for (int sh = 32; sh; sh >>= 1) {
    keyedLines += __shfl_xor(keyedLines, sh);
    dropped += __shfl_xor(dropped, sh);
    numericLines += __shfl_xor(numericLines, sh);
  }
  if (lane == 0) {
    if (keyedLines) atomicAdd(o.nKeyed, static_cast<unsigned long long>(keyedLines));
    if (dropped) atomicAdd(o.nDropped, static_cast<unsigned long long>(dropped));
    if (numericLines) atomicAdd(o.nNumeric, static_cast<unsigned long long>(numericLines));
  }
}

// per occupied slot: its record's rank (k_uniq_text.h: uqRank) and, when the rank is below the cap,
// the record's seven values - stats has four rows of `cap` cells; *nDistinct = the scan's total
__global__ void __launch_bounds__(256)
k_gr_emit(const unsigned long long *table, const unsigned long long *side, uint64_t slots,
          const uint32_t *firstBits, const uint64_t *popBases, const uint16_t *lanePre,
          uint64_t nChunks, uint64_t cap, uint64_t *first, uint64_t *length, uint64_t *count,
          uint64_t *stats, uint64_t *nDistinct) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *nDistinct = popBases[nChunks];
  if (!cap || (!first && !length && !count && !stats)) return;  // (uniform)
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x; s < slots; s += step) {
    const unsigned long long k = table[2 * s];
    if (!k) continue;
    const uint64_t at = (k >> 24) - 1;
    const uint64_t rank = uqRank(at, firstBits, popBases, lanePre, cap);
    if (rank >= cap) continue;
    if (first) first[rank] = at;
    if (length) length[rank] = k & (kUqMaxItem - 1);
    if (count) count[rank] = table[2 * s + 1];
    if (stats) {
#pragma unroll
      for (int row = 0; row < 4; ++row) stats[row * cap + rank] = side[row * slots + s];
    }
  }
}

template <int KIND, int MODE>
hipError_t launchGroupK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                        uint64_t keyIndex, uint64_t valueIndex, int which, const GrOut &o,
                        const LaunchCfg &cfg, hipStream_t stream) {
  // resident workgroups by k_text.h's rule (textBlocks) for k_ct_count's LDS; the front fits in what
  // that rule leaves of the LDS (groupLdsSlotsK).  Beside collectLane's chain a lane carries two
  // spans, the item count and its bound: under the LDS placements 768 threads, as k_dedup_text's
  // MATCH and FIELD and k_sum_text, and no private memory (profiles/group_text_resources.md)
  constexpr int kThreads = kStagedLds<KIND> ? 768 : 256;
  const size_t ldsBytes = tallyLdsOff<KIND>(d) + size_t(o.ldsSlots) * 48 + 16;
  const hipError_t e = setLds(k_group_text<KIND, kThreads, MODE>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks =
      textBlocks<KIND>(b.nChunks, 512 + ldsTableBytes<KIND>(d), kThreads, cfg);
  hipLaunchKernelGGL((k_group_text<KIND, kThreads, MODE>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, len, b, keyIndex, valueIndex, which, o);
  return hipGetLastError();
}
