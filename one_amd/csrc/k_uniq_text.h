// k_uniq_text.h - grep -o | sort | uniq -c keyed by the matched BYTES (or grep | sort | uniq -c: by
// the selected line): which strings occur in a raw text and how often - one record per distinct
// byte string leaves the chip, in the order of first appearance (Red::collect, lib/Red.cpp:103-116,
// or search<style,doLeader>, include/Matcher.h:557-640, inside the line loop of
// tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_extract_text.h,
// whose xtLoad8 it uses).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   open[chunk], and the FIRST bitmap (one bit per byte of the text, the delimiter
//                   bitmap's layout) zeroed;
//   k_uq_zero       the hash table and the counters zeroed;
//   k_uniq_text     ONE pass: table staged once per workgroup, a wave per chunk, chunks
//                   grid-strided, rounds of 64 lines (k_text.h: textLines).  A lane runs
//                   gpLine<VERB> (LINES: the item is a selected line) or collectLane (MATCHES: the
//                   item is the span extract_text emits).  Only when an item's span [a, e) is known
//                   does the lane read those bytes again, hash them (uqHash) and insert;
//   k_uq_mark       per occupied slot bit `first` of the FIRST bitmap set: distinct strings have
//                   distinct first offsets;
//   k_uq_pop        per 16 KiB chunk the popcount of its part of that bitmap, and per 256 bytes of
//                   the chunk the set bits in front of them (u16);
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) popBases[chunk] = records in front of
//                   the chunk, popBases[nChunks] = n_distinct;
//   k_uq_emit       per occupied slot rank = popBases[chunk] + the set bits in front of its own
//                   (the 256 bytes' count and at most eight words of the bitmap); record `rank` is
//                   written when rank < cap; *n_distinct.
// The hash table (open addressing, linear probing, no deletion): a slot is two 64-bit words,
// key = (start + 1) << 24 | length (0 = empty) and count.  An empty slot is claimed with ONE
// atomicCAS of the key, which carries everything a reader needs; an occupied one is compared -
// the length, then the text's bytes at the key's start against the item's own.  Equal: atomicAdd
// of the count, and atomicMin of the key when the item begins in front of it (equal strings have
// equal lengths, so the minimum of the packed word is the minimum start, and any representative
// serves a compare - a stale key is as good as a fresh one).  Unequal: the next slot.  A slot's
// string never changes, so two lanes with one string walk the same slots and meet in the first
// that either claims.  No lane waits for another: every loop is bounded by the table's size or by
// the item's length; an item that finds neither its string nor an empty slot in `slots` probes is
// counted in *n_dropped.
// The LDS front: a workgroup keeps L (key, 32-bit count, 32-bit tag) slots behind the DFA table
// (where k_tally_text.h keeps its bins, sized by the same rule so that it never lowers residency;
// L = 0 when the table leaves no room, for texts of 4 GiB and more, and under plain).  An item
// tries kUqFrontProbes slots there first; one that finds no place goes to the global table
// directly.  The tag is the hash's low 32 bits, written by the lane that claimed the slot: a slot
// whose tag differs is passed over without a look at the text, so an item that does not belong
// in the front costs LDS reads and no memory access.  A tag read as 0 - the slot was claimed a
// moment ago, by another lane of the same wave as a rule - decides nothing: the bytes are
// compared.  The tag is also all of the hash the global insert needs (the table has at most 2^32
// slots), so the flush reads no text to hash it again.
// The front is flushed once, at workgroup end, through the global insert, weighted by its counts.
#pragma once

constexpr uint32_t kUqLdsSlots = 1024;  // at most 16 KiB of front per workgroup
constexpr uint32_t kUqLdsMin = 64;  // a front of fewer slots is not worth its flush: none then
constexpr uint32_t kUqFrontProbes = 2;
constexpr uint64_t kUqMaxItem = 1ull << 24;  // items of this length and more are dropped
constexpr int kUqLines = 0, kUqLinesMatch = 1, kUqMatches = 2;  // MODE

struct UqOut {
  unsigned long long *table;  // [2 * slots]: key, count
  uint64_t slots;             // a power of two
  unsigned long long *nItems, *nDropped;  // zeroed on the stream
  uint32_t ldsSlots;          // L: a power of two, or 0
};

// where the front begins (k_tally_text.h: tallyLdsOff) and the slots the workgroup's share of the
// LDS has room for behind the table: a power of two, 16 bytes each
template <int KIND>
__host__ inline uint32_t uniqLdsSlotsK(const DevDfa &d) {
  const size_t share = size_t(160) * 1024 / tallyPerCu<KIND>(d);
  const size_t used = tallyLdsOff<KIND>(d) + 16;
  const size_t room = share > used ? (share - used) / 16 : 0;
  uint32_t l = kUqLdsSlots;
  while (l && l > room) l >>= 1;
  return l >= kUqLdsMin ? l : 0;
}

// `take` (1..8) bytes of the text from s, the rest of the word zero
__device__ __forceinline__ uint64_t uqLoad(const uint8_t *data, uint64_t len, uint64_t s,
                                           uint32_t take) {
  const uint64_t v = xtLoad8(data, len, s, take);
  return take < 8 ? v & ((1ull << (8u * take)) - 1) : v;
}

// the hash of data[a, a + n): the bytes read again, eight at a time
__device__ __forceinline__ uint64_t uqHash(const uint8_t *data, uint64_t len, uint64_t a,
                                           uint64_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (n * 0xFF51AFD7ED558CCDull);
  auto mix = [&](uint64_t w) {
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  };
  uint64_t i = 0;
  // (a long item: four loads in flight; a + i + 32 <= a + n <= len)
  for (; i + 32 <= n; i += 32) {
    const uint64_t *q = reinterpret_cast<const uint64_t *>(data + a + i);
    const uint64_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    mix(w0);
    mix(w1);
    mix(w2);
    mix(w3);
  }
  for (; i < n; i += 8) {
    const uint32_t take = n - i < 8 ? uint32_t(n - i) : 8u;
    h = (h ^ uqLoad(data, len, a + i, take)) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  }
  return h ^ (h >> 32);
}

// data[x, x + n) == data[y, y + n)
__device__ __forceinline__ bool uqEqual(const uint8_t *data, uint64_t len, uint64_t x, uint64_t y,
                                        uint64_t n) {
  if (x == y) return true;
  for (uint64_t i = 0; i < n; i += 8) {
    const uint32_t take = n - i < 8 ? uint32_t(n - i) : 8u;
    if (uqLoad(data, len, x + i, take) != uqLoad(data, len, y + i, take)) return false;
  }
  return true;
}

__device__ __forceinline__ unsigned long long uqKey(uint64_t a, uint64_t n) {
  return ((a + 1) << 24) | n;
}

constexpr uint64_t kUqNoSlot = ~0ull;  // (no table has this many slots)

// `weight` occurrences of data[a, a + n), hash h, the earliest of them at a: the slot that holds the
// string now, or kUqNoSlot = the table is full and does not hold it
__device__ __forceinline__ uint64_t uqInsertSlot(unsigned long long *table, uint64_t slots,
                                                 const uint8_t *data, uint64_t len, uint64_t a,
                                                 uint64_t n, uint64_t h,
                                                 unsigned long long weight) {
  const unsigned long long mine = uqKey(a, n);
  const uint64_t mask = slots - 1;
  uint64_t s = h & mask;
  for (uint64_t probe = 0; probe < slots; ++probe, s = (s + 1) & mask) {
    unsigned long long *slot = table + 2 * s;
    unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) k = atomicCAS(slot, 0ull, mine);
    if (k == 0) {
      atomicAdd(slot + 1, weight);
      return s;
    }
    if ((k & (kUqMaxItem - 1)) == n && uqEqual(data, len, (k >> 24) - 1, a, n)) {
      atomicAdd(slot + 1, weight);
      if (mine < k) atomicMin(slot, mine);
      return s;
    }
  }
  return kUqNoSlot;
}

// the same for a caller that needs no slot: false = the table is full and does not hold the string
__device__ __forceinline__ bool uqInsert(const UqOut &o, const uint8_t *data, uint64_t len,
                                         uint64_t a, uint64_t n, uint64_t h,
                                         unsigned long long weight) {
  return uqInsertSlot(o.table, o.slots, data, len, a, n, h, weight) != kUqNoSlot;
}

constexpr uint32_t kUqNoFront = ~0u;

// one occurrence of data[a, a + n) into the workgroup's front: the front's slot that counted it, or
// kUqNoFront = no place within kUqFrontProbes slots (or there is no front)
__device__ __forceinline__ uint32_t uqFrontSlot(unsigned long long *keys, uint32_t *counts,
                                                uint32_t L, const uint8_t *data, uint64_t len,
                                                uint64_t a, uint64_t n, uint64_t h) {
  if (!L) return kUqNoFront;
  const unsigned long long mine = uqKey(a, n);
  // (the slot from the hash's high bits: the global slot takes the low ones)
  volatile uint32_t *tags = counts + L;
  const uint32_t tag = uint32_t(h);
  uint32_t s = uint32_t(h >> 40) & (L - 1);
  for (uint32_t probe = 0; probe < kUqFrontProbes; ++probe, s = (s + 1) & (L - 1)) {
    unsigned long long k = *reinterpret_cast<volatile unsigned long long *>(keys + s);
    if (k == 0) {
      k = atomicCAS(keys + s, 0ull, mine);
      if (k == 0) {
        tags[s] = tag;
        atomicAdd(counts + s, 1u);
        return s;
      }
    }
    const uint32_t t = tags[s];
    if ((t == tag || t == 0) && (k & (kUqMaxItem - 1)) == n &&
        uqEqual(data, len, (k >> 24) - 1, a, n)) {
      atomicAdd(counts + s, 1u);
      if (mine < k) atomicMin(keys + s, mine);
      return s;
    }
  }
  return kUqNoFront;
}

// the same for a caller that needs no slot: false = no place (or there is no front)
__device__ __forceinline__ bool uqFront(unsigned long long *keys, uint32_t *counts, uint32_t L,
                                        const uint8_t *data, uint64_t len, uint64_t a, uint64_t n,
                                        uint64_t h) {
  return uqFrontSlot(keys, counts, L, data, len, a, n, h) != kUqNoFront;
}

// the workgroup's front flushed through the global insert, weighted by its counts (every thread
// calls, at workgroup end): the occurrences of this thread's slots that found no place
template <int kThreads>
__device__ __forceinline__ uint64_t uqFlush(const UqOut &o, const uint8_t *data, uint64_t len,
                                            const unsigned long long *keys, const uint32_t *counts,
                                            uint32_t L) {
  uint64_t dropped = 0;
  if (L) {  // (uniform)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < L; i += kThreads) {
      const unsigned long long k = keys[i];
      if (!k) continue;
      const uint64_t a = (k >> 24) - 1, n = k & (kUqMaxItem - 1);
      if (!uqInsert(o, data, len, a, n, counts[L + i], counts[i])) dropped += counts[i];
    }
  }
  return dropped;
}

// zeroes the table (two words per slot) and the four counters
__global__ void __launch_bounds__(256)
k_uq_zero(unsigned long long *table, uint64_t words, unsigned long long *nItems,
          unsigned long long *nDropped, uint64_t *nDistinct) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < words; i += step) table[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *nItems = 0;
    *nDropped = 0;
    *nDistinct = 0;
  }
}

template <int KIND, int kThreads, int MODE>
__global__ void __launch_bounds__(kThreads)
k_uniq_text(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, int style, int lead,
            uint64_t maxPer, UqOut o) {
  extern __shared__ __align__(16) uint8_t lds[];
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds + tallyLdsOff<KIND>(d));
  uint32_t *counts = reinterpret_cast<uint32_t *>(keys + o.ldsSlots);
  const uint32_t L = o.ldsSlots;
  // (zeroed in front of stageTab's barrier)
  for (uint32_t i = threadIdx.x; i < L; i += kThreads) {
    keys[i] = 0;
    counts[i] = 0;
    counts[L + i] = 0;  // (the tags)
  }
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  uint64_t items = 0, dropped = 0;  // this lane's
  // the item data[a, e)
  auto item = [&](uint64_t a, uint64_t e) {
    ++items;
    const uint64_t n = e - a;
    if (n >= kUqMaxItem) {
      ++dropped;
      return;
    }
    const uint64_t h = uqHash(data, len, a, n);
    if (uqFront(keys, counts, L, data, len, a, n, h)) return;
    if (!uqInsert(o, data, len, a, n, h, 1ull)) ++dropped;
  };
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (!have) return;
      if constexpr (MODE == kUqMatches) {
        uint64_t left = maxPer;
        if (left)
          collectLane(tab, c, data + beg, fin - beg,
                      [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
            item(beg + at, beg + mE);
            return --left != 0;
          });
      } else {
        uint64_t st, en;
        const int32_t r = gpLine<MODE == kUqLines ? kSearch : kMatch>(tab, c, data + beg, fin - beg,
                                                                      style, lead != 0, st, en);
        if (r > 0) item(beg, fin);
      }
    });
  }
  for (int sh = 32; sh; sh >>= 1) items += __shfl_xor(items, sh);
  if (lane == 0 && items) atomicAdd(o.nItems, static_cast<unsigned long long>(items));
  dropped += uqFlush<kThreads>(o, data, len, keys, counts, L);
  for (int sh = 32; sh; sh >>= 1) dropped += __shfl_xor(dropped, sh);
  if (lane == 0 && dropped) atomicAdd(o.nDropped, static_cast<unsigned long long>(dropped));
}

// per occupied slot: bit `first` of the FIRST bitmap (the delimiter bitmap's layout)
__global__ void __launch_bounds__(256)
k_uq_mark(const unsigned long long *table, uint64_t slots, uint32_t *firstBits) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x; s < slots; s += step) {
    const unsigned long long k = table[2 * s];
    if (!k) continue;
    const uint64_t first = (k >> 24) - 1;
    atomicOr(firstBits + (first >> 5), 1u << (first & 31u));
  }
}

// per chunk: the set bits of its part of the FIRST bitmap, and per lane (256 bits) those of the
// chunk in front of the lane's
__global__ void __launch_bounds__(256)
k_uq_pop(const uint16_t *firstBits, uint64_t nChunks, uint64_t *pops, uint16_t *lanePre) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < nChunks; ch += waves) {
    GpChunk g;
    g.m = gpLoadBits(firstBits, ch, lane);
    g.scan(lane);
    lanePre[ch * 64 + lane] = uint16_t(g.excl);  // (below 16,384)
    if (lane == 0) pops[ch] = g.total;
  }
}

// the rank of the record whose string first appears at `at` = the strings that first appear in front
// of it; a value at or above cap may be short of the rank (the caller writes nothing then)
__device__ __forceinline__ uint64_t uqRank(uint64_t at, const uint32_t *firstBits,
                                           const uint64_t *popBases, const uint16_t *lanePre,
                                           uint64_t cap) {
  uint64_t rank = popBases[at / kSplitChunk];
  if (rank >= cap) return rank;
  // the chunk's bits in front of the 256 the bit is among, those words in front of the bit's
  // own, then the bits below it
  rank += lanePre[at >> 8];
  const uint64_t w0 = (at >> 8) << 3, w1 = at >> 5;
  for (uint64_t w = w0; w < w1; ++w) rank += uint32_t(__popc(firstBits[w]));
  rank += uint32_t(__popc(firstBits[w1] & ((1u << (at & 31u)) - 1u)));
  return rank;
}

// per occupied slot: its record's rank (uqRank), and the record when the rank is below the cap;
// *nDistinct = the scan's total
__global__ void __launch_bounds__(256)
k_uq_emit(const unsigned long long *table, uint64_t slots, const uint32_t *firstBits,
          const uint64_t *popBases, const uint16_t *lanePre, uint64_t nChunks, uint64_t cap,
          uint64_t *first,
          uint64_t *length, uint64_t *count, uint64_t *nDistinct) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *nDistinct = popBases[nChunks];
  if (!cap || (!first && !length && !count)) return;  // (uniform)
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
  }
}

template <int KIND, int MODE>
hipError_t launchUniqK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                       int style, int lead, uint64_t maxPer, const UqOut &o, const LaunchCfg &cfg,
                       hipStream_t stream) {
  // threads and resident workgroups by k_text.h's rule (textBlocks) for k_ct_count's LDS; the
  // front fits in what that rule leaves of the LDS (uniqLdsSlotsK), so the rule holds here as well
  constexpr int kThreads = kStagedThreads<KIND>;
  const size_t ldsBytes = tallyLdsOff<KIND>(d) + size_t(o.ldsSlots) * 16 + 16;
  const hipError_t e = setLds(k_uniq_text<KIND, kThreads, MODE>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks =
      textBlocks<KIND>(b.nChunks, 512 + ldsTableBytes<KIND>(d), kThreads, cfg);
  hipLaunchKernelGGL((k_uniq_text<KIND, kThreads, MODE>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, len, b, style, lead, maxPer, o);
  return hipGetLastError();
}
