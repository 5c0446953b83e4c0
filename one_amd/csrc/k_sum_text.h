// k_sum_text.h - awk '{ n[c]++; s[c] += $x; if ($x > m[c]) m[c] = $x }' over a raw text: per result
// the count, sum, minimum and maximum of the decimal numbers found in the matches - four 64-bit
// words per slot leave the chip, nothing else (Red::collect, lib/Red.cpp:103-116, inside the line
// loop of tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_extract_text.h,
// whose xtLoad8 it uses, and k_tally_text.h, whose LDS layout rule it uses).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk] (unused here), open[chunk]; no selected / hit bitmap exists;
//   k_sm_zero       the caller's slots emptied (count 0, sum 0, min ~0, max 0; not under
//                   accumulate) and the two counters zeroed;
//   k_sum_text      ONE pass: table staged once per workgroup, a wave per chunk, chunks
//                   grid-strided, rounds of 64 lines (k_text.h: textLines).  A lane runs collectLane
//                   with the four-argument callback (the item is the span extract_text emits, its
//                   slot the result collect_text reports), and only when an item's span [a, e) is
//                   known does it read those bytes again for the digits (smFirst / smLast).
// The number: the first (FIRST) or last (LAST) maximal run of bytes 0x30..0x39 INSIDE the span, read
// as an unsigned decimal; an item without a digit, or whose run is 2^64 or more, is counted among
// the items and enters no statistic.  FIRST reads forward from the span's begin and stops behind the
// run; LAST reads backward from the span's end and stops in front of the run, 16 bytes a request -
// either way the cost follows the distance to the run and the run's length, not the span's length.
// Overflow is seen while accumulating, in 64 bits: FIRST compares with (2^64 - 1) / 10 before it
// multiplies, LAST adds digit * 10^k (k <= 19) and looks at the carry.
// The statistics: slots [0, L) are (count, sum, min, max) of 64-bit words in LDS behind the table
// (where k_tally_text.h keeps its counters: the same 16 KiB at most, so that the residency of
// textBlocks' rule holds), emptied before the first round and flushed ONCE at workgroup end - a slot
// with a count costs four 64-bit global atomics (add, add, umin, umax).  Slots at or above L, and
// the "everything else" slot when it lies beyond L, go straight to global memory with the same four.
// Everything is 64-bit, so no text is too long for the LDS front.
// The hot slot does not serialise the wave (k_tally_text.h: tallyWave's reason): a lane carries
// (slot, count, sum, min, max) along its line and flushes on a change of slot; the runs the lanes end
// their lines with are peeled per round - the first pending lane's slot, a ballot of the lanes equal
// to it, the four values reduced across those lanes by shuffles, ONE set of atomics.  kTallyPeel
// slots are peeled so; what is left goes by per-lane atomics where the slot is in LDS, and is peeled
// to the end where it is in global memory.
// plain = 1 is the form without any of that (four atomics per item), kept to be measured against.
#pragma once

constexpr uint32_t kSumLdsBins = 512;  // at most 16 KiB of statistics per workgroup
constexpr int kSumFirst = 0, kSumLast = 1;  // WHICH
constexpr uint64_t kSumMax10 = 1844674407370955161ull;  // (2^64 - 1) / 10; (2^64 - 1) % 10 == 5

struct SumOut {
  unsigned long long *stats;  // [4][nBins + 1]: count, sum, min, max
  unsigned long long *nItems, *nNumeric;  // zeroed on the stream
  uint64_t stride;            // nBins + 1
  uint32_t nBins;             // <= 2^31
  uint32_t ldsBins;           // L: the slots kept in LDS
};

// the slots the workgroup's share of the LDS has room for behind the table (k_tally_text.h:
// tallyLdsBinsK's room rule), 32 bytes each; a multiple of 4
template <int KIND>
__host__ inline uint32_t sumLdsBinsK(const DevDfa &d) {
  const size_t share = size_t(160) * 1024 / tallyPerCu<KIND>(d);
  const size_t used = tallyLdsOff<KIND>(d) + 16;
  const size_t room = share > used ? (share - used) / 32 : 0;
  return uint32_t(room < kSumLdsBins ? room : kSumLdsBins) & ~3u;
}

// empties the slots (n = 0: none) and zeroes the two counters
__global__ void __launch_bounds__(256)
k_sm_zero(unsigned long long *stats, uint64_t n, unsigned long long *nItems,
          unsigned long long *nNumeric) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += step) {
    stats[i] = 0;
    stats[n + i] = 0;
    stats[2 * n + i] = ~0ull;
    stats[3 * n + i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *nItems = 0;
    *nNumeric = 0;
  }
}

// the first run of digits of data[a, e): false = there is none, or it is 2^64 or more.  16 bytes a
// request as walkBytes makes them, but ONE request in flight: walkBytes' four would cost the lane
// twelve registers more beside the chain's own, and the run is a few bytes away as a rule.
__device__ __forceinline__ bool smFirst(const uint8_t *data, uint64_t len, uint64_t a, uint64_t e,
                                        uint64_t &v) {
  uint64_t val = 0;
  uint32_t st = 0;  // 0 = no digit yet, 1 = in the run, 2 = too large
  auto step = [&](uint32_t byte) -> bool {
    const uint32_t dg = byte - 0x30u;
    if (dg > 9u) return st == 0;  // (behind the run: done)
    if (val > kSumMax10 || (val == kSumMax10 && dg > 5u)) {
      st = 2;
      return false;
    }
    val = val * 10u + dg;
    st = 1;
    return true;
  };
  uint64_t pos = a;
  while (pos < e) {
    const uint64_t rem = e - pos;
    bool on = true;
    if (rem >= 16) {
      const uint4 w = *reinterpret_cast<const uint4 *>(data + pos);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (on) on = step((words[i >> 2] >> (8 * (i & 3))) & 0xffu);
      }
      pos += 16;
    } else {
      const uint32_t take = rem < 8 ? uint32_t(rem) : 8u;
      const uint64_t w = xtLoad8(data, len, pos, take);
      for (uint32_t i = 0; i < take && on; ++i) on = step(uint32_t(w >> (8u * i)) & 0xffu);
      pos += take;
    }
    if (!on) break;
  }
  v = val;
  return st == 1;
}

// the last run of digits of data[a, e), read from the back: digit k from the right adds
// digit * 10^k.  Below k = 19 the sum stays below 10^(k + 1) <= 10^19; at k = 19 a digit above 1 is
// too large and a 1 may carry out of 64 bits; from k = 20 on only zeros fit.
__device__ __forceinline__ bool smLast(const uint8_t *data, uint64_t len, uint64_t a, uint64_t e,
                                       uint64_t &v) {
  uint64_t val = 0, pw = 1;
  uint32_t k = 0, st = 0;  // k = digits taken (saturating at 20); st as smFirst's
  auto step = [&](uint32_t byte) -> bool {
    const uint32_t dg = byte - 0x30u;
    if (dg > 9u) return st == 0;  // (in front of the run: done)
    st = 1;
    if (dg) {
      const uint64_t add = dg * pw;
      val += add;
      if (k > 19u || (k == 19u && dg > 1u) || val < add) {
        st = 2;
        return false;
      }
    }
    if (k < 19u) pw *= 10u;
    if (k < 20u) ++k;
    return true;
  };
  uint64_t pos = e;
  while (pos > a) {
    const uint64_t rem = pos - a;
    if (rem >= 16) {
      // (inside the span: a <= pos - 16)
      const uint4 w = *reinterpret_cast<const uint4 *>(data + pos - 16);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
      bool on = true;
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        if (on) on = step((words[i >> 2] >> (8 * (i & 3))) & 0xffu);
      }
      if (!on) break;
      pos -= 16;
    } else {
      const uint32_t take = rem < 8 ? uint32_t(rem) : 8u;
      const uint64_t w = xtLoad8(data, len, pos - take, take);
      bool on = true;
      for (uint32_t i = take; i-- && on;) on = step(uint32_t(w >> (8u * i)) & 0xffu);
      if (!on) break;
      pos -= take;
    }
  }
  v = val;
  return st == 1;
}

// one group of numeric items of one slot.  A group that goes to global memory is also counted in
// the workgroup's numeric items here; one that goes to the front is counted when the front is
// flushed.
__device__ __forceinline__ void sumAdd(const SumOut &o, unsigned long long *front,
                                       unsigned long long *wgNumeric, uint32_t slot,
                                       unsigned long long count, unsigned long long sum,
                                       unsigned long long lo, unsigned long long hi) {
  if (slot < o.ldsBins) {
    unsigned long long *p = front + 4u * slot;
    atomicAdd(p, count);
    atomicAdd(p + 1, sum);
    atomicMin(p + 2, lo);
    atomicMax(p + 3, hi);
  } else {
    unsigned long long *p = o.stats + slot;
    atomicAdd(p, count);
    atomicAdd(p + o.stride, sum);
    atomicMin(p + 2 * o.stride, lo);
    atomicMax(p + 3 * o.stride, hi);
    // (last, so that the two branches do not end alike: the compiler then merges their final
    // atomics into ONE on a pointer of either address space, a flat atomic)
    atomicAdd(wgNumeric, count);
  }
}

// the wave's pending groups (every lane calls; pending = count != 0): k_tally_text.h's tallyWave
// with four values to reduce instead of one weight.  A slot that one lane alone holds needs no
// reduction.
__device__ __forceinline__ void sumWave(const SumOut &o, unsigned long long *front,
                                        unsigned long long *wgNumeric, uint32_t lane,
                                        uint32_t slot, uint64_t count, uint64_t sum, uint64_t lo,
                                        uint64_t hi) {
  bool pending = count != 0;
  uint64_t pend = __ballot(pending);
  auto peel = [&] {
    const int first = __ffsll(static_cast<long long>(pend)) - 1;
    const uint32_t s = __shfl(slot, first);
    const bool same = pending && slot == s;
    const uint64_t sameMask = __ballot(same);
    uint64_t c = same ? count : 0, t = same ? sum : 0, l = same ? lo : ~0ull, h = same ? hi : 0;
    if (sameMask & (sameMask - 1)) {  // (uniform)
      for (int sh = 32; sh; sh >>= 1) {
        c += __shfl_xor(c, sh);
        t += __shfl_xor(t, sh);
        const uint64_t l2 = __shfl_xor(l, sh), h2 = __shfl_xor(h, sh);
        l = l2 < l ? l2 : l;
        h = h2 > h ? h2 : h;
      }
    }
    if (int(lane) == first) sumAdd(o, front, wgNumeric, s, c, t, l, h);
    pending = pending && !same;
    pend &= ~sameMask;
  };
#pragma unroll
  for (int p = 0; p < kTallyPeel; ++p) {
    if (!pend) return;  // (uniform)
    peel();
  }
  if (pending && slot < o.ldsBins) {
    sumAdd(o, front, wgNumeric, slot, count, sum, lo, hi);
    pending = false;
  }
  pend = __ballot(pending);
  while (pend) peel();  // (uniform)
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_sum_text(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, int which, uint64_t maxPer,
           int plain, SumOut o) {
  extern __shared__ __align__(16) uint8_t lds[];
  unsigned long long *front = reinterpret_cast<unsigned long long *>(lds + tallyLdsOff<KIND>(d));
  // (behind the front: the workgroup's items and its numeric items)
  unsigned long long *wgItems = front + 4u * size_t(o.ldsBins);
  unsigned long long *wgNumeric = wgItems + 1;
  // (emptied in front of stageTab's barrier)
  for (uint32_t i = threadIdx.x; i < o.ldsBins; i += kThreads) {
    front[4u * i] = 0;
    front[4u * i + 1] = 0;
    front[4u * i + 2] = ~0ull;
    front[4u * i + 3] = 0;
  }
  if (threadIdx.x == 0) {
    *wgItems = 0;
    *wgNumeric = 0;
  }
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  uint64_t items = 0;  // this lane's
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      // the run the lane carries along its line
      // (a run of 2^32 - 1 items is flushed as a change of slot is)
      uint32_t runSlot = 0, run = 0;
      uint64_t runSum = 0, runLo = ~0ull, runHi = 0;
      uint64_t left = maxPer;
      if (have && left) {
        collectLane(tab, c, data + beg, fin - beg,
                    [&](uint32_t accS, uint64_t, uint64_t mE, uint64_t at) {
          ++items;
          uint64_t v;
          const bool numeric = which == kSumLast ? smLast(data, len, beg + at, beg + mE, v)
                                                 : smFirst(data, len, beg + at, beg + mE, v);
          if (numeric) {
            const int32_t r = c.res[accS];
            const uint32_t slot = uint32_t(r) < o.nBins ? uint32_t(r) : o.nBins;
            if (plain) sumAdd(o, front, wgNumeric, slot, 1ull, v, v, v);
            else {
              if (run && (slot != runSlot || run == ~0u)) {
                sumAdd(o, front, wgNumeric, runSlot, run, runSum, runLo, runHi);
                run = 0;
                runSum = 0;
                runLo = ~0ull;
                runHi = 0;
              }
              runSlot = slot;
              ++run;
              runSum += v;
              runLo = v < runLo ? v : runLo;
              runHi = v > runHi ? v : runHi;
            }
          }
          return --left != 0;
        });
      }
      if (!plain) sumWave(o, front, wgNumeric, lane, runSlot, run, runSum, runLo, runHi);
    });
  }
  for (int sh = 32; sh; sh >>= 1) items += __shfl_xor(items, sh);
  if (lane == 0 && items) atomicAdd(wgItems, static_cast<unsigned long long>(items));
  __syncthreads();
  uint64_t flushed = 0;  // the numeric items this thread takes out of the front
  for (uint32_t i = threadIdx.x; i < o.ldsBins; i += kThreads) {
    const unsigned long long n = front[4u * i];
    if (!n) continue;
    flushed += n;
    unsigned long long *p = o.stats + i;
    atomicAdd(p, n);
    atomicAdd(p + o.stride, front[4u * i + 1]);
    atomicMin(p + 2 * o.stride, front[4u * i + 2]);
    atomicMax(p + 3 * o.stride, front[4u * i + 3]);
  }
  for (int sh = 32; sh; sh >>= 1) flushed += __shfl_xor(flushed, sh);
  if (lane == 0 && flushed) atomicAdd(wgNumeric, static_cast<unsigned long long>(flushed));
  __syncthreads();
  if (threadIdx.x == 0) {
    if (*wgItems) atomicAdd(o.nItems, *wgItems);
    if (*wgNumeric) atomicAdd(o.nNumeric, *wgNumeric);
  }
}

template <int KIND>
hipError_t launchSumK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                      int which, uint64_t maxPer, int plain, const SumOut &o,
                      const LaunchCfg &cfg, hipStream_t stream) {
  // resident workgroups by k_text.h's rule (textBlocks) for k_ct_count's LDS; the front fits in
  // what that rule leaves of the LDS (sumLdsBinsK), so the rule holds here as well.  Under the LDS
  // placements 768 threads, not kStagedThreads' 1,024: beside the chain a lane carries its run
  // (slot, count, sum, min, max), the pieces left and the item count, about 150 registers against the
  // 128 of a 1,024-thread workgroup - 12 waves a CU without private memory instead of 16 with it,
  // as k_fields_text.h's sizing pass (profiles/sum_text_resources.md)
  constexpr int kThreads = kStagedLds<KIND> ? 768 : 256;
  const size_t ldsBytes = tallyLdsOff<KIND>(d) + size_t(o.ldsBins) * 32 + 16;
  const hipError_t e = setLds(k_sum_text<KIND, kThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks =
      textBlocks<KIND>(b.nChunks, 512 + ldsTableBytes<KIND>(d), kThreads, cfg);
  hipLaunchKernelGGL((k_sum_text<KIND, kThreads>), dim3(blocks), dim3(kThreads), ldsBytes, stream,
                     d, data, len, b, which, maxPer, plain, o);
  return hipGetLastError();
}
