// k_tally_text.h - grep -c per result over a raw text (or grep -o | sort | uniq -c): how many
// lines, or how many matches, report each result - a histogram, nothing else leaves the chip
// (Red::collect, lib/Red.cpp:103-116, or search<style,doLeader>, include/Matcher.h:557-640, inside
// the line loop of tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_collect_text.h;
// DESIGN 4.3i).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk] (unused here), open[chunk]; no selected / hit bitmap exists;
//   k_tl_zero       the caller's bins zeroed (not under accumulate) and the item count zeroed;
//   k_tally_text    ONE pass: table staged once per workgroup, a wave per chunk, chunks
//                   grid-strided, rounds of 64 lines (k_text.h: textLines).  A lane runs
//                   gpLine<VERB> (LINES: one item per line, its value the line's result) or
//                   collectLane (MATCHES: one item per match) and counts its items by value.
// The histogram: bins [0, L) are 32-bit counters in LDS behind the table (where k_scan_marked and
// k_lists put their extra areas), zeroed before the first round and flushed ONCE at workgroup end
// - a non-zero slot costs one 64-bit global atomic.  Values at or above L, and the "everything
// else" slot when it lies beyond L, go straight to global memory with 64-bit atomics.
// The hot bin does not serialise the wave (a wave's adds to ONE LDS word are taken one by one):
//   LINES    value 0 - the lines that do not match, 99 % of a log - is counted with a ballot into
//            a register and added once per wave; of the rest, per round, kTallyPeel values are
//            peeled: the first pending lane's value, a ballot of the lanes equal to it, ONE add
//            of the popcount; what is left goes by per-lane atomics where the counter is in LDS,
//            and is peeled to the end where it is in global memory (tallyWave);
//   MATCHES  a lane carries (value, run length) along its line and adds on change; the pairs the
//            lanes end their lines with are peeled the same way, weighted by their runs.
// plain = 1 is the form without any of that (an atomic per item), kept to be measured against:
// level with this one while the counters are in LDS, 1.3x (MATCHES) to 8x (LINES) slower where a
// hot one is not.
#pragma once

constexpr uint32_t kTallyLdsBins = 4096;  // at most 16 KiB of counters per workgroup
constexpr int kTallyPeel = 2;
constexpr int kTallyLines = 0, kTallyLinesMatch = 1, kTallyMatches = 2;  // MODE

struct TallyOut {
  unsigned long long *bins;    // [nBins + 1]
  unsigned long long *nItems;  // zeroed on the stream
  uint32_t nBins;              // <= 2^31
  uint32_t ldsBins;            // L: the bins kept in LDS
};

// the resident workgroups k_common.h's rule (stagedPerCu) gives k_ct_count for this DFA, and the
// LDS a workgroup may take without lowering them
template <int KIND>
__host__ inline uint64_t tallyPerCu(const DevDfa &d) {
  return stagedPerCu<KIND>(512 + ldsTableBytes<KIND>(d));
}

// where the counters begin, and what follows them: 16 bytes (the workgroup's item count)
template <int KIND>
__host__ __device__ inline size_t tallyLdsOff(const DevDfa &d) {
  return 512 + ((ldsTableBytes<KIND>(d) + 15) & ~size_t(15));
}

template <int KIND>
__host__ inline uint32_t tallyLdsBinsK(const DevDfa &d) {
  const size_t share = size_t(160) * 1024 / tallyPerCu<KIND>(d);
  const size_t used = tallyLdsOff<KIND>(d) + 16;
  const size_t room = share > used ? share - used : 0;
  // (a multiple of 4, so that what follows the counters stays 16-byte aligned)
  return uint32_t(room / 4 < kTallyLdsBins ? room / 4 : kTallyLdsBins) & ~3u;
}

__global__ void __launch_bounds__(256)
k_tl_zero(unsigned long long *bins, uint64_t n, unsigned long long *nItems) {
  const uint64_t step = uint64_t(gridDim.x) * 256;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += step) bins[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *nItems = 0;
}

// one item group: `count` items of value r.  A 32-bit LDS counter cannot overflow before the
// flush: the launcher keeps counters in LDS only for texts below 4 GiB, an item has a byte of its
// own (a line its delimiter, a match of collectLane at least the byte it ends behind), so ALL the
// items of the text are fewer than 2^32.
__device__ __forceinline__ void tallyAdd(const TallyOut &o, uint32_t *hist, int32_t r,
                                         uint32_t count) {
  const uint32_t slot = uint32_t(r) < o.nBins ? uint32_t(r) : o.nBins;
  if (slot < o.ldsBins) atomicAdd(hist + slot, count);
  else atomicAdd(o.bins + slot, static_cast<unsigned long long>(count));
}

// the wave's pending (value, weight) pairs (every lane calls; UNIT: every weight is 1).
// kTallyPeel values are taken out with one add each.  Of what is left, the lanes whose counter is
// in LDS add on their own - adds to different LDS words run side by side - and the lanes whose
// counter is in global memory go on peeling until none is left: 64-bit global atomics on one word
// are taken one at a time by the whole device (measured: 0.18 G adds/s on three words, DESIGN
// 4.3i), a round costs at most one per distinct value this way.
template <bool UNIT>
__device__ __forceinline__ void tallyWave(const TallyOut &o, uint32_t *hist, uint32_t lane,
                                          bool pending, int32_t r, uint32_t weight) {
  uint64_t pend = __ballot(pending);
  auto peel = [&] {
    const int first = __ffsll(static_cast<long long>(pend)) - 1;
    const int32_t v = __shfl(r, first);
    const bool same = pending && r == v;
    const uint64_t sameMask = __ballot(same);
    uint32_t sum;
    if constexpr (UNIT) sum = uint32_t(__popcll(sameMask));
    else {
      sum = same ? weight : 0u;
      for (int sh = 32; sh; sh >>= 1) sum += __shfl_xor(sum, sh);
    }
    if (int(lane) == first) tallyAdd(o, hist, v, sum);
    pending = pending && !same;
    pend &= ~sameMask;
  };
#pragma unroll
  for (int p = 0; p < kTallyPeel; ++p) {
    if (!pend) return;  // (uniform)
    peel();
  }
  const uint32_t slot = uint32_t(r) < o.nBins ? uint32_t(r) : o.nBins;
  if (pending && slot < o.ldsBins) {
    tallyAdd(o, hist, r, weight);
    pending = false;
  }
  pend = __ballot(pending);
  while (pend) peel();  // (uniform)
}

template <int KIND, int kThreads, int MODE>
__global__ void __launch_bounds__(kThreads)
k_tally_text(DevDfa d, const uint8_t *data, GpBufs b, int style, int lead, int plain, TallyOut o) {
  extern __shared__ __align__(16) uint8_t lds[];
  uint32_t *hist = reinterpret_cast<uint32_t *>(lds + tallyLdsOff<KIND>(d));
  unsigned long long *wgItems = reinterpret_cast<unsigned long long *>(
      lds + tallyLdsOff<KIND>(d) + ((size_t(o.ldsBins) * 4 + 15) & ~size_t(15)));
  // (zeroed in front of stageTab's barrier)
  for (uint32_t i = threadIdx.x; i < o.ldsBins; i += kThreads) hist[i] = 0;
  if (threadIdx.x == 0) *wgItems = 0;
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  uint64_t items = 0;  // this lane's items of value > 0 (LINES) / matches (MATCHES)
  uint64_t zeros = 0;  // LINES: the wave's lines of value 0 (uniform)
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if constexpr (MODE == kTallyMatches) {
        int32_t runVal = 0;
        uint32_t run = 0;
        if (have) {
          items += collectLane(tab, c, data + beg, fin - beg,
                               [&](uint32_t accS, uint64_t, uint64_t) {
            const int32_t r = c.res[accS];
            if (plain) tallyAdd(o, hist, r, 1u);
            else if (run && r == runVal) ++run;
            else {
              if (run) tallyAdd(o, hist, runVal, run);
              runVal = r;
              run = 1;
            }
            return true;
          });
        }
        if (!plain) tallyWave<false>(o, hist, lane, run != 0, runVal, run);
      } else {
        int32_t r = 0;
        if (have) {
          uint64_t st, en;
          r = gpLine<MODE == kTallyLines ? kSearch : kMatch>(tab, c, data + beg, fin - beg, style,
                                                             lead != 0, st, en);
          items += r > 0;
        }
        if (plain) {
          if (have) tallyAdd(o, hist, r, 1u);
        } else {
          zeros += uint64_t(__popcll(__ballot(have && r == 0)));
          tallyWave<true>(o, hist, lane, have && r != 0, r, 1u);
        }
      }
    });
  }
  if (MODE != kTallyMatches && !plain && lane == 0 && zeros) {
    // value 0 lands in slot 0 whatever nBins is (nBins == 0: slot 0 IS "everything else"); the
    // wave's zeros are below 2^32 as all items are, see tallyAdd
    if (o.ldsBins) atomicAdd(hist, uint32_t(zeros));
    else atomicAdd(o.bins, static_cast<unsigned long long>(zeros));
  }
  for (int sh = 32; sh; sh >>= 1) items += __shfl_xor(items, sh);
  if (lane == 0 && items) atomicAdd(wgItems, static_cast<unsigned long long>(items));
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < o.ldsBins; i += kThreads) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(o.bins + i, static_cast<unsigned long long>(v));
  }
  if (threadIdx.x == 0 && *wgItems) atomicAdd(o.nItems, *wgItems);
}

template <int KIND, int MODE>
hipError_t launchTallyK(const DevDfa &d, const uint8_t *data, const GpBufs &b, int style, int lead,
                        int plain, const TallyOut &o, const LaunchCfg &cfg, hipStream_t stream) {
  // threads and resident workgroups by k_text.h's rule (textBlocks) for k_ct_count's LDS; the
  // counters fit in what that rule leaves of the LDS (tallyLdsBinsK), so the rule holds here as well
  constexpr int kThreads = kStagedThreads<KIND>;
  const size_t ldsBytes = tallyLdsOff<KIND>(d) + ((size_t(o.ldsBins) * 4 + 15) & ~size_t(15)) + 16;
  const hipError_t e = setLds(k_tally_text<KIND, kThreads, MODE>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks =
      textBlocks<KIND>(b.nChunks, 512 + ldsTableBytes<KIND>(d), kThreads, cfg);
  hipLaunchKernelGGL((k_tally_text<KIND, kThreads, MODE>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, b, style, lead, plain, o);
  return hipGetLastError();
}
