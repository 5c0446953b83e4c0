// k_grep.h - grep over a raw text: the lines that contain the pattern, as compact records in text
// order (include/Red.h:65 "searchInstant() - appropriate for grep"; tools/skim_red.cpp:36-46's loop
// over the lines lib/Util.cpp:109-130 cuts, search<style,doLeader> of include/Matcher.h:557-640 per
// line)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_text.h).
//
// The lines are driven from the split's delimiter bitmap (k_text.h), so nothing is proportional to
// the line count and nothing waits for it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h), and the
//                   SELECTED bitmap zeroed;
//   k_gp_select     table staged once per workgroup, then a WAVE per chunk, chunks grid-strided,
//                   rounds of 64 lines (k_text.h: textLines).  No LDS beside the table.  The lane
//                   walks its line (searchLane, or what launchBatch's normalisation makes of it)
//                   however long it is, and sets the line's bit in the selected bitmap (atomic or,
//                   at the line's delimiter); selCounts[chunk] = lines selected;
//   k_split_scan    again, over selCounts: selBases[chunk] = records in front of the chunk;
//   k_gp_total      *n_selected = min(total, max_count);
//   k_gp_write      (skipped when the call only counts) a wave per chunk again, over the SELECTED
//                   bitmap; record index = selBases[chunk] + rank, placed when below min(cap,
//                   max_count); line / begin / finish from the delimiter bitmap (k_text.h:
//                   TextHits - rank and predecessor of the bit inside the lane that holds it) and
//                   bases / open; the Outcome by walking the selected line again - under invert it
//                   is (0, 0, 0) and nothing is walked.
// No workgroup waits for another: the order of the records comes from the passes.
#pragma once

template <int KIND, int kThreads, int VERB>
__global__ void __launch_bounds__(kThreads)
k_gp_select(DevDfa d, const uint8_t *data, GpBufs b, int style, int lead, int invert) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    uint32_t selected = 0;
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      bool sel = false;
      if (have) {
        uint64_t st, en;
        const int32_t r = gpLine<VERB>(tab, c, data + beg, fin - beg, style, lead != 0, st, en);
        sel = (r > 0) != (invert != 0);
        if (sel) {
          const uint64_t bit = fin;  // the line's delimiter
          atomicOr(reinterpret_cast<uint32_t *>(b.selMasks) + (bit >> 5), 1u << (bit & 31u));
        }
      }
      selected += uint32_t(__popcll(__ballot(sel)));
    });
    if (lane == 0) b.selCounts[ch] = selected;
  }
}

__global__ void __launch_bounds__(64)
k_gp_total(const uint64_t *total, uint64_t maxCount, uint64_t *nSelected) {
  if (threadIdx.x == 0) *nSelected = *total < maxCount ? *total : maxCount;
}

struct GpOut {
  uint64_t limit;  // records to place: min(cap, max_count)
  uint64_t *line, *begin, *finish;
  int32_t *result;
  uint64_t *start, *end;
};

// walk = the Outcome is wanted and comes from the lane function (not under invert)
template <int KIND, int kThreads, int VERB>
__global__ void __launch_bounds__(kThreads)
k_gp_write(DevDfa d, const uint8_t *data, GpBufs b, int style, int lead, int walk, GpOut out) {
  extern __shared__ __align__(16) uint8_t lds[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  // (without a walk nothing of the table is touched, and the launch asks for no LDS)
  const Tab<KIND> tab = walk ? stageTab<KIND, kThreads>(d, lds) : Tab<KIND>(nullptr, nullptr, 0);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    const uint64_t first = b.selBases[ch];
    if (first >= out.limit || b.selCounts[ch] == 0) continue;  // (uniform)
    const TextHits h(b, ch, lane);
    for (uint32_t k0 = 0; k0 < h.s.total && first + k0 < out.limit; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool have = k < h.s.total;
      uint64_t beg, fin;
      uint32_t index;
      h.line(h.s.select(have ? k : h.s.total - 1), beg, fin, index);  // the selected line
      const uint64_t rec = first + k;
      if (have && rec < out.limit) {  // (every lane is back at the next round's shuffles)
        if (out.line) out.line[rec] = b.bases[ch] + index;
        if (out.begin) out.begin[rec] = beg;
        if (out.finish) out.finish[rec] = fin;
        int32_t r = 0;
        uint64_t st = 0, en = 0;
        if (walk) r = gpLine<VERB>(tab, c, data + beg, fin - beg, style, lead != 0, st, en);
        if (out.result) out.result[rec] = r;
        if (out.start) out.start[rec] = st;
        if (out.end) out.end[rec] = en;
      }
    }
  }
}

template <int KIND, int VERB>
hipError_t launchGrepK(const DevDfa &d, const uint8_t *data, const GpBufs &b, int style, int lead,
                       int invert, const GpOut &out, bool write, uint64_t *total,
                       uint64_t maxCount, uint64_t *nSelected, uint64_t *selBases,
                       uint64_t *dummy, const LaunchCfg &cfg, hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_gp_select<KIND, kThreads, VERB>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_gp_write<KIND, kThreads, VERB>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks = textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg);
  if (b.nChunks) {
    hipLaunchKernelGGL((k_gp_select<KIND, kThreads, VERB>), dim3(blocks), dim3(kThreads), ldsBytes,
                       stream, d, data, b, style, lead, invert);
  }
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, b.selCounts, b.nChunks, selBases,
                     total, dummy, uint64_t(0));
  hipLaunchKernelGGL(k_gp_total, dim3(1), dim3(64), 0, stream, total, maxCount, nSelected);
  if (write && b.nChunks) {
    const bool outcome = out.result || out.start || out.end;
    const int walk = outcome && !invert ? 1 : 0;
    hipLaunchKernelGGL((k_gp_write<KIND, kThreads, VERB>), dim3(blocks), dim3(kThreads),
                       walk ? ldsBytes : 0, stream, d, data, b, style, lead, walk, out);
  }
  return hipGetLastError();
}
