// k_fields_text.h - awk -F / cut over a raw text: the selected fields of every line, joined by `sep`,
// each line followed by the delimiter, in text order.  The separators of a line are the pieces
// k_extract_text.h emits for it (Red::collect, lib/Red.cpp:103-116: the spans replace<styLast,false>
// substitutes, include/Matcher.h:643-706, from where the successful attempt BEGAN to the match's
// end), over the lines lib/Util.cpp:109-130 cuts; a field is what lies between two of them, in
// front of the first or behind the last - re.split's fields, which may be empty
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_extract_text.h,
// whose XtWindow / xtLoad8 it uses, and k_replace_text.h, whose rtCopyWave it uses).
//
// The lines are driven as k_text.h drives them - from the split's delimiter bitmap, a wave per
// 16 KiB chunk, a chunk owning the lines that END in it - so nothing is proportional to the line
// count or to the field count, and nothing waits for either.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   as they stand: the delimiter bitmap,
//                   bases[chunk], open[chunk], and - under only_delimited alone - the HIT bitmap
//                   zeroed;
//   k_fd_size       table staged once per workgroup, a wave per chunk, chunks grid-strided, rounds of
//                   64 lines (k_text.h: textLines).  A lane runs the collect chain (collectLane) over
//                   its line with a field index, `prev` (the end of the last separator) and the
//                   fields written so far: a separator [at, mE) closes the field [prev, at), the
//                   chain's end closes [prev, n) (fdSizeLane).  The chain is LEFT behind separator
//                   min(S, hi) - S = max_fields - 1, hi = the highest selected field - so a line is
//                   not walked behind the last field anyone asked for.  outBytes[chunk],
//                   lineCounts[chunk], fieldCounts[chunk], all u64; under only_delimited an
//                   emitted line sets its delimiter's bit in the hit bitmap;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_fd_totals     one workgroup: *n_emitted, *n_fields = the sums, *out_len = the total;
//   k_fd_write      (skipped when the call only sizes) k_xt_write's shape: a wave per chunk over the
//                   emitted lines' bitmap - the hit bitmap under only_delimited, else the delimiter
//                   bitmap ITSELF (every line is emitted; no second, identical bitmap is written).
//                   Per round of 64 lines a lane sizes its line again, the wave's exclusive prefix
//                   plus the carry gives it ONE contiguous run f1 sep f2 sep ... d, and the lane
//                   assembles it in XtWindow: fields 8 bytes at a time, sep in one put, the
//                   delimiter in one put.  A field of kXtHand bytes or more is handed to the whole
//                   wave (rtCopyWave) - from inside the callback when a separator closed it, from
//                   behind the chain when it is the line's last.
// No per-line or per-field value is stored anywhere; no workgroup waits for another.  Nothing is
// read outside data[0, len) and nothing is written at or behind out_cap, or outside a lane's run.
//
// scratch (kernels.hip: FieldsScratch): replace_text's layout plus one u64 per chunk - two
// bitmaps of len / 8 bytes (rounded up to whole chunks), 52 bytes per chunk, 8 per 1,024 chunks
// and 72, rounded up to 16.
#pragma once

struct FdBufs {
  uint64_t *outBytes;        // [nChunks] output bytes of the chunk's lines
  uint64_t *lineCounts;      // [nChunks] emitted lines of the chunk
  uint64_t *fieldCounts;     // [nChunks] fields written of the chunk's lines
  const uint64_t *outBases;  // [nChunks + 1] exclusive scan of outBytes, the total behind it
};

struct FdArgs {
  uint64_t select;  // bit k - 1 = field k; bit 63 = field 64 and every later one
  uint64_t lim;     // the chain is left behind this many separators: min(S, hi)
  uint64_t sep;     // the joiner's bytes, little-endian
  uint32_t sepLen;  // 0..8
  uint32_t delim;
  int onlyDelimited;
};

// is field f (0-based) selected
__device__ __forceinline__ bool fdSelected(const FdArgs &a, uint64_t f) {
  return (a.select >> (f < 63 ? f : 63)) & 1u;
}

// the output line of p[0..n) added to bytes (its length with the delimiter) and to fields (the
// fields it holds); false, and nothing added, when the line is not emitted.  Behind separator a.lim
// the chain is left; what the line has from `prev` on is then ONE field, of index a.lim: the rest of
// the line when S ended the chain, and not selected when hi did (hi is the highest selected field)
// - so it closes by the same test.  (A line without a separator has closed no field when that is
// found out: the sums are added to directly, there is nothing to take back.)
template <class T>
__device__ __forceinline__ bool fdSizeLane(const T &tab, const LaneCtx &c, const uint8_t *p,
                                           uint64_t n, const FdArgs &a, uint64_t &bytes,
                                           uint64_t &fields) {
  uint64_t seen = 0, prev = 0;
  bool wrote = false;
  auto close = [&](uint64_t f, uint64_t flen) {
    if (fdSelected(a, f)) {
      bytes += flen + (wrote ? a.sepLen : 0u);
      ++fields;
      wrote = true;
    }
  };
  if (a.lim) {
    collectLane(tab, c, p, n, [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
      close(seen, at - prev);
      prev = mE;
      return ++seen < a.lim;
    });
  }
  if (a.onlyDelimited && seen == 0) return false;
  close(seen, n - prev);
  ++bytes;
  return true;
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_fd_size(DevDfa d, const uint8_t *data, GpBufs b, FdBufs x, FdArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    uint64_t bytes = 0, fields = 0;
    uint32_t mine = 0;  // (a chunk has 16,384 lines at the most)
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (have) {
        if (fdSizeLane(tab, c, data + beg, fin - beg, a, bytes, fields)) {
          ++mine;
          // (without only_delimited every line is emitted: the delimiter bitmap says it all)
          if (a.onlyDelimited)
            atomicOr(reinterpret_cast<uint32_t *>(b.selMasks) + (fin >> 5), 1u << (fin & 31u));
        }
      }
    });
    for (int o = 32; o; o >>= 1) {
      bytes += __shfl_xor(bytes, o);
      mine += __shfl_xor(mine, o);
      fields += __shfl_xor(fields, o);
    }
    if (lane == 0) {
      x.outBytes[ch] = bytes;
      x.lineCounts[ch] = mine;
      x.fieldCounts[ch] = fields;
    }
  }
}

// one workgroup: *nEmitted / *nFields = the sums of lineCounts / fieldCounts, *outLen = the scan's
// total (outTotal == nullptr: the text is empty)
__global__ void __launch_bounds__(1024)
k_fd_totals(const uint64_t *lineCounts, const uint64_t *fieldCounts, uint64_t nChunks,
            const uint64_t *outTotal, uint64_t *outLen, uint64_t *nEmitted, uint64_t *nFields) {
  __shared__ uint64_t ws[2][16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t lines = 0, fields = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 1024) {
    lines += lineCounts[i];
    fields += fieldCounts[i];
  }
  for (int o = 32; o; o >>= 1) {
    lines += __shfl_xor(lines, o);
    fields += __shfl_xor(fields, o);
  }
  if (lane == 0) {
    ws[0][wave] = lines;
    ws[1][wave] = fields;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t allLines = 0, allFields = 0;
    for (int w = 0; w < 16; ++w) {
      allLines += ws[0][w];
      allFields += ws[1][w];
    }
    *nEmitted = allLines;
    *nFields = allFields;
    *outLen = outTotal ? *outTotal : 0;
  }
}

template <int KIND, int kThreads>
__global__ void __launch_bounds__(kThreads)
k_fd_write(DevDfa d, const uint8_t *data, uint64_t len, GpBufs b, FdBufs x, FdArgs a, uint8_t *out,
           uint64_t cap) {
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
    // (b.selMasks: the emitted lines' bitmap - the hit bitmap, or the delimiter bitmap itself)
    const TextHits h(b, ch, lane);
    uint64_t carry = first;  // where the round's first run goes
    for (uint32_t k0 = 0; k0 < h.s.total && carry < cap; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool have = k < h.s.total;
      uint64_t beg, fin;
      uint32_t index;  // (not needed here)
      h.line(h.s.select(have ? k : h.s.total - 1), beg, fin, index);  // the emitted line
      // the sizing walk, then the lanes' exclusive prefix
      uint64_t mine = 0, nf = 0;  // (nf: not needed here)
      if (have) fdSizeLane(tab, c, data + beg, fin - beg, a, mine, nf);
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
      // the line's state across the hand-overs: separators seen, the end of the last one (where
      // the open field begins, and where the chain goes on), whether a field is written yet
      uint64_t seen = 0, prev = 0;
      bool wrote = false;
      bool more = mine != 0 && dst < cap;
      while (__ballot(more)) {
        uint64_t bigSrc = 0, bigDst = 0, bigLen = 0;
        if (more) {
          more = false;
          // the selected field data[s, s + n) behind what the window holds, sep in front of it
          // unless it is the line's first: true = handed to the wave, the window begins again
          // behind it
          auto emit = [&](uint64_t s, uint64_t n) -> bool {
            if (wrote && a.sepLen) w.put(a.sep, a.sepLen);
            wrote = true;
            if (n >= kXtHand) {
              w.close();
              bigSrc = s;
              bigDst = w.at - mis;
              bigLen = n;
              w.open(w.at + n);
              return true;
            }
            for (; n; s += 8) {
              const uint32_t take = n < 8 ? uint32_t(n) : 8u;
              w.put(xtLoad8(data, len, s, take), take);
              n -= take;
            }
            return false;
          };
          bool handed = false;
          if (seen < a.lim) {
            const uint64_t from = prev;  // the chain goes on behind the last separator
            collectLane(tab, c, data + beg + from, fin - beg - from,
                        [&](uint32_t, uint64_t, uint64_t mE, uint64_t at) {
              const uint64_t s = beg + prev, n = from + at - prev;
              prev = from + mE;
              if (fdSelected(a, seen++)) handed = emit(s, n);
              if (handed) {
                more = !w.full();
                return false;
              }
              return seen < a.lim && !w.full();
            });
          }
          // behind the chain: the last field (fdSizeLane has why one test closes it), the delimiter
          if (!handed && !w.full()) {
            if (fdSelected(a, seen)) emit(beg + prev, fin - beg - prev);
            w.put(a.delim, 1);
          }
        }
        // the fields handed over, one after the other, by the whole wave
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
hipError_t launchFieldsTextK(const DevDfa &d, const uint8_t *data, uint64_t len, const GpBufs &b,
                             const FdBufs &x, const FdArgs &a, bool size, uint8_t *out,
                             uint64_t cap, const LaunchCfg &cfg, hipStream_t stream) {
  // resident workgroups by k_text.h's rule (textBlocks).  Under the LDS placements the sizing pass
  // runs 768 threads, not kStagedThreads' 1,024: beside the chain a lane carries the field index,
  // `prev` and two 64-bit sums, which is 2-6 registers more than the 128 a 1,024-thread workgroup
  // has - 12 waves a CU without private memory instead of 16 with it.  The write pass runs 512
  // threads there, as launchExtractTextK's, and does not spill either
  // (profiles/fields_text_resources.md)
  constexpr int kThreads = kStagedLds<KIND> ? 768 : 256;
  constexpr int kWriteThreads = kStagedLds<KIND> ? 512 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_fd_size<KIND, kThreads>, ldsBytes);
  if (e == hipSuccess) e = setLds(k_fd_write<KIND, kWriteThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  if (size) {
    hipLaunchKernelGGL((k_fd_size<KIND, kThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg)), dim3(kThreads),
                       ldsBytes, stream, d, data, b, x, a);
  } else {
    hipLaunchKernelGGL((k_fd_write<KIND, kWriteThreads>),
                       dim3(textBlocks<KIND>(b.nChunks, ldsBytes, kWriteThreads, cfg)),
                       dim3(kWriteThreads), ldsBytes, stream, d, data, len, b, x, a, out, cap);
  }
  return hipGetLastError();
}
