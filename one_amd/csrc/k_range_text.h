// k_range_text.h - sed's /open/,/close/ line ranges of a raw text: the lines between a line whose
// search<style,doLeader> result is open_result and the next line whose result is close_result
// (sed -n '/A/,/B/p', awk '/A/,/B/'; under invert sed '/A/,/B/d'), put together as a text, and one
// record per range.  The first verb of the family in which a line's fate depends on the lines in
// front of it: a two-state machine (outside / inside) runs over the lines in text order
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, after k_route_text.h;
// DESIGN 4.3p).
//
// A line's value is k_tally_text.h's LINES item.  What is kept per line is "is open" and "is close",
// in two bit-planes laid out like the delimiter bitmap (the bit at the line's delimiter); with
// open_result == close_result (the TOGGLE form: sed -n '/```/,/```/p') the one plane says both.  An
// EVENT is a line with a bit in either plane.  The machine's rule, per line (rgStep):
//   outside: an open line begins a range and is its OPEN line, anything else stays outside;
//   inside:  a close line is the range's CLOSE line, anything else is a BODY line.
// The lines are driven as k_text.h drives them - a wave per 16 KiB chunk, a chunk owning the lines
// that END in it.  All queued on the caller's stream:
//   k_split_count / k_split_scan / k_gp_last / k_gp_open   the line index (k_text.h); the planes
//                   zeroed (a memset on the stream);
//   k_rg_class      k_ro_class's walk: table staged once per workgroup, a wave per chunk, rounds of
//                   64 lines; a line of value open_result ors its delimiter bit into the open
//                   plane, one of value close_result into the close plane.  The only pass that
//                   touches the table or the text's bytes before the copy;
//   k_rg_events     no table from here on.  Two results: carry[chunk] = 2 * (1 + the position of the
//                   chunk's last event) + (it is an open), 0 = it has none.  Toggle:
//                   events[chunk] = its events;
//   k_gp_open       (k_text.h, two results) the exclusive max-scan in place: carry[chunk] = the last
//                   event in front of the chunk, bit 0 its kind - the state after a line is the kind
//                   of the last event at or before it;
//   k_split_scan    (k_split.h, toggle) carry[chunk] = the events in front of the chunk - the state
//                   is their parity.  Either way the machine is INSIDE at the chunk's first line iff
//                   carry[chunk] & 1;
//   k_rg_starts     a wave per chunk.  A lane's entry state from the lanes below it (rgLaneInside:
//                   the same max-scan / parity over the lanes, seeded with the chunk's), then it
//                   steps through the events among its own 256 bits in registers;
//                   starts[chunk] = the ranges that begin in the chunk;
//   k_split_scan    startBases[chunk] = ranges that begin in front of the chunk, and their total;
//   k_rg_mark       a wave per chunk.  A lane's entry state again and the ranges that begin in front
//                   of its bits; it steps through its own delimiters with the state and the current
//                   range's number in registers: the lines of ranges numbered max_ranges and above
//                   are outside; a line is emitted as emit_open / emit_close / invert say; an open
//                   line stores first_line[r] and begin[r], a close line last_line[r] and end[r]
//                   (r < rec_cap).  The lane's 256 EMIT bits are stored over its open plane (a chunk
//                   reads its own bits only, and they are in registers by then);
//                   emitBytes[chunk], emitLines[chunk]; the last chunk's wave also leaves the final
//                   state and the position behind the text's last delimiter;
//   k_scan_partials / k_scan_tops / k_scan_fill   (k_misc.h) outBases[chunk] = output bytes in front
//                   of the chunk, outBases[nChunks] = their total;
//   k_rg_totals     one workgroup: *n_emitted, *out_len, *n_ranges = min(ranges, max_ranges), and
//                   the end of a last range that is still open behind the last line;
//   k_ft_write      (k_filter_text.h, as it stands; skipped when the call only sizes) the runs of
//                   emitted lines copied by ftWriteRuns, cut at out_cap.
// No per-line value is stored anywhere but the two planes; no workgroup waits for another; every
// loop is bounded by a lane's 256 bits or by the chunk count.  Nothing is read outside
// data[0, len) and nothing is written at or behind out_cap or rec_cap.  Line numbers, range numbers
// and offsets are 64-bit.  Scratch: three bitmaps of len / 8, and 64 bytes per chunk, 8 per 1,024
// chunks and 72, rounded up to 16.
#pragma once

struct RgBufs {
  uint16_t *openBits;          // the plane of the open lines; k_rg_mark leaves the EMIT bitmap here
  uint16_t *closeBits;         // the plane of the close lines (toggle: not used)
  uint64_t *carry;             // [nChunks] bit 0: the machine is inside at the chunk's first line
  uint32_t *events;            // [nChunks] toggle: the chunk's events
  uint32_t *starts;            // [nChunks] ranges that begin in the chunk
  const uint64_t *startBases;  // [nChunks] ranges that begin in front of the chunk
  uint64_t *emitBytes;         // [nChunks] bytes of the chunk's emitted lines
  uint32_t *emitLines;         // [nChunks] their number
  uint64_t *fin;               // [2] the state behind the last line, where the last delimiter ends
  int32_t openResult, closeResult;
  int toggle;
};

struct RgArgs {
  int emitOpen, emitClose, invert;
  uint64_t maxRanges, recCap;
  uint64_t *firstLine, *lastLine, *begin, *end;  // [recCap] each, any may be null
};

enum : uint32_t { kRgOutside = 0, kRgOpen = 1, kRgBody = 2, kRgClose = 3 };

// the machine's step over one line: what the line is, and the state behind it
__device__ __forceinline__ uint32_t rgStep(bool &inside, bool isOpen, bool isClose) {
  if (!inside) {
    inside = isOpen;
    return isOpen ? kRgOpen : kRgOutside;
  }
  inside = !isClose;
  return isClose ? kRgClose : kRgBody;
}

// a lane's bits of the two planes (toggle: the open plane is the close plane too)
struct RgPlanes {
  GpBits o, c;
  __device__ __forceinline__ RgPlanes(const RgBufs &r, uint64_t ch, uint32_t lane) {
    o = gpLoadBits(r.openBits, ch, lane);
    c = r.toggle ? o : gpLoadBits(r.closeBits, ch, lane);
  }
  __device__ __forceinline__ GpBits events() const {
    return GpBits{{o.w[0] | c.w[0], o.w[1] | c.w[1], o.w[2] | c.w[2], o.w[3] | c.w[3]}};
  }
  // the ranges that begin among this lane's bits when it is entered in state `inside`
  __device__ __forceinline__ uint32_t starts(bool inside) const {
    uint32_t n = 0;
    ftEachUp(events(), [&](auto word, uint64_t bit) {
      constexpr int k = decltype(word)::value;
      n += rgStep(inside, (o.w[k] & bit) != 0, (c.w[k] & bit) != 0) == kRgOpen;
    });
    return n;
  }
};

// is the machine inside in front of this lane's bits (chunkCarry: carry[chunk]; every lane calls)
__device__ __forceinline__ bool rgLaneInside(const RgBufs &r, const RgPlanes &p, uint64_t chunkCarry,
                                             uint32_t lane) {
  if (r.toggle) {  // (uniform) the parity of the events in front
    const uint32_t own = p.o.count();
    uint32_t incl = own;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o);
      if (lane >= uint32_t(o)) incl += v;
    }
    return ((incl - own + uint32_t(chunkCarry)) & 1u) != 0;
  }
  // the kind of the last event in front: 2 * (1 + its lane) + (it is an open), 0 = none
  const uint32_t lastOpen = p.o.last(), lastClose = p.c.last();
  uint32_t v = (lastOpen | lastClose) ? ((lane + 1) << 1 | uint32_t(lastOpen > lastClose)) : 0u;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= uint32_t(o) && u > v) v = u;
  }
  v = __shfl_up(v, 1);
  if (lane == 0) v = 0;
  return ((v ? v : uint32_t(chunkCarry)) & 1u) != 0;
}

template <int KIND, int kThreads, int VERB>
__global__ void __launch_bounds__(kThreads)
k_rg_class(DevDfa d, const uint8_t *data, GpBufs b, int style, int lead, RgBufs r) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Tab<KIND> tab = stageTab<KIND, kThreads>(d, lds);
  const LaneCtx c = gpCtx<KIND>(d, lds);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t ch = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); ch < b.nChunks;
       ch += waves) {
    textLines(b, ch, lane, [&](bool have, uint64_t beg, uint64_t fin) {
      if (have) {
        uint64_t st, en;
        const int32_t v = gpLine<VERB>(tab, c, data + beg, fin - beg, style, lead != 0, st, en);
        // (toggle: the two results are equal and the close plane stays empty)
        uint16_t *plane = v == r.openResult ? r.openBits : v == r.closeResult ? r.closeBits : nullptr;
        if (plane) atomicOr(reinterpret_cast<uint32_t *>(plane) + (fin >> 5), 1u << (fin & 31u));
      }
    });
  }
}

__global__ void __launch_bounds__(256) k_rg_events(RgBufs r, uint64_t nChunks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < nChunks; ch += waves) {
    const RgPlanes p(r, ch, lane);
    if (r.toggle) {  // (uniform)
      uint32_t n = p.o.count();
      for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
      if (lane == 0) r.events[ch] = n;
    } else {
      const uint32_t lastOpen = p.o.last(), lastClose = p.c.last();
      const uint32_t last = lastOpen > lastClose ? lastOpen : lastClose;
      uint64_t v = 0;
      if (last) v = (ch * kSplitChunk + lane * 256u + last) << 1 | uint64_t(lastOpen > lastClose);
      for (int o = 32; o; o >>= 1) {
        const uint64_t u = __shfl_xor(v, o);
        v = u > v ? u : v;
      }
      if (lane == 0) r.carry[ch] = v;
    }
  }
}

__global__ void __launch_bounds__(256) k_rg_starts(RgBufs r, uint64_t nChunks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < nChunks; ch += waves) {
    const RgPlanes p(r, ch, lane);
    uint32_t n = p.starts(rgLaneInside(r, p, r.carry[ch], lane));
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) r.starts[ch] = n;
  }
}

// b.selMasks = the open plane: its bits are read first, and the chunk's EMIT bits stored over them
__global__ void __launch_bounds__(256) k_rg_mark(GpBufs b, RgBufs r, RgArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < b.nChunks; ch += waves) {
    const TextHits h(b, ch, lane);  // (h.s: the open plane)
    const RgPlanes p(r, ch, lane);
    const bool entry = rgLaneInside(r, p, r.carry[ch], lane);
    // the ranges that begin in front of this lane's bits
    const uint32_t own = p.starts(entry);
    uint32_t incl = own;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o);
      if (lane >= uint32_t(o)) incl += v;
    }
    uint64_t begun = r.startBases[ch] + (incl - own);
    const uint64_t lineBase = b.bases[ch] + h.g.excl;  // the number of the lane's first line
    bool inside = entry;
    GpBits e{{0, 0, 0, 0}};
    uint64_t bytes = 0, begin = h.behind;
    uint32_t t = 0, lines = 0;
    ftEachUp(h.g.m, [&](auto word, uint64_t bit) {
      constexpr int k = decltype(word)::value;
      const uint64_t i = lineBase + t++;
      const uint64_t behind = h.base + lane * 256u + uint32_t(64 * k) +
                              uint32_t(__ffsll(static_cast<long long>(bit)));
      const uint32_t kind = rgStep(inside, (p.o.w[k] & bit) != 0, (p.c.w[k] & bit) != 0);
      if (kind == kRgOpen) ++begun;
      // (a line that is not outside has a range in front of or at it: begun >= 1)
      const uint64_t range = begun - 1;
      const bool counted = kind != kRgOutside && range < a.maxRanges;
      if (counted && range < a.recCap) {
        if (kind == kRgOpen) {
          if (a.firstLine) a.firstLine[range] = i;
          if (a.begin) a.begin[range] = begin;
        } else if (kind == kRgClose) {
          if (a.lastLine) a.lastLine[range] = i;
          if (a.end) a.end[range] = behind;
        }
      }
      const bool chosen = counted && (kind == kRgBody || (kind == kRgOpen && a.emitOpen) ||
                                      (kind == kRgClose && a.emitClose));
      if (chosen != (a.invert != 0)) {
        e.w[k] |= bit;
        bytes += behind - begin;
        ++lines;
      }
      begin = behind;
    });
    ftStoreBits(b.selMasks, ch, lane, e);
    for (int o = 32; o; o >>= 1) {
      bytes += __shfl_xor(bytes, o);
      lines += __shfl_xor(lines, o);
    }
    if (lane == 0) {
      r.emitBytes[ch] = bytes;
      r.emitLines[ch] = lines;
    }
    if (ch + 1 == b.nChunks && lane == 63) {
      r.fin[0] = inside;
      r.fin[1] = h.srcEnd ? h.srcEnd : b.open[ch];
    }
  }
}

// one workgroup: *nEmitted = the sum of emitLines, *outLen = the scan's total, *nRanges =
// min(*begun, maxRanges), and the record of a last counted range that no line closes: it ends with
// the last line (outTotal == nullptr: the text is empty; nLines, nRanges, nEmitted may be null)
__global__ void __launch_bounds__(1024)
k_rg_totals(RgBufs r, RgArgs a, uint64_t nChunks, const uint64_t *outTotal, const uint64_t *begun,
            const uint64_t *linesFound, uint64_t *nLines, uint64_t *nRanges, uint64_t *nEmitted,
            uint64_t *outLen) {
  __shared__ uint64_t ws[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t sum = 0;
  for (uint64_t i = threadIdx.x; i < nChunks; i += 1024) sum += r.emitLines[i];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) ws[wave] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint64_t all = 0;
  for (int w = 0; w < 16; ++w) all += ws[w];
  const uint64_t found = *linesFound, ranges = nChunks ? *begun : 0;
  if (nLines) *nLines = found;
  if (nRanges) *nRanges = ranges < a.maxRanges ? ranges : a.maxRanges;
  if (nEmitted) *nEmitted = all;
  *outLen = outTotal ? *outTotal : 0;
  if (nChunks && ranges && ranges <= a.maxRanges && ranges - 1 < a.recCap && r.fin[0]) {
    if (a.lastLine) a.lastLine[ranges - 1] = found - 1;
    if (a.end) a.end[ranges - 1] = r.fin[1];
  }
}

template <int KIND, int VERB>
hipError_t launchRangeClassK(const DevDfa &d, const uint8_t *data, const GpBufs &b, int style,
                             int lead, const RgBufs &r, const LaunchCfg &cfg, hipStream_t stream) {
  constexpr int kThreads = kStagedThreads<KIND>;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  const hipError_t e = setLds(k_rg_class<KIND, kThreads, VERB>, ldsBytes);
  if (e != hipSuccess) return e;
  const uint32_t blocks = textBlocks<KIND>(b.nChunks, ldsBytes, kThreads, cfg);
  hipLaunchKernelGGL((k_rg_class<KIND, kThreads, VERB>), dim3(blocks), dim3(kThreads), ldsBytes,
                     stream, d, data, b, style, lead, r);
  return hipGetLastError();
}
