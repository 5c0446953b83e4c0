// k_text.h - what the raw-text verbs share (k_grep.h, k_collect_text.h, k_tally_text.h,
// k_replace_text.h): the views of the split's delimiter bitmap, the line index behind it (k_gp_last,
// k_gp_open), the line walk (textLines), the hit-line lookup (TextHits), the lane context, and on
// the host the launch geometry (textBlocks; the scratch cursor, Carve, is k_common.h's)
// (included by kernels.hip inside namespace redgpu { namespace { ... } }, in front of k_grep.h;
// DESIGN 4.3f).
//
// Lines are never listed: they are driven from the split's delimiter bitmap (k_split.h: one bit per
// byte, which k_split_count leaves as u16 per 16 bytes in byte order - read here as a plain
// bitmap), so nothing is proportional to the line count and nothing waits for it.  The line index
// (kernels.hip: launchTextIndex) is
//   k_split_count   (k_split.h, as it stands) the delimiter bitmap and counts[chunk];
//   k_split_scan    (likewise) bases[chunk] = lines that end in front of the chunk, *n_lines;
//   k_gp_last       per 16 KiB split chunk the position behind its last delimiter (0 = none), and
//                   the chunk's part of the verb's SELECTED / HIT bitmap zeroed;
//   k_gp_open       one workgroup, an exclusive max-scan of those in place: open[chunk] = where the
//                   line that is in progress at the chunk's first byte begins (it may begin many
//                   chunks back).
// A verb's passes then give a WAVE to a chunk, chunks grid-strided.  A chunk owns the lines that END
// in it.  A lane holds 256 bits of the chunk's bitmap (four u64).
#pragma once

// lane context for the lane functions, with the start-byte filters searchLane reads (k_generic's)
template <int KIND>
__device__ __forceinline__ LaneCtx gpCtx(const DevDfa &d, uint8_t *lds) {
  LaneCtx c{lds, lds + 256, resOf<KIND>(d, lds), d.init, d.leaderNext, d.nPureDead, d.firstAccept,
            d.leaderLen};
  c.startWord[0] = d.startFreeWord; c.startCount[0] = d.startFreeCount;
  c.startWord[1] = d.startLeadWord; c.startCount[1] = d.startLeadCount;
  c.start2Word[0] = d.start2FreeWord; c.start2Count[0] = d.start2FreeCount;
  c.start2Word[1] = d.start2LeadWord; c.start2Count[1] = d.start2LeadCount;
  c.suffixClosed = d.suffixClosed;
  return c;
}

// the verb launchBatch would run for search over this DFA (normalizeVerbStyle), on one line.
// match<styLast> goes through matchLastLane's form WITH the exit test for every DFA: k_generic
// picks the no-exit form (walkAllBytes) under deadAbsorbing && !earlyDeath, which gives the same
// Outcome (past an absorbing dead end nothing accepts) but needs more registers than a
// 1024-thread k_gp_select has (137 VGPRs, 40 bytes of private memory per lane when built in)
template <int VERB, class T>
__device__ __forceinline__ int32_t gpLine(const T &tab, const LaneCtx &c, const uint8_t *p,
                                          uint64_t n, int style, bool lead, uint64_t &st,
                                          uint64_t &en) {
  if constexpr (VERB == kSearch) return searchLane(tab, c, p, n, style, lead, st, en);
  else
    return style == kStyLast ? matchLastLane(tab, c, p, n, lead, st, en)
                             : matchLane(tab, c, p, n, style, lead, st, en);
}

// a lane's 256 bits of a chunk's bitmap: bit b of w[k] = byte 256 * lane + 64 * k + b of the chunk
struct GpBits {
  uint64_t w[4];
  __device__ __forceinline__ uint32_t count() const {
    return __popcll(w[0]) + __popcll(w[1]) + __popcll(w[2]) + __popcll(w[3]);
  }
  // 1 + the highest set bit (0 = none)
  __device__ __forceinline__ uint32_t last() const {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (w[k]) r = uint32_t(64 * k + 64 - __clzll(static_cast<long long>(w[k])));
    return r;
  }
};

__device__ __forceinline__ GpBits gpLoadBits(const uint16_t *bitmap, uint64_t chunk, uint32_t lane) {
  // (the bitmap is 16-byte aligned and a chunk has 2048 bytes of it: two aligned 16-byte loads)
  const uint4 *q = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(bitmap) +
                                                   chunk * (kSplitChunk / 8) + lane * 32u);
  const uint4 a = q[0], b = q[1];
  GpBits r;
  r.w[0] = uint64_t(a.x) | (uint64_t(a.y) << 32);
  r.w[1] = uint64_t(a.z) | (uint64_t(a.w) << 32);
  r.w[2] = uint64_t(b.x) | (uint64_t(b.y) << 32);
  r.w[3] = uint64_t(b.z) | (uint64_t(b.w) << 32);
  return r;
}

__device__ __forceinline__ GpBits gpShflBits(const GpBits &m, uint32_t from) {
  GpBits r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = __shfl(uint32_t(m.w[k]), int(from));
    const uint32_t hi = __shfl(uint32_t(m.w[k] >> 32), int(from));
    r.w[k] = uint64_t(lo) | (uint64_t(hi) << 32);
  }
  return r;
}

// position of the k-th (0-based) set bit of x, which has more than k
__device__ __forceinline__ uint32_t gpSelect64(uint64_t x, uint32_t k) {
  uint32_t pos = 0;
  uint32_t v = uint32_t(x);
  uint32_t c = __popc(v);
  if (k >= c) { k -= c; pos = 32; v = uint32_t(x >> 32); }
  c = __popc(v & 0xffffu);
  if (k >= c) { k -= c; pos += 16; v >>= 16; }
  v &= 0xffffu;
  c = __popc(v & 0xffu);
  if (k >= c) { k -= c; pos += 8; v >>= 8; }
  v &= 0xffu;
  for (uint32_t i = 0; i < k; ++i) v &= v - 1;  // (at most 7 times)
  return pos + uint32_t(__ffs(int(v))) - 1;
}

// position, inside the 256 bits, of their k-th set bit
__device__ __forceinline__ uint32_t gpSelect256(const GpBits &m, uint32_t k) {
  uint32_t pos = 0;
  uint64_t x = m.w[0];
  bool found = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t c = __popcll(m.w[i]);
    if (!found && k >= c) { k -= c; pos = 64 * (i + 1); x = m.w[i + 1]; }
    else found = true;
  }
  return pos + gpSelect64(x, k);
}

// the wave's view of one chunk's bitmap: every lane's bits, the lanes' exclusive prefix counts
struct GpChunk {
  GpBits m;
  uint32_t excl, total;
  __device__ __forceinline__ void scan(uint32_t lane) {
    const uint32_t c = m.count();
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o);
      if (lane >= uint32_t(o)) incl += v;
    }
    excl = incl - c;
    total = __shfl(incl, 63);
  }
  // chunk-relative position of the chunk's k-th set bit (k < total; every lane calls)
  __device__ __forceinline__ uint32_t select(uint32_t k) const {
    // the last lane whose prefix count is <= k
    uint32_t lo = 0;
#pragma unroll
    for (int step = 32; step; step >>= 1) {
      const uint32_t e = __shfl(excl, int(lo + step));
      if (e <= k) lo += step;
    }
    const uint32_t e = __shfl(excl, int(lo));
    const GpBits o = gpShflBits(m, lo);
    return lo * 256u + gpSelect256(o, k - e);
  }
};

// per chunk: the position behind its last delimiter (0 = it has none); its selected bits zeroed
// (selMasks may be null: nothing is zeroed then)
__global__ void __launch_bounds__(256)
k_gp_last(const uint16_t *masks, const uint32_t *counts, uint64_t nChunks, uint64_t *open,
          uint16_t *selMasks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t ch = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ch < nChunks; ch += waves) {
    if (selMasks) {  // (uniform; k_tally_text.h has no selected bitmap)
      uint4 *z = reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(selMasks) +
                                           ch * (kSplitChunk / 8) + lane * 32u);
      z[0] = make_uint4(0, 0, 0, 0);
      z[1] = make_uint4(0, 0, 0, 0);
    }
    uint32_t last = 0;
    if (counts[ch]) {  // (uniform)
      const uint32_t mine = gpLoadBits(masks, ch, lane).last();
      last = mine ? lane * 256u + mine : 0u;
      for (int o = 32; o; o >>= 1) {
        const uint32_t v = __shfl_xor(last, o);
        last = v > last ? v : last;
      }
    }
    if (lane == 0) open[ch] = last ? ch * kSplitChunk + last : 0;
  }
}

// one workgroup: open[chunk] = max of the chunks' values in front of it (exclusive, in place):
// the position behind the last delimiter in front of the chunk
__global__ void __launch_bounds__(1024) k_gp_open(uint64_t *open, uint64_t nChunks) {
  __shared__ uint64_t waveMax[2][16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  int buf = 0;
  for (uint64_t tile = 0; tile < nChunks; tile += 1024, buf ^= 1) {
    const uint64_t i = tile + threadIdx.x;
    const uint64_t own = i < nChunks ? open[i] : 0;
    uint64_t incl = own;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t v = __shfl_up(incl, o);
      if (lane >= uint32_t(o) && v > incl) incl = v;
    }
    if (lane == 63) waveMax[buf][wave] = incl;
    __syncthreads();  // (the other buffer is rewritten only after the next tile's barrier)
    uint64_t before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const uint64_t v = waveMax[buf][w];
      if (w < int(wave) && v > before) before = v;
      if (v > all) all = v;
    }
    uint64_t below = __shfl_up(incl, 1);  // the lanes in front of this one, inside the wave
    if (lane == 0) below = 0;
    if (i < nChunks) open[i] = below > before ? below : before;
    carry = all;
  }
}

struct GpBufs {
  const uint16_t *masks;    // the delimiter bitmap (k_split_count)
  uint16_t *selMasks;       // the selected lines' delimiters, same layout
  const uint64_t *bases;    // [nChunks] lines that end in front of the chunk
  const uint64_t *open;     // [nChunks] where the line in progress at the chunk's first byte begins
  uint32_t *selCounts;      // [nChunks] lines of the chunk that are selected
  const uint64_t *selBases; // [nChunks] records in front of the chunk
  uint64_t nChunks;
};

// The line walk: the wave's chunk ch, in rounds of 64 lines.  Per round the wave takes the chunk's
// next 64 delimiters, lane j the j-th: it finds the lane that holds it (binary search over the
// lanes' prefix counts, through shuffles), fetches that lane's words, selects the bit; the line
// begins behind the delimiter of the lane below (round 0, lane 0: open[chunk]).  Registers and
// shuffles only, so 1 line or 16,384 lines per chunk differ in the number of rounds (1 .. 256)
// alone.  f(have, beg, fin) is called by ALL 64 lanes of every round, converged - it may ballot
// and shuffle; have = the lane has a line, data[beg, fin), its delimiter at fin.
template <class F>
__device__ __forceinline__ void textLines(const GpBufs &b, uint64_t ch, uint32_t lane, F &&f) {
  GpChunk g;
  g.m = gpLoadBits(b.masks, ch, lane);
  g.scan(lane);
  const uint64_t base = ch * kSplitChunk;
  uint64_t begin0 = b.open[ch];  // where the round's first line begins
  for (uint32_t k0 = 0; k0 < g.total; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool have = k < g.total;
    const uint64_t fin = base + g.select(have ? k : g.total - 1);
    uint64_t beg = __shfl_up(fin, 1) + 1;
    if (lane == 0) beg = begin0;
    begin0 = __shfl(fin, 63) + 1;
    f(have, beg, fin);
  }
}

// The hit-line lookup of the write passes: the wave's views of one chunk's SELECTED / HIT bitmap
// and of its delimiter bitmap, from which a hit line's begin, finish and index come without a
// walk over the lines in front of it.
struct TextHits {
  GpChunk s, g;     // the hit bitmap, the delimiter bitmap
  uint64_t base;    // the chunk's first byte
  uint64_t behind;  // position behind the last delimiter in front of this lane's bits
  uint64_t srcEnd;  // position behind the chunk's last delimiter (0 = it has none)

  // (every lane calls)
  __device__ __forceinline__ TextHits(const GpBufs &b, uint64_t ch, uint32_t lane) {
    s.m = gpLoadBits(b.selMasks, ch, lane);
    s.scan(lane);
    g.m = gpLoadBits(b.masks, ch, lane);
    g.scan(lane);
    base = ch * kSplitChunk;
    const uint32_t own = g.m.last();
    behind = own ? base + lane * 256u + own : 0;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t v = __shfl_up(behind, o);
      if (lane >= uint32_t(o) && v > behind) behind = v;
    }
    srcEnd = __shfl(behind, 63);
    behind = __shfl_up(behind, 1);
    if (lane == 0) behind = 0;
    const uint64_t opened = b.open[ch];
    if (opened > behind) behind = opened;
  }

  // the line whose delimiter is the chunk's byte pos: data[beg, fin), and index = the chunk's
  // lines in front of it (+ bases[chunk] = its number in the text).  Every lane calls.
  __device__ __forceinline__ void line(uint32_t pos, uint64_t &beg, uint64_t &fin,
                                       uint32_t &index) const {
    // the lane that holds it: the delimiters below it there, and the one just below
    const uint32_t holder = pos >> 8, inLane = pos & 255u;
    const GpBits o = gpShflBits(g.m, holder);
    const uint32_t oExcl = __shfl(g.excl, int(holder));
    const uint64_t oBehind = __shfl(behind, int(holder));
    uint32_t rank = 0, prev = 0;  // prev = 1 + the highest delimiter bit below inLane
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t lo = uint32_t(64 * w);
      uint64_t x = o.w[w];
      if (inLane < lo + 64) x = inLane > lo ? x & ((1ull << (inLane - lo)) - 1) : 0;
      rank += uint32_t(__popcll(x));
      if (x) prev = lo + 64 - uint32_t(__clzll(static_cast<long long>(x)));
    }
    fin = base + pos;
    beg = prev ? base + holder * 256u + prev : oBehind;
    index = oExcl + rank;
  }
};

// The launch geometry of a pass that stages the table per workgroup and gives a wave to a chunk
// (k_common.h: kStagedThreads, stagedPerCu): at most one wave of resident workgroups.
template <int KIND>
__host__ inline uint32_t textBlocks(uint64_t nChunks, size_t ldsBytes, int threads,
                                    const LaunchCfg &cfg) {
  const uint64_t waves = uint64_t(threads) / 64;
  const uint64_t most = uint64_t(cfg.numCUs) * stagedPerCu<KIND>(ldsBytes);
  const uint64_t blocks = (nChunks + waves - 1) / waves;
  return uint32_t(blocks > most ? most : blocks);
}

// ... of a pass without a table: a wave per chunk, four to a workgroup, at most 8 per CU
__host__ inline uint32_t smallBlocks(uint64_t nChunks, int numCUs) {
  const uint64_t blocks = (nChunks + 3) / 4, most = uint64_t(numCUs) * 8;
  return uint32_t(blocks > most ? most : blocks);
}

// ... and of a pass over `words` words (zeroing, the passes over uniq_text's table): 256 to a
// workgroup, at most 8 per CU; 0 for no words
__host__ inline uint32_t wordBlocks(uint64_t words, int numCUs) {
  const uint64_t blocks = (words + 255) / 256, most = uint64_t(numCUs) * 8;
  return uint32_t(blocks > most ? most : blocks);
}
