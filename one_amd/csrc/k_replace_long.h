// k_replace_long.h - replaceCore (include/Matcher.h:643-706) over ONE long text, across the chip
// (included by kernels.hip inside its namespace, after k_collect_long.h).
//
// replaceCore is collect's chain with another attempt: at position `in` one anchored attempt under
// the call's style (and the leader test); on success the bytes [in, found + 1) become the
// replacement and the chain goes on at found + 1, otherwise one byte is copied and it goes on at
// in + 1.  The chain is k_collect_long.h's, instantiated kClReplace (LongAttempt: style and leader;
// lean slots: attempt position u32 + end u64 = 12 bytes per text byte).  What is new here is the
// assembly, a pure function of the final records, numbered k = 0, 1, ... by the scan of the chunk
// counts; only k < max count:
//   k_rl_sum     a wave per chunk: the bytes its counted records remove (end - at), and the end
//                of its last one;
//   scans        (k_long.h's k_long_scan1, k_rl_scan2) exclusive scan of (sum, max) over the
//                chunks: in front of chunk j, `rem` bytes were removed and the text is covered up
//                to `cov`; *count and *out_len;
//   k_rl_copy    driven by TILES OF THE INPUT (kRlTile bytes, 16 per lane), not by the chunk that
//                owns a record: a kept byte x lands at x - (removed before x) + repl_len *
//                (records before x), replacement k at the landing place of its attempt position.
//                A tile marks the records that start in it (LDS: a flag and the end per start
//                byte), scans "covered up to" (max) and the output lengths (sum) over its lanes,
//                and stages its output - kept bytes and replacements - in LDS windows of kRlStage
//                bytes laid out at the destination's 16-byte alignment, which all lanes flush
//                with 16-byte stores.  A tile without a record start that is not covered is a
//                plain shifted copy: unaligned 16-byte loads, aligned 16-byte stores.  A match
//                that spans many chunks, or everything behind the max-th match, is thereby
//                skipped or copied by every tile on its own, in parallel.
// A work item is a run of whole chunks of at most kRlTile bytes, or one chunk longer than that,
// whose tiles the workgroup takes in order (carrying the output position and the record cursor).
#pragma once

constexpr uint32_t kRlTile = 4096;
constexpr uint32_t kRlThreads = 256;
constexpr uint32_t kRlStage = 8192;

struct RlBufs {
  uint64_t *rem, *cov;            // [m] per chunk: removed bytes / end of the last counted record;
                                  //     after the scans: exclusive sum / exclusive max
  uint64_t *blockRem, *blockCov;  // [nb] the same per 1024 chunks
};

__device__ __forceinline__ uint64_t rlFirstRecord(const ClBufs &b, uint64_t j) {
  return b.blockOff[j / 1024] + b.off[j];
}

__global__ void __launch_bounds__(256) k_rl_sum(ClBufs b, RlBufs r, uint64_t max) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * 4;
  for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < b.m; j += waves) {
    const uint64_t k0 = rlFirstRecord(b, j);
    const uint64_t lo = j * b.chunk;
    const uint64_t base = j * b.slots;
    uint64_t cnt = b.cnt[j];
    if (k0 >= max) cnt = 0;
    else if (max - k0 < cnt) cnt = max - k0;
    uint64_t sum = 0;
    for (uint64_t i = lane; i < cnt; i += 64) sum += b.ren[base + i] - (lo + b.rat[base + i]);
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
      r.rem[j] = sum;
      r.cov[j] = cnt ? b.ren[base + cnt - 1] : 0;
    }
  }
}

// one workgroup: exclusive (sum, max) of the block totals in place (k_long.h); *count =
// min(found, max), *outLen = n - removed + replLen * *count
__global__ void __launch_bounds__(1024)
k_rl_scan2(RlBufs r, uint64_t nb, uint64_t n, uint64_t replLen, uint64_t max, uint64_t *count,
           uint64_t *outLen) {
  __shared__ uint64_t s[1024], x[1024];
  const uint64_t removed = longScanTotals<true>(s, x, r.blockRem, r.blockCov, nb);
  if (threadIdx.x == 0) {
    const uint64_t found = *count;
    const uint64_t done = found < max ? found : max;
    *count = done;
    *outLen = n - removed + replLen * done;
  }
}

// the empty text
__global__ void __launch_bounds__(64) k_rl_empty(uint64_t *count, uint64_t *outLen) {
  if (threadIdx.x == 0) { *count = 0; *outLen = 0; }
}

// exclusive scans over the kRlThreads lanes of a workgroup (4 waves); `ws` is 4 words of LDS.
// Every lane gets the total too.
__device__ __forceinline__ uint64_t rlScanSum(uint64_t v, uint64_t *ws, uint64_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up(incl, o);
    if (lane >= uint32_t(o)) incl += u;
  }
  __syncthreads();
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint64_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += ws[w];
  total = ws[0] + ws[1] + ws[2] + ws[3];
  return before + incl - v;
}

__device__ __forceinline__ uint32_t rlScanMax(uint32_t v, uint32_t *ws) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(incl, o);
    if (lane >= uint32_t(o) && u > incl) incl = u;
  }
  uint32_t excl = __shfl_up(incl, 1);
  if (lane == 0) excl = 0;
  __syncthreads();
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  for (uint32_t w = 0; w < wave; ++w)
    if (ws[w] > excl) excl = ws[w];
  return excl;
}

// cnt bytes from src (LDS or global, any alignment) to dst (global): the bytes in front of dst's
// first 16-byte boundary and behind its last one singly, the rest as aligned 16-byte stores
__device__ __forceinline__ void rlStoreWide(uint8_t *dst, const uint8_t *src, uint64_t cnt) {
  if (cnt == 0) return;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  if (head > cnt) head = cnt;
  const uint64_t groups = (cnt - head) >> 4;
  const uint64_t tail = head + (groups << 4);
  for (uint64_t g = threadIdx.x; g < groups; g += kRlThreads) {
    uint4 v;
    __builtin_memcpy(&v, src + head + (g << 4), 16);
    *reinterpret_cast<uint4 *>(dst + head + (g << 4)) = v;
  }
  if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
  const uint64_t rest = cnt - tail;  // < 16
  if (threadIdx.x >= 32 && threadIdx.x - 32 < rest) dst[tail + threadIdx.x - 32] = src[tail + threadIdx.x - 32];
}

__global__ void __launch_bounds__(kRlThreads)
k_rl_copy(const uint8_t *p, uint64_t n, ClBufs b, RlBufs r, const uint8_t *repl, uint64_t replLen,
          uint64_t max, uint64_t nItems, uint32_t perItem, uint8_t *out, uint64_t outCap) {
  __shared__ __align__(16) uint8_t sStart[kRlTile];   // a counted record starts at this byte
  __shared__ __align__(16) uint16_t sEnd[kRlTile];    // ... and ends here (tile-relative, clipped)
  __shared__ __align__(16) uint8_t sStage[kRlStage];
  __shared__ uint64_t sWs[4];
  __shared__ uint32_t sWm[4];
  __shared__ uint64_t sPend;
  __shared__ uint32_t sAny;
  const uint32_t tid = threadIdx.x;
  for (uint64_t item = blockIdx.x; item < nItems; item += gridDim.x) {
    const uint64_t j0 = item * perItem;
    const uint64_t j1 = j0 + perItem < b.m ? j0 + perItem : b.m;
    const uint64_t itemLo = j0 * b.chunk;
    const uint64_t itemHi = j1 * b.chunk < n ? j1 * b.chunk : n;
    // in front of the item: records, removed bytes (whole records), covered up to
    const uint64_t k0 = rlFirstRecord(b, j0);
    const uint64_t before = k0 < max ? k0 : max;
    const uint64_t rem0 = r.blockRem[j0 / 1024] + r.rem[j0];
    uint64_t pend = r.cov[j0];
    if (r.blockCov[j0 / 1024] > pend) pend = r.blockCov[j0 / 1024];
    uint64_t outAt = itemLo - (rem0 - (pend > itemLo ? pend - itemLo : 0)) + replLen * before;
    uint32_t cur = 0;  // (perItem == 1) records of the chunk in front of the tile
    for (uint64_t a = itemLo; a < itemHi; a += kRlTile) {
      const uint32_t len = uint32_t(itemHi - a < kRlTile ? itemHi - a : kRlTile);
      __syncthreads();  // the tile before is done with the LDS arrays
      *reinterpret_cast<uint4 *>(sStart + 16 * tid) = make_uint4(0, 0, 0, 0);
      if (tid == 0) { sPend = pend; sAny = 0; }
      __syncthreads();
      // the counted records that start in [a, a + len)
      auto mark = [&](uint64_t j, uint64_t i) {
        const uint64_t at = j * b.chunk + b.rat[j * b.slots + i];
        const uint64_t e = b.ren[j * b.slots + i];
        sStart[at - a] = 1;
        sEnd[at - a] = uint16_t((e < a + len ? e : a + len) - a);
        sAny = 1;
        if (e > a + len) sPend = e;  // (one record at most reaches past the tile)
      };
      if (perItem == 1) {
        const uint64_t kj = k0 + cur;
        uint64_t cnt = b.cnt[j0];
        if (kj >= max) cnt = cur;
        else if (max - k0 < cnt) cnt = max - k0;
        const uint64_t rel = a + len - itemLo;
        for (uint64_t i = cur + tid; i < cnt && b.rat[j0 * b.slots + i] < rel; i += kRlThreads)
          mark(j0, i);
      } else {
        for (uint64_t j = j0 + (tid >> 6); j < j1; j += kRlThreads / 64) {
          const uint64_t kj = rlFirstRecord(b, j);
          uint64_t cnt = b.cnt[j];
          if (kj >= max) cnt = 0;
          else if (max - kj < cnt) cnt = max - kj;
          for (uint64_t i = tid & 63u; i < cnt; i += 64) mark(j, i);
        }
      }
      __syncthreads();
      const uint32_t c0 = pend > a ? uint32_t((pend < a + len ? pend : a + len) - a) : 0u;
      const bool any = sAny != 0;
      const uint64_t pendNext = sPend;
      if (!any) {
        // no record starts here: covered, a plain shifted copy, or both in turn
        const uint64_t cnt = len - c0;
        if (out && cnt && outAt < outCap)
          rlStoreWide(out + outAt, p + a + c0, cnt < outCap - outAt ? cnt : outCap - outAt);
        outAt += cnt;
        pend = pendNext;
        continue;
      }
      // this lane's 16 bytes
      const uint32_t x0 = 16 * tid;
      uint32_t words[4] = {0, 0, 0, 0};
      if (x0 + 16 <= len) {
        uint4 v;
        __builtin_memcpy(&v, p + a + x0, 16);
        words[0] = v.x; words[1] = v.y; words[2] = v.z; words[3] = v.w;
      } else {
        for (uint32_t k = 0; x0 + k < len; ++k) words[k >> 2] |= uint32_t(p[a + x0 + k]) << (8 * (k & 3));
      }
      const uint4 sv = *reinterpret_cast<const uint4 *>(sStart + x0);
      const uint32_t starts[4] = {sv.x, sv.y, sv.z, sv.w};
      uint32_t nStarts = 0, lastEnd = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((starts[k >> 2] >> (8 * (k & 3))) & 1u) { ++nStarts; lastEnd = sEnd[x0 + k]; }
      uint32_t cov = rlScanMax(lastEnd, sWm);
      if (c0 > cov) cov = c0;
      // which of the 16 are kept (bit k), walking "covered up to" through the record starts
      uint32_t kept = 0;
      {
        uint32_t cv = cov;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if ((starts[k >> 2] >> (8 * (k & 3))) & 1u) cv = sEnd[x0 + k];
          if (x0 + k >= cv && x0 + k < len) kept |= 1u << k;
        }
      }
      uint64_t tileOut = 0;
      const uint64_t mine = uint64_t(__popc(kept)) + replLen * nStarts;
      const uint64_t off = rlScanSum(mine, sWs, tileOut);
      uint32_t tileStarts = 0;
      if (perItem == 1) {
        uint64_t ts = 0;
        (void)rlScanSum(nStarts, sWs, ts);
        tileStarts = uint32_t(ts);
      }
      // the tile's output [outAt, outAt + tileOut) below outCap, staged in windows of kRlStage
      // bytes whose byte 0 sits on a 16-byte boundary of the destination
      const uint64_t room = outAt < outCap ? outCap - outAt : 0;
      const uint64_t put = out ? (tileOut < room ? tileOut : room) : 0;
      if (put) {
        uint8_t *dst = out + outAt;
        const uint64_t mis = reinterpret_cast<uintptr_t>(dst) & 15;
        for (uint64_t w0 = 0; w0 < mis + put; w0 += kRlStage) {
          // window: stage coordinates [w0, w0 + kRlStage), output offset = coordinate - mis
          const uint64_t lo = w0 > mis ? w0 : mis;
          const uint64_t hi = w0 + kRlStage < mis + put ? w0 + kRlStage : mis + put;
          __syncthreads();  // the window before is flushed
          if (mis + off < hi && mis + off + mine > lo) {
            uint64_t o = mis + off;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              if ((starts[k >> 2] >> (8 * (k & 3))) & 1u) {
                const uint64_t f = o > lo ? o : lo;
                const uint64_t t = o + replLen < hi ? o + replLen : hi;
                for (uint64_t i = f; i < t; ++i) sStage[i - w0] = repl[i - o];
                o += replLen;
              }
              if ((kept >> k) & 1u) {
                if (o >= lo && o < hi) sStage[o - w0] = uint8_t(words[k >> 2] >> (8 * (k & 3)));
                ++o;
              }
            }
          }
          __syncthreads();
          rlStoreWide(dst + (lo - mis), sStage + (lo - w0), hi - lo);
        }
      }
      outAt += tileOut;
      cur += tileStarts;
      pend = pendNext;
    }
  }
}

// the assembly behind a final chain: sums, scans, sizes, and (out != nullptr) the copy
inline hipError_t launchRlAssemble(const uint8_t *p, uint64_t n, const ClBufs &b, const RlBufs &r,
                                   const uint8_t *repl, uint64_t replLen, uint64_t max,
                                   uint64_t *count, uint64_t *outLen, bool plan, uint8_t *out,
                                   uint64_t outCap, const LaunchCfg &cfg, hipStream_t stream) {
  const uint64_t nb = (b.m + 1023) / 1024;
  if (plan) {
    uint64_t sb = (b.m + 3) / 4;
    if (sb > uint64_t(cfg.numCUs) * 16) sb = uint64_t(cfg.numCUs) * 16;
    hipLaunchKernelGGL(k_rl_sum, dim3(uint32_t(sb)), dim3(256), 0, stream, b, r, max);
    hipLaunchKernelGGL((k_long_scan1<true, uint64_t>), dim3(uint32_t(nb)), dim3(1024), 0, stream, b.m,
                       static_cast<const uint64_t *>(r.rem), r.rem, r.cov, r.blockRem, r.blockCov,
                       static_cast<const uint32_t *>(nullptr));
    hipLaunchKernelGGL(k_rl_scan2, dim3(1), dim3(1024), 0, stream, r, nb, n, replLen, max, count,
                       outLen);
  }
  if (out && outCap) {
    const uint32_t perItem = b.chunk >= kRlTile ? 1u : kRlTile / b.chunk;
    const uint64_t nItems = (b.m + perItem - 1) / perItem;
    uint64_t blocks = nItems;
    if (blocks > uint64_t(cfg.numCUs) * 32) blocks = uint64_t(cfg.numCUs) * 32;
    hipLaunchKernelGGL(k_rl_copy, dim3(uint32_t(blocks)), dim3(kRlThreads), 0, stream, p, n, b, r,
                       repl, replLen, max, nItems, perItem, out, outCap);
  }
  return hipGetLastError();
}
