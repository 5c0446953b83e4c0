// k_long.h - what the long-text verbs share (k_collect_long.h, k_replace_long.h, k_search_long.h,
// k_match_all_long.h): the anchored attempt (longChain), the 1024-wide exclusive scan of a sum and
// an optional prefix max (longScan and the two scan kernels), a chunk's span, and on the host the
// launch plan (longPlan)
// (included by kernels.hip inside its namespace, in front of k_collect_long.h).
#pragma once

// the bytes [lo, hi) of chunk j, of `chunk` bytes, of a text of n
struct LongSpan {
  uint64_t lo, hi;
};
__device__ __forceinline__ LongSpan longSpan(uint64_t j, uint32_t chunk, uint64_t n) {
  const uint64_t lo = j * chunk;
  return LongSpan{lo, lo + chunk < n ? lo + chunk : n};
}

// whose attempt runs at a position: the style, and the leader test (lookingAt) in front
struct LongAttempt {
  int style = kStyLast;
  int lead = 0;
};

struct LongHit {
  int how;        // 0 = every position failed, 1 = a match, 2 = suffix-closed stop, 3 = out of budget
  uint64_t at;    // the attempt position (how != 0)
  uint32_t acc;   // the accepting state the result is read from
  uint64_t ms, me;
};

// The attempts at the positions [q, hi) of p[0, n) in order, up to the first that does not fail.
// An attempt is searchCore's inner loop (include/Matcher.h:557-640; replaceCore's is the same):
// Instant stops at the first accept, First and Tangent at the first non-accept behind one (First
// also where the result changes), Last at a pure dead end, Full likewise and only counts an accept
// in its last state; start is the last "left the initial state" (Matcher.h:588-593).  `left` = the
// bytes the attempts may still walk past their first (an attempt that never dies would otherwise
// walk to the end of the text on every lane); it is counted down per attempt.
// mark (search only): the leader test stands in front of a DFA whose initial state accepts -
// searchCore's result is that state's when NO position passes the test (Matcher.h:571,577-578),
// so the test comes first and a pass is noted in *ran.
// FIXED: the attempt is k_collect's, <styLast, false>, whatever `a` says - no style
// branch is compiled.  TRACK: ms is kept (else it is the attempt position).
template <bool FIXED, bool TRACK, class T>
__device__ __forceinline__ LongHit longChain(const T &tab, const LaneCtx &c, const StartFilter &flt,
                                             const uint8_t *p, uint64_t n, uint64_t q, uint64_t hi,
                                             uint64_t &left, const LongAttempt a, int mark = 0,
                                             uint64_t *ran = nullptr) {
  const int style = FIXED ? kStyLast : a.style;
  const int lead = FIXED ? 0 : a.lead;
  LongHit h{0, hi, 0, 0, 0};
  walkBytesPeek(p, q, hi, flt, [] {}, [&](uint32_t byte, uint64_t i, uint32_t nextByte) -> bool {
    // lookingAt's first byte (search only: in replace's chain the shortcut costs k_cl_rewalk and
    // k_cl_serial registers, profiles/long_shared_resources.md)
    if (TRACK && lead && c.eq[byte] != c.leader[0]) return true;
    if (mark) {
      if (!lookingAt(c, p, i, n)) return true;
      *ran = 1;
    }
    uint32_t st = tab.next(c.init, byte);
    bool any = false;
    uint64_t ms = i, me = i;
    uint32_t aS = 0;
    int32_t prev = 0;  // (styFirst) the result of the accepts so far
    if (st >= c.firstAccept) {
      aS = st; me = i + 1; any = true;
      if (style == kStyFirst) prev = c.res[st];
    }
    else if (st < c.nPureDead) return true;
    else if (nextByte != kNoPeek && tab.next(st, nextByte) < c.nPureDead) return true;
    if (lead && !mark && !lookingAt(c, p, i, n)) return true;
    const uint64_t lim = n - i - 1 > left ? i + 1 + left : n;
    uint64_t at = i + 1;
    auto stepOne = [&](uint32_t b2, uint64_t q2) -> bool {
      const uint32_t was = st;
      st = tab.next(st, b2);
      at = q2 + 1;
      if (TRACK && was == c.init && st != was) ms = q2;
      if (st >= c.firstAccept) {
        if (style == kStyFirst) {
          const int32_t r = c.res[st];
          if (prev && r != prev) return false;
          prev = r;
        }
        aS = st; me = q2 + 1; any = true;
        return style != kStyInstant;
      }
      if (style == kStyFull) any = false;
      else if (any && (style == kStyFirst || style == kStyTangent)) return false;
      return st >= c.nPureDead;
    };
    uint64_t q2 = i + 1;
    bool alive = !(any && style == kStyInstant);
    for (uint32_t k = 0; k < 6 && q2 < lim && alive; ++k, ++q2) alive = stepOne(uint32_t(p[q2]), q2);
    if (alive)
      walkBytes(p, q2, lim, [&](uint32_t b2, uint64_t q3) -> bool { return alive = stepOne(b2, q3); });
    left -= at - i - 1;
    h.at = i;
    if (alive && lim < n) { h.how = 3; return false; }
    if (!any) {
      if (c.suffixClosed && alive && !lead) { h.how = 2; return false; }  // L = SIGMA* L
      return true;
    }
    h.how = 1; h.acc = aS; h.ms = ms; h.me = me;
    return false;
  });
  if (h.how == 0) h.at = hi;
  return h;
}

template <int KIND>
__device__ __forceinline__ LaneCtx longCtx(const DevDfa &d, uint8_t *lds) {
  LaneCtx c{lds, lds + 256, resOf<KIND>(d, lds), d.init, d.leaderNext, d.nPureDead, d.firstAccept,
            d.leaderLen};
  c.suffixClosed = d.suffixClosed;
  return c;
}

__device__ __forceinline__ StartFilter longFilter(const DevDfa &d) {
  return StartFilter{d.startFreeWord, d.startFreeCount <= 4 ? d.startFreeCount : 0u,
                     d.start2FreeWord, d.start2FreeCount <= 4 ? d.start2FreeCount : 0u, false};
}

// What one of the 1024 threads of a workgroup gets from the scan of their values v (and w, MAX):
// the sum (max) of the threads in front of it, and of all 1024
struct LongScan {
  uint64_t sum, total, max, totalMax;
};

// s, x: 1024 words of LDS each (x unused without MAX); every thread calls, and may call again at once
template <bool MAX>
__device__ __forceinline__ LongScan longScan(uint64_t *s, uint64_t *x, uint64_t v, uint64_t w) {
  s[threadIdx.x] = v;
  if (MAX) x[threadIdx.x] = w;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const uint64_t add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    const uint64_t mx = MAX && threadIdx.x >= o ? x[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    if (MAX && mx > x[threadIdx.x]) x[threadIdx.x] = mx;
    __syncthreads();
  }
  LongScan r{s[threadIdx.x] - v, s[1023], 0, 0};
  if (MAX) {
    r.max = threadIdx.x ? x[threadIdx.x - 1] : 0;
    r.totalMax = x[1023];
  }
  __syncthreads();
  return r;
}

// one workgroup: the exclusive scans of the nb block totals in place (sum; mx, MAX); returns the sum
template <bool MAX>
__device__ __forceinline__ uint64_t longScanTotals(uint64_t *s, uint64_t *x, uint64_t *sum,
                                                   uint64_t *mx, uint64_t nb) {
  uint64_t carry = 0, carryMax = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += 1024) {
    const uint64_t i = t0 + threadIdx.x;
    const LongScan r = longScan<MAX>(s, x, i < nb ? sum[i] : 0, MAX && i < nb ? mx[i] : 0);
    if (i < nb) {
      sum[i] = carry + r.sum;
      if (MAX) mx[i] = r.max > carryMax ? r.max : carryMax;
    }
    carry += r.total;
    if (r.totalMax > carryMax) carryMax = r.totalMax;
  }
  return carry;
}

// fold 1: per 1024 chunks the exclusive sum of in[] to off[] and (MAX) the exclusive max of mx[] in
// place, block totals behind.  go: null, or a word that shuts the kernel when it is 0.
template <bool MAX, class V>
__global__ void __launch_bounds__(1024)
k_long_scan1(uint64_t m, const V *in, uint64_t *off, uint64_t *mx, uint64_t *blockSum,
             uint64_t *blockMax, const uint32_t *go) {
  __shared__ uint64_t s[1024], x[MAX ? 1024 : 1];
  if (go && !*go) return;
  const uint64_t j = uint64_t(blockIdx.x) * 1024 + threadIdx.x;
  const LongScan r = longScan<MAX>(s, x, j < m ? in[j] : 0, MAX && j < m ? mx[j] : 0);
  if (j < m) {
    off[j] = r.sum;
    if (MAX) mx[j] = r.max;
  }
  if (threadIdx.x == 1023) {
    blockSum[blockIdx.x] = r.total;
    if (MAX) blockMax[blockIdx.x] = r.totalMax;
  }
}

// fold 2: one workgroup, the same scans over the block totals in place; *count = the sum, 0 when
// `go` shuts the kernel
template <bool MAX>
__global__ void __launch_bounds__(1024)
k_long_scan2(uint64_t *blockSum, uint64_t *blockMax, uint64_t nb, const uint32_t *go,
             uint64_t *count) {
  __shared__ uint64_t s[1024], x[MAX ? 1024 : 1];
  if (go && !*go) {
    if (threadIdx.x == 0) *count = 0;
    return;
  }
  const uint64_t total = longScanTotals<MAX>(s, x, blockSum, blockMax, nb);
  if (threadIdx.x == 0) *count = total;
}

// The launch plan of a verb over m chunks of `chunk` bytes: the walk kernels stage the table
// (kStagedThreads<KIND> threads, at most one wave of resident workgroups), the bookkeeping kernels
// have 256 threads, and speculative attempts are bounded - 16 bytes per chunk byte past their
// first, and 1 KiB.
struct LongPlan {
  int threads;
  size_t ldsBytes;
  uint32_t blocks, small;
  uint64_t budget;
};

template <int KIND>
inline LongPlan longPlan(const DevDfa &d, uint64_t m, uint32_t chunk, const LaunchCfg &cfg) {
  LongPlan g{kStagedThreads<KIND>, 512 + ldsTableBytes<KIND>(d), 0, 0, uint64_t(chunk) * 16 + 1024};
  const uint64_t most = uint64_t(cfg.numCUs) * stagedPerCu<KIND>(g.ldsBytes);
  uint64_t blocks = (m + g.threads - 1) / g.threads;
  if (blocks > most) blocks = most;
  g.blocks = uint32_t(blocks ? blocks : 1);
  const uint64_t small = (m + 255) / 256;
  g.small = uint32_t(small > uint64_t(cfg.numCUs) * 8 ? uint64_t(cfg.numCUs) * 8 : small);
  return g;
}
