// host_stage_plan_test.cpp - one_amd/csrc/host_stage_plan.h on the host, under ASan + UBSan:
// stagePlan against a brute-force statement of its rule (a byte map: does this byte sit on a page
// that lies wholly inside the buffer?) and chunkCuts against the properties runHost relies on.
// Addresses are plain integers: nothing is allocated at them.
//   usage: host_stage_plan_test <random cases>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host_stage_plan.h"

using namespace redgpu;

static uint64_t gCases = 0;

#define REQUIRE(cond, ...)                                      \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                 \
      std::printf("\n");                                        \
      std::exit(1);                                             \
    }                                                           \
  } while (0)

// ---- the brute-force rule ------------------------------------------------------------------
// by division, not by the plan's masks: the page of byte i of [a, a + n) lies inside the buffer
static bool owned(uint64_t a, uint64_t n, uint64_t i) {
  const uint64_t page = (a + i) / 4096;
  return page * 4096 >= a && (page + 1) * 4096 <= a + n;
}

static uint64_t ownedBytes(uint64_t a, uint64_t n) {  // whole pages inside, page by page
  uint64_t got = 0;
  for (uint64_t page = a / 4096; page * 4096 < a + n; ++page)
    if (page * 4096 >= a && (page + 1) * 4096 <= a + n) got += 4096;
  return got;
}

struct Want {
  int route;
  bool plainAll;     // one plain segment over everything
  bool plainOwned;   // plain = exactly the owned bytes
};

static Want wanted(uint64_t a, uint64_t n, bool callDirect, bool direct, bool pinned, bool reg) {
  const bool small = !direct && !callDirect && n <= (16u << 20);
  if (small) return {1, false, false};
  if (direct || pinned) return {0, true, false};
  if (reg && ownedBytes(a, n) >= 16 * 4096) return {2, false, true};
  return {1, false, false};  // refused, or fewer than 16 whole pages to register
}

// every property of one plan; byteMap: check every byte (else the segments' edges)
static void checkPlan(uint64_t a, uint64_t n, bool callDirect, bool direct, bool pinned, bool reg,
                      bool byteMap) {
  ++gCases;
  const StagePlan p = stagePlan(uintptr_t(a), size_t(n), callDirect, direct, pinned, reg);
  if (n == 0) {  // nothing moves, nothing is counted
    REQUIRE(p.segs.empty(), "a transfer of 0 bytes with %zu segments", p.segs.size());
    return;
  }
  const Want w = wanted(a, n, callDirect, direct, pinned, reg);
  REQUIRE(p.route == w.route, "a=%llu n=%llu cd=%d d=%d pin=%d reg=%d route %d want %d",
          (unsigned long long)a, (unsigned long long)n, callDirect, direct, pinned, reg, p.route,
          w.route);
  REQUIRE(p.route >= 0 && p.route <= 2, "route %d (never pageable)", p.route);
  // the segments tile [0, n) exactly once, in any order
  std::vector<StageSegment> s = p.segs;
  std::sort(s.begin(), s.end(),
            [](const StageSegment &x, const StageSegment &y) { return x.offset < y.offset; });
  uint64_t at = 0, plainBytes = 0, plainSegs = 0;
  for (const StageSegment &g : s) {
    REQUIRE(g.bytes > 0 && g.offset == at, "a=%llu n=%llu gap or overlap at %llu",
            (unsigned long long)a, (unsigned long long)n, (unsigned long long)at);
    at += g.bytes;
    if (g.bounced) {
      REQUIRE(g.bytes <= kStagePiece, "piece of %zu bytes", g.bytes);
    } else {
      plainBytes += g.bytes;
      ++plainSegs;
    }
  }
  REQUIRE(at == n, "a=%llu n=%llu tiled to %llu", (unsigned long long)a, (unsigned long long)n,
          (unsigned long long)at);
  if (p.route == 0) REQUIRE(plainSegs == 1 && plainBytes == n, "route 0 not one plain copy");
  if (p.route == 1) REQUIRE(plainSegs == 0, "route 1 with a plain segment");
  if (p.route == 2) {
    REQUIRE(plainSegs == 1 && !p.segs[0].bounced, "route 2: the plain segment comes first");
    const StageSegment &g = p.segs[0];
    REQUIRE((a + g.offset) % 4096 == 0 && (a + g.offset + g.bytes) % 4096 == 0, "not on pages");
    REQUIRE(g.bytes >= 16 * 4096, "plain segment of %zu bytes", g.bytes);
    REQUIRE(plainBytes == ownedBytes(a, n), "plain %llu owned %llu", (unsigned long long)plainBytes,
            (unsigned long long)ownedBytes(a, n));
    // plain exactly where the byte map says "owned"
    auto agree = [&](uint64_t i) {
      const bool inPlain = i >= g.offset && i < g.offset + g.bytes;
      REQUIRE(inPlain == owned(a, n, i), "a=%llu n=%llu byte %llu", (unsigned long long)a,
              (unsigned long long)n, (unsigned long long)i);
    };
    if (byteMap) {
      std::vector<uint8_t> map(n);
      for (uint64_t i = 0; i < n; ++i) map[i] = owned(a, n, i);
      for (uint64_t i = 0; i < n; ++i)
        REQUIRE((i >= g.offset && i < g.offset + g.bytes) == (map[i] != 0), "a=%llu n=%llu byte %llu",
                (unsigned long long)a, (unsigned long long)n, (unsigned long long)i);
    } else {
      for (const StageSegment &q : s) {
        agree(q.offset);
        agree(q.offset + q.bytes - 1);
      }
      agree(0);
      agree(n - 1);
    }
  }
}

static void planEdges() {
  const uint64_t P = 4096, lens[] = {0, 1, 16 * P - 1, 16 * P, 16 * P + 1, kStagePiece - 1,
                                     kStagePiece, kStagePiece + 1, kStageBounceMax,
                                     kStageBounceMax + 1, kStageDirectFrom - 1, kStageDirectFrom,
                                     kStageDirectFrom + 1,
                                     // where a buffer at any offset first owns 16 whole pages
                                     17 * P - 1, 17 * P, 17 * P + 1};
  const uint64_t base = uint64_t(0x7f12) << 28;  // page-aligned
  for (uint64_t off = 0; off < P; ++off)
    for (uint64_t n : lens)
      for (int bits = 0; bits < 16; ++bits) {
        const bool cd = bits & 1, d = bits & 2, pin = bits & 4, reg = bits & 8;
        // every byte against the map where the plan can register and the map is small
        const bool map = n <= 17 * P + 1 && cd && !d && !pin && reg;
        checkPlan(base + off, n, cd, d, pin, reg, map);
      }
}

static void planRandom(uint64_t count, std::mt19937_64 &rng) {
  for (uint64_t k = 0; k < count; ++k) {
    const uint64_t a = (rng() >> 20) + 4096;
    uint64_t n;
    switch (rng() % 4) {
      case 0: n = rng() % (40 * 4096); break;
      case 1: n = rng() % (uint64_t(40) << 20); break;
      case 2: n = 16 * 4096 + rng() % 8192 - 4096; break;
      default: n = (rng() % 64) * 4096 + rng() % 3 - 1 + 4096; break;
    }
    const int bits = int(rng() % 16);
    checkPlan(a, n, bits & 1, bits & 2, bits & 4, bits & 8, n <= (uint64_t(1) << 20) && k % 8 == 0);
  }
}

// buffers back to back (numpy's result / start / end): what is registered of one never shares a
// page with what is registered of its neighbour
static void planNeighbours(uint64_t count, std::mt19937_64 &rng) {
  for (uint64_t k = 0; k < count; ++k) {
    uint64_t a = (rng() >> 20) + 4096;
    uint64_t lastPage = 0;  // one past the last registered page so far
    bool any = false;
    for (int b = 0; b < 3; ++b) {
      const uint64_t n = rng() % 2 ? 4 * (rng() % (6u << 20)) : 16 * 4096 + rng() % 12288 - 4096;
      ++gCases;
      const StagePlan p = stagePlan(uintptr_t(a), size_t(n), true, false, false, true);
      if (p.route == 2) {
        const uint64_t lo = (a + p.segs[0].offset) / 4096;
        const uint64_t hi = (a + p.segs[0].offset + p.segs[0].bytes + 4095) / 4096;
        REQUIRE(!any || lo >= lastPage, "neighbours share registered page %llu",
                (unsigned long long)lo);
        // and only pages of this buffer alone
        REQUIRE(lo * 4096 >= a && hi * 4096 <= a + n, "registered outside the buffer");
        lastPage = hi;
        any = true;
      }
      a += n;  // the next one begins where this one ends
    }
  }
}

// ---- chunkCuts ---------------------------------------------------------------------------
static void checkCuts(const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t chunkBytes) {
  ++gCases;
  const uint64_t total = offsets ? offsets[n] : stride * n;
  const uint64_t base0 = offsets ? offsets[0] : 0;
  const std::vector<uint64_t> cuts = chunkCuts(offsets, stride, n, total, chunkBytes);
  REQUIRE(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == n, "cuts do not span 0..n");
  for (size_t c = 0; c + 1 < cuts.size(); ++c)
    REQUIRE(cuts[c] < cuts[c + 1], "cuts not ascending at %zu", c);
  auto startOf = [&](uint64_t line) { return offsets ? offsets[line] : line * stride; };
  if (total - base0 <= 2 * chunkBytes || n < 4096) {
    REQUIRE(cuts.size() == 2, "a small batch cut into %zu chunks", cuts.size() - 1);
    return;
  }
  for (size_t c = 0; c + 2 < cuts.size(); ++c) {  // every chunk but the last
    const uint64_t lo = cuts[c], hi = cuts[c + 1];
    if (offsets) {
      // at least chunkBytes of line starts, and no line more than needed for that
      REQUIRE(startOf(hi) - startOf(lo) >= chunkBytes, "chunk %zu too small", c);
      REQUIRE(hi == lo + 1 || startOf(hi - 1) - startOf(lo) < chunkBytes,
              "chunk %zu holds more than chunkBytes plus its last line", c);
    } else {
      REQUIRE(hi % 1024 == 0 && lo % 1024 == 0, "fixed-stride cut not a multiple of 1024 lines");
      // chunkBytes rounded down to 1024 lines, but never fewer than 1024 lines
      const uint64_t per = hi - lo;
      REQUIRE(per * stride <= chunkBytes || per == 1024, "fixed chunk %zu of %llu lines", c,
              (unsigned long long)per);
      REQUIRE((per + 1024) * stride > chunkBytes, "fixed chunk %zu smaller than it could be", c);
    }
  }
  if (!offsets)
    for (size_t c = 0; c + 1 < cuts.size(); ++c) REQUIRE(cuts[c] % 1024 == 0, "cut %zu", c);
}

static void cutsAll(uint64_t count, std::mt19937_64 &rng) {
  const uint64_t chunks[] = {uint64_t(8) << 20, uint64_t(32) << 20};
  const uint64_t strides[] = {1, 3, 7, 64, 100, 1000, 4096, 8191, 8192, 65536, 1 << 20, 9u << 20, 0};
  for (uint64_t cb : chunks)
    for (uint64_t st : strides) {
      const uint64_t around = st ? 2 * cb / st : 5000;
      for (uint64_t n : {uint64_t(1), uint64_t(4095), uint64_t(4096), uint64_t(4097), around - 1,
                         around, around + 1, around + 1025, 3 * around + 17, uint64_t(100000)})
        if (n >= 1 && n < (uint64_t(1) << 40) / (st ? st : 1)) checkCuts(nullptr, st, n, cb);
    }
  std::vector<uint64_t> off;
  for (uint64_t k = 0; k < count; ++k) {
    const uint64_t cb = chunks[rng() % 2];
    const uint64_t n = k % 5 == 0 ? 1 + rng() % 4200 : 4096 + rng() % 60000;
    // totals around 2 * cb and well beyond; now and then a line longer than a chunk
    const uint64_t want = rng() % 3 ? 2 * cb - 4096 + rng() % 8192 : cb + rng() % (6 * cb);
    const uint64_t avg = want / n + 1;
    off.assign(n + 1, 0);
    off[0] = rng() % 2 ? 0 : rng() % (3 * cb);  // a sub-batch: offsets[0] != 0
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t len = rng() % (2 * avg);
      if (rng() % 20000 == 0) len = cb + rng() % cb;
      if (rng() % 50 == 0) len = 0;
      off[i + 1] = off[i] + len;
    }
    checkCuts(off.data(), rng() % 2, n, cb);
  }
  // exactly at the edge: total - offsets[0] == 2 * chunkBytes, and one byte more
  for (uint64_t cb : chunks)
    for (uint64_t base : {uint64_t(0), uint64_t(12345)})
      for (uint64_t extra : {uint64_t(0), uint64_t(1)}) {
        const uint64_t n = 8192;
        off.assign(n + 1, 0);
        for (uint64_t i = 0; i <= n; ++i) off[i] = base + (2 * cb + extra) * i / n;
        checkCuts(off.data(), 0, n, cb);
      }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: host_stage_plan_test <random cases>\n");
    return 2;
  }
  const uint64_t count = std::strtoull(argv[1], nullptr, 10);
  std::mt19937_64 rng(20240521);
  planEdges();
  planRandom(count, rng);
  planNeighbours(count, rng);
  const uint64_t plans = gCases;
  cutsAll(count / 4 + 1, rng);
  std::printf("host stage plan ok: %llu transfer plans agreed with the brute-force rule, "
              "%llu chunk plans held\n",
              (unsigned long long)plans, (unsigned long long)(gCases - plans));
  return 0;
}
