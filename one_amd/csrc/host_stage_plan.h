// host_stage_plan.h - the DECISIONS of the host-buffer staging as pure functions: which way one
// transfer of caller memory goes (HostStage::move executes the plan) and where a host-buffer
// batch is cut into chunks (runHost).  No HIP in here: tests/cpp/host_stage_plan_test.cpp compiles
// this header alone on the host and holds both against a brute-force statement of their rules.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace redgpu {

// a transfer of up to kStageBounceMax bytes, in a call that uploads less than kStageDirectFrom,
// goes through the thread's pinned arena, in pieces of at most kStagePiece; registration is by
// pages of kStagePage, and fewer than kStageMinPages whole pages are not worth registering
constexpr size_t kStageBounceMax = size_t(16) << 20;
constexpr size_t kStageDirectFrom = size_t(8) << 20;
constexpr size_t kStagePiece = size_t(4) << 20;
constexpr uintptr_t kStagePage = 4096;
constexpr size_t kStageMinPages = 16;

// routes, as redgpu_host_route_counts counts them (3, "handed over pageable", is never planned)
enum StageRoute : int { kRouteCallerPinned = 0, kRouteArena = 1, kRouteRegistered = 2 };

struct StageSegment {
  size_t offset, bytes;  // [offset, offset + bytes) of the transfer
  bool bounced;          // through the arena (one piece) / copied as it is
};

struct StagePlan {
  int route;
  std::vector<StageSegment> segs;  // tile [0, bytes) exactly once
};

// One transfer of `bytes` of caller memory at `address`.
//  * callDirect: the call uploads kStageDirectFrom bytes or more (HostStage::beginCall);
//  * direct: the entry point knows the caller pinned the memory;
//  * pinnedBothEnds: the runtime knows the first and the last byte as pinned (only looked at
//    where the transfer does not go through the arena anyway);
//  * registerSucceeds: the runtime registers the whole pages of the range when asked.
// Route 2's plain segment comes first: the whole pages that lie inside the range, registered for
// the call; the partial pages at its two ends follow as arena pieces.
inline StagePlan stagePlan(uintptr_t address, size_t bytes, bool callDirect, bool direct,
                           bool pinnedBothEnds, bool registerSucceeds) {
  StagePlan p{kRouteArena, {}};
  if (bytes == 0) return p;
  auto bounced = [&](size_t at, size_t n) {
    for (size_t done = 0; done < n; done += kStagePiece)
      p.segs.push_back(StageSegment{at + done, n - done < kStagePiece ? n - done : kStagePiece, true});
  };
  if (!direct && !callDirect && bytes <= kStageBounceMax) {
    bounced(0, bytes);
    return p;
  }
  if (direct || pinnedBothEnds) {
    p.route = kRouteCallerPinned;
    p.segs.push_back(StageSegment{0, bytes, false});
    return p;
  }
  const uintptr_t a = address;
  const uintptr_t lo = (a + kStagePage - 1) & ~(kStagePage - 1), hi = (a + bytes) & ~(kStagePage - 1);
  if (hi > lo && hi - lo >= kStageMinPages * kStagePage && registerSucceeds) {
    p.route = kRouteRegistered;
    const size_t head = lo - a, tail = a + bytes - hi;
    p.segs.push_back(StageSegment{head, size_t(hi - lo), false});
    bounced(0, head);
    bounced(bytes - tail, tail);
    return p;
  }
  bounced(0, bytes);
  return p;
}

// chunk plan of a host-buffer batch: cuts[c] .. cuts[c + 1] are the lines of chunk c
inline std::vector<uint64_t> chunkCuts(const uint64_t *offsets, uint64_t stride, uint64_t n,
                                       uint64_t total, uint64_t chunkBytes) {
  std::vector<uint64_t> cuts{0};
  const uint64_t base0 = offsets ? offsets[0] : 0;
  if (total - base0 > 2 * chunkBytes && n >= 4096) {
    if (!offsets) {
      uint64_t per = (chunkBytes / (stride ? stride : 1)) & ~uint64_t(1023);
      if (per < 1024) per = 1024;
      for (uint64_t lo = per; lo < n; lo += per) cuts.push_back(lo);
    } else {
      uint64_t lo = 0;
      while (lo < n) {
        // first line whose start is >= chunkBytes past this chunk's start
        const uint64_t target = offsets[lo] + chunkBytes;
        uint64_t a = lo + 1, b = n;
        while (a < b) {
          const uint64_t mid = (a + b) / 2;
          if (offsets[mid] >= target) b = mid; else a = mid + 1;
        }
        lo = a;
        if (lo < n) cuts.push_back(lo);
      }
    }
  }
  cuts.push_back(n);
  return cuts;
}

}  // namespace redgpu
