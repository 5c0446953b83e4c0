// extract_window_test.cpp - k_extract_text.h's XtWindow on the host: random outputs cut into random
// runs ("lanes"), each written through a window in random order with random put sizes, stretches
// skipped as the hand-off to the wave skips them, random out_cap and all 16 alignments of out.
// Every byte below the cap must be right and no byte outside [out, out + cap) touched; built with
// -fsanitize=address,undefined by tests/test_extract_text_window.py, which cuts the struct out of
// the header into xt_window.inc.  Usage: extract_window_test <iterations>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <utility>
#define __device__
#define __forceinline__ inline
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
#include "xt_window.inc"  // struct XtWindow, cut out of k_extract_text.h by the test

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const int iters = atoi(argv[1]);
  srand(12345);
  for (int iter = 0; iter < iters; ++iter) {
    const int mis = rand() % 16;
    const int total = 1 + rand() % 300;
    // exact-size allocations: the sanitizer sees a store outside [out - mis rounded, ...)
    std::vector<uint8_t> want(total), backing(16 + total + 16, 0x55);
    // out at a chosen misalignment inside an aligned block
    uint8_t *raw = backing.data();
    uint8_t *aligned = raw + ((16 - (reinterpret_cast<uintptr_t>(raw) & 15)) & 15);
    if (aligned + 16 + total > raw + backing.size()) continue;
    uint8_t *out = aligned + mis;
    const uint64_t cap = rand() % 3 ? uint64_t(total) : uint64_t(rand() % (total + 1));
    // lanes: consecutive runs
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (uint64_t d = 0; d < uint64_t(total);) {
      uint64_t mine = 1 + rand() % 40;
      if (d + mine > uint64_t(total)) mine = total - d;
      runs.push_back({d, mine});
      d += mine;
    }
    for (auto &x : want) x = uint8_t(rand());
    for (size_t i = runs.size(); i > 1; --i) std::swap(runs[i - 1], runs[rand() % i]);
    for (auto &r : runs) {
      uint64_t dst = r.first, mine = r.second;
      XtWindow w;
      w.base = out - mis;
      const uint64_t stop = dst + mine < cap ? dst + mine : cap;
      w.end = mis + stop;
      w.open(mis + dst);
      // pieces of 1..8 bytes, sometimes a skipped stretch (a piece handed to the wave)
      uint64_t at = dst;
      while (at < dst + mine) {
        uint64_t left = dst + mine - at;
        if (rand() % 7 == 0 && dst < cap) {
          uint64_t n = 1 + rand() % 20;
          if (n > left) n = left;
          w.close();
          if (w.at != mis + at && !w.full()) { printf("at mismatch\n"); return 1; }
          // the wave's copy, cut at cap
          for (uint64_t i = 0; i < n; ++i) if (at + i < cap) out[at + i] = want[at + i];
          w.open(mis + at + n);
          at += n;
          continue;
        }
        uint32_t k = 1 + rand() % 8;
        if (k > left) k = uint32_t(left);
        uint64_t v = 0;
        memcpy(&v, want.data() + at, k);
        if (k < 8) v |= 0xAAAAAAAAAAAAAAAAull << (8 * k);  // garbage above the k bytes
        w.put(v, k);
        at += k;
      }
      w.close();
    }
    const uint64_t k = cap < uint64_t(total) ? cap : total;
    if (memcmp(out, want.data(), k)) { printf("MISMATCH iter %d mis %d total %d cap %lu\n", iter, mis, total, cap); return 1; }
    for (uint8_t *p = raw; p < out; ++p) if (*p != 0x55) { printf("front sentinel iter %d\n", iter); return 1; }
    for (uint8_t *p = out + k; p < raw + backing.size(); ++p) if (*p != 0x55) { printf("back sentinel iter %d mis %d total %d cap %lu at %ld\n", iter, mis, total, cap, long(p - out)); return 1; }
  }
  printf("window ok\n");
  return 0;
}
