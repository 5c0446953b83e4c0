// uniq_text_test.cpp - redgpu::uniqText (include/redgpu.hpp) through the C-ABI.
// Usage: uniq_text_test <dfa.reda> <text file> <max distinct>
// Prints "matches <lines> <items> <dropped> <records>" and one "<first> <length> <count>" row per
// record, then the same under "lines" for the lines styInstant selects; the pytest side compares
// them with what it computes from the oracle.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "redgpu.hpp"

using namespace redgpu;

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static void show(const char *what, const std::vector<UniqRecord> &recs, size_t lines, size_t items,
                 size_t dropped) {
  std::printf("%s %zu %zu %zu %zu\n", what, lines, items, dropped, recs.size());
  for (const UniqRecord &r : recs)
    std::printf("%llu %llu %llu\n", static_cast<unsigned long long>(r.first),
                static_cast<unsigned long long>(r.length),
                static_cast<unsigned long long>(r.count));
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t maxDistinct = size_t(std::strtoull(argv[3], nullptr, 10));
    size_t lines = 0, items = 0, dropped = 99;
    std::vector<UniqRecord> recs = uniqText(rex, text, true, maxDistinct, styInstant, true, SIZE_MAX,
                                            '\n', &items, &dropped, &lines);
    show("matches", recs, lines, items, dropped);
    recs = uniqText(rex, text, false, maxDistinct, styInstant, true, SIZE_MAX, '\n', &items,
                    &dropped, &lines);
    show("lines", recs, lines, items, dropped);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
