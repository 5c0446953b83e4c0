// group_text_test.cpp - redgpu::groupText (include/redgpu.hpp) through the C-ABI.
// Usage: group_text_test <dfa.reda> <text file> <key_index> <value_index>
// Runs groupMatch under FIRST and groupField under LAST and prints per call
// "<what> <lines> <keyed> <numeric> <distinct> <dropped>" and then per record
// "<first> <length> <count> <numeric> <sum> <min> <max>"; the pytest side compares them with what
// the rule gives on the oracle's lines and pieces.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "redgpu.hpp"

using namespace redgpu;

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static void report(const char *what, const GroupResult &r) {
  using ull = unsigned long long;
  std::printf("%s %llu %llu %llu %llu %llu\n", what, ull(r.lines), ull(r.keyed), ull(r.numeric),
              ull(r.distinct), ull(r.dropped));
  for (const GroupRecord &g : r.records)
    std::printf("%llu %llu %llu %llu %llu %llu %llu\n", ull(g.first), ull(g.length), ull(g.count),
                ull(g.numeric), ull(g.sum), ull(g.min), ull(g.max));
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t k = size_t(std::strtoull(argv[3], nullptr, 10));
    const size_t v = size_t(std::strtoull(argv[4], nullptr, 10));
    report("match", groupText(rex, text, groupMatch, k, v, false, 4096));
    report("field", groupText(rex, text, groupField, k, v, true, 4096));
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
