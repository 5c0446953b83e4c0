// sum_text_test.cpp - redgpu::sumText (include/redgpu.hpp) through the C-ABI.
// Usage: sum_text_test <dfa.reda> <text file> <nBins>
// Prints "first", "last", "one" (maxPerLine = 1) and "default" blocks: a "<name> scalars" row with
// lines, items and numeric, then "<name> count" / "sum" / "min" / "max" rows of nBins + 1 values;
// the pytest side compares them with what it computes from the oracle.
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

static void row(const char *what, const char *which, const std::vector<uint64_t> &v) {
  std::printf("%s_%s", what, which);
  for (uint64_t x : v) std::printf(" %llu", static_cast<unsigned long long>(x));
  std::printf("\n");
}

static void block(const char *what, const SumStats &s) {
  row(what, "scalars", {s.lines, s.items, s.numeric});
  row(what, "count", s.count);
  row(what, "sum", s.sum);
  row(what, "min", s.min);
  row(what, "max", s.max);
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t nBins = size_t(std::strtoull(argv[3], nullptr, 10));
    block("first", sumText(rex, text, nBins, false));
    block("last", sumText(rex, text, nBins, true, SIZE_MAX, '\n'));
    block("one", sumText(rex, text, nBins, false, 1));
    // the defaults: the first run, every piece, '\n'
    block("default", sumText(rex, text, nBins));
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
