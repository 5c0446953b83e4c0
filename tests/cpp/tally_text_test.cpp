// tally_text_test.cpp - redgpu::tallyText (include/redgpu.hpp) through the C-ABI.
// Usage: tally_text_test <dfa.reda> <text file> <nBins>
// Prints "matches", "lines instant", "lines last" and "default" rows, each followed by its
// nBins + 1 counts; the pytest side compares them with what it computes from the oracle.
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

static void row(const char *what, const std::vector<uint64_t> &bins) {
  std::printf("%s", what);
  for (uint64_t v : bins) std::printf(" %llu", static_cast<unsigned long long>(v));
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t nBins = size_t(std::strtoull(argv[3], nullptr, 10));
    row("matches", tallyText(rex, text, nBins, true));
    row("instant", tallyText(rex, text, nBins, false, styInstant, true, '\n'));
    row("last", tallyText(rex, text, nBins, false, styLast, false));
    // the defaults: one item per match, '\n'
    row("default", tallyText(rex, text, nBins));
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
