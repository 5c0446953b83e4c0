// route_text_test.cpp - redgpu::routeText (include/redgpu.hpp) through the C-ABI.
// Usage: route_text_test <dfa.reda> <text file> <n_bins> <out prefix>
// Writes <prefix>.all (every line, grouped by bucket) and <prefix>.matched (the lines that do not
// match left out) and prints per call "all <lines> <routed>" / "matched <lines> <routed>", then
// "lines <bin_lines ...>" and "offsets <bin_offsets ...>"; the pytest side compares them with what
// it computes from the oracle.
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

static void spill(const std::string &path, const std::string &bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), std::streamsize(bytes.size()));
}

static void show(const char *what, const std::vector<uint64_t> &v) {
  std::printf("%s", what);
  for (uint64_t x : v) std::printf(" %llu", static_cast<unsigned long long>(x));
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t nBins = size_t(std::strtoull(argv[3], nullptr, 10));
    const std::string prefix = argv[4];
    std::string out = "stale";
    std::vector<uint64_t> binLines(3, 99), binOffsets;
    size_t lines = 0;
    size_t routed = routeText(rex, styInstant, true, text, nBins, out, binLines, binOffsets);
    std::printf("all %zu %zu\n", size_t(0), routed);
    show("lines", binLines);
    show("offsets", binOffsets);
    spill(prefix + ".all", out);
    routed = routeText(rex, styInstant, true, text, nBins, out, binLines, binOffsets, true, '\n',
                       &lines);
    std::printf("matched %zu %zu\n", lines, routed);
    show("lines", binLines);
    show("offsets", binOffsets);
    spill(prefix + ".matched", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
