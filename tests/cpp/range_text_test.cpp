// range_text_test.cpp - redgpu::rangeText (include/redgpu.hpp) through the C-ABI.
// Usage: range_text_test <dfa.reda> <text file> <open_result> <close_result> <out prefix>
// Writes <prefix>.print (sed -n '/open/,/close/p'), <prefix>.delete (sed '/open/,/close/d') and
// <prefix>.body (the ranges without their open and close lines, the first three ranges only) and
// prints per call "<what> <ranges> <emitted>", and behind the first call one line
// "range <first_line> <last_line> <begin> <end>" per range; the pytest side compares them with
// what the rule gives on the oracle's per-line values.
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

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const int32_t open = int32_t(std::strtol(argv[3], nullptr, 10));
    const int32_t close = int32_t(std::strtol(argv[4], nullptr, 10));
    const std::string prefix = argv[5];
    std::string out = "stale";
    std::vector<TextRange> ranges(2, TextRange{9, 9, 9, 9});
    size_t emitted = 0;
    size_t n = rangeText(rex, styInstant, true, text, open, close, out, true, true, false, SIZE_MAX,
                         '\n', &ranges, &emitted);
    std::printf("print %zu %zu\n", n, emitted);
    for (const TextRange &r : ranges)
      std::printf("range %llu %llu %llu %llu\n", static_cast<unsigned long long>(r.firstLine),
                  static_cast<unsigned long long>(r.lastLine),
                  static_cast<unsigned long long>(r.begin), static_cast<unsigned long long>(r.end));
    spill(prefix + ".print", out);
    n = rangeText(rex, styInstant, true, text, open, close, out, true, true, true, SIZE_MAX, '\n',
                  nullptr, &emitted);
    std::printf("delete %zu %zu\n", n, emitted);
    spill(prefix + ".delete", out);
    n = rangeText(rex, styInstant, true, text, open, close, out, false, false, false, 3, '\n',
                  nullptr, &emitted);
    std::printf("body %zu %zu\n", n, emitted);
    spill(prefix + ".body", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
