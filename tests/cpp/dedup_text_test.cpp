// dedup_text_test.cpp - redgpu::dedupText (include/redgpu.hpp) through the C-ABI.
// Usage: dedup_text_test <dfa.reda> <text file> <key_index> <out prefix>
// Writes <prefix>.whole (awk '!seen[$0]++'), <prefix>.lines (the selected lines that occur once,
// the unselected ones kept), <prefix>.match (the first line per piece key_index) and
// <prefix>.field (every later duplicate of field key_index) and prints per call
// "<what> <lines> <keyed> <distinct> <dropped> <emitted> <out_len>"; the pytest side compares
// them with what the rule gives on the oracle's lines and pieces.
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

static void report(const char *what, const std::string &prefix, const DedupResult &r) {
  std::printf("%s %llu %llu %llu %llu %llu %llu\n", what,
              static_cast<unsigned long long>(r.lines), static_cast<unsigned long long>(r.keyed),
              static_cast<unsigned long long>(r.distinct),
              static_cast<unsigned long long>(r.dropped),
              static_cast<unsigned long long>(r.emitted),
              static_cast<unsigned long long>(r.outLen));
  std::ofstream f(prefix + "." + what, std::ios::binary);
  f.write(r.text.data(), std::streamsize(r.text.size()));
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t k = size_t(std::strtoull(argv[3], nullptr, 10));
    const std::string prefix = argv[4];
    report("whole", prefix, dedupText(rex, text));
    report("lines", prefix, dedupText(rex, text, dedupLines, 1, 1, 1, false, true, 4096));
    report("match", prefix, dedupText(rex, text, dedupMatch, k, 1, UINT64_MAX, false, false, 4096));
    report("field", prefix, dedupText(rex, text, dedupField, k, 1, UINT64_MAX, true, false, 4096));
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
