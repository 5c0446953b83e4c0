// collect_text_test.cpp - redgpu::collectText / collectTextCount (include/redgpu.hpp) through the
// C-ABI.
// Usage: collect_text_test <dfa.reda> <text file> <cap>
// Prints "count <collectTextCount> <lines>", "matches <n>" and one "line begin result start end"
// row per match; the pytest side compares them with what it computes from the oracle.
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

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t cap = size_t(std::strtoull(argv[3], nullptr, 10));
    size_t lines = 0;
    const size_t count = collectTextCount(rex, text, '\n', &lines);
    std::printf("count %zu %zu\n", count, lines);
    const std::vector<TextMatch> ms = collectText(rex, text, '\n', cap);
    std::printf("matches %zu\n", ms.size());
    for (const TextMatch &m : ms)
      std::printf("%zu %zu %d %zu %zu\n", m.line_, m.begin_, int(m.outcome_.result_),
                  m.outcome_.start_, m.outcome_.end_);
    // the defaults: '\n', no cap
    std::printf("default %zu\n", collectText(rex, text).size());
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
