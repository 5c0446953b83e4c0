// grep_text_test.cpp - redgpu::grepText / grepCount (include/redgpu.hpp) through the C-ABI.
// Usage: grep_text_test <dfa.reda> <text file> <style> <doLeader> <invert> <max>
// Prints "count <grepCount>", "hits <n>" and one "line begin end result start end" row per hit;
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

int main(int argc, char **argv) {
  if (argc < 7) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const Style style = Style(std::atoi(argv[3]));
    const bool lead = std::atoi(argv[4]) != 0, invert = std::atoi(argv[5]) != 0;
    const size_t max = size_t(std::strtoull(argv[6], nullptr, 10));
    std::printf("count %zu\n", grepCount(rex, text, style, lead, invert, '\n', max));
    const std::vector<GrepHit> hits = grepText(rex, text, style, lead, invert, '\n', max);
    std::printf("hits %zu\n", hits.size());
    for (const GrepHit &h : hits)
      std::printf("%zu %zu %zu %d %zu %zu\n", h.line_, h.begin_, h.end_, int(h.outcome_.result_),
                  h.outcome_.start_, h.outcome_.end_);
    // the defaults: styInstant, the leader, no invert, '\n', no limit
    std::printf("default %zu %zu\n", grepText(rex, text).size(), grepCount(rex, text));
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
