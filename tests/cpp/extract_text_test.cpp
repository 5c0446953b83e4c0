// extract_text_test.cpp - redgpu::extractText (include/redgpu.hpp) through the C-ABI.
// Usage: extract_text_test <dfa.reda> <text file> <max per line> <out prefix>
// Writes <prefix>.all (every match of every line, one per line) and <prefix>.some (the first
// <max per line> of a line) and prints "all <matches> <lines>", "some <matches> <lines>"; the pytest
// side compares them with what it computes from the oracle.
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

static void spill(const std::string &path, const std::string &bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), std::streamsize(bytes.size()));
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t most = size_t(std::strtoull(argv[3], nullptr, 10));
    const std::string prefix = argv[4];
    std::string out = "stale";
    size_t lines = 0;
    size_t found = extractText(rex, text, out, SIZE_MAX, '\n', &lines);
    std::printf("all %zu %zu\n", found, lines);
    spill(prefix + ".all", out);
    found = extractText(rex, text, out, most, '\n', &lines);
    std::printf("some %zu %zu\n", found, lines);
    spill(prefix + ".some", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
