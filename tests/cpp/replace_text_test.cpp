// replace_text_test.cpp - redgpu::replaceText (include/redgpu.hpp) through the C-ABI.
// Usage: replace_text_test <dfa.reda> <text file> <repl> <max> <out prefix>
// Writes <prefix>.all (every line rewritten, styLast), <prefix>.changed (onlyChanged) and
// <prefix>.default (the defaults: no max, every line, '\n') and prints "all <replacements>",
// "changed <replacements>", "default <replacements>"; the pytest side compares them with what it
// computes from the oracle.
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
  if (argc < 6) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const std::string repl = argv[3];
    const size_t max = size_t(std::strtoull(argv[4], nullptr, 10));
    const std::string prefix = argv[5];
    std::string out = "stale";
    std::printf("all %zu\n", replaceText(rex, styLast, true, text, repl, out, max, false, '\n'));
    spill(prefix + ".all", out);
    std::printf("changed %zu\n", replaceText(rex, styLast, true, text, repl, out, max, true));
    spill(prefix + ".changed", out);
    std::printf("default %zu\n", replaceText(rex, styLast, true, text, repl, out));
    spill(prefix + ".default", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
