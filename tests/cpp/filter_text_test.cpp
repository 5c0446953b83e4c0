// filter_text_test.cpp - redgpu::filterText (include/redgpu.hpp) through the C-ABI.
// Usage: filter_text_test <dfa.reda> <text file> <before> <after> <most> <out prefix>
// Writes <prefix>.plain (the defaults: the selected lines alone), <prefix>.context (before / after
// lines around them) and <prefix>.inverted (the first <most> lines that do NOT match, with the same
// context) and prints "plain <selected> <emitted>", "context ...", "inverted ..."; the pytest side
// compares them with what it computes from the oracle.
#include <algorithm>
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
  if (argc < 7) return 2;
  try {
    Executable rex(slurp(argv[1]));
    const std::string text = slurp(argv[2]);
    const size_t before = size_t(std::strtoull(argv[3], nullptr, 10));
    const size_t after = size_t(std::strtoull(argv[4], nullptr, 10));
    const size_t most = size_t(std::strtoull(argv[5], nullptr, 10));
    const std::string prefix = argv[6];
    std::string out = "stale";
    size_t emitted = 0;
    size_t selected = filterText(rex, styLast, true, text, out);
    std::printf("plain %zu %zu\n", selected, size_t(std::count(out.begin(), out.end(), '\n')));
    spill(prefix + ".plain", out);
    selected = filterText(rex, styLast, true, text, out, false, before, after, SIZE_MAX, '\n',
                          &emitted);
    std::printf("context %zu %zu\n", selected, emitted);
    spill(prefix + ".context", out);
    selected = filterText(rex, styLast, true, text, out, true, before, after, most, '\n', &emitted);
    std::printf("inverted %zu %zu\n", selected, emitted);
    spill(prefix + ".inverted", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
