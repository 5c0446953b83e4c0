// fields_text_test.cpp - redgpu::fieldsText (include/redgpu.hpp) through the C-ABI.
// Usage: fields_text_test <dfa.reda> <text file> <select mask, hex> <max fields> <out prefix>
// Writes <prefix>.all (the selected fields of every line joined by ", ") and <prefix>.some (the
// same under <max fields>, lines without a separator left out, joined by nothing) and prints
// "all <emitted> <fields> <lines>", "some <emitted> <fields> <lines>"; the pytest side compares
// them with what it computes from the oracle.
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
    const uint64_t select = std::strtoull(argv[3], nullptr, 16);
    const size_t most = size_t(std::strtoull(argv[4], nullptr, 10));
    const std::string prefix = argv[5];
    std::string out = "stale";
    size_t lines = 0, fields = 0;
    size_t emitted = fieldsText(rex, text, select, out, ", ", 0, false, '\n', &lines, &fields);
    std::printf("all %zu %zu %zu\n", emitted, fields, lines);
    spill(prefix + ".all", out);
    emitted = fieldsText(rex, text, select, out, "", most, true, '\n', &lines, &fields);
    std::printf("some %zu %zu %zu\n", emitted, fields, lines);
    spill(prefix + ".some", out);
  } catch (const std::exception &ex) {
    std::printf("EXCEPTION %s\n", ex.what());
    return 1;
  }
  return 0;
}
