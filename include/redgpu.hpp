// redgpu.hpp - C++ mirror of RED's matcher interface over the C-ABI of redgpu.h.
//
// Same names, argument meaning and error behaviour as the reference for the hot path
// (citations relative to /root/reference/quol/red/):
//   Executable        include/Executable.h:28-76   (validated serialized DFA; move-only)
//   Style             include/Matcher.h:67-74
//   Result / Outcome  include/Types.h:22, include/Outcome.h:32-51
//   check/match/scan  include/Matcher.h:79-92 (run-time style, doLeader = true) and
//                     :133-169 (template <Style, bool doLeader>)
//   RedExcept*        include/Except.h:30-107
// plus the batch forms (checkBatch / matchBatch / scanBatch) that replace the callers'
// per-input loops (tools/bench.cpp:60-71, tools/thr_red.cpp:36-47).  Header-only; link with
// one_amd/libredgpu.so.  Single-input calls are batches of one ON THE GPU - there is no CPU
// matcher behind this header.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "redgpu.h"

namespace redgpu {

typedef uint8_t Byte;
typedef int32_t Result;

enum Style {
  styInvalid = 0,
  styInstant = 1,
  styFirst = 2,
  styTangent = 3,
  styLast = 4,
  styFull = 5,
};

struct Outcome {
  Result result_;
  size_t start_;
  size_t end_;
  bool operator==(const Outcome &rhs) const {
    return result_ == rhs.result_ && start_ == rhs.start_ && end_ == rhs.end_;
  }
  explicit operator bool() const { return result_ > 0; }
  static Outcome fail() { return Outcome{0, 0, 0}; }
};

class RedExcept : public std::runtime_error { using std::runtime_error::runtime_error; };
class RedExceptInternal : public RedExcept { using RedExcept::RedExcept; };
class RedExceptUser : public RedExcept { using RedExcept::RedExcept; };
class RedExceptLimit : public RedExcept { using RedExcept::RedExcept; };
class RedExceptExec : public RedExceptInternal { using RedExceptInternal::RedExceptInternal; };
class RedExceptApi : public RedExceptUser { using RedExceptUser::RedExceptUser; };
class RedExceptHip : public RedExceptExec { using RedExceptExec::RedExceptExec; };  // new

inline void throwOnError(int rc) {
  if (rc == REDGPU_OK) return;
  const std::string msg = redgpu_last_error();
  switch (rc) {
  case REDGPU_EAPI: throw RedExceptApi(msg);
  case REDGPU_EEXEC: throw RedExceptExec(msg);
  case REDGPU_ELIMIT: throw RedExceptLimit(msg);
  case REDGPU_EHIP: throw RedExceptHip(msg);
  default: throw RedExcept(msg);
  }
}

namespace detail {
// a size_t limit (SIZE_MAX = none) as the uint64_t count of the C calls
inline uint64_t clampCount(size_t n) { return n > (1ull << 62) ? 1ull << 62 : uint64_t(n); }

// `out` of a verb that assembles a text: call(out, cap) makes the C call with that output, which
// leaves out_len in outLen.  A first call with (nullptr, 0) only sizes; the second one fetches, when
// there are bytes or alsoFetch() - asked once, behind the first call - has something of its own.
template <class F, class G = bool (*)()>
void sizedText(std::string &out, const uint64_t &outLen, F &&call,
               G alsoFetch = [] { return false; }) {
  call(nullptr, 0);
  out.resize(size_t(outLen));
  if (alsoFetch() || outLen) call(reinterpret_cast<Byte *>(out.data()), outLen);
}
}  // namespace detail

// tag types kept for source compatibility (include/Types.h:43-53); every constructor COPIES
struct CopyTag {};
constexpr CopyTag gCopyTag;
struct UnownedTag {};
constexpr UnownedTag gUnownedTag;

class Executable {
public:
  Executable() : h_(nullptr) {}
  Executable(Executable &&other) : h_(std::exchange(other.h_, nullptr)) {}
  explicit Executable(std::string &&buf, int device = REDGPU_DEVICE_CURRENT) : h_(nullptr) {
    if (buf.empty()) throw RedExceptApi("serialized dfa move-string is empty");
    init(buf.data(), buf.size(), device);
  }
  Executable(const CopyTag &, std::string_view sv, int device = REDGPU_DEVICE_CURRENT)
      : h_(nullptr) {
    if (sv.empty()) throw RedExceptApi("serialized dfa string_view is empty");
    init(sv.data(), sv.size(), device);
  }
  Executable(const UnownedTag &, std::string_view sv, int device = REDGPU_DEVICE_CURRENT)
      : h_(nullptr) {
    if (!sv.data()) throw RedExceptApi("serialized dfa unowned-view is empty");
    init(sv.data(), sv.size(), device);
  }
  ~Executable() { redgpu_dfa_destroy(h_); }
  Executable &operator=(Executable &&rhs) {
    if (this != &rhs) {
      redgpu_dfa_destroy(h_);
      h_ = std::exchange(rhs.h_, nullptr);
    }
    return *this;
  }
  Executable(const Executable &) = delete;
  Executable &operator=(const Executable &) = delete;

  std::string_view serialized() const {
    const void *p = nullptr;
    size_t n = 0;
    throwOnError(redgpu_dfa_serialized(h_, &p, &n));
    return std::string_view(static_cast<const char *>(p), n);
  }
  redgpu_info info() const {
    redgpu_info i;
    throwOnError(redgpu_dfa_info(h_, &i));
    return i;
  }
  const redgpu_dfa *handle() const { return h_; }

private:
  void init(const void *p, size_t n, int device) {
    redgpu_opts o{};
    o.device = device;
    throwOnError(redgpu_dfa_create(p, n, &o, &h_));
  }
  redgpu_dfa *h_;
};

// ---- batch forms: line i = data[offsets[i], offsets[i+1]) (offsets has n+1 entries), or with
// offsets == nullptr, data[i*stride, (i+1)*stride).  Host buffers. -----------------------------
template <Style style, bool doLeader>
void checkBatch(const Executable &exec, const Byte *data, const uint64_t *offsets, uint64_t stride,
                uint64_t n, Result *result) {
  throwOnError(redgpu_check_batch(exec.handle(), style, doLeader, data, offsets, stride, n, result));
}

template <Style style, bool doLeader>
void matchBatch(const Executable &exec, const Byte *data, const uint64_t *offsets, uint64_t stride,
                uint64_t n, Result *result, uint64_t *start, uint64_t *end) {
  throwOnError(redgpu_match_batch(exec.handle(), style, doLeader, data, offsets, stride, n, result,
                                  start, end));
}

template <Style style, bool doLeader>
void scanBatch(const Executable &exec, const Byte *data, const uint64_t *offsets, uint64_t stride,
               uint64_t n, Result *result) {
  throwOnError(redgpu_scan_batch(exec.handle(), style, doLeader, data, offsets, stride, n, result));
}

inline std::vector<Outcome> matchBatch(const Executable &exec, const std::vector<std::string_view> &lines,
                                       Style style, bool doLeader = true) {
  std::string flat;
  std::vector<uint64_t> off(lines.size() + 1, 0);
  for (size_t i = 0; i < lines.size(); ++i) {
    flat.append(lines[i]);
    off[i + 1] = flat.size();
  }
  std::vector<Result> r(lines.size());
  std::vector<uint64_t> s(lines.size()), e(lines.size());
  throwOnError(redgpu_match_batch(exec.handle(), style, doLeader,
                                  reinterpret_cast<const Byte *>(flat.data()), off.data(), 0,
                                  lines.size(), r.data(), s.data(), e.data()));
  std::vector<Outcome> out(lines.size());
  for (size_t i = 0; i < lines.size(); ++i) out[i] = Outcome{r[i], size_t(s[i]), size_t(e[i])};
  return out;
}

// The lines of a text blob (lib/Util.cpp:109-130's rule: [start, delimiter), bytes behind the last
// delimiter are not a line), each matched - the loop of tools/skim_red.cpp:36-46 in one call.
// lineStarts (optional) receives where each line begins in `text`; Outcome positions are relative
// to that, as if the line had been handed to match() on its own.
inline std::vector<Outcome> matchText(const Executable &exec, std::string_view text, Style style,
                                      bool doLeader = true, char delim = '\n',
                                      std::vector<size_t> *lineStarts = nullptr) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t n = 0, none = 0;
  throwOnError(redgpu_split_lines(exec.handle(), p, text.size(), Byte(delim), &none, 0, &n));
  std::vector<uint64_t> off(n + 1, 0), s(n), e(n);
  std::vector<Result> r(n);
  throwOnError(redgpu_match_text(exec.handle(), style, doLeader, p, text.size(), Byte(delim),
                                 off.data(), n, &n, r.data(), s.data(), e.data()));
  std::vector<Outcome> out(r.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = Outcome{r[i], size_t(s[i]), size_t(e[i])};
  if (lineStarts) lineStarts->assign(off.begin(), off.begin() + out.size());
  return out;
}

// grep (include/Red.h:65: "searchInstant() - appropriate for grep"; tools/skim_red.cpp:36-46): the
// lines of a text blob that search<style,doLeader> selects - result > 0, or the others under
// invert - in text order, at most max of them.  line_ = the line's 0-based index, [begin_, end_) =
// the line in `text` (end_ = its delimiter), outcome_ = search on that line alone (positions
// relative to begin_; {0, 0, 0} under invert).
struct GrepHit {
  size_t line_, begin_, end_;
  Outcome outcome_;
};

// room for text.size() / 128 + 16 records first, one retry with the exact count
inline std::vector<GrepHit> grepText(const Executable &exec, std::string_view text,
                                     Style style = styInstant, bool doLeader = true,
                                     bool invert = false, char delim = '\n',
                                     size_t max = SIZE_MAX) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t cap = text.size() / 128 + 16, found = 0;
  std::vector<uint64_t> ln, bg, fn, s, e;
  std::vector<Result> r;
  for (int attempt = 0; attempt < 2; ++attempt) {
    ln.resize(cap); bg.resize(cap); fn.resize(cap); s.resize(cap); e.resize(cap); r.resize(cap);
    throwOnError(redgpu_grep_text(exec.handle(), style, doLeader, invert, p, text.size(),
                                  Byte(delim), max, cap, nullptr, &found, ln.data(), bg.data(),
                                  fn.data(), r.data(), s.data(), e.data()));
    if (found <= cap) break;
    cap = found;
  }
  std::vector<GrepHit> out(found < cap ? found : cap);
  for (size_t i = 0; i < out.size(); ++i)
    out[i] = GrepHit{size_t(ln[i]), size_t(bg[i]), size_t(fn[i]),
                     Outcome{r[i], size_t(s[i]), size_t(e[i])}};
  return out;
}

// grep -c: the count alone, no records
inline size_t grepCount(const Executable &exec, std::string_view text, Style style = styInstant,
                        bool doLeader = true, bool invert = false, char delim = '\n',
                        size_t max = SIZE_MAX) {
  uint64_t found = 0;
  throwOnError(redgpu_grep_text(exec.handle(), style, doLeader, invert,
                                reinterpret_cast<const Byte *>(text.data()), text.size(),
                                Byte(delim), max, 0, nullptr, &found, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr));
  return size_t(found);
}

// grep -o (Red::collect, lib/Red.cpp:103-116, inside tools/skim_red.cpp:36-46's line loop): every
// match of every line of a text blob, in text order, at most cap of them.  line_ = the line's
// 0-based index, begin_ = where it begins in `text`, outcome_ = the match with start_ / end_ as
// offsets in `text` (collectLong's convention; start_ - begin_ is the position in the line).
struct TextMatch {
  size_t line_, begin_;
  Outcome outcome_;
};

// room for text.size() / 64 + 16 records first, one retry with the exact count
inline std::vector<TextMatch> collectText(const Executable &exec, std::string_view text,
                                          char delim = '\n', size_t cap = SIZE_MAX) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t room = text.size() / 64 + 16, found = 0;
  if (room > cap) room = cap;
  std::vector<uint64_t> ln, bg, s, e;
  std::vector<Result> r;
  for (int attempt = 0; attempt < 2; ++attempt) {
    ln.resize(room); bg.resize(room); s.resize(room); e.resize(room); r.resize(room);
    throwOnError(redgpu_collect_text(exec.handle(), p, text.size(), Byte(delim), room, nullptr,
                                     &found, ln.data(), bg.data(), r.data(), s.data(), e.data()));
    if (found <= room || room == cap) break;
    room = found < cap ? found : cap;
  }
  std::vector<TextMatch> out(found < room ? found : room);
  for (size_t i = 0; i < out.size(); ++i)
    out[i] = TextMatch{size_t(ln[i]), size_t(bg[i]), Outcome{r[i], size_t(s[i]), size_t(e[i])}};
  return out;
}

// the counts alone, no records: the matches of all lines; lines (optional) = delimiters found
inline size_t collectTextCount(const Executable &exec, std::string_view text, char delim = '\n',
                               size_t *lines = nullptr) {
  uint64_t found = 0, nLines = 0;
  throwOnError(redgpu_collect_text(exec.handle(), reinterpret_cast<const Byte *>(text.data()),
                                   text.size(), Byte(delim), 0, &nLines, &found, nullptr, nullptr,
                                   nullptr, nullptr, nullptr));
  if (lines) *lines = size_t(nLines);
  return size_t(found);
}

// grep -c per result / grep -o | sort | uniq -c (redgpu_tally_text): nBins + 1 counts, [r] = the
// items of value r < nBins, [nBins] = everything else.  matches = true: one item per match of
// every line (collectText's records, style and doLeader not looked at); false: one item per line,
// its value the result of search<style,doLeader> on it, 0 when it does not match.
inline std::vector<uint64_t> tallyText(const Executable &exec, std::string_view text, size_t nBins,
                                       bool matches = true, Style style = styInstant,
                                       bool doLeader = true, char delim = '\n') {
  std::vector<uint64_t> bins(nBins + 1);
  throwOnError(redgpu_tally_text(exec.handle(), matches ? REDGPU_TALLY_MATCHES : REDGPU_TALLY_LINES,
                                 style, doLeader, reinterpret_cast<const Byte *>(text.data()),
                                 text.size(), Byte(delim), nBins, 0, nullptr, nullptr,
                                 bins.data()));
  return bins;
}

// per result the count, sum, minimum and maximum of the numbers in the matches (redgpu_sum_text):
// nBins + 1 slots, [r] = the items of result r < nBins, [nBins] = everything else.  The items are
// extractText's pieces (at most maxPerLine of a line); an item's number is the first (last = false)
// or last run of digits 0-9 inside the piece, read as an unsigned decimal.  An item without a digit,
// or with a run of 2^64 or more, is in `items` and in no statistic.  Sums are modulo 2^64; a slot
// without numeric items has count 0, sum 0, min 2^64 - 1, max 0.
struct SumStats {
  std::vector<uint64_t> count, sum, min, max;  // nBins + 1 each
  uint64_t lines = 0, items = 0, numeric = 0;  // delimiters found, pieces, pieces with a number
};
inline SumStats sumText(const Executable &exec, std::string_view text, size_t nBins,
                        bool last = false, size_t maxPerLine = SIZE_MAX, char delim = '\n') {
  const size_t slots = nBins + 1;
  const uint64_t most = detail::clampCount(maxPerLine);
  std::vector<uint64_t> stats(4 * slots);
  SumStats out;
  throwOnError(redgpu_sum_text(exec.handle(), last ? REDGPU_SUM_LAST : REDGPU_SUM_FIRST,
                               reinterpret_cast<const Byte *>(text.data()), text.size(),
                               Byte(delim), most, nBins, 0, &out.lines, &out.items, &out.numeric,
                               stats.data()));
  auto row = [&](int r) {
    return std::vector<uint64_t>(stats.begin() + r * slots, stats.begin() + (r + 1) * slots);
  };
  out.count = row(REDGPU_SUM_COUNT);
  out.sum = row(REDGPU_SUM_SUM);
  out.min = row(REDGPU_SUM_MIN);
  out.max = row(REDGPU_SUM_MAX);
  return out;
}

// grep -o | sort | uniq -c keyed by the matched bytes (redgpu_uniq_text): one UniqRecord per
// distinct byte string among the text's items, in the order of first appearance - the string is
// text.substr(first, length), count all its occurrences.  matches = true: the items are
// extractText's pieces (at most maxPerLine of a line); false: the lines search<style,doLeader>
// selects, without their delimiters.  The hash table holds the power of two at or above
// 2 * maxDistinct (at least 64) strings; *dropped = the items in no record (2^24 bytes or longer,
// or the table was full: call again with a larger maxDistinct), *items = all items, *lines =
// delimiters found.
struct UniqRecord {
  uint64_t first, length, count;
};
inline std::vector<UniqRecord> uniqText(const Executable &exec, std::string_view text,
                                        bool matches = true, size_t maxDistinct = size_t(1) << 20,
                                        Style style = styInstant, bool doLeader = true,
                                        size_t maxPerLine = SIZE_MAX, char delim = '\n',
                                        size_t *items = nullptr, size_t *dropped = nullptr,
                                        size_t *lines = nullptr) {
  uint64_t slots = 64;
  while (slots < 2 * uint64_t(maxDistinct) && slots < (1ull << 32)) slots *= 2;
  const uint64_t rows = slots < text.size() ? slots : text.size();
  std::vector<uint64_t> first(rows), length(rows), count(rows);
  uint64_t nLines = 0, nItems = 0, nDistinct = 0, nDropped = 0;
  throwOnError(redgpu_uniq_text(exec.handle(), matches ? REDGPU_UNIQ_MATCHES : REDGPU_UNIQ_LINES,
                                style, doLeader, reinterpret_cast<const Byte *>(text.data()),
                                text.size(), Byte(delim), maxPerLine, slots, rows, &nLines, &nItems,
                                &nDistinct, &nDropped, first.data(), length.data(), count.data()));
  std::vector<UniqRecord> out(size_t(nDistinct < rows ? nDistinct : rows));
  for (size_t j = 0; j < out.size(); ++j) out[j] = UniqRecord{first[j], length[j], count[j]};
  if (items) *items = size_t(nItems);
  if (dropped) *dropped = size_t(nDropped);
  if (lines) *lines = size_t(nLines);
  return out;
}

// sed (replace<style,doLeader>, include/Matcher.h:186-191, inside tools/skim_red.cpp:36-46's line
// loop): every line of a text blob rewritten and the text put back together in `out` - the lines,
// their delimiters, and the tail behind the last delimiter unchanged.  max is per line (1 = sed
// s/x/y/, SIZE_MAX = s/x/y/g); onlyChanged = sed -n 's/x/y/p': the changed lines alone, no tail.
// Returns the replacements made.  `out` is sized from a first call that only sizes.
inline size_t replaceText(const Executable &exec, Style style, bool doLeader,
                          std::string_view text, std::string_view repl, std::string &out,
                          size_t max = SIZE_MAX, bool onlyChanged = false, char delim = '\n') {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  const Byte *r = reinterpret_cast<const Byte *>(repl.data());
  uint64_t made = 0, outLen = 0;
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_replace_text(exec.handle(), style, doLeader, onlyChanged, p, text.size(),
                                     Byte(delim), r, repl.size(), detail::clampCount(max), nullptr,
                                     &made, &outLen, o, cap));
  });
  return size_t(made);
}

// grep (redgpu_filter_text): the lines of a text blob that search<style,doLeader> selects - the
// others under invert, the first `most` of them - with `before` lines in front of and `after` lines
// behind each (grep -B / -A), put together in `out`: every emitted line once, in text order, with
// its delimiter, no group separator; the tail behind the last delimiter is never emitted.  Returns
// the lines selected; *emitted = the lines in `out`.  `out` is sized from a first call that only sizes.
inline size_t filterText(const Executable &exec, Style style, bool doLeader, std::string_view text,
                         std::string &out, bool invert = false, size_t before = 0,
                         size_t after = 0, size_t most = SIZE_MAX, char delim = '\n',
                         size_t *emitted = nullptr) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t selected = 0, lines = 0, outLen = 0;
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_filter_text(exec.handle(), style, doLeader, invert, before, after,
                                    detail::clampCount(most), p, text.size(), Byte(delim), nullptr,
                                    &selected, &lines, &outLen, o, cap));
  });
  if (emitted) *emitted = size_t(lines);
  return size_t(selected);
}

// awk '{ print > file[class] }' (redgpu_route_text): every line of a text blob put in `out`, grouped
// by the result search<style,doLeader> reports for it - bucket r for a result r < nBins, bucket
// nBins for everything else (nBins <= 255), the lines of a bucket in text order with their
// delimiters; lines that do not match are left out under dropUnmatched (and still counted).
// binLines[b] = the lines of bucket b (nBins + 1 of them), binOffsets[b] = where its section begins
// in `out` (nBins + 2: the last one is out.size()).  Returns the lines emitted; *lines = delimiters
// found.  `out` is sized from a first call that only sizes.
inline size_t routeText(const Executable &exec, Style style, bool doLeader, std::string_view text,
                        size_t nBins, std::string &out, std::vector<uint64_t> &binLines,
                        std::vector<uint64_t> &binOffsets, bool dropUnmatched = false,
                        char delim = '\n', size_t *lines = nullptr) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  if (nBins > 255) throw RedExceptLimit("n_bins too large");
  binLines.assign(nBins + 1, 0);
  binOffsets.assign(nBins + 2, 0);
  uint64_t found = 0, routed = 0, outLen = 0;
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_route_text(exec.handle(), style, doLeader, dropUnmatched, p, text.size(),
                                   Byte(delim), nBins, &found, &routed, binLines.data(),
                                   binOffsets.data(), &outLen, o, cap));
  });
  if (lines) *lines = size_t(found);
  return size_t(routed);
}

// one /open/,/close/ range of rangeText: its first and last line, and text[begin, end)
struct TextRange {
  uint64_t firstLine, lastLine, begin, end;
};

// sed -n '/open/,/close/p' (redgpu_range_text): the lines of a text blob read in text order -
// outside a range a line whose search<style,doLeader> result is openResult begins one, inside it
// the next line whose result is closeResult ends it (openResult == closeResult: one pattern
// toggles), a range still open at the last line ends there; only the first `most` ranges count.
// `out` gets a counted range's body lines, its open line under emitOpen and its close line under
// emitClose - under invert exactly the other lines (sed '/A/,/B/d') - in text order with their
// delimiters; the tail behind the last delimiter is never emitted.  ranges, when given, gets one
// record per counted range, whatever is emitted.  Returns the ranges counted; *emitted = the lines
// in `out`.  `out` and the records are sized from a first call that only sizes.
inline size_t rangeText(const Executable &exec, Style style, bool doLeader, std::string_view text,
                        int32_t openResult, int32_t closeResult, std::string &out,
                        bool emitOpen = true, bool emitClose = true, bool invert = false,
                        size_t most = SIZE_MAX, char delim = '\n',
                        std::vector<TextRange> *ranges = nullptr, size_t *emitted = nullptr) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t found = 0, lines = 0, outLen = 0, n = 0;
  std::vector<uint64_t> rec;  // the four columns, n each: sized behind the first call
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    uint64_t *r = n ? rec.data() : nullptr;
    throwOnError(redgpu_range_text(exec.handle(), style, doLeader, openResult, closeResult,
                                   emitOpen, emitClose, invert, detail::clampCount(most), p,
                                   text.size(), Byte(delim), nullptr, &found, &lines, &outLen, o,
                                   cap, n, r, r ? r + n : nullptr, r ? r + 2 * n : nullptr,
                                   r ? r + 3 * n : nullptr));
  }, [&] {
    rec.resize(ranges ? size_t(found) * 4 : 0);
    return (n = rec.size() / 4) != 0;
  });
  if (ranges) {
    ranges->clear();
    for (uint64_t i = 0; i < n; ++i)
      ranges->push_back(TextRange{rec[i], rec[n + i], rec[2 * n + i], rec[3 * n + i]});
  }
  if (emitted) *emitted = size_t(lines);
  return size_t(found);
}

// what dedupText says beside the text: redgpu_dedup_text's six counters and the emitted lines
struct DedupResult {
  uint64_t lines = 0, keyed = 0, distinct = 0, dropped = 0, emitted = 0, outLen = 0;
  std::string text;
};

// which bytes of a line are its key (REDGPU_DEDUP_*)
enum DedupWhat { dedupWhole = 0, dedupLines = 1, dedupMatch = 2, dedupField = 3 };

// awk '!seen[$k]++' (redgpu_dedup_text): the lines of a text blob chosen by the content of their
// keys - a line's key is the line (dedupWhole; the DFA is not walked), the line if
// search<style,doLeader> selects it (dedupLines), piece keyIndex extractText emits for it
// (dedupMatch) or its field keyIndex with the DFA as the separator (dedupField); a line without
// one is unkeyed.  A keyed line is marked iff it holds the earliest occurrence of its key's string
// and minCount <= count <= maxCount; the text gets the keyed lines with marked != invert and,
// under keepUnkeyed, the unkeyed ones, in text order with their delimiters; the tail behind the
// last delimiter is never emitted.  The hash table holds the power of two at or above
// 2 * maxDistinct (at least 64) strings; dropped = the keyed lines whose key got no record (2^24
// bytes or longer, or the table was full: call again with a larger maxDistinct).  The text is
// sized from a first call that only sizes.
inline DedupResult dedupText(const Executable &exec, std::string_view text,
                             DedupWhat what = dedupWhole, size_t keyIndex = 1,
                             uint64_t minCount = 1, uint64_t maxCount = UINT64_MAX,
                             bool invert = false, bool keepUnkeyed = false,
                             size_t maxDistinct = size_t(1) << 20, Style style = styInstant,
                             bool doLeader = true, char delim = '\n') {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t slots = 64;
  while (slots < 2 * uint64_t(maxDistinct) && slots < (1ull << 32)) slots *= 2;
  DedupResult r;
  detail::sizedText(r.text, r.outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_dedup_text(exec.handle(), what, style, doLeader, keyIndex, minCount,
                                   maxCount, invert, keepUnkeyed, p, text.size(), Byte(delim),
                                   slots, &r.lines, &r.keyed, &r.distinct, &r.dropped, &r.emitted,
                                   &r.outLen, o, cap));
  });
  return r;
}

// one key of groupText: the key is text.substr(first, length), its earliest occurrence; count = the
// keyed lines with that key; numeric / sum (modulo 2^64) / min / max over those of them that have a
// number (0, 0, 2^64 - 1, 0 without any)
struct GroupRecord {
  uint64_t first, length, count, numeric, sum, min, max;
};

// what groupText says: the records in the order of first appearance and redgpu_group_text's scalars
struct GroupResult {
  std::vector<GroupRecord> records;
  uint64_t lines = 0, keyed = 0, numeric = 0, distinct = 0, dropped = 0;
};

// which items a line is cut into (REDGPU_GROUP_*)
enum GroupWhat { groupMatch = 0, groupField = 1 };

// awk '{ n[$k]++; s[$k] += $v; if ($v > m[$k]) m[$k] = $v }' (redgpu_group_text): one GroupRecord
// per distinct key string of a text blob's lines.  A line's items are the pieces extractText emits
// for it (groupMatch) or its fields with the DFA as the separator (groupField), numbered from 1;
// item keyIndex is the key - a line with fewer items is unkeyed - and item valueIndex (0 = none) the
// value, whose number is sumText's: the first (last = false) or last run of digits 0-9 inside the
// item.  The hash table holds the power of two at or above 2 * maxDistinct (at least 64) strings;
// dropped = the keyed lines in no record (a key of 2^24 bytes or longer, or the table was full: call
// again with a larger maxDistinct), which enter no record with either their count or their number.
inline GroupResult groupText(const Executable &exec, std::string_view text,
                             GroupWhat what = groupField, size_t keyIndex = 1,
                             size_t valueIndex = 2, bool last = false,
                             size_t maxDistinct = size_t(1) << 20, char delim = '\n') {
  uint64_t slots = 64;
  while (slots < 2 * uint64_t(maxDistinct) && slots < (1ull << 32)) slots *= 2;
  const uint64_t rows = slots < text.size() ? slots : text.size();
  std::vector<uint64_t> first(rows), length(rows), count(rows), stats(4 * rows);
  GroupResult r;
  throwOnError(redgpu_group_text(exec.handle(), what, keyIndex, valueIndex,
                                 last ? REDGPU_SUM_LAST : REDGPU_SUM_FIRST,
                                 reinterpret_cast<const Byte *>(text.data()), text.size(),
                                 Byte(delim), slots, rows, &r.lines, &r.keyed, &r.numeric,
                                 &r.distinct, &r.dropped, first.data(), length.data(),
                                 count.data(), stats.data()));
  r.records.resize(size_t(r.distinct < rows ? r.distinct : rows));
  for (size_t j = 0; j < r.records.size(); ++j)
    r.records[j] = GroupRecord{first[j], length[j], count[j],
                               stats[REDGPU_SUM_COUNT * rows + j], stats[REDGPU_SUM_SUM * rows + j],
                               stats[REDGPU_SUM_MIN * rows + j], stats[REDGPU_SUM_MAX * rows + j]};
  return r;
}

// grep -o as a text (redgpu_extract_text): every match of every line of a text blob put in `out`,
// one per line - the bytes replace<styLast,false> would substitute, each followed by the delimiter,
// in text order; at most maxPerLine of a line (1 = its first match).  Output line j is the bytes of
// collectText's record j, from where the matching attempt began (at or before start_) to end_.
// Returns the matches emitted; *lines = delimiters found.  `out` is sized from a first call that
// only sizes.
inline size_t extractText(const Executable &exec, std::string_view text, std::string &out,
                          size_t maxPerLine = SIZE_MAX, char delim = '\n',
                          size_t *lines = nullptr) {
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t found = 0, nLines = 0, outLen = 0;
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_extract_text(exec.handle(), p, text.size(), Byte(delim),
                                     detail::clampCount(maxPerLine), &nLines, &found, &outLen, o,
                                     cap));
  });
  if (lines) *lines = size_t(nLines);
  return size_t(found);
}

// awk -F / cut as a text (redgpu_fields_text): the DFA describes the separator; the fields of every
// line of a text blob that `select` names (bit k - 1 = field k, bit 63 = field 64 and every later
// one) put in `out`, joined by sep (at most 8 bytes), one output line per emitted line.  maxFields
// > 0: a line has at most that many fields, the last is the rest of the line.  onlyDelimited
// (cut -s): lines without a separator are left out.  Returns the lines emitted; *lines =
// delimiters found, *fields = fields written.  `out` is sized from a first call that only sizes.
inline size_t fieldsText(const Executable &exec, std::string_view text, uint64_t select,
                         std::string &out, std::string_view sep = " ", size_t maxFields = 0,
                         bool onlyDelimited = false, char delim = '\n', size_t *lines = nullptr,
                         size_t *fields = nullptr) {
  if (sep.size() > 8) throw RedExceptApi("fieldsText: sep is longer than 8 bytes");
  const Byte *p = reinterpret_cast<const Byte *>(text.data());
  uint64_t sepWord = 0;
  for (size_t i = 0; i < sep.size(); ++i) sepWord |= uint64_t(Byte(sep[i])) << (8 * i);
  const uint32_t sepLen = uint32_t(sep.size());
  uint64_t nLines = 0, emitted = 0, nFields = 0, outLen = 0;
  detail::sizedText(out, outLen, [&](Byte *o, uint64_t cap) {
    throwOnError(redgpu_fields_text(exec.handle(), p, text.size(), Byte(delim), select, maxFields,
                                    onlyDelimited, sepWord, sepLen, &nLines, &emitted, &nFields,
                                    &outLen, o, cap));
  });
  if (lines) *lines = size_t(nLines);
  if (fields) *fields = size_t(nFields);
  return size_t(emitted);
}

// ---- several GPUs of one node: one image per device, contiguous shards, results in the caller's
// arrays - the device form of tools/thr_red.cpp:84-91 (N workers over one shared Red).  devices
// may name a device more than once (the shards then share it). ----------------------------------
class Group {
public:
  Group(std::string_view serialized, const std::vector<int32_t> &devices) : g_(nullptr) {
    if (serialized.empty()) throw RedExceptApi("serialized dfa string_view is empty");
    throwOnError(redgpu_group_create(serialized.data(), serialized.size(), nullptr, devices.data(),
                                     uint32_t(devices.size()), &g_));
  }
  ~Group() { redgpu_group_destroy(g_); }
  Group(const Group &) = delete;
  Group &operator=(const Group &) = delete;
  uint32_t size() const { return redgpu_group_size(g_); }
  const redgpu_dfa *member(uint32_t i) const { return redgpu_group_member(g_, i); }
  // shard g = lines [cuts[g], cuts[g + 1]): equal lines, or equal bytes when offsets are given
  std::vector<uint64_t> plan(const uint64_t *offsets, uint64_t stride, uint64_t n) const {
    std::vector<uint64_t> cuts(size() + 1);
    throwOnError(redgpu_group_plan(g_, offsets, stride, n, cuts.data()));
    return cuts;
  }
  template <Style style, bool doLeader>
  void matchBatch(const Byte *data, const uint64_t *offsets, uint64_t stride, uint64_t n,
                  Result *result, uint64_t *start, uint64_t *end) const {
    throwOnError(redgpu_group_batch(g_, REDGPU_VERB_MATCH, style, doLeader, data, offsets, stride, n,
                                    result, start, end));
  }
  template <Style style, bool doLeader>
  void checkBatch(const Byte *data, const uint64_t *offsets, uint64_t stride, uint64_t n,
                  Result *result) const {
    throwOnError(redgpu_group_batch(g_, REDGPU_VERB_CHECK, style, doLeader, data, offsets, stride, n,
                                    result, nullptr, nullptr));
  }
  redgpu_group *handle() const { return g_; }

private:
  redgpu_group *g_;
};

// ---- single-input forms with the reference's signatures (a batch of one on the GPU) ---------
namespace detail {
inline Result one(int (*fn)(const redgpu_dfa *, int, int, const uint8_t *, const uint64_t *,
                            uint64_t, uint64_t, int32_t *),
                  const Executable &exec, const void *ptr, size_t len, int style, bool lead) {
  const uint64_t off[2] = {0, len};
  Result r = 0;
  throwOnError(fn(exec.handle(), style, lead, static_cast<const Byte *>(ptr), off, 0, 1, &r));
  return r;
}
} // namespace detail

template <Style style, bool doLeader>
Result check(const Executable &exec, const void *ptr, size_t len) {
  return detail::one(redgpu_check_batch, exec, ptr, len, style, doLeader);
}
template <Style style, bool doLeader>
Result check(const Executable &exec, std::string_view sv) {
  return check<style, doLeader>(exec, sv.data(), sv.size());
}
template <Style style, bool doLeader>
Result scan(const Executable &exec, const void *ptr, size_t len) {
  return detail::one(redgpu_scan_batch, exec, ptr, len, style, doLeader);
}
template <Style style, bool doLeader>
Result scan(const Executable &exec, std::string_view sv) {
  return scan<style, doLeader>(exec, sv.data(), sv.size());
}
template <Style style, bool doLeader>
Outcome match(const Executable &exec, const void *ptr, size_t len) {
  const uint64_t off[2] = {0, len};
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_match_batch(exec.handle(), style, doLeader, static_cast<const Byte *>(ptr),
                                  off, 0, 1, &r, &s, &e));
  return Outcome{r, size_t(s), size_t(e)};
}
template <Style style, bool doLeader>
Outcome match(const Executable &exec, std::string_view sv) {
  return match<style, doLeader>(exec, sv.data(), sv.size());
}

// search<style,doLeader>: include/Matcher.h:172-182,557-640 (sliding-window match)
template <Style style, bool doLeader>
Outcome search(const Executable &exec, std::string_view sv) {
  const uint64_t off[2] = {0, sv.size()};
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_search_batch(exec.handle(), style, doLeader,
                                   reinterpret_cast<const Byte *>(sv.data()), off, 0, 1, &r, &s, &e));
  return Outcome{r, size_t(s), size_t(e)};
}
inline Outcome search(const Executable &exec, std::string_view sv, Style style) {
  const uint64_t off[2] = {0, sv.size()};
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_search_batch(exec.handle(), style, 1,
                                   reinterpret_cast<const Byte *>(sv.data()), off, 0, 1, &r, &s, &e));
  return Outcome{r, size_t(s), size_t(e)};
}
template <Style style, bool doLeader>
void searchBatch(const Executable &exec, const Byte *data, const uint64_t *offsets, uint64_t stride,
                 uint64_t n, Result *result, uint64_t *start, uint64_t *end) {
  throwOnError(redgpu_search_batch(exec.handle(), style, doLeader, data, offsets, stride, n, result,
                                   start, end));
}

namespace detail {
// the two list verbs: first try with room for 16 records, retry once with the exact count
template <class F>
size_t listOne(F call, const Executable &exec, std::string_view sv, std::vector<Outcome> &out) {
  const uint64_t off[2] = {0, sv.size()};
  uint64_t cap = 16, found = 0;
  std::vector<Result> r;
  std::vector<uint64_t> s, e;
  for (int pass = 0; pass < 2; ++pass) {
    r.assign(cap, 0);
    s.assign(cap, 0);
    e.assign(cap, 0);
    throwOnError(call(exec.handle(), reinterpret_cast<const Byte *>(sv.data()), off, cap, &found,
                      r.data(), s.data(), e.data()));
    if (found <= cap) break;
    cap = found;
  }
  out.clear();
  for (uint64_t i = 0; i < found; ++i) out.push_back(Outcome{r[i], size_t(s[i]), size_t(e[i])});
  return out.size();
}
} // namespace detail

// matchAll(exec, sv, out): include/Matcher.h:127, lib/Matcher.cpp:97-102 (doLeader = true)
inline size_t matchAll(const Executable &exec, std::string_view sv, std::vector<Outcome> &out) {
  return detail::listOne(
      [](const redgpu_dfa *h, const Byte *p, const uint64_t *off, uint64_t cap, uint64_t *cnt,
         Result *r, uint64_t *s, uint64_t *e) {
        return redgpu_match_all_batch(h, 1, p, off, 0, 1, cap, cnt, r, s, e);
      },
      exec, sv, out);
}

// Red::collect(text, out): include/Red.h:115, lib/Red.cpp:103-116
inline size_t collect(const Executable &exec, std::string_view sv, std::vector<Outcome> &out) {
  return detail::listOne(
      [](const redgpu_dfa *h, const Byte *p, const uint64_t *off, uint64_t cap, uint64_t *cnt,
         Result *r, uint64_t *s, uint64_t *e) {
        return redgpu_collect_batch(h, p, off, 0, 1, cap, cnt, r, s, e);
      },
      exec, sv, out);
}

// Red::collect(text, out) over one long text, chunk-parallel on the device (redgpu_collect_long):
// room for 16 records first, one retry with the exact count, as detail::listOne
inline size_t collectLong(const Executable &exec, std::string_view sv, std::vector<Outcome> &out) {
  uint64_t cap = 16, found = 0;
  std::vector<Result> r;
  std::vector<uint64_t> s, e;
  for (int pass = 0; pass < 2; ++pass) {
    r.assign(cap, 0);
    s.assign(cap, 0);
    e.assign(cap, 0);
    throwOnError(redgpu_collect_long(exec.handle(), reinterpret_cast<const Byte *>(sv.data()),
                                     sv.size(), 0, cap, &found, r.data(), s.data(), e.data()));
    if (found <= cap) break;
    cap = found;
  }
  out.clear();
  for (uint64_t i = 0; i < found; ++i) out.push_back(Outcome{r[i], size_t(s[i]), size_t(e[i])});
  return out.size();
}

// matchAll(exec, sv, out) (include/Matcher.h:127, lib/Matcher.cpp:97-102: doLeader = true) over one
// long text, chunk-parallel on the device (redgpu_match_all_long): room for 16 records first, one
// retry with the exact count, as collectLong
inline size_t matchAllLong(const Executable &exec, std::string_view sv, std::vector<Outcome> &out) {
  uint64_t cap = 16, found = 0;
  std::vector<Result> r;
  std::vector<uint64_t> s, e;
  for (int pass = 0; pass < 2; ++pass) {
    r.assign(cap, 0);
    s.assign(cap, 0);
    e.assign(cap, 0);
    throwOnError(redgpu_match_all_long(exec.handle(), 1, reinterpret_cast<const Byte *>(sv.data()),
                                       sv.size(), 0, cap, &found, r.data(), s.data(), e.data()));
    if (found <= cap) break;
    cap = found;
  }
  out.clear();
  for (uint64_t i = 0; i < found; ++i) out.push_back(Outcome{r[i], size_t(s[i]), size_t(e[i])});
  return out.size();
}

// replace(exec, sv, repl, out, max, style): include/Matcher.h:119-124, lib/Matcher.cpp:72-92
// (run-time style, doLeader = true); the templates of Matcher.h:186-211 below it
namespace detail {
inline size_t replaceOne(const Executable &exec, std::string_view sv, std::string_view repl,
                         std::string &out, size_t max, int style, int doLeader) {
  const uint64_t off[2] = {0, sv.size()};
  uint64_t cnt = 0, ooff[2] = {0, 0};
  out.assign(sv.size() + 64, '\0');
  for (int pass = 0; pass < 2; ++pass) {
    throwOnError(redgpu_replace_batch(exec.handle(), style, doLeader,
                                      reinterpret_cast<const Byte *>(sv.data()), off, 0, 1,
                                      reinterpret_cast<const Byte *>(repl.data()), repl.size(), max,
                                      &cnt, ooff, reinterpret_cast<Byte *>(out.data()),
                                      out.size()));
    if (ooff[1] <= out.size()) break;
    out.assign(size_t(ooff[1]), '\0');
  }
  out.resize(size_t(ooff[1]));
  return size_t(cnt);
}
} // namespace detail

inline size_t replace(const Executable &exec, std::string_view sv, std::string_view repl,
                      std::string &out, size_t max, Style style) {
  return detail::replaceOne(exec, sv, repl, out, max, style, 1);
}
template <Style style, bool doLeader>
size_t replace(const Executable &exec, std::string_view sv, std::string_view repl, std::string &out,
               size_t max) {
  return detail::replaceOne(exec, sv, repl, out, max, style, doLeader);
}

// replace(exec, sv, repl, out, max, style) over one long text, chunk-parallel on the device
// (redgpu_replace_long): the run-time-style signature of lib/Matcher.cpp:72-92, doLeader = true.
// Room for about the input's length first, one more call with the exact size otherwise.
inline size_t replaceLong(const Executable &exec, std::string_view sv, std::string_view repl,
                          std::string &out, size_t max, Style style) {
  uint64_t cnt = 0, len = 0;
  out.assign(sv.size() + 64, '\0');
  for (int pass = 0; pass < 2; ++pass) {
    throwOnError(redgpu_replace_long(exec.handle(), style, 1,
                                     reinterpret_cast<const Byte *>(sv.data()), sv.size(), 0,
                                     reinterpret_cast<const Byte *>(repl.data()), repl.size(), max,
                                     &cnt, &len, reinterpret_cast<Byte *>(out.data()), out.size()));
    if (len <= out.size()) break;
    out.assign(size_t(len), '\0');
  }
  out.resize(size_t(len));
  return size_t(cnt);
}

// search(exec, sv, style) over one long text, chunk-parallel on the device (redgpu_search_long):
// the run-time-style signature, doLeader = true; the template as Matcher.h:172-173
inline Outcome searchLong(const Executable &exec, std::string_view sv, Style style) {
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_search_long(exec.handle(), style, 1,
                                  reinterpret_cast<const Byte *>(sv.data()), sv.size(), 0, &r, &s,
                                  &e));
  return Outcome{r, size_t(s), size_t(e)};
}
template <Style style, bool doLeader>
Outcome searchLong(const Executable &exec, std::string_view sv) {
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_search_long(exec.handle(), style, doLeader,
                                  reinterpret_cast<const Byte *>(sv.data()), sv.size(), 0, &r, &s,
                                  &e));
  return Outcome{r, size_t(s), size_t(e)};
}

// StatefulMatcher: include/Matcher.h:770-792.  advance(Byte) as in the reference, plus
// advance(ptr, len) for a whole chunk per launch.  exec must outlive this object.
class StatefulMatcher {
public:
  explicit StatefulMatcher(const Executable &exec) : exec_(exec) { advance(nullptr, 0); }

  Result advance(Byte input) { return advance(&input, 1); }
  Result advance(const Byte *p, size_t len) {
    const uint64_t off[2] = {0, len};
    const Byte dummy = 0;
    throwOnError(redgpu_advance_batch(exec_.handle(), p ? p : &dummy, off, 0, 1, &state_,
                                      &result_));
    return result_;
  }
  Result result() const { return result_; }

private:
  const Executable &exec_;
  uint32_t state_ = REDGPU_STATE_INITIAL;
  Result result_ = 0;
};

// run-time style: doLeader = true, unknown style -> RedExceptExec("unsupported style")
// (lib/Matcher.cpp:37-67)
inline Result check(const Executable &exec, std::string_view sv, Style style) {
  return detail::one(redgpu_check_batch, exec, sv.data(), sv.size(), style, true);
}
inline Result scan(const Executable &exec, std::string_view sv, Style style) {
  return detail::one(redgpu_scan_batch, exec, sv.data(), sv.size(), style, true);
}
inline Outcome match(const Executable &exec, std::string_view sv, Style style) {
  const uint64_t off[2] = {0, sv.size()};
  Result r = 0;
  uint64_t s = 0, e = 0;
  throwOnError(redgpu_match_batch(exec.handle(), style, 1,
                                  reinterpret_cast<const Byte *>(sv.data()), off, 0, 1, &r, &s, &e));
  return Outcome{r, size_t(s), size_t(e)};
}

} // namespace redgpu
