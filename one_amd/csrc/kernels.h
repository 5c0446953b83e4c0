// kernels.h - launch interface between the C-ABI (redgpu.cpp) and the gfx950 kernels.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace redgpu {

enum Verb : int { kCheck = 0, kMatch = 1, kScan = 2, kSearch = 3 };

// Device-resident DFA image (pointers are device addresses). Built once per redgpu_dfa.
struct DevDfa {
  const uint8_t *table;    // packed table, layout per tableKind (REDGPU_TAB_*)
  const int32_t *result;   // [nStates] result code per device state
  const uint8_t *equivLeader; // 256 bytes equivalence map, then 256 bytes class-space leader
  uint8_t *sink;           // 64 writable bytes nobody reads: where lanes with nothing to report
                           // store, so that result stores need no branch (k_stream.h)
  uint32_t tableKind;
  uint32_t tableBytes;
  uint32_t nStates;
  uint32_t nClasses;
  uint32_t init;
  uint32_t leaderNext;
  uint32_t nPureDead;
  uint32_t firstAccept;
  uint32_t leaderLen;
  uint32_t deadAbsorbing;
  // REDGPU_TAB_HOT_ROWS (dfa_image.h), else 0: hot states [hotLo, hotLo + nHot), the 64 KB
  // [hot index][byte] u8 table at table + hot8Off, hot index = s - hotLo + hotShift
  uint32_t hotLo, nHot, hot8Off, hotShift;
  uint32_t clsOff, clsRowBytes, clsBytes;  // streaming form of the class table, or 0
  uint32_t clsIndexForm;         // its entries are state indices (tables above 64 KB), not row offsets
  uint32_t sparseCombOff, sparseDefault;  // REDGPU_TAB_LDS_SPARSE: byte offset of the slots, default target
  uint32_t earlyDeath;           // the visit model sees walks die within 16 bytes
  uint32_t tuned;                // hot rows ranked by observed visits
  uint32_t forgetful;            // the walk is mostly in the initial state (k_chunk.h)
  uint32_t uniformResult;        // every accepting state has the same result (dfa_image.h)
  uint32_t suffixClosed;         // L = SIGMA* L (dfa_image.h): a failed attempt that reached the end
                                 // of the line ends scan / search / collect
  uint32_t gatherNt;             // REDGPU_GATHER_NT=1: non-temporal table gathers (tuning experiment)
  uint32_t leaderForced;         // the leader is the table's own forced prefix chain (dfa_image.h)
  // start bytes for scan / search (dfa_image.h): packed members, count (0xff = no filter)
  uint32_t startLeadWord, startLeadCount, startFreeWord, startFreeCount;
  uint32_t start2LeadWord, start2LeadCount, start2FreeWord, start2FreeCount;
  // full start / follow flag tables behind equivLeader: [512..768) without the leader,
  // [768..1024) with it (DfaImage::startFlags); how many start bytes; whether bit 1 means anything
  uint32_t startTotal[2], startFollow[2];
};

// One batch of lines (device pointers).
struct Batch {
  const uint8_t  *data;
  const uint64_t *offsets; // n+1 entries, or nullptr => fixed stride
  uint64_t stride;         // fixed stride; with offsets: trailing delimiter bytes each line
                           // carries and the verbs must not see (0, or 1 after redgpu_split_lines)
  uint64_t n;
  int32_t  *result;
  uint64_t *start;         // may be nullptr
  uint64_t *end;           // may be nullptr
  uint32_t *state = nullptr; // advance only: per-line StatefulMatcher state, in/out
  const uint32_t *perm = nullptr; // k_ragged only: slot -> line (lines bucketed by length)
  const uint8_t *pad = nullptr;   // k_ragged only: copy of the buffer's last 128 bytes + zeros
  // k_ragged only: the lines much longer than the batch's mean (k_ragged_outliers), walked first
  const uint64_t *outRec = nullptr; // [nOut][2] = the line's offsets[] pair
  const uint32_t *outLn = nullptr;  // [nOut] = its index
  const uint32_t *outCtl = nullptr; // [0] = nOut, [1] = the length from which a line is one
  // ... and the lines of at least 8 x that length, cut into pieces that are walked at once
  // (k_ragged_long.h "pieces"; DFAs that forget their past): records
  // per piece, folded into the lines' Outcomes by k_ragged_pieces_fold; states as global ids
  int32_t *pieceRes = nullptr;      // [nPieces] last accepting state | accepted << 31
  uint64_t *pieceEnd = nullptr;     // [nPieces] end of that accept, from the piece's first walked
                                    // byte | exit state << 32 | entry guess << 48
  uint64_t *pieceStart = nullptr;   // [nPieces] last "left the initial state", likewise
  uint32_t *hugeLn = nullptr;       // [nHuge] the line, [nHuge] its first piece (outCtl[2] = nHuge)
  uint32_t *hugeFirst = nullptr;
  // k_ragged family only (launchBatch answers hipErrorNotSupported for the others): the line
  // count is still on the device - min(*nDev, n) lines, n = what the arrays have room for
  // (redgpu_*_text_dev: the count comes from the line split queued just before)
  const uint64_t *nDev = nullptr;
  uint32_t spread = 1;            // k_generic only: one line per `spread` lanes (table in L2)
  uint32_t ignoreAcceptUpTo = 0;  // k_stream / k_stream_multi, check<..., true> over a forced leader:
                                  // accepts at positions <= this (the post-leader state's own
                                  // result, include/Matcher.h:370-381) are not seen
};

struct LaunchCfg {
  int numCUs;
  int forceGeneric;
  int noBucketing = 0;  // k_ragged: keep lines in input order (REDGPU_F_NO_BUCKETING)
  int forceStream = 0;  // whole-line kernels even for early-death DFAs (REDGPU_F_FORCE_STREAM)
  int noChunking = 0;   // never cut long lines into speculative chunks (REDGPU_F_NO_CHUNKING)
  int forceChunking = 0; // ... or whenever the shape allows, whatever the DFA (REDGPU_F_FORCE_CHUNKING)
  int forceEarly = 0;    // k_early for match over any LDS-resident table, whatever the DFA and
                         // the batch size (REDGPU_F_FORCE_EARLY; tests)
  int forceLean = 0;     // long fixed-stride lines: k_stream_multi's lean step (REDGPU_F_FORCE_LEAN)
  int leanChains4 = 0;   // ... with four lines per lane (REDGPU_F_LEAN_CHAINS_4)
  int streamChains = 0;  // fixed-stride hot path: 0 = by batch size, 2 = k_stream.h always,
                         // 3 / 4 = k_stream4.hip always (REDGPU_F_STREAM_CHAINS_*; tests, tuning)
  int forcePieces = 0;   // k_ragged: huge lines in pieces whatever the DFA (REDGPU_F_FORCE_PIECES)
};

// Launches the kernel for (verb, style, doLeader) on `stream`; returns hipSuccess or the
// launch error. *kernelName receives a static string naming the kernel chosen.
hipError_t launchBatch(const DevDfa &dfa, const Batch &b, int verb, int style, int doLeader,
                       const LaunchCfg &cfg, hipStream_t stream, const char **kernelName);

// The same for nb batches in the order given, as nb calls of launchBatch on `stream` would run
// them - except that runs of batches the streaming kernel takes (fixed stride, whole 64-byte
// blocks, styles Last / Full of check / match) with one stride go out as ONE launch each
// (k_stream_multi.h: table staged once, tiles handed out across batch boundaries).
hipError_t launchBatches(const DevDfa &dfa, const Batch *bs, uint32_t nb, int verb, int style,
                         int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                         const char **kernelName);
hipError_t launchStreamBatches(const DevDfa &dfa, const Batch *bs, uint32_t nb, int verb, int style,
                               int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                               const char **kernelName, uint32_t *taken);

// Red::collect per line (lib/Red.cpp:103-116): up to `cap` records per line at
// [line*cap, line*cap+cap) of result/start/end, counts[line] = number found.
hipError_t launchCollect(const DevDfa &dfa, const Batch &b, uint64_t cap, uint64_t *counts,
                         const LaunchCfg &cfg, hipStream_t stream);

// Red::collect over ONE text of n bytes (k_collect_long.h): *count = matches found, the first
// min(count, cap) records at result/start/end[0..); chunkBytes = 0 chooses the chunk size.
// *kernelName = the route: "k_collect_long", "k_collect_long<closed>" or "k_collect".
hipError_t launchCollectLong(const DevDfa &dfa, const uint8_t *data, uint64_t n, uint32_t chunkBytes,
                             uint64_t cap, uint64_t *count, int32_t *result, uint64_t *start,
                             uint64_t *end, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName);

// matchAll per line (include/Matcher.h:711-766): same record layout as launchCollect.
// *kernelName = the kernel launched: "k_matchall" (one walk per lane, a test per byte) or the
// block-wise "k_matchall_blocks<THREADS,W>" with THREADS = 1024 | 512 and W = 1 | 2.
hipError_t launchMatchAll(const DevDfa &dfa, const Batch &b, uint64_t cap, uint64_t *counts,
                          int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                          const char **kernelName);

// matchAll over ONE text of n bytes (k_match_all_long.h): *count = records found, the first
// min(count, cap) complete at result/start/end[0..); chunkBytes = 0 chooses the chunk size.
// *kernelName = the route: "k_match_all_long" or "k_matchall".  *ctl = the chunked route's 8 control
// words in the stream's scratch (k_match_all_long.h: queued per round, first open chunk, leader
// passed, chunks the serial lane walked, chunks), or nullptr on the one-lane route.
hipError_t launchMatchAllLong(const DevDfa &dfa, int doLeader, const uint8_t *data, uint64_t n,
                              uint32_t chunkBytes, uint64_t cap, uint64_t *count, int32_t *result,
                              uint64_t *start, uint64_t *end, const LaunchCfg &cfg,
                              hipStream_t stream, const char **kernelName, const uint32_t **ctl);

// StatefulMatcher::advance over one chunk per line (include/Matcher.h:770-792):
// state[line] in/out (device state index, >= nStates means "fresh matcher"), b.result out.
hipError_t launchAdvance(const DevDfa &dfa, const Batch &b, uint32_t *state, const LaunchCfg &cfg,
                         hipStream_t stream, const char **kernelName);

// redgpu_dfa_tune's profiling pass: hist[device state] += 1 per byte the anchored walk of
// match<styLast,false> consumes over the sample (hist zeroed by the caller).
hipError_t launchVisits(const DevDfa &dfa, const Batch &b, uint32_t *hist, const LaunchCfg &cfg,
                        hipStream_t stream);

// replaceCore over ONE text of n bytes (k_replace_long.h): *count = replacements made (at most
// max), *outLen = the rewritten text's length, its first min(*outLen, outCap) bytes in out (may
// be null).  phases: 1 = count and size, 2 = write out from what phase 1 left in this stream's
// scratch, 3 = both.  *kernelName = the route: "k_replace_long" or "k_replace_long<one>".
hipError_t launchReplaceLong(const DevDfa &dfa, int style, int doLeader, const uint8_t *data,
                             uint64_t n, uint32_t chunkBytes, const uint8_t *repl, uint64_t replLen,
                             uint64_t max, uint64_t *count, uint64_t *outLen, uint8_t *out,
                             uint64_t outCap, int phases, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName);

// searchCore over ONE text of n bytes (k_search_long.h): *result, *start, *end (the last two may
// be null) = the Outcome of search<style, doLeader>; chunkBytes = 0 chooses the chunk size.
// *kernelName = the route: "k_search_long" or "k_search_long<one>".
hipError_t launchSearchLong(const DevDfa &dfa, int style, int doLeader, const uint8_t *data,
                            uint64_t n, uint32_t chunkBytes, int32_t *result, uint64_t *start,
                            uint64_t *end, const LaunchCfg &cfg, hipStream_t stream,
                            const char **kernelName);

// replaceCore per line (include/Matcher.h:643-706): counts[n], outOffsets[n + 1] (exclusive scan
// of the rewritten lengths, [n] = total) always; with out != nullptr also the rewritten bytes of
// every line that fits below outCap.  repl is device memory.
hipError_t launchReplace(const DevDfa &dfa, const Batch &b, int style, int doLeader,
                         const uint8_t *repl, uint64_t replLen, uint64_t max, uint64_t *counts,
                         uint64_t *outOffsets, uint8_t *out, uint64_t outCap,
                         const LaunchCfg &cfg, hipStream_t stream);

// Line splitting (lib/Util.cpp:109-130's rule): offsets[0] = 0, offsets[k+1] = position after the
// k-th delimiter, for k < cap; *nLines = delimiters found.  counts: uint32[splitChunks(len)],
// bases: uint64[splitChunks(len)], masks: splitMaskBytes(len) bytes (16-byte aligned) - scratch,
// all device memory.
uint64_t splitChunks(uint64_t len);
uint64_t splitMaskBytes(uint64_t len);
hipError_t launchSplitLines(const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *offsets,
                            uint64_t cap, uint64_t *nLines, uint32_t *counts, uint64_t *bases,
                            uint16_t *masks, hipStream_t stream);

// The line index of the raw-text verbs (k_text.h): launchSplitLines' count and scan without the
// scatter (counts, bases, masks as there; *nLines, or spare[0] when nLines is null), then
// open[chunk] = where the line in progress at the chunk's first byte begins (uint64[splitChunks(len)])
// and, unless zeroMasks is null, a second bitmap of masks' size zeroed.  spare: uint64[2].
hipError_t launchTextIndex(const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *nLines,
                           uint32_t *counts, uint64_t *bases, uint16_t *masks, uint64_t *open,
                           uint16_t *zeroMasks, uint64_t *spare, int numCUs, hipStream_t stream);

// grep over a raw text (k_grep.h): the lines of launchSplitLines' rule that search<style, doLeader>
// selects (result > 0, or the others under invert), as records in text order: *nSelected =
// min(selected, maxCount), the first min(*nSelected, cap) records in line / begin / finish /
// result / start / end (each may be null, nLines too).  scratch: grepScratchBytes(len) bytes of
// device memory, 16-byte aligned.  *kernelName = "k_grep_text".
uint64_t grepScratchBytes(uint64_t len);
hipError_t launchGrepText(const DevDfa &dfa, int style, int doLeader, int invert, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t maxCount, uint64_t cap,
                          uint64_t *nLines, uint64_t *nSelected, uint64_t *line, uint64_t *begin,
                          uint64_t *finish, int32_t *result, uint64_t *start, uint64_t *end,
                          void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                          const char **kernelName);

// grep -o over a raw text (k_collect_text.h): Red::collect over every line of launchSplitLines' rule,
// the records in text order: *nMatches = records found, the first min(*nMatches, cap) of them in
// line / begin / result / start / end (each may be null, nLines too; start and end are offsets in
// data).  scratch: collectTextScratchBytes(len) bytes of device memory, 16-byte aligned.
// *kernelName = "k_collect_text".
uint64_t collectTextScratchBytes(uint64_t len);
hipError_t launchCollectText(const DevDfa &dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                             uint64_t cap, uint64_t *nLines, uint64_t *nMatches, uint64_t *line,
                             uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end,
                             void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName);

// grep -c per result over a raw text (k_tally_text.h): one item per line of launchSplitLines' rule
// (what = REDGPU_TALLY_LINES: its value the result of search<style, doLeader> on the line, by
// launchGrepText's normalisation) or per record launchCollectText would report (REDGPU_TALLY_MATCHES:
// its value the record's result), counted in bins[value] for (uint32_t)value < nBins, else in
// bins[nBins]: overwritten, or added to under accumulate.  *nItems = items of value > 0; nLines and
// nItems may be null.  plain != 0: an atomic per item (the form the ballot / peel form is measured
// against).  scratch: tallyTextScratchBytes(len) bytes of device memory, 16-byte aligned.
// *kernelName = "k_tally_text".  tallyLdsBins: the leading bins the kernel keeps in LDS for a DFA of
// this table kind, staged table size (DevDfa::tableBytes) and state count - a host function.
uint64_t tallyTextScratchBytes(uint64_t len);
uint32_t tallyLdsBins(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates);
hipError_t launchTallyText(const DevDfa &dfa, int what, int style, int doLeader, const uint8_t *data,
                           uint64_t len, uint8_t delim, uint64_t nBins, int accumulate, int plain,
                           uint64_t *nLines, uint64_t *nItems, uint64_t *bins, void *scratch,
                           const LaunchCfg &cfg, hipStream_t stream, const char **kernelName);

// per result the count, sum, minimum and maximum of the numbers in a raw text's matches
// (k_sum_text.h): an item is a piece launchExtractText would emit under maxPerLine, its slot the
// result launchCollectText reports for it ((uint32_t)result < nBins, else nBins), its number the
// first (which = REDGPU_SUM_FIRST) or last (REDGPU_SUM_LAST) run of digits inside the piece, read as
// an unsigned decimal; an item without a digit or with a run of 2^64 or more enters no statistic.
// stats[row * (nBins + 1) + slot], rows count, sum (modulo 2^64), min, max: overwritten (an empty
// slot 0, 0, 2^64 - 1, 0), or merged into under accumulate.  *nItems = all items, *nNumeric = those
// in the statistics; nLines, nItems and nNumeric may be null.  plain != 0: four atomics per item (the
// form the carried run and the peel are measured against).  scratch: sumTextScratchBytes(len) bytes
// of device memory, 16-byte aligned.  *kernelName = "k_sum_text".  sumLdsBins: the leading slots the
// kernel keeps in LDS for a DFA of this table kind, staged table size and state count - a host
// function.
uint64_t sumTextScratchBytes(uint64_t len);
uint32_t sumLdsBins(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates);
hipError_t launchSumText(const DevDfa &dfa, int which, const uint8_t *data, uint64_t len,
                         uint8_t delim, uint64_t maxPerLine, uint64_t nBins, int accumulate,
                         int plain, uint64_t *nLines, uint64_t *nItems, uint64_t *nNumeric,
                         uint64_t *stats, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                         const char **kernelName);

// sed over a raw text (k_replace_text.h): replace<style, doLeader>(line, repl, max) over every line
// of launchSplitLines' rule, the rewritten lines and their delimiters put back together (and the
// tail behind them; under onlyChanged the changed lines alone, no tail): *outLen = the output's
// length, *nReplaced = the replacements made, the first min(*outLen, outCap) bytes in out and
// nothing behind them (out, nLines and nReplaced may be null; repl is device memory).  phases: 1 =
// split, count and size, 2 = write out from what phase 1 left in scratch, 3 = both.  scratch:
// replaceTextScratchBytes(len) bytes of device memory, 16-byte aligned.
// *kernelName = "k_replace_text".
uint64_t replaceTextScratchBytes(uint64_t len);
hipError_t launchReplaceText(const DevDfa &dfa, int style, int doLeader, int onlyChanged,
                             const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                             uint64_t replLen, uint64_t max, uint64_t *nLines, uint64_t *nReplaced,
                             uint64_t *outLen, uint8_t *out, uint64_t outCap, int phases,
                             void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName);

// grep's output over a raw text (k_filter_text.h): the lines launchGrepText selects (the first
// maxCount of them), `before` lines in front of and `after` lines behind each, every emitted line
// once and in text order with its delimiter: *nSelected = min(selected, maxCount), *nEmitted = lines
// emitted, *outLen = their bytes, the first min(*outLen, outCap) bytes in out and nothing behind them
// (out, nLines, nSelected and nEmitted may be null).  phases: 1 = index, select, mark and size, 2 =
// write out from what phase 1 left in scratch, 3 = both.  scratch: filterTextScratchBytes(len) bytes
// of device memory, 16-byte aligned.  *kernelName = "k_filter_text".
uint64_t filterTextScratchBytes(uint64_t len);
hipError_t launchFilterText(const DevDfa &dfa, int style, int doLeader, int invert, uint64_t before,
                            uint64_t after, uint64_t maxCount, const uint8_t *data, uint64_t len,
                            uint8_t delim, uint64_t *nLines, uint64_t *nSelected,
                            uint64_t *nEmitted, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                            int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                            const char **kernelName);

// grep -o's output as a text (k_extract_text.h): the first maxPerLine pieces of every line of
// launchSplitLines' rule - a piece is [where the matching attempt began, the match's end), the chain
// launchCollectText's - each followed by delim, in text order: *nMatches = pieces emitted, *outLen =
// their bytes with the delimiters, the first min(*outLen, outCap) bytes in out and nothing behind them
// (out, nLines and nMatches may be null).  hand: pieces from this length on are copied by the whole
// wave (0 = the default).  phases: 1 = index and size, 2 = write out from what phase 1 left in
// scratch, 3 = both.  scratch: extractTextScratchBytes(len) bytes of device memory, 16-byte
// aligned.  *kernelName = "k_extract_text".
uint64_t extractTextScratchBytes(uint64_t len);
hipError_t launchExtractText(const DevDfa &dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                             uint64_t maxPerLine, uint32_t hand, uint64_t *nLines,
                             uint64_t *nMatches, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                             int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName);

// awk -F's columns of a raw text (k_fields_text.h): the separators of a line of launchSplitLines'
// rule are the first maxFields - 1 (maxFields = 0: all) pieces launchExtractText would emit for it,
// its fields what lies between them; an emitted line holds its fields selected by `select` (bit
// k - 1 = field k, bit 63 = field 64 and every later one; not 0) that exist, in order, joined by the
// sepLen (0..8) low bytes of sep, then delim.  onlyDelimited: lines without a separator are not
// emitted.  *nEmitted = output lines, *nFields = fields written, *outLen = the output's bytes, the
// first min(*outLen, outCap) bytes in out and nothing behind them (out, nLines, nEmitted and
// nFields may be null).  phases: 1 = index and size, 2 = write out from what phase 1 left in
// scratch, 3 = both.  scratch: fieldsTextScratchBytes(len) bytes of device memory, 16-byte
// aligned.  *kernelName = "k_fields_text".
uint64_t fieldsTextScratchBytes(uint64_t len);
hipError_t launchFieldsText(const DevDfa &dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t select, uint64_t maxFields, int onlyDelimited, uint64_t sep,
                            uint32_t sepLen, uint64_t *nLines, uint64_t *nEmitted,
                            uint64_t *nFields, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                            int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                            const char **kernelName);

// a raw text's lines grouped by result (k_route_text.h): every line of launchSplitLines' rule goes to
// bucket r (its launchTallyText LINES value, (uint32_t)r < nBins) or nBins; the output is bucket
// 0's lines, then bucket 1's, ..., each in text order with its delimiter - lines of value 0 left
// out under dropUnmatched.  binLines[nBins + 1] = lines per bucket (dropped ones included),
// binOffsets[nBins + 2] = where each bucket's section begins and the total, *outLen = the total,
// *nRouted = lines emitted, the first min(*outLen, outCap) bytes in out and nothing behind them
// (out, nLines, nRouted and binLines may be null).  nBins <= 255.  phases: 1 = index, class, size
// and scan, 2 = write out from what phase 1 left in scratch, 3 = both.  scratch:
// routeTextScratchBytes(len, nBins, dropUnmatched) bytes of device memory, 16-byte aligned.
// *kernelName = "k_route_text".
uint64_t routeTextScratchBytes(uint64_t len, uint64_t nBins, int dropUnmatched);
hipError_t launchRouteText(const DevDfa &dfa, int style, int doLeader, int dropUnmatched,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t nBins,
                           uint64_t *nLines, uint64_t *nRouted, uint64_t *binLines,
                           uint64_t *binOffsets, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                           int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                           const char **kernelName);

// sed's /open/,/close/ line ranges of a raw text (k_range_text.h): over the lines of
// launchSplitLines' rule, in text order, a range begins at a line of value openResult met outside a
// range (its launchTallyText LINES value) and ends with the next line of value closeResult behind
// it, or with the last line; only ranges numbered below maxRanges count.  Emitted are a counted
// range's body lines, its open line under emitOpen and its close line under emitClose - under invert
// exactly the other lines - in text order with their delimiters.  *nRanges = min(ranges,
// maxRanges), *nEmitted = lines emitted, *outLen = the whole output's length, the first
// min(*outLen, outCap) bytes in out and nothing behind them; for every counted range r < recCap
// firstLine[r], lastLine[r] = its line numbers, begin[r], end[r] = its bytes (out, nLines, nRanges,
// nEmitted and the four arrays may be null).  openResult, closeResult >= 1.  phases: 1 = index,
// class, carry, mark (the records too) and scan, 2 = write out from what phase 1 left in scratch,
// 3 = both.  scratch: rangeTextScratchBytes(len) bytes of device memory, 16-byte aligned.
// *kernelName = "k_range_text".
uint64_t rangeTextScratchBytes(uint64_t len);
hipError_t launchRangeText(const DevDfa &dfa, int style, int doLeader, int32_t openResult,
                           int32_t closeResult, int emitOpen, int emitClose, int invert,
                           uint64_t maxRanges, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t *nLines, uint64_t *nRanges, uint64_t *nEmitted,
                           uint64_t *outLen, uint8_t *out, uint64_t outCap, uint64_t recCap,
                           uint64_t *firstLine, uint64_t *lastLine, uint64_t *begin, uint64_t *end,
                           int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                           const char **kernelName);

// a raw text's distinct items counted by their bytes (k_uniq_text.h): an item is a piece
// launchExtractText would emit under maxPerLine (what = REDGPU_UNIQ_MATCHES) or a line
// launchGrepText selects without invert (REDGPU_UNIQ_LINES, its normalisation), without its
// delimiter.  Record j = distinct string j in the order of first appearance: first[j] its earliest
// offset, length[j], count[j] all its occurrences; the first min(*nDistinct, cap) records written
// and nothing behind them (each array may be null).  *nItems = all items, *nDropped = those in no
// record (2^24 bytes or longer, or the table full); tableSlots a power of two.  plain = 1: no LDS
// front.  Every counter may be null.  scratch: uniqTextScratchBytes(len, tableSlots) bytes of
// device memory, 16-byte aligned.  *kernelName = "k_uniq_text".
// uniqLdsSlots: the slots of the LDS front for a DFA of this table (0 = the table leaves no room).
uint64_t uniqTextScratchBytes(uint64_t len, uint64_t tableSlots);
uint32_t uniqLdsSlots(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates);
hipError_t launchUniqText(const DevDfa &dfa, int what, int style, int doLeader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t maxPerLine, uint64_t tableSlots,
                          uint64_t cap, int plain, uint64_t *nLines, uint64_t *nItems,
                          uint64_t *nDistinct, uint64_t *nDropped, uint64_t *first,
                          uint64_t *length, uint64_t *count, void *scratch, const LaunchCfg &cfg,
                          hipStream_t stream, const char **kernelName);

// a raw text's lines chosen by their keys' strings (k_dedup_text.h): a line's key is the line
// (what = REDGPU_DEDUP_WHOLE), the line when launchGrepText selects it (LINES, its normalisation),
// piece keyIndex launchExtractText would emit for it (MATCH) or field keyIndex launchFieldsText
// cuts it into (FIELD); a line without one is unkeyed.  A keyed line is marked iff it holds the
// earliest occurrence of its key's string and the string's count lies in [minCount, maxCount];
// emitted are the keyed lines with marked != invert, and the unkeyed ones under keepUnkeyed, in
// text order with their delimiters.  *nKeyed = keyed lines, *nDistinct = strings with a record,
// *nDropped = keyed lines whose key got none (2^24 bytes or longer, or the table full),
// *nEmitted = lines emitted, *outLen = the whole output's length, the first min(*outLen, outCap)
// bytes in out and nothing behind them (out and every counter but outLen may be null).  tableSlots
// a power of two; keyIndex >= 1.  plain = 1: no LDS front.  phases: 1 = index, walk, mark, emit and
// scan, 2 = write out from what phase 1 left in scratch, 3 = both.  scratch:
// dedupTextScratchBytes(len, tableSlots) bytes of device memory, 16-byte aligned.
// *kernelName = "k_dedup_text".
uint64_t dedupTextScratchBytes(uint64_t len, uint64_t tableSlots);
hipError_t launchDedupText(const DevDfa &dfa, int what, int style, int doLeader, uint64_t keyIndex,
                           uint64_t minCount, uint64_t maxCount, int invert, int keepUnkeyed,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t tableSlots,
                           int plain, uint64_t *nLines, uint64_t *nKeyed, uint64_t *nDistinct,
                           uint64_t *nDropped, uint64_t *nEmitted, uint64_t *outLen, uint8_t *out,
                           uint64_t outCap, int phases, void *scratch, const LaunchCfg &cfg,
                           hipStream_t stream, const char **kernelName);

// a raw text's lines grouped by their keys' strings, with the numbers of a second item of the line
// (k_group_text.h): an item is a piece launchExtractText would emit for the line (what =
// REDGPU_GROUP_MATCH) or a field launchFieldsText cuts it into (FIELD); item keyIndex (>= 1) is the
// key - a line without one is unkeyed - and item valueIndex (0 = none) the value, whose number is
// launchSumText's under `which`.  Record j = distinct key string j in the order of first
// appearance: first[j], length[j], count[j] = its keyed lines, stats[row * cap + j] = count, sum
// (modulo 2^64), min, max of its numeric lines (0, 0, ~0, 0 without any); the first
// min(*nDistinct, cap) records written and nothing behind them (each array may be null).
// *nKeyed = keyed lines, *nNumeric = numeric lines whose key holds a record, *nDropped = keyed lines
// in no record (a key of 2^24 bytes or more, or the table full); every counter may be null.
// tableSlots a power of two.  plain = 1: no LDS front.  scratch: groupTextScratchBytes(len,
// tableSlots) bytes of device memory, 16-byte aligned.  *kernelName = "k_group_text".
// groupLdsSlots: the slots of the LDS front for a DFA of this table (0 = the table leaves no room).
uint64_t groupTextScratchBytes(uint64_t len, uint64_t tableSlots);
uint32_t groupLdsSlots(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates);
hipError_t launchGroupText(const DevDfa &dfa, int what, uint64_t keyIndex, uint64_t valueIndex,
                           int which, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t tableSlots, uint64_t cap, int plain, uint64_t *nLines,
                           uint64_t *nKeyed, uint64_t *nNumeric, uint64_t *nDistinct,
                           uint64_t *nDropped, uint64_t *first, uint64_t *length, uint64_t *count,
                           uint64_t *stats, void *scratch, const LaunchCfg &cfg,
                           hipStream_t stream, const char **kernelName);

// bench.py's read-bandwidth calibration: one streaming pass over `bytes` (16-byte aligned).
hipError_t launchDiagRead(const void *data, uint64_t bytes, uint32_t *sink, int numCUs,
                          hipStream_t stream);

// bench.py's read + write calibration: the streaming walk's memory side alone over nLines lines of
// 64 bytes - each lane requests its line as k_stream does and stores one Outcome-shaped record
// (int32 + 2 x uint64) per line; nLines is rounded down to a multiple of 1024.
// lineBytes = 64, or a multiple of 128: the long-line request pattern, reads only.
hipError_t launchDiagLines(const uint8_t *data, uint64_t nLines, uint32_t lineBytes, int32_t *res,
                           uint64_t *st, uint64_t *en, uint32_t *sink, int numCUs,
                           hipStream_t stream);

// bench.py's L2 gather calibration: `rounds` dependent 2-byte gathers per chain from a table of
// 2^20 uint16 (2 MiB, device memory, any contents), 2 chains per lane, 2048 lanes per CU, no input
// side; *lookups = gathers the launch performs.
hipError_t launchDiagL2(const uint16_t *table, uint32_t rounds, uint32_t *sink, int numCUs,
                        hipStream_t stream, uint64_t *lookups);

// k_stream4.hip: the fixed-stride hot path with 3-4 chains per lane (mode = k_stream.h's
// StreamMode value: Last+start+end 0, Last+end 1, Full+start 3, Full 4).
bool stream4Eligible(const DevDfa &dfa, const Batch &b, const LaunchCfg &cfg);
hipError_t launchStream4(int mode, const DevDfa &dfa, const Batch &b, const LaunchCfg &cfg,
                         hipStream_t stream);

// Device scratch for the launches that need some (host_stage.cpp): a pool per HOST THREAD keyed
// by (current device, stream) - the buffer carries state between the kernels of one call, so no
// other thread may be handed it - bounded, freed at thread exit / redgpu_thread_release(),
// entries of a library-owned stream dropped with the stream.  scratchEntries: all threads'.
hipError_t scratchFor(hipStream_t stream, size_t bytes, void **out);
// The same entry's CONTROL words: two slots of 8 x uint32 that only k_ragged's launch sequence
// touches (the scratch buffer itself is shared with every other launch family of the thread and
// stream).  *out = the slot of this call, zero on arrival; *next = the other one, which the
// call's first kernel zeroes for the call after it - so no launch sequence starts with a memset.
hipError_t scratchCtlFor(hipStream_t stream, uint32_t **out, uint32_t **next);
void scratchDrop(int device, hipStream_t stream);
void scratchReleaseThread();
size_t scratchEntries();

// bench.py's calibrations.  launchDiagLds: `rounds` x 64 dependent table lookups per chain, 4
// chains per lane, 512 lanes per CU, bytes from registers (no input traffic): the LDS gather
// roof of the one-lookup-per-byte walk; *lookups receives the number issued.
// launchWalked: *walked (device u64, zeroed by the caller) += the bytes match<styLast,lead>'s loop
// (include/Matcher.h:443-479) consumes per line - what an early-exit walk actually reads.
hipError_t launchDiagLds(const DevDfa &dfa, uint32_t rounds, uint32_t *sink, int numCUs,
                         hipStream_t stream, uint64_t *lookups);
hipError_t launchWalked(const DevDfa &dfa, const Batch &b, int doLeader, unsigned long long *walked,
                        const LaunchCfg &cfg, hipStream_t stream);

// launchBatch's / launchAdvance's kernel families, one translation unit each (kernels.hip is
// compiled per family, -DREDGPU_TU): *handled = false when the batch is not the family's.
hipError_t launchFixedFamily(const DevDfa &dfa, const Batch &b, int verb, int style, int doLeader,
                             const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                             bool *handled);
hipError_t launchRaggedFamily(const DevDfa &dfa, const Batch &b, int verb, int style, int doLeader,
                              const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                              bool *handled);
hipError_t launchAdvanceStream(const DevDfa &dfa, const Batch &b, uint32_t *state,
                               const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                               bool *handled);

// True when the specialised fixed-stride kernels can run this DFA at all.
bool fastPathEligible(const DevDfa &dfa);

} // namespace redgpu
