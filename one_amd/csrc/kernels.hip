// kernels.hip - hand-written gfx950 (CDNA4 / MI355X) kernels for RED's DFA match execution.
//
// What is restated here, one input line per lane (citations relative to
// /root/reference/quol/red/):
//   checkCore  include/Matcher.h:363-410      matchCore  include/Matcher.h:413-495
//   scanCore   include/Matcher.h:498-554      lookingAt / compareThrough  :333-360
//   the per-byte step DfaProxy::next/result/pureDeadEnd   include/Proxy.h:131-147
// over the renumbered device image of dfa_image.h (s < nPureDead <=> pureDeadEnd,
// s >= firstAccept <=> result > 0, so the per-byte predicates are integer compares).
//
// Map of the kernel families, one header each, all included below inside the namespace
// (DESIGN.md section 4 has the measurements):
//   k_common.h        table accessors, table staging (and the geometry of a pass that stages), the
//                     scratch cursor, lane context, the byte readers
//   k_lanes.h         the lane functions: direct restatements of the reference's cores
//   k_generic.h       k_generic<KIND, THREADS, VERB>: any verb / style / table, one line per lane
//   k_early.h         k_early: match / check over early-death DFAs (probe, park, drain)
//   k_scan_marked.h   k_scan_marked: scan / search in two passes (mark candidates, visit them)
//   k_fixed.h         k_fixed: strides that are not whole blocks, early exits on small batches
//   k_stream.h        k_stream<MODE, HALVES, THREADS, TABK>: the hot path - fixed-stride lines of
//                     whole 64-byte blocks, styles Last / Full, inline-asm byte step over a fused u8
//                     table, a big DFA's hot rows (sink + re-walk) or a class table in LDS
//   k_stream_lean.h   the same step with its bookkeeping deferred (opt-in, long lines)
//   k_stream_multi.h  k_stream_multi: several batches in one launch (redgpu_*_batches_dev)
//   k_ragged.h        k_ragged<MODE, TABK>: the walk over ragged lines, lanes refilled from a
//                     workgroup cursor; the tail pad; k_generic's bucketing pre-pass
//   k_ragged_long.h   k_ragged_outliers (the long lines of a batch: listed, walked first, huge ones as
//                     pieces), k_ragged_pieces_fold (the pieces' records -> their lines' Outcomes)
//   k_lists.h         k_collect, k_matchall, k_matchall_blocks (record lists per line)
//   k_long.h          what the long-text verbs share: the anchored attempt (longChain), the 1024-wide
//                     scan kernels (sum and prefix max), a chunk's span, the launch plan
//   k_replace_long.h  k_rl_*: replaceCore over ONE long text: k_collect_long.h's chain under any
//                     style, then the assembly (sums, scans, a tile-driven copy/insert)
//   k_collect_long.h  k_cl_*: Red::collect over ONE long text, chunk-parallel (guessed entries,
//                     re-walk rounds, serial finish, scan + scatter)
//   k_match_all_long.h  k_ml_*: matchAllCore over ONE long text: chunks from guessed entry STATES,
//                     re-walk rounds, serial finish, (sum, max) scan, records emitted in place
//   k_search_long.h   k_sl_*: searchCore over ONE long text: every chunk tries its own positions in
//                     order, the lowest success wins (atomic min), windows in text order and an
//                     early exit, bounded attempts and a serial finish
//   k_style_blocks.h  k_style_blocks: early-exit styles and odd strides over the block walk
//   k_misc.h          k_advance, k_replace (+ the 64-bit scan, launchScan64), k_visits, k_walked
//   k_split.h         line splitting on the device
//   k_text.h          what the raw-text verbs share: the bitmap views, the line index (k_gp_last,
//                     k_gp_open), the line walk, the hit-line lookup, launch geometry
//   k_grep.h          k_gp_*: grep over a raw text - the split's delimiter bitmap drives the lines,
//                     a wave per 16 KiB chunk selects, a scan orders, a second pass writes records
//   k_collect_text.h  k_ct_*: grep -o over a raw text - k_grep.h's line driver, Red::collect per line,
//                     a count pass, a scan, and a write pass that puts record j at slot j
//   k_tally_text.h    k_tally_text: grep -c per result over a raw text - the same line driver, ONE pass,
//                     the counts in a privatised LDS histogram flushed once per workgroup
//   k_replace_text.h  k_rt_*: sed over a raw text - the same line driver, replaceCore per line, a
//                     sizing pass, a scan, and a write pass whose waves copy the unchanged bytes
//   k_filter_text.h   k_ft_*: grep's output with -A / -B context over a raw text - k_grep.h's select pass,
//                     the context as arithmetic on line numbers over the two bitmaps, a scan, and a
//                     write pass that only copies runs of emitted lines
//   k_extract_text.h  k_xt_*: grep -o's output as a text - k_collect_text.h's chain per line, a sizing
//                     pass, a scan, and a write pass whose lanes assemble their pieces in a 16-byte
//                     register window
//   k_route_text.h    k_ro_*: a raw text's lines grouped by result - k_grep.h's walk leaves each line's
//                     bucket in bit-planes, a sizing pass per (bucket, chunk), ONE scan, and
//                     k_filter_text.h's run copy once per bucket present in a chunk
//   k_range_text.h    k_rg_*: sed's /open/,/close/ line ranges of a raw text - k_route_text.h's walk leaves
//                     "is open" / "is close" in two bit-planes, a two-state machine is carried across
//                     the chunks by k_gp_open's or k_split_scan's scan, and k_filter_text.h's run copy
//   k_uniq_text.h     k_uq_*: a raw text's distinct matches (or selected lines) counted by their BYTES -
//                     k_tally_text.h's walk, a hash table keyed by the text's own bytes behind an LDS
//                     front, and an ordering pass over a first-occurrence bitmap
//   k_fields_text.h   k_fd_*: awk -F's columns of a raw text - k_extract_text.h's chain per line with the
//                     GAPS between the matches as the fields, left behind the last field asked for;
//                     a sizing pass, a scan, and a write pass through k_extract_text.h's window
//   k_sum_text.h      k_sum_text: per result the count, sum, min and max of the numbers in a raw text's
//                     matches - k_tally_text.h's walk, the digits read once a piece's span is known,
//                     four 64-bit words per slot behind an LDS front
//   k_dedup_text.h    k_dd_*: awk '!seen[$k]++' over a raw text - k_uniq_text.h's walk and table with one key
//                     per line, a pass that turns table slots into line bits, the EMIT bitmap from
//                     three bitmaps, and k_filter_text.h's run copy
//   k_group_text.h    k_gr_*: awk '{ s[$k] += $v }' over a raw text - k_dedup_text.h's walk with a key and a
//                     value per line, k_uniq_text.h's table and front with four 64-bit statistics beside
//                     each slot, and its ordering pass
//   k_diag.h         bench.py's calibration kernels
//   launchers.h       grid / LDS / instantiation per family; includes k_chunk.h (speculative
//                     chunking of few long lines)
//   here              the dispatch: launchBatch / launchBatches and friends - which kernel runs what.
// No MFMA anywhere: this is a gather workload bounded by the LDS gather rate and HBM streaming.
#include "kernels.h"

#include <cstdlib>
#include <type_traits>

#include "../../include/redgpu.h"

// This file is compiled fifteen times in parallel (Makefile: -DREDGPU_TU=1/2/.../15): the templates are
// instantiated where their launchers are CALLED, so each translation unit only pays for one
// family of kernels - 1 = the fixed-stride family (k_stream, k_chunk, k_fixed), 2 = k_ragged,
// 3 = everything else and the dispatch, 4 = k_grep and k_filter_text (which runs k_grep's select), 5 = k_collect_text, 6 = k_replace_text,
// 7 = k_tally_text, 8 = k_extract_text, 9 = k_route_text, 10 = k_uniq_text,
// 11 = k_fields_text, 12 = k_sum_text, 13 = k_range_text, 14 = k_dedup_text,
// 15 = k_group_text.
// REDGPU_TU undefined or 0 = all of it in one unit.
#ifndef REDGPU_TU
#define REDGPU_TU 0
#endif
#define REDGPU_TU_STREAM (REDGPU_TU == 0 || REDGPU_TU == 1)
#define REDGPU_TU_RAGGED (REDGPU_TU == 0 || REDGPU_TU == 2)
#define REDGPU_TU_GENERIC (REDGPU_TU == 0 || REDGPU_TU == 3)
#define REDGPU_TU_GREP (REDGPU_TU == 0 || REDGPU_TU == 4)
#define REDGPU_TU_COLLECT_TEXT (REDGPU_TU == 0 || REDGPU_TU == 5)
#define REDGPU_TU_REPLACE_TEXT (REDGPU_TU == 0 || REDGPU_TU == 6)
#define REDGPU_TU_TALLY_TEXT (REDGPU_TU == 0 || REDGPU_TU == 7)
#define REDGPU_TU_EXTRACT_TEXT (REDGPU_TU == 0 || REDGPU_TU == 8)
#define REDGPU_TU_ROUTE_TEXT (REDGPU_TU == 0 || REDGPU_TU == 9)
#define REDGPU_TU_UNIQ_TEXT (REDGPU_TU == 0 || REDGPU_TU == 10)
#define REDGPU_TU_FIELDS_TEXT (REDGPU_TU == 0 || REDGPU_TU == 11)
#define REDGPU_TU_SUM_TEXT (REDGPU_TU == 0 || REDGPU_TU == 12)
#define REDGPU_TU_RANGE_TEXT (REDGPU_TU == 0 || REDGPU_TU == 13)
#define REDGPU_TU_DEDUP_TEXT (REDGPU_TU == 0 || REDGPU_TU == 14)
#define REDGPU_TU_GROUP_TEXT (REDGPU_TU == 0 || REDGPU_TU == 15)

// return CALL(KIND) for the table kind of the DevDfa `d` in scope: a launcher's instantiation per kind
#define REDGPU_KIND_SWITCH(CALL)                                                          \
  switch (d.tableKind) {                                                                  \
  case REDGPU_TAB_LDS_FUSED_U8: return CALL(REDGPU_TAB_LDS_FUSED_U8);                     \
  case REDGPU_TAB_LDS_FUSED_U16: return CALL(REDGPU_TAB_LDS_FUSED_U16);                   \
  case REDGPU_TAB_LDS_CLASS_U16: return CALL(REDGPU_TAB_LDS_CLASS_U16);                   \
  case REDGPU_TAB_GLOBAL_U16: return CALL(REDGPU_TAB_GLOBAL_U16);                         \
  case REDGPU_TAB_HOT_ROWS: return CALL(REDGPU_TAB_HOT_ROWS);                               \
  case REDGPU_TAB_LDS_SPARSE: return CALL(REDGPU_TAB_LDS_SPARSE);                         \
  default: return CALL(REDGPU_TAB_GLOBAL_U32);                                            \
  }

namespace redgpu {

namespace {

#include "k_common.h"
#include "k_lanes.h"
#include "k_generic.h"
#include "k_early.h"
#include "k_scan_marked.h"
#include "k_fixed.h"
#include "k_stream.h"
#include "k_stream_lean.h"
#include "k_stream_multi.h"
#include "k_ragged.h"
#include "k_lists.h"
#include "k_long.h"
#include "k_collect_long.h"
#include "k_replace_long.h"
#include "k_search_long.h"
#include "k_match_all_long.h"
#include "k_style_blocks.h"
#include "k_misc.h"
#include "k_split.h"
#include "k_diag.h"
#include "launchers.h"
#include "k_text.h"
#include "k_grep.h"
#include "k_collect_text.h"
#include "k_tally_text.h"
#include "k_replace_text.h"
#include "k_filter_text.h"
#include "k_extract_text.h"
#include "k_route_text.h"
#include "k_uniq_text.h"
#include "k_fields_text.h"
#include "k_sum_text.h"
#include "k_range_text.h"
#include "k_dedup_text.h"
#include "k_group_text.h"

} // namespace

// REDGPU_TAB_HOT_ROWS DFAs whose hot set the streaming kernel can index with one byte
[[maybe_unused]] static bool hotStreamEligible(const DevDfa &d) {
  return d.tableKind == REDGPU_TAB_HOT_ROWS && d.nHot > 0 && d.hot8Off != 0 &&
         d.deadAbsorbing;
}

// DFAs of more than 256 states with a class table of at most 64 KB: k_stream's class-table form
[[maybe_unused]] static bool clsStreamEligible(const DevDfa &d) {
  return d.clsOff != 0 && d.deadAbsorbing &&
         d.clsBytes <= (d.clsIndexForm ? kStreamBigLds : kStreamTabBytes + 1024);
}

// lines that are whole blocks of `unit` bytes at a fixed stride below 2 GiB, from a 16-byte
// aligned base: what k_stream (unit 64) and k_fixed (unit 16) load
[[maybe_unused]] static bool wholeBlocks(const Batch &b, uint64_t unit) {
  return !b.offsets && b.stride >= unit && b.stride % unit == 0 && b.stride < (1ull << 31) &&
         (reinterpret_cast<uintptr_t>(b.data) % 16) == 0;
}

[[maybe_unused]] static bool lastOrFull(int style) { return style == kStyLast || style == kStyFull; }

// check / match under styLast / styFull: the whole-line walks of k_stream and k_ragged
[[maybe_unused]] static bool wholeLineWalk(int verb, int style) {
  return (verb == kCheck || verb == kMatch) && lastOrFull(style);
}

// the StreamMode of such a walk
[[maybe_unused]] static int streamMode(int style, bool wantStart) {
  return style == kStyLast ? (wantStart ? kSmLastStartEnd : kSmLastEnd)
                           : (wantStart ? kSmFullStart : kSmFull);
}

// the batch as check's kernels see it: no positions to store
[[maybe_unused]] static Batch withoutPositions(const Batch &b, int verb) {
  Batch sb = b;
  if (verb == kCheck) { sb.start = nullptr; sb.end = nullptr; }
  return sb;
}

// return CALL(MODE) for the StreamMode `mode` in scope (kSmAdvance and kSmChunk have call sites of
// their own)
#define REDGPU_MODE_SWITCH(CALL)                                                          \
  switch (mode) {                                                                         \
  case kSmLastStartEnd: return CALL(kSmLastStartEnd);                                     \
  case kSmLastEnd: return CALL(kSmLastEnd);                                               \
  case kSmFullStart: return CALL(kSmFullStart);                                           \
  default: return CALL(kSmFull);                                                          \
  }

// The kernel names, by StreamMode (2 is no mode) and by table form: kTabFused, kTabHot, kTabCls -
// kTabClsBig runs under kTabCls's name (nameForm).
[[maybe_unused]] static int nameForm(int tabk) { return tabk == kTabClsBig ? kTabCls : tabk; }

#if REDGPU_TU_GENERIC
bool fastPathEligible(const DevDfa &d) {
  return d.tableKind == REDGPU_TAB_LDS_FUSED_U8 && d.deadAbsorbing &&
         size_t(d.tableBytes) + size_t(d.nStates) * 4 <= 150 * 1024;
}
#endif

#if REDGPU_TU_STREAM
static const char *const kStreamNames[5][3] = {
    {"k_stream<last,start,end>", "k_stream<last,start,end,hot>", "k_stream<last,start,end,cls>"},
    {"k_stream<last,end>", "k_stream<last,end,hot>", "k_stream<last,end,cls>"},
    {},
    {"k_stream<full,start>", "k_stream<full,start,hot>", "k_stream<full,start,cls>"},
    {"k_stream<full>", "k_stream<full,hot>", "k_stream<full,cls>"}};
static const char *const kStream4Names[5] = {"k_stream4<last,start,end>", "k_stream4<last,end>",
                                             nullptr, "k_stream4<full,start>", "k_stream4<full>"};
// ([mode][lean]; kSmFull has no lean step, launchStreamMultiT)
static const char *const kStreamMultiNames[5][2] = {
    {"k_stream_multi<last,start,end>", "k_stream_multi<last,start,end,lean>"},
    {"k_stream_multi<last,end>", "k_stream_multi<last,end,lean>"},
    {},
    {"k_stream_multi<full,start>", "k_stream_multi<full,start,lean>"},
    {"k_stream_multi<full>", "k_stream_multi<full>"}};

// k_stream<mode> over the table form tabk
static hipError_t launchStreamMode(int mode, int tabk, const DevDfa &d, const Batch &b,
                                   const LaunchCfg &cfg, hipStream_t stream) {
#define SM_FUSED(M) launchStreamT<M>(d, b, cfg, stream)
#define SM_HOT(M) launchStreamHot<M, kTabHot>(d, b, cfg, stream)
#define SM_CLS(M) launchStreamHot<M, kTabCls>(d, b, cfg, stream)
#define SM_CLS_BIG(M) launchStreamHot<M, kTabClsBig>(d, b, cfg, stream)
  switch (tabk) {
  case kTabFused: REDGPU_MODE_SWITCH(SM_FUSED)
  case kTabHot: REDGPU_MODE_SWITCH(SM_HOT)
  case kTabCls: REDGPU_MODE_SWITCH(SM_CLS)
  default: REDGPU_MODE_SWITCH(SM_CLS_BIG)
  }
#undef SM_CLS_BIG
#undef SM_CLS
#undef SM_HOT
#undef SM_FUSED
}

// StatefulMatcher chunks the streaming kernels can take (k_stream<advance...>); *handled says so
hipError_t launchAdvanceStream(const DevDfa &d, const Batch &b, uint32_t *state,
                               const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                               bool *handled) {
  *handled = false;
  // chunks that are whole 64-byte blocks at a fixed stride: the streaming kernel
  if (cfg.forceGeneric || !wholeBlocks(b, 64)) return hipSuccess;
  const bool fused = fastPathEligible(d) && d.tableBytes <= kStreamTabBytes && d.nStates <= 256;
  const bool cls = !fused && clsStreamEligible(d);
  if (!fused && !cls && !hotStreamEligible(d)) return hipSuccess;
  Batch sb = b;
  sb.state = state;
  sb.start = nullptr;
  sb.end = nullptr;
  *handled = true;
  if (fused) {
    *kernelName = "k_stream<advance>";
    return launchStreamT<kSmAdvance>(d, sb, cfg, stream);
  }
  if (cls) {
    *kernelName = "k_stream<advance,cls>";
    return d.clsIndexForm ? launchStreamHot<kSmAdvance, kTabClsBig>(d, sb, cfg, stream)
                          : launchStreamHot<kSmAdvance, kTabCls>(d, sb, cfg, stream);
  }
  *kernelName = "k_stream<advance,hot>";
  return launchStreamHot<kSmAdvance>(d, sb, cfg, stream);
}

// The fixed-stride family of launchBatch: speculative chunks, k_stream (fused / hot / class
// table), k_fixed.  *handled = false: not this family's batch.
hipError_t launchStreamBatches(const DevDfa &d, const Batch *bs, uint32_t nb, int verb, int style,
                               int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                               const char **kernelName, uint32_t *taken);
hipError_t launchFixedFamily(const DevDfa &d, const Batch &b, int verb, int style, int doLeader,
                             const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                             bool *handled) {
  *handled = true;
  const bool lead = doLeader && d.leaderLen > 0;
  const bool dying = d.earlyDeath && !cfg.forceStream;
  const bool leadCheck = lead && verb == kCheck;
  // Fixed-stride hot path: check / match, whole 16-byte multiples, 16-byte aligned base.
  // check<.., true> consumes the leader and starts in the post-leader state at byte
  // leaderLen (Matcher.h:370-375); match only peeks it (Matcher.h:424-435).
  const bool fixedOk = !cfg.forceGeneric && !dying && fastPathEligible(d) &&
                       (verb == kCheck || verb == kMatch) && wholeBlocks(b, 16) && !leadCheck;
  // ... and check<styLast / styFull, true> when the leader is the table's own forced chain
  // (dfa_image.h: leaderForced): the plain walk from the initial state, deaf to whatever accepts
  // up to the leader's end (a line that IS the leader would report the post-leader state's
  // result: left to k_generic).  (wholeBlocks' stride >= 64 says nothing new here: a multiple of
  // 64 above leaderLen > 0.)
  const bool leadCheckOk = leadCheck && d.leaderForced && b.stride > d.leaderLen &&
                           lastOrFull(style) && !cfg.forceGeneric && !dying &&
                           fastPathEligible(d) && wholeBlocks(b, 64);
  // Streaming kernel: styles Last / Full on lines that are whole 64-byte blocks.
  const bool streamOk = (fixedOk || leadCheckOk) && lastOrFull(style) && b.stride % 64 == 0 &&
                        d.tableBytes <= kStreamTabBytes && d.nStates <= 256;
  // The same streaming walk for DFAs too big for LDS: hot rows as a one-byte-indexed table,
  // cold excursions re-walked per 64-byte half-block (k_stream.h, HOT).
  const bool hotStreamOk = !cfg.forceGeneric && !dying && hotStreamEligible(d) &&
                           wholeLineWalk(verb, style) && wholeBlocks(b, 64) && !leadCheck;
  // ... and for mid-size DFAs whose class table fits 64 KB of LDS (two lookups per byte)
  const bool clsStreamOk = !cfg.forceGeneric && !dying && clsStreamEligible(d) &&
                           wholeLineWalk(verb, style) && wholeBlocks(b, 64) && !leadCheck;
  // Few long lines over a DFA that forgets its past: chunks of every line walked at once from
  // the initial state as a guess, wrong guesses re-walked (k_chunk.h)
  // (leadCheck is only ever true here with leadCheckOk)
  if ((streamOk || hotStreamOk || clsStreamOk) && !cfg.noChunking && !leadCheck &&
      (d.forgetful || cfg.forceChunking) &&
      (fewLines(b, cfg) || cfg.forceChunking)) {
    const uint32_t m = chunksPerLine(b, cfg);
    if (m) {
      *kernelName = d.tableKind == REDGPU_TAB_HOT_ROWS ? "k_stream<chunk,hot>+k_chunk"
                    : d.tableKind == REDGPU_TAB_LDS_FUSED_U8 ? "k_stream<chunk>+k_chunk"
                                                             : "k_stream<chunk,cls>+k_chunk";
      hipError_t e = launchChunked(d, withoutPositions(b, verb), m, style, cfg, stream);
      if (e != hipSuccess) return e;
      return lead ? launchLeaderFilter(d, b, cfg, stream) : hipSuccess;
    }
  }
  // k_stream over the fused table, else the hot rows, else the class table
  if (streamOk || hotStreamOk || clsStreamOk) {
    const int tabk = streamOk      ? kTabFused
                     : hotStreamOk ? kTabHot
                                   : (d.clsIndexForm ? kTabClsBig : kTabCls);
    Batch sb = withoutPositions(b, verb);
    const int mode = streamMode(style, sb.start != nullptr);
    hipError_t e;
    if (streamOk) {
      if (leadCheck) sb.ignoreAcceptUpTo = d.leaderLen;
      static const int labLean = multiLabInt("REDGPU_LEAN", 0, 1, 0);
      static const int labSingle = multiLabInt("REDGPU_MULTI_SINGLE", 0, 1, 0);
      if (cfg.forceLean || labLean || labSingle) {
        // opt-in: k_stream_multi (its deferred-bookkeeping form for long lines) for a batch on its own
        uint32_t taken = 0;
        e = launchStreamBatches(d, &b, 1, verb, style, doLeader, cfg, stream, kernelName, &taken);
        if (e != hipSuccess || taken) return e;
      }
    }
    if (streamOk && !leadCheck && stream4Eligible(d, sb, cfg)) {
      *kernelName = kStream4Names[mode];
      e = launchStream4(mode, d, sb, cfg, stream);
    } else {
      *kernelName = kStreamNames[mode][nameForm(tabk)];
      e = launchStreamMode(mode, tabk, d, sb, cfg, stream);
    }
    if (e != hipSuccess) return e;
    // (check with the leader ran as the walk itself: nothing to filter)
    return lead && !leadCheck ? launchLeaderFilter(d, b, cfg, stream) : hipSuccess;
  }
  if (fixedOk) {
    hipError_t e;
    if (verb == kCheck) {
      *kernelName = "k_fixed<check>";
      e = launchFixedS<false, false>(style, d, b, 0, d.init, cfg, stream);
    } else if (b.start) {
      *kernelName = "k_fixed<match,start>";
      e = launchFixedS<true, true>(style, d, b, 0, d.init, cfg, stream);
    } else {
      *kernelName = "k_fixed<match>";
      e = launchFixedS<true, false>(style, d, b, 0, d.init, cfg, stream);
    }
    if (e != hipSuccess) return e;
    return lead ? launchLeaderFilter(d, b, cfg, stream) : hipSuccess;
  }

  *handled = false;
  return hipSuccess;
}

// Several batches, one launch (k_stream_multi.h).  *taken = how many of bs[0..nb) the launch
// covers: the longest run of leading batches that launchFixedFamily would each give to
// k_stream's plain form, with one stride and the same outputs asked for; 0 = bs[0] is not
// such a batch, or the run is a single batch (the caller then runs it on its own).
hipError_t launchStreamBatches(const DevDfa &d, const Batch *bs, uint32_t nb, int verb, int style,
                               int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                               const char **kernelName, uint32_t *taken) {
  *taken = 0;
  const bool lead = doLeader && d.leaderLen > 0;
  const bool dying = d.earlyDeath && !cfg.forceStream;
  if (cfg.forceGeneric || cfg.forceEarly || cfg.forceChunking || dying || !fastPathEligible(d) ||
      !wholeLineWalk(verb, style) || (lead && verb == kCheck) ||
      d.tableBytes > kStreamTabBytes || d.nStates > 256)
    return hipSuccess;
  auto plain = [&](const Batch &b) {
    // (few long lines over a forgetful DFA are launchFixedFamily's speculative chunks)
    const bool chunky = fewLines(b, cfg) && d.forgetful && !cfg.noChunking && b.stride >= 4096 &&
                        !cfg.forceLean;
    return wholeBlocks(b, 64) && b.n > 0 && !chunky && b.n < (1ull << 40) &&
           !stream4Eligible(d, b, cfg);
  };
  const bool wantStart = verb == kMatch && bs[0].start;
  MultiIo m;
  m.nb = 0;
  m.lineLen = uint32_t(bs[0].stride);
  m.ignoreAcceptUpTo = 0;
  m.tileStart[0] = 0;
  // tiles of 1024 lines: the unit of the decision below and of every form but the 64-byte one,
  // which recounts tileStart for its own tiles (launchStreamMultiN)
  const uint64_t lpt = uint64_t(kStreamThreads) * kStreamChains;
  for (uint32_t k = 0; k < nb && m.nb < uint32_t(kMultiMax); ++k) {
    const Batch &b = bs[k];
    if (!plain(b) || b.stride != bs[0].stride || (verb == kMatch && bool(b.start) != wantStart))
      break;
    const uint64_t tiles = (b.n + lpt - 1) / lpt;
    if (uint64_t(m.tileStart[m.nb]) + tiles >= (1ull << 31)) break;
    m.b[m.nb] = MultiPtrs{b.data, b.result, verb == kMatch ? b.start : nullptr,
                          verb == kMatch ? b.end : nullptr, b.n};
    m.tileStart[m.nb + 1] = m.tileStart[m.nb] + uint32_t(tiles);
    ++m.nb;
  }
  // (fewer tiles than CUs in all: the single-batch launches spread such lines better)
  // (one batch on its own keeps k_stream - unless its lines are long enough for the lean step,
  // or the lab says otherwise: REDGPU_MULTI_SINGLE=1)
  static const int labSingle = multiLabInt("REDGPU_MULTI_SINGLE", 0, 1, 0);
  const int mode = streamMode(style, wantStart);
  const bool lean = leanWanted(m, cfg) && mode != kSmFull;
  if (m.nb < ((labSingle || lean) ? 1u : 2u) ||
      (m.tileStart[m.nb] < uint32_t(cfg.numCUs) && !(lean && cfg.forceLean)))
    return hipSuccess;
  for (uint32_t k = m.nb; k < uint32_t(kMultiMax); ++k) m.tileStart[k + 1] = m.tileStart[m.nb];
  *kernelName = kStreamMultiNames[mode][lean ? 1 : 0];
#define MU_CALL(M) launchStreamMultiT<M>(d, m, cfg, stream)
  hipError_t e = [&]() -> hipError_t { REDGPU_MODE_SWITCH(MU_CALL) }();
#undef MU_CALL
  if (e != hipSuccess) return e;
  if (lead) {
    // match<..., true> only peeks the leader (Matcher.h:424-435): lines that fail it report {0,0,0}
    for (uint32_t k = 0; k < m.nb; ++k)
      if ((e = launchLeaderFilter(d, bs[k], cfg, stream)) != hipSuccess) return e;
  }
  *taken = m.nb;
  return hipSuccess;
}
#endif  // REDGPU_TU_STREAM

#if REDGPU_TU_RAGGED
static const char *const kRaggedNames[5][3] = {
    {"k_ragged<last,start,end>", "k_ragged<last,start,end,hot>", "k_ragged<last,start,end,cls>"},
    {"k_ragged<last,end>", "k_ragged<last,end,hot>", "k_ragged<last,end,cls>"},
    {},
    {"k_ragged<full,start>", "k_ragged<full,start,hot>", "k_ragged<full,start,cls>"},
    {"k_ragged<full>", "k_ragged<full,hot>", "k_ragged<full,cls>"}};

// k_ragged<mode> over the table form tabk
static hipError_t launchRaggedMode(int mode, int tabk, const DevDfa &d, const Batch &b,
                                   const LaunchCfg &cfg, hipStream_t stream) {
#define RG_FUSED(M) launchRaggedT<M, kTabFused>(d, b, cfg, stream)
#define RG_HOT(M) launchRaggedT<M, kTabHot>(d, b, cfg, stream)
#define RG_CLS(M) launchRaggedT<M, kTabCls>(d, b, cfg, stream)
#define RG_CLS_BIG(M) launchRaggedT<M, kTabClsBig>(d, b, cfg, stream)
  switch (tabk) {
  case kTabFused: REDGPU_MODE_SWITCH(RG_FUSED)
  case kTabHot: REDGPU_MODE_SWITCH(RG_HOT)
  case kTabCls: REDGPU_MODE_SWITCH(RG_CLS)
  default: REDGPU_MODE_SWITCH(RG_CLS_BIG)
  }
#undef RG_CLS_BIG
#undef RG_CLS
#undef RG_HOT
#undef RG_FUSED
}

// The ragged family of launchBatch: k_ragged over the fused, hot-row and class tables.
hipError_t launchRaggedFamily(const DevDfa &d, const Batch &b, int verb, int style, int doLeader,
                              const LaunchCfg &cfg, hipStream_t stream, const char **kernelName,
                              bool *handled) {
  *handled = false;
  const bool lead = doLeader && d.leaderLen > 0;
  const bool dying = d.earlyDeath && !cfg.forceStream;
  // Ragged lines, styles Last / Full of check / match, no leader to honour: k_ragged walks every
  // line; blocks that would reach past the end of the buffer come from a padded copy of its last
  // bytes.
  if (cfg.forceGeneric || dying || !b.offsets || b.n >= (1ull << 32) ||
      !wholeLineWalk(verb, style) || lead)
    return hipSuccess;
  // The fused-u8 table ...
  const bool raggedOk =
      fastPathEligible(d) && d.tableBytes <= kStreamTabBytes && d.nStates <= 256;
  // ... and the same for DFAs too big for LDS (hot rows, cold excursions re-walked per block).
  // On ragged text matches sit at any offset, so with the create-time ranking some lane of a
  // wave is in a cold excursion in nearly every block and the re-walks dominate (URI-V6 on
  // geometric-length text with a URL every ~8 lines: 128 GB/s untuned, 556 GB/s after
  // redgpu_dfa_tune) - still ahead of k_generic on the same lines (98 GB/s: its one-line-per-
  // lane walk also pays the wave-max of the line lengths); without URLs 629 vs 107 GB/s.
  const bool hotRaggedOk = !raggedOk && hotStreamEligible(d);
  // ... and for mid-size DFAs with a class table of at most 64 KB
  if (!raggedOk && !hotRaggedOk && !clsStreamEligible(d)) return hipSuccess;
  const int tabk = raggedOk      ? kTabFused
                   : hotRaggedOk ? kTabHot
                                 : (d.clsIndexForm ? kTabClsBig : kTabCls);
  const Batch sb = withoutPositions(b, verb);
  const int mode = streamMode(style, sb.start != nullptr);
  *handled = true;
  *kernelName = kRaggedNames[mode][nameForm(tabk)];
  return launchRaggedMode(mode, tabk, d, sb, cfg, stream);
}
#endif  // REDGPU_TU_RAGGED


#if REDGPU_TU_GENERIC
hipError_t launchCollect(const DevDfa &d, const Batch &b, uint64_t cap, uint64_t *counts,
                         const LaunchCfg &cfg, hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
#define CO_CALL(K) launchCollectK<K>(d, b, cap, counts, cfg, stream)
  REDGPU_KIND_SWITCH(CO_CALL)
#undef CO_CALL
}

// The scratch of the long-text verbs, for b.m chunks (collect, replace: of b.slots record slots
// each): every array rounded up to 16 bytes, 64 bytes of control words; returns the size, and over
// a null base hands out nothing else.
static uint64_t carveCollectLong(void *scratch, ClBufs &b) {
  Carve c{static_cast<uint8_t *>(scratch)};
  const uint64_t nb = (b.m + 1023) / 1024, recs = b.m * b.slots;
  b.ent = c.take16<uint64_t>(b.m);
  b.exit = c.take16<uint64_t>(b.m);
  b.off = c.take16<uint64_t>(b.m);
  b.blockOff = c.take16<uint64_t>(nb);
  b.ren = c.take16<uint64_t>(recs);
  b.rst = c.take16<uint64_t>(recs);
  b.res = c.take16<int32_t>(recs);
  b.rat = c.take16<uint32_t>(recs);
  b.cnt = c.take16<uint32_t>(b.m);
  b.work = c.take16<uint32_t>(b.m);
  b.ctl = c.take16<uint32_t>(16);
  return c.at;
}

static uint64_t carveReplaceLong(void *scratch, ClBufs &b, RlBufs &r) {
  Carve c{static_cast<uint8_t *>(scratch)};
  const uint64_t nb = (b.m + 1023) / 1024, recs = b.m * b.slots;
  b.ent = c.take16<uint64_t>(b.m);
  b.exit = c.take16<uint64_t>(b.m);
  b.off = c.take16<uint64_t>(b.m);
  r.rem = c.take16<uint64_t>(b.m);
  r.cov = c.take16<uint64_t>(b.m);
  b.blockOff = c.take16<uint64_t>(nb);
  r.blockRem = c.take16<uint64_t>(nb);
  r.blockCov = c.take16<uint64_t>(nb);
  b.ren = c.take16<uint64_t>(recs);
  b.rat = c.take16<uint32_t>(recs);
  b.cnt = c.take16<uint32_t>(b.m);
  b.work = c.take16<uint32_t>(b.m);
  b.ctl = c.take16<uint32_t>(16);
  return c.at;
}

static uint64_t carveSearchLong(void *scratch, SlBufs &b) {
  Carve c{static_cast<uint8_t *>(scratch)};
  b.ctl = c.take16<uint64_t>(8);
  b.rst = c.take16<uint64_t>(b.m);
  b.ren = c.take16<uint64_t>(b.m);
  b.res = c.take16<int32_t>(b.m);
  b.state = c.take16<uint32_t>(b.m);
  return c.at;
}

static uint64_t carveMatchAllLong(void *scratch, MlBufs &b) {
  Carve c{static_cast<uint8_t *>(scratch)};
  const uint64_t nb = (b.m + 1023) / 1024;
  b.esc = c.take16<uint64_t>(b.m);
  b.off = c.take16<uint64_t>(b.m);
  b.blockOff = c.take16<uint64_t>(nb);
  b.blockEsc = c.take16<uint64_t>(nb);
  b.ent = c.take16<uint32_t>(b.m);
  b.exit = c.take16<uint32_t>(b.m);
  b.cnt = c.take16<uint32_t>(b.m);
  b.head = c.take16<uint32_t>(b.m);
  b.work = c.take16<uint32_t>(b.m);
  b.ctl = c.take16<uint32_t>(16);
  return c.at;
}

// Red::collect over one text (k_collect_long.h): the chunked chain, the suffix-closed route or
// the one-lane k_collect - the same records either way.
hipError_t launchCollectLong(const DevDfa &d, const uint8_t *data, uint64_t n, uint32_t chunkBytes,
                             uint64_t cap, uint64_t *count, int32_t *result, uint64_t *start,
                             uint64_t *end, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName) {
  // attempts that end early: at a pure dead end, or (suffix-closed) by ending the chain; with
  // neither (SYN-256) every attempt runs to the end of the text and chunks would be quadratic
  const bool closed = d.nPureDead == 0 && d.suffixClosed && d.startFreeCount > 4 && cap > 0;
  const uint64_t c = collectLongChunk(n, chunkBytes, cfg);
  if (n == 0 || (!chunkBytes && n < kClMinText) || (d.nPureDead == 0 && !closed)) {
    *kernelName = "k_collect";
    const Batch b{data, nullptr, n, 1, result, start, end};
    return launchCollect(d, b, cap, count, cfg, stream);
  }
  if (closed) {
    // no pure dead state and L = SIGMA* L: the attempt at 0 walks the whole text, and nothing can
    // match behind its last accept - the chain is that one attempt, match<styLast,false>
    *kernelName = "k_collect_long<closed>";
    const Batch b{data, nullptr, n, 1, result, start, end};
    const char *inner = "";
    hipError_t e = launchBatch(d, b, kMatch, kStyLast, 0, cfg, stream, &inner);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cl_closed, dim3(1), dim3(64), 0, stream, result, count);
    return hipGetLastError();
  }
  *kernelName = "k_collect_long";
  ClBufs b{};
  b.m = (n + c - 1) / c;
  b.chunk = uint32_t(c);
  b.slots = c < n ? c : n;
  void *scratch = nullptr;
  hipError_t e = raggedScratch(stream, carveCollectLong(nullptr, b), &scratch);
  if (e != hipSuccess) return e;
  carveCollectLong(scratch, b);
#define CL_CALL(K) launchCollectLongK<K>(d, data, n, b, cap, count, result, start, end, cfg, stream)
  REDGPU_KIND_SWITCH(CL_CALL)
#undef CL_CALL
}

// replaceCore over one text (k_replace_long.h): the chain of k_collect_long.h under the call's
// style and leader setting, then the assembly.  phases: 1 = the chain, *count and *outLen; 2 = the
// copy into out, from the scratch phase 1 left on this stream; 3 = both.
hipError_t launchReplaceLong(const DevDfa &d, int style, int doLeader, const uint8_t *data,
                             uint64_t n, uint32_t chunkBytes, const uint8_t *repl, uint64_t replLen,
                             uint64_t max, uint64_t *count, uint64_t *outLen, uint8_t *out,
                             uint64_t outCap, int phases, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName) {
  *kernelName = "k_replace_long";
  if (n == 0) {
    if (phases & 1) hipLaunchKernelGGL(k_rl_empty, dim3(1), dim3(64), 0, stream, count, outLen);
    return hipGetLastError();
  }
  const LongAttempt a{style, doLeader && d.leaderLen > 0 ? 1 : 0};
  // one chunk (the chain in order, on one lane) for a short text, and where failing attempts
  // cannot end early: no pure dead state, under a style that walks on behind an accept
  const bool early = d.nPureDead > 0 || style == kStyInstant || style == kStyFirst ||
                     style == kStyTangent;
  uint64_t c = collectLongChunk(n, chunkBytes, cfg);
  if (!chunkBytes && (n < kClMinText || !early)) c = n;
  if (c > (1ull << 30)) c = 1ull << 30;  // (positions inside a chunk are 32-bit)
  if (c >= n) *kernelName = "k_replace_long<one>";
  ClBufs b{};
  RlBufs r{};
  b.m = (n + c - 1) / c;
  b.chunk = uint32_t(c < n ? c : n);
  b.slots = b.chunk;
  void *scratch = nullptr;
  hipError_t e = raggedScratch(stream, carveReplaceLong(nullptr, b, r), &scratch);
  if (e != hipSuccess) return e;
  carveReplaceLong(scratch, b, r);
  if (phases & 1) {
    e = [&]() -> hipError_t {
#define RL_CALL(K) launchClChain<K, kClReplace>(d, data, n, b, a, count, cfg, stream)
      REDGPU_KIND_SWITCH(RL_CALL)
#undef RL_CALL
    }();
    if (e != hipSuccess) return e;
  }
  return launchRlAssemble(data, n, b, r, repl, replLen, max, count, outLen, (phases & 1) != 0,
                          (phases & 2) ? out : nullptr, outCap, cfg, stream);
}

// searchCore over one text (k_search_long.h): chunks that try their own attempt positions, or the
// batch kernels over a batch of one - the same Outcome either way.
hipError_t launchSearchLong(const DevDfa &d, int style, int doLeader, const uint8_t *data, uint64_t n,
                            uint32_t chunkBytes, int32_t *result, uint64_t *start, uint64_t *end,
                            const LaunchCfg &cfg, hipStream_t stream, const char **kernelName) {
  const int lead = doLeader && d.leaderLen > 0 ? 1 : 0;
  // failing attempts end early at a pure dead end, or under a style that stops behind an accept
  const bool early = d.nPureDead > 0 || style == kStyInstant || style == kStyFirst ||
                     style == kStyTangent;
  // one lane: the empty text; and at the automatic size short texts, attempts that cannot end
  // early, and suffix-closed DFAs without the leader - their search is ONE anchored walk
  // (normalizeVerbStyle), which chunks of attempt positions would only repeat
  if (n == 0 || (!chunkBytes && (n < kClMinText || !early || (d.suffixClosed && !lead)))) {
    *kernelName = "k_search_long<one>";
    const Batch b{data, nullptr, n, 1, result, start, end};
    const char *inner = "";
    return launchBatch(d, b, kSearch, style, doLeader, cfg, stream, &inner);
  }
  *kernelName = "k_search_long";
  uint64_t c = searchLongChunk(n, chunkBytes, cfg);
  if (c > (1ull << 30)) c = 1ull << 30;  // (positions inside a chunk are 31-bit)
  SlBufs b{};
  b.m = (n + c - 1) / c;
  b.chunk = uint32_t(c);
  void *scratch = nullptr;
  hipError_t e = raggedScratch(stream, carveSearchLong(nullptr, b), &scratch);
  if (e != hipSuccess) return e;
  carveSearchLong(scratch, b);
  const LongAttempt a{style, lead};
  // the leader test in front of an accepting initial state: its passes are noted (k_long.h)
  const int mark = lead && d.init >= d.firstAccept ? 1 : 0;
#define SL_CALL(K) launchSearchLongK<K>(d, data, n, b, a, mark, result, start, end, cfg, stream)
  REDGPU_KIND_SWITCH(SL_CALL)
#undef SL_CALL
}

hipError_t launchMatchAll(const DevDfa &d, const Batch &b, uint64_t cap, uint64_t *counts,
                          int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                          const char **kernelName) {
  *kernelName = "k_matchall";
  if (b.n == 0) return hipSuccess;
  const int lead = doLeader && d.leaderLen > 0;
#define MA_CALL(K) launchMatchAllK<K>(d, b, cap, counts, lead, cfg, stream, kernelName)
  REDGPU_KIND_SWITCH(MA_CALL)
#undef MA_CALL
}

// matchAllCore over one text (k_match_all_long.h): the chunked walk, or the batch kernels over a
// batch of one - the same records either way.
hipError_t launchMatchAllLong(const DevDfa &d, int doLeader, const uint8_t *data, uint64_t n,
                              uint32_t chunkBytes, uint64_t cap, uint64_t *count, int32_t *result,
                              uint64_t *start, uint64_t *end, const LaunchCfg &cfg,
                              hipStream_t stream, const char **kernelName, const uint32_t **ctl) {
  *ctl = nullptr;
  // one lane: the empty text, short texts at the automatic size, and pure dead ends with a way
  // out - the walk's stop at one (Matcher.h:755-756) is then observable, and k_matchall has it
  if (n == 0 || (!chunkBytes && n < kClMinText) || !d.deadAbsorbing) {
    const Batch b{data, nullptr, n, 1, result, start, end};
    const char *inner = "";  // (the route's name stays "k_matchall", whichever instantiation runs)
    const hipError_t e = launchMatchAll(d, b, cap, count, doLeader, cfg, stream, &inner);
    *kernelName = "k_matchall";
    return e;
  }
  *kernelName = "k_match_all_long";
  const uint64_t c = collectLongChunk(n, chunkBytes, cfg);
  MlBufs b{};
  b.m = (n + c - 1) / c;
  b.chunk = uint32_t(c);
  void *scratch = nullptr;
  hipError_t e = raggedScratch(stream, carveMatchAllLong(nullptr, b), &scratch);
  if (e != hipSuccess) return e;
  carveMatchAllLong(scratch, b);
  *ctl = b.ctl;
  const int lead = doLeader && d.leaderLen > 0 ? 1 : 0;
#define ML_CALL(K) launchMatchAllLongK<K>(d, data, n, b, lead, cap, count, result, start, end, cfg, stream)
  REDGPU_KIND_SWITCH(ML_CALL)
#undef ML_CALL
}

template <int KIND>
hipError_t launchReplaceK(const DevDfa &d, const Batch &b, int style, int lead, const uint8_t *repl,
                          uint64_t replLen, uint64_t max, uint64_t *counts, uint64_t *outLens,
                          const uint64_t *outOffsets, uint8_t *out, uint64_t outCap,
                          const LaunchCfg &cfg, hipStream_t stream) {
  constexpr bool kLds = Tab<KIND>::kInLds || KIND == REDGPU_TAB_HOT_ROWS;
  constexpr int kThreads = kLds ? 1024 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_replace<KIND, kThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  uint64_t blocks = (b.n + kThreads - 1) / kThreads;
  const uint64_t perCu = kLds ? (ldsBytes <= 80 * 1024 ? 2 : 1) : 8;
  const uint64_t capBlocks = uint64_t(cfg.numCUs) * perCu;
  if (blocks > capBlocks) blocks = capBlocks;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL((k_replace<KIND, kThreads>), dim3(uint32_t(blocks)), dim3(kThreads), ldsBytes,
                     stream, d, b, style, lead, repl, replLen, max, counts, outLens, outOffsets,
                     out, outCap);
  return hipGetLastError();
}

static hipError_t launchReplacePass(const DevDfa &d, const Batch &b, int style, int lead,
                                    const uint8_t *repl, uint64_t replLen, uint64_t max,
                                    uint64_t *counts, uint64_t *outLens,
                                    const uint64_t *outOffsets, uint8_t *out, uint64_t outCap,
                                    const LaunchCfg &cfg, hipStream_t stream) {
#define RP_CALL(K) launchReplaceK<K>(d, b, style, lead, repl, replLen, max, counts, outLens, \
                                     outOffsets, out, outCap, cfg, stream)
  REDGPU_KIND_SWITCH(RP_CALL)
#undef RP_CALL
}

hipError_t launchReplace(const DevDfa &d, const Batch &b, int style, int doLeader,
                         const uint8_t *repl, uint64_t replLen, uint64_t max, uint64_t *counts,
                         uint64_t *outOffsets, uint8_t *out, uint64_t outCap,
                         const LaunchCfg &cfg, hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
  const int lead = doLeader && d.leaderLen > 0;
  // scratch: lens u64[n] + partials u64[ceil(n / 1024)]
  const uint64_t nPart = (b.n + 1023) / 1024;
  void *scratch = nullptr;
  hipError_t e = raggedScratch(stream, size_t(b.n + nPart) * 8 + 64, &scratch);
  if (e != hipSuccess) return e;
  uint64_t *lens = static_cast<uint64_t *>(scratch);
  uint64_t *partials = lens + b.n;
  e = launchReplacePass(d, b, style, lead, repl, replLen, max, counts, lens, nullptr, nullptr, 0,
                        cfg, stream);
  if (e != hipSuccess) return e;
  launchScan64(lens, b.n, partials, outOffsets, stream);
  e = hipGetLastError();
  if (e != hipSuccess || !out) return e;
  return launchReplacePass(d, b, style, lead, repl, replLen, max, counts, lens, outOffsets, out,
                           outCap, cfg, stream);
}

uint64_t splitChunks(uint64_t len) { return (len + kSplitChunk - 1) / kSplitChunk; }

uint64_t splitMaskBytes(uint64_t len) { return splitChunks(len) * (kSplitChunk / 8); }

// the grid of k_split_count and k_split_scatter: a workgroup takes kSplitGroup chunks
static uint32_t splitGroups(uint64_t nChunks) {
  return uint32_t((nChunks + kSplitGroup - 1) / kSplitGroup);
}

hipError_t launchSplitLines(const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *offsets,
                            uint64_t cap, uint64_t *nLines, uint32_t *counts, uint64_t *bases,
                            uint16_t *masks, hipStream_t stream) {
  const uint64_t nChunks = splitChunks(len);
  const uint32_t groups = splitGroups(nChunks);
  if (nChunks)
    hipLaunchKernelGGL(k_split_count, dim3(groups), dim3(kSplitThreads), 0, stream, data, len,
                       uint32_t(delim), nChunks, counts, masks);
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, counts, nChunks, bases, nLines,
                     offsets, cap);
  if (nChunks)
    hipLaunchKernelGGL(k_split_scatter, dim3(groups), dim3(kSplitThreads), 0, stream, masks,
                       nChunks, bases, offsets, cap);
  return hipGetLastError();
}

hipError_t launchTextIndex(const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *nLines,
                           uint32_t *counts, uint64_t *bases, uint16_t *masks, uint64_t *open,
                           uint16_t *zeroMasks, uint64_t *spare, int numCUs, hipStream_t stream) {
  const uint64_t nChunks = splitChunks(len);
  if (nChunks) {
    hipLaunchKernelGGL(k_split_count, dim3(splitGroups(nChunks)), dim3(kSplitThreads), 0, stream,
                       data, len, uint32_t(delim), nChunks, counts, masks);
  }
  // (k_split_scan's offsets[0] store goes to a spare word)
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, counts, nChunks, bases,
                     nLines ? nLines : spare, spare + 1, uint64_t(0));
  if (nChunks) {
    hipLaunchKernelGGL(k_gp_last, dim3(smallBlocks(nChunks, numCUs)), dim3(256), 0, stream, masks,
                       counts, nChunks, open, zeroMasks);
    hipLaunchKernelGGL(k_gp_open, dim3(1), dim3(1024), 0, stream, open, nChunks);
  }
  return hipGetLastError();
}

hipError_t launchDiagRead(const void *data, uint64_t bytes, uint32_t *sink, int numCUs,
                          hipStream_t stream) {
  if (bytes < 16) return hipSuccess;
  hipLaunchKernelGGL(k_diag_read, dim3(uint32_t(numCUs)), dim3(512), 0, stream,
                     static_cast<const uint4 *>(data), bytes / 16, sink);
  return hipGetLastError();
}

hipError_t launchDiagL2(const uint16_t *table, uint32_t rounds, uint32_t *sink, int numCUs,
                        hipStream_t stream, uint64_t *lookups) {
  constexpr int kCh = 2;
  hipLaunchKernelGGL((k_diag_l2<kCh>), dim3(uint32_t(numCUs) * 8), dim3(256), 0, stream, table, rounds,
                     sink);
  if (lookups) *lookups = uint64_t(numCUs) * 8 * 256 * kCh * rounds;
  return hipGetLastError();
}

hipError_t launchDiagLines(const uint8_t *data, uint64_t nLines, uint32_t lineBytes, int32_t *res,
                           uint64_t *st, uint64_t *en, uint32_t *sink, int numCUs,
                           hipStream_t stream) {
  if (lineBytes != 64) {
    if (nLines < 1024) return hipSuccess;
    hipLaunchKernelGGL(k_diag_long, dim3(uint32_t(numCUs)), dim3(512), 0, stream, data, nLines,
                       lineBytes, sink);
    return hipGetLastError();
  }
  // two workgroups per CU when the tiles allow, as launchStreamMultiN
  const uint64_t tiles = nLines / (2 * uint64_t(kResidentThreads)), want = uint64_t(numCUs) * 2;
  if (tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_diag_lines<kResidentThreads>, dim3(uint32_t(tiles < want ? tiles : want)),
                     dim3(kResidentThreads), 0, stream, data, nLines, res, st, en, sink);
  return hipGetLastError();
}

template <int KIND>
hipError_t launchWalkedK(const DevDfa &d, const Batch &b, int lead, unsigned long long *walked,
                         const LaunchCfg &cfg, hipStream_t stream) {
  constexpr bool kLds = Tab<KIND>::kInLds || KIND == REDGPU_TAB_HOT_ROWS;
  constexpr int kThreads = kLds ? 1024 : 256;
  const size_t ldsBytes = 512 + ldsTableBytes<KIND>(d);
  hipError_t e = setLds(k_walked<KIND, kThreads>, ldsBytes);
  if (e != hipSuccess) return e;
  uint64_t blocks = (b.n + kThreads - 1) / kThreads;
  const uint64_t perCu = kLds ? (ldsBytes <= 80 * 1024 ? 2 : 1) : 8;
  const uint64_t capBlocks = uint64_t(cfg.numCUs) * perCu;
  if (blocks > capBlocks) blocks = capBlocks;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL((k_walked<KIND, kThreads>), dim3(uint32_t(blocks)), dim3(kThreads), ldsBytes,
                     stream, d, b, lead, walked);
  return hipGetLastError();
}

hipError_t launchWalked(const DevDfa &d, const Batch &b, int doLeader, unsigned long long *walked,
                        const LaunchCfg &cfg, hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
  const int lead = doLeader && d.leaderLen > 0;
#define WK_CALL(K) launchWalkedK<K>(d, b, lead, walked, cfg, stream)
  REDGPU_KIND_SWITCH(WK_CALL)
#undef WK_CALL
}

hipError_t launchVisits(const DevDfa &d, const Batch &b, uint32_t *hist, const LaunchCfg &cfg,
                        hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
#define VI_CALL(K) launchVisitsK<K>(d, b, hist, cfg, stream)
  REDGPU_KIND_SWITCH(VI_CALL)
#undef VI_CALL
}

hipError_t launchAdvance(const DevDfa &d, const Batch &b, uint32_t *state, const LaunchCfg &cfg,
                         hipStream_t stream, const char **kernelName) {
  *kernelName = "k_advance";
  if (b.n == 0) return hipSuccess;
  bool handled = false;
  hipError_t se = launchAdvanceStream(d, b, state, cfg, stream, kernelName, &handled);
  if (handled || se != hipSuccess) return se;
#define AD_CALL(K) launchAdvanceK<K>(d, b, state, cfg, stream)
  REDGPU_KIND_SWITCH(AD_CALL)
#undef AD_CALL
}

#endif  // REDGPU_TU_GENERIC

// The identities launchBatch applies before it picks a kernel.
[[maybe_unused]] static void normalizeVerbStyle(const DevDfa &d, const LaunchCfg &cfg, bool lead, int &verb,
                               int &style) {
  // L = SIGMA* L (DfaImage::suffixClosed - patterns added with a loose start) and no leader: the
  // sliding loops of scan and search (Matcher.h:511-553, :575-621) ARE their first attempt.  It
  // cannot meet a pure dead end (from any reachable state something is still accepted), so it
  // either returns per the style's rules - as check / match from position 0 would, same loop
  // body - or reads the line to its end without an accepting state, and then no later start
  // position can accept either: the text it would read is a suffix of what this attempt read.
  // The reference walks every one of them (O(n^2) on a line without a match) to that same 0.
  if (d.suffixClosed && !lead) {
    if (verb == kScan) verb = kCheck;
    else if (verb == kSearch) verb = kMatch;
  }
  // check over a DFA whose accepting states all report ONE result (a single pattern): styInstant,
  // styFirst and styTangent each return the result of SOME accepting state of the walk, styLast
  // that of the last one - the same value, and 0 alike when none accepts (Matcher.h:382-409).
  // styLast is the style the streaming kernels run; an early-death DFA keeps its early exits.
  if (verb == kCheck && !lead && d.uniformResult && !d.earlyDeath && !cfg.forceGeneric &&
      (style == kStyInstant || style == kStyFirst || style == kStyTangent))
    style = kStyLast;
}

// A line verb of the raw-text family (does this line match?): the leader flag, and search under the
// call's style as normalizeVerbStyle leaves them - verb = kSearch or kMatch.  normalize = false: the
// form at hand is no line verb (tally_text's and uniq_text's MATCHES), only the leader flag is wanted.
struct LineVerb {
  int lead, verb, style;
};
[[maybe_unused]] static LineVerb lineVerb(const DevDfa &d, const LaunchCfg &cfg, int doLeader,
                                          int style, bool normalize = true) {
  LineVerb v{doLeader && d.leaderLen > 0 ? 1 : 0, kSearch, style};
  if (normalize) normalizeVerbStyle(d, cfg, v.lead != 0, v.verb, v.style);
  return v;
}

// LAUNCH<K, kSearch>(args) or LAUNCH<K, kMatch>(args), by the LineVerb `v` in scope
#define REDGPU_LINE_VERB(LAUNCH, K, ...) \
  (v.verb == kSearch ? LAUNCH<K, kSearch>(__VA_ARGS__) : LAUNCH<K, kMatch>(__VA_ARGS__))

// the DevDfa the LDS-room rules of tally_text, sum_text and uniq_text read
[[maybe_unused]] static DevDfa ldsRoomDfa(uint32_t tableKind, uint32_t tableBytes,
                                          uint32_t nStates) {
  DevDfa d{};
  d.tableKind = tableKind;
  d.tableBytes = tableBytes;
  d.nStates = nStates;
  return d;
}

#if REDGPU_TU_GREP || REDGPU_TU_COLLECT_TEXT
// the scratch of grep and of grep -o, for a text of nChunks split chunks: what launchTextIndex
// fills, a count and a base per chunk for the records, four spare words, the two bitmaps
struct RecordScratch {
  uint64_t *bases, *open, *recBases;  // [nChunks] each
  uint32_t *counts, *recCounts;       // [nChunks] each
  uint64_t *misc;                     // [4]: lines, the scans' spare word, two of the verb's
  uint16_t *masks, *hitMasks;         // the delimiter bitmap, the selected / hit bitmap
  uint64_t bytes;
  RecordScratch(void *scratch, uint64_t nChunks) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    recBases = c.take<uint64_t>(nChunks);
    counts = c.take<uint32_t>(nChunks);
    recCounts = c.take<uint32_t>(nChunks);
    misc = c.take<uint64_t>(4);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    hitMasks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};
#endif

#if REDGPU_TU_GREP
// grep over a raw text (k_grep.h): the line index (launchTextIndex), then the k_gp_* passes.
// scratch: grepScratchBytes(len) bytes, 16-byte aligned.
uint64_t grepScratchBytes(uint64_t len) { return RecordScratch(nullptr, splitChunks(len)).bytes; }

hipError_t launchGrepText(const DevDfa &d, int style, int doLeader, int invert, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t maxCount, uint64_t cap,
                          uint64_t *nLines, uint64_t *nSelected, uint64_t *line, uint64_t *begin,
                          uint64_t *finish, int32_t *result, uint64_t *start, uint64_t *end,
                          void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                          const char **kernelName) {
  *kernelName = "k_grep_text";
  const uint64_t nChunks = splitChunks(len);
  const RecordScratch m(scratch, nChunks);
  uint64_t *dummy = m.misc + 1, *total = m.misc + 2;
  const hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                       m.hitMasks, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  const LineVerb v = lineVerb(d, cfg, doLeader, style);
  const GpBufs b{m.masks, m.hitMasks, m.bases, m.open, m.recCounts, m.recBases, nChunks};
  const GpOut out{cap < maxCount ? cap : maxCount, line, begin, finish, result, start, end};
  const bool write = out.limit > 0 && (line || begin || finish || result || start || end);
#define GP_CALL(K)                                                                              \
  REDGPU_LINE_VERB(launchGrepK, K, d, data, b, v.style, v.lead, invert, out, write, total,      \
                   maxCount, nSelected, m.recBases, dummy, cfg, stream)
  REDGPU_KIND_SWITCH(GP_CALL)
#undef GP_CALL
}

// grep's output over a raw text (k_filter_text.h): the line index (launchTextIndex), k_grep.h's
// select pass, then the k_ft_* passes around k_gp_open's and k_misc.h's scans.  scratch:
// filterTextScratchBytes(len) bytes, 16-byte aligned: the two bitmaps (len / 4), and 68 bytes per
// chunk, 8 per 1,024 chunks and 72, rounded up to 16.
struct FilterScratch {
  uint64_t *bases, *open, *selBases, *prevSel, *nextRev, *emitBytes;  // [nChunks] each
  uint64_t *outBases;                                                 // [nChunks + 1]
  uint64_t *partials;                                                 // [nPart]
  uint64_t *misc;  // [8]: lines, the scans' spare word, the selected total, 3 for absent counts, 2 spare
  uint32_t *counts, *selCounts, *emitLines;  // [nChunks] each
  uint16_t *masks, *selMasks;  // the delimiter bitmap, the SELECTED bitmap and then the EMIT one
  uint64_t nPart, bytes;
  FilterScratch(void *scratch, uint64_t nChunks) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    selBases = c.take<uint64_t>(nChunks);
    prevSel = c.take<uint64_t>(nChunks);
    nextRev = c.take<uint64_t>(nChunks);
    emitBytes = c.take<uint64_t>(nChunks);
    outBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    selCounts = c.take<uint32_t>(nChunks);
    emitLines = c.take<uint32_t>(nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    selMasks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t filterTextScratchBytes(uint64_t len) {
  return FilterScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchFilterText(const DevDfa &d, int style, int doLeader, int invert, uint64_t before,
                            uint64_t after, uint64_t maxCount, const uint8_t *data, uint64_t len,
                            uint8_t delim, uint64_t *nLines, uint64_t *nSelected,
                            uint64_t *nEmitted, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                            int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                            const char **kernelName) {
  *kernelName = "k_filter_text";
  const uint64_t nChunks = splitChunks(len);
  const FilterScratch m(scratch, nChunks);
  uint64_t *dummy = m.misc + 1, *total = m.misc + 2;
  const GpBufs b{m.masks, m.selMasks, m.bases, m.open, m.selCounts, m.selBases, nChunks};
  const uint32_t small = smallBlocks(nChunks, cfg.numCUs);
  if (phases & 1) {
    hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                   m.selMasks, m.misc, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    const LineVerb v = lineVerb(d, cfg, doLeader, style);
    // k_gp_select, the scan of selCounts and k_gp_total; no records
    const GpOut none{};
#define FT_CALL(K)                                                                              \
  REDGPU_LINE_VERB(launchGrepK, K, d, data, b, v.style, v.lead, invert, none, false, total,     \
                   maxCount, nSelected ? nSelected : m.misc + 3, m.selBases, dummy, cfg, stream)
    e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(FT_CALL) }();
#undef FT_CALL
    if (e != hipSuccess) return e;
    if (nChunks) {
      hipLaunchKernelGGL(k_ft_edges, dim3(small), dim3(256), 0, stream, b, maxCount, m.prevSel,
                         m.nextRev);
      hipLaunchKernelGGL(k_gp_open, dim3(1), dim3(1024), 0, stream, m.prevSel, nChunks);
      hipLaunchKernelGGL(k_gp_open, dim3(1), dim3(1024), 0, stream, m.nextRev, nChunks);
      hipLaunchKernelGGL(k_ft_mark, dim3(small), dim3(256), 0, stream, b, maxCount, before, after,
                         m.prevSel, m.nextRev, m.emitBytes, m.emitLines);
      launchScan64(m.emitBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_ft_totals, dim3(1), dim3(1024), 0, stream, m.emitLines, nChunks,
                       nChunks ? m.outBases + nChunks : nullptr, outLen,
                       nEmitted ? nEmitted : m.misc + 4);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) {
    hipLaunchKernelGGL(k_ft_write, dim3(small), dim3(256), 0, stream, data, b,
                       m.emitBytes, m.outBases, out, outCap);
  }
  return hipGetLastError();
}
#endif  // REDGPU_TU_GREP

#if REDGPU_TU_COLLECT_TEXT
// grep -o over a raw text (k_collect_text.h): the line index (launchTextIndex), then the k_ct_*
// passes.  scratch: collectTextScratchBytes(len) bytes, 16-byte aligned - what grep takes.
uint64_t collectTextScratchBytes(uint64_t len) {
  return RecordScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchCollectText(const DevDfa &d, const uint8_t *data, uint64_t len, uint8_t delim,
                             uint64_t cap, uint64_t *nLines, uint64_t *nMatches, uint64_t *line,
                             uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end,
                             void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName) {
  *kernelName = "k_collect_text";
  const uint64_t nChunks = splitChunks(len);
  const RecordScratch m(scratch, nChunks);
  uint64_t *dummy = m.misc + 1;
  const hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                       m.hitMasks, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  const GpBufs b{m.masks, m.hitMasks, m.bases, m.open, m.recCounts, m.recBases, nChunks};
  const CtOut out{cap, line, begin, result, start, end};
  const bool write = cap > 0 && (line || begin || result || start || end);
#define CT_CALL(K) \
  launchCollectTextK<K>(d, data, b, out, write, nMatches, m.recBases, dummy, cfg, stream)
  REDGPU_KIND_SWITCH(CT_CALL)
#undef CT_CALL
}
#endif  // REDGPU_TU_COLLECT_TEXT

#if REDGPU_TU_TALLY_TEXT || REDGPU_TU_SUM_TEXT
// grep -c per result over a raw text (k_tally_text.h): the line index (launchTextIndex), then
// k_tl_zero and the one pass of k_tally_text.  scratch: tallyTextScratchBytes(len) bytes, 16-byte
// aligned: ONE bitmap and 20 bytes per chunk.
struct TallyScratch {
  uint64_t *bases, *open;  // [nChunks] each
  uint64_t *misc;          // [4]: lines, the scan's spare word, items, one spare
  uint16_t *masks;         // the delimiter bitmap
  uint32_t *counts;        // [nChunks]
  uint64_t bytes;
  TallyScratch(void *scratch, uint64_t nChunks) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    misc = c.take<uint64_t>(4);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    counts = c.take<uint32_t>(nChunks);
    c.align(16);
    bytes = c.at;
  }
};
#endif

#if REDGPU_TU_TALLY_TEXT
uint64_t tallyTextScratchBytes(uint64_t len) {
  return TallyScratch(nullptr, splitChunks(len)).bytes;
}

uint32_t tallyLdsBins(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates) {
  const DevDfa d = ldsRoomDfa(tableKind, tableBytes, nStates);
#define TL_BINS(K) tallyLdsBinsK<K>(d)
  REDGPU_KIND_SWITCH(TL_BINS)
#undef TL_BINS
}

hipError_t launchTallyText(const DevDfa &d, int what, int style, int doLeader, const uint8_t *data,
                           uint64_t len, uint8_t delim, uint64_t nBins, int accumulate, int plain,
                           uint64_t *nLines, uint64_t *nItems, uint64_t *bins, void *scratch,
                           const LaunchCfg &cfg, hipStream_t stream, const char **kernelName) {
  *kernelName = "k_tally_text";
  const uint64_t nChunks = splitChunks(len);
  const TallyScratch m(scratch, nChunks);
  // (no selected bitmap to zero)
  hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                 nullptr, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  const uint64_t toZero = accumulate ? 0 : nBins + 1;
  const uint32_t zb = wordBlocks(toZero, cfg.numCUs);
  TallyOut o{reinterpret_cast<unsigned long long *>(bins),
             reinterpret_cast<unsigned long long *>(nItems ? nItems : m.misc + 2), uint32_t(nBins),
             0};
  hipLaunchKernelGGL(k_tl_zero, dim3(zb ? zb : 1), dim3(256), 0, stream, o.bins, toZero, o.nItems);
  e = hipGetLastError();
  if (e != hipSuccess || nChunks == 0) return e;
  const LineVerb v = lineVerb(d, cfg, doLeader, style, what == REDGPU_TALLY_LINES);
  // L: the leading bins kept in LDS.  32-bit counters hold a text below 4 GiB whatever it is
  // (k_tally_text.h: tallyAdd); a longer text counts in global memory alone
  const uint32_t room = len < (1ull << 32) ? tallyLdsBins(d.tableKind, d.tableBytes, d.nStates) : 0u;
  o.ldsBins = nBins + 1 < room ? uint32_t(nBins + 1) : room;
  const GpBufs b{m.masks, nullptr, m.bases, m.open, nullptr, nullptr, nChunks};
#define TL_ARGS d, data, b, v.style, v.lead, plain, o, cfg, stream
#define TL_CALL(K)                                                                    \
  (what == REDGPU_TALLY_MATCHES ? launchTallyK<K, kTallyMatches>(TL_ARGS)             \
   : v.verb == kSearch          ? launchTallyK<K, kTallyLines>(TL_ARGS)               \
                                : launchTallyK<K, kTallyLinesMatch>(TL_ARGS))
  REDGPU_KIND_SWITCH(TL_CALL)
#undef TL_CALL
#undef TL_ARGS
}
#endif  // REDGPU_TU_TALLY_TEXT

#if REDGPU_TU_SUM_TEXT
// per result the count, sum, min and max of the numbers in a raw text's matches (k_sum_text.h): the
// line index (launchTextIndex), then k_sm_zero and the one pass of k_sum_text.  scratch:
// sumTextScratchBytes(len) bytes, 16-byte aligned: launchTallyText's.
uint64_t sumTextScratchBytes(uint64_t len) {
  return TallyScratch(nullptr, splitChunks(len)).bytes;
}

uint32_t sumLdsBins(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates) {
  const DevDfa d = ldsRoomDfa(tableKind, tableBytes, nStates);
#define SM_BINS(K) sumLdsBinsK<K>(d)
  REDGPU_KIND_SWITCH(SM_BINS)
#undef SM_BINS
}

hipError_t launchSumText(const DevDfa &d, int which, const uint8_t *data, uint64_t len,
                         uint8_t delim, uint64_t maxPerLine, uint64_t nBins, int accumulate,
                         int plain, uint64_t *nLines, uint64_t *nItems, uint64_t *nNumeric,
                         uint64_t *stats, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                         const char **kernelName) {
  *kernelName = "k_sum_text";
  const uint64_t nChunks = splitChunks(len);
  const TallyScratch m(scratch, nChunks);
  // (no selected bitmap to zero)
  hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                 nullptr, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  const uint64_t toZero = accumulate ? 0 : nBins + 1;
  const uint32_t zb = wordBlocks(toZero, cfg.numCUs);
  SumOut o{reinterpret_cast<unsigned long long *>(stats),
           reinterpret_cast<unsigned long long *>(nItems ? nItems : m.misc + 2),
           reinterpret_cast<unsigned long long *>(nNumeric ? nNumeric : m.misc + 3),
           nBins + 1, uint32_t(nBins), 0};
  hipLaunchKernelGGL(k_sm_zero, dim3(zb ? zb : 1), dim3(256), 0, stream, o.stats, toZero, o.nItems,
                     o.nNumeric);
  e = hipGetLastError();
  if (e != hipSuccess || nChunks == 0 || maxPerLine == 0) return e;
  // L: the leading slots kept in LDS; 64-bit words, so a text of any length may use them
  const uint32_t room = sumLdsBins(d.tableKind, d.tableBytes, d.nStates);
  o.ldsBins = nBins + 1 < room ? uint32_t(nBins + 1) : room;
  const GpBufs b{m.masks, nullptr, m.bases, m.open, nullptr, nullptr, nChunks};
#define SM_CALL(K) launchSumK<K>(d, data, len, b, which, maxPerLine, plain, o, cfg, stream)
  REDGPU_KIND_SWITCH(SM_CALL)
#undef SM_CALL
}
#endif  // REDGPU_TU_SUM_TEXT

#if REDGPU_TU_REPLACE_TEXT || REDGPU_TU_EXTRACT_TEXT
// the scratch of sed and of grep -o's text, for a text of nChunks split chunks: what launchTextIndex
// fills, the output bytes and the replacements (extract_text: the pieces) per chunk, the scan's
// arrays, eight spare words, the two bitmaps - the two bitmaps, and 44 bytes per chunk, 8 per 1,024
// chunks and 72, rounded up to 16
struct ReplaceScratch {
  uint64_t *bases, *open, *outBytes, *replCounts;  // [nChunks] each
  uint64_t *outBases;                              // [nChunks + 1]
  uint64_t *partials;                              // [nPart]
  uint64_t *misc;               // [8]: lines, the scan's spare word, replaced, tailAt[2], 3 spare
  uint32_t *counts;             // [nChunks]
  uint16_t *masks, *hitMasks;   // the delimiter bitmap, the hit bitmap
  uint64_t nPart, bytes;
  ReplaceScratch(void *scratch, uint64_t nChunks) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    outBytes = c.take<uint64_t>(nChunks);
    replCounts = c.take<uint64_t>(nChunks);
    outBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    hitMasks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};
#endif

#if REDGPU_TU_REPLACE_TEXT
// sed over a raw text (k_replace_text.h): the line index (launchTextIndex), then the k_rt_* passes
// around k_misc.h's 64-bit scan.  scratch: replaceTextScratchBytes(len) bytes, 16-byte aligned.
uint64_t replaceTextScratchBytes(uint64_t len) {
  return ReplaceScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchReplaceText(const DevDfa &d, int style, int doLeader, int onlyChanged,
                             const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                             uint64_t replLen, uint64_t max, uint64_t *nLines, uint64_t *nReplaced,
                             uint64_t *outLen, uint8_t *out, uint64_t outCap, int phases,
                             void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName) {
  *kernelName = "k_replace_text";
  const uint64_t nChunks = splitChunks(len);
  const ReplaceScratch m(scratch, nChunks);
  uint64_t *tailAt = m.misc + 3;
  const int lead = doLeader && d.leaderLen > 0 ? 1 : 0;
  const GpBufs b{m.masks, m.hitMasks, m.bases, m.open, nullptr, nullptr, nChunks};
  const RtBufs r{m.outBytes, m.replCounts, m.outBases};
  const RtArgs a{style, lead, onlyChanged, uint32_t(delim), repl, replLen, max};
#define RT_CALL(K) launchReplaceTextK<K>(d, data, b, r, a, count, out, outCap, cfg, stream)
  auto pass = [&](bool count) { REDGPU_KIND_SWITCH(RT_CALL) };
#undef RT_CALL
  if (phases & 1) {
    hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                   m.hitMasks, m.misc, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (nChunks) {
      e = pass(true);
      if (e != hipSuccess) return e;
      launchScan64(m.outBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_rt_totals, dim3(1), dim3(1024), 0, stream, m.replCounts, nChunks,
                       nChunks ? m.outBases + nChunks : nullptr, m.masks, m.open, len, onlyChanged,
                       tailAt, outLen, nReplaced ? nReplaced : m.misc + 2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) {
    const hipError_t e = pass(false);
    if (e != hipSuccess) return e;
    if (!onlyChanged) {
      hipLaunchKernelGGL(k_rt_tail, dim3(uint32_t(cfg.numCUs) * 4), dim3(256), 0, stream, data, len,
                         tailAt, out, outCap);
    }
  }
  return hipGetLastError();
}
#endif  // REDGPU_TU_REPLACE_TEXT

#if REDGPU_TU_EXTRACT_TEXT
// grep -o's output as a text (k_extract_text.h): the line index (launchTextIndex), then the k_xt_*
// passes around k_misc.h's 64-bit scan.  scratch: extractTextScratchBytes(len) bytes, 16-byte
// aligned - what sed takes (ReplaceScratch: replCounts holds the chunks' pieces).
uint64_t extractTextScratchBytes(uint64_t len) {
  return ReplaceScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchExtractText(const DevDfa &d, const uint8_t *data, uint64_t len, uint8_t delim,
                             uint64_t maxPerLine, uint32_t hand, uint64_t *nLines,
                             uint64_t *nMatches, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                             int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                             const char **kernelName) {
  *kernelName = "k_extract_text";
  const uint64_t nChunks = splitChunks(len);
  const ReplaceScratch m(scratch, nChunks);
  const GpBufs b{m.masks, m.hitMasks, m.bases, m.open, nullptr, nullptr, nChunks};
  const XtBufs x{m.outBytes, m.replCounts, m.outBases};
  if (hand == 0) hand = kXtHand;
#define XT_CALL(K) \
  launchExtractTextK<K>(d, data, len, b, x, maxPerLine, delim, hand, size, out, outCap, cfg, stream)
  auto pass = [&](bool size) { REDGPU_KIND_SWITCH(XT_CALL) };
#undef XT_CALL
  if (phases & 1) {
    hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                   m.hitMasks, m.misc, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (nChunks) {
      e = pass(true);
      if (e != hipSuccess) return e;
      launchScan64(m.outBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_xt_totals, dim3(1), dim3(1024), 0, stream, m.replCounts, nChunks,
                       nChunks ? m.outBases + nChunks : nullptr, outLen,
                       nMatches ? nMatches : m.misc + 2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) return pass(false);
  return hipGetLastError();
}
#endif  // REDGPU_TU_EXTRACT_TEXT

#if REDGPU_TU_FIELDS_TEXT
// awk -F's columns of a raw text (k_fields_text.h): the line index (launchTextIndex), then the
// k_fd_* passes around k_misc.h's 64-bit scan.  scratch: fieldsTextScratchBytes(len) bytes, 16-byte
// aligned: what sed takes (ReplaceScratch's layout) plus one u64 per chunk - the two bitmaps, and
// 52 bytes per chunk, 8 per 1,024 chunks and 72, rounded up to 16.
struct FieldsScratch {
  uint64_t *bases, *open, *outBytes, *lineCounts, *fieldCounts;  // [nChunks] each
  uint64_t *outBases;                                            // [nChunks + 1]
  uint64_t *partials;                                            // [nPart]
  uint64_t *misc;               // [8]: lines, the scan's spare word, emitted, fields, 4 spare
  uint32_t *counts;             // [nChunks]
  uint16_t *masks, *hitMasks;   // the delimiter bitmap, the hit bitmap (only_delimited)
  uint64_t nPart, bytes;
  FieldsScratch(void *scratch, uint64_t nChunks) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    outBytes = c.take<uint64_t>(nChunks);
    lineCounts = c.take<uint64_t>(nChunks);
    fieldCounts = c.take<uint64_t>(nChunks);
    outBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    hitMasks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t fieldsTextScratchBytes(uint64_t len) {
  return FieldsScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchFieldsText(const DevDfa &d, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t select, uint64_t maxFields, int onlyDelimited, uint64_t sep,
                            uint32_t sepLen, uint64_t *nLines, uint64_t *nEmitted,
                            uint64_t *nFields, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                            int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                            const char **kernelName) {
  *kernelName = "k_fields_text";
  const uint64_t nChunks = splitChunks(len);
  const FieldsScratch m(scratch, nChunks);
  // without only_delimited every line is emitted: the write pass is driven from the delimiter
  // bitmap itself, and there is no hit bitmap to zero or to fill
  uint16_t *emitted = onlyDelimited ? m.hitMasks : m.masks;
  const GpBufs b{m.masks, emitted, m.bases, m.open, nullptr, nullptr, nChunks};
  const FdBufs x{m.outBytes, m.lineCounts, m.fieldCounts, m.outBases};
  // the chain is left behind separator min(S, hi): S = maxFields - 1 (0 = unbounded), hi = the
  // highest selected field (bit 63 = unbounded)
  const uint64_t most = maxFields ? maxFields - 1 : ~0ull;
  uint64_t hi = ~0ull;
  if (!(select >> 63)) {
    hi = 0;
    while (select >> hi) ++hi;
  }
  const FdArgs a{select, most < hi ? most : hi, sep, sepLen, uint32_t(delim), onlyDelimited ? 1 : 0};
#define FD_CALL(K) launchFieldsTextK<K>(d, data, len, b, x, a, size, out, outCap, cfg, stream)
  auto pass = [&](bool size) { REDGPU_KIND_SWITCH(FD_CALL) };
#undef FD_CALL
  if (phases & 1) {
    hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                   onlyDelimited ? m.hitMasks : nullptr, m.misc, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (nChunks) {
      e = pass(true);
      if (e != hipSuccess) return e;
      launchScan64(m.outBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_fd_totals, dim3(1), dim3(1024), 0, stream, m.lineCounts, m.fieldCounts,
                       nChunks, nChunks ? m.outBases + nChunks : nullptr, outLen,
                       nEmitted ? nEmitted : m.misc + 2, nFields ? nFields : m.misc + 3);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) return pass(false);
  return hipGetLastError();
}
#endif  // REDGPU_TU_FIELDS_TEXT

#if REDGPU_TU_ROUTE_TEXT
// a raw text's lines grouped by result (k_route_text.h): the line index (launchTextIndex), then the
// k_ro_* passes around k_misc.h's scan.  A line's code is its bucket, except under nBins == 0 with
// dropUnmatched, where it is "the line matches" (k_route_text.h: zeroCode).  scratch:
// routeTextScratchBytes(len, nBins, dropUnmatched) bytes, 16-byte aligned: 1 + P bitmaps (len / 8
// each), 20 bytes per chunk, 20 per (code, chunk), 8 per 1,024 of those and 72, rounded up to 16.
struct RouteScratch {
  uint64_t *bases, *open;  // [nChunks] each
  uint64_t *sizes;         // [nCodes * nChunks]
  uint64_t *outBases;      // [nCodes * nChunks + 1]
  uint64_t *partials;      // [nPart]
  uint64_t *misc;          // [8]: lines, the scan's two spare words, 5 spare
  uint32_t *counts;        // [nChunks]
  uint32_t *lines;         // [nCodes * nChunks]
  uint16_t *masks, *planes;  // the delimiter bitmap, the nPlanes planes of the lines' codes
  uint32_t nCodes, nPlanes;
  int zeroCode;
  uint64_t nCells, nPart, bytes;
  RouteScratch(void *scratch, uint64_t nChunks, uint64_t nBins, int dropUnmatched) {
    zeroCode = nBins == 0 && dropUnmatched;
    nCodes = zeroCode ? 2u : uint32_t(nBins) + 1;
    nPlanes = 0;
    while ((nCodes - 1) >> nPlanes) ++nPlanes;
    nCells = uint64_t(nCodes) * nChunks;
    nPart = (nCells + 1023) / 1024;
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    sizes = c.take<uint64_t>(nCells);
    outBases = c.take<uint64_t>(nCells + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    lines = c.take<uint32_t>(nCells);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    planes = c.take<uint16_t>(nPlanes * nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t routeTextScratchBytes(uint64_t len, uint64_t nBins, int dropUnmatched) {
  return RouteScratch(nullptr, splitChunks(len), nBins, dropUnmatched).bytes;
}

hipError_t launchRouteText(const DevDfa &d, int style, int doLeader, int dropUnmatched,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t nBins,
                           uint64_t *nLines, uint64_t *nRouted, uint64_t *binLines,
                           uint64_t *binOffsets, uint64_t *outLen, uint8_t *out, uint64_t outCap,
                           int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                           const char **kernelName) {
  *kernelName = "k_route_text";
  const uint64_t nChunks = splitChunks(len);
  const RouteScratch m(scratch, nChunks, nBins, dropUnmatched);
  // (TextHits loads a verb's bitmap beside the delimiters': there is none here, it gets the latter)
  const GpBufs b{m.masks, m.masks, m.bases, m.open, nullptr, nullptr, nChunks};
  const RoBufs r{m.planes, nChunks * (kSplitChunk / 16), m.counts, m.sizes, m.lines, m.outBases,
                 uint32_t(nBins), m.nCodes, m.nPlanes, m.zeroCode, dropUnmatched ? 1 : 0};
  const uint32_t small = smallBlocks(nChunks, cfg.numCUs);
  if (phases & 1) {
    // (no bitmap for k_gp_last to zero: the planes are zeroed here, all of them at once)
    hipError_t e = launchTextIndex(data, len, delim, m.misc, m.counts, m.bases, m.masks, m.open,
                                   nullptr, m.misc + 1, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (nChunks) {
      if (m.nPlanes) {
        e = hipMemsetAsync(m.planes, 0, size_t(m.nPlanes) * nChunks * (kSplitChunk / 8), stream);
        if (e != hipSuccess) return e;
      }
      const LineVerb v = lineVerb(d, cfg, doLeader, style);
#define RO_CALL(K) \
  REDGPU_LINE_VERB(launchRouteClassK, K, d, data, b, v.style, v.lead, r, cfg, stream)
      e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(RO_CALL) }();
#undef RO_CALL
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_ro_size, dim3(small), dim3(256), 0, stream, b, r);
      launchScan64(m.sizes, m.nCells, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_ro_finish, dim3(m.nCodes), dim3(256), 0, stream, r, nChunks, m.misc, nLines,
                       nRouted, binLines, binOffsets, outLen);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) {
    hipLaunchKernelGGL(k_ro_write, dim3(small), dim3(256), 0, stream, data, b, r, out,
                       outCap);
  }
  return hipGetLastError();
}
#endif  // REDGPU_TU_ROUTE_TEXT

#if REDGPU_TU_RANGE_TEXT
// sed's /open/,/close/ line ranges of a raw text (k_range_text.h): the line index (launchTextIndex),
// the class walk, the machine's carry (k_gp_open or k_split_scan), the k_rg_* passes around
// k_split_scan and k_misc.h's scan, and k_filter_text.h's write pass.  scratch:
// rangeTextScratchBytes(len) bytes, 16-byte aligned: three bitmaps (len / 8 each), and 64 bytes per
// chunk, 8 per 1,024 chunks and 72, rounded up to 16.
struct RangeScratch {
  uint64_t *bases, *open, *carry, *startBases, *emitBytes;  // [nChunks] each
  uint64_t *outBases;                                       // [nChunks + 1]
  uint64_t *partials;                                       // [nPart]
  // [8]: lines, the index scan's two spare words, ranges begun, a scan's spare word, events, the
  // state behind the last line, the position behind the last delimiter
  uint64_t *misc;
  uint32_t *counts, *events, *starts, *emitLines;  // [nChunks] each
  uint16_t *masks, *openBits, *closeBits;  // the delimiter bitmap, the two planes (open: then EMIT)
  uint64_t nPart, bytes;
  RangeScratch(void *scratch, uint64_t nChunks) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    carry = c.take<uint64_t>(nChunks);
    startBases = c.take<uint64_t>(nChunks);
    emitBytes = c.take<uint64_t>(nChunks);
    outBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    events = c.take<uint32_t>(nChunks);
    starts = c.take<uint32_t>(nChunks);
    emitLines = c.take<uint32_t>(nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    openBits = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    closeBits = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t rangeTextScratchBytes(uint64_t len) {
  return RangeScratch(nullptr, splitChunks(len)).bytes;
}

hipError_t launchRangeText(const DevDfa &d, int style, int doLeader, int32_t openResult,
                           int32_t closeResult, int emitOpen, int emitClose, int invert,
                           uint64_t maxRanges, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t *nLines, uint64_t *nRanges, uint64_t *nEmitted,
                           uint64_t *outLen, uint8_t *out, uint64_t outCap, uint64_t recCap,
                           uint64_t *firstLine, uint64_t *lastLine, uint64_t *begin, uint64_t *end,
                           int phases, void *scratch, const LaunchCfg &cfg, hipStream_t stream,
                           const char **kernelName) {
  *kernelName = "k_range_text";
  const uint64_t nChunks = splitChunks(len);
  const RangeScratch m(scratch, nChunks);
  const int toggle = openResult == closeResult;
  // (TextHits' verb bitmap is the open plane, which k_rg_mark turns into the EMIT bitmap)
  const GpBufs b{m.masks, m.openBits, m.bases, m.open, nullptr, nullptr, nChunks};
  const RgBufs r{m.openBits, m.closeBits, m.carry, m.events, m.starts, m.startBases, m.emitBytes,
                 m.emitLines, m.misc + 6, openResult, closeResult, toggle};
  const RgArgs a{emitOpen, emitClose, invert, maxRanges, recCap, firstLine, lastLine, begin, end};
  const uint32_t small = smallBlocks(nChunks, cfg.numCUs);
  if (phases & 1) {
    // (no bitmap for k_gp_last to zero: the planes are zeroed here, both at once)
    hipError_t e = launchTextIndex(data, len, delim, m.misc, m.counts, m.bases, m.masks, m.open,
                                   nullptr, m.misc + 1, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (nChunks) {
      e = hipMemsetAsync(m.openBits, 0, size_t(toggle ? 1 : 2) * nChunks * (kSplitChunk / 8), stream);
      if (e != hipSuccess) return e;
      const LineVerb v = lineVerb(d, cfg, doLeader, style);
#define RG_CALL(K) \
  REDGPU_LINE_VERB(launchRangeClassK, K, d, data, b, v.style, v.lead, r, cfg, stream)
      e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(RG_CALL) }();
#undef RG_CALL
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_rg_events, dim3(small), dim3(256), 0, stream, r, nChunks);
      if (toggle) {
        hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, m.events, nChunks, m.carry,
                           m.misc + 5, m.misc + 4, uint64_t(0));
      } else {
        hipLaunchKernelGGL(k_gp_open, dim3(1), dim3(1024), 0, stream, m.carry, nChunks);
      }
      hipLaunchKernelGGL(k_rg_starts, dim3(small), dim3(256), 0, stream, r, nChunks);
      hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(1024), 0, stream, m.starts, nChunks,
                         m.startBases, m.misc + 3, m.misc + 4, uint64_t(0));
      hipLaunchKernelGGL(k_rg_mark, dim3(small), dim3(256), 0, stream, b, r, a);
      launchScan64(m.emitBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_rg_totals, dim3(1), dim3(1024), 0, stream, r, a, nChunks,
                       nChunks ? m.outBases + nChunks : nullptr, m.misc + 3, m.misc, nLines, nRanges,
                       nEmitted, outLen);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) {
    hipLaunchKernelGGL(k_ft_write, dim3(small), dim3(256), 0, stream, data, b,
                       m.emitBytes, m.outBases, out, outCap);
  }
  return hipGetLastError();
}
#endif  // REDGPU_TU_RANGE_TEXT

#if REDGPU_TU_DEDUP_TEXT
// a raw text's lines chosen by their keys' strings (k_dedup_text.h): the line index (launchTextIndex),
// k_uq_zero, the one pass of k_dedup_text, k_dd_mark over the table, k_dd_emit, k_misc.h's scan,
// k_ft_totals and k_filter_text.h's write pass.  scratch: dedupTextScratchBytes(len, tableSlots)
// bytes, 16-byte aligned: 16 bytes per slot, three bitmaps (len / 8 each), 40 bytes per chunk, 8 per
// 1,024 chunks and 72, rounded up to 16.
struct DedupScratch {
  uint64_t *table;                    // [2 * slots]
  uint64_t *bases, *open, *emitBytes; // [nChunks] each
  uint64_t *outBases;                 // [nChunks + 1]
  uint64_t *partials;                 // [nPart]
  // [8]: lines, the index scan's two spare words, keyed, dropped, distinct, emitted, 1 spare
  uint64_t *misc;
  uint32_t *counts, *emitLines;       // [nChunks] each
  uint16_t *masks, *keyedBits, *markBits;  // the delimiter bitmap, KEYED, MARK (then EMIT)
  uint64_t nPart, bytes;
  DedupScratch(void *scratch, uint64_t nChunks, uint64_t slots) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    table = c.take<uint64_t>(2 * slots);
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    emitBytes = c.take<uint64_t>(nChunks);
    outBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    emitLines = c.take<uint32_t>(nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    keyedBits = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    markBits = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t dedupTextScratchBytes(uint64_t len, uint64_t tableSlots) {
  return DedupScratch(nullptr, splitChunks(len), tableSlots).bytes;
}

hipError_t launchDedupText(const DevDfa &d, int what, int style, int doLeader, uint64_t keyIndex,
                           uint64_t minCount, uint64_t maxCount, int invert, int keepUnkeyed,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t tableSlots,
                           int plain, uint64_t *nLines, uint64_t *nKeyed, uint64_t *nDistinct,
                           uint64_t *nDropped, uint64_t *nEmitted, uint64_t *outLen, uint8_t *out,
                           uint64_t outCap, int phases, void *scratch, const LaunchCfg &cfg,
                           hipStream_t stream, const char **kernelName) {
  *kernelName = "k_dedup_text";
  const uint64_t nChunks = splitChunks(len);
  const DedupScratch m(scratch, nChunks, tableSlots);
  // (TextHits' verb bitmap is MARK, which k_dd_emit turns into the EMIT bitmap)
  const GpBufs b{m.masks, m.markBits, m.bases, m.open, nullptr, nullptr, nChunks};
  const uint32_t small = smallBlocks(nChunks, cfg.numCUs);
  if (phases & 1) {
    // (no bitmap for k_gp_last to zero: KEYED and MARK are zeroed here, both at once)
    hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                   nullptr, m.misc, cfg.numCUs, stream);
    if (e != hipSuccess) return e;
    if (!nDistinct) nDistinct = m.misc + 5;
    UqOut o{reinterpret_cast<unsigned long long *>(m.table), tableSlots,
            reinterpret_cast<unsigned long long *>(nKeyed ? nKeyed : m.misc + 3),
            reinterpret_cast<unsigned long long *>(nDropped ? nDropped : m.misc + 4), 0};
    // (an empty text needs no table: the counters alone are zeroed)
    const uint64_t words = nChunks ? 2 * tableSlots : 0;
    const uint32_t zb = wordBlocks(words, cfg.numCUs);
    hipLaunchKernelGGL(k_uq_zero, dim3(zb ? zb : 1), dim3(256), 0, stream, o.table, words, o.nItems,
                       o.nDropped, nDistinct);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nChunks) {
      e = hipMemsetAsync(m.keyedBits, 0, size_t(2) * nChunks * (kSplitChunk / 8), stream);
      if (e != hipSuccess) return e;
      const LineVerb v = lineVerb(d, cfg, doLeader, style, what == REDGPU_DEDUP_LINES);
      // L: the front's slots, by k_uniq_text.h's rule: none for a text of 4 GiB and more (32-bit
      // counts) and under plain; WHOLE has the whole front, there is no table in front of it
      if (!plain && len < (1ull << 32))
        o.ldsSlots = what == REDGPU_DEDUP_WHOLE
                         ? kUqLdsSlots
                         : uniqLdsSlots(d.tableKind, d.tableBytes, d.nStates);
      uint32_t *keyed = reinterpret_cast<uint32_t *>(m.keyedBits);
#define DD_ARGS d, data, len, b, v.style, v.lead, keyIndex, o, keyed, cfg, stream
#define DD_CALL(K)                                                           \
  (what == REDGPU_DEDUP_MATCH   ? launchDedupK<K, kDdMatch>(DD_ARGS)         \
   : what == REDGPU_DEDUP_FIELD ? launchDedupK<K, kDdField>(DD_ARGS)         \
   : v.verb == kSearch          ? launchDedupK<K, kDdLines>(DD_ARGS)         \
                                : launchDedupK<K, kDdLinesMatch>(DD_ARGS))
      if (what == REDGPU_DEDUP_WHOLE) e = launchDedupK<REDGPU_TAB_GLOBAL_U32, kDdWhole>(DD_ARGS);
      else e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(DD_CALL) }();
#undef DD_CALL
#undef DD_ARGS
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_dd_mark, dim3(wordBlocks(tableSlots, cfg.numCUs)), dim3(256), 0, stream,
                         o.table, tableSlots, minCount, maxCount,
                         reinterpret_cast<const uint32_t *>(m.masks), nChunks * (kSplitChunk / 32),
                         reinterpret_cast<uint32_t *>(m.markBits),
                         reinterpret_cast<unsigned long long *>(nDistinct));
      hipLaunchKernelGGL(k_dd_emit, dim3(small), dim3(256), 0, stream, b, m.keyedBits, invert,
                         keepUnkeyed, m.emitBytes, m.emitLines);
      launchScan64(m.emitBytes, nChunks, m.partials, m.outBases, stream);
    }
    hipLaunchKernelGGL(k_ft_totals, dim3(1), dim3(1024), 0, stream, m.emitLines, nChunks,
                       nChunks ? m.outBases + nChunks : nullptr, outLen,
                       nEmitted ? nEmitted : m.misc + 6);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((phases & 2) && out && outCap && nChunks) {
    hipLaunchKernelGGL(k_ft_write, dim3(small), dim3(256), 0, stream, data, b, m.emitBytes,
                       m.outBases, out, outCap);
  }
  return hipGetLastError();
}
#endif  // REDGPU_TU_DEDUP_TEXT

#if REDGPU_TU_UNIQ_TEXT
// a raw text's distinct items counted by their bytes (k_uniq_text.h): the line index
// (launchTextIndex, which also zeroes the FIRST bitmap), k_uq_zero, the one pass of k_uniq_text, and
// the ordering pass around k_misc.h's scan.  scratch: uniqTextScratchBytes(len, tableSlots) bytes,
// 16-byte aligned: 16 bytes per slot, the two bitmaps (len / 4), 164 bytes per chunk, 8 per 1,024
// chunks and 72, rounded up to 16.
struct UniqScratch {
  uint64_t *table;          // [2 * slots]
  uint64_t *bases, *open;   // [nChunks] each
  uint64_t *pops;           // [nChunks]
  uint64_t *popBases;       // [nChunks + 1]
  uint64_t *partials;       // [nPart]
  uint64_t *misc;           // [8]: lines, the scan's two spare words, items, dropped, distinct, 2 spare
  uint32_t *counts;         // [nChunks]
  uint16_t *lanePre;        // [64 * nChunks]
  uint16_t *masks, *firsts; // the delimiter bitmap, the FIRST bitmap
  uint64_t nPart, bytes;
  UniqScratch(void *scratch, uint64_t nChunks, uint64_t slots) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    table = c.take<uint64_t>(2 * slots);
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    pops = c.take<uint64_t>(nChunks);
    popBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    lanePre = c.take<uint16_t>(64 * nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    firsts = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t uniqTextScratchBytes(uint64_t len, uint64_t tableSlots) {
  return UniqScratch(nullptr, splitChunks(len), tableSlots).bytes;
}

uint32_t uniqLdsSlots(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates) {
  const DevDfa d = ldsRoomDfa(tableKind, tableBytes, nStates);
#define UQ_SLOTS(K) uniqLdsSlotsK<K>(d)
  REDGPU_KIND_SWITCH(UQ_SLOTS)
#undef UQ_SLOTS
}

hipError_t launchUniqText(const DevDfa &d, int what, int style, int doLeader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t maxPerLine, uint64_t tableSlots,
                          uint64_t cap, int plain, uint64_t *nLines, uint64_t *nItems,
                          uint64_t *nDistinct, uint64_t *nDropped, uint64_t *first,
                          uint64_t *length, uint64_t *count, void *scratch, const LaunchCfg &cfg,
                          hipStream_t stream, const char **kernelName) {
  *kernelName = "k_uniq_text";
  const uint64_t nChunks = splitChunks(len);
  const UniqScratch m(scratch, nChunks, tableSlots);
  hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                 m.firsts, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  if (!nDistinct) nDistinct = m.misc + 5;
  UqOut o{reinterpret_cast<unsigned long long *>(m.table), tableSlots,
          reinterpret_cast<unsigned long long *>(nItems ? nItems : m.misc + 3),
          reinterpret_cast<unsigned long long *>(nDropped ? nDropped : m.misc + 4), 0};
  // (an empty text needs no table: the counters alone are zeroed)
  const uint64_t words = nChunks ? 2 * tableSlots : 0;
  const uint32_t zb = wordBlocks(words, cfg.numCUs);
  hipLaunchKernelGGL(k_uq_zero, dim3(zb ? zb : 1), dim3(256), 0, stream, o.table, words, o.nItems,
                     o.nDropped, nDistinct);
  e = hipGetLastError();
  if (e != hipSuccess || nChunks == 0) return e;
  const LineVerb v = lineVerb(d, cfg, doLeader, style, what == REDGPU_UNIQ_LINES);
  // L: the front's slots.  32-bit counts hold a text below 4 GiB whatever it is (k_tally_text.h:
  // tallyAdd); a longer text, and the plain form, go to the global table alone
  if (!plain && len < (1ull << 32)) o.ldsSlots = uniqLdsSlots(d.tableKind, d.tableBytes, d.nStates);
  const GpBufs b{m.masks, nullptr, m.bases, m.open, nullptr, nullptr, nChunks};
#define UQ_ARGS d, data, len, b, v.style, v.lead, maxPerLine, o, cfg, stream
#define UQ_CALL(K)                                                              \
  (what == REDGPU_UNIQ_MATCHES ? launchUniqK<K, kUqMatches>(UQ_ARGS)            \
   : v.verb == kSearch         ? launchUniqK<K, kUqLines>(UQ_ARGS)              \
                               : launchUniqK<K, kUqLinesMatch>(UQ_ARGS))
  e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(UQ_CALL) }();
#undef UQ_CALL
#undef UQ_ARGS
  if (e != hipSuccess) return e;
  // the grid of the passes over the table
  const uint32_t tb = wordBlocks(tableSlots, cfg.numCUs);
  hipLaunchKernelGGL(k_uq_mark, dim3(tb), dim3(256), 0, stream, o.table, tableSlots,
                     reinterpret_cast<uint32_t *>(m.firsts));
  hipLaunchKernelGGL(k_uq_pop, dim3(smallBlocks(nChunks, cfg.numCUs)), dim3(256), 0, stream,
                     m.firsts, nChunks, m.pops, m.lanePre);
  launchScan64(m.pops, nChunks, m.partials, m.popBases, stream);
  hipLaunchKernelGGL(k_uq_emit, dim3(tb), dim3(256), 0, stream, o.table, tableSlots,
                     reinterpret_cast<const uint32_t *>(m.firsts), m.popBases, m.lanePre, nChunks,
                     cap, first, length, count, nDistinct);
  return hipGetLastError();
}
#endif  // REDGPU_TU_UNIQ_TEXT

#if REDGPU_TU_GROUP_TEXT
// a raw text's lines grouped by their keys' strings (k_group_text.h): the line index (launchTextIndex,
// which also zeroes the FIRST bitmap), k_uq_zero, k_gr_zero, the one pass of k_group_text, and
// k_uniq_text.h's ordering pass with k_gr_emit at its end.  scratch: groupTextScratchBytes(len,
// tableSlots) bytes, 16-byte aligned: 16 + 32 bytes per slot, the two bitmaps (len / 4), 164 bytes
// per chunk, 8 per 1,024 chunks and 72, rounded up to 16.
struct GroupScratch {
  uint64_t *table;          // [2 * slots]
  uint64_t *side;           // [4][slots]: numeric count, sum, min, max
  uint64_t *bases, *open;   // [nChunks] each
  uint64_t *pops;           // [nChunks]
  uint64_t *popBases;       // [nChunks + 1]
  uint64_t *partials;       // [nPart]
  // [8]: lines, the scan's two spare words, keyed, dropped, distinct, numeric, 1 spare
  uint64_t *misc;
  uint32_t *counts;         // [nChunks]
  uint16_t *lanePre;        // [64 * nChunks]
  uint16_t *masks, *firsts; // the delimiter bitmap, the FIRST bitmap
  uint64_t nPart, bytes;
  GroupScratch(void *scratch, uint64_t nChunks, uint64_t slots) : nPart((nChunks + 1023) / 1024) {
    Carve c{static_cast<uint8_t *>(scratch)};
    table = c.take<uint64_t>(2 * slots);
    side = c.take<uint64_t>(4 * slots);
    bases = c.take<uint64_t>(nChunks);
    open = c.take<uint64_t>(nChunks);
    pops = c.take<uint64_t>(nChunks);
    popBases = c.take<uint64_t>(nChunks + 1);
    partials = c.take<uint64_t>(nPart);
    misc = c.take<uint64_t>(8);
    counts = c.take<uint32_t>(nChunks);
    lanePre = c.take<uint16_t>(64 * nChunks);
    c.align(16);
    masks = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    firsts = c.take<uint16_t>(nChunks * (kSplitChunk / 16));
    bytes = c.at;
  }
};

uint64_t groupTextScratchBytes(uint64_t len, uint64_t tableSlots) {
  return GroupScratch(nullptr, splitChunks(len), tableSlots).bytes;
}

uint32_t groupLdsSlots(uint32_t tableKind, uint32_t tableBytes, uint32_t nStates) {
  const DevDfa d = ldsRoomDfa(tableKind, tableBytes, nStates);
#define GR_SLOTS(K) groupLdsSlotsK<K>(d)
  REDGPU_KIND_SWITCH(GR_SLOTS)
#undef GR_SLOTS
}

hipError_t launchGroupText(const DevDfa &d, int what, uint64_t keyIndex, uint64_t valueIndex,
                           int which, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t tableSlots, uint64_t cap, int plain, uint64_t *nLines,
                           uint64_t *nKeyed, uint64_t *nNumeric, uint64_t *nDistinct,
                           uint64_t *nDropped, uint64_t *first, uint64_t *length, uint64_t *count,
                           uint64_t *stats, void *scratch, const LaunchCfg &cfg,
                           hipStream_t stream, const char **kernelName) {
  *kernelName = "k_group_text";
  const uint64_t nChunks = splitChunks(len);
  const GroupScratch m(scratch, nChunks, tableSlots);
  hipError_t e = launchTextIndex(data, len, delim, nLines, m.counts, m.bases, m.masks, m.open,
                                 m.firsts, m.misc, cfg.numCUs, stream);
  if (e != hipSuccess) return e;
  if (!nDistinct) nDistinct = m.misc + 5;
  GrOut o{reinterpret_cast<unsigned long long *>(m.table),
          reinterpret_cast<unsigned long long *>(m.side), tableSlots,
          reinterpret_cast<unsigned long long *>(nKeyed ? nKeyed : m.misc + 3),
          reinterpret_cast<unsigned long long *>(nDropped ? nDropped : m.misc + 4),
          reinterpret_cast<unsigned long long *>(nNumeric ? nNumeric : m.misc + 6), 0};
  // (an empty text needs no table: the counters alone are zeroed)
  const uint64_t words = nChunks ? 2 * tableSlots : 0;
  const uint32_t zb = wordBlocks(words, cfg.numCUs);
  hipLaunchKernelGGL(k_uq_zero, dim3(zb ? zb : 1), dim3(256), 0, stream, o.table, words, o.nKeyed,
                     o.nDropped, nDistinct);
  const uint64_t cells = nChunks ? tableSlots : 0;
  const uint32_t sb = wordBlocks(cells, cfg.numCUs);
  hipLaunchKernelGGL(k_gr_zero, dim3(sb ? sb : 1), dim3(256), 0, stream, o.side, cells, o.nNumeric);
  e = hipGetLastError();
  if (e != hipSuccess || nChunks == 0) return e;
  // L: the front's slots, by k_uniq_text.h's rule: none for a text of 4 GiB and more (32-bit counts)
  // and under plain
  if (!plain && len < (1ull << 32)) o.ldsSlots = groupLdsSlots(d.tableKind, d.tableBytes, d.nStates);
  const GpBufs b{m.masks, nullptr, m.bases, m.open, nullptr, nullptr, nChunks};
#define GR_ARGS d, data, len, b, keyIndex, valueIndex, which, o, cfg, stream
#define GR_CALL(K)                                                      \
  (what == REDGPU_GROUP_MATCH ? launchGroupK<K, kGrMatch>(GR_ARGS)      \
                              : launchGroupK<K, kGrField>(GR_ARGS))
  e = [&]() -> hipError_t { REDGPU_KIND_SWITCH(GR_CALL) }();
#undef GR_CALL
#undef GR_ARGS
  if (e != hipSuccess) return e;
  // the grid of the passes over the table
  const uint32_t tb = wordBlocks(tableSlots, cfg.numCUs);
  hipLaunchKernelGGL(k_uq_mark, dim3(tb), dim3(256), 0, stream, o.table, tableSlots,
                     reinterpret_cast<uint32_t *>(m.firsts));
  hipLaunchKernelGGL(k_uq_pop, dim3(smallBlocks(nChunks, cfg.numCUs)), dim3(256), 0, stream,
                     m.firsts, nChunks, m.pops, m.lanePre);
  launchScan64(m.pops, nChunks, m.partials, m.popBases, stream);
  hipLaunchKernelGGL(k_gr_emit, dim3(tb), dim3(256), 0, stream, o.table, o.side, tableSlots,
                     reinterpret_cast<const uint32_t *>(m.firsts), m.popBases, m.lanePre, nChunks,
                     cap, first, length, count, stats, nDistinct);
  return hipGetLastError();
}
#endif  // REDGPU_TU_GROUP_TEXT

#if REDGPU_TU_GENERIC
hipError_t launchBatches(const DevDfa &d, const Batch *bs, uint32_t nb, int verb, int style,
                         int doLeader, const LaunchCfg &cfg, hipStream_t stream,
                         const char **kernelName) {
  *kernelName = "none";
  int nverb = verb, nstyle = style;
  normalizeVerbStyle(d, cfg, doLeader && d.leaderLen > 0, nverb, nstyle);
  for (uint32_t k = 0; k < nb;) {
    if (bs[k].n == 0) { ++k; continue; }
    uint32_t taken = 0;
    hipError_t e = launchStreamBatches(d, bs + k, nb - k, nverb, nstyle, doLeader, cfg, stream,
                                       kernelName, &taken);
    if (e != hipSuccess) return e;
    if (!taken) {
      e = launchBatch(d, bs[k], verb, style, doLeader, cfg, stream, kernelName);
      if (e != hipSuccess) return e;
      taken = 1;
    }
    k += taken;
  }
  return hipSuccess;
}

hipError_t launchBatch(const DevDfa &d, const Batch &b, int verb, int style, int doLeader,
                       const LaunchCfg &cfg, hipStream_t stream, const char **kernelName) {
  if (b.n == 0) {
    *kernelName = "none";
    return hipSuccess;
  }
  const bool lead = doLeader && d.leaderLen > 0;
  normalizeVerbStyle(d, cfg, lead, verb, style);
  if (b.nDev) {
    // the line count is on the device: only the k_ragged family reads it there
    bool handled = false;
    hipError_t fe = launchRaggedFamily(d, b, verb, style, doLeader, cfg, stream, kernelName, &handled);
    return handled || fe != hipSuccess ? fe : hipErrorNotSupported;
  }
  // DFAs the visit model sees dying within 16 bytes (anchored patterns on arbitrary text) stay
  // with k_generic: the whole-line kernels below read and walk every byte, k_generic stops
  // where the reference's loop stops - measured on ERR 1.3x (64-byte lines) to 38x (4 KiB
  // lines) faster (scripts/bench_anchored.py).
  // match over an early-death DFA whose table lives in LDS: probe every line for a few bytes,
  // park the survivors, walk them densely (k_early)
  const bool earlyKind = d.tableKind == REDGPU_TAB_LDS_FUSED_U8 || d.tableKind == REDGPU_TAB_LDS_FUSED_U16 ||
                         d.tableKind == REDGPU_TAB_LDS_CLASS_U16 || d.tableKind == REDGPU_TAB_LDS_SPARSE;
  // (check with a leader consumes it and starts in the post-leader state: k_generic's checkLane)
  if ((verb == kMatch || (verb == kCheck && !lead)) && earlyKind && !cfg.forceGeneric &&
      b.n < (1ull << 32) && d.nStates <= 65535 &&
      size_t(d.tableBytes) + 512 + 16384 + 1024 <= size_t(160) * 1024 &&
      (cfg.forceEarly || (d.earlyDeath && !cfg.forceStream && b.n >= 16384))) {
    *kernelName = verb == kMatch ? "k_early<match>" : "k_early<check>";
    switch (d.tableKind) {
    case REDGPU_TAB_LDS_FUSED_U8: return launchEarlyK<REDGPU_TAB_LDS_FUSED_U8>(d, b, verb, style, lead, cfg, stream);
    case REDGPU_TAB_LDS_FUSED_U16: return launchEarlyK<REDGPU_TAB_LDS_FUSED_U16>(d, b, verb, style, lead, cfg, stream);
    case REDGPU_TAB_LDS_CLASS_U16: return launchEarlyK<REDGPU_TAB_LDS_CLASS_U16>(d, b, verb, style, lead, cfg, stream);
    default: return launchEarlyK<REDGPU_TAB_LDS_SPARSE>(d, b, verb, style, lead, cfg, stream);
    }
  }

  // check / match with an early-exit style, no leader, table in LDS: the block kernel
  // ... and the whole-line styles on a fixed stride that is not a multiple of 64 (100-byte
  // records, 250-byte lines: k_fixed / k_generic gave those a lane each at 1-1.7 TB/s)
  const bool oddStride = !b.offsets && b.stride >= 32 && b.stride % 64 != 0;
  if ((verb == kCheck || verb == kMatch) && !lead && !cfg.forceGeneric && !d.earlyDeath &&
      (style == kStyInstant || style == kStyFirst || style == kStyTangent ||
       ((style == kStyLast || style == kStyFull) && oddStride)) && b.n >= 4096) {
    bool taken = false;
    const bool pos = verb == kMatch && (b.start || b.end);
    hipError_t se = hipSuccess;
    switch (d.tableKind) {
    case REDGPU_TAB_LDS_FUSED_U8: se = launchStyleBlocksK<REDGPU_TAB_LDS_FUSED_U8>(d, b, style, pos, cfg, stream, &taken); break;
    case REDGPU_TAB_LDS_FUSED_U16: se = launchStyleBlocksK<REDGPU_TAB_LDS_FUSED_U16>(d, b, style, pos, cfg, stream, &taken); break;
    case REDGPU_TAB_LDS_CLASS_U16: se = launchStyleBlocksK<REDGPU_TAB_LDS_CLASS_U16>(d, b, style, pos, cfg, stream, &taken); break;
    case REDGPU_TAB_LDS_SPARSE: se = launchStyleBlocksK<REDGPU_TAB_LDS_SPARSE>(d, b, style, pos, cfg, stream, &taken); break;
    default: break;
    }
    if (se != hipSuccess) return se;
    if (taken) {
      *kernelName = verb == kMatch ? "k_style_blocks<match>" : "k_style_blocks<check>";
      return hipSuccess;
    }
  }

  {
    bool handled = false;
    hipError_t fe = launchFixedFamily(d, b, verb, style, doLeader, cfg, stream, kernelName, &handled);
    if (handled || fe != hipSuccess) return fe;
    fe = launchRaggedFamily(d, b, verb, style, doLeader, cfg, stream, kernelName, &handled);
    if (handled || fe != hipSuccess) return fe;
  }

  // (launchGeneric names the kernel it launches: k_scan_marked or k_generic)
#define GE_CALL(K) launchGeneric<K>(d, b, verb, style, lead, cfg, stream, kernelName)
  REDGPU_KIND_SWITCH(GE_CALL)
#undef GE_CALL
}

#endif  // REDGPU_TU_GENERIC

} // namespace redgpu
