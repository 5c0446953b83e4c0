/* redgpu.h - C-ABI of the MI355X-native DFA match-execution path for RED (zezax/one, quol/red).
 *
 * This is the drop-in boundary.  RED has no FFI layer of its own: the seam is the C++ value
 * type `Executable` (a validated serialized-DFA blob, include/Executable.h:28-76) and the free
 * functions `check / match / scan (const Executable&, const void* ptr, size_t len[, Style])`
 * (include/Matcher.h:79-98,133-169).  Every entry point below names the reference interface it
 * replaces; citations are relative to /root/reference/quol/red/.  The reference-side binding a
 * maintainer would add is shown in INTEGRATION.md; the C++ mirror of the reference's names is
 * include/redgpu.hpp.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns 0 (REDGPU_OK) or a negative code
 *     and leaves a message for redgpu_last_error() (thread-local).  The reference signals the
 *     same conditions with exceptions (include/Except.h:9-19): EAPI <-> RedExceptApi,
 *     EEXEC <-> RedExceptExec, ELIMIT <-> RedExceptLimit.  "No match" is result 0, not an error.
 *   - a redgpu_dfa is immutable after creation; all *_batch calls are re-entrant on a shared
 *     handle from any number of host threads (the reference's threading contract,
 *     doc/Performance.md:81-84, tools/thr_red.cpp:86-91).
 *   - inputs: line i is data[offsets[i], offsets[i+1]) when offsets != NULL (n+1 entries),
 *     else data[i*stride, (i+1)*stride).  Inputs/outputs are caller-owned and never retained.
 *     A single ragged line of 4 GiB or more: the host-buffer entry points route the batch to
 *     the general kernel (64-bit positions); through the _dev entry points such a batch must be
 *     created with REDGPU_F_FORCE_GENERIC (the block-wise kernels keep positions in 32 bits and
 *     cannot see the offsets before the launch).
 *     Device-pointer (_dev) entry points may read any byte of data[0, offsets[n]) (idle lanes
 *     re-read the first block), so the whole range must be device memory even when
 *     offsets[0] > 0; the host-buffer entry points copy only [offsets[0], offsets[n]).
 *   - outputs are the fields of the reference's Outcome (include/Outcome.h:32-35):
 *     result int32, start/end uint64 (size_t).  `start` and `end` may be NULL.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails
 *     with REDGPU_EHIP.
 */
#ifndef REDGPU_H
#define REDGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REDGPU_OK      0
#define REDGPU_EAPI   (-1) /* bad blob / bad arguments      (RedExceptApi)   */
#define REDGPU_EEXEC  (-2) /* unsupported format / style    (RedExceptExec)  */
#define REDGPU_ELIMIT (-3) /* capacity exceeded             (RedExceptLimit) */
#define REDGPU_EHIP   (-5) /* HIP runtime / device failure  (new)            */
#define REDGPU_ERCCL  (-6) /* RCCL unavailable or failed    (new, groups)    */

/* include/Matcher.h:67-74 */
#define REDGPU_STY_INSTANT 1
#define REDGPU_STY_FIRST   2
#define REDGPU_STY_TANGENT 3
#define REDGPU_STY_LAST    4
#define REDGPU_STY_FULL    5

#define REDGPU_DEVICE_CURRENT (-1) /* upload to the calling thread's current HIP device */
#define REDGPU_DEVICE_NONE    (-2) /* validate + repack on the host only (no HIP call);
                                      batch calls on such a handle fail with REDGPU_EAPI */

typedef struct redgpu_dfa redgpu_dfa;

typedef struct redgpu_opts {
  int32_t  device;        /* HIP device ordinal, or REDGPU_DEVICE_CURRENT / _NONE */
  uint32_t lds_table_max; /* 0 = default; cap (bytes) on the LDS-resident table */
  uint32_t flags;         /* REDGPU_F_* */
  uint32_t reserved[5];
} redgpu_opts;

#define REDGPU_F_FORCE_GENERIC 1u /* never pick the specialised fixed-stride kernels */
#define REDGPU_F_FORCE_GLOBAL  2u /* keep the transition table in HBM/L2 even if it fits LDS */
#define REDGPU_F_NO_BUCKETING  8u /* ragged fast path: walk lines in input order instead of
                                     bucketing them by length first (tests, tuning) */
#define REDGPU_F_FORCE_STREAM 16u /* whole-line streaming kernels even for a DFA flagged
                                     early_death (tests, tuning) */
#define REDGPU_F_NO_CHUNKING  32u /* never cut long lines into speculatively walked chunks */
#define REDGPU_F_FORCE_CHUNKING 64u /* ... or always, whatever the DFA looks like (tests) */
#define REDGPU_F_STREAM_CHAINS_2 128u /* fixed-stride hot path: always the two-chain kernel ... */
#define REDGPU_F_STREAM_CHAINS_4 256u /* ... or always the four-chain one, whatever the batch size
                                         (default: by batch size; tests, tuning) */
#define REDGPU_F_FORCE_EARLY 512u /* match: the probe-and-drain kernel of the early-death DFAs for any
                                    LDS-resident table and any batch size (tests, tuning) */
#define REDGPU_F_FORCE_LEAN 1024u /* fixed-stride lines of 512 bytes and more: the deferred-bookkeeping
                                     step (k_stream_lean.h: 2.75 VALU per byte instead of 6, the two
                                     pieces that hold a line's last accept and last start re-walked at
                                     its end) instead of the exact one.  Built because the exact step
                                     looked issue-bound; measured it is not - 4 KiB lines +2 % (URI-D)
                                     / -3 % (SYN-256), 512-byte lines -8 % - so it is opt-in */
#define REDGPU_F_LEAN_CHAINS_4 2048u /* ... with four lines per lane (two chain groups, counted
                                     waits) instead of two */
#define REDGPU_F_FORCE_PIECES 4096u /* ragged lines: huge lines are walked in pieces (k_ragged.h) even
                                     when the DFA is not flagged `forgetful` - the entry-state
                                     guesses are then mostly wrong and the pieces walked again
                                     one by one: correct, slow (tests) */
#define REDGPU_F_FORCE_HOT     4u /* a table too big for LDS always gets hot rows in LDS, even
                                     when the visit model finds no locality (tests, tuning) */

/* table placements reported by redgpu_dfa_info */
#define REDGPU_TAB_LDS_FUSED_U8   1 /* [state][byte] -> next state, u8,  in LDS */
#define REDGPU_TAB_LDS_FUSED_U16  2 /* [state][byte] -> next state, u16, in LDS */
#define REDGPU_TAB_LDS_CLASS_U16  3 /* [state][class] u16 + equivalence map, both in LDS */
#define REDGPU_TAB_GLOBAL_U16     4 /* [state][class] u16 in HBM/L2, equivalence map in LDS */
#define REDGPU_TAB_GLOBAL_U32     5 /* [state][class] u32 in HBM/L2, equivalence map in LDS */
#define REDGPU_TAB_HOT_ROWS       6 /* [state][class] u16 in HBM/L2 for every state, plus a 64 KB
                                       [hot index][byte] u8 table in LDS over the n_hot (<= 254)
                                       most-visited states (device states [hot_lo, hot_lo +
                                       n_hot)): entry = hot index of the target, 255 = the
                                       target is not hot (look it up in the class table) */
#define REDGPU_TAB_LDS_SPARSE     7 /* class table too big for LDS but sparse (signature sets:
                                       94 % of LOG-100's transitions lead to the dead state):
                                       row-displacement ("comb") form in LDS - base[state] u16,
                                       then u32 slots (owner state << 16 | target) at
                                       base + class; a slot owned by another state means the
                                       DFA's most common target */

typedef struct redgpu_info {
  uint32_t format;        /* 1, 2, 4: FileHeader.format_ (include/Serializer.h:34-40,47) */
  uint32_t n_classes;     /* maxChar_ + 1 */
  uint32_t leader_len;
  uint32_t states_total;  /* FileHeader.stateCnt_ */
  uint32_t states_used;   /* reachable from the initial state (what the device image holds) */
  uint32_t n_pure_dead;   /* device states [0, n_pure_dead) are pure dead ends (Proxy.h:139) */
  uint32_t first_accept;  /* device states [first_accept, states_used) have result > 0 */
  uint32_t table_kind;    /* REDGPU_TAB_* */
  uint64_t table_bytes;
  int32_t  max_result;
  int32_t  device;
  uint32_t checksum;      /* FileHeader.checksum_ */
  uint32_t fast_path;     /* 1 if the fixed-stride specialised kernels apply to this DFA */
  uint32_t n_hot;         /* REDGPU_TAB_HOT_ROWS: rows resident in LDS (else 0) */
  uint32_t hot_lo;        /* REDGPU_TAB_HOT_ROWS: first device state with an LDS row */
  uint32_t hot_coverage_ppm; /* REDGPU_TAB_HOT_ROWS: share of the modelled visits (random-byte
                             walk from the initial state) that land on LDS rows, per million */
  uint32_t early_death;   /* 1 if the same model sees most walks reach a pure dead end within 16
                             bytes (an anchored DFA on arbitrary text): such DFAs keep the
                             early-exit kernels */
  uint32_t forgetful;     /* 1 if the model's walk is back in the initial state >= 70 % of the
                             time: long lines may be cut into speculatively walked chunks */
  uint32_t image_refs;    /* handles currently sharing this handle's device image (the loader
                             cache: same blob + device + build options -> one repack, one upload) */
  uint32_t suffix_closed; /* 1 if the DFA accepts behind any prefix whatever it accepts (L = SIGMA* L:
                             patterns added with a loose start).  scan / search / collect then stop at
                             the first attempt that reaches the end of the line without accepting -
                             no later start position can accept; the reference walks them all
                             (include/Matcher.h:511-553, :575-621) to the same result */
} redgpu_info;

/* Replaces checkHeader (include/Serializer.h:109, lib/Serializer.cpp:270-298): returns
 * REDGPU_OK, or REDGPU_EAPI with *msg (if msg != NULL) pointing at a static string that is
 * byte-for-byte the reference's message. */
int redgpu_reda_check(const void *reda, size_t len, const char **msg);

/* Loader cache (cf. the reference's load path lib/Serializer.cpp:257-267, which
 * builds a fresh Executable per call): handles created from byte-identical blobs on the same
 * device with the same lds_table_max and FORCE_GLOBAL / FORCE_HOT flags share one validated
 * copy, one repacked image and one set of device tables (redgpu_info.image_refs counts them);
 * the image is released with its last handle.  redgpu_dfa_tune detaches the tuned handle. */

/* Replaces Executable(gCopyTag, string_view) + Executable::validate
 * (include/Executable.h:37, lib/Executable.cpp:53-70,159-170): validates exactly as
 * checkHeader does, additionally bounds-checks every row offset (the GPU must never chase a
 * corrupt pointer), COPIES the blob, repacks it and uploads the image to opts->device.
 * opts == NULL means {REDGPU_DEVICE_CURRENT, 0, 0}.  The caller's buffer may be freed or
 * scrambled immediately (test/red.cpp:55-78). */
int redgpu_dfa_create(const void *reda, size_t len, const redgpu_opts *opts, redgpu_dfa **out);

/* Replaces ~Executable (lib/Executable.cpp:127-139). */
void redgpu_dfa_destroy(redgpu_dfa *dfa);

/* Replaces the Executable accessors (include/Executable.h:52-60). */
int redgpu_dfa_info(const redgpu_dfa *dfa, redgpu_info *out);

/* No counterpart in the reference - there the table lives in CPU caches, which adapt to the
 * input on their own.  For a DFA placed as REDGPU_TAB_HOT_ROWS this is the explicit version:
 * walks a SAMPLE of real input (anchored, as match<styLast,false> does: include/Matcher.h:413-495)
 * counting visits per state, then re-ranks the hot rows by those counts and rebuilds and
 * re-uploads the image.  Results never change, only which transitions are served from LDS.
 * Not re-entrant: call it before the handle is shared between threads; it waits for all work
 * queued on the device.  State tokens of redgpu_advance_batch taken before the call are
 * invalid after it.  Other placements: validates its arguments and does nothing. */
int redgpu_dfa_tune(redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                    uint64_t stride, uint64_t n);
int redgpu_dfa_tune_dev(redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                        uint64_t stride, uint64_t n, void *stream);

/* Replaces Executable::serialized() (include/Executable.h:50): the handle's own copy. */
int redgpu_dfa_serialized(const redgpu_dfa *dfa, const void **reda, size_t *len);

/* ---- batch verbs over HOST buffers (allocates device staging, copies in and out) ---------
 * Each replaces the caller's per-input loop (tools/bench.cpp:60-71, tools/thr_red.cpp:36-47)
 * around one reference function:
 *   redgpu_check_batch <-> check<style,doLeader>(exec, ptr, len)  include/Matcher.h:133-134,363-410
 *   redgpu_match_batch <-> match<style,doLeader>(exec, ptr, len)  include/Matcher.h:146-147,413-495
 *                          (style 4 = styLast is the "matchLong" of BASELINE.json)
 *   redgpu_scan_batch  <-> scan<style,doLeader>(exec, ptr, len)   include/Matcher.h:159-160,498-554
 * The run-time-style overloads of the reference (Matcher.h:79-92, Matcher.cpp:53-67) are these
 * with do_leader = 1.
 * Lines: offsets == NULL -> line i = data[i*stride, (i+1)*stride).  offsets != NULL (n + 1
 * entries) -> line i = data[offsets[i], offsets[i+1] - stride): here `stride` is the number of
 * trailing bytes each line carries that the matcher must not see - 0 normally, 1 for the
 * delimiter-terminated lines redgpu_split_lines produces. */
int redgpu_check_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result);
int redgpu_match_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                       uint64_t *start, uint64_t *end);
int redgpu_scan_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                      const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result);
/*   redgpu_search_batch <-> search<style,doLeader>(exec, ptr, len) include/Matcher.h:172-173,557-640
 *                           (scan with positions; the first of SURVEY 8(f)'s "next" rows) */
int redgpu_search_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                        const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                        uint64_t *start, uint64_t *end);

/*   redgpu_collect_batch <-> Red::collect(string_view, vector<Outcome>&)  include/Red.h:115,
 *                            lib/Red.cpp:103-116: every non-overlapping match of each line, in
 *                            order (repeated search<styLast,false>).  Line i's records go to
 *                            result/start/end[i*cap .. i*cap+cap); counts[i] = matches FOUND,
 *                            which may exceed cap (then only the first cap are stored). */
int redgpu_collect_batch(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                         uint64_t stride, uint64_t n, uint64_t cap, uint64_t *counts,
                         int32_t *result, uint64_t *start, uint64_t *end);

/*   redgpu_collect_long <-> Red::collect(string_view, vector<Outcome>&)  include/Red.h:115,
 *                           lib/Red.cpp:103-116, over ONE long text, chunk-parallel across the
 *                           device (redgpu_collect_batch walks a line per lane: a single text is
 *                           one lane).  Positions are absolute in the text.  *count = matches
 *                           FOUND, which may exceed cap (then only the first cap records are
 *                           stored: redgpu_collect_batch's rule); start and end may be NULL.
 *                           chunk_bytes = 0 sizes the chunks automatically; non-zero forces the
 *                           chunk size (for tests: many chunk borders in a small text).  The
 *                           records are exactly Red::collect's whatever the chunk size.  The
 *                           host form uploads the whole text once (the chain of matches crosses
 *                           all of it): texts larger than device memory are not streamed.
 *                           redgpu_last_kernel() names the route: "k_collect_long" (chunks),
 *                           "k_collect_long<closed>" (suffix-closed DFAs without a pure dead
 *                           state: one attempt covers the text) or "k_collect" (one lane: short
 *                           texts, DFAs whose attempts cannot end early, cap = 0 on a closed
 *                           DFA).  Record slots at or past *count may be overwritten. */
int redgpu_collect_long(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                        uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                        uint64_t *start, uint64_t *end);

/*   redgpu_match_all_batch <-> matchAll(exec, string_view, vector<Outcome>&)  include/Matcher.h:127,
 *                              lib/Matcher.cpp:97-102, core include/Matcher.h:711-766 (also
 *                              Red::allMatches, lib/Red.cpp:713-715): ONE anchored walk per line
 *                              reporting every maximal run of bytes with the same accepted result
 *                              (RE2::Set::Match style).  The reference's public entry always
 *                              runs with doLeader = true: pass do_leader = 1 for parity with it.
 *                              Record layout and counts[] exactly as redgpu_collect_batch.
 *                              redgpu_last_kernel() names the kernel launched: "k_matchall" (a
 *                              test per byte: tables outside LDS, REDGPU_F_FORCE_GENERIC, a pure
 *                              dead end with a way out) or the block-wise form,
 *                              "k_matchall_blocks<1024,1>", "k_matchall_blocks<512,1>" (at most
 *                              256 states, one staged byte per position),
 *                              "k_matchall_blocks<1024,2>" or "k_matchall_blocks<512,2>" (two);
 *                              1024 or 512 threads, whichever keeps more lanes on a CU. */
int redgpu_match_all_batch(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t cap,
                           uint64_t *counts, int32_t *result, uint64_t *start, uint64_t *end);

/*   redgpu_match_all_long <-> matchAll(exec, string_view, vector<Outcome>&)  include/Matcher.h:127,
 *                             lib/Matcher.cpp:97-102, core include/Matcher.h:711-766, over ONE long
 *                             text, chunk-parallel across the device (redgpu_match_all_batch walks
 *                             a line per lane: a single text is one lane).  Positions are absolute
 *                             in the text.  *count = records FOUND, which may exceed cap; the first
 *                             min(*count, cap) records are stored complete (record cap-1 with its
 *                             final end); start and end may be NULL, result only when cap = 0.
 *                             do_leader as in redgpu_match_all_batch (1 = the reference's entry).
 *                             chunk_bytes = 0 sizes the chunks automatically; non-zero forces the
 *                             chunk size (for tests).  The records are exactly matchAll's whatever
 *                             the chunk size.  The host form uploads the whole text once.
 *                             redgpu_last_kernel() names the route: "k_match_all_long" (chunks) or
 *                             "k_matchall" (one lane: the empty text, texts under 16 KiB at the
 *                             automatic size, DFAs with a pure dead end that has a way out).
 *                             Record slots at or past *count may be overwritten. */
int redgpu_match_all_long(const redgpu_dfa *dfa, int do_leader, const uint8_t *data, uint64_t len,
                          uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                          uint64_t *start, uint64_t *end);

/*   redgpu_advance_batch <-> StatefulMatcher (include/Matcher.h:770-792, lib/Matcher.cpp:106-158),
 *                            n independent matchers advanced by one CHUNK each: state[i] is
 *                            matcher i's state_ on entry and on return (an opaque token, valid
 *                            only with the handle that produced it; REDGPU_STATE_INITIAL = a
 *                            freshly constructed StatefulMatcher - a buffer memset to 0xff is n
 *                            fresh matchers), result[i] = result() after the chunk's last byte.
 *                            Feeding a stream in chunks of any sizes gives the same states and
 *                            results as advance() byte by byte: inputs larger than device memory
 *                            are walked chunk by chunk. */
#define REDGPU_STATE_INITIAL 0xffffffffu
int redgpu_advance_batch(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                         uint64_t stride, uint64_t n, uint32_t *state, int32_t *result);

/*   redgpu_replace_batch <-> replace<style,doLeader>(exec, ptr, len, repl, out, max)
 *                            include/Matcher.h:186-191, core :643-706 (run-time-style overloads:
 *                            do_leader = 1, lib/Matcher.cpp:72-92): every line rewritten with each
 *                            match replaced by `repl`, at most max_count replacements per line.
 *                            counts[i] = replacements made in line i (the function's return
 *                            value); out_offsets[n + 1] = exclusive scan of the rewritten lengths
 *                            (out_offsets[n] = total bytes); line i's result is
 *                            out[out_offsets[i] .. out_offsets[i + 1]).  out may be NULL (sizes
 *                            only); with out != NULL every line that fits entirely below out_cap
 *                            is written - check out_offsets[n] <= out_cap, else call again with
 *                            a buffer of out_offsets[n] bytes. */
int redgpu_replace_batch(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                         const uint64_t *offsets, uint64_t stride, uint64_t n, const uint8_t *repl,
                         uint64_t repl_len, uint64_t max_count, uint64_t *counts,
                         uint64_t *out_offsets, uint8_t *out, uint64_t out_cap);

/*   redgpu_replace_long <-> replace<style,doLeader>(exec, ptr, len, repl, out, max)
 *                           include/Matcher.h:186-191, core :643-706, which Red's twenty
 *                           replaceOne* / replaceAll* and Red::replace end in (include/Red.h:
 *                           139-238), over ONE long text, chunk-parallel across the device
 *                           (redgpu_replace_batch walks a line per lane: a single text is one
 *                           lane).  *count = replaceCore's return value, *out_len = the size of
 *                           its `out` string; both are always written.  out may be NULL (sizes
 *                           only); with out != NULL the first min(*out_len, out_cap) bytes of the
 *                           rewritten text are written (redgpu_collect_long's "first cap records"
 *                           rule applied to bytes; bytes at or past *out_len may be overwritten,
 *                           up to out_cap).  out must not overlap data.  max_count is
 *                           replaceCore's `max`: only the first max_count matches in chain order
 *                           are replaced, everything behind them is copied (0 copies the text;
 *                           Red's replaceOne* is max_count = 1).  style is any of the five;
 *                           do_leader as in redgpu_replace_batch.  chunk_bytes as in
 *                           redgpu_collect_long (0 = automatic, non-zero forces it, for tests).
 *                           The output is exactly the reference's whatever the chunk size.
 *                           redgpu_last_kernel() names the route: "k_replace_long" (chunks) or
 *                           "k_replace_long<one>" (one chunk, so one lane runs the chain in
 *                           order: short texts, and DFAs without a pure dead state under
 *                           styLast / styFull, whose failing attempts cannot end early); both
 *                           assemble the output with the same tile-parallel copy.  The host form
 *                           uploads the text once, sizes the device output from the first phase's
 *                           *out_len and downloads min(*out_len, out_cap) bytes. */
int redgpu_replace_long(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                        uint64_t len, uint32_t chunk_bytes, const uint8_t *repl, uint64_t repl_len,
                        uint64_t max_count, uint64_t *count, uint64_t *out_len, uint8_t *out,
                        uint64_t out_cap);

/*   redgpu_search_long <-> search<style,doLeader>(exec, ptr, len)  include/Matcher.h:172-173, core
 *                          :557-640, which Red::searchInstant ... Red::searchFull, Red::partialMatch
 *                          and findAndConsume end in, over ONE long text, chunk-parallel across the
 *                          device (redgpu_search_batch walks a line per lane: a single text is one
 *                          lane).  *result, *start, *end = the fields of that Outcome: the match of
 *                          the lowest start position whose attempt succeeds, 0 / 0 / 0 when there
 *                          is none, searchCore's own answer on an empty text.  result is required;
 *                          start and end may be NULL (result only: scan's use).  style is any of
 *                          the five; do_leader as in redgpu_search_batch.  chunk_bytes as in
 *                          redgpu_collect_long (0 = automatic, non-zero forces it, for tests).
 *                          The Outcome is exactly the reference's whatever the chunk size.  A
 *                          match near the front ends the call early: chunks are handed out in
 *                          text order and dropped once a lower position has matched.
 *                          redgpu_last_kernel() names the route: "k_search_long" (chunks) or
 *                          "k_search_long<one>" (the batch kernels over a batch of one: the empty
 *                          text, texts under 16 KiB, DFAs without a pure dead state under styLast
 *                          / styFull, whose failing attempts cannot end early, and suffix-closed
 *                          DFAs without the leader, whose search is one anchored walk).  The host
 *                          form uploads the text once and downloads the three values. */
int redgpu_search_long(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                       uint64_t len, uint32_t chunk_bytes, int32_t *result, uint64_t *start,
                       uint64_t *end);

/* ---- the same verbs over DEVICE-resident buffers, asynchronous on `stream` ---------------
 * data/offsets/result/start/end are device pointers on the handle's device; `stream` is a
 * hipStream_t (NULL = the default stream).  Nothing is copied or synchronised; the only
 * allocation is the scratch some launches need (the ragged kernels' tail pad, their list of long
 * lines and the records of huge lines walked in pieces - up to ~16 bytes per line of the batch -,
 * the chunked walk's records, replace's partial sums, line splitting's delimiter masks - 1/8 of
 * the text): kept per HOST THREAD and (device, stream)
 * and re-used by that thread's later calls on the stream - so any number of threads may issue
 * _dev calls on one stream, the default one included - (re)allocated, with a device
 * synchronisation, only when a call needs more than the cached buffer holds; freed when the
 * thread exits or calls redgpu_thread_release(). */
int redgpu_check_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n,
                           int32_t *result, void *stream);
int redgpu_match_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n,
                           int32_t *result, uint64_t *start, uint64_t *end, void *stream);
int redgpu_scan_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          const uint64_t *offsets, uint64_t stride, uint64_t n, int32_t *result,
                          void *stream);
int redgpu_search_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                            const uint64_t *offsets, uint64_t stride, uint64_t n,
                            int32_t *result, uint64_t *start, uint64_t *end, void *stream);

/* ---- several device-resident batches per call ----------------------------------------------
 * The reference's callers hold many inputs and loop over them (tools/bench.cpp:60-71: every
 * line of the file, `iters` times; tools/thr_red.cpp:36-47).  A caller that holds K buffers of
 * lines hands all K over at once:
 *   redgpu_check_batches_dev <-> for each batch: check<style,doLeader> per line, Matcher.h:363-410
 *   redgpu_match_batches_dev <-> for each batch: match<style,doLeader> per line, Matcher.h:413-495
 * The results are exactly those of n_batches calls of the single-batch entry point in the order
 * given, on `stream` (a batch may read what an earlier one wrote only through the single-batch
 * calls: the batches of ONE call must not alias each other's outputs).  What the call buys: runs
 * of consecutive batches that the streaming kernel takes - fixed stride, the same for all, a
 * multiple of 64 bytes; styLast / styFull; the same outputs asked for (start NULL in all or in
 * none) - go out as ONE launch per 32 batches in which the DFA table is staged once per CU and
 * tiles of lines are handed out across batch boundaries, so the head and tail a 64 MiB launch
 * pays (a third of it) are paid once per call.  Anything else in the list runs as its own launch,
 * as redgpu_*_batch_dev would run it.  start / end of redgpu_batch are ignored by check. */
typedef struct redgpu_batch {
  const uint8_t  *data;
  const uint64_t *offsets; /* n + 1 entries, or NULL: fixed stride */
  uint64_t stride;
  uint64_t n;
  int32_t  *result;
  uint64_t *start;         /* may be NULL */
  uint64_t *end;           /* may be NULL */
} redgpu_batch;
int redgpu_check_batches_dev(const redgpu_dfa *dfa, int style, int do_leader,
                             const redgpu_batch *batches, uint32_t n_batches, void *stream);
int redgpu_match_batches_dev(const redgpu_dfa *dfa, int style, int do_leader,
                             const redgpu_batch *batches, uint32_t n_batches, void *stream);

int redgpu_collect_batch_dev(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                             uint64_t stride, uint64_t n, uint64_t cap, uint64_t *counts,
                             int32_t *result, uint64_t *start, uint64_t *end, void *stream);

/* device pointers (count too), asynchronous on stream; nothing is read back to the host */
int redgpu_collect_long_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len,
                            uint32_t chunk_bytes, uint64_t cap, uint64_t *count, int32_t *result,
                            uint64_t *start, uint64_t *end, void *stream);

int redgpu_match_all_batch_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                               const uint64_t *offsets, uint64_t stride, uint64_t n,
                               uint64_t cap, uint64_t *counts, int32_t *result, uint64_t *start,
                               uint64_t *end, void *stream);

/* device pointers (count too), asynchronous on stream; nothing is read back to the host */
int redgpu_match_all_long_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                              uint64_t len, uint32_t chunk_bytes, uint64_t cap, uint64_t *count,
                              int32_t *result, uint64_t *start, uint64_t *end, void *stream);

int redgpu_advance_batch_dev(const redgpu_dfa *dfa, const uint8_t *data, const uint64_t *offsets,
                             uint64_t stride, uint64_t n, uint32_t *state, int32_t *result,
                             void *stream);

/* every pointer is device memory, count and out_len too; asynchronous on stream; nothing is
 * read back to the host */
int redgpu_replace_long_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                            uint64_t len, uint32_t chunk_bytes, const uint8_t *repl,
                            uint64_t repl_len, uint64_t max_count, uint64_t *count,
                            uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream);

/* every pointer is device memory, result, start and end too; asynchronous on stream; nothing is
 * read back to the host */
int redgpu_search_long_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                           uint64_t len, uint32_t chunk_bytes, int32_t *result, uint64_t *start,
                           uint64_t *end, void *stream);

/* repl is device memory too */
int redgpu_replace_batch_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                             const uint64_t *offsets, uint64_t stride, uint64_t n,
                             const uint8_t *repl, uint64_t repl_len, uint64_t max_count,
                             uint64_t *counts, uint64_t *out_offsets, uint8_t *out,
                             uint64_t out_cap, void *stream);

/* The step BEFORE the path, on the device (the reference does it on the host:
 * lib/Util.cpp:109-130 sampleLines, and every tool that walks a text blob line by line): finds
 * the delimiters of a raw text buffer and writes the offsets[] array the ragged verbs take.
 * A line is [start, delimiter); the next starts after the delimiter; bytes after the last
 * delimiter are not a line (sampleLines' rule).  offsets[0] = 0 and offsets[k+1] = position
 * just past the k-th delimiter, so line k = [offsets[k], offsets[k+1]) INCLUDES its delimiter:
 * pass these offsets to the *_batch verbs with stride = 1 ("one trailing byte per line that the
 * matcher must not see").  cap = lines offsets[] has room for (cap + 1 entries); *n_lines =
 * delimiters FOUND, which may exceed cap (then only the first cap lines are stored).
 * _dev: everything device-resident (n_lines too), asynchronous on `stream`. */
int redgpu_split_lines(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                       uint64_t *offsets, uint64_t cap, uint64_t *n_lines);
int redgpu_split_lines_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t *offsets, uint64_t cap, uint64_t *n_lines, void *stream);

/* Raw text in, one Outcome per line out, in ONE call: the loop of tools/skim_red.cpp:36-46 over
 * the lines lib/Util.cpp:109-130 cuts (find the delimiter, hand [start, delimiter) to the
 * matcher, go on behind it).  Equal to redgpu_split_lines[_dev] followed by
 * redgpu_check/match_batch[_dev] over (offsets, stride = 1) - same offsets[] (cap + 1 entries, the
 * caller's: positions are relative to a line's start, so the caller needs them to place a match
 * in the buffer), same *n_lines (delimiters found, may exceed cap), result/start/end filled for
 * the first min(*n_lines, cap) lines - but the line count never visits the host in between:
 * for the DFAs the ragged streaming kernels take (styles Last / Full, no leader to honour, table
 * in LDS or hot rows - redgpu_last_kernel says "k_ragged...") the walk reads it on the device and
 * the _dev call is asynchronous on `stream` from end to end; for the others the call waits for
 * the split once (8 bytes back) and launches what redgpu_*_batch_dev would.
 * _dev: all pointers device memory.  redgpu_match_text: host buffers; start / end may be NULL
 * (both NULL = check). */
int redgpu_check_text_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                          uint64_t *n_lines, int32_t *result, void *stream);
int redgpu_match_text_dev(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                          uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                          uint64_t *n_lines, int32_t *result, uint64_t *start, uint64_t *end,
                          void *stream);
int redgpu_match_text(const redgpu_dfa *dfa, int style, int do_leader, const uint8_t *data,
                      uint64_t len, uint8_t delim, uint64_t *offsets, uint64_t cap,
                      uint64_t *n_lines, int32_t *result, uint64_t *start, uint64_t *end);

/* grep: raw text in, only the lines that match out - include/Red.h:65 names the use
 * ("searchInstant() - appropriate for grep"), tools/skim_red.cpp:36-46 is its loop: the lines
 * lib/Util.cpp:109-130 cuts, each handed to search<style,doLeader> (include/Matcher.h:172-173,
 * core 557-640).
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter are not a line.
 *  - Line k is selected iff (search<style,do_leader>(line k).result_ > 0) != (invert != 0)
 *    (invert = grep -v).  The verb goes through the identities every batch launch applies first;
 *    for every DFA the Outcome is exactly what redgpu_search_batch gives for that line.
 *  - The selected lines are reported in text order, as record j of line / begin / finish /
 *    result / start / end: line[j] = the 0-based index of the line, begin[j] = the offset of its
 *    first byte in data, finish[j] = the offset of its delimiter, result/start/end[j] = the
 *    Outcome of search on that line alone, positions relative to begin[j] (redgpu_match_text's
 *    convention); under invert the Outcome of a selected line is (0, 0, 0).
 *  - *n_selected = min(selected lines, max_count) (max_count = grep -m); it may exceed cap, and
 *    then only the first cap records are stored.  *n_lines = delimiters found.
 *  - Every array pointer and n_lines may be NULL, each on its own; all arrays NULL, or cap == 0,
 *    gives the count only (grep -c), and no line is walked twice.
 *  - REDGPU_EAPI for a NULL n_selected or a NULL data with len > 0 (checked before the handle's
 *    device is looked at), REDGPU_EEXEC for a style that does not exist, REDGPU_ELIMIT for a
 *    text redgpu_split_lines refuses.
 *  - An empty text, or one without a delimiter: *n_lines = 0 and *n_selected = 0 (the _dev form
 *    writes them on the stream).
 * redgpu_last_kernel() says "k_grep_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - no count is read
 * back, and no per-line array is needed from the caller or in scratch (the lines are driven from
 * the split's delimiter bitmap; scratch is len / 4 + 32 bytes per 16 KiB of text).
 * redgpu_grep_text: host buffers - one upload of the text, then n_lines, n_selected and the
 * filled prefixes back. */
int redgpu_grep_text(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                     const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_count,
                     uint64_t cap, uint64_t *n_lines, uint64_t *n_selected, uint64_t *line,
                     uint64_t *begin, uint64_t *finish, int32_t *result, uint64_t *start,
                     uint64_t *end);
int redgpu_grep_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                         const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_count,
                         uint64_t cap, uint64_t *n_lines, uint64_t *n_selected, uint64_t *line,
                         uint64_t *begin, uint64_t *finish, int32_t *result, uint64_t *start,
                         uint64_t *end, void *stream);

/* grep -o: raw text in, every match of every line out - Red::collect (lib/Red.cpp:103-116) inside
 * the line loop of tools/skim_red.cpp:36-46, over the lines lib/Util.cpp:109-130 cuts.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter are not a line (a match in them is not reported).
 *  - The records are, for line k = 0, 1, ... in order, the Outcomes of Red::collect on that line
 *    alone, in order: repeated search<styLast,false> (include/Matcher.h:557-640) from the end of
 *    the previous match - exactly what redgpu_collect_batch gives for that line with an unbounded
 *    cap.  Record j is line[j] = k, begin[j] = the offset in data of the line's first byte,
 *    result[j], start[j], end[j].  start and end are ABSOLUTE offsets in data
 *    (redgpu_collect_long's convention: the two verbs return the same record shape);
 *    start[j] - begin[j] is the position in the line.
 *  - *n_matches = the records FOUND over all lines; it may exceed cap, and then only the first
 *    cap records are stored - slots from min(*n_matches, cap) on are not written.  The cap cuts
 *    the global list, never a line's.  *n_lines = delimiters found.
 *  - line, begin, result, start, end and n_lines may be NULL, each on its own; all five arrays
 *    NULL, or cap == 0, gives the counts only, and then no line is walked a second time.
 *  - REDGPU_EAPI for a NULL handle, a NULL n_matches or a NULL data with len > 0 (the two
 *    argument checks run before the handle's device is looked at) and for a REDGPU_DEVICE_NONE
 *    handle; REDGPU_ELIMIT for a text redgpu_split_lines refuses.  In every error case
 *    *n_matches is untouched.
 *  - An empty text, or one without a delimiter: *n_lines = 0 and *n_matches = 0 (the _dev form
 *    writes them on the stream).
 *  - The records of the lines that END in one aligned 16 MiB of the text are counted in 32 bits
 *    (as the split counts its delimiters): only lines of gigabytes can hold more.
 * redgpu_last_kernel() says "k_collect_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - no count is read
 * back, and no per-line array is needed from the caller or in scratch (the lines are driven from
 * the split's delimiter bitmap; scratch is what redgpu_grep_text_dev takes, len / 4 + 32 bytes
 * per 16 KiB of text, from the thread's pool).
 * redgpu_collect_text: host buffers - one upload of the text, then n_lines, n_matches and the
 * filled prefixes back. */
int redgpu_collect_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t cap, uint64_t *n_lines, uint64_t *n_matches, uint64_t *line,
                        uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end);
int redgpu_collect_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t cap, uint64_t *n_lines, uint64_t *n_matches, uint64_t *line,
                            uint64_t *begin, int32_t *result, uint64_t *start, uint64_t *end,
                            void *stream);

/* grep -c per result, or grep -o | sort | uniq -c: raw text in, how many of each result out -
 * search<style,doLeader> (include/Matcher.h:557-640) or Red::collect (lib/Red.cpp:103-116) inside
 * the line loop of tools/skim_red.cpp:36-46, over the lines lib/Util.cpp:109-130 cuts, with only
 * the histogram of the results leaving the device: its size does not depend on the text.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter are not a line and contribute nothing.
 *  - what == REDGPU_TALLY_LINES: every line is one item, its value the result of
 *    search<style,do_leader> on that line alone - exactly redgpu_search_batch's result for it
 *    (and redgpu_grep_text's: the same verb and style normalisation).  A line that does not match
 *    has value 0.
 *  - what == REDGPU_TALLY_MATCHES: every record redgpu_collect_text would report is one item, its
 *    value the record's result.  style and do_leader are not looked at.  No item has value 0.
 *  - bins has n_bins + 1 slots.  An item of value r is counted in bins[r] when
 *    (uint32_t)r < n_bins, else in bins[n_bins] ("everything else").  n_bins == 0 is legal: one
 *    slot.  The slots sum to *n_lines (LINES) or to redgpu_collect_text's *n_matches (MATCHES).
 *  - accumulate == 0: all n_bins + 1 slots are overwritten.  accumulate != 0: the call's counts
 *    are added to what the slots hold - a stream of buffers tallied into one histogram.  n_lines
 *    and n_items are always overwritten.
 *  - *n_items = the items of value > 0: under LINES redgpu_grep_text's unbounded n_selected
 *    (without invert), under MATCHES redgpu_collect_text's n_matches.  *n_lines = delimiters found.
 *    n_lines and n_items may be NULL, each on its own; bins is required.
 *  - Counts are 64-bit and exact: integer sums, so the result does not depend on scheduling and
 *    is bit-identical from run to run.
 *  - REDGPU_EAPI for a NULL handle, a NULL bins, a NULL data with len > 0, a `what` other than the
 *    two above (the argument checks run before the handle's device is looked at) and for a
 *    REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style that does not exist (LINES only);
 *    REDGPU_ELIMIT for a text redgpu_split_lines refuses or n_bins > 2^31.  In every error case
 *    nothing the caller passed is written.
 *  - An empty text, or one without a delimiter: *n_lines = 0, *n_items = 0, the bins zeroed (left
 *    alone under accumulate); the _dev form does this on the stream.
 * redgpu_last_kernel() says "k_tally_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back.  Scratch is what the line driver needs (ONE bitmap and 20 bytes per 16 KiB chunk: len / 8
 * + 20 bytes per chunk + 32, from the thread's pool): no selected or hit bitmap, nothing
 * proportional to n_bins.
 * redgpu_tally_text: host buffers - one upload of the text, device bins of its own, n_bins + 1
 * counts and the two totals back; under accumulate they are added on the host.
 * redgpu_tally_lds_bins: how many leading bins the kernel keeps in on-chip memory (LDS) for this
 * handle, for texts below 4 GiB: min(4096, what the table leaves of a workgroup's share of the
 * LDS), 0 when the table leaves no room; values from there on are counted in device memory
 * directly.  A text of 4 GiB or more runs WITHOUT the LDS bins - every value is counted in device
 * memory directly: the same counts, at a lower rate where few values take most of the items.  A
 * pure host function, valid for REDGPU_DEVICE_NONE handles too; 0 for a NULL handle. */
#define REDGPU_TALLY_LINES   0  /* one item per line: search<style,do_leader> on the line */
#define REDGPU_TALLY_MATCHES 1  /* one item per match: Red::collect on the line */
int redgpu_tally_text(const redgpu_dfa *dfa, int what, int style, int do_leader,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                      int accumulate, uint64_t *n_lines, uint64_t *n_items, uint64_t *bins);
int redgpu_tally_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                          const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                          int accumulate, uint64_t *n_lines, uint64_t *n_items, uint64_t *bins,
                          void *stream);
uint32_t redgpu_tally_lds_bins(const redgpu_dfa *dfa);

/* sed: raw text in, the text with every line rewritten out - replace<style,doLeader>
 * (include/Matcher.h:186-191, core :643-706; what Red's replaceOne* / replaceAll* and
 * Red::replace / Red::globalReplace, include/Red.h:139-251, end in) inside the line loop of
 * tools/skim_red.cpp:36-46, over the lines lib/Util.cpp:109-130 cuts.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line.
 *  - only_changed == 0: the output is, for line k = 0, 1, ... in order,
 *    replace<style,do_leader>(line k, repl, max_count) followed by the delimiter, and behind the
 *    last line the tail, copied unchanged: the tail is never rewritten.  A line's rewritten bytes
 *    are exactly what redgpu_replace_batch gives for that line.
 *  - max_count is PER LINE: 1 is sed s/x/y/, 1 << 62 is s/x/y/g, 0 copies the text.
 *  - only_changed != 0 (sed -n 's/x/y/p'): only the lines with at least one replacement are
 *    emitted, each rewritten and followed by its delimiter; the tail is dropped.
 *  - *n_replaced = the sum of the per-line return values of replace; *out_len = the length of the
 *    whole output, whatever out_cap is; *n_lines = delimiters found.  n_lines and n_replaced may
 *    be NULL, each on its own; out_len is required.
 *  - out == NULL or out_cap == 0 gives the sizes only, and no line is walked a second time.
 *    Otherwise exactly the first min(*out_len, out_cap) bytes of the output are written - the cut
 *    may fall inside a line or inside a replacement - and bytes of out from there on are NOT
 *    written (redgpu_collect_text's rule, not redgpu_replace_long's): out may be the middle of a
 *    larger buffer.  out must not overlap data.  repl may be NULL when repl_len == 0.
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0, a NULL repl with
 *    repl_len > 0 (the argument checks run before the handle's device is looked at) and for a
 *    REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style that does not exist; REDGPU_ELIMIT for a
 *    text redgpu_split_lines refuses.  In every error case the three counts are untouched.
 *  - An empty text, or one without a delimiter: *n_lines = 0, *n_replaced = 0, *out_len = len (0
 *    under only_changed), and the text is copied when out is given (the _dev form writes the
 *    counts on the stream).
 *  - A single line of megabytes is walked by one lane, and an unchanged stretch of megabytes that
 *    ends in one 16 KiB chunk is copied by one wave: correct, and slow.
 * redgpu_last_kernel() says "k_replace_text": there is no other route.
 * _dev: every pointer device memory, repl too; asynchronous on `stream` from end to end - nothing
 * is read back, and no per-line array is needed from the caller or in scratch (the lines are
 * driven from the split's delimiter bitmap; scratch is the two bitmaps and a few words per 16 KiB
 * chunk: len / 4 + 44 bytes per chunk + 8 bytes per 1,024 chunks + 72, rounded up to 16, from
 * the thread's pool).
 * redgpu_replace_text: host buffers, as redgpu_replace_long - one upload of the text, a sizes
 * pass, a device output sized from *out_len, and min(*out_len, out_cap) bytes downloaded. */
int redgpu_replace_text(const redgpu_dfa *dfa, int style, int do_leader, int only_changed,
                        const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                        uint64_t repl_len, uint64_t max_count, uint64_t *n_lines,
                        uint64_t *n_replaced, uint64_t *out_len, uint8_t *out, uint64_t out_cap);
int redgpu_replace_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int only_changed,
                            const uint8_t *data, uint64_t len, uint8_t delim, const uint8_t *repl,
                            uint64_t repl_len, uint64_t max_count, uint64_t *n_lines,
                            uint64_t *n_replaced, uint64_t *out_len, uint8_t *out, uint64_t out_cap,
                            void *stream);

/* grep: raw text in, the selected lines out as a text, with grep's -A / -B / -C context - the line
 * loop of tools/skim_red.cpp:36-46 over the lines lib/Util.cpp:109-130 cuts, printing the line
 * where it prints the match.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line and are never emitted.
 *    This is the family's rule, not GNU grep's, which prints an unterminated last line.
 *  - Line k is SELECTED iff (search<style,do_leader>(line k).result_ > 0) != (invert != 0):
 *    exactly redgpu_grep_text's rule, verb and style normalisation.
 *  - Only the first max_count selected lines count (grep -m): a later matching line is not
 *    selected, though it can still be emitted as context of a counted one.
 *  - Line i is EMITTED iff some counted selected line j has j - before <= i <= j + after.  before
 *    and after are line counts and any value is legal, values above the number of lines too:
 *    nothing overflows.  0, 0 is plain grep; grep -C n is before = after = n.
 *  - The output is the emitted lines in text order, each followed by its delimiter, each ONCE:
 *    overlapping contexts do not duplicate a line, and there is no group separator between runs
 *    (grep --no-group-separator).  The output is a raw text every text verb accepts.
 *  - *n_selected = min(selected, max_count); *n_emitted = lines emitted; *out_len = the length of
 *    the whole output, whatever out_cap is; *n_lines = delimiters found.  n_lines, n_selected and
 *    n_emitted may be NULL, each on its own; out_len is required.
 *  - out == NULL or out_cap == 0 gives the sizes only.  Otherwise exactly the first
 *    min(*out_len, out_cap) bytes of the output are written - the cut may fall inside a line - and
 *    bytes of out from there on are NOT written (redgpu_replace_text's rule): out may be the middle
 *    of a larger buffer.  out must not overlap data.
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0 (the argument checks
 *    run before the handle's device is looked at) and for a REDGPU_DEVICE_NONE handle;
 *    REDGPU_EEXEC for a style that does not exist; REDGPU_ELIMIT for a text redgpu_split_lines
 *    refuses.  In every error case nothing of the caller's is written.
 *  - An empty text, or one without a delimiter: all four counts are 0 and nothing is written to
 *    out (the _dev form writes the counts on the stream).
 *  - A single line of megabytes is walked by one lane, and a run of emitted lines that ends in one
 *    16 KiB chunk is copied by one wave however far back it begins: correct, and slow.
 * redgpu_last_kernel() says "k_filter_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line array is needed from the caller or in scratch (the context is arithmetic
 * on line numbers over the split's delimiter bitmap and the SELECTED bitmap, which the EMIT bitmap
 * then overwrites; scratch is the two bitmaps and a few words per 16 KiB chunk: len / 4 + 68 bytes
 * per chunk + 8 bytes per 1,024 chunks + 72, rounded up to 16, from the thread's pool).
 * redgpu_filter_text: host buffers, as redgpu_replace_text - one upload of the text, a sizes pass,
 * a device output sized from *out_len, and min(*out_len, out_cap) bytes downloaded. */
int redgpu_filter_text(const redgpu_dfa *dfa, int style, int do_leader, int invert, uint64_t before,
                       uint64_t after, uint64_t max_count, const uint8_t *data, uint64_t len,
                       uint8_t delim, uint64_t *n_lines, uint64_t *n_selected, uint64_t *n_emitted,
                       uint64_t *out_len, uint8_t *out, uint64_t out_cap);
int redgpu_filter_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int invert,
                           uint64_t before, uint64_t after, uint64_t max_count,
                           const uint8_t *data, uint64_t len, uint8_t delim, uint64_t *n_lines,
                           uint64_t *n_selected, uint64_t *n_emitted, uint64_t *out_len,
                           uint8_t *out, uint64_t out_cap, void *stream);

/* grep -o as a text: raw text in, every match of every line out as bytes, one per output line -
 * Red::collect (lib/Red.cpp:103-116) inside the line loop of tools/skim_red.cpp:36-46, over the lines
 * lib/Util.cpp:109-130 cuts, printing the match; redgpu_collect_text's text-valued form.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter are not a line and contribute nothing.
 *  - The PIECES of line k are the spans replace<styLast,false>(line k, ., all) substitutes
 *    (include/Matcher.h:643-706), in order.  Piece j is line[a_j, e_j): e_j is the end of
 *    Red::collect's j-th Outcome on that line (redgpu_collect_text's end[] minus the line's begin),
 *    a_j the position at which the successful search<styLast,false> attempt began - the first
 *    position at or behind e_{j-1} from which the DFA accepts.  a_j <= start_j always (a loose-start
 *    DFA reports as start where it left its initial state, which lies behind a_j and can lie behind
 *    e_j: text[start:end] is NOT the match there), and a_j < e_j: a piece is never empty and never
 *    holds the delimiter.  The chain is Red::collect's and replaceCore's - the same one: the next
 *    attempt begins at e_j.  No style or leader argument, as in redgpu_collect_text.
 *  - Only the first max_per_line pieces of a line are emitted: 1 << 62 emits all of them, 1 the
 *    first match of every line, 0 nothing (*n_matches = 0, *out_len = 0).
 *  - The output is every emitted piece followed by delim, in line order, then match order: a raw
 *    text every text verb accepts (extract -> tally / grep / extract with another DFA stays on the
 *    device).
 *  - *n_matches = pieces emitted - with an unbounded max_per_line redgpu_collect_text's n_matches,
 *    and output line j is the bytes of its record j; *out_len = the length of the whole output,
 *    whatever out_cap is: the sum of the piece lengths plus *n_matches; *n_lines = delimiters found.
 *    n_lines and n_matches may be NULL, each on its own; out_len is required.
 *  - out == NULL or out_cap == 0 gives the sizes only, and no line is walked a second time.
 *    Otherwise exactly the first min(*out_len, out_cap) bytes of the output are written - the cut
 *    may fall inside a piece or on a separator - and bytes of out from there on are NOT written
 *    (redgpu_filter_text's rule): out may be the middle of a larger buffer.  out must not overlap
 *    data.
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0 (the argument checks
 *    run before the handle's device is looked at) and for a REDGPU_DEVICE_NONE handle;
 *    REDGPU_ELIMIT for a text redgpu_split_lines refuses.  In every error case nothing of the
 *    caller's is written.
 *  - An empty text, or one without a delimiter: all three counts are 0 and nothing is written to
 *    out (the _dev form writes the counts on the stream).
 *  - A single line of megabytes is walked by one lane, which also writes its pieces: correct, and
 *    slow.
 * redgpu_last_kernel() says "k_extract_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line or per-match array is needed from the caller or in scratch (the lines are
 * driven from the split's delimiter bitmap, a lane's place in the output comes from a scan over
 * per-chunk sums and a prefix inside the wave; scratch is the two bitmaps and a few words per
 * 16 KiB chunk, what redgpu_replace_text_dev takes: len / 4 + 44 bytes per chunk + 8 bytes per
 * 1,024 chunks + 72, rounded up to 16, from the thread's pool).
 * redgpu_extract_text: host buffers, as redgpu_filter_text - one upload of the text, a sizes pass,
 * a device output sized from *out_len, and min(*out_len, out_cap) bytes downloaded. */
int redgpu_extract_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                        uint64_t max_per_line, uint64_t *n_lines, uint64_t *n_matches,
                        uint64_t *out_len, uint8_t *out, uint64_t out_cap);
int redgpu_extract_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                            uint64_t max_per_line, uint64_t *n_lines, uint64_t *n_matches,
                            uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream);

/* awk -F / cut: raw text in, the selected COLUMNS of every line out as a text - what a log pipeline
 * does behind selecting and rewriting: cut -d, -f1,3, awk -F'[ \t]+' '{print $1, $4}'.  The DFA
 * describes the SEPARATOR; a field is what lies between two separators.
 *  - Lines are redgpu_split_lines' lines (lib/Util.cpp:109-130): [start, delimiter), the next one
 *    begins behind the delimiter, bytes after the last delimiter are not a line and contribute
 *    nothing (redgpu_extract_text's rule).
 *  - The SEPARATORS of a line are exactly the pieces redgpu_extract_text would emit for it: the
 *    spans replace<styLast,false> substitutes (include/Matcher.h:643-706), [a_j, e_j) along
 *    Red::collect's chain (lib/Red.cpp:103-116), never empty, never holding the delimiter.  No
 *    style or leader argument, as in redgpu_collect_text / redgpu_extract_text.  Only the first S
 *    separators of a line count: S = max_fields - 1 when max_fields > 0, all of them when it is 0.
 *  - With m counted separators a line has m + 1 FIELDS: field 1 is line[0, a_1), field j is
 *    line[e_{j-1}, a_j), the last is line[e_m, end).  Fields may be empty: a leading separator gives
 *    an empty field 1 - awk -F',' and re.split, not awk's default whitespace mode.  An empty line
 *    has one empty field; max_fields = 1 makes every line one field (and no line has a counted
 *    separator then).
 *  - select is a mask: bit k - 1 stands for field k (1..63), bit 63 for field 64 AND every later
 *    one, so cut's 5- is bits 4..63.  select == 0 is REDGPU_EAPI.
 *  - An emitted line becomes exactly one output line: its selected fields that exist, in ascending
 *    order, joined by sep, then delim - cut's rule: a selected field the line does not have adds
 *    nothing (no padding), and a line with none of them becomes an empty output line.  sep is 0..8
 *    bytes, passed BY VALUE: the sep_len low bytes of sep, little-endian (byte i of the joiner is
 *    (sep >> 8 i) & 255).  sep_len > 8 is REDGPU_EAPI.  Fields are not reordered.
 *  - only_delimited (cut -s): lines without a counted separator are not emitted.  Otherwise every
 *    line is emitted, and output line k corresponds to input line k.
 *  - *n_lines = delimiters found, *n_emitted = output lines, *n_fields = fields written,
 *    *out_len = the length of the whole output, whatever out_cap is.  out_len is required; the
 *    others may be NULL, each on its own.
 *  - out == NULL or out_cap == 0 gives the sizes only, and no line is walked a second time.
 *    Otherwise exactly the first min(*out_len, out_cap) bytes of the output are written - the cut
 *    may fall anywhere - and bytes of out from there on are NOT written (redgpu_filter_text's
 *    rule).  out must not overlap data.
 *  - The output is a raw text every text verb accepts: fields -> uniq_text of lines is
 *    cut -f3 | sort | uniq -c on the device.
 *  - A line is not walked behind the last field anyone asked for: with k the highest selected
 *    field (bit 63 clear), the search for separators ends behind the line's k-th.
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0, select == 0,
 *    sep_len > 8 (the argument checks run before the handle's device is looked at) and for a
 *    REDGPU_DEVICE_NONE handle; REDGPU_ELIMIT for a text redgpu_split_lines refuses.  In every
 *    error case nothing of the caller's is written.
 *  - An empty text, or one without a delimiter: all four counts are 0 and nothing is written to
 *    out (the _dev form writes the counts on the stream).
 *  - A single line of megabytes is walked by one lane: correct, and slow.
 * redgpu_last_kernel() says "k_fields_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line or per-field array is needed from the caller or in scratch (scratch is
 * what redgpu_replace_text_dev takes plus 8 bytes per 16 KiB chunk: len / 4 + 52 bytes per chunk +
 * 8 bytes per 1,024 chunks + 72, rounded up to 16, from the thread's pool).
 * redgpu_fields_text: host buffers, as redgpu_extract_text - one upload of the text, a sizes pass,
 * a device output sized from *out_len, and min(*out_len, out_cap) bytes downloaded. */
int redgpu_fields_text(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                       uint64_t select, uint64_t max_fields, int only_delimited,
                       uint64_t sep, uint32_t sep_len,
                       uint64_t *n_lines, uint64_t *n_emitted, uint64_t *n_fields,
                       uint64_t *out_len, uint8_t *out, uint64_t out_cap);
int redgpu_fields_text_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t len, uint8_t delim,
                           uint64_t select, uint64_t max_fields, int only_delimited,
                           uint64_t sep, uint32_t sep_len,
                           uint64_t *n_lines, uint64_t *n_emitted, uint64_t *n_fields,
                           uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream);

/* awk '{ print > file[class] }': raw text in, ALL its lines out as a text, grouped by the result
 * search reports for each - the fourth thing a log pipeline does with a many-pattern DFA, beside
 * selecting (grep_text, filter_text), rewriting (replace_text, extract_text) and counting
 * (tally_text).  The output is the text stably partitioned by bucket, and where each bucket begins.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line and are never emitted.
 *  - A line's VALUE is search<style,do_leader>(line).result_, 0 when it does not match: exactly
 *    redgpu_tally_text's REDGPU_TALLY_LINES item, with redgpu_grep_text's verb and style
 *    normalisation.  Its BUCKET is r when (uint32_t)r < n_bins, else n_bins ("everything else"):
 *    redgpu_tally_text's slot rule, n_bins + 1 buckets.  n_bins == 0 is legal: one bucket, the
 *    output is the text without its tail.  n_bins > 255 is REDGPU_ELIMIT: a line's bucket is kept
 *    in at most 8 bit-planes of the delimiter bitmap's layout.
 *  - The output is bucket 0's lines, then bucket 1's, ..., then bucket n_bins': inside a bucket the
 *    lines are in text order, each followed by its delimiter.  Every section is a raw text every
 *    text verb accepts.
 *  - drop_unmatched != 0: lines of value 0 are not emitted - they are still counted in
 *    bin_lines[0].  (Under n_bins == 0 bucket 0 then still holds the lines that match.)
 *  - bin_lines[n_bins + 1] = lines per bucket, dropped ones included: redgpu_tally_text's LINES bins,
 *    bit for bit.  May be NULL.
 *  - bin_offsets[n_bins + 2] = the byte offset in the output at which bucket b's section begins (an
 *    exclusive prefix sum of the sections' lengths); bin_offsets[n_bins + 1] == *out_len.  Required.
 *  - *out_len = the length of the whole output, whatever out_cap is (required); *n_lines =
 *    delimiters found, *n_routed = lines emitted; both may be NULL, each on its own.
 *  - out == NULL or out_cap == 0 gives the sizes only.  Otherwise exactly the first
 *    min(*out_len, out_cap) bytes of the concatenated output are written - the cut may fall inside
 *    a line or between two sections - and bytes of out from there on are NOT written
 *    (redgpu_filter_text's rule): out may be the middle of a larger buffer.  out must not overlap
 *    data.
 *  - REDGPU_EAPI for a NULL handle, a NULL bin_offsets, a NULL out_len, a NULL data with len > 0
 *    (the argument checks run before the handle's device is looked at) and for a
 *    REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style that does not exist; REDGPU_ELIMIT for a
 *    text redgpu_split_lines refuses and for n_bins > 255.  In every error case nothing of the
 *    caller's is written.
 *  - An empty text, or one without a delimiter: all counts and offsets are 0 and nothing is
 *    written to out (the _dev form writes them on the stream).
 *  - A single line of megabytes is walked by one lane; a chunk whose lines alternate between many
 *    buckets is copied as many short runs, each by a whole wave: correct, and slow.
 * redgpu_last_kernel() says "k_route_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line array is needed from the caller or in scratch (a line's bucket lives in
 * P bit-planes, P = the bit width of n_bins, 1 under n_bins == 0 with drop_unmatched; the sizes are
 * per (bucket, 16 KiB chunk), C = n_bins + 1 buckets, 2 in that case; scratch is (1 + P) * len / 8
 * for the bitmaps + (20 + 20 * C) bytes per chunk + 8 bytes per 1,024 (bucket, chunk) pairs + 72,
 * rounded up to 16, from the thread's pool).
 * redgpu_route_text: host buffers, as redgpu_filter_text - one upload of the text, a sizes pass,
 * a device output sized from *out_len, and min(*out_len, out_cap) bytes downloaded. */
int redgpu_route_text(const redgpu_dfa *dfa, int style, int do_leader, int drop_unmatched,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                      uint64_t *n_lines, uint64_t *n_routed, uint64_t *bin_lines,
                      uint64_t *bin_offsets, uint64_t *out_len, uint8_t *out, uint64_t out_cap);
int redgpu_route_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int drop_unmatched,
                          const uint8_t *data, uint64_t len, uint8_t delim, uint64_t n_bins,
                          uint64_t *n_lines, uint64_t *n_routed, uint64_t *bin_lines,
                          uint64_t *bin_offsets, uint64_t *out_len, uint8_t *out, uint64_t out_cap,
                          void *stream);

/* sed -n '/open/,/close/p': raw text in, the lines of its RANGES out as a text - the first verb in
 * which a line's fate depends on the lines in front of it: a stack trace, a request from "start"
 * to "done", a -----BEGIN / -----END block, a fenced block whose one pattern toggles.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line and are never emitted.
 *  - Line k's VALUE v_k is search<style,do_leader>(line k).result_, 0 when it does not match:
 *    exactly redgpu_route_text's and redgpu_tally_text's REDGPU_TALLY_LINES value, with
 *    redgpu_grep_text's verb and style normalisation.
 *  - The lines are read in text order with a state that is OUTSIDE or INSIDE; it starts outside,
 *    and ranges are numbered from 0:
 *      outside, v == open_result:  range r begins at this line, its OPEN line; the state becomes
 *        inside.  The line is never also the close line, even when open_result == close_result:
 *        sed tests the second address from the next line on;
 *      inside, v == close_result:  the range's CLOSE line; the state becomes outside behind it;
 *      inside, anything else:      a BODY line - also v == open_result when the two results differ;
 *      outside, anything else:     the line is outside - also a close line with no range open.
 *    A range still open at the last line ends there, as sed's does.  open_result == close_result
 *    is the TOGGLE form, sed -n '/```/,/```/p'.
 *  - Only ranges numbered below max_ranges are COUNTED; the lines of later ranges are outside.
 *  - Without invert a line of a counted range is emitted if it is a body line, if it is the open
 *    line and emit_open != 0, or if it is the close line and emit_close != 0.  Under invert exactly
 *    the other lines are emitted: sed '/A/,/B/d' is invert with both flags set.
 *  - The output is the emitted lines in text order, each once, each with its delimiter: a raw text
 *    every text verb accepts.
 *  - *n_lines = delimiters found, *n_ranges = min(ranges, max_ranges), *n_emitted = lines emitted,
 *    *out_len = the length of the whole output, whatever out_cap is.  out_len is required; the
 *    other three may be NULL, each on its own.
 *  - out == NULL or out_cap == 0 gives the sizes only.  Otherwise exactly the first
 *    min(*out_len, out_cap) bytes of the output are written - the cut may fall inside a line - and
 *    bytes of out from there on are NOT written (redgpu_filter_text's rule).  out must not overlap
 *    data.
 *  - The RECORDS are optional and do not depend on emit_open, emit_close or invert: first_line,
 *    last_line, begin and end hold rec_cap entries each, and each may be NULL on its own.  For every
 *    counted range r < rec_cap: first_line[r] and last_line[r] are the numbers of its open line and
 *    of its last line, begin[r] is the offset of the open line's first byte, end[r] is one past the
 *    delimiter of its last line - data[begin[r], end[r]) is a raw text.  Nothing is written at or
 *    behind min(*n_ranges, rec_cap).
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0, open_result < 1 or
 *    close_result < 1 - the message names the argument - (the argument checks run before the
 *    handle's device is looked at) and for a REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style
 *    that does not exist; REDGPU_ELIMIT for a text redgpu_split_lines refuses.  In every error case
 *    nothing of the caller's is written.
 *  - An empty text, or one without a delimiter: all four counts are 0 and nothing is written to out
 *    or to the records (the _dev form writes the counts on the stream).
 *  - A single line of megabytes is walked by one lane; a text whose ranges are one line long is
 *    copied as many short runs, each by a whole wave: correct, and slow.
 * redgpu_last_kernel() says "k_range_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line array is needed from the caller or in scratch ("is open" and "is close"
 * live in two bit-planes of the delimiter bitmap's layout, the state is carried across the 16 KiB
 * chunks by a scan; scratch is 3 * len / 8 for the bitmaps + 64 bytes per chunk + 8 bytes per 1,024
 * chunks + 72, rounded up to 16, from the thread's pool).
 * redgpu_range_text: host buffers, as redgpu_filter_text - one upload of the text, a sizes pass,
 * a device output sized from *out_len, and min(*out_len, out_cap) bytes and
 * min(*n_ranges, rec_cap) records downloaded. */
int redgpu_range_text(const redgpu_dfa *dfa, int style, int do_leader, int32_t open_result,
                      int32_t close_result, int emit_open, int emit_close, int invert,
                      uint64_t max_ranges, const uint8_t *data, uint64_t len, uint8_t delim,
                      uint64_t *n_lines, uint64_t *n_ranges, uint64_t *n_emitted, uint64_t *out_len,
                      uint8_t *out, uint64_t out_cap, uint64_t rec_cap, uint64_t *first_line,
                      uint64_t *last_line, uint64_t *begin, uint64_t *end);
int redgpu_range_text_dev(const redgpu_dfa *dfa, int style, int do_leader, int32_t open_result,
                          int32_t close_result, int emit_open, int emit_close, int invert,
                          uint64_t max_ranges, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t *n_lines, uint64_t *n_ranges, uint64_t *n_emitted,
                          uint64_t *out_len, uint8_t *out, uint64_t out_cap, uint64_t rec_cap,
                          uint64_t *first_line, uint64_t *last_line, uint64_t *begin,
                          uint64_t *end, void *stream);

/* grep -o | sort | uniq -c, by the matched BYTES: raw text in, one record per distinct byte string
 * out - which IPs, URIs or error strings occur, and how often.  redgpu_tally_text counts by result
 * number; this verb counts by content, and only the distinct strings leave the device.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line and contribute nothing.
 *  - what == REDGPU_UNIQ_MATCHES: the items are the pieces redgpu_extract_text would emit under
 *    max_per_line - the same chain, the same span (from where the matching attempt began to the
 *    record's end), without the delimiter extract_text puts behind each.  style and do_leader are
 *    not looked at.
 *  - what == REDGPU_UNIQ_LINES: the items are the lines redgpu_grep_text selects with
 *    search<style,do_leader> and no invert (its verb and style normalisation), each without its
 *    delimiter.  An empty selected line is an item of length 0.  max_per_line is not looked at.
 *  - Record j is distinct string j, in the order of FIRST APPEARANCE in the text: first[j] = the
 *    absolute offset of the string's earliest occurrence (strictly ascending in j), length[j] =
 *    its length in bytes - the string is data[first[j], first[j] + length[j]) - and count[j] =
 *    all its occurrences, exact.  Exactly min(*n_distinct, cap) records are written and nothing
 *    behind them; each array may be NULL on its own; cap == 0 gives the counts only.
 *  - *n_lines = delimiters found, *n_items = every item (dropped ones included), *n_distinct =
 *    the records that exist, whatever cap is, *n_dropped = the items in no record.  Each may be
 *    NULL.  Over ALL records, sum(count) + *n_dropped == *n_items.
 *  - table_slots is the size of the hash table the strings are kept in: a power of two,
 *    64 <= table_slots <= 2^32, 16 bytes each from the thread's scratch pool.  At most table_slots
 *    distinct strings get a record; twice the expected number keeps the probes short.
 *  - An item is dropped in exactly two cases.  It is 2^24 bytes or longer: decided before it is
 *    hashed, deterministic.  Or the table is full and does not hold its string.
 *  - *n_dropped == 0: every output is bit-identical from run to run.  When the table overflows,
 *    every record written is still exact for its string (count = all its occurrences, first = its
 *    earliest: an item is either counted in its string's record or dropped, never lost in
 *    between), *n_distinct == table_slots, and WHICH strings got a record depends on scheduling.
 *    The remedy is the caller's: call again with a larger table.
 *  - REDGPU_EAPI for a NULL handle, a NULL data with len > 0, a `what` other than the two below, a
 *    table_slots that is no power of two in [64, 2^32] (the argument checks run before the
 *    handle's device is looked at) and for a REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style
 *    that does not exist (LINES only); REDGPU_ELIMIT for a text redgpu_split_lines refuses or one
 *    of 2^40 - 1 bytes or more (an offset + 1 shares a 64-bit word with the 24-bit length).  In
 *    every error case nothing the caller passed is written.
 *  - An empty text, or one without a delimiter: all counts are 0 and no record is written (the
 *    _dev form does this on the stream).
 *  - A single line of megabytes is walked by one lane, and a table near full is probed slot by
 *    slot: correct, and slow.
 * redgpu_last_kernel() says "k_uniq_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back.  Scratch: 16 bytes per slot, two bitmaps (len / 4), 164 bytes per 16 KiB chunk, from the
 * thread's pool.
 * redgpu_uniq_text: host buffers - one upload of the text, a device table, the four counts and
 * min(*n_distinct, cap) records back.
 * redgpu_uniq_lds_slots: how many (string, count) slots a workgroup keeps in on-chip memory (LDS)
 * in front of the table for this handle, for texts below 4 GiB: a power of two up to 1024, what
 * the DFA's table leaves of a workgroup's share of the LDS; 0 when that is fewer than 64 - every
 * item then goes to the table in device memory directly.  The results do not depend on it.  A
 * text of 4 GiB or more runs WITHOUT the LDS front, whatever this returns: the same records, at
 * a lower rate where few strings take most of the items.  A pure host function, valid for
 * REDGPU_DEVICE_NONE handles too; 0 for a NULL handle. */
#define REDGPU_UNIQ_LINES   0  /* an item per selected line: search<style,do_leader> on the line */
#define REDGPU_UNIQ_MATCHES 1  /* an item per match: redgpu_extract_text's pieces */
int redgpu_uniq_text(const redgpu_dfa *dfa, int what, int style, int do_leader,
                     const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_per_line,
                     uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_items,
                     uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *first, uint64_t *length,
                     uint64_t *count);
int redgpu_uniq_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                         const uint8_t *data, uint64_t len, uint8_t delim, uint64_t max_per_line,
                         uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_items,
                         uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *first,
                         uint64_t *length, uint64_t *count, void *stream);
uint32_t redgpu_uniq_lds_slots(const redgpu_dfa *dfa);

/* awk '!seen[$k]++': raw text in, the lines CHOSEN BY CONTENT out as a text - the first line per
 * session id, every line whose request id occurs once, a message without its repeats: sort -u -k in
 * text order, uniq -u, uniq -d, and under invert awk 'seen[$k]++'.  redgpu_uniq_text returns the
 * distinct strings as records; this verb returns the lines they stand in.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line: never emitted, and they
 *    contribute no key.
 *  - Every line has at most ONE KEY, a byte range inside [line begin, delimiter]; a line without
 *    one is UNKEYED.
 *      what == REDGPU_DEDUP_WHOLE: the key is the line without its delimiter (an empty line has
 *        the empty key).  The DFA is not walked; style, do_leader and key_index are not looked at.
 *      what == REDGPU_DEDUP_LINES: the key is the line, if redgpu_grep_text selects it with
 *        search<style,do_leader> and no invert - redgpu_uniq_text's REDGPU_UNIQ_LINES item, with its
 *        verb and style normalisation; every other line is unkeyed.  key_index is not looked at.
 *      what == REDGPU_DEDUP_MATCH: the key is the key_index-th (1-based) piece
 *        redgpu_extract_text would emit for the line; a line with fewer pieces is unkeyed.  style
 *        and do_leader are not looked at.
 *      what == REDGPU_DEDUP_FIELD: the DFA is the SEPARATOR and the key is field key_index
 *        (1-based) under redgpu_fields_text's field rule with every separator counted
 *        (max_fields == 0).  A key may be EMPTY - the empty field at the very end of a line
 *        included; a line with fewer than key_index fields is unkeyed.  The line is not walked
 *        behind its key_index-th separator.  style and do_leader are not looked at.
 *  - Two keys are equal iff their bytes are.  Among all keyed lines a line is MARKED iff it holds
 *    the earliest occurrence of its key's string and min_count <= count <= max_count, count being
 *    the string's exact number of occurrences.  min_count = 1, max_count = 2^64 - 1 is
 *    awk '!seen[k]++'; 1, 1 is uniq -u in text order; 2, 2^64 - 1 is uniq -d in text order;
 *    min_count > max_count marks nothing and is legal.
 *  - Line i is EMITTED iff it is keyed and marked != (invert != 0), or it is unkeyed and
 *    keep_unkeyed != 0.  With the default window, invert is awk 'seen[k]++': every later duplicate.
 *  - The output is the emitted lines in text order, each once, each with its delimiter: a raw text
 *    every text verb accepts (fields_text | dedup_text, dedup_text | tally_text).
 *  - *n_lines = delimiters found, *n_keyed = keyed lines (dropped ones included), *n_distinct =
 *    the strings that hold a table record, whatever their counts, *n_dropped = keyed lines whose
 *    key got no record, *n_emitted = lines emitted, *out_len = the length of the whole output,
 *    whatever out_cap is.  out_len is required; the other five may be NULL, each on its own.
 *    While *n_dropped == 0: with the default window *n_emitted == *n_distinct, with invert beside
 *    it *n_emitted == *n_keyed - *n_distinct, and *n_distinct is redgpu_uniq_text's on the same
 *    items.
 *  - out == NULL or out_cap == 0 gives the sizes only.  Otherwise exactly the first
 *    min(*out_len, out_cap) bytes of the output are written - the cut may fall inside a line - and
 *    bytes of out from there on are NOT written (redgpu_filter_text's rule).  out must not overlap
 *    data.
 *  - table_slots is the size of the hash table the strings are kept in, as redgpu_uniq_text's: a
 *    power of two, 64 <= table_slots <= 2^32, 16 bytes each from the thread's scratch pool.
 *  - A key is dropped in redgpu_uniq_text's two cases.  It is 2^24 bytes or longer: decided before
 *    it is hashed, deterministic.  Or the table is full and does not hold its string.  A dropped
 *    line is keyed and NOT marked.
 *  - *n_dropped == 0: every output is bit-identical from run to run.  When the table overflows,
 *    every marked line is still a correct mark (its record's count and first offset are exact), and
 *    *n_distinct == table_slots; without invert the output is the exact output minus the lines
 *    whose string got no record, and WHICH lines those are depends on scheduling.  The remedy is
 *    the caller's: call again with a larger table.
 *  - REDGPU_EAPI for a NULL handle, a NULL out_len, a NULL data with len > 0, a `what` other than
 *    the four below, key_index == 0 under MATCH or FIELD, a table_slots that is no power of two in
 *    [64, 2^32] - the message names the argument - (the argument checks run before the handle's
 *    device is looked at) and for a REDGPU_DEVICE_NONE handle; REDGPU_EEXEC for a style that does
 *    not exist (LINES only); REDGPU_ELIMIT for a text redgpu_split_lines refuses or one of 2^40 - 1
 *    bytes or more.  In every error case nothing of the caller's is written.
 *  - An empty text, or one without a delimiter: all six counts are 0 and nothing is written to out
 *    (the _dev form writes the counts on the stream).
 *  - A single line of megabytes is walked by one lane, the mark of a string whose first line is
 *    that long scans the line's bits word by word, and a table near full is probed slot by slot:
 *    correct, and slow.
 * redgpu_last_kernel() says "k_dedup_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and no per-line array is needed from the caller or in scratch ("is keyed" and "is marked"
 * live in two bitmaps of the delimiter bitmap's layout; scratch is 16 bytes per slot + 3 * len / 8
 * for the bitmaps + 40 bytes per 16 KiB chunk + 8 bytes per 1,024 chunks + 72, rounded up to 16,
 * from the thread's pool).  A text of 4 GiB or more runs without the on-chip front of the table,
 * as redgpu_uniq_text's: the same output.
 * redgpu_dedup_text: host buffers, as redgpu_filter_text - one upload of the text, a sizes pass
 * that leaves the table and the bitmaps on the device, a device output sized from *out_len, and
 * min(*out_len, out_cap) bytes downloaded. */
#define REDGPU_DEDUP_WHOLE 0  /* every line is keyed by its own bytes; the DFA is not walked */
#define REDGPU_DEDUP_LINES 1  /* the lines grep_text selects (search<style,do_leader>), keyed by their bytes */
#define REDGPU_DEDUP_MATCH 2  /* key = piece number key_index of the line (extract_text's pieces) */
#define REDGPU_DEDUP_FIELD 3  /* the DFA is the SEPARATOR; key = field number key_index (fields_text's fields, max_fields = 0) */
int redgpu_dedup_text(const redgpu_dfa *dfa, int what, int style, int do_leader, uint64_t key_index,
                      uint64_t min_count, uint64_t max_count, int invert, int keep_unkeyed,
                      const uint8_t *data, uint64_t len, uint8_t delim, uint64_t table_slots,
                      uint64_t *n_lines, uint64_t *n_keyed, uint64_t *n_distinct,
                      uint64_t *n_dropped, uint64_t *n_emitted, uint64_t *out_len, uint8_t *out,
                      uint64_t out_cap);
int redgpu_dedup_text_dev(const redgpu_dfa *dfa, int what, int style, int do_leader,
                          uint64_t key_index, uint64_t min_count, uint64_t max_count, int invert,
                          int keep_unkeyed, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t table_slots, uint64_t *n_lines, uint64_t *n_keyed,
                          uint64_t *n_distinct, uint64_t *n_dropped, uint64_t *n_emitted,
                          uint64_t *out_len, uint8_t *out, uint64_t out_cap, void *stream);

/* awk '{ n[c]++; s[c] += $x; if ($x > m[c]) m[c] = $x }': raw text in, per result the count, sum,
 * minimum and maximum of the decimal numbers found in the matches out - Red::collect
 * (lib/Red.cpp:103-116) inside the line loop of tools/skim_red.cpp:36-46, over the lines
 * lib/Util.cpp:109-130 cuts, with only four 64-bit words per slot leaving the device.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter are not a line and contribute nothing.
 *  - The items are exactly the pieces redgpu_extract_text would emit under the same max_per_line:
 *    piece j of a line is the span [a_j, e_j) along Red::collect's chain - from where the matching
 *    attempt began to the match's end.  An item's result is the result of redgpu_collect_text's
 *    record for that match.  There is no style or leader argument, as in redgpu_extract_text.
 *    max_per_line: 1 << 62 = all pieces, 1 = the first match of each line, 0 = nothing.
 *  - The number of an item.  A digit is a byte 0x30..0x39; the runs of a piece are its maximal
 *    substrings of digits - only the piece's OWN bytes are looked at, so a digit next to the piece
 *    in the text is not part of a run.  which == REDGPU_SUM_FIRST takes the first run,
 *    which == REDGPU_SUM_LAST the last (for patterns such as " 200 [0-9]+", whose context carries
 *    digits of its own).  The item's value is that run read as an unsigned decimal integer;
 *    leading zeros are allowed and count against nothing.  The item is NUMERIC iff it has a run
 *    and the value is below 2^64; otherwise (no digit, or 2^64 and more) it is counted in *n_items
 *    and in no statistic.  Signs, fractions, hex and thousands separators are not interpreted:
 *    "-5" is 5, "3.14" is 3 under FIRST and 14 under LAST.
 *  - Slots follow redgpu_tally_text's rule: an item of result r goes to slot r when
 *    (uint32_t)r < n_bins, else to slot n_bins.  n_bins == 0 is legal: one slot.
 *  - stats holds 4 * (n_bins + 1) 64-bit words, row-major: stats[row * (n_bins + 1) + slot], the
 *    rows REDGPU_SUM_COUNT, REDGPU_SUM_SUM, REDGPU_SUM_MIN, REDGPU_SUM_MAX over the slot's numeric
 *    items.  A slot without numeric items has count 0, sum 0, min 2^64 - 1, max 0.  Sums are
 *    modulo 2^64.
 *  - accumulate == 0: all slots are overwritten.  accumulate != 0: the call's statistics are merged
 *    into what the slots hold - counts and sums added (modulo 2^64), the smaller min and the larger
 *    max kept: a stream of buffers reduced into one table.  The three scalars are always
 *    overwritten.
 *  - *n_lines = delimiters found; *n_items = pieces considered (redgpu_extract_text's n_matches
 *    for the same max_per_line); *n_numeric = items in the statistics (what this call adds to the
 *    count row).  Each of the three may be NULL, on its own; stats is required.
 *  - Every operation is a commutative integer operation: all outputs are exact and bit-identical
 *    from run to run, whatever the scheduling.  A text of 4 GiB and more is treated as any other.
 *  - REDGPU_EAPI for a NULL handle, a NULL stats, a NULL data with len > 0, a `which` other than
 *    the two above (the argument checks run before the handle's device is looked at) and for a
 *    REDGPU_DEVICE_NONE handle; REDGPU_ELIMIT for a text redgpu_split_lines refuses or
 *    n_bins > 2^31.  In every error case nothing the caller passed is written.
 *  - An empty text, or one without a delimiter: the three scalars 0, the slots emptied (left alone
 *    under accumulate); the _dev form does this on the stream.
 * redgpu_last_kernel() says "k_sum_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back.  Scratch is what redgpu_tally_text_dev takes (ONE bitmap and 20 bytes per 16 KiB chunk):
 * nothing proportional to n_bins.
 * redgpu_sum_text: host buffers - one upload of the text, device stats of its own, the table and
 * the three scalars back; under accumulate the merge happens on the host.
 * redgpu_sum_lds_bins: how many leading slots the kernel keeps in on-chip memory (LDS) for this
 * handle: min(512, what the table leaves of a workgroup's share of the LDS / 32), a multiple of 4;
 * slots from there on are kept in device memory directly.  The results do not depend on it.  A
 * pure host function, valid for REDGPU_DEVICE_NONE handles too; 0 for a NULL handle. */
#define REDGPU_SUM_FIRST 0  /* an item's number is its first run of digits */
#define REDGPU_SUM_LAST  1  /* ... its last run of digits */
#define REDGPU_SUM_COUNT 0  /* the rows of stats */
#define REDGPU_SUM_SUM   1
#define REDGPU_SUM_MIN   2
#define REDGPU_SUM_MAX   3
int redgpu_sum_text(const redgpu_dfa *dfa, int which, const uint8_t *data, uint64_t len,
                    uint8_t delim, uint64_t max_per_line, uint64_t n_bins, int accumulate,
                    uint64_t *n_lines, uint64_t *n_items, uint64_t *n_numeric, uint64_t *stats);
int redgpu_sum_text_dev(const redgpu_dfa *dfa, int which, const uint8_t *data, uint64_t len,
                        uint8_t delim, uint64_t max_per_line, uint64_t n_bins, int accumulate,
                        uint64_t *n_lines, uint64_t *n_items, uint64_t *n_numeric, uint64_t *stats,
                        void *stream);
uint32_t redgpu_sum_lds_bins(const redgpu_dfa *dfa);

/* awk '{ n[$k]++; s[$k] += $v; if ($v > m[$k]) m[$k] = $v }': raw text in, ONE RECORD PER KEY out -
 * bytes served per client address, latency minimum and maximum per endpoint, rows and total per
 * customer id.  redgpu_sum_text groups the numbers by result number and redgpu_uniq_text counts
 * strings; this verb keeps redgpu_sum_text's four statistics per distinct key STRING.
 *  - Lines are redgpu_split_lines' lines: [start, delimiter), the next one begins behind the
 *    delimiter, bytes after the last delimiter (the tail) are not a line and contribute nothing.
 *  - The ITEMS of a line, numbered from 1 (redgpu_dedup_text's key rule, word for word):
 *      what == REDGPU_GROUP_MATCH: item j is the j-th piece redgpu_extract_text would emit for the
 *        line.
 *      what == REDGPU_GROUP_FIELD: the DFA is the SEPARATOR and item j is field j under
 *        redgpu_fields_text's field rule with every separator counted (max_fields == 0).  A field
 *        may be EMPTY - the empty field at the very end of a line included.
 *  - key_index (>= 1) names the line's KEY item and value_index (0 = no value) its VALUE item;
 *    value_index may be below, equal to or above key_index.  A line with fewer than key_index items
 *    is UNKEYED and contributes nothing: its value is not looked at.  The line is not walked behind
 *    its max(key_index, value_index)-th piece (MATCH) or separator (FIELD).
 *  - The value's number follows redgpu_sum_text's rule on the value item's OWN bytes: its first
 *    (which == REDGPU_SUM_FIRST) or last (REDGPU_SUM_LAST) maximal run of digits 0x30..0x39, read as
 *    an unsigned decimal; leading zeros are allowed, and digits next to the item but outside it are
 *    not seen.  A keyed line is NUMERIC iff its value item exists, has a run, and the run's value is
 *    below 2^64.  With value_index == 0 no line is numeric.
 *  - Two keys are equal iff their bytes are.  There is one record per distinct key string, in the
 *    order of FIRST APPEARANCE (redgpu_uniq_text's order): first[j] is strictly ascending.
 *      first[j], length[j]: the key is data[first[j], first[j] + length[j]), its earliest occurrence;
 *      count[j]: the keyed lines with that key;
 *      stats: four rows with row stride cap - stats[row * cap + j], the rows REDGPU_SUM_COUNT (the
 *        key's numeric lines), REDGPU_SUM_SUM (modulo 2^64), REDGPU_SUM_MIN and REDGPU_SUM_MAX.  A key
 *        without numeric lines has 0, 0, 2^64 - 1, 0.
 *    Exactly min(*n_distinct, cap) records are written and nothing behind them in any array, no row
 *    of stats excepted.  Each of the four arrays may be NULL on its own; cap == 0 gives the scalars
 *    only.
 *  - *n_lines = delimiters found; *n_keyed = keyed lines, dropped ones included; *n_numeric =
 *    numeric lines whose key holds a record (the sum of the COUNT row over ALL records, whatever cap
 *    is); *n_distinct = the strings that hold a record, whatever cap is; *n_dropped = keyed lines in
 *    no record.  Over all records sum(count) + *n_dropped == *n_keyed.  Each of the five may be
 *    NULL.
 *  - table_slots is the size of the hash table the strings are kept in, as redgpu_uniq_text's: a
 *    power of two, 64 <= table_slots <= 2^32; here a slot takes 16 + 32 bytes from the thread's
 *    scratch pool.
 *  - A key is dropped in redgpu_uniq_text's two cases: it is 2^24 bytes or longer (decided before it
 *    is hashed, deterministic), or the table is full and does not hold its string.  A dropped line
 *    enters no record, neither with its count nor with its number.  A record that exists is exact in
 *    all seven values whatever was dropped: a line is either wholly in its key's record or dropped.
 *  - *n_dropped == 0: every output is bit-identical from run to run - all operations are commutative
 *    integer operations.  When the table overflows, *n_distinct == table_slots and WHICH strings
 *    hold the records depends on scheduling; the remedy is the caller's: a larger table.
 *  - REDGPU_EAPI for a NULL handle, a NULL data with len > 0, a `what` other than the two below, a
 *    `which` other than redgpu_sum_text's two, key_index == 0, a table_slots that is no power of two
 *    in [64, 2^32] - the message names the argument - (the argument checks run before the handle's
 *    device is looked at) and for a REDGPU_DEVICE_NONE handle; REDGPU_ELIMIT for a text
 *    redgpu_split_lines refuses or one of 2^40 - 1 bytes or more.  In every error case nothing of
 *    the caller's is written.
 *  - An empty text, or one without a delimiter: the five scalars are 0 and no record is written
 *    (the _dev form writes the scalars on the stream).
 *  - A single line of megabytes is walked by one lane and a table near full is probed slot by slot:
 *    correct, and slow.
 * redgpu_last_kernel() says "k_group_text": there is no other route.
 * _dev: every pointer device memory; asynchronous on `stream` from end to end - nothing is read
 * back, and there is no per-line array (scratch is 16 + 32 bytes per slot - the table and the
 * statistics beside it - + len / 4 for the two bitmaps + 164 bytes per 16 KiB chunk + 8 bytes per
 * 1,024 chunks + 72, rounded up to 16, from the thread's pool).  A text of 4 GiB or more runs
 * without the on-chip front of the table, as redgpu_uniq_text's: the same output.
 * redgpu_group_text: host buffers - one upload of the text, the table in the stream's scratch,
 * device records of the call's own, then the five scalars and min(*n_distinct, cap) records back.
 * redgpu_group_lds_slots: how many (string, count, statistics) slots a workgroup keeps in on-chip
 * memory (LDS) for this handle: the largest power of two <= 256 that the table leaves room for in a
 * workgroup's share of the LDS at 48 bytes a slot, or 0 when that is below 64.  The results do not
 * depend on it; REDGPU_UNIQ_PLAIN=1 in the environment runs without the front.  A pure host
 * function, valid for REDGPU_DEVICE_NONE handles too; 0 for a NULL handle. */
#define REDGPU_GROUP_MATCH 0  /* item j = piece number j of the line (extract_text's pieces) */
#define REDGPU_GROUP_FIELD 1  /* the DFA is the SEPARATOR; item j = field number j (fields_text's fields, max_fields = 0) */
int redgpu_group_text(const redgpu_dfa *dfa, int what, uint64_t key_index, uint64_t value_index,
                      int which, const uint8_t *data, uint64_t len, uint8_t delim,
                      uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_keyed,
                      uint64_t *n_numeric, uint64_t *n_distinct, uint64_t *n_dropped,
                      uint64_t *first, uint64_t *length, uint64_t *count, uint64_t *stats);
int redgpu_group_text_dev(const redgpu_dfa *dfa, int what, uint64_t key_index, uint64_t value_index,
                          int which, const uint8_t *data, uint64_t len, uint8_t delim,
                          uint64_t table_slots, uint64_t cap, uint64_t *n_lines, uint64_t *n_keyed,
                          uint64_t *n_numeric, uint64_t *n_distinct, uint64_t *n_dropped,
                          uint64_t *first, uint64_t *length, uint64_t *count, uint64_t *stats,
                          void *stream);
uint32_t redgpu_group_lds_slots(const redgpu_dfa *dfa);

/* Measurement aid, no counterpart in the reference: one streaming read of `bytes` of device
 * memory (16-byte aligned) on the handle's device, asynchronous on `stream` - the read-bandwidth
 * calibration bench.py reports beside the roofline.  `sink` is a device uint32 the kernel may
 * increment (it keeps the loads alive); its value carries no meaning. */
int redgpu_diag_read_dev(const redgpu_dfa *dfa, const void *data, uint64_t bytes, uint32_t *sink,
                         void *stream);

/* More calibration kernels behind bench.py's roofline block (device-resident, asynchronous):
 *  - redgpu_diag_lds_dev: the walk without its memory side - `rounds` x 64 dependent table
 *    lookups per chain, 4 chains per lane, 512 lanes per CU, input bytes from registers; times
 *    the LDS gather rate that bounds a one-lookup-per-byte walk.  *lookups (host) receives the
 *    number of lookups the launch performs.
 *  - redgpu_diag_walked_dev: adds to *walked (device uint64, zeroed by the caller) the bytes the
 *    loop of match<styLast,doLeader> (include/Matcher.h:424-479) consumes over the batch: the
 *    bytes an early-exit walk actually reads, as opposed to the bytes of the lines. */
int redgpu_diag_lds_dev(const redgpu_dfa *dfa, uint32_t rounds, uint32_t *sink, uint64_t *lookups,
                        void *stream);
/*  - redgpu_diag_lines_dev: the memory side of the fixed-stride walk and nothing else.
 *    line_bytes = 64: every lane requests its line the way the streaming kernel does and stores
 *    one Outcome-shaped record per line (result int32, start / end uint64; the values are
 *    meaningless) - 64 B read + 20 B written per line; what HBM sustains for that mix is the roof
 *    of BASELINE configs[1]'s shape.  line_bytes a multiple of 128: the long-line request pattern
 *    (a lane asks for one whole cache line of each of its two lines at a time, so a wave touches
 *    64 cache lines a line length apart), reads only (result / start / end may be NULL) - the
 *    roof of configs[2]'s and configs[4]'s shapes.  n_lines is rounded down to a multiple of
 *    1024. */
int redgpu_diag_lines_dev(const redgpu_dfa *dfa, const uint8_t *data, uint64_t n_lines,
                          uint64_t line_bytes, int32_t *result, uint64_t *start, uint64_t *end,
                          uint32_t *sink, void *stream);
/*  - redgpu_diag_l2_dev: the gather rate of a table that lives in L2 - `rounds` DEPENDENT 2-byte
 *    gathers per chain (the next index is computed from the value just read, as a walk's next
 *    state is) over `table`, 2^20 uint16 of device memory (2 MiB, any contents), 2 chains per lane,
 *    2048 lanes per CU, no input side: the roof of a one-lookup-per-byte walk over a
 *    REDGPU_TAB_GLOBAL_* DFA (SYN-4K), measured in the run instead of derived from L2's nominal
 *    bandwidth.  *lookups (host) = gathers performed. */
int redgpu_diag_l2_dev(const redgpu_dfa *dfa, const uint16_t *table, uint32_t rounds, uint32_t *sink,
                       uint64_t *lookups, void *stream);
/*  - redgpu_diag_match_all_long_dev: how the calling thread's last redgpu_match_all_long_dev call
 *    on `stream` resolved its chunks (route "k_match_all_long"; EAPI after any other).  Queues a
 *    copy of 8 words into stats (device memory): [0..3] chunks walked again in each of the four
 *    rounds, [4] the first chunk still inconsistent behind them (= [7] when there is none),
 *    [5] 1 = the leader test passed, [6] chunks the serial lane walked again, [7] chunks. */
int redgpu_diag_match_all_long_dev(const redgpu_dfa *dfa, uint32_t *stats, void *stream);
int redgpu_diag_walked_dev(const redgpu_dfa *dfa, int do_leader, const uint8_t *data,
                           const uint64_t *offsets, uint64_t stride, uint64_t n, uint64_t *walked,
                           void *stream);

/* The host-buffer entry points stage through device buffers and two private streams that each
 * HOST THREAD keeps per device (no allocation, stream creation or device-wide synchronisation per
 * call).  They - and the thread's launch scratch - are released when the thread exits; a
 * long-lived thread that is done with the library may release them early.
 * redgpu_scratch_entries: launch scratch buffers currently cached by all threads together
 * (bounded per thread; diagnostics / tests).
 * redgpu_host_pins_held: over the calling thread's stages, the registrations made for a call that
 * are not yet released plus the downloads not yet copied into the caller's buffers - 0 whenever a
 * host-buffer entry point has returned (diagnostics / tests). */
void redgpu_thread_release(void);
uint64_t redgpu_scratch_entries(void);
uint64_t redgpu_host_pins_held(void);
/* Diagnostics: how the host-buffer entry points have moved caller memory so far, transfers by
 * route - [0] memory the caller pinned, [1] through the calling thread's pinned arena (calls that
 * upload < 8 MiB), [2] registered for the duration of the call, [3] handed to the runtime
 * pageable (nothing else was possible). */
void redgpu_host_route_counts(uint64_t counts[4]);

/* A caller that keeps its buffers from call to call (tools/thr_red.cpp's workers do) can pin them
 * ONCE: the host-buffer entry points recognise pinned memory (registered here, or allocated by
 * hipHostMalloc / torch's pin_memory) and then cut even a batch of a few MiB into 8 MiB chunks
 * whose uploads, walks and downloads overlap on the thread's two streams - pageable memory is
 * only pipelined above 64 MiB, where pinning it for the duration of one call pays.  The range
 * must stay mapped until redgpu_host_unregister; (un)registering costs about a millisecond per
 * 16 MiB, which is why the library does not do it per call on its own. */
int redgpu_host_register(void *ptr, size_t bytes);
int redgpu_host_unregister(void *ptr);

/* ---- several GPUs of one node --------------------------------------------------------------
 * The reference scales by calling its read-only matcher from N threads over one shared Red
 * (tools/thr_red.cpp:84-91).  The device form of that picture: a GROUP holds one image of the
 * same blob per device ("uploaded once" per GPU); a batch is cut into contiguous shards - equal
 * line counts for a fixed stride, equal BYTES for ragged lines - every device scans its shard
 * with no data-path exchange, and only the per-line results travel.
 *   redgpu_group_create      devices[] may name a device more than once (the shards then share
 *                            that GPU: how a one-GPU box rehearses the sharding); opts->device
 *                            is ignored.  Fails as redgpu_dfa_create does.
 *   redgpu_group_plan        cuts[0..n_devices]: shard g = lines [cuts[g], cuts[g+1]).
 *   redgpu_group_batch       HOST buffers, verb = REDGPU_VERB_*: one host thread per device runs
 *                            its shard through the host-buffer entry point of that verb; results
 *                            land in the caller's arrays (start / end NULL for check and scan).
 *   redgpu_group_batch_dev   shard g already resident on device g (data[g], offsets[g] or NULL,
 *                            n[g] lines; ragged offsets are relative to data[g]).  Every device
 *                            scans on a stream of its own; results are packed into compact
 *                            records (result in 1/2/4 bytes by the DFA's largest result, start /
 *                            end in 1/2/4 bytes by the stride, 4 bytes for ragged lines - 8 on a
 *                            handle made with REDGPU_F_FORCE_GENERIC), moved to the ROOT device
 *                            (devices[0]) over xGMI - REDGPU_GATHER_PEER: peer copies,
 *                            REDGPU_GATHER_RCCL: ncclSend / ncclRecv (librccl.so loaded on first
 *                            use) - and widened there into result / start / end (memory of the
 *                            root device, sum(n[]) entries, shard order).  Asynchronous, no host
 *                            synchronisation: the results are complete when `root_stream` (a
 *                            stream of the root device, NULL = its null stream) has reached this
 *                            point.  shard_streams[g] (a stream of device g, or shard_streams ==
 *                            NULL): the stream on which shard g's inputs were produced and on
 *                            which the caller will touch them next - the shard's scan starts where
 *                            that stream stands at the call, and the stream in turn waits until
 *                            the scan has read the shard, so inputs may be reused or freed
 *                            stream-ordered.  With shard_streams == NULL every input must be
 *                            complete at the call and stay untouched until root_stream has passed
 *                            it.  One such call at a time per group (serialised internally).
 *                            The peer / RCCL paths between DISTINCT devices have not run on
 *                            hardware yet (single-GPU boxes only): see INTEGRATION.md. */
typedef struct redgpu_group redgpu_group;
#define REDGPU_VERB_CHECK  0
#define REDGPU_VERB_MATCH  1
#define REDGPU_VERB_SCAN   2
#define REDGPU_VERB_SEARCH 3
#define REDGPU_GATHER_PEER 0
#define REDGPU_GATHER_RCCL 1
int redgpu_group_create(const void *reda, size_t len, const redgpu_opts *opts,
                        const int32_t *devices, uint32_t n_devices, redgpu_group **out);
void redgpu_group_destroy(redgpu_group *group);
uint32_t redgpu_group_size(const redgpu_group *group);
const redgpu_dfa *redgpu_group_member(const redgpu_group *group, uint32_t i);
int redgpu_group_plan(const redgpu_group *group, const uint64_t *offsets, uint64_t stride,
                      uint64_t n, uint64_t *cuts);
int redgpu_group_batch(const redgpu_group *group, int verb, int style, int do_leader,
                       const uint8_t *data, const uint64_t *offsets, uint64_t stride, uint64_t n,
                       int32_t *result, uint64_t *start, uint64_t *end);
int redgpu_group_batch_dev(redgpu_group *group, int verb, int style, int do_leader,
                           const uint8_t *const *data, const uint64_t *const *offsets,
                           uint64_t stride, const uint64_t *n, int32_t *result, uint64_t *start,
                           uint64_t *end, int gather, void *const *shard_streams,
                           void *root_stream);

/* The compact record format of redgpu_group_batch_dev, for callers that move the results
 * themselves (one process per GPU over torch.distributed / RCCL: one_amd/sharding.py).  A
 * shard's n Outcomes become three planes, each starting on a 16-byte boundary:
 *   [result: n x result_width][start: n x pos_width (absent when start == NULL)][end: n x pos_width]
 * little-endian, result_width in {1,2,4} (results are >= 0, include/Types.h:22), pos_width in
 * {1,2,4,8}; the caller picks widths that hold the DFA's largest result and the longest line.
 *   redgpu_records_bytes       size of a packed shard
 *   redgpu_records_pack_dev    device arrays -> packed (device) buffer, on `stream`
 *   redgpu_records_unpack_dev  packed buffer -> int32 result / 64-bit start, end (device), on `stream`
 * All pointers are memory of `device` (REDGPU_DEVICE_CURRENT = the caller's current device). */
uint64_t redgpu_records_bytes(uint64_t n, int result_width, int pos_width, int with_start);
int redgpu_records_pack_dev(int32_t device, const int32_t *result, const uint64_t *start,
                            const uint64_t *end, uint64_t n, int result_width, int pos_width,
                            void *records, void *stream);
int redgpu_records_unpack_dev(int32_t device, const void *records, uint64_t n, int result_width,
                              int pos_width, int32_t *result, uint64_t *start, uint64_t *end,
                              void *stream);

/* Name of the kernel the last *_batch* call on this thread launched (for profiles), or "". */
const char *redgpu_last_kernel(void);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *redgpu_last_error(void);

/* Library version: major*10000 + minor*100 + patch. */
int redgpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REDGPU_H */
