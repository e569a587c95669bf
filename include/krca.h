/*
 * krca.h — C-ABI of libkrca.so, the MI355X (gfx950) numeric core behind the RCA agents.
 *
 * The reference (vobbilis/kubernetes-rca-system) is pure Python, so there is no FFI of its own
 * to mirror; these entry points replace the per-pod Python loops of its non-LLM agents and are
 * bound from Python with ctypes (kubernetes-rca-system_amd/krca/native.py; INTEGRATION.md shows
 * the binding a maintainer would add to the reference).  Each entry cites the reference code
 * whose loop it replaces.
 *
 * Conventions:
 *  - every buffer argument is a caller-owned DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous unless noted;
 *  - no allocation on the hot path: scratch comes from caller workspaces sized by the
 *    *_workspace_size / *_num_* helpers;
 *  - return 0 on success, a negative errno-style code on failure; krca_last_error() returns a
 *    thread-local message; no C++ exception crosses the ABI;
 *  - re-entrant per stream; integer outputs are deterministic (no order-dependent reductions);
 *  - buffer contents before a call: unless an entry says otherwise, every output is written over its
 *    whole logical extent and every workspace is initialised by the call itself, so neither needs any
 *    initialisation and may hold anything; no call writes outside the sizes given here or by its
 *    size function.  Each entry states it per buffer ("Buffers:"); DESIGN.md "Buffer contracts" names
 *    the write behind each statement and tests/test_gpu_buffers.py checks them under poison patterns.
 */
#ifndef KRCA_H
#define KRCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KRCA_OK 0
#define KRCA_EINVAL (-22)
#define KRCA_ENOMEM (-12)
#define KRCA_EDEVICE (-5) /* HIP runtime error */
#define KRCA_ENOTCONV (-70) /* PageRank did not converge within max_iter */

#define KRCA_NCAT 13 /* log error categories, ref:agents/logs_agent.py:20-34 */

/* flag bits of krca_usage_flags / krca_rolling_score (ref:agents/metrics_agent.py:93,101,140,148) */
#define KRCA_F_CPU80 1u
#define KRCA_F_CPU90 2u
#define KRCA_F_MEM80 4u
#define KRCA_F_MEM90 8u

int krca_version(void);
const char* krca_last_error(void);
int krca_device_count(int* n_host);

/* Kernel-development switches and test hooks: KRCA_SCORE_IMPL, KRCA_PPR_GRID, KRCA_PPR_DICT, KRCA_CORR_DEBUG,
 * KRCA_CORR_RS_GRID, KRCA_CORR_BATCH, KRCA_CORR_AMB_TILE, KRCA_PPR_FUSE, KRCA_PPR_NT, KRCA_PPR_XCD, KRCA_LOG_FUSED,
 * KRCA_CORR_RS_GROUP, KRCA_CORR_SIDE, KRCA_CORR_RS_Q16, KRCA_CORR_CAPC, KRCA_CORR_KM_EXTRA, KRCA_CORR_RSG_GRID,
 * KRCA_CORR_PROJ, KRCA_TRACE_IMPL, KRCA_GRAPH_GRID (meanings and defaults: csrc/krca_common.h).  Initialised once from the
 * environment variables of the same names when the library loads; launchers never call getenv.  Process-global,
 * not thread-safe (set them before launching work).  Unknown names: KRCA_EINVAL. */
int krca_tune_set(const char* name, int32_t value);
int krca_tune_get(const char* name, int32_t* value_host);

/* ---- a1/a2: instantaneous usage thresholds ------------------------------------------------
 * Replaces the pod loops of MetricsAgent._analyze_cpu_usage / _analyze_memory_usage
 * (ref:agents/metrics_agent.py:88-94, 135-141): flags[p] gets KRCA_F_CPU80 iff usage[p][0] > 80,
 * KRCA_F_CPU90 iff > 90, KRCA_F_MEM80 / KRCA_F_MEM90 likewise for usage[p][1] (strict, float32).
 * Buffers: flags [P] fully written, no initialisation needed; no workspace. */
int krca_usage_flags(const float* usage /*[P][2]*/, int64_t P, uint8_t* flags /*[P]*/, void* stream);

/* ---- a5: rolling z-score anomaly scoring (new primitive; plugs in at
 * ref:agents/metrics_agent.py:44-47).  x is time-major [T][P][M] float32 (series s = p*M+m).
 * For t in [W, T), over the trailing window x[t-W..t-1] (float64 sliding sums s1, s2 in a fixed
 * order): A = W*x_t - s1, B = W*s2 - s1^2 (= W^2 var, ddof 0), z = A/sqrt(B) = (x_t - mean)/std;
 * exceed(t) = B > 1e-12*W^2 && A^2 > z_thr^2 * B.  z_thr is float32 in every scoring call (the
 * rolling and the stream ones): a binding that holds a float64 threshold rounds it to float32, and
 * z_thr^2 is the float64 square of that float32 value.   Outputs:
 *   z_last[p][m] = z at t = T-1 (0 if B <= 1e-12*W^2),   score[p] = max_m |z_last|,
 *   n_exceed[p]  = sum over m, t of exceed(t) (bit-exact vs oracle/krca_oracle.c),
 *   flags[p]     = KRCA_F_* of x[T-1][p][0] (CPU %) and x[T-1][p][1] (memory %) if M >= 2.
 * M must be a power of two <= 64.  Samples are expected finite (a missing sample is the caller's
 * to impute); a NaN / Inf never faults and gives what oracle/krca_oracle.c gives (tested).
 * Buffers: z_last [P][M], score / n_exceed / flags [P] fully written by every kernel form, no
 * initialisation needed; no workspace. */
int krca_rolling_score(const float* x, int64_t P, int32_t M, int32_t T, int32_t W, float z_thr,
                       float* z_last, float* score, int32_t* n_exceed, uint8_t* flags, void* stream);
/* which kernel krca_rolling_score launches for these sizes (host query, no device work):
 * KRCA_SCORE_PIPE software-pipelined chunks (the default), KRCA_SCORE_PIPE_ROWS the same with one
 * buffer descriptor per row (series counts past the 2^31-byte descriptor range),
 * KRCA_SCORE_RING plain loads (T <= W), KRCA_SCORE_REREAD any W.  The knob KRCA_SCORE_IMPL = 1 / 4
 * forces KRCA_SCORE_RING / KRCA_SCORE_PIPE_ROWS at T > W (how tests reach them at small shapes);
 * any other non-zero value behaves as 0.  The codes 2 and 5 belonged to removed kernels: retired,
 * not reused. */
#define KRCA_SCORE_PIPE 0
#define KRCA_SCORE_RING 1
#define KRCA_SCORE_REREAD 3
#define KRCA_SCORE_PIPE_ROWS 4
int krca_rolling_score_variant(int64_t P, int32_t M, int32_t T, int32_t W);

/* ---- a5t: anomaly timeline -- WHEN each pod went bad (new primitive; plugs in at
 * ref:agents/metrics_agent.py:44-47 beside krca_rolling_score).  One pass over x; z_last, score,
 * n_exceed and flags are bit-identical to krca_rolling_score on the same input.  Episodes, per
 * series s = p*M + m, over exceed(t) above for t in [W, T), with gap tolerance gap >= 0 and minimum
 * count min_count >= 1:
 *   an episode is a maximal run of exceedance steps with consecutive exceedances at most `gap`
 *   steps apart (t - last <= gap continues it, t - last > gap starts a new one); it records its
 *   first step (onset), its last step, its number of exceedances (cnt) and
 *   peak = max over its exceedances of (float)(fabs(A) / sqrt(B)) (float64, rounded to float32);
 *   it is sustained when cnt >= min_count.  The series keeps its sustained episode of the largest
 *   peak (the later one on equal peaks), or none.
 * Per pod, over its M series: the anchor is the series whose kept episode has the largest peak
 * (ties: lowest m); members are the series with a kept episode such that onset_m <= last_a + gap
 * and onset_a <= last_m + gap.   Outputs:
 *   onset[p] = min of the members' onsets,   last[p] = max of their last steps,
 *   count[p] = sum of their cnt,   peak[p] = the anchor's peak,
 *   lead[p] = the member with the smallest onset (ties: lowest m),   n_metrics[p] = members.
 * A pod with no kept episode (always when T <= W): onset = last = -1, count = 0, peak = 0,
 * lead = -1, n_metrics = 0.  A NaN sample never exceeds.  The software-pipelined kernels run
 * wherever krca_rolling_score runs them (KRCA_SCORE_PIPE / KRCA_SCORE_PIPE_ROWS), the re-reading
 * form everywhere else.
 * Buffers: the four scoring outputs and onset / last / count / peak / lead / n_metrics [P] are fully
 * written (a pod without an episode gets the values above), no initialisation needed; no workspace. */
int krca_rolling_timeline(const float* x, int64_t P, int32_t M, int32_t T, int32_t W, float z_thr,
                          int32_t gap, int32_t min_count,
                          float* z_last, float* score, int32_t* n_exceed, uint8_t* flags, /* as krca_rolling_score */
                          int32_t* onset /*[P]*/, int32_t* last /*[P]*/, int32_t* count /*[P]*/, float* peak /*[P]*/,
                          int8_t* lead /*[P]*/, uint8_t* n_metrics /*[P]*/, void* stream);

/* ---- a5s: level-shift score -- a sustained change of level against a robust baseline (new
 * primitive; stands beside krca_rolling_score, whose last-step z cannot see a fault that began
 * inside its own window).  x as krca_rolling_score reads it.  Per series s = p*M + m:
 *   baseline = the B samples at t in [T-R-G-B, T-R-G), recent = the R samples at t in [T-R, T);
 *   the G guard rows between them are not read.
 *   Order: the total order of the key k(x) = (bits & 0x80000000) ? ~bits : bits | 0x80000000,
 *   compared unsigned: -0 < +0, a positive-sign NaN above +Inf, a negative-sign NaN below -Inf.
 *   lmed(n values) = the element of 0-based rank (n-1)/2 in that order, with its own bits.
 *   base_med = lmed(baseline);  base_mad = lmed(fabsf(x_i - base_med)) over the baseline (float32
 *   subtraction, one rounding);  recent_med = lmed(recent);
 *   den = 1.4826 * (double)base_mad;  if (!(den > (double)min_scale)) den = min_scale;
 *   shift = den > 0 ? (float)(((double)recent_med - (double)base_med) / den) : 0.0f  (signed).
 * Per pod: score[p] = max over m of fabsf(shift) skipping NaN (all NaN: 0); lead[p] = the lowest m
 * that attains it when score > 0, else -1.
 * KRCA_EINVAL before any device work (nothing written): M no power of two <= 64, B outside
 * [2, krca_shift_max_baseline()], R outside [1, krca_shift_max_recent()], G < 0, B + G + R > T,
 * min_scale not finite or < 0, P < 0 or P*M >= 2^32.  P == 0 is a no-op success.
 * Samples are expected finite; a NaN / Inf never faults and gives NaN where tests/shift_ref.py gives
 * NaN and the same bits elsewhere.
 * Buffers: shift / base_med / base_mad / recent_med [P][M] and score / lead [P] are fully written, no
 * initialisation needed; no workspace; one kernel, no memset (safe for graph capture). */
int32_t krca_shift_max_baseline(void); /* 256 */
int32_t krca_shift_max_recent(void);   /* 64 */
int krca_shift_score(const float* x, int64_t P, int32_t M, int32_t T, int32_t B, int32_t R, int32_t G,
                     float min_scale,
                     float* shift /*[P][M]*/, float* base_med /*[P][M]*/, float* base_mad /*[P][M]*/,
                     float* recent_med /*[P][M]*/, float* score /*[P]*/, int8_t* lead /*[P]*/, void* stream);

/* ---- a5p: peer deviation score -- a pod against the other members of its group now (its replicas, the
 * pods of its node, the other nodes), not against its own past (new primitive; stands beside
 * krca_shift_score and reuses its order, lmed and scale).  v [P][M] is any per-pod statistic, usually
 * krca_shift_score's shift or recent_med.  Group g's members are member[grp_ptr[g] .. grp_ptr[g+1]); an id
 * outside [0, P) is ignored as if it were not listed; a pod listed twice, or in two groups, has
 * unspecified values but causes no out-of-bounds access.  Per (g, m) over the n valid members:
 *   grp_med = lmed(v);  grp_mad = lmed(fabsf(v_i - grp_med)) (float32 subtraction);  n == 0: both 0;
 *   den = 1.4826 * (double)grp_mad;  if (!(den > (double)min_scale)) den = min_scale;
 *   peer[p][m] = den > 0 ? (float)(((double)v - (double)grp_med) / den) : 0.0f;
 *   n < min_members: the medians are still written, the members' peer is 0 and grp_out is 0;
 *   grp_out = the number of members with fabsf(peer) > out_thr (a NaN does not count).
 * Per pod: score[p] = max over m of fabsf(peer) skipping NaN; lead[p] = the lowest m that attains it, or -1
 * when the score is 0.  A pod in no group: peer 0, score 0, lead -1.
 * KRCA_EINVAL before any device work (nothing written): M no power of two <= 64, min_members < 1, min_scale
 * or out_thr negative or not finite, P, G or n_member negative, P*M >= 2^32, G >= 2^32.  G == 0 is valid
 * (every pod gets the defaults); P == 0 is a no-op success.
 * Buffers: peer [P][M], score / lead [P], grp_med / grp_mad / grp_out [G][M] are fully written, no
 * initialisation needed; ws = krca_peer_ws_size(P, M, G, n_member) bytes, initialised by the call; no
 * memset by the caller, no device-to-host sync, no allocation (safe for graph capture); every output is
 * deterministic.  Groups of up to krca_peer_small_max() members take one wave each, up to
 * krca_peer_lds_cap() an LDS tile, larger ones the workspace (csrc/peer.hip). */
int32_t krca_peer_small_max(void); /* 64 */
int32_t krca_peer_lds_cap(void);   /* 4096 */
int64_t krca_peer_ws_size(int64_t P, int32_t M, int64_t G, int64_t n_member);
int krca_peer_score(const float* v /*[P][M]*/, int64_t P, int32_t M,
                    const int64_t* grp_ptr /*[G+1]*/, const int32_t* member /*[n_member]*/,
                    int64_t G, int64_t n_member,
                    int32_t min_members, float min_scale, float out_thr,
                    float* peer /*[P][M]*/, float* score /*[P]*/, int8_t* lead /*[P]*/,
                    float* grp_med /*[G][M]*/, float* grp_mad /*[G][M]*/, int32_t* grp_out /*[G][M]*/,
                    void* ws, void* stream);

/* Onset precedence over the pull-CSR (row k = the callers j of k, edges j -> k), single device, whole
 * graph; onset as krca_rolling_timeline writes it (< 0: none).  An edge j -> k with j != k,
 * onset_j >= 0 and onset_k >= 0 is classified, with slack >= 0:  k EARLIER than j when
 * onset_k + slack < onset_j,  k LATER when onset_j + slack < onset_k,  CONCURRENT otherwise.
 * Per caller j, over the rows j appears in: dep_earlier[j], dep_concurrent[j] = its earlier /
 * concurrent dependencies, dep_first[j] = min of ((int64)onset_k << 32) | k over its earlier
 * dependencies (INT64_MAX: none).  Per callee k: caller_later[k] (callers k is earlier than),
 * caller_concurrent[k], caller_earlier[k] (callers k is later than).  Pods with onset < 0 get zeros
 * and INT64_MAX.  Only the rows of pods with an onset are walked; integer counts and an integer min:
 * independent of the schedule.  ws: krca_rca_precede_ws_size(N) bytes, no initialisation needed;
 * every output is [N] and fully written.  Not for graph capture (memsets).
 * krca_rca_first_mover_key: a pod with onset >= 0 and dep_earlier == 0 is a first mover;
 * key = (min(caller_later + caller_concurrent, 2^20 - 1) << 32) | float bits of peak (peak >= 0:
 * monotone) for a first mover, 0 for every other pod; feed it to krca_topk_i64.
 * Buffers: ws = {pod list int32 [N] | counter}: the call zeroes the counter and reads only the list
 * entries it appended; the five counts are zeroed and dep_first set to INT64_MAX by the call before
 * the rows are walked; key [N] fully written.  None needs initialisation. */
int64_t krca_rca_precede_ws_size(int64_t N);
int krca_rca_precede(const int32_t* onset, int64_t N, int32_t slack, const int64_t* row_ptr, const int32_t* col,
                     int32_t* dep_earlier, int32_t* dep_concurrent, int64_t* dep_first,
                     int32_t* caller_later, int32_t* caller_concurrent, int32_t* caller_earlier,
                     void* ws, void* stream);
int krca_rca_first_mover_key(const int32_t* onset, const float* peak, const int32_t* dep_earlier,
                             const int32_t* caller_later, const int32_t* caller_concurrent, int64_t N,
                             int64_t* key, void* stream);

/* ---- a11/a12: 13-category log histograms (ref:agents/logs_agent.py:124-181) ----------------
 * text = UTF-8 bytes of D container logs, container d = text[doc_off[d], doc_off[d+1]).
 * Contract: doc_off[0] == 0, doc_off[D] == nbytes, doc_off non-decreasing, each container valid
 * UTF-8 on its own (the host wrappers check the offsets; off-contract offsets are clamped on the
 * device so they cannot fault, but the results are then unspecified).
 * Lines are str.splitlines() lines; a line is in category c iff
 * re.search(pattern_c, line, re.IGNORECASE) (compiled DFA, csrc/log_dfa_tables.h).
 * krca_log_scan below is the one-call protocol.  The two-call protocol (the line count is
 * data-dependent), which a caller may use on its own and which finishes a krca_log_scan whose line
 * arrays were too small:
 *   krca_log_index: per-chunk line-start counts + scan into block_base (workspace of
 *                   krca_log_index_size(nbytes) int64) and *n_lines (device int64).
 *   krca_log_match: (same workspace; it also keeps the first line id of every 256-byte chunk
 *                   there) per line start/end byte offsets and 13-bit mask; per container the line
 *                   count and the 13-bin histogram — atomics-free segmented reduction.  The first
 *                   three matching lines per bin (the reference's evidence, :159-163) are marked in
 *                   the line masks: bit 16 + c of line_mask[l] is set iff line l is one of the first
 *                   three lines of its container in category c (bits 0-12: the categories).
 *                   examples (nullable) additionally receives them as a dense id table
 *                   [D][13][3] (-1 when fewer).
 * Buffers: the workspace (krca_log_index_size(nbytes) int64) needs no initialisation by the caller:
 *   krca_log_index and krca_log_scan write every chunk count, chunk base and tile base, the
 *   chunk -> container map of every chunk that holds a text byte (the only ones read), and zero the
 *   look-back status words, the tile ticket and the long-line count themselves; the long-line queue is
 *   read up to the count appended.  krca_log_match reads the index one of those two calls left in the
 *   SAME workspace: it must not be touched in between.  *n_lines (device) is written by
 *   krca_log_index.  line_start / line_end / line_mask [0, n_lines) and doc_lines, hist, examples,
 *   doc_line0 [D] are fully written; krca_log_scan leaves the line arrays past the line count (and all
 *   of them when *n_lines_host > line_cap) as they were.  No output needs initialisation. */
/* The compiled matcher's identity: the Unicode version of the interpreter that generated the
 * tables (re.IGNORECASE folds, \d, str.splitlines separators; non-ASCII text matches the
 * reference exactly only under that version) and gen_log_dfa.pattern_digest of the 13 patterns
 * (krca/agents/logs.py refuses an edited LogsAgent.error_patterns that no longer matches it). */
const char* krca_log_dfa_unicode(void);
uint64_t krca_log_dfa_digest(void);
int64_t krca_log_index_size(int64_t nbytes);
int krca_log_index(const uint8_t* text, int64_t nbytes, const int64_t* doc_off, int64_t ndocs,
                   int64_t* workspace, int64_t* n_lines, void* stream);
int krca_log_match(const uint8_t* text, int64_t nbytes, const int64_t* doc_off, int64_t ndocs,
                   int64_t* workspace, int64_t n_lines,
                   int64_t* line_start /*[L]*/, int64_t* line_end /*[L]*/, uint32_t* line_mask /*[L]*/,
                   int32_t* doc_lines /*[D]*/, int32_t* hist /*[D][13]*/, int32_t* examples /*[D][13][3], nullable*/,
                   int64_t* doc_line0 /*[D], nullable: first line id of each container*/, void* stream);
/* krca_log_scan: krca_log_index + krca_log_match in one call when the caller's line arrays hold
 * line_cap lines (the same loop, ref:agents/logs_agent.py:140-151): the line index is built in ONE
 * pass over the text (decoupled look-back for the line ids), the later kernels read the line count
 * on the device, and the stream is synchronised once, at the end, for *n_lines_host.  When
 * *n_lines_host > line_cap the outputs past the index are not valid: size the arrays and call
 * krca_log_match with the same workspace (the index is kept there). */
int krca_log_scan(const uint8_t* text, int64_t nbytes, const int64_t* doc_off, int64_t ndocs,
                  int64_t* workspace, int64_t line_cap,
                  int64_t* line_start /*[line_cap]*/, int64_t* line_end /*[line_cap]*/, uint32_t* line_mask /*[line_cap]*/,
                  int32_t* doc_lines /*[D]*/, int32_t* hist /*[D][13]*/, int32_t* examples /*[D][13][3], nullable*/,
                  int64_t* doc_line0 /*[D], nullable*/, int64_t* n_lines_host, void* stream);

/* ---- a11/a12 with pattern tables compiled at run time -------------------------------------------
 * The calls above match the 13 patterns compiled into the library.  These match any pattern set the
 * host compiler (krca/logdfa.py compile_patterns) accepts: same text / doc_off contract, same lines,
 * same line_mask layout (bits 0..ncat-1 the categories, bits 16..16+ncat-1 the example marks), with
 * hist [D][ncat] and examples [D][ncat][3] strided by the tables' ncat.
 *
 * Pattern subset: every regex expands to a finite set of alternatives of single-code-point atoms
 * (literals, '.', \d \D \w \W \s \S, bracket classes; {n}, {m,n}, ? on one atom), fixed-length by
 * default.  compile_patterns(..., unbounded=True) also takes * + {m,} {,} on one atom (x{m,} is m
 * copies of x and a loop item on x); quantifiers on a group, lazy / possessive forms, anchors, \b,
 * nested groups, back-references, look-around, inline flags and alternatives that can match the
 * empty string stay refused.  The tables are one product DFA: a \d+-style loop is nearly free, each
 * ".*" between literals roughly doubles the states (one fits beside the 13 shipped patterns, two
 * pass KRCA_LOG_MAX_NSTATE).
 *
 * Long lines (over 1 KiB) take a wave per line, 64 segments.  log_dfa_long starts each segment
 * from the start state after a warm-up of `warm` code points (the longest alternative minus one):
 * exact only when no match is longer than warm + 1 code points, i.e. for fixed-length sets.  Tables
 * with KRCA_LOG_FLAG_CARRY (bit 0 of the header's flag word; the compiler sets it for a set with
 * loop items) take its carrying form instead: after the same speculative pass each lane compares
 * its entry state with its predecessor's exit state, and the lanes that differ re-walk their
 * segment from it, until a wave-wide vote finds no difference.  After round r lanes 0..r are final,
 * so at most 63 rounds and the result is exact for every DFA; `warm` (loops at their minimum, at
 * most 63) is only the speculation's warm-up.  Worst case (a state that survives every boundary,
 * "error.*" seen in the first segment): one serial walk of the line.  No workspace, no atomics; the
 * walk of lines up to 1 KiB (a lane per line from its first byte) is the same for both.
 *
 * Table image (host memory, little-endian, version 1):
 *   offset  0  uint32 magic = KRCA_LOG_IMAGE_MAGIC, version = KRCA_LOG_IMAGE_VERSION,
 *              ncat, nsym, nstate, nrange, warm, other   (eight uint32)
 *          32  uint64 digest (patterns.pattern_digest of the (name, regex) pairs)
 *          40  uint32 nbytes (the whole image), uint32 flags (KRCA_LOG_FLAG_CARRY or 0)
 *          48  uint8  ascii_sym[128]        symbol of each ASCII code point, KRCA_LOG_SYM_SEP for a separator
 *         176  uint32 ranges[nrange][3]     {lo, hi, symbol}: non-ASCII code points, every other one -> `other`
 *              uint16 trans[nstate * nsym]  target state of (state, symbol); state 0 is the start state
 *              uint16 out[nstate]           category mask reported on entering the state
 *              zero padding to a multiple of 8 bytes
 * Limits: 1 <= ncat <= 16, 1 <= nsym <= 63, 1 <= nstate <= 1024, nrange <= 1024, warm <= 63.
 *
 * krca_log_tables_check (host only, no GPU needed): validates an image -- magic, version, sizes, the
 *   limits, every transition < nstate, every mask < 1 << ncat, ranges sorted, disjoint, lo <= hi, above
 *   0x7F and below 0x110000, every symbol < nsym (or KRCA_LOG_SYM_SEP), other < nsym and no flag bit
 *   but KRCA_LOG_FLAG_CARRY -- and fills *dims (nullable; dims->flags reports the flag word).  KRCA_EINVAL with krca_last_error() naming the field otherwise.
 * krca_log_tables_dev_size (host only): bytes of the device form for these dimensions (0 when they
 *   break a limit).  The device form is the walk kernels' LDS layout, copied as it is: 16-bit entries
 *   (target state | 0x8000 when the target reports a category; category masks are read from out[]
 *   on flagged entries only) in rows of 32 columns (nsym <= 31) or 64, the last column the identity
 *   for bytes outside the line and UTF-8 continuation bytes; out[]; the byte -> symbol table; ranges.
 *   16-bit entries hold every set inside the limits in one form (1024 states x 64 columns = 128 KiB
 *   of the CU's 160 KiB; 32-bit entries carrying the masks stop at 640 states of 64 columns) and keep
 *   the 13 shipped patterns at 25 KB where the compiled walk's 32-bit table takes 49 KB.
 * krca_log_tables_upload: validates the image first (nothing is written when it fails), then writes the
 *   device form to tables_dev [tables_dev_bytes >= krca_log_tables_dev_size] on `stream` and
 *   synchronises it; *dims receives the dimensions the scan calls take.
 * krca_log_scan_tables / krca_log_match_tables mirror krca_log_scan / krca_log_match (same workspace:
 *   krca_log_index_size; krca_log_index is pattern-independent and serves both).  They re-check *dims
 *   against the limits and tables_dev_bytes against the device form's size, ask the runtime how much
 *   LDS a launch may take (opting in above the default), and fail with KRCA_EINVAL before any launch
 *   when the table cannot be launched.  The kernels sanitise what they copy into LDS (targets clamped
 *   to nstate - 1, symbols to the row width, masks to ncat bits), so a corrupted device form gives
 *   wrong masks but never an index outside the LDS allocation.
 *   KRCA_LOG_FUSED does not apply to these calls: they always run the two-pass path (line index, then
 *   the walk).
 * Buffers: as krca_log_scan / krca_log_match -- the workspace and every output need no initialisation;
 *   line arrays [0, n_lines), doc_lines / doc_line0 [D], hist [D][ncat], examples [D][ncat][3] fully
 *   written; nbytes == 0 (text may be null) writes zeros (examples -1) and launches no kernel that
 *   reads text.  tables_dev is read only. */
#define KRCA_LOG_IMAGE_MAGIC 0x544C524Bu /* "KRLT" */
#define KRCA_LOG_IMAGE_VERSION 1u
#define KRCA_LOG_SYM_SEP 0xFFu
#define KRCA_LOG_MAX_NCAT 16
#define KRCA_LOG_MAX_NSYM 63
#define KRCA_LOG_MAX_NSTATE 1024
#define KRCA_LOG_MAX_NRANGE 1024
#define KRCA_LOG_MAX_WARM 63
#define KRCA_LOG_FLAG_CARRY 1u /* long lines: carry the state from segment to segment */
typedef struct krca_log_dims {
  int32_t ncat, nsym, nstate, nrange, warm, other;
  uint64_t digest;
  uint32_t flags; /* the image's flag word (trailing: the fields above keep their offsets) */
} krca_log_dims;
int krca_log_tables_check(const void* image_host, int64_t image_bytes, krca_log_dims* dims_host /*nullable*/);
int64_t krca_log_tables_dev_size(const krca_log_dims* dims_host);
int krca_log_tables_upload(const void* image_host, int64_t image_bytes, void* tables_dev, int64_t tables_dev_bytes,
                           krca_log_dims* dims_host, void* stream);
int krca_log_match_tables(const uint8_t* text, int64_t nbytes, const int64_t* doc_off, int64_t ndocs,
                          int64_t* workspace, const void* tables_dev, int64_t tables_dev_bytes,
                          const krca_log_dims* dims_host, int64_t n_lines,
                          int64_t* line_start /*[L]*/, int64_t* line_end /*[L]*/, uint32_t* line_mask /*[L]*/,
                          int32_t* doc_lines /*[D]*/, int32_t* hist /*[D][ncat]*/,
                          int32_t* examples /*[D][ncat][3], nullable*/, int64_t* doc_line0 /*[D], nullable*/,
                          void* stream);
int krca_log_scan_tables(const uint8_t* text, int64_t nbytes, const int64_t* doc_off, int64_t ndocs,
                         int64_t* workspace, const void* tables_dev, int64_t tables_dev_bytes,
                         const krca_log_dims* dims_host, int64_t line_cap,
                         int64_t* line_start /*[line_cap]*/, int64_t* line_end /*[line_cap]*/,
                         uint32_t* line_mask /*[line_cap]*/, int32_t* doc_lines /*[D]*/, int32_t* hist /*[D][ncat]*/,
                         int32_t* examples /*[D][ncat][3], nullable*/, int64_t* doc_line0 /*[D], nullable*/,
                         int64_t* n_lines_host, void* stream);

/* ---- a13: error-template hashing + per-container template histograms (new primitive) ------
 * template(line) = line bytes with every maximal [A-Za-z0-9_] run that contains an ASCII digit or
 * is >= 8 hex digits long replaced by the one byte 0xFF (shown as "<*>"; never in UTF-8 text);
 * hash = FNV-1a-64(template) (csrc/template.hip).
 * krca_template_hash: hash[l] for every line [line_start[l], line_end[l]) (krca_log_match's lines;
 *   fastest when the starts ascend, as there: a workgroup reads its lines through one window from
 *   its first line's start; lines outside that window are read directly, same hash).
 * krca_template_hist: per container d, the distinct hashes of its lines in ascending order and
 *   their counts, written to out_hash/out_count at the container's own line range
 *   [doc_line0[d], doc_line0[d] + n_templates[d]), then 0 in the slots up to doc_line0[d] + doc_lines[d]
 *   (every slot of the line range is written; those of containers above krca_template_max_lines()
 *   by krca_template_hist_huge).  Sort-based.  Containers of <= 8 lines are sorted
 *   in one lane's registers, <= 64 by a wave, <= krca_template_max_lines() by a workgroup, all on
 *   device lists (no host round trip).  workspace: krca_template_hist_ws_size(ndocs) bytes, int32
 *   {mid, big, huge counts, 0 | mid list [D] | big list [D] | huge list [D]}: containers above
 *   krca_template_max_lines() lines are only LISTED (count at int32 [2], ids from int32 [4 + 2D]);
 *   the caller runs krca_template_hist_huge on each.
 * Buffers: hash [n_lines] fully written.  krca_template_hist zeroes its workspace's four counters
 *   and reads only the list entries it appended; it writes n_templates[d] of every container up to
 *   krca_template_max_lines() lines and every out_hash / out_count slot of their line ranges, and
 *   leaves n_templates[d] and the slots of the larger (listed) containers to krca_template_hist_huge.
 *   No initialisation needed for any of them. */
int krca_template_hash(const uint8_t* text, int64_t nbytes, const int64_t* line_start, const int64_t* line_end,
                       int64_t n_lines, uint64_t* hash, void* stream);
int64_t krca_template_hist_ws_size(int64_t ndocs);
int krca_template_hist(const uint64_t* hash, const int32_t* doc_lines, const int64_t* doc_line0, int64_t ndocs,
                       void* workspace, uint64_t* out_hash, int32_t* out_count, int32_t* n_templates, void* stream);
int32_t krca_template_max_lines(void);
/* containers with more than krca_template_max_lines() lines, one call each: the same output for
 * the container's n_lines hashes (hash, out_hash, out_count already offset to its doc_line0),
 * *n_templates set on the device; exact via a distinct-hash table + bucketed LDS sorts.
 * workspace: krca_template_huge_ws_size(n_lines) bytes, 16-byte aligned; *flag (device int32) = 1
 * if a bucket overflowed (then the output is incomplete and the caller must fail).
 * Buffers: the workspace's hash table, bucket counts and counters are initialised by the call, its
 * bucket offsets and sorted pairs written before they are read; every out_hash / out_count slot of
 * the n_lines, *n_templates and *flag are written.  No initialisation needed. */
int64_t krca_template_huge_ws_size(int64_t n_lines);
int krca_template_hist_huge(const uint64_t* hash, int64_t n_lines, void* workspace, uint64_t* out_hash,
                            int32_t* out_count, int32_t* n_templates, int32_t* flag, void* stream);

/* ---- a9: cross-pod Pearson correlation with per-pod top-k (new primitive; the
 * reference's only "correlation" is the string group-by of ref:agents/coordinator.py:118-155).
 * r(p,q) = Pearson over the T samples of metric channel `channel` of x[T][P][M] (population
 * std; a flat series correlates 0 with everything).  Per pod p: the k partners with the largest
 * |r| (self excluded, ties -> lower index) with r re-scored exactly (float64 over fp32 z), the
 * exact count of partners with |r| > tau (tau is float64, the type r is compared in: a float tau
 * of 0.6 would be 0.60000002 and miss pairs just above 0.6; the fp16 MFMA screening product decides every pair
 * farther than krca_corr_eps(T) from tau; the pairs within it are re-scored in float64: fails with
 * KRCA_EINVAL if more than 256*P + 2^20 pairs fall there, i.e. tau sits in the bulk of |r|), and
 * cert[p] > 0 iff the reported set is provably the exact top-k (pods whose first merge cannot
 * prove it have all their candidates re-scored; only a pod whose candidate buffer overflows twice
 * reports -1) (csrc/corr.hip).  Buffers: mean/scale [P]; z32 [P*T]; zh [krca_corr_pad_rows(P) *
 * krca_corr_pad_steps(T)] (fp16 bits); cand [krca_corr_cand_size(P, T, k) 4-byte words]; count [P];
 * out_idx/out_val [P*k]; cert [P].  k <= krca_corr_max_k(), 2 <= P <= 2^22.  krca_corr_topk
 * synchronises the stream once (it reads how many candidate buffers overflowed to decide on the
 * second pass).  The series must be finite: the certificates and the exact counts are proofs over
 * finite rows (a NaN row's products compare false everywhere; its results are unspecified).
 * Workspace size: cand holds the per-pod candidate buffers (krca_corr_cand_cap() = 4096 entries of
 * 8 bytes: 32 KiB per pod), the threshold sample's lists, the two ambiguous-pair lists of a
 * main-pass batch (capped per batch), their by-pod copy and the re-score's int16 partner rows (2
 * bytes per step per pod): at T = 1440, k = 10 krca_corr_cand_size gives 0.40 GB at 10k pods, 4.6 GB
 * at 100k, 46.2 GB at 1M.
 * Buffers: krca_corr_prepare writes mean / scale [P], z32 [P*T] and ALL of zh, its padding rows and
 * steps as zeros (krca_corr_topk's MFMA tiles read them): zh needs no initialisation.  cand needs
 * none either: krca_corr_topk zeroes the fill counts, list lengths and overflow / deep-pass counters,
 * presets the sample's partner ids (-1), the self products (1) and the second-pass thresholds, and
 * reads candidate, list and queue entries only up to the counts it appended; the re-score's rows
 * (error norms, int16 copies, projections) are written by the call for every pod before they are
 * read.  count [P] is zeroed by the call; out_idx / out_val [P*k] and cert [P] are fully written. */
int64_t krca_corr_pad_rows(int64_t P);
int32_t krca_corr_pad_steps(int32_t T);
int64_t krca_corr_cand_size(int64_t P, int32_t T, int32_t k);
int32_t krca_corr_max_k(void);
/* candidates buffered per pod by the main pass (cand's first [P][cap] int2 entries, then the [P] fill counts) */
int32_t krca_corr_cand_cap(void);
float krca_corr_eps(int32_t T);
int krca_corr_prepare(const float* x, int64_t P, int32_t M, int32_t T, int32_t channel, float* mean, float* scale,
                      float* z32, uint16_t* zh, void* stream);
int krca_corr_topk(const uint16_t* zh, const float* z32, int64_t P, int32_t T, int32_t k, double tau, void* cand,
                   int32_t* count, int32_t* out_idx, float* out_val, float* cert, void* stream);
/* Lead/lag correlation along dependency edges (csrc/corr_edges.hip), single device,
 * whole graph.  z float32 [N][T], pod-major, in the layout krca_corr_prepare writes as z32; the call
 * standardises nothing itself (krca_corr_prepare scales a row to unit NORM, so that a dot product is
 * r: for c_0 = r below, pass rows of unit variance, i.e. z32 times sqrt(T) -- the Python wrapper's
 * corr_unit_variance_device).  The pull-CSR as krca_rca_precede takes it: row k = the callers j of
 * k, edges j -> k.  L = max_lag, 0 <= L <= KRCA_CORR_MAX_LAG; tau >= 0; 0 <= slack <= L; mask uint8
 * [N] or NULL.  For the edge at CSR position e, in row k with j = col[e], and each l in [-L, L]:
 *   S_l = sum over t = max(0,-l) .. min(T, T-l) - 1  of  z[j][t+l] * z[k][t],      c_l = S_l / T
 * (empty overlap, |l| >= T: 0).  For standardised rows c_0 is Pearson r and |c_l| <= 1 (the biased
 * cross-correlation estimator); l > 0: the caller's series follows the dependency's by l steps.
 * The reference evaluates this in float64 over the float32 inputs; the device accumulates S_l in
 * float32 (fused multiply-adds) in a fixed order per edge with no float atomics -- two launches give
 * the same bits -- and finishes with one correctly rounded division, (float)((double)S / (double)T).
 * Per edge [E], fully written:  r0[e] = c_0;  lag[e] = the l of the largest |c_l| (compared as |S_l|),
 * visiting 0, +1, -1, +2, -2, ... and replacing only on strictly greater (ties: the smaller |l|, then
 * the positive l);  r_lag[e] = c_lag.  A self loop (j == k), an edge with mask[j] == 0 or
 * mask[k] == 0, or a column outside [0, N) gets r0 = r_lag = 0, lag = 0 and is not classified.
 * An edge is CORRELATED when fabsf(r_lag[e]) > tau (float32 compare of the stored value); a correlated
 * edge is DEP_LEADS when lag > slack, CALLER_LEADS when lag < -slack, SYNC otherwise.
 * Per caller j [N], over the rows j appears in: dep_lead[j], dep_sync[j] (counts), dep_best[j] = max
 * over j's DEP_LEADS edges of ((int64)bits(|r_lag|) << 32) | (uint32)(0x7FFFFFFF - k): the strongest
 * leading dependency, ties to the lower id; 0: none.  Per callee k [N]: caller_follow[k] (the
 * DEP_LEADS edges of row k), caller_sync[k], caller_lead[k].  Integer counts and an integer max:
 * independent of the schedule.  Rows of more than 512 callers are walked in 512-caller chunks by
 * separate waves.  T + 2 L <= 16384 (a wave keeps the dependency's row in LDS); 16-byte loads when
 * T % 4 == 0 and z is 16-byte aligned, 4-byte loads otherwise (same results).
 * krca_corr_lead_key: key = (min(caller_follow, 2^20 - 1) << 32) | float bits of score for a pod with
 * dep_lead == 0, caller_follow > 0 and score > 0 (a NaN score fails the compare), 0 for every other
 * pod; feed it to krca_topk_i64, as krca_rca_first_mover_key's.
 * Buffers: every output is fully written by the call: r0 / lag / r_lag [E] by the waves that walk the
 * edges (masked rows included), dep_lead / dep_sync / dep_best [N] zeroed by the call and then updated
 * with integer atomics, caller_* [N] stored for every row (chunks past the first add atomically
 * afterwards); key [N] fully written.  ws: krca_corr_edges_ws_size(N, E) bytes, 8-byte aligned, no
 * initialisation needed: {counter | chunk list}; the call zeroes the counter and reads only the list
 * entries it appended.  Not for graph capture (memsets). */
#define KRCA_CORR_MAX_LAG 16
int64_t krca_corr_edges_ws_size(int64_t N, int64_t E);
int krca_corr_edges(const float* z, int64_t N, int32_t T, const int64_t* row_ptr, const int32_t* col, int32_t max_lag,
                    float tau, int32_t slack, const uint8_t* mask /*[N] or NULL*/, float* r0 /*[E]*/,
                    int8_t* lag /*[E]*/, float* r_lag /*[E]*/, int32_t* dep_lead, int32_t* dep_sync, int64_t* dep_best,
                    int32_t* caller_follow, int32_t* caller_sync, int32_t* caller_lead, void* ws, void* stream);
int krca_corr_lead_key(const int32_t* dep_lead, const int32_t* caller_follow, const float* score, int64_t N,
                       int64_t* key, void* stream);
/* a9 pod-sharded (kubernetes-rca-system_amd/krca/corr_dist.py): rank g of G owns pods
 * [lo, lo + n_loc), lo a multiple of 256; zh / z32 / phi are the all-gathered full arrays.  The
 * upper triangle is split by super-tile (every G-th from g); candidates travel to their pod's
 * owner in one all-to-all of int4 {pod, partner, r bits, 0} entries; count and raw_cnt [P] are
 * all-reduced (sum) by the caller.  ws: krca_corr_shard_ws_size(P, T, k, n_loc, G) 4-byte words. */
int64_t krca_corr_shard_ws_size(int64_t P, int32_t T, int32_t k, int64_t n_loc, int32_t G);
int krca_corr_shard_sample(const uint16_t* zh, int64_t P, int32_t T, int32_t k, int64_t lo, int64_t n_loc,
                           int32_t G, void* ws, float* phi, void* stream);
int krca_corr_shard_tiles(const uint16_t* zh, const float* z32, int64_t P, int32_t T, int32_t k, double tau, int32_t G,
                          int32_t g, const float* phi, int64_t n_loc, void* ws, int32_t* count, int32_t* raw_cnt,
                          void* stream);
int krca_corr_shard_pack_sizes(int64_t P, int32_t T, int32_t k, int64_t n_loc, int32_t G, int64_t n_max, void* ws,
                               int64_t* tot_host /*[G], synchronous*/, void* stream);
int krca_corr_shard_pack(int64_t P, int32_t T, int32_t k, int64_t n_loc, int32_t G, int64_t n_max, void* ws,
                         void* send, void* stream);
int krca_corr_shard_unpack(int64_t P, int32_t T, int32_t k, int64_t n_loc, int32_t G, int64_t lo, void* ws,
                           const void* recv, int64_t n_recv, void* stream);
int krca_corr_shard_merge(const uint16_t* zh, const float* z32, int64_t P, int32_t T, int32_t k, double tau,
                          int64_t lo, int64_t n_loc, int32_t G, const float* phi, int32_t* lcnt, void* ws,
                          int32_t* out_idx, float* out_val, float* cert, void* stream);

/* ---- a10: personalized PageRank root-cause propagation (replaces the sink of
 * Coordinator._identify_root_causes, ref:agents/coordinator.py:157-184; networkx 3.4.2
 * pagerank semantics: dangling mass follows the personalization, L1 stop rule err < N*tol,
 * tol <= 0 = exactly max_iter iterations).  Pull-CSR: row i lists the sources j of edges j->i;
 * outdeg[j] = out-degree of j.  Personalization p_i ∝ max(seed_i - seed_floor, 0) (uniform if
 * all are at the floor).  Arithmetic is 2^-60 fixed point in int64: results do not depend on
 * summation order or GPU count and are bit-identical to oracle/krca_oracle.c.  The per-node edge
 * weight floor(r_j * alpha / outdeg_j) travels as a 32-bit code (26 significant bits + shift,
 * truncating; csrc/ppr.hip wenc/wdec, restated in the oracle), so the gathered table is 4 B/node.
 * The codes bound the reachable tolerance: each sweep carries ~2^-26 of the mass in truncation, so
 * a tol below ~2^-26 / N (e.g. 1e-9 on a 2-node cycle) is not met -- krca_ppr then fails with
 * KRCA_ENOTCONV as the oracle reports no convergence (networkx would raise
 * PowerIterationFailedConvergence at its own, float64, limit).  networkx's default 1e-6 is met at
 * every N.
 * krca_ppr runs the whole iteration on one device (synchronous: returns *iters_host; since round
 * 3 with the folded steps below, one kernel per iteration); the
 * krca_ppr_shard_* steps are the same kernels for G pod-sharded ranks.  Per iteration:
 * krca_ppr_shard_step (pull SpMV fused with the rank update: gathers w_all, writes r_local and
 * this rank's send slice of krca_ppr_slice_words(n_max) int64 words: [n_max uint32 weight codes,
 * padded to 8 bytes | krca_ppr_nslot() int64 partial-sum slots]), then the host exchange (G > 1:
 * RCCL all-gather of send into w_all[G][slice]; G = 1: swap of two
 * buffers, no copy), then krca_ppr_shard_reduce (kubernetes-rca-system_amd/krca/rca.py).
 * ctl: krca_ppr_ctl_size(n_local) bytes, zero-filled by the caller once (long-row accumulators
 * live there and reset themselves).
 * Buffers of krca_ppr: the workspace ({ctl | q [N] | two slices | r [N]}, krca_ppr_workspace_size(N)
 * bytes) needs no initialisation: the call zero-fills its ctl part and both slices' partial-sum
 * slots, the init writes q, r, the row coefficients and the first slice's codes, and each step
 * writes the codes of the slice it sends before the next step gathers them.  r_out, r_fixed and q_out
 * [N] are fully written.  The krca_ppr_shard_* calls leave the zeroing to their caller, as stated
 * above (ctl once) and below (the send slots). */
int32_t krca_ppr_nslot(void);
int64_t krca_ppr_slice_words(int64_t n_max); /* ceil(n_max / 2) + krca_ppr_nslot() */
int64_t krca_ppr_plan_size(const int64_t* row_ptr_host, int64_t N);
int krca_ppr_plan(const int64_t* row_ptr_host, int64_t N, int64_t* plan_host /*{rb,code,e0,e1} per block*/,
                  int64_t plan_len);
int64_t krca_ppr_workspace_size(int64_t N);
int krca_ppr(const int64_t* row_ptr, const int32_t* col /*pk*/, const int32_t* outdeg, int64_t N,
             const int64_t* plan, int64_t plan_len, const uint16_t* lane /*krca_ppr_pack*/, const float* seed,
             float seed_floor, double alpha, int32_t max_iter, double tol, void* workspace, float* r_out, int64_t* r_fixed /*nullable*/,
             int64_t* q_out /*nullable: quantised seeds*/, int32_t* iters_host, void* stream);
int64_t krca_ppr_ctl_size(int64_t n_local);
/* Host (no device work): the plan of krca_ppr_plan plus the packed column array pk_host[E]
 * (E = row_ptr_host[N]) the step kernel gathers through.  Columns are remapped to the exchange
 * layout in uint32 units (j + (j / n_max) * (2 * krca_ppr_slice_words(n_max) - n_max); n_max = N on
 * one device).  A short-row block whose distinct
 * columns are few enough becomes a DICTIONARY block: pk[e0, e0+nu) = its distinct columns
 * (ascending), then two uint16 slots per int32 word (16-byte aligned), one per edge; the plan
 * entry's first word carries nu in its high 32 bits (0 = direct block: pk[e] = column of edge e).
 * Each distinct column is gathered once per block instead of once per edge.  The DEVICE copy of
 * pk must have 64 zero words of padding past E (the step issues clamped 16-byte loads).  lane_host
 * [krca_ppr_lane_size(plan_len)] uint16: per block 2 x 256 words.  The block's non-empty rows get
 * consecutive sum slots 0, 1, ...; word t (lane t) = (slot of the row holding edge 8t) << 8 | the
 * bits of the edges 8t + 1 .. 8t + 7 that start a row, and word 256 + r = the slot of row rb + r
 * (256 for a row without edges), so the step's segmented row sums need neither a search nor the
 * row offsets.  Returns the number of dictionary blocks (>= 0) or a negative error (KRCA_EINVAL for a
 * column outside [0, N) or a remapped column id >= 2^30: the step addresses the gathered table at
 * 32-bit byte offsets).
 * (KRCA_PPR_DICT=0 packs every block direct; krca_ppr_remap_cols remaps a column array alone.) */
int64_t krca_ppr_lane_size(int64_t plan_len);
int64_t krca_ppr_pack(const int64_t* row_ptr_host, const int32_t* col_host, int64_t N, int64_t n_max,
                      int64_t* plan_host, int64_t plan_len, int32_t* pk_host, uint16_t* lane_host);
int krca_ppr_remap_cols(const int32_t* col, int64_t E, int64_t n_max, int32_t* out, void* stream);
/* p[0 .. n) = value by a kernel (not hipMemsetAsync): safe inside a HIP-graph capture whatever
 * the runtime's graph packet capture setting (the solve's zeroing uses kernels only) */
int krca_fill_i64(int64_t* p, int64_t n, int64_t value, void* stream);
/* Seeds are quantised to q = 2^32 per unit above seed_floor, clamped at 256 units (q <= 2^40; NaN
 * and values at or below the floor are 0), so the int64 seed total needs N <= 2^23 (KRCA_EINVAL
 * above). */
int krca_ppr_shard_init(const float* seed, float seed_floor, const int32_t* outdeg, int64_t n_local,
                        int64_t n_max, int64_t N, double alpha, void* ctl, int64_t* q_local,
                        int64_t* r_local, int64_t* send /*[krca_ppr_slice_words(n_max)]*/, void* stream);
int krca_ppr_shard_init_warm(const float* seed, float seed_floor, const int32_t* outdeg, int64_t n_local,
                             int64_t n_max, int64_t N, double alpha, void* ctl, int64_t* q_local,
                             const int64_t* r_local /*start vector: the previous solve*/, int64_t* send, void* stream);
/* flags of krca_ppr_shard_step: KRCA_PPR_RESIDUAL = accumulate |r_new - r_old| for the L1 stop
 * rule (reads r_local; needed when tol > 0), KRCA_PPR_WRITE_R = store r_new into r_local (every
 * iteration when tol > 0; a fixed-iteration solve needs it only on its last iteration). */
#define KRCA_PPR_RESIDUAL 1
#define KRCA_PPR_WRITE_R 2
int krca_ppr_shard_step(const int64_t* row_ptr, const int32_t* col /*pk*/, const int64_t* plan, int64_t plan_len,
                        const uint16_t* lane /*krca_ppr_pack*/, const int64_t* w_all /*[G][slice]*/, const int32_t* outdeg,
                        const int64_t* q_local, int64_t n_local, int64_t n_max, int64_t N, double alpha,
                        int32_t flags, int64_t* r_local, int64_t* send /*!= w_all*/, void* ctl, void* stream);
int krca_ppr_shard_reduce(const int64_t* w_all, int32_t G, int64_t n_max, int64_t N, double alpha,
                          double tol, int32_t first, void* ctl, int64_t* send_next, void* stream);
/* Folded iterations (the default of krca/rca.py): init (partial sums in slot set 0 of send; the
 * send slots and, at G = 1, the other buffer's must be zero before it), exchange, then per
 * iteration it = 1, 2, ...: krca_ppr_shard_step_folded + exchange, and krca_ppr_shard_finish(it =
 * the last) after the loop.  Step `it` does the reduction of step it - 1 itself (every workgroup
 * sums slot set (it - 1) % 3 of the G slices of w_all: convergence, teleport scale, iteration
 * count), adds its own partial sums into set it % 3 of send and zeroes set (it + 1) % 3 of
 * next_target, the buffer the NEXT step writes: at G = 1 the ping-pong buffer it gathers from
 * (w_all), at G > 1 the rank's send itself (the next step writes send again).  next_target is
 * send at G > 1; at G = 1 it is w_all when the exchange swaps the two buffers, or send when the
 * exchange copies send into w_all (a one-rank collective: krca.rca.Comm(collective=True)).  One
 * kernel and one exchange per iteration instead of two kernels; results bit-identical to the
 * unfolded sequence. */
int krca_ppr_shard_step_folded(const int64_t* row_ptr, const int32_t* col /*pk*/, const int64_t* plan, int64_t plan_len,
                               const uint16_t* lane, const int64_t* w_all, int32_t G, const int32_t* outdeg,
                               const int64_t* q_local, int64_t n_local, int64_t n_max, int64_t N, double alpha,
                               double tol, int32_t it, int32_t flags, int64_t* r_local, int64_t* send,
                               int64_t* next_target, void* ctl, void* stream);
int krca_ppr_shard_finish(const int64_t* w_all, int32_t G, int64_t n_max, int64_t N, double alpha, double tol,
                          int32_t it, void* ctl, void* stream);
/* Single device (G = 1, n_max = N): krca_ppr_shard_step with the iteration's krca_ppr_shard_reduce
 * (first = 0) done by the step's last workgroup — one launch per iteration instead of two.  Reads
 * the codes of w, writes r and send, zeroes w's partial-sum slots (w is the next step's write
 * target: the caller swaps w and send, exactly as around krca_ppr_shard_reduce). */
int krca_ppr_solo_step(const int64_t* row_ptr, const int32_t* col /*pk*/, const int64_t* plan, int64_t plan_len,
                       const uint16_t* lane, int64_t* w /*[slice(N)]*/, const int32_t* outdeg, const int64_t* q,
                       int64_t N, double alpha, int32_t flags, double tol, int64_t* r, int64_t* send /*!= w*/,
                       void* ctl, void* stream);
int krca_ppr_ctl_read(const void* ctl, int32_t* iters_host, int32_t* converged_host, void* stream);
/* the same two numbers without a synchronisation: enqueues their copy into host[0] = iteration at
 * convergence (0 = running), host[1] = iterations done; host should be pinned memory, read after
 * an event recorded behind it (the host's convergence polls then overlap the next iterations) */
int krca_ppr_ctl_copy(const void* ctl, int32_t* host /*[2]*/, void* stream);
int krca_ppr_fixed_to_float(const int64_t* r, int64_t n, float* out, void* stream);
/* root-cause key = bits of (double)r_i * (double)q_i: ranks pods by propagated mass times their
 * own anomaly; order-preserving as int64, fed to krca_topk_i64 (krca.rca.Config key "rq") */
int krca_ppr_rca_key(const int64_t* r, const int64_t* q, int64_t n, int64_t* key, void* stream);
/* The default root-cause key (krca.rca.Config key "explained"; the sink of
 * ref:agents/coordinator.py:157-184, edge direction of ref:agents/topology_agent.py:94-159: caller
 * -> dependency).  krca_rca_explain: over the WHOLE pull-CSR and the scores of every pod (score_all
 * [N]; q_j = the quantised seed of krca_ppr_shard_init), for each anomalous pod k A_k = its edges
 * from anomalous callers and S_k = the sum of their q; an anomalous dependency k of an anomalous pod
 * j (edge j -> k, j != k) explains j when (A_k - 1 >= A_j or q_k >= 2 q_j) and A_k q_j <= 3 S_k;
 * d_local[j - lo] = the largest q_k over the dependencies that explain j, for the pods [lo, hi) (0:
 * none).  Only anomalous pods' rows are walked; integer counts, sums and maxima, so bit-identical
 * to oracle/krca_oracle.c krco_rca_explain (S_k and A_k q_j in 128 bits: exact for any row).
 * ws: krca_rca_explain_ws_size(N) bytes, 16-byte aligned, no initialisation needed ({S int128 [N] |
 * A int32 [N] | pod list int32 [N] | counter}: the call zeroes the counter, reads only the list entries
 * it appended and A / S of listed pods, written before the scatter); d_local [hi - lo] is zeroed by
 * the call, then raised: fully defined.
 * krca_rca_key_explained: key_i = bits(((double)recv_i + (double)t_i / 32) * (double)u_i) with u_i =
 * q_i - d_i (0 when <= 0), t_i the row's teleport share in the solve's last step (from the scale the
 * step recorded in ctl) and recv_i = r_i - t_i, the mass the row received from its callers: the rows
 * and ctl of a finished krca_ppr_shard_* / krca_ppr solve, N = the mesh's node count. */
int64_t krca_rca_explain_ws_size(int64_t N);
int krca_rca_explain(const float* score_all, int64_t N, float seed_floor, const int64_t* row_ptr, const int32_t* col,
                     int64_t lo, int64_t hi, int64_t* d_local /*[hi - lo]*/, void* ws, void* stream);
int krca_rca_key_explained(const int64_t* r_local, const int64_t* q_local, const int64_t* d_local, int64_t n_local,
                           int64_t N, const void* ctl, int64_t* key, void* stream);

/* ---- top-k (descending value, ties -> lower index), float32 or int64 keys; NaN keys are never
 * selected: with fewer than k non-NaN keys the remaining slots are idx -1, val -inf / INT64_MIN.
 * Buffers: workspace (krca_topk_workspace_size(N, k) bytes) = the stage-1 candidates: every workgroup
 * writes its k (value, index) slots, sentinels included, before stage 2 reads them; idx / val [k]
 * fully written.  No initialisation needed. */
int64_t krca_topk_workspace_size(int64_t N, int32_t k);
int krca_topk_f32(const float* v, int64_t N, int32_t k, void* workspace, int32_t* idx, float* val,
                  void* stream);
int krca_topk_i64(const int64_t* v, int64_t N, int32_t k, void* workspace, int32_t* idx, int64_t* val,
                  void* stream);

/* ---- streaming rescoring (BASELINE configs[4]): krca_rolling_score carried
 * forward over a stream, delta new steps [delta][P][M] per call, global steps t0 .. t0+delta-1
 * (t0 == 0 starts the stream).  Outputs as krca_rolling_score over the whole series so far, with
 * n_exceed counted over the last H evaluated steps.  state: krca_stream_state_size bytes of plain
 * data (no pointers; set up by the t0 == 0 call): a copy to the host and back checkpoints the stream.
 * Buffers: state needs no initialisation before the t0 == 0 call: that call zeroes the exceedance
 * bits, ignores the stored sums and counts (it writes them at its end) and a ring row is written at
 * step t before step t + W reads it; later calls carry the state.  The last 64 bytes are spare and
 * never touched.  z_last [P][M], score / n_exceed / flags [P] fully written by every call. */
int64_t krca_stream_state_size(int64_t P, int32_t M, int32_t W, int32_t H);
int krca_stream_score(const float* x_new, int64_t P, int32_t M, int32_t delta, int64_t t0, int32_t W, int32_t H,
                      float z_thr, void* state, float* z_last, float* score, int32_t* n_exceed, uint8_t* flags,
                      void* stream);

/* ---- streaming anomaly timeline: krca_rolling_timeline carried forward over a stream, the episodes
 * of every series kept between calls.  exceed(t), z = (float)(fabs(A) / sqrt(B)), the episode fields
 * (onset, last, cnt, peak), gap, min_count and "sustained" are krca_rolling_timeline's.  New: the
 * state lives between calls, and an episode stops being reported H steps after its last exceedance
 * (the H that bounds n_exceed).  Per series, the state is the open episode (c_*) and the kept one
 * (k_*); with `now` the global step being processed:
 *   hit(t, z):   an open episode with t - c_last <= gap is extended (c_last = t, ++c_cnt, c_peak =
 *                max(c_peak, z)); otherwise close(t), then a new episode opens at t.
 *   close(now):  the open episode replaces the kept one when it is sustained and either the kept one
 *                is absent or expired (now - k_last >= H), or c_peak >= k_peak.
 *   view at the end of a call (now = t0 + delta - 1; it does not modify the state, the open episode
 *                stays open for the next call): the kept episode is valid when it exists and
 *                now - k_last < H; the open one is valid when it is sustained and now - c_last < H.
 *                The series reports the open one when it is valid and the kept one is invalid or
 *                c_peak >= k_peak; otherwise the kept one if valid; otherwise none.
 * Per pod, the M views are combined exactly as krca_rolling_timeline combines kept episodes (anchor,
 * members, the six outputs); onsets are global step indices.  Consequences: (1) while H exceeds the
 * number of steps so far nothing expires, and after every call the six outputs equal
 * krca_rolling_timeline over the whole series so far, bit for bit; (2) expiry is a function of
 * (last, now) only, so the outputs at step `now` do not depend on how the steps were split into calls.
 * state: krca_stream_score's rolling state (same layout, same size function); after each call its
 * defined bytes and z_last / score / n_exceed / flags are what krca_stream_score leaves for the same
 * input.  ep_state: krca_stream_episode_state_size bytes of plain data (no pointers; a copy to the
 * host and back checkpoints it), 4-byte aligned: 4-byte planes [8][S] over the series S = P*M --
 * c_on, c_last, c_cnt (int32), c_peak (float32), k_on, k_last, k_cnt (int32), k_peak (float32).
 * Rules for the caller: a stream uses this call from t0 == 0 on, with the same W, H, gap and
 * min_count every time; mixing it with krca_stream_score on the same state loses episodes (that call
 * advances the sums and sees no exceedance).  t0 + delta <= INT32_MAX (onsets are int32), gap >= 0,
 * min_count >= 1; P == 0 returns KRCA_OK.
 * Buffers: state as for krca_stream_score.  ep_state needs no initialisation before the t0 == 0 call:
 * that call ignores what it holds and every series stores its state at the end; a later call stores
 * only the series whose episodes changed.  The four scoring outputs and onset / last / count / peak /
 * lead / n_metrics [P] are fully written by every call (a pod that reports no episode: onset = last
 * = -1, count = 0, peak = 0, lead = -1, n_metrics = 0). */
int64_t krca_stream_episode_state_size(int64_t P, int32_t M);
int krca_stream_timeline(const float* x_new, int64_t P, int32_t M, int32_t delta, int64_t t0, int32_t W, int32_t H,
                         float z_thr, int32_t gap, int32_t min_count, void* state, void* ep_state,
                         float* z_last, float* score, int32_t* n_exceed, uint8_t* flags, /* as krca_stream_score */
                         int32_t* onset /*[P]*/, int32_t* last /*[P]*/, int32_t* count /*[P]*/, float* peak /*[P]*/,
                         int8_t* lead /*[P]*/, uint8_t* n_metrics /*[P]*/, void* stream);

/* ---- f3: betweenness centrality for the SPOF check (TopologyAgent._analyze_single_points_of_failure,
 * ref:agents/topology_agent.py:322-356, networkx 3.4.2 betweenness_centrality): Brandes over the
 * OUT-edge CSR (row u = successors of u), `batch` sources in flight (one workgroup each),
 * float64, normalized / directed as networkx.  ws: krca_betweenness_ws_size(N, batch) bytes.
 * Buffers: ws = {per-workgroup sigma, delta, dist, order, level offsets | dependency rows [batch][N]}:
 * the call sets dist = -1 and sigma = 0 everywhere and zeroes the dependency rows (re-zeroed after
 * each batch); delta, order and the level offsets are written per source before they are read.  bc [N]
 * is zeroed by the call, then accumulated.  No initialisation needed. */
int64_t krca_betweenness_ws_size(int64_t N, int32_t batch);
int krca_betweenness(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t normalized, int32_t directed,
                     int32_t batch, void* ws, double* bc, void* stream);

/* ---- f2: service-graph construction from Kubernetes objects (TopologyAgent._build_service_graph
 * ref:agents/topology_agent.py:94-160, _infer_dependencies_from_env :228-260; the same selector
 * test in ResourceAnalyzer._find_matching_pods ref:agents/resource_analyzer.py:835-854).
 * selector_match: bits[d * ceil(S/64) + s/64] bit s%64 = every item id of selector s occurs among
 *   the item ids of object d (ids interned by the host: krca/topograph.py); bit-exact.
 * substr_match: every (value v, key k) with key k occurring in value v (bytes), appended to
 *   out[cap] as v*K + k (once per occurrence, unordered); *n_out (device u64) = occurrences, may
 *   exceed cap.  lens = the distinct key lengths >= 1, ascending; table / hash from
 *   krca_substr_prepare (table_size = krca_substr_table_size(K) int32 slots).
 * Buffers: bits [D * ceil(S/64)] fully written.  krca_substr_prepare fills the table with -1 before
 *   inserting and writes hash [K]; krca_substr_match zeroes *n_out itself and writes out[0 ..
 *   min(*n_out, cap)), nothing past cap.  No initialisation needed. */
int krca_selector_match(const int32_t* lab, const int64_t* lab_off, int64_t D, const int32_t* sel,
                        const int64_t* sel_off, int64_t S, uint64_t* bits, void* stream);
int64_t krca_substr_table_size(int64_t K);
int krca_substr_prepare(const uint8_t* pat, const int64_t* pat_off, int64_t K, int32_t* table, int64_t table_size,
                        uint64_t* hash, void* stream);
int krca_substr_match(const uint8_t* text, const int64_t* val_off, int64_t V, const uint8_t* pat,
                      const int64_t* pat_off, int64_t K, const int32_t* table, int64_t table_size,
                      const uint64_t* hash, const int32_t* lens, int32_t n_lens, int64_t* out, int64_t cap,
                      uint64_t* n_out, void* stream);

/* ---- f1: pod status categorisation (ResourceAnalyzer._analyze_pods + _is_pod_healthy,
 * ref:agents/resource_analyzer.py:264-380, :856-895) over columnar pod status (encoding in
 * csrc/podstate.hip and krca/podstate.py): mask[p] bit b = membership of status group b in the
 * reference's dict order; hist[krca_pod_groups()] = group sizes.  Bit-exact.
 * Buffers: mask [P] fully written; hist zeroed by the call, then added into.  No initialisation needed. */
int32_t krca_pod_groups(void);
int krca_pod_classify(const uint8_t* pod_code, const int64_t* cont_off, const uint16_t* cont_code, int64_t P,
                      uint16_t* mask, int32_t* hist, void* stream);

/* ---- f4: group-bys of EventsAgent (ref:agents/events_agent.py:105-133 objects, :169-228 scheduling,
 * :230-290 volumes, :330-375 control plane, :377-446 nodes) and Coordinator._correlate_findings
 * (ref:agents/coordinator.py:118-155: group by component, max severity).  N membership records
 * (slot[i], key[i]); slots outside [0, S) are ignored; key < 0 = member that is not selected.
 * Output: one 8 x int64 record per slot, rec[s*8 + j]:
 *   j = 0      first member index (dict insertion order; INT32_MAX if the slot is empty)
 *   j = 1      (members << 32) | (members with key >= 0)
 *   j = 2 + r  r-th largest key >= 0 (-1 if none), r < R; ranks r >= 1 only over i < n_ranked.
 * Keys must be distinct within a slot for r >= 1 (the host packs (rank << 32) | (2^31-1-index)).
 * Bit-exact; 1 <= R <= krca_group_max_rank(), N < 2^31, 0 <= n_ranked <= N.
 * Buffers: rec [S][8]: all eight words of every slot are set by the call (INT32_MAX, 0, -1 ...)
 * before the records are reduced into them.  No initialisation needed; no workspace. */
int32_t krca_group_max_rank(void);
int krca_group_reduce(const int32_t* slot, const int64_t* key, int64_t N, int64_t n_ranked, int32_t S, int32_t R,
                      int64_t* rec, void* stream);

/* ---- t1: trace analytics from columnar spans.  The reference's TracesAgent emits canned findings
 * (ref:agents/traces_agent.py:209-381); the schemas computed here are the ones its data-access layer
 * serves (ref:utils/mock_k8s_client.py:1146-1311: get_service_latency_stats {p50, p90, p95, p99, count},
 * get_error_rate_by_service, get_service_dependencies, find_slow_operations).  One entry per span
 * (krca/tracecols.py): svc in [0, S), parent = index of the parent span in the table (-1 = root or
 * outside the window), dur_us, err (0 / 1).  All outputs are integers and bit-exact (integer add / max /
 * or only); N < 2^31.
 *
 * Buckets: log-linear, 32 per octave, krca_trace_nbuckets() = 896.  d < 64: b = d.  Otherwise
 * e = floor(log2 d), m = d >> (e-5) in [32, 63], b = 64 + (e-6)*32 + (m-32), lo(b) = m << (e-5),
 * hi(b) = ((m+1) << (e-5)) - 1: lo <= d <= hi, hi - lo < lo/32, hi(895) = 2^32 - 1.  The three bucket
 * helpers and krca_trace_lds_max_slots() are host functions without device work.
 *
 * krca_trace_link: a span is BAD if svc is outside [0, S): caller_svc = -1, self_us = 0, flags = 0, it
 *   contributes to nothing and is counted in the first int64 of ws.  A parent is VALID if
 *   0 <= parent[i] < N, parent[i] != i and the parent span is not bad; anything else is read as -1.
 *   caller_svc[i] = svc[parent[i]] if the parent is valid and its service differs from svc[i], else -1
 *   (a child span inside the same service is not a call);
 *   self_us[i] = max(dur_us[i] - sum of dur_us over the valid children, 0), summed in 64 bits;
 *   flags bit 0 = err, bit 1 = origin (errs and no valid child errs), bit 2 = propagated (errs, the
 *   valid parent errs and caller_svc >= 0).  ws: krca_trace_link_ws_size(N) bytes, zeroed by the call.
 * krca_trace_edges: the distinct keys caller*S + callee of the spans with caller_svc in [0, S) (and svc
 *   in [0, S)), ASCENDING in edge_key[0 .. *n_edges_host); edge_slot[i] = rank of span i's key or -1.
 *   SYNCHRONOUS (the distinct keys are ordered on the host inside the call).  If *n_edges_host > cap the
 *   value is a lower bound and edge_key / edge_slot are undefined: grow cap and call again (as
 *   krca_log_scan's line_cap).  ws: krca_trace_edge_ws_size(cap) bytes.
 * krca_trace_stats: records (slot, val, flags); slots outside [0, S) are ignored.
 *   rec[s] = {n, sum val, max val, n with bit 0, n with bit 1, n with bit 2, 0, 0}, hist[s][bucket(val)] += 1.
 *   accumulate == 0: outputs zeroed first; != 0: added into what is there (max for word 2), so windows
 *   or shards merge exactly.  S <= krca_trace_lds_max_slots(): LDS tables per workgroup; above: global
 *   atomics behind a per-wave fold and a per-workgroup LDS cache of the records (KRCA_TRACE_IMPL: 0 by
 *   size, 1 LDS, 2 folded + cached, 3 one atomic set per lane).  hist must be 8-byte aligned.
 * krca_trace_quantiles: nearest rank, k = (q*n + 999) / 1000 for q = permille_host[j] in [1, 1000],
 *   b* = first bucket whose cumulative count reaches k, out[s][j] = min(hi(b*), rec max), 0 where n = 0:
 *   never below the true quantile and less than 1/32 above it.  Q <= 16.
 * Buffers: krca_trace_link zeroes its whole workspace (above) and writes caller_svc / self_us / flags
 *   [N].  krca_trace_edges: ws = {8 counters | key table | rank table}: counters zeroed and the key
 *   table filled with -1 by the call, a rank written for every occupied slot before the lookup reads
 *   it; edge_key [0, *n_edges_host) and ALL of edge_slot [N] (-1 for a span that is no edge) are
 *   written when *n_edges_host <= cap, nothing past edge_key[cap - 1] ever.  krca_trace_stats:
 *   accumulate == 0 zeroes rec [S][8] and hist [S][NB] itself; accumulate != 0 adds into them, so the
 *   CALLER zeroes them before the first window.  krca_trace_quantiles writes out [S][Q] fully.
 *   Except for that accumulate form, no initialisation needed.
 *
 * krca_trace_critical: which of a span's microseconds its request was waiting for.  start_us (any common
 *   origin) adds the one input the calls above lack: span i occupies [s_i, e_i), e_i = s_i + dur_us[i], in
 *   64 bits.  A span is BAD if svc is outside [0, S) (as in link) or start_us outside [-2^62, 2^62): its
 *   outputs are 0, it is nobody's child and nobody's valid parent, and it is counted in the first int64
 *   of ws.  A parent is VALID as in link (in range, not the span itself, not bad); a span that is not bad
 *   and has no valid parent is a ROOT.
 *   Sweep of a span p over its valid children: child c is clipped to cs = max(s_c, s_p),
 *   ce = min(e_c, e_p); a child with ce <= cs is never selected.  cursor = e_p; among the children with
 *   ce <= cursor the one with the largest ce (ties: smallest cs, then lowest span index) is SELECTED,
 *   cursor = cs; repeat until no child qualifies (a child still running at the cursor was hidden behind
 *   the one chosen; every selection lowers the cursor, so no child is selected twice).
 *   A root is ON THE PATH.  A non-root is on the path iff for some k <= D = krca_trace_critical_max_depth()
 *   = 4096 its k-th valid ancestor is a root and the span and every ancestor below that root are
 *   SELECTED: parent cycles and spans deeper than D are off the path.
 *   path[i]: bit 0 = SELECTED, bit 1 = on the path, bit 2 = root.  crit_us[i] = dur_us[i] - sum of
 *   (ce - cs) over the SELECTED children if the span is on the path, else 0 (the pieces are disjoint and
 *   inside the span: no clamp).  Where every child's interval lies inside its parent's, the crit_us of a
 *   trace sum to its root's dur_us exactly; a child that overruns its parent keeps its full own time, so
 *   the sum then exceeds the root's duration.
 *   Parents with at most krca_trace_critical_small_max() children are swept by one lane each, heavier
 *   ones by one workgroup each: same bits.  Both helpers and krca_trace_critical_ws_size are host
 *   functions without device work.  No host synchronisation, no allocation.
 * Buffers: crit_us [N] and path [N] are written for every i.  ws: krca_trace_critical_ws_size(N) bytes,
 *   8-byte aligned = {8 counters | clipped child intervals | valid parent | child count | list cursor |
 *   child index | heavy parents | scan tile sums | selected}: counters and counts zeroed by the call,
 *   every other word written before it is read (the heavy list only up to its counter).  No
 *   initialisation needed. */
int32_t krca_trace_nbuckets(void);
int32_t krca_trace_bucket(uint32_t d);
int krca_trace_bucket_bounds(int32_t b, uint32_t* lo_host, uint32_t* hi_host);
int32_t krca_trace_lds_max_slots(void);
int64_t krca_trace_link_ws_size(int64_t N);
int krca_trace_link(const int32_t* svc, const int32_t* parent, const uint32_t* dur_us, const uint8_t* err, int64_t N,
                    int32_t S, int32_t* caller_svc, uint32_t* self_us, uint8_t* flags, void* ws, void* stream);
int64_t krca_trace_edge_ws_size(int64_t cap);
int krca_trace_edges(const int32_t* caller_svc, const int32_t* svc, int64_t N, int32_t S, int64_t cap, void* ws,
                     int64_t* edge_key, int32_t* edge_slot, int64_t* n_edges_host, void* stream);
int krca_trace_stats(const int32_t* slot, const uint32_t* val, const uint8_t* flags, int64_t N, int32_t S,
                     int32_t accumulate, int64_t* rec, uint32_t* hist, void* stream);
int krca_trace_quantiles(const int64_t* rec, const uint32_t* hist, int32_t S, const int32_t* permille_host, int32_t Q,
                         uint32_t* out, void* stream);
int32_t krca_trace_critical_max_depth(void);
int32_t krca_trace_critical_small_max(void);
int64_t krca_trace_critical_ws_size(int64_t N);
int krca_trace_critical(const int32_t* svc, const int32_t* parent, const int64_t* start_us, const uint32_t* dur_us,
                        int64_t N, int32_t S, uint32_t* crit_us, uint8_t* path, void* ws, void* stream);

/* ---- g1: structure of the dependency graph (replaces nx.simple_cycles and the all-pairs
 * nx.all_simple_paths search of TopologyAgent._analyze_service_dependencies,
 * ref:agents/topology_agent.py:262-320, and tracecols.first_cycle; csrc/graph_struct.hip).
 * The graph: row_ptr int64 [N + 1], col int32 [E = row_ptr[N]] and `pull`: 0 = row u lists the
 * successors of u (krca_betweenness's layout), 1 = row v lists the predecessors of v (krca_ppr's).
 * Every output is a function of the edge set {u -> v} alone: the same graph in either layout, with its
 * rows in any order, gives identical bytes.  Duplicate edges and self-loops are legal.  A col entry
 * outside [0, N) is no edge: it is never used as an index and is counted in n_bad_edges.
 * 0 <= N <= 2^31 - 2 and pull in {0, 1}, else KRCA_EINVAL before any device work; N == 0 returns the
 * empty stats without touching a pointer.  The three calls SYNCHRONISE the stream (as krca_trace_edges):
 * their rounds are plain launches on `stream` driven from the host, which reads a "changed" word back
 * after each batch; every such loop gives up after N + 2 rounds with KRCA_ENOTCONV.  rounds_host
 * (nullable) receives the rounds run.  The size functions are host functions without device work.
 *
 * krca_graph_scc:  comp[v] = the smallest node id of v's strongly connected component;
 *   flags[v]: bit 0 = the component is cyclic (two or more nodes, or a self-loop), bit 1 = v has a
 *   self-loop, bit 2 = v is the representative (comp[v] == v);
 *   stats_host[6] = {n_components, n_cyclic (components), n_cyclic_nodes, largest_size,
 *   first_cyclic_label (the smallest; -1: none), n_bad_edges};
 *   rounds_host[4] = {colouring passes, trim rounds, colouring rounds, reachability rounds}.
 * krca_graph_chain: comp as krca_graph_scc wrote it.  Over the condensation (one node per component,
 *   the edges between different components):  depth_dn[v] = components on the longest chain that starts
 *   at v's component and follows edges forward (1 at a sink), depth_up[v] the same following edges
 *   backward, next[v] = the label of the forward neighbour component with depth_dn one less (ties: the
 *   smallest label; -1 at a sink), the same for every node of a component;
 *   stats_host[2] = {longest = max depth_dn (0 when N = 0), start = the smallest label that attains it
 *   (-1 when N = 0)}; rounds_host[1].  On an acyclic graph `longest` is the node count of the longest
 *   simple path; on a cyclic graph it is a LOWER BOUND of it (the longest simple path is NP-hard there).
 *   A comp that is no component labelling (a label outside [0, N), or labels whose condensation has a
 *   cycle) never faults: KRCA_EINVAL, outputs unspecified.
 * krca_graph_cycle: with d(v) = the BFS distance from v to `root` along edges, for the nodes of root's
 *   component:  hop[v] = the smallest-id successor w of v in the component with d(w) = d(v) - 1 for
 *   v != root;  hop[root] = the successor w of root in the component with the smallest d(w) (ties: the
 *   smallest id; root itself when it has a self-loop), -1 when the component is not cyclic;  hop = -1
 *   outside the component.  root, hop[root], hop[hop[root]], ... back to root is a shortest cycle
 *   through root.  0 <= root < N; rounds_host[1].
 * Buffers: comp / flags [N], depth_dn / depth_up / next [N] and hop [N] are fully written, no
 *   initialisation needed.  ws (krca_graph_scc_ws_size / _chain_ws_size / _cycle_ws_size (N) bytes,
 *   8-byte aligned) needs none either: each call zeroes the control words it reads back and its
 *   accumulators, and writes every per-node word (krca_graph_scc: colour and mark, later the label
 *   minimum and size; krca_graph_chain: the two depths and next per label; krca_graph_cycle: distance
 *   and hop key) for all N nodes before a round reads it.  Not for graph capture (memsets, read-backs). */
int64_t krca_graph_scc_ws_size(int64_t N);
int64_t krca_graph_chain_ws_size(int64_t N);
int64_t krca_graph_cycle_ws_size(int64_t N);
int krca_graph_scc(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, void* ws, int32_t* comp /*[N]*/,
                   uint8_t* flags /*[N]*/, int64_t* stats_host /*[6]*/, int32_t* rounds_host /*[4], nullable*/,
                   void* stream);
int krca_graph_chain(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, const int32_t* comp, void* ws,
                     int32_t* depth_dn /*[N]*/, int32_t* depth_up /*[N]*/, int32_t* next /*[N]*/,
                     int64_t* stats_host /*[2]*/, int32_t* rounds_host /*[1], nullable*/, void* stream);
int krca_graph_cycle(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, const int32_t* comp,
                     int64_t root, void* ws, int32_t* hop /*[N]*/, int32_t* rounds_host /*[1], nullable*/, void* stream);

/* ---- g1: blast radius of up to 64 sources (the ranked root causes): multi-source reachability over
 * the dependency graph and the greedy cover of the marked (anomalous) nodes by the sources' radii
 * (csrc/graph_reach.hip; a caller of the reference could only run nx.ancestors per
 * candidate on the host).  Graph arguments and `pull` as krca_graph_scc: either layout, duplicate
 * edges and self-loops legal, a col entry outside [0, N) is no edge and never used as an index.
 * dir: KRCA_REACH_DEPENDENTS = bits flow against the edges (who transitively calls the source),
 * KRCA_REACH_DEPENDENCIES = along them (what the source transitively calls).
 * KRCA_EINVAL before any device work: K outside [1, 64], H outside [2, 64], dir or pull outside {0, 1},
 * a src_host[k] outside [0, N), N > 2^31 - 2, and N == 0 (no source can be valid).  Duplicate sources
 * are legal: each gets its own bit and identical results.  mark (uint8 [N], device) == NULL means every
 * node is marked, in both calls.  Both calls SYNCHRONISE the stream: the levels (and the cover's
 * steps) are plain launches driven from the host, which reads a "changed" word per level (64 counters
 * per step) back; the level loop gives up after N + 2 rounds with KRCA_ENOTCONV.
 *
 * krca_graph_reach: with d_k(v) = the BFS distance from src[k] to v in direction dir (0 at the source;
 *   infinite when v is unreachable, or beyond max_hops when max_hops > 0; max_hops <= 0 = unbounded):
 *   reach[v] bit k = d_k(v) is finite, bits K..63 are 0;
 *   hist_host[0][k][h] = the nodes with d_k = h for h < H - 1, the last bin (h = H - 1) the nodes with
 *   finite d_k >= H - 1;  hist_host[1][k][h] = the same over the nodes with mark != 0;
 *   depth_host[k] = the largest finite d_k;  rounds_host[1] (nullable) = the levels run (informational).
 *   Every output is a function of the edge set, the sources and mark alone: either layout, any row
 *   order, and dir swapped together with the transposed arrays give identical bytes.
 * krca_graph_reach_cover: greedy set cover of the marked nodes by the sources' radii.  Step j picks the
 *   k with the largest gain = the marked v that have bit k of reach[v] and no previously chosen bit
 *   (ties: the lowest k) and stops when the largest gain is 0:  order_host[j], gain_host[j] = the pick
 *   and its gain, unused slots -1 and 0;  exclusive_host[k] = the marked v with reach[v] == 1 << k;
 *   totals_host[2] = {marked nodes, marked nodes with reach != 0}.  Bits K..63 of reach are ignored.
 *   One count launch and one read-back per step.
 * Buffers: reach [N] is fully written by krca_graph_reach (it is the BFS's "seen" word).  ws
 *   (krca_graph_reach_ws_size(N) bytes, 8-byte aligned, for both calls) needs no initialisation: each
 *   call zeroes the control words, histogram bins and counters it reads back, and krca_graph_reach
 *   writes both per-node frontier words for all N nodes before a level reads them.
 *   Not for graph capture (memsets, read-backs). */
#define KRCA_REACH_MAX_SRC 64
#define KRCA_REACH_DEPENDENTS 0
#define KRCA_REACH_DEPENDENCIES 1
int64_t krca_graph_reach_ws_size(int64_t N);
int krca_graph_reach(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull,
                     const int32_t* src_host /*[K]*/, int32_t K, int32_t dir, int32_t max_hops,
                     const uint8_t* mark /*[N] device, nullable*/, int32_t H, void* ws,
                     uint64_t* reach /*[N] device*/, int64_t* hist_host /*[2][K][H]*/,
                     int32_t* depth_host /*[K]*/, int32_t* rounds_host /*[1], nullable*/, void* stream);
int krca_graph_reach_cover(const uint64_t* reach, const uint8_t* mark /*nullable*/, int64_t N, int32_t K,
                           void* ws, int32_t* order_host /*[K]*/, int64_t* gain_host /*[K]*/,
                           int64_t* exclusive_host /*[K]*/, int64_t* totals_host /*[2]*/, void* stream);

/* ---- a13b: log-template novelty across windows (csrc/template_novelty.hip, csrc/tmpl_novelty_layout.h,
 * DESIGN.md §3.18; the reference keeps no log state between two analyses).  A device-resident table maps
 * the exact key (group int32 >= 0, template hash uint64) to the record {first_win, last_win, n_win,
 * total int64}; a record with n_win == 0 is absent.  tests/template_novelty_ref.py restates the
 * semantics on the host; every quantity is an integer and the device equals it bit for bit.
 *
 * One window w (the caller passes strictly increasing windows): the entries are, for every container d
 * of [0, ndocs) with group[d] >= 0 (group == NULL: every container in group 0) and j < n_templates[d],
 * the triple (group[d], tmpl_hash[doc_line0[d] + j], tmpl_count[doc_line0[d] + j]) as krca_template_hist
 * left them (after krca_template_hist_huge); an entry with count <= 0, or whose slot lies outside
 * [0, n_lines), is skipped and its slot never read.  A hash equal to the table's empty marker (2^64 - 1)
 * is counted under 2^64 - 2.  Per key: cur_lines = the sum of the counts, cur_docs = the entries
 * showing it (the containers: krca_template_hist lists a hash once per container; arrays that list one
 * twice count it twice), first_doc = the lowest such d.  cur_lines and cur_docs share one 64-bit word
 * (40 + 24 bits): a key whose counts sum to 2^40 or more in one window is outside the contract -- its
 * record and report are then UNDEFINED (never a fault); 2^40 lines exceed any window's n_lines here.  With `absent` = n_win == 0, or ttl > 0 and
 * last_win < w - ttl (the history is then discarded; ttl == 0 never expires):
 *   NOVEL (flag 1): absent;   SURGE (flag 2): present, cur_lines >= surge_min and
 *   cur_lines * (w - first_win) >= surge_ratio * total (exact 128-bit products, total before w).
 * Commit: first_win = w if absent, last_win = w, n_win = 1 if absent else n_win + 1, total (0 if absent)
 * += cur_lines.  report == 0 commits and flags nothing (n_novel = n_surge = n_reported = 0, doc_* = 0).
 *
 * counts_host[6] = {n_entries, n_keys_touched, n_novel, n_surge, n_reported, n_live_slots (records
 *   with n_win > 0 in the table, those whose ttl ran out untouched included)}; read back synchronously
 *   (the call SYNCHRONISES the stream once, as krca_log_scan).
 * report_out: cap records of 48 bytes {uint64 hash, int64 total_before, int64 cur_lines, int32 group,
 *   flags, cur_docs, first_doc, first_win (w when novel), pad}, one per NOVEL or SURGE key in any order;
 *   min(n_reported, cap) are written, all distinct; the counts stay exact beyond cap.
 * doc_novel / doc_surge (int32 [ndocs], each nullable): the container's entries whose key is NOVEL /
 *   SURGE this window; every element written.
 * KRCA_ENOMEM: a key found no slot.  The records are then exactly those before the call (slots claimed
 *   by the failed window stay behind as absent records); rehash into a larger table and repeat.
 * krca_template_novelty_rehash: new_state (krca_template_novelty_state_size(new_capacity) bytes, needs
 *   no initialisation, must not overlap old_state) receives every record with n_win > 0 and
 *   last_win >= min_last_window; KRCA_ENOMEM when they do not fit.  Synchronises.
 * KRCA_EINVAL before any device work: a capacity that is no power of two in [64, 2^30]; negative ndocs,
 *   n_lines, window, ttl or cap; ndocs > 2^24 - 1; surge_ratio < 1 or surge_min < 1; report != 0 with
 *   cap > 0 and a null report_out; a null state or counts_host.  ndocs == 0 is a valid empty window.
 *   A state that krca_template_novelty_init did not write: no kernel touches it past its first 256
 *   bytes, KRCA_EINVAL after the read-back.
 * Buffers: state = krca_template_novelty_state_size(capacity) bytes, 8-byte aligned, fully defined by
 *   krca_template_novelty_init (the touched list behind the slots is written before it is read).  The
 *   update needs no initialisation of its outputs.  Not for graph capture (a read-back).
 * krca_template_novelty_layout(which): 0 header bytes, 1 slot bytes, 2 report record bytes, 3 bits of
 *   cur_lines in the packed per-window word, 4 the largest ndocs; krca_template_novelty_home_slot: the
 *   slot a key's probe starts at (-1 for a bad capacity or group); host functions for the mirror in
 *   krca/novelty.py. */
int64_t krca_template_novelty_layout(int32_t which);
int64_t krca_template_novelty_home_slot(uint64_t hash, int32_t group, int64_t capacity);
int64_t krca_template_novelty_state_size(int64_t capacity);
int krca_template_novelty_init(void* state, int64_t capacity, void* stream);
int krca_template_novelty_update(void* state, const uint64_t* tmpl_hash, const int32_t* tmpl_count, int64_t n_lines,
                                 const int32_t* n_templates, const int64_t* doc_line0,
                                 const int32_t* group /*[ndocs], nullable*/, int64_t ndocs, int32_t window, int32_t ttl,
                                 int32_t surge_ratio, int32_t surge_min, int32_t report,
                                 void* report_out /*cap records, device*/, int32_t cap,
                                 int32_t* doc_novel /*[ndocs], nullable*/, int32_t* doc_surge /*[ndocs], nullable*/,
                                 int64_t* counts_host /*[6]*/, void* stream);
int krca_template_novelty_rehash(const void* old_state, void* new_state, int64_t new_capacity, int32_t min_last_window,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KRCA_H */
