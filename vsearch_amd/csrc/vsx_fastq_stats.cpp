// vsx_fastq_stats.cpp -- host side of vsx_fastq_stats and vsx_fastq_chars (include/vsx_fastq_stats.h): option checks, the error
// table, the window pipeline around the kernels of vsx_fastq_stats.hip, and the host restatements of both accumulations.
//
//   table    10^(-score/10) by quality SYMBOL, score = symbol - ascii and 0 below ascii (std::pow on the host)
//   tables   the counters live on the device for the whole call; length_counts follows from the lengths on the host; ee_counts and
//            q_counts are the suffix sums of the downloaded histogram of prefix lengths
//   windows  the pipeline of vsx_window.h with the staging of vsx_eestats.cpp: consecutive reads spanning at most the staging
//            capacity, one memcpy per blob into pinned memory, two slots with a stream each.  In vsx_fastq_stats the ordered sum
//            (vsx_launch_eestats_sum, unchanged) of window k + 1 waits for the sum of window k through an event, so every chain of
//            sum_ee sees the reads in input order.
//   checks   the kernels report per read (lowest and highest quality character; a byte outside 33 ... 126); the host walks those
//            in input order, so the first offending read is the one the host restatement names
//   host     stats_host and chars_host are written from the specification, not from the kernels: the fallback (VSX_FASTQ_STATS=host,
//            a matrix beyond the budget, more than UINT32_MAX reads) and what the tests without a device call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vsx_fastq_stats_internal.h"
#include "vsx_window.h"

#pragma clang fp contract(off)

using vsxp::align64;
using vsxp::fail;
using vsxp::now_s;
using vsxp::zeroed;
using vsxp::DevBuf;
using vsxp::PinnedBuf;

namespace {

constexpr const char * WHO_STATS = "vsx_fastq_stats";
constexpr const char * WHO_CHARS = "vsx_fastq_chars";
constexpr uint64_t SPAN_CAPACITY = (uint64_t) 16 << 20;      // bytes of a blob a window may span
constexpr uint64_t WINDOW_READS = 32768;
constexpr uint64_t WINDOW_READS_MAX = (uint64_t) 1 << 22;
constexpr uint64_t MATRIX_BYTES = (uint64_t) 256 << 20;      // the default window shrinks so that a slot's matrix stays below this
constexpr int SYMS = VSX_FQS_SYMS, FIRST = VSX_FQS_FIRST;
constexpr double EE_THRESHOLDS[4] = { 1.0, 0.5, 0.25, 0.1 };
constexpr int Q_THRESHOLDS[4] = { 5, 10, 15, 20 };

thread_local vsx_fastq_stats_stats g_stats {};
thread_local vsx_fastq_chars_stats g_chars {};

struct Input {
  const uint8_t * seq;          // NULL in vsx_fastq_stats
  const uint8_t * qual;
  const uint64_t * off;
  const uint32_t * len;
  uint64_t n;
};

struct Lengths {
  uint64_t symbols = 0, len_min = 0, len_max = 0;
};

// the reference's check of a read's lowest and highest quality character: the scores compared as unsigned, the lowest first
int check_range(const vsx_fastq_stats_opts & o, int low, int high)
{
  for (const int c : { low, high })
    {
      const unsigned score = c < o.ascii ? 0u : (unsigned) (c - (int) o.ascii);
      if (score < (unsigned) o.qmin || score > (unsigned) o.qmax)
        return fail(VSX_EINVAL, "%s: FASTQ quality value (%u) out of range (%lld-%lld)", WHO_STATS, score, (long long) o.qmin, (long long) o.qmax);
    }
  return VSX_OK;
}

int bad_byte(const char * who) { return fail(VSX_EINVAL, "%s: a quality character outside 33 ... 126", who); }

// ---- the host restatements -----------------------------------------------------------------------------------------------------
int stats_host(const vsx_fastq_stats_opts & o, const Input & in, const double * q2e, vsx_fastq_stats_out & out)
{
  for (uint64_t k = 0; k < in.n; ++k)
    {
      const uint8_t * q = in.qual + in.off[k];
      const uint64_t len = in.len[k];
      if (len == 0) continue;
      const auto mm = std::minmax_element(q, q + len);
      if (*mm.first < FIRST || *mm.second >= FIRST + SYMS) return bad_byte(WHO_STATS);
      const int rc = check_range(o, *mm.first, *mm.second);
      if (rc != VSX_OK) return rc;
      double ee = 0.0;
      int lowest = INT_MAX;
      for (uint64_t i = 0; i < len; ++i)
        {
          const int sym = q[i];
          ++out.symbol_counts[i * SYMS + (sym - FIRST)];
          lowest = std::min(lowest, sym < o.ascii ? 0 : sym - (int) o.ascii);
          for (int t = 0; t < 4; ++t)
            if (lowest > Q_THRESHOLDS[t]) ++out.q_counts[i * 4 + t];
          ee += q2e[sym];
          out.sum_ee[i] += ee;
          for (int t = 0; t < 4; ++t)
            if (ee <= EE_THRESHOLDS[t]) ++out.ee_counts[i * 4 + t];
        }
    }
  return VSX_OK;
}

int map_symbol(int raw) { return (unsigned) ((raw | 0x20) - 'a') < 26u ? (raw & 0xDF) : 'N'; }

int chars_host(const vsx_fastq_chars_opts & o, const Input & in, vsx_fastq_chars_out & out)
{
  for (uint64_t k = 0; k < in.n; ++k)
    {
      const uint8_t * s = in.seq + in.off[k];
      const uint8_t * q = in.qual + in.off[k];
      const uint64_t len = in.len[k];
      for (uint64_t i = 0; i < len; ++i)
        if (q[i] < FIRST || q[i] >= FIRST + SYMS) return bad_byte(WHO_CHARS);
      int run_char = -1, run = 0;
      for (uint64_t i = 0; i < len; ++i)
        {
          const int c = map_symbol(s[i]);
          ++out.seq_counts[c];
          ++out.qual_counts[q[i]];
          if (c == 'N') { out.qmin_n = std::min(out.qmin_n, q[i]); out.qmax_n = std::max(out.qmax_n, q[i]); }
          if (c == run_char) { ++run; out.maxrun[c] = std::max(out.maxrun[c], run); }
          else { run_char = c; run = 0; }
        }
      if ((int64_t) len >= o.tail)
        {
          bool equal = true;
          for (uint64_t i = len - (uint64_t) o.tail; i < len; ++i) equal = equal && q[i] == q[len - 1];
          if (equal) ++out.tail_counts[q[len - 1]];
        }
    }
  return VSX_OK;
}

// ---- the window pipeline (vsx_window.h) ------------------------------------------------------------------------------------------
enum { EV_IN, EV_RUN, EV_WALKED, EV_SUM, EV_DONE, EVENTS };

struct Slot : vsxp::Slot<EVENTS> {
  PinnedBuf<uint8_t> h_in;              // items + the span of each blob
  PinnedBuf<uint32_t> h_flag;
  DevBuf<uint8_t> d_in;
  DevBuf<uint32_t> d_flag;              // per read: minmax (stats) or the bad-byte flag (chars)
  DevBuf<double> d_matrix;
  bool summed = false;
};

// what differs between the two calls
struct Device {
  const char * who = nullptr;
  bool chars = false;
  VsxFastqStatsParams P {};
  DevBuf<double> d_sum;
  uint32_t tail = 0;
  DevBuf<VsxFastqCharsAcc> d_acc;
  double * seconds_stage = nullptr;
};

int create_slots(Slot (&slot)[2], const Device & D, uint64_t window, uint64_t matrix_elems)
{
  for (Slot & s : slot)
    {
      const int rc = s.create(D.who);
      if (rc != VSX_OK) return rc;
      VSX_HIP_AS(D.who, s.h_flag.alloc(window));
      VSX_HIP_AS(D.who, s.d_flag.alloc(window));
      if (matrix_elems) VSX_HIP_AS(D.who, s.d_matrix.alloc(matrix_elems));
    }
  return VSX_OK;
}

// stage window [w0, w0 + n) into the slot and enqueue copy-in, the kernel(s) and the copy-out of the per-read flags on its stream
int submit_window(Slot & s, const Slot & previous, const Input & in, const Device & D, uint64_t w0, const vsxp::Window & W,
                  uint64_t reserve_in)
{
  const double t0 = now_s();
  const uint64_t n = W.n;
  const vsxp::Span span = W.span[0];
  const uint64_t blobs = D.chars ? 2 : 1;
  const uint64_t items_bytes = align64(n * sizeof(VsxEestatsItem));
  const uint64_t span_bytes = align64(span.hi - span.lo + 64);
  const uint64_t in_bytes = items_bytes + blobs * span_bytes;
  const int rc = vsxp::grow_pair(D.who, s.h_in, s.d_in, in_bytes, std::max(in_bytes, reserve_in));
  if (rc != VSX_OK) return rc;
  VsxEestatsItem * items = reinterpret_cast<VsxEestatsItem *>(s.h_in.p);
  for (uint64_t j = 0; j < n; ++j) items[j] = VsxEestatsItem { (uint32_t) (in.off[w0 + j] - span.lo), in.len[w0 + j] };
  std::memcpy(s.h_in.p + items_bytes, in.qual + span.lo, span.hi - span.lo);
  if (D.chars) std::memcpy(s.h_in.p + items_bytes + span_bytes, in.seq + span.lo, span.hi - span.lo);
  s.w0 = w0; s.n = n;
  const VsxEestatsItem * d_items = reinterpret_cast<const VsxEestatsItem *>(s.d_in.p);
  const uint8_t * d_qual = s.d_in.p + items_bytes;
  VSX_HIP_AS(D.who, hipEventRecord(s.ev[EV_IN], s.st));
  VSX_HIP_AS(D.who, hipMemcpyAsync(s.d_in.p, s.h_in.p, in_bytes, hipMemcpyHostToDevice, s.st));
  VSX_HIP_AS(D.who, hipEventRecord(s.ev[EV_RUN], s.st));
  if (D.chars)
    VSX_HIP_AS(D.who, vsx_launch_fastq_chars(d_items, (uint32_t) n, d_qual + span_bytes, d_qual, D.tail, D.d_acc.p, s.d_flag.p, s.st));
  else
    {
      VsxFastqStatsParams P = D.P;
      P.matrix = s.d_matrix.p;
      VSX_HIP_AS(D.who, vsx_launch_fastq_stats_walk(d_items, (uint32_t) n, d_qual, P, s.d_flag.p, s.st));
    }
  VSX_HIP_AS(D.who, hipEventRecord(s.ev[EV_WALKED], s.st));
  VSX_HIP_AS(D.who, hipMemcpyAsync(s.h_flag.p, s.d_flag.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s.st));
  if (!D.chars)
    {
      // the chains continue where the previous window's sums ended
      if (previous.summed) VSX_HIP_AS(D.who, hipStreamWaitEvent(s.st, previous.ev[EV_DONE], 0));
      VSX_HIP_AS(D.who, hipEventRecord(s.ev[EV_SUM], s.st));
      VSX_HIP_AS(D.who, vsx_launch_eestats_sum(s.d_matrix.p, D.P.stride, d_items, (uint32_t) n, D.P.len_max, D.d_sum.p, s.st));
      VSX_HIP_AS(D.who, hipEventRecord(s.ev[EV_DONE], s.st));
      s.summed = true;
    }
  s.busy = true;
  *D.seconds_stage += now_s() - t0;
  return VSX_OK;
}

// wait for the slot's window and add its device times
int wait_window(Slot & s, const Device & D)
{
  VSX_HIP_AS(D.who, hipStreamSynchronize(s.st));
  s.busy = false;
  VSX_HIP_AS(D.who, s.add_elapsed(EV_IN, EV_RUN, D.chars ? g_chars.seconds_h2d : g_stats.seconds_h2d));
  VSX_HIP_AS(D.who, s.add_elapsed(EV_RUN, EV_WALKED, D.chars ? g_chars.seconds_kernel : g_stats.seconds_walk));
  if (!D.chars) VSX_HIP_AS(D.who, s.add_elapsed(EV_SUM, EV_DONE, g_stats.seconds_sum));
  return VSX_OK;
}

// the first offending read of the call, in read order, ends it
int collect_stats_window(Slot & s, const Device & D, const vsx_fastq_stats_opts & o)
{
  const double t0 = now_s();
  int rc = wait_window(s, D);
  for (uint64_t j = 0; j < s.n && rc == VSX_OK; ++j)
    {
      const uint32_t mm = s.h_flag.p[j];
      if (mm == VSX_FQS_NO_SYMBOL) continue;
      const int low = (int) (mm & 255), high = (int) (mm >> 8 & 255);
      rc = low < FIRST || high >= FIRST + SYMS ? bad_byte(WHO_STATS) : check_range(o, low, high);
    }
  g_stats.seconds_d2h_output += now_s() - t0;
  return rc;
}

int collect_chars_window(Slot & s, const Device & D)
{
  const double t0 = now_s();
  int rc = wait_window(s, D);
  for (uint64_t j = 0; j < s.n && rc == VSX_OK; ++j)
    if (s.h_flag.p[j]) rc = bad_byte(WHO_CHARS);
  g_chars.seconds_d2h_output += now_s() - t0;
  return rc;
}

template <typename Collect>
int run_windows(Slot (&slot)[2], const Input & in, const Device & D, uint64_t window, uint64_t & windows, Collect collect)
{
  // the first window of a slot sizes its input buffers for every later one (a single read above the capacity grows them when it comes)
  uint64_t bytes = 0;
  for (uint64_t k = 0; k < in.n; ++k) bytes = std::max(bytes, in.off[k] + in.len[k]);
  const uint64_t reserve_in = align64(window * sizeof(VsxEestatsItem)) + (D.chars ? 2 : 1) * align64(std::min(SPAN_CAPACITY, bytes) + 64);
  const vsxp::Side side { in.off, in.len };
  return vsxp::run_windows(slot, in.n,
    [&](uint64_t w0) { vsxp::Stopwatch t(*D.seconds_stage); return vsxp::plan_window(&side, 1, w0, in.n, window, SPAN_CAPACITY); },
    [&](Slot & s, Slot & previous, uint64_t w0, const vsxp::Window & W) { return submit_window(s, previous, in, D, w0, W, reserve_in); },
    collect, windows);
}

uint64_t stats_window(const vsx_fastq_stats_opts & o, uint64_t n, uint64_t len_max)
{
  uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_READS;
  if (o.window <= 0 && len_max) window = std::max<uint64_t>(VSX_FQS_THREADS, std::min(window, MATRIX_BYTES / (8 * len_max)));
  return std::min({ window, WINDOW_READS_MAX, std::max<uint64_t>(n, 1) });
}

int stats_device(vsx_ctx * ctx, const vsx_fastq_stats_opts & o, const Input & in, const Lengths & L, const double * q2e,
                 vsx_fastq_stats_out & out)
{
  VSX_HIP_AS(WHO_STATS, hipSetDevice(vsx_internal_device(ctx)));
  const uint64_t window = stats_window(o, in.n, L.len_max);
  const uint64_t hist_row = L.len_max + 1;

  Device D;
  D.who = WHO_STATS;
  D.seconds_stage = &g_stats.seconds_stage;
  DevBuf<double> d_q2e;
  DevBuf<uint32_t> d_sc, d_prefix;
  VSX_HIP_AS(WHO_STATS, d_q2e.alloc(256));
  VSX_HIP_AS(WHO_STATS, hipMemcpy(d_q2e.p, q2e, 256 * sizeof(double), hipMemcpyHostToDevice));
  int rc;
  if ((rc = zeroed(WHO_STATS, d_sc, L.len_max * SYMS)) != VSX_OK) return rc;
  if ((rc = zeroed(WHO_STATS, d_prefix, 8 * hist_row)) != VSX_OK) return rc;
  if ((rc = zeroed(WHO_STATS, D.d_sum, L.len_max)) != VSX_OK) return rc;
  VSX_HIP_AS(WHO_STATS, hipStreamSynchronize(nullptr));        // the slots' streams do not wait for the null stream
  D.P.ascii = (int32_t) o.ascii; D.P.stride = (uint32_t) window; D.P.len_max = (uint32_t) L.len_max;
  D.P.q2e = d_q2e.p; D.P.symbol_counts = d_sc.p; D.P.prefix_hist = d_prefix.p;

  Slot slot[2];
  if ((rc = create_slots(slot, D, window, window * L.len_max)) != VSX_OK) return rc;
  if ((rc = run_windows(slot, in, D, window, g_stats.windows, [&](Slot & s) { return collect_stats_window(s, D, o); })) != VSX_OK) return rc;

  const double t0 = now_s();
  std::vector<uint32_t> sc(L.len_max * SYMS), prefix(8 * hist_row);
  VSX_HIP_AS(WHO_STATS, hipMemcpy(sc.data(), d_sc.p, sc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::copy(sc.begin(), sc.end(), out.symbol_counts);
  VSX_HIP_AS(WHO_STATS, hipMemcpy(prefix.data(), d_prefix.p, prefix.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  VSX_HIP_AS(WHO_STATS, hipMemcpy(out.sum_ee, D.d_sum.p, L.len_max * sizeof(double), hipMemcpyDeviceToHost));
  // a read counts at position i when its prefix is longer than i
  for (int k = 0; k < 8; ++k)
    {
      uint64_t * const table = k < 4 ? out.ee_counts + k : out.q_counts + (k - 4);
      uint64_t longer = 0;
      for (uint64_t i = L.len_max; i-- > 0;)
        {
          longer += prefix[k * hist_row + i + 1];
          table[i * 4] = longer;
        }
    }
  g_stats.seconds_d2h_output += now_s() - t0;
  return VSX_OK;
}

int chars_device(vsx_ctx * ctx, const vsx_fastq_chars_opts & o, const Input & in, vsx_fastq_chars_out & out)
{
  VSX_HIP_AS(WHO_CHARS, hipSetDevice(vsx_internal_device(ctx)));
  const uint64_t window = std::min({ o.window > 0 ? (uint64_t) o.window : WINDOW_READS, WINDOW_READS_MAX, in.n });

  Device D;
  D.who = WHO_CHARS;
  D.chars = true;
  D.seconds_stage = &g_chars.seconds_stage;
  D.tail = (uint32_t) std::min<int64_t>(o.tail, (int64_t) 1 << 31);
  VsxFastqCharsAcc acc;
  std::memset(&acc, 0, sizeof acc);
  acc.qmin_n = 255;
  VSX_HIP_AS(WHO_CHARS, D.d_acc.alloc(1));
  VSX_HIP_AS(WHO_CHARS, hipMemcpy(D.d_acc.p, &acc, sizeof acc, hipMemcpyHostToDevice));
  VSX_HIP_AS(WHO_CHARS, hipStreamSynchronize(nullptr));

  Slot slot[2];
  int rc;
  if ((rc = create_slots(slot, D, window, 0)) != VSX_OK) return rc;
  if ((rc = run_windows(slot, in, D, window, g_chars.windows, [&](Slot & s) { return collect_chars_window(s, D); })) != VSX_OK) return rc;

  const double t0 = now_s();
  VSX_HIP_AS(WHO_CHARS, hipMemcpy(&acc, D.d_acc.p, sizeof acc, hipMemcpyDeviceToHost));
  for (int c = 0; c < 256; ++c)
    {
      out.seq_counts[c] = acc.seq[c]; out.qual_counts[c] = acc.qual[c]; out.tail_counts[c] = acc.tail[c];
      out.maxrun[c] = acc.maxrun[c];
    }
  out.qmin_n = (uint8_t) acc.qmin_n; out.qmax_n = (uint8_t) acc.qmax_n;
  g_chars.seconds_d2h_output += now_s() - t0;
  return VSX_OK;
}

// before anything is staged: every read inside its blob, every length an int; the lengths' figures on the way
int scan_lengths(const char * who, uint64_t n, const vsx_fastx_reads & reads, Lengths & L)
{
  L.len_min = n ? UINT64_MAX : 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      const uint64_t off = reads.off[k], len = reads.len[k];
      if (len > (uint64_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a read is longer than INT32_MAX", who);
      if (off > reads.bytes || len > reads.bytes - off) return fail(VSX_EINVAL, "%s: a read exceeds its blob", who);
      L.symbols += len; L.len_min = std::min(L.len_min, len); L.len_max = std::max(L.len_max, len);
    }
  return VSX_OK;
}

bool host_mode() { return vsxp::env_is_host("VSX_FASTQ_STATS"); }

// what the reference's check_parameters refuses
int check_stats_options(const vsx_fastq_stats_opts & o)
{
  const char * bad = nullptr;
  if (o.ascii != 33 && o.ascii != 64) bad = "the quality offset must be 33 or 64";
  else if (o.qmin > o.qmax) bad = "qmin cannot be greater than qmax";
  else if (o.ascii + o.qmin < 33) bad = "the quality offset plus qmin must be no less than 33";
  else if (o.ascii + o.qmax > 126) bad = "the quality offset plus qmax must be no more than 126";
  else if (o.window < 0) bad = "window cannot be negative";
  return bad ? fail(VSX_EINVAL, "%s: %s", WHO_STATS, bad) : VSX_OK;
}

void release(vsx_fastq_stats_out * out)
{
  std::free(out->length_counts); std::free(out->symbol_counts); std::free(out->sum_ee); std::free(out->ee_counts); std::free(out->q_counts);
  std::memset(out, 0, sizeof *out);
}

int run_stats(vsx_ctx * ctx, const vsx_fastq_stats_opts & o, const Input & in, const Lengths & L, bool host_all, vsx_fastq_stats_out & out)
{
  double q2e[256];
  for (int c = 0; c < 256; ++c) q2e[c] = vsxp::phred_error_probability(c < o.ascii ? 0 : c - (int) o.ascii);

  out.n = in.n; out.symbols = L.symbols; out.len_min = L.len_min; out.len_max = L.len_max;
  out.length_counts = static_cast<uint64_t *>(std::calloc(L.len_max + 1, sizeof(uint64_t)));
  if (!out.length_counts) return fail(VSX_ENOMEM, "%s: out of memory", WHO_STATS);
  for (uint64_t k = 0; k < in.n; ++k) ++out.length_counts[in.len[k]];
  if (L.len_max)
    {
      out.symbol_counts = static_cast<uint64_t *>(std::calloc(L.len_max * SYMS, sizeof(uint64_t)));
      out.sum_ee = static_cast<double *>(std::calloc(L.len_max, sizeof(double)));
      out.ee_counts = static_cast<uint64_t *>(std::calloc(L.len_max * 4, sizeof(uint64_t)));
      out.q_counts = static_cast<uint64_t *>(std::calloc(L.len_max * 4, sizeof(uint64_t)));
      if (!out.symbol_counts || !out.sum_ee || !out.ee_counts || !out.q_counts) return fail(VSX_ENOMEM, "%s: out of memory", WHO_STATS);
    }
  g_stats.reads = in.n;

  const bool over_budget = stats_window(o, in.n, L.len_max) * L.len_max > VSX_FASTQ_STATS_MATRIX_BUDGET_BYTES / sizeof(double);
  if (host_all || over_budget || in.n > (uint64_t) UINT32_MAX)
    {
      g_stats.reads_host = in.n;
      return stats_host(o, in, q2e, out);
    }
  if (L.symbols == 0) return VSX_OK;           // nothing to walk: every table is empty
  return stats_device(ctx, o, in, L, q2e, out);
}

}  // namespace

extern "C" {

void vsx_fastq_stats_opts_default(vsx_fastq_stats_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->ascii = 33;
  o->qmin = 0; o->qmax = 41;
}

void vsx_fastq_stats_last_stats(vsx_fastq_stats_stats * out) { if (out) *out = g_stats; }

void vsx_fastq_stats_out_free(vsx_fastq_stats_out * out) { if (out) release(out); }

int vsx_fastq_stats(vsx_ctx * ctx, const vsx_fastq_stats_opts * opts, uint64_t n, const vsx_fastx_reads * reads, vsx_fastq_stats_out * out)
{
  g_stats = vsx_fastq_stats_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !reads) return fail(VSX_EINVAL, "%s: null argument", WHO_STATS);
  std::memset(out, 0, sizeof *out);
  if (n && (!reads->qual || !reads->off || !reads->len)) return fail(VSX_EINVAL, "%s: null argument", WHO_STATS);
  const bool host_all = host_mode();
  if (!ctx && !host_all) return fail(VSX_EINVAL, "%s: no context (only VSX_FASTQ_STATS=host runs without one)", WHO_STATS);
  int rc = check_stats_options(*opts);
  if (rc != VSX_OK) return rc;
  const double t0 = now_s();
  Lengths L;
  if ((rc = scan_lengths(WHO_STATS, n, *reads, L)) != VSX_OK) return rc;
  g_stats.seconds_stage += now_s() - t0;
  const Input in { nullptr, reinterpret_cast<const uint8_t *>(reads->qual), reads->off, reads->len, n };
  rc = run_stats(ctx, *opts, in, L, host_all, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

void vsx_fastq_chars_opts_default(vsx_fastq_chars_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->tail = 4;
}

void vsx_fastq_chars_last_stats(vsx_fastq_chars_stats * out) { if (out) *out = g_chars; }

// (the output owns no memory; the call is there so that every output of the library is released the same way)
void vsx_fastq_chars_out_free(vsx_fastq_chars_out * out) { if (out) std::memset(out, 0, sizeof *out); }

int vsx_fastq_chars(vsx_ctx * ctx, const vsx_fastq_chars_opts * opts, uint64_t n, const vsx_fastx_reads * reads, vsx_fastq_chars_out * out)
{
  g_chars = vsx_fastq_chars_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !reads) return fail(VSX_EINVAL, "%s: null argument", WHO_CHARS);
  std::memset(out, 0, sizeof *out);
  if (n && (!reads->seq || !reads->qual || !reads->off || !reads->len)) return fail(VSX_EINVAL, "%s: null argument (sequence and quality are both read)", WHO_CHARS);
  const bool host_all = host_mode();
  if (!ctx && !host_all) return fail(VSX_EINVAL, "%s: no context (only VSX_FASTQ_STATS=host runs without one)", WHO_CHARS);
  if (opts->tail < 1) return fail(VSX_EINVAL, "%s: tail must be at least 1", WHO_CHARS);
  if (opts->window < 0) return fail(VSX_EINVAL, "%s: window cannot be negative", WHO_CHARS);
  const double t0 = now_s();
  Lengths L;
  int rc = scan_lengths(WHO_CHARS, n, *reads, L);
  if (rc != VSX_OK) return rc;
  g_chars.seconds_stage += now_s() - t0;
  out->n = n; out->total_chars = L.symbols;
  out->qmin_n = 255; out->qmax_n = 0;
  g_chars.reads = n;
  const Input in { reinterpret_cast<const uint8_t *>(reads->seq), reinterpret_cast<const uint8_t *>(reads->qual), reads->off, reads->len, n };
  if (host_all || n > (uint64_t) UINT32_MAX)
    {
      g_chars.reads_host = n;
      rc = chars_host(*opts, in, *out);
    }
  else if (L.symbols) rc = chars_device(ctx, *opts, in, *out);
  if (rc != VSX_OK) { std::memset(out, 0, sizeof *out); return rc; }
  g_chars.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
