// vsx_eestats.cpp -- host side of vsx_fastq_eestats (include/vsx_eestats.h): option checks, the table, the window pipeline around
// the kernels of vsx_eestats.hip, and the host restatement of the reference's --fastq_eestats / --fastq_eestats2 accumulation.
//
//   table    10^(-max(q, 0)/10) by quality SYMBOL for ascii + qmin .. ascii + qmax (std::pow on the host, as the merge and filter
//            tables), 0 elsewhere
//   tables   quality counts, the expected-error histogram, the per-position sums and the cutoff counts live on the device for the
//            whole call (32-bit counters: a call has at most UINT32_MAX reads here); reads_at follows from the lengths on the host
//   windows  a window is a run of consecutive reads whose quality bytes span at most the staging capacity, copied into pinned
//            memory with one memcpy; the kernels follow the caller's offsets, rebased to the span.  Two slots, one stream each:
//            window k + 1 is staged and walked while window k's ordered sum runs.  The sum of window k + 1 waits for the sum of
//            window k through an event, so every chain sees the reads in input order.  Planner, slot base and driver are
//            those of vsx_window.h; the slot, submit_window and collect_window below are this command's.
//   host     accumulate_host below is written from the specification, not from the kernels: the fallback (VSX_EESTATS=host, a
//            histogram beyond the budget, more than UINT32_MAX reads) and what the tests without a device call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vsx_eestats_internal.h"
#include "vsx_window.h"

#pragma clang fp contract(off)

using vsxp::align64;
using vsxp::fail;
using vsxp::now_s;
using vsxp::zeroed;
using vsxp::DevBuf;
using vsxp::PinnedBuf;

namespace {

constexpr const char * WHO = "vsx_fastq_eestats";
constexpr uint64_t SPAN_CAPACITY = (uint64_t) 16 << 20;      // bytes of the quality blob a window may span
constexpr uint64_t WINDOW_READS = 32768;
constexpr uint64_t WINDOW_READS_MAX = (uint64_t) 1 << 22;
constexpr uint64_t MATRIX_BYTES = (uint64_t) 256 << 20;      // the default window shrinks so that a slot's matrix stays below this
constexpr int64_t RESOLUTION = VSX_EESTATS_RESOLUTION;
constexpr uint64_t HOST_LEN_MAX = 2147483;                   // 1000 * (i + 1) is an int in the reference
const double DEFAULT_CUTOFFS[3] = { 0.5, 1.0, 2.0 };

thread_local vsx_fastq_eestats_stats g_stats {};

uint64_t ee_start(uint64_t i) { return i * ((uint64_t) RESOLUTION * (i + 1) + 2) / 2; }

struct Lengths {
  uint64_t symbols = 0, len_min = 0, len_max = 0, len_steps = 0;
};

struct Input {
  const uint8_t * qual;
  const uint64_t * off;
  const uint32_t * len;
  uint64_t n;
};

int alloc_out(const vsx_fastq_eestats_opts & o, const Lengths & L, bool tables, bool cutoffs, vsx_fastq_eestats_out & out)
{
  out.qual_cols = tables ? (uint64_t) (o.qmax + 2) : 0;
  if (tables && L.len_max)
    {
      out.reads_at = static_cast<uint64_t *>(std::calloc(L.len_max, sizeof(uint64_t)));
      out.qual_counts = static_cast<uint64_t *>(std::calloc(L.len_max * out.qual_cols, sizeof(uint64_t)));
      out.sum_ee = static_cast<double *>(std::calloc(L.len_max, sizeof(double)));
      out.ee_bins = static_cast<int64_t *>(std::calloc(L.len_max * 5, sizeof(int64_t)));
      if (!out.reads_at || !out.qual_counts || !out.sum_ee || !out.ee_bins) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
    }
  if (cutoffs)
    {
      out.len_steps = L.len_steps;
      out.n_ee_cutoffs = o.n_ee_cutoffs;
      out.cutoff_counts = static_cast<uint64_t *>(std::calloc(std::max<uint64_t>(L.len_steps * o.n_ee_cutoffs, 1), sizeof(uint64_t)));
      if (!out.cutoff_counts) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
    }
  return VSX_OK;
}

// reads longer than i, from the lengths alone
void fill_reads_at(const Input & in, uint64_t len_max, uint64_t * reads_at)
{
  std::vector<uint64_t> ends(len_max + 1, 0);
  for (uint64_t k = 0; k < in.n; ++k) ++ends[in.len[k]];
  uint64_t longer = in.n;
  for (uint64_t i = 0; i < len_max; ++i) { longer -= ends[i]; reads_at[i] = longer; }
}

// ---- the host restatement ----------------------------------------------------------------------------------------------------
// First the reads in input order: the range check in the reference's reading order and the eestats2 counts.  Then, for the
// eestats tables, position by position over the reads in input order -- the order of the additions into sum_ee[i] -- with each
// read's running sum kept between positions, so that only one row of the histogram exists at a time.
int accumulate_host(const vsx_fastq_eestats_opts & o, const Input & in, const Lengths & L, const double * q2e, bool tables, bool cutoffs,
                    vsx_fastq_eestats_out & out)
{
  for (uint64_t k = 0; k < in.n; ++k)
    {
      const uint8_t * q = in.qual + in.off[k];
      const int64_t len = in.len[k];
      double ee = 0.0;
      int64_t next = o.len_shortest;                 // the next length of the eestats2 table, and its row
      uint64_t x = 0;
      for (int64_t i = 0; i < len; ++i)
        {
          const int v = (int) (int8_t) q[i] - (int) o.ascii;
          if (v < o.qmin) return vsxp::quality_failure(WHO, 1, v, (long long) o.qmin, (long long) o.qmax);
          if (v > o.qmax) return vsxp::quality_failure(WHO, 2, v, (long long) o.qmin, (long long) o.qmax);
          ee += q2e[q[i] & 127];
          if (cutoffs && i + 1 == next && x < L.len_steps)
            {
              for (uint64_t y = 0; y < o.n_ee_cutoffs; ++y)
                if (ee <= o.ee_cutoffs[y]) ++out.cutoff_counts[x * o.n_ee_cutoffs + y];
              next += o.len_increment;
              ++x;
            }
        }
    }
  if (!tables || !L.len_max) return VSX_OK;

  fill_reads_at(in, L.len_max, out.reads_at);
  std::vector<double> running(in.n, 0.0);
  std::vector<uint64_t> row;
  for (uint64_t i = 0; i < L.len_max; ++i)
    {
      const int64_t limit = RESOLUTION * (int64_t) (i + 1);
      row.assign((size_t) limit + 1, 0);
      uint64_t * const qc = out.qual_counts + i * out.qual_cols;
      double sum = 0.0;
      for (uint64_t k = 0; k < in.n; ++k)
        {
          if (in.len[k] <= i) continue;
          const uint8_t c = in.qual[in.off[k] + i];
          const int v = (int) (int8_t) c - (int) o.ascii;
          ++qc[std::max(v, 0)];
          double & ee = running[k];
          ee += q2e[c & 127];
          ++row[(size_t) std::min<int64_t>(limit, (int) ((double) RESOLUTION * ee))];
          sum += ee;
        }
      out.sum_ee[i] = sum;
      // the reference's scan: over the non-zero bins in ascending order, the running count a double
      const double reads = (double) (int64_t) out.reads_at[i];
      int64_t b[5] = { -1, -1, -1, -1, -1 };
      double n = 0;
      for (int64_t e = 0; e <= limit; ++e)
        {
          if (!row[(size_t) e]) continue;
          n += (double) (int64_t) row[(size_t) e];
          if (b[0] < 0) b[0] = e;
          if (b[1] < 0 && n >= 0.25 * reads) b[1] = e;
          if (b[2] < 0 && n >= 0.50 * reads) b[2] = e;
          if (b[3] < 0 && n >= 0.75 * reads) b[3] = e;
          b[4] = e;
        }
      std::copy(b, b + 5, out.ee_bins + i * 5);
    }
  return VSX_OK;
}

// ---- the window pipeline (vsx_window.h) ---------------------------------------------------------------------------------------
enum { EV_IN, EV_RUN, EV_WALKED, EV_SUM, EV_DONE, EVENTS };

struct Slot : vsxp::Slot<EVENTS> {
  PinnedBuf<uint8_t> h_in;              // items + quality span
  PinnedBuf<uint32_t> h_err;
  DevBuf<uint8_t> d_in;
  DevBuf<uint32_t> d_err;
  DevBuf<double> d_matrix;
  bool summed = false;
};

struct Device {
  VsxEestatsParams P {};
  uint32_t len_max = 0;
  bool tables = false;
  DevBuf<double> d_sum;
};

// stage window [w0, w0 + n) into the slot and enqueue copy-in, the walk, the ordered sum (behind the previous window's) and the
// copy-out of the per-read error positions on its stream
int submit_window(Slot & s, const Slot & previous, const Input & in, const Device & D, uint64_t w0, const vsxp::Window & W,
                  uint64_t reserve_in)
{
  const double t0 = now_s();
  const uint64_t n = W.n;
  const vsxp::Span span = W.span[0];
  const uint64_t items_bytes = align64(n * sizeof(VsxEestatsItem));
  const uint64_t in_bytes = items_bytes + align64(span.hi - span.lo + 64);
  const int rc = vsxp::grow_pair(WHO, s.h_in, s.d_in, in_bytes, std::max(in_bytes, reserve_in));
  if (rc != VSX_OK) return rc;
  VsxEestatsItem * items = reinterpret_cast<VsxEestatsItem *>(s.h_in.p);
  for (uint64_t j = 0; j < n; ++j) items[j] = VsxEestatsItem { (uint32_t) (in.off[w0 + j] - span.lo), in.len[w0 + j] };
  std::memcpy(s.h_in.p + items_bytes, in.qual + span.lo, span.hi - span.lo);
  s.w0 = w0; s.n = n;
  const VsxEestatsItem * d_items = reinterpret_cast<const VsxEestatsItem *>(s.d_in.p);
  VsxEestatsParams P = D.P;
  P.matrix = s.d_matrix.p;
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_IN], s.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(s.d_in.p, s.h_in.p, in_bytes, hipMemcpyHostToDevice, s.st));
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_RUN], s.st));
  VSX_HIP_AS(WHO, vsx_launch_eestats_walk(d_items, (uint32_t) n, s.d_in.p + items_bytes, P, s.d_err.p, s.st));
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_WALKED], s.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(s.h_err.p, s.d_err.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s.st));
  if (D.tables)
    {
      // the chains continue where the previous window's sums ended
      if (previous.summed) VSX_HIP_AS(WHO, hipStreamWaitEvent(s.st, previous.ev[EV_DONE], 0));
      VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_SUM], s.st));
      VSX_HIP_AS(WHO, vsx_launch_eestats_sum(s.d_matrix.p, P.stride, d_items, (uint32_t) n, D.len_max, D.d_sum.p, s.st));
      VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_DONE], s.st));
      s.summed = true;
    }
  s.busy = true;
  g_stats.seconds_stage += now_s() - t0;
  return VSX_OK;
}

// wait for the slot's window; the first out-of-range quality of the call, in read order, ends it
int collect_window(Slot & s, const vsx_fastq_eestats_opts & o, const Input & in, bool tables)
{
  const double t0 = now_s();
  VSX_HIP_AS(WHO, hipStreamSynchronize(s.st));
  s.busy = false;
  VSX_HIP_AS(WHO, s.add_elapsed(EV_IN, EV_RUN, g_stats.seconds_h2d));
  VSX_HIP_AS(WHO, s.add_elapsed(EV_RUN, EV_WALKED, g_stats.seconds_walk));
  if (tables) VSX_HIP_AS(WHO, s.add_elapsed(EV_SUM, EV_DONE, g_stats.seconds_sum));
  for (uint64_t j = 0; j < s.n; ++j)
    if (s.h_err.p[j] != VSX_EESTATS_NO_ERROR)
      {
        const int v = (int) (int8_t) in.qual[in.off[s.w0 + j] + s.h_err.p[j]] - (int) o.ascii;
        return vsxp::quality_failure(WHO, v < o.qmin ? 1 : 2, v, (long long) o.qmin, (long long) o.qmax);
      }
  g_stats.seconds_d2h_output += now_s() - t0;
  return VSX_OK;
}

int accumulate_device(vsx_ctx * ctx, const vsx_fastq_eestats_opts & o, const Input & in, const Lengths & L, const double * q2e,
                      bool tables, bool cutoffs, vsx_fastq_eestats_out & out)
{
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  tables = tables && L.len_max;
  uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_READS;
  if (o.window <= 0 && tables) window = std::max<uint64_t>(VSX_EESTATS_THREADS, std::min(window, MATRIX_BYTES / (8 * L.len_max)));
  window = std::min({ window, WINDOW_READS_MAX, in.n });

  Device D;
  D.tables = tables;
  D.len_max = (uint32_t) L.len_max;
  DevBuf<double> d_q2e, d_cutoffs;
  DevBuf<uint32_t> d_qc, d_hist, d_cut;
  DevBuf<uint64_t> d_reads_at;
  DevBuf<int64_t> d_bins;
  VSX_HIP_AS(WHO, d_q2e.alloc(128));
  VSX_HIP_AS(WHO, hipMemcpy(d_q2e.p, q2e, 128 * sizeof(double), hipMemcpyHostToDevice));
  VSX_HIP_AS(WHO, d_cutoffs.alloc(cutoffs ? o.n_ee_cutoffs : 0));
  if (cutoffs) VSX_HIP_AS(WHO, hipMemcpy(d_cutoffs.p, o.ee_cutoffs, o.n_ee_cutoffs * sizeof(double), hipMemcpyHostToDevice));
  int rc = zeroed(WHO, d_cut, cutoffs ? L.len_steps * o.n_ee_cutoffs : 0);
  if (rc != VSX_OK) return rc;
  if (tables)
    {
      if ((rc = zeroed(WHO, d_qc, L.len_max * out.qual_cols)) != VSX_OK) return rc;
      if ((rc = zeroed(WHO, d_hist, ee_start(L.len_max))) != VSX_OK) return rc;
      if ((rc = zeroed(WHO, D.d_sum, L.len_max)) != VSX_OK) return rc;
      fill_reads_at(in, L.len_max, out.reads_at);
      VSX_HIP_AS(WHO, d_reads_at.alloc(L.len_max));
      VSX_HIP_AS(WHO, hipMemcpy(d_reads_at.p, out.reads_at, L.len_max * sizeof(uint64_t), hipMemcpyHostToDevice));
      VSX_HIP_AS(WHO, d_bins.alloc(L.len_max * 5));
    }
  VSX_HIP_AS(WHO, hipStreamSynchronize(nullptr));        // the slots' streams do not wait for the null stream
  VsxEestatsParams & P = D.P;
  P.ascii = (int32_t) o.ascii; P.qmin = (int32_t) o.qmin; P.qmax = (int32_t) o.qmax; P.cols = (int32_t) (o.qmax + 2);
  P.want_tables = tables ? 1 : 0; P.want_cutoffs = cutoffs && L.len_steps ? 1 : 0;
  P.shortest = (int32_t) o.len_shortest; P.increment = (int32_t) o.len_increment;
  P.len_steps = (int32_t) L.len_steps; P.n_cutoffs = cutoffs ? (int32_t) o.n_ee_cutoffs : 0;
  P.stride = (uint32_t) window;
  P.q2e = d_q2e.p; P.cutoffs = d_cutoffs.p;
  P.qual_counts = d_qc.p; P.hist = d_hist.p; P.cutoff_counts = d_cut.p;

  Slot slot[2];
  for (Slot & s : slot)
    {
      if ((rc = s.create(WHO)) != VSX_OK) return rc;
      VSX_HIP_AS(WHO, s.h_err.alloc(window));
      VSX_HIP_AS(WHO, s.d_err.alloc(window));
      if (tables) VSX_HIP_AS(WHO, s.d_matrix.alloc(window * L.len_max));
    }
  // the first window of a slot sizes its input buffers for every later one (a single read above the capacity grows them when it comes)
  uint64_t bytes = 0;
  for (uint64_t k = 0; k < in.n; ++k) bytes = std::max(bytes, in.off[k] + in.len[k]);
  const uint64_t reserve_in = align64(window * sizeof(VsxEestatsItem)) + align64(std::min(SPAN_CAPACITY, bytes) + 64);
  const vsxp::Side side { in.off, in.len };
  rc = vsxp::run_windows(slot, in.n,
    [&](uint64_t w0) { vsxp::Stopwatch t(g_stats.seconds_stage); return vsxp::plan_window(&side, 1, w0, in.n, window, SPAN_CAPACITY); },
    [&](Slot & s, Slot & previous, uint64_t w0, const vsxp::Window & W) { return submit_window(s, previous, in, D, w0, W, reserve_in); },
    [&](Slot & s) { return collect_window(s, o, in, tables); },
    g_stats.windows);
  if (rc != VSX_OK) return rc;

  const double t0 = now_s();
  if (tables)
    {
      Slot & s = slot[0];
      VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_IN], s.st));
      VSX_HIP_AS(WHO, vsx_launch_eestats_quantile(d_hist.p, d_reads_at.p, D.len_max, d_bins.p, s.st));
      VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_DONE], s.st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(s.st));
      float ms = 0.f;
      VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, s.ev[EV_IN], s.ev[EV_DONE]));
      g_stats.seconds_quantile = ms * 1e-3;
      std::vector<uint32_t> qc(L.len_max * out.qual_cols);
      VSX_HIP_AS(WHO, hipMemcpy(qc.data(), d_qc.p, qc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      std::copy(qc.begin(), qc.end(), out.qual_counts);
      VSX_HIP_AS(WHO, hipMemcpy(out.sum_ee, D.d_sum.p, L.len_max * sizeof(double), hipMemcpyDeviceToHost));
      VSX_HIP_AS(WHO, hipMemcpy(out.ee_bins, d_bins.p, L.len_max * 5 * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
  if (cutoffs && L.len_steps)
    {
      std::vector<uint32_t> cut(L.len_steps * o.n_ee_cutoffs);
      VSX_HIP_AS(WHO, hipMemcpy(cut.data(), d_cut.p, cut.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      std::copy(cut.begin(), cut.end(), out.cutoff_counts);
    }
  g_stats.seconds_d2h_output += now_s() - t0;
  return VSX_OK;
}

// what the reference's check_parameters, args_get_length_cutoffs and args_get_ee_cutoffs refuse
int check_options(const vsx_fastq_eestats_opts & o)
{
  const char * bad = nullptr;
  if (o.ascii != 33 && o.ascii != 64) bad = "the quality offset must be 33 or 64";
  else if (o.qmin > o.qmax) bad = "qmin cannot be greater than qmax";
  else if (o.ascii + o.qmin < 33) bad = "the quality offset plus qmin must be no less than 33";
  else if (o.ascii + o.qmax > 126) bad = "the quality offset plus qmax must be no more than 126";
  else if (o.qmax < -1) bad = "qmax below -1 leaves the quality table without a column";
  else if (o.len_shortest < 1 || o.len_shortest > o.len_longest || o.len_increment < 1 || o.len_longest > INT_MAX || o.len_increment > INT_MAX)
    bad = "invalid length cutoffs";
  else if (o.want == 0 || (o.want & ~(VSX_EESTATS_WANT_EESTATS | VSX_EESTATS_WANT_EESTATS2))) bad = "want: eestats, eestats2 or both";
  else if (o.window < 0) bad = "window cannot be negative";
  else if (o.want & VSX_EESTATS_WANT_EESTATS2)
    {
      if (!o.ee_cutoffs || o.n_ee_cutoffs == 0 || o.n_ee_cutoffs > (uint64_t) INT_MAX) bad = "invalid expected-error cutoffs";
      else
        for (uint64_t y = 0; y < o.n_ee_cutoffs; ++y)
          if (!(o.ee_cutoffs[y] > 0.0)) bad = "invalid expected-error cutoffs";
    }
  return bad ? fail(VSX_EINVAL, "%s: %s", WHO, bad) : VSX_OK;
}

void release(vsx_fastq_eestats_out * out)
{
  std::free(out->reads_at); std::free(out->qual_counts); std::free(out->sum_ee); std::free(out->ee_bins); std::free(out->cutoff_counts);
  std::memset(out, 0, sizeof *out);
}

int run(vsx_ctx * ctx, const vsx_fastq_eestats_opts & o, const Input & in, const Lengths & L, bool host_all, vsx_fastq_eestats_out & out)
{
  const bool tables = o.want & VSX_EESTATS_WANT_EESTATS, cutoffs = o.want & VSX_EESTATS_WANT_EESTATS2;
  double q2e[128];
  std::fill(q2e, q2e + 128, 0.0);
  for (int64_t v = o.qmin; v <= o.qmax; ++v) q2e[o.ascii + v] = vsxp::phred_error_probability((int) std::max<int64_t>(v, 0));

  out.n = in.n; out.symbols = L.symbols; out.len_min = L.len_min; out.len_max = L.len_max;
  if (tables && L.len_max > HOST_LEN_MAX) return fail(VSX_EINVAL, "%s: a read is longer than the reference's histogram can index", WHO);
  const int rc = alloc_out(o, L, tables, cutoffs, out);
  if (rc != VSX_OK) return rc;
  g_stats.reads = in.n;

  const uint64_t budget = o.hist_budget ? std::min<uint64_t>(o.hist_budget, VSX_EESTATS_HIST_BUDGET_BYTES) : VSX_EESTATS_HIST_BUDGET_BYTES;
  const bool over_budget = tables && ee_start(L.len_max) * sizeof(uint32_t) > budget;
  if (host_all || over_budget || in.n > (uint64_t) UINT32_MAX)
    {
      g_stats.reads_host = in.n;
      return accumulate_host(o, in, L, q2e, tables, cutoffs, out);
    }
  if (L.symbols == 0) return VSX_OK;           // nothing to walk: every table is empty
  return accumulate_device(ctx, o, in, L, q2e, tables, cutoffs, out);
}

}  // namespace

extern "C" {

void vsx_fastq_eestats_opts_default(vsx_fastq_eestats_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->ascii = 33;
  o->qmin = 0; o->qmax = 41;
  o->len_shortest = 50; o->len_longest = INT_MAX; o->len_increment = 50;
  o->ee_cutoffs = DEFAULT_CUTOFFS; o->n_ee_cutoffs = 3;
  o->want = VSX_EESTATS_WANT_EESTATS | VSX_EESTATS_WANT_EESTATS2;
}

void vsx_fastq_eestats_last_stats(vsx_fastq_eestats_stats * out) { if (out) *out = g_stats; }

void vsx_fastq_eestats_out_free(vsx_fastq_eestats_out * out) { if (out) release(out); }

int vsx_fastq_eestats(vsx_ctx * ctx, const vsx_fastq_eestats_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
                      vsx_fastq_eestats_out * out)
{
  g_stats = vsx_fastq_eestats_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !reads) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (n && (!reads->qual || !reads->off || !reads->len)) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const bool host_all = vsxp::env_is_host("VSX_EESTATS");
  if (!ctx && !host_all) return fail(VSX_EINVAL, "%s: no context (only VSX_EESTATS=host runs without one)", WHO);
  const int rc_opts = check_options(*opts);
  if (rc_opts != VSX_OK) return rc_opts;
  // before anything is staged: every read inside its blob, every length an int; the lengths' figures on the way
  const double t0 = now_s();
  Lengths L;
  L.len_min = n ? UINT64_MAX : 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      const uint64_t off = reads->off[k], len = reads->len[k];
      if (len > (uint64_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a read is longer than INT32_MAX", WHO);
      if (off > reads->bytes || len > reads->bytes - off) return fail(VSX_EINVAL, "%s: a read exceeds its blob", WHO);
      L.symbols += len; L.len_min = std::min(L.len_min, len); L.len_max = std::max(L.len_max, len);
    }
  if (L.len_max)
    {
      // (C integer division, as the reference: it truncates toward zero)
      const int64_t high = (int64_t) std::min<uint64_t>(L.len_max, (uint64_t) opts->len_longest);
      L.len_steps = (uint64_t) (1 + std::max<int64_t>(0, (high - opts->len_shortest) / opts->len_increment));
    }
  g_stats.seconds_stage += now_s() - t0;
  const Input in { reinterpret_cast<const uint8_t *>(reads->qual), reads->off, reads->len, n };
  const int rc = run(ctx, *opts, in, L, host_all, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
