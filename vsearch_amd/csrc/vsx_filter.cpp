// vsx_filter.cpp -- host side of vsx_fastx_filter (include/vsx_filter.h): option checks, the table, the window pipeline around
// the kernel of vsx_filter.hip, and the host restatement of the reference's `analyse`.
//
//   table    10^(-q/10) by quality SYMBOL for offset + qmin .. offset + qmax (std::pow on the host, as the merge tables), 0 elsewhere
//   windows  a window is a run of consecutive reads whose bytes span at most the staging capacity: [min offset, max offset + length).
//            The span is copied into pinned memory with one memcpy per blob and the kernel follows the caller's offsets, rebased to
//            the span -- no per-read packing.  Scattered or overlapping offsets merely give small windows; a single read always fits.
//            Two slots (pinned + device buffers, one stream each): window k + 1 is staged while window k's kernel runs.  Planner,
//            slot base and driver are those of vsx_window.h.
//   host     analyse_host below is written from the specification, not from the kernel; VSX_FILTER=host sends every read through it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "vsx_filter_internal.h"
#include "vsx_window.h"

#pragma clang fp contract(off)

using vsxp::align64;
using vsxp::fail;
using vsxp::now_s;
using vsxp::DevBuf;
using vsxp::PinnedBuf;

namespace {

constexpr const char * WHO = "vsx_fastx_filter";
constexpr uint64_t SPAN_CAPACITY = (uint64_t) 16 << 20;      // bytes of one blob a window may span
constexpr uint64_t WINDOW_READS = 65536;

thread_local vsx_fastx_filter_stats g_stats {};

struct QualError { int kind = 0; int value = 0; };           // kind 1: below qmin, 2: above qmax

// ---- the host restatement: one read -------------------------------------------------------------------------------------------
// qual == nullptr: FASTA input.  Returns false on an out-of-range quality (err filled).
bool analyse_host(const vsx_fastx_filter_opts & o, const double * q2e, const uint8_t * seq, const uint8_t * qual, int64_t full,
                  VsxFilterDevRec & rec, QualError & err)
{
  int64_t start = 0, len = full;
  if (o.stripleft < len) { start += o.stripleft; len -= o.stripleft; } else { start = len; len = 0; }
  if (o.stripright < len) len -= o.stripright; else len = 0;
  if (o.trunclen >= 0) len = std::min(len, o.trunclen);
  if (o.trunclen_keep >= 0) len = std::min(len, o.trunclen_keep);
  bool discarded = false;
  double ee = -1.0;
  if (qual)
    {
      ee = 0.0;
      const uint8_t * q = qual + start;
      for (int64_t i = 0; i < len; ++i)
        {
          const int v = (int) (int8_t) q[i] - (int) o.ascii;
          if (v < o.qmin) { err.kind = 1; err.value = v; return false; }
          if (v > o.qmax) { err.kind = 2; err.value = v; return false; }
          const double e = q2e[q[i] & 127];
          ee += e;
          if ((int64_t) v <= o.truncqual || ee > o.truncee || ee > o.truncee_rate * (double) (i + 1))
            {
              ee -= e;
              len = i;
              break;
            }
          if ((int64_t) v < o.minqual) discarded = true;
        }
      if (ee > o.maxee) discarded = true;
      if (len > 0 && ee / (double) len > o.maxee_rate) discarded = true;
    }
  if (o.trunclen >= 0 && len < o.trunclen) discarded = true;
  if (len < o.minlen || len > o.maxlen) discarded = true;
  int64_t ncount = 0;
  for (int64_t i = 0; i < len; ++i) ncount += seq[start + i] == 'N' || seq[start + i] == 'n';
  if (ncount > o.maxns) discarded = true;
  rec = VsxFilterDevRec {};
  rec.start = (int32_t) start; rec.length = (int32_t) len; rec.ee = ee;
  rec.discarded = discarded; rec.truncated = len < full;
  return true;
}

// ---- output: device records become the caller's, the abundance filter and the totals are applied in input order --------------
struct Sides {
  const vsx_fastx_reads * side[2];
  int n_sides;
};

int put_read(const vsx_fastx_filter_opts & o, const Sides & in, vsx_fastx_filter_out & out, uint64_t k, const VsxFilterDevRec * const d[2])
{
  bool discarded = false, truncated = false;
  for (int s = 0; s < in.n_sides; ++s)
    {
      const VsxFilterDevRec & r = *d[s];
      if (r.qerr) return vsxp::quality_failure(WHO, r.qerr, r.qerr_value, (long long) o.qmin, (long long) o.qmax);
      vsx_fastx_filter_record & w = (s ? out.rev : out.fwd)[k];
      std::memset(&w, 0, sizeof w);
      w.start = r.start; w.length = r.length; w.ee = r.ee; w.truncated = r.truncated;
      const uint64_t * ab = in.side[s]->abundance;
      const int64_t abundance = ab ? (int64_t) std::min<uint64_t>(ab[k], (uint64_t) INT64_MAX) : 1;
      w.discarded = r.discarded || abundance < o.minsize || abundance > o.maxsize;
      discarded |= w.discarded != 0; truncated |= w.truncated != 0;
    }
  out.pair_discarded[k] = discarded;
  if (discarded) ++out.discarded;
  else { ++out.kept; if (truncated) ++out.kept_truncated; }
  return VSX_OK;
}

// ---- the window pipeline (vsx_window.h) ---------------------------------------------------------------------------------------
enum { EV_IN, EV_RUN, EV_DONE, EVENTS };

struct Slot : vsxp::Slot<EVENTS> {
  PinnedBuf<uint8_t> h_in, h_out;       // in: per side items + sequence span + quality span; out: per side records
  DevBuf<uint8_t> d_in, d_out;
};

// stage window [w0, w0 + n) into the slot and enqueue copy-in, one kernel per side, copy-out on its stream
int submit_window(Slot & s, const Sides & in, const VsxFilterParams & P, uint64_t w0, const vsxp::Window & W, uint64_t reserve_in, uint64_t reserve_out)
{
  const double t0 = now_s();
  const uint64_t n = W.n;
  const vsxp::Span * const span = W.span;
  const uint64_t items_bytes = align64(n * sizeof(VsxFilterItem)), recs_bytes = align64(n * sizeof(VsxFilterDevRec));
  uint64_t side_off[2] = { 0, 0 }, seq_off[2], qual_off[2], in_bytes = 0;
  for (int k = 0; k < in.n_sides; ++k)
    {
      const uint64_t bytes = align64(span[k].hi - span[k].lo + VSX_FILTER_PAD);
      side_off[k] = in_bytes; seq_off[k] = in_bytes + items_bytes;
      qual_off[k] = seq_off[k] + bytes;
      in_bytes = qual_off[k] + (P.has_qual ? bytes : 0);
    }
  const uint64_t out_bytes = recs_bytes * in.n_sides;
  int rc = vsxp::grow_pair(WHO, s.h_in, s.d_in, in_bytes, std::max(in_bytes, reserve_in));
  if (rc == VSX_OK) rc = vsxp::grow_pair(WHO, s.h_out, s.d_out, out_bytes, std::max(out_bytes, reserve_out));
  if (rc != VSX_OK) return rc;
  for (int k = 0; k < in.n_sides; ++k)
    {
      const vsx_fastx_reads & r = *in.side[k];
      VsxFilterItem * items = reinterpret_cast<VsxFilterItem *>(s.h_in.p + side_off[k]);
      for (uint64_t j = 0; j < n; ++j) items[j] = VsxFilterItem { (uint32_t) (r.off[w0 + j] - span[k].lo), r.len[w0 + j] };
      const uint64_t bytes = span[k].hi - span[k].lo;
      std::memcpy(s.h_in.p + seq_off[k], r.seq + span[k].lo, bytes);
      if (P.has_qual) std::memcpy(s.h_in.p + qual_off[k], r.qual + span[k].lo, bytes);
    }
  s.w0 = w0; s.n = n;
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_IN], s.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(s.d_in.p, s.h_in.p, in_bytes, hipMemcpyHostToDevice, s.st));
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_RUN], s.st));
  for (int k = 0; k < in.n_sides; ++k)
    VSX_HIP_AS(WHO, vsx_launch_filter(reinterpret_cast<const VsxFilterItem *>(s.d_in.p + side_off[k]), (uint32_t) n, s.d_in.p + seq_off[k],
                                      s.d_in.p + qual_off[k], P, reinterpret_cast<VsxFilterDevRec *>(s.d_out.p + k * recs_bytes), s.st));
  VSX_HIP_AS(WHO, hipEventRecord(s.ev[EV_DONE], s.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(s.h_out.p, s.d_out.p, recs_bytes * in.n_sides, hipMemcpyDeviceToHost, s.st));
  s.busy = true;
  g_stats.seconds_stage += now_s() - t0;
  return VSX_OK;
}

// wait for the slot's window and append its reads to the output, in order
int collect_window(Slot & s, const vsx_fastx_filter_opts & o, const Sides & in, vsx_fastx_filter_out & out)
{
  const double t0 = now_s();
  VSX_HIP_AS(WHO, hipStreamSynchronize(s.st));
  s.busy = false;
  VSX_HIP_AS(WHO, s.add_elapsed(EV_IN, EV_RUN, g_stats.seconds_h2d));
  VSX_HIP_AS(WHO, s.add_elapsed(EV_RUN, EV_DONE, g_stats.seconds_kernel));
  const uint64_t recs_bytes = align64(s.n * sizeof(VsxFilterDevRec));
  const VsxFilterDevRec * recs[2] = { reinterpret_cast<const VsxFilterDevRec *>(s.h_out.p), reinterpret_cast<const VsxFilterDevRec *>(s.h_out.p + recs_bytes) };
  for (uint64_t j = 0; j < s.n; ++j)
    {
      const VsxFilterDevRec * const d[2] = { recs[0] + j, recs[1] + j };
      const int rc = put_read(o, in, out, s.w0 + j, d);
      if (rc != VSX_OK) return rc;
    }
  g_stats.seconds_d2h_output += now_s() - t0;
  return VSX_OK;
}

// what the reference's check_parameters refuses, and the limit of the table's index
int check_options(const vsx_fastx_filter_opts & o)
{
  const char * bad = nullptr;
  if (std::signbit(o.truncee_rate)) bad = "truncee_rate cannot be negative";
  else if (o.minqual < 0) bad = "minqual cannot be negative";
  else if (!(o.maxee > 0.0)) bad = "maxee must be positive";
  else if (std::signbit(o.maxee_rate)) bad = "maxee_rate cannot be negative";
  else if (std::signbit(o.truncee)) bad = "truncee cannot be negative";
  else if (o.maxlen < 1) bad = "maxlen must be a positive integer";
  else if (o.maxns < 0) bad = "maxns must be a non-negative integer";
  else if (o.minlen < 1) bad = "minlen must be a positive integer";
  else if (o.trunclen != -1 && o.trunclen < 1) bad = "trunclen must be a positive integer";
  else if (o.trunclen_keep != -1 && o.trunclen_keep < 1) bad = "trunclen_keep must be a positive integer";
  else if (o.truncqual != LONG_MIN && (o.truncqual < 0 || o.truncqual > 93)) bad = "truncqual must be in range 0..93";
  else if (o.stripleft < 0) bad = "stripleft must be a non-negative integer";
  else if (o.stripright < 0) bad = "stripright must be a non-negative integer";
  else if (o.window < 0) bad = "window cannot be negative";
  // quality symbols are table indices: every symbol the call can accept must be a 7-bit character
  else if (o.ascii < 0 || o.ascii > 127 || o.qmin > o.qmax || o.ascii + o.qmin < 0 || o.ascii + o.qmax > 127)
    bad = "the quality offset plus qmin / qmax must lie within 0..127";
  return bad ? fail(VSX_EINVAL, "%s: %s", WHO, bad) : VSX_OK;
}

void release(vsx_fastx_filter_out * out)
{
  std::free(out->fwd); std::free(out->rev); std::free(out->pair_discarded);
  std::memset(out, 0, sizeof *out);
}

int run(vsx_ctx * ctx, const vsx_fastx_filter_opts & o, uint64_t n, const Sides & in, bool host_all, vsx_fastx_filter_out & out)
{
  const bool has_qual = n && in.side[0]->qual;
  double q2e[128];
  std::fill(q2e, q2e + 128, 0.0);
  for (int64_t v = o.qmin; v <= o.qmax; ++v) q2e[o.ascii + v] = vsxp::phred_error_probability((int) v);

  out.n = n;
  out.fwd = static_cast<vsx_fastx_filter_record *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(vsx_fastx_filter_record)));
  out.rev = in.n_sides > 1 ? static_cast<vsx_fastx_filter_record *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(vsx_fastx_filter_record))) : nullptr;
  out.pair_discarded = static_cast<uint8_t *>(std::calloc(std::max<uint64_t>(n, 1), 1));
  if (!out.fwd || !out.pair_discarded || (in.n_sides > 1 && !out.rev)) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  g_stats.reads = n * in.n_sides;

  if (host_all)
    {
      for (uint64_t k = 0; k < n; ++k)
        {
          VsxFilterDevRec d[2];
          for (int s = 0; s < in.n_sides; ++s)
            {
              const vsx_fastx_reads & r = *in.side[s];
              const uint8_t * seq = reinterpret_cast<const uint8_t *>(r.seq) + r.off[k];
              QualError e;
              if (!analyse_host(o, q2e, seq, has_qual ? reinterpret_cast<const uint8_t *>(r.qual) + r.off[k] : nullptr, r.len[k], d[s], e))
                return vsxp::quality_failure(WHO, e.kind, e.value, (long long) o.qmin, (long long) o.qmax);
            }
          const VsxFilterDevRec * const dp[2] = { &d[0], &d[1] };
          const int rc = put_read(o, in, out, k, dp);
          if (rc != VSX_OK) return rc;
        }
      g_stats.reads_host = g_stats.reads;
      return VSX_OK;
    }

  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  DevBuf<double> d_q2e;
  VSX_HIP_AS(WHO, d_q2e.alloc(128));
  VSX_HIP_AS(WHO, hipMemcpy(d_q2e.p, q2e, sizeof q2e, hipMemcpyHostToDevice));
  VsxFilterParams P {};
  P.stripleft = o.stripleft; P.stripright = o.stripright; P.trunclen = o.trunclen; P.trunclen_keep = o.trunclen_keep;
  P.truncqual = o.truncqual; P.minqual = o.minqual; P.minlen = o.minlen; P.maxlen = o.maxlen; P.maxns = o.maxns;
  P.maxee = o.maxee; P.maxee_rate = o.maxee_rate; P.truncee = o.truncee; P.truncee_rate = o.truncee_rate;
  P.ascii = (int32_t) o.ascii; P.qmin = (int32_t) o.qmin; P.qmax = (int32_t) o.qmax; P.has_qual = has_qual ? 1 : 0;
  P.q2e = d_q2e.p;

  const uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_READS;
  Slot slot[2];
  for (Slot & s : slot) { const int rc = s.create(WHO); if (rc != VSX_OK) return rc; }
  // the first window of a slot sizes its buffers for every later one (a single read above the capacity grows them when it comes)
  uint64_t reserve_in = 0;
  for (int s = 0; s < in.n_sides; ++s)
    reserve_in += align64(std::min(window, n) * sizeof(VsxFilterItem))
                  + (has_qual ? 2 : 1) * align64(std::min(SPAN_CAPACITY, in.side[s]->bytes) + VSX_FILTER_PAD);
  const uint64_t reserve_out = in.n_sides * align64(std::min(window, n) * sizeof(VsxFilterDevRec));
  vsxp::Side side[2] = { { in.side[0]->off, in.side[0]->len }, { nullptr, nullptr } };
  if (in.n_sides > 1) side[1] = { in.side[1]->off, in.side[1]->len };
  return vsxp::run_windows(slot, n,
    [&](uint64_t w0) { vsxp::Stopwatch t(g_stats.seconds_stage); return vsxp::plan_window(side, in.n_sides, w0, n, window, SPAN_CAPACITY); },
    [&](Slot & s, Slot &, uint64_t w0, const vsxp::Window & W) { return submit_window(s, in, P, w0, W, reserve_in, reserve_out); },
    [&](Slot & s) { return collect_window(s, o, in, out); },
    g_stats.windows);
}

}  // namespace

extern "C" {

void vsx_fastx_filter_opts_default(vsx_fastx_filter_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->ascii = 33;
  o->qmin = 0; o->qmax = 41;
  o->stripleft = 0; o->stripright = 0;
  o->trunclen = -1; o->trunclen_keep = -1;
  o->truncqual = LONG_MIN;
  o->minqual = 0;
  o->minlen = 1; o->maxlen = INT64_MAX;
  o->maxns = INT64_MAX;
  o->minsize = 0; o->maxsize = INT64_MAX;
  o->maxee = DBL_MAX; o->maxee_rate = DBL_MAX;
  o->truncee = DBL_MAX; o->truncee_rate = DBL_MAX;
}

void vsx_fastx_filter_last_stats(vsx_fastx_filter_stats * out) { if (out) *out = g_stats; }

void vsx_fastx_filter_out_free(vsx_fastx_filter_out * out) { if (out) release(out); }

int vsx_fastx_filter(vsx_ctx * ctx, const vsx_fastx_filter_opts * opts, uint64_t n,
                     const vsx_fastx_reads * fwd, const vsx_fastx_reads * rev, vsx_fastx_filter_out * out)
{
  g_stats = vsx_fastx_filter_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !fwd) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  Sides in { { fwd, rev }, rev ? 2 : 1 };
  for (int s = 0; s < in.n_sides; ++s)
    if (n && (!in.side[s]->seq || !in.side[s]->off || !in.side[s]->len)) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (rev && n && (fwd->qual == nullptr) != (rev->qual == nullptr))
    return fail(VSX_EINVAL, "%s: the forward and the reverse reads must both have qualities or both have none", WHO);
  const bool host_all = vsxp::env_is_host("VSX_FILTER");
  if (!ctx && !host_all) return fail(VSX_EINVAL, "%s: no context (only VSX_FILTER=host runs without one)", WHO);
  const int rc_opts = check_options(*opts);
  if (rc_opts != VSX_OK) return rc_opts;
  // before anything is staged: every read inside its blob, every length an int
  for (int s = 0; s < in.n_sides; ++s)
    for (uint64_t k = 0; k < n; ++k)
      {
        const vsx_fastx_reads & r = *in.side[s];
        if (r.len[k] > (uint32_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a read is longer than INT32_MAX", WHO);
        if (r.off[k] > r.bytes || r.len[k] > r.bytes - r.off[k]) return fail(VSX_EINVAL, "%s: a read exceeds its blob", WHO);
      }
  const int rc = run(ctx, *opts, n, in, host_all, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
