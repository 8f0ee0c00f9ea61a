// vsx_merge.cpp -- host side of vsx_merge_pairs (include/vsx_merge.h): the tables, the window pipeline around the kernel of
// vsx_merge.hip, and the host restatement of the same functions.
//
//   tables   built once per call as the reference's precompute_qual builds them (std::pow / log10 / log2 / round on the host;
//            no transcendental runs on the device), by quality SYMBOL, zero outside 33..126 like the reference's static arrays.
//            The device gets the square over the symbols a call can meet: offset + qmin .. offset + qmax, and the offset itself
//            (the quality N's are forced to).
//   pipeline windows of pairs; two slots of pinned staging + device buffers, one stream each.  Window k+1 is packed and copied
//            while window k's kernel runs; windows are unpacked in input order, so results do not depend on the window size.
//   host     reads above VSX_MERGE_MAX_LEN, and every pair under VSX_MERGE=host, go through merge_pair_host below: the same
//            census (counted on the diagonal), the same order of additions, the same rejection chain.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vsx_merge_internal.h"
#include "vsx_window.h"

#pragma clang fp contract(off)

using vsxp::fail;
using vsxp::now_s;
using vsxp::DevBuf;
using vsxp::PinnedBuf;

namespace {

thread_local vsx_merge_stats g_stats {};

// ---- tables ---------------------------------------------------------------------------------------------------------------
struct Tables {
  std::vector<double>  match, mism;        // 128 x 128, by symbol
  std::vector<uint8_t> same, diff;         // 128 x 128
  double q2p[128];
};

double symbol_error_probability(int symbol, int64_t ascii)
{
  const int value = symbol - (int) ascii;
  if (value < 2) return 0.75;
  return vsxp::phred_error_probability(value);
}

// Edgar & Flyvbjerg (2015) posterior qualities and the log-odds scores of an observed match / mismatch
void build_tables(const vsx_merge_opts & o, Tables & T)
{
  T.match.assign(128 * 128, 0.0); T.mism.assign(128 * 128, 0.0);
  T.same.assign(128 * 128, 0);    T.diff.assign(128 * 128, 0);
  std::fill(T.q2p, T.q2p + 128, 0.0);
  const double qmaxout = (double) o.fastq_qmaxout, qminout = (double) o.fastq_qminout, offset = (double) o.fastq_ascii;
  for (int x = 33; x <= 126; ++x)
    {
      const double px = symbol_error_probability(x, o.fastq_ascii);
      T.q2p[x] = px;
      for (int y = 33; y <= 126; ++y)
        {
          const double py = symbol_error_probability(y, o.fastq_ascii);
          double p = px * py / 3.0 / (1.0 - px - py + (4.0 * px * py / 3.0));
          double q = std::round(-10.0 * std::log10(p));
          q = std::max(std::min(q, qmaxout), qminout);
          T.same[x * 128 + y] = (uint8_t) (char) (offset + q);
          p = px * (1.0 - (py / 3.0)) / (px + py - (4.0 * px * py / 3.0));
          q = std::round(-10.0 * std::log10(p));
          q = std::max(std::min(q, qmaxout), qminout);
          T.diff[x * 128 + y] = (uint8_t) (char) (offset + q);
          p = 1.0 - px - py + (px * py * 4.0 / 3.0);
          T.match[x * 128 + y] = std::log2(p / 0.25);
          T.mism[x * 128 + y] = std::min(std::log2((1.0 - p) / 0.75), -4.0);
        }
    }
}

struct HostParams {
  vsx_merge_opts o;
  int mindiagcount;
  double minscore;
};

struct QualError { int kind = 0; int value = 0; };     // kind 1: below qmin, 2: above qmax

// ---- the host restatement: one pair -------------------------------------------------------------------------------------------
// seq / qual: the raw bytes.  Returns false on an out-of-range quality (err filled).  mseq / mqual receive the merged read.
bool merge_pair_host(const HostParams & H, const Tables & T, const uint8_t * fseq, const uint8_t * fqual, int64_t F,
                     const uint8_t * rseq, const uint8_t * rqual, int64_t R, VsxMergeDevRec & rec, std::string & mseq, std::string & mqual,
                     QualError & err)
{
  const vsx_merge_opts & o = H.o;
  rec = VsxMergeDevRec {};
  rec.fwd_trunc = (int32_t) F; rec.rev_trunc = (int32_t) R;
  bool skip = false;
  if (F < o.fastq_minlen || R < o.fastq_minlen) { rec.reason = VSX_MERGE_MINLEN; skip = true; }
  if (F > o.fastq_maxlen || R > o.fastq_maxlen) { rec.reason = VSX_MERGE_MAXLEN; skip = true; }
  int64_t trunc[2] = { F, R };
  for (int side = 0; side < 2 && !skip; ++side)
    {
      const uint8_t * q = side ? rqual : fqual;
      const int64_t len = side ? R : F;
      for (int64_t p = 0; p < len; ++p)
        {
          const int v = (int) (int8_t) q[p] - (int) o.fastq_ascii;
          if (v < o.fastq_qmin) { err.kind = 1; err.value = v; return false; }
          if (v > o.fastq_qmax) { err.kind = 2; err.value = v; return false; }
          if ((int64_t) v <= o.fastq_truncqual) { trunc[side] = p; break; }
        }
      if (trunc[side] < o.fastq_minlen) { rec.reason = VSX_MERGE_MINLEN; skip = true; }
    }
  const int64_t ftr = trunc[0], rtr = trunc[1];
  rec.fwd_trunc = (int32_t) ftr; rec.rev_trunc = (int32_t) rtr;
  if (skip) return true;

  // forward read and reverse-complemented reverse read, N qualities forced to the offset symbol
  std::vector<uint8_t> fs(ftr), fq(ftr), fc(ftr), rs(rtr), rq(rtr), rc(rtr);
  int64_t nf = 0, nr = 0;
  for (int64_t p = 0; p < ftr; ++p)
    {
      const uint8_t c = vsx_mg_upcase(fseq[p]);
      fs[p] = c; fq[p] = fqual[p]; fc[p] = vsx_mg_code(c, 4);
      if (c == 'N') { fq[p] = (uint8_t) o.fastq_ascii; ++nf; }
    }
  for (int64_t t = 0; t < rtr; ++t)
    {
      const int64_t r = rtr - 1 - t;
      const uint8_t c = vsx_mg_upcase(rseq[r]);
      const uint8_t cc = vsx_mg_complement(c);
      rs[t] = cc; rq[t] = rqual[r]; rc[t] = vsx_mg_code(cc, 5);
      if (c == 'N') { rq[t] = (uint8_t) o.fastq_ascii; ++nr; }
    }
  if (nf > o.fastq_maxns || nr > o.fastq_maxns) { rec.reason = VSX_MERGE_MAXNS; return true; }

  int hits = 0, ndiag = 0;
  int64_t best_i = 0, best_diffs = 0;
  double best_score = 0.0;
  for (int64_t i = 1; i <= ftr + rtr - 1; ++i)
    {
      const int64_t t_lo = i > ftr ? i - ftr : 0, t_hi = std::min(i, rtr), shift = ftr - i;
      int run = 0, cnt = 0;
      for (int64_t t = t_lo; t < t_hi; ++t) { run = fc[shift + t] == rc[t] ? run + 1 : 0; cnt += run >= 5; }
      if (cnt < H.mindiagcount) continue;
      ++ndiag;
      double score = 0.0, score_high = 0.0, dropmax = 0.0;
      int64_t diffs = 0;
      for (int64_t t = t_hi - 1; t >= t_lo; --t)
        {
          const int64_t f = shift + t;
          const size_t ti = (size_t) (fq[f] & 127) * 128 + (rq[t] & 127);
          if (fs[f] == rs[t]) { score += T.match[ti]; score_high = std::max(score, score_high); }
          else
            {
              score += T.mism[ti]; ++diffs;
              if (score < score_high - dropmax) dropmax = score_high - score;
            }
        }
      if (dropmax >= 16.0) score = 0.0;
      if (score >= H.minscore) ++hits;
      if (score > best_score) { best_score = score; best_i = i; best_diffs = diffs; }
    }
  rec.ndiag = ndiag;
  const int64_t mergelen0 = ftr + rtr - best_i;
  int reason = VSX_MERGE_OK;
  if (hits > 1) reason = VSX_MERGE_REPEAT;
  else if (!o.fastq_allowmergestagger && best_i > ftr) reason = VSX_MERGE_STAGGERED;
  else if (best_diffs > o.fastq_maxdiffs) reason = VSX_MERGE_MAXDIFFS;
  else if (100.0 * (double) best_diffs / (double) best_i > o.fastq_maxdiffpct) reason = VSX_MERGE_MAXDIFFPCT;
  else if (ndiag == 0) reason = VSX_MERGE_NOKMERS;
  else if (best_score < H.minscore) reason = VSX_MERGE_MINSCORE;
  else if (best_i < o.fastq_minovlen) reason = VSX_MERGE_MINOVLEN;
  else if ((int64_t) (int) mergelen0 < o.fastq_minmergelen) reason = VSX_MERGE_MINMERGELEN;
  else if ((int64_t) (int) mergelen0 > o.fastq_maxmergelen) reason = VSX_MERGE_MAXMERGELEN;
  if (reason != VSX_MERGE_OK || best_i <= 0) { rec.reason = reason; return true; }

  const int64_t f5 = ftr > best_i ? ftr - best_i : 0, r3 = best_i > ftr ? best_i - ftr : 0;
  const int64_t nm = std::min(ftr - f5, rtr - r3), mergelen = f5 + (rtr - r3);
  mseq.resize(mergelen); mqual.resize(mergelen);
  double ee_m = 0.0, ee_f = 0.0, ee_r = 0.0;
  int ferr = 0, rerr = 0;
  for (int64_t m = 0; m < mergelen; ++m)
    {
      uint8_t sym, q;
      if (m < f5) { sym = fs[m]; q = fq[m]; ee_f += T.q2p[q & 127]; }
      else if (m < f5 + nm)
        {
          const int64_t t = r3 + (m - f5);
          const uint8_t a0 = fs[m], b0 = rs[t], qa = fq[m], qb = rq[t];
          const uint8_t a = (int8_t) qa < 2 ? (uint8_t) 'N' : a0, b = (int8_t) qb < 2 ? (uint8_t) 'N' : b0;
          if (b == 'N') { sym = a; q = qa; }
          else if (a == 'N') { sym = b; q = qb; }
          else if (a == b) { sym = a; q = T.same[(size_t) (qa & 127) * 128 + (qb & 127)]; }
          else if ((int8_t) qa > (int8_t) qb) { sym = a; q = T.diff[(size_t) (qa & 127) * 128 + (qb & 127)]; }
          else { sym = b; q = T.diff[(size_t) (qb & 127) * 128 + (qa & 127)]; }
          ferr += sym != a0; rerr += sym != b0;
          ee_f += T.q2p[qa & 127]; ee_r += T.q2p[qb & 127];
        }
      else { const int64_t t = r3 + (m - f5); sym = rs[t]; q = rq[t]; ee_r += T.q2p[q & 127]; }
      ee_m += T.q2p[q & 127];
      mseq[m] = (char) sym; mqual[m] = (char) q;
    }
  rec.merged_length = (int32_t) mergelen; rec.fwd_errors = ferr; rec.rev_errors = rerr;
  rec.ee_merged = ee_m; rec.ee_fwd = ee_f; rec.ee_rev = ee_r;
  if (ee_m <= o.fastq_maxee) { rec.reason = VSX_MERGE_OK; rec.merged = 1; } else rec.reason = VSX_MERGE_MAXEE;
  return true;
}

// ---- output ---------------------------------------------------------------------------------------------------------------------
struct OutBuilder {
  vsx_merge_record * rec = nullptr;
  char * seq = nullptr, * qual = nullptr;
  uint64_t used = 0, cap = 0;
  ~OutBuilder() { std::free(rec); std::free(seq); std::free(qual); }
  bool room(uint64_t more)
  {
    if (used + more <= cap) return true;
    const uint64_t want = std::max<uint64_t>((cap + (cap >> 1)), used + more + 4096);
    char * s = static_cast<char *>(std::realloc(seq, want));
    if (!s) return false;
    seq = s;
    char * q = static_cast<char *>(std::realloc(qual, want));
    if (!q) return false;
    qual = q; cap = want;
    return true;
  }
  // false: out of memory
  bool put(uint64_t k, const VsxMergeDevRec & d, const char * mseq, const char * mqual)
  {
    vsx_merge_record & r = rec[k];
    std::memset(&r, 0, sizeof r);
    r.merged = d.merged; r.reason = d.reason; r.fwd_trunc = d.fwd_trunc; r.rev_trunc = d.rev_trunc;
    r.blob_off = used;
    if (!d.merged) return true;
    r.merged_length = d.merged_length; r.overlap_length = d.fwd_trunc + d.rev_trunc - d.merged_length;
    r.fwd_errors = d.fwd_errors; r.rev_errors = d.rev_errors;
    r.ee_merged = d.ee_merged; r.ee_fwd = d.ee_fwd; r.ee_rev = d.ee_rev;
    if (!room((uint64_t) d.merged_length)) return false;
    std::memcpy(seq + used, mseq, (size_t) d.merged_length);
    std::memcpy(qual + used, mqual, (size_t) d.merged_length);
    used += (uint64_t) d.merged_length;
    return true;
  }
};

int quality_failure(const vsx_merge_opts & o, const QualError & e)
{
  return vsxp::quality_failure("vsx_merge_pairs", e.kind, e.value, (long long) o.fastq_qmin, (long long) o.fastq_qmax);
}

// ---- the window pipeline (vsx_window.h) ---------------------------------------------------------------------------------------
enum { EV_RUN, EV_DONE, EVENTS };

struct Slot : vsxp::Slot<EVENTS> {
  PinnedBuf<uint8_t> h_in, h_out;                            // in: items + blob; out: recs + seq + qual
  DevBuf<uint8_t> d_in, d_out;                               // (each as large as its pinned twin)
  uint64_t blob_off = 0, out_bytes = 0;                      // of the window in flight
};

uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t) 15; }

struct Inputs {
  const uint8_t * fs, * fq, * rs, * rq;
  const uint64_t * foff, * roff;
  const uint32_t * flen, * rlen;
};

// pack window [w0, w0 + n) into the slot and enqueue copy-in, kernel, copy-out on its stream
int submit_window(Slot & s, const Inputs & in, const VsxMergeParams & P, uint64_t w0, uint64_t n)
{
  const double t0 = now_s();
  const uint64_t items_bytes = align16(n * sizeof(VsxMergeItem));
  uint64_t blob = 0, outb = 0;
  for (uint64_t k = w0; k < w0 + n; ++k)
    if (in.flen[k] <= VSX_MERGE_MAX_LEN && in.rlen[k] <= VSX_MERGE_MAX_LEN)
      { blob += 2 * ((uint64_t) in.flen[k] + in.rlen[k]); outb += (uint64_t) in.flen[k] + in.rlen[k]; }
  const uint64_t recs_bytes = align16(n * sizeof(VsxMergeDevRec));
  outb = align16(outb);
  // a window that outgrows the slot's buffers replaces them with an eighth of headroom
  const uint64_t in_bytes = items_bytes + blob + 16, out_bytes = recs_bytes + 2 * outb + 16;
  int rc = vsxp::grow_pair("vsx_merge_pairs", s.h_in, s.d_in, in_bytes, in_bytes + (in_bytes >> 3));
  if (rc == VSX_OK) rc = vsxp::grow_pair("vsx_merge_pairs", s.h_out, s.d_out, out_bytes, out_bytes + (out_bytes >> 3));
  if (rc != VSX_OK) return rc;
  VsxMergeItem * items = reinterpret_cast<VsxMergeItem *>(s.h_in.p);
  uint8_t * hb = s.h_in.p + items_bytes;
  uint64_t bo = 0, oo = 0;
  for (uint64_t k = w0; k < w0 + n; ++k)
    {
      VsxMergeItem & it = items[k - w0];
      const uint32_t F = in.flen[k], R = in.rlen[k];
      if (F > VSX_MERGE_MAX_LEN || R > VSX_MERGE_MAX_LEN) { it = VsxMergeItem { 0, 0, 0, 0, 1, 0 }; continue; }
      it = VsxMergeItem { bo, oo, F, R, 0, 0 };
      std::memcpy(hb + bo, in.fs + in.foff[k], F); bo += F;
      std::memcpy(hb + bo, in.fq + in.foff[k], F); bo += F;
      std::memcpy(hb + bo, in.rs + in.roff[k], R); bo += R;
      std::memcpy(hb + bo, in.rq + in.roff[k], R); bo += R;
      oo += (uint64_t) F + R;
    }
  s.w0 = w0; s.n = n; s.blob_off = items_bytes; s.out_bytes = recs_bytes + 2 * outb;
  VSX_HIP_AS("vsx_merge_pairs", hipMemcpyAsync(s.d_in.p, s.h_in.p, items_bytes + blob, hipMemcpyHostToDevice, s.st));
  VSX_HIP_AS("vsx_merge_pairs", hipEventRecord(s.ev[EV_RUN], s.st));
  VSX_HIP_AS("vsx_merge_pairs", vsx_launch_merge(reinterpret_cast<const VsxMergeItem *>(s.d_in.p), (uint32_t) n, s.d_in.p + items_bytes, P,
                        reinterpret_cast<VsxMergeDevRec *>(s.d_out.p), s.d_out.p + recs_bytes, s.d_out.p + recs_bytes + outb, s.st));
  VSX_HIP_AS("vsx_merge_pairs", hipEventRecord(s.ev[EV_DONE], s.st));
  VSX_HIP_AS("vsx_merge_pairs", hipMemcpyAsync(s.h_out.p, s.d_out.p, s.out_bytes, hipMemcpyDeviceToHost, s.st));
  s.busy = true;
  g_stats.seconds_stage += now_s() - t0;
  return VSX_OK;
}

// wait for the slot's window and append its pairs to the output, in order
int collect_window(Slot & s, const Inputs & in, const HostParams & H, const Tables & T, OutBuilder & ob)
{
  const double t0 = now_s();
  VSX_HIP_AS("vsx_merge_pairs", hipStreamSynchronize(s.st));
  s.busy = false;
  VSX_HIP_AS("vsx_merge_pairs", s.add_elapsed(EV_RUN, EV_DONE, g_stats.seconds_kernel));
  const VsxMergeItem * items = reinterpret_cast<const VsxMergeItem *>(s.h_in.p);
  const VsxMergeDevRec * recs = reinterpret_cast<const VsxMergeDevRec *>(s.h_out.p);
  const uint64_t recs_bytes = align16(s.n * sizeof(VsxMergeDevRec));
  const uint64_t outb = (s.out_bytes - recs_bytes) / 2;
  const char * oseq = reinterpret_cast<const char *>(s.h_out.p + recs_bytes), * oqual = oseq + outb;
  std::string mseq, mqual;
  for (uint64_t j = 0; j < s.n; ++j)
    {
      const uint64_t k = s.w0 + j;
      if (items[j].host)
        {
          VsxMergeDevRec d;
          QualError e;
          if (!merge_pair_host(H, T, in.fs + in.foff[k], in.fq + in.foff[k], in.flen[k], in.rs + in.roff[k], in.rq + in.roff[k], in.rlen[k],
                               d, mseq, mqual, e))
            return quality_failure(H.o, e);
          ++g_stats.pairs_host;
          g_stats.diagonals_scored += (uint64_t) d.ndiag;
          if (!ob.put(k, d, mseq.data(), mqual.data())) return fail(VSX_ENOMEM, "vsx_merge_pairs: out of memory");
          continue;
        }
      const VsxMergeDevRec & d = recs[j];
      if (d.qerr) { QualError e; e.kind = d.qerr; e.value = d.qerr_value; return quality_failure(H.o, e); }
      g_stats.diagonals_scored += (uint64_t) d.ndiag;
      if (!ob.put(k, d, oseq + items[j].out_off, oqual + items[j].out_off)) return fail(VSX_ENOMEM, "vsx_merge_pairs: out of memory");
    }
  g_stats.seconds_unpack += now_s() - t0;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_merge_opts_default(vsx_merge_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->fastq_ascii = 33;
  o->fastq_qmin = 0;  o->fastq_qmax = 41;
  o->fastq_qminout = 0; o->fastq_qmaxout = 41;
  o->fastq_minovlen = 10;
  o->fastq_maxdiffs = 10;
  o->fastq_maxdiffpct = 100.0;
  o->fastq_minmergelen = 0;
  o->fastq_maxmergelen = 1000000;
  o->fastq_maxee = DBL_MAX;
  o->fastq_truncqual = LONG_MIN;
  o->fastq_maxns = INT64_MAX;
  o->fastq_minlen = 1;
  o->fastq_maxlen = INT64_MAX;
  o->fastq_allowmergestagger = 0;
}

void vsx_merge_last_stats(vsx_merge_stats * out) { if (out) *out = g_stats; }

void vsx_merge_out_free(vsx_merge_out * out)
{
  if (!out) return;
  std::free(out->rec); std::free(out->seq_blob); std::free(out->qual_blob);
  std::memset(out, 0, sizeof *out);
}

int vsx_merge_pairs(vsx_ctx * ctx, const vsx_merge_opts * opts, uint64_t n,
                    const char * fwd_seq, const char * fwd_qual, uint64_t fwd_bytes, const uint64_t * fwd_off, const uint32_t * fwd_len,
                    const char * rev_seq, const char * rev_qual, uint64_t rev_bytes, const uint64_t * rev_off, const uint32_t * rev_len,
                    vsx_merge_out * out)
{
  g_stats = vsx_merge_stats {};
  const double t_begin = now_s();
  if (!opts || !out || (n && (!fwd_seq || !fwd_qual || !fwd_off || !fwd_len || !rev_seq || !rev_qual || !rev_off || !rev_len)))
    return fail(VSX_EINVAL, "vsx_merge_pairs: null argument");
  std::memset(out, 0, sizeof *out);
  const bool host_all = vsxp::env_is_host("VSX_MERGE");
  if (!ctx && !host_all) return fail(VSX_EINVAL, "vsx_merge_pairs: no context (only VSX_MERGE=host runs without one)");

  HostParams H;
  H.o = *opts;
  vsx_merge_opts & o = H.o;
  if (o.fastq_minovlen < 5) o.fastq_minovlen = 5;
  H.mindiagcount = o.fastq_minovlen < 9 ? (int) (o.fastq_minovlen - 4) : 4;
  H.minscore = o.fastq_minovlen < 9 ? 1.6 * (double) o.fastq_minovlen : 16.0;
  // quality symbols are table indices: every symbol the call can read or write must be a 7-bit character
  if (o.fastq_ascii < 0 || o.fastq_ascii > 127 || o.fastq_qmin > o.fastq_qmax || o.fastq_qminout > o.fastq_qmaxout ||
      o.fastq_ascii + o.fastq_qmin < 0 || o.fastq_ascii + o.fastq_qmax > 127 ||
      o.fastq_ascii + o.fastq_qminout < 0 || o.fastq_ascii + o.fastq_qmaxout > 127)
    return fail(VSX_EINVAL, "vsx_merge_pairs: the quality offset plus qmin / qmax / qminout / qmaxout must lie within 0..127");
  for (uint64_t k = 0; k < n; ++k)
    if (fwd_off[k] + fwd_len[k] > fwd_bytes || rev_off[k] + rev_len[k] > rev_bytes)
      return fail(VSX_EINVAL, "vsx_merge_pairs: a read exceeds its blob");

  Tables T;
  build_tables(o, T);
  Inputs in { reinterpret_cast<const uint8_t *>(fwd_seq), reinterpret_cast<const uint8_t *>(fwd_qual),
              reinterpret_cast<const uint8_t *>(rev_seq), reinterpret_cast<const uint8_t *>(rev_qual), fwd_off, rev_off, fwd_len, rev_len };
  OutBuilder ob;
  ob.rec = static_cast<vsx_merge_record *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(vsx_merge_record)));
  if (!ob.rec || !ob.room(1)) return fail(VSX_ENOMEM, "vsx_merge_pairs: out of memory");
  g_stats.pairs = n;

  if (host_all)
    {
      std::string mseq, mqual;
      for (uint64_t k = 0; k < n; ++k)
        {
          VsxMergeDevRec d;
          QualError e;
          if (!merge_pair_host(H, T, in.fs + fwd_off[k], in.fq + fwd_off[k], fwd_len[k], in.rs + rev_off[k], in.rq + rev_off[k], rev_len[k],
                               d, mseq, mqual, e))
            return quality_failure(o, e);
          g_stats.diagonals_scored += (uint64_t) d.ndiag;
          if (!ob.put(k, d, mseq.data(), mqual.data())) return fail(VSX_ENOMEM, "vsx_merge_pairs: out of memory");
        }
      g_stats.pairs_host = n;
    }
  else
    {
      VSX_HIP_AS("vsx_merge_pairs", hipSetDevice(vsx_internal_device(ctx)));
      // device tables: the square over the symbols this call can meet
      const int tlo = (int) std::min(o.fastq_ascii + o.fastq_qmin, o.fastq_ascii), thi = (int) std::max(o.fastq_ascii + o.fastq_qmax, o.fastq_ascii);
      const int D = thi - tlo + 1;
      const size_t dd = (size_t) D * D, dd16 = (size_t) align16(dd);
      std::vector<uint8_t> ht(2 * dd * 8 + 128 * 8 + 2 * dd16);
      double * h_match = reinterpret_cast<double *>(ht.data()), * h_mism = h_match + dd, * h_q2p = h_mism + dd;
      uint8_t * h_same = reinterpret_cast<uint8_t *>(h_q2p + 128), * h_diff = h_same + dd16;
      for (int x = 0; x < D; ++x)
        for (int y = 0; y < D; ++y)
          {
            const size_t s = (size_t) (x + tlo) * 128 + (y + tlo), d = (size_t) x * D + y;
            h_match[d] = T.match[s]; h_mism[d] = T.mism[s]; h_same[d] = T.same[s]; h_diff[d] = T.diff[s];
          }
      std::memcpy(h_q2p, T.q2p, sizeof T.q2p);
      DevBuf<uint8_t> dt;
      VSX_HIP_AS("vsx_merge_pairs", dt.alloc(ht.size()));
      VSX_HIP_AS("vsx_merge_pairs", hipMemcpy(dt.p, ht.data(), ht.size(), hipMemcpyHostToDevice));
      VsxMergeParams P {};
      P.truncqual = o.fastq_truncqual; P.maxns = o.fastq_maxns; P.minlen = o.fastq_minlen; P.maxlen = o.fastq_maxlen;
      P.minovlen = o.fastq_minovlen; P.maxdiffs = o.fastq_maxdiffs; P.minmergelen = o.fastq_minmergelen; P.maxmergelen = o.fastq_maxmergelen;
      P.maxdiffpct = o.fastq_maxdiffpct; P.maxee = o.fastq_maxee; P.minscore = H.minscore;
      P.ascii = (int32_t) o.fastq_ascii; P.qmin = (int32_t) o.fastq_qmin; P.qmax = (int32_t) o.fastq_qmax;
      P.mindiagcount = H.mindiagcount; P.allowstagger = o.fastq_allowmergestagger ? 1 : 0; P.tlo = tlo; P.tdim = D;
      P.match = reinterpret_cast<const double *>(dt.p); P.mism = P.match + dd; P.q2p = P.mism + dd;
      P.qual_same = reinterpret_cast<const uint8_t *>(P.q2p + 128); P.qual_diff = P.qual_same + dd16;

      const uint64_t window = o.window > 0 ? (uint64_t) o.window : 32768;
      Slot slot[2];
      for (Slot & s : slot) { const int rc = s.create("vsx_merge_pairs"); if (rc != VSX_OK) return rc; }
      // (fixed windows of `window` pairs: the pairs are packed, so no span limits a window)
      const int rc = vsxp::run_windows(slot, n,
        [&](uint64_t w0) { vsxp::Window W; W.n = std::min(window, n - w0); return W; },
        [&](Slot & s, Slot &, uint64_t w0, const vsxp::Window & W) { return submit_window(s, in, P, w0, W.n); },
        [&](Slot & s) { return collect_window(s, in, H, T, ob); },
        g_stats.windows);
      if (rc != VSX_OK) return rc;
    }

  out->n = n; out->rec = ob.rec; out->seq_blob = ob.seq; out->qual_blob = ob.qual; out->blob_bytes = ob.used;
  ob.rec = nullptr; ob.seq = nullptr; ob.qual = nullptr;
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
