// vsx_hitout.cpp -- alignment rows, symbol rows and MD strings of search hits (include/vsx_hitout.h): the host side of
// vsx_hitout.hip and the host restatement.
//
// Restated from the reference (src/, v2.31.0): core/showalign.cpp (get_alignment_row :151-176, get_aligment_symbol :122-137, the
// query symbol of a minus-strand hit :179-185,345), core/results.cpp (the trimmed rows :100-155,459-481, build_sam_strings :791-920)
// and core/search.cpp:294-303 (each strand of a query is masked on its own).
//
// Both routes share the O(runs) staging: every CIGAR is parsed into run words and checked against the two lengths, the trimmed column
// range is derived, the offsets of the rows are laid out.  The device route then runs hits in windows: jobs and run words up, the
// row kernel, MD count -> scan -> fill, rows and strings down.  The host route walks every hit column by column on host threads; it
// is written from the reference's loops and not from the kernels.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "../../include/vsx_hitout.h"
#include "vsx_hitout_internal.h"
#include "vsx_private.h"
#include "vsx_search_internal.h"

using vsxp::array_of;
using vsxp::fail;
using vsxp::now_s;

// what a searcher keeps between calls: grow-only device buffers, the database text uploaded once
struct VsxHitoutIndex {
  vsxp::DevBuf<uint8_t> dbtext, qtext, rows, md, temp;
  vsxp::DevBuf<uint32_t> runs, md_len;
  vsxp::DevBuf<uint64_t> md_off;
  vsxp::DevBuf<VsxHitJob> jobs;
  bool db_uploaded = false;
};

namespace {

constexpr const char * WHO = "vsx_hits_render";
constexpr uint64_t HIT_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr uint64_t DEFAULT_WINDOW = 262144;
constexpr int HOST_THREADS = 16;

thread_local vsx_hitout_stats g_stats {};

// the database as text, the queries as given, what of the options matters
struct Input {
  uint64_t n_db; const char * db; uint64_t db_bytes; const uint64_t * db_off; const uint32_t * db_len;
  uint64_t nq; const char * qblob; uint64_t qbytes; const uint64_t * qoff; const uint32_t * qlen;
  const vsx_hits * hits;
  uint32_t want;
  int qmode;                   // 0 none, 1 soft, 2 dust
  bool hardq, both, n_mismatch;
  int nth;
  uint64_t window;
};

// everything the staging derives; the offsets are the result's
struct Staged {
  std::string qtext;                                   // plus strands, then (both) the minus strands
  std::vector<uint64_t> qplus, qminus;
  std::vector<uint32_t> runs;                          // all hits, text order
  std::vector<uint64_t> run_off;                       // n_hits + 1
  std::vector<uint32_t> ncols;
  std::vector<uint64_t> qrow, trow, sym, aln;          // result offsets (NONE where not wanted)
  std::vector<uint64_t> aln_dev;                       // what the row pass writes: NONE where the --alnout row is the qrow
  uint64_t row_bytes = 0;
};

template <typename F>
void parallel_for(int nth, uint64_t n, uint64_t grain, F && f)
{
  const int use = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) nth, n / grain + 1));
  std::atomic<uint64_t> next {0};
  vsxp::run_pool(use, [&](int) {
    for (;;)
      {
        const uint64_t k0 = next.fetch_add(grain);
        if (k0 >= n) break;
        for (uint64_t k = k0; k < std::min(n, k0 + grain); ++k) f(k);
      }
  });
}

// ---- the strands' texts ------------------------------------------------------------------------------------------------------------
void mask_queries(const Input & in, Staged & S)
{
  const uint64_t nq = in.nq;
  uint64_t total = 0;
  S.qplus.resize(nq);
  for (uint64_t q = 0; q < nq; ++q) { S.qplus[q] = total; total += in.qlen[q]; }
  if (in.both) { S.qminus.resize(nq); for (uint64_t q = 0; q < nq; ++q) S.qminus[q] = total + S.qplus[q]; }
  S.qtext.assign(in.both ? 2 * total : total, '\0');
  const bool dust = in.qmode == 2;
  parallel_for(in.nth, nq, 32, [&](uint64_t q) {
    thread_local std::vector<char> scratch;
    const uint32_t L = in.qlen[q];
    if (L == 0) return;
    char * plus = &S.qtext[S.qplus[q]];
    std::memcpy(plus, in.qblob + in.qoff[q], L);
    char * strand[2] = { plus, nullptr };
    if (in.both)
      {
        char * minus = strand[1] = &S.qtext[S.qminus[q]];
        for (uint32_t x = 0; x < L; ++x) minus[x] = vsxs::complement((unsigned char) plus[L - 1 - x]);
      }
    for (char * p : strand)
      {
        if (!p) continue;
        if (dust) vsx_internal_dust_one(p, (int64_t) L, scratch, in.hardq);
        else if (in.hardq) for (uint32_t x = 0; x < L; ++x) if (((unsigned char) p[x] & 0x20u) != 0u) p[x] = 'N';
      }
  });
}

// ---- CIGARs -> run words -----------------------------------------------------------------------------------------------------------
// the runs of one NUL-terminated CIGAR; out == NULL: their number only.  false: not a CIGAR
bool parse_cigar(const char * p, const char * end, uint32_t * out, uint64_t & nruns, uint64_t & cols, uint64_t & sq, uint64_t & st)
{
  nruns = cols = sq = st = 0;
  while (p < end && *p)
    {
      uint64_t len = 0;
      bool digits = false;
      while (p < end && *p >= '0' && *p <= '9') { len = len * 10 + (uint64_t) (*p - '0'); digits = true; if (len >= (1u << 30)) return false; ++p; }
      if (!digits) len = 1;
      if (p >= end || len == 0) return false;
      uint32_t op;
      switch (*p) { case 'M': op = 0; sq += len; st += len; break; case 'I': op = 1; st += len; break; case 'D': op = 2; sq += len; break; default: return false; }
      ++p;
      cols += len;
      if (cols >= (1ull << 31)) return false;
      if (out) out[nruns] = (uint32_t) (len << 2) | op;
      ++nruns;
    }
  return p < end;                                      // the terminator lies inside the blob
}

int stage(const Input & in, Staged & S)
{
  const vsx_hits & H = *in.hits;
  const uint64_t nh = H.n_hits;
  const char * cig_end = H.cigar_blob + H.cigar_bytes;
  // which query lists hit h
  for (uint64_t q = 0; q < in.nq; ++q)
    {
      if (H.first[q] > H.first[q + 1] || H.first[q + 1] > nh) return fail(VSX_EINVAL, "%s: hits.first does not ascend to n_hits", WHO);
      for (uint64_t h = H.first[q]; h < H.first[q + 1]; ++h)
        if (H.hit[h].query != q) return fail(VSX_EINVAL, "%s: hit %llu is listed under query %llu and names query %u", WHO, (unsigned long long) h, (unsigned long long) q, H.hit[h].query);
    }
  if ((in.nq ? H.first[0] : 0) != 0 || (in.nq ? H.first[in.nq] : 0) != nh) return fail(VSX_EINVAL, "%s: hits.first does not cover the hits", WHO);
  // pass 1: count the runs, refuse what is out of range
  S.run_off.assign(nh + 1, 0);
  std::atomic<int> bad {0};
  parallel_for(in.nth, nh, 1024, [&](uint64_t h) {
    const vsx_hit & x = H.hit[h];
    uint64_t n = 0, c, a, b;
    if (x.target >= in.n_db || x.cigar_off >= H.cigar_bytes || (x.strand && !in.both) || !parse_cigar(H.cigar_blob + x.cigar_off, cig_end, nullptr, n, c, a, b))
      { bad.store(1); return; }
    S.run_off[h + 1] = n;
  });
  if (bad.load()) return fail(VSX_EINVAL, "%s: a hit names a target or a CIGAR that is not there, or a strand that was not searched", WHO);
  for (uint64_t h = 0; h < nh; ++h) S.run_off[h + 1] += S.run_off[h];
  S.runs.resize(S.run_off[nh]);
  S.ncols.resize(nh);
  // pass 2: the run words, the sums against the lengths, the trimmed range
  parallel_for(in.nth, nh, 1024, [&](uint64_t h) {
    const vsx_hit & x = H.hit[h];
    uint64_t n, cols, sq, st;
    parse_cigar(H.cigar_blob + x.cigar_off, cig_end, S.runs.data() + S.run_off[h], n, cols, sq, st);
    S.ncols[h] = (uint32_t) cols;
    const int64_t c0 = (int64_t) x.trim_q_left + x.trim_t_left;
    if (sq != in.qlen[x.query] || st != in.db_len[x.target]) bad.store(2);
    else if (x.trim_q_left < 0 || x.trim_t_left < 0 || x.internal_alignmentlength < 0 || c0 + x.internal_alignmentlength > (int64_t) cols) bad.store(3);
  });
  if (bad.load() == 2) return fail(VSX_EINVAL, "%s: a CIGAR's runs do not sum to the lengths of its query and target", WHO);
  if (bad.load() == 3) return fail(VSX_EINVAL, "%s: a hit's trimmed columns do not lie inside its alignment", WHO);
  // the rows' places
  const bool rows = (in.want & VSX_HITOUT_ROWS) != 0, syms = (in.want & VSX_HITOUT_SYMBOLS) != 0;
  if (rows) { S.qrow.resize(nh); S.trow.resize(nh); }
  if (syms) { S.sym.resize(nh); S.aln.resize(nh); S.aln_dev.resize(nh); }
  uint64_t at = 0;
  for (uint64_t h = 0; h < nh; ++h)
    {
      const uint64_t L = (uint64_t) H.hit[h].internal_alignmentlength;
      if (rows) { S.qrow[h] = at; S.trow[h] = at + L; at += 2 * L; }
      if (syms)
        {
          S.sym[h] = at; at += L;
          if (H.hit[h].strand || !rows) { S.aln[h] = S.aln_dev[h] = at; at += L; }
          else { S.aln[h] = S.qrow[h]; S.aln_dev[h] = VSX_HITOUT_NONE; }
        }
    }
  S.row_bytes = at;
  return VSX_OK;
}

// ---- the host restatement ----------------------------------------------------------------------------------------------------------
inline char host_symbol(unsigned char qc, unsigned char tc, bool n_mismatch)
{
  const uint8_t q = vsxp::map4(qc), t = vsxp::map4(tc);
  if (n_mismatch && (q == 15 || t == 15)) return ' ';
  if (q == t && !vsxp::ambiguous4(q)) return '|';
  if ((q & t) != 0) return '+';
  return ' ';
}

// one hit, run by run as the reference's loops go
void host_rows(const Input & in, const Staged & S, uint64_t h, char * row_blob)
{
  const vsx_hit & x = in.hits->hit[h];
  const uint32_t ql = in.qlen[x.query];
  const char * qs = S.qtext.data() + (x.strand ? S.qminus[x.query] : S.qplus[x.query]);
  const char * qp = S.qtext.data() + S.qplus[x.query];
  const char * ts = in.db + in.db_off[x.target];
  const int64_t c0 = (int64_t) x.trim_q_left + x.trim_t_left, c1 = c0 + x.internal_alignmentlength;
  char * qrow = S.qrow.empty() ? nullptr : row_blob + S.qrow[h];
  char * trow = S.trow.empty() ? nullptr : row_blob + S.trow[h];
  char * sym = S.sym.empty() ? nullptr : row_blob + S.sym[h];
  char * aln = (S.aln_dev.empty() || S.aln_dev[h] == VSX_HITOUT_NONE) ? nullptr : row_blob + S.aln_dev[h];
  int64_t col = 0;
  uint64_t qpos = 0, tpos = 0;
  for (uint64_t r = S.run_off[h]; r < S.run_off[h + 1]; ++r)
    {
      const uint32_t op = S.runs[r] & 3u;
      for (uint32_t k = S.runs[r] >> 2; k != 0; --k, ++col)
        {
          const char qc = op != 1 ? qs[qpos] : '-', tc = op != 2 ? ts[tpos] : '-';
          if (col >= c0 && col < c1)
            {
              const int64_t i = col - c0;
              if (qrow) qrow[i] = qc;
              if (trow) trow[i] = tc;
              if (sym)
                {
                  char ac = qc;
                  if (x.strand && op != 1) ac = vsxs::complement((unsigned char) qp[ql - 1 - qpos]);
                  sym[i] = op == 0 ? host_symbol((unsigned char) ac, (unsigned char) tc, in.n_mismatch) : ' ';
                  if (aln) aln[i] = ac;
                }
            }
          if (op != 1) ++qpos;
          if (op != 2) ++tpos;
        }
    }
}

// build_sam_strings' MD half (results.cpp:791-920)
void host_md(const Input & in, const Staged & S, uint64_t h, std::string & md)
{
  const vsx_hit & x = in.hits->hit[h];
  const char * qs = S.qtext.data() + (x.strand ? S.qminus[x.query] : S.qplus[x.query]);
  const char * ts = in.db + in.db_off[x.target];
  uint64_t qpos = 0, tpos = 0;
  unsigned matched = 0;
  bool flag = false;                                   // the string ends with a number
  md.clear();
  for (uint64_t r = S.run_off[h]; r < S.run_off[h + 1]; ++r)
    {
      const uint32_t op = S.runs[r] & 3u, run = S.runs[r] >> 2;
      if (op == 0)
        for (uint32_t k = 0; k < run; ++k, ++qpos, ++tpos)
          {
            if (vsxp::map4((unsigned char) qs[qpos]) == vsxp::map4((unsigned char) ts[tpos])) { ++matched; continue; }
            if (!flag) { md += std::to_string(matched); matched = 0; }
            md += ts[tpos];
            flag = false;
          }
      else if (op == 2) qpos += run;
      else
        {
          if (!flag) { md += std::to_string(matched); matched = 0; }
          md += '^';
          md.append(ts + tpos, run);
          tpos += run;
          flag = false;
        }
    }
  if (!flag) md += std::to_string(matched);
}

template <typename T>
bool copy_out(T *& dst, const std::vector<T> & v)
{
  dst = array_of<T>(v.size());
  if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
  return dst != nullptr;
}

void release(vsx_hit_text * t)
{
  std::free(t->row_blob); std::free(t->row_len); std::free(t->qrow_off); std::free(t->trow_off); std::free(t->sym_off); std::free(t->aln_off);
  std::free(t->md_blob); std::free(t->md_off); std::free(t->md_len); std::free(t->qtext); std::free(t->qplus_off); std::free(t->qminus_off);
  std::memset(t, 0, sizeof *t);
}

// what both routes hand out before the rows and strings are made
int begin_result(const Input & in, const Staged & S, vsx_hit_text & out)
{
  const uint64_t nh = in.hits->n_hits;
  out.n_queries = in.nq; out.n_hits = nh; out.want = in.want; out.both = in.both ? 1 : 0;
  out.row_len = array_of<uint32_t>(nh);
  out.qtext = array_of<char>(S.qtext.size());
  bool ok = out.row_len && out.qtext && copy_out(out.qplus_off, S.qplus);
  if (ok && in.both) ok = copy_out(out.qminus_off, S.qminus);
  if (ok && (in.want & VSX_HITOUT_ROWS)) ok = copy_out(out.qrow_off, S.qrow) && copy_out(out.trow_off, S.trow);
  if (ok && (in.want & VSX_HITOUT_SYMBOLS)) ok = copy_out(out.sym_off, S.sym) && copy_out(out.aln_off, S.aln);
  if (ok && (in.want & (VSX_HITOUT_ROWS | VSX_HITOUT_SYMBOLS))) { out.row_blob = array_of<char>(S.row_bytes); ok = out.row_blob != nullptr; }
  if (ok && (in.want & VSX_HITOUT_SAM)) { out.md_off = array_of<uint64_t>(nh); out.md_len = array_of<uint32_t>(nh); ok = out.md_off && out.md_len; }
  if (!ok) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  out.row_bytes = (in.want & (VSX_HITOUT_ROWS | VSX_HITOUT_SYMBOLS)) ? S.row_bytes : 0;
  out.qtext_bytes = S.qtext.size();
  if (!S.qtext.empty()) std::memcpy(out.qtext, S.qtext.data(), S.qtext.size());
  for (uint64_t h = 0; h < nh; ++h) out.row_len[h] = (uint32_t) in.hits->hit[h].internal_alignmentlength;
  return VSX_OK;
}

int host_route(const Input & in, const Staged & S, vsx_hit_text & out)
{
  const double t0 = now_s();
  const uint64_t nh = in.hits->n_hits;
  if (out.row_blob) parallel_for(in.nth, nh, 256, [&](uint64_t h) { host_rows(in, S, h, out.row_blob); });
  if (in.want & VSX_HITOUT_SAM)
    {
      std::vector<std::string> md(nh);
      parallel_for(in.nth, nh, 256, [&](uint64_t h) { host_md(in, S, h, md[h]); });
      uint64_t total = 0;
      for (uint64_t h = 0; h < nh; ++h) { out.md_off[h] = total; out.md_len[h] = (uint32_t) md[h].size(); total += md[h].size(); }
      out.md_blob = array_of<char>(total);
      if (!out.md_blob) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
      out.md_bytes = total;
      parallel_for(in.nth, nh, 256, [&](uint64_t h) { std::memcpy(out.md_blob + out.md_off[h], md[h].data(), md[h].size()); });
    }
  g_stats.hits_host = nh;
  g_stats.seconds_host += now_s() - t0;
  return VSX_OK;
}

// ---- the device route --------------------------------------------------------------------------------------------------------------
// the bytes window [h0, h1) takes on the device, the MD strings at their upper bound (three bytes per column, one more number)
uint64_t window_bytes(const Input & in, const Staged & S, uint64_t h0, uint64_t h1, uint64_t rows_lo, uint64_t rows_hi)
{
  uint64_t cols = 0;
  if (in.want & VSX_HITOUT_SAM) for (uint64_t h = h0; h < h1; ++h) cols += S.ncols[h];
  return (rows_hi - rows_lo) + (S.run_off[h1] - S.run_off[h0]) * 4 + (h1 - h0) * (sizeof(VsxHitJob) + 12) + 3 * cols + 16 * (h1 - h0);
}

// where the rows of hit h begin (the rows of a hit are contiguous and the hits follow each other)
uint64_t rows_begin(const Input & in, const Staged & S, uint64_t h)
{
  if (h >= in.hits->n_hits) return S.row_bytes;
  return !S.qrow.empty() ? S.qrow[h] : !S.sym.empty() ? S.sym[h] : 0;
}

int device_route(vsx_searcher * SR, const Input & in, const Staged & S, vsx_hit_text & out)
{
  vsx_ctx * ctx = SR->ctx;
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  if (!SR->hidx) SR->hidx = new VsxHitoutIndex;
  VsxHitoutIndex & X = *SR->hidx;
  const uint64_t nh = in.hits->n_hits;
  const bool any_rows = (in.want & (VSX_HITOUT_ROWS | VSX_HITOUT_SYMBOLS)) != 0, sam = (in.want & VSX_HITOUT_SAM) != 0;
  double t0 = now_s();
  if (!X.db_uploaded)
    {
      VSX_HIP_AS(WHO, X.dbtext.alloc(in.db_bytes));
      if (in.db_bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(X.dbtext.p, in.db, in.db_bytes, hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      X.db_uploaded = true;
      g_stats.db_text_uploaded = 1;
    }
  VSX_HIP_AS(WHO, X.qtext.ensure(S.qtext.size()));
  if (!S.qtext.empty()) VSX_HIP_AS(WHO, hipMemcpyAsync(X.qtext.p, S.qtext.data(), S.qtext.size(), hipMemcpyHostToDevice, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_h2d += now_s() - t0;

  std::vector<VsxHitJob> jobs;
  std::vector<char> md_all;
  std::vector<uint64_t> woff;
  std::vector<uint32_t> wlen;
  for (uint64_t h0 = 0; h0 < nh; h0 += in.window)
    {
      const uint64_t h1 = std::min(nh, h0 + in.window), wn = h1 - h0;
      const uint64_t rows_lo = rows_begin(in, S, h0), rows_hi = rows_begin(in, S, h1), r0 = S.run_off[h0], nr = S.run_off[h1] - r0;
      // ---- jobs
      t0 = now_s();
      jobs.resize(wn);
      for (uint64_t k = 0; k < wn; ++k)
        {
          const uint64_t h = h0 + k;
          const vsx_hit & x = in.hits->hit[h];
          VsxHitJob & J = jobs[k];
          J.q_off = x.strand ? S.qminus[x.query] : S.qplus[x.query];
          J.qp_off = S.qplus[x.query];
          J.t_off = in.db_off[x.target];
          J.run_off = S.run_off[h] - r0;
          J.qrow_off = S.qrow.empty() ? VSX_HITJOB_NO : S.qrow[h] - rows_lo;
          J.trow_off = S.trow.empty() ? VSX_HITJOB_NO : S.trow[h] - rows_lo;
          J.sym_off = S.sym.empty() ? VSX_HITJOB_NO : S.sym[h] - rows_lo;
          J.aln_off = (S.aln_dev.empty() || S.aln_dev[h] == VSX_HITOUT_NONE) ? VSX_HITJOB_NO : S.aln_dev[h] - rows_lo;
          J.nruns = (uint32_t) (S.run_off[h + 1] - S.run_off[h]);
          J.qlen = in.qlen[x.query];
          J.ncols = S.ncols[h];
          J.c0 = (uint32_t) (x.trim_q_left + x.trim_t_left);
          J.ilen = (uint32_t) x.internal_alignmentlength;
          J.minus = x.strand ? 1u : 0u;
        }
      g_stats.seconds_stage += now_s() - t0;
      // ---- up
      t0 = now_s();
      VSX_HIP_AS(WHO, X.jobs.ensure(wn));
      VSX_HIP_AS(WHO, X.runs.ensure(nr));
      VSX_HIP_AS(WHO, hipMemcpyAsync(X.jobs.p, jobs.data(), wn * sizeof(VsxHitJob), hipMemcpyHostToDevice, st));
      if (nr) VSX_HIP_AS(WHO, hipMemcpyAsync(X.runs.p, S.runs.data() + r0, nr * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      g_stats.seconds_h2d += now_s() - t0;
      // ---- rows
      if (any_rows)
        {
          t0 = now_s();
          VSX_HIP_AS(WHO, X.rows.ensure(rows_hi - rows_lo));
          VSX_HIP_AS(WHO, vsx_launch_hitout_rows(X.jobs.p, (uint32_t) wn, X.qtext.p, X.dbtext.p, X.runs.p, X.rows.p, in.n_mismatch ? 1 : 0, st));
          VSX_HIP_AS(WHO, hipStreamSynchronize(st));
          g_stats.seconds_rows += now_s() - t0;
          t0 = now_s();
          if (rows_hi > rows_lo) VSX_HIP_AS(WHO, hipMemcpy(out.row_blob + rows_lo, X.rows.p, rows_hi - rows_lo, hipMemcpyDeviceToHost));
          g_stats.seconds_d2h += now_s() - t0;
        }
      // ---- MD: count, scan, fill
      if (sam)
        {
          t0 = now_s();
          size_t temp_bytes = 0;
          VSX_HIP_AS(WHO, vsx_launch_hitout_md_scan(nullptr, &temp_bytes, nullptr, nullptr, (uint32_t) wn, st));
          VSX_HIP_AS(WHO, X.temp.ensure(temp_bytes));
          VSX_HIP_AS(WHO, X.md_len.ensure(wn));
          VSX_HIP_AS(WHO, X.md_off.ensure(wn));
          temp_bytes = X.temp.n;
          VSX_HIP_AS(WHO, vsx_launch_hitout_md_count(X.jobs.p, (uint32_t) wn, X.qtext.p, X.dbtext.p, X.runs.p, X.md_len.p, st));
          VSX_HIP_AS(WHO, vsx_launch_hitout_md_scan(X.temp.p, &temp_bytes, X.md_len.p, X.md_off.p, (uint32_t) wn, st));
          woff.resize(wn); wlen.resize(wn);
          VSX_HIP_AS(WHO, hipMemcpyAsync(woff.data(), X.md_off.p, wn * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
          VSX_HIP_AS(WHO, hipMemcpyAsync(wlen.data(), X.md_len.p, wn * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
          VSX_HIP_AS(WHO, hipStreamSynchronize(st));
          g_stats.seconds_md_count += now_s() - t0;
          // the lengths are checked before a byte is written by them: a string has at most "0^" and a symbol per column, and a last number
          uint64_t total = 0;
          for (uint64_t k = 0; k < wn; ++k)
            {
              if (woff[k] != total || wlen[k] == 0 || wlen[k] > 3ull * S.ncols[h0 + k] + 12) return fail(VSX_EHIP, "%s: the MD count pass gave an impossible length", WHO);
              total += wlen[k];
            }
          t0 = now_s();
          VSX_HIP_AS(WHO, X.md.ensure(total));
          VSX_HIP_AS(WHO, vsx_launch_hitout_md_fill(X.jobs.p, (uint32_t) wn, X.qtext.p, X.dbtext.p, X.runs.p, X.md_off.p, X.md.p, st));
          VSX_HIP_AS(WHO, hipStreamSynchronize(st));
          g_stats.seconds_md_fill += now_s() - t0;
          t0 = now_s();
          const uint64_t base = md_all.size();
          md_all.resize(base + total);
          if (total) VSX_HIP_AS(WHO, hipMemcpy(md_all.data() + base, X.md.p, total, hipMemcpyDeviceToHost));
          for (uint64_t k = 0; k < wn; ++k) { out.md_off[h0 + k] = base + woff[k]; out.md_len[h0 + k] = wlen[k]; }
          g_stats.seconds_d2h += now_s() - t0;
        }
      ++g_stats.windows;
    }
  if (sam)
    {
      out.md_blob = array_of<char>(md_all.size());
      if (!out.md_blob) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
      out.md_bytes = md_all.size();
      if (!md_all.empty()) std::memcpy(out.md_blob, md_all.data(), md_all.size());
    }
  g_stats.hits_device = nh;
  return VSX_OK;
}

int check(const Input & in, const vsx_hitout_opts * o, vsx_hit_text * out)
{
  if (!o || !out || !in.hits) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if ((in.nq && (!in.qoff || !in.qlen)) || (in.qbytes && !in.qblob) || (in.n_db && (!in.db_off || !in.db_len)) || (in.db_bytes && !in.db))
    return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (o->threads < 0) return fail(VSX_EINVAL, "%s: threads cannot be negative", WHO);
  if (o->want & ~(VSX_HITOUT_ROWS | VSX_HITOUT_SYMBOLS | VSX_HITOUT_SAM)) return fail(VSX_EINVAL, "%s: unknown bit in want", WHO);
  const vsx_hits & H = *in.hits;
  if (H.n_queries != in.nq) return fail(VSX_EINVAL, "%s: %llu queries, but the hits are of %llu", WHO, (unsigned long long) in.nq, (unsigned long long) H.n_queries);
  if ((in.nq && !H.first) || (H.n_hits && (!H.hit || !H.cigar_blob || !in.nq))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  for (uint64_t q = 0; q < in.nq; ++q)
    if (in.qoff[q] > in.qbytes || in.qlen[q] > in.qbytes - in.qoff[q]) return fail(VSX_EINVAL, "%s: query %llu lies outside its blob", WHO, (unsigned long long) q);
  for (uint64_t t = 0; t < in.n_db; ++t)
    if (in.db_off[t] > in.db_bytes || in.db_len[t] > in.db_bytes - in.db_off[t]) return fail(VSX_EINVAL, "%s: target %llu lies outside its text", WHO, (unsigned long long) t);
  return VSX_OK;
}

int run(vsx_searcher * SR, Input & in, const vsx_hitout_opts * o, vsx_hit_text * out)
{
  g_stats = vsx_hitout_stats {};
  const double t_begin = now_s();
  int rc = check(in, o, out);
  if (rc != VSX_OK) return rc;
  std::memset(out, 0, sizeof *out);
  in.want = o->want;
  in.nth = o->threads > 0 ? o->threads : std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS));
  in.window = o->window ? o->window : DEFAULT_WINDOW;
  const uint64_t nh = in.hits->n_hits;

  Staged S;
  double t0 = now_s();
  mask_queries(in, S);
  g_stats.seconds_mask += now_s() - t0;
  t0 = now_s();
  rc = stage(in, S);
  g_stats.seconds_stage += now_s() - t0;
  if (rc == VSX_OK) rc = begin_result(in, S, *out);
  if (rc != VSX_OK) { release(out); return rc; }

  bool host_all = true;
  if (!SR || !SR->ctx) g_stats.host_no_context = 1;
  else
    {
      const uint64_t device_hits = std::min<uint64_t>(HIT_LIMIT, vsxp::env_u64("VSX_HITOUT_DEVICE_HITS", HIT_LIMIT, true));
      if (vsxp::env_is_host("VSX_HITOUT")) g_stats.host_environment = 1;
      else if (nh > device_hits) g_stats.host_hit_count = 1;
      else host_all = false;
      if (!host_all && nh)
        {
          uint64_t need = 0;
          for (uint64_t h0 = 0; h0 < nh; h0 += in.window)
            {
              const uint64_t h1 = std::min(nh, h0 + in.window);
              need = std::max(need, window_bytes(in, S, h0, h1, rows_begin(in, S, h0), rows_begin(in, S, h1)));
            }
          need += S.qtext.size() + ((uint64_t) 64 << 20);
          if (!SR->hidx || !SR->hidx->db_uploaded) need += in.db_bytes;
          bool fits = false;
          if ((rc = vsxp::device_fits(SR->ctx, WHO, need, "VSX_HITOUT_PRETEND_BYTES", &fits)) != VSX_OK) { release(out); return rc; }
          if (!fits) { host_all = true; g_stats.host_memory = 1; }
        }
    }
  rc = host_all ? host_route(in, S, *out) : device_route(SR, in, S, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

void masking_of(const vsx_search_opts & so, Input & in)
{
  in.qmode = so.qmask ? so.qmask - 1 : so.soft_mask;
  in.hardq = (so.hardmask & 2) != 0 && in.qmode != 0;
  in.both = so.strand_both != 0;
}

}  // namespace

void vsx_internal_hitout_index_destroy(VsxHitoutIndex * X) { delete X; }

extern "C" {

void vsx_hitout_opts_default(vsx_hitout_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->want = VSX_HITOUT_ROWS | VSX_HITOUT_SYMBOLS | VSX_HITOUT_SAM;
}

void vsx_hits_render_last_stats(vsx_hitout_stats * out) { if (out) *out = g_stats; }

void vsx_hit_text_free(vsx_hit_text * t) { if (t) release(t); }

int vsx_hits_render(vsx_searcher * s, const vsx_hitout_opts * o, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                    const uint64_t * qoffsets, const uint32_t * qlengths, const vsx_hits * hits, vsx_hit_text * out)
{
  if (!s) return fail(VSX_EINVAL, "%s: null argument", WHO);
  Input in {};
  in.n_db = s->len.size(); in.db = s->blob.data(); in.db_bytes = s->blob.empty() ? 0 : s->blob.size() - 1;
  in.db_off = s->off.data(); in.db_len = s->len.data();
  in.nq = n_queries; in.qblob = qblob; in.qbytes = qblob_bytes; in.qoff = qoffsets; in.qlen = qlengths; in.hits = hits;
  masking_of(s->o, in);
  in.n_mismatch = s->scoring.n_mismatch != 0;
  return run(s, in, o, out);
}

int vsx_internal_hits_render_host(const vsx_scoring * scoring, const vsx_search_opts * sopts, const vsx_hitout_opts * o,
                                  uint64_t n_db, const char * db_text, uint64_t db_bytes, const uint64_t * db_offsets, const uint32_t * db_lengths,
                                  uint64_t n_queries, const char * qblob, uint64_t qblob_bytes, const uint64_t * qoffsets,
                                  const uint32_t * qlengths, const vsx_hits * hits, vsx_hit_text * out)
{
  if (!scoring || !sopts) return fail(VSX_EINVAL, "%s: null argument", WHO);
  Input in {};
  in.n_db = n_db; in.db = db_text; in.db_bytes = db_bytes; in.db_off = db_offsets; in.db_len = db_lengths;
  in.nq = n_queries; in.qblob = qblob; in.qbytes = qblob_bytes; in.qoff = qoffsets; in.qlen = qlengths; in.hits = hits;
  masking_of(*sopts, in);
  in.n_mismatch = scoring->n_mismatch != 0;
  return run(nullptr, in, o, out);
}

}  // extern "C"
