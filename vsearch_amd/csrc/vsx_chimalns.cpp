// vsx_chimalns.cpp -- the --uchimealns alignment block of chimera records (include/vsx_chimalns.h): selection, re-alignment of every
// selected query with its two parents (vsx_chimera.cpp's align_pairs: one plan per window), the routes, and the host restatement of
// the reference's loops (core/chimera.cpp:761-875 maxi and the parents' rows, :1258-1276 the query row, :1281-1360 ignore / lower case
// / diffs, :1366-1495 the column scan, :1523-1570 votes / model / crossover, :1741-1795 the line ends).
//
//   per window   pairs (query, parent_a), (query, parent_b) of the selected records -> hit records + run words; the run words come to
//                the host as well: the exact alnlen of every record (the layout of the text and of the line ends), the checks the
//                kernel relies on, and the host route all read them
//   kernel       vsx_chimalns.hip, one workgroup per record, straight from the exported run words and the texts on the device
//   host         a pair the 16-bit aligner refused (vsx_lma_align), a query above VSX_CHIMERA_MAX_QLEN, an alignment above
//                VSX_CHIMALNS_MAX_COLS, VSX_CHIMALNS=host
// Whatever the route, the recomputed h and counts must equal the record's.
#include "../../include/vsx_chimalns.h"
#include "vsx_chimalns_internal.h"
#include "vsx_internal.h"
#include "vsx_private.h"

#include <hip/hip_runtime.h>
#include <atomic>

#pragma clang fp contract(off)

using vsxp::fail;
using vsxp::now_s;
using vsxp::map4;
using vsxp::ambiguous4;
using vsxp::DevBuf;

namespace {

thread_local vsx_chimalns_stats g_stats {};

typedef std::vector<uint32_t> Runs;        // run words in TEXT order

// CIGAR text (vsx_lma_align) -> run words in text order
Runs runs_from_cigar(const char * s)
{
  Runs out;
  while (*s)
    {
      uint32_t n = 0;
      bool digits = false;
      while (*s >= '0' && *s <= '9') { n = n * 10 + (uint32_t) (*s - '0'); ++s; digits = true; }
      if (!digits) n = 1;
      if (!*s) break;
      const char op = *s++;
      out.push_back((n << 2) | (op == 'M' ? 0u : op == 'I' ? 1u : 2u));
    }
  return out;
}

// what both routes rely on: the runs span the two sequences, none is empty, no two target-only runs are adjacent
bool runs_ok(const Runs & r, uint32_t qlen, uint32_t tlen)
{
  uint64_t qn = 0, tn = 0;
  uint32_t prev = 3;
  for (uint32_t w : r)
    {
      const uint32_t len = w >> 2, op = w & 3u;
      if (len == 0 || op > 2u || (op == 1u && prev == 1u)) return false;
      if (op != 1u) qn += len;
      if (op != 2u) tn += len;
      prev = op;
    }
  return qn == qlen && tn == tlen;
}

// query length + the longer target-only run in front of each position (both lists ascend in the query position)
uint64_t alnlen_of(const Runs & ra, const Runs & rb, uint32_t qlen)
{
  std::vector<std::pair<uint32_t, uint32_t>> ia, ib;
  for (int p = 0; p < 2; ++p)
    {
      uint32_t pos = 0;
      for (uint32_t w : p ? rb : ra)
        {
          if ((w & 3u) == 1u) (p ? ib : ia).emplace_back(pos, w >> 2);
          else pos += w >> 2;
        }
    }
  uint64_t total = qlen;
  size_t x = 0, y = 0;
  while (x < ia.size() || y < ib.size())
    {
      if (y == ib.size() || (x < ia.size() && ia[x].first < ib[y].first)) total += ia[x++].second;
      else if (x == ia.size() || ib[y].first < ia[x].first) total += ib[y++].second;
      else { total += std::max(ia[x].second, ib[y].second); ++x; ++y; }
    }
  return total;
}

inline char upcase(char c) { return ((c | 0x20) >= 'a' && (c | 0x20) <= 'z') ? (char) (c & 0xDF) : 'N'; }      // chrmap_upcase

struct Block {
  uint32_t alnlen = 0;
  std::vector<char> rows;                  // A, Q, B, Diffs, Votes, Model
  std::vector<uint32_t> line_end;          // A, Q, B per line
  int best_i = -1;
  double h = -1.0;
  int counts[6] = {0, 0, 0, 0, 0, 0};
  bool scored = false, reverse = false;
};

// The reference's loops on one (query, parent A, parent B) triple; runs[p] in text order, checked by runs_ok.  With reverse set (the
// parents were not given in the record's order) nothing behind the column scan is filled in.
void render_host(const char * q, int L, const char * const t[2], const Runs runs[2], double xn, double dn, int alignwidth, Block & B)
{
  // fill_max_alignment_length, find_total_alignment_length
  std::vector<int> maxi((size_t) L + 1, 0);
  for (int p = 0; p < 2; ++p)
    {
      int pos = 0;
      for (uint32_t w : runs[p])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 1) maxi[(size_t) pos] = std::max(len, maxi[(size_t) pos]);
          else pos += len;
        }
    }
  int alnlen = L;
  for (int m : maxi) alnlen += m;
  B.alnlen = (uint32_t) alnlen;
  B.rows.assign((size_t) alnlen * 6, ' ');
  char * paln[2] = {B.rows.data(), B.rows.data() + (size_t) alnlen * 2};
  char * qaln = B.rows.data() + (size_t) alnlen;
  char * diffs = B.rows.data() + (size_t) alnlen * 3, * votes = diffs + alnlen, * model = votes + alnlen;

  // fill_alignment_parents
  for (int p = 0; p < 2; ++p)
    {
      char * aln = paln[p];
      bool is_inserted = false;
      int qpos = 0, tpos = 0, alnpos = 0;
      for (uint32_t w : runs[p])
        {
          const int len = (int) (w >> 2), op = (int) (w & 3u);
          if (op == 1)
            {
              for (int j = 0; j < maxi[(size_t) qpos]; ++j) aln[alnpos++] = j < len ? upcase(t[p][tpos++]) : '-';
              is_inserted = true;
            }
          else
            for (int j = 0; j < len; ++j)
              {
                if (!is_inserted) { std::fill_n(aln + alnpos, maxi[(size_t) qpos], '-'); alnpos += maxi[(size_t) qpos]; }
                aln[alnpos++] = op == 0 ? upcase(t[p][tpos++]) : '-';
                ++qpos;
                is_inserted = false;
              }
        }
      if (!is_inserted) { std::fill_n(aln + alnpos, maxi[(size_t) qpos], '-'); alnpos += maxi[(size_t) qpos]; }
    }
  // the query row
  {
    char * o = qaln;
    for (int i = 0; i < L; ++i)
      {
        for (int j = 0; j < maxi[(size_t) i]; ++j) *o++ = '-';
        *o++ = upcase(q[i]);
      }
    for (int j = 0; j < maxi[(size_t) L]; ++j) *o++ = '-';
  }
  // ignore, lower-cased parents, diffs
  std::vector<uint8_t> ignore((size_t) alnlen, 0);
  for (int i = 0; i < alnlen; ++i)
    {
      const uint8_t qsym = map4((unsigned char) qaln[i]), p1sym = map4((unsigned char) paln[0][i]), p2sym = map4((unsigned char) paln[1][i]);
      if (qsym == 0 || p1sym == 0 || p2sym == 0)
        {
          ignore[(size_t) i] = 1;
          if (i > 0) ignore[(size_t) i - 1] = 1;
          if (i < alnlen - 1) ignore[(size_t) i + 1] = 1;
        }
      if (ambiguous4(qsym) || ambiguous4(p1sym) || ambiguous4(p2sym)) ignore[(size_t) i] = 1;
      if (p1sym != 0 && p1sym != qsym) paln[0][i] = (char) (paln[0][i] | 0x20);
      if (p2sym != 0 && p2sym != qsym) paln[1][i] = (char) (paln[1][i] | 0x20);
      char diff = ' ';
      if (qsym != 0 && p1sym != 0 && p2sym != 0)
        {
          if (p1sym == p2sym) diff = qsym == p1sym ? ' ' : 'N';
          else diff = qsym == p1sym ? 'A' : (qsym == p2sym ? 'B' : '?');
        }
      diffs[i] = diff;
    }
  // the column scan
  int sumA = 0, sumB = 0, sumN = 0;
  for (int i = 0; i < alnlen; ++i)
    {
      if (ignore[(size_t) i]) continue;
      if (diffs[i] == 'A') ++sumA;
      else if (diffs[i] == 'B') ++sumB;
      else if (diffs[i] != ' ') ++sumN;
    }
  int left_n = 0, left_a = 0, left_y = 0, right_n = sumA, right_a = sumN, right_y = sumB;
  double best_h = -1;
  int best_i = -1;
  bool best_is_reverse = false;
  for (int i = 0; i < alnlen; ++i)
    {
      if (ignore[(size_t) i] || diffs[i] == ' ') continue;
      const char d = diffs[i];
      if (d == 'A') { ++left_y; --right_n; }
      else if (d == 'B') { ++left_n; --right_y; }
      else { ++left_a; --right_a; }
      if ((left_y > left_n) && (right_y > right_n))
        {
          const double left_h = left_y / ((xn * (left_n + dn)) + left_a);
          const double right_h = right_y / ((xn * (right_n + dn)) + right_a);
          const double h = left_h * right_h;
          if (h > best_h)
            {
              best_is_reverse = false; best_h = h; best_i = i;
              B.counts[0] = left_y; B.counts[1] = left_n; B.counts[2] = left_a;
              B.counts[3] = right_y; B.counts[4] = right_n; B.counts[5] = right_a;
            }
        }
      else if ((left_n > left_y) && (right_n > right_y))
        {
          const double left_h = left_n / ((xn * (left_y + dn)) + left_a);
          const double right_h = right_n / ((xn * (right_y + dn)) + right_a);
          const double h = left_h * right_h;
          if (h > best_h)
            {
              best_is_reverse = true; best_h = h; best_i = i;
              B.counts[0] = left_n; B.counts[1] = left_y; B.counts[2] = left_a;
              B.counts[3] = right_n; B.counts[4] = right_y; B.counts[5] = right_a;
            }
        }
    }
  B.h = best_h;
  B.best_i = best_i;
  B.scored = best_h >= 0.0;
  B.reverse = best_is_reverse;
  if (!B.scored || B.reverse) return;
  // votes and model, lower-cased diffs, the crossover
  for (int i = 0; i < alnlen; ++i)
    {
      const char m = i <= best_i ? 'A' : 'B';
      model[i] = m;
      char v = ' ';
      if (!ignore[(size_t) i])
        {
          const char d = diffs[i];
          if (d == 'A' || d == 'B') v = d == m ? '+' : '!';
          else if (d == 'N' || d == '?') v = '0';
        }
      votes[i] = v;
      if (v == '!') diffs[i] = (char) (diffs[i] | 0x20);
    }
  for (int i = best_i + 1; i < alnlen; ++i)
    {
      if (diffs[i] == ' ' || diffs[i] == 'A') model[i] = 'x';
      else break;
    }
  // the line ends
  const int width = alignwidth > 0 ? alignwidth : alnlen;
  int qpos = 0, p1pos = 0, p2pos = 0;
  for (int i = 0; i < alnlen; i += width)
    {
      const int w = std::min(alnlen - i, width);
      for (int j = 0; j < w; ++j)
        {
          if (qaln[i + j] != '-') ++qpos;
          if (paln[0][i + j] != '-') ++p1pos;
          if (paln[1][i + j] != '-') ++p2pos;
        }
      B.line_end.push_back((uint32_t) p1pos);
      B.line_end.push_back((uint32_t) qpos);
      B.line_end.push_back((uint32_t) p2pos);
    }
}

inline uint64_t lines_of(uint64_t alnlen, int alignwidth) { return alignwidth > 0 ? (alnlen + (uint64_t) alignwidth - 1) / (uint64_t) alignwidth : 1; }

// the result under construction: vectors, copied into the caller's malloc'ed arrays at the end
struct Building {
  std::vector<uint64_t> record, text_off, line_first;
  std::vector<uint32_t> alnlen, line_end;
  std::vector<char> text;
  std::vector<int32_t> best_i, counts;
  std::vector<double> h;
};

template <typename T>
bool give(T *& dst, const std::vector<T> & v)
{
  dst = vsxp::host_array<T>(v.size());
  if (!dst) return false;
  if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
  return true;
}

int finish(Building & G, vsx_chimalns_out * out)
{
  G.line_first.push_back(G.line_end.size() / 3);
  out->n = G.record.size();
  out->text_bytes = G.text.size();
  out->n_lines = G.line_end.size() / 3;
  if (!give(out->record, G.record) || !give(out->alnlen, G.alnlen) || !give(out->text_off, G.text_off) || !give(out->text, G.text) ||
      !give(out->line_first, G.line_first) || !give(out->line_end, G.line_end) || !give(out->best_i, G.best_i) || !give(out->h, G.h) ||
      !give(out->counts, G.counts))
    {
      vsx_chimalns_out_free(out);
      return fail(VSX_ENOMEM, "vsx_chimera_alns: out of host memory");
    }
  return VSX_OK;
}

// a rendered record joins the result: the layout first (reserve), the bytes when its route has them
void reserve_record(Building & G, uint64_t rec, uint32_t alnlen, int alignwidth)
{
  G.record.push_back(rec);
  G.alnlen.push_back(alnlen);
  G.text_off.push_back(G.text.size());
  G.line_first.push_back(G.line_end.size() / 3);
  G.text.resize(G.text.size() + (size_t) alnlen * 6);
  G.line_end.resize(G.line_end.size() + 3 * lines_of(alnlen, alignwidth));
  G.best_i.push_back(-1);
  G.h.push_back(0.0);
  G.counts.resize(G.counts.size() + 6, 0);
}

int opts_check(const vsx_chimalns_opts * O, const char * who)
{
  if (!O) return fail(VSX_EINVAL, "%s: null options", who);
  if (!(O->xn > 0.0) || !(O->dn >= 0.0)) return fail(VSX_EINVAL, "%s: xn must be > 0, dn >= 0", who);
  if (O->alignwidth < 0) return fail(VSX_EINVAL, "%s: alignwidth must be >= 0", who);
  if (O->select & ~(VSX_CHIMALNS_Y | VSX_CHIMALNS_BORDERLINE | VSX_CHIMALNS_N)) return fail(VSX_EINVAL, "%s: unknown bits in select", who);
  if (O->window < 0 || O->threads < 0) return fail(VSX_EINVAL, "%s: window and threads must be >= 0", who);
  return VSX_OK;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the recomputed values against the record the caller gave
int verify(uint64_t k, const vsx_chimera_result & r, bool scored, bool reverse, double h, const int32_t * c)
{
  if (!scored) return fail(VSX_EINVAL, "vsx_chimera_alns: record %llu: no column gives an h score for these sequences", (unsigned long long) k);
  if (reverse) return fail(VSX_EINVAL, "vsx_chimera_alns: record %llu: parent_a and parent_b are not in the record's order", (unsigned long long) k);
  if (!same_bits(h, r.score) || c[0] != r.left_yes || c[1] != r.left_no || c[2] != r.left_abstain || c[3] != r.right_yes || c[4] != r.right_no ||
      c[5] != r.right_abstain)
    return fail(VSX_EINVAL, "vsx_chimera_alns: record %llu: the recomputed score (%.17g; %d %d %d / %d %d %d) differs from the record's (%.17g; %d %d %d / %d %d %d)",
                (unsigned long long) k, h, c[0], c[1], c[2], c[3], c[4], c[5], r.score, r.left_yes, r.left_no, r.left_abstain, r.right_yes,
                r.right_no, r.right_abstain);
  return VSX_OK;
}

// the kernel route of one window: jobs up, the kernel, the verdicts, then rows and line ends down.  check(x, rec) judges job x's
// verdict before anything of it is fetched (a record that was not rendered left its bytes unwritten).
struct KernelRoute {
  DevBuf<uint8_t> d_text;
  DevBuf<VsxChimAlnJob> d_jobs;
  DevBuf<VsxChimAlnRec> d_rec;
  DevBuf<uint32_t> d_lines;

  template <class Check>
  int run(const char * who, hipStream_t st, const std::vector<VsxChimAlnJob> & jobs, uint64_t ktext, uint64_t klines, const uint8_t * d_qtext,
          uint64_t qtext_bytes, const uint8_t * d_dbtext, uint64_t dbbytes, const uint32_t * d_runs, uint64_t nruns, const vsx_chimalns_opts & O,
          Check && check, std::vector<VsxChimAlnRec> & recs, std::vector<char> & text, std::vector<uint32_t> & lines)
  {
    double t0 = now_s();
    VSX_HIP_AS(who, d_jobs.ensure(jobs.size()));
    VSX_HIP_AS(who, d_rec.ensure(jobs.size()));
    VSX_HIP_AS(who, d_text.ensure(ktext));
    VSX_HIP_AS(who, d_lines.ensure(3 * klines));
    VSX_HIP_AS(who, hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(VsxChimAlnJob), hipMemcpyHostToDevice, st));
    VSX_HIP_AS(who, vsx_launch_chimalns(d_jobs.p, (uint32_t) jobs.size(), d_qtext, qtext_bytes, d_dbtext, dbbytes, d_runs, nruns, O.xn, O.dn,
                                        d_text.p, d_lines.p, d_rec.p, st));
    VSX_HIP_AS(who, hipStreamSynchronize(st));
    g_stats.seconds_kernel += now_s() - t0;
    t0 = now_s();
    recs.resize(jobs.size());
    VSX_HIP_AS(who, hipMemcpy(recs.data(), d_rec.p, recs.size() * sizeof(VsxChimAlnRec), hipMemcpyDeviceToHost));
    for (size_t x = 0; x < jobs.size(); ++x)
      {
        if (recs[x].status == VSX_CHIMALN_BAD_JOB) return fail(VSX_EHIP, "%s: the kernel refused job %zu", who, x);
        const int rc = check(x, recs[x]);
        if (rc != VSX_OK) return rc;
      }
    text.resize(ktext);
    lines.resize(3 * klines);
    VSX_HIP_AS(who, hipMemcpy(text.data(), d_text.p, ktext, hipMemcpyDeviceToHost));
    VSX_HIP_AS(who, hipMemcpy(lines.data(), d_lines.p, 3 * klines * 4, hipMemcpyDeviceToHost));
    g_stats.seconds_download += now_s() - t0;
    return VSX_OK;
  }
};

}  // namespace

extern "C" {

void vsx_chimalns_opts_default(vsx_chimalns_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->xn = 8.0;
  o->dn = 1.4;
  o->alignwidth = 80;
  o->select = VSX_CHIMALNS_Y;
}

void vsx_chimalns_out_free(vsx_chimalns_out * o)
{
  if (!o) return;
  std::free(o->record); std::free(o->alnlen); std::free(o->text_off); std::free(o->text); std::free(o->line_first);
  std::free(o->line_end); std::free(o->best_i); std::free(o->h); std::free(o->counts);
  std::memset(o, 0, sizeof *o);
}

void vsx_chimalns_last_stats(vsx_chimalns_stats * out) { if (out) *out = g_stats; }

int vsx_internal_chimalns_host(const char * q, uint32_t qlen, const char * a, uint32_t alen, const char * b, uint32_t blen,
                               const char * cigar_a, const char * cigar_b, const vsx_chimalns_opts * O, vsx_chimalns_out * out)
{
  const char * who = "vsx_internal_chimalns_host";
  int rc = opts_check(O, who);
  if (rc != VSX_OK) return rc;
  if (!out || !q || !a || !b || !cigar_a || !cigar_b || qlen == 0) return fail(VSX_EINVAL, "%s: null argument or empty query", who);
  std::memset(out, 0, sizeof *out);
  const Runs runs[2] = {runs_from_cigar(cigar_a), runs_from_cigar(cigar_b)};
  if (!runs_ok(runs[0], qlen, alen) || !runs_ok(runs[1], qlen, blen)) return fail(VSX_EINVAL, "%s: a CIGAR does not span its two sequences", who);
  const char * const t[2] = {a, b};
  Block B;
  render_host(q, (int) qlen, t, runs, O->xn, O->dn, O->alignwidth, B);
  if (!B.scored) return fail(VSX_EINVAL, "%s: no column gives an h score", who);
  if (B.reverse) return fail(VSX_EINVAL, "%s: the reverse branch wins: give the parents in the record's order", who);
  Building G;
  reserve_record(G, 0, B.alnlen, O->alignwidth);
  std::memcpy(G.text.data(), B.rows.data(), B.rows.size());
  std::copy(B.line_end.begin(), B.line_end.end(), G.line_end.begin());
  G.best_i[0] = B.best_i;
  G.h[0] = B.h;
  std::copy(B.counts, B.counts + 6, G.counts.begin());
  return finish(G, out);
}

int vsx_internal_chimalns_device(vsx_ctx * ctx, uint64_t n, const char * const * q, const uint32_t * qlen, const char * const * a,
                                 const uint32_t * alen, const char * const * b, const uint32_t * blen, const char * const * cigar_a,
                                 const char * const * cigar_b, const vsx_chimalns_opts * O, vsx_chimalns_out * out)
{
  const char * who = "vsx_internal_chimalns_device";
  g_stats = vsx_chimalns_stats {};
  int rc = opts_check(O, who);
  if (rc != VSX_OK) return rc;
  if (!ctx || !out || (n && (!q || !qlen || !a || !alen || !b || !blen || !cigar_a || !cigar_b))) return fail(VSX_EINVAL, "%s: null argument", who);
  std::memset(out, 0, sizeof *out);
  // one text for queries and parents, the run words in the order a plan exports them: last column first
  std::string text;
  std::vector<uint32_t> runs;
  std::vector<VsxChimAlnJob> jobs(n);
  Building G;
  uint64_t ktext = 0, klines = 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      const Runs r[2] = {runs_from_cigar(cigar_a[k]), runs_from_cigar(cigar_b[k])};
      if (qlen[k] == 0 || !runs_ok(r[0], qlen[k], alen[k]) || !runs_ok(r[1], qlen[k], blen[k]))
        return fail(VSX_EINVAL, "%s: triple %llu: a CIGAR does not span its two sequences", who, (unsigned long long) k);
      const uint64_t alnlen = alnlen_of(r[0], r[1], qlen[k]);
      if (qlen[k] > VSX_CHIMERA_MAX_QLEN || alnlen > VSX_CHIMALNS_MAX_COLS)
        return fail(VSX_EINVAL, "%s: triple %llu is beyond the kernel (host route)", who, (unsigned long long) k);
      VsxChimAlnJob & J = jobs[k];
      J = VsxChimAlnJob {};
      J.q_off = text.size(); text.append(q[k], qlen[k]);
      J.a_off = text.size(); text.append(a[k], alen[k]);
      J.b_off = text.size(); text.append(b[k], blen[k]);
      J.runs_a = runs.size(); runs.insert(runs.end(), r[0].rbegin(), r[0].rend());
      J.runs_b = runs.size(); runs.insert(runs.end(), r[1].rbegin(), r[1].rend());
      J.nruns_a = (uint32_t) r[0].size();
      J.nruns_b = (uint32_t) r[1].size();
      J.text_off = ktext;
      J.line_off = klines;
      J.qlen = qlen[k]; J.alen = alen[k]; J.blen = blen[k];
      J.alnlen = (uint32_t) alnlen;
      J.width = O->alignwidth > 0 ? (uint32_t) O->alignwidth : (uint32_t) alnlen;
      ktext += alnlen * 6;
      klines += lines_of(alnlen, O->alignwidth);
      reserve_record(G, k, (uint32_t) alnlen, O->alignwidth);
    }
  if (n)
    {
      VSX_HIP_AS(who, hipSetDevice(vsx_internal_device(ctx)));
      hipStream_t st = vsx_internal_stream(ctx);
      DevBuf<uint8_t> d_text;
      DevBuf<uint32_t> d_runs;
      VSX_HIP_AS(who, vsxp::upload(d_text, reinterpret_cast<const uint8_t *>(text.data()), text.size(), st));
      VSX_HIP_AS(who, vsxp::upload(d_runs, runs.data(), runs.size(), st));
      KernelRoute K;
      std::vector<VsxChimAlnRec> recs;
      std::vector<char> ktextbuf;
      std::vector<uint32_t> klinebuf;
      rc = K.run(who, st, jobs, ktext, klines, d_text.p, text.size(), d_text.p, text.size(), d_runs.p, runs.size(), *O,
                 [&](size_t x, const VsxChimAlnRec & r) {
                   if (r.status != VSX_CHIMALN_OK) return fail(VSX_EINVAL, "%s: triple %zu: no column gives an h score", who, x);
                   if (r.reverse) return fail(VSX_EINVAL, "%s: triple %zu: the reverse branch wins: give the parents in the record's order", who, x);
                   return (int) VSX_OK;
                 }, recs, ktextbuf, klinebuf);
      if (rc != VSX_OK) return rc;
      std::memcpy(G.text.data(), ktextbuf.data(), ktext);                    // (the same layout: every triple is rendered, in order)
      std::memcpy(G.line_end.data(), klinebuf.data(), 12 * klines);
      for (uint64_t k = 0; k < n; ++k)
        {
          G.best_i[k] = recs[k].best_i;
          G.h[k] = recs[k].h;
          std::copy(recs[k].counts, recs[k].counts + 6, G.counts.begin() + 6 * (ptrdiff_t) k);
        }
      g_stats.records_kernel = n;
    }
  return finish(G, out);
}

int vsx_chimera_alns(vsx_searcher * S, const vsx_chimalns_opts * O, uint64_t n, const char * qblob, uint64_t qbytes,
                     const uint64_t * qoff, const uint32_t * qlen, const vsx_chimera_result * records, vsx_chimalns_out * out)
{
  const char * who = "vsx_chimera_alns";
  g_stats = vsx_chimalns_stats {};
  const double t_begin = now_s();
  int rc = opts_check(O, who);
  if (rc != VSX_OK) return rc;
  if (!S || !out || (n && !records)) return fail(VSX_EINVAL, "%s: null argument", who);
  std::memset(out, 0, sizeof *out);
  const bool denovo = qblob == nullptr;
  if (!denovo && n && (!qoff || !qlen)) return fail(VSX_EINVAL, "%s: null argument", who);
  const char * dbtext;
  const uint64_t * dboff;
  const uint32_t * dblen;
  vsx_internal_searcher_text(S, &dbtext, &dboff, &dblen);
  const vsx_seqset * dbset = vsx_internal_searcher_dbset(S);
  const uint64_t ndb = vsx_seqset_count(dbset);
  if (denovo && n != ndb) return fail(VSX_EINVAL, "%s: the de novo form takes one record per sequence of the searcher", who);
  uint64_t dbbytes = 0;
  for (uint64_t i = 0; i < ndb; ++i) dbbytes = std::max(dbbytes, dboff[i] + dblen[i]);
  const char * qtext = denovo ? dbtext : qblob;
  const uint64_t * qo = denovo ? dboff : qoff;
  const uint32_t * ql = denovo ? dblen : qlen;
  const uint64_t qtext_bytes = denovo ? dbbytes : qbytes;

  // selection
  const uint32_t select = O->select ? O->select : VSX_CHIMALNS_Y;
  std::vector<uint64_t> sel;
  for (uint64_t k = 0; k < n; ++k)
    {
      const vsx_chimera_result & r = records[k];
      if (r.status != VSX_CHIMERA_SCORED) continue;
      const uint32_t bit = r.flag == 'Y' ? VSX_CHIMALNS_Y : r.flag == '?' ? VSX_CHIMALNS_BORDERLINE : VSX_CHIMALNS_N;
      if (!(select & bit)) continue;
      if (r.parent_a >= ndb || r.parent_b >= ndb) return fail(VSX_EINVAL, "%s: record %llu names a parent outside the database", who, (unsigned long long) k);
      if ((rc = vsxp::check_spans(who, "query", 1, qo + k, ql + k, qtext_bytes)) != VSX_OK) return rc;      // (selected records only)
      if (ql[k] == 0) return fail(VSX_EINVAL, "%s: record %llu: empty query", who, (unsigned long long) k);
      sel.push_back(k);
    }
  g_stats.records_selected = sel.size();
  Building G;
  if (sel.empty())
    {
      rc = finish(G, out);
      g_stats.seconds_total = now_s() - t_begin;
      return rc;
    }

  vsx_ctx * ctx = vsx_internal_searcher_ctx(S);
  const vsx_scoring * sc = vsx_internal_searcher_scoring(S);
  const bool host_all = vsxp::env_is_host("VSX_CHIMALNS");
  const uint64_t window = O->window > 0 ? (uint64_t) O->window : 4096;
  const int nth = std::max(1, O->threads > 0 ? (int) O->threads : vsxp::usable_cpus());
  VSX_HIP_AS(who, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  // the texts on the device: the database once per call, the queries of the reference-based form as well
  DevBuf<uint8_t> d_dbtext, d_qtext;
  KernelRoute K;
  bool texts_up = false;

  for (uint64_t w0 = 0; w0 < sel.size(); w0 += window)
    {
      const uint64_t nw = std::min<uint64_t>(window, sel.size() - w0);
      ++g_stats.windows;
      // ---- re-alignment: (query, parent_a), (query, parent_b) ----
      double t0 = now_s();
      std::vector<uint32_t> qidx(2 * nw), tidx(2 * nw);
      vsx_seqset * wset = nullptr;
      struct SetGuard { vsx_seqset * s; ~SetGuard() { vsx_seqset_destroy(s); } } sg {nullptr};
      if (!denovo)
        {
          std::string wblob;
          std::vector<uint64_t> woff(nw);
          std::vector<uint32_t> wlen(nw);
          for (uint64_t j = 0; j < nw; ++j)
            {
              const uint64_t k = sel[w0 + j];
              woff[j] = wblob.size();
              wlen[j] = ql[k];
              wblob.append(qtext + qo[k], ql[k]);
            }
          rc = vsx_seqset_create(ctx, &wset, nw, wblob.data(), wblob.size(), woff.data(), wlen.data());
          if (rc != VSX_OK) return rc;
          sg.s = wset;
        }
      for (uint64_t j = 0; j < nw; ++j)
        {
          const uint64_t k = sel[w0 + j];
          qidx[2 * j] = qidx[2 * j + 1] = denovo ? (uint32_t) k : (uint32_t) j;
          tidx[2 * j] = records[k].parent_a;
          tidx[2 * j + 1] = records[k].parent_b;
        }
      VsxRealigned * R = nullptr;
      rc = vsx_internal_chimera_realign(S, denovo ? dbset : wset, qidx, tidx, who, &R);
      struct RGuard { VsxRealigned * r; ~RGuard() { vsx_internal_chimera_realigned_free(r); } } rg {R};
      if (rc != VSX_OK) return rc;
      const VsxPairOut * hits;
      const uint32_t * d_runs;
      uint64_t nruns;
      vsx_internal_chimera_realigned_view(R, &hits, &d_runs, &nruns);
      std::vector<uint32_t> h_runs(nruns);
      if (nruns) VSX_HIP_AS(who, hipMemcpy(h_runs.data(), d_runs, nruns * 4, hipMemcpyDeviceToHost));
      // run words in text order per pair; a refused pair through the scalar aligner
      std::vector<Runs> pr(2 * nw);
      std::vector<uint8_t> sentinel(nw, 0);
      for (uint64_t j = 0; j < nw; ++j)
        {
          const uint64_t k = sel[w0 + j];
          for (int p = 0; p < 2; ++p)
            {
              const VsxPairOut & h = hits[2 * j + p];
              const uint32_t tg = tidx[2 * j + p];
              if (h.score == VSX_SCORE_SENTINEL)
                {
                  sentinel[j] = 1;
                  ++g_stats.sentinel_pairs;
                  int64_t score, alen, ma, mi, ga;
                  char * cig = nullptr;
                  rc = vsx_lma_align(sc, qtext + qo[k], ql[k], dbtext + dboff[tg], dblen[tg], &score, &alen, &ma, &mi, &ga, &cig);
                  if (rc != VSX_OK) return rc;
                  pr[2 * j + p] = runs_from_cigar(cig);
                  std::free(cig);
                }
              else
                pr[2 * j + p].assign(h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off - h.nruns), h_runs.rbegin() + (ptrdiff_t) (nruns - h.run_off));
              if (!runs_ok(pr[2 * j + p], ql[k], dblen[tg]))
                return fail(VSX_EHIP, "%s: record %llu: the alignment with parent %u does not span the two sequences", who, (unsigned long long) k, tg);
            }
        }
      g_stats.seconds_align += now_s() - t0;

      // ---- layout and routes ----
      const size_t g0 = G.record.size();
      std::vector<VsxChimAlnJob> jobs;
      std::vector<size_t> job_rec, host_rec;
      uint64_t ktext = 0, klines = 0;
      for (uint64_t j = 0; j < nw; ++j)
        {
          const uint64_t k = sel[w0 + j];
          const uint64_t alnlen = alnlen_of(pr[2 * j], pr[2 * j + 1], ql[k]);
          if (alnlen > 0x7FFFFFFFull / 6) return fail(VSX_EINVAL, "%s: record %llu: alignment too long", who, (unsigned long long) k);
          reserve_record(G, k, (uint32_t) alnlen, O->alignwidth);
          const bool long_q = ql[k] > VSX_CHIMERA_MAX_QLEN, long_a = alnlen > VSX_CHIMALNS_MAX_COLS;
          if (host_all || sentinel[j] || long_q || long_a)
            {
              if (host_all) ++g_stats.host_forced;
              else if (sentinel[j]) {}
              else if (long_q) ++g_stats.host_long_query;
              else ++g_stats.host_long_alignment;
              host_rec.push_back(j);
              continue;
            }
          VsxChimAlnJob J {};
          J.q_off = qo[k];
          J.a_off = dboff[records[k].parent_a];
          J.b_off = dboff[records[k].parent_b];
          J.runs_a = hits[2 * j].run_off;
          J.runs_b = hits[2 * j + 1].run_off;
          J.nruns_a = hits[2 * j].nruns;
          J.nruns_b = hits[2 * j + 1].nruns;
          J.text_off = ktext;
          J.line_off = klines;
          J.qlen = ql[k];
          J.alen = dblen[records[k].parent_a];
          J.blen = dblen[records[k].parent_b];
          J.alnlen = (uint32_t) alnlen;
          J.width = O->alignwidth > 0 ? (uint32_t) O->alignwidth : (uint32_t) alnlen;
          ktext += alnlen * 6;
          klines += lines_of(alnlen, O->alignwidth);
          jobs.push_back(J);
          job_rec.push_back(j);
        }

      // ---- kernel route ----
      if (!jobs.empty())
        {
          t0 = now_s();
          if (!texts_up)
            {
              VSX_HIP_AS(who, vsxp::upload(d_dbtext, reinterpret_cast<const uint8_t *>(dbtext), dbbytes, st));
              if (!denovo) VSX_HIP_AS(who, vsxp::upload(d_qtext, reinterpret_cast<const uint8_t *>(qblob), qbytes, st));
              texts_up = true;
            }
          std::vector<VsxChimAlnRec> recs;
          std::vector<char> ktextbuf;
          std::vector<uint32_t> klinebuf;
          rc = K.run(who, st, jobs, ktext, klines, denovo ? d_dbtext.p : d_qtext.p, qtext_bytes, d_dbtext.p, dbbytes, d_runs, nruns, *O,
                     [&](size_t x, const VsxChimAlnRec & r) {
                       const uint64_t k = sel[w0 + job_rec[x]];
                       return verify(k, records[k], r.status == VSX_CHIMALN_OK, r.reverse != 0, r.h, r.counts);
                     }, recs, ktextbuf, klinebuf);
          if (rc != VSX_OK) return rc;
          for (size_t x = 0; x < jobs.size(); ++x)
            {
              const size_t g = g0 + job_rec[x];
              const VsxChimAlnJob & J = jobs[x];
              std::memcpy(G.text.data() + G.text_off[g], ktextbuf.data() + J.text_off, (size_t) J.alnlen * 6);
              std::memcpy(G.line_end.data() + 3 * G.line_first[g], klinebuf.data() + 3 * J.line_off, 12 * lines_of(J.alnlen, O->alignwidth));
              G.best_i[g] = recs[x].best_i;
              G.h[g] = recs[x].h;
              std::copy(recs[x].counts, recs[x].counts + 6, G.counts.begin() + 6 * (ptrdiff_t) g);
            }
          g_stats.records_kernel += jobs.size();
        }

      // ---- host route ----
      if (!host_rec.empty())
        {
          t0 = now_s();
          std::atomic<size_t> next {0};
          std::vector<int> codes(host_rec.size(), VSX_OK);
          std::vector<Block> blocks(host_rec.size());
          vsxp::run_pool(std::min<int>(nth, (int) host_rec.size()), [&](int) {
            for (size_t x = next++; x < host_rec.size(); x = next++)
              {
                const uint64_t j = host_rec[x], k = sel[w0 + j];
                const char * const t[2] = {dbtext + dboff[records[k].parent_a], dbtext + dboff[records[k].parent_b]};
                const Runs runs[2] = {pr[2 * j], pr[2 * j + 1]};
                render_host(qtext + qo[k], (int) ql[k], t, runs, O->xn, O->dn, O->alignwidth, blocks[x]);
              }
          });
          for (size_t x = 0; x < host_rec.size(); ++x)
            {
              const uint64_t j = host_rec[x], k = sel[w0 + j];
              const Block & B = blocks[x];
              rc = verify(k, records[k], B.scored, B.reverse, B.h, B.counts);
              if (rc != VSX_OK) return rc;
              const size_t g = g0 + j;
              std::memcpy(G.text.data() + G.text_off[g], B.rows.data(), B.rows.size());
              std::copy(B.line_end.begin(), B.line_end.end(), G.line_end.begin() + 3 * (ptrdiff_t) G.line_first[g]);
              G.best_i[g] = B.best_i;
              G.h[g] = B.h;
              std::copy(B.counts, B.counts + 6, G.counts.begin() + 6 * (ptrdiff_t) g);
            }
          g_stats.records_host += host_rec.size();
          g_stats.seconds_host += now_s() - t0;
        }
    }
  rc = finish(G, out);
  g_stats.seconds_total = now_s() - t_begin;
  return rc;
}

}  // extern "C"
