// vsx_chimalns.hip -- the --uchimealns alignment block of one chimera record per workgroup (include/vsx_chimalns.h): the three-row
// alignment of the query with parent A and parent B, the rows Diffs / Votes / Model, the end positions of every output line and the
// recomputed h (reference core/chimera.cpp:761-875, :1258-1570, :1741-1795).  The host form is chimalns_host in vsx_chimalns.cpp.
//
// Unlike the scoring kernel (vsx_chimera.hip, query-position space) this one works in COLUMN space, as the reference's loops do:
//
//   maxi[0 .. L]   the longer of the two parents' target-only runs in front of each query position.  One wave per parent takes the
//                  alignment's run words 64 at a time, one per lane; a wave scan of the lengths gives every run its first query and
//                  target position, with carries from chunk to chunk (any number of runs); the lanes holding target-only runs raise
//                  maxi with an LDS max.
//   col[i]         the column of query position i = i + sum maxi[0 .. i], a workgroup scan in place; alnlen = col[L].
//   rows           three byte rows in LDS, '-' everywhere first.  Q: position i at col[i].  A parent: a second walk over the same
//                  chunks, the runs of a chunk handed round the wave, lanes over the run's symbols: an M run puts symbol j at
//                  col[q + j], a target-only run of r symbols at col[q] - maxi[q] + j (left-aligned in the maxi columns), a
//                  query-only run leaves the '-'.  Everything through map_uppercase.
//   per column     4-bit codes of the three bytes; gap = some code is 0; ignored = a gap here or in a neighbouring column, or an
//                  ambiguous code; parent symbols that differ from the query are lower-cased (ignored columns too); diff class.
//   counts, h      a workgroup prefix scan over the columns of the A / B / abstain votes packed into one 64-bit word (21 bits each),
//                  h in both orientations with the reference's doubles, arg-max = largest h, then lowest column.  The same loop
//                  scans the non-gap bytes of the three rows and writes the end positions where an output line ends.
//   votes, model   per column; the crossover run 'x' starts behind best_i and ends at the first column whose diff, AFTER the
//                  lower-casing of '!' votes, is neither ' ' nor 'A': a min-reduction.
//   stores         six rows to HBM, lane = column.
//
// LDS atomics only (max, add, min of integers: the result does not depend on their order); no global atomics: two calls give the
// same bytes.  Every shuffle is executed by all 64 lanes of its wave.  LDS: 3 x 8 KiB rows + 8 KiB column flags + 16 KiB col[] +
// 5 KiB arg-max slots = ~53 KiB per 256-thread workgroup, 3 workgroups per CU.
#include "vsx_chimalns_internal.h"
#include "../../include/vsx_chimalns.h"

#include <hip/hip_runtime.h>
#include "vsx_devutil.h"
#include "vsx_symbols.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

#define DEV __device__ __forceinline__

constexpr int CA_THREADS = 256;
constexpr int CA_WAVES = CA_THREADS / 64;
constexpr u32 CA_LMAX = VSX_CHIMERA_MAX_QLEN;
constexpr u32 CA_CMAX = VSX_CHIMALNS_MAX_COLS;
constexpr u64 M21 = (1ull << 21) - 1;
static_assert(CA_CMAX < (1u << 21) && CA_LMAX < CA_CMAX, "layout");

// column flags: bits 0-1 diff class (0 ' ', 1 'A', 2 'B', 3 'N' / '?'), 2: class 3 is '?', 3: gap column, 4: gap or ambiguous here
constexpr u32 F_QMARK = 4u, F_GAP = 8u, F_SELF = 16u;

using vsxd::lane_id;
using vsxd::wave_incl_sum;
using vsxsym::ambiguous4;
using vsxsym::map4;
using vsxsym::upcase;

// maxi[i] from the scanned col[]: col[i] - col[i - 1] = 1 + maxi[i]
DEV u32 maxi_at(const u32 * col, u32 i) { return i ? col[i] - col[i - 1] - 1u : col[0]; }

// One wave over one alignment (nruns run words, stored last column first, `words` = the first stored one).  FILL = false: maxi (in
// col[]) is raised to every target-only run's length.  FILL = true: col[] is scanned; the parent's symbols go to their columns of row.
template <bool FILL>
DEV void walk_runs(const u32 * __restrict__ words, u32 nruns, const uint8_t * __restrict__ t, u32 tl, u32 L, u32 alnlen, u32 * col, uint8_t * row)
{
  const u32 lane = lane_id();
  u32 sum_q = 0, sum_t = 0;
  for (u32 base = 0; base < nruns; base += 64u)
    {
      const u32 k = base + lane;
      const bool have = k < nruns;
      const u32 w = have ? words[nruns - 1u - k] : 0u;
      const u32 len = w >> 2, op = w & 3u;
      const u32 dq = op != 1u ? len : 0u, dt = op != 2u ? len : 0u;
      const u32 iq = wave_incl_sum(dq), it = wave_incl_sum(dt);
      const u32 qs = sum_q + (iq - dq), ts = sum_t + (it - dt);
      sum_q += (u32) __shfl((int) iq, 63, 64);
      sum_t += (u32) __shfl((int) it, 63, 64);
      if (!FILL)
        {
          if (have && op == 1u && qs <= L) atomicMax(&col[qs], len);
          continue;
        }
      const u32 cnt = nruns - base < 64u ? nruns - base : 64u;
      for (u32 r = 0; r < cnt; ++r)                                           // (uniform: every lane runs every turn)
        {
          const u32 rw = (u32) __shfl((int) w, (int) r, 64), rq = (u32) __shfl((int) qs, (int) r, 64), rt = (u32) __shfl((int) ts, (int) r, 64);
          const u32 rlen = rw >> 2, rop = rw & 3u;
          if (rop == 0u)
            {
              for (u32 j = lane; j < rlen; j += 64u)
                {
                  const u32 qp = rq + j, tp = rt + j;
                  if (qp < L && tp < tl)
                    {
                      const u32 c = col[qp];
                      if (c < alnlen) row[c] = (uint8_t) upcase(t[tp]);
                    }
                }
            }
          else if (rop == 1u && rq <= L)
            {
              const u32 m = maxi_at(col, rq);
              const u32 c0 = col[rq] - m;
              for (u32 j = lane; j < rlen && j < m; j += 64u)
                {
                  const u32 tp = rt + j, c = c0 + j;
                  if (tp < tl && c < alnlen) row[c] = (uint8_t) upcase(t[tp]);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(CA_THREADS)
vsx_chimalns_kernel(const VsxChimAlnJob * __restrict__ jobs, const uint8_t * __restrict__ qtext, u64 qtext_bytes, const uint8_t * __restrict__ dbtext,
                    u64 dbtext_bytes, const u32 * __restrict__ runs, u64 n_runs, double xn, double dn, uint8_t * __restrict__ text,
                    u32 * __restrict__ line_end, VsxChimAlnRec * __restrict__ recs)
{
  __shared__ u32 s_col[CA_LMAX + 1];
  __shared__ __align__(16) uint8_t s_row[3][CA_CMAX];          // Q, A, B
  __shared__ uint8_t s_cat[CA_CMAX];
  __shared__ u64 s_tot, s_wsum[CA_WAVES];
  __shared__ u32 s_xend;
  __shared__ int s_best;
  __shared__ double s_h[CA_THREADS];
  __shared__ int s_i[CA_THREADS];
  __shared__ u64 s_pk[CA_THREADS];

  const VsxChimAlnJob J = jobs[blockIdx.x];
  VsxChimAlnRec * rec = recs + blockIdx.x;
  const u32 tid = threadIdx.x, wave = tid >> 6;
  const u32 L = J.qlen, alnlen = J.alnlen;
  // (the host sends no such job; nothing of it is read or written)
  const bool bad = L == 0u || L > CA_LMAX || alnlen < L || alnlen > CA_CMAX || J.width == 0u || J.q_off + L > qtext_bytes ||
                   J.a_off + J.alen > dbtext_bytes || J.b_off + J.blen > dbtext_bytes || J.runs_a + J.nruns_a > n_runs || J.runs_b + J.nruns_b > n_runs;
  if (bad)
    {
      if (tid == 0) { VsxChimAlnRec z = {}; z.best_i = -1; z.status = VSX_CHIMALN_BAD_JOB; *rec = z; }
      return;
    }
  const uint8_t * __restrict__ q = qtext + J.q_off;
  const uint8_t * __restrict__ ta = dbtext + J.a_off;
  const uint8_t * __restrict__ tb = dbtext + J.b_off;
  uint8_t * qrow = s_row[0], * arow = s_row[1], * brow = s_row[2];

  // ---- maxi ----
  for (u32 i = tid; i <= L; i += CA_THREADS) s_col[i] = 0u;
  for (u32 c = tid; c < alnlen; c += CA_THREADS) { qrow[c] = '-'; arow[c] = '-'; brow[c] = '-'; }
  if (tid == 0) { s_tot = 0ull; s_xend = alnlen; }
  __syncthreads();
  if (wave == 0) walk_runs<false>(runs + J.runs_a, J.nruns_a, ta, J.alen, L, alnlen, s_col, arow);
  else if (wave == 1) walk_runs<false>(runs + J.runs_b, J.nruns_b, tb, J.blen, L, alnlen, s_col, brow);
  __syncthreads();

  // ---- col[i] = i + sum maxi[0 .. i] ----
  {
    u64 carry = 0ull;
    for (u32 base = 0; base <= L; base += CA_THREADS)
      {
        const u32 i = base + tid;
        const u64 v = i <= L ? (u64) s_col[i] + 1ull : 0ull;
        u64 chunk = 0ull;
        const u64 incl = vsxd::block_scan<CA_WAVES>(v, s_wsum, &chunk) + carry;
        carry += chunk;
        if (i <= L) s_col[i] = (u32) (incl - 1ull);
      }
  }
  __syncthreads();
  if (s_col[L] != alnlen)                                     // (uniform)
    {
      if (tid == 0) { VsxChimAlnRec z = {}; z.best_i = -1; z.alnlen = s_col[L]; z.status = VSX_CHIMALN_BAD_JOB; *rec = z; }
      return;
    }

  // ---- rows ----
  for (u32 i = tid; i < L; i += CA_THREADS)
    {
      const u32 c = s_col[i];
      if (c < alnlen) qrow[c] = (uint8_t) upcase(q[i]);
    }
  if (wave == 0) walk_runs<true>(runs + J.runs_a, J.nruns_a, ta, J.alen, L, alnlen, s_col, arow);
  else if (wave == 1) walk_runs<true>(runs + J.runs_b, J.nruns_b, tb, J.blen, L, alnlen, s_col, brow);
  __syncthreads();

  // ---- per column: codes, gap / ambiguity, lower-cased parents, diff class ----
  for (u32 c = tid; c < alnlen; c += CA_THREADS)
    {
      const u32 ab = arow[c], bb = brow[c];
      const u32 qv = map4(qrow[c]), av = map4(ab), bv = map4(bb);
      const bool gap = qv == 0u || av == 0u || bv == 0u;
      const bool self = gap || ambiguous4(qv) || ambiguous4(av) || ambiguous4(bv);
      if (av != 0u && av != qv) arow[c] = (uint8_t) (ab | 0x20u);
      if (bv != 0u && bv != qv) brow[c] = (uint8_t) (bb | 0x20u);
      u32 cls = 0u, qm = 0u;
      if (!gap)
        {
          if (av == bv) cls = qv == av ? 0u : 3u;
          else if (qv == av) cls = 1u;
          else if (qv == bv) cls = 2u;
          else { cls = 3u; qm = F_QMARK; }
        }
      s_cat[c] = (uint8_t) (cls | qm | (gap ? F_GAP : 0u) | (self ? F_SELF : 0u));
    }
  __syncthreads();
  // ignored: a gap or an ambiguous code here, or a gap in a neighbouring column
  auto ignored = [&](u32 c) -> bool {
    return (s_cat[c] & F_SELF) || (c > 0u && (s_cat[c - 1u] & F_GAP)) || (c + 1u < alnlen && (s_cat[c + 1u] & F_GAP));
  };
  {
    u64 tot_local = 0ull;
    for (u32 c = tid; c < alnlen; c += CA_THREADS)
      {
        const u32 cls = s_cat[c] & 3u;
        if (cls && !ignored(c)) tot_local += 1ull << (21 * (cls - 1u));
      }
    if (tot_local) atomicAdd(&s_tot, tot_local);
  }
  __syncthreads();
  const u64 tot = s_tot;
  const int sumA = (int) (tot & M21), sumB = (int) ((tot >> 21) & M21), sumN = (int) (tot >> 42);

  // ---- left / right counts by prefix scan, h per column in both orientations; the non-gap symbols of the rows, line ends ----
  double bh = -1.0;
  int bi = -1;
  u64 bpk = 0ull;
  {
    u64 carry = 0ull, gcarry = 0ull;
    u32 * __restrict__ le = line_end + 3ull * J.line_off;
    for (u32 base = 0; base < alnlen; base += CA_THREADS)
      {
        const u32 c = base + tid;
        u64 v = 0ull, g = 0ull;
        if (c < alnlen)
          {
            const u32 cls = s_cat[c] & 3u;
            if (cls && !ignored(c)) v = 1ull << (21 * (cls - 1u));
            g = (arow[c] != '-' ? 1ull : 0ull) | (qrow[c] != '-' ? 1ull << 21 : 0ull) | (brow[c] != '-' ? 1ull << 42 : 0ull);
          }
        u64 chunk = 0ull, gchunk = 0ull;
        const u64 incl = vsxd::block_scan<CA_WAVES>(v, s_wsum, &chunk) + carry;
        const u64 gincl = vsxd::block_scan<CA_WAVES>(g, s_wsum, &gchunk) + gcarry;
        carry += chunk;
        gcarry += gchunk;
        if (c < alnlen && ((c + 1u) % J.width == 0u || c + 1u == alnlen))
          {
            const u64 l = c / J.width;
            le[3ull * l + 0] = (u32) (gincl & M21);
            le[3ull * l + 1] = (u32) ((gincl >> 21) & M21);
            le[3ull * l + 2] = (u32) (gincl >> 42);
          }
        if (v)
          {
            const int left_y = (int) (incl & M21), left_n = (int) ((incl >> 21) & M21), left_a = (int) (incl >> 42);
            const int right_n = sumA - left_y, right_y = sumB - left_n, right_a = sumN - left_a;
            if ((left_y > left_n) && (right_y > right_n))
              {
                const double left_h = left_y / ((xn * (left_n + dn)) + left_a);
                const double right_h = right_y / ((xn * (right_n + dn)) + right_a);
                const double h = left_h * right_h;
                if (h > bh) { bh = h; bi = (int) c; bpk = incl; }
              }
            else if ((left_n > left_y) && (right_n > right_y))
              {
                const double left_h = left_n / ((xn * (left_y + dn)) + left_a);
                const double right_h = right_n / ((xn * (right_y + dn)) + right_a);
                const double h = left_h * right_h;
                if (h > bh) { bh = h; bi = (int) c; bpk = incl | (1ull << 63); }
              }
          }
      }
  }
  s_h[tid] = bh;
  s_i[tid] = bi;
  s_pk[tid] = bpk;
  __syncthreads();
  if (tid == 0)
    {
      int bt = -1;
      for (int t = 0; t < CA_THREADS; ++t)
        if (s_i[t] >= 0 && (bt < 0 || s_h[t] > s_h[bt] || (s_h[t] == s_h[bt] && s_i[t] < s_i[bt]))) bt = t;
      s_best = bt;
    }
  __syncthreads();
  const int bt = s_best;
  if (bt < 0)
    {
      if (tid == 0) { VsxChimAlnRec z = {}; z.best_i = -1; z.alnlen = alnlen; z.status = VSX_CHIMALN_NO_SCORE; *rec = z; }
      return;
    }
  const int best_i = s_i[bt];
  const bool rev = (s_pk[bt] >> 63) != 0ull;

  // ---- crossover: the first column behind best_i whose diff (after the lower-casing of '!') is neither ' ' nor 'A'.  Behind best_i
  // the model is B: an 'A' that votes becomes 'a', only an ignored one stays ----
  {
    u32 first = alnlen;
    for (u32 c = (u32) best_i + 1u + tid; c < alnlen; c += CA_THREADS)
      {
        const u32 cls = s_cat[c] & 3u;
        if (cls >= 2u || (cls == 1u && !ignored(c))) { first = c; break; }
      }
    if (first < alnlen) atomicMin(&s_xend, first);
  }
  __syncthreads();
  const u32 xend = s_xend;

  // ---- votes, model, lower-cased diffs; the six rows to HBM, lane = column ----
  uint8_t * __restrict__ out = text + J.text_off;
  for (u32 c = tid; c < alnlen; c += CA_THREADS)
    {
      const u32 f = s_cat[c], cls = f & 3u;
      const bool left = (int) c <= best_i;
      u32 d = cls == 0u ? (u32) ' ' : cls == 1u ? (u32) 'A' : cls == 2u ? (u32) 'B' : ((f & F_QMARK) ? (u32) '?' : (u32) 'N');
      u32 vote = ' ';
      if (!ignored(c))
        {
          if (cls == 1u || cls == 2u) vote = (cls == 1u) == left ? (u32) '+' : (u32) '!';
          else if (cls == 3u) vote = '0';
        }
      if (vote == '!') d |= 0x20u;
      const u32 model = left ? (u32) 'A' : (c < xend ? (u32) 'x' : (u32) 'B');
      out[c] = arow[c];
      out[(u64) alnlen + c] = qrow[c];
      out[2ull * alnlen + c] = brow[c];
      out[3ull * alnlen + c] = (uint8_t) d;
      out[4ull * alnlen + c] = (uint8_t) vote;
      out[5ull * alnlen + c] = (uint8_t) model;
    }
  if (tid != 0) return;
  const u64 pk = s_pk[bt] & ~(1ull << 63);
  const int left_y = (int) (pk & M21), left_n = (int) ((pk >> 21) & M21), left_a = (int) (pk >> 42);
  const int right_n = sumA - left_y, right_y = sumB - left_n, right_a = sumN - left_a;
  VsxChimAlnRec r = {};
  r.h = s_h[bt];
  r.best_i = best_i;
  r.counts[0] = rev ? left_n : left_y;
  r.counts[1] = rev ? left_y : left_n;
  r.counts[2] = left_a;
  r.counts[3] = rev ? right_n : right_y;
  r.counts[4] = rev ? right_y : right_n;
  r.counts[5] = right_a;
  r.alnlen = alnlen;
  r.reverse = rev ? 1u : 0u;
  r.status = VSX_CHIMALN_OK;
  *rec = r;
}

}  // namespace

extern "C" hipError_t vsx_launch_chimalns(const VsxChimAlnJob * d_jobs, uint32_t n, const uint8_t * d_qtext, uint64_t qtext_bytes, const uint8_t * d_dbtext,
                                          uint64_t dbtext_bytes, const uint32_t * d_runs, uint64_t n_runs, double xn, double dn, uint8_t * d_text,
                                          uint32_t * d_line_end, VsxChimAlnRec * d_rec, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_chimalns_kernel, dim3(n), dim3(CA_THREADS), 0, st, d_jobs, d_qtext, (u64) qtext_bytes, d_dbtext, (u64) dbtext_bytes, d_runs,
                     (u64) n_runs, xn, dn, d_text, d_line_end, d_rec);
  return hipGetLastError();
}
