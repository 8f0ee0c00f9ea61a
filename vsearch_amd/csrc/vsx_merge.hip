// vsx_merge.hip -- paired-end read merging on gfx950: one wavefront per read pair, the whole pair in LDS.
//
// The reference (core/mergepairs.cpp: process -> optimize -> merge) scores every overlap diagonal of a pair on which its 5-mer
// hash finds enough common words.  The hash only decides WHICH diagonals are scored: diags[d] is the number of length-5
// windows on diagonal d in which the forward read and the reverse-complemented reverse read carry the same 2-bit codes and no
// ambiguous symbol, so a lane counts that directly on its diagonal (a run-length count, no hash).  The floating-point work is
// sequential double additions of host-built table values; a diagonal is never split across lanes, so the sums are the
// reference's sequence of additions (-ffp-contract=off keeps them apart from the compares around them).
//
// Phases of a pair (all 64 lanes, barriers between them):
//   1. truncate / filter: first quality at or below truncqual, out-of-range quality, N count, N quality forced to the offset
//   2. stage in LDS: forward read, reverse-complemented reverse read, their qualities and 2-bit codes
//   3. census: lane per diagonal i = 1 .. fwd_trunc + rev_trunc - 1; qualifying diagonals are appended to an LDS list
//   4. scoring: lane per LISTED diagonal (on real data a handful per pair, so one round), best / hits by wave reduction --
//      "first i wins ties, strict >" is the order-free rule (greater score, then smaller i) among scores > 0
//   5. rejection chain in the reference's order, then merge: lane per merged position; the three expected-error sums are
//      order-dependent and are accumulated by one lane each, in position order
// Output: vector stores only.
#include <hip/hip_runtime.h>
#include "vsx_merge_internal.h"
#include "vsx_devutil.h"

namespace {

constexpr int MG_L = VSX_MERGE_MAX_LEN;
constexpr int MG_T = VSX_MERGE_THREADS;

using vsxd::wave_min;
using vsxd::wave_sum;

// first position p < len whose quality is out of range or at / below truncqual (len if none), as the reference's loop meets it
__device__ inline int first_stop(const uint8_t * q, int len, const VsxMergeParams & P, int lane)
{
  int first = len;
  for (int p = lane; p < len; p += MG_T)
    {
      const int v = (int) (int8_t) q[p] - P.ascii;
      if (v < P.qmin || v > P.qmax || (int64_t) v <= P.truncqual) { first = p; break; }
    }
  return wave_min(first);
}

__global__ __launch_bounds__(VSX_MERGE_THREADS)
void vsx_merge_kernel(const VsxMergeItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ blob, VsxMergeParams P,
                      VsxMergeDevRec * __restrict__ recs, uint8_t * __restrict__ oseq, uint8_t * __restrict__ oqual)
{
  __shared__ uint8_t  s_fs[MG_L], s_fq[MG_L], s_fc[MG_L];      // forward read: symbol, quality symbol, 2-bit code (4: ambiguous)
  __shared__ uint8_t  s_rs[MG_L], s_rq[MG_L], s_rc[MG_L];      // reverse read, reverse-complemented (5: ambiguous)
  __shared__ uint8_t  s_mq[2 * MG_L];                          // merged quality
  __shared__ uint16_t s_list[2 * MG_L];                        // diagonals that passed the census
  __shared__ double   s_q2p[128];
  __shared__ int      s_nlist;

  const uint32_t pair = blockIdx.x;
  if (pair >= n_items) return;
  const int lane = threadIdx.x;
  const VsxMergeItem it = items[pair];
  if (it.host) return;
  const int F = (int) it.flen, R = (int) it.rlen;
  if (F > MG_L || R > MG_L) return;                            // (the host never sends one; the LDS arrays end at MG_L)
  const uint8_t * g_fs = blob + it.in_off, * g_fq = g_fs + F, * g_rs = g_fq + F, * g_rq = g_rs + R;

  VsxMergeDevRec rec;
  rec.merged = 0; rec.reason = VSX_MERGE_OK; rec.fwd_trunc = F; rec.rev_trunc = R; rec.merged_length = 0;
  rec.fwd_errors = 0; rec.rev_errors = 0; rec.qerr = 0; rec.qerr_value = 0; rec.ndiag = 0;
  rec.ee_merged = 0.0; rec.ee_fwd = 0.0; rec.ee_rev = 0.0;

  for (int k = lane; k < 128; k += MG_T) s_q2p[k] = P.q2p[k];
  if (lane == 0) s_nlist = 0;

  // ---- 1. lengths, truncation, quality range (every decision below is wave-uniform)
  bool skip = false;
  if (F < P.minlen || R < P.minlen) { rec.reason = VSX_MERGE_MINLEN; skip = true; }
  if (F > P.maxlen || R > P.maxlen) { rec.reason = VSX_MERGE_MAXLEN; skip = true; }
  int ftr = F, rtr = R;
  for (int side = 0; side < 2 && !skip; ++side)
    {
      const uint8_t * q = side ? g_rq : g_fq;
      const int len = side ? R : F;
      const int first = first_stop(q, len, P, lane);
      if (first < len)
        {
          const int v = (int) (int8_t) q[first] - P.ascii;
          if (v < P.qmin || v > P.qmax)
            {
              rec.qerr = v < P.qmin ? 1 : 2; rec.qerr_value = v;
              rec.fwd_trunc = ftr; rec.rev_trunc = rtr;
              if (lane == 0) recs[pair] = rec;
              return;
            }
        }
      if (side) rtr = first; else ftr = first;
      if (first < P.minlen) { rec.reason = VSX_MERGE_MINLEN; skip = true; }
    }
  rec.fwd_trunc = ftr; rec.rev_trunc = rtr;

  // ---- 2. stage; N's are counted and their quality becomes the offset symbol (the reference rewrites it in place)
  if (!skip)
    {
      int nf = 0, nr = 0;
      for (int p = lane; p < ftr; p += MG_T)
        {
          const uint8_t c = vsx_mg_upcase(g_fs[p]);
          uint8_t q = g_fq[p];
          if (c == 'N') { q = (uint8_t) P.ascii; ++nf; }
          s_fs[p] = c; s_fq[p] = q; s_fc[p] = vsx_mg_code(c, 4);
        }
      for (int t = lane; t < rtr; t += MG_T)
        {
          const int r = rtr - 1 - t;
          const uint8_t c = vsx_mg_upcase(g_rs[r]);
          uint8_t q = g_rq[r];
          if (c == 'N') { q = (uint8_t) P.ascii; ++nr; }
          const uint8_t cc = vsx_mg_complement(c);
          s_rs[t] = cc; s_rq[t] = q; s_rc[t] = vsx_mg_code(cc, 5);
        }
      nf = wave_sum(nf); nr = wave_sum(nr);
      if ((int64_t) nf > P.maxns || (int64_t) nr > P.maxns) { rec.reason = VSX_MERGE_MAXNS; skip = true; }
    }
  __syncthreads();
  if (skip) { if (lane == 0) recs[pair] = rec; return; }

  // ---- 3. census.  Diagonal i: forward position f = ftr - i + t faces reverse-complement position t,
  //         t in [max(0, i - ftr), min(i, rtr))
  const int i2 = ftr + rtr - 1;
  for (int i = lane + 1; i <= i2; i += MG_T)
    {
      const int t_lo = i > ftr ? i - ftr : 0, t_hi = i < rtr ? i : rtr;
      const int shift = ftr - i;
      int run = 0, cnt = 0;
      for (int t = t_lo; t < t_hi; ++t)
        {
          run = s_fc[shift + t] == s_rc[t] ? run + 1 : 0;
          cnt += run >= 5;
        }
      if (cnt >= P.mindiagcount) s_list[atomicAdd(&s_nlist, 1)] = (uint16_t) i;
    }
  __syncthreads();
  const int nlist = s_nlist;
  rec.ndiag = nlist;

  // ---- 4. scoring, from the forward read's 3' end (t descending), the reference's order of additions
  int hits = 0, best_i = 0, best_diffs = 0;
  double best_score = 0.0;
  for (int k = lane; k < nlist; k += MG_T)
    {
      const int i = s_list[k];
      const int t_lo = i > ftr ? i - ftr : 0, t_hi = i < rtr ? i : rtr;
      const int shift = ftr - i;
      double score = 0.0, score_high = 0.0, dropmax = 0.0;
      int diffs = 0;
      for (int t = t_hi - 1; t >= t_lo; --t)
        {
          const int f = shift + t;
          const int ti = ((int) s_fq[f] - P.tlo) * P.tdim + ((int) s_rq[t] - P.tlo);
          if (s_fs[f] == s_rs[t])
            {
              score += P.match[ti];
              score_high = score > score_high ? score : score_high;
            }
          else
            {
              score += P.mism[ti];
              ++diffs;
              if (score < score_high - dropmax) dropmax = score_high - score;
            }
        }
      if (dropmax >= 16.0) score = 0.0;
      if (score >= P.minscore) ++hits;
      if (score > best_score || (score == best_score && score > 0.0 && i < best_i)) { best_score = score; best_i = i; best_diffs = diffs; }
    }
  hits = wave_sum(hits);
  for (int m = 32; m >= 1; m >>= 1)
    {
      const double os = __shfl_xor(best_score, m, 64);
      const int oi = __shfl_xor(best_i, m, 64), od = __shfl_xor(best_diffs, m, 64);
      if (os > best_score || (os == best_score && os > 0.0 && oi < best_i)) { best_score = os; best_i = oi; best_diffs = od; }
    }

  // ---- 5. the rejection chain (0 / 0 is NaN and compares false, as in the reference)
  int reason = VSX_MERGE_OK;
  const int mergelen0 = ftr + rtr - best_i;
  if (hits > 1) reason = VSX_MERGE_REPEAT;
  else if (!P.allowstagger && best_i > ftr) reason = VSX_MERGE_STAGGERED;
  else if ((int64_t) best_diffs > P.maxdiffs) reason = VSX_MERGE_MAXDIFFS;
  else if (100.0 * (double) best_diffs / (double) best_i > P.maxdiffpct) reason = VSX_MERGE_MAXDIFFPCT;
  else if (nlist == 0) reason = VSX_MERGE_NOKMERS;
  else if (best_score < P.minscore) reason = VSX_MERGE_MINSCORE;
  else if ((int64_t) best_i < P.minovlen) reason = VSX_MERGE_MINOVLEN;
  else if ((int64_t) mergelen0 < P.minmergelen) reason = VSX_MERGE_MINMERGELEN;
  else if ((int64_t) mergelen0 > P.maxmergelen) reason = VSX_MERGE_MAXMERGELEN;
  if (reason != VSX_MERGE_OK || best_i <= 0) { rec.reason = reason; if (lane == 0) recs[pair] = rec; return; }

  // ---- merge: forward 5' overhang, the overlap, the reverse read's 5' overhang
  const int f5 = ftr > best_i ? ftr - best_i : 0;              // forward bases before the overlap
  const int r3 = best_i > ftr ? best_i - ftr : 0;              // reverse-complement positions left of the forward read (dropped)
  const int nm = (ftr - f5) < (rtr - r3) ? (ftr - f5) : (rtr - r3);
  const int mergelen = f5 + (rtr - r3);
  int ferr = 0, rerr = 0;
  uint8_t * o_s = oseq + it.out_off, * o_q = oqual + it.out_off;
  for (int m = lane; m < mergelen; m += MG_T)
    {
      uint8_t sym, q;
      if (m < f5) { sym = s_fs[m]; q = s_fq[m]; }
      else if (m < f5 + nm)
        {
          const int t = r3 + (m - f5);
          const uint8_t fsym = s_fs[m], rsym = s_rs[t], fq = s_fq[m], rq = s_rq[t];
          const uint8_t a = (int8_t) fq < 2 ? (uint8_t) 'N' : fsym, b = (int8_t) rq < 2 ? (uint8_t) 'N' : rsym;
          const int fi = (int) fq - P.tlo, ri = (int) rq - P.tlo;
          if (b == 'N') { sym = a; q = fq; }
          else if (a == 'N') { sym = b; q = rq; }
          else if (a == b) { sym = a; q = P.qual_same[fi * P.tdim + ri]; }
          else if ((int8_t) fq > (int8_t) rq) { sym = a; q = P.qual_diff[fi * P.tdim + ri]; }
          else { sym = b; q = P.qual_diff[ri * P.tdim + fi]; }
          ferr += sym != fsym; rerr += sym != rsym;
        }
      else { const int t = r3 + (m - f5); sym = s_rs[t]; q = s_rq[t]; }
      o_s[m] = sym; o_q[m] = q; s_mq[m] = q;
    }
  ferr = wave_sum(ferr); rerr = wave_sum(rerr);
  __syncthreads();

  // expected errors: lane 0 the merged read, lane 1 the forward read's part, lane 2 the reverse read's part, each in position order
  double ee = 0.0;
  if (lane < 3)
    for (int m = 0; m < mergelen; ++m)
      {
        if (lane == 0) ee += s_q2p[s_mq[m] & 127];
        else if (lane == 1) { if (m < f5 + nm) ee += s_q2p[s_fq[m] & 127]; }
        else if (m >= f5) ee += s_q2p[s_rq[r3 + (m - f5)] & 127];
      }
  rec.ee_merged = __shfl(ee, 0, 64); rec.ee_fwd = __shfl(ee, 1, 64); rec.ee_rev = __shfl(ee, 2, 64);
  rec.merged_length = mergelen; rec.fwd_errors = ferr; rec.rev_errors = rerr;
  if (rec.ee_merged <= P.maxee) { rec.reason = VSX_MERGE_OK; rec.merged = 1; } else rec.reason = VSX_MERGE_MAXEE;
  if (lane == 0) recs[pair] = rec;
}

}  // namespace

extern "C" hipError_t vsx_launch_merge(const VsxMergeItem * d_items, uint32_t n_items, const uint8_t * d_blob, VsxMergeParams P,
                                       VsxMergeDevRec * d_recs, uint8_t * d_oseq, uint8_t * d_oqual, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_merge_kernel, dim3(n_items), dim3(VSX_MERGE_THREADS), 0, st, d_items, n_items, d_blob, P, d_recs, d_oseq, d_oqual);
  return hipGetLastError();
}
