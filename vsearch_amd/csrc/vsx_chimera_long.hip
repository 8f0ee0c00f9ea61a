// vsx_chimera_long.hip -- parent selection and evaluation of --chimeras_denovo on the device: find_best_parents_long +
// eval_parents_long (reference core/chimera.cpp:505-624, :995-1242), one workgroup per query.  The host form of the same two
// functions is vsx_internal_chimeras_long_eval_host in vsx_chimera.cpp (queries beyond the limits below, sentinel pairs, a
// diff_pct that is no multiple of 2^-13, VSX_CHIMERA=host, and the tests' checker).
//
// Inputs: the whole-query alignments of a query against its <= VSX_CHIMERAS_LONG_MAX_CAND candidates as the traceback left them in
// HBM (hit records + run words) and the 4-bit codes of the query and the candidates.
//
//   find_matches (:367-413)   per candidate one row of match bits (a NONZERO 4-bit AND of the aligned symbols) and one row of
//                             "an insertion stands in front of this position" bits; one wave walks one candidate's runs, lanes over
//                             a run
//   rounds (:521-595)         one thread per candidate walks the query left to right over its two rows and the shared `used` bits:
//                             a position that is used, or that has an insertion in front of it while a segment is open, closes the
//                             segment and is itself skipped; inside a segment the longest run of match bits is kept, the leftmost
//                             among equals (with diff_pct = 0 that is scan_matches' answer: a mismatch costs 100 and a match earns
//                             nothing, so a substring scores >= 0 iff it has no mismatch).  With a tolerance the walker runs
//                             scan_scaled below: scan_matches in 32-bit integers, in units of 2^-13.  The round's winner is the
//                             longest region, then the lowest candidate: what the reference's "scan only a longer segment,
//                             replace only by a strictly longer region" visit keeps.  Its positions become used
//   eval_parents_long         the alignment rows are never built.  Per parent: the columns with equal codes = matched-run positions
//                             with equal codes + deleted positions whose query code is 0 + inserted symbols whose code is 0 + the
//                             insertion columns it leaves empty (sum of maxi - its own insertions); maxi (the longest insertion in
//                             front of each position over the parents) by atomic max in LDS
//
// Exact arithmetic: the identities and the divergence are the reference's double expressions, separately rounded.
//
// LDS: two bit matrices of 64 rows x 65 words (rows padded by one word: the per-candidate walkers read the same word index of
// different rows, and a stride of 64 words would put them all on one bank) = 33 280 B, + 1 184 B of round state: 34 464 B per
// 256-thread workgroup, 4 workgroups (16 waves) per CU of 160 KiB; 46 VGPRs, no scratch.  maxi (<= 2049 ints) reuses the insertion
// matrix.  With a tolerance each workgroup of a launch also owns 2 048 x 64 ints of global scratch (the suffix sums), which is why
// such a launch has at most VSX_CHIMLONG_SCRATCH_GROUPS workgroups.
#include "vsx_internal.h"
#include "../../include/vsx_search.h"

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_LMAX = VSX_CHIMERAS_LONG_MAX_QLEN;
constexpr int CL_CMAX = VSX_CHIMERAS_LONG_MAX_CAND;
constexpr int CL_PMAX = VSX_CHIMERAS_LONG_MAX_PARENTS;
constexpr int CL_W = CL_LMAX / 32;                  // bit words per row
constexpr int CL_STRIDE = CL_W + 1;                 // row stride in words (bank spread)
constexpr int CL_SLOTS = CL_LMAX;                   // scratch ints per candidate (diff_pct != 0)
static_assert(CL_LMAX % 32 == 0, "layout");
static_assert((CL_LMAX + 1) <= CL_CMAX * CL_STRIDE, "maxi reuses the insertion matrix");

// (kept beside vsx_devutil.h's butterfly: only lane 0 reads the sum, and the downward shuffle is an instruction per step shorter)
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;                                         // lane 0 holds the sum
}


#define CL_BIT(row, p) (((row)[(p) >> 5] >> ((p) & 31)) & 1u)

// One candidate's round for diff_pct != 0, in integers: a match scores gain = diff_pct * 2^13, a mismatch gain - 100 * 2^13 (the
// host sends only percentages for which gain is an integer; every partial sum of a segment of <= 2 048 positions is then an integer
// below 2^31, and a multiple of 2^-13 below 2^18 in the reference's doubles, so both compare alike).  Per segment this is
// scan_matches (:439-502): with p the prefix sums and q their suffix maxima, sfx[k] = q[k] - p[k] = max(0, sfx[k + 1] + score[k])
// is filled right to left into the workgroup's scratch (one int per position and candidate, candidates adjacent: the walkers advance
// in step and their stores coalesce), and the two pointers keep W = p[j] - p[i - 1], so that q[j] - p[i - 1] = sfx[j] + W.
// A segment is scanned only if it is longer than the best region so far, a region replaces it only if strictly longer.
__device__ void scan_scaled(const uint32_t * mrow, const uint32_t * irow, const uint32_t * used, int L, int gain, int32_t * sfx,
                            int * best_len, int * best_start)
{
  const int loss = gain - 100 * 8192;
  // positions outside every segment (used, or an insertion in front while a segment is open) are marked, then sfx right to left
  for (int j = 0, seg = 0; j < L; ++j)
    {
      const bool out = CL_BIT(used, j) || (seg > 0 && CL_BIT(irow, j));
      seg = out ? 0 : seg + 1;
      sfx[(size_t) j * CL_CMAX] = out ? -1 : 0;
    }
  int32_t s = 0;
  for (int j = L - 1; j >= 0; --j)
    {
      if (sfx[(size_t) j * CL_CMAX] < 0) s = 0;                               // the slot behind a segment's last position
      else s = max(0, s + (CL_BIT(mrow, j) ? gain : loss));
      sfx[(size_t) j * CL_CMAX] = s;
    }
  int best = 0, bstart = 0;
  for (int j0 = 0; j0 < L; ++j0)
    {
      const int start = j0;
      while (j0 < L && !CL_BIT(used, j0) && (j0 == start || !CL_BIT(irow, j0))) ++j0;
      const int len = j0 - start;
      if (len <= best) continue;
      int i = 1, j = 1, bi = 0, bd = -1;
      int32_t W = CL_BIT(mrow, start) ? gain : loss;
      while (j <= len)
        {
          const int32_t sj = j == len ? 0 : sfx[(size_t) (start + j) * CL_CMAX];
          if (sj + W >= 0)
            {
              if (j - i + 1 > bd) { bi = i; bd = j - i + 1; }
              ++j;
              if (j <= len) W += CL_BIT(mrow, start + j - 1) ? gain : loss;
            }
          else
            {
              W -= CL_BIT(mrow, start + i - 1) ? gain : loss;
              ++i;
            }
        }
      if (bd > best) { best = bd; bstart = start + bi - 1; }
    }
  *best_len = best;
  *best_start = bstart;
}

__global__ void __launch_bounds__(CL_THREADS)
vsx_chimeras_long_kernel(const VsxChimLongItem * __restrict__ items, const uint8_t * __restrict__ qcodes, const uint64_t * __restrict__ qoff,
                         const uint32_t * __restrict__ qlen, const uint8_t * __restrict__ tcodes, const uint64_t * __restrict__ toff,
                         const uint32_t * __restrict__ tlen, const VsxPairOut * __restrict__ hits, const uint32_t * __restrict__ pair_target,
                         uint64_t n_pairs, const uint32_t * __restrict__ runs, uint64_t n_runs, VsxChimLongParams P,
                         int32_t * __restrict__ scratch, vsx_chimeras_long_result * __restrict__ out)
{
  __shared__ uint32_t s_mb[CL_CMAX * CL_STRIDE];    // match bits
  __shared__ uint32_t s_ib[CL_CMAX * CL_STRIDE];    // insertion-in-front bits; later maxi
  __shared__ uint32_t s_used[CL_W];
  __shared__ int s_len[CL_CMAX], s_start[CL_CMAX];
  __shared__ int s_pc[CL_PMAX], s_ps[CL_PMAX], s_pl[CL_PMAX];      // parents: candidate, start, length
  __shared__ int s_eq[CL_PMAX], s_ins[CL_PMAX];
  __shared__ int s_round[3];                                          // winner of the round: candidate, start, length
  __shared__ int s_maxi_sum;

  const VsxChimLongItem it = items[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int L = (int) qlen[it.q];
  const int nc = (int) it.ncand;
  const uint8_t * q = qcodes + qoff[it.q];
  vsx_chimeras_long_result * res = out + it.out;
  const int parents_max = P.parents_max < CL_PMAX ? P.parents_max : CL_PMAX;

  // (the host sends no item beyond the limits; answered "no parents" rather than read past the LDS rows)
  const bool refuse = L > CL_LMAX || nc > CL_CMAX || nc < 1 || L < 1 || (uint64_t) it.pair0 + (uint64_t) nc > n_pairs;

  // ---- find_matches ----
  for (int k = tid; k < CL_CMAX * CL_STRIDE; k += CL_THREADS) { s_mb[k] = 0u; s_ib[k] = 0u; }
  for (int k = tid; k < CL_W; k += CL_THREADS) s_used[k] = 0u;
  __syncthreads();
  if (!refuse)
    for (int c = wave; c < nc; c += CL_WAVES)
      {
        const VsxPairOut h = hits[it.pair0 + c];
        const uint32_t tg = pair_target[it.pair0 + c];
        const uint8_t * t = tcodes + toff[tg];
        const int tl = (int) tlen[tg];
        int qp = 0, tp = 0;
        for (int k = (int) h.nruns - 1; k >= 0; --k)          // run words are stored last column first
          {
            const uint64_t ri = h.run_off + (uint64_t) k;
            if (ri >= n_runs) break;
            const uint32_t word = runs[ri];
            const int len = (int) (word >> 2), op = (int) (word & 3u);
            if (op == 0)
              {
                for (int j = lane; j < len; j += 64)
                  {
                    const int a = qp + j, b = tp + j;
                    if (a < L && b < tl && (q[a] & t[b]) != 0) atomicOr(&s_mb[c * CL_STRIDE + (a >> 5)], 1u << (a & 31));
                  }
                qp += len;
                tp += len;
              }
            else if (op == 1)
              {
                if (lane == 0 && qp < L) atomicOr(&s_ib[c * CL_STRIDE + (qp >> 5)], 1u << (qp & 31));
                tp += len;
              }
            else qp += len;
          }
      }
  __syncthreads();

  // ---- find_best_parents_long: up to parents_max rounds ----
  int np = 0, covered = 0;
  if (!refuse)
    for (int f = 0; f < parents_max; ++f)
      {
        if (tid < nc)
          {
            const uint32_t * mrow = s_mb + tid * CL_STRIDE;
            const uint32_t * irow = s_ib + tid * CL_STRIDE;
            int best = 0, bstart = 0;
            if (P.gain == 0)
              {
                int seg = 0, run = 0, rstart = 0;
                for (int w = 0; w * 32 < L; ++w)
                  {
                    const uint32_t mw = mrow[w], iw = irow[w], uw = s_used[w];
                    const int nb = L - w * 32 < 32 ? L - w * 32 : 32;
                    for (int b = 0; b < nb; ++b)
                      {
                        const bool u = (uw >> b) & 1u, in = (iw >> b) & 1u, m = (mw >> b) & 1u;
                        if (u || (seg > 0 && in)) { seg = 0; run = 0; }       // closes the segment; the position itself is skipped
                        else
                          {
                            ++seg;
                            if (m)
                              {
                                if (run == 0) rstart = w * 32 + b;
                                ++run;
                                if (run > best) { best = run; bstart = rstart; }
                              }
                            else run = 0;
                          }
                      }
                  }
              }
            else
              scan_scaled(mrow, irow, s_used, L, P.gain, scratch + (size_t) blockIdx.x * CL_SLOTS * CL_CMAX + tid, &best, &bstart);
            s_len[tid] = best;
            s_start[tid] = bstart;
          }
        __syncthreads();
        if (tid == 0)
          {
            int bl = 0, bc = -1;
            for (int c = 0; c < nc; ++c)
              if (s_len[c] > bl) { bl = s_len[c]; bc = c; }
            s_round[0] = bc;
            s_round[1] = bc >= 0 ? s_start[bc] : 0;
            s_round[2] = bl;
          }
        __syncthreads();
        const int bc = s_round[0], bs = s_round[1], bl = s_round[2];
        if (bc < 0 || bl < P.length_min) break;                                // (uniform: every thread reads the same winner)
        if (tid == 0) { s_pc[np] = bc; s_ps[np] = bs; s_pl[np] = bl; }
        for (int w = tid; w * 32 < L; w += CL_THREADS)
          {
            const int lo = bs > w * 32 ? bs - w * 32 : 0;
            const int hi = bs + bl - w * 32 < 32 ? bs + bl - w * 32 : 32;
            if (lo < hi) s_used[w] |= (hi - lo == 32 ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u) << lo);
          }
        ++np;
        covered += bl;
        __syncthreads();
      }

  // parents by start (regions are disjoint: the starts differ)
  if (tid == 0)
    for (int a = 1; a < np; ++a)
      {
        const int c = s_pc[a], s = s_ps[a], l = s_pl[a];
        int b = a - 1;
        for (; b >= 0 && s_ps[b] > s; --b) { s_pc[b + 1] = s_pc[b]; s_ps[b + 1] = s_ps[b]; s_pl[b + 1] = s_pl[b]; }
        s_pc[b + 1] = c; s_ps[b + 1] = s; s_pl[b + 1] = l;
      }
  __syncthreads();

  // the record is zeroed by all threads and its fields are then stored in place by thread 0 (no 432-byte copy on a lane's stack)
  for (int k = tid; k < (int) (sizeof(vsx_chimeras_long_result) / 4); k += CL_THREADS) reinterpret_cast<uint32_t *>(res)[k] = 0u;
  __syncthreads();
  const bool chimeric = np > 1 && covered == L;
  if (tid == 0)
    {
      res->status = chimeric ? VSX_CHIMERA_CHIMERIC : VSX_CHIMERA_NO_PARENTS;
      res->flag = chimeric ? 'Y' : 'N';
      res->n_parents = np;
      for (int f = 0; f < np; ++f) { res->parent[f] = pair_target[it.pair0 + s_pc[f]]; res->start[f] = s_ps[f]; res->len[f] = s_pl[f]; }
    }
  if (!chimeric) return;

  // ---- eval_parents_long ----
  int * maxi = reinterpret_cast<int *>(s_ib);
  for (int k = tid; k <= L; k += CL_THREADS) maxi[k] = 0;
  if (tid == 0) s_maxi_sum = 0;
  __syncthreads();
  for (int f = wave; f < np; f += CL_WAVES)
    {
      const int c = s_pc[f];
      const VsxPairOut h = hits[it.pair0 + c];
      const uint32_t tg = pair_target[it.pair0 + c];
      const uint8_t * t = tcodes + toff[tg];
      const int tl = (int) tlen[tg];
      int qp = 0, tp = 0, eq = 0, ins = 0;
      for (int k = (int) h.nruns - 1; k >= 0; --k)
        {
          const uint64_t ri = h.run_off + (uint64_t) k;
          if (ri >= n_runs) break;
          const uint32_t word = runs[ri];
          const int len = (int) (word >> 2), op = (int) (word & 3u);
          if (op == 0)
            {
              for (int j = lane; j < len; j += 64)
                {
                  const int a = qp + j, b = tp + j;
                  if (a < L && b < tl && q[a] == t[b]) ++eq;
                }
              qp += len;
              tp += len;
            }
          else if (op == 1)
            {
              for (int j = lane; j < len; j += 64)
                if (tp + j < tl && t[tp + j] == 0) ++eq;                      // an inserted symbol without a code equals the query's gap
              if (lane == 0 && qp <= L) { atomicMax(&maxi[qp], len); ins += len; }
              tp += len;
            }
          else
            {
              for (int j = lane; j < len; j += 64)
                if (qp + j < L && q[qp + j] == 0) ++eq;                       // the parent's gap equals a query symbol without a code
              qp += len;
            }
        }
      eq = wave_sum(eq);
      if (lane == 0) { s_eq[f] = eq; s_ins[f] = ins; }
    }
  __syncthreads();
  int ms = 0;
  for (int k = tid; k <= L; k += CL_THREADS) ms += maxi[k];
  ms = wave_sum(ms);
  if (lane == 0 && ms) atomicAdd(&s_maxi_sum, ms);
  __syncthreads();
  if (tid != 0) return;

  const int alnlen = L + s_maxi_sum;
  res->alnlen = alnlen;
  double QT = 0.0;
  for (int f = 0; f < np; ++f)
    {
      const int matches = s_eq[f] + (s_maxi_sum - s_ins[f]);
      const double QP = 100.0 * matches / alnlen;
      res->id_query_parent[f] = QP;
      QT = QT < QP ? QP : QT;
    }
  res->id_query_top = QT;
  res->divergence = 100.0 * (100.0 - QT) / QT;
}

}  // namespace

extern "C" hipError_t vsx_launch_chimeras_long(const VsxChimLongItem * d_items, uint32_t nitems, const uint8_t * qcodes, const uint64_t * qoff,
                                               const uint32_t * qlen, const uint8_t * tcodes, const uint64_t * toff, const uint32_t * tlen,
                                               const VsxPairOut * d_hits, const uint32_t * d_pair_target, uint64_t n_pairs,
                                               const uint32_t * d_runs, uint64_t n_runs, VsxChimLongParams P, int32_t * d_scratch,
                                               void * d_out, hipStream_t st)
{
  if (P.gain != 0 && !d_scratch) return hipErrorInvalidValue;
  // with a scratch the grid is at most VSX_CHIMLONG_SCRATCH_GROUPS workgroups (one scratch block each); the launches follow each
  // other on the stream
  const uint32_t step = P.gain != 0 ? VSX_CHIMLONG_SCRATCH_GROUPS : nitems;
  for (uint32_t at = 0; at < nitems; at += step)
    {
      const uint32_t n = nitems - at < step ? nitems - at : step;
      hipLaunchKernelGGL(vsx_chimeras_long_kernel, dim3(n), dim3(CL_THREADS), 0, st, d_items + at, qcodes, qoff, qlen, tcodes, toff, tlen,
                         d_hits, d_pair_target, n_pairs, d_runs, n_runs, P, d_scratch, static_cast<vsx_chimeras_long_result *>(d_out));
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}
